// MFMA fragment helpers shared by the gfx950 attention kernels
// (flash_attn*.hip, paged_attn*.hip).
//
// mfma_f32_16x16x32_bf16 fragment layouts (HW-validated by mfma_layout_probe
// + the asymmetric-input check in tests/test_ops_gpu.py):
//   A (16x32): lane l holds A[l%16][(l/16)*8 + j], j=0..7   (one frag8)
//   B (32x16): lane l holds B[(l/16)*8 + j][l%16]
//   C (16x16): lane l, reg r holds C[(l/16)*4 + r][l%16]
//
// mfma_f32_32x32x16_bf16 fragment layouts (mfma32_layout_probe):
//   A (32x16): lane l holds A[l&31][(l>>5)*8 + j]
//   B (16x32): lane l holds B[(l>>5)*8 + j][l&31]
//   C (32x32): lane l, reg r holds C[crow32(r, l>>5)][l&31]
//
// Operand-layout cheat sheet (X row-major [row][col] in LDS):
//   "B-frag contraction over col of X" (e.g. S=QK^T contracts d):
//       read x_lds[n*16 + l16][kk*32 + lk8 .. +8]        (contiguous)
//   "B-frag contraction over row of X" (e.g. O=PV contracts kv):
//       needs X transposed in LDS: xt_lds[col][row]
#pragma once

#include "common.h"

typedef short8v frag8;   // 8 bf16: one lane's A or B operand

__device__ __forceinline__ f32x4 mfma16(frag8 a, frag8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x16 mfma32(frag8 a, frag8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// C row of 32x32 accumulator register r in lane half hi (= lane >> 5)
__device__ __forceinline__ int crow32(int r, int hi) {
    return (r & 3) + 8 * (r >> 2) + 4 * hi;
}

// XOR swizzle for a row-major bf16 LDS tile (stride LD elements): a tile
// read as column slices is a 32-way bank conflict; byte offset ^
// ((row&7)<<4) spreads each column over 8 distinct 16-byte slots.  It is
// bijective within an 8-row stripe and keeps 16B alignment, so b128
// reads/writes stay legal.  Writes and reads must both go through it.
template <int LD>
__device__ __forceinline__ char* swz(ushort_t* base, int row, int col_elem) {
    return reinterpret_cast<char*>(base) +
           (((row * LD + col_elem) * 2) ^ ((row & 7) << 4));
}

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
    return (unsigned)f32_to_bf16(a) | ((unsigned)f32_to_bf16(b) << 16);
}

// T12: convert one 16-row slice (regs rb..rb+7 of a 32x32 C tile) into the
// 8 packed bf16 values each lane needs for the transpose-contraction
// fragment: lane ends up with X[other = hi*8 + j] at its own column.
// swap(pack(p0,p1), pack(p4,p5)) delivers words {0,2} and
// swap(pack(p2,p3), pack(p6,p7)) words {1,3}; no LDS round trip.
__device__ __forceinline__ frag8 t12_convert(const f32x16& p, int rb) {
    unsigned w[4];
    {
        unsigned lo0 = pack_bf16(p[rb + 0], p[rb + 1]);
        unsigned hi0 = pack_bf16(p[rb + 4], p[rb + 5]);
        auto rr = __builtin_amdgcn_permlane32_swap(lo0, hi0, false, false);
        w[0] = rr[0]; w[2] = rr[1];
    }
    {
        unsigned lo1 = pack_bf16(p[rb + 2], p[rb + 3]);
        unsigned hi1 = pack_bf16(p[rb + 6], p[rb + 7]);
        auto rr = __builtin_amdgcn_permlane32_swap(lo1, hi1, false, false);
        w[1] = rr[0]; w[3] = rr[1];
    }
    frag8 f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        f[j * 2] = (short)(w[j] & 0xffff);
        f[j * 2 + 1] = (short)(w[j] >> 16);
    }
    return f;
}
