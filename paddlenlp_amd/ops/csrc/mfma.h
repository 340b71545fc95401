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

// ---------------------------------------------------------------------------
// Softmax arithmetic helpers of the v2 attention kernels.
//
// Next to MFMAs a packed f32 VALU instruction costs more than the two plain
// ones it replaces, and under -O3 the SLP vectoriser packs adjacent
// multiplies, adds and fmas of a tile into v_pk_*_f32.  It builds its packs
// backwards from a vector's elements, and an element that comes out of an asm
// statement is where it stops: sm_opaque(x) is x behind an EMPTY asm
// statement (no instruction is emitted, so the compiler still schedules and
// pads every real instruction itself).  It also keeps a product a product:
// the optimiser cannot contract it into an fma with a later add, which would
// round differently.
//
// fmaxf on an MFMA result gets a canonicalising v_max_f32 x, x, x in front,
// so the forward's row max is taken with sm_max3, a real instruction in an
// asm statement.  The compiler does not model what is inside one and pads no
// hazard for it: sm_fence() holds the wait states an MFMA result needs before
// a VALU instruction may read it (12 after an 8-pass MFMA) and must stand
// between the MFMA chain that wrote a tile and the first sm_max3 that reads
// it.  The reader depends on the fence's output, so it is not scheduled above
// it.  The result of sm_max3 goes to compiler-visible instructions only.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float sm_opaque(float x) {
    asm("" : "+v"(x));
    return x;
}
__device__ __forceinline__ void sm_fence(f32x16& a, f32x16& b) {
    asm volatile("s_nop 11" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float sm_max3(float a, float b, float c) {
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// max over the 16 registers of a C tile, as 8 v_max3_f32
__device__ __forceinline__ float sm_tile_max(float m, const f32x16& s) {
#pragma unroll
    for (int r = 0; r < 16; r += 2) m = sm_max3(m, s[r], s[r + 1]);
    return m;
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

// two floats to one word of two bf16 (a low, b high), round-to-nearest-even:
// as a 2-vector conversion this is ONE v_cvt_pk_bf16_f32; two scalar
// conversions joined by shift and or cost four instructions for the same bits
// (used by every t12_convert caller: flash_attn*_v2.hip, and by paged_attn_mfma.hip)
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
    union { bf16x2v h; unsigned u; } r;
    r.h = __builtin_convertvector(f32x2{a, b}, bf16x2v);
    return r.u;
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

// ---------------------------------------------------------------------------
// Dual-use LDS image of a [rows][128] bf16 tile: the same bytes serve
// ds_read_b128 row reads (contraction over the 128 columns) and
// ds_read_b64_tr_b16 transposed reads (contraction over the rows), so no
// second, transposed copy is staged.  The tile is cut into 8-row x 32-column
// subtiles of 512 B (64-byte subtile rows); img_off is the byte offset of
// 16-byte chunk ch (0..15) of row `row`.  The XOR keeps both kinds of read
// conflict-free for the 32x32x16 operands, and a 32-row operand needs only
// two address registers per kind of read (everything else is an immediate).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int img_off(int row, int ch) {
    return 2048 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) +
           16 * ((ch & 3) ^ ((row >> 2) & 3));
}

typedef short short4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) short4v lds_short4v;

// LDS-DMA fill (global_load_lds_dwordx4): one wave-instruction writes 1 KiB
// lane-linear (lane l lands at 1024*piece + 16*l), which is two subtiles:
// rows 8*(piece>>1) .. +7, columns 64*(piece&1) .. +63.  The hardware cannot
// scatter the destination, so the XOR goes on the per-lane SOURCE chunk.
// img_fill_row / img_fill_chunk give the source coordinate of the 16 bytes
// lane `lane` must fetch for `piece`.
__device__ __forceinline__ int img_fill_row(int piece, int lane) {
    return 8 * (piece >> 1) + ((lane >> 2) & 7);
}
__device__ __forceinline__ int img_fill_chunk(int piece, int lane) {
    const int row = img_fill_row(piece, lane);
    return 4 * (2 * (piece & 1) + (lane >> 5)) + ((lane & 3) ^ ((row >> 2) & 3));
}
//
// The DMA is issued from inline assembly, not through
// __builtin_amdgcn_global_load_lds: the compiler treats the builtin as a
// pending write to all of LDS and puts s_waitcnt vmcnt(0) ahead of the next
// ds_read of ANY buffer, which drains a prefetch the moment it is issued.
// An instruction inside an asm statement is not counted, so the caller must
// retire it with lds_dma_wait_all() and a barrier before the data is read.
// M0 carries the wave-uniform LDS destination and is restored in the same
// statement (the compiler owns M0 outside it).
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(unsigned long long)p;   // low half of a generic LDS pointer
}
// lds_dst: wave-uniform destination (image base + 1024*piece)
__device__ __forceinline__ void lds_dma16(const void* src, const void* lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_addr(lds_dst)) : "memory");
}
// 4-byte form: lane l lands at lds_dst + 4*l
__device__ __forceinline__ void lds_dma4(const void* src, const void* lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_addr(lds_dst)) : "memory");
}
__device__ __forceinline__ void lds_dma_wait_all() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Row-read A/B operand of mfma32 whose contraction runs over the image's
// columns: lane takes X[row][kk*16 + hi*8 .. +8].
__device__ __forceinline__ frag8 img_row_frag(const ushort_t* img, int row, int kk, int hi) {
    return *reinterpret_cast<const frag8*>(
        reinterpret_cast<const char*>(img) + img_off(row, kk * 2 + hi));
}

// Transposed-read B operand of mfma32 whose contraction runs over the image's
// rows: lane takes X[ks*16 + hi*8 + j][n*32 + (lane&31)], j = 0..7, as two
// ds_read_b64_tr_b16.  Each 16-lane group gathers a 4-row x 16-column block;
// lane 4q+p of the group supplies the address of row q, columns 4p..4p+3, and
// lane i receives column i.  EXEC must be all ones (wave-uniform control flow
// only).
__device__ __forceinline__ frag8 img_tr_frag(const ushort_t* img, int ks, int n, int lane) {
    const int i = lane & 15, qq = i >> 2, p = i & 3;
    const int hi = lane >> 5;
    const int c0 = n * 4 + ((lane >> 4) & 1) * 2 + (p >> 1);
    const char* base = reinterpret_cast<const char*>(img) + 8 * (p & 1);
    frag8 f;
#pragma unroll
    for (int jj = 0; jj < 2; jj++) {
        const int row = ks * 16 + hi * 8 + jj * 4 + qq;
        short4v t = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_short4v*)(base + img_off(row, c0)));
#pragma unroll
        for (int e = 0; e < 4; e++) f[jj * 4 + e] = t[e];
    }
    return f;
}

// The lane id, re-derived by an instruction the compiler can neither hoist
// nor merge with another copy: kernels at the register cap use it so that
// address terms are recomputed where they are needed, not kept live (and
// spilled) across a loop.
__device__ __forceinline__ int fresh_lane_id() {
    int ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0"
                 : "=v"(ln));
    return ln;
}

// ---------------------------------------------------------------------------
// Block -> (tile, batch*head) order for the 2-D attention grids (x = tile,
// y = batch*head).  Workgroups are dealt round-robin to the 8 XCDs, so
// xcd = flat & 7, and every head keeps all its tiles on one XCD (its shared
// K/V or Q/dO tiles re-hit that XCD's L2).  Inside an XCD the heads are taken
// in groups of W; inside a group the tiles go heaviest-first under the causal
// mask (ASCENDING for kv tiles, descending for q tiles) with the W heads
// interleaved, so the last blocks to start are the lightest ones.  Grids
// whose y is no multiple of 8 keep the plain order.
//
// W trades the scheduling tail against L2 re-hits (a larger W spreads one
// head's tiles in time).  Measured interleaved at B8 S4096 32:8 heads and
// B4 S8192 (profiles/fa_dkv_lds_dma.md): W = 1 keeps the tail, W = 2 removes
// most of it, W = 4 is best or tied for fwd, dq and dkv at both shapes, all
// heads of the XCD at once is no better.  One constant serves all three.
// ---------------------------------------------------------------------------
#define FA_ORDER_W 4
template <int W, bool ASCENDING>
__device__ __forceinline__ void xcd_grouped_tile(int& tile, int& bh) {
    const int T = gridDim.x;
    if ((gridDim.y & 7) != 0) {
        tile = blockIdx.x;
        bh = blockIdx.y;
        return;
    }
    const int flat = blockIdx.x + T * blockIdx.y;
    const int idx = flat >> 3;
    const int hp = gridDim.y >> 3;            // heads per XCD
    const int grp = idx / (W * T);
    const int rem = idx - grp * (W * T);
    const int wg = min(W, hp - grp * W);      // the last group may be short
    const int rank = rem / wg;
    tile = ASCENDING ? rank : T - 1 - rank;
    bh = (flat & 7) * hp + grp * W + (rem - rank * wg);
}
