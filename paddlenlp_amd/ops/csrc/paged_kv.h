// Paged-KV cache access of the MFMA decode and append kernels
// (paged_attn_mfma.hip): workgroup geometry, cache record addressing and the
// per-mode dequantising loads; and the fold of per-split partials that every
// paged attention kernel's split path ends in.
//
// Cache layout: [num_blocks, block_size, Hk, D] per layer; MODE 0 = bf16,
// 1 = int8, 2 = int4 packed nibbles (offset-binary q+8); quantised modes
// carry one fp32 scale per (token, kv-head) record.
#pragma once

#include "mfma.h"

#define PD3_WAVES 4
#define PD3_BLOCK (PD3_WAVES * 64)
#define PD3_TILE 128
#define PD3_MAXG 16

// index of the (token, kv-head) record of sequence position tok
__device__ __forceinline__ long long pkv_record(const int* __restrict__ bt, int tok,
                                                int block_size, int Hk, int hk) {
    int blk = bt[tok / block_size];
    return ((long long)blk * block_size + (tok % block_size)) * Hk + hk;
}

// K row of record rec as the A-fragments of S^T = K·Q^T: lane group lg
// takes K[rec][kk*32 + lg*8 + j]
template <int D, int MODE>
__device__ __forceinline__ void pkv_load_k_frags(frag8 (&ak)[D / 32],
                                                 const void* __restrict__ k_cache,
                                                 const float* __restrict__ k_scale,
                                                 long long rec, int lg) {
    constexpr int KD = D / 32;
    if (MODE == 1) {
        float ks = k_scale[rec];
        const signed char* kb = (const signed char*)k_cache + rec * D;
#pragma unroll
        for (int kk = 0; kk < KD; kk++)
#pragma unroll
            for (int j = 0; j < 8; j++)
                ak[kk][j] = (short)f32_to_bf16(
                    (float)kb[kk * 32 + lg * 8 + j] * ks);
    } else if (MODE == 2) {
        float ks = k_scale[rec];
        const unsigned char* kb = (const unsigned char*)k_cache + rec * D / 2;
#pragma unroll
        for (int kk = 0; kk < KD; kk++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                unsigned byte = kb[(kk * 32 + lg * 8) / 2 + j];
                ak[kk][j * 2] = (short)f32_to_bf16(((int)(byte >> 4) - 8) * ks);
                ak[kk][j * 2 + 1] = (short)f32_to_bf16(((int)(byte & 0xF) - 8) * ks);
            }
    } else {
        const ushort_t* kb = (const ushort_t*)k_cache + rec * D;
#pragma unroll
        for (int kk = 0; kk < KD; kk++)
            ak[kk] = *reinterpret_cast<const frag8*>(kb + kk * 32 + lg * 8);
    }
}

// 32 columns (s_c .. s_c+31) of the V row of record rec, dequantised to bf16
template <int D, int MODE>
__device__ __forceinline__ void pkv_load_v_row(short8v (&vr)[4],
                                               const void* __restrict__ v_cache,
                                               const float* __restrict__ v_scale,
                                               long long rec, int s_c) {
    long long base = rec * D + s_c;
    if (MODE == 1) {
        float vs = v_scale[rec];
        const signed char* v8 = (const signed char*)v_cache;
#pragma unroll
        for (int cc = 0; cc < 4; cc++)
#pragma unroll
            for (int j = 0; j < 8; j++)
                vr[cc][j] = (short)f32_to_bf16((float)v8[base + cc * 8 + j] * vs);
    } else if (MODE == 2) {
        float vs = v_scale[rec];
        const unsigned char* v4 = (const unsigned char*)v_cache + (rec * D + s_c) / 2;
#pragma unroll
        for (int cc = 0; cc < 4; cc++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                unsigned byte = v4[cc * 4 + j];
                vr[cc][j * 2] = (short)f32_to_bf16(((int)(byte >> 4) - 8) * vs);
                vr[cc][j * 2 + 1] = (short)f32_to_bf16(((int)(byte & 0xF) - 8) * vs);
            }
    } else {
        const ushort_t* v16 = (const ushort_t*)v_cache;
#pragma unroll
        for (int cc = 0; cc < 4; cc++)
            vr[cc] = *reinterpret_cast<const short8v*>(v16 + base + cc * 8);
    }
}

// a thread's V token row-pair -> the transposed, swizzled V^T LDS tile
// ([D][PD3_TILE], u32 = two adjacent tokens of one column)
__device__ __forceinline__ void pkv_write_vt(ushort_t* vt_lds, const short8v (&vr)[2][4],
                                             int s_c, int s_r0) {
#pragma unroll
    for (int cc = 0; cc < 4; cc++) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            unsigned p32 = ((unsigned)(unsigned short)vr[0][cc][j]) |
                           (((unsigned)(unsigned short)vr[1][cc][j]) << 16);
            *reinterpret_cast<unsigned*>(
                swz<PD3_TILE>(vt_lds, s_c + cc * 8 + j, s_r0)) = p32;
        }
    }
}

// Fold the fp32 partials {m, l, acc[D]} of one query row, one record per kv
// split split_stride floats apart from base, into the bf16 row out_row: one
// wave per row, lane takes D/64 columns.  Split sp covers positions
// sp*chunk .. of kv_end; the splits past kv_end wrote nothing.
template <int D>
__device__ __forceinline__ void pkv_fold_splits(const float* __restrict__ base,
                                                long long split_stride, int nsplit,
                                                int chunk, int kv_end,
                                                ushort_t* __restrict__ out_row) {
    constexpr int EPL = D / 64;
    const int lane = threadIdx.x & 63;
    float gm = -INFINITY;
    for (int sp = 0; sp < nsplit; sp++) {
        if (sp * chunk >= kv_end) break;
        gm = fmaxf(gm, base[sp * split_stride]);
    }
    float gl = 0.f;
    float oacc[EPL] = {0.f};
    for (int sp = 0; sp < nsplit; sp++) {
        if (sp * chunk >= kv_end) break;
        const float* pp = base + sp * split_stride;
        float a = (pp[0] == -INFINITY) ? 0.f : __expf(pp[0] - gm);
        gl += pp[1] * a;
#pragma unroll
        for (int e = 0; e < EPL; e++)
            oacc[e] += pp[2 + lane * EPL + e] * a;
    }
    float inv = (gl > 0.f) ? 1.0f / gl : 0.f;
#pragma unroll
    for (int e = 0; e < EPL; e++)
        out_row[lane * EPL + e] = f32_to_bf16(oacc[e] * inv);
}
