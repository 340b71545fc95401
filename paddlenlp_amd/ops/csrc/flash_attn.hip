// FlashAttention-2 forward + backward, v1 — hand-written gfx950 (CDNA4) MFMA.
//
// MI355X-native replacement for the reference's training attention
// (paddle `flash_attention` fused op; the csrc append_attn
// family is the inference-side sibling).  Not a CUDA port: tiles are sized
// for 64-wide waves and mfma_f32_16x16x32_bf16, K/V staged through LDS with
// +8-element padded rows (≤2-way bank aliasing, free on CDNA4 per guide G4),
// fp32 online-softmax state in registers.
//
// v1 is the plain fallback: every D=64 and D=32 model runs it, and D=128
// runs it only when the v2 8-wave 32x32 kernels (flash_attn_v2.hip,
// flash_attn_bwd_v2.hip) decline the shape or force_v1 is set.
//
// Structure: block = 4 waves (256 thr); Q tile 64 rows (16/wave, one M-frag);
// KV tile 64; LDS addressed linearly with LDS_PAD.
//
// What was tried on this structure and rejected (co-compiled A/B at the
// bench shape B8 S4096 Hq32 Hk8 D128; table in
// profiles/r01_fa_variant_ab.md).  The code is gone, the numbers stay:
//   fwd: one M-frag + padded-linear LDS ~167 TF (kept).
//     two M-frags per wave: 298 VGPR -> 1 wave/SIMD, 80 TF.
//     XOR-swizzled LDS: codegen-unstable 149-174 TF; conflicts are hidden
//       behind the staging barrier in this 2-phase structure (guide T2 gate).
//     global_load_lds K staging: 128 TF (the unpadded tile it needs
//       re-exposes 16-way read conflicts).
//     register-staged software pipeline (next tile's loads issued before
//       PV): 152 TF; loses to the multi-workgroup overlap the occupancy
//       already provides.  The async-stage split lives on in v2.
//   bwd: padded-linear ~200 TF (kept); XOR swizzle -15% (the extra LDS
//     tiles make the swizzle's address VALU the bottleneck).
//
// Fragment layouts and the operand-layout cheat sheet are in mfma.h.
#include "launchers.h"
#include "mfma.h"
#include <cstdlib>

#define FA_WAVES 4
#define FA_BLOCK (FA_WAVES * 64)
#define BLK_M 64   // = FA_WAVES * 16
#define BLK_N 64
#define LDS_PAD 8

// ---------------------------------------------------------------------------
// layout probe: one wave computes C = A @ B for 16x32 @ 32x16.  Used by the
// GPU layout-validation test with asymmetric random inputs (transpose-
// detecting, guide G9).
// ---------------------------------------------------------------------------
__global__ void mfma_layout_probe(const ushort_t* A, const ushort_t* B, float* C) {
    int l = threadIdx.x;
    frag8 a, b;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        a[j] = (short)A[(l % 16) * 32 + (l / 16) * 8 + j];
        b[j] = (short)B[((l / 16) * 8 + j) * 16 + (l % 16)];
    }
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = mfma16(a, b, c);
#pragma unroll
    for (int r = 0; r < 4; r++) C[((l / 16) * 4 + r) * 16 + (l % 16)] = c[r];
}

// ---------------------------------------------------------------------------
// forward.  Each wave owns 16 q rows of the 64-row Q tile.
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(FA_BLOCK) void flash_fwd_kernel(
    const ushort_t* __restrict__ q,   // [B, Sq, Hq, D]
    const ushort_t* __restrict__ k,   // [B, Skv, Hk, D]
    const ushort_t* __restrict__ v,   // [B, Skv, Hk, D]
    ushort_t* __restrict__ o,         // [B, Sq, Hq, D]
    float* __restrict__ lse,          // [B, Hq, Sq]
    const int* __restrict__ startend, // FlashMask [B, Skv] or nullptr:
                                      // key j visible to queries j<=i<start[j]
    int B, int Sq, int Skv, int Hq, int Hk, float scale, int causal) {
    constexpr int KD = D / 32;   // MFMA K-steps over the head dim
    constexpr int ND = D / 16;   // d-frags of the O accumulator
    constexpr int NN = BLK_N / 16;
    constexpr int LDK = D + LDS_PAD;
    constexpr int LDT = BLK_N + LDS_PAD;

    __shared__ ushort_t k_lds[BLK_N][LDK];       // K row-major [kv][d]
    __shared__ ushort_t vt_lds[D][LDT];          // V transposed [d][kv]
    __shared__ ushort_t p_lds[BLK_M][LDT];   // P row-major [q][kv]

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int l16 = lane & 15;
    const int lk8 = (lane >> 4) * 8;

    int qt, bh;
    if ((gridDim.y & 7) == 0) {
        // XCD-aware remap (see flash_attn_v2.hip): one (b,h) per XCD
        const int flat = blockIdx.x + gridDim.x * blockIdx.y;
        const int idx = flat >> 3;
        qt = idx % gridDim.x;
        bh = (flat & 7) * (gridDim.y >> 3) + idx / gridDim.x;
    } else {
        qt = blockIdx.x;
        bh = blockIdx.y;
    }
    const int b = bh / Hq, hq = bh % Hq;
    const int hk = hq / (Hq / Hk);
    const int q_base = qt * BLK_M;
    const int causal_off = Skv - Sq;  // kv visible iff kv <= q + off

    const long long q_row_stride = (long long)Hq * D;
    const long long kv_row_stride = (long long)Hk * D;
    const ushort_t* q_ptr = q + ((long long)b * Sq * Hq + hq) * D;
    const ushort_t* k_ptr = k + ((long long)b * Skv * Hk + hk) * D;
    const ushort_t* v_ptr = v + ((long long)b * Skv * Hk + hk) * D;

    // Q A-frags in registers (16 rows x D per wave)
    frag8 aq[KD];
    {
        int qrow = q_base + wave * 16 + l16;
        if (qrow < Sq) {
#pragma unroll
            for (int kk = 0; kk < KD; kk++)
                aq[kk] = *reinterpret_cast<const frag8*>(
                    q_ptr + (long long)qrow * q_row_stride + kk * 32 + lk8);
        } else {
#pragma unroll
            for (int kk = 0; kk < KD; kk++) aq[kk] = frag8{0};
        }
    }
    const int qrow0 = q_base + wave * 16 + (lane >> 4) * 4;

    float m_run[4], l_run[4];
#pragma unroll
    for (int r = 0; r < 4; r++) { m_run[r] = -INFINITY; l_run[r] = 0.f; }
    f32x4 acc_o[ND];
#pragma unroll
    for (int n = 0; n < ND; n++) acc_o[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    int n_kv_tiles = (Skv + BLK_N - 1) / BLK_N;
    if (causal) {
        int max_kv = q_base + BLK_M - 1 + causal_off;
        int lim = (max_kv + BLK_N) / BLK_N;
        n_kv_tiles = min(n_kv_tiles, max(lim, 0));
    }

    for (int kvt = 0; kvt < n_kv_tiles; kvt++) {
        const int kv_base = kvt * BLK_N;
        // stage K row-major (vector) + V transposed (b32-packed: two kv rows
        // per thread so the LDS transpose writes are 4-byte, halving ds ops)
        for (int idx = tid * 8; idx < (BLK_N / 2) * D; idx += FA_BLOCK * 8) {
            int rr = idx / D, col = idx % D;
            int row0 = rr * 2;
            int kvg0 = kv_base + row0;
            short8v k8a = {0,0,0,0,0,0,0,0}, k8b = {0,0,0,0,0,0,0,0};
            short8v v8a = {0,0,0,0,0,0,0,0}, v8b = {0,0,0,0,0,0,0,0};
            if (kvg0 < Skv) {
                k8a = *reinterpret_cast<const short8v*>(k_ptr + (long long)kvg0 * kv_row_stride + col);
                v8a = *reinterpret_cast<const short8v*>(v_ptr + (long long)kvg0 * kv_row_stride + col);
            }
            if (kvg0 + 1 < Skv) {
                k8b = *reinterpret_cast<const short8v*>(k_ptr + (long long)(kvg0 + 1) * kv_row_stride + col);
                v8b = *reinterpret_cast<const short8v*>(v_ptr + (long long)(kvg0 + 1) * kv_row_stride + col);
            }
            *reinterpret_cast<short8v*>(&k_lds[row0][col]) = k8a;
            *reinterpret_cast<short8v*>(&k_lds[row0 + 1][col]) = k8b;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                unsigned int packed = ((unsigned int)(unsigned short)v8a[j]) |
                                      (((unsigned int)(unsigned short)v8b[j]) << 16);
                *reinterpret_cast<unsigned int*>(&vt_lds[col + j][row0]) = packed;
            }
        }
        __syncthreads();

        // S = Q K^T (contract d; B-frag from K row-major), then softmax with
        // P written in place into the S accumulator, then P -> LDS
        f32x4 acc_s[NN];
#pragma unroll
        for (int n = 0; n < NN; n++) {
            acc_s[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KD; kk++) {
                frag8 bk = *reinterpret_cast<const frag8*>(&k_lds[n * 16 + l16][kk * 32 + lk8]);
                acc_s[n] = mfma16(aq[kk], bk, acc_s[n]);
            }
        }
#pragma unroll
        for (int n = 0; n < NN; n++) {
            int kvg = kv_base + n * 16 + l16;
            int kv_end = (startend && kvg < Skv)
                             ? startend[(long long)b * Skv + kvg] : Sq + causal_off;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                int qg = qrow0 + r;
                bool vis = (kvg < Skv) && (qg < Sq);
                if (causal) vis = vis && (kvg <= qg + causal_off);
                if (startend) vis = vis && (qg < kv_end);
                acc_s[n][r] = vis ? acc_s[n][r] * scale : -INFINITY;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float row_max = -INFINITY;
#pragma unroll
            for (int n = 0; n < NN; n++) row_max = fmaxf(row_max, acc_s[n][r]);
#pragma unroll
            for (int off = 8; off > 0; off >>= 1)
                row_max = fmaxf(row_max, __shfl_xor(row_max, off, 64));
            float m_new = fmaxf(m_run[r], row_max);
            float alpha;
            if (m_new == -INFINITY) {
                alpha = 1.f;
            } else if (m_run[r] == -INFINITY) {
                alpha = 0.f;
            } else {
                alpha = __expf(m_run[r] - m_new);
            }
            float row_sum = 0.f;
#pragma unroll
            for (int n = 0; n < NN; n++) {
                float p = (m_new == -INFINITY || acc_s[n][r] == -INFINITY)
                              ? 0.f : __expf(acc_s[n][r] - m_new);
                acc_s[n][r] = p;  // reuse the S accumulator for P
                row_sum += p;
            }
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) row_sum += __shfl_xor(row_sum, off, 64);
            l_run[r] = l_run[r] * alpha + row_sum;
            m_run[r] = m_new;
#pragma unroll
            for (int n = 0; n < ND; n++) acc_o[n][r] *= alpha;
        }
#pragma unroll
        for (int n = 0; n < NN; n++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                p_lds[wave * 16 + (lane >> 4) * 4 + r][n * 16 + l16] =
                    f32_to_bf16(acc_s[n][r]);
        // each wave reads back only its own p_lds rows: a wave-local LDS
        // drain is enough (no cross-wave barrier needed here)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

        // O += P V  (contract kv; A from p_lds, B from vt_lds)
#pragma unroll
        for (int kk = 0; kk < BLK_N / 32; kk++) {
            frag8 ap = *reinterpret_cast<const frag8*>(&p_lds[wave * 16 + l16][kk * 32 + lk8]);
#pragma unroll
            for (int n = 0; n < ND; n++) {
                frag8 bv = *reinterpret_cast<const frag8*>(&vt_lds[n * 16 + l16][kk * 32 + lk8]);
                acc_o[n] = mfma16(ap, bv, acc_o[n]);
            }
        }
        __syncthreads();
    }

    // epilogue: O/l and LSE
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int qg = qrow0 + r;
        if (qg >= Sq) continue;
        float inv_l = (l_run[r] > 0.f) ? 1.0f / l_run[r] : 0.f;
        ushort_t* orow = o + ((long long)b * Sq + qg) * q_row_stride + (long long)hq * D;
#pragma unroll
        for (int n = 0; n < ND; n++)
            orow[n * 16 + l16] = f32_to_bf16(acc_o[n][r] * inv_l);
        if (l16 == 0) {
            float lv = (l_run[r] > 0.f) ? (m_run[r] + __logf(l_run[r])) : -INFINITY;
            lse[((long long)b * Hq + hq) * Sq + qg] = lv;
        }
    }
}

// ---------------------------------------------------------------------------
// backward preprocess: delta[b,h,q] = rowsum(dO * O).  Shared with the v2
// backward (flash_attn_bwd_v2.hip) through launch_flash_bwd_delta.
//
// A block takes DELTA_QT consecutive q positions of one batch entry with all
// their heads: DELTA_QT*Hq rows that are contiguous in dO and O.  D/8 lanes
// share a row (one 16-byte load of each tensor per lane, 64/(D/8) rows per
// wave) and the row sums go through LDS, which turns the [q][h] order they
// are produced in into the [h][q] order of delta: every head's DELTA_QT
// floats are written as one contiguous segment.
// ---------------------------------------------------------------------------
#define DELTA_BLOCK 256
#define DELTA_QT 32
template <int D>
__global__ __launch_bounds__(DELTA_BLOCK) void flash_bwd_delta_kernel(
    const ushort_t* __restrict__ dout, const ushort_t* __restrict__ o,
    float* __restrict__ delta, int B, int Sq, int Hq) {
    constexpr int LPR = D / 8;                  // lanes per row
    constexpr int RPI = DELTA_BLOCK / LPR;      // rows per block iteration
    extern __shared__ float delta_lds[];        // [Hq][DELTA_QT + 1]
    const int ntq = (Sq + DELTA_QT - 1) / DELTA_QT;
    const int b = blockIdx.x / ntq;
    const int q0 = (blockIdx.x % ntq) * DELTA_QT;
    const int nq = min(DELTA_QT, Sq - q0);
    const int nrows = nq * Hq;
    const long long base = ((long long)b * Sq + q0) * Hq * D + (threadIdx.x % LPR) * 8;
    const ushort_t* dop = dout + base;
    const ushort_t* op = o + base;
#pragma unroll 4
    for (int r = threadIdx.x / LPR; r < nrows; r += RPI) {
        short8v dv = *reinterpret_cast<const short8v*>(dop + (long long)r * D);
        short8v ov = *reinterpret_cast<const short8v*>(op + (long long)r * D);
        // Summation tree of the one-row-per-wave kernel this replaces (lane l
        // summed elements 2l and 2l+1, then a 64-lane xor butterfly from
        // offset 32 down to 1), so delta, and dq/dk/dv after it, keep their
        // bits: pair sums pr[m] stand for that kernel's lanes 4*j + m (j =
        // this lane within the row); butterfly over j first, then over m.
        float pr[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            pr[m] = 0.f;
            pr[m] += bf16_to_f32((ushort_t)dv[2 * m]) * bf16_to_f32((ushort_t)ov[2 * m]);
            pr[m] += bf16_to_f32((ushort_t)dv[2 * m + 1]) * bf16_to_f32((ushort_t)ov[2 * m + 1]);
        }
#pragma unroll
        for (int off = LPR / 2; off > 0; off >>= 1)
#pragma unroll
            for (int m = 0; m < 4; m++) pr[m] += __shfl_xor(pr[m], off, 64);
        float acc = (pr[0] + pr[2]) + (pr[1] + pr[3]);
        if (threadIdx.x % LPR == 0)
            delta_lds[(r % Hq) * (DELTA_QT + 1) + r / Hq] = acc;   // r = qi*Hq + h
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < Hq * DELTA_QT; idx += DELTA_BLOCK) {
        int h = idx / DELTA_QT, qi = idx % DELTA_QT;
        if (qi < nq)
            delta[((long long)b * Hq + h) * Sq + q0 + qi] = delta_lds[h * (DELTA_QT + 1) + qi];
    }
}
// ---------------------------------------------------------------------------
// backward dQ: fixed q tile, loop kv tiles.
//   S = scale*QK^T; P = exp(S - lse); dP = dO V^T;
//   dS = P*(dP - delta)*scale; dQ += dS K
// LDS: K row-major (S B-frag), V row-major (dP B-frag),
//      K^T (dQ B-frag), dS staging.
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(FA_BLOCK) void flash_bwd_dq_kernel(
    const ushort_t* __restrict__ q, const ushort_t* __restrict__ k,
    const ushort_t* __restrict__ v, const ushort_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    ushort_t* __restrict__ dq, const int* __restrict__ startend,
    int B, int Sq, int Skv, int Hq, int Hk, float scale, int causal) {
    constexpr int KD = D / 32;
    constexpr int ND = D / 16;
    constexpr int NN = BLK_N / 16;
    constexpr int LDK = D + LDS_PAD;
    constexpr int LDT = BLK_N + LDS_PAD;

    __shared__ ushort_t k_lds[BLK_N][LDK];
    __shared__ ushort_t v_lds[BLK_N][LDK];
    __shared__ ushort_t kt_lds[D][LDT];
    __shared__ ushort_t ds_lds[BLK_M][LDT];

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int l16 = lane & 15;
    const int lk8 = (lane >> 4) * 8;

    int qt, bh;
    if ((gridDim.y & 7) == 0) {
        // XCD-aware remap (see flash_attn_v2.hip): one (b,h) per XCD
        const int flat = blockIdx.x + gridDim.x * blockIdx.y;
        const int idx = flat >> 3;
        qt = idx % gridDim.x;
        bh = (flat & 7) * (gridDim.y >> 3) + idx / gridDim.x;
    } else {
        qt = blockIdx.x;
        bh = blockIdx.y;
    }
    const int b = bh / Hq, hq = bh % Hq;
    const int hk = hq / (Hq / Hk);
    const int q_base = qt * BLK_M;
    const int causal_off = Skv - Sq;

    const long long q_row_stride = (long long)Hq * D;
    const long long kv_row_stride = (long long)Hk * D;
    const ushort_t* q_ptr = q + ((long long)b * Sq * Hq + hq) * D;
    const ushort_t* k_ptr = k + ((long long)b * Skv * Hk + hk) * D;
    const ushort_t* v_ptr = v + ((long long)b * Skv * Hk + hk) * D;
    const ushort_t* do_ptr = dout + ((long long)b * Sq * Hq + hq) * D;
    const float* lse_row = lse + ((long long)b * Hq + hq) * Sq;
    const float* dl_row = delta + ((long long)b * Hq + hq) * Sq;

    frag8 aq[KD], ado[KD];
    {
        int qrow = q_base + wave * 16 + l16;
        if (qrow < Sq) {
#pragma unroll
            for (int kk = 0; kk < KD; kk++) {
                aq[kk] = *reinterpret_cast<const frag8*>(
                    q_ptr + (long long)qrow * q_row_stride + kk * 32 + lk8);
                ado[kk] = *reinterpret_cast<const frag8*>(
                    do_ptr + (long long)qrow * q_row_stride + kk * 32 + lk8);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < KD; kk++) { aq[kk] = frag8{0}; ado[kk] = frag8{0}; }
        }
    }
    const int qrow0 = q_base + wave * 16 + (lane >> 4) * 4;
    float lse_r[4], dl_r[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int qg = qrow0 + r;
        lse_r[r] = (qg < Sq) ? lse_row[qg] : INFINITY;
        dl_r[r] = (qg < Sq) ? dl_row[qg] : 0.f;
    }

    f32x4 acc_dq[ND];
#pragma unroll
    for (int n = 0; n < ND; n++) acc_dq[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    int n_kv_tiles = (Skv + BLK_N - 1) / BLK_N;
    if (causal) {
        int max_kv = q_base + BLK_M - 1 + causal_off;
        int lim = (max_kv + BLK_N) / BLK_N;
        n_kv_tiles = min(n_kv_tiles, max(lim, 0));
    }

    for (int kvt = 0; kvt < n_kv_tiles; kvt++) {
        const int kv_base = kvt * BLK_N;
        for (int idx = tid * 8; idx < (BLK_N / 2) * D; idx += FA_BLOCK * 8) {
            int rr = idx / D, col = idx % D;
            int row0 = rr * 2;
            int kvg0 = kv_base + row0;
            short8v k8a = {0,0,0,0,0,0,0,0}, k8b = {0,0,0,0,0,0,0,0};
            short8v v8a = {0,0,0,0,0,0,0,0}, v8b = {0,0,0,0,0,0,0,0};
            if (kvg0 < Skv) {
                k8a = *reinterpret_cast<const short8v*>(k_ptr + (long long)kvg0 * kv_row_stride + col);
                v8a = *reinterpret_cast<const short8v*>(v_ptr + (long long)kvg0 * kv_row_stride + col);
            }
            if (kvg0 + 1 < Skv) {
                k8b = *reinterpret_cast<const short8v*>(k_ptr + (long long)(kvg0 + 1) * kv_row_stride + col);
                v8b = *reinterpret_cast<const short8v*>(v_ptr + (long long)(kvg0 + 1) * kv_row_stride + col);
            }
            *reinterpret_cast<short8v*>(&k_lds[row0][col]) = k8a;
            *reinterpret_cast<short8v*>(&k_lds[row0 + 1][col]) = k8b;
            *reinterpret_cast<short8v*>(&v_lds[row0][col]) = v8a;
            *reinterpret_cast<short8v*>(&v_lds[row0 + 1][col]) = v8b;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                unsigned int packed = ((unsigned int)(unsigned short)k8a[j]) |
                                      (((unsigned int)(unsigned short)k8b[j]) << 16);
                *reinterpret_cast<unsigned int*>(&kt_lds[col + j][row0]) = packed;
            }
        }
        __syncthreads();

        // S and dP
        f32x4 acc_s[NN], acc_dp[NN];
#pragma unroll
        for (int n = 0; n < NN; n++) {
            acc_s[n] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc_dp[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KD; kk++) {
                frag8 bk = *reinterpret_cast<const frag8*>(&k_lds[n * 16 + l16][kk * 32 + lk8]);
                frag8 bv = *reinterpret_cast<const frag8*>(&v_lds[n * 16 + l16][kk * 32 + lk8]);
                acc_s[n] = mfma16(aq[kk], bk, acc_s[n]);
                acc_dp[n] = mfma16(ado[kk], bv, acc_dp[n]);
            }
        }

        // dS = P * (dP - delta) * scale   (C layout)
#pragma unroll
        for (int n = 0; n < NN; n++) {
            int kvg = kv_base + n * 16 + l16;
            int kv_end = (startend && kvg < Skv)
                             ? startend[(long long)b * Skv + kvg] : Sq + causal_off;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                int qg = qrow0 + r;
                bool vis = (kvg < Skv) && (qg < Sq);
                if (causal) vis = vis && (kvg <= qg + causal_off);
                if (startend) vis = vis && (qg < kv_end);
                float p = vis ? __expf(acc_s[n][r] * scale - lse_r[r]) : 0.f;
                float ds = p * (acc_dp[n][r] - dl_r[r]) * scale;
                ds_lds[wave * 16 + (lane >> 4) * 4 + r][n * 16 + l16] = f32_to_bf16(ds);
            }
        }
        // ds_lds rows are wave-private: wave-local LDS drain suffices
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

        // dQ += dS K  (contract kv; B from kt_lds)
#pragma unroll
        for (int kk = 0; kk < BLK_N / 32; kk++) {
            frag8 ads = *reinterpret_cast<const frag8*>(&ds_lds[wave * 16 + l16][kk * 32 + lk8]);
#pragma unroll
            for (int n = 0; n < ND; n++) {
                frag8 bkt = *reinterpret_cast<const frag8*>(&kt_lds[n * 16 + l16][kk * 32 + lk8]);
                acc_dq[n] = mfma16(ads, bkt, acc_dq[n]);
            }
        }
        __syncthreads();
    }

    // store dQ
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int qg = qrow0 + r;
        if (qg >= Sq) continue;
        ushort_t* dqr = dq + ((long long)b * Sq + qg) * q_row_stride + (long long)hq * D;
#pragma unroll
        for (int n = 0; n < ND; n++)
            dqr[n * 16 + l16] = f32_to_bf16(acc_dq[n][r]);
    }
}

// ---------------------------------------------------------------------------
// backward dK/dV: fixed kv tile, loop q tiles.  Wave owns 16 kv rows.
//   S^T = scale*K Q^T;  P^T = exp(S^T - lse[q]);
//   dV += P^T dO;  dP^T = V dO^T;  dS^T = P^T*(dP^T - delta[q])*scale;
//   dK += dS^T Q
// GQA: outputs are PER Q-HEAD ([B, Skv, Hq, D]); python sums head groups.
// LDS: Q row-major (S^T B), Q^T (dK B), dO row-major (dP^T B),
//      dO^T (dV B), P^T/dS^T staging (one reused buffer).
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(FA_BLOCK) void flash_bwd_dkv_kernel(
    const ushort_t* __restrict__ q, const ushort_t* __restrict__ k,
    const ushort_t* __restrict__ v, const ushort_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    ushort_t* __restrict__ dk,   // [B, Skv, Hk, D] (GQA group summed in-kernel)
    ushort_t* __restrict__ dv,   // [B, Skv, Hk, D]
    const int* __restrict__ startend,
    int B, int Sq, int Skv, int Hq, int Hk, float scale, int causal) {
    constexpr int KD = D / 32;
    constexpr int ND = D / 16;
    constexpr int NN = BLK_M / 16;  // q-frags per tile
    constexpr int LDK = D + LDS_PAD;
    constexpr int LDT = BLK_M + LDS_PAD;

    __shared__ ushort_t q_lds[BLK_M][LDK];
    __shared__ ushort_t do_lds[BLK_M][LDK];
    __shared__ ushort_t qt_lds[D][LDT];
    __shared__ ushort_t dot_lds[D][LDT];
    __shared__ ushort_t pt_lds[BLK_N][LDT];  // P^T then dS^T (reused)

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int l16 = lane & 15;
    const int lk8 = (lane >> 4) * 8;

    int kvt, bh;
    if ((gridDim.y & 7) == 0) {
        // XCD-aware remap (see flash_attn_v2.hip): one (b,h) per XCD
        const int flat = blockIdx.x + gridDim.x * blockIdx.y;
        const int idx = flat >> 3;
        kvt = idx % gridDim.x;
        bh = (flat & 7) * (gridDim.y >> 3) + idx / gridDim.x;
    } else {
        kvt = blockIdx.x;
        bh = blockIdx.y;
    }
    const int b = bh / Hk, hk = bh % Hk;
    const int G = Hq / Hk;               // q heads accumulated in-kernel
    const int kv_base = kvt * BLK_N;
    const int causal_off = Skv - Sq;

    const long long q_row_stride = (long long)Hq * D;
    const long long kv_row_stride = (long long)Hk * D;
    const ushort_t* k_ptr = k + ((long long)b * Skv * Hk + hk) * D;
    const ushort_t* v_ptr = v + ((long long)b * Skv * Hk + hk) * D;

    // K and V A-frags in registers (wave's 16 kv rows, fixed all kernel)
    frag8 ak[KD], av[KD];
    {
        int kvrow = kv_base + wave * 16 + l16;
        if (kvrow < Skv) {
#pragma unroll
            for (int kk = 0; kk < KD; kk++) {
                ak[kk] = *reinterpret_cast<const frag8*>(
                    k_ptr + (long long)kvrow * kv_row_stride + kk * 32 + lk8);
                av[kk] = *reinterpret_cast<const frag8*>(
                    v_ptr + (long long)kvrow * kv_row_stride + kk * 32 + lk8);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < KD; kk++) { ak[kk] = frag8{0}; av[kk] = frag8{0}; }
        }
    }

    f32x4 acc_dk[ND], acc_dv[ND];
#pragma unroll
    for (int n = 0; n < ND; n++) {
        acc_dk[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc_dv[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    int qt_start = 0;
    if (causal) {
        // first q that can see kv_base: q >= kv_base - off
        int first_q = kv_base - causal_off;
        if (first_q > 0) qt_start = first_q / BLK_M;
    }
    int n_q_tiles = (Sq + BLK_M - 1) / BLK_M;

    // accumulate the whole GQA group into acc_dk/acc_dv: K/V stream from HBM
    // once per kv head, and the outputs are written [B, Skv, Hk, D] directly
    // (no per-q-head buffers + reduction pass)
    for (int g = 0; g < G; g++) {
    const int hq = hk * G + g;
    const ushort_t* q_ptr = q + ((long long)b * Sq * Hq + hq) * D;
    const ushort_t* do_ptr = dout + ((long long)b * Sq * Hq + hq) * D;
    const float* lse_row = lse + ((long long)b * Hq + hq) * Sq;
    const float* dl_row = delta + ((long long)b * Hq + hq) * Sq;
    for (int qt = qt_start; qt < n_q_tiles; qt++) {
        const int q_base = qt * BLK_M;
        for (int idx = tid * 8; idx < (BLK_M / 2) * D; idx += FA_BLOCK * 8) {
            int rr = idx / D, col = idx % D;
            int row0 = rr * 2;
            int qg0 = q_base + row0;
            short8v q8a = {0,0,0,0,0,0,0,0}, q8b = {0,0,0,0,0,0,0,0};
            short8v d8a = {0,0,0,0,0,0,0,0}, d8b = {0,0,0,0,0,0,0,0};
            if (qg0 < Sq) {
                q8a = *reinterpret_cast<const short8v*>(q_ptr + (long long)qg0 * q_row_stride + col);
                d8a = *reinterpret_cast<const short8v*>(do_ptr + (long long)qg0 * q_row_stride + col);
            }
            if (qg0 + 1 < Sq) {
                q8b = *reinterpret_cast<const short8v*>(q_ptr + (long long)(qg0 + 1) * q_row_stride + col);
                d8b = *reinterpret_cast<const short8v*>(do_ptr + (long long)(qg0 + 1) * q_row_stride + col);
            }
            *reinterpret_cast<short8v*>(&q_lds[row0][col]) = q8a;
            *reinterpret_cast<short8v*>(&q_lds[row0 + 1][col]) = q8b;
            *reinterpret_cast<short8v*>(&do_lds[row0][col]) = d8a;
            *reinterpret_cast<short8v*>(&do_lds[row0 + 1][col]) = d8b;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                unsigned int pq = ((unsigned int)(unsigned short)q8a[j]) |
                                  (((unsigned int)(unsigned short)q8b[j]) << 16);
                unsigned int pd = ((unsigned int)(unsigned short)d8a[j]) |
                                  (((unsigned int)(unsigned short)d8b[j]) << 16);
                *reinterpret_cast<unsigned int*>(&qt_lds[col + j][row0]) = pq;
                *reinterpret_cast<unsigned int*>(&dot_lds[col + j][row0]) = pd;
            }
        }
        __syncthreads();

        // S^T = K Q^T and dP^T = V dO^T   (M = kv, N = q, contract d)
        f32x4 acc_s[NN], acc_dp[NN];
#pragma unroll
        for (int n = 0; n < NN; n++) {
            acc_s[n] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc_dp[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KD; kk++) {
                frag8 bq = *reinterpret_cast<const frag8*>(&q_lds[n * 16 + l16][kk * 32 + lk8]);
                frag8 bdo = *reinterpret_cast<const frag8*>(&do_lds[n * 16 + l16][kk * 32 + lk8]);
                acc_s[n] = mfma16(ak[kk], bq, acc_s[n]);
                acc_dp[n] = mfma16(av[kk], bdo, acc_dp[n]);
            }
        }

        // P^T (C layout: row = kv, col = q); lse/delta gathered per col
        const int kvrow0 = kv_base + wave * 16 + (lane >> 4) * 4;
        float pt_vals[NN][4], dst_vals[NN][4];
#pragma unroll
        for (int n = 0; n < NN; n++) {
            int qg = q_base + n * 16 + l16;
            float lse_q = (qg < Sq) ? lse_row[qg] : INFINITY;
            float dl_q = (qg < Sq) ? dl_row[qg] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                int kvg = kvrow0 + r;
                bool vis = (kvg < Skv) && (qg < Sq);
                if (causal) vis = vis && (kvg <= qg + causal_off);
                if (startend) vis = vis && (kvg < Skv) &&
                    (qg < startend[(long long)b * Skv + kvg]);
                float p = vis ? __expf(acc_s[n][r] * scale - lse_q) : 0.f;
                pt_vals[n][r] = p;
                dst_vals[n][r] = p * (acc_dp[n][r] - dl_q) * scale;
            }
        }

        // stage P^T; dV += P^T dO (contract q; B from dot_lds)
#pragma unroll
        for (int n = 0; n < NN; n++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                pt_lds[wave * 16 + (lane >> 4) * 4 + r][n * 16 + l16] =
                    f32_to_bf16(pt_vals[n][r]);
        // pt_lds rows are wave-private: wave-local drain, no block barrier
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int kk = 0; kk < BLK_M / 32; kk++) {
            frag8 apt = *reinterpret_cast<const frag8*>(&pt_lds[wave * 16 + l16][kk * 32 + lk8]);
#pragma unroll
            for (int n = 0; n < ND; n++) {
                frag8 bdot = *reinterpret_cast<const frag8*>(&dot_lds[n * 16 + l16][kk * 32 + lk8]);
                acc_dv[n] = mfma16(apt, bdot, acc_dv[n]);
            }
        }
        // the pt_lds reads above are this wave's own rows; overwriting with
        // dS^T next is also wave-local (no cross-wave barrier)

        // stage dS^T; dK += dS^T Q (contract q; B from qt_lds)
#pragma unroll
        for (int n = 0; n < NN; n++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                pt_lds[wave * 16 + (lane >> 4) * 4 + r][n * 16 + l16] =
                    f32_to_bf16(dst_vals[n][r]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int kk = 0; kk < BLK_M / 32; kk++) {
            frag8 adst = *reinterpret_cast<const frag8*>(&pt_lds[wave * 16 + l16][kk * 32 + lk8]);
#pragma unroll
            for (int n = 0; n < ND; n++) {
                frag8 bqt = *reinterpret_cast<const frag8*>(&qt_lds[n * 16 + l16][kk * 32 + lk8]);
                acc_dk[n] = mfma16(adst, bqt, acc_dk[n]);
            }
        }
        __syncthreads();
    }
    }  // g loop over the GQA group

    // store dK/dV directly in [B, Skv, Hk, D]
    const int kvrow0 = kv_base + wave * 16 + (lane >> 4) * 4;
    const long long out_row_stride = (long long)Hk * D;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int kvg = kvrow0 + r;
        if (kvg >= Skv) continue;
        long long base = ((long long)b * Skv + kvg) * out_row_stride + (long long)hk * D;
#pragma unroll
        for (int n = 0; n < ND; n++) {
            dk[base + n * 16 + l16] = f32_to_bf16(acc_dk[n][r]);
            dv[base + n * 16 + l16] = f32_to_bf16(acc_dv[n][r]);
        }
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void launch_mfma_probe(const void* A, const void* B, float* C, hipStream_t stream) {
    hipLaunchKernelGGL(mfma_layout_probe, dim3(1), dim3(64), 0, stream,
                       (const ushort_t*)A, (const ushort_t*)B, C);
}

// PNLP_FLASHMASK_KERNEL=1 forces the v1 FlashMask kernels (A/B against v2)
static bool flashmask_force_v1() {
    static const bool force = [] {
        const char* e = getenv("PNLP_FLASHMASK_KERNEL");
        return e && e[0] == '1';
    }();
    return force;
}

template <int D>
static void flash_fwd_t(const void* q, const void* k, const void* v, void* o,
                        float* lse, const int* startend,
                        int B, int Sq, int Skv, int Hq, int Hk,
                        float scale, bool causal, hipStream_t stream) {
    dim3 grid((Sq + BLK_M - 1) / BLK_M, B * Hq);
    hipLaunchKernelGGL((flash_fwd_kernel<D>), grid, dim3(FA_BLOCK), 0, stream,
                       (const ushort_t*)q, (const ushort_t*)k, (const ushort_t*)v,
                       (ushort_t*)o, lse, startend, B, Sq, Skv, Hq, Hk, scale,
                       causal ? 1 : 0);
}

static void flash_fwd_v1(const void* q, const void* k, const void* v, void* o,
                         float* lse, const int* startend,
                         int B, int Sq, int Skv, int Hq, int Hk, int D,
                         float scale, bool causal, hipStream_t stream) {
    switch (D) {
        case 128: flash_fwd_t<128>(q, k, v, o, lse, startend, B, Sq, Skv, Hq, Hk, scale, causal, stream); break;
        case 64: flash_fwd_t<64>(q, k, v, o, lse, startend, B, Sq, Skv, Hq, Hk, scale, causal, stream); break;
        case 32: flash_fwd_t<32>(q, k, v, o, lse, startend, B, Sq, Skv, Hq, Hk, scale, causal, stream); break;
        default: unsupported_head_dim("flash attention forward", D);
    }
}

void launch_flash_fwd(const void* q, const void* k, const void* v, void* o,
                      float* lse, int B, int Sq, int Skv, int Hq, int Hk, int D,
                      float scale, bool causal, bool force_v1, hipStream_t stream) {
    if (!force_v1 &&
        launch_flash_fwd2(q, k, v, o, lse, B, Sq, Skv, Hq, Hk, D, scale, causal, stream))
        return;
    flash_fwd_v1(q, k, v, o, lse, nullptr, B, Sq, Skv, Hq, Hk, D, scale, causal, stream);
}

void launch_flash_fwd_mask(const void* q, const void* k, const void* v, void* o,
                           float* lse, const int* startend,
                           int B, int Sq, int Skv, int Hq, int Hk, int D,
                           float scale, hipStream_t stream) {
    if (!flashmask_force_v1() &&
        launch_flash_fwd2_mask(q, k, v, o, lse, startend,
                               B, Sq, Skv, Hq, Hk, D, scale, stream))
        return;
    flash_fwd_v1(q, k, v, o, lse, startend, B, Sq, Skv, Hq, Hk, D, scale, true, stream);
}

template <int D>
static void flash_bwd_delta_t(const void* dout, const void* o, float* delta,
                              int B, int Sq, int Hq, hipStream_t stream) {
    if (B <= 0 || Sq <= 0) return;
    size_t lds = (size_t)Hq * (DELTA_QT + 1) * sizeof(float);
    if (lds > 64 * 1024)
        throw std::runtime_error("flash attention backward: delta kernel takes at most " +
                                 std::to_string(64 * 1024 / ((DELTA_QT + 1) * 4)) + " heads");
    int grid = B * ((Sq + DELTA_QT - 1) / DELTA_QT);
    hipLaunchKernelGGL(flash_bwd_delta_kernel<D>, dim3(grid), dim3(DELTA_BLOCK), lds, stream,
                       (const ushort_t*)dout, (const ushort_t*)o, delta, B, Sq, Hq);
}

void launch_flash_bwd_delta(const void* dout, const void* o, float* delta,
                            int B, int Sq, int Hq, int D, hipStream_t stream) {
    switch (D) {
        case 128: flash_bwd_delta_t<128>(dout, o, delta, B, Sq, Hq, stream); break;
        case 64: flash_bwd_delta_t<64>(dout, o, delta, B, Sq, Hq, stream); break;
        case 32: flash_bwd_delta_t<32>(dout, o, delta, B, Sq, Hq, stream); break;
        default: unsupported_head_dim("flash attention backward", D);
    }
}

template <int D>
static void flash_bwd_t(const void* dout, const void* q, const void* k, const void* v,
                        const float* lse, const float* delta,
                        void* dq, void* dk, void* dv, const int* startend,
                        int B, int Sq, int Skv, int Hq, int Hk,
                        float scale, bool causal, hipStream_t stream) {
    dim3 gq((Sq + BLK_M - 1) / BLK_M, B * Hq);
    hipLaunchKernelGGL((flash_bwd_dq_kernel<D>), gq, dim3(FA_BLOCK), 0, stream,
                       (const ushort_t*)q, (const ushort_t*)k, (const ushort_t*)v,
                       (const ushort_t*)dout, lse, delta, (ushort_t*)dq, startend,
                       B, Sq, Skv, Hq, Hk, scale, causal ? 1 : 0);
    dim3 gkv((Skv + BLK_N - 1) / BLK_N, B * Hk);
    hipLaunchKernelGGL((flash_bwd_dkv_kernel<D>), gkv, dim3(FA_BLOCK), 0, stream,
                       (const ushort_t*)q, (const ushort_t*)k, (const ushort_t*)v,
                       (const ushort_t*)dout, lse, delta, (ushort_t*)dk, (ushort_t*)dv,
                       startend, B, Sq, Skv, Hq, Hk, scale, causal ? 1 : 0);
}

static void flash_bwd_v1(const void* dout, const void* q, const void* k, const void* v,
                         const void* o, const float* lse, float* delta,
                         void* dq, void* dk, void* dv, const int* startend,
                         int B, int Sq, int Skv, int Hq, int Hk, int D,
                         float scale, bool causal, hipStream_t stream) {
    launch_flash_bwd_delta(dout, o, delta, B, Sq, Hq, D, stream);
    switch (D) {
        case 128: flash_bwd_t<128>(dout, q, k, v, lse, delta, dq, dk, dv, startend, B, Sq, Skv, Hq, Hk, scale, causal, stream); break;
        case 64: flash_bwd_t<64>(dout, q, k, v, lse, delta, dq, dk, dv, startend, B, Sq, Skv, Hq, Hk, scale, causal, stream); break;
        case 32: flash_bwd_t<32>(dout, q, k, v, lse, delta, dq, dk, dv, startend, B, Sq, Skv, Hq, Hk, scale, causal, stream); break;
        default: unsupported_head_dim("flash attention backward", D);
    }
}

void launch_flash_bwd(const void* dout, const void* q, const void* k, const void* v,
                      const void* o, const float* lse, float* delta,
                      void* dq, void* dk, void* dv,
                      int B, int Sq, int Skv, int Hq, int Hk, int D,
                      float scale, bool causal, bool force_v1, hipStream_t stream) {
    if (!force_v1 &&
        launch_flash_bwd2(dout, q, k, v, o, lse, delta, dq, dk, dv,
                          B, Sq, Skv, Hq, Hk, D, scale, causal, stream))
        return;
    flash_bwd_v1(dout, q, k, v, o, lse, delta, dq, dk, dv, nullptr,
                 B, Sq, Skv, Hq, Hk, D, scale, causal, stream);
}

void launch_flash_bwd_mask(const void* dout, const void* q, const void* k, const void* v,
                           const void* o, const float* lse, float* delta,
                           void* dq, void* dk, void* dv, const int* startend,
                           int B, int Sq, int Skv, int Hq, int Hk, int D,
                           float scale, hipStream_t stream) {
    if (!flashmask_force_v1() &&
        launch_flash_bwd2_mask(dout, q, k, v, o, lse, delta, dq, dk, dv,
                               startend, B, Sq, Skv, Hq, Hk, D, scale, stream))
        return;
    flash_bwd_v1(dout, q, k, v, o, lse, delta, dq, dk, dv, startend,
                 B, Sq, Skv, Hq, Hk, D, scale, true, stream);
}
