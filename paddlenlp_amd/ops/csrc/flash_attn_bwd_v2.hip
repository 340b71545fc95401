// FlashAttention-2 backward v2 — 8-wave 32x32 MFMA structure for gfx950.
//
// Same technique set as the v2 forward (flash_attn_v2.hip): 32x32x16
// MFMA, tiles staged by LDS-DMA into dual-use LDS images (read by rows and
// transposed, mfma.h img_off), in-register P/dS-to-fragment conversion via
// permlane32_swap.
//
// The key structural choice: backward has NO online softmax — lse and
// delta are precomputed arrays — so the C-layout orientation of the two
// recompute GEMMs is free.  Each kernel picks the orientation that makes
// P and dS directly convertible (cvt-pack + permlane32_swap, guide T12)
// into the A/B fragments of the GEMMs that consume them:
//
//   dKV kernel (kv stationary): compute S and dP in C-layout [q][kv]
//     (col = kv = lane's own column).  The T12 swap then yields, per
//     lane, P^T[kv = l&31][q-slice] — exactly the A-fragment of
//     dV += P^T·dO and dK += dS^T·Q.  No LDS round trip for P/dS.
//   dQ kernel (q stationary): compute S^T and dP^T in C-layout [kv][q]
//     (col = q).  The swap yields dS[q = l&31][kv-slice] — the
//     A-fragment of dQ += dS·K.
//
// v1 (flash_attn.hip) staged P^T/dS^T through LDS between every GEMM
// pair; measured A/B at the bench shape: v1 191 TF/s -> v2 (this file).
//
// Softmax recompute (mfma.h, profiles/fa_softmax_diet.md): both kernels
// take a wave-uniform full-tile path per 32 x 32 sub-block with no compare
// and no select; the masked path (diagonal, ragged and FlashMask boundary
// tiles) selects masked pairs to exact zeros after the arithmetic.  P and dS
// are rounded exactly as before (fma, mul, exp, sub, mul, mul per score), so
// dq, dk and dv keep their bits; no packed f32 VALU; bf16 pairs packed by one
// v_cvt_pk_bf16_f32; the dkv kernel reads lse and delta 16 bytes at a time.
// (Starting the chains from the row constants and moving the scale of dS to
// the epilogue is faster still but moves the last place of dS, and with it
// the benchmark's outputs: not used.)
#include "launchers.h"
#include "mfma.h"

#define FB2_WAVES 8
#define FB2_BLOCK (FB2_WAVES * 64)

// ---------------------------------------------------------------------------
// dQ kernel: q stationary (8 waves x 32 q = 256 q rows/block), kv iterated
// in tiles of 64.  Orientation: S^T and dP^T in C-layout [kv][q] so lse and
// delta are per-lane scalars (q = lane&31) and the T12 swap hands dS to the
// dQ MFMA directly.
// ---------------------------------------------------------------------------
template <int D, bool MASKED = false>
__global__ __launch_bounds__(FB2_BLOCK) void flash_bwd2_dq_kernel(
    const ushort_t* __restrict__ q, const ushort_t* __restrict__ k,
    const ushort_t* __restrict__ v, const ushort_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    ushort_t* __restrict__ dq, const int* __restrict__ startend,
    FlashStrides rs,   // row strides (elements) of q, k/v, dq; dout is contiguous
    int B, int Sq, int Skv, int Hq, int Hk, float scale, int causal) {
    static_assert(D == 128, "the dual-use image is laid out for 128-column tiles");
    constexpr int BLKN = 64;
    constexpr int DSTEPS = D / 16;
    constexpr int NDT = D / 32;
    constexpr int BLKM = FB2_WAVES * 32;

    // [buffer][0 = K, 1 = V] dual-use images filled by LDS-DMA, double-
    // buffered with one barrier per KV tile; FlashMask bounds in three slots,
    // filled two tiles ahead (see flash_attn_v2.hip)
    __shared__ __attribute__((aligned(16))) ushort_t kv_lds[2][2][BLKN * D];
    __shared__ int se_lds[3][MASKED ? BLKN : 1];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int l32 = lane & 31;
    const int hi = lane >> 5;

    // one (b,h)'s tiles stay on one XCD (shared K/V re-hit its L2); heaviest
    // q tiles first (see mfma.h xcd_grouped_tile)
    int qt, bh;
    xcd_grouped_tile<FA_ORDER_W, false>(qt, bh);
    const int b = bh / Hq, hq = bh % Hq;
    const int hk = hq / (Hq / Hk);
    const int q_base = qt * BLKM;
    const int qw = q_base + wave * 32;
    const int qg = qw + l32;
    const int causal_off = Skv - Sq;

    // q, k, v, dq point at head 0 of token 0 and may be slices of a packed
    // [B, S, (Hq + 2*Hk)*D] tensor (see flash_attn_v2.hip)
    const long long q_row_stride = rs.q;
    const long long kv_row_stride = rs.kv;
    const long long do_row_stride = (long long)Hq * D;
    const ushort_t* q_ptr = q + (long long)b * Sq * q_row_stride + (long long)hq * D;
    const ushort_t* do_ptr = dout + ((long long)b * Sq * Hq + hq) * D;
    const ushort_t* k_ptr = k + (long long)b * Skv * kv_row_stride + (long long)hk * D;
    const ushort_t* v_ptr = v + (long long)b * Skv * kv_row_stride + (long long)hk * D;

    // stationary per-lane: Q^T and dO^T B-fragments (one q row each)
    frag8 aq[DSTEPS], ado[DSTEPS];
    float lse_q = INFINITY, dl_q = 0.f;
    if (qg < Sq) {
#pragma unroll
        for (int kk = 0; kk < DSTEPS; kk++) {
            aq[kk] = *reinterpret_cast<const frag8*>(
                q_ptr + (long long)qg * q_row_stride + kk * 16 + hi * 8);
            ado[kk] = *reinterpret_cast<const frag8*>(
                do_ptr + (long long)qg * do_row_stride + kk * 16 + hi * 8);
        }
        lse_q = lse[((long long)b * Hq + hq) * Sq + qg];
        dl_q = delta[((long long)b * Hq + hq) * Sq + qg];
    } else {
#pragma unroll
        for (int kk = 0; kk < DSTEPS; kk++) { aq[kk] = frag8{0}; ado[kk] = frag8{0}; }
    }

    f32x16 acc_dq[NDT];
#pragma unroll
    for (int n = 0; n < NDT; n++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc_dq[n][r] = 0.f;

    int n_kv_tiles = (Skv + BLKN - 1) / BLKN;
    if (causal) {
        int max_kv = q_base + BLKM - 1 + causal_off;
        int lim = (max_kv + BLKN) / BLKN;
        n_kv_tiles = min(n_kv_tiles, max(lim, 0));
    }

    // DMA of the kv tile at kv_base into buffer buf: each wave fills image
    // rows 8*wave .. +7 of K and of V (2 x 1 KiB each).  A ragged tile
    // cannot be zero-filled by DMA: rows past Skv re-read row Skv-1 (finite
    // data); the kvg < Skv visibility test makes P = 0 and dS = 0 there, so
    // the clamped K rows are multiplied by exact zeros.  The launcher checks
    // that the k/v bases and the row stride are 16-byte aligned.
    auto issue_tile = [&](int kv_base, int buf) {
        // recomputed per tile, not hoisted and spilled (see the dkv kernel)
        const int ln = fresh_lane_id();
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int piece = wave * 2 + i;
            const int src_row = min(kv_base + img_fill_row(piece, ln), Skv - 1);
            const long long off = (long long)src_row * kv_row_stride +
                                  img_fill_chunk(piece, ln) * 8;
            lds_dma16(k_ptr + off, &kv_lds[buf][0][piece * 512]);
            lds_dma16(v_ptr + off, &kv_lds[buf][1][piece * 512]);
        }
    };
    // FlashMask bounds of tile `tile` into slot tile % 3 (wave 0; columns
    // past Skv repeat the last one: the max is unchanged and their
    // kvg >= Skv test hides them)
    auto issue_bounds = [&](int tile, int slot) {
        if (MASKED && wave == 0) {
            const int ln = fresh_lane_id();
            lds_dma4(startend + (long long)b * Skv + min(tile * BLKN + ln, Skv - 1),
                     &se_lds[slot][0]);
        }
    };
    // per-wave (min, max) of a landed tile's 64 bounds, out of LDS: the max
    // drives the skips, the min the full-tile test
    auto tile_bounds = [&](int slot, int& mn_out) -> int {
        int mx = se_lds[slot][lane], mn = mx;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            mx = max(mx, __shfl_xor(mx, off, 64));
            mn = min(mn, __shfl_xor(mn, off, 64));
        }
        mn_out = __builtin_amdgcn_readfirstlane(mn);
        return __builtin_amdgcn_readfirstlane(mx);
    };

    // retire the stationary loads here: left pending, the compiler waits for
    // them with a counted vmcnt inside the tile loop, and that count would
    // also drain the (uncounted) DMA in flight
#pragma unroll
    for (int kk = 0; kk < DSTEPS; kk++)
        asm volatile("" :: "v"(aq[kk]), "v"(ado[kk]));
    asm volatile("" :: "v"(lse_q), "v"(dl_q));
    if (n_kv_tiles > 0) {
        issue_tile(0, 0);
        issue_bounds(0, 0);
        if (n_kv_tiles > 1) issue_bounds(1, 1);
    }
    int se_min_cur = 0, se_max_cur = 0x7fffffff;
    int se_slot = 0;   // kvt % 3

    for (int kvt = 0; kvt < n_kv_tiles; kvt++) {
        const int kv_base = kvt * BLKN;
        const int cur = kvt & 1;
        // tile kvt (and the bounds of kvt+1) have landed and every wave is
        // done reading the other buffer, which tile kvt+1 now overwrites
        // while tile kvt is computed
        lds_dma_wait_all();
        __syncthreads();
        const int se_slot_next = (se_slot == 2) ? 0 : se_slot + 1;
        if (MASKED && kvt == 0) se_max_cur = tile_bounds(0, se_min_cur);
        int se_min_next = 0, se_max_next = 0x7fffffff;
        if (kvt + 1 < n_kv_tiles) {
            bool stage_skip = false;
            if (MASKED) {
                se_max_next = tile_bounds(se_slot_next, se_min_next);
                // whole block past every bound: skip the K/V staging too
                stage_skip = (q_base >= se_max_next);
            }
            if (!stage_skip) issue_tile(kv_base + BLKN, cur ^ 1);
            // slot (kvt+2) % 3 was last read as tile kvt-1
            if (kvt + 2 < n_kv_tiles)
                issue_bounds(kvt + 2, (se_slot_next == 2) ? 0 : se_slot_next + 1);
        }
        const ushort_t* k_img = kv_lds[cur][0];
        const ushort_t* v_img = kv_lds[cur][1];
        const int lane_t = fresh_lane_id();   // for the transposed reads

        // wave-uniform: the transposed reads below need EXEC all ones
        bool wave_skip =
            causal && (kv_base > qw + 31 + causal_off);
        // FlashMask whole-tile skip (see fwd): no bound exceeds this
        // wave's first q row -> nothing visible
        if (MASKED && qw >= se_max_cur) wave_skip = true;

        // two 32-kv sub-iterations: one (S^T, dP^T) register pair live at
        // a time (register-pressure; see dkv kernel note)
        auto process_sub = [&](int sub) {
            f32x16 st, dp;
#pragma unroll
            for (int r = 0; r < 16; r++) { st[r] = 0.f; dp[r] = 0.f; }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < DSTEPS; kk++) {
                frag8 ak = img_row_frag(k_img, sub * 32 + l32, kk, hi);
                frag8 av = img_row_frag(v_img, sub * 32 + l32, kk, hi);
                st = mfma32(ak, aq[kk], st);
                dp = mfma32(av, ado[kk], dp);
            }
            __builtin_amdgcn_s_setprio(0);

            // P^T = exp(S^T*scale - lse_q); dS^T = P^T*(dP^T - delta_q)*
            // scale (all per-lane: q = l32), rounded as before.  When every
            // (q, kv) pair of this 32 x 32 sub-block is visible, the common
            // case away from the diagonal, there is no compare and no
            // select.  On the other path a masked pair is selected to an
            // exact 0 after the arithmetic, whatever its row's lse (-inf for
            // a row without keys, +inf past Sq) made of the exponent.
            const int kv_sub = kv_base + sub * 32;
            const bool full_sub =
                (kv_sub + 32 <= Skv) && (qw + 31 < Sq) &&
                (!causal || (kv_sub + 31 <= qw + causal_off)) &&
                (!MASKED || (qw + 31 < se_min_cur));
#pragma unroll
            for (int r = 0; r < 16; r++) {
                float p = __expf(__builtin_fmaf(st[r], scale, -lse_q));
                st[r] = sm_opaque(p * (dp[r] - dl_q) * scale);  // = dS^T
            }
            if (!full_sub) {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    int row = sub * 32 + crow32(r, hi);
                    int kvg = kv_base + row;
                    bool vis = (kvg < Skv) && (qg < Sq) &&
                               (!causal || kvg <= qg + causal_off);
                    if (MASKED) vis = vis && (qg < se_lds[se_slot][row]);
                    st[r] = vis ? st[r] : 0.f;
                }
            }

            // dQ += dS·K: A = T12(dS^T) (lane: dS[q=l32][kv-slice]),
            // B = K[kv][d] column slices: the K image read transposed
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ksl = 0; ksl < 2; ksl++) {
                const int ks = sub * 2 + ksl;
                frag8 ads = t12_convert(st, ksl * 8);
#pragma unroll
                for (int n = 0; n < NDT; n++) {
                    frag8 bkf = img_tr_frag(k_img, ks, n, lane_t);
                    acc_dq[n] = mfma32(ads, bkf, acc_dq[n]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        };

        if (!wave_skip) {
            process_sub(0);
            process_sub(1);
        }
        if (MASKED) { se_max_cur = se_max_next; se_min_cur = se_min_next; }
        se_slot = se_slot_next;
    }

    // epilogue: acc_dq C-layout [q][d] (col = d, row = q)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        int qrow = qw + crow32(r, hi);
        if (qrow >= Sq) continue;
        ushort_t* dqr = dq + ((long long)b * Sq + qrow) * rs.dq + (long long)hq * D;
#pragma unroll
        for (int n = 0; n < NDT; n++)
            dqr[n * 32 + l32] = f32_to_bf16(acc_dq[n][r]);
    }
}

// ---------------------------------------------------------------------------
// dKV kernel: kv stationary (8 waves x 32 kv = 256 kv rows/block), q iterated
// in tiles of 64 across the whole GQA group.  Orientation: S and dP in
// C-layout [q][kv] (col = kv) so T12 feeds dV += P^T·dO and dK += dS^T·Q.
//
// Staging: each 64 x 128 Q and dO tile lives in ONE dual-use LDS image
// (mfma.h img_off): S and dP read it by rows, dV and dK read the same bytes
// transposed with ds_read_b64_tr_b16.  The images and the tile's lse/delta
// are filled by LDS-DMA, which needs no staging registers, so tile t+1 is in
// flight into the other buffer while tile t is computed.  The GQA g-loop and
// the q-tile loop run as one flattened tile sequence: the pipeline is primed
// once per block, not once per g.
// ---------------------------------------------------------------------------
template <int D, bool MASKED = false>
__global__ __launch_bounds__(FB2_BLOCK, 1) void flash_bwd2_dkv_kernel(
    const ushort_t* __restrict__ q, const ushort_t* __restrict__ k,
    const ushort_t* __restrict__ v, const ushort_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    ushort_t* __restrict__ dk, ushort_t* __restrict__ dv,
    const int* __restrict__ startend,
    FlashStrides rs,   // row strides (elements) of q, k/v, dk/dv; dout is contiguous
    int B, int Sq, int Skv, int Hq, int Hk, float scale, int causal) {
    static_assert(D == 128, "the dual-use image is laid out for 128-column tiles");
    constexpr int BLKQ = 64;               // q tile
    constexpr int DSTEPS = D / 16;
    constexpr int NDT = D / 32;
    constexpr int BLKKV = FB2_WAVES * 32;  // 256 kv rows per block

    // [buffer][0 = Q, 1 = dO] dual-use images, [buffer][0 = lse, 1 = delta]
    __shared__ __attribute__((aligned(16))) ushort_t qd_lds[2][2][BLKQ * D];
    __shared__ __attribute__((aligned(16))) float ld_lds[2][2][BLKQ];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int l32 = lane & 31;
    const int hi = lane >> 5;

    // heaviest kv tiles first (see mfma.h xcd_grouped_tile)
    int kvt, bh;
    xcd_grouped_tile<FA_ORDER_W, true>(kvt, bh);
    const int b = bh / Hk, hk = bh % Hk;
    const int G = Hq / Hk;
    const int kv_base = kvt * BLKKV;
    const int kvw = kv_base + wave * 32;     // this wave's first kv row
    const int kvg_lane = kvw + l32;          // lane's kv column
    const int causal_off = Skv - Sq;
    // FlashMask: lane owns one kv column -> one bound scalar; the
    // wave-max bound drives whole-q-tile skipping and the BLOCK max ends
    // the tile sequence of every g: q tiles wholly past it are invisible
    // to every kv row in the block and are neither staged nor computed
    __shared__ int blk_max_lds[MASKED ? FB2_WAVES : 1];
    int kv_end_lane = 0x7fffffff;
    int wave_max_end = 0x7fffffff;
    int wave_min_end = 0x7fffffff;   // q rows below it clear every bound: full-tile test
    if (MASKED) {
        kv_end_lane = (kvg_lane < Skv)
            ? startend[(long long)b * Skv + kvg_lane] : 0;
        wave_max_end = kv_end_lane;
        wave_min_end = kv_end_lane;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            wave_max_end = max(wave_max_end,
                               __shfl_xor(wave_max_end, off, 64));
            wave_min_end = min(wave_min_end,
                               __shfl_xor(wave_min_end, off, 64));
        }
        wave_max_end = __builtin_amdgcn_readfirstlane(wave_max_end);
        wave_min_end = __builtin_amdgcn_readfirstlane(wave_min_end);
        if (lane == 0) blk_max_lds[wave] = wave_max_end;
    }

    const long long do_row_stride = (long long)Hq * D;
    const ushort_t* k_ptr = k + (long long)b * Skv * rs.kv + (long long)hk * D;
    const ushort_t* v_ptr = v + (long long)b * Skv * rs.kv + (long long)hk * D;

    // stationary per-lane: K^T and V^T B-fragments (one kv row each).
    // Ordinary global loads: they retire before the first DMA is issued.
    frag8 bk[DSTEPS], bv[DSTEPS];
    if (kvg_lane < Skv) {
#pragma unroll
        for (int kk = 0; kk < DSTEPS; kk++) {
            bk[kk] = *reinterpret_cast<const frag8*>(
                k_ptr + (long long)kvg_lane * rs.kv + kk * 16 + hi * 8);
            bv[kk] = *reinterpret_cast<const frag8*>(
                v_ptr + (long long)kvg_lane * rs.kv + kk * 16 + hi * 8);
        }
    } else {
#pragma unroll
        for (int kk = 0; kk < DSTEPS; kk++) { bk[kk] = frag8{0}; bv[kk] = frag8{0}; }
    }

    f32x16 acc_dk[NDT], acc_dv[NDT];
#pragma unroll
    for (int n = 0; n < NDT; n++)
#pragma unroll
        for (int r = 0; r < 16; r++) { acc_dk[n][r] = 0.f; acc_dv[n][r] = 0.f; }

    // q tiles [qt0, qt_end) of each g: under causal only q >= kv_base - off
    // contribute
    int qt0 = 0;
    if (causal) qt0 = max(0, (kv_base - causal_off) / BLKQ);
    int qt_end = (Sq + BLKQ - 1) / BLKQ;
    if (MASKED) {
        __syncthreads();
        int block_max_end = blk_max_lds[0];
#pragma unroll
        for (int w = 1; w < FB2_WAVES; w++)
            block_max_end = max(block_max_end, blk_max_lds[w]);
        block_max_end = __builtin_amdgcn_readfirstlane(block_max_end);
        if (block_max_end < Sq)
            qt_end = (max(block_max_end, 0) + BLKQ - 1) / BLKQ;
    }
    const int n_tiles = G * max(qt_end - qt0, 0);   // flattened (g, qt)

    // DMA of tile (g, qt) into buffer buf: each wave fills image rows
    // 8*wave .. +7 of Q and of dO (2 x 1 KiB each; waves 0/1: plus
    // lse/delta).  A ragged tile cannot be zero-filled by DMA: rows past Sq
    // re-read row Sq-1 (finite data) and the qgl < Sq visibility test zeroes
    // their P and dS.
    auto issue_tile = [&](int g, int qt, int buf) {
        const int hq = hk * G + g;
        // the DMA source must be 16-byte aligned: the launcher checks the q
        // base and row stride, a head starts at a multiple of 256 bytes
        const long long do_off = ((long long)b * Sq * Hq + hq) * D;
        const long long q_off = (long long)b * Sq * rs.q + (long long)hq * D;
        const int q_tb = qt * BLKQ;
        // the kernel sits at the register cap: recompute the per-lane source
        // offsets every tile (a few VALU ops) rather than let the compiler
        // hoist them out of the tile loop and spill them, since a scratch
        // reload after the DMA issue waits vmcnt(0) and drains the prefetch
        const int ln = fresh_lane_id();
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int piece = wave * 2 + i;
            const int src_row = min(q_tb + img_fill_row(piece, ln), Sq - 1);
            const int chunk = img_fill_chunk(piece, ln) * 8;
            lds_dma16(q + (q_off + (long long)src_row * rs.q + chunk),
                      &qd_lds[buf][0][piece * 512]);
            lds_dma16(dout + (do_off + (long long)src_row * do_row_stride + chunk),
                      &qd_lds[buf][1][piece * 512]);
        }
        if (wave < 2) {
            const float* row = (wave == 0 ? lse : delta) +
                               ((long long)b * Hq + hq) * Sq;
            lds_dma4(row + min(q_tb + ln, Sq - 1), &ld_lds[buf][wave][0]);
        }
    };

    int g_next = 0, qt_next = qt0;   // next tile to stage
    auto advance_next = [&]() {
        if (++qt_next == qt_end) { qt_next = qt0; g_next++; }
    };
    // retire the K/V fragment loads here: left pending, the compiler waits
    // for them with a counted vmcnt inside the tile loop, and that count
    // would also drain the (uncounted) DMA in flight
#pragma unroll
    for (int kk = 0; kk < DSTEPS; kk++)
        asm volatile("" :: "v"(bk[kk]), "v"(bv[kk]));
    if (n_tiles > 0) { issue_tile(g_next, qt_next, 0); advance_next(); }

    int qt = qt0;
    for (int t = 0; t < n_tiles; t++) {
        const int cur = t & 1;
        // tile t has landed (the compiler does not count the DMA, hence the
        // explicit wait) and every wave is done reading the other buffer,
        // which tile t+1 now overwrites while tile t is computed
        lds_dma_wait_all();
        __syncthreads();
        if (t + 1 < n_tiles) { issue_tile(g_next, qt_next, cur ^ 1); advance_next(); }

        const int q_tb = qt * BLKQ;
        const ushort_t* q_img = qd_lds[cur][0];
        const ushort_t* do_img = qd_lds[cur][1];
        // skip q tiles fully below this wave's causal diagonal, or
        // (FlashMask) entirely past every bound this wave holds.  Wave-
        // uniform: the transposed reads below need EXEC all ones.
        bool wave_skip =
            causal && (q_tb + BLKQ - 1 + causal_off < kvw);
        if (MASKED && q_tb >= wave_max_end) wave_skip = true;

        // process the 64-q tile as two 32-q sub-iterations: only one
        // (S, dP) register pair is live at a time
        if (!wave_skip) {
#pragma unroll 1
            for (int sub = 0; sub < 2; sub++) {
                f32x16 st, dp;
#pragma unroll
                for (int r = 0; r < 16; r++) { st[r] = 0.f; dp[r] = 0.f; }
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int kk = 0; kk < DSTEPS; kk++) {
                    frag8 aqf = img_row_frag(q_img, sub * 32 + l32, kk, hi);
                    frag8 adf = img_row_frag(do_img, sub * 32 + l32, kk, hi);
                    st = mfma32(aqf, bk[kk], st);
                    dp = mfma32(adf, bv[kk], dp);
                }
                __builtin_amdgcn_s_setprio(0);

                // P = exp(S*scale - lse[q]) overwrites S; dS = P*(dP -
                // delta[q])*scale overwrites dP, rounded as before.  Rows are
                // q, and registers 4g .. 4g+3 hold rows 8g + 4*hi .. +3
                // (crow32): one 16-byte LDS read each of lse and delta per g.
                // When every (q, kv) pair of this 32 x 32 sub-block is visible
                // there is no compare and no select.  On the other path a
                // masked pair is selected to an exact 0 after the arithmetic,
                // whatever its row's lse (-inf for a row without keys, whose
                // pairs are all masked) made of the exponent: every value
                // that survives the select was computed from finite numbers.
                const int q_sub = q_tb + sub * 32;
                const bool full_sub =
                    (q_sub + 32 <= Sq) && (kvw + 32 <= Skv) &&
                    (!causal || (kvw + 31 <= q_sub + causal_off)) &&
                    (!MASKED || (q_sub + 31 < wave_min_end));
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const int row0 = sub * 32 + 8 * g + 4 * hi;
                    const f32x4 ls4 = *reinterpret_cast<const f32x4*>(&ld_lds[cur][0][row0]);
                    const f32x4 dl4 = *reinterpret_cast<const f32x4*>(&ld_lds[cur][1][row0]);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int r = 4 * g + j;
                        float p = sm_opaque(__expf(__builtin_fmaf(st[r], scale, -ls4[j])));
                        st[r] = p;
                        dp[r] = sm_opaque(p * (dp[r] - dl4[j]) * scale);  // dS
                    }
                }
                if (!full_sub) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        int qgl = q_sub + crow32(r, hi);
                        bool vis = (qgl < Sq) && (kvg_lane < Skv) &&
                                   (!causal || kvg_lane <= qgl + causal_off);
                        if (MASKED) vis = vis && (qgl < kv_end_lane);
                        st[r] = vis ? st[r] : 0.f;
                        dp[r] = vis ? dp[r] : 0.f;
                    }
                }

                // dV += P^T·dO, dK += dS^T·Q (contract q: the 2
                // k-steps of this sub-tile)
                // All four A fragments are packed before the first MFMA, so
                // the 32 f32 registers of P and dS are dead (16 packed ones
                // live) while the transposed operands are read: this kernel
                // sits at the register cap.
                frag8 apt[2], ads[2];
#pragma unroll
                for (int ksl = 0; ksl < 2; ksl++) {
                    apt[ksl] = t12_convert(st, ksl * 8);
                    ads[ksl] = t12_convert(dp, ksl * 8);
                }
                asm volatile("" : "+v"(apt[0]), "+v"(apt[1]), "+v"(ads[0]), "+v"(ads[1]));
                // the lane id of the transposed reads, re-derived here so that
                // it is not live across the S and dP chains
                const int lane_t = fresh_lane_id();
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int ksl = 0; ksl < 2; ksl++) {
                    const int ks = sub * 2 + ksl;
#pragma unroll
                    for (int n = 0; n < NDT; n++) {
                        frag8 bdo = img_tr_frag(do_img, ks, n, lane_t);
                        frag8 bq = img_tr_frag(q_img, ks, n, lane_t);
                        acc_dv[n] = mfma32(apt[ksl], bdo, acc_dv[n]);
                        acc_dk[n] = mfma32(ads[ksl], bq, acc_dk[n]);
                    }
                }
                __builtin_amdgcn_s_setprio(0);
            }
        }
        if (++qt == qt_end) qt = qt0;
    }

    // epilogue: acc C-layout [kv][d] (col = d, row = kv within the wave)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        int kvr = kvw + crow32(r, hi);
        if (kvr >= Skv) continue;
        long long base = ((long long)b * Skv + kvr) * rs.dkv + (long long)hk * D;
#pragma unroll
        for (int n = 0; n < NDT; n++) {
            dk[base + n * 32 + l32] = f32_to_bf16(acc_dk[n][r]);
            dv[base + n * 32 + l32] = f32_to_bf16(acc_dv[n][r]);
        }
    }
}

// dual-use image probe: one wave fills a 64 x 128 image by LDS-DMA with the
// source swizzle and returns it as read by the row path and by the
// transposed path (both must reproduce X exactly).
__global__ __launch_bounds__(64) void lds_image_probe(
    const ushort_t* __restrict__ X, ushort_t* __restrict__ out_row,
    ushort_t* __restrict__ out_tr) {
    __shared__ __attribute__((aligned(16))) ushort_t img[64 * 128];
    const int lane = threadIdx.x;
    const int l32 = lane & 31, hi = lane >> 5;
#pragma unroll 1
    for (int piece = 0; piece < 16; piece++)
        lds_dma16(X + img_fill_row(piece, lane) * 128 + img_fill_chunk(piece, lane) * 8,
                  &img[piece * 512]);
    lds_dma_wait_all();
    __syncthreads();
    for (int sub = 0; sub < 2; sub++)
        for (int kk = 0; kk < 8; kk++) {
            frag8 f = img_row_frag(img, sub * 32 + l32, kk, hi);
            *reinterpret_cast<frag8*>(
                out_row + (sub * 32 + l32) * 128 + kk * 16 + hi * 8) = f;
        }
    for (int ks = 0; ks < 4; ks++)
        for (int n = 0; n < 4; n++) {
            frag8 f = img_tr_frag(img, ks, n, lane);
#pragma unroll
            for (int j = 0; j < 8; j++)
                out_tr[(ks * 16 + hi * 8 + j) * 128 + n * 32 + l32] = (ushort_t)f[j];
        }
}

void launch_lds_image_probe(const void* X, void* out_row, void* out_tr,
                            hipStream_t stream) {
    hipLaunchKernelGGL(lds_image_probe, dim3(1), dim3(64), 0, stream,
                       (const ushort_t*)X, (ushort_t*)out_row, (ushort_t*)out_tr);
}

// ---------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------
bool launch_flash_bwd2(const void* dout, const void* q, const void* k, const void* v,
                       const void* o, const float* lse, float* delta,
                       void* dq, void* dk, void* dv,
                       int B, int Sq, int Skv, int Hq, int Hk, int D,
                       float scale, bool causal, hipStream_t stream, int parts,
                       const FlashStrides* strides) {
    if (D != 128 || (Hq % Hk) != 0) return false;
    const FlashStrides rs = strides ? *strides : flash_contiguous_strides(Hq, Hk, D);
    // dq stages K and V, dkv stages Q and dO (contiguous) by LDS-DMA, which
    // needs 16-byte aligned sources
    if (!flash_dma_aligned(q, rs.q) || !flash_dma_aligned(k, rs.kv) ||
        !flash_dma_aligned(v, rs.kv) || !flash_dma_aligned(dout, Hq * D))
        return false;
    if (parts & FLASH_BWD_DELTA)
        launch_flash_bwd_delta(dout, o, delta, B, Sq, Hq, D, stream);
    if (parts & FLASH_BWD_DQ) {
        dim3 gq((Sq + 255) / 256, B * Hq);
        hipLaunchKernelGGL((flash_bwd2_dq_kernel<128, false>), gq, dim3(FB2_BLOCK), 0, stream,
                           (const ushort_t*)q, (const ushort_t*)k, (const ushort_t*)v,
                           (const ushort_t*)dout, lse, delta, (ushort_t*)dq,
                           (const int*)nullptr, rs,
                           B, Sq, Skv, Hq, Hk, scale, causal ? 1 : 0);
    }
    if (parts & FLASH_BWD_DKV) {
        dim3 gkv((Skv + 255) / 256, B * Hk);
        hipLaunchKernelGGL((flash_bwd2_dkv_kernel<128, false>), gkv, dim3(FB2_BLOCK), 0, stream,
                           (const ushort_t*)q, (const ushort_t*)k, (const ushort_t*)v,
                           (const ushort_t*)dout, lse, delta, (ushort_t*)dk, (ushort_t*)dv,
                           (const int*)nullptr, rs,
                           B, Sq, Skv, Hq, Hk, scale, causal ? 1 : 0);
    }
    return true;
}

bool launch_flash_bwd2_mask(const void* dout, const void* q, const void* k,
                            const void* v, const void* o, const float* lse,
                            float* delta, void* dq, void* dk, void* dv,
                            const int* startend,
                            int B, int Sq, int Skv, int Hq, int Hk, int D,
                            float scale, hipStream_t stream,
                            const FlashStrides* strides) {
    if (D != 128 || (Hq % Hk) != 0) return false;
    const FlashStrides rs = strides ? *strides : flash_contiguous_strides(Hq, Hk, D);
    if (!flash_dma_aligned(q, rs.q) || !flash_dma_aligned(k, rs.kv) ||
        !flash_dma_aligned(v, rs.kv) || !flash_dma_aligned(dout, Hq * D))
        return false;
    launch_flash_bwd_delta(dout, o, delta, B, Sq, Hq, D, stream);
    dim3 gq((Sq + 255) / 256, B * Hq);
    hipLaunchKernelGGL((flash_bwd2_dq_kernel<128, true>), gq, dim3(FB2_BLOCK), 0, stream,
                       (const ushort_t*)q, (const ushort_t*)k, (const ushort_t*)v,
                       (const ushort_t*)dout, lse, delta, (ushort_t*)dq, startend, rs,
                       B, Sq, Skv, Hq, Hk, scale, 1);
    dim3 gkv((Skv + 255) / 256, B * Hk);
    hipLaunchKernelGGL((flash_bwd2_dkv_kernel<128, true>), gkv, dim3(FB2_BLOCK), 0, stream,
                       (const ushort_t*)q, (const ushort_t*)k, (const ushort_t*)v,
                       (const ushort_t*)dout, lse, delta, (ushort_t*)dk, (ushort_t*)dv,
                       startend, rs, B, Sq, Skv, Hq, Hk, scale, 1);
    return true;
}
