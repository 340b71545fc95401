// FlashAttention-2 forward v2 — 8-wave 32x32 MFMA structure for gfx950.
//
// Replaces the v1 4-wave 16x16 kernel (flash_attn.hip) on the causal/dense
// D=128 hot path.  Structure follows the CDNA4 guide's verified attention
// ladder (§B "8-warp 32x32", ~900 TF at the GQA bench shape):
//
//   * mfma_f32_32x32x16_bf16 (8-cycle, 32 KFLOP per issue) instead of
//     16x16x32: 2x the FLOP per instruction slot at equal issue rate.
//   * SWAPPED QK^T: compute S^T = K·Q^T so the MFMA C-layout
//     (col = lane&31 = q, row = kv) puts a full softmax row (all kv for
//     one q) into ONE lane's registers — the row max/sum needs no
//     cross-lane shuffles beyond a single permlane32_swap combining the
//     two lane-halves.  (v1 spent 8 shfl_xor rounds per 4-row group.)
//   * In-register P -> PV A-fragment conversion via packed bf16 +
//     permlane32_swap (guide T12): no p_lds round trip at all.
//   * K and V staged by LDS-DMA into one dual-use LDS image each (mfma.h
//     img_off): S^T reads the K image by rows (ds_read_b128), PV reads the
//     V image transposed (ds_read_b64_tr_b16), so no V^T copy is written and
//     no staging registers are held.  Tile t+1 is in flight into the other
//     buffer while tile t is computed; one barrier per tile.  Measured
//     against register staging with a transposing ds_write_b32 pass:
//     profiles/fa_fwd_dq_lds_dma.md.
//   * Softmax VALU diet (mfma.h, profiles/fa_softmax_diet.md): scale > 0, so
//     the row max is taken over the RAW scores (v_max3_f32 pairs) and scaled
//     once per lane; a masked score (-inf) gives exp(-inf) = 0 without a
//     test; on a fully visible tile nothing is compared or selected per
//     score; no packed f32 VALU.  Every value is rounded as before, so o and
//     lse keep their bits.  (An exp2-domain form with the scale folded into
//     one fma per score is faster still but moves the last place of P, and
//     the 32-layer bf16 model turns that into percents of the logits: not
//     used.)
//   * Defer-max rescale (guide T13, THR=8): O-rescale only runs when the
//     running max actually grew, saving the per-tile O sweep.
//   * s_setprio(1) around the MFMA clusters (guide T5).
//
// Reference behavior: paddle `flash_attention` fused op;
// numerics oracle: tests/test_ops_gpu.py vs fp32 torch attention.
#include "launchers.h"
#include "mfma.h"

#define FA2_WAVES 8
#define FA2_BLOCK (FA2_WAVES * 64)
#define FA2_BLKN 64
#define FA2_QW 32            // q rows per wave
#define FA2_BLKM (FA2_WAVES * FA2_QW)
#define DEFER_THR 8.0f

// ---------------------------------------------------------------------------
// layout probe for mfma_f32_32x32x16_bf16: one wave computes C = A(32x16) @
// B(16x32); asymmetric-input GPU test validates the A/B/C lane mappings.
//   A: lane l holds A[l&31][(l>>5)*8 + j]
//   B: lane l holds B[(l>>5)*8 + j][l&31]
// ---------------------------------------------------------------------------
__global__ void mfma32_layout_probe(const ushort_t* A, const ushort_t* B, float* C) {
    int l = threadIdx.x;
    int l32 = l & 31, hi = l >> 5;
    frag8 a, b;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        a[j] = (short)A[l32 * 16 + hi * 8 + j];
        b[j] = (short)B[(hi * 8 + j) * 32 + l32];
    }
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; r++) c[r] = 0.f;
    c = mfma32(a, b, c);
#pragma unroll
    for (int r = 0; r < 16; r++) C[crow32(r, hi) * 32 + l32] = c[r];
}

// permlane32_swap semantics probe: out0/out1 = the two results of
// swap(x, y) where x = lane, y = 1000+lane.
__global__ void permlane_probe(int* out0, int* out1) {
    int l = threadIdx.x;
    auto r = __builtin_amdgcn_permlane32_swap((unsigned)l, (unsigned)(1000 + l),
                                              false, false);
    out0[l] = (int)r[0];
    out1[l] = (int)r[1];
}

// ---------------------------------------------------------------------------
// forward v2
// ---------------------------------------------------------------------------
template <int D, bool MASKED = false>
__global__ __launch_bounds__(FA2_BLOCK) void flash_fwd2_kernel(
    const ushort_t* __restrict__ q,   // [B, Sq, Hq, D]
    const ushort_t* __restrict__ k,   // [B, Skv, Hk, D]
    const ushort_t* __restrict__ v,   // [B, Skv, Hk, D]
    ushort_t* __restrict__ o,         // [B, Sq, Hq, D]
    float* __restrict__ lse,          // [B, Hq, Sq]
    const int* __restrict__ startend, // FlashMask [B, Skv] (MASKED only)
    FlashStrides rs,                  // row strides of q and k/v (elements)
    int B, int Sq, int Skv, int Hq, int Hk, float scale, int causal) {
    static_assert(D == 128, "the dual-use image is laid out for 128-column tiles");
    constexpr int DSTEPS = D / 16;    // K-steps of the S^T MFMAs
    constexpr int NDT = D / 32;       // 32-col d-tiles of O
    constexpr int KVT = FA2_BLKN / 32;  // kv sub-tiles (2)

    // [buffer][0 = K, 1 = V] dual-use images (mfma.h img_off), filled by
    // LDS-DMA: tile t+1 lands in buf[(t+1)&1] while tile t is computed from
    // buf[t&1], with ONE barrier per KV tile (the barrier drain before
    // s_barrier is the dominant structural stall, guide §5)
    __shared__ __attribute__((aligned(16))) ushort_t kv_lds[2][2][FA2_BLKN * D];
    // per-tile FlashMask column bounds, filled by 4-byte LDS-DMA two tiles
    // ahead (three slots): when tile t is computed the bounds of tile t+1
    // have landed too, so every wave reduces them out of LDS (6 shfl_xor)
    // for the whole-tile skip and the whole-block staging skip, and the
    // tile loop holds no ordinary global load at all
    __shared__ int se_lds[3][MASKED ? FA2_BLKN : 1];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int l32 = lane & 31;
    const int hi = lane >> 5;

    // XCD-aware remap: the dispatcher round-robins flat workgroup ids
    // over the 8 XCDs, so with the natural (qt fastest) order every XCD
    // streams every head's KV and no L2 ever re-hits it.  Remap so one
    // (b,h)'s q-tiles run on ONE XCD: its workgroups then consume each
    // KV tile out of that XCD's L2.  Within the XCD the heaviest (last)
    // q tiles of a small group of heads go first, so the causal tail ends
    // on light blocks (mfma.h xcd_grouped_tile).
    int qt, bh;
    xcd_grouped_tile<FA_ORDER_W, false>(qt, bh);
    const int b = bh / Hq, hq = bh % Hq;
    const int hk = hq / (Hq / Hk);
    const int q_base = qt * FA2_BLKM;
    const int qw = q_base + wave * FA2_QW;   // this wave's first q row
    const int qg = qw + l32;                 // this lane's q row (softmax owner)
    const int causal_off = Skv - Sq;

    // q, k, v point at head 0 of token 0 and may be slices of one packed
    // [B, S, (Hq + 2*Hk)*D] tensor: a token row is rs.* elements apart and
    // a batch entry S rows.  o is contiguous.
    const long long q_row_stride = rs.q;
    const long long kv_row_stride = rs.kv;
    const long long o_row_stride = (long long)Hq * D;
    const ushort_t* q_ptr = q + (long long)b * Sq * q_row_stride + (long long)hq * D;
    const ushort_t* k_ptr = k + (long long)b * Skv * kv_row_stride + (long long)hk * D;
    const ushort_t* v_ptr = v + (long long)b * Skv * kv_row_stride + (long long)hk * D;

    // Q B-fragments in registers: lane l holds Q[qw + l32][kk*16 + hi*8 + j]
    frag8 aq[DSTEPS];
    if (qg < Sq) {
#pragma unroll
        for (int kk = 0; kk < DSTEPS; kk++)
            aq[kk] = *reinterpret_cast<const frag8*>(
                q_ptr + (long long)qg * q_row_stride + kk * 16 + hi * 8);
    } else {
#pragma unroll
        for (int kk = 0; kk < DSTEPS; kk++) aq[kk] = frag8{0};
    }

    float m_run = -INFINITY, l_run = 0.f;
    f32x16 acc_o[NDT];
#pragma unroll
    for (int n = 0; n < NDT; n++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc_o[n][r] = 0.f;

    int n_kv_tiles = (Skv + FA2_BLKN - 1) / FA2_BLKN;
    if (causal) {
        int max_kv = q_base + FA2_BLKM - 1 + causal_off;
        int lim = (max_kv + FA2_BLKN) / FA2_BLKN;
        n_kv_tiles = min(n_kv_tiles, max(lim, 0));
    }

    // DMA of the kv tile at kv_base into buffer buf: each wave fills image
    // rows 8*wave .. +7 of K and of V (2 x 1 KiB each).  A ragged tile
    // cannot be zero-filled by DMA: rows past Skv re-read row Skv-1 (finite
    // data); S is set to -inf for kvg >= Skv, so P = 0 there and the clamped
    // V rows are multiplied by exact zeros.  The source must be 16-byte
    // aligned: the launcher checks the k/v bases and the row stride, a head
    // starts at a multiple of 256 bytes.
    auto issue_tile = [&](int kv_base, int buf) {
        // per-lane source offsets are recomputed every tile from a lane id
        // the compiler cannot hoist: kept live across the loop they spill,
        // and a scratch reload after the DMA issue would drain the prefetch
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
    // past Skv repeat the last one, which changes neither min nor max, and
    // their kvg >= Skv test hides them)
    auto issue_bounds = [&](int tile, int slot) {
        if (MASKED && wave == 0) {
            const int ln = fresh_lane_id();
            lds_dma4(startend + (long long)b * Skv + min(tile * FA2_BLKN + ln, Skv - 1),
                     &se_lds[slot][0]);
        }
    };
    // every wave reduces a landed tile's 64 bounds itself: returns (min,
    // max) uniform across the wave
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

    // retire the Q fragment loads here: left pending, the compiler waits for
    // them with a counted vmcnt inside the tile loop, and that count would
    // also drain the (uncounted) DMA in flight
#pragma unroll
    for (int kk = 0; kk < DSTEPS; kk++) asm volatile("" :: "v"(aq[kk]));
    if (n_kv_tiles > 0) {
        issue_tile(0, 0);
        issue_bounds(0, 0);
        if (n_kv_tiles > 1) issue_bounds(1, 1);
    }
    int se_min_cur = 0, se_max_cur = 0x7fffffff;
    int se_slot = 0;   // kvt % 3

    for (int kvt = 0; kvt < n_kv_tiles; kvt++) {
        const int kv_base = kvt * FA2_BLKN;
        const int cur = kvt & 1;
        // tile kvt (and the bounds of kvt+1) have landed (the compiler does
        // not count the DMA, hence the explicit wait) and every wave is done
        // reading the other buffer, which tile kvt+1 now overwrites while
        // tile kvt is computed
        lds_dma_wait_all();
        __syncthreads();
        const int se_slot_next = (se_slot == 2) ? 0 : se_slot + 1;
        if (MASKED && kvt == 0) se_max_cur = tile_bounds(0, se_min_cur);
        // FlashMask: when the whole BLOCK's first q row clears the next
        // tile's max bound, nothing will read it: skip the 32 KB K/V stage
        int se_min_next = 0, se_max_next = 0x7fffffff;
        if (kvt + 1 < n_kv_tiles) {
            bool stage_skip = false;
            if (MASKED) {
                se_max_next = tile_bounds(se_slot_next, se_min_next);
                stage_skip = (q_base >= se_max_next);
            }
            if (!stage_skip) issue_tile(kv_base + FA2_BLKN, cur ^ 1);
            // slot (kvt+2) % 3 was last read as tile kvt-1
            if (kvt + 2 < n_kv_tiles)
                issue_bounds(kvt + 2, (se_slot_next == 2) ? 0 : se_slot_next + 1);
        }
        const ushort_t* k_img = kv_lds[cur][0];
        const ushort_t* v_img = kv_lds[cur][1];
        const int lane_t = fresh_lane_id();   // for the transposed reads

        // a wave whose q rows all precede this kv tile contributes nothing:
        // skip its compute but keep it in the staging and the barriers.
        // Wave-uniform: the transposed reads below need EXEC all ones.
        bool wave_skip =
            causal && (kv_base > qw + FA2_QW - 1 + causal_off);
        // FlashMask whole-tile skip: every kv bound in this tile is at or
        // below the wave's first q row -> no visible pair
        if (MASKED && qw >= se_max_cur) wave_skip = true;

        f32x16 st[KVT];
        if (!wave_skip) {
#pragma unroll
            for (int nt = 0; nt < KVT; nt++)
#pragma unroll
                for (int r = 0; r < 16; r++) st[nt][r] = 0.f;
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < DSTEPS; kk++) {
#pragma unroll
                for (int nt = 0; nt < KVT; nt++) {
                    frag8 ak = img_row_frag(k_img, nt * 32 + l32, kk, hi);
                    st[nt] = mfma32(ak, aq[kk], st[nt]);
                }
            }
            __builtin_amdgcn_s_setprio(0);

            // the MFMA results may now be read by sm_max3 (mfma.h); the fence
            // names every S tile, so a third one must be added here too
            static_assert(KVT == 2, "sm_fence below covers exactly two S tiles");
            sm_fence(st[0], st[1]);

            // mask, on RAW scores.  A tile is "full" when every (q, kv) pair
            // in this wave's sub-block is visible, the common case away from
            // the diagonal: no compare and no select at all.
            const bool full_tile =
                (kv_base + FA2_BLKN <= Skv) &&
                (!causal || (kv_base + FA2_BLKN - 1 <= qw + causal_off)) &&
                (!MASKED || (qw + FA2_QW - 1 < se_min_cur));
            if (!full_tile) {
#pragma unroll
                for (int nt = 0; nt < KVT; nt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        int row = nt * 32 + crow32(r, hi);
                        int kvg = kv_base + row;
                        bool vis = (kvg < Skv) &&
                                   (!causal || kvg <= qg + causal_off);
                        if (MASKED) vis = vis && (qg < se_lds[se_slot][row]);
                        st[nt][r] = vis ? st[nt][r] : -INFINITY;
                    }
            }

            // per-lane row max over the 32 kv values (v_max3 pairs) + one
            // half-swap combine.  scale > 0 and rounding is monotone, so the
            // max of the scaled scores is the scaled max of the raw ones: one
            // multiply per lane, not one per score, and the same bits.
            float pm = -INFINITY;
#pragma unroll
            for (int nt = 0; nt < KVT; nt++) pm = sm_tile_max(pm, st[nt]);
            pm *= scale;
            {
                union { float f; unsigned u; } x{pm};
                auto rr = __builtin_amdgcn_permlane32_swap(x.u, x.u, false, false);
                union { unsigned u; float f; } a{rr[0]}, c{rr[1]};
                pm = fmaxf(a.f, c.f);
            }

            // defer-max (T13): only rescale O when the max actually grew.
            // The decision comes before this tile's P is formed and after the
            // previous tile's P.V is complete, and alpha scales l_run and O
            // together.
            bool grew = pm > m_run + DEFER_THR ||
                        (m_run == -INFINITY && pm > -INFINITY);
            if (__any(grew)) {
                float m_new = fmaxf(m_run, pm);
                float alpha = (m_run == -INFINITY)
                                  ? 0.f
                                  : __expf(m_run - m_new);
                if (m_new == -INFINITY) alpha = 1.f;
                l_run *= alpha;
                m_run = m_new;
                // O rows are C-layout rows (q = crow32): fetch each row's
                // alpha from the lane that owns that q
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    float ar = __shfl(alpha, crow32(r, hi), 64);
#pragma unroll
                    for (int n = 0; n < NDT; n++) acc_o[n][r] *= ar;
                }
            }

            // P = exp(S*scale - m), rounded exactly as before (the product,
            // the difference and the exponent's log2(e) multiply each round
            // once: sm_opaque keeps the product out of an fma), so o and lse
            // keep their bits.  A masked score is -inf and gives exp(-inf) =
            // 0 by itself, with no test per score.  A row that has seen no
            // key yet (all its scores so far are -inf, the wave is not
            // skipped because of its other rows) takes an effective max of
            // 0, once per tile per lane: -inf - -inf would be NaN.
            const float m_eff = (m_run == -INFINITY) ? 0.f : m_run;
            float ps = 0.f;
#pragma unroll
            for (int nt = 0; nt < KVT; nt++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    float p = sm_opaque(__expf(sm_opaque(st[nt][r] * scale) - m_eff));
                    st[nt][r] = p;
                    ps += p;
                }
            {
                union { float f; unsigned u; } x{ps};
                auto rr = __builtin_amdgcn_permlane32_swap(x.u, x.u, false, false);
                union { unsigned u; float f; } a{rr[0]}, c{rr[1]};
                ps = a.f + c.f;
            }
            l_run += ps;

            // P (C-layout, rows = kv) -> PV A-fragments, fully in-register
            // (T12, mfma.h).  For k-step ks the lane needs P[q = l32][kv =
            // ks*16 + hi*8 + j]: the 8-register slice (ks&1)*8 of sub-tile
            // ks>>1.
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ks = 0; ks < FA2_BLKN / 16; ks++) {
                frag8 pa = t12_convert(st[ks >> 1], (ks & 1) * 8);
#pragma unroll
                for (int n = 0; n < NDT; n++) {
                    frag8 bv = img_tr_frag(v_img, ks, n, lane_t);
                    acc_o[n] = mfma32(pa, bv, acc_o[n]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        }

        if (MASKED) { se_max_cur = se_max_next; se_min_cur = se_min_next; }
        se_slot = se_slot_next;
    }

    // epilogue: O / l, LSE.  inv_l lives in the lane that owns q; O rows
    // fetch it by shfl like the rescale.
    float inv_l = (l_run > 0.f) ? 1.0f / l_run : 0.f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        int qrow = qw + crow32(r, hi);
        if (qrow >= Sq) continue;
        float il = __shfl(inv_l, crow32(r, hi), 64);
        ushort_t* orow = o + ((long long)b * Sq + qrow) * o_row_stride + (long long)hq * D;
#pragma unroll
        for (int n = 0; n < NDT; n++)
            orow[n * 32 + l32] = f32_to_bf16(acc_o[n][r] * il);
    }
    if (hi == 0 && qg < Sq) {
        float lv = (l_run > 0.f) ? (m_run + __logf(l_run)) : -INFINITY;
        lse[((long long)b * Hq + hq) * Sq + qg] = lv;
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void launch_mfma32_probe(const void* A, const void* B, float* C, hipStream_t stream) {
    hipLaunchKernelGGL(mfma32_layout_probe, dim3(1), dim3(64), 0, stream,
                       (const ushort_t*)A, (const ushort_t*)B, C);
}

void launch_permlane_probe(int* out0, int* out1, hipStream_t stream) {
    hipLaunchKernelGGL(permlane_probe, dim3(1), dim3(64), 0, stream, out0, out1);
}

bool launch_flash_fwd2(const void* q, const void* k, const void* v, void* o,
                       float* lse, int B, int Sq, int Skv, int Hq, int Hk,
                       int D, float scale, bool causal, hipStream_t stream,
                       const FlashStrides* strides) {
    if (D != 128 || (Hq % Hk) != 0) return false;
    const FlashStrides rs = strides ? *strides : flash_contiguous_strides(Hq, Hk, D);
    // K and V tiles are staged by LDS-DMA, which needs 16-byte aligned sources
    if (!flash_dma_aligned(k, rs.kv) || !flash_dma_aligned(v, rs.kv)) return false;
    dim3 grid((Sq + FA2_BLKM - 1) / FA2_BLKM, B * Hq);
    hipLaunchKernelGGL((flash_fwd2_kernel<128, false>), grid, dim3(FA2_BLOCK), 0, stream,
                       (const ushort_t*)q, (const ushort_t*)k, (const ushort_t*)v,
                       (ushort_t*)o, lse, (const int*)nullptr, rs,
                       B, Sq, Skv, Hq, Hk, scale, causal ? 1 : 0);
    return true;
}

bool launch_flash_fwd2_mask(const void* q, const void* k, const void* v,
                            void* o, float* lse, const int* startend,
                            int B, int Sq, int Skv, int Hq, int Hk,
                            int D, float scale, hipStream_t stream,
                            const FlashStrides* strides) {
    if (D != 128 || (Hq % Hk) != 0) return false;
    const FlashStrides rs = strides ? *strides : flash_contiguous_strides(Hq, Hk, D);
    if (!flash_dma_aligned(k, rs.kv) || !flash_dma_aligned(v, rs.kv)) return false;
    dim3 grid((Sq + FA2_BLKM - 1) / FA2_BLKM, B * Hq);
    hipLaunchKernelGGL((flash_fwd2_kernel<128, true>), grid, dim3(FA2_BLOCK), 0,
                       stream, (const ushort_t*)q, (const ushort_t*)k,
                       (const ushort_t*)v, (ushort_t*)o, lse, startend, rs,
                       B, Sq, Skv, Hq, Hk, scale, 1);
    return true;
}
