// Paged-KV append attention: T new tokens per sequence attend to the cache
// that already holds them (append first, then attend) under a causal mask —
// gfx950.  This is the middle case between flash prefill (empty cache) and
// paged decode (one token): chunked prefill, multi-turn continuation and
// speculative verification all run through it.
//
// The kernel is the MFMA decode kernel (paged_attn_v2.hip) with the 16-column
// N dimension of mfma_f32_16x16x32_bf16 carrying (token, head) query rows
// instead of the GQA group's heads alone:
//
//   * query row n = t*G + g (token-major), so the 16 rows of a tile sit on
//     consecutive positions and the tile's kv range is tight; G need not
//     divide 16, t and g are derived per lane;
//   * one workgroup = 4 waves per (batch, kv-head, row group, kv split); a
//     row group is R 16-row tiles.  The K A-fragments and the staged V^T tile
//     are loaded once and reused for the R tiles, which is what makes a chunk
//     of hundreds of tokens cheaper than R times the decode traffic;
//   * a workgroup's kv range ends at the position of its last valid row; it
//     loads no K, V or block-table entry past that;
//   * in the S^T C-layout a lane's column is one query row, so the causal
//     limit is one per-lane scalar per tile.  A wave's 32-token quarter that
//     lies below the smallest limit of the workgroup takes the unmasked path
//     (the decode kernel's `full` flag); a quarter at or above a tile's
//     largest limit skips that tile altogether;
//   * rows at or past token_counts[b] have limit 0: they stay at m = -inf,
//     l = 0 and are never written (the caller zero-fills the output);
//   * the 4 waves merge through LDS one tile at a time, writing the output
//     or fp32 partials [B, Hk, row group, split, 16R rows, 2 + D] that
//     paged_append_merge_kernel folds.
//
// Reference behavior: csrc/gpu/append_attn, multi-token path.
#include "launchers.h"
#include "paged_kv.h"

// end (exclusive) of the kv range of the row group starting at row n0
__device__ __forceinline__ int append_kv_end(int before, int n0, int rows,
                                             int n_valid, int G) {
    return before + (min(n0 + rows, n_valid) - 1) / G + 1;
}

// Two workgroups per CU: R = 2 lands at ~300 registers without the bound (one
// workgroup per CU); asking for three spills the R = 1 int8 variant.
template <int D, int MODE, int R>
__global__ __launch_bounds__(PD3_BLOCK, 2) void paged_append_attn_kernel(
    const ushort_t* __restrict__ q,            // [B, T, Hq, D]
    const void* __restrict__ k_cache,
    const void* __restrict__ v_cache,
    const float* __restrict__ k_scale,
    const float* __restrict__ v_scale,
    const int* __restrict__ block_table,
    const int* __restrict__ seq_lens_before,
    const int* __restrict__ token_counts,      // [B] or null (= T)
    ushort_t* __restrict__ out,                // [B, T, Hq, D], zero-filled
    float* __restrict__ partials,
    int B, int T, int Hq, int Hk, int block_size, int max_blocks, float scale,
    int nsplit, int nrg) {
    constexpr int KD = D / 32;
    constexpr int ND = D / 16;
    constexpr int ROWS = 16 * R;
    // vt (32 KB) + per-wave P staging (4 x R x 1 KB); the one-tile merge
    // scratch aliases them
    constexpr int VT_ELEMS = D * PD3_TILE;
    constexpr int P_ELEMS = PD3_WAVES * R * 16 * 32;
    constexpr int MERGE_FLOATS = PD3_WAVES * 16 * (2 + D);
    constexpr int SMEM = ((VT_ELEMS + P_ELEMS) * 2 > MERGE_FLOATS * 4)
                             ? (VT_ELEMS + P_ELEMS) * 2 : MERGE_FLOATS * 4;
    __shared__ char smem[SMEM];
    ushort_t* vt_lds = reinterpret_cast<ushort_t*>(smem);
    ushort_t* p_lds = vt_lds + VT_ELEMS;   // [wave][R][16 q][32 kv]
    float* mrg = reinterpret_cast<float*>(smem);

    const int G = Hq / Hk;
    const int b = blockIdx.x / nrg;
    // longest kv range first
    const int rg = nrg - 1 - (blockIdx.x - b * nrg);
    const int hk = blockIdx.y;
    const int split = blockIdx.z;
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int l16 = lane & 15;
    const int lg = lane >> 4;
    const int before = seq_lens_before[b];
    const int n_tok = token_counts ? min(max(token_counts[b], 0), T) : T;
    const int n_valid = n_tok * G;     // valid query rows of this (b, hk)
    const int n0 = rg * ROWS;
    if (n0 >= n_valid || before < 0) return;

    const int kv_end = append_kv_end(before, n0, ROWS, n_valid, G);
    const int chunk = (kv_end + nsplit - 1) / nsplit;
    const int c0 = split * chunk;
    const int c1 = min(kv_end, c0 + chunk);
    if (c0 >= c1) return;              // the merge skips empty splits too
    // smallest causal limit among the workgroup's rows (row n0 is valid)
    const int min_lim = min(c1, before + n0 / G + 1);

    const int* bt = block_table + (long long)b * max_blocks;

    // per tile: this lane's query row, its causal limit (exclusive, clamped
    // to the split) and the tile's largest limit
    int lim[R], tile_end[R];
    frag8 qT[R][KD];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int n = n0 + r * 16 + l16;
        const int t = n / G;
        if (n < n_valid) {
            lim[r] = min(before + t + 1, c1);
            const ushort_t* qp =
                q + (((long long)b * T + t) * Hq + hk * G + (n - t * G)) * D;
#pragma unroll
            for (int kk = 0; kk < KD; kk++)
                qT[r][kk] = *reinterpret_cast<const frag8*>(qp + kk * 32 + lg * 8);
        } else {
            lim[r] = 0;
#pragma unroll
            for (int kk = 0; kk < KD; kk++) qT[r][kk] = frag8{0};
        }
        const int nl = min(n0 + r * 16 + 16, n_valid) - 1;   // tile's last valid row
        tile_end[r] = (nl >= n0 + r * 16) ? min(before + nl / G + 1, c1) : 0;
    }

    float m_run[R], l_run[R];
    f32x4 acc_o[R][ND];
#pragma unroll
    for (int r = 0; r < R; r++) {
        m_run[r] = -INFINITY;
        l_run[r] = 0.f;
#pragma unroll
        for (int n = 0; n < ND; n++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc_o[r][n][e] = 0.f;
    }

    // staging: thread owns V token row-pair (tid&63)*2, cols wave*32..+31
    const int s_r0 = (tid & 63) * 2;
    const int s_c = wave * 32;
    short8v vr[2][4];

    auto load_tile = [&](int t0) {
#pragma unroll
        for (int rr = 0; rr < 2; rr++) {
            int tok = t0 + s_r0 + rr;
            if (tok < c1) {
                long long rec = pkv_record(bt, tok, block_size, Hk, hk);
                pkv_load_v_row<D, MODE>(vr[rr], v_cache, v_scale, rec, s_c);
            } else {
#pragma unroll
                for (int cc = 0; cc < 4; cc++)
                    vr[rr][cc] = short8v{0,0,0,0,0,0,0,0};
            }
        }
    };

    load_tile(c0);
    pkv_write_vt(vt_lds, vr, s_c, s_r0);
    __syncthreads();
    for (int t0 = c0; t0 < c1; t0 += PD3_TILE) {
        if (t0 + PD3_TILE < c1) load_tile(t0 + PD3_TILE);

        const int tq0 = t0 + wave * 32;
        if (tq0 < c1) {
            bool act[R];
#pragma unroll
            for (int r = 0; r < R; r++) act[r] = tq0 < tile_end[r];

            // ---- S^T: two 16-token K tiles, each against the R row tiles ----
            f32x4 st[R][2];
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int s = 0; s < 2; s++)
#pragma unroll
                    for (int e = 0; e < 4; e++) st[r][s][e] = 0.f;
#pragma unroll
            for (int s = 0; s < 2; s++) {
                int tok = tq0 + s * 16 + l16;
                int tokc = min(tok, c1 - 1);
                long long rec = pkv_record(bt, tokc, block_size, Hk, hk);
                frag8 ak[KD];
                pkv_load_k_frags<D, MODE>(ak, k_cache, k_scale, rec, lg);
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    if (!act[r]) continue;
#pragma unroll
                    for (int kk = 0; kk < KD; kk++)
                        st[r][s] = mfma16(ak[kk], qT[r][kk], st[r][s]);
                }
                __builtin_amdgcn_s_setprio(0);
            }

            // mask + online softmax (C row = kv = s*16 + lg*4 + e, col = row n)
            const bool full = (tq0 + 32 <= min_lim);
            ushort_t* pw = p_lds + wave * R * 16 * 32;
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (!act[r]) continue;
#pragma unroll
                for (int s = 0; s < 2; s++)
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        int tok = tq0 + s * 16 + lg * 4 + e;
                        st[r][s][e] = (full || tok < lim[r]) ? st[r][s][e] * scale
                                                             : -INFINITY;
                    }
                float pm = -INFINITY;
#pragma unroll
                for (int s = 0; s < 2; s++)
#pragma unroll
                    for (int e = 0; e < 4; e++) pm = fmaxf(pm, st[r][s][e]);
                pm = fmaxf(pm, __shfl_xor(pm, 16, 64));
                pm = fmaxf(pm, __shfl_xor(pm, 32, 64));
                bool grew = pm > m_run[r] + 8.0f ||
                            (m_run[r] == -INFINITY && pm > -INFINITY);
                if (__any(grew)) {
                    float m_new = fmaxf(m_run[r], pm);
                    float alpha = (m_run[r] == -INFINITY) ? 0.f
                                                          : __expf(m_run[r] - m_new);
                    if (m_new == -INFINITY) alpha = 1.f;
                    l_run[r] *= alpha;
                    m_run[r] = m_new;
                    // O rows are query rows lg*4 + e: alpha from the owner lane
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        float ar = __shfl(alpha, lg * 4 + e, 64);
#pragma unroll
                        for (int n = 0; n < ND; n++) acc_o[r][n][e] *= ar;
                    }
                }
                float ps = 0.f;
#pragma unroll
                for (int s = 0; s < 2; s++)
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        float sv = st[r][s][e];
                        float p = (sv == -INFINITY) ? 0.f : __expf(sv - m_run[r]);
                        st[r][s][e] = p;
                        ps += p;
                    }
                ps += __shfl_xor(ps, 16, 64);
                ps += __shfl_xor(ps, 32, 64);
                l_run[r] += ps;

                // P -> per-wave LDS ([16 rows][32 kv], u32-packed pairs)
#pragma unroll
                for (int s = 0; s < 2; s++)
#pragma unroll
                    for (int e = 0; e < 4; e += 2)
                        *reinterpret_cast<unsigned*>(
                            swz<32>(pw + r * 16 * 32, l16, s * 16 + lg * 4 + e)) =
                            pack_bf16(st[r][s][e], st[r][s][e + 1]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            frag8 pa[R];
#pragma unroll
            for (int r = 0; r < R; r++)
                pa[r] = *reinterpret_cast<const frag8*>(
                    swz<32>(pw + r * 16 * 32, l16, lg * 8));
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int n = 0; n < ND; n++) {
                frag8 bv = *reinterpret_cast<const frag8*>(
                    swz<PD3_TILE>(vt_lds, n * 16 + l16, wave * 32 + lg * 8));
#pragma unroll
                for (int r = 0; r < R; r++)
                    if (act[r]) acc_o[r][n] = mfma16(pa[r], bv, acc_o[r][n]);
            }
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
        if (t0 + PD3_TILE < c1) {
            pkv_write_vt(vt_lds, vr, s_c, s_r0);
            __syncthreads();
        }
    }

    // ---- merge the 4 waves, one row tile at a time ----
    constexpr int rec = 2 + D;
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r > 0) __syncthreads();
        if (lg == 0) {
            mrg[(wave * 16 + l16) * rec + 0] = m_run[r];
            mrg[(wave * 16 + l16) * rec + 1] = l_run[r];
        }
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int n = 0; n < ND; n++)
                mrg[(wave * 16 + lg * 4 + e) * rec + 2 + n * 16 + l16] = acc_o[r][n][e];
        __syncthreads();
        for (int idx = tid; idx < 16 * D; idx += PD3_BLOCK) {
            const int row = idx / D, d = idx % D;
            const int n = n0 + r * 16 + row;
            if (n >= n_valid) continue;
            float gm = -INFINITY;
#pragma unroll
            for (int w = 0; w < PD3_WAVES; w++)
                gm = fmaxf(gm, mrg[(w * 16 + row) * rec]);
            float gl = 0.f, oa = 0.f;
#pragma unroll
            for (int w = 0; w < PD3_WAVES; w++) {
                float mw = mrg[(w * 16 + row) * rec];
                float a = (mw == -INFINITY) ? 0.f : __expf(mw - gm);
                gl += mrg[(w * 16 + row) * rec + 1] * a;
                oa += mrg[(w * 16 + row) * rec + 2 + d] * a;
            }
            if (nsplit == 1) {
                const int t = n / G;
                float inv = (gl > 0.f) ? 1.0f / gl : 0.f;
                out[(((long long)b * T + t) * Hq + hk * G + (n - t * G)) * D + d] =
                    f32_to_bf16(oa * inv);
            } else {
                float* pp = partials +
                    (((((long long)b * Hk + hk) * nrg + rg) * nsplit + split) * ROWS +
                     r * 16 + row) * rec;
                if (d == 0) { pp[0] = gm; pp[1] = gl; }
                pp[2 + d] = oa;
            }
        }
    }
}

// fold the per-split partials: one wave per query row
template <int D>
__global__ void paged_append_merge_kernel(
    const float* __restrict__ partials, ushort_t* __restrict__ out,
    const int* __restrict__ seq_lens_before, const int* __restrict__ token_counts,
    int B, int T, int Hq, int Hk, int nsplit, int nrg, int rows) {
    const int b = blockIdx.x / nrg;
    const int rg = blockIdx.x - b * nrg;
    const int hk = blockIdx.y;
    const int row = blockIdx.z;
    const int G = Hq / Hk;
    const int lane = threadIdx.x & 63;
    constexpr int EPL = D / 64;
    constexpr int rec = 2 + D;
    const int before = seq_lens_before[b];
    const int n_tok = token_counts ? min(max(token_counts[b], 0), T) : T;
    const int n_valid = n_tok * G;
    const int n0 = rg * rows;
    const int n = n0 + row;
    if (n >= n_valid || before < 0) return;
    const int kv_end = append_kv_end(before, n0, rows, n_valid, G);
    const int chunk = (kv_end + nsplit - 1) / nsplit;
    const float* base = partials +
        (((((long long)b * Hk + hk) * nrg + rg) * nsplit) * rows + row) * rec;
    const long long sstride = (long long)rows * rec;
    float gm = -INFINITY;
    for (int sp = 0; sp < nsplit; sp++) {
        if (sp * chunk >= kv_end) break;
        gm = fmaxf(gm, base[sp * sstride]);
    }
    float gl = 0.f;
    float oacc[EPL] = {0.f};
    for (int sp = 0; sp < nsplit; sp++) {
        if (sp * chunk >= kv_end) break;
        const float* pp = base + sp * sstride;
        float a = (pp[0] == -INFINITY) ? 0.f : __expf(pp[0] - gm);
        gl += pp[1] * a;
#pragma unroll
        for (int e = 0; e < EPL; e++)
            oacc[e] += pp[2 + lane * EPL + e] * a;
    }
    float inv = (gl > 0.f) ? 1.0f / gl : 0.f;
    const int t = n / G;
    ushort_t* op = out + (((long long)b * T + t) * Hq + hk * G + (n - t * G)) * D;
#pragma unroll
    for (int e = 0; e < EPL; e++)
        op[lane * EPL + e] = f32_to_bf16(oacc[e] * inv);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
bool paged_append_plan(int B, int T, int Hq, int Hk, int D, int r_tiles,
                       int* R, int* nrg, int* nsplit) {
    if (D != 128 || Hk <= 0 || (Hq % Hk) != 0 || Hq / Hk > PD3_MAXG || T <= 0)
        return false;
    const int rows = T * (Hq / Hk);
    // One tile when the rows fit it, otherwise two: R = 2 is the fastest or
    // tied at every measured shape, R = 4 (~467 registers, one workgroup per
    // CU) lost everywhere and is not instantiated
    // (profiles/paged_append_attn.md).
    int r = r_tiles;
    if (r != 1 && r != 2) r = rows <= 16 ? 1 : 2;
    *R = r;
    *nrg = (rows + 16 * r - 1) / (16 * r);
    *nsplit = paged_decode_nsplit(B * *nrg, Hk);
    return true;
}

bool launch_paged_append_attn(const void* q, const void* k_cache, const void* v_cache,
                              const float* k_scale, const float* v_scale,
                              const int* block_table, const int* seq_lens_before,
                              const int* token_counts, void* out, float* partials,
                              int r_tiles, int B, int T, int Hq, int Hk, int D,
                              int block_size, int max_blocks, float scale,
                              int cache_mode, hipStream_t stream) {
    int R, nrg, nsplit;
    if (!paged_append_plan(B, T, Hq, Hk, D, r_tiles, &R, &nrg, &nsplit)) return false;
    dim3 grid(B * nrg, Hk, nsplit);
#define PAA_LAUNCH(MM, RR)                                                          \
    hipLaunchKernelGGL((paged_append_attn_kernel<128, MM, RR>), grid,               \
                       dim3(PD3_BLOCK), 0, stream, (const ushort_t*)q, k_cache,     \
                       v_cache, k_scale, v_scale, block_table, seq_lens_before,     \
                       token_counts, (ushort_t*)out, partials, B, T, Hq, Hk,        \
                       block_size, max_blocks, scale, nsplit, nrg)
#define PAA_MODE(RR)                                                                \
    do {                                                                            \
        if (cache_mode == 2) PAA_LAUNCH(2, RR);                                     \
        else if (cache_mode == 1) PAA_LAUNCH(1, RR);                                \
        else PAA_LAUNCH(0, RR);                                                     \
    } while (0)
    if (R == 1) PAA_MODE(1);
    else PAA_MODE(2);
#undef PAA_MODE
#undef PAA_LAUNCH
    if (nsplit > 1) {
        dim3 mgrid(B * nrg, Hk, 16 * R);
        hipLaunchKernelGGL(paged_append_merge_kernel<128>, mgrid, dim3(64), 0, stream,
                           partials, (ushort_t*)out, seq_lens_before, token_counts,
                           B, T, Hq, Hk, nsplit, nrg, 16 * R);
    }
    return true;
}
