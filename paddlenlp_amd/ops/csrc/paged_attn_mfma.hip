// Paged-KV attention on mfma_f32_16x16x32_bf16 — gfx950: single-token decode
// and multi-token append (T new tokens per sequence attend, under a causal
// mask, to the cache that already holds them: chunked prefill, multi-turn
// continuation, speculative verification).  Both are one tile loop,
// paged_mfma_attend, over the kv range of a workgroup; they differ in which
// query rows ride in the 16-column N dimension of the MFMA, and a row map
// (DecodeRows, AppendRows) says so.  Shapes the loop does not take (D != 128
// or a GQA group > 16) run the scalar kernel in paged_attn.hip.
//
// The loop:
//
//   * one workgroup = 4 waves per (batch, kv-head, row group, kv split).  The
//     block cooperatively stages a 128-token V tile into LDS, transposed via
//     u32 row-pair packing and XOR-swizzled, and prefetches the next tile's
//     rows into registers meanwhile; K is read straight from the cache as
//     per-lane A-fragments (the rows stream through L1; no reuse to justify
//     LDS);
//   * each wave runs a 32-token quarter as two 16-token S^T = K·Q^T tiles.
//     In the C-layout a lane's column is one query row, so the online softmax
//     is per-lane plus two shfl_xor combines, and the causal limit is one
//     per-lane scalar per row tile.  P goes through 1 KB of per-wave LDS per
//     row tile and O += P·V accumulates against the staged V^T;
//   * a row group is R 16-row tiles.  The K fragments and the V^T tile are
//     loaded once and reused for the R tiles, which is what makes a chunk of
//     hundreds of tokens cheaper than R times the decode traffic;
//   * a quarter that lies below the smallest limit of the workgroup takes the
//     unmasked path; a quarter at or above a tile's largest limit skips that
//     tile altogether; nothing of K, V or the block table is loaded past the
//     workgroup's kv end;
//   * the 4 waves' (m, l, acc) merge through LDS (aliased over the V staging
//     buffer) one row tile at a time, writing the output or fp32 partials
//     that a split fold (pkv_fold_splits) finishes.
//
// Decode rows: row g is head g of the GQA group (G <= 16 of the 16 columns;
// decode is bandwidth-bound, the idle columns are free), every row sees the
// whole split, R = 1.  Partials are [B, Hk, split, G, 2 + D], the layout the
// scalar kernel writes and paged_decode_merge_kernel reads.
//
// Append rows: row n = t*G + g (token-major), so the 16 rows of a tile sit on
// consecutive positions and the tile's kv range is tight; G need not divide
// 16, t and g are derived per lane.  A workgroup's kv range ends at the
// position of its last valid row.  Rows at or past token_counts[b] have limit
// 0: they stay at m = -inf, l = 0 and are never written (the caller
// zero-fills the output).  Partials are [B, Hk, row group, split, 16R rows,
// 2 + D].
//
// Why 16x16 fragments: 32x32x16 tiles with the P -> PV conversion in
// registers hold ~254 VGPRs -> 2 waves/SIMD; decode is HBM-latency-bound, so
// trading MFMA width for wave count wins.  16x16 fragments cut the
// accumulator to 32 registers per row tile (8 d-tiles x f32x4) and the LDS
// footprint to one 32 KB V^T tile + 4 KB P staging per row tile.  Fragment
// layouts are in mfma.h.
//
// Reference behavior: csrc/gpu/append_attn, decode and
// multi-token paths.
#include "launchers.h"
#include "paged_kv.h"

// A row map supplies, for row tile r of its workgroup:
//   query(r, l16, qp, lim)  whether lane column l16 carries a query row; its
//                           address and causal limit (exclusive, clamped to
//                           the split)
//   tile_end(r), min_lim()  the largest limit of tile r, the smallest limit of
//                           the workgroup
//   merge_rows()            rows per wave in the merge scratch
//   valid(r, row), out_row(r, row), partial_row(r, row)
//                           where merged row `row` of tile r goes

template <int D>
struct DecodeRows {
    const ushort_t* q;     // [B, Hq, D]
    ushort_t* out;         // [B, Hq, D]
    float* partials;
    int b, hk, split, nsplit, Hq, Hk, G, c1;

    __device__ __forceinline__ bool query(int, int l16, const ushort_t*& qp,
                                          int& lim) const {
        lim = c1;
        if (l16 >= G) return false;
        qp = q + ((long long)b * Hq + hk * G + l16) * D;
        return true;
    }
    __device__ __forceinline__ int tile_end(int) const { return c1; }
    __device__ __forceinline__ int min_lim() const { return c1; }
    __device__ __forceinline__ int merge_rows() const { return G; }
    __device__ __forceinline__ bool valid(int, int) const { return true; }
    __device__ __forceinline__ ushort_t* out_row(int, int g) const {
        return out + ((long long)b * Hq + hk * G + g) * D;
    }
    __device__ __forceinline__ float* partial_row(int, int g) const {
        return partials +
            (((long long)b * Hk + hk) * nsplit + split) * (long long)G * (2 + D) +
            (long long)g * (2 + D);
    }
};

// end (exclusive) of the kv range of the row group starting at row n0
__device__ __forceinline__ int append_kv_end(int before, int n0, int rows,
                                             int n_valid, int G) {
    return before + (min(n0 + rows, n_valid) - 1) / G + 1;
}

template <int D, int R>
struct AppendRows {
    const ushort_t* q;     // [B, T, Hq, D]
    ushort_t* out;         // [B, T, Hq, D]
    float* partials;
    int b, hk, rg, split, nsplit, nrg, T, Hq, Hk, G;
    int before, n0, n_valid, c1;

    __device__ __forceinline__ long long row_offset(int n) const {
        const int t = n / G;
        return (((long long)b * T + t) * Hq + hk * G + (n - t * G)) * D;
    }
    __device__ __forceinline__ bool query(int r, int l16, const ushort_t*& qp,
                                          int& lim) const {
        const int n = n0 + r * 16 + l16;
        lim = 0;
        if (n >= n_valid) return false;
        lim = min(before + n / G + 1, c1);
        qp = q + row_offset(n);
        return true;
    }
    __device__ __forceinline__ int tile_end(int r) const {
        const int nl = min(n0 + r * 16 + 16, n_valid) - 1;   // tile's last valid row
        return (nl >= n0 + r * 16) ? min(before + nl / G + 1, c1) : 0;
    }
    // row n0 is valid
    __device__ __forceinline__ int min_lim() const {
        return min(c1, before + n0 / G + 1);
    }
    __device__ __forceinline__ int merge_rows() const { return 16; }
    __device__ __forceinline__ bool valid(int r, int row) const {
        return n0 + r * 16 + row < n_valid;
    }
    __device__ __forceinline__ ushort_t* out_row(int r, int row) const {
        return out + row_offset(n0 + r * 16 + row);
    }
    __device__ __forceinline__ float* partial_row(int r, int row) const {
        return partials +
            (((((long long)b * Hk + hk) * nrg + rg) * nsplit + split) * (16 * R) +
             r * 16 + row) * (2 + D);
    }
};

// Attention of the workgroup's R row tiles over kv positions c0..c1 of the
// sequence whose block-table row is bt.  MODE: 0 = bf16 cache, 1 = int8,
// 2 = int4 packed nibbles (q+8 offset).  An empty range still merges (m =
// -inf, l = 0).
template <int D, int MODE, int R, class Rows>
__device__ __forceinline__ void paged_mfma_attend(
    const Rows& rows, const void* __restrict__ k_cache,
    const void* __restrict__ v_cache, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, const int* __restrict__ bt,
    int Hk, int hk, int block_size, float scale, int c0, int c1, int nsplit) {
    constexpr int KD = D / 32;     // S^T k-steps (4 at D=128)
    constexpr int ND = D / 16;     // O d-tiles (8)
    // vt (32 KB) + per-wave P staging (4 x R x 1 KB); the one-tile merge
    // scratch aliases them
    constexpr int VT_ELEMS = D * PD3_TILE;
    constexpr int P_ELEMS = PD3_WAVES * R * 16 * 32;
    constexpr int MERGE_FLOATS = PD3_WAVES * PD3_MAXG * (2 + D);
    constexpr int SMEM = ((VT_ELEMS + P_ELEMS) * 2 > MERGE_FLOATS * 4)
                             ? (VT_ELEMS + P_ELEMS) * 2 : MERGE_FLOATS * 4;
    __shared__ char smem[SMEM];
    ushort_t* vt_lds = reinterpret_cast<ushort_t*>(smem);
    ushort_t* p_lds = vt_lds + VT_ELEMS;   // [wave][R][16 rows][32 kv]
    float* mrg = reinterpret_cast<float*>(smem);

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int l16 = lane & 15;
    const int lg = lane >> 4;          // lane group 0..3

    // Q^T B-fragments: lane holds Q[row l16 of tile r][kk*32 + lg*8 + j]
    int lim[R], tile_end[R];
    frag8 qT[R][KD];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const ushort_t* qp;
        if (rows.query(r, l16, qp, lim[r])) {
#pragma unroll
            for (int kk = 0; kk < KD; kk++)
                qT[r][kk] = *reinterpret_cast<const frag8*>(qp + kk * 32 + lg * 8);
        } else {
#pragma unroll
            for (int kk = 0; kk < KD; kk++) qT[r][kk] = frag8{0};
        }
        tile_end[r] = rows.tile_end(r);
    }
    const int min_lim = rows.min_lim();

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

    if (c0 < c1) {
        load_tile(c0);
        pkv_write_vt(vt_lds, vr, s_c, s_r0);
        __syncthreads();
    }
    for (int t0 = c0; t0 < c1; t0 += PD3_TILE) {
        if (t0 + PD3_TILE < c1) load_tile(t0 + PD3_TILE);

        const int tq0 = t0 + wave * 32;
        if (tq0 < c1) {
            bool act[R];
#pragma unroll
            for (int r = 0; r < R; r++) act[r] = tq0 < tile_end[r];

            // ---- S^T: two 16-token K tiles (per-lane K-row fragments), each
            // against the R row tiles ----
            f32x4 st[R][2];
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int s = 0; s < 2; s++)
#pragma unroll
                    for (int e = 0; e < 4; e++) st[r][s][e] = 0.f;
            // Both K tiles' block-table entries are fetched before either
            // K row: the two entry -> row load chains overlap instead of
            // running one after the other.
            long long krec[2];
#pragma unroll
            for (int s = 0; s < 2; s++)
                krec[s] = pkv_record(bt, min(tq0 + s * 16 + l16, c1 - 1),
                                     block_size, Hk, hk);
#pragma unroll
            for (int s = 0; s < 2; s++) {
                frag8 ak[KD];
                pkv_load_k_frags<D, MODE>(ak, k_cache, k_scale, krec[s], lg);
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

            // mask + online softmax (C row = kv = s*16 + lg*4 + e, col = row)
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
                // defer the rescale until some row's max grew by more than 8
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
    const int mr = rows.merge_rows();
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r > 0) __syncthreads();
        if (lg == 0 && l16 < mr) {
            mrg[(wave * mr + l16) * rec + 0] = m_run[r];
            mrg[(wave * mr + l16) * rec + 1] = l_run[r];
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int row = lg * 4 + e;    // O row = query row
            if (row < mr) {
#pragma unroll
                for (int n = 0; n < ND; n++)
                    mrg[(wave * mr + row) * rec + 2 + n * 16 + l16] = acc_o[r][n][e];
            }
        }
        __syncthreads();
        for (int idx = tid; idx < mr * D; idx += PD3_BLOCK) {
            const int row = idx / D, d = idx % D;
            if (!rows.valid(r, row)) continue;
            float gm = -INFINITY;
#pragma unroll
            for (int w = 0; w < PD3_WAVES; w++)
                gm = fmaxf(gm, mrg[(w * mr + row) * rec]);
            float gl = 0.f, oa = 0.f;
#pragma unroll
            for (int w = 0; w < PD3_WAVES; w++) {
                float mw = mrg[(w * mr + row) * rec];
                float a = (mw == -INFINITY) ? 0.f : __expf(mw - gm);
                gl += mrg[(w * mr + row) * rec + 1] * a;
                oa += mrg[(w * mr + row) * rec + 2 + d] * a;
            }
            if (nsplit == 1) {
                float inv = (gl > 0.f) ? 1.0f / gl : 0.f;
                rows.out_row(r, row)[d] = f32_to_bf16(oa * inv);
            } else {
                float* pp = rows.partial_row(r, row);
                if (d == 0) { pp[0] = gm; pp[1] = gl; }
                pp[2 + d] = oa;
            }
        }
    }
}

template <int D, int MODE>
__global__ __launch_bounds__(PD3_BLOCK) void paged_decode_attn3_kernel(
    const ushort_t* __restrict__ q,
    const void* __restrict__ k_cache,
    const void* __restrict__ v_cache,
    const float* __restrict__ k_scale,
    const float* __restrict__ v_scale,
    const int* __restrict__ block_table,
    const int* __restrict__ seq_lens,
    ushort_t* __restrict__ out,
    float* __restrict__ partials,
    int B, int Hq, int Hk, int block_size, int max_blocks, float scale,
    int nsplit) {
    const int b = blockIdx.x;
    const int hk = blockIdx.y;
    const int split = blockIdx.z;
    const int seq_len = seq_lens[b];
    if (seq_len <= 0) return;
    const int chunk = (seq_len + nsplit - 1) / nsplit;
    const int c0 = split * chunk;
    const int c1 = min(seq_len, c0 + chunk);
    const DecodeRows<D> rows{q, out, partials, b, hk, split, nsplit, Hq, Hk,
                             Hq / Hk, c1};
    paged_mfma_attend<D, MODE, 1>(rows, k_cache, v_cache, k_scale, v_scale,
                                  block_table + (long long)b * max_blocks, Hk, hk,
                                  block_size, scale, c0, c1, nsplit);
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
    constexpr int ROWS = 16 * R;
    const int G = Hq / Hk;
    const int b = blockIdx.x / nrg;
    // longest kv range first
    const int rg = nrg - 1 - (blockIdx.x - b * nrg);
    const int hk = blockIdx.y;
    const int split = blockIdx.z;
    const int before = seq_lens_before[b];
    const int n_tok = token_counts ? min(max(token_counts[b], 0), T) : T;
    const int n_valid = n_tok * G;     // valid query rows of this (b, hk)
    const int n0 = rg * ROWS;
    if (n0 >= n_valid || before < 0) return;

    const int kv_end = append_kv_end(before, n0, ROWS, n_valid, G);
    const int chunk = (kv_end + nsplit - 1) / nsplit;
    const int c0 = split * chunk;
    const int c1 = min(kv_end, c0 + chunk);
    if (c0 >= c1) return;              // the split fold skips empty splits too
    const AppendRows<D, R> rows{q, out, partials, b, hk, rg, split, nsplit, nrg,
                                T, Hq, Hk, G, before, n0, n_valid, c1};
    paged_mfma_attend<D, MODE, R>(rows, k_cache, v_cache, k_scale, v_scale,
                                  block_table + (long long)b * max_blocks, Hk, hk,
                                  block_size, scale, c0, c1, nsplit);
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
    const int t = n / G;
    pkv_fold_splits<D>(base, (long long)rows * rec, nsplit, chunk, kv_end,
                       out + (((long long)b * T + t) * Hq + hk * G + (n - t * G)) * D);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
bool launch_paged_decode_attn3(const void* q, const void* k_cache, const void* v_cache,
                               const float* k_scale, const float* v_scale,
                               const int* block_table, const int* seq_lens, void* out,
                               float* partials, int nsplit,
                               int B, int Hq, int Hk, int D, int block_size,
                               int max_blocks, float scale, int cache_mode,
                               hipStream_t stream) {
    if (D != 128 || (Hq % Hk) != 0 || Hq / Hk > PD3_MAXG) return false;
    dim3 grid(B, Hk, nsplit);
    dispatch_cache_mode(cache_mode, [&](auto mode) {
        hipLaunchKernelGGL((paged_decode_attn3_kernel<128, decltype(mode)::value>),
                           grid, dim3(PD3_BLOCK), 0, stream, (const ushort_t*)q,
                           k_cache, v_cache, k_scale, v_scale, block_table, seq_lens,
                           (ushort_t*)out, partials, B, Hq, Hk, block_size,
                           max_blocks, scale, nsplit);
    });
    return true;
}

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
    dispatch_cache_mode(cache_mode, [&](auto mode) {
        constexpr int M = decltype(mode)::value;
        auto kernel = R == 1 ? paged_append_attn_kernel<128, M, 1>
                             : paged_append_attn_kernel<128, M, 2>;
        hipLaunchKernelGGL(kernel, grid, dim3(PD3_BLOCK), 0, stream,
                           (const ushort_t*)q, k_cache, v_cache, k_scale, v_scale,
                           block_table, seq_lens_before, token_counts,
                           (ushort_t*)out, partials, B, T, Hq, Hk, block_size,
                           max_blocks, scale, nsplit, nrg);
    });
    if (nsplit > 1) {
        dim3 mgrid(B * nrg, Hk, 16 * R);
        hipLaunchKernelGGL(paged_append_merge_kernel<128>, mgrid, dim3(64), 0, stream,
                           partials, (ushort_t*)out, seq_lens_before, token_counts,
                           B, T, Hq, Hk, nsplit, nrg, 16 * R);
    }
    return true;
}
