// Fused MoE FFN for decode — gfx950.
//
//   out[t] = sum_k w[t,k] * ( silu(x[t] @ w1[e]) * (x[t] @ w3[e]) ) @ w2[e],
//   e = topk_ids[t,k]
//
// over stacked expert weights stored [E, K, N] with N contiguous
// (w1/w3: [E, H, I], w2: [E, I, H]).  Reference behavior: the reference's
// fused_moe op (fused_transformer_layers.py:951-1008).
//
// Every launch has a grid that depends on tensor shapes only; what the routing
// leaves empty exits early, a whole workgroup at a time.  There is no host
// sync and no atomic anywhere, so the path can be captured into a graph and
// two runs on the same inputs are bit-identical.
//
//   moe_route    one wave per token, a lane per expert: fp32 softmax over all
//                E, top-k, renormalise the k weights to sum to 1.
//                TIE RULE: among equal probabilities the LOWER expert index
//                wins, and the k results are in descending-probability order
//                (ops.reference.moe_route states the same rule).
//   moe_align    one workgroup: groups the T*K flat rows (t*K + k) by expert,
//                ascending flat row inside an expert, each expert's segment
//                padded to a multiple of the row tile.
//                P = roundup(T*K + E*(MT-1), MT) rows are always enough.
//   moe_gemm<1>  gate/up grouped GEMM with fused SwiGLU: grid (I/128, P/MT).
//   moe_gemm<0>  down grouped GEMM, contraction split over blockIdx.z into
//                fp32 partials [ksplit, P, H].
//   moe_combine  out[t] = bf16(sum_k w[t,k] * sum_s partial[s, row_pos[t,k]]),
//                both sums in index order.
//
// Tile choice: MT = 32 rows with the 32x32x16 MFMA, N tile 128 (one 32-column
// sub-tile per wave, 4 waves), K chunk 64.  The weights are contracted over
// their ROWS, which is the case mfma.h's dual-use image and its transposed
// read (img_tr_frag, ds_read_b64_tr_b16) exist for, and both are laid out and
// hardware-checked for the 32x32x16 operands; 16-row tiles would need a
// 16-wide transposed read derived and checked from scratch, and the kernel is
// bound by the weight stream, not by the MFMA rows a short tile wastes.
//
// The weight slabs ([64][128] per chunk, w1 and w3 in the gated kernel) and
// the gathered activation rows ([32][64] per chunk) are staged by LDS-DMA,
// double-buffered with one barrier per chunk as in flash_fwd2.  The DMA cannot
// zero-fill, so a padding row is fetched from a row of zeros the caller
// provides: it is staged as zeros, nothing is masked, and EXEC stays all ones
// around the transposed reads.  Per docs/kernels.md the DMA is waited for
// explicitly before the barrier and no compiler-issued load is pending inside
// the chunk loop (the per-lane row lookup is retired ahead of it).
//
// Weight-only int8 experts (moe_gemm_wint8_kernel, both GEMMs): the weights
// are stored contraction-major, [E, N, Kd] int8 with Kd contiguous, plus one
// fp32 scale per (expert, column) [E, N].  Same tiles and the same loop, with
// K chunk 128: a weight chunk is a [128 n][128 k]-byte image (16 KB, the bytes
// the bf16 kernel has in flight), the activation chunk [32][128] bf16 (8 KB).
// With Kd contiguous the B operand needs no transposed read.  A lane reads 16
// consecutive bytes of its column, W[n][32*kk + 16*hi .. +16], as one
// ds_read_b128 and uses them for TWO MFMA steps (low and high 8 bytes); the
// activation fragment of a step takes the same k (the order of k inside a
// chunk is free as long as both operands agree).  int8 -> bf16 is exact
// (v_cvt_f32_i32 on a sign-extended byte, v_cvt_pk_bf16_f32), the MFMA is the
// bf16 one, and the column scale multiplies the fp32 sum once, in the
// epilogue.  Padding rows still come from the zero row; EXEC stays full.
//
// LDS banks of the int8 path (64 banks of 4 bytes; a ds_read_b128 is served in
// four groups of 16 lanes, {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same
// + 32, 256 bytes each, so a group is conflict-free when its 16 addresses are
// 16 distinct 16-byte slots modulo 256 bytes):
//   weights    row n (128 bytes) holds source chunk c in slot c ^ ((n>>1) & 7).
//              A group reads one chunk c of 8 even and 8 odd rows.  Even rows
//              lie in banks 0-31, odd rows in banks 32-63, and (n>>1) & 7
//              takes all 8 values over the 8 rows of either parity in every
//              group (rows 0,2,12,14,20,22,24,26 -> 0,1,6,7,2,3,4,5; rows
//              4,6,8,10,16,18,28,30 -> 2,3,4,5,0,1,6,7), so the 16 lanes cover
//              the 64 banks once.  An 8-byte read per MFMA step with this XOR
//              would put two rows of a 32-lane group on every bank pair.
//   activation row m (256 bytes, starts at bank 0) holds source unit u (8 bf16)
//              in slot u ^ (m & 15); a group reads one unit of 16 rows whose
//              m & 15 are all different, so again 64 banks once.
// The DMA destination is lane-linear, so both XORs are applied to the per-lane
// source address.
#include "common.h"
#include "launchers.h"
#include "mfma.h"

#define MOE_MT 32
#define MOE_NT 128
#define MOE_KC 64
#define MOE_KC8 128                    // K chunk of the int8-weight kernels
#define MOE_WAVES 4
#define MOE_BLOCK (MOE_WAVES * 64)
#define MOE_MAX_E kMoeMaxExperts
#define MOE_MAX_ROWS kMoeMaxFlatRows   // T*K the align kernel ranks in LDS

static_assert(MOE_MT == kMoeRowTile, "launchers.h states the row tile");
static_assert(MOE_MAX_E <= 64, "routing gives every expert a lane");

// ---------------------------------------------------------------------------
// routing
// ---------------------------------------------------------------------------
template <typename LT>
__device__ __forceinline__ float moe_logit(const LT* p, long long i);
template <>
__device__ __forceinline__ float moe_logit<float>(const float* p, long long i) {
    return p[i];
}
template <>
__device__ __forceinline__ float moe_logit<ushort_t>(const ushort_t* p, long long i) {
    return bf16_to_f32(p[i]);
}

template <typename LT>
__global__ __launch_bounds__(MOE_BLOCK) void moe_route_kernel(
    const LT* __restrict__ logits,   // [T, E]
    int* __restrict__ topk_ids,      // [T, K]
    float* __restrict__ topk_w,      // [T, K]
    int T, int E, int K) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * MOE_WAVES + (threadIdx.x >> 6);
    if (t >= T) return;              // a whole wave at a time

    const float x = lane < E ? moe_logit<LT>(logits, (long long)t * E + lane) : -INFINITY;
    const float m = wave_reduce_max(x);
    const float ex = lane < E ? expf(x - m) : 0.f;
    const float s = wave_reduce_sum(ex);
    float p = lane < E ? ex / s : -1.f;     // -1: never selected

    float my_p = 0.f, sum = 0.f;
    int my_i = 0;
    for (int k = 0; k < K; k++) {
        float bv = p;
        int bi = lane;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == k) { my_p = bv; my_i = bi; }
        if (lane == bi) p = -1.f;
        sum += bv;                           // k order, the same in every lane
    }
    if (lane < K) {
        topk_ids[(long long)t * K + lane] = my_i;
        topk_w[(long long)t * K + lane] = my_p / sum;
    }
}

// ---------------------------------------------------------------------------
// alignment (one workgroup)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MOE_BLOCK) void moe_align_kernel(
    const int* __restrict__ topk_ids,   // [N] flat rows
    int* __restrict__ sorted_rows,      // [P]
    int* __restrict__ tile_expert,      // [P / MT]
    int* __restrict__ row_pos,          // [N]
    int* __restrict__ num_tiles,        // [1]
    int N, int E, int P) {
    __shared__ int rank[MOE_MAX_ROWS];
    __shared__ int cnt[MOE_MAX_E];
    __shared__ int off[MOE_MAX_E + 1];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    // rank of every flat row inside its expert, ascending flat order: wave w
    // takes experts w, w + 4, ... and walks the rows 64 at a time
    for (int e = wave; e < E; e += MOE_WAVES) {
        int c = 0;
        for (int i0 = 0; i0 < N; i0 += 64) {
            const int i = i0 + lane;
            const bool mine = i < N && topk_ids[i] == e;
            const unsigned long long b = __ballot(mine);
            if (mine) rank[i] = c + __popcll(b & ((1ull << lane) - 1ull));
            c += __popcll(b);
        }
        if (lane == 0) cnt[e] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int e = 0; e < E; e++) {
            off[e] = o;
            o += (cnt[e] + MOE_MT - 1) / MOE_MT * MOE_MT;
        }
        off[E] = o;
        num_tiles[0] = o / MOE_MT;
    }
    __syncthreads();

    // padding slots and the tile -> expert map; the slots of real rows are
    // written by the scatter below (disjoint, so no ordering is needed)
    for (int p = tid; p < P; p += MOE_BLOCK) {
        int e = -1;
        for (int j = 0; j < E; j++)
            if (p >= off[j] && p < off[j + 1]) e = j;
        if ((p % MOE_MT) == 0) tile_expert[p / MOE_MT] = e;
        if (e < 0 || p >= off[e] + cnt[e]) sorted_rows[p] = -1;
    }
    for (int i = tid; i < N; i += MOE_BLOCK) {
        const int e = topk_ids[i];
        int pos = -1;
        if (e >= 0 && e < E) {
            pos = off[e] + rank[i];
            sorted_rows[pos] = i;
        }
        row_pos[i] = pos;
    }
}

// ---------------------------------------------------------------------------
// grouped GEMM: C[32 rows of one tile][128] = A[32][Kd] @ W[e][Kd][n0 .. +128]
// ---------------------------------------------------------------------------
template <bool GATED>
__global__ __launch_bounds__(MOE_BLOCK) void moe_gemm_kernel(
    const ushort_t* __restrict__ a,          // GATED: x [T, Kd]; else act [P, Kd]
    const ushort_t* __restrict__ zero_row,   // GATED: Kd zeros (padding rows)
    const ushort_t* __restrict__ wa,         // [E, Kd, N]  (w1 / w2)
    const ushort_t* __restrict__ wb,         // [E, Kd, N]  (w3; GATED only)
    const int* __restrict__ sorted_rows,     // [P] (GATED only)
    const int* __restrict__ tile_expert,     // [P / MT]
    const int* __restrict__ num_tiles,       // [1]
    ushort_t* __restrict__ act_out,          // GATED: [P, N]
    float* __restrict__ partial,             // else: [ksplit, P, N]
    int Kd, int N, int topk, int P, int chunks_per_split) {
    constexpr int NW = GATED ? 2 : 1;
    // [buffer][matrix] dual-use images of one [64][128] weight chunk and the
    // [32][64] activation chunk (128-byte rows, 16-byte slots XORed with
    // row & 7 so the 32 rows of an A fragment spread over the banks)
    __shared__ __attribute__((aligned(16))) ushort_t w_lds[2][NW][MOE_KC * MOE_NT];
    __shared__ __attribute__((aligned(16))) ushort_t a_lds[2][MOE_MT * MOE_KC];

    const int tile = blockIdx.y;
    if (tile >= num_tiles[0]) return;        // whole workgroup, before any LDS traffic
    const int e = tile_expert[tile];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int l32 = lane & 31;
    const int hi = lane >> 5;
    const int n0 = blockIdx.x * MOE_NT;

    const int nch = Kd / MOE_KC;
    const int c0 = blockIdx.z * chunks_per_split;
    const int c1 = min(nch, c0 + chunks_per_split);

    // activation staging: wave w fills rows 8w .. 8w+7 of the chunk with one
    // 1 KiB DMA; lane l lands in row 8w + (l >> 3), slot l & 7, and so
    // fetches source chunk (l & 7) ^ (row & 7)
    const int a_row = 8 * wave + (lane >> 3);
    const ushort_t* a_src;
    if (GATED) {
        const int sr = sorted_rows[tile * MOE_MT + a_row];
        a_src = sr < 0 ? zero_row : a + (long long)(sr / topk) * Kd;
    } else {
        a_src = a + (long long)(tile * MOE_MT + a_row) * Kd;
    }
    a_src += ((lane & 7) ^ ((lane >> 3) & 7)) * 8;
    // retire the row lookup: left pending, its counted vmcnt wait inside the
    // loop would also drain the (uncounted) DMA in flight
    asm volatile("" :: "v"(a_src));

    // weight staging: 16 pieces of 1 KiB per image, 4 per wave
    int w_off[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int piece = wave * 4 + i;
        w_off[i] = img_fill_row(piece, lane) * N + img_fill_chunk(piece, lane) * 8;
    }
    const ushort_t* wa_e = wa + (long long)e * Kd * N + n0;
    const ushort_t* wb_e = GATED ? wb + (long long)e * Kd * N + n0 : nullptr;

    auto issue_chunk = [&](int c, int buf) {
        const long long k0 = (long long)c * MOE_KC;
        lds_dma16(a_src + k0, &a_lds[buf][wave * 512]);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int piece = wave * 4 + i;
            lds_dma16(wa_e + k0 * N + w_off[i], &w_lds[buf][0][piece * 512]);
            if (GATED)
                lds_dma16(wb_e + k0 * N + w_off[i], &w_lds[buf][NW - 1][piece * 512]);
        }
    };

    f32x16 acc_a, acc_b;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc_a[r] = 0.f; acc_b[r] = 0.f; }

    if (c0 < c1) issue_chunk(c0, 0);
    for (int c = c0; c < c1; c++) {
        const int cur = (c - c0) & 1;
        // chunk c has landed and every wave is done reading the other
        // buffer, which chunk c+1 now overwrites while chunk c is computed
        lds_dma_wait_all();
        __syncthreads();
        if (c + 1 < c1) issue_chunk(c + 1, cur ^ 1);

        const char* a_img = reinterpret_cast<const char*>(a_lds[cur]);
        const int lane_t = fresh_lane_id();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < MOE_KC / 16; ks++) {
            // A[row = l32][k = ks*16 + hi*8 .. +8]
            const frag8 af = *reinterpret_cast<const frag8*>(
                a_img + 128 * l32 + 16 * ((ks * 2 + hi) ^ (l32 & 7)));
            const frag8 b0 = img_tr_frag(w_lds[cur][0], ks, wave, lane_t);
            acc_a = mfma32(af, b0, acc_a);
            if (GATED) {
                const frag8 b1 = img_tr_frag(w_lds[cur][NW - 1], ks, wave, lane_t);
                acc_b = mfma32(af, b1, acc_b);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    }

    // C row crow32(r, hi), column l32 of this wave's 32-column sub-tile
    const int col = n0 + wave * 32 + l32;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const long long row = (long long)tile * MOE_MT + crow32(r, hi);
        if (GATED) {
            const float g = acc_a[r], u = acc_b[r];
            act_out[row * N + col] = f32_to_bf16(g / (1.f + __expf(-g)) * u);
        } else {
            partial[((long long)blockIdx.z * P + row) * N + col] = acc_a[r];
        }
    }
}

// ---------------------------------------------------------------------------
// grouped GEMM over weight-only int8 experts: the same tile loop, with the
// weights stored [E, N, Kd] int8 (Kd contiguous) and one fp32 scale per
// (expert, column).  See the file header for the LDS images and their banks.
// ---------------------------------------------------------------------------
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// 8 int8 (two dwords, ascending k) -> 8 bf16.  Every value of -128..127 has at
// most 8 significant bits, so both conversions are exact.
__device__ __forceinline__ frag8 moe_dequant8(unsigned lo, unsigned hi) {
    union { frag8 f; unsigned u[4]; } r;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const unsigned w = h ? hi : lo;
        r.u[2 * h] = pack_bf16((float)(signed char)(w & 0xff),
                               (float)(signed char)((w >> 8) & 0xff));
        r.u[2 * h + 1] = pack_bf16((float)(signed char)((w >> 16) & 0xff),
                                   (float)(signed char)(w >> 24));
    }
    return r.f;
}

template <bool GATED>
__global__ __launch_bounds__(MOE_BLOCK) void moe_gemm_wint8_kernel(
    const ushort_t* __restrict__ a,          // GATED: x [T, Kd]; else act [P, Kd]
    const ushort_t* __restrict__ zero_row,   // GATED: Kd zeros (padding rows)
    const signed char* __restrict__ qa,      // [E, N, Kd]  (q1 / q2)
    const signed char* __restrict__ qb,      // [E, N, Kd]  (q3; GATED only)
    const float* __restrict__ sa,            // [E, N] scales of qa
    const float* __restrict__ sb,            // [E, N] scales of qb (GATED only)
    const int* __restrict__ sorted_rows,     // [P] (GATED only)
    const int* __restrict__ tile_expert,     // [P / MT]
    const int* __restrict__ num_tiles,       // [1]
    ushort_t* __restrict__ act_out,          // GATED: [P, N]
    float* __restrict__ partial,             // else: [ksplit, P, N]
    int Kd, int N, int topk, int P, int chunks_per_split) {
    constexpr int NW = GATED ? 2 : 1;
    // [buffer][matrix] images of one [128 n][128 k] int8 weight chunk and the
    // [32][128] bf16 activation chunk
    __shared__ __attribute__((aligned(16))) signed char w_lds[2][NW][MOE_NT * MOE_KC8];
    __shared__ __attribute__((aligned(16))) ushort_t a_lds[2][MOE_MT * MOE_KC8];

    const int tile = blockIdx.y;
    if (tile >= num_tiles[0]) return;        // whole workgroup, before any LDS traffic
    const int e = tile_expert[tile];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int l32 = lane & 31;
    const int hi = lane >> 5;
    const int n0 = blockIdx.x * MOE_NT;

    const int nch = Kd / MOE_KC8;
    const int c0 = blockIdx.z * chunks_per_split;
    const int c1 = min(nch, c0 + chunks_per_split);

    // activation staging: wave w fills rows 8w .. 8w+7 of the chunk with two
    // 1 KiB DMAs of four 256-byte rows; lane l lands in row 8w + 4i + (l >> 4),
    // slot l & 15, and so fetches source unit (l & 15) ^ (row & 15)
    const ushort_t* a_src[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int a_row = 8 * wave + 4 * i + (lane >> 4);
        if (GATED) {
            const int sr = sorted_rows[tile * MOE_MT + a_row];
            a_src[i] = sr < 0 ? zero_row : a + (long long)(sr / topk) * Kd;
        } else {
            a_src[i] = a + (long long)(tile * MOE_MT + a_row) * Kd;
        }
        a_src[i] += ((lane & 15) ^ (a_row & 15)) * 8;
    }
    // retire the row lookups: left pending, their counted vmcnt wait inside
    // the loop would also drain the (uncounted) DMA in flight
    asm volatile("" :: "v"(a_src[0]), "v"(a_src[1]));

    // weight staging: 16 pieces of 1 KiB (eight 128-byte rows) per image, 4 per
    // wave, which are the 32 rows the wave itself reads; lane l lands in row
    // 8*piece + (l >> 3), slot l & 7, and fetches source chunk
    // (l & 7) ^ ((row >> 1) & 7)
    int w_off[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = 8 * (wave * 4 + i) + (lane >> 3);
        w_off[i] = row * Kd + 16 * ((lane & 7) ^ ((row >> 1) & 7));
    }
    const signed char* qa_e = qa + ((long long)e * N + n0) * Kd;
    const signed char* qb_e = GATED ? qb + ((long long)e * N + n0) * Kd : nullptr;

    auto issue_chunk = [&](int c, int buf) {
        const long long k0 = (long long)c * MOE_KC8;
#pragma unroll
        for (int i = 0; i < 2; i++)
            lds_dma16(a_src[i] + k0, &a_lds[buf][(wave * 2 + i) * 512]);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int piece = wave * 4 + i;
            lds_dma16(qa_e + k0 + w_off[i], &w_lds[buf][0][piece * 1024]);
            if (GATED)
                lds_dma16(qb_e + k0 + w_off[i], &w_lds[buf][NW - 1][piece * 1024]);
        }
    };

    f32x16 acc_a, acc_b;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc_a[r] = 0.f; acc_b[r] = 0.f; }

    // this lane's weight row and the XOR terms of both images
    const int w_row = 128 * (wave * 32 + l32);
    const int w_x = hi ^ ((l32 >> 1) & 7);
    const int a_x = (2 * hi) ^ (l32 & 15);

    if (c0 < c1) issue_chunk(c0, 0);
    for (int c = c0; c < c1; c++) {
        const int cur = (c - c0) & 1;
        // chunk c has landed and every wave is done reading the other
        // buffer, which chunk c+1 now overwrites while chunk c is computed
        lds_dma_wait_all();
        __syncthreads();
        if (c + 1 < c1) issue_chunk(c + 1, cur ^ 1);

        const char* a_img = reinterpret_cast<const char*>(a_lds[cur]) + 256 * l32;
        const char* wa_img = reinterpret_cast<const char*>(w_lds[cur][0]) + w_row;
        const char* wb_img = reinterpret_cast<const char*>(w_lds[cur][NW - 1]) + w_row;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < MOE_KC8 / 32; kk++) {
            // W[n][k = 32*kk + 16*hi .. +16]: MFMA steps 2kk (low 8 bytes)
            // and 2kk + 1 (high 8 bytes)
            const u32x4 qa4 = *reinterpret_cast<const u32x4*>(wa_img + 16 * ((2 * kk) ^ w_x));
            u32x4 qb4;
            if (GATED) qb4 = *reinterpret_cast<const u32x4*>(wb_img + 16 * ((2 * kk) ^ w_x));
#pragma unroll
            for (int half = 0; half < 2; half++) {
                // A[row = l32][k = 32*kk + 16*hi + 8*half .. +8]
                const frag8 af = *reinterpret_cast<const frag8*>(
                    a_img + 16 * ((4 * kk + half) ^ a_x));
                acc_a = mfma32(af, moe_dequant8(qa4[2 * half], qa4[2 * half + 1]), acc_a);
                if (GATED)
                    acc_b = mfma32(af, moe_dequant8(qb4[2 * half], qb4[2 * half + 1]), acc_b);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    }

    // C row crow32(r, hi), column l32 of this wave's 32-column sub-tile; the
    // column's scale is applied once, to the fp32 sum
    const int col = n0 + wave * 32 + l32;
    const float scale_a = sa[(long long)e * N + col];
    const float scale_b = GATED ? sb[(long long)e * N + col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const long long row = (long long)tile * MOE_MT + crow32(r, hi);
        if (GATED) {
            const float g = acc_a[r] * scale_a, u = acc_b[r] * scale_b;
            act_out[row * N + col] = f32_to_bf16(g / (1.f + __expf(-g)) * u);
        } else {
            partial[((long long)blockIdx.z * P + row) * N + col] = acc_a[r] * scale_a;
        }
    }
}

// ---------------------------------------------------------------------------
// combine
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MOE_BLOCK) void moe_combine_kernel(
    const float* __restrict__ partial,   // [ksplit, P, H]
    const int* __restrict__ row_pos,     // [T, K]
    const float* __restrict__ topk_w,    // [T, K]
    ushort_t* __restrict__ out,          // [T, H]
    int K, int H, int P, int ksplit) {
    const int t = blockIdx.y;
    const int col = (blockIdx.x * MOE_BLOCK + threadIdx.x) * 4;
    if (col >= H) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k++) {
        const int pos = row_pos[t * K + k];
        if (pos < 0) continue;
        const float w = topk_w[t * K + k];
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int z = 0; z < ksplit; z++)
            s += *reinterpret_cast<const f32x4*>(
                partial + ((long long)z * P + pos) * H + col);
        acc += w * s;
    }
    short4v o;
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = (short)f32_to_bf16(acc[j]);
    *reinterpret_cast<short4v*>(out + (long long)t * H + col) = o;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int moe_padded_rows(int T, int K, int E) {
    return (T * K + E * (MOE_MT - 1) + MOE_MT - 1) / MOE_MT * MOE_MT;
}

// Splits of the down GEMM's contraction, from shapes only: T*K rows occupy at
// least ceil(T*K / MT) row tiles, each H/128 workgroups wide; split until
// that lower bound reaches the 256 CUs, then round to splits of equal chunk
// counts, none of them empty.  kc is the kernel's K chunk.
static int moe_down_ksplit_of(int T, int K, int H, int I, int kc) {
    const int nch = I / kc;
    const int min_tiles = (T * K + MOE_MT - 1) / MOE_MT;
    const int wgs = (H / MOE_NT) * min_tiles;
    int want = (256 + wgs - 1) / wgs;
    want = want < 1 ? 1 : (want > nch ? nch : want);
    const int per = (nch + want - 1) / want;
    return (nch + per - 1) / per;
}
int moe_down_ksplit(int T, int K, int H, int I) {
    return moe_down_ksplit_of(T, K, H, I, MOE_KC);
}
int moe_down_ksplit_wint8(int T, int K, int H, int I) {
    return moe_down_ksplit_of(T, K, H, I, MOE_KC8);
}

void launch_moe_route(const void* logits, bool logits_bf16, int* topk_ids,
                      float* topk_w, int T, int E, int K, hipStream_t stream) {
    if (T == 0) return;
    dim3 grid((T + MOE_WAVES - 1) / MOE_WAVES);
    if (logits_bf16)
        hipLaunchKernelGGL(moe_route_kernel<ushort_t>, grid, dim3(MOE_BLOCK), 0, stream,
                           (const ushort_t*)logits, topk_ids, topk_w, T, E, K);
    else
        hipLaunchKernelGGL(moe_route_kernel<float>, grid, dim3(MOE_BLOCK), 0, stream,
                           (const float*)logits, topk_ids, topk_w, T, E, K);
}

void launch_moe_align(const int* topk_ids, int* sorted_rows, int* tile_expert,
                      int* row_pos, int* num_tiles, int T, int K, int E,
                      hipStream_t stream) {
    hipLaunchKernelGGL(moe_align_kernel, dim3(1), dim3(MOE_BLOCK), 0, stream,
                       topk_ids, sorted_rows, tile_expert, row_pos, num_tiles,
                       T * K, E, moe_padded_rows(T, K, E));
}

void launch_moe_gate_up(const void* x, const void* zero_row, const void* w1,
                        const void* w3, const int* sorted_rows,
                        const int* tile_expert, const int* num_tiles,
                        void* act_sorted, int T, int K, int E, int H, int I,
                        hipStream_t stream) {
    const int P = moe_padded_rows(T, K, E);
    dim3 grid(I / MOE_NT, P / MOE_MT);
    hipLaunchKernelGGL(moe_gemm_kernel<true>, grid, dim3(MOE_BLOCK), 0, stream,
                       (const ushort_t*)x, (const ushort_t*)zero_row,
                       (const ushort_t*)w1, (const ushort_t*)w3, sorted_rows,
                       tile_expert, num_tiles, (ushort_t*)act_sorted,
                       (float*)nullptr, H, I, K, P, H / MOE_KC);
}

void launch_moe_down(const void* act_sorted, const void* w2,
                     const int* tile_expert, const int* num_tiles,
                     float* partial, int ksplit, int T, int K, int E, int H,
                     int I, hipStream_t stream) {
    const int P = moe_padded_rows(T, K, E);
    const int nch = I / MOE_KC;
    dim3 grid(H / MOE_NT, P / MOE_MT, ksplit);
    hipLaunchKernelGGL(moe_gemm_kernel<false>, grid, dim3(MOE_BLOCK), 0, stream,
                       (const ushort_t*)act_sorted, (const ushort_t*)nullptr,
                       (const ushort_t*)w2, (const ushort_t*)nullptr,
                       (const int*)nullptr, tile_expert, num_tiles,
                       (ushort_t*)nullptr, partial, I, H, K, P,
                       (nch + ksplit - 1) / ksplit);
}

void launch_moe_gate_up_wint8(const void* x, const void* zero_row, const void* q1,
                              const float* s1, const void* q3, const float* s3,
                              const int* sorted_rows, const int* tile_expert,
                              const int* num_tiles, void* act_sorted, int T, int K,
                              int E, int H, int I, hipStream_t stream) {
    const int P = moe_padded_rows(T, K, E);
    dim3 grid(I / MOE_NT, P / MOE_MT);
    hipLaunchKernelGGL(moe_gemm_wint8_kernel<true>, grid, dim3(MOE_BLOCK), 0, stream,
                       (const ushort_t*)x, (const ushort_t*)zero_row,
                       (const signed char*)q1, (const signed char*)q3, s1, s3,
                       sorted_rows, tile_expert, num_tiles, (ushort_t*)act_sorted,
                       (float*)nullptr, H, I, K, P, H / MOE_KC8);
}

void launch_moe_down_wint8(const void* act_sorted, const void* q2, const float* s2,
                           const int* tile_expert, const int* num_tiles,
                           float* partial, int ksplit, int T, int K, int E, int H,
                           int I, hipStream_t stream) {
    const int P = moe_padded_rows(T, K, E);
    const int nch = I / MOE_KC8;
    dim3 grid(H / MOE_NT, P / MOE_MT, ksplit);
    hipLaunchKernelGGL(moe_gemm_wint8_kernel<false>, grid, dim3(MOE_BLOCK), 0, stream,
                       (const ushort_t*)act_sorted, (const ushort_t*)nullptr,
                       (const signed char*)q2, (const signed char*)nullptr, s2,
                       (const float*)nullptr, (const int*)nullptr, tile_expert,
                       num_tiles, (ushort_t*)nullptr, partial, I, H, K, P,
                       (nch + ksplit - 1) / ksplit);
}

void launch_moe_combine(const float* partial, const int* row_pos,
                        const float* topk_w, void* out, int ksplit, int T,
                        int K, int E, int H, hipStream_t stream) {
    if (T == 0) return;
    dim3 grid((H / 4 + MOE_BLOCK - 1) / MOE_BLOCK, T);
    hipLaunchKernelGGL(moe_combine_kernel, grid, dim3(MOE_BLOCK), 0, stream,
                       partial, row_pos, topk_w, (ushort_t*)out, K, H,
                       moe_padded_rows(T, K, E), ksplit);
}
