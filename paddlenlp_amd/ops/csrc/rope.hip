// Fused rotary position embedding (Llama rotate-half convention) — gfx950.
//
// Replaces the reference's fused_rotary_position_embedding.
// q: [B, S, Hq, D], k: [B, S, Hk, D] bf16; cos/sin: [S, D] fp32 host-built
// tables (guide Appendix B: precompute trig on host, never sinf on device).
//
//   out[..., i]       = x[i] * cos[i] - x[i + D/2] * sin[i]        (i < D/2)
//   out[..., i+D/2]   = x[i+D/2] * cos[i+D/2] + x[i] * sin[i+D/2]
// backward = rotation by -theta (sign flip on sin).
#include "common.h"
#include "launchers.h"

// One rotation pair, shared by the out-of-place and the packed in-place
// kernel so that both round identically.
static __device__ __forceinline__ void rope_pair(float a, float b, float c1, float s1,
                                                 float c2, float s2, float sign,
                                                 ushort_t& o1, ushort_t& o2) {
    o1 = f32_to_bf16(a * c1 - sign * b * s1);
    o2 = f32_to_bf16(b * c2 + sign * a * s2);
}

// one thread handles 4 (i, i+D/2) pairs => 8 bf16 loads/stores, coalesced
// within the half-rows.  Layout: token-row = (b*S + s)*H*D + h*D.
__global__ void rope_kernel(
    const ushort_t* __restrict__ x, ushort_t* __restrict__ out,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    long long n_rows,  // B*S*H (q and k launched separately)
    int H, int D, int S, float sign) {
    int half = D / 2;
    long long total = n_rows * half;  // one work-item per rotation pair
    for (long long idx = (long long)blockIdx.x * blockDim.x * 4 + threadIdx.x * 4;
         idx < total; idx += (long long)gridDim.x * blockDim.x * 4) {
        long long row = idx / half;
        int i = (int)(idx % half);
        if (i + 4 > half) continue;  // tails handled by alignment (D%8==0)
        long long s = (row / H) % S;
        const ushort_t* xr = x + row * D;
        ushort_t* outr = out + row * D;
        const float* cr = cos_t + s * D;
        const float* sr = sin_t + s * D;

        short4v x1 = *reinterpret_cast<const short4v*>(xr + i);
        short4v x2 = *reinterpret_cast<const short4v*>(xr + i + half);
        f32x4 c1 = *reinterpret_cast<const f32x4*>(cr + i);
        f32x4 s1 = *reinterpret_cast<const f32x4*>(sr + i);
        f32x4 c2 = *reinterpret_cast<const f32x4*>(cr + i + half);
        f32x4 s2 = *reinterpret_cast<const f32x4*>(sr + i + half);
        short4v o1, o2;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float a = bf16_to_f32((ushort_t)x1[j]);
            float b = bf16_to_f32((ushort_t)x2[j]);
            ushort_t r1, r2;
            rope_pair(a, b, c1[j], s1[j], c2[j], s2[j], sign, r1, r2);
            o1[j] = (short)r1;
            o2[j] = (short)r2;
        }
        *reinterpret_cast<short4v*>(outr + i) = o1;
        *reinterpret_cast<short4v*>(outr + i + half) = o2;
    }
}

// Packed in-place variant: the fused QKV projection's rows are
// [(Hq + 2*Hk) * D]; the first NH = Hq + Hk heads are rotated where they
// lie and the V heads are skipped.  One wave per token: a lane owns 8 pairs
// (two 16-byte loads and stores) at a fixed column slot and walks the heads,
// so the token's cos/sin values are loaded once and reused for every head.
// A wave iteration covers 64 / (D/16) whole heads, i.e. one contiguous span.
#define ROPE_PK_BLOCK 256
__global__ __launch_bounds__(ROPE_PK_BLOCK) void rope_packed_kernel(
    ushort_t* __restrict__ qkv,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    long long n_tokens, int NH, int row_elems, int D, int S, float sign) {
    const int half = D / 2;
    const int cpt = half / 8;              // 16-byte column slots per half head
    const int lane = threadIdx.x & 63;
    const int c = lane % cpt;
    const int hs = lane / cpt;
    const int hpw = 64 / cpt;              // heads per wave iteration
    const long long wave0 = (long long)blockIdx.x * (ROPE_PK_BLOCK / 64) + (threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * (ROPE_PK_BLOCK / 64);
    for (long long tok = wave0; tok < n_tokens; tok += nwaves) {
        const long long s = tok % S;
        const float* cr = cos_t + s * D + c * 8;
        const float* sr = sin_t + s * D + c * 8;
        f32x4 c1[2], s1[2], c2[2], s2[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            c1[u] = *reinterpret_cast<const f32x4*>(cr + u * 4);
            s1[u] = *reinterpret_cast<const f32x4*>(sr + u * 4);
            c2[u] = *reinterpret_cast<const f32x4*>(cr + half + u * 4);
            s2[u] = *reinterpret_cast<const f32x4*>(sr + half + u * 4);
        }
        ushort_t* row = qkv + tok * row_elems + c * 8;
        auto rotate = [&](short8v x1, short8v x2, short8v& o1, short8v& o2) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                ushort_t r1, r2;
                rope_pair(bf16_to_f32((ushort_t)x1[j]), bf16_to_f32((ushort_t)x2[j]),
                          c1[j >> 2][j & 3], s1[j >> 2][j & 3],
                          c2[j >> 2][j & 3], s2[j >> 2][j & 3], sign, r1, r2);
                o1[j] = (short)r1;
                o2[j] = (short)r2;
            }
        };
        // two heads per step, loads first: four 16-byte loads in flight
        for (int h = hs; h < NH; h += 2 * hpw) {
            ushort_t* pa = row + (long long)h * D;
            ushort_t* pb = pa + (long long)hpw * D;
            const bool has_b = h + hpw < NH;
            short8v a1 = *reinterpret_cast<const short8v*>(pa);
            short8v a2 = *reinterpret_cast<const short8v*>(pa + half);
            short8v b1 = a1, b2 = a2;
            if (has_b) {
                b1 = *reinterpret_cast<const short8v*>(pb);
                b2 = *reinterpret_cast<const short8v*>(pb + half);
            }
            short8v o1, o2;
            rotate(a1, a2, o1, o2);
            *reinterpret_cast<short8v*>(pa) = o1;
            *reinterpret_cast<short8v*>(pa + half) = o2;
            if (has_b) {
                rotate(b1, b2, o1, o2);
                *reinterpret_cast<short8v*>(pb) = o1;
                *reinterpret_cast<short8v*>(pb + half) = o2;
            }
        }
    }
}

void launch_rope(const void* x, void* out, const float* cos_t, const float* sin_t,
                 long long n_rows, int H, int D, int S, bool backward,
                 hipStream_t stream) {
    long long total = n_rows * (D / 2) / 4;
    int grid = memgrid(total, 256);
    hipLaunchKernelGGL(rope_kernel, dim3(grid), dim3(256), 0, stream,
                       (const ushort_t*)x, (ushort_t*)out, cos_t, sin_t,
                       n_rows, H, D, S, backward ? -1.0f : 1.0f);
}

void launch_rope_packed(void* qkv, const float* cos_t, const float* sin_t,
                        long long n_tokens, int Hq, int Hk, int D, int S,
                        bool backward, hipStream_t stream) {
    if (n_tokens <= 0) return;
    int grid = memgrid(n_tokens * 64, ROPE_PK_BLOCK);
    hipLaunchKernelGGL(rope_packed_kernel, dim3(grid), dim3(ROPE_PK_BLOCK), 0, stream,
                       (ushort_t*)qkv, cos_t, sin_t, n_tokens, Hq + Hk,
                       (Hq + 2 * Hk) * D, D, S, backward ? -1.0f : 1.0f);
}
