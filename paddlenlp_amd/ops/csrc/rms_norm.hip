// RMSNorm forward/backward, optionally fused with the residual add that
// precedes it — gfx950, bf16 in / bf16 out, fp32 math.
//
// Replaces the reference's fused_rms_norm (paddlenlp fused op, SURVEY §2.9
// "training-side fused ops").  Memory-bound: vectorized short8 loads
// (guide G13), one workgroup per row, fp32 accumulation.
//
// fwd:  y = x * rsqrt(mean(x^2) + eps) * w          (saves invrms per row)
// bwd:  dx = invrms * (dy*w - x * invrms^2 * mean(dy*w*x))
//       dw = sum_rows(dy * x * invrms)   (two-pass partial reduction)
//
// With HAS_RES the same kernels also do the residual add around the norm:
// fwd:  h = bf16(residual + delta); y = rms_norm(h)   (from the rounded h)
// bwd:  dx = bf16(bf16(dx_norm) + dh)    (what autograd's separate add gives)
// Both flavours are one template, so their arithmetic and reduction order
// are the same and the fused op is bit-equal to the two separate ops.
//
// Register path (H <= RMS_REG_MAX_H): a thread owns the columns
// (v*RMS_BLOCK + tid)*8 .. +7 for v < NV.  A row is read once and kept in
// registers between the reduction and the output pass, and dw accumulates in
// NV*8 fp32 registers per thread that are written once, as one partial row
// per block.  Larger H takes the streaming path (NV = 0): rows are re-read
// for the output pass and dw accumulates in a zero-filled global partial row.
#include "common.h"
#include "launchers.h"

#define RMS_BLOCK 256
#define RMS_MAX_NV 4
#define RMS_REG_MAX_H (RMS_BLOCK * 8 * RMS_MAX_NV)   // 8192

static __device__ __forceinline__ short8v ld8(const ushort_t* p) {
    return *reinterpret_cast<const short8v*>(p);
}
static __device__ __forceinline__ void st8(ushort_t* p, short8v v) {
    *reinterpret_cast<short8v*>(p) = v;
}

// bf16(a + b), the bf16 add of the unfused composition
static __device__ __forceinline__ short8v add8(short8v a, short8v b) {
    short8v r;
#pragma unroll
    for (int j = 0; j < 8; j++)
        r[j] = (short)f32_to_bf16(bf16_to_f32((ushort_t)a[j]) + bf16_to_f32((ushort_t)b[j]));
    return r;
}

static __device__ __forceinline__ float sumsq8(short8v v, float ss) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        float f = bf16_to_f32((ushort_t)v[j]);
        ss += f * f;
    }
    return ss;
}

static __device__ __forceinline__ short8v norm8(short8v v, short8v wv, float inv) {
    short8v out;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        float f = bf16_to_f32((ushort_t)v[j]) * inv * bf16_to_f32((ushort_t)wv[j]);
        out[j] = (short)f32_to_bf16(f);
    }
    return out;
}

// one block per row; H must be a multiple of 8 (hidden sizes are).
// HAS_RES: x is the residual, delta is added to it and the sum is written to h.
template <bool HAS_RES, int NV>
__global__ __launch_bounds__(RMS_BLOCK) void rms_norm_fwd_kernel(
    const ushort_t* __restrict__ x, const ushort_t* __restrict__ delta,
    const ushort_t* __restrict__ w, ushort_t* __restrict__ h,
    ushort_t* __restrict__ y, float* __restrict__ invrms,
    int H, float eps, long long rows) {
    __shared__ float scratch[16];
    const int tid = threadIdx.x;
    short8v wv[NV > 0 ? NV : 1];
    if constexpr (NV > 0) {
#pragma unroll
        for (int v = 0; v < NV; v++) {
            int i = (v * RMS_BLOCK + tid) * 8;
            if (i < H) wv[v] = ld8(w + i);
        }
    }
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const ushort_t* xr = x + row * H;
        ushort_t* yr = y + row * H;
        float ss = 0.f;
        if constexpr (NV > 0) {
            short8v xv[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) {
                int i = (v * RMS_BLOCK + tid) * 8;
                if (i < H) {
                    xv[v] = ld8(xr + i);
                    if constexpr (HAS_RES) {
                        xv[v] = add8(xv[v], ld8(delta + row * H + i));
                        st8(h + row * H + i, xv[v]);
                    }
                    ss = sumsq8(xv[v], ss);
                }
            }
            ss = block_reduce_sum(ss, scratch);
            float inv = rsqrtf(ss / H + eps);
            if (tid == 0) invrms[row] = inv;
#pragma unroll
            for (int v = 0; v < NV; v++) {
                int i = (v * RMS_BLOCK + tid) * 8;
                if (i < H) st8(yr + i, norm8(xv[v], wv[v], inv));
            }
        } else {
            for (int i = tid * 8; i < H; i += RMS_BLOCK * 8) {
                short8v v = ld8(xr + i);
                if constexpr (HAS_RES) {
                    v = add8(v, ld8(delta + row * H + i));
                    st8(h + row * H + i, v);
                }
                ss = sumsq8(v, ss);
            }
            ss = block_reduce_sum(ss, scratch);
            float inv = rsqrtf(ss / H + eps);
            if (tid == 0) invrms[row] = inv;
            // each thread re-reads the columns it wrote itself
            const ushort_t* hr = HAS_RES ? h + row * H : xr;
            for (int i = tid * 8; i < H; i += RMS_BLOCK * 8)
                st8(yr + i, norm8(ld8(hr + i), ld8(w + i), inv));
        }
    }
}

// c += sum_j dy*w*x
static __device__ __forceinline__ float dot3_8(short8v dv, short8v wv, short8v xv, float c) {
#pragma unroll
    for (int j = 0; j < 8; j++)
        c += bf16_to_f32((ushort_t)dv[j]) * bf16_to_f32((ushort_t)wv[j]) * bf16_to_f32((ushort_t)xv[j]);
    return c;
}

// dx for 8 columns (plus the residual gradient when HAS_RES); dw[j] gets
// this row's dy*x*invrms
template <bool HAS_RES, typename DW>
static __device__ __forceinline__ short8v bwd8(short8v dv, short8v xv, short8v wv, short8v dhv,
                                               float inv, float k, DW&& dw) {
    short8v out;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        float dyf = bf16_to_f32((ushort_t)dv[j]);
        float xf = bf16_to_f32((ushort_t)xv[j]);
        float wf = bf16_to_f32((ushort_t)wv[j]);
        float dxf = inv * (dyf * wf - xf * k);
        ushort_t o = f32_to_bf16(dxf);
        if constexpr (HAS_RES)
            o = f32_to_bf16(bf16_to_f32(o) + bf16_to_f32((ushort_t)dhv[j]));
        out[j] = (short)o;
        dw(j, dyf * xf * inv);
    }
    return out;
}

// Register path.  x is the norm's input (h of the fused forward); dh is the
// gradient that reaches h from the residual stream.  Block b writes partial
// row b of dw_partial once, after its last row; no zero-fill is needed.  The
// next row's loads are issued before the block reduction of the current row,
// so a block keeps two rows in flight.
template <bool HAS_RES, int NV>
__global__ __launch_bounds__(RMS_BLOCK) void rms_norm_bwd_dx_kernel(
    const ushort_t* __restrict__ dy, const ushort_t* __restrict__ x,
    const ushort_t* __restrict__ dh, const ushort_t* __restrict__ w,
    const float* __restrict__ invrms,
    ushort_t* __restrict__ dx, float* __restrict__ dw_partial,
    int H, long long rows) {
    __shared__ float scratch[16];
    const int tid = threadIdx.x;
    short8v wv[NV], cdy[NV], cx[NV], cdh[NV], ndy[NV], nx[NV], ndh[NV];
    float dwacc[NV][8];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        int i = (v * RMS_BLOCK + tid) * 8;
        wv[v] = (i < H) ? ld8(w + i) : short8v{0, 0, 0, 0, 0, 0, 0, 0};
        cdy[v] = wv[v]; cx[v] = wv[v]; cdh[v] = wv[v];
        ndy[v] = wv[v]; nx[v] = wv[v]; ndh[v] = wv[v];
#pragma unroll
        for (int j = 0; j < 8; j++) dwacc[v][j] = 0.f;
    }
    long long row = blockIdx.x;
    if (row < rows) {
#pragma unroll
        for (int v = 0; v < NV; v++) {
            int i = (v * RMS_BLOCK + tid) * 8;
            if (i < H) {
                cdy[v] = ld8(dy + row * H + i);
                cx[v] = ld8(x + row * H + i);
                if constexpr (HAS_RES) cdh[v] = ld8(dh + row * H + i);
            }
        }
    }
    for (; row < rows; row += gridDim.x) {
        float inv = invrms[row];
        // pass 1: c = sum(dy * w * x) (fp32)
        float c = 0.f;
#pragma unroll
        for (int v = 0; v < NV; v++) {
            int i = (v * RMS_BLOCK + tid) * 8;
            if (i < H) c = dot3_8(cdy[v], wv[v], cx[v], c);
        }
        long long next = row + gridDim.x;
        if (next < rows) {
#pragma unroll
            for (int v = 0; v < NV; v++) {
                int i = (v * RMS_BLOCK + tid) * 8;
                if (i < H) {
                    ndy[v] = ld8(dy + next * H + i);
                    nx[v] = ld8(x + next * H + i);
                    if constexpr (HAS_RES) ndh[v] = ld8(dh + next * H + i);
                }
            }
        }
        c = block_reduce_sum(c, scratch);
        float k = c * inv * inv / H;
        // pass 2: dx + dw partials
#pragma unroll
        for (int v = 0; v < NV; v++) {
            int i = (v * RMS_BLOCK + tid) * 8;
            if (i < H) {
                float* acc = dwacc[v];
                st8(dx + row * H + i,
                    bwd8<HAS_RES>(cdy[v], cx[v], wv[v], cdh[v], inv, k,
                                  [&](int j, float t) { acc[j] += t; }));
            }
        }
#pragma unroll
        for (int v = 0; v < NV; v++) { cdy[v] = ndy[v]; cx[v] = nx[v]; cdh[v] = ndh[v]; }
    }
    float* dwp = dw_partial + (long long)blockIdx.x * H;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        int i = (v * RMS_BLOCK + tid) * 8;
        if (i < H) {
            *reinterpret_cast<f32x4*>(dwp + i) =
                f32x4{dwacc[v][0], dwacc[v][1], dwacc[v][2], dwacc[v][3]};
            *reinterpret_cast<f32x4*>(dwp + i + 4) =
                f32x4{dwacc[v][4], dwacc[v][5], dwacc[v][6], dwacc[v][7]};
        }
    }
}

// Streaming path for H > RMS_REG_MAX_H: rows are read twice and dw
// accumulates in the block's zero-filled fp32 partial row in global memory.
template <bool HAS_RES>
__global__ __launch_bounds__(RMS_BLOCK) void rms_norm_bwd_dx_stream_kernel(
    const ushort_t* __restrict__ dy, const ushort_t* __restrict__ x,
    const ushort_t* __restrict__ dh, const ushort_t* __restrict__ w,
    const float* __restrict__ invrms,
    ushort_t* __restrict__ dx, float* __restrict__ dw_partial,
    int H, long long rows) {
    __shared__ float scratch[16];
    float* dwp = dw_partial + (long long)blockIdx.x * H;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const ushort_t* dyr = dy + row * H;
        const ushort_t* xr = x + row * H;
        float inv = invrms[row];
        float c = 0.f;
        for (int i = threadIdx.x * 8; i < H; i += RMS_BLOCK * 8)
            c = dot3_8(ld8(dyr + i), ld8(w + i), ld8(xr + i), c);
        c = block_reduce_sum(c, scratch);
        float k = c * inv * inv / H;
        for (int i = threadIdx.x * 8; i < H; i += RMS_BLOCK * 8) {
            short8v dhv = short8v{0, 0, 0, 0, 0, 0, 0, 0};
            if constexpr (HAS_RES) dhv = ld8(dh + row * H + i);
            float* acc = dwp + i;
            st8(dx + row * H + i,
                bwd8<HAS_RES>(ld8(dyr + i), ld8(xr + i), ld8(w + i), dhv, inv, k,
                              [&](int j, float t) { acc[j] += t; }));
        }
    }
}

// reduce dw partials [P, H] -> dw32 [H] fp32.  Parallelized over BOTH axes:
// grid.x covers columns, grid.y slices the P partials; one atomicAdd per
// (column, slice) — ~grid.y adders per address, negligible contention (G12).
__global__ void rms_norm_bwd_dw_reduce_kernel(
    const float* __restrict__ dw_partial, float* __restrict__ dw32,
    int H, int P) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H) return;
    int p0 = blockIdx.y;
    float acc = 0.f;
    for (int p = p0; p < P; p += gridDim.y) acc += dw_partial[(long long)p * H + i];
    atomicAdd(&dw32[i], acc);
}

__global__ void rms_norm_bwd_dw_cast_kernel(
    const float* __restrict__ dw32, ushort_t* __restrict__ dw, int H) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < H) dw[i] = f32_to_bf16(dw32[i]);
}

// ---- launchers (called from bindings.cpp) ----
// columns of 8 per thread on the register path; 0 = streaming path
static int rms_nv(int H) {
    if (H > RMS_REG_MAX_H) return 0;
    int nv = (H + RMS_BLOCK * 8 - 1) / (RMS_BLOCK * 8);
    return nv == 3 ? 4 : nv;
}

template <bool HAS_RES>
static void rms_norm_fwd_t(const ushort_t* x, const ushort_t* delta, const ushort_t* w,
                           ushort_t* h, ushort_t* y, float* invrms,
                           long long rows, int H, float eps, hipStream_t stream) {
    int grid = (int)(rows < 8192 ? rows : 8192);
#define RMS_FWD(NV)                                                                  \
    hipLaunchKernelGGL((rms_norm_fwd_kernel<HAS_RES, NV>), dim3(grid), dim3(RMS_BLOCK), \
                       0, stream, x, delta, w, h, y, invrms, H, eps, rows)
    switch (rms_nv(H)) {
        case 1: RMS_FWD(1); break;
        case 2: RMS_FWD(2); break;
        case 4: RMS_FWD(4); break;
        default: RMS_FWD(0); break;
    }
#undef RMS_FWD
}

void launch_rms_norm_fwd(const void* x, const void* delta, const void* w, void* h,
                         void* y, float* invrms,
                         long long rows, int H, float eps, hipStream_t stream) {
    if (rows <= 0) return;
    if (delta)
        rms_norm_fwd_t<true>((const ushort_t*)x, (const ushort_t*)delta, (const ushort_t*)w,
                             (ushort_t*)h, (ushort_t*)y, invrms, rows, H, eps, stream);
    else
        rms_norm_fwd_t<false>((const ushort_t*)x, nullptr, (const ushort_t*)w,
                              nullptr, (ushort_t*)y, invrms, rows, H, eps, stream);
}

int rms_norm_bwd_partials(long long rows, int H, bool* needs_zero) {
    *needs_zero = rms_nv(H) == 0;
    // 2048 partial rows on both paths.  Fewer would do for the register path
    // (512 shorten the reduce kernel from 15 to 6 us at H = 4096), but the
    // row -> partial -> slice summation tree decides the rounding of dw, and
    // this one keeps dw, and with it a whole training run, bit-identical to
    // what the global-accumulation scheme produced.
    long long cap = 2048;
    return (int)(rows < cap ? (rows > 0 ? rows : 1) : cap);
}

template <bool HAS_RES>
static void rms_norm_bwd_dx_t(const ushort_t* dy, const ushort_t* x, const ushort_t* dh,
                              const ushort_t* w, const float* invrms, ushort_t* dx,
                              float* dw_partial, long long rows, int H, int P,
                              hipStream_t stream) {
#define RMS_BWD(NV)                                                                    \
    hipLaunchKernelGGL((rms_norm_bwd_dx_kernel<HAS_RES, NV>), dim3(P), dim3(RMS_BLOCK), \
                       0, stream, dy, x, dh, w, invrms, dx, dw_partial, H, rows)
    switch (rms_nv(H)) {
        case 1: RMS_BWD(1); break;
        case 2: RMS_BWD(2); break;
        case 4: RMS_BWD(4); break;
        default:
            hipLaunchKernelGGL((rms_norm_bwd_dx_stream_kernel<HAS_RES>), dim3(P),
                               dim3(RMS_BLOCK), 0, stream, dy, x, dh, w, invrms, dx,
                               dw_partial, H, rows);
            break;
    }
#undef RMS_BWD
}

void launch_rms_norm_bwd(const void* dy, const void* x, const void* dh, const void* w,
                         const float* invrms, void* dx, float* dw_partial,
                         float* dw32, void* dw, bool dw_is_bf16,
                         long long rows, int H, int P, hipStream_t stream) {
    if (dh)
        rms_norm_bwd_dx_t<true>((const ushort_t*)dy, (const ushort_t*)x, (const ushort_t*)dh,
                                (const ushort_t*)w, invrms, (ushort_t*)dx, dw_partial,
                                rows, H, P, stream);
    else
        rms_norm_bwd_dx_t<false>((const ushort_t*)dy, (const ushort_t*)x, nullptr,
                                 (const ushort_t*)w, invrms, (ushort_t*)dx, dw_partial,
                                 rows, H, P, stream);
    int rgrid = (H + 255) / 256;
    int pslices = P > 64 ? 64 : P;
    hipLaunchKernelGGL(rms_norm_bwd_dw_reduce_kernel, dim3(rgrid, pslices), dim3(256), 0, stream,
                       dw_partial, dw32, H, P);
    if (dw_is_bf16) {
        hipLaunchKernelGGL(rms_norm_bwd_dw_cast_kernel, dim3(rgrid), dim3(256), 0, stream,
                           dw32, (ushort_t*)dw, H);
    }
}
