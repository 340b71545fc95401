// Host-side launcher prototypes for the gfx950 kernel pack.  Included by
// bindings.cpp and by every .hip file that defines or calls a launcher, so a
// signature that drifts fails to compile in the defining file.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

// A head dim without a compiled kernel is an error, never a silent no-op.
[[noreturn]] inline void unsupported_head_dim(const char* op, int D) {
    throw std::runtime_error(std::string(op) + ": no kernel for head dim " +
                             std::to_string(D));
}

// ---- rms_norm.hip / rope.hip / swiglu.hip / cross_entropy.hip ----
// delta != nullptr fuses the residual add: h = bf16(x + delta), y = norm(h).
// Without it h is unused and y = norm(x).
void launch_rms_norm_fwd(const void* x, const void* delta, const void* w, void* h,
                         void* y, float* invrms,
                         long long rows, int H, float eps, hipStream_t stream);
// Number of fp32 partial dw rows [P, H] the backward needs for this shape,
// and whether they must be zero-filled (only the streaming path for
// H > 8192 accumulates into them; the register path overwrites them).
int rms_norm_bwd_partials(long long rows, int H, bool* needs_zero);
// dh != nullptr adds the residual-stream gradient: dx = bf16(bf16(dx_norm) + dh).
// dw32 must be zero-filled.
void launch_rms_norm_bwd(const void* dy, const void* x, const void* dh, const void* w,
                         const float* invrms, void* dx, float* dw_partial,
                         float* dw32, void* dw, bool dw_is_bf16,
                         long long rows, int H, int P, hipStream_t stream);
void launch_rope(const void* x, void* out, const float* cos_t, const float* sin_t,
                 long long n_rows, int H, int D, int S, bool backward,
                 hipStream_t stream);
// In-place rotation of the first Hq + Hk heads of each packed
// [(Hq + 2*Hk) * D] row; the V heads are not touched.  D % 16 == 0.
void launch_rope_packed(void* qkv, const float* cos_t, const float* sin_t,
                        long long n_tokens, int Hq, int Hk, int D, int S,
                        bool backward, hipStream_t stream);
void launch_swiglu_fwd(const void* x, void* y, long long N, int I, hipStream_t stream);
void launch_swiglu_bwd(const void* dy, const void* x, void* dx, long long N, int I,
                       hipStream_t stream);
void launch_ce_fwd(const void* logits, const long long* labels, float* loss,
                   float* maxlse, long long N, int V, long long ignore_index,
                   hipStream_t stream);
void launch_ce_bwd(const float* dloss, const void* logits, const long long* labels,
                   const float* maxlse, void* dlogits, long long N, int V,
                   long long ignore_index, hipStream_t stream);

// ---- adamw.hip ----
struct AdamWChunk {
    void* param;       // bf16 or fp32
    const void* grad;  // matches param dtype
    float* m;
    float* v;
    float* master;     // nullptr when param is fp32
    long long offset;  // element offset of this chunk within the tensor
    long long n;       // elements in this chunk
    int is_bf16;
};
void launch_adamw(const AdamWChunk* dev_chunks, int n_chunks,
                  float lr, float beta1, float beta2, float eps, float wd,
                  float bias1, float bias2, hipStream_t stream);

// ---- flash_attn.hip: public attention entry points.  The default tries the
// v2 (D=128) kernels and falls back to v1; force_v1 skips v2. ----
void launch_mfma_probe(const void* A, const void* B, float* C, hipStream_t stream);
void launch_flash_fwd(const void* q, const void* k, const void* v, void* o,
                      float* lse, int B, int Sq, int Skv, int Hq, int Hk, int D,
                      float scale, bool causal, bool force_v1, hipStream_t stream);
void launch_flash_bwd(const void* dout, const void* q, const void* k, const void* v,
                      const void* o, const float* lse, float* delta,
                      void* dq, void* dk, void* dv,
                      int B, int Sq, int Skv, int Hq, int Hk, int D,
                      float scale, bool causal, bool force_v1, hipStream_t stream);
void launch_flash_fwd_mask(const void* q, const void* k, const void* v, void* o,
                           float* lse, const int* startend,
                           int B, int Sq, int Skv, int Hq, int Hk, int D,
                           float scale, hipStream_t stream);
void launch_flash_bwd_mask(const void* dout, const void* q, const void* k, const void* v,
                           const void* o, const float* lse, float* delta,
                           void* dq, void* dk, void* dv, const int* startend,
                           int B, int Sq, int Skv, int Hq, int Hk, int D,
                           float scale, hipStream_t stream);
// delta[b,h,q] = rowsum(dO * O), shared by the v1 and v2 backward
void launch_flash_bwd_delta(const void* dout, const void* o, float* delta,
                            int B, int Sq, int Hq, int D, hipStream_t stream);

// ---- flash_attn_v2.hip / flash_attn_bwd_v2.hip: 8-wave 32x32 kernels.
// Return false (nothing launched) when the shape is not theirs. ----
//
// Row strides, in elements, of the tensors the v2 kernels may read or write
// in place inside a packed [B, S, (Hq + 2*Hk)*D] qkv / dqkv tensor.  Each
// pointer addresses head 0 of token 0 of its tensor; token rows are one
// stride apart and a batch entry is S rows.  o, dout, lse and delta are
// always contiguous.  k and v have one shape and come from one place, so
// they share a stride (kv), as do dk and dv (dkv): the kernels compute one
// row offset for the pair.  nullptr strides = contiguous [B,S,H,D] tensors.
struct FlashStrides { int q, kv, dq, dkv; };
inline FlashStrides flash_contiguous_strides(int Hq, int Hk, int D) {
    return {Hq * D, Hk * D, Hq * D, Hk * D};
}
inline FlashStrides flash_packed_strides(int Hq, int Hk, int D) {
    int w = (Hq + 2 * Hk) * D;
    return {w, w, w, w};
}
// The v2 kernels stage tiles by LDS-DMA in 16-byte pieces: a tensor staged
// that way needs a 16-byte aligned base and a row stride that is a multiple
// of 8 bf16 elements (a head starts at a multiple of D * 2 = 256 bytes).
// The launchers decline anything else, like a shape that is not theirs.
inline bool flash_dma_aligned(const void* p, int row_stride) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && row_stride % 8 == 0;
}
void launch_mfma32_probe(const void* A, const void* B, float* C, hipStream_t stream);
void launch_permlane_probe(int* out0, int* out1, hipStream_t stream);
// X, out_row, out_tr: 64 x 128 bf16 (see mfma.h dual-use image)
void launch_lds_image_probe(const void* X, void* out_row, void* out_tr,
                            hipStream_t stream);
bool launch_flash_fwd2(const void* q, const void* k, const void* v, void* o,
                       float* lse, int B, int Sq, int Skv, int Hq, int Hk,
                       int D, float scale, bool causal, hipStream_t stream,
                       const FlashStrides* strides = nullptr);
bool launch_flash_fwd2_mask(const void* q, const void* k, const void* v,
                            void* o, float* lse, const int* startend,
                            int B, int Sq, int Skv, int Hq, int Hk,
                            int D, float scale, hipStream_t stream,
                            const FlashStrides* strides = nullptr);
// parts: which of the three backward launches to issue (tools/bench_fa.py
// times dq and dkv on their own; everything else takes all three)
enum { FLASH_BWD_DELTA = 1, FLASH_BWD_DQ = 2, FLASH_BWD_DKV = 4, FLASH_BWD_ALL = 7 };
bool launch_flash_bwd2(const void* dout, const void* q, const void* k, const void* v,
                       const void* o, const float* lse, float* delta,
                       void* dq, void* dk, void* dv,
                       int B, int Sq, int Skv, int Hq, int Hk, int D,
                       float scale, bool causal, hipStream_t stream,
                       int parts = FLASH_BWD_ALL,
                       const FlashStrides* strides = nullptr);
bool launch_flash_bwd2_mask(const void* dout, const void* q, const void* k,
                            const void* v, const void* o, const float* lse,
                            float* delta, void* dq, void* dk, void* dv,
                            const int* startend,
                            int B, int Sq, int Skv, int Hq, int Hk, int D,
                            float scale, hipStream_t stream,
                            const FlashStrides* strides = nullptr);

// ---- paged-KV inference.  cache_mode: 0 = bf16 cache, 1 = int8, 2 = int4
// packed nibbles; the kernels take it as a template argument. ----
// f(std::integral_constant<int, cache_mode>{})
template <class F>
inline void dispatch_cache_mode(int cache_mode, F&& f) {
    if (cache_mode == 2) f(std::integral_constant<int, 2>{});
    else if (cache_mode == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}

// ---- paged_attn.hip: decode entry point, scalar decode kernel, split fold,
// rope + cache append ----
int paged_decode_nsplit(int B, int Hk);
void launch_paged_decode_attn(const void* q, const void* k_cache, const void* v_cache,
                              const float* k_scale, const float* v_scale,
                              const int* block_table, const int* seq_lens, void* out,
                              float* partials, int nsplit,
                              int B, int Hq, int Hk, int D, int block_size,
                              int max_blocks, float scale, int cache_mode,
                              hipStream_t stream);
void launch_rope_cache_append(const void* qkv, void* q_out, void* k_cache, void* v_cache,
                              float* k_scale, float* v_scale,
                              const int* block_table, const int* seq_lens_before,
                              const float* cos_t, const float* sin_t,
                              int B, int T, int Hq, int Hk, int D, int block_size,
                              int max_blocks, const int* token_counts,
                              int cache_mode, hipStream_t stream);

// ---- paged_attn_mfma.hip: the MFMA tile loop behind decode and append ----
// MFMA decode kernel; false (nothing launched) unless D==128 and G<=16.
// Writes out (nsplit == 1) or the partials the split-merge kernel consumes.
bool launch_paged_decode_attn3(const void* q, const void* k_cache, const void* v_cache,
                               const float* k_scale, const float* v_scale,
                               const int* block_table, const int* seq_lens, void* out,
                               float* partials, int nsplit,
                               int B, int Hq, int Hk, int D, int block_size,
                               int max_blocks, float scale, int cache_mode,
                               hipStream_t stream);
// Append: T new tokens per sequence over the cache that already holds them.
// q/out are [B, T, Hq, D]; query token t of sequence b sits at
// seq_lens_before[b] + t and attends to positions 0..that.
// Launch geometry: R = 1 or 2 16-row query tiles per workgroup (r_tiles = 0
// picks it from the shape), row groups per (b, kv-head) and kv splits.  false
// when the kernel does not take the shape (D != 128 or GQA group > 16).
bool paged_append_plan(int B, int T, int Hq, int Hk, int D, int r_tiles,
                       int* R, int* nrg, int* nsplit);
// false (nothing launched) for a shape paged_append_plan refuses.  out must
// be zero-filled: rows at or past token_counts[b] are not written.  partials
// holds B*Hk*nrg*nsplit*16R*(2+D) floats when nsplit > 1.
bool launch_paged_append_attn(const void* q, const void* k_cache, const void* v_cache,
                              const float* k_scale, const float* v_scale,
                              const int* block_table, const int* seq_lens_before,
                              const int* token_counts, void* out, float* partials,
                              int r_tiles, int B, int T, int Hq, int Hk, int D,
                              int block_size, int max_blocks, float scale,
                              int cache_mode, hipStream_t stream);

// ---- wint8_gemv.hip / skinny_gemm.hip ----
void launch_wint8_gemv(const void* x, const void* wq, const float* scale, void* y,
                       int M, int N, int K, hipStream_t stream);
void launch_fp8_rowwise_quant(const void* x, void* y, float* scales,
                              long long R, int K, hipStream_t stream);
int skinny_gemm_ksplit(int N, int K, int ksplit_req);
void launch_skinny_gemm(const void* x, const void* w, float* partial, void* y,
                        int M, int N, int K, int ksplit, hipStream_t stream);

// ---- moe_ffn.hip: routed FFN over stacked expert weights [E, K, N].  Every
// grid depends on shapes only; nothing syncs with the host. ----
constexpr int kMoeRowTile = 32;     // MT: rows of one grouped-GEMM tile
constexpr int kMoeMaxExperts = 64;
constexpr int kMoeMaxTopK = 8;
constexpr int kMoeMaxFlatRows = 4096;   // T * K the align kernel takes
// P = roundup(T*K + E*(MT-1), MT): rows of the expert-sorted, tile-padded batch
int moe_padded_rows(int T, int K, int E);
int moe_down_ksplit(int T, int K, int H, int I);
// logits [T, E] fp32 or bf16 -> topk_ids [T, K], topk_w [T, K] (softmax over
// E, top-k, renormalised; ties go to the lower expert index)
void launch_moe_route(const void* logits, bool logits_bf16, int* topk_ids,
                      float* topk_w, int T, int E, int K, hipStream_t stream);
// sorted_rows [P] (flat row t*K + k, -1 = padding), tile_expert [P/MT],
// row_pos [T, K] (inverse of sorted_rows), num_tiles [1]
void launch_moe_align(const int* topk_ids, int* sorted_rows, int* tile_expert,
                      int* row_pos, int* num_tiles, int T, int K, int E,
                      hipStream_t stream);
// act_sorted [P, I] = silu(x @ w1[e]) * (x @ w3[e]) per row tile; zero_row
// holds H bf16 zeros (the source of padding rows).  H % 128 == I % 128 == 0,
// all bases 16-byte aligned.
void launch_moe_gate_up(const void* x, const void* zero_row, const void* w1,
                        const void* w3, const int* sorted_rows,
                        const int* tile_expert, const int* num_tiles,
                        void* act_sorted, int T, int K, int E, int H, int I,
                        hipStream_t stream);
// partial [ksplit, P, H] fp32, ksplit = moe_down_ksplit(...)
void launch_moe_down(const void* act_sorted, const void* w2,
                     const int* tile_expert, const int* num_tiles,
                     float* partial, int ksplit, int T, int K, int E, int H,
                     int I, hipStream_t stream);
void launch_moe_combine(const float* partial, const int* row_pos,
                        const float* topk_w, void* out, int ksplit, int T,
                        int K, int E, int H, hipStream_t stream);
// Weight-only int8 experts: q1/q3 [E, I, H], q2 [E, H, I] int8 (contraction
// contiguous), s1/s3 [E, I], s2 [E, H] fp32 per-column scales.  Route, align
// and combine are the launches above; the down split is counted in this
// path's own 128-deep chunks (moe_down_ksplit_wint8).
int moe_down_ksplit_wint8(int T, int K, int H, int I);
void launch_moe_gate_up_wint8(const void* x, const void* zero_row, const void* q1,
                              const float* s1, const void* q3, const float* s3,
                              const int* sorted_rows, const int* tile_expert,
                              const int* num_tiles, void* act_sorted, int T, int K,
                              int E, int H, int I, hipStream_t stream);
void launch_moe_down_wint8(const void* act_sorted, const void* q2, const float* s2,
                           const int* tile_expert, const int* num_tiles,
                           float* partial, int ksplit, int T, int K, int E, int H,
                           int I, hipStream_t stream);

// ---- sampling.hip ----
void launch_repetition_penalty(void* logits, const long long* pre_ids,
                               const int* pre_lens, const float* rep_pen,
                               int B, long long V, int max_len, hipStream_t s);
void launch_topp_sample(const void* logits, const float* temperature,
                        const float* top_p, const float* uniform,
                        const long long* ban_eos, int n_ban,
                        const int* cur_lens, const int* min_lens,
                        long long* out, int B, long long V, hipStream_t s);
void launch_decode_update(long long* tokens, signed char* stop_flags,
                          const signed char* active, long long* pre_ids,
                          int* pre_lens, int* seq_lens,
                          const long long* eos_ids, int n_eos,
                          int* not_need_stop, const int* max_new,
                          long long pad_id, int B, int max_len, hipStream_t s);
void launch_block_step(int* block_table, int* seq_lens, signed char* stop_flags,
                       signed char* active, int* free_list, int* free_count,
                       signed char* is_block_step, int B, int block_size,
                       int max_blocks, hipStream_t s);
