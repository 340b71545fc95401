// Python bindings for the paddlenlp_amd gfx950 kernel pack.
// Built by setup.py via torch.utils.cpp_extension (hipcc, PYTORCH_ROCM_ARCH=gfx950).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <vector>

#include "launchers.h"

#define CHECK_GPU(x) TORCH_CHECK(x.is_cuda(), #x " must be on GPU")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")
#define CHECK_BF16(x) TORCH_CHECK(x.scalar_type() == torch::kBFloat16, #x " must be bf16")

static hipStream_t cur_stream() {
    return at::hip::getCurrentHIPStream().stream();
}

// ---------------------------------------------------------------------------
// delta defined: h = bf16(x + delta), y = rms_norm(h); returns {h, y, invrms}.
// Otherwise y = rms_norm(x); returns {y, invrms}.
static std::vector<torch::Tensor> rms_norm_fwd_impl(const torch::Tensor& x,
                                                    const torch::Tensor* delta,
                                                    const torch::Tensor& w, double eps) {
    CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x); CHECK_BF16(w);
    int H = x.size(-1);
    TORCH_CHECK(H % 8 == 0, "hidden size must be a multiple of 8");
    TORCH_CHECK(w.numel() == H && w.is_contiguous(), "weight must be a contiguous [H] tensor");
    long long rows = x.numel() / H;
    auto y = torch::empty_like(x);
    auto invrms = torch::empty({rows}, x.options().dtype(torch::kFloat32));
    if (!delta) {
        launch_rms_norm_fwd(x.data_ptr(), nullptr, w.data_ptr(), nullptr, y.data_ptr(),
                            invrms.data_ptr<float>(), rows, H, (float)eps, cur_stream());
        return {y, invrms};
    }
    CHECK_GPU((*delta)); CHECK_CONTIG((*delta)); CHECK_BF16((*delta));
    TORCH_CHECK(delta->sizes() == x.sizes(), "residual and delta shapes must agree");
    auto h = torch::empty_like(x);
    launch_rms_norm_fwd(x.data_ptr(), delta->data_ptr(), w.data_ptr(), h.data_ptr(),
                        y.data_ptr(), invrms.data_ptr<float>(), rows, H, (float)eps,
                        cur_stream());
    return {h, y, invrms};
}

// dh defined: dx = bf16(bf16(dx_norm) + dh), the gradient of both addends.
static std::vector<torch::Tensor> rms_norm_bwd_impl(const torch::Tensor& dy,
                                                    const torch::Tensor* dh,
                                                    const torch::Tensor& x,
                                                    const torch::Tensor& w,
                                                    const torch::Tensor& invrms) {
    CHECK_GPU(dy); CHECK_CONTIG(dy); CHECK_BF16(dy);
    CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
    TORCH_CHECK(dy.sizes() == x.sizes(), "dy must be shaped like x");
    int H = x.size(-1);
    TORCH_CHECK(H % 8 == 0, "hidden size must be a multiple of 8");
    long long rows = x.numel() / H;
    TORCH_CHECK(invrms.numel() == rows, "invrms must have one entry per row");
    if (dh) {
        CHECK_GPU((*dh)); CHECK_CONTIG((*dh)); CHECK_BF16((*dh));
        TORCH_CHECK(dh->sizes() == x.sizes(), "dh must be shaped like x");
    }
    bool needs_zero = false;
    int P = rms_norm_bwd_partials(rows, H, &needs_zero);
    auto dx = torch::empty_like(x);
    auto f32 = x.options().dtype(torch::kFloat32);
    auto dw_partial = needs_zero ? torch::zeros({P, H}, f32) : torch::empty({P, H}, f32);
    bool w_bf16 = w.scalar_type() == torch::kBFloat16;
    auto dw32 = torch::zeros({H}, f32);
    auto dw = w_bf16 ? torch::empty_like(w) : dw32;
    launch_rms_norm_bwd(dy.data_ptr(), x.data_ptr(), dh ? dh->data_ptr() : nullptr,
                        w.data_ptr(), invrms.data_ptr<float>(), dx.data_ptr(),
                        dw_partial.data_ptr<float>(), dw32.data_ptr<float>(),
                        dw.data_ptr(), w_bf16, rows, H, P, cur_stream());
    return {dx, dw};
}

std::vector<torch::Tensor> rms_norm_fwd(torch::Tensor x, torch::Tensor w, double eps) {
    return rms_norm_fwd_impl(x, nullptr, w, eps);
}

std::vector<torch::Tensor> rms_norm_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w,
                                        torch::Tensor invrms) {
    return rms_norm_bwd_impl(dy, nullptr, x, w, invrms);
}

std::vector<torch::Tensor> add_rms_norm_fwd(torch::Tensor residual, torch::Tensor delta,
                                            torch::Tensor w, double eps) {
    return rms_norm_fwd_impl(residual, &delta, w, eps);
}

std::vector<torch::Tensor> add_rms_norm_bwd(torch::Tensor dy, torch::Tensor dh,
                                            torch::Tensor h, torch::Tensor w,
                                            torch::Tensor invrms) {
    return rms_norm_bwd_impl(dy, &dh, h, w, invrms);
}

// ---------------------------------------------------------------------------
std::vector<torch::Tensor> rope_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor cos_t, torch::Tensor sin_t,
                                    bool backward) {
    CHECK_GPU(q); CHECK_CONTIG(q); CHECK_BF16(q);
    CHECK_GPU(k); CHECK_CONTIG(k); CHECK_BF16(k);
    CHECK_GPU(cos_t); CHECK_GPU(sin_t);
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4, "q/k must be [B,S,H,D]");
    int B = q.size(0), S = q.size(1), Hq = q.size(2), D = q.size(3);
    int Hk = k.size(2);
    TORCH_CHECK(k.size(0) == B && k.size(1) == S && k.size(3) == D,
                "k must agree with q in B, S and D");
    TORCH_CHECK(D % 8 == 0, "head dim must be a multiple of 8");
    auto cf = cos_t.to(torch::kFloat32).contiguous();
    auto sf = sin_t.to(torch::kFloat32).contiguous();
    TORCH_CHECK(cf.size(0) == S && cf.size(-1) == D && cf.numel() == (int64_t)S * D &&
                    sf.sizes() == cf.sizes(),
                "cos/sin tables must be [S, D]");
    auto q_out = torch::empty_like(q);
    auto k_out = torch::empty_like(k);
    launch_rope(q.data_ptr(), q_out.data_ptr(), cf.data_ptr<float>(), sf.data_ptr<float>(),
                (long long)B * S * Hq, Hq, D, S, backward, cur_stream());
    launch_rope(k.data_ptr(), k_out.data_ptr(), cf.data_ptr<float>(), sf.data_ptr<float>(),
                (long long)B * S * Hk, Hk, D, S, backward, cur_stream());
    return {q_out, k_out};
}

// Rotates the q and k heads of packed [B, S, (Hq + 2*Hk)*D] rows in place
// (backward: by -theta, on dqkv) and leaves the v heads alone.
void rope_packed_(torch::Tensor qkv, torch::Tensor cos_t, torch::Tensor sin_t,
                  int64_t Hq, int64_t Hk, bool backward) {
    CHECK_GPU(qkv); CHECK_CONTIG(qkv); CHECK_BF16(qkv);
    TORCH_CHECK(qkv.dim() == 3, "qkv must be [B, S, (Hq+2*Hk)*D]");
    TORCH_CHECK(Hq > 0 && Hk > 0 && qkv.size(2) % (Hq + 2 * Hk) == 0,
                "last dim must be (Hq + 2*Hk) * D");
    int B = qkv.size(0), S = qkv.size(1);
    int D = (int)(qkv.size(2) / (Hq + 2 * Hk));
    TORCH_CHECK(D % 16 == 0 && D <= 1024 && 64 % (D / 16) == 0,
                "packed rope takes head dims 16, 32, 64, 128, 256, 512, 1024; got ", D);
    auto cf = cos_t.to(torch::kFloat32).contiguous();
    auto sf = sin_t.to(torch::kFloat32).contiguous();
    TORCH_CHECK(cf.dim() == 2 && cf.size(0) == S && cf.size(1) == D &&
                    sf.sizes() == cf.sizes(),
                "cos/sin tables must be [S, D]");
    launch_rope_packed(qkv.data_ptr(), cf.data_ptr<float>(), sf.data_ptr<float>(),
                       (long long)B * S, (int)Hq, (int)Hk, D, S, backward, cur_stream());
}

// ---------------------------------------------------------------------------
torch::Tensor swiglu_fwd(torch::Tensor x) {
    CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
    int twoI = x.size(-1);
    TORCH_CHECK(twoI % 16 == 0, "last dim must be a multiple of 16");
    int I = twoI / 2;
    long long N = x.numel() / twoI;
    auto sizes = x.sizes().vec();
    sizes.back() = I;
    auto y = torch::empty(sizes, x.options());
    launch_swiglu_fwd(x.data_ptr(), y.data_ptr(), N, I, cur_stream());
    return y;
}

torch::Tensor swiglu_bwd(torch::Tensor dy, torch::Tensor x) {
    CHECK_GPU(dy); CHECK_CONTIG(dy); CHECK_BF16(dy);
    CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
    int twoI = x.size(-1);
    TORCH_CHECK(twoI % 16 == 0, "last dim must be a multiple of 16");
    int I = twoI / 2;
    auto dy_sizes = x.sizes().vec();
    dy_sizes.back() = I;
    TORCH_CHECK(dy.sizes() == c10::IntArrayRef(dy_sizes),
                "dy must be shaped like x with half the last dim");
    long long N = x.numel() / twoI;
    auto dx = torch::empty_like(x);
    launch_swiglu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), N, I, cur_stream());
    return dx;
}

// ---------------------------------------------------------------------------
std::vector<torch::Tensor> cross_entropy_fwd(torch::Tensor logits, torch::Tensor labels,
                                             int64_t ignore_index) {
    CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
    TORCH_CHECK(logits.dim() == 2, "logits must be [N, V]");
    long long N = logits.size(0);
    int V = logits.size(1);
    TORCH_CHECK(V % 8 == 0, "vocab must be a multiple of 8");
    CHECK_GPU(labels);
    TORCH_CHECK(labels.numel() == N, "labels must have one entry per row");
    auto labels64 = labels.to(torch::kInt64).contiguous();
    auto loss =torch::empty({N}, logits.options().dtype(torch::kFloat32));
    auto maxlse = torch::empty({N, 2}, logits.options().dtype(torch::kFloat32));
    launch_ce_fwd(logits.data_ptr(), reinterpret_cast<const long long*>(labels64.data_ptr<int64_t>()),
                  loss.data_ptr<float>(), maxlse.data_ptr<float>(), N, V,
                  ignore_index, cur_stream());
    return {loss, maxlse};
}

torch::Tensor cross_entropy_bwd(torch::Tensor dloss, torch::Tensor logits,
                                torch::Tensor labels, torch::Tensor maxlse,
                                int64_t ignore_index) {
    CHECK_GPU(dloss);
    CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
    TORCH_CHECK(logits.dim() == 2, "logits must be [N, V]");
    long long N = logits.size(0);
    int V = logits.size(1);
    TORCH_CHECK(V % 8 == 0, "vocab must be a multiple of 8");
    CHECK_GPU(labels); CHECK_GPU(maxlse);
    TORCH_CHECK(labels.numel() == N, "labels must have one entry per row");
    TORCH_CHECK(dloss.numel() == N, "dloss must have one entry per row");
    TORCH_CHECK(maxlse.scalar_type() == torch::kFloat32 && maxlse.is_contiguous() &&
                    maxlse.dim() == 2 && maxlse.size(0) == N && maxlse.size(1) == 2,
                "maxlse must be the contiguous fp32 [N, 2] the forward returned");
    auto labels64 = labels.to(torch::kInt64).contiguous();
    auto dl = dloss.to(torch::kFloat32).contiguous();
    auto dlogits = torch::empty_like(logits);
    launch_ce_bwd(dl.data_ptr<float>(), logits.data_ptr(),
                  reinterpret_cast<const long long*>(labels64.data_ptr<int64_t>()), maxlse.data_ptr<float>(),
                  dlogits.data_ptr(), N, V, ignore_index, cur_stream());
    return dlogits;
}

// ---------------------------------------------------------------------------
torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B) {
    CHECK_GPU(A); CHECK_BF16(A);
    auto C = torch::empty({16, 16}, A.options().dtype(torch::kFloat32));
    launch_mfma_probe(A.contiguous().data_ptr(), B.contiguous().data_ptr(),
                      C.data_ptr<float>(), cur_stream());
    return C;
}

void apply_repetition_penalty(torch::Tensor logits, torch::Tensor pre_ids,
                              torch::Tensor pre_lens, torch::Tensor rep_pen) {
    CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
    int B = logits.size(0);
    long long V = logits.size(1);
    launch_repetition_penalty(logits.data_ptr(),
                              reinterpret_cast<const long long*>(pre_ids.data_ptr<int64_t>()),
                              pre_lens.data_ptr<int>(), rep_pen.data_ptr<float>(),
                              B, V, pre_ids.size(1), cur_stream());
}

torch::Tensor topp_sample(torch::Tensor logits, torch::Tensor temperature,
                          torch::Tensor top_p, torch::Tensor uniform,
                          c10::optional<torch::Tensor> ban_eos,
                          c10::optional<torch::Tensor> cur_lens,
                          c10::optional<torch::Tensor> min_lens) {
    CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
    int B = logits.size(0);
    long long V = logits.size(1);
    auto out = torch::empty({B}, logits.options().dtype(torch::kInt64));
    launch_topp_sample(
        logits.data_ptr(), temperature.data_ptr<float>(), top_p.data_ptr<float>(),
        uniform.data_ptr<float>(),
        ban_eos ? reinterpret_cast<const long long*>(ban_eos->data_ptr<int64_t>()) : nullptr,
        ban_eos ? (int)ban_eos->numel() : 0,
        cur_lens ? cur_lens->data_ptr<int>() : nullptr,
        min_lens ? min_lens->data_ptr<int>() : nullptr,
        reinterpret_cast<long long*>(out.data_ptr<int64_t>()), B, V, cur_stream());
    return out;
}

void decode_update(torch::Tensor tokens, torch::Tensor stop_flags, torch::Tensor active,
                   torch::Tensor pre_ids, torch::Tensor pre_lens, torch::Tensor seq_lens,
                   torch::Tensor eos_ids, torch::Tensor not_need_stop,
                   c10::optional<torch::Tensor> max_new, int64_t pad_id) {
    int B = tokens.size(0);
    launch_decode_update(
        reinterpret_cast<long long*>(tokens.data_ptr<int64_t>()),
        stop_flags.data_ptr<signed char>(), active.data_ptr<signed char>(),
        reinterpret_cast<long long*>(pre_ids.data_ptr<int64_t>()),
        pre_lens.data_ptr<int>(), seq_lens.data_ptr<int>(),
        reinterpret_cast<const long long*>(eos_ids.data_ptr<int64_t>()),
        (int)eos_ids.numel(), not_need_stop.data_ptr<int>(),
        max_new ? max_new->data_ptr<int>() : nullptr,
        (long long)pad_id, B, (int)pre_ids.size(1), cur_stream());
}

void block_step(torch::Tensor block_table, torch::Tensor seq_lens,
                torch::Tensor stop_flags, torch::Tensor active,
                torch::Tensor free_list, torch::Tensor free_count,
                torch::Tensor is_block_step, int64_t block_size) {
    int B = block_table.size(0);
    launch_block_step(block_table.data_ptr<int>(), seq_lens.data_ptr<int>(),
                      stop_flags.data_ptr<signed char>(), active.data_ptr<signed char>(),
                      free_list.data_ptr<int>(), free_count.data_ptr<int>(),
                      is_block_step.data_ptr<signed char>(), B, (int)block_size,
                      (int)block_table.size(1), cur_stream());
}

torch::Tensor mfma32_probe(torch::Tensor A, torch::Tensor B) {
    CHECK_GPU(A); CHECK_BF16(A);
    auto C = torch::empty({32, 32}, A.options().dtype(torch::kFloat32));
    launch_mfma32_probe(A.contiguous().data_ptr(), B.contiguous().data_ptr(),
                        C.data_ptr<float>(), cur_stream());
    return C;
}

std::vector<torch::Tensor> permlane_probe() {
    auto opt = torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA);
    auto o0 = torch::empty({64}, opt);
    auto o1 = torch::empty({64}, opt);
    launch_permlane_probe(o0.data_ptr<int>(), o1.data_ptr<int>(), cur_stream());
    return {o0, o1};
}

// dual-use LDS image probe: X [64,128] bf16 -> (row view, transposed view)
std::vector<torch::Tensor> lds_image_probe(torch::Tensor X) {
    CHECK_GPU(X); CHECK_BF16(X);
    TORCH_CHECK(X.dim() == 2 && X.size(0) == 64 && X.size(1) == 128,
                "lds_image_probe: X must be [64,128]");
    auto Xc = X.contiguous();
    auto out_row = torch::empty_like(Xc);
    auto out_tr = torch::empty_like(Xc);
    launch_lds_image_probe(Xc.data_ptr(), out_row.data_ptr(), out_tr.data_ptr(),
                           cur_stream());
    return {out_row, out_tr};
}

// ---------------------------------------------------------------------------
// flash attention.  Every entry point validates through check_attn_args, so
// a shape without a kernel is an error before anything is launched.
// ---------------------------------------------------------------------------
// q [B,Sq,Hq,D]; k, v [B,Skv,Hk,D]; backward adds dout, o (shaped like q)
// and lse [B,Hq,Sq] fp32; FlashMask adds startend with B*Skv elements.
static void check_attn_args(const torch::Tensor& q, const torch::Tensor& k,
                            const torch::Tensor& v,
                            const torch::Tensor* dout = nullptr,
                            const torch::Tensor* o = nullptr,
                            const torch::Tensor* lse = nullptr,
                            const torch::Tensor* startend = nullptr) {
    auto check4d = [](const torch::Tensor& t, const char* name) {
        TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
        TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
        TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
        TORCH_CHECK(t.dim() == 4, name, " must be [B,S,H,D]");
    };
    check4d(q, "q");
    check4d(k, "k");
    check4d(v, "v");
    int64_t B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
    int64_t Skv = k.size(1), Hk = k.size(2);
    TORCH_CHECK(D == 128 || D == 64 || D == 32, "head dim must be 32/64/128, got ", D);
    TORCH_CHECK(k.sizes() == v.sizes(), "k and v shapes must agree");
    TORCH_CHECK(k.size(0) == B && k.size(3) == D, "k/v must be [B,Skv,Hk,D] matching q");
    TORCH_CHECK(Hk > 0 && Hq % Hk == 0, "GQA requires Hq % Hk == 0");
    if (dout) {
        check4d(*dout, "dout");
        TORCH_CHECK(dout->sizes() == q.sizes(), "dout must be shaped like q");
    }
    if (o) {
        check4d(*o, "o");
        TORCH_CHECK(o->sizes() == q.sizes(), "o must be shaped like q");
    }
    if (lse) {
        TORCH_CHECK(lse->is_cuda() && lse->is_contiguous() &&
                        lse->scalar_type() == torch::kFloat32 &&
                        lse->sizes() == at::IntArrayRef({B, Hq, Sq}),
                    "lse must be a contiguous fp32 [B,Hq,Sq] GPU tensor");
    }
    if (startend) {
        TORCH_CHECK(startend->is_cuda(), "startend must be on GPU");
        TORCH_CHECK(startend->numel() == B * Skv, "startend must be [B, Skv]");
    }
}

std::vector<torch::Tensor> flash_attn_fwd_ex(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                             bool causal, bool force_v1) {
    check_attn_args(q, k, v);
    int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
    int Skv = k.size(1), Hk = k.size(2);
    auto o = torch::empty_like(q);
    auto lse = torch::empty({B, Hq, Sq}, q.options().dtype(torch::kFloat32));
    float scale = 1.0f / std::sqrt((float)D);
    launch_flash_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                     lse.data_ptr<float>(), B, Sq, Skv, Hq, Hk, D, scale, causal,
                     force_v1, cur_stream());
    return {o, lse};
}

std::vector<torch::Tensor> flash_attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                          bool causal) {
    return flash_attn_fwd_ex(q, k, v, causal, /*force_v1=*/false);
}

std::vector<torch::Tensor> flash_attn_bwd_ex(torch::Tensor dout, torch::Tensor q,
                                             torch::Tensor k, torch::Tensor v,
                                             torch::Tensor o, torch::Tensor lse,
                                             bool causal, bool force_v1) {
    check_attn_args(q, k, v, &dout, &o, &lse);
    int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
    int Skv = k.size(1), Hk = k.size(2);
    auto dq = torch::empty_like(q);
    auto dk_h = torch::empty({B, Skv, Hk, D}, k.options());
    auto dv_h = torch::empty({B, Skv, Hk, D}, v.options());
    auto delta = torch::empty({B, Hq, Sq}, q.options().dtype(torch::kFloat32));
    float scale = 1.0f / std::sqrt((float)D);
    launch_flash_bwd(dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
                     o.data_ptr(), lse.data_ptr<float>(), delta.data_ptr<float>(),
                     dq.data_ptr(), dk_h.data_ptr(), dv_h.data_ptr(),
                     B, Sq, Skv, Hq, Hk, D, scale, causal, force_v1, cur_stream());
    return {dq, dk_h, dv_h};
}

std::vector<torch::Tensor> flash_attn_bwd(torch::Tensor dout, torch::Tensor q,
                                          torch::Tensor k, torch::Tensor v,
                                          torch::Tensor o, torch::Tensor lse,
                                          bool causal) {
    return flash_attn_bwd_ex(dout, q, k, v, o, lse, causal, /*force_v1=*/false);
}

// delta[b,h,q] = rowsum(dO * O): the backward's preprocess on its own (every
// head dim the backward takes), for tests and tools/bench_layer_ops.py.
torch::Tensor flash_bwd_delta(torch::Tensor dout, torch::Tensor o) {
    CHECK_GPU(dout); CHECK_CONTIG(dout); CHECK_BF16(dout);
    CHECK_GPU(o); CHECK_CONTIG(o); CHECK_BF16(o);
    TORCH_CHECK(dout.dim() == 4 && dout.sizes() == o.sizes(), "dout, o must be [B,S,H,D]");
    int B = o.size(0), Sq = o.size(1), Hq = o.size(2), D = o.size(3);
    auto delta = torch::empty({B, Hq, Sq}, o.options().dtype(torch::kFloat32));
    launch_flash_bwd_delta(dout.data_ptr(), o.data_ptr(), delta.data_ptr<float>(),
                           B, Sq, Hq, D, cur_stream());
    return delta;
}

// The v2 backward with only some of its launches (FLASH_BWD_* mask: 1 delta,
// 2 dq, 4 dkv), so tools/bench_fa.py can time dq and dkv on their own.
// Outputs of launches left out are uninitialised.
std::vector<torch::Tensor> flash_attn_bwd2_parts(torch::Tensor dout, torch::Tensor q,
                                                 torch::Tensor k, torch::Tensor v,
                                                 torch::Tensor o, torch::Tensor lse,
                                                 torch::Tensor delta, bool causal,
                                                 int64_t parts) {
    check_attn_args(q, k, v, &dout, &o, &lse);
    TORCH_CHECK(delta.is_cuda() && delta.is_contiguous() &&
                    delta.scalar_type() == torch::kFloat32 &&
                    delta.sizes() == lse.sizes(),
                "delta must be a contiguous fp32 GPU tensor shaped like lse");
    int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
    int Skv = k.size(1), Hk = k.size(2);
    auto dq = torch::empty_like(q);
    auto dk_h = torch::empty({B, Skv, Hk, D}, k.options());
    auto dv_h = torch::empty({B, Skv, Hk, D}, v.options());
    float scale = 1.0f / std::sqrt((float)D);
    TORCH_CHECK(launch_flash_bwd2(dout.data_ptr(), q.data_ptr(), k.data_ptr(),
                                  v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(),
                                  delta.data_ptr<float>(), dq.data_ptr(),
                                  dk_h.data_ptr(), dv_h.data_ptr(), B, Sq, Skv, Hq,
                                  Hk, D, scale, causal, cur_stream(), (int)parts),
                "flash_attn_bwd2_parts: no v2 kernel for this shape");
    return {dq, dk_h, dv_h};
}

// ---------------------------------------------------------------------------
// Packed attention: q, k, v are read in place from the fused projection's
// output qkv [B, S, (Hq + 2*Hk)*D] (per token: Hq q heads, Hk k heads, Hk v
// heads) and the backward writes dq, dk, dv straight into one dqkv of the
// same layout.  Only the v2 kernels take row strides, so these entry points
// exist for the shapes v2 takes (D = 128); anything else is an error and
// the caller keeps the split + contiguous path.
// ---------------------------------------------------------------------------
struct PackedDims { int B, S, Hq, Hk, D; int64_t k_off, v_off; };

static PackedDims check_packed(const torch::Tensor& qkv, int64_t Hq, int64_t Hk,
                               const torch::Tensor* startend) {
    TORCH_CHECK(qkv.is_cuda(), "qkv must be on GPU");
    TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16, "qkv must be bf16");
    TORCH_CHECK(qkv.is_contiguous(), "qkv must be contiguous");
    TORCH_CHECK(qkv.dim() == 3, "qkv must be [B, S, (Hq+2*Hk)*D]");
    TORCH_CHECK(Hq > 0 && Hk > 0 && Hq % Hk == 0, "GQA requires Hq % Hk == 0");
    TORCH_CHECK(qkv.size(2) % (Hq + 2 * Hk) == 0, "last dim must be (Hq + 2*Hk) * D");
    PackedDims d;
    d.B = qkv.size(0); d.S = qkv.size(1); d.Hq = (int)Hq; d.Hk = (int)Hk;
    d.D = (int)(qkv.size(2) / (Hq + 2 * Hk));
    TORCH_CHECK(d.D == 128, "packed attention needs head dim 128 (the v2 kernels), got ", d.D);
    TORCH_CHECK(qkv.size(2) < (1LL << 31), "packed row too long");
    // the dkv kernel's LDS-DMA and every 16-byte load need 16-byte aligned
    // sources: base pointer, row stride and slice offsets (multiples of
    // D * 2 = 256 bytes)
    TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
                "qkv must be 16-byte aligned");
    d.k_off = Hq * d.D;
    d.v_off = (Hq + Hk) * d.D;
    if (startend) {
        TORCH_CHECK(startend->is_cuda(), "startend must be on GPU");
        TORCH_CHECK(startend->numel() == (int64_t)d.B * d.S, "startend must be [B, S]");
    }
    return d;
}

static void check_packed_bwd(const PackedDims& d, const torch::Tensor& dout,
                             const torch::Tensor& o, const torch::Tensor& lse) {
    auto check_o = [&](const torch::Tensor& t, const char* name) {
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 && t.is_contiguous(),
                    name, " must be a contiguous bf16 GPU tensor");
        TORCH_CHECK(t.sizes() == at::IntArrayRef({d.B, d.S, d.Hq, d.D}),
                    name, " must be [B,S,Hq,D]");
    };
    check_o(dout, "dout");
    check_o(o, "o");
    TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                    lse.scalar_type() == torch::kFloat32 &&
                    lse.sizes() == at::IntArrayRef({d.B, d.Hq, d.S}),
                "lse must be a contiguous fp32 [B,Hq,S] GPU tensor");
}

static std::vector<torch::Tensor> packed_fwd(const torch::Tensor& qkv, int64_t Hq, int64_t Hk,
                                             bool causal, const torch::Tensor* startend) {
    PackedDims d = check_packed(qkv, Hq, Hk, startend);
    auto o = torch::empty({d.B, d.S, d.Hq, d.D}, qkv.options());
    auto lse = torch::empty({d.B, d.Hq, d.S}, qkv.options().dtype(torch::kFloat32));
    if (d.B == 0 || d.S == 0) return {o, lse};
    const auto* base = static_cast<const at::BFloat16*>(qkv.data_ptr());
    FlashStrides rs = flash_packed_strides(d.Hq, d.Hk, d.D);
    float scale = 1.0f / std::sqrt((float)d.D);
    bool ok;
    if (startend) {
        auto se = startend->to(torch::kInt32).contiguous();
        ok = launch_flash_fwd2_mask(base, base + d.k_off, base + d.v_off, o.data_ptr(),
                                    lse.data_ptr<float>(), se.data_ptr<int>(),
                                    d.B, d.S, d.S, d.Hq, d.Hk, d.D, scale, cur_stream(), &rs);
    } else {
        ok = launch_flash_fwd2(base, base + d.k_off, base + d.v_off, o.data_ptr(),
                               lse.data_ptr<float>(), d.B, d.S, d.S, d.Hq, d.Hk, d.D,
                               scale, causal, cur_stream(), &rs);
    }
    TORCH_CHECK(ok, "packed attention: no v2 kernel for this shape");
    return {o, lse};
}

static torch::Tensor packed_bwd(const torch::Tensor& dout, const torch::Tensor& qkv,
                                const torch::Tensor& o, const torch::Tensor& lse,
                                int64_t Hq, int64_t Hk, bool causal,
                                const torch::Tensor* startend) {
    PackedDims d = check_packed(qkv, Hq, Hk, startend);
    check_packed_bwd(d, dout, o, lse);
    auto dqkv = torch::empty_like(qkv);
    if (d.B == 0 || d.S == 0) return dqkv;
    TORCH_CHECK(reinterpret_cast<uintptr_t>(dout.data_ptr()) % 16 == 0,
                "dout must be 16-byte aligned");
    auto delta = torch::empty({d.B, d.Hq, d.S}, qkv.options().dtype(torch::kFloat32));
    const auto* base = static_cast<const at::BFloat16*>(qkv.data_ptr());
    auto* dbase = static_cast<at::BFloat16*>(dqkv.data_ptr());
    FlashStrides rs = flash_packed_strides(d.Hq, d.Hk, d.D);
    float scale = 1.0f / std::sqrt((float)d.D);
    bool ok;
    if (startend) {
        auto se = startend->to(torch::kInt32).contiguous();
        ok = launch_flash_bwd2_mask(dout.data_ptr(), base, base + d.k_off, base + d.v_off,
                                    o.data_ptr(), lse.data_ptr<float>(),
                                    delta.data_ptr<float>(), dbase, dbase + d.k_off,
                                    dbase + d.v_off, se.data_ptr<int>(),
                                    d.B, d.S, d.S, d.Hq, d.Hk, d.D, scale, cur_stream(), &rs);
    } else {
        ok = launch_flash_bwd2(dout.data_ptr(), base, base + d.k_off, base + d.v_off,
                               o.data_ptr(), lse.data_ptr<float>(), delta.data_ptr<float>(),
                               dbase, dbase + d.k_off, dbase + d.v_off,
                               d.B, d.S, d.S, d.Hq, d.Hk, d.D, scale, causal, cur_stream(),
                               FLASH_BWD_ALL, &rs);
    }
    TORCH_CHECK(ok, "packed attention: no v2 kernel for this shape");
    return dqkv;
}

std::vector<torch::Tensor> flash_attn_packed_fwd(torch::Tensor qkv, int64_t Hq, int64_t Hk,
                                                 bool causal) {
    return packed_fwd(qkv, Hq, Hk, causal, nullptr);
}

torch::Tensor flash_attn_packed_bwd(torch::Tensor dout, torch::Tensor qkv, torch::Tensor o,
                                    torch::Tensor lse, int64_t Hq, int64_t Hk, bool causal) {
    return packed_bwd(dout, qkv, o, lse, Hq, Hk, causal, nullptr);
}

std::vector<torch::Tensor> flashmask_attn_packed_fwd(torch::Tensor qkv, int64_t Hq, int64_t Hk,
                                                     torch::Tensor startend) {
    return packed_fwd(qkv, Hq, Hk, true, &startend);
}

torch::Tensor flashmask_attn_packed_bwd(torch::Tensor dout, torch::Tensor qkv, torch::Tensor o,
                                        torch::Tensor lse, int64_t Hq, int64_t Hk,
                                        torch::Tensor startend) {
    return packed_bwd(dout, qkv, o, lse, Hq, Hk, true, &startend);
}

// ---------------------------------------------------------------------------
void fused_adamw(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads,
                 std::vector<torch::Tensor> exp_avgs, std::vector<torch::Tensor> exp_avg_sqs,
                 std::vector<torch::Tensor> masters,
                 double lr, double beta1, double beta2, double eps, double wd,
                 int64_t step) {
    TORCH_CHECK(!params.empty());
    bool has_master = !masters.empty();
    TORCH_CHECK(grads.size() == params.size() && exp_avgs.size() == params.size() &&
                    exp_avg_sqs.size() == params.size() &&
                    (!has_master || masters.size() == params.size()),
                "params, grads, exp_avgs, exp_avg_sqs and masters must have the same length");
    const long long CHUNK = 1 << 22;  // 4M elements per chunk
    std::vector<AdamWChunk> chunks;
    // gradients converted to the param's dtype or layout; the chunk table
    // points into them, so they live until after the launch
    std::vector<torch::Tensor> held_grads;
    auto check_state = [](const torch::Tensor& t, const torch::Tensor& p, const char* what) {
        TORCH_CHECK(t.is_cuda() && t.device() == p.device() && t.is_contiguous() &&
                        t.scalar_type() == torch::kFloat32 && t.numel() == p.numel(),
                    what, " must be a contiguous fp32 GPU tensor of the param's numel");
    };
    for (size_t i = 0; i < params.size(); i++) {
        auto& p = params[i];
        CHECK_GPU(p); CHECK_CONTIG(p);
        bool is_bf16 = p.scalar_type() == torch::kBFloat16;
        TORCH_CHECK(is_bf16 || p.scalar_type() == torch::kFloat32,
                    "params must be bf16 or fp32");
        TORCH_CHECK(p.device() == params[0].device(), "params must be on one device");
        TORCH_CHECK(!is_bf16 || has_master, "bf16 params need master weights");
        long long n = p.numel();
        check_state(exp_avgs[i], p, "exp_avg");
        check_state(exp_avg_sqs[i], p, "exp_avg_sq");
        if (has_master && is_bf16) check_state(masters[i], p, "master");
        torch::Tensor g = grads[i];
        TORCH_CHECK(g.is_cuda() && g.device() == p.device() && g.numel() == n,
                    "grad must be a GPU tensor of the param's numel");
        if (g.scalar_type() != p.scalar_type() || !g.is_contiguous()) {
            g = g.to(p.scalar_type()).contiguous();
            held_grads.push_back(g);
        }
        for (long long off = 0; off < n; off += CHUNK) {
            AdamWChunk c;
            c.param = p.data_ptr();
            c.grad = g.data_ptr();
            c.m = exp_avgs[i].data_ptr<float>();
            c.v = exp_avg_sqs[i].data_ptr<float>();
            c.master = is_bf16 ? masters[i].data_ptr<float>() : nullptr;
            c.offset = off;
            c.n = std::min(CHUNK, n - off);
            c.is_bf16 = is_bf16 ? 1 : 0;
            chunks.push_back(c);
        }
    }
    auto meta = torch::from_blob(chunks.data(), {(long long)(chunks.size() * sizeof(AdamWChunk))},
                                 torch::kUInt8).clone();
    auto dev_meta = meta.to(params[0].device(), /*non_blocking=*/true);
    float bias1 = 1.0f - std::pow((float)beta1, (float)step);
    float bias2 = 1.0f - std::pow((float)beta2, (float)step);
    launch_adamw(reinterpret_cast<const AdamWChunk*>(dev_meta.data_ptr()),
                 (int)chunks.size(), (float)lr, (float)beta1, (float)beta2,
                 (float)eps, (float)wd, bias1, bias2, cur_stream());
}

std::vector<torch::Tensor> flashmask_attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                              torch::Tensor startend) {
    check_attn_args(q, k, v, nullptr, nullptr, nullptr, &startend);
    int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
    int Skv = k.size(1), Hk = k.size(2);
    auto se = startend.to(torch::kInt32).contiguous();
    auto o = torch::empty_like(q);
    auto lse = torch::empty({B, Hq, Sq}, q.options().dtype(torch::kFloat32));
    float scale = 1.0f / std::sqrt((float)D);
    launch_flash_fwd_mask(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                          lse.data_ptr<float>(), se.data_ptr<int>(),
                          B, Sq, Skv, Hq, Hk, D, scale, cur_stream());
    return {o, lse};
}

std::vector<torch::Tensor> flashmask_attn_bwd(torch::Tensor dout, torch::Tensor q,
                                              torch::Tensor k, torch::Tensor v,
                                              torch::Tensor o, torch::Tensor lse,
                                              torch::Tensor startend) {
    check_attn_args(q, k, v, &dout, &o, &lse, &startend);
    int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
    int Skv = k.size(1), Hk = k.size(2);
    auto se = startend.to(torch::kInt32).contiguous();
    auto dq = torch::empty_like(q);
    auto dk_h = torch::empty({B, Skv, Hk, D}, k.options());
    auto dv_h = torch::empty({B, Skv, Hk, D}, v.options());
    auto delta = torch::empty({B, Hq, Sq}, q.options().dtype(torch::kFloat32));
    float scale = 1.0f / std::sqrt((float)D);
    launch_flash_bwd_mask(dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
                          o.data_ptr(), lse.data_ptr<float>(), delta.data_ptr<float>(),
                          dq.data_ptr(), dk_h.data_ptr(), dv_h.data_ptr(),
                          se.data_ptr<int>(), B, Sq, Skv, Hq, Hk, D, scale, cur_stream());
    return {dq, dk_h, dv_h};
}

// ---------------------------------------------------------------------------
// paged-KV inference ops
// ---------------------------------------------------------------------------
// 0 = bf16 cache, 1 = int8, 2 = int4 packed nibbles, from the cache dtype
static int kv_cache_mode(const torch::Tensor& k_cache,
                         const c10::optional<torch::Tensor>& k_scale,
                         const c10::optional<torch::Tensor>& v_scale) {
    int cache_mode = 0;
    if (k_cache.scalar_type() == torch::kChar) cache_mode = 1;
    else if (k_cache.scalar_type() == torch::kByte) cache_mode = 2;
    TORCH_CHECK(cache_mode == 0 || (k_scale.has_value() && v_scale.has_value()),
                "quantized KV cache needs k_scale/v_scale");
    return cache_mode;
}

torch::Tensor paged_decode_attn(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                                torch::Tensor block_table, torch::Tensor seq_lens,
                                c10::optional<torch::Tensor> k_scale,
                                c10::optional<torch::Tensor> v_scale) {
    CHECK_GPU(q); CHECK_CONTIG(q); CHECK_BF16(q);
    TORCH_CHECK(q.dim() == 3, "q must be [B, Hq, D] (single decode token)");
    int B = q.size(0), Hq = q.size(1), D = q.size(2);
    int block_size = k_cache.size(1), Hk = k_cache.size(2);
    int max_blocks = block_table.size(1);
    const int cache_mode = kv_cache_mode(k_cache, k_scale, v_scale);
    TORCH_CHECK(cache_mode != 2 || (D == 128 && Hq / Hk <= 16),
                "int4 KV cache requires head dim 128 and GQA group <= 16");
    auto out = torch::empty_like(q);
    float scale = 1.0f / std::sqrt((float)D);
    int G = Hq / Hk;
    int nsplit = paged_decode_nsplit(B, Hk);
    torch::Tensor partials;
    float* pptr = nullptr;
    if (nsplit > 1) {
        partials = torch::empty({(long)B, (long)Hk, (long)nsplit, (long)G * (2 + D)},
                                q.options().dtype(torch::kFloat32));
        pptr = partials.data_ptr<float>();
    }
    launch_paged_decode_attn(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                             cache_mode ? k_scale->data_ptr<float>() : nullptr,
                             cache_mode ? v_scale->data_ptr<float>() : nullptr,
                             block_table.data_ptr<int>(), seq_lens.data_ptr<int>(),
                             out.data_ptr(), pptr, nsplit, B, Hq, Hk, D, block_size,
                             max_blocks, scale, cache_mode, cur_stream());
    return out;
}

// T new tokens per sequence over the cache that already holds them
// (rope_cache_append first).  r_tiles forces the kernel's row tiles per
// workgroup (tools/bench_append.py); 0 lets the launcher choose.
torch::Tensor paged_append_attn(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                                torch::Tensor block_table, torch::Tensor seq_lens_before,
                                c10::optional<torch::Tensor> token_counts,
                                c10::optional<torch::Tensor> k_scale,
                                c10::optional<torch::Tensor> v_scale,
                                int64_t r_tiles) {
    CHECK_GPU(q); CHECK_CONTIG(q); CHECK_BF16(q);
    TORCH_CHECK(q.dim() == 4, "q must be [B, T, Hq, D]");
    int B = q.size(0), T = q.size(1), Hq = q.size(2), D = q.size(3);
    int block_size = k_cache.size(1), Hk = k_cache.size(2);
    int max_blocks = block_table.size(1);
    const int cache_mode = kv_cache_mode(k_cache, k_scale, v_scale);
    TORCH_CHECK(block_table.size(0) == B && seq_lens_before.numel() == B,
                "block_table / seq_lens_before must have one row per sequence");
    TORCH_CHECK(!token_counts.has_value() || token_counts->numel() == B,
                "token_counts must be [B]");
    // zeros: rows at or past token_counts[b] are not written by the kernel
    auto out = torch::zeros_like(q);
    if (B == 0 || T == 0) return out;
    int R = 0, nrg = 0, nsplit = 0;
    TORCH_CHECK(paged_append_plan(B, T, Hq, Hk, D, (int)r_tiles, &R, &nrg, &nsplit),
                "paged_append_attn: no kernel for head dim D=", D, " with GQA group G=",
                Hk > 0 ? Hq / Hk : 0, " (needs D == 128, G <= 16, Hq % Hk == 0)");
    float scale = 1.0f / std::sqrt((float)D);
    torch::Tensor partials;
    float* pptr = nullptr;
    if (nsplit > 1) {
        partials = torch::empty({(long)B * Hk * nrg, (long)nsplit, (long)16 * R, (long)(2 + D)},
                                q.options().dtype(torch::kFloat32));
        pptr = partials.data_ptr<float>();
    }
    bool ok = launch_paged_append_attn(
        q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
        cache_mode ? k_scale->data_ptr<float>() : nullptr,
        cache_mode ? v_scale->data_ptr<float>() : nullptr,
        block_table.data_ptr<int>(), seq_lens_before.data_ptr<int>(),
        token_counts.has_value() ? token_counts->data_ptr<int>() : nullptr,
        out.data_ptr(), pptr, (int)r_tiles, B, T, Hq, Hk, D, block_size, max_blocks,
        scale, cache_mode, cur_stream());
    TORCH_CHECK(ok, "paged_append_attn: kernel refused D=", D, " G=", Hq / Hk);
    return out;
}

torch::Tensor rope_cache_append(torch::Tensor qkv, torch::Tensor k_cache, torch::Tensor v_cache,
                                torch::Tensor block_table, torch::Tensor seq_lens_before,
                                torch::Tensor cos_t, torch::Tensor sin_t,
                                int64_t Hq, int64_t Hk,
                                c10::optional<torch::Tensor> token_counts,
                                c10::optional<torch::Tensor> k_scale,
                                c10::optional<torch::Tensor> v_scale) {
    CHECK_GPU(qkv); CHECK_CONTIG(qkv); CHECK_BF16(qkv);
    TORCH_CHECK(qkv.dim() == 3, "qkv must be [B, T, (Hq+2Hk)*D]");
    int B = qkv.size(0), T = qkv.size(1);
    const int cache_mode = kv_cache_mode(k_cache, k_scale, v_scale);
    int D = (int)k_cache.size(3) * (cache_mode == 2 ? 2 : 1);
    int block_size = k_cache.size(1);
    int max_blocks = block_table.size(1);
    // zeros (not empty): tokens beyond token_counts[b] are skipped by the
    // kernel and must compare deterministically
    auto q_out = torch::zeros({B, T, Hq, (long)D}, qkv.options());
    auto cf = cos_t.to(torch::kFloat32).contiguous();
    auto sf = sin_t.to(torch::kFloat32).contiguous();
    const int* tc = nullptr;
    if (token_counts.has_value()) tc = token_counts->data_ptr<int>();
    TORCH_CHECK(cache_mode != 2 || D == 128, "int4 KV cache requires head dim 128");
    launch_rope_cache_append(qkv.data_ptr(), q_out.data_ptr(),
                             k_cache.data_ptr(), v_cache.data_ptr(),
                             cache_mode ? k_scale->data_ptr<float>() : nullptr,
                             cache_mode ? v_scale->data_ptr<float>() : nullptr,
                             block_table.data_ptr<int>(), seq_lens_before.data_ptr<int>(),
                             cf.data_ptr<float>(), sf.data_ptr<float>(),
                             B, T, (int)Hq, (int)Hk, D, block_size, max_blocks, tc,
                             cache_mode, cur_stream());
    return q_out;
}

torch::Tensor skinny_gemm(torch::Tensor x, torch::Tensor w, int64_t ksplit) {
    CHECK_GPU(x); CHECK_BF16(x); CHECK_BF16(w);
    auto x2 = x.contiguous().view({-1, x.size(-1)});
    int M = x2.size(0), K = x2.size(1), N = w.size(0);
    TORCH_CHECK(M <= 64, "skinny_gemm is for decode batches (M <= 64)");
    TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8");
    int ks = skinny_gemm_ksplit(N, K, (int)ksplit);
    auto partial = torch::empty({(long)ks, (long)M, (long)N},
                                x.options().dtype(torch::kFloat32));
    auto sizes = x.sizes().vec();
    sizes.back() = N;
    auto y = torch::empty(sizes, x.options());
    launch_skinny_gemm(x2.data_ptr(), w.contiguous().data_ptr(),
                       partial.data_ptr<float>(), y.data_ptr(),
                       M, N, K, (int)ksplit, cur_stream());
    return y;
}

std::vector<torch::Tensor> fp8_rowwise_quant(torch::Tensor x) {
    CHECK_GPU(x); CHECK_BF16(x);
    auto x2 = x.contiguous().view({-1, x.size(-1)});
    long long R = x2.size(0);
    int K = x2.size(1);
    TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8");
    auto y = torch::empty({R, (long)K}, x.options().dtype(torch::kFloat8_e4m3fn));
    auto scales = torch::empty({R}, x.options().dtype(torch::kFloat32));
    launch_fp8_rowwise_quant(x2.data_ptr(), y.data_ptr(), scales.data_ptr<float>(),
                             R, K, cur_stream());
    return {y, scales};
}

torch::Tensor wint8_gemv(torch::Tensor x, torch::Tensor wq, torch::Tensor scale) {
    CHECK_GPU(x); CHECK_BF16(x);
    auto x2 = x.contiguous().view({-1, x.size(-1)});
    int M = x2.size(0), K = x2.size(1), N = wq.size(0);
    TORCH_CHECK(M <= 16, "wint8_gemv is for decode shapes (M <= 16)");
    TORCH_CHECK(K % 128 == 0, "K must be a multiple of 128");
    auto sizes = x.sizes().vec();
    sizes.back() = N;
    auto y = torch::empty(sizes, x.options());
    launch_wint8_gemv(x2.data_ptr(), wq.data_ptr(), scale.data_ptr<float>(),
                      y.data_ptr(), M, N, K, cur_stream());
    return y;
}

// ---- moe_ffn.hip ----
static void check_moe_route_args(const torch::Tensor& logits, int64_t top_k) {
    CHECK_GPU(logits); CHECK_CONTIG(logits);
    TORCH_CHECK(logits.dim() == 2, "router logits must be [T, E]");
    TORCH_CHECK(logits.scalar_type() == torch::kFloat32 ||
                logits.scalar_type() == torch::kBFloat16,
                "router logits must be fp32 or bf16");
    TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) <= kMoeMaxExperts,
                "moe: at most ", kMoeMaxExperts, " experts");
    TORCH_CHECK(top_k >= 1 && top_k <= kMoeMaxTopK && top_k <= logits.size(1),
                "moe: top_k must be in 1..min(E, ", kMoeMaxTopK, ")");
}

std::vector<torch::Tensor> moe_route(torch::Tensor logits, int64_t top_k) {
    check_moe_route_args(logits, top_k);
    const int T = logits.size(0), E = logits.size(1), K = (int)top_k;
    auto ids = torch::empty({(long)T, (long)K}, logits.options().dtype(torch::kInt32));
    auto w = torch::empty({(long)T, (long)K}, logits.options().dtype(torch::kFloat32));
    launch_moe_route(logits.data_ptr(), logits.scalar_type() == torch::kBFloat16,
                     ids.data_ptr<int>(), w.data_ptr<float>(), T, E, K, cur_stream());
    return {ids, w};
}

// topk_ids [T, K] int32 -> sorted_rows [P], tile_expert [P / 32], row_pos
// [T, K], num_tiles [1]
std::vector<torch::Tensor> moe_align(torch::Tensor topk_ids, int64_t num_experts) {
    CHECK_GPU(topk_ids); CHECK_CONTIG(topk_ids);
    TORCH_CHECK(topk_ids.dim() == 2 && topk_ids.scalar_type() == torch::kInt32,
                "topk_ids must be [T, K] int32");
    const int T = topk_ids.size(0), K = topk_ids.size(1), E = (int)num_experts;
    TORCH_CHECK(E >= 1 && E <= kMoeMaxExperts, "moe: at most ", kMoeMaxExperts, " experts");
    TORCH_CHECK((long)T * K <= kMoeMaxFlatRows, "moe: T * top_k must be <= ",
                kMoeMaxFlatRows);
    const long P = moe_padded_rows(T, K, E);
    auto opt = topk_ids.options();
    auto sorted_rows = torch::empty({P}, opt);
    auto tile_expert = torch::empty({P / kMoeRowTile}, opt);
    auto row_pos = torch::empty({(long)T, (long)K}, opt);
    auto num_tiles = torch::empty({1}, opt);
    launch_moe_align(topk_ids.data_ptr<int>(), sorted_rows.data_ptr<int>(),
                     tile_expert.data_ptr<int>(), row_pos.data_ptr<int>(),
                     num_tiles.data_ptr<int>(), T, K, E, cur_stream());
    return {sorted_rows, tile_expert, row_pos, num_tiles};
}

static bool aligned16(const torch::Tensor& t) {
    return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

torch::Tensor moe_ffn(torch::Tensor x, torch::Tensor router_logits, torch::Tensor w1,
                      torch::Tensor w3, torch::Tensor w2, int64_t top_k) {
    CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
    CHECK_GPU(w1); CHECK_CONTIG(w1); CHECK_BF16(w1);
    CHECK_GPU(w3); CHECK_CONTIG(w3); CHECK_BF16(w3);
    CHECK_GPU(w2); CHECK_CONTIG(w2); CHECK_BF16(w2);
    check_moe_route_args(router_logits, top_k);
    TORCH_CHECK(x.dim() == 2 && w1.dim() == 3 && w3.dim() == 3 && w2.dim() == 3,
                "moe_ffn: x [T, H], w1/w3 [E, H, I], w2 [E, I, H]");
    const int T = x.size(0), H = x.size(1);
    const int E = w1.size(0), I = w1.size(2), K = (int)top_k;
    TORCH_CHECK(router_logits.size(0) == T && router_logits.size(1) == E,
                "moe_ffn: router logits must be [T, E]");
    TORCH_CHECK(w1.size(1) == H && w3.sizes() == w1.sizes() && w2.size(0) == E &&
                w2.size(1) == I && w2.size(2) == H,
                "moe_ffn: w1/w3 [E, H, I], w2 [E, I, H]");
    TORCH_CHECK(H % 128 == 0 && I % 128 == 0,
                "moe_ffn: H and I must be multiples of 128");
    TORCH_CHECK((long)T * K <= kMoeMaxFlatRows, "moe_ffn: T * top_k must be <= ",
                kMoeMaxFlatRows);
    // LDS-DMA sources: 16-byte aligned bases (rows are multiples of 256 bytes)
    TORCH_CHECK(aligned16(x) && aligned16(w1) && aligned16(w3) && aligned16(w2),
                "moe_ffn: x and the weights must be 16-byte aligned");
    auto out = torch::empty({(long)T, (long)H}, x.options());
    if (T == 0) return out;

    auto stream = cur_stream();
    auto i32 = x.options().dtype(torch::kInt32);
    auto f32 = x.options().dtype(torch::kFloat32);
    const long P = moe_padded_rows(T, K, E);
    const int ks = moe_down_ksplit(T, K, H, I);
    auto ids = torch::empty({(long)T, (long)K}, i32);
    auto topw = torch::empty({(long)T, (long)K}, f32);
    auto sorted_rows = torch::empty({P}, i32);
    auto tile_expert = torch::empty({P / kMoeRowTile}, i32);
    auto row_pos = torch::empty({(long)T, (long)K}, i32);
    auto num_tiles = torch::empty({1}, i32);
    auto zero_row = torch::zeros({(long)H}, x.options());
    auto act = torch::empty({P, (long)I}, x.options());
    auto partial = torch::empty({(long)ks, P, (long)H}, f32);

    launch_moe_route(router_logits.data_ptr(),
                     router_logits.scalar_type() == torch::kBFloat16,
                     ids.data_ptr<int>(), topw.data_ptr<float>(), T, E, K, stream);
    launch_moe_align(ids.data_ptr<int>(), sorted_rows.data_ptr<int>(),
                     tile_expert.data_ptr<int>(), row_pos.data_ptr<int>(),
                     num_tiles.data_ptr<int>(), T, K, E, stream);
    launch_moe_gate_up(x.data_ptr(), zero_row.data_ptr(), w1.data_ptr(), w3.data_ptr(),
                       sorted_rows.data_ptr<int>(), tile_expert.data_ptr<int>(),
                       num_tiles.data_ptr<int>(), act.data_ptr(), T, K, E, H, I, stream);
    launch_moe_down(act.data_ptr(), w2.data_ptr(), tile_expert.data_ptr<int>(),
                    num_tiles.data_ptr<int>(), partial.data_ptr<float>(), ks,
                    T, K, E, H, I, stream);
    launch_moe_combine(partial.data_ptr<float>(), row_pos.data_ptr<int>(),
                       topw.data_ptr<float>(), out.data_ptr(), ks, T, K, E, H, stream);
    return out;
}

// Weight-only int8 experts: q1/q3 [E, I, H], q2 [E, H, I] int8 with the
// contraction dimension contiguous, s1/s3 [E, I], s2 [E, H] fp32.
torch::Tensor moe_ffn_wint8(torch::Tensor x, torch::Tensor router_logits,
                            torch::Tensor q1, torch::Tensor s1, torch::Tensor q3,
                            torch::Tensor s3, torch::Tensor q2, torch::Tensor s2,
                            int64_t top_k) {
    CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
    CHECK_GPU(q1); CHECK_CONTIG(q1); CHECK_GPU(s1); CHECK_CONTIG(s1);
    CHECK_GPU(q3); CHECK_CONTIG(q3); CHECK_GPU(s3); CHECK_CONTIG(s3);
    CHECK_GPU(q2); CHECK_CONTIG(q2); CHECK_GPU(s2); CHECK_CONTIG(s2);
    TORCH_CHECK(q1.scalar_type() == torch::kInt8 && q3.scalar_type() == torch::kInt8 &&
                q2.scalar_type() == torch::kInt8, "moe_ffn_wint8: q1/q3/q2 must be int8");
    TORCH_CHECK(s1.scalar_type() == torch::kFloat32 && s3.scalar_type() == torch::kFloat32 &&
                s2.scalar_type() == torch::kFloat32, "moe_ffn_wint8: s1/s3/s2 must be fp32");
    check_moe_route_args(router_logits, top_k);
    TORCH_CHECK(x.dim() == 2 && q1.dim() == 3 && q3.dim() == 3 && q2.dim() == 3 &&
                s1.dim() == 2 && s3.dim() == 2 && s2.dim() == 2,
                "moe_ffn_wint8: x [T, H], q1/q3 [E, I, H], q2 [E, H, I], "
                "s1/s3 [E, I], s2 [E, H]");
    const int T = x.size(0), H = x.size(1);
    const int E = q1.size(0), I = q1.size(1), K = (int)top_k;
    TORCH_CHECK(router_logits.size(0) == T && router_logits.size(1) == E,
                "moe_ffn_wint8: router logits must be [T, E]");
    TORCH_CHECK(q1.size(2) == H && q3.sizes() == q1.sizes() && q2.size(0) == E &&
                q2.size(1) == H && q2.size(2) == I,
                "moe_ffn_wint8: q1/q3 [E, I, H], q2 [E, H, I]");
    TORCH_CHECK(s1.size(0) == E && s1.size(1) == I && s3.sizes() == s1.sizes() &&
                s2.size(0) == E && s2.size(1) == H,
                "moe_ffn_wint8: s1/s3 [E, I], s2 [E, H]");
    TORCH_CHECK(H % 128 == 0 && I % 128 == 0,
                "moe_ffn_wint8: H and I must be multiples of 128");
    TORCH_CHECK((long)T * K <= kMoeMaxFlatRows, "moe_ffn_wint8: T * top_k must be <= ",
                kMoeMaxFlatRows);
    // LDS-DMA sources: 16-byte aligned bases (rows are multiples of 128 bytes)
    TORCH_CHECK(aligned16(x) && aligned16(q1) && aligned16(q3) && aligned16(q2),
                "moe_ffn_wint8: x and the weights must be 16-byte aligned");
    auto out = torch::empty({(long)T, (long)H}, x.options());
    if (T == 0) return out;

    auto stream = cur_stream();
    auto i32 = x.options().dtype(torch::kInt32);
    auto f32 = x.options().dtype(torch::kFloat32);
    const long P = moe_padded_rows(T, K, E);
    const int ks = moe_down_ksplit_wint8(T, K, H, I);
    auto ids = torch::empty({(long)T, (long)K}, i32);
    auto topw = torch::empty({(long)T, (long)K}, f32);
    auto sorted_rows = torch::empty({P}, i32);
    auto tile_expert = torch::empty({P / kMoeRowTile}, i32);
    auto row_pos = torch::empty({(long)T, (long)K}, i32);
    auto num_tiles = torch::empty({1}, i32);
    auto zero_row = torch::zeros({(long)H}, x.options());
    auto act = torch::empty({P, (long)I}, x.options());
    auto partial = torch::empty({(long)ks, P, (long)H}, f32);

    launch_moe_route(router_logits.data_ptr(),
                     router_logits.scalar_type() == torch::kBFloat16,
                     ids.data_ptr<int>(), topw.data_ptr<float>(), T, E, K, stream);
    launch_moe_align(ids.data_ptr<int>(), sorted_rows.data_ptr<int>(),
                     tile_expert.data_ptr<int>(), row_pos.data_ptr<int>(),
                     num_tiles.data_ptr<int>(), T, K, E, stream);
    launch_moe_gate_up_wint8(x.data_ptr(), zero_row.data_ptr(), q1.data_ptr(),
                             s1.data_ptr<float>(), q3.data_ptr(), s3.data_ptr<float>(),
                             sorted_rows.data_ptr<int>(), tile_expert.data_ptr<int>(),
                             num_tiles.data_ptr<int>(), act.data_ptr(), T, K, E, H, I,
                             stream);
    launch_moe_down_wint8(act.data_ptr(), q2.data_ptr(), s2.data_ptr<float>(),
                          tile_expert.data_ptr<int>(), num_tiles.data_ptr<int>(),
                          partial.data_ptr<float>(), ks, T, K, E, H, I, stream);
    launch_moe_combine(partial.data_ptr<float>(), row_pos.data_ptr<int>(),
                       topw.data_ptr<float>(), out.data_ptr(), ks, T, K, E, H, stream);
    return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("rms_norm_fwd", &rms_norm_fwd);
    m.def("rms_norm_bwd", &rms_norm_bwd);
    m.def("add_rms_norm_fwd", &add_rms_norm_fwd);
    m.def("add_rms_norm_bwd", &add_rms_norm_bwd);
    m.def("rope_fwd", &rope_fwd);
    m.def("rope_packed_", &rope_packed_);
    m.def("flash_attn_packed_fwd", &flash_attn_packed_fwd);
    m.def("flash_attn_packed_bwd", &flash_attn_packed_bwd);
    m.def("flashmask_attn_packed_fwd", &flashmask_attn_packed_fwd);
    m.def("flashmask_attn_packed_bwd", &flashmask_attn_packed_bwd);
    m.def("swiglu_fwd", &swiglu_fwd);
    m.def("swiglu_bwd", &swiglu_bwd);
    m.def("cross_entropy_fwd", &cross_entropy_fwd);
    m.def("cross_entropy_bwd", &cross_entropy_bwd);
    m.def("mfma_probe", &mfma_probe);
    m.def("mfma32_probe", &mfma32_probe);
    m.def("permlane_probe", &permlane_probe);
    m.def("lds_image_probe", &lds_image_probe);
    m.def("flash_attn_bwd2_parts", &flash_attn_bwd2_parts);
    m.def("flash_bwd_delta", &flash_bwd_delta);
    m.def("apply_repetition_penalty", &apply_repetition_penalty);
    m.def("topp_sample", &topp_sample,
          py::arg("logits"), py::arg("temperature"), py::arg("top_p"),
          py::arg("uniform"), py::arg("ban_eos") = py::none(),
          py::arg("cur_lens") = py::none(), py::arg("min_lens") = py::none());
    m.def("decode_update", &decode_update,
          py::arg("tokens"), py::arg("stop_flags"), py::arg("active"),
          py::arg("pre_ids"), py::arg("pre_lens"), py::arg("seq_lens"),
          py::arg("eos_ids"), py::arg("not_need_stop"),
          py::arg("max_new") = py::none(), py::arg("pad_id") = 0);
    m.def("block_step", &block_step);
    m.def("flash_attn_fwd", &flash_attn_fwd);
    m.def("flash_attn_fwd_ex", &flash_attn_fwd_ex);
    m.def("flash_attn_bwd", &flash_attn_bwd);
    m.def("flash_attn_bwd_ex", &flash_attn_bwd_ex);
    m.def("flashmask_attn_fwd", &flashmask_attn_fwd);
    m.def("flashmask_attn_bwd", &flashmask_attn_bwd);
    m.def("fused_adamw", &fused_adamw);
    m.def("paged_decode_attn", &paged_decode_attn,
          py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("block_table"), py::arg("seq_lens"),
          py::arg("k_scale") = c10::nullopt, py::arg("v_scale") = c10::nullopt);
    m.def("paged_append_attn", &paged_append_attn,
          py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("block_table"), py::arg("seq_lens_before"),
          py::arg("token_counts") = c10::nullopt,
          py::arg("k_scale") = c10::nullopt, py::arg("v_scale") = c10::nullopt,
          py::arg("r_tiles") = 0);
    m.def("rope_cache_append", &rope_cache_append,
          py::arg("qkv"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("block_table"), py::arg("seq_lens_before"),
          py::arg("cos_t"), py::arg("sin_t"), py::arg("Hq"), py::arg("Hk"),
          py::arg("token_counts") = c10::nullopt,
          py::arg("k_scale") = c10::nullopt, py::arg("v_scale") = c10::nullopt);
    m.def("wint8_gemv", &wint8_gemv);
    m.def("fp8_rowwise_quant", &fp8_rowwise_quant);
    m.def("skinny_gemm", &skinny_gemm, py::arg("x"), py::arg("w"),
          py::arg("ksplit") = 8);
    m.def("moe_route", &moe_route, py::arg("logits"), py::arg("top_k"));
    m.def("moe_align", &moe_align, py::arg("topk_ids"), py::arg("num_experts"));
    m.def("moe_ffn", &moe_ffn, py::arg("x"), py::arg("router_logits"),
          py::arg("w1"), py::arg("w3"), py::arg("w2"), py::arg("top_k"));
    m.def("moe_down_ksplit", &moe_down_ksplit);
    m.def("moe_ffn_wint8", &moe_ffn_wint8, py::arg("x"), py::arg("router_logits"),
          py::arg("q1"), py::arg("s1"), py::arg("q3"), py::arg("s3"),
          py::arg("q2"), py::arg("s2"), py::arg("top_k"));
    m.def("moe_down_ksplit_wint8", &moe_down_ksplit_wint8);
}
