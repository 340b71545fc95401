"""Dispatch layer for fused ops: HIP/CDNA4 kernels on GPU, torch reference on CPU.

Design rule (BASELINE.json north star): on a GPU box the hand-written gfx950
extension is MANDATORY — if a CUDA tensor reaches one of these ops and the
extension is missing, we raise instead of silently falling back to eager
PyTorch.  The CPU path uses ops.reference (plain fp32 torch) so plumbing
tests run without a GPU.
"""
from __future__ import annotations

from typing import Optional

import os

import torch

from . import reference

_C = None
_C_IMPORT_ERROR = None


def _load_extension():
    global _C, _C_IMPORT_ERROR
    if _C is not None:
        return _C
    try:
        from . import _C as ext  # built in-tree by setup.py build_ext --inplace
        _C = ext
    except ImportError as e:  # pragma: no cover - GPU-box only
        _C_IMPORT_ERROR = e
        raise RuntimeError(
            "paddlenlp_amd.ops._C (the gfx950 HIP extension) is not built. "
            "Run `python setup.py build_ext --inplace` (or __graft_entry__.build()). "
            f"Original error: {e}"
        ) from e
    return _C


def extension_available() -> bool:
    try:
        _load_extension()
        return True
    except RuntimeError:
        return False


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------
class _RMSNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        C = _load_extension()
        x = x.contiguous()
        y, invrms = C.rms_norm_fwd(x, weight, eps)
        ctx.save_for_backward(x, weight, invrms)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = _load_extension()
        x, weight, invrms = ctx.saved_tensors
        dx, dw = C.rms_norm_bwd(dy.contiguous(), x, weight, invrms)
        return dx, dw, None


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    # PNLP_DETERMINISTIC=1: the fused backward reduces dw with fp32 atomics
    # (run-to-run nondeterministic ordering); route through the pure-torch
    # path for bitwise-reproducible CI runs (reference determinism knobs
    # FLAGS_cudnn_deterministic / FLAGS_embedding_deterministic).
    if x.is_cuda and os.environ.get("PNLP_DETERMINISTIC", "0") != "1":
        return _RMSNormFunction.apply(x, weight, eps)
    return reference.rms_norm(x, weight, eps)


def layer_fusion_enabled() -> bool:
    """PNLP_LAYER_FUSION=0 selects the unfused layer composition (separate
    residual adds, split + contiguous q/k/v, out-of-place rope) for A/B runs.
    Default: the fused add+norm and the packed rope/attention path."""
    return os.environ.get("PNLP_LAYER_FUSION", "1") != "0"


class _AddRMSNormFunction(torch.autograd.Function):
    """h = residual + delta; y = rms_norm(h).  One kernel each way; both are
    bit-equal to the separate add and rms_norm."""

    @staticmethod
    def forward(ctx, residual, delta, weight, eps):
        C = _load_extension()
        h, y, invrms = C.add_rms_norm_fwd(residual.contiguous(), delta.contiguous(), weight, eps)
        ctx.save_for_backward(h, weight, invrms)
        ctx.set_materialize_grads(False)
        return h, y

    @staticmethod
    def backward(ctx, dh, dy):
        C = _load_extension()
        h, weight, invrms = ctx.saved_tensors
        if dy is None:
            return dh, dh, None, None
        if dh is None:  # h has no other consumer (the final norm)
            dx, dw = C.rms_norm_bwd(dy.contiguous(), h, weight, invrms)
        else:
            dx, dw = C.add_rms_norm_bwd(dy.contiguous(), dh.contiguous(), h, weight, invrms)
        return dx, dx, dw, None


def add_rms_norm(residual: torch.Tensor, delta: torch.Tensor, weight: torch.Tensor,
                 eps: float = 1e-6):
    """Returns (h, y) with h = residual + delta and y = rms_norm(h)."""
    if (residual.is_cuda and residual.dtype == torch.bfloat16
            and delta.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and residual.shape == delta.shape and residual.shape[-1] % 8 == 0
            and os.environ.get("PNLP_DETERMINISTIC", "0") != "1"):
        return _AddRMSNormFunction.apply(residual, delta, weight, eps)
    h = residual + delta
    return h, rms_norm(h, weight, eps)


# ---------------------------------------------------------------------------
# Rotary position embedding (fused, Llama rotate-half convention)
# ---------------------------------------------------------------------------
class _RopeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin):
        C = _load_extension()
        q_out, k_out = C.rope_fwd(q.contiguous(), k.contiguous(), cos, sin, False)
        ctx.save_for_backward(cos, sin)
        return q_out, k_out

    @staticmethod
    def backward(ctx, dq, dk):
        C = _load_extension()
        cos, sin = ctx.saved_tensors
        # rotation is orthogonal: bwd = rotate by -theta
        dq_in, dk_in = C.rope_fwd(dq.contiguous(), dk.contiguous(), cos, sin, True)
        return dq_in, dk_in, None, None


def fused_rope(q, k, cos, sin):
    """q: [B,S,Hq,D], k: [B,S,Hk,D], cos/sin: [S,D]."""
    if q.is_cuda:
        return _RopeFunction.apply(q, k, cos, sin)
    return reference.apply_rope(q, k, cos, sin)


build_rope_cache = reference.build_rope_cache


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------
class _SwiGLUFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        C = _load_extension()
        x = x.contiguous()
        y = C.swiglu_fwd(x)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = _load_extension()
        (x,) = ctx.saved_tensors
        return C.swiglu_bwd(dy.contiguous(), x)


def swiglu(x: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """silu(gate) * up.  x = cat([gate, up], -1) when y is None."""
    if y is not None:
        x = torch.cat([x, y], dim=-1)
    if x.is_cuda:
        return _SwiGLUFunction.apply(x)
    return reference.swiglu(x)


# ---------------------------------------------------------------------------
# FlashAttention (CDNA4 MFMA kernel; [B,S,H,D] layout, GQA native)
# ---------------------------------------------------------------------------
class _FlashAttnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal):
        C = _load_extension()
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        o, lse = C.flash_attn_fwd(q, k, v, causal)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal = causal
        return o

    @staticmethod
    def backward(ctx, do):
        C = _load_extension()
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = C.flash_attn_bwd(do.contiguous(), q, k, v, o, lse, ctx.causal)
        return dq, dk, dv, None


class _FlashMaskFunction(torch.autograd.Function):
    """FlashMask sparse-causal attention (reference flashmask_attention,
    llama/fusion_ops.py:218-238): key j visible to queries j <= i < start[j]."""

    @staticmethod
    def forward(ctx, q, k, v, startend):
        C = _load_extension()
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        o, lse = C.flashmask_attn_fwd(q, k, v, startend)
        ctx.save_for_backward(q, k, v, o, lse, startend)
        return o

    @staticmethod
    def backward(ctx, do):
        C = _load_extension()
        q, k, v, o, lse, startend = ctx.saved_tensors
        dq, dk, dv = C.flashmask_attn_bwd(do.contiguous(), q, k, v, o, lse, startend)
        return dq, dk, dv, None


def flash_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    causal: bool = True,
    attn_mask: Optional[torch.Tensor] = None,
    startend_row_indices: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """q: [B,S,Hq,D]; k,v: [B,S,Hk,D].  Returns [B,S,Hq,D]."""
    if q.is_cuda and attn_mask is None:
        if startend_row_indices is None:
            return _FlashAttnFunction.apply(q, k, v, causal)
        if causal:
            # [B, h(=1), Skv, 1] -> [B, Skv] (per-head masks pending)
            se = startend_row_indices
            if se.dim() == 4:
                assert se.shape[1] == 1, "per-kv-head FlashMask pending"
                se = se[:, 0, :, 0]
            return _FlashMaskFunction.apply(q, k, v, se.contiguous())
    return reference.flash_attention(
        q, k, v, causal=causal, attn_mask=attn_mask,
        startend_row_indices=startend_row_indices,
    )


class _PackedRopeAttnFunction(torch.autograd.Function):
    """Rope + causal attention on the fused QKV projection's output
    [B, S, (Hq + 2*Hk)*D], with no layout copies: rope rotates the q and k
    heads in place, the v2 attention kernels read q/k/v through row strides,
    and the backward writes dq/dk/dv into one packed dqkv that the rope
    backward then rotates in place."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, Hq, Hk, startend):
        C = _load_extension()
        C.rope_packed_(qkv, cos, sin, Hq, Hk, False)
        ctx.mark_dirty(qkv)
        if startend is None:
            o, lse = C.flash_attn_packed_fwd(qkv, Hq, Hk, True)
        else:
            o, lse = C.flashmask_attn_packed_fwd(qkv, Hq, Hk, startend)
        ctx.save_for_backward(qkv, o, lse, cos, sin, startend)
        ctx.heads = (Hq, Hk)
        ctx.set_materialize_grads(False)
        return qkv, o

    @staticmethod
    def backward(ctx, dqkv_rot, do):
        C = _load_extension()
        qkv, o, lse, cos, sin, startend = ctx.saved_tensors
        Hq, Hk = ctx.heads
        if do is None:
            dqkv = torch.zeros_like(qkv) if dqkv_rot is None else dqkv_rot.clone()
        else:
            if startend is None:
                dqkv = C.flash_attn_packed_bwd(do.contiguous(), qkv, o, lse, Hq, Hk, True)
            else:
                dqkv = C.flashmask_attn_packed_bwd(do.contiguous(), qkv, o, lse, Hq, Hk,
                                                   startend)
            if dqkv_rot is not None:  # the rotated qkv has another consumer
                dqkv += dqkv_rot
        C.rope_packed_(dqkv, cos, sin, Hq, Hk, True)
        return dqkv, None, None, None, None, None


def packed_rope_attention_supported(qkv: torch.Tensor, num_heads: int, num_kv_heads: int,
                                    startend_row_indices=None) -> bool:
    """True where the packed path has kernels: a contiguous bf16 GPU tensor
    that owns its memory, head dim 128 (the v2 attention kernels)."""
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3):
        return False
    # rope runs in place: not on a view of other data, not on a parameter
    if not qkv.is_contiguous() or qkv._is_view() or (qkv.is_leaf and qkv.requires_grad):
        return False
    if num_kv_heads <= 0 or num_heads % num_kv_heads:
        return False
    if qkv.shape[-1] != (num_heads + 2 * num_kv_heads) * 128:
        return False
    if startend_row_indices is not None:
        if os.environ.get("PNLP_FLASHMASK_KERNEL", "0") == "1":  # v1 FlashMask forced
            return False
        if startend_row_indices.dim() == 4 and startend_row_indices.shape[1] != 1:
            return False
    return True


def packed_rope_attention(qkv, cos, sin, num_heads: int, num_kv_heads: int,
                          startend_row_indices=None) -> torch.Tensor:
    """Causal (optionally FlashMask) attention with rope on packed qkv
    [B, S, (Hq + 2*Hk)*D]; cos/sin: [S, D].  Rotates qkv IN PLACE and returns
    the attention output [B, S, Hq, D].  Call only where
    packed_rope_attention_supported() holds."""
    se = startend_row_indices
    if se is not None:
        if se.dim() == 4:
            se = se[:, 0, :, 0]
        se = se.contiguous()
    _, o = _PackedRopeAttnFunction.apply(qkv, cos, sin, num_heads, num_kv_heads, se)
    return o


# ---------------------------------------------------------------------------
# Fused cross-entropy (chunked; avoids materializing fp32 [N, V] twice)
# ---------------------------------------------------------------------------
class _CrossEntropyFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        C = _load_extension()
        # the backward reads the saved logits with a row stride of V, so it
        # gets the contiguous tensor the forward ran on, not the caller's view
        logits = logits.contiguous()
        loss, lse = C.cross_entropy_fwd(logits, labels, ignore_index)
        ctx.save_for_backward(logits, labels, lse)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, dloss):
        C = _load_extension()
        logits, labels, lse = ctx.saved_tensors
        dlogits = C.cross_entropy_bwd(dloss.contiguous(), logits, labels, lse, ctx.ignore_index)
        return dlogits, None, None


def cross_entropy(logits, labels, ignore_index: int = -100, reduction: str = "none"):
    """Per-token loss [N] from logits [N, V]; reduction applied on top.

    The fused gfx950 kernel handles bf16 logits with V % 8 == 0 (the LLM
    vocab shapes); anything else computes eager on the same device."""
    if logits.is_cuda and logits.dtype == torch.bfloat16 and logits.shape[-1] % 8 == 0:
        loss = _CrossEntropyFunction.apply(logits, labels, ignore_index)
    else:
        loss = reference.cross_entropy(logits, labels, ignore_index, reduction="none")
    if reduction == "none":
        return loss
    mask = labels != ignore_index
    n = mask.sum().clamp(min=1)
    if reduction == "mean":
        return loss.sum() / n
    return loss.sum()


# ---------------------------------------------------------------------------
# Fused AdamW (multi-tensor)
# ---------------------------------------------------------------------------
def fused_adamw(
    params, grads, exp_avgs, exp_avg_sqs, masters,
    lr: float, beta1: float, beta2: float, eps: float,
    weight_decay: float, step: int,
):
    """Multi-tensor AdamW.  `masters` may be None (fp32 params) or a list of
    fp32 master weights matching bf16 `params`."""
    if params and params[0].is_cuda:
        C = _load_extension()
        C.fused_adamw(
            list(params), list(grads), list(exp_avgs), list(exp_avg_sqs),
            list(masters) if masters is not None else [],
            lr, beta1, beta2, eps, weight_decay, step,
        )
        return
    for i, p in enumerate(params):
        reference.adamw_step(
            p, grads[i], exp_avgs[i], exp_avg_sqs[i],
            masters[i] if masters is not None else None,
            lr, beta1, beta2, eps, weight_decay, step,
        )


# ---------------------------------------------------------------------------
# Routed MoE FFN (moe_ffn.hip): on-device routing + grouped MFMA GEMMs
# ---------------------------------------------------------------------------
MOE_MAX_EXPERTS = 64
MOE_MAX_TOP_K = 8
MOE_MAX_FLAT_ROWS = 4096   # T * top_k the alignment kernel takes


def _moe_route_supported(logits: torch.Tensor, top_k: int) -> bool:
    return (logits.is_cuda and logits.dim() == 2
            and logits.dtype in (torch.float32, torch.bfloat16)
            and 1 <= logits.shape[1] <= MOE_MAX_EXPERTS
            and 1 <= top_k <= min(MOE_MAX_TOP_K, logits.shape[1]))


def moe_ffn_supported(x: torch.Tensor, router_logits: torch.Tensor, w1: torch.Tensor,
                      w3: torch.Tensor, w2: torch.Tensor, top_k: int) -> bool:
    """True when the fused kernels take these arguments: bf16 x and contiguous
    bf16 weights on the GPU, H and I multiples of 128, 16-byte aligned bases
    (the LDS-DMA source requirement), E <= 64, top_k <= 8, T * top_k <= 4096."""
    if not (x.is_cuda and x.dim() == 2 and w1.dim() == 3 and w2.dim() == 3):
        return False
    T, H = x.shape
    E, _, I = w1.shape
    if not _moe_route_supported(router_logits, top_k):
        return False
    if tuple(router_logits.shape) != (T, E) or T * top_k > MOE_MAX_FLAT_ROWS:
        return False
    if H % 128 or I % 128:
        return False
    if w1.shape != (E, H, I) or w3.shape != (E, H, I) or w2.shape != (E, I, H):
        return False
    for t in (x, w1, w3, w2):
        if t.dtype != torch.bfloat16 or not t.is_cuda:
            return False
    for w in (w1, w3, w2):
        if not w.is_contiguous() or w.data_ptr() % 16:
            return False
    return True


def moe_route(logits: torch.Tensor, top_k: int):
    """Router logits [T, E] -> (expert ids [T, K] int32, weights [T, K] fp32):
    fp32 softmax over E, top-k, renormalised.  Ties go to the lower expert
    index (reference.moe_route)."""
    if _moe_route_supported(logits, top_k):
        C = _load_extension()
        ids, w = C.moe_route(logits.contiguous(), top_k)
        return ids, w
    return reference.moe_route(logits, top_k)


def moe_ffn(x: torch.Tensor, router_logits: torch.Tensor, w1: torch.Tensor,
            w3: torch.Tensor, w2: torch.Tensor, top_k: int) -> torch.Tensor:
    """Routed SwiGLU FFN over stacked expert weights (w1/w3 [E, H, I], w2
    [E, I, H]); x [T, H] -> [T, H] in x.dtype.  On the GPU path nothing syncs
    with the host and only the selected experts' weights are read."""
    if moe_ffn_supported(x, router_logits, w1, w3, w2, top_k):
        C = _load_extension()
        xc = x.contiguous()
        if xc.data_ptr() % 16:
            xc = xc.clone()
        return C.moe_ffn(xc, router_logits.contiguous(), w1, w3, w2, top_k)
    return reference.moe_ffn(x, router_logits, w1, w3, w2, top_k).to(x.dtype)


def moe_ffn_wint8_supported(x: torch.Tensor, router_logits: torch.Tensor,
                            q1: torch.Tensor, s1: torch.Tensor, q3: torch.Tensor,
                            s3: torch.Tensor, q2: torch.Tensor, s2: torch.Tensor,
                            top_k: int) -> bool:
    """True when the fused int8-weight kernels take these arguments: bf16 x on
    the GPU, contiguous int8 q1/q3 [E, I, H] and q2 [E, H, I] with 16-byte
    aligned bases, contiguous fp32 scales s1/s3 [E, I] and s2 [E, H], H and I
    multiples of 128, E <= 64, top_k <= 8, T * top_k <= 4096."""
    if not (x.is_cuda and x.dim() == 2 and q1.dim() == 3 and q2.dim() == 3):
        return False
    T, H = x.shape
    E, I, _ = q1.shape
    if not _moe_route_supported(router_logits, top_k):
        return False
    if tuple(router_logits.shape) != (T, E) or T * top_k > MOE_MAX_FLAT_ROWS:
        return False
    if H % 128 or I % 128 or x.dtype != torch.bfloat16:
        return False
    if q1.shape != (E, I, H) or q3.shape != (E, I, H) or q2.shape != (E, H, I):
        return False
    if s1.shape != (E, I) or s3.shape != (E, I) or s2.shape != (E, H):
        return False
    for q in (q1, q3, q2):
        if (q.dtype != torch.int8 or not q.is_cuda or not q.is_contiguous()
                or q.data_ptr() % 16):
            return False
    for s in (s1, s3, s2):
        if s.dtype != torch.float32 or not s.is_cuda or not s.is_contiguous():
            return False
    return True


def moe_ffn_wint8(x: torch.Tensor, router_logits: torch.Tensor, q1: torch.Tensor,
                  s1: torch.Tensor, q3: torch.Tensor, s3: torch.Tensor,
                  q2: torch.Tensor, s2: torch.Tensor, top_k: int) -> torch.Tensor:
    """moe_ffn over weight-only int8 experts in the layout of
    quantization.quantize_moe_int8 (q1/q3 [E, I, H], q2 [E, H, I] int8, one
    fp32 scale per expert and output column); x [T, H] -> [T, H] in x.dtype.
    The kernels stream the int8 bytes of the selected experts only, convert
    them to bf16 in registers (exactly) and apply the scale to the fp32 sums."""
    if moe_ffn_wint8_supported(x, router_logits, q1, s1, q3, s3, q2, s2, top_k):
        C = _load_extension()
        xc = x.contiguous()
        if xc.data_ptr() % 16:
            xc = xc.clone()
        return C.moe_ffn_wint8(xc, router_logits.contiguous(), q1, s1, q3, s3, q2, s2,
                               top_k)
    return reference.moe_ffn_wint8(x, router_logits, q1, s1, q3, s3, q2, s2,
                                   top_k).to(x.dtype)
