"""Plain-PyTorch fp32 reference implementations of every fused op.

These serve two purposes:
  1. the CPU execution path (tests, plumbing configs — no GPU in CI), and
  2. the numerics oracle that GPU tests compare the HIP kernels against.

They are intentionally simple and written for clarity, not speed.  On a GPU
box the HIP extension (paddlenlp_amd.ops._C) is mandatory — see functional.py.

Reference op semantics follow PaddleNLP's fused ops:
fused_rms_norm, fused_rotary_position_embedding, swiglu, flash_attention,
fused cross-entropy (ParallelCrossEntropy's local form), fused AdamW.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """y = x / rms(x) * weight, computed in fp32."""
    dtype = x.dtype
    x32 = x.float()
    variance = x32.pow(2).mean(-1, keepdim=True)
    y = x32 * torch.rsqrt(variance + eps)
    return (y * weight.float()).to(dtype)


def build_rope_cache(
    seq_len: int,
    head_dim: int,
    base: float = 10000.0,
    dtype: torch.dtype = torch.float32,
    device=None,
    position_ids: Optional[torch.Tensor] = None,
    scaling_factor: float = 1.0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos/sin tables of shape [seq_len, head_dim] (half-duplicated).

    Matches the Llama convention: inv_freq over even dims, table is
    cat(freqs, freqs) so that rotate_half applies to (x1, x2) halves.
    """
    inv_freq = 1.0 / (base ** (torch.arange(0, head_dim, 2, dtype=torch.float32, device=device) / head_dim))
    if position_ids is None:
        t = torch.arange(seq_len, dtype=torch.float32, device=device)
    else:
        t = position_ids.float()
    t = t / scaling_factor
    freqs = torch.outer(t, inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _rotate_half(x: torch.Tensor) -> torch.Tensor:
    x1 = x[..., : x.shape[-1] // 2]
    x2 = x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def apply_rope(
    q: torch.Tensor,  # [B, S, Hq, D]
    k: torch.Tensor,  # [B, S, Hk, D]
    cos: torch.Tensor,  # [S, D]
    sin: torch.Tensor,  # [S, D]
) -> Tuple[torch.Tensor, torch.Tensor]:
    cos = cos.to(q.dtype)[None, :, None, :]
    sin = sin.to(q.dtype)[None, :, None, :]
    q_out = q * cos + _rotate_half(q) * sin
    k_out = k * cos + _rotate_half(k) * sin
    return q_out, k_out


def swiglu(x: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """silu(gate) * up.  Single-arg form takes cat([gate, up], -1)."""
    if y is None:
        x, y = x.chunk(2, dim=-1)
    return F.silu(x) * y


def moe_route(logits: torch.Tensor, top_k: int):
    """Router: fp32 softmax over all E experts, top-k, then the k weights
    renormalised to sum to 1.  logits [T, E] -> (ids [T, K] int32, weights
    [T, K] fp32), in descending-probability order.

    Tie rule (the same as the moe_route kernel's): among equal probabilities
    the LOWER expert index wins.  A stable descending sort gives exactly that;
    torch.topk leaves the order of ties unspecified."""
    probs = logits.float().softmax(-1)
    sp, si = torch.sort(probs, dim=-1, descending=True, stable=True)
    w = sp[:, :top_k]
    return si[:, :top_k].to(torch.int32), w / w.sum(-1, keepdim=True)


def moe_ffn(x: torch.Tensor, router_logits: torch.Tensor, w1: torch.Tensor,
            w3: torch.Tensor, w2: torch.Tensor, top_k: int) -> torch.Tensor:
    """Routed SwiGLU FFN, fp32 math on whatever dtype it is given; returns
    fp32 [T, H].  x [T, H], router_logits [T, E], w1/w3 [E, H, I], w2
    [E, I, H]:

        out[t] = sum_k w[t,k] * (silu(x[t] @ w1[e]) * (x[t] @ w3[e])) @ w2[e],
        (e, w) = moe_route(router_logits, top_k)[t, k]

    Only the selected experts are visited, so an unselected expert's weights
    may hold anything (NaN included).  The k contributions are added in k
    order."""
    ids, w = moe_route(router_logits, top_k)
    x32 = x.float()
    out = torch.zeros_like(x32)
    for k in range(top_k):
        for e in torch.unique(ids[:, k]).tolist():
            rows = (ids[:, k] == e).nonzero(as_tuple=True)[0]
            xe = x32[rows]
            act = F.silu(xe @ w1[e].float()) * (xe @ w3[e].float())
            out[rows] += (act @ w2[e].float()) * w[rows, k, None]
    return out


def moe_ffn_wint8(x: torch.Tensor, router_logits: torch.Tensor,
                  q1: torch.Tensor, s1: torch.Tensor, q3: torch.Tensor, s3: torch.Tensor,
                  q2: torch.Tensor, s2: torch.Tensor, top_k: int) -> torch.Tensor:
    """moe_ffn over weight-only int8 experts as quantization.quantize_moe_int8
    packs them: q1/q3 [E, I, H], q2 [E, H, I] int8 (contraction contiguous),
    s1/s3 [E, I], s2 [E, H] fp32.  The weights are dequantized to fp32
    (q * scale, then the layout of moe_ffn) and handed to moe_ffn; returns fp32
    [T, H].

    Only the selected experts are dequantized, the others stay zero and are
    never visited, so an unselected expert may hold anything (NaN scales
    included)."""
    from ..quantization import dequantize_moe_int8

    ids, _ = moe_route(router_logits, top_k)
    sel = torch.unique(ids).long()

    def deq(q, s):
        w = torch.zeros(q.shape[0], q.shape[2], q.shape[1], dtype=torch.float32,
                        device=q.device)
        w[sel] = dequantize_moe_int8(q[sel], s[sel], torch.float32)
        return w

    return moe_ffn(x, router_logits, deq(q1, s1), deq(q3, s3), deq(q2, s2), top_k)


def flash_attention(
    q: torch.Tensor,  # [B, S, Hq, D]
    k: torch.Tensor,  # [B, S, Hk, D]
    v: torch.Tensor,  # [B, S, Hk, D]
    causal: bool = True,
    attn_mask: Optional[torch.Tensor] = None,
    startend_row_indices: Optional[torch.Tensor] = None,
    return_lse: bool = False,
):
    """Reference attention in fp32 (materializes scores — small inputs only).

    GQA: k/v heads are repeated to match q heads.
    `startend_row_indices` is the FlashMask sparse-mask form
    (reference: flashmask_attention, llama/fusion_ops.py:218-238):
    [B, Hk_or_1, S, 1] int32 — for causal masking, key j attends to query
    rows i with j <= i < startend[j]; rows >= startend[j] are masked.
    """
    B, S, Hq, D = q.shape
    Hk = k.shape[2]
    if Hk != Hq:
        rep = Hq // Hk
        k = k.repeat_interleave(rep, dim=2)
        v = v.repeat_interleave(rep, dim=2)
    q32 = q.permute(0, 2, 1, 3).float()  # [B, H, S, D]
    k32 = k.permute(0, 2, 1, 3).float()
    v32 = v.permute(0, 2, 1, 3).float()
    scores = q32 @ k32.transpose(-1, -2) / math.sqrt(D)
    Skv = k32.shape[-2]
    if startend_row_indices is not None:
        # FlashMask: key column j is visible to query rows j <= i < start[j]
        start = startend_row_indices.to(torch.long)  # [B, h, Skv, 1]
        rows = torch.arange(S, device=q.device).view(1, 1, S, 1)
        cols_start = start.transpose(-1, -2)  # [B, h, 1, Skv]
        causal_m = torch.arange(Skv, device=q.device).view(1, 1, 1, Skv) <= rows
        visible = causal_m & (rows < cols_start)
        scores = scores.masked_fill(~visible, float("-inf"))
    elif causal:
        mask = torch.ones(S, Skv, dtype=torch.bool, device=q.device).tril(Skv - S)
        scores = scores.masked_fill(~mask, float("-inf"))
    if attn_mask is not None:
        scores = scores + attn_mask.float()
    probs = scores.softmax(-1)
    # fully-masked rows produce NaN via softmax(-inf row); zero them
    probs = torch.nan_to_num(probs, nan=0.0)
    out = probs @ v32  # [B, H, S, D]
    out = out.permute(0, 2, 1, 3).to(q.dtype)
    if return_lse:
        lse = torch.logsumexp(scores, dim=-1)  # [B, H, S]; -inf for masked rows
        return out, lse
    return out


def cross_entropy(
    logits: torch.Tensor,  # [N, V]
    labels: torch.Tensor,  # [N]
    ignore_index: int = -100,
    reduction: str = "none",
) -> torch.Tensor:
    return F.cross_entropy(
        logits.float(), labels, ignore_index=ignore_index, reduction=reduction
    )


@torch.no_grad()
def adamw_step(
    param: torch.Tensor,
    grad: torch.Tensor,
    exp_avg: torch.Tensor,
    exp_avg_sq: torch.Tensor,
    master: Optional[torch.Tensor],
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
    step: int,
) -> None:
    """Single-tensor AdamW in fp32 with optional bf16 param + fp32 master."""
    p32 = master if master is not None else param
    g32 = grad.float()
    exp_avg.mul_(beta1).add_(g32, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g32, g32, value=1 - beta2)
    bias1 = 1 - beta1**step
    bias2 = 1 - beta2**step
    denom = (exp_avg_sq / bias2).sqrt_().add_(eps)
    p32.mul_(1 - lr * weight_decay)
    p32.addcdiv_(exp_avg / bias1, denom, value=-lr)
    if master is not None:
        param.copy_(p32.to(param.dtype))


# ---------------------------------------------------------------------------
# float64 oracles of the training elementwise kernels (rms_norm, rope, swiglu,
# cross_entropy, adamw) and the rule their outputs are compared by.
#
# An oracle upcasts the bf16/fp32 inputs to float64 and returns, for every
# output, the exact result `ref` and a `scale` of the same shape: the sum of
# the absolute values of the terms `ref` was formed from.  Backward formulas
# are written out (tests/test_train_ops_oracle.py checks them against float64
# autograd).  A kernel output `out` passes when, elementwise,
#
#     |out - ref| <= R * |ref| + c * scale      (+ ORACLE_BF16_TINY for bf16)
#
# R = 2^-8 for a bf16 output (one round-to-nearest to 8 significant bits),
# R = 0 for an fp32 output; c covers the fp32 arithmetic and the fast
# exp/log intrinsics and is one constant per op, at most ORACLE_C_CAP.  The
# relative bounds hold for normal numbers only.  Below 2^-126, the smallest
# normal of bf16 and of fp32 alike, a subnormal keeps fewer bits, and the
# fast intrinsics flush a subnormal fp32 result to 0 (measured: __expf(-90)
# in the cross-entropy backward gives 0 for 1.4e-40).  ORACLE_BF16_TINY
# admits that as an absolute error of up to 2^-126 on a bf16 output.
# ---------------------------------------------------------------------------
ORACLE_R_BF16 = 2.0 ** -8
ORACLE_C_CAP = 2.0 ** -12
ORACLE_BF16_TINY = 2.0 ** -126

# 4x the largest (|out - ref| - R|ref|) / scale measured on an MI355X over the
# sweep of tests/test_train_ops_edges_gpu.py, rounded up to a power of two.
# A bf16 output mostly needs none: R|ref| exceeds the half ulp by the
# mantissa's excess over 1, which already covers fp32-sized errors; what is
# measured there comes from elements whose terms cancel (scale >> |ref|).
ORACLE_C = {
    "rms_norm": 2.0 ** -21,       # measured 1.15e-7 (invrms, 8200 x 64)
    "rope": 2.0 ** -23,           # measured 1.68e-8 (dq, 4 x 1040 x 8 x 128)
    "swiglu": 2.0 ** -24,         # measured 0 on every output: the fp32 unit roundoff
    "cross_entropy": 2.0 ** -20,  # measured 1.38e-7 (loss, 4100 x 1024)
    "adamw": 2.0 ** -16,          # measured 3.63e-6 (delta at step 2, n = 4M + 3): the
                                  # host's 1 - powf(beta2, step) is good to 2^-24 / bias2
}


def oracle_margin(out, ref, scale, R=None, floor=None):
    """The c each element of `out` needs to pass the rule above (0 where
    R * |ref| alone covers it, inf for a non-finite element or an error where
    scale is 0).  R defaults to the output's dtype: 2^-8 for bf16, 0 for
    fp32.  `floor` is an optional absolute allowance (tensor or float)."""
    tiny = 0.0
    if R is None:
        if out.dtype == torch.bfloat16:
            R, tiny = ORACLE_R_BF16, ORACLE_BF16_TINY
        elif out.dtype == torch.float32:
            R = 0.0
        else:
            raise TypeError(f"no default R for {out.dtype}")
    o = out.detach().double().cpu()
    assert o.shape == ref.shape == scale.shape, (o.shape, ref.shape, scale.shape)
    excess = (o - ref).abs() - R * ref.abs() - tiny
    if floor is not None:
        excess = excess - floor
    need = torch.where(excess <= 0, torch.zeros_like(excess), excess / scale)
    return torch.where(torch.isfinite(o), need, torch.full_like(need, float("inf")))


def oracle_close(out, ref, scale, c, R=None, floor=None) -> bool:
    return bool((oracle_margin(out, ref, scale, R=R, floor=floor) <= c).all())


def _f64(t):
    return t.double().cpu()   # keeps the autograd graph of a float64 input


def _f32_value(x: float) -> float:
    """A scalar as the kernel receives it: rounded to fp32."""
    return float(torch.tensor(x, dtype=torch.float32))


def rms_norm_oracle(x, weight, eps: float = 1e-6):
    """x [rows, H], weight [H] -> {y, y_scale, invrms, invrms_scale}."""
    x, w = _f64(x), _f64(weight)
    inv = torch.rsqrt(x.pow(2).mean(-1) + _f32_value(eps))
    y = x * inv[:, None] * w
    return {"y": y, "y_scale": y.abs(), "invrms": inv, "invrms_scale": inv.abs()}


def rms_norm_bwd_oracle(dy, x, weight, eps: float = 1e-6):
    """dx = inv * (dy*w - x * inv^2 * mean(dy*w*x)); dw = sum_rows dy*x*inv.
    -> {dx, dx_scale, dw, dw_scale}."""
    dy, x, w = _f64(dy), _f64(x), _f64(weight)
    H = x.shape[-1]
    inv = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + _f32_value(eps))
    t = dy * w * x
    dx = inv * (dy * w - x * inv.pow(2) * t.sum(-1, keepdim=True) / H)
    dx_scale = inv * ((dy * w).abs() + x.abs() * inv.pow(2) * t.abs().sum(-1, keepdim=True) / H)
    dwt = dy * x * inv
    return {"dx": dx, "dx_scale": dx_scale, "dw": dwt.sum(0), "dw_scale": dwt.abs().sum(0)}


def rope_oracle(x, cos, sin, backward: bool = False):
    """One of q/k, [B, S, H, D], with cos/sin [S, D]:
        out[i]       = x[i]*cos[i]         - sign * x[i + D/2]*sin[i]
        out[i + D/2] = x[i + D/2]*cos[i + D/2] + sign * x[i]*sin[i + D/2]
    sign = +1 forward, -1 backward (rotation by -theta, the gradient for the
    half-duplicated tables of build_rope_cache).  -> (out, scale)."""
    x, c, s = _f64(x), _f64(cos)[None, :, None, :], _f64(sin)[None, :, None, :]
    half = x.shape[-1] // 2
    sign = -1.0 if backward else 1.0
    partner = torch.cat((-x[..., half:], x[..., :half]), dim=-1)
    a, b = x * c, sign * partner * s
    return a + b, a.abs() + b.abs()


def swiglu_oracle(x):
    """x = [gate | up], [N, 2I] -> (y, scale), y = gate * sigmoid(gate) * up."""
    g, u = _f64(x).chunk(2, dim=-1)
    y = g * torch.sigmoid(g) * u
    return y, y.abs()


def swiglu_bwd_oracle(dy, x):
    """dg = dy*u*sig*(1 + g*(1 - sig)), du = dy*g*sig
    -> {dg, dg_scale, du, du_scale}.  1 - sig is taken as sigmoid(-g), so
    nothing cancels at large |g|."""
    dy = _f64(dy)
    g, u = _f64(x).chunk(2, dim=-1)
    sig, one_minus = torch.sigmoid(g), torch.sigmoid(-g)
    lead = dy * u * sig
    du = dy * g * sig
    return {"dg": lead * (1 + g * one_minus),
            "dg_scale": lead.abs() * (1 + g.abs() * one_minus),
            "du": du, "du_scale": du.abs()}


def cross_entropy_oracle(logits, labels, ignore_index: int = -100, dloss=None):
    """logits [N, V] (-inf allowed off the target and off the row maximum),
    labels [N].  With m the row maximum and lse = log(sum exp(l - m)):
        loss = lse - (l_y - m)                  scale |lse| + |l_y - m|
        full = m + lse   (the log-sum-exp)      scale |m| + |lse|
        dlogits = dloss * (p - 1{v == y})       scale |dloss| * (p + 1{v == y})
    An ignored row has loss 0 and dlogits 0, both with scale 0.
    dlogits_floor = |dloss| * 2^-126 is the absolute allowance (oracle_margin's
    `floor`) for a probability below the smallest fp32 normal: the kernel's
    __expf flushes it to 0 before the multiply by dloss, which can bring the
    exact product back above 2^-126 (measured: 2.3e-38 came out as 0).
    -> {max, lse, loss, loss_scale, full, full_scale
        [, dlogits, dlogits_scale, dlogits_floor]}."""
    l, y = _f64(logits), labels.cpu().long()
    N, V = l.shape
    keep = y != ignore_index
    m = l.max(-1).values
    e = torch.exp(l - m[:, None])
    se = e.sum(-1)
    lse = se.log()
    safe = torch.where(keep, y, torch.zeros_like(y))
    t = l.gather(1, safe[:, None]).squeeze(1) - m
    zero = torch.zeros_like(lse)
    out = {"max": m, "lse": lse,
           "loss": torch.where(keep, lse - t, zero),
           "loss_scale": torch.where(keep, lse.abs() + t.abs(), zero),
           "full": m + lse, "full_scale": m.abs() + lse.abs()}
    if dloss is not None:
        dl = torch.where(keep, _f64(dloss), zero)[:, None]
        p = e / se[:, None]
        onehot = torch.zeros_like(p)
        onehot[keep, y[keep]] = 1.0
        out["dlogits"] = dl * (p - onehot)
        out["dlogits_scale"] = dl.abs() * (p + onehot)
        out["dlogits_floor"] = (dl.abs() * 2.0 ** -126).expand(N, V)
    return out


class AdamWOracle:
    """float64 AdamW state machine for one tensor.  `start` is the fp32
    master (bf16 params) or the fp32 param itself; m and v start at 0.  The
    scalars are taken as the kernel receives them, rounded to fp32, and the
    gradient as the kernel reads it, rounded to `param_dtype` first.

    step(grad) advances one step and returns
        {m, m_scale, v, v_scale, delta, w}
    with delta = w_after - w_before = -lr*wd*w - lr * (m/bias1) / (sqrt(v/bias2) + eps),
    m_scale = |beta1*m| + |(1-beta1)*g| and v_scale likewise (= v).

    Left alone it runs on its own float64 state.  step(grad, state=(m, v, w))
    first takes over the fp32 state a kernel under test starts the step from:
    an element whose m nearly cancels carries the earlier steps' rounding at
    a scale that this step's m_scale no longer has, so a tight per-step check
    compares each step on the inputs the kernel had."""

    def __init__(self, start, param_dtype, lr, beta1, beta2, eps, weight_decay):
        self.w = _f64(start).clone()
        self.m = torch.zeros_like(self.w)
        self.v = torch.zeros_like(self.w)
        self.param_dtype = param_dtype
        self.lr, self.beta1, self.beta2, self.eps, self.wd = (
            _f32_value(h) for h in (lr, beta1, beta2, eps, weight_decay))
        self.steps = 0

    def step(self, grad, state=None):
        if state is not None:   # (m, v, w) the kernel under test starts this step from
            self.m, self.v, self.w = (_f64(t).reshape(self.w.shape).clone() for t in state)
        self.steps += 1
        g = _f64(grad.detach().to(self.param_dtype)).reshape(self.w.shape)
        b1, b2 = self.beta1, self.beta2
        m_scale = (b1 * self.m).abs() + ((1 - b1) * g).abs()
        v_scale = (b2 * self.v).abs() + ((1 - b2) * g * g).abs()
        self.m = b1 * self.m + (1 - b1) * g
        self.v = b2 * self.v + (1 - b2) * g * g
        bias1 = 1 - b1 ** self.steps
        bias2 = 1 - b2 ** self.steps
        denom = (self.v / bias2).sqrt() + self.eps
        delta = -self.lr * self.wd * self.w - self.lr * (self.m / bias1) / denom
        self.w = self.w + delta
        return {"m": self.m, "m_scale": m_scale, "v": self.v, "v_scale": v_scale,
                "delta": delta, "w": self.w}
