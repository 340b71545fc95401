"""GPU checks for the decoder layer's fused elementwise path: residual add +
RMSNorm in one kernel, rope in place on the packed QKV rows, attention reading
q/k/v through row strides, and the vectorized delta kernel.

None of these ops contains a GEMM, so the fused ops are compared bit for bit
(torch.equal) with the unfused composition built from the same extension."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    from paddlenlp_amd.ops.functional import _load_extension

    return _load_extension()


def _rand(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g).to(torch.bfloat16)


# ---------------------------------------------------------------------------
# add + rms_norm.  (70, 4096): the register dw path at the bench width;
# (2053, 512): more rows than blocks, ragged grid-stride; (9, 8200): H above
# the 8192 register bound, i.e. the streaming path.
# ---------------------------------------------------------------------------
ADD_NORM_SHAPES = [(3, 512), (70, 4096), (2053, 512), (9, 8200)]


@pytest.mark.parametrize("rows,H", ADD_NORM_SHAPES)
def test_add_rms_norm_matches_unfused_and_reference(C, rows, H):
    from paddlenlp_amd import ops

    eps = 1e-6
    residual = _rand(rows, H, seed=1)
    delta = _rand(rows, H, seed=2)
    w = _rand(H, seed=3)
    dy = _rand(rows, H, seed=4)
    dh = _rand(rows, H, seed=5)

    h, y, invrms = C.add_rms_norm_fwd(residual, delta, w, eps)
    h_ref = residual + delta
    assert torch.equal(h, h_ref)
    y_un, invrms_un = C.rms_norm_fwd(h_ref, w, eps)
    assert torch.equal(y, y_un)
    assert torch.equal(invrms, invrms_un)

    dx, dw = C.add_rms_norm_bwd(dy, dh, h, w, invrms)
    dx_norm, dw_un = C.rms_norm_bwd(dy, h_ref, w, invrms_un)
    assert torch.equal(dx, dx_norm + dh)

    # fp32 reference on the same bf16 inputs, tolerances of test_rms_norm_fwd_bwd
    hr = h_ref.float().requires_grad_()
    wr = w.float().requires_grad_()
    yr = ops.reference.rms_norm(hr, wr, eps)
    yr.backward(dy.float())
    dxr = hr.grad + dh.float()
    assert torch.allclose(y.float(), yr, atol=2e-2, rtol=2e-2)
    assert torch.allclose(dx.float(), dxr, atol=5e-2, rtol=5e-2)
    assert torch.allclose(dw.float(), wr.grad, atol=2e-1, rtol=5e-2)
    assert torch.allclose(dw_un.float(), wr.grad, atol=2e-1, rtol=5e-2)


def test_add_rms_norm_autograd_matches_unfused(C):
    """The autograd wrapper: one gradient for both addends, equal to what the
    separate add and rms_norm give, also when h has no other consumer."""
    from paddlenlp_amd import ops

    rows, H = 70, 4096
    w0 = _rand(H, seed=3)
    gh = _rand(rows, H, seed=6)
    gy = _rand(rows, H, seed=7)
    for use_h in (True, False):
        grads = []
        for fused in (True, False):
            r = _rand(rows, H, seed=1).requires_grad_()
            d = _rand(rows, H, seed=2).requires_grad_()
            w = w0.clone().requires_grad_()
            if fused:
                h, y = ops.add_rms_norm(r, d, w, 1e-6)
            else:
                h = r + d
                y = ops.rms_norm(h, w, 1e-6)
            loss = (y * gy).sum()
            if use_h:
                loss = loss + (h * gh).sum()
            loss.backward()
            grads.append((r.grad, d.grad, w.grad))
        (rf, df, wf), (ru, du, wu) = grads
        assert torch.equal(rf, ru) and torch.equal(df, du)
        # dw goes through fp32 atomics: equal up to the bf16 rounding of the sum
        assert torch.allclose(wf.float(), wu.float(), atol=2e-1, rtol=5e-2)


# ---------------------------------------------------------------------------
# packed rope
# ---------------------------------------------------------------------------
def _split_packed(qkv, Hq, Hk, D):
    B, S, _ = qkv.shape
    q, k, v = qkv.split([Hq * D, Hk * D, Hk * D], dim=-1)
    return (q.reshape(B, S, Hq, D).contiguous(), k.reshape(B, S, Hk, D).contiguous(),
            v.reshape(B, S, Hk, D).contiguous())


@pytest.mark.parametrize("B,S,Hq,Hk,D", [(2, 64, 4, 2, 128), (1, 5, 2, 1, 64)])
@pytest.mark.parametrize("backward", [False, True])
def test_rope_packed_matches_out_of_place(C, B, S, Hq, Hk, D, backward):
    from paddlenlp_amd import ops

    qkv = _rand(B, S, (Hq + 2 * Hk) * D, seed=11)
    cos, sin = ops.build_rope_cache(S, D, device="cuda")
    q, k, v = _split_packed(qkv, Hq, Hk, D)
    q_ref, k_ref = C.rope_fwd(q, k, cos, sin, backward)
    out = qkv.clone()
    C.rope_packed_(out, cos, sin, Hq, Hk, backward)
    q_out, k_out, v_out = _split_packed(out, Hq, Hk, D)
    assert torch.equal(q_out, q_ref)
    assert torch.equal(k_out, k_ref)
    assert torch.equal(v_out, v)


# ---------------------------------------------------------------------------
# packed attention: (1,128,..) one tile; (1,100,..) ragged; (2,300,..) several
# q/kv blocks and a batch stride
# ---------------------------------------------------------------------------
PACKED_SHAPES = [(1, 128, 4, 2, 128), (1, 100, 2, 2, 128), (2, 300, 8, 2, 128)]


def _check_packed_attention(C, B, S, Hq, Hk, D, startend):
    qkv = _rand(B, S, (Hq + 2 * Hk) * D, seed=21)
    q, k, v = _split_packed(qkv, Hq, Hk, D)
    do = _rand(B, S, Hq, D, seed=22)
    if startend is None:
        o_ref, lse_ref = C.flash_attn_fwd(q, k, v, True)
        o, lse = C.flash_attn_packed_fwd(qkv, Hq, Hk, True)
        dq, dk, dv = C.flash_attn_bwd(do, q, k, v, o_ref, lse_ref, True)
        dqkv = C.flash_attn_packed_bwd(do, qkv, o, lse, Hq, Hk, True)
    else:
        o_ref, lse_ref = C.flashmask_attn_fwd(q, k, v, startend)
        o, lse = C.flashmask_attn_packed_fwd(qkv, Hq, Hk, startend)
        dq, dk, dv = C.flashmask_attn_bwd(do, q, k, v, o_ref, lse_ref, startend)
        dqkv = C.flashmask_attn_packed_bwd(do, qkv, o, lse, Hq, Hk, startend)
    assert torch.equal(o, o_ref)
    assert torch.equal(lse, lse_ref)
    dq_p, dk_p, dv_p = _split_packed(dqkv, Hq, Hk, D)
    assert torch.equal(dq_p, dq)
    assert torch.equal(dk_p, dk)
    assert torch.equal(dv_p, dv)


@pytest.mark.parametrize("B,S,Hq,Hk,D", PACKED_SHAPES)
def test_packed_attention_matches_contiguous(C, B, S, Hq, Hk, D):
    _check_packed_attention(C, B, S, Hq, Hk, D, None)


def test_packed_flashmask_matches_contiguous(C):
    B, S, Hq, Hk, D = 2, 300, 8, 2, 128
    # three packed samples with boundaries off every tile edge
    se = torch.empty(B, S, dtype=torch.int32, device="cuda")
    se[:, :77] = 77
    se[:, 77:205] = 205
    se[:, 205:] = 300
    _check_packed_attention(C, B, S, Hq, Hk, D, se)


def test_packed_rope_attention_autograd_matches_unfused(C):
    """The autograd function (in-place rope, attention, one dqkv with the rope
    backward run in place on it) against fused_rope + flash_attention on the
    split views."""
    from paddlenlp_amd import ops

    B, S, Hq, Hk, D = 2, 300, 8, 2, 128
    cos, sin = ops.build_rope_cache(S, D, device="cuda")
    do = _rand(B, S, Hq, D, seed=32)
    outs = []
    for packed in (True, False):
        x = _rand(B, S, (Hq + 2 * Hk) * D, seed=31).requires_grad_()
        qkv = x.clone()
        if packed:
            assert ops.packed_rope_attention_supported(qkv, Hq, Hk)
            o = ops.packed_rope_attention(qkv, cos, sin, Hq, Hk)
        else:
            q, k, v = qkv.split([Hq * D, Hk * D, Hk * D], dim=-1)
            q, k = ops.fused_rope(q.view(B, S, Hq, D), k.view(B, S, Hk, D), cos, sin)
            o = ops.flash_attention(q, k, v.view(B, S, Hk, D), causal=True)
        o.backward(do)
        outs.append((o.detach(), x.grad))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------------------
# delta = rowsum(dO * O).  bf16 products are exact in fp32, so the error is
# the fp32 accumulation of D terms: at most D * 2^-23 * sum|dO*O| per row.
# ---------------------------------------------------------------------------
def _delta_bound_check(delta, do, o):
    D = do.shape[-1]
    prod = do.double() * o.double()
    ref = prod.sum(-1).permute(0, 2, 1)          # [B, Hq, S]
    bound = D * 2.0 ** -23 * prod.abs().sum(-1).permute(0, 2, 1)
    err = (delta.double() - ref).abs()
    assert (err <= bound).all(), (err - bound).max().item()


@pytest.mark.parametrize("B,S,H,D", [(1, 100, 2, 128), (2, 64, 4, 128)])
def test_delta_v2(C, B, S, H, D):
    q, k, v = (_rand(B, S, H, D, seed=s) for s in (41, 42, 43))
    o = _rand(B, S, H, D, seed=44)
    do = _rand(B, S, H, D, seed=45)
    lse = torch.zeros(B, H, S, device="cuda")
    delta = torch.full((B, H, S), float("nan"), device="cuda")
    C.flash_attn_bwd2_parts(do, q, k, v, o, lse, delta, True, 1)
    _delta_bound_check(delta, do, o)


def test_delta_d64_v1_backward(C):
    """D = 64 has no v2 kernel: the v1 backward runs the shared delta kernel.
    flash_bwd_delta is that launch on its own; the v1 backward built on it is
    checked against the fp32 reference at the existing backward tolerances."""
    from paddlenlp_amd import ops

    B, S, Hq, Hk, D = 2, 72, 4, 2, 64
    q = _rand(B, S, Hq, D, seed=51)
    k = _rand(B, S, Hk, D, seed=52)
    v = _rand(B, S, Hk, D, seed=53)
    do = _rand(B, S, Hq, D, seed=54)
    o, lse = C.flash_attn_fwd_ex(q, k, v, True, True)
    _delta_bound_check(C.flash_bwd_delta(do, o), do, o)

    dq, dk, dv = C.flash_attn_bwd_ex(do, q, k, v, o, lse, True, True)
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    ops.reference.flash_attention(qr, kr, vr, causal=True).backward(do.float())
    assert torch.allclose(dq.float(), qr.grad, atol=5e-2, rtol=5e-2)
    assert torch.allclose(dk.float(), kr.grad, atol=5e-2, rtol=5e-2)
    assert torch.allclose(dv.float(), vr.grad, atol=5e-2, rtol=5e-2)


# ---------------------------------------------------------------------------
# tiny llama, fused path on and off
# ---------------------------------------------------------------------------
def _tiny_llama_run(monkeypatch, fusion, recompute):
    from paddlenlp_amd.transformers import LlamaConfig, LlamaForCausalLM

    monkeypatch.setenv("PNLP_LAYER_FUSION", "1" if fusion else "0")
    torch.manual_seed(0)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=256, intermediate_size=512,
        num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
        max_position_embeddings=256, recompute=recompute,
    )
    model = LlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device="cuda")
    model.train()
    ids = torch.randint(0, 512, (2, 128), device="cuda")
    labels = torch.randint(0, 512, (2, 128), device="cuda")
    loss, _ = model(input_ids=ids, labels=labels)
    loss.backward()
    return loss.item(), {n: p.grad for n, p in model.named_parameters()}


@pytest.mark.parametrize("recompute", [False, True])
def test_tiny_llama_fused_matches_unfused(C, monkeypatch, recompute):
    """Every non-GEMM op of the two paths is bit-equal (tests above) and the
    GEMMs see the same operands, so what may differ is the fp32 atomic order
    in the norm dw and a reordered GEMM reduction: a few ulps of bf16 (2^-8
    relative) at the scale of each tensor.  4 ulps are allowed."""
    loss_on, g_on = _tiny_llama_run(monkeypatch, True, recompute)
    loss_off, g_off = _tiny_llama_run(monkeypatch, False, recompute)
    assert 4.0 < loss_on < 9.0
    assert abs(loss_on - loss_off) <= 2.0 ** -6 * abs(loss_off)
    for n, g in g_off.items():
        assert g_on[n] is not None and torch.isfinite(g_on[n]).all(), n
        scale = g.float().abs().max().item()
        assert torch.allclose(g_on[n].float(), g.float(), rtol=2.0 ** -6,
                              atol=2.0 ** -6 * scale), n
