"""GPU checks for the LDS-DMA staging of the v2 forward and dq kernels.

Both kernels fill one dual-use LDS image of K and one of V per tile
(mfma.h img_off) and read it by rows and transposed.  They are compared
against the fp32 reference on the same bf16 inputs with the project's
tolerances (atol = rtol = 3e-2 for o, 5e-2 for dq, dk and dv, as
test_ops_gpu).  q, k, v and dO are independent random tensors, so a swapped
chunk or a wrong transposed read gives errors of order 1."""
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128


@pytest.fixture(scope="module")
def C():
    from paddlenlp_amd.ops.functional import _load_extension

    return _load_extension()


def _inputs(B, Sq, Skv, Hq, Hk, seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, Sq, Hq, D, device="cuda").to(torch.bfloat16).requires_grad_()
    k = torch.randn(B, Skv, Hk, D, device="cuda").to(torch.bfloat16).requires_grad_()
    v = torch.randn(B, Skv, Hk, D, device="cuda").to(torch.bfloat16).requires_grad_()
    do = torch.randn(B, Sq, Hq, D, device="cuda").to(torch.bfloat16)
    return q, k, v, do


def _check(q, k, v, do, **kw):
    from paddlenlp_amd import ops

    out = ops.flash_attention(q, k, v, **kw)
    out.backward(do)
    qr = q.detach().float().requires_grad_()
    kr = k.detach().float().requires_grad_()
    vr = v.detach().float().requires_grad_()
    ref = ops.reference.flash_attention(qr, kr, vr, **kw)
    ref.backward(do.float())
    assert torch.isfinite(out).all(), "out"
    assert torch.allclose(out.float(), ref, atol=3e-2, rtol=3e-2), \
        ("out", (out.float() - ref).abs().max())
    for name, got, want in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad),
                            ("dv", v.grad, vr.grad)):
        assert torch.isfinite(got).all(), name
        assert torch.allclose(got.float(), want, atol=5e-2, rtol=5e-2), \
            (name, (got.float() - want).abs().max())


@pytest.mark.parametrize("B,Sq,Skv,Hq,Hk,causal", [
    (1, 64, 64, 4, 1, True),      # a single kv tile: prime and compute only
    (1, 100, 100, 2, 2, True),    # one ragged tile: clamped source rows
    (2, 192, 192, 4, 2, True),    # 3 tiles: buffer parity
    (1, 300, 300, 8, 2, True),    # two q blocks, ragged last tile, some waves
                                  # skip compute while still staging
    (1, 577, 577, 4, 1, True),    # three q blocks, ragged by one
    (1, 128, 320, 4, 2, True),    # causal offset != 0
    (1, 300, 300, 4, 2, False),   # non-causal: no skipping
    (8, 320, 320, 8, 8, True),    # B*Hq a multiple of 8: grouped tile order
])
def test_fwd_dq_staging(C, B, Sq, Skv, Hq, Hk, causal):
    q, k, v, do = _inputs(B, Sq, Skv, Hq, Hk)
    _check(q, k, v, do, causal=causal)


def test_fwd_dq_staging_packed(C):
    """k and v as strided slices of one packed qkv tensor (row stride
    (Hq + 2*Hk)*D): the packed path against the unpacked ops on the same
    values, which the cases above hold to the reference."""
    from paddlenlp_amd import ops

    B, S, Hq, Hk = 2, 192, 4, 2
    cos, sin = ops.build_rope_cache(S, D, device="cuda")
    torch.manual_seed(3)
    x0 = torch.randn(B, S, (Hq + 2 * Hk) * D, device="cuda").to(torch.bfloat16)
    do = torch.randn(B, S, Hq, D, device="cuda").to(torch.bfloat16)
    outs = []
    for packed in (True, False):
        x = x0.clone().requires_grad_()
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
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    # the same kernels on the same values: only the addressing differs
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("S,bounds", [
    (320, (70, 200, 320)),    # segment boundaries off the 64 grid
    (576, (200, 256, 576)),   # q block 1 clears every bound of kv tiles 0-3:
                              # their staging is skipped for whole tiles
])
def test_fwd_dq_staging_flashmask(C, S, bounds):
    B, Hq, Hk = 1, 4, 2
    q, k, v, do = _inputs(B, S, S, Hq, Hk, seed=2)
    se = torch.empty(B, 1, S, 1, dtype=torch.int32, device="cuda")
    lo = 0
    for hi in bounds:
        se[:, 0, lo:hi, 0] = hi
        lo = hi
    _check(q, k, v, do, causal=True, startend_row_indices=se)


def test_misaligned_kv_takes_v1(C):
    """LDS-DMA needs 16-byte aligned sources.  The v2 launchers decline a k
    that is 8 bytes off, as they decline a shape that is not theirs, and the
    v1 kernels run: the result is v1's, bit for bit."""
    B, S, Hq, Hk = 1, 100, 2, 2
    q, k, v, do = _inputs(B, S, S, Hq, Hk, seed=4)
    q, k, v = q.detach(), k.detach(), v.detach()
    buf = torch.empty(k.numel() + 4, device="cuda", dtype=torch.bfloat16)
    k_off = buf[4:].view_as(k)
    k_off.copy_(k)
    assert k_off.is_contiguous() and k_off.data_ptr() % 16 == 8
    o_v1, lse_v1 = C.flash_attn_fwd_ex(q, k, v, True, True)
    o, lse = C.flash_attn_fwd_ex(q, k_off, v, True, False)
    torch.cuda.synchronize()
    assert torch.equal(o, o_v1) and torch.equal(lse, lse_v1)
    dq_v1, dk_v1, dv_v1 = C.flash_attn_bwd_ex(do, q, k, v, o_v1, lse_v1, True, True)
    dq, dk, dv = C.flash_attn_bwd_ex(do, q, k_off, v, o, lse, True, False)
    torch.cuda.synchronize()
    assert torch.equal(dq, dq_v1) and torch.equal(dk, dk_v1) and torch.equal(dv, dv_v1)
