"""GPU checks for the dkv kernel's LDS-DMA staging and the grouped tile order.

The dual-use LDS image (mfma.h img_off) is compared element for element
through its probe; the attention kernels are compared against the fp32
reference on the same bf16 inputs with the project's backward tolerance
(atol = rtol = 5e-2, as test_ops_gpu.test_flash_attention_bwd; 3e-2 for the
forward output, as test_flash_attention_fwd).  q, k, v and dO are independent
random tensors, so a transposed or chunk-swapped read cannot cancel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128


@pytest.fixture(scope="module")
def C():
    from paddlenlp_amd.ops.functional import _load_extension

    return _load_extension()


def test_lds_image_probe_exact(C):
    """Row view and transposed view of a DMA-filled 64 x 128 image reproduce
    the tile exactly: all 8,192 elements, seeded random bit patterns (the
    XOR can swap the two 16-byte chunks of a 32-byte span without a fault,
    and a spot check can pass)."""
    g = torch.Generator().manual_seed(1234)
    bits = torch.randint(-32768, 32768, (64, 128), generator=g, dtype=torch.int32)
    X = bits.to(torch.int16).cuda().view(torch.bfloat16)
    out_row, out_tr = C.lds_image_probe(X)
    torch.cuda.synchronize()
    want = X.view(torch.int16)
    assert out_row.shape == (64, 128) and out_tr.shape == (64, 128)
    assert torch.equal(out_row.view(torch.int16), want), \
        (out_row.view(torch.int16) != want).nonzero()[:8]
    assert torch.equal(out_tr.view(torch.int16), want), \
        (out_tr.view(torch.int16) != want).nonzero()[:8]


def _inputs(B, Sq, Skv, Hq, Hk, seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, Sq, Hq, D, device="cuda").to(torch.bfloat16).requires_grad_()
    k = torch.randn(B, Skv, Hk, D, device="cuda").to(torch.bfloat16).requires_grad_()
    v = torch.randn(B, Skv, Hk, D, device="cuda").to(torch.bfloat16).requires_grad_()
    do = torch.randn(B, Sq, Hq, D, device="cuda").to(torch.bfloat16)
    return q, k, v, do


def _check(q, k, v, do, check_fwd=False, **kw):
    from paddlenlp_amd import ops

    out = ops.flash_attention(q, k, v, **kw)
    out.backward(do)
    qr = q.detach().float().requires_grad_()
    kr = k.detach().float().requires_grad_()
    vr = v.detach().float().requires_grad_()
    ref = ops.reference.flash_attention(qr, kr, vr, **kw)
    ref.backward(do.float())
    if check_fwd:
        assert torch.allclose(out.float(), ref, atol=3e-2, rtol=3e-2), \
            ("out", (out.float() - ref).abs().max())
    for name, got, want in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad),
                            ("dv", v.grad, vr.grad)):
        assert torch.isfinite(got).all(), name
        assert torch.allclose(got.float(), want, atol=5e-2, rtol=5e-2), \
            (name, (got.float() - want).abs().max())


@pytest.mark.parametrize("B,Sq,Skv,Hq,Hk,causal", [
    (1, 64, 64, 4, 1, True),      # single q tile, G = 4: buffer reuse across g
    (1, 100, 100, 2, 2, True),    # one ragged tile: clamped source rows
    (2, 192, 192, 4, 2, True),    # 3 q tiles per g: buffer parity flips per g
    (1, 300, 300, 8, 2, True),    # two kv blocks, ragged last q tile, G = 4
    (1, 577, 577, 4, 1, True),    # three kv blocks, 10 q tiles, ragged by one
    (1, 128, 320, 4, 2, True),    # causal offset != 0
    (1, 300, 300, 4, 2, False),   # non-causal: no tile skipping at all
])
def test_dkv_staging_bwd(C, B, Sq, Skv, Hq, Hk, causal):
    q, k, v, do = _inputs(B, Sq, Skv, Hq, Hk)
    _check(q, k, v, do, causal=causal)


@pytest.mark.parametrize("B,S,Hq,Hk", [
    (8, 320, 8, 8),   # B*Hq and B*Hk multiples of 8: grouped heaviest-first order
    (1, 320, 4, 1),   # neither is: plain order
])
def test_tile_order_fwd_bwd(C, B, S, Hq, Hk):
    q, k, v, do = _inputs(B, S, S, Hq, Hk, seed=1)
    _check(q, k, v, do, check_fwd=True, causal=True)


@pytest.mark.parametrize("S,bounds", [
    (320, (70, 200, 320)),    # segment boundaries off the 64 grid
    (576, (200, 256, 576)),   # kv block 0 holds no bound past 256: its q-tile
                              # sequence ends early while later tiles exist
])
def test_dkv_staging_flashmask(C, S, bounds):
    B, Hq, Hk = 1, 4, 2
    q, k, v, do = _inputs(B, S, S, Hq, Hk, seed=2)
    se = torch.empty(B, 1, S, 1, dtype=torch.int32, device="cuda")
    lo = 0
    for hi in bounds:
        se[:, 0, lo:hi, 0] = hi
        lo = hi
    _check(q, k, v, do, check_fwd=True, causal=True, startend_row_indices=se)
