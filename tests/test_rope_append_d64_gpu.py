"""rope_cache_append at head dim 64: 32 rotation pairs per head, fewer than
the 64 lanes of the wave that handles it.  (The kernel once computed
"pairs per lane" as 32 / 64 = 0: q came back zero and K was never written to
the cache, which the engines' loose end-to-end allowances did not show.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    from paddlenlp_amd.ops.functional import _load_extension

    return _load_extension()


def _inputs(D):
    from paddlenlp_amd import ops

    torch.manual_seed(1)
    B, T, Hq, Hk = 2, 6, 4, 2
    bs, nblocks, max_blocks = 4, 32, 8
    qkv = torch.randn(B, T, (Hq + 2 * Hk) * D, device="cuda", dtype=torch.bfloat16)
    block_table = torch.arange(B * max_blocks, dtype=torch.int32).reshape(B, max_blocks).cuda()
    lens_before = torch.tensor([3, 0], dtype=torch.int32, device="cuda")
    counts = torch.tensor([6, 4], dtype=torch.int32, device="cuda")
    cos, sin = ops.build_rope_cache(64, D, device="cuda")
    return qkv, block_table, lens_before, counts, cos, sin, (B, T, Hq, Hk, bs, nblocks)


def test_rope_cache_append_d64_bf16(C):
    """Same tolerances as test_inference_gpu.test_rope_cache_append (D = 128)."""
    from paddlenlp_amd.experimental.fused_transformer import rope_cache_append_ref

    D = 64
    qkv, block_table, lens_before, counts, cos, sin, (B, T, Hq, Hk, bs, nblocks) = _inputs(D)
    k_cache = torch.zeros(nblocks, bs, Hk, D, device="cuda", dtype=torch.bfloat16)
    v_cache = torch.zeros_like(k_cache)
    q_out = C.rope_cache_append(qkv, k_cache, v_cache, block_table, lens_before,
                                cos, sin, Hq, Hk, counts)
    kc_ref = torch.zeros(nblocks, bs, Hk, D, dtype=torch.bfloat16)
    vc_ref = torch.zeros_like(kc_ref)
    q_ref = rope_cache_append_ref(qkv.cpu(), kc_ref, vc_ref, block_table.cpu(),
                                  lens_before.cpu(), cos.cpu(), sin.cpu(), Hq, Hk,
                                  counts.cpu())
    assert q_ref.abs().max() > 1 and kc_ref.abs().max() > 1   # the reference is not trivial
    assert torch.allclose(q_out.cpu().float(), q_ref.float(), atol=2e-2, rtol=2e-2), \
        (q_out.cpu().float() - q_ref.float()).abs().max()
    assert torch.allclose(k_cache.cpu().float(), kc_ref.float(), atol=2e-2, rtol=2e-2), \
        (k_cache.cpu().float() - kc_ref.float()).abs().max()
    assert torch.allclose(v_cache.cpu().float(), vc_ref.float(), atol=2e-2, rtol=2e-2)


def test_rope_cache_append_d64_int8(C):
    """int8 cache: dequantised K/V within one quantisation step (absmax/127)
    plus the bf16 rounding of the rotation of the bf16 reference cache."""
    from paddlenlp_amd.experimental.fused_transformer import rope_cache_append_ref

    D = 64
    qkv, block_table, lens_before, counts, cos, sin, (B, T, Hq, Hk, bs, nblocks) = _inputs(D)
    k_cache = torch.zeros(nblocks, bs, Hk, D, device="cuda", dtype=torch.int8)
    v_cache = torch.zeros_like(k_cache)
    k_scale = torch.zeros(nblocks, bs, Hk, device="cuda", dtype=torch.float32)
    v_scale = torch.zeros_like(k_scale)
    q_out = C.rope_cache_append(qkv, k_cache, v_cache, block_table, lens_before,
                                cos, sin, Hq, Hk, counts, k_scale, v_scale)
    kc_ref = torch.zeros(nblocks, bs, Hk, D, dtype=torch.bfloat16)
    vc_ref = torch.zeros_like(kc_ref)
    q_ref = rope_cache_append_ref(qkv.cpu(), kc_ref, vc_ref, block_table.cpu(),
                                  lens_before.cpu(), cos.cpu(), sin.cpu(), Hq, Hk,
                                  counts.cpu())
    assert torch.allclose(q_out.cpu().float(), q_ref.float(), atol=2e-2, rtol=2e-2)
    for cache, scale, ref in ((k_cache, k_scale, kc_ref), (v_cache, v_scale, vc_ref)):
        deq = cache.cpu().float() * scale.cpu()[..., None]
        step = ref.float().abs().amax(-1, keepdim=True) / 127.0
        err = (deq - ref.float()).abs()
        assert (err <= step + 2e-2 * ref.float().abs() + 1e-6).all(), err.max()
