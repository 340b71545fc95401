"""Edge shapes of the MFMA paged decode kernel against paged_decode_attn_ref:
the four-wave merge, the split path for GQA groups of 16, 7 and 1, and the
direct-write path.

As in test_append_attn_gpu.py every unused block-table entry points at one
spare block, and that block and every cache slot at or past seq_lens hold NaN,
so an output that is finite and matches proves the kv bound."""
import pytest
import torch

from tests.test_append_attn_gpu import _bf16_case

pytestmark = pytest.mark.gpu

# across the 32-token wave quarter and the 128-token V tile
SPLIT_LENS = [1, 32, 33, 128, 129, 300]


@pytest.fixture(scope="module")
def C():
    from paddlenlp_amd.ops.functional import _load_extension

    return _load_extension()


def decode_case(Hq, Hk, seq_lens, seed):
    """(q [B, Hq, D], k_cache, v_cache, block_table, seq_lens) on the CPU,
    D = 128, block size 16."""
    B = len(seq_lens)
    q, kc, vc, bt, before, _ = _bf16_case(B=B, T=1, Hq=Hq, Hk=Hk,
                                          before=[n - 1 for n in seq_lens],
                                          counts=[1] * B, seed=seed)
    return q[:, 0].contiguous(), kc, vc, bt, before + 1


def direct_write_lens():
    g = torch.Generator().manual_seed(14)
    return torch.randint(1, 201, (64,), generator=g).tolist()


def _check(C, case):
    from paddlenlp_amd.experimental.fused_transformer import paged_decode_attn_ref

    q, kc, vc, bt, seq_lens = case
    out = C.paged_decode_attn(q.cuda(), kc.cuda(), vc.cuda(), bt.cuda(),
                              seq_lens.cuda()).cpu()
    ref = paged_decode_attn_ref(q, kc, vc, bt, seq_lens)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()
    err = (out.float() - ref.float()).abs().max()
    print(f"max abs err {err:.4g}")
    assert torch.allclose(out.float(), ref.float(), atol=3e-2, rtol=3e-2), err


@pytest.mark.parametrize("Hq,Hk", [(16, 1), (7, 1), (4, 4)])
def test_split_and_merge(C, Hq, Hk):
    """B*Hk is 6 or 24, so nsplit > 1 (64 or 22): short sequences leave most
    splits empty, the partials go through paged_decode_merge_kernel<128>.
    G = 16 fills the MFMA N dimension, G = 7 and G = 1 leave idle columns."""
    _check(C, decode_case(Hq, Hk, SPLIT_LENS, seed=10 + Hq))


def test_direct_write(C):
    """B*Hk = 512 workgroups: nsplit == 1, each workgroup runs its whole
    sequence (1..200 tokens, up to two V tiles), merges its four waves and
    writes the output itself."""
    _check(C, decode_case(8, 8, direct_write_lens(), seed=14))
