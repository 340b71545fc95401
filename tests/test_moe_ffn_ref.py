"""CPU checks of the routed-FFN oracles in ops.reference (moe_route, moe_ffn),
which the GPU kernels of moe_ffn.hip are tested against."""
import torch
import torch.nn.functional as F

from paddlenlp_amd import ops
from paddlenlp_amd.ops import reference


def test_reference_moe_ffn_matches_dense_expert_loop():
    """fp32 on both sides; they differ only in summation order -> atol 1e-5."""
    torch.manual_seed(0)
    T, H, I, E, K = 7, 32, 48, 4, 2
    x = torch.randn(T, H)
    logits = torch.randn(T, E)
    w1 = torch.randn(E, H, I) / H ** 0.5
    w3 = torch.randn(E, H, I) / H ** 0.5
    w2 = torch.randn(E, I, H) / I ** 0.5

    # dense: every expert on every token, weighted by a [T, E] gate matrix
    probs = logits.softmax(-1)
    topw, tope = probs.topk(K, dim=-1)
    gate = torch.zeros(T, E).scatter_(1, tope, topw / topw.sum(-1, keepdim=True))
    want = torch.zeros(T, H)
    for e in range(E):
        y = (F.silu(x @ w1[e]) * (x @ w3[e])) @ w2[e]
        want += gate[:, e, None] * y

    got = reference.moe_ffn(x, logits, w1, w3, w2, K)
    assert got.dtype == torch.float32 and got.shape == (T, H)
    assert torch.allclose(got, want, atol=1e-5), (got - want).abs().max()
    # the dispatching op takes the reference off the GPU and keeps x.dtype
    out = ops.moe_ffn(x, logits, w1, w3, w2, K)
    assert out.dtype == x.dtype
    assert torch.equal(out, got)


def test_reference_moe_ffn_skips_unselected_experts():
    torch.manual_seed(1)
    T, H, I, E, K = 3, 32, 48, 4, 2
    x = torch.randn(T, H)
    logits = torch.tensor([[3.0, 2.0, 0.0, -1.0]]).repeat(T, 1)   # experts 0, 1
    w1 = torch.randn(E, H, I) / H ** 0.5
    w3 = torch.randn(E, H, I) / H ** 0.5
    w2 = torch.randn(E, I, H) / I ** 0.5
    want = reference.moe_ffn(x, logits, w1, w3, w2, K)
    for w in (w1, w3, w2):
        w[2:] = float("nan")
    got = reference.moe_ffn(x, logits, w1, w3, w2, K)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


def test_reference_moe_ffn_matches_engine_moe_ffn():
    """The engine's capacity-padded torch path (tiny Mixtral config of
    test_inference_engine.py, CPU fp32) computes the same function."""
    from paddlenlp_amd.experimental import FusedMultiTransformer
    from paddlenlp_amd.transformers.mixtral import MixtralConfig, MixtralForCausalLM

    torch.manual_seed(13)
    cfg = MixtralConfig(
        vocab_size=128, hidden_size=64, intermediate_size=96,
        num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
        num_local_experts=4, num_experts_per_tok=2,
        max_position_embeddings=64, dtype="float32",
    )
    model = MixtralForCausalLM.from_config(cfg)
    eng = FusedMultiTransformer.from_model(model, block_size=4, max_seq_len=64)
    assert eng.moe_impl == "auto" and eng.moe_fused_max_tokens > 0
    h = torch.randn(2, 5, 64)
    for i in range(2):
        got = eng._moe_ffn(h, i)
        x = h.reshape(-1, 64)
        want = reference.moe_ffn(x, x @ eng.moe_gates[i].t(), eng.moe_w1[i],
                                 eng.moe_w3[i], eng.moe_w2[i], 2)
        assert got.shape == h.shape
        assert torch.allclose(got.reshape(-1, 64), want, atol=1e-5), \
            (got.reshape(-1, 64) - want).abs().max()


def test_reference_moe_route_tie_rule():
    """All-equal logits: experts 0..K-1, weights 1/K (lower index wins)."""
    for E, K in ((8, 2), (4, 1), (16, 4)):
        ids, w = reference.moe_route(torch.full((3, E), 0.25), K)
        assert ids.dtype == torch.int32 and w.dtype == torch.float32
        assert torch.equal(ids, torch.arange(K, dtype=torch.int32).expand(3, K))
        assert torch.allclose(w, torch.full((3, K), 1.0 / K), atol=1e-7)
    # partial tie: 1 and 3 tie for the top, 0 and 2 for the rest
    ids, w = reference.moe_route(torch.tensor([[0.0, 1.0, 0.0, 1.0]]), 3)
    assert ids.tolist() == [[1, 3, 0]]
    assert w[0, 0] == w[0, 1] and w[0, 1] > w[0, 2]
    assert abs(float(w.sum()) - 1.0) < 1e-6
    # the dispatching op is the reference off the GPU
    ids2, w2 = ops.moe_route(torch.tensor([[0.0, 1.0, 0.0, 1.0]]), 3)
    assert torch.equal(ids2, ids) and torch.equal(w2, w)


def test_reference_moe_route_matches_topk_without_ties():
    torch.manual_seed(2)
    logits = torch.randn(33, 8)
    ids, w = reference.moe_route(logits, 2)
    topw, tope = logits.softmax(-1).topk(2, dim=-1)
    assert torch.equal(ids.long(), tope)
    assert torch.allclose(w, topw / topw.sum(-1, keepdim=True), atol=1e-7)
