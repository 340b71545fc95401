"""CPU checks of weight-only int8 MoE experts: the packer
(quantization.quantize_moe_int8), the oracle (ops.reference.moe_ffn_wint8) the
GPU kernels are tested against, the dispatching op off the GPU, and the
engine's quantize() / _moe_ffn on a tiny fp32 Mixtral."""
import os
import sys

import pytest
import torch

from paddlenlp_amd import ops
from paddlenlp_amd.ops import reference
from paddlenlp_amd.quantization import (
    dequantize_moe_int8, quantize_int8, quantize_moe_int8)


def test_packer_shapes_and_rounding_bound():
    torch.manual_seed(0)
    w = torch.randn(4, 32, 48)
    w[1, :, 7] = 0.0                     # an all-zero column
    q, s = quantize_moe_int8(w)
    assert q.shape == (4, 48, 32) and q.dtype == torch.int8 and q.is_contiguous()
    assert s.shape == (4, 48) and s.dtype == torch.float32
    assert int(q.abs().max()) <= 127
    back = dequantize_moe_int8(q, s, torch.float32)
    assert back.shape == w.shape and back.dtype == torch.float32
    # the rounding bound of a symmetric quantizer, per (expert, column)
    bound = 0.5 * s[:, None, :] * (1 + 1e-6)
    assert ((back - w).abs() <= bound).all(), ((back - w).abs() - bound).max()
    assert (q[1, 7] == 0).all() and torch.isfinite(s[1, 7]) and s[1, 7] > 0
    assert dequantize_moe_int8(q, s, torch.bfloat16).dtype == torch.bfloat16


def test_packer_follows_quantize_int8():
    """Per expert it is quantize_int8 of the transposed matrix."""
    torch.manual_seed(1)
    w = torch.randn(3, 16, 24)
    q, s = quantize_moe_int8(w)
    for e in range(3):
        qe, se = quantize_int8(w[e].t().contiguous())
        assert torch.equal(q[e], qe) and torch.equal(s[e], se)


def _packed_case(seed, T=7, H=32, I=48, E=4):
    torch.manual_seed(seed)
    x = torch.randn(T, H)
    w1 = torch.randn(E, H, I) / H ** 0.5
    w3 = torch.randn(E, H, I) / H ** 0.5
    w2 = torch.randn(E, I, H) / I ** 0.5
    packed = []
    for w in (w1, w3, w2):
        packed += list(quantize_moe_int8(w))
    return x, packed


def test_oracle_is_moe_ffn_on_dequantized_weights():
    x, (q1, s1, q3, s3, q2, s2) = _packed_case(2)
    logits = torch.randn(x.shape[0], 4)
    got = reference.moe_ffn_wint8(x, logits, q1, s1, q3, s3, q2, s2, 2)
    want = reference.moe_ffn(x, logits, dequantize_moe_int8(q1, s1, torch.float32),
                             dequantize_moe_int8(q3, s3, torch.float32),
                             dequantize_moe_int8(q2, s2, torch.float32), 2)
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert torch.equal(got, want)


def test_oracle_skips_unselected_experts():
    x, (q1, s1, q3, s3, q2, s2) = _packed_case(3, T=3)
    logits = torch.tensor([[3.0, 2.0, 0.0, -1.0]]).repeat(3, 1)   # experts 0, 1
    want = reference.moe_ffn_wint8(x, logits, q1, s1, q3, s3, q2, s2, 2)
    for s in (s1, s3, s2):
        s[2:] = float("nan")
    got = reference.moe_ffn_wint8(x, logits, q1, s1, q3, s3, q2, s2, 2)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_op_on_cpu_is_the_oracle(dtype):
    x, (q1, s1, q3, s3, q2, s2) = _packed_case(4)
    x = x.to(dtype)
    logits = torch.randn(x.shape[0], 4)
    args = (x, logits, q1, s1, q3, s3, q2, s2, 2)
    assert not ops.moe_ffn_wint8_supported(*args)
    out = ops.moe_ffn_wint8(*args)
    assert out.dtype == dtype
    assert torch.equal(out, reference.moe_ffn_wint8(*args).to(dtype))


# ---------------------------------------------------------------------------
# engine (the tiny fp32 Mixtral config of test_moe_ffn_ref.py)
# ---------------------------------------------------------------------------
def _tiny_mixtral(seed=13):
    from paddlenlp_amd.transformers.mixtral import MixtralConfig, MixtralForCausalLM

    torch.manual_seed(seed)
    cfg = MixtralConfig(
        vocab_size=128, hidden_size=64, intermediate_size=96,
        num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
        num_local_experts=4, num_experts_per_tok=2,
        max_position_embeddings=64, dtype="float32",
    )
    model = MixtralForCausalLM.from_config(cfg)
    model.eval()
    return model


def _engine(model):
    from paddlenlp_amd.experimental import FusedMultiTransformer

    return FusedMultiTransformer.from_model(model, block_size=4, max_seq_len=64)


def test_engine_quantize_packs_and_frees_experts():
    eng = _engine(_tiny_mixtral())
    gates = [g.data.clone() for g in eng.moe_gates]
    w1 = [w.data.clone() for w in eng.moe_w1]
    eng.quantize("weight_only_int8")
    assert eng.quant_algo == "weight_only_int8"
    for name, shape in (("moe_w1", (4, 96, 64)), ("moe_w3", (4, 96, 64)),
                        ("moe_w2", (4, 64, 96))):
        assert len(eng._qw[name]) == 2
        for i, (q, s) in enumerate(eng._qw[name]):
            assert q.dtype == torch.int8 and tuple(q.shape) == shape
            assert s.dtype == torch.float32 and tuple(s.shape) == shape[:2]
            assert getattr(eng, name)[i].numel() == 1      # bf16 copy freed
    for i in range(2):
        want_q, want_s = quantize_moe_int8(w1[i])
        assert torch.equal(eng._qw["moe_w1"][i][0], want_q)
        assert torch.equal(eng._qw["moe_w1"][i][1], want_s)
        assert torch.equal(eng.moe_gates[i].data, gates[i])   # router untouched
    # the attention projections are quantized as before
    assert "qkv_weights" in eng._qw and "out_proj_weights" in eng._qw


def test_engine_moe_ffn_matches_oracle_on_packed_experts():
    """fp32 on both sides; they differ only in summation order -> atol 1e-5."""
    eng = _engine(_tiny_mixtral())
    eng.quantize("weight_only_int8")
    torch.manual_seed(5)
    h = torch.randn(2, 5, 64)
    x = h.reshape(-1, 64)
    for i in range(2):
        (q1, s1), (q3, s3), (q2, s2) = (eng._qw[n][i] for n in ("moe_w1", "moe_w3", "moe_w2"))
        want = reference.moe_ffn_wint8(x, x @ eng.moe_gates[i].t(), q1, s1, q3, s3,
                                       q2, s2, 2)
        for impl in ("auto", "torch"):
            eng.moe_impl = impl
            got = eng._moe_ffn(h, i)
            assert got.shape == h.shape
            assert torch.allclose(got.reshape(-1, 64), want, atol=1e-5), \
                (got.reshape(-1, 64) - want).abs().max()


def test_engine_names_select_the_experts_only():
    eng = _engine(_tiny_mixtral())
    eng.quantize("weight_only_int8", names=("moe_experts",))
    assert sorted(eng._qw) == ["moe_w1", "moe_w2", "moe_w3"]
    assert eng.qkv_weights[0].numel() > 1


def test_engine_fp8_leaves_experts_alone():
    eng = _engine(_tiny_mixtral())
    w1 = [w.data.clone() for w in eng.moe_w1]
    eng.quantize("fp8")
    assert not any(n.startswith("moe_") for n in eng._qw)
    for i in range(2):
        assert torch.equal(eng.moe_w1[i].data, w1[i])
    with pytest.raises(ValueError):
        _engine(_tiny_mixtral()).quantize("fp8", names=("moe_experts",))


def test_dense_engine_refuses_moe_experts():
    from paddlenlp_amd.transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=64, hidden_size=32, intermediate_size=64,
                      num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
                      max_position_embeddings=64, dtype="float32")
    eng = _engine(LlamaForCausalLM.from_config(cfg))
    with pytest.raises(ValueError):
        eng.quantize("weight_only_int8", names=("moe_experts",))
    eng.quantize("weight_only_int8")          # the default set has no experts here
    assert not any(n.startswith("moe_") for n in eng._qw)


def test_engine_quantized_prefill_close_to_unquantized():
    """The criterion of test_engine_quantized_decode: max|delta| / max|logits| < 0.2."""
    from paddlenlp_amd.experimental import BlockManager

    model = _tiny_mixtral()
    torch.manual_seed(7)
    ids = torch.randint(3, 128, (2, 9))
    lens = torch.tensor([9, 9], dtype=torch.int32)
    logits = []
    for quant in (False, True):
        eng = _engine(model)
        if quant:
            eng.quantize("weight_only_int8")
        eng.allocate_caches(num_blocks=16, device="cpu")
        mgr = BlockManager(16, 4, 8, 2)
        slots = [mgr.allocate_slot(9) for _ in range(2)]
        bt = torch.stack([mgr.block_table[s] for s in slots]).to(torch.int32)
        logits.append(eng.prefill(ids, bt, lens).float())
    ref, got = logits
    assert torch.isfinite(got).all()
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"tiny mixtral int8 prefill: max|delta| / max|logits| = {rel:.4f}")
    assert rel < 0.2, rel


def test_predictor_quant_type_reaches_the_experts():
    """llm/predict/predictor.py: quant_type weight_only_int8 on a Mixtral."""
    sys.path.insert(0, os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llm", "predict"))
    import importlib

    import predictor as predictor_mod
    from tokenizers import Tokenizer, models, pre_tokenizers

    from paddlenlp_amd.transformers.tokenizer_utils import PretrainedTokenizer

    importlib.reload(predictor_mod)
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2}
    for i, w in enumerate("the quick brown fox jumps over lazy dog a and".split()):
        vocab[w] = 3 + i
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    tok = PretrainedTokenizer(tokenizer=tok, bos_token="<s>", eos_token="</s>",
                              pad_token="</s>", unk_token="<unk>")
    args = predictor_mod.PredictorArgument(
        batch_size=2, block_size=4, max_length=4, src_length=16,
        total_max_length=64, decode_strategy="greedy", dtype="float32",
        quant_type="weight_only_int8",
    )
    pred = predictor_mod.create_predictor(args, model=_tiny_mixtral(), tokenizer=tok)
    assert isinstance(pred, predictor_mod.BlockInferencePredictor)
    assert "moe_w1" in pred.engine._qw
    outs = pred.predict(["the quick brown fox", "lazy dog"])
    assert len(outs) == 2 and all(isinstance(o, str) for o in outs)
