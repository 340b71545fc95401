"""Paged append attention on the CPU paths: the oracle against dense causal
attention, engine.extend / chunked prefill against the dygraph model, and the
predictor's prefill_chunk_size."""
import importlib
import os
import sys

import pytest
import torch

from paddlenlp_amd.experimental import BlockManager, FusedMultiTransformer
from paddlenlp_amd.experimental.fused_transformer import paged_append_attn_ref
from paddlenlp_amd.ops import reference
from paddlenlp_amd.transformers import LlamaConfig, LlamaForCausalLM


def tiny_llama(seed=0):
    # the model of tests/test_inference_engine.py
    torch.manual_seed(seed)
    cfg = LlamaConfig(
        vocab_size=128, hidden_size=64, intermediate_size=128,
        num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
        max_position_embeddings=256, dtype="float32", eos_token_id=2,
    )
    m = LlamaForCausalLM.from_config(cfg)
    m.eval()
    return m


# ---------------------------------------------------------------------------
# oracle vs dense attention
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("before,counts", [
    ([0, 0], [6, 6]),        # empty prefix: plain causal attention
    ([5, 9], [6, 6]),        # prefixes that are no multiple of the block size
    ([5, 0], [3, 0]),        # token_counts < T, one sequence with none
])
def test_oracle_matches_dense_attention(before, counts):
    g = torch.Generator().manual_seed(0)
    B, T, Hq, Hk, D, bs, nblk, maxb = 2, 6, 4, 2, 16, 4, 16, 5
    q = torch.randn(B, T, Hq, D, generator=g)
    k_cache = torch.randn(nblk, bs, Hk, D, generator=g)
    v_cache = torch.randn(nblk, bs, Hk, D, generator=g)
    bt = torch.randperm(nblk, generator=g)[:B * maxb].view(B, maxb).to(torch.int32)
    before_t = torch.tensor(before, dtype=torch.int32)
    counts_t = torch.tensor(counts, dtype=torch.int32)

    out = paged_append_attn_ref(q, k_cache, v_cache, bt, before_t, counts_t)
    assert out.shape == q.shape
    for b in range(B):
        n, L = counts[b], before[b] + counts[b]
        assert torch.equal(out[b, n:], torch.zeros_like(out[b, n:]))
        if n == 0:
            continue
        k = k_cache[bt[b].long()].reshape(-1, Hk, D)[:L]
        v = v_cache[bt[b].long()].reshape(-1, Hk, D)[:L]
        if before[b] == 0:
            ref = reference.flash_attention(q[b:b + 1, :n], k[None], v[None], causal=True)
        else:
            # queries are the last n rows of a causal [L, L] problem
            qfull = torch.cat([torch.zeros(before[b], Hq, D), q[b, :n]])[None]
            ref = reference.flash_attention(qfull, k[None], v[None], causal=True)[:, before[b]:]
        assert torch.allclose(out[b, :n], ref[0], atol=1e-5), (out[b, :n] - ref[0]).abs().max()

    if counts == [6, 6]:
        # token_counts=None means all T tokens
        out2 = paged_append_attn_ref(q, k_cache, v_cache, bt, before_t)
        assert torch.equal(out, out2)


# ---------------------------------------------------------------------------
# engine: extend and chunked prefill vs one-shot prefill / dygraph
# ---------------------------------------------------------------------------
def _setup(model, lens_list, T):
    eng = FusedMultiTransformer.from_llama(model, block_size=4, max_seq_len=64)
    eng.allocate_caches(num_blocks=32, device="cpu")
    B = len(lens_list)
    ids = torch.randint(3, 128, (B, T), generator=torch.Generator().manual_seed(1))
    lens = torch.tensor(lens_list, dtype=torch.int32)
    mgr = BlockManager(32, 4, 16, B)
    bt = torch.stack([mgr.block_table[mgr.allocate_slot(n)] for n in lens_list]).to(torch.int32)
    return eng, ids, lens, bt


def _cached(eng, bt, lens):
    """Per layer, the cached K/V of every sequence's valid positions."""
    out = []
    for kc, vc in zip(eng.k_caches, eng.v_caches):
        for b in range(bt.shape[0]):
            L = int(lens[b])
            out.append(kc[bt[b].long()].reshape(-1, *kc.shape[2:])[:L].clone())
            out.append(vc[bt[b].long()].reshape(-1, *vc.shape[2:])[:L].clone())
    return out


@pytest.fixture(scope="module")
def prefill_case():
    model = tiny_llama()
    eng, ids, lens, bt = _setup(model, [10, 7], 10)
    eng.prefill(ids, bt, lens)
    with torch.no_grad():
        ref_full = model(input_ids=ids).float()
    return model, ids, lens, bt, ref_full, _cached(eng, bt, lens)


def _check_last(logits, ref_full, lens):
    for b in range(len(lens)):
        ref = ref_full[b, int(lens[b]) - 1]
        assert torch.allclose(logits[b], ref, atol=1e-3), (b, (logits[b] - ref).abs().max())


def test_prefill_then_extend_matches_dygraph(prefill_case):
    model, ids, lens, bt, ref_full, caches = prefill_case
    eng, _, _, _ = _setup(model, [10, 7], 10)
    four = torch.tensor([4, 4], dtype=torch.int32)
    eng.prefill(ids[:, :4], bt, four)
    logits = eng.extend(ids[:, 4:], bt, four, torch.tensor([6, 3], dtype=torch.int32))
    _check_last(logits, ref_full, lens)
    for got, want in zip(_cached(eng, bt, lens), caches):
        assert torch.allclose(got, want, atol=1e-5)


def test_chunked_prefill_matches_dygraph(prefill_case):
    model, ids, lens, bt, ref_full, caches = prefill_case
    eng, _, _, _ = _setup(model, [10, 7], 10)
    logits = eng.prefill(ids, bt, lens, chunk_size=4)
    _check_last(logits, ref_full, lens)
    for got, want in zip(_cached(eng, bt, lens), caches):
        assert torch.allclose(got, want, atol=1e-5)


def test_extend_all_logits(prefill_case):
    model, ids, lens, bt, ref_full, _ = prefill_case
    eng, _, _, _ = _setup(model, [10, 7], 10)
    four = torch.tensor([4, 4], dtype=torch.int32)
    counts = [6, 3]
    eng.prefill(ids[:, :4], bt, four)
    logits = eng.extend(ids[:, 4:], bt, four, torch.tensor(counts, dtype=torch.int32),
                        all_logits=True)
    assert logits.shape == (2, 6, 128)
    assert torch.isfinite(logits).all()
    for b in range(2):
        got, ref = logits[b, :counts[b]], ref_full[b, 4:4 + counts[b]]
        assert torch.allclose(got, ref, atol=1e-3), (b, (got - ref).abs().max())


def test_extend_zero_count_writes_nothing():
    model = tiny_llama()
    eng, ids, lens, bt = _setup(model, [10, 7], 10)
    four = torch.tensor([4, 4], dtype=torch.int32)
    eng.prefill(ids[:, :4], bt, four)
    k0 = [k.clone() for k in eng.k_caches]
    logits = eng.extend(ids[:, 4:], bt, four, torch.tensor([6, 0], dtype=torch.int32))
    assert torch.isfinite(logits).all()
    # sequence 1 appended nothing: its blocks are untouched
    for k_new, k_old in zip(eng.k_caches, k0):
        assert torch.equal(k_new[bt[1, :2].long()], k_old[bt[1, :2].long()])


# ---------------------------------------------------------------------------
# predictor
# ---------------------------------------------------------------------------
def _make_tiny_tokenizer():
    # the tokenizer of tests/test_inference_engine.py
    from tokenizers import Tokenizer, models, pre_tokenizers

    from paddlenlp_amd.transformers.tokenizer_utils import PretrainedTokenizer

    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2}
    for i, w in enumerate("the quick brown fox jumps over lazy dog a and".split()):
        vocab[w] = 3 + i
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    return PretrainedTokenizer(tokenizer=tok, bos_token="<s>", eos_token="</s>",
                               pad_token="</s>", unk_token="<unk>")


def test_predictor_prefill_chunk_size():
    sys.path.insert(0, os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llm", "predict"))
    import predictor as predictor_mod

    importlib.reload(predictor_mod)
    tok = _make_tiny_tokenizer()
    torch.manual_seed(0)
    cfg = LlamaConfig(
        vocab_size=16, hidden_size=32, intermediate_size=64,
        num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
        max_position_embeddings=128, dtype="float32", eos_token_id=2,
    )
    model = LlamaForCausalLM.from_config(cfg)
    model.eval()
    assert predictor_mod.PredictorArgument().prefill_chunk_size == 0

    texts = ["the quick brown fox jumps over the lazy dog", "lazy dog", "a and the"]
    outs = {}
    for chunk in (0, 4):
        args = predictor_mod.PredictorArgument(
            batch_size=2, block_size=4, max_length=6, src_length=16,
            total_max_length=64, decode_strategy="greedy", dtype="float32",
            prefill_chunk_size=chunk,
        )
        pred = predictor_mod.create_predictor(args, model=model, tokenizer=tok)
        outs[chunk] = pred.predict(texts)
    assert outs[4] == outs[0], outs
