"""GPU tests of the fused MoE FFN over weight-only int8 experts
(moe_gemm_wint8_kernel in moe_ffn.hip, ops.moe_ffn_wint8) and of the Mixtral
engine with quantized experts.

The cases are built the way tests/test_moe_ffn_gpu.py builds them: H = 256,
I = 384 (more than one 128-wide tile and more than one 128-deep chunk in both
GEMMs), constructed router logits (a permutation of 0.4 * arange(E) plus noise
of at most 0.05, gap asserted on the CPU), bf16 x = 2 * randn, weights
randn / sqrt(fan_in) packed with quantize_moe_int8.  Experts no token selects
get NaN scales and random bytes.

Numerics: e_fused <= 1.5 * e_torch, both max-abs differences from the fp32
oracle (ops.reference.moe_ffn_wint8, CPU); e_torch is the plain bf16 torch
formulation on the GPU over the weights dequantized to bf16.  The int8 kernel
rounds where the bf16 kernel rounds (activation to bf16, output), its weights
are exact; 1.5 is the project's margin for the scatter of a max over a sample.
Measured on MI355X: see profiles/moe_ffn_wint8.md.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H, I = 256, 384


@pytest.fixture(scope="module")
def C():
    from paddlenlp_amd.ops.functional import _load_extension

    return _load_extension()


def _logits_from_prefs(prefs, E, gen):
    """prefs[t]: a permutation of range(E), most preferred expert first."""
    T = len(prefs)
    logits = torch.empty(T, E)
    ladder = 0.4 * torch.arange(E - 1, -1, -1, dtype=torch.float32)
    for t, p in enumerate(prefs):
        assert sorted(p) == list(range(E))
        logits[t, torch.tensor(p)] = ladder
    logits += (torch.rand(T, E, generator=gen) * 2 - 1) * 0.05
    return logits


def _assert_gap(logits, K):
    """The top-(K+1) probabilities of every token are distinct by a wide
    margin (ratio of neighbours > 1.2), on the CPU, before the logits are used."""
    p = logits.float().softmax(-1).sort(-1, descending=True).values[:, :K + 1]
    assert (p[:, :-1] / p[:, 1:] > 1.2).all()


def _prefs_with_top(top, E, gen):
    rest = [e for e in torch.randperm(E, generator=gen).tolist() if e not in top]
    return list(top) + rest


_SEEDS = dict(t1_nan=21, t5_same_two=22, t40_skewed=23, t64_permuted=24,
              t9_e4_k1=25, t9_e16_k4=26, t3_all_equal=27, t5_h128_one_chunk=28,
              t9_extreme_bytes=29)
CASES = list(_SEEDS)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> dict(x, logits and the packed experts on the GPU, K, the fp32
    oracle on the CPU); built once per case and shared, never modified."""
    from paddlenlp_amd.ops import reference
    from paddlenlp_amd.quantization import quantize_moe_int8

    gen = torch.Generator().manual_seed(_SEEDS[name])
    E, K, h, i = 8, 2, H, I
    unused = []
    if name == "t1_nan":
        T = 1
        prefs = [_prefs_with_top((5, 2), E, gen)]
        unused = [0, 1, 3, 4, 6, 7]
    elif name == "t5_same_two":
        T = 5
        prefs = [_prefs_with_top((3, 6) if t % 2 else (6, 3), E, gen) for t in range(T)]
        unused = [0, 1, 2, 4, 5, 7]
    elif name == "t40_skewed":
        # expert 2: 33 rows (two row tiles, the second holding one row),
        # expert 6: exactly 32, experts 0/4/7 share the other 15, 1/3/5 none
        T = 40
        tops = [(2, 6) if t % 3 else (6, 2) for t in range(32)] + [(0, 2)]
        tops += [(0, 4), (4, 7), (7, 0), (4, 0), (7, 4), (0, 7), (4, 7)]
        prefs = []
        for top in tops:
            rest = [e for e in (0, 4, 7) if e not in top]
            prefs.append(list(top) + rest + [e for e in (2, 6) if e not in top] + [1, 3, 5])
        unused = [1, 3, 5]
    elif name == "t64_permuted":
        T = 64
        prefs = [torch.randperm(E, generator=gen).tolist() for _ in range(T)]
    elif name == "t9_e4_k1":
        T, E, K = 9, 4, 1
        prefs = [torch.randperm(E, generator=gen).tolist() for _ in range(T)]
    elif name == "t9_e16_k4":
        T, E, K = 9, 16, 4
        prefs = [torch.randperm(E, generator=gen).tolist() for _ in range(T)]
    elif name == "t3_all_equal":
        T = 3
        prefs = None
        unused = [2, 3, 4, 5, 6, 7]       # the tie rule picks experts 0 and 1
    elif name == "t5_h128_one_chunk":
        # one 128-deep chunk in both GEMMs: the loop body runs once, right
        # after the prologue, and nothing is prefetched inside it
        T, h, i = 5, 128, 128
        prefs = [torch.randperm(E, generator=gen).tolist() for _ in range(T)]
    elif name == "t9_extreme_bytes":
        T = 9
        prefs = [torch.randperm(E, generator=gen).tolist() for _ in range(T)]
    else:
        raise KeyError(name)
    if prefs is None:
        logits = torch.full((T, E), 0.5)
    else:
        logits = _logits_from_prefs(prefs, E, gen)
        _assert_gap(logits, K)
    ids, _ = reference.moe_route(logits, K)
    used = set(ids.reshape(-1).tolist())
    assert not used & set(unused)
    if name == "t40_skewed":
        counts = torch.bincount(ids.reshape(-1).long(), minlength=E).tolist()
        assert counts[2] == 33 and counts[6] == 32
    if name in ("t1_nan", "t5_same_two", "t3_all_equal"):
        assert len(unused) == E - 2

    x = (2.0 * torch.randn(T, h, generator=gen)).to(torch.bfloat16)
    packed = {}
    for key, shape, fan_in in (("1", (E, h, i), h), ("3", (E, h, i), h), ("2", (E, i, h), i)):
        w = torch.randn(shape, generator=gen) / fan_in ** 0.5
        q, s = quantize_moe_int8(w)
        if name == "t9_extreme_bytes":
            # -128 (which the packer never emits) and +127 in every selected
            # expert, one byte in sixteen each
            hit = torch.rand(q.shape, generator=gen)
            q[hit < 1 / 16] = -128
            q[hit > 15 / 16] = 127
            assert (q[sorted(used)] == -128).any()
        if unused:
            q[unused] = torch.randint(-128, 128, q[unused].shape, generator=gen,
                                      dtype=torch.int8)
            s[unused] = float("nan")
        packed["q" + key], packed["s" + key] = q, s
    oracle = reference.moe_ffn_wint8(x, logits, packed["q1"], packed["s1"], packed["q3"],
                                     packed["s3"], packed["q2"], packed["s2"], K)
    assert torch.isfinite(oracle).all()
    dev = {k: v.cuda() for k, v in dict(x=x, logits=logits, **packed).items()}
    return dict(K=K, E=E, T=T, H=h, oracle=oracle, **dev)


def _args(c):
    return (c["x"], c["logits"], c["q1"], c["s1"], c["q3"], c["s3"], c["q2"], c["s2"],
            c["K"])


def _torch_bf16_moe(c):
    """The plain bf16 formulation on the GPU over the experts dequantized to
    bf16: per selected expert (silu(x@w1[e]) * (x@w3[e])) @ w2[e], weighted
    and summed in bf16."""
    from paddlenlp_amd.ops import reference
    from paddlenlp_amd.quantization import dequantize_moe_int8

    x = c["x"]
    w1, w3, w2 = (dequantize_moe_int8(c["q" + k], c["s" + k], torch.bfloat16)
                  for k in "132")
    ids, w = reference.moe_route(c["logits"], c["K"])
    w = w.to(x.dtype)
    out = torch.zeros_like(x)
    for k in range(c["K"]):
        for e in torch.unique(ids[:, k]).tolist():
            rows = (ids[:, k] == e).nonzero(as_tuple=True)[0]
            xe = x[rows]
            y = (F.silu(xe @ w1[e]) * (xe @ w3[e])) @ w2[e]
            out[rows] += y * w[rows, k, None]
    return out


@pytest.mark.parametrize("name", CASES)
def test_moe_ffn_wint8_matches_oracle(C, name):
    from paddlenlp_amd import ops

    c = _case(name)
    assert ops.moe_ffn_wint8_supported(*_args(c))
    out = ops.moe_ffn_wint8(*_args(c))
    assert out.shape == (c["T"], c["H"]) and out.dtype == torch.bfloat16
    assert torch.isfinite(out).all()
    e_fused = (out.float().cpu() - c["oracle"]).abs().max().item()
    e_torch = (_torch_bf16_moe(c).float().cpu() - c["oracle"]).abs().max().item()
    print(f"moe_ffn_wint8 {name}: |oracle|max={c['oracle'].abs().max().item():.3f} "
          f"e_fused={e_fused:.3e} e_torch={e_torch:.3e}")
    assert e_fused <= 1.5 * e_torch, (e_fused, e_torch)


def test_moe_ffn_wint8_deterministic(C):
    c = _case("t40_skewed")
    a = C.moe_ffn_wint8(*_args(c))
    b = C.moe_ffn_wint8(*_args(c))
    assert torch.equal(a, b)


def _refused(C, args):
    from paddlenlp_amd import ops

    assert not ops.moe_ffn_wint8_supported(*args)
    with pytest.raises(RuntimeError):
        C.moe_ffn_wint8(*args)


def test_moe_ffn_wint8_refuses_unsupported_arguments(C):
    c = _case("t5_same_two")
    x, logits, q1, s1, q3, s3, q2, s2, K = _args(c)
    # H = 64
    _refused(C, (x[:, :64].contiguous(), logits, q1[:, :, :64].contiguous(), s1,
                 q3[:, :, :64].contiguous(), s3, q2[:, :64].contiguous(),
                 s2[:, :64].contiguous(), K))
    # a non-contiguous q of the right shape
    wide = torch.zeros(q1.shape[0], q1.shape[1], 2 * q1.shape[2], dtype=torch.int8,
                       device="cuda")
    q1_nc = wide[:, :, ::2]
    assert q1_nc.shape == q1.shape and not q1_nc.is_contiguous()
    _refused(C, (x, logits, q1_nc, s1, q3, s3, q2, s2, K))
    # a bf16 scale
    _refused(C, (x, logits, q1, s1.bfloat16(), q3, s3, q2, s2, K))
    # a scale of the wrong shape
    _refused(C, (x, logits, q1, s1, q3, s3, q2, s2[:, :-1].contiguous(), K))
    _refused(C, (x, logits, q1, s1, q3, s3.t().contiguous(), q2, s2, K))


def test_down_split_functions(C):
    """The int8 split counts 128-deep chunks: every split is non-empty and
    together they cover all chunks.  The bf16 function is unchanged: values
    computed by the code before the int8 path existed."""
    n = 0
    for T in (1, 2, 5, 16, 33, 64, 100, 256, 512, 1024, 2048, 4096):
        for K in (1, 2, 4, 8):
            if T * K > 4096:
                continue
            for Hh in (128, 256, 1664, 4096):
                for Ii in (128, 384, 640, 896, 14336):
                    ks = C.moe_down_ksplit_wint8(T, K, Hh, Ii)
                    nch = Ii // 128
                    assert 1 <= ks <= nch, (T, K, Hh, Ii, ks)
                    per = (nch + ks - 1) // ks         # what the launcher gives a split
                    assert (ks - 1) * per < nch <= ks * per, (T, K, Hh, Ii, ks)
                    n += 1
    assert n > 500
    pinned = {(1, 2, 4096, 14336): 8, (16, 2, 4096, 14336): 8, (64, 2, 4096, 14336): 2,
              (256, 2, 4096, 14336): 1, (48, 2, 4096, 14336): 3, (5, 2, 256, 384): 6,
              (40, 2, 256, 384): 6, (1, 2, 1024, 640): 10, (100, 1, 1664, 640): 5,
              (3, 2, 128, 896): 14}
    for shape, want in pinned.items():
        assert C.moe_down_ksplit(*shape) == want, shape


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------
ENGINE_SEED = 3


def _mixtral_engine(seed, quantize=True):
    from paddlenlp_amd.experimental import FusedMultiTransformer
    from paddlenlp_amd.transformers.mixtral import MixtralConfig, MixtralForCausalLM

    torch.manual_seed(seed)
    cfg = MixtralConfig(
        vocab_size=512, hidden_size=256, intermediate_size=384,
        num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
        num_local_experts=8, num_experts_per_tok=2,
        max_position_embeddings=256,
    )
    model = MixtralForCausalLM.from_config(cfg, dtype=torch.bfloat16, device="cuda")
    model.eval()
    eng = FusedMultiTransformer.from_mixtral(model, block_size=16, max_seq_len=256).to("cuda")
    del model
    if quantize:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        eng.quantize("weight_only_int8")
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated()
        experts_bf16 = 2 * 3 * 8 * 256 * 384 * 2
        print(f"mixtral test engine memory_allocated: {before} -> {after} bytes "
              f"(bf16 experts {experts_bf16} bytes)")
    eng.allocate_caches(num_blocks=64, device="cuda")
    return eng


def _spy(monkeypatch, name):
    from paddlenlp_amd import ops

    calls = []
    real = getattr(ops, name)

    def spy(*a, **kw):
        calls.append(a[0].shape[0])
        return real(*a, **kw)

    monkeypatch.setattr(ops, name, spy)
    return calls


def _engine_logits(eng, ids, next_tokens=None):
    """Prefill + 3 decode steps on fresh caches -> (list of 4 logits, tokens
    fed).  next_tokens: teacher-forced decode inputs (default: own argmax)."""
    from paddlenlp_amd.experimental import BlockManager

    eng.allocate_caches(num_blocks=64, device="cuda")
    B, T = ids.shape
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    mgr = BlockManager(64, 16, 16, B)
    slots = [mgr.allocate_slot(T) for _ in range(B)]
    bt = torch.stack([mgr.block_table[s] for s in slots]).to("cuda", torch.int32)
    out = [eng.prefill(ids, bt, lens)]
    fed = []
    for step in range(3):
        nxt = out[-1].argmax(-1, keepdim=True) if next_tokens is None else next_tokens[step]
        fed.append(nxt)
        lens_before = torch.tensor([int(mgr.seq_lens[s]) for s in slots],
                                   dtype=torch.int32, device="cuda")
        for s in slots:
            assert mgr.extend(s, 1)
        bt = torch.stack([mgr.block_table[s] for s in slots]).to("cuda", torch.int32)
        out.append(eng.decode_step(nxt, bt, lens_before))
    return out, fed


def test_mixtral_engine_wint8_fused_matches_fallback(C, monkeypatch):
    """Same quantized engine, same tokens: the fused int8 path against the
    dequantize-and-torch fallback (moe_impl="torch"), under the project's bf16
    end-to-end allowances (atol 0.5 / rtol 5e-2, near-optimal-token margin
    0.25) at every step."""
    eng = _mixtral_engine(ENGINE_SEED)
    assert eng.moe_impl == "auto"
    for name in ("moe_w1", "moe_w3", "moe_w2"):
        assert len(eng._qw[name]) == 2 and getattr(eng, name)[0].numel() == 1
    ids = torch.randint(3, 512, (2, 24), device="cuda")
    w8_calls = _spy(monkeypatch, "moe_ffn_wint8")
    bf16_calls = _spy(monkeypatch, "moe_ffn")
    fused, fed = _engine_logits(eng, ids)
    # the prefill (48 tokens) and every decode step (2 tokens), both layers
    assert w8_calls == [48, 48] + [2] * 6
    eng.moe_impl = "torch"
    del w8_calls[:]
    plain, _ = _engine_logits(eng, ids, fed)
    assert w8_calls == [] and bf16_calls == []
    for step, (a, b) in enumerate(zip(fused, plain)):
        assert torch.isfinite(a).all()
        diff = (a - b).abs().max().item()
        chosen = b.gather(-1, a.argmax(-1, keepdim=True)).squeeze(-1)
        margin = (b.max(-1).values - chosen).max().item()
        print(f"mixtral int8 engine fused vs fallback step {step}: "
              f"max diff {diff:.4f} margin {margin:.4f}")
        assert torch.allclose(a, b, atol=0.5, rtol=5e-2), (step, diff)
        assert margin < 0.25, (step, margin)


def test_mixtral_engine_wint8_close_to_bf16(C):
    """The criterion of test_engine_quantized_decode at prefill."""
    from paddlenlp_amd.experimental import BlockManager

    ids = torch.randint(3, 512, (2, 24), device="cuda")
    lens = torch.full((2,), 24, dtype=torch.int32, device="cuda")
    logits = []
    for quantize in (False, True):
        eng = _mixtral_engine(ENGINE_SEED, quantize=quantize)
        mgr = BlockManager(64, 16, 16, 2)
        slots = [mgr.allocate_slot(24) for _ in range(2)]
        bt = torch.stack([mgr.block_table[s] for s in slots]).to("cuda", torch.int32)
        logits.append(eng.prefill(ids, bt, lens).float())
    ref, got = logits
    assert torch.isfinite(got).all()
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"mixtral int8 engine vs bf16 engine, prefill: max|delta| / max|logits| = {rel:.4f}")
    assert rel < 0.2, rel


def test_mixtral_wint8_graph_decode_runner_matches_eager(C):
    """Single-stream capture of the quantized Mixtral decode step (no parallel
    branches) replays bit-identical to eager decode.  Modelled on
    test_moe_ffn_gpu.test_mixtral_graph_decode_runner_matches_eager."""
    from paddlenlp_amd.experimental.block_manager import BlockManager
    from paddlenlp_amd.experimental.fused_transformer import GraphDecodeRunner

    eng = _mixtral_engine(0)
    device = torch.device("cuda:0")
    runner = GraphDecodeRunner(eng)
    B = 2
    mgr = BlockManager(64, 16, 8, B)
    prompt = 13
    ids = torch.randint(3, 512, (B, prompt), device=device)
    lens = torch.full((B,), prompt, dtype=torch.int32, device=device)
    slots = [mgr.allocate_slot(prompt) for _ in range(B)]
    bt = torch.stack([mgr.block_table[s] for s in slots]).to(device, torch.int32)
    eng.prefill(ids, bt, lens)
    tok = torch.randint(3, 512, (B, 1), device=device)
    for step in range(3):
        lens_before = torch.tensor(
            [int(mgr.seq_lens[s]) for s in slots], dtype=torch.int32, device=device)
        for s in slots:
            assert mgr.extend(s, 1)
        bt = torch.stack([mgr.block_table[s] for s in slots]).to(device, torch.int32)
        eager = eng.decode_step(tok, bt, lens_before)
        graphed = runner(tok, bt, lens_before)
        torch.testing.assert_close(graphed, eager, rtol=0, atol=0)
        tok = eager.argmax(-1, keepdim=True)
    for s in slots:
        mgr.release(s)
