"""GPU numerics of the paged append-attention kernel against its CPU oracle,
and engine.extend / chunked prefill against the dygraph model on device.

Every unused block-table entry points at one spare block; that block and
every cache slot past seq_lens_before + token_counts hold NaN, so an output
that is finite and matches proves the kv bound and the causal mask."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def C():
    from paddlenlp_amd.ops.functional import _load_extension

    return _load_extension()


def _tables(B, T, before, counts, bs, g):
    """randperm block tables; unused entries -> the spare (last) block."""
    maxb = (max(before) + T + bs - 1) // bs + 1
    nblocks = B * maxb + 1
    perm = torch.randperm(nblocks, generator=g)
    spare = int(perm[-1])
    bt = perm[:B * maxb].reshape(B, maxb).clone()
    for b in range(B):
        used = (before[b] + counts[b] + bs - 1) // bs
        bt[b, used:] = spare
    return bt.to(torch.int32), nblocks, spare


def _dead_slots(bt, before, counts, bs, spare):
    """(block, slot) index lists of every cache slot no query may read."""
    blk, slot = [], []
    for b in range(bt.shape[0]):
        L = before[b] + counts[b]
        for pos in range(L, (L + bs - 1) // bs * bs):
            blk.append(int(bt[b, pos // bs]))
            slot.append(pos % bs)
    blk += [spare] * bs
    slot += list(range(bs))
    return torch.tensor(blk), torch.tensor(slot)


def _bf16_case(B, T, Hq, Hk, before, counts, seed=0, bs=16, D=128):
    g = torch.Generator().manual_seed(seed)
    bt, nblocks, spare = _tables(B, T, before, counts, bs, g)
    q = torch.randn(B, T, Hq, D, generator=g).to(torch.bfloat16)
    kc = torch.randn(nblocks, bs, Hk, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(nblocks, bs, Hk, D, generator=g).to(torch.bfloat16)
    blk, slot = _dead_slots(bt, before, counts, bs, spare)
    kc[blk, slot] = NAN
    vc[blk, slot] = NAN
    return (q, kc, vc, bt, torch.tensor(before, dtype=torch.int32),
            torch.tensor(counts, dtype=torch.int32))


def _check(C, case, scales=None, r_tiles=0, atol=3e-2, rtol=3e-2, use_counts=True):
    from paddlenlp_amd.experimental.fused_transformer import paged_append_attn_ref

    q, kc, vc, bt, before, counts = case
    ks, vs = scales if scales is not None else (None, None)
    dev = lambda t: None if t is None else t.cuda()
    out = C.paged_append_attn(dev(q), dev(kc), dev(vc), dev(bt), dev(before),
                              dev(counts) if use_counts else None, dev(ks), dev(vs),
                              r_tiles).cpu()
    ref = paged_append_attn_ref(q, kc, vc, bt, before, counts, ks, vs)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()
    for b in range(q.shape[0]):
        n = int(counts[b])
        assert torch.equal(out[b, n:], torch.zeros_like(out[b, n:])), b
    err = (out.float() - ref.float()).abs().max()
    print(f"max abs err {err:.4g}")
    if atol is not None:
        assert torch.allclose(out.float(), ref.float(), atol=atol, rtol=rtol), err
    return out, ref


BASE = dict(B=3, T=9, Hq=8, Hk=2, before=[0, 37, 130], counts=[9, 5, 1])


@pytest.mark.parametrize("r_tiles", [0, 1, 2])
def test_base(C, r_tiles):
    """Empty prefix, a partial 16-row tile (36 rows), the mask diagonal
    crossing the 128-token V tile, a one-token row, zero rows.  The grid is
    small, so the kv range is split and the merge kernel runs."""
    _check(C, _bf16_case(**BASE), r_tiles=r_tiles)


def test_group_of_seven(C):
    """G = 7: tokens straddle the 16-row tiles."""
    _check(C, _bf16_case(B=1, T=5, Hq=7, Hk=1, before=[20], counts=[5], seed=1),
           use_counts=False)


@pytest.mark.parametrize("r_tiles", [1, 2])
@pytest.mark.parametrize("T", [33, 70])
def test_mha_many_row_tiles(C, T, r_tiles):
    """G = 1: 33 rows are 2 tiles + 1 row, 70 rows 4 tiles + 6; both R run
    full row groups and a remainder group."""
    _check(C, _bf16_case(B=1, T=T, Hq=2, Hk=2, before=[0], counts=[T], seed=2),
           r_tiles=r_tiles)


def test_single_token_equals_decode(C):
    """Append at T = 1 and decode run the same tile loop over the same kv
    range, sum for sum: the outputs are equal bit for bit."""
    case = _bf16_case(B=3, T=1, Hq=8, Hk=2, before=[0, 37, 130], counts=[1, 1, 1], seed=3)
    out, _ = _check(C, case)
    q, kc, vc, bt, before, _ = case
    dec = C.paged_decode_attn(q[:, 0].contiguous().cuda(), kc.cuda(), vc.cuda(),
                              bt.cuda(), (before + 1).cuda()).cpu()
    assert torch.equal(out[:, 0], dec), (out[:, 0].float() - dec.float()).abs().max()


def test_direct_write_no_split(C):
    """B*Hk = 512 workgroups: nsplit == 1, the kernel writes the output
    itself."""
    B = 64
    g = torch.Generator().manual_seed(4)
    before = torch.randint(0, 40, (B,), generator=g).tolist()
    counts = torch.randint(0, 3, (B,), generator=g).tolist()
    _check(C, _bf16_case(B=B, T=2, Hq=32, Hk=8, before=before, counts=counts, seed=4))


def _quant_case(C, mode, seed=5, bs=16, D=128):
    """Base shape over a quantised cache filled through rope_cache_append."""
    from paddlenlp_amd import ops

    B, T, Hq, Hk = BASE["B"], BASE["T"], BASE["Hq"], BASE["Hk"]
    before, counts = BASE["before"], BASE["counts"]
    g = torch.Generator().manual_seed(seed)
    bt, nblocks, spare = _tables(B, T, before, counts, bs, g)
    total = [x + y for x, y in zip(before, counts)]
    qkv = torch.randn(B, max(total), (Hq + 2 * Hk) * D, generator=g).to(torch.bfloat16).cuda()
    if mode == "int8":
        kc = torch.zeros(nblocks, bs, Hk, D, dtype=torch.int8, device="cuda")
    else:
        kc = torch.zeros(nblocks, bs, Hk, D // 2, dtype=torch.uint8, device="cuda")
    vc = torch.zeros_like(kc)
    ks = torch.zeros(nblocks, bs, Hk, dtype=torch.float32, device="cuda")
    vs = torch.zeros_like(ks)
    cos, sin = ops.build_rope_cache(256, D, device="cuda")
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    C.rope_cache_append(qkv, kc, vc, bt.cuda(), zero, cos, sin, Hq, Hk,
                        torch.tensor(total, dtype=torch.int32, device="cuda"), ks, vs)
    ks, vs = ks.cpu(), vs.cpu()
    blk, slot = _dead_slots(bt, before, counts, bs, spare)
    ks[blk, slot] = NAN      # a NaN scale makes the dequantised slot NaN
    vs[blk, slot] = NAN
    q = torch.randn(B, T, Hq, D, generator=g).to(torch.bfloat16)
    case = (q, kc.cpu(), vc.cpu(), bt, torch.tensor(before, dtype=torch.int32),
            torch.tensor(counts, dtype=torch.int32))
    return case, (ks, vs)


def test_int8_cache(C):
    """Tolerance of test_int8_kv_cache_kernels: max error below 3% of the
    largest reference value."""
    case, scales = _quant_case(C, "int8")
    out, ref = _check(C, case, scales, atol=None)
    rel = (out.float() - ref.float()).abs().max() / ref.float().abs().max()
    assert rel < 0.03, rel


def test_int4_cache(C):
    """Tolerance of test_int4_kv_cache_gpu (atol = rtol = 5e-2); kernel and
    oracle read the same GPU-written cache."""
    case, scales = _quant_case(C, "int4")
    _check(C, case, scales, atol=5e-2, rtol=5e-2)


def test_refused_shape_raises(C):
    q = torch.zeros(1, 2, 4, 64, dtype=torch.bfloat16, device="cuda")
    kc = torch.zeros(4, 16, 2, 64, dtype=torch.bfloat16, device="cuda")
    bt = torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    before = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="D=64.*G=2"):
        C.paged_append_attn(q, kc, kc, bt, before)


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------
def _engine(hidden):
    from paddlenlp_amd.experimental import BlockManager, FusedMultiTransformer
    from paddlenlp_amd.transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(3)
    cfg = LlamaConfig(
        vocab_size=512, hidden_size=hidden, intermediate_size=2 * hidden,
        num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
        max_position_embeddings=256,
    )
    model = LlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device="cuda")
    model.eval()
    eng = FusedMultiTransformer.from_llama(model, block_size=16, max_seq_len=256).to("cuda")
    eng.allocate_caches(num_blocks=64, device="cuda")
    B, T = 2, 24
    ids = torch.randint(3, 512, (B, T), device="cuda")
    mgr = BlockManager(64, 16, 16, B)
    slots = [mgr.allocate_slot(T) for _ in range(B)]
    bt = torch.stack([mgr.block_table[s] for s in slots]).to("cuda", torch.int32)
    with torch.no_grad():
        ref = model(input_ids=ids).float()
    return eng, ids, bt, ref


def _close_to_dygraph(logits, ref):
    # the tolerances of test_engine_decode_gpu_matches_dygraph
    assert torch.allclose(logits, ref, atol=0.5, rtol=5e-2), (logits - ref).abs().max()
    chosen = ref.gather(-1, logits.argmax(-1, keepdim=True)).squeeze(-1)
    assert (ref.max(-1).values - chosen < 0.25).all()


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


def test_engine_extend_matches_dygraph(C):
    eng, ids, bt, ref = _engine(512)          # head dim 128: the append kernel
    eng.prefill(ids[:, :16], bt, _i32([16, 16]))
    logits = eng.extend(ids[:, 16:24], bt, _i32([16, 16]))
    _close_to_dygraph(logits, ref[:, -1])

    for k in eng.k_caches + eng.v_caches:
        k.zero_()
    logits = eng.prefill(ids, bt, _i32([24, 24]), chunk_size=8)
    _close_to_dygraph(logits, ref[:, -1])


def test_engine_extend_per_token_fallback(C):
    eng, ids, bt, ref = _engine(256)          # head dim 64: decode kernel per token
    eng.prefill(ids[:, :16], bt, _i32([16, 16]))
    logits = eng.extend(ids[:, 16:24], bt, _i32([16, 16]), _i32([8, 5]))
    assert torch.isfinite(logits).all()
    _close_to_dygraph(logits, torch.stack([ref[0, 23], ref[1, 20]]))
    # rows past token_counts come back zero from the attention itself
    q = torch.randn(2, 8, 4, 64, device="cuda", dtype=torch.bfloat16)
    attn = eng._paged_append_attn(0, q, bt, _i32([16, 16]), _i32([8, 5]))
    assert torch.isfinite(attn.float()).all()
    assert not attn[1, 5:].any() and attn[1, :5].any()
