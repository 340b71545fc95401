"""Paged append attention: the multi-token kernel against the per-token
decode-kernel loop, timed interleaved in one process (docs/kernels.md).

Kernel mode (default) uses Llama-3-8B head geometry (Hq 32, Hk 8, D 128):
  * verification shape  B 64, ctx 4096, T in {2, 5, 8}
  * chunk shape         B 4,  ctx 4096, T 512, for every instantiated R
--engine times one FusedMultiTransformer.extend step (T = 5) next to one
decode_step at B 64 / ctx 4096 on the 8B engine (random weights; the cache is
addressed but not prefilled, attention cost does not depend on its values).

One JSON line per measurement; the numbers live in
profiles/paged_append_attn.md.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

HQ, HK, D, BS = 32, 8, 128, 64
R_TILES = (1, 2)


def time_interleaved(variants, reps, iters):
    """variants: {name: fn}.  Each rep times every variant once (iters calls
    between two events); returns {name: median ms per call}."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters)
    return {k: statistics.median(v) for k, v in times.items()}


def make_cache(B, ctx, T, cachekv, device):
    nb_seq = (ctx + T + BS - 1) // BS
    nblocks = B * nb_seq
    bt = torch.randperm(nblocks, device=device).to(torch.int32).view(B, nb_seq)
    scales = (None, None)
    if cachekv == "bf16":
        kc = torch.randn(nblocks, BS, HK, D, device=device, dtype=torch.bfloat16)
        vc = torch.randn_like(kc)
    else:
        last = D if cachekv == "int8" else D // 2
        dt = torch.int8 if cachekv == "int8" else torch.uint8
        lo, hi = (-127, 128) if cachekv == "int8" else (0, 256)
        kc = torch.randint(lo, hi, (nblocks, BS, HK, last), device=device).to(dt)
        vc = torch.randint(lo, hi, (nblocks, BS, HK, last), device=device).to(dt)
        scales = (torch.rand(nblocks, BS, HK, device=device) * 0.02,
                  torch.rand(nblocks, BS, HK, device=device) * 0.02)
    return kc, vc, bt, scales


def bench_kernel(C, B, ctx, T, r_list, cachekv, reps, iters, device):
    kc, vc, bt, (ks, vs) = make_cache(B, ctx, T, cachekv, device)
    q = torch.randn(B, T, HQ, D, device=device, dtype=torch.bfloat16)
    before = torch.full((B,), ctx, dtype=torch.int32, device=device)
    q_tok = [q[:, t].contiguous() for t in range(T)]
    lens_tok = [before + (t + 1) for t in range(T)]

    def loop():
        for t in range(T):
            C.paged_decode_attn(q_tok[t], kc, vc, bt, lens_tok[t], ks, vs)

    variants = {"decode_loop": loop}
    for r in r_list:
        variants[f"append_r{r}"] = (
            lambda r=r: C.paged_append_attn(q, kc, vc, bt, before, None, ks, vs, r))
    ms = time_interleaved(variants, reps, iters)
    for name, v in ms.items():
        print(json.dumps({
            "metric": "paged_append_attn_ms", "variant": name, "B": B, "ctx": ctx,
            "T": T, "cachekv": cachekv, "value": round(v, 4),
            "vs_decode_loop": round(ms["decode_loop"] / v, 3),
        }), flush=True)


def bench_engine(B, ctx, T, reps, iters, device):
    from paddlenlp_amd.experimental import FusedMultiTransformer
    from paddlenlp_amd.transformers import LlamaConfig, LlamaForCausalLM
    from bench_infer import MODELS

    cfg = LlamaConfig(**MODELS["llama3-8b"], dtype="bfloat16")
    model = LlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=device)
    model.eval()
    eng = FusedMultiTransformer.from_llama(model, block_size=BS, max_seq_len=8192).to(device)
    del model
    torch.cuda.empty_cache()
    nb_seq = (ctx + T + BS - 1) // BS
    eng.allocate_caches(B * nb_seq, device)
    bt = torch.randperm(B * nb_seq, device=device).to(torch.int32).view(B, nb_seq)
    before = torch.full((B,), ctx, dtype=torch.int32, device=device)
    ids = torch.randint(3, cfg.vocab_size, (B, T), device=device)
    ms = time_interleaved({
        "decode_step": lambda: eng.decode_step(ids[:, :1], bt, before),
        "extend": lambda: eng.extend(ids, bt, before),
    }, reps, iters)
    for name, v in ms.items():
        print(json.dumps({
            "metric": "engine_step_ms", "variant": name, "model": "llama3-8b",
            "B": B, "ctx": ctx, "T": 1 if name == "decode_step" else T,
            "value": round(v, 3),
        }), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--engine", action="store_true")
    p.add_argument("--cachekv", default="bf16", choices=["bf16", "int8", "int4"])
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--ctx", type=int, default=4096)
    args = p.parse_args()
    device = "cuda:0"
    if args.engine:
        bench_engine(64, args.ctx, 5, args.reps, args.iters, device)
        return
    from paddlenlp_amd.ops.functional import _load_extension

    C = _load_extension()
    for T in (2, 5, 8):
        bench_kernel(C, 64, args.ctx, T, R_TILES, args.cachekv, args.reps, args.iters, device)
    bench_kernel(C, 4, args.ctx, 512, R_TILES, args.cachekv, args.reps, args.iters, device)


if __name__ == "__main__":
    main()
