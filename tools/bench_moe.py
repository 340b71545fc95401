"""Routed MoE FFN of one Mixtral-8x7B layer (H=4096, I=14336, E=8, top-2):
the engine's torch path vs the fused kernels (moe_ffn.hip), interleaved in one
process, for decode-sized token counts with random routing.

Per T: median microseconds of each path (device events around one call of
FusedMultiTransformer._moe_ffn, router GEMM included in both), their ratio,
and the fused path's achieved rate over the weight bytes of the experts that
were actually selected (n_active * 3 * H * I * 2 bytes / time) - that figure
only tells how far from streaming the kernels are; the comparison that counts
is against the torch path in the same run.  The torch path's .item() stall is
inside its time (the host waits for the device mid-call); it is not timed
separately.

With --wint8 the fused path over weight-only int8 experts (the same weights
packed by quantize_moe_int8, ops.moe_ffn_wint8) is one more column, timed in
the same loop on the same inputs; its rate is over the int8 bytes it reads
(n_active * 3 * H * I bytes / time) and its ratio is against the fused bf16
column of the same run.

    python tools/bench_moe.py [--tokens 1 4 16 64 256] [--reps 30] [--wint8]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from paddlenlp_amd.experimental.fused_transformer import (
    FusedMultiTransformer, FusedMultiTransformerConfig)
from paddlenlp_amd.ops import reference
from paddlenlp_amd.ops.functional import _load_extension


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[1, 4, 16, 64, 256])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--inter", type=int, default=14336)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--top-k", type=int, default=2)
    ap.add_argument("--nsets", type=int, default=4,
                    help="distinct inputs cycled through, so that the selected experts vary")
    ap.add_argument("--wint8", action="store_true",
                    help="also time the fused path over int8 expert weights")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_moe needs a GPU"
    C = _load_extension()
    H, I, E, K = args.hidden, args.inter, args.experts, args.top_k

    cfg = FusedMultiTransformerConfig(
        hidden_size=H, num_heads=H // 128, num_kv_heads=max(1, H // 512),
        intermediate_size=I, num_layers=1, vocab_size=128, max_seq_len=128,
        moe_num_experts=E, moe_top_k=K)
    with torch.device("cuda"):
        eng = FusedMultiTransformer(cfg)
    gen = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        eng.moe_gates[0].copy_(torch.randn(E, H, device="cuda", generator=gen) / H ** 0.5)
        for w, fan_in in ((eng.moe_w1[0], H), (eng.moe_w3[0], H), (eng.moe_w2[0], I)):
            for e in range(E):
                w[e].copy_(torch.randn(w.shape[1:], device="cuda", generator=gen) / fan_in ** 0.5)
    eng.moe_fused_max_tokens = 1 << 30

    packed = {}
    if args.wint8:
        from paddlenlp_amd.quantization import quantize_moe_int8

        for name in ("moe_w1", "moe_w3", "moe_w2"):
            packed[name] = [quantize_moe_int8(getattr(eng, name)[0].data)]

    def run(impl, h):
        # "wint8": the engine's own dispatch with the packed experts in place
        eng._qw = packed if impl == "wint8" else {}
        eng.moe_impl = "auto" if impl == "wint8" else impl
        with torch.no_grad():
            return eng._moe_ffn(h, 0)

    rows = []
    for T in args.tokens:
        hs = [torch.randn(T, H, device="cuda", dtype=torch.bfloat16, generator=gen)
              for _ in range(args.nsets)]
        n_active = []
        for h in hs:
            ids, _ = reference.moe_route(h @ eng.moe_gates[0].t(), K)
            n_active.append(int(torch.unique(ids).numel()))
        diff = (run("auto", hs[0]).float() - run("torch", hs[0]).float()).abs().max().item()
        for h in hs:           # warm every shape the paths use
            run("torch", h), run("auto", h)
            if args.wint8:
                run("wint8", h)
        torch.cuda.synchronize()
        t_torch, t_fused, t_w8 = [], [], []
        for r in range(args.reps):
            h = hs[r % args.nsets]
            t_torch.append(timed(lambda: run("torch", h))[0])
            t_fused.append(timed(lambda: run("auto", h))[0])
            if args.wint8:
                t_w8.append(timed(lambda: run("wint8", h))[0])
        mt, mf = statistics.median(t_torch), statistics.median(t_fused)
        act = sum(n_active) / len(n_active)
        row = dict(T=T, torch_us=round(mt, 1), fused_us=round(mf, 1),
                   torch_min_us=round(min(t_torch), 1), fused_min_us=round(min(t_fused), 1),
                   speedup=round(mt / mf, 2), n_active=act,
                   fused_TBps=round(act * 3 * H * I * 2 / (mf * 1e-6) / 1e12, 2),
                   ksplit=C.moe_down_ksplit(T, K, H, I),
                   max_abs_diff=round(diff, 4))
        if args.wint8:
            m8 = statistics.median(t_w8)
            d8 = (run("wint8", hs[0]).float() - run("auto", hs[0]).float()).abs().max().item()
            row.update(wint8_us=round(m8, 1), wint8_min_us=round(min(t_w8), 1),
                       fused_over_wint8=round(mf / m8, 3),
                       wint8_TBps=round(act * 3 * H * I / (m8 * 1e-6) / 1e12, 2),
                       wint8_ksplit=C.moe_down_ksplit_wint8(T, K, H, I),
                       wint8_vs_fused_max_abs_diff=round(d8, 4))
        rows.append(row)
        print(json.dumps(row), flush=True)

    print(f"\n| T | torch us | fused us | torch/fused | active experts | fused TB/s over active weights | ksplit |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['T']} | {r['torch_us']} | {r['fused_us']} | {r['speedup']} | "
              f"{r['n_active']} | {r['fused_TBps']} | {r['ksplit']} |")
    if args.wint8:
        print("\n| T | fused bf16 us (min) | fused int8 us (min) | bf16 / int8 | "
              "bf16 TB/s | int8 TB/s | ksplit bf16 / int8 |")
        print("|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['T']} | {r['fused_us']} ({r['fused_min_us']}) | "
                  f"{r['wint8_us']} ({r['wint8_min_us']}) | {r['fused_over_wint8']} | "
                  f"{r['fused_TBps']} | {r['wint8_TBps']} | "
                  f"{r['ksplit']} / {r['wint8_ksplit']} |")


if __name__ == "__main__":
    main()
