"""Within-probe A/B microbenchmark for the flash-attention kernels.

Guide rule #13: cross-run/cross-box deltas under 10% are noise — kernels
must be timed interleaved in ONE process on ONE box.

The v2 forward, dq and dkv kernels are reported separately (the backward
binding flash_attn_bwd2_parts launches a chosen subset), next to the v1
forward and combined backward.  A kernel variant under development goes into
KERNELS as one more row, so it is timed in the same interleaved loop.
"""
import argparse
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from paddlenlp_amd.ops.functional import _load_extension

BWD_DELTA, BWD_DQ, BWD_DKV = 1, 2, 4

# matmul counts: fwd 2 (S, PV); dq 3 (S, dP, dQ); dkv 4 (S, dP, dV, dK); the
# v1 combined backward recomputes S and dP once per kernel like v2 (7)
# name -> (matmuls, fn(C, t)) with t the dict of tensors built in main()
KERNELS = {
    "fwd v2-32x32": (2, lambda C, t: C.flash_attn_fwd_ex(t["q"], t["k"], t["v"], True, False)),
    "fwd v1-linear": (2, lambda C, t: C.flash_attn_fwd_ex(t["q"], t["k"], t["v"], True, True)),
    "dq  v2-32x32": (3, lambda C, t: C.flash_attn_bwd2_parts(
        t["do"], t["q"], t["k"], t["v"], t["o"], t["lse"], t["delta"], True, BWD_DQ)),
    "dkv v2-32x32": (4, lambda C, t: C.flash_attn_bwd2_parts(
        t["do"], t["q"], t["k"], t["v"], t["o"], t["lse"], t["delta"], True, BWD_DKV)),
    "bwd v2-32x32": (7, lambda C, t: C.flash_attn_bwd_ex(
        t["do"], t["q"], t["k"], t["v"], t["o"], t["lse"], True, False)),
    "bwd v1-linear": (7, lambda C, t: C.flash_attn_bwd_ex(
        t["do"], t["q"], t["k"], t["v"], t["o"], t["lse"], True, True)),
}


def _time_interleaved(C, t, reps):
    """Per-kernel device times (ms) with the kernels alternating inside each rep."""
    results = {name: [] for name in KERNELS}
    for _, fn in KERNELS.values():   # warm-up
        fn(C, t)
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, (_, fn) in KERNELS.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(C, t)
            e1.record()
            e1.synchronize()
            results[name].append(e0.elapsed_time(e1))
    return results


def _report(results, matmul_flops):
    for name, times in results.items():
        ts = sorted(times)[1:-1] or times  # trim outliers
        mean = sum(ts) / len(ts)
        flops = KERNELS[name][0] * matmul_flops
        print(f"  {name:<14}: {mean:8.3f} ms  {flops/mean/1e9:7.1f} TF/s")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--B", type=int, default=8)
    p.add_argument("--S", type=int, default=4096)
    p.add_argument("--Hq", type=int, default=32)
    p.add_argument("--Hk", type=int, default=8)
    p.add_argument("--D", type=int, default=128)
    p.add_argument("--reps", type=int, default=10)
    args = p.parse_args()

    C = _load_extension()
    torch.manual_seed(0)
    dev = "cuda:0"
    q = torch.randn(args.B, args.S, args.Hq, args.D, device=dev, dtype=torch.bfloat16)
    k = torch.randn(args.B, args.S, args.Hk, args.D, device=dev, dtype=torch.bfloat16)
    v = torch.randn(args.B, args.S, args.Hk, args.D, device=dev, dtype=torch.bfloat16)

    # one causal attention matmul (0.5 visibility), 2 flops per MAC
    matmul_flops = 0.5 * 2 * args.B * args.Hq * args.S * args.S * args.D

    # correctness cross-check first: v2 against v1
    ref_o, ref_lse = C.flash_attn_fwd_ex(q, k, v, True, True)
    o, lse = C.flash_attn_fwd_ex(q, k, v, True, False)
    err = (o.float() - ref_o.float()).abs().max().item()
    print(f"  fwd v2 vs v1 max err: {err:.4f}")
    assert err < 3e-2, err

    do = torch.randn_like(o)
    ref_dq, ref_dk, ref_dv = C.flash_attn_bwd_ex(do, q, k, v, o, lse, True, True)
    dq2, dk2, dv2 = C.flash_attn_bwd_ex(do, q, k, v, o, lse, True, False)
    for nm, a, b in (("dq", ref_dq, dq2), ("dk", ref_dk, dk2), ("dv", ref_dv, dv2)):
        err = (a.float() - b.float()).abs().max().item()
        print(f"  bwd v2 vs v1 {nm} max err: {err:.4f}")

    # delta = rowsum(dO * O) as [B, Hq, S] for the dq/dkv-only launches
    delta = (do.float() * o.float()).sum(-1).permute(0, 2, 1).contiguous()
    t = dict(q=q, k=k, v=v, o=o, lse=lse, do=do, delta=delta)

    print(f"shape B{args.B} S{args.S} Hq{args.Hq} Hk{args.Hk} D{args.D}, {args.reps} reps:")
    _report(_time_interleaved(C, t, args.reps), matmul_flops)


if __name__ == "__main__":
    main()
