"""Within-probe A/B microbenchmark for the flash-attention kernels.

Guide rule #13: cross-run/cross-box deltas under 10% are noise — kernels
must be timed interleaved in ONE process on ONE box.
"""
import argparse
import sys
import os
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from paddlenlp_amd.ops.functional import _load_extension

# name -> force_v1: the default path (v2 8-wave 32x32 kernels at D=128) against
# the v1 4-wave 16x16 fallback
KERNELS = {"v2-32x32": False, "v1-linear": True}


def _time_interleaved(fn, reps):
    """Per-kernel wall times with the kernels alternating inside each rep."""
    results = {name: [] for name in KERNELS}
    for _ in range(reps):
        for name, force_v1 in KERNELS.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(force_v1)
            torch.cuda.synchronize()
            results[name].append(time.perf_counter() - t0)
    return results


def _report(tag, results, flops):
    for name, times in results.items():
        ts = sorted(times)[1:-1] or times  # trim outliers
        mean = sum(ts) / len(ts)
        print(f"  {tag} {name:<9}: {mean*1e3:8.2f} ms  {flops/mean/1e12:7.1f} TF/s")


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

    # causal attention matmul FLOPs (0.5 visibility): 2 matmuls x 2 flops
    flops = 0.5 * 2 * 2 * args.B * args.Hq * args.S * args.S * args.D

    # correctness cross-check first: v2 against v1
    ref_o, ref_lse = C.flash_attn_fwd_ex(q, k, v, True, True)
    o, lse = C.flash_attn_fwd_ex(q, k, v, True, False)
    err = (o.float() - ref_o.float()).abs().max().item()
    print(f"  fwd v2 vs v1 max err: {err:.4f}")
    assert err < 3e-2, err

    print(f"shape B{args.B} S{args.S} Hq{args.Hq} Hk{args.Hk} D{args.D}, {args.reps} reps:")
    _report("fwd", _time_interleaved(
        lambda force_v1: C.flash_attn_fwd_ex(q, k, v, True, force_v1), args.reps), flops)

    do = torch.randn_like(o)
    ref_dq, ref_dk, ref_dv = C.flash_attn_bwd_ex(do, q, k, v, o, lse, True, True)
    dq2, dk2, dv2 = C.flash_attn_bwd_ex(do, q, k, v, o, lse, True, False)
    for nm, a, b in (("dq", ref_dq, dq2), ("dk", ref_dk, dk2), ("dv", ref_dv, dv2)):
        err = (a.float() - b.float()).abs().max().item()
        print(f"  bwd v2 vs v1 {nm} max err: {err:.4f}")
    bwd_flops = flops * 3.5  # 7 matmuls vs fwd's 2
    _report("bwd", _time_interleaved(
        lambda force_v1: C.flash_attn_bwd_ex(do, q, k, v, o, lse, True, force_v1),
        args.reps), bwd_flops)

if __name__ == "__main__":
    main()
