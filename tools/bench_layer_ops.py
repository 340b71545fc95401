"""Within-process A/B microbenchmark for the decoder layer's elementwise ops.

Each row pairs today's unfused composition ("old": separate bf16 add, norm,
out-of-place rope on contiguous copies, cat of dq/dk/dv) with the fused op
that replaces it ("new"), timed interleaved in ONE process on ONE box at the
training bench shape (llama3-8b, mb8 x s4096).  GB/s counts only the bytes
the new op has to move, for both columns, so the two are comparable.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from paddlenlp_amd import ops
from paddlenlp_amd.ops.functional import _load_extension


def _build_cases(C, a):
    dev = "cuda:0"
    bf = dict(device=dev, dtype=torch.bfloat16)
    N, H = a.B * a.S, a.H
    Hq, Hk, D = a.Hq, a.Hk, a.D
    W = (Hq + 2 * Hk) * D
    T = N * H * 2                       # one [N, H] bf16 pass
    res, dlt = torch.randn(N, H, **bf), torch.randn(N, H, **bf)
    w = torch.randn(H, **bf)
    dy, dh = torch.randn(N, H, **bf), torch.randn(N, H, **bf)
    h, _, invrms = C.add_rms_norm_fwd(res, dlt, w, 1e-6)
    qkv = torch.randn(a.B, a.S, W, **bf)
    cos, sin = ops.build_rope_cache(a.S, D, device=dev)
    o = torch.randn(a.B, a.S, Hq, D, **bf)
    do = torch.randn(a.B, a.S, Hq, D, **bf)
    rope_bytes = 2 * N * (Hq + Hk) * D * 2

    def split(t):
        q, k, v = t.split([Hq * D, Hk * D, Hk * D], dim=-1)
        return (q.reshape(a.B, a.S, Hq, D).contiguous(),
                k.reshape(a.B, a.S, Hk, D).contiguous(),
                v.reshape(a.B, a.S, Hk, D).contiguous())

    def old_add_norm_fwd():
        C.rms_norm_fwd(res + dlt, w, 1e-6)

    def old_add_norm_bwd():
        dx, _ = C.rms_norm_bwd(dy, h, w, invrms)
        return dx + dh

    def old_rope_fwd():     # split copies + rope on q and k
        q, k, v = split(qkv)
        C.rope_fwd(q, k, cos, sin, False)

    def old_rope_bwd():     # rope on dq and dk + cat into dqkv
        q, k, v = dqkv_parts
        dq, dk = C.rope_fwd(q, k, cos, sin, True)
        torch.cat([dq.view(a.B, a.S, -1), dk.view(a.B, a.S, -1), v.view(a.B, a.S, -1)], dim=-1)

    dqkv_parts = split(qkv)
    # name -> (bytes the new op must move, old fn, new fn)
    return {
        "add+norm fwd": (4 * T, old_add_norm_fwd,
                         lambda: C.add_rms_norm_fwd(res, dlt, w, 1e-6)),
        "add+norm bwd": (4 * T, old_add_norm_bwd,
                         lambda: C.add_rms_norm_bwd(dy, dh, h, w, invrms)),
        "norm bwd": (3 * T, None, lambda: C.rms_norm_bwd(dy, h, w, invrms)),
        "rope fwd (+split)": (rope_bytes, old_rope_fwd,
                              lambda: C.rope_packed_(qkv, cos, sin, Hq, Hk, False)),
        "rope bwd (+cat)": (rope_bytes, old_rope_bwd,
                            lambda: C.rope_packed_(qkv, cos, sin, Hq, Hk, True)),
        "delta": (2 * N * Hq * D * 2 + N * Hq * 4, None, lambda: C.flash_bwd_delta(do, o)),
    }


def _time(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3    # us


def _trimmed_mean(ts):
    ts = sorted(ts)[1:-1] or ts
    return sum(ts) / len(ts)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--B", type=int, default=8)
    p.add_argument("--S", type=int, default=4096)
    p.add_argument("--H", type=int, default=4096)
    p.add_argument("--Hq", type=int, default=32)
    p.add_argument("--Hk", type=int, default=8)
    p.add_argument("--D", type=int, default=128)
    p.add_argument("--reps", type=int, default=10)
    a = p.parse_args()

    C = _load_extension()
    torch.manual_seed(0)
    cases = _build_cases(C, a)
    for _, old, new in cases.values():   # warm-up
        if old:
            old()
        new()
    torch.cuda.synchronize()
    times = {name: ([], []) for name in cases}
    for _ in range(a.reps):
        for name, (_, old, new) in cases.items():
            if old:
                times[name][0].append(_time(old))
            times[name][1].append(_time(new))
    print(f"shape B{a.B} S{a.S} H{a.H} Hq{a.Hq} Hk{a.Hk} D{a.D}, {a.reps} reps:")
    print(f"  {'op':<18} {'old us':>9} {'new us':>9} {'new GB/s':>9}")
    for name, (nbytes, _, _) in cases.items():
        t_old, t_new = times[name]
        new_us = _trimmed_mean(t_new)
        old_s = f"{_trimmed_mean(t_old):9.1f}" if t_old else f"{'-':>9}"
        print(f"  {name:<18} {old_s} {new_us:9.1f} {nbytes / new_us / 1e3:9.0f}")


if __name__ == "__main__":
    main()
