"""GPU checks for the softmax arithmetic and the mask-free full-tile paths of
the v2 flash-attention kernels (forward, dq, dkv; dense and FlashMask).

The oracle is materialised attention in float64 on the same bf16 inputs, with
the visibility rules of ops.reference.flash_attention (causal with offset
Skv - Sq, FlashMask column bounds); gradients come by autograd.  The metric
per output is ||got - want||_2 / ||want||_2 over the finite entries, plus the
largest absolute error for lse.

The bounds are not tolerances chosen for this code: PARENT_MAX holds, per
case and output, the largest value the kernels measured BEFORE the softmax
diet (per-element scaling and masking everywhere) over seeds 0-4, with the
same measurement (`measure` below; figures and method in
profiles/fa_softmax_diet.md), to every digit.  The test evaluates seed 0 and
asks for at most the five-seed maximum, with no factor on top.  Where seed 0
is the earlier kernels' own worst seed that leaves no margin at all: an
exp2-domain version that moved only the last place of P and dS (errors within
0.93-1.09 of the earlier ones per seed, above and below alike) missed three
such comparisons, and is not what the kernels do now.  They round every value
as the earlier kernels did, so their figures are the earlier kernels' figures.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
OUTPUTS = ("o", "lse", "lse_abs", "dq", "dk", "dv")

# name -> (B, Sq, Skv, Hq, Hk, causal, FlashMask bounds or None, q/k factor)
CASES = {
    # a single diagonal tile: masked path only
    "diag64": (1, 64, 64, 4, 1, True, None, 1.0),
    # q block 1 has full tiles and a diagonal tile in one wave's loop, in all
    # three kernels; dkv gets full and diagonal q tiles
    "full_and_diag320": (1, 320, 320, 4, 2, True, None, 1.0),
    # ragged: the full-tile test must not fire on a tile with rows >= Sq/Skv
    "ragged100": (1, 100, 100, 2, 2, True, None, 1.0),
    "ragged577": (1, 577, 577, 4, 1, True, None, 1.0),
    # causal offset > 0
    "offset_pos": (1, 128, 320, 4, 2, True, None, 1.0),
    # every tile full except the ragged last one
    "noncausal300": (1, 300, 300, 4, 2, False, None, 1.0),
    # offset < 0: q rows 0-127 see no key
    "offset_neg": (1, 192, 64, 2, 1, True, None, 1.0),
    # rows 70-95 share a wave with rows 64-69 and see nothing in kv tile 0:
    # their running max is still -inf while the wave is not skipped
    "flashmask320": (1, 320, 320, 4, 2, True, (70, 200, 320), 1.0),
    # FlashMask with whole-tile staging skips
    "flashmask576": (1, 576, 576, 4, 2, True, (200, 256, 576), 1.0),
    # scaled scores with std ~ 16, far above the defer-max threshold of 8: the
    # threshold, the rescale and underflow of the exponential to 0 all run
    "large_logits320": (1, 320, 320, 4, 2, True, None, 4.0),
}

# Largest value over seeds 0-4 of the kernels before the softmax diet.
PARENT_MAX = {
    "diag64": dict(o=0.0018440583999855644, lse=5.084652662297605e-08,
                  lse_abs=6.068474149856229e-07, dq=0.002735502344150692,
                  dk=0.0027191739975590498, dv=0.0023451799833142588),
    "full_and_diag320": dict(o=0.0019846881498597453, lse=4.8959364003282516e-08,
                            lse_abs=8.925375842849803e-07, dq=0.002562641406766907,
                            dk=0.0025534694451762093, dv=0.0022849932187860517),
    "ragged100": dict(o=0.001907532222203388, lse=5.1019779728625764e-08,
                     lse_abs=6.648776071926932e-07, dq=0.0027465595730521235,
                     dk=0.0026555480170579668, dv=0.002370877352788356),
    "ragged577": dict(o=0.002027679611883012, lse=4.8306735190610076e-08,
                     lse_abs=9.540110355032994e-07, dq=0.002541452264594257,
                     dk=0.002519809077609224, dv=0.002387096901763521),
    "offset_pos": dict(o=0.002302001278256103, lse=4.87864142156081e-08,
                      lse_abs=8.638748187905776e-07, dq=0.002431978834265219,
                      dk=0.00241351011129007, dv=0.0023774261444360276),
    "noncausal300": dict(o=0.002314100293655246, lse=4.8627534156717534e-08,
                        lse_abs=8.869618364215626e-07, dq=0.002403980354465414,
                        dk=0.0023769428246263407, dv=0.002379330353043663),
    "offset_neg": dict(o=0.001861089768561212, lse=4.646169118249306e-08,
                      lse_abs=5.730881076360106e-07, dq=0.0027011444956437937,
                      dk=0.002713694727224844, dv=0.0023983794281437504),
    "flashmask320": dict(o=0.0019017661149763898, lse=4.9443846372172446e-08,
                        lse_abs=8.315312705065026e-07, dq=0.0026509728239382823,
                        dk=0.002636383775899946, dv=0.0022734339275372445),
    "flashmask576": dict(o=0.0019422204607527063, lse=4.9443654449945686e-08,
                        lse_abs=8.866540301966097e-07, dq=0.0025527763614520585,
                        dk=0.002563720798635028, dv=0.002283946395918837),
    "large_logits320": dict(o=0.0014169162940047592, lse=6.627799685047851e-08,
                           lse_abs=1.3841557887417366e-05, dq=0.006412335214080109,
                           dk=0.006257592564936913, dv=0.001998958205551562),
}


@pytest.fixture(scope="module")
def C():
    from paddlenlp_amd.ops.functional import _load_extension

    return _load_extension()


def _inputs(case, seed):
    B, Sq, Skv, Hq, Hk, causal, bounds, factor = CASES[case]
    torch.manual_seed(seed)
    q = (torch.randn(B, Sq, Hq, D, device="cuda") * factor).to(torch.bfloat16)
    k = (torch.randn(B, Skv, Hk, D, device="cuda") * factor).to(torch.bfloat16)
    v = torch.randn(B, Skv, Hk, D, device="cuda").to(torch.bfloat16)
    do = torch.randn(B, Sq, Hq, D, device="cuda").to(torch.bfloat16)
    se = None
    if bounds is not None:
        se = torch.empty(B, Skv, dtype=torch.int32, device="cuda")
        lo = 0
        for hi in bounds:
            se[:, lo:hi] = hi
            lo = hi
    return q, k, v, do, se


def _visible(Sq, Skv, causal, se):
    """[B or 1, 1, Sq, Skv] bool, as ops.reference.flash_attention."""
    rows = torch.arange(Sq, device="cuda").view(1, 1, Sq, 1)
    cols = torch.arange(Skv, device="cuda").view(1, 1, 1, Skv)
    if se is not None:
        return (cols <= rows) & (rows < se.long().view(-1, 1, 1, Skv))
    if causal:
        return cols <= rows + (Skv - Sq)
    return torch.ones(1, 1, Sq, Skv, dtype=torch.bool, device="cuda")


def oracle(q, k, v, do, causal, se):
    """float64 attention; fully masked rows give o = 0 and lse = -inf."""
    G = q.shape[2] // k.shape[2]
    q64 = q.double().requires_grad_()
    k64 = k.double().requires_grad_()
    v64 = v.double().requires_grad_()
    kr = k64.repeat_interleave(G, dim=2)
    vr = v64.repeat_interleave(G, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", q64, kr) / math.sqrt(D)
    vis = _visible(q.shape[1], k.shape[1], causal, se).expand_as(s)
    s = torch.where(vis, s, torch.zeros_like(s))       # no inf enters autograd
    m = torch.where(vis, s, torch.full_like(s, -1e300)).amax(-1, keepdim=True).detach()
    m = torch.where(m > -1e299, m, torch.zeros_like(m))   # rows without a key
    e = torch.where(vis, torch.exp(s - m), torch.zeros_like(s))
    l = e.sum(-1, keepdim=True)
    some = l > 0
    p = e / torch.where(some, l, torch.ones_like(l))
    o = torch.einsum("bhqk,bkhd->bqhd", p, vr)
    o.backward(do.double())
    lse = torch.where(some, m + torch.log(torch.where(some, l, torch.ones_like(l))),
                      torch.full_like(l, -math.inf)).squeeze(-1)
    return dict(o=o.detach(), lse=lse.detach(), dq=q64.grad, dk=k64.grad, dv=v64.grad)


def run_kernels(C, q, k, v, do, causal, se):
    if se is not None:
        o, lse = C.flashmask_attn_fwd(q, k, v, se)
        dq, dk, dv = C.flashmask_attn_bwd(do, q, k, v, o, lse, se)
    else:
        o, lse = C.flash_attn_fwd_ex(q, k, v, causal, False)
        dq, dk, dv = C.flash_attn_bwd_ex(do, q, k, v, o, lse, causal, False)
    torch.cuda.synchronize()
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


_ORACLE_CACHE = {}


def _case(C, case, seed):
    """(inputs, kernel outputs, oracle outputs); the oracle is computed once
    per (case, seed) and shared."""
    q, k, v, do, se = _inputs(case, seed)
    causal = CASES[case][5]
    key = (case, seed)
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = oracle(q, k, v, do, causal, se)
    return (q, k, v, do, se), run_kernels(C, q, k, v, do, causal, se), _ORACLE_CACHE[key]


def _rel_l2(got, want):
    got, want = got.double(), want.double()
    fin = torch.isfinite(want)
    return ((got[fin] - want[fin]).norm() / want[fin].norm()).item()


def measure(C, case, seed):
    """The figures PARENT_MAX bounds, for one case and seed."""
    _, got, want = _case(C, case, seed)
    out = {n: _rel_l2(got[n], want[n]) for n in ("o", "lse", "dq", "dk", "dv")}
    fin = torch.isfinite(want["lse"])
    out["lse_abs"] = (got["lse"].double()[fin] - want["lse"][fin]).abs().max().item()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_against_fp64_oracle(C, case):
    _, got, want = _case(C, case, 0)
    for n in ("o", "dq", "dk", "dv"):
        assert torch.isfinite(got[n]).all(), n
    # rows without a visible key: lse = -inf there and nowhere else
    assert torch.equal(torch.isinf(got["lse"]), torch.isinf(want["lse"]))
    assert not torch.isnan(got["lse"]).any()
    assert (got["lse"][torch.isinf(got["lse"])] < 0).all()
    fig = measure(C, case, 0)
    print(case, {n: f"{fig[n]:.6e}" for n in OUTPUTS})
    for n in OUTPUTS:
        assert fig[n] <= PARENT_MAX[case][n], (case, n, fig[n], PARENT_MAX[case][n])


def test_rows_without_keys_are_exact_zeros(C):
    """Skv < Sq under the causal mask: q rows 0-127 see no key.  o and dq are
    exactly 0 there and lse is -inf; everything else is finite."""
    _, got, want = _case(C, "offset_neg", 0)
    empty = torch.isinf(want["lse"])          # [B, Hq, Sq]
    assert empty[0, :, :128].all() and not empty[0, :, 128:].any()
    assert (got["lse"][empty] == -math.inf).all()
    rows = empty.permute(0, 2, 1)             # [B, Sq, Hq]
    assert (got["o"][rows] == 0).all()
    assert (got["dq"][rows] == 0).all()
    for n in ("o", "dq", "dk", "dv"):
        assert torch.isfinite(got[n]).all(), n


def test_two_launches_are_bit_equal(C):
    (q, k, v, do, se), first, _ = _case(C, "full_and_diag320", 0)
    second = run_kernels(C, q, k, v, do, True, se)
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(first[n], second[n]), n
