"""CPU checks of the float64 oracles in ops.reference for the training
elementwise kernels (rms_norm, rope, swiglu, cross_entropy, adamw) and of the
comparison rule the GPU tests apply (tests/test_train_ops_edges_gpu.py):

(a) every written-out backward oracle equals float64 autograd of the forward;
(b) the rule accepts a torch emulation of each kernel (fp32 arithmetic in the
    kernel's order, one final bf16 rounding) at the op's constant ORACLE_C;
(c) the rule rejects deliberately wrong emulations even at the cap
    ORACLE_C_CAP = 2^-12, which no op's constant may exceed.
"""
import pytest
import torch

from paddlenlp_amd.ops import reference as ref

BF = torch.bfloat16
CAP = ref.ORACLE_C_CAP


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(BF)


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _passes(op, out, want, scale, **kw):
    return ref.oracle_close(out, want, scale, ref.ORACLE_C[op], **kw)


def _fails_at_cap(out, want, scale, **kw):
    return not ref.oracle_close(out, want, scale, CAP, **kw)


def test_constants_respect_the_cap():
    assert set(ref.ORACLE_C) == {"rms_norm", "rope", "swiglu", "cross_entropy", "adamw"}
    for op, c in ref.ORACLE_C.items():
        assert 0 < c <= CAP, (op, c)


def test_rule_itself():
    want = torch.tensor([1.0, -3.0, 0.0], dtype=torch.float64)
    scale = want.abs()
    # exact bf16 roundings pass with c = 0, fp32 outputs get no R
    assert ref.oracle_close(torch.tensor([1.0, -3.0, 0.0], dtype=BF), want, scale, 0.0)
    assert ref.oracle_close((want * (1 + 2.0 ** -9)).to(BF), want, scale, 0.0)
    assert not ref.oracle_close(want.float() * (1 + 2.0 ** -9), want, scale, CAP)
    # one bf16 ulp off fails, an error where scale is 0 fails, NaN fails
    assert not ref.oracle_close(torch.tensor([1.0078125, -3.0, 0.0], dtype=BF), want, scale, CAP)
    assert not ref.oracle_close(torch.tensor([1.0, -3.0, 1e-30], dtype=BF), want, scale, CAP)
    assert not ref.oracle_close(torch.tensor([1.0, float("nan"), 0.0], dtype=BF), want, scale, CAP)
    # below the smallest normal a bf16 result may be flushed to 0, above it not
    tiny = torch.tensor([1e-38], dtype=torch.float64)
    assert ref.oracle_close(torch.zeros(1, dtype=BF), tiny, tiny, 0.0)
    assert not ref.oracle_close(torch.zeros(1, dtype=BF), tiny * 2, tiny * 2, CAP)
    assert not ref.oracle_close(torch.zeros(1), tiny, tiny, CAP)      # fp32: no allowance


# ---------------------------------------------------------------------------
# (a) written-out backward == float64 autograd of the forward oracle
# ---------------------------------------------------------------------------
def _same(a, b, scale):
    return bool(((a - b).abs() <= 1e-12 * (1 + scale)).all())


def test_rms_norm_bwd_oracle_is_the_gradient():
    g = _gen(1)
    x = torch.randn(5, 24, dtype=torch.float64, generator=g, requires_grad=True)
    w = torch.randn(24, dtype=torch.float64, generator=g, requires_grad=True)
    dy = torch.randn(5, 24, dtype=torch.float64, generator=g)
    (ref.rms_norm_oracle(x, w, 1e-6)["y"] * dy).sum().backward()
    o = ref.rms_norm_bwd_oracle(dy, x.detach(), w.detach(), 1e-6)
    assert _same(o["dx"], x.grad, o["dx_scale"])
    assert _same(o["dw"], w.grad, o["dw_scale"])


def test_rope_bwd_oracle_is_the_gradient():
    g = _gen(2)
    cos, sin = ref.build_rope_cache(6, 16)
    for H in (3, 1):
        x = torch.randn(2, 6, H, 16, dtype=torch.float64, generator=g, requires_grad=True)
        dout = torch.randn(2, 6, H, 16, dtype=torch.float64, generator=g)
        (ref.rope_oracle(x, cos, sin)[0] * dout).sum().backward()
        dx, scale = ref.rope_oracle(dout, cos, sin, backward=True)
        assert _same(dx, x.grad, scale)


def test_swiglu_bwd_oracle_is_the_gradient():
    g = _gen(3)
    x = torch.randn(4, 32, dtype=torch.float64, generator=g) * 3
    x[0, :4] = torch.tensor([0.0, -0.0, 30.0, -30.0], dtype=torch.float64)
    x.requires_grad_()
    dy = torch.randn(4, 16, dtype=torch.float64, generator=g)
    (ref.swiglu_oracle(x)[0] * dy).sum().backward()
    o = ref.swiglu_bwd_oracle(dy, x.detach())
    want_dg, want_du = x.grad.chunk(2, dim=-1)
    assert _same(o["dg"], want_dg, o["dg_scale"])
    assert _same(o["du"], want_du, o["du_scale"])


def test_cross_entropy_bwd_oracle_is_the_gradient():
    g = _gen(4)
    l = torch.randn(6, 16, dtype=torch.float64, generator=g) * 4
    l[2, 3:6] = float("-inf")
    labels = torch.tensor([0, 15, 7, -100, 5, 5])
    dloss = torch.randn(6, dtype=torch.float64, generator=g)
    l.requires_grad_()
    (ref.cross_entropy_oracle(l, labels)["loss"] * dloss).sum().backward()
    o = ref.cross_entropy_oracle(l.detach(), labels, dloss=dloss)
    assert _same(o["dlogits"], l.grad, o["dlogits_scale"])
    assert (o["dlogits"][3] == 0).all() and (o["dlogits"][2, 3:6] == 0).all()
    assert o["loss"][3] == 0 and torch.isfinite(o["loss"]).all()
    # and the forward is torch's own float64 cross entropy
    want = torch.nn.functional.cross_entropy(l.detach(), labels, reduction="none")
    assert _same(o["loss"], want, o["loss_scale"])


def test_adamw_oracle_matches_torch_adamw():
    """Three steps of torch.optim.AdamW in float64, scalars exact in fp32."""
    g = _gen(5)
    lr, b1, b2, eps, wd = 2.0 ** -10, 0.875, 0.9990234375, 2.0 ** -27, 0.125
    p = torch.randn(37, dtype=torch.float64, generator=g).requires_grad_()
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    orc = ref.AdamWOracle(p.detach().float(), torch.float32, lr, b1, b2, eps, wd)
    p.data = p.detach().float().double()
    for _ in range(3):
        grad = torch.randn(37, generator=g)
        before = p.detach().clone()
        p.grad = grad.double()
        opt.step()
        o = orc.step(grad)
        assert _same(o["delta"], p.detach() - before, o["delta"].abs())
        assert _same(o["w"], p.detach(), o["w"].abs())
        assert _same(o["m"], opt.state[p]["exp_avg"], o["m_scale"])
        assert _same(o["v"], opt.state[p]["exp_avg_sq"], o["v_scale"])


def test_adamw_oracle_reads_the_gradient_in_the_param_dtype():
    grad = torch.tensor([1.00390625, -2.0])        # 1 + 2^-8: not a bf16 number
    a = ref.AdamWOracle(torch.zeros(2), BF, 1e-3, 0.9, 0.999, 1e-8, 0.0).step(grad)
    b = ref.AdamWOracle(torch.zeros(2), BF, 1e-3, 0.9, 0.999, 1e-8, 0.0).step(grad.to(BF))
    c = ref.AdamWOracle(torch.zeros(2), torch.float32, 1e-3, 0.9, 0.999, 1e-8, 0.0).step(grad)
    assert torch.equal(a["m"], b["m"]) and not torch.equal(a["m"], c["m"])


# ---------------------------------------------------------------------------
# (b) + (c) emulations of the kernels: fp32 in the kernel's order, one bf16
# rounding at the end; `bug` selects a deliberately wrong variant
# ---------------------------------------------------------------------------
def _rnd(t, on):
    """A stray bf16 rounding of an intermediate."""
    return t.to(BF).float() if on else t


def _emu_rms_fwd(x, w, eps, bug=None):
    x32, w32 = x.float(), w.float()
    H = x.shape[-1]
    ss = (x32 * x32).sum(-1, keepdim=True)
    inv = torch.rsqrt(ss / (H + 8 if bug == "mean_h8" else H) + _f32(eps))
    y = _rnd(x32 * inv, bug == "round") * w32
    return y.to(BF), inv.squeeze(-1)


def _emu_rms_bwd(dy, x, w, inv, bug=None):
    dy32, x32, w32, inv = dy.float(), x.float(), w.float(), inv[:, None]
    H = x.shape[-1]
    c = (dy32 * w32 * x32).sum(-1, keepdim=True)
    k = c * inv * inv / H
    dx = inv * _rnd(dy32 * w32 - x32 * k, bug == "round")
    dw = (_rnd(dy32 * x32, bug == "round") * inv).sum(0)
    return dx.to(BF), dw.to(BF)


def _rms_case():
    x = _bf(6, 40, seed=10)
    x[1] = 0
    x[2] *= 1024
    return x, _bf(40, seed=11), _bf(6, 40, seed=12), 1e-6


def test_rms_norm_emulation_passes():
    x, w, dy, eps = _rms_case()
    y, inv = _emu_rms_fwd(x, w, eps)
    o = ref.rms_norm_oracle(x, w, eps)
    assert _passes("rms_norm", y, o["y"], o["y_scale"])
    assert _passes("rms_norm", inv, o["invrms"], o["invrms_scale"])
    dx, dw = _emu_rms_bwd(dy, x, w, inv)
    b = ref.rms_norm_bwd_oracle(dy, x, w, eps)
    assert _passes("rms_norm", dx, b["dx"], b["dx_scale"])
    assert _passes("rms_norm", dw, b["dw"], b["dw_scale"])


@pytest.mark.parametrize("bug", ["round", "mean_h8"])
def test_rms_norm_mutants_fail(bug):
    x, w, dy, eps = _rms_case()
    o = ref.rms_norm_oracle(x, w, eps)
    b = ref.rms_norm_bwd_oracle(dy, x, w, eps)
    y, inv = _emu_rms_fwd(x, w, eps, bug)
    assert _fails_at_cap(y, o["y"], o["y_scale"])
    if bug == "mean_h8":
        assert _fails_at_cap(inv, o["invrms"], o["invrms_scale"])
        return
    dx, dw = _emu_rms_bwd(dy, x, w, _emu_rms_fwd(x, w, eps)[1], bug)
    assert _fails_at_cap(dx, b["dx"], b["dx_scale"])
    assert _fails_at_cap(dw, b["dw"], b["dw_scale"])


def _emu_rope(x, cos, sin, backward=False, bug=None):
    """x [B, S, H, D]; the kernel's rope_pair."""
    S, D = cos.shape
    half = D // 2
    pos = torch.arange(S)
    if bug == "pos_plus_1":
        pos = (pos + 1) % S
    c = cos.float()[pos][None, :, None, :]
    s = sin.float()[pos][None, :, None, :]
    sign = -1.0 if backward and bug != "sin_sign" else 1.0
    x32 = x.float()
    a, b = x32[..., :half], x32[..., half:]
    o1 = _rnd(a * c[..., :half], bug == "round") - _rnd(sign * b * s[..., :half], bug == "round")
    o2 = _rnd(b * c[..., half:], bug == "round") + _rnd(sign * a * s[..., half:], bug == "round")
    return torch.cat((o1, o2), dim=-1).to(BF)


def _rope_case():
    cos, sin = ref.build_rope_cache(9, 16)
    return _bf(2, 9, 3, 16, seed=20), _bf(2, 9, 1, 16, seed=21), cos, sin


def test_rope_emulation_passes():
    q, k, cos, sin = _rope_case()
    for x in (q, k):
        for backward in (False, True):
            want, scale = ref.rope_oracle(x, cos, sin, backward)
            assert _passes("rope", _emu_rope(x, cos, sin, backward), want, scale)


def test_rope_mutants_fail():
    q, k, cos, sin = _rope_case()
    for backward in (False, True):
        want, scale = ref.rope_oracle(q, cos, sin, backward)
        assert _fails_at_cap(_emu_rope(q, cos, sin, backward, "round"), want, scale)
    want, scale = ref.rope_oracle(q, cos, sin, True)
    assert _fails_at_cap(_emu_rope(q, cos, sin, True, "sin_sign"), want, scale)
    want, scale = ref.rope_oracle(k, cos, sin, False)
    assert _fails_at_cap(_emu_rope(k, cos, sin, False, "pos_plus_1"), want, scale)


def _emu_swiglu(x, dy=None, bug=None):
    g, u = x.float().chunk(2, dim=-1)
    sig = 1.0 / (1.0 + torch.exp(-g))
    if dy is None:
        return (_rnd(g * sig, bug == "round") * u).to(BF)
    dy32 = dy.float()
    dg = _rnd(dy32 * u * sig, bug == "round") * (1.0 + g * (1.0 - sig))
    du = dy32 * (sig if bug == "du_sig" else _rnd(g * sig, bug == "round"))
    return dg.to(BF), du.to(BF)


def _swiglu_case():
    x = _bf(5, 48, seed=30)
    x[0, :6] = torch.tensor([0.0, -0.0, 88.0, -88.0, 100.0, -100.0]).to(BF)
    return x, _bf(5, 24, seed=31)


def test_swiglu_emulation_passes():
    x, dy = _swiglu_case()
    want, scale = ref.swiglu_oracle(x)
    assert _passes("swiglu", _emu_swiglu(x), want, scale)
    dg, du = _emu_swiglu(x, dy)
    b = ref.swiglu_bwd_oracle(dy, x)
    assert _passes("swiglu", dg, b["dg"], b["dg_scale"])
    assert _passes("swiglu", du, b["du"], b["du_scale"])


def test_swiglu_mutants_fail():
    x, dy = _swiglu_case()
    want, scale = ref.swiglu_oracle(x)
    b = ref.swiglu_bwd_oracle(dy, x)
    assert _fails_at_cap(_emu_swiglu(x, bug="round"), want, scale)
    dg, du = _emu_swiglu(x, dy, "round")
    assert _fails_at_cap(dg, b["dg"], b["dg_scale"])
    assert _fails_at_cap(du, b["du"], b["du_scale"])
    dg, du = _emu_swiglu(x, dy, "du_sig")
    assert _passes("swiglu", dg, b["dg"], b["dg_scale"])
    assert _fails_at_cap(du, b["du"], b["du_scale"])


def _emu_ce(logits, labels, dloss, ignore_index=-100, bug=None):
    l = logits.float()
    N, V = l.shape
    keep = labels != ignore_index
    y = torch.where(keep, labels, torch.zeros_like(labels))
    if bug == "target_off_by_one":
        y = (y + 1) % V
    m = l.max(-1, keepdim=True).values
    se = torch.exp(l - m).sum(-1, keepdim=True)
    lse = se.log()
    loss = torch.where(keep, _rnd(lse, bug == "round").squeeze(1) - (l.gather(1, y[:, None]) - m).squeeze(1),
                       torch.zeros(N))
    dl = dloss.float() if bug == "ignored_not_zeroed" else torch.where(keep, dloss.float(), torch.zeros(N))
    p = _rnd(torch.exp(l - m) * torch.exp(-lse), bug == "round")
    onehot = torch.zeros_like(p)
    onehot[keep, y[keep]] = 1.0
    return loss, (m + lse).squeeze(1), (dl[:, None] * (p - onehot)).to(BF)


def _ce_case():
    l = _bf(6, 40, seed=40, scale=3.0)
    l[1] = 1.5
    l[2, 5:9] = float("-inf")
    labels = torch.tensor([0, 39, 20, -100, 7, int(l[5].float().argmax())])
    dloss = torch.randn(6, generator=_gen(41))
    return l, labels, dloss


def test_cross_entropy_emulation_passes():
    l, labels, dloss = _ce_case()
    loss, full, dlogits = _emu_ce(l, labels, dloss)
    o = ref.cross_entropy_oracle(l, labels, dloss=dloss)
    assert _passes("cross_entropy", loss, o["loss"], o["loss_scale"])
    assert _passes("cross_entropy", full, o["full"], o["full_scale"])
    assert _passes("cross_entropy", dlogits, o["dlogits"], o["dlogits_scale"],
           floor=o["dlogits_floor"])


@pytest.mark.parametrize("bug", ["round", "target_off_by_one", "ignored_not_zeroed"])
def test_cross_entropy_mutants_fail(bug):
    l, labels, dloss = _ce_case()
    loss, full, dlogits = _emu_ce(l, labels, dloss, bug=bug)
    o = ref.cross_entropy_oracle(l, labels, dloss=dloss)
    assert _fails_at_cap(dlogits, o["dlogits"], o["dlogits_scale"],
           floor=o["dlogits_floor"])
    if bug != "ignored_not_zeroed":
        assert _fails_at_cap(loss, o["loss"], o["loss_scale"])


def _emu_adamw(p, g, m, v, master, lr, b1, b2, eps, wd, step, bug=None):
    """One kernel step on clones; returns (p, m, v, master) after it."""
    lr, b1, b2, eps, wd = (_f32(h) for h in (lr, b1, b2, eps, wd))
    one = _f32(1.0)
    g32 = g.to(p.dtype).float()
    w = (master if master is not None else p).clone()
    bias1 = one - b1.pow(step)
    bias2 = one - b2.pow(step - 1 if bug == "bias2_prev_step" else step)
    inv_b1, inv_b2, decay = one / bias1, one / bias2, one - lr * wd
    m2 = b1 * m + (one - b1) * g32
    v2 = b2 * v + (one - b2) * g32 * g32
    denom = torch.sqrt(v2 * inv_b2) + eps
    w2 = w * decay - lr * _rnd(m2 * inv_b1, bug == "round") / denom
    if bug == "tail_untouched":
        n4 = (p.numel() // 4) * 4
        m2[n4:], v2[n4:], w2[n4:] = m[n4:], v[n4:], w[n4:]
    return w2.to(p.dtype), m2, v2, w2


def _adamw_run(dtype, bug=None, n=11, wd=0.1):
    """Three steps; the comparison of every step as a list of bools."""
    g = _gen(50)
    hyper = (1e-3, 0.9, 0.999, 1e-8, wd)
    master = torch.randn(n, generator=g)
    p = master.to(dtype)
    if dtype == BF:
        master = p.float()
    m, v = torch.zeros(n), torch.zeros(n)
    orc = ref.AdamWOracle(master, dtype, *hyper)
    c = CAP if bug else ref.ORACLE_C["adamw"]
    ok = []
    for step in (1, 2, 3):
        grad = torch.randn(n, generator=g)
        before = master
        o = orc.step(grad, state=(m, v, before))
        p, m, v, master = _emu_adamw(p, grad, m, v, before, *hyper, step, bug=bug)
        delta = master.double() - before.double()
        ok.append(ref.oracle_close(m, o["m"], o["m_scale"], c)
                  and ref.oracle_close(v, o["v"], o["v_scale"], c)
                  and ref.oracle_close(delta, o["delta"], o["delta"].abs(), c, R=0.0,
                                       floor=2.0 ** -22 * before.double().abs())
                  and torch.equal(p, master.to(dtype)))
    return ok


@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adamw_emulation_passes(dtype, wd):
    assert _adamw_run(dtype, wd=wd) == [True, True, True]


def test_adamw_mutants_fail():
    # bias2 of step 0 is 0: the first step already goes wrong (division by 0)
    assert _adamw_run(BF, "bias2_prev_step") == [False, False, False]
    assert _adamw_run(BF, "tail_untouched") == [False, False, False]
    assert _adamw_run(BF, "tail_untouched", n=12) == [True, True, True]   # no tail
    # at step 1 m/bias1 is the bf16 gradient itself, so rounding it is no error
    assert _adamw_run(BF, "round") == [True, False, False]
