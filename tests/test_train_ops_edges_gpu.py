"""Edge-shape checks of the training elementwise kernels (rms_norm, rope,
swiglu, cross_entropy, adamw) against the float64 oracles of ops.reference.

Every numeric check is ops.reference's rule |out - ref| <= R|ref| + c*scale
with the op's constant ORACLE_C (tests/test_train_ops_oracle.py shows on the
CPU what that rule accepts and rejects).  Each check prints the c it needed
before it asserts, which is how the constants were measured.  The layout and
mixed-dtype tests compare bit for bit.

Known precondition, not tested: cross-entropy labels are either ignore_index
or in [0, V); the kernel reads logits[row, label] unchecked.
"""
import pytest
import torch

from paddlenlp_amd import ops
from paddlenlp_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def C():
    from paddlenlp_amd.ops.functional import _load_extension

    return _load_extension()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, dtype=BF, scale=1.0):
    """Seeded on the CPU, so the values do not depend on the device."""
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(dtype).to(DEV)


def _check(op, what, out, want, scale, **kw):
    need = float(ref.oracle_margin(out, want, scale, **kw).max())
    print(f"[margin] {op} {what}: {need:.4e}")
    assert need <= ref.ORACLE_C[op], (op, what, need)


# ---------------------------------------------------------------------------
# rms_norm: H = 8; NV = 2 with a partly filled second slot (2056); NV = 3
# promoted to 4 with a masked slot (5120); NV = 4 full (8192); the streaming
# path (8200); more rows than the forward grid and several rows per backward
# block (8200 rows)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows,H", [(5, 8), (3, 2056), (4, 5120), (3, 8192), (2, 8200),
                                    (8200, 64)])
def test_rms_norm_edges(C, rows, H):
    eps = 1e-6
    x = _randn(rows, H, seed=rows + H)
    x[rows - 1] = 0                 # inv = rsqrt(eps)
    x[rows - 2] *= 1024
    w = _randn(H, seed=H + 1)
    assert (w > 0).any() and (w < 0).any()
    dy = _randn(rows, H, seed=H + 2)

    y, inv = C.rms_norm_fwd(x, w, eps)
    o = ref.rms_norm_oracle(x, w, eps)
    _check("rms_norm", "y", y, o["y"], o["y_scale"])
    _check("rms_norm", "invrms", inv, o["invrms"], o["invrms_scale"])
    assert y.dtype == BF and inv.dtype == torch.float32

    dx, dw = C.rms_norm_bwd(dy, x, w, inv)
    b = ref.rms_norm_bwd_oracle(dy, x, w, eps)
    _check("rms_norm", "dx", dx, b["dx"], b["dx_scale"])
    _check("rms_norm", "dw", dw, b["dw"], b["dw_scale"])
    assert dx.dtype == BF and dw.dtype == BF


# ---------------------------------------------------------------------------
# rope: q, k, dq and dk; Hq != Hk with B > 1 (the position is (row / H) % S);
# the last shape needs more threads than the grid holds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,Hq,Hk,D", [(2, 7, 3, 1, 8), (1, 33, 2, 2, 32), (3, 5, 4, 2, 64),
                                         (4, 1040, 8, 2, 128)])
def test_rope_edges(C, B, S, Hq, Hk, D):
    cos, sin = ops.build_rope_cache(S, D, device=DEV)
    assert cos.shape == (S, D) and cos.dtype == torch.float32
    q = _randn(B, S, Hq, D, seed=S)
    k = _randn(B, S, Hk, D, seed=S + 1)
    dq = _randn(B, S, Hq, D, seed=S + 2)
    dk = _randn(B, S, Hk, D, seed=S + 3)
    if B * S * Hq * (D // 8) > 2048 * 256:
        assert B * S * Hk * (D // 8) <= 2048 * 256   # k stays within one pass
    for backward, (a, b) in ((False, (q, k)), (True, (dq, dk))):
        a_out, b_out = C.rope_fwd(a, b, cos, sin, backward)
        tag = "d" if backward else ""
        _check("rope", tag + "q", a_out, *ref.rope_oracle(a, cos, sin, backward))
        _check("rope", tag + "k", b_out, *ref.rope_oracle(b, cos, sin, backward))


# ---------------------------------------------------------------------------
# swiglu: one vector, a few, and more than the grid holds; gates at +-0 and on
# both sides of where exp(-g) over- and underflows in fp32
# ---------------------------------------------------------------------------
_SPECIAL_GATES = [0.0, -0.0, 88.0, -88.0, 100.0, -100.0]


@pytest.mark.parametrize("N,I", [(1, 8), (3, 24), (1030, 4096)])
def test_swiglu_edges(C, N, I):
    x = _randn(N, 2 * I, seed=N + I)
    special = torch.tensor(_SPECIAL_GATES, dtype=BF, device=DEV)
    x[0, :6] = special
    x[N - 1, I - 6:I] = special      # the last gate columns of the last row
    if N * I // 8 > 2048 * 256:
        spots = torch.randint(0, I, (N, 6), generator=_gen(7)).to(DEV)
        x[:, :I].scatter_(1, spots, special.expand(N, 6).contiguous())
    dy = _randn(N, I, seed=N + I + 1)

    y = C.swiglu_fwd(x)
    _check("swiglu", "y", y, *ref.swiglu_oracle(x))
    dx = C.swiglu_bwd(dy, x)
    b = ref.swiglu_bwd_oracle(dy, x)
    _check("swiglu", "dg", dx[:, :I], b["dg"], b["dg_scale"])
    _check("swiglu", "du", dx[:, I:], b["du"], b["du_scale"])
    # "0 or g": at g = -100 the output is 0, at g = +100 it is g * u
    g, u = x[:, :I].float(), x[:, I:].float()
    assert (y.float()[g == -100] == 0).all()
    assert torch.equal(y[g == 100], (100 * u[g == 100]).to(BF))


# ---------------------------------------------------------------------------
# cross_entropy: V = 8; V one vector past the block's pass (4104); several
# passes (32000); more rows than the grid (4100)
# ---------------------------------------------------------------------------
def _ce_case(N, V):
    """Row 0: logits spanning -80..+80 with the target at the minimum (column
    0), the maximum in column 1 and -inf in three other columns.  (With the
    target at the maximum of such a row the loss is exp(-gap), below the fp32
    resolution of the sum 1 + exp(-gap); the target there is the minimum.)
    Row 1: all logits equal, label V - 1.  Row 2: ignored.  Row 3: target at
    the arg max.  The rest: 3 * randn with random labels, some 0 and V - 1,
    every seventh row ignored."""
    l = torch.randn(N, V, generator=_gen(N + V)) * 3
    labels = torch.randint(0, V, (N,), generator=_gen(N + V + 1))
    l[0] *= 79 / l[0].abs().max()
    l[0, 0], l[0, 1] = -80, 80
    l[0, [2, 3, 5]] = float("-inf")
    labels[0] = 0
    l[1] = 1.5
    labels[1] = V - 1
    labels[2] = -100
    l = l.to(BF)
    if N > 3:
        labels[3] = l[3].float().argmax()
    if N > 8:
        labels[4], labels[5] = 0, V - 1
        labels[6::7] = -100
        labels[N - 2], labels[N - 1] = V - 1, -100    # in the second pass of the row loop
    dloss = torch.randn(N, generator=_gen(N + V + 2))
    return l.to(DEV), labels.to(DEV), dloss.to(DEV)


@pytest.mark.parametrize("N,V", [(3, 8), (5, 4104), (4, 32000), (4100, 1024)])
def test_cross_entropy_edges(C, N, V):
    l, labels, dloss = _ce_case(N, V)
    loss, maxlse = C.cross_entropy_fwd(l, labels, -100)
    dlogits = C.cross_entropy_bwd(dloss, l, labels, maxlse, -100)
    o = ref.cross_entropy_oracle(l, labels, -100, dloss=dloss)
    assert torch.isfinite(o["loss"]).all() and torch.isfinite(o["dlogits"]).all()

    assert loss.dtype == torch.float32 and maxlse.dtype == torch.float32
    assert torch.equal(maxlse[:, 0].double().cpu(), o["max"])
    _check("cross_entropy", "loss", loss, o["loss"], o["loss_scale"])
    full = maxlse[:, 0].double() + maxlse[:, 1].double()
    _check("cross_entropy", "lse", full, o["full"], o["full_scale"], R=0.0)
    _check("cross_entropy", "dlogits", dlogits, o["dlogits"], o["dlogits_scale"],
           floor=o["dlogits_floor"])

    ignored = labels == -100
    assert ignored.any() and (~ignored).any()
    assert (loss[ignored] == 0).all() and (dlogits[ignored] == 0).all()
    assert (dlogits[0, [2, 3, 5]] == 0).all()         # the -inf columns


def test_cross_entropy_all_ignored_mean(C):
    l = _randn(6, 40, seed=3).requires_grad_()
    labels = torch.full((6,), -100, device=DEV)
    loss = ops.cross_entropy(l, labels, reduction="mean")
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert torch.equal(l.grad, torch.zeros_like(l))


# ---------------------------------------------------------------------------
# adamw
# ---------------------------------------------------------------------------
_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


class _AdamTensor:
    """One parameter with its kernel state and its oracle."""

    def __init__(self, n, dtype, wd, seed):
        self.n, self.dtype, self.seed = n, dtype, seed
        start = torch.randn(n, generator=_gen(seed))
        self.p = start.to(dtype).to(DEV)
        self.master = self.p.float() if dtype == BF else None
        self.m = torch.zeros(n, device=DEV)
        self.v = torch.zeros(n, device=DEV)
        self.oracle = ref.AdamWOracle(self.weights(), dtype, weight_decay=wd, **_HYPER)

    def weights(self):
        return self.master if self.master is not None else self.p

    def new_grad(self, step, dtype):
        g = torch.randn(self.n, generator=_gen(self.seed * 16 + step))
        g[4::5] = 0         # v = 0 there on the first step: the update is 0 / eps
        return g.to(dtype).to(DEV)

    def state(self):
        return self.m.clone(), self.v.clone(), self.weights().clone()

    def check(self, grad, state, what):
        """`state`: (m, v, weights) from before the kernel's step."""
        o = self.oracle.step(grad, state)
        before = state[2]
        _check("adamw", what + " m", self.m, o["m"], o["m_scale"])
        _check("adamw", what + " v", self.v, o["v"], o["v_scale"])
        delta = self.weights().double() - before.double()
        _check("adamw", what + " delta", delta, o["delta"], o["delta"].abs(), R=0.0,
               floor=2.0 ** -22 * before.double().abs().cpu())
        if self.master is not None:
            assert torch.equal(self.p, self.master.to(BF)), what


def _adamw_steps(C, tensors, wd, steps, grad_dtype=None):
    for step in range(1, steps + 1):
        grads = [t.new_grad(step, grad_dtype or t.dtype) for t in tensors]
        before = [t.state() for t in tensors]
        masters = [t.master for t in tensors]
        C.fused_adamw([t.p for t in tensors], grads, [t.m for t in tensors],
                      [t.v for t in tensors], [] if masters[0] is None else masters,
                      _HYPER["lr"], _HYPER["beta1"], _HYPER["beta2"], _HYPER["eps"], wd, step)
        for i, t in enumerate(tensors):
            t.check(grads[i], before[i], f"n={t.n} step={step}")


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("n", [1, 3, 1001])
def test_adamw_bf16_sizes_three_steps(C, n, wd):
    """n = 1, 3: the scalar tail alone; 1001: vector loop and tail."""
    _adamw_steps(C, [_AdamTensor(n, BF, wd, seed=n)], wd, steps=3)


def test_adamw_bf16_across_the_chunk_boundary(C):
    """4M + 3 elements: a second host chunk that is all tail.  Two steps, so
    the second runs on non-zero moments."""
    n = 4 * 2 ** 20 + 3
    _adamw_steps(C, [_AdamTensor(n, BF, 0.1, seed=9)], 0.1, steps=2)


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adamw_fp32_params_without_masters(C, wd):
    _adamw_steps(C, [_AdamTensor(1001, torch.float32, wd, seed=21)], wd, steps=3)


def test_adamw_five_tensors_one_launch(C):
    sizes = (1, 6, 1001, 4096, 70003)
    tensors = [_AdamTensor(n, BF, 0.1, seed=30 + i) for i, n in enumerate(sizes)]
    _adamw_steps(C, tensors, 0.1, steps=3)


def test_adamw_fp32_grads_for_bf16_params(C):
    """Each converted gradient has to live until the launch: two params of
    equal numel, so that a released conversion buffer would be reused by the
    next one, each checked against its own oracle."""
    tensors = [_AdamTensor(1001, BF, 0.0, seed=40), _AdamTensor(1001, BF, 0.0, seed=41)]
    _adamw_steps(C, tensors, 0.0, steps=2, grad_dtype=torch.float32)
    assert not torch.equal(tensors[0].m, tensors[1].m)


def test_adamw_rejects_inconsistent_arguments(C):
    t = _AdamTensor(16, BF, 0.0, seed=50)
    g = t.new_grad(1, BF)
    args = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    with pytest.raises(RuntimeError):
        C.fused_adamw([t.p], [g], [t.m, t.m], [t.v], [t.master], *args)
    with pytest.raises(RuntimeError):
        C.fused_adamw([t.p], [g], [t.m[:8]], [t.v], [t.master], *args)
    with pytest.raises(RuntimeError):
        C.fused_adamw([t.p], [g], [t.m], [t.v.to(BF)], [t.master], *args)
    with pytest.raises(RuntimeError):
        C.fused_adamw([t.p], [g], [t.m], [t.v], [t.master[:8]], *args)
    with pytest.raises(RuntimeError):
        C.fused_adamw([t.p], [g[:8]], [t.m], [t.v], [t.master], *args)


# ---------------------------------------------------------------------------
# layout: a public wrapper given a non-contiguous input returns what it
# returns for .contiguous() of the same data, bit for bit
# ---------------------------------------------------------------------------
def _leaf(t):
    return t.detach().requires_grad_()


def _column_slice(rows, cols, seed):
    return _randn(rows, cols + 24, seed=seed)[:, :cols]


def _transposed(rows, cols, seed):
    return _randn(cols, rows, seed=seed).t()


@pytest.mark.parametrize("make", [_column_slice, _transposed])
def test_rms_norm_layout(C, make):
    # two rows: the sum of dw's two fp32 partials does not depend on the
    # order of the reduce kernel's atomics
    x_nc = make(2, 264, seed=60)
    dy_nc = make(2, 264, seed=61)
    assert not x_nc.is_contiguous() and not dy_nc.is_contiguous()
    w = _randn(264, seed=62)
    got, want = [], []
    for out, x, dy in ((got, x_nc, dy_nc), (want, x_nc.contiguous(), dy_nc.contiguous())):
        x, wl = _leaf(x), _leaf(w)
        y = ops.rms_norm(x, wl, 1e-6)
        y.backward(dy)
        out += [y.detach(), x.grad, wl.grad]
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("make", [_column_slice, _transposed])
def test_swiglu_layout(C, make):
    x_nc = make(5, 48, seed=63)
    dy_nc = make(5, 24, seed=64)
    assert not x_nc.is_contiguous() and not dy_nc.is_contiguous()
    got, want = [], []
    for out, x, dy in ((got, x_nc, dy_nc), (want, x_nc.contiguous(), dy_nc.contiguous())):
        x = _leaf(x)
        y = ops.swiglu(x)
        y.backward(dy)
        out += [y.detach(), x.grad]
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("make", [_column_slice, _transposed])
def test_cross_entropy_layout(C, make):
    """A column slice is what logits_padded[:, :V] of a padded vocabulary is."""
    N, V = 9, 40
    l_nc = make(N, V, seed=65)
    assert not l_nc.is_contiguous()
    labels = torch.randint(0, V, (N,), generator=_gen(66)).to(DEV)
    labels[4] = -100
    weights = _randn(N, seed=67, dtype=torch.float32)
    got, want = [], []
    for out, l in ((got, l_nc), (want, l_nc.contiguous())):
        l = _leaf(l)
        loss = ops.cross_entropy(l, labels)
        (loss * weights).sum().backward()
        mean = ops.cross_entropy(l.detach(), labels, reduction="mean")
        out += [loss.detach(), mean, l.grad]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # and the gradient is the right one, not only the same one
    o = ref.cross_entropy_oracle(l_nc, labels, dloss=weights)
    _check("cross_entropy", "dlogits of a view", got[2], o["dlogits"], o["dlogits_scale"],
           floor=o["dlogits_floor"])


def _packed_qk(B, S, Hq, Hk, D, seed):
    """q and k as the views of a packed qkv projection."""
    qkv = _randn(B, S, (Hq + 2 * Hk) * D, seed=seed)
    q, k, _ = qkv.split([Hq * D, Hk * D, Hk * D], dim=-1)
    return q.view(B, S, Hq, D), k.view(B, S, Hk, D)


def _transposed_qk(B, S, Hq, Hk, D, seed):
    return (_randn(B, Hq, S, D, seed=seed).transpose(1, 2),
            _randn(B, Hk, S, D, seed=seed + 1).transpose(1, 2))


@pytest.mark.parametrize("make", [_packed_qk, _transposed_qk])
def test_fused_rope_layout(C, make):
    B, S, Hq, Hk, D = 2, 5, 4, 2, 16
    q_nc, k_nc = make(B, S, Hq, Hk, D, seed=68)
    dq_nc, dk_nc = make(B, S, Hq, Hk, D, seed=78)
    for t in (q_nc, k_nc, dq_nc, dk_nc):
        assert not t.is_contiguous()
    cos, sin = ops.build_rope_cache(S, D, device=DEV)
    got, want = [], []
    for out, q, k, dq, dk in ((got, q_nc, k_nc, dq_nc, dk_nc),
                              (want, q_nc.contiguous(), k_nc.contiguous(),
                               dq_nc.contiguous(), dk_nc.contiguous())):
        q, k = _leaf(q), _leaf(k)
        q1, k1 = ops.fused_rope(q, k, cos, sin)
        torch.autograd.backward([q1, k1], [dq, dk])
        out += [q1.detach(), k1.detach(), q.grad, k.grad]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    _check("rope", "dk of a view", got[3], *ref.rope_oracle(dk_nc, cos, sin, True))


def test_bindings_reject_strided_saved_tensors(C):
    """The backward bindings read their saved inputs with dense strides; a
    view has to raise, not miscompute."""
    l = _column_slice(4, 16, seed=71)
    labels = torch.zeros(4, dtype=torch.long, device=DEV)
    _, maxlse = C.cross_entropy_fwd(l.contiguous(), labels, -100)
    dloss = torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError):
        C.cross_entropy_bwd(dloss, l, labels, maxlse, -100)
    with pytest.raises(RuntimeError):
        C.cross_entropy_bwd(dloss, l.contiguous(), labels[:3], maxlse, -100)
    with pytest.raises(RuntimeError):
        C.cross_entropy_bwd(dloss, l.contiguous(), labels, maxlse[:3], -100)
    x = _column_slice(4, 32, seed=72)
    dy = _randn(4, 16, seed=73)
    with pytest.raises(RuntimeError):
        C.swiglu_bwd(dy, x)
    with pytest.raises(RuntimeError):
        C.swiglu_bwd(dy[:, :8].contiguous(), x.contiguous())
