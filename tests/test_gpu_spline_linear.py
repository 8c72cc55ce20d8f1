"""GPU: order="linear" — naz_rls_fwd / naz_rls_inv / naz_rls_bwd and the nsa / nsc flows built on
them against the float64 restatement of pyro's rational-linear spline (tests/spline_linear_ref.py),
with the same restatement in float32 as the reference-precision yardstick.

Criterion: tests/parity.py, unchanged.  Inputs: raw ~ N(0, 1), x ~ 2·N(0, 1), seeded on the CPU
(about 13 % of the inputs land in the identity tails).  The inverse is fed independent draws, not
forward outputs: on forward outputs the float32 reference itself errs by up to 7e-3 where the
slope is near 1e-4, so a round trip would test nothing.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import naz_oracle as O
from tests import spline_linear_ref as R
from tests.parity import assert_parity, grad_floor

pytestmark = pytest.mark.gpu

DEV = "cuda"
DENSE, ARN = R.LAYOUT_DENSE, R.LAYOUT_ARN
# Dt = 5, K = 5: 51 rows per workgroup, 95 floats per raw row and a ragged last block — the
# unaligned LDS copy path
CASES = [(4096, 8, 8, DENSE), (257, 5, 5, ARN), (33, 1, 8, ARN), (1, 3, 16, DENSE)]


def _cuda(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def _np(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from naz_amd import _lib
    _lib.lib()


@functools.lru_cache(maxsize=None)
def _case(B, Dt, K, layout):
    """Seeded inputs and the restatement's outputs, (y, ld) per direction and precision."""
    g = torch.Generator().manual_seed(1000 * K + 10 * Dt + layout + B)
    raw = torch.randn(B, Dt * (4 * K - 1), generator=g)
    x = 2 * torch.randn(B, Dt, generator=g)
    ref = {}
    for inverse in (False, True):
        ref[inverse, 64] = tuple(t.numpy() for t in R.rls_from_raw(x.double(), raw.double(), Dt, K, layout, inverse))
        ref[inverse, 32] = tuple(t.numpy() for t in R.rls_from_raw(x, raw, Dt, K, layout, inverse))
    return x, raw, ref


# ------------------------------------------------------------------ forward / inverse kernels
@pytest.mark.parametrize("B,Dt,K,layout", CASES)
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("fast", [False, True], ids=["libm", "fast"])
def test_rls_kernel_vs_restatement(B, Dt, K, layout, inverse, fast):
    from naz_amd import ops
    x, raw, ref = _case(B, Dt, K, layout)
    y, ld = ops.rqs(_cuda(x), _cuda(raw), K, layout, inverse=inverse, fast=fast, order="linear")
    (y64, ld64), (y32, ld32) = ref[inverse, 64], ref[inverse, 32]
    assert np.all(np.isfinite(y32)) and np.all(np.isfinite(ld32))
    print(assert_parity(_np(y), y64, y32, what="y"))
    print(assert_parity(_np(ld), ld64, ld32, what="ld"))
    tail = np.abs(x.numpy()) > 3.0
    assert np.array_equal(_np(y)[tail], x.double().numpy()[tail]) and np.all(_np(ld)[tail] == 0)


@pytest.mark.parametrize("B,Dt,K,layout", CASES + [(0, 5, 5, ARN)])
@pytest.mark.parametrize("inverse", [False, True])
def test_rls_evaluators_agree(B, Dt, K, layout, inverse):
    """Both evaluators, from one set of inputs, are within the criterion of the same reference
    (the float64 restatement, the float32 restatement as yardstick, as in every test here), and
    they return the same tails; B = 0 returns empty results without a launch."""
    from naz_amd import ops
    x, raw, ref = _case(B, Dt, K, layout)
    yf, lf = ops.rqs(_cuda(x), _cuda(raw), K, layout, inverse=inverse, fast=True, order="linear")
    ya, la = ops.rqs(_cuda(x), _cuda(raw), K, layout, inverse=inverse, fast=False, order="linear")
    assert yf.shape == ya.shape == (B, Dt) and lf.shape == la.shape == (B, Dt)
    if B:
        (y64, ld64), (y32, ld32) = ref[inverse, 64], ref[inverse, 32]
        for tag, y, ld in (("fast", yf, lf), ("libm", ya, la)):
            print(tag, assert_parity(_np(y), y64, y32, what=f"{tag} y"))
            print(tag, assert_parity(_np(ld), ld64, ld32, what=f"{tag} ld"))
        tail = _cuda(x).abs() > 3.0
        assert torch.equal(yf[tail], ya[tail]) and torch.equal(lf[tail], la[tail])


def test_rls_ld_modes_and_strides():
    from naz_amd import ops
    B, Dt, K, layout = CASES[0]
    xc, rc, _ = _case(B, Dt, K, layout)
    x, raw = _cuda(xc), _cuda(rc)
    P = raw.shape[1]
    kw = dict(inverse=True, order="linear")
    y_ref, per = ops.rqs(x, raw, K, ld_mode=ops.LD_PERDIM, **kw)
    _, rs = ops.rqs(x, raw, K, ld_mode=ops.LD_ROWSUM, **kw)
    acc = torch.full((B,), 2.0, device=DEV)
    ops.rqs(x, raw, K, ld_mode=ops.LD_ROWSUM_ADD, ld_out=acc, **kw)
    sub = torch.full((B,), 2.0, device=DEV)
    ops.rqs(x, raw, K, ld_mode=ops.LD_ROWSUM_SUB, ld_out=sub, **kw)
    s = per.sum(-1)
    torch.testing.assert_close(rs, s, rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(acc, s + 2.0, rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(sub, 2.0 - s, rtol=1e-6, atol=1e-5)
    # strided views: x as a column slice of a wider tensor, output into a slice
    wide = torch.zeros(B, Dt + 3, device=DEV)
    wide[:, 1:1 + Dt] = x
    out = torch.zeros(B, Dt + 5, device=DEV)
    ops.rqs(wide[:, 1:1 + Dt], raw, K, out=out[:, 2:2 + Dt], **kw)
    assert torch.equal(out[:, 2:2 + Dt], y_ref)
    # a padded raw (row stride > row length) equals the packed one
    padded = torch.full((B, P + 3), 7.0, device=DEV)
    padded[:, :P] = raw
    for fast in (False, True):
        y0, l0 = ops.rqs(x, raw, K, fast=fast, **kw)
        y1, l1 = ops.rqs(x, padded[:, :P], K, fast=fast, **kw)
        assert torch.equal(y0, y1) and torch.equal(l0, l1)
        # one broadcast row (row stride 0) equals that row repeated B times
        y2, l2 = ops.rqs(x, raw[5], K, broadcast_raw=True, fast=fast, **kw)
        y3, l3 = ops.rqs(x, raw[5:6].expand(B, P).contiguous(), K, fast=fast, **kw)
        assert torch.equal(y2, y3) and torch.equal(l2, l3)


# ------------------------------------------------------------------ VJP
def _ref_grads(x, raw, Dt, K, layout, inverse, a, b, dtype, broadcast):
    xo = x.to(dtype).requires_grad_(True)
    ro = raw.to(dtype).requires_grad_(True)
    y, ld = R.rls_from_raw(xo, ro.expand(x.shape[0], -1) if broadcast else ro, Dt, K, layout, inverse)
    loss = (y * a.to(dtype)).sum() + (ld.sum(-1) * b.to(dtype)).sum()
    return torch.autograd.grad(loss, [xo, ro])


@pytest.mark.parametrize("B,Dt,K,layout,broadcast", [(257, 5, 5, ARN, False), (64, 8, 8, DENSE, False),
                                                     (257, 3, 8, DENSE, True)])
@pytest.mark.parametrize("inverse", [False, True])
def test_rls_vjp_vs_fp64_autograd(B, Dt, K, layout, broadcast, inverse):
    from naz_amd import autograd as ag
    g = torch.Generator().manual_seed(77 + B + Dt)
    raw = torch.randn(Dt * (4 * K - 1), generator=g) if broadcast else torch.randn(B, Dt * (4 * K - 1), generator=g)
    x = 2 * torch.randn(B, Dt, generator=g)
    a, b = torch.randn(B, Dt, generator=g), torch.randn(B, generator=g)
    xd, rd = _cuda(x).requires_grad_(True), _cuda(raw).requires_grad_(True)
    y, ld = ag.rqs(xd, rd, K, layout, inverse, 3.0, broadcast=broadcast, order="linear")
    ((y * _cuda(a)).sum() + (ld * _cuda(b)).sum()).backward()
    g64 = _ref_grads(x, raw, Dt, K, layout, inverse, a, b, torch.float64, broadcast)
    g32 = _ref_grads(x, raw, Dt, K, layout, inverse, a, b, torch.float32, broadcast)
    for name, v, r64, r32 in zip(("d/dx", "d/draw"), (xd.grad, rd.grad), g64, g32):
        r64 = r64.numpy()
        print(name, assert_parity(_np(v), r64, r32.numpy(), what=name, floor=grad_floor(r64), count_factor=None))


@pytest.mark.parametrize("inverse", [False, True])
def test_rls_vjp_tails_are_selected(inverse):
    """Tail inputs next to inside ones in one 16-row group: g_x = g_out and no parameter gradient
    there, everything finite, and the inside rows untouched bit for bit."""
    from naz_amd import autograd as ag
    B, Dt, K = 16, 8, 8
    g = torch.Generator().manual_seed(5)
    raw = torch.randn(B, Dt * (4 * K - 1), generator=g)
    x = torch.randn(B, Dt, generator=g).clamp(-2.9, 2.9)
    inf = float("inf")
    specials = [3.0, -3.0, 3.0 + 1e-6, -(3.0 + 1e-6), 1e30, -1e30, inf, -inf]
    for j, v in enumerate(specials):  # rows 1, 3, ..., 15 carry one special value each, in dim j
        x[2 * j + 1, j] = v
    x[9, :] = torch.tensor(specials)  # and one row is special in every dim
    a, b = torch.randn(B, Dt, generator=g), torch.randn(B, generator=g)

    def grads(rows):
        xd, rd = _cuda(x[rows]).requires_grad_(True), _cuda(raw[rows]).requires_grad_(True)
        y, ld = ag.rqs(xd, rd, K, DENSE, inverse, 3.0, order="linear")
        return torch.autograd.grad([y, ld], [xd, rd], [_cuda(a[rows]), _cuda(b[rows])])

    gx, gr = grads(torch.arange(B))
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gr).all())
    tail = _cuda(x).abs() > 3.0
    assert int(tail.sum()) == 5 + 6  # five single elements and six of row 9; ±3 exactly are inside the box
    assert torch.equal(gx[tail], _cuda(a)[tail])
    for blk in R.split_raw_params4(gr, Dt, K, DENSE):
        assert bool((blk[tail] == 0).all())
    inside_rows = torch.arange(0, B, 2)
    gx_in, gr_in = grads(inside_rows)
    assert torch.equal(gx[inside_rows.to(DEV)], gx_in) and torch.equal(gr[inside_rows.to(DEV)], gr_in)


# ------------------------------------------------------------------ flows
SPECS = {
    "nsa": dict(flow_type="nsa", D=4, C=2, hidden=[16, 16], L=2, K=5),
    "nsc": dict(flow_type="nsc", D=6, C=3, hidden=[16, 16], L=2, K=8, split=2),
    "nsc_uncond": dict(flow_type="nsc", D=6, C=0, hidden=[16, 16], L=2, K=8, split=2),
}
B_FLOW = 257


@functools.lru_cache(maxsize=None)
def _flow_inputs(name):
    spec = SPECS[name]
    state = R.random_state(spec, seed=21)
    g = torch.Generator().manual_seed(22)
    x = 1.5 * torch.randn(B_FLOW, spec["D"], generator=g)
    z = torch.randn(B_FLOW, spec["D"], generator=g)
    ctx = torch.randn(B_FLOW, spec["C"], generator=g) if spec["C"] else None
    return spec, state, x, z, ctx


def _product_flow(spec, state, bounds=None):
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import io as fio
    args = [spec["D"], spec["C"], spec["hidden"], spec["L"], spec["K"]] + ([spec["split"]] if "split" in spec else [])
    f = NormalizingFlow(spec["flow_type"], bounds, *args, order="linear")
    fio.load_state(f, {k: v.numpy() for k, v in state.items()})
    assert not f.fused
    return f


def _dt(t, dtype):
    return None if t is None else t.to(dtype)


@pytest.mark.parametrize("name", list(SPECS))
def test_linear_flow_log_prob_and_sample_transform(name):
    spec, state, x, z, ctx = _flow_inputs(name)
    f = _product_flow(spec, state)
    o64, o32 = R.build_flow(spec, state, torch.float64), R.build_flow(spec, state, torch.float32)
    c = None if ctx is None else _cuda(ctx)
    with torch.no_grad():
        lp = f.log_prob(_cuda(x), condition=c)
        ld = torch.zeros(B_FLOW, device=DEV)
        y = _cuda(z)
        for t in f._pdf(c).transforms:
            y = t._call_acc(y, ld)
    print(assert_parity(_np(lp), o64.log_prob(x.double(), _dt(ctx, torch.float64)).numpy(),
                        o32.log_prob(x, ctx).numpy(), what=f"{name} log_prob"))
    y64, ld64 = o64.forward_with_logdet(z.double(), _dt(ctx, torch.float64))
    y32, ld32 = o32.forward_with_logdet(z, ctx)
    print(assert_parity(_np(y), y64.numpy(), y32.numpy(), what=f"{name} sample y"))
    print(assert_parity(_np(ld), ld64.numpy(), ld32.numpy(), what=f"{name} sample ld"))


@pytest.mark.parametrize("name", list(SPECS))
def test_linear_flow_log_prob_with_bounds(name):
    spec, state, _, _, ctx = _flow_inputs(name)
    D = spec["D"]
    low = torch.tensor([-4.0, -3, -2, -5, -1, -6][:D])
    high = torch.tensor([4.0, 3, 5, 5, 2, 6][:D])
    x = low + (high - low) * (0.02 + 0.96 * torch.rand(B_FLOW, D, generator=torch.Generator().manual_seed(8)))
    bounds = {"low": low, "high": high}
    f = _product_flow(spec, state, bounds)
    with torch.no_grad():
        lp = f.log_prob(_cuda(x), condition=None if ctx is None else _cuda(ctx))
    o64 = R.build_flow(dict(spec, bounds=bounds), state, torch.float64)
    o32 = R.build_flow(dict(spec, bounds=bounds), state, torch.float32)
    print(assert_parity(_np(lp), o64.log_prob(x.double(), _dt(ctx, torch.float64)).numpy(),
                        o32.log_prob(x, ctx).numpy(), what=f"{name} bounded log_prob"))


def _ref_nll_grads(spec, state, x, ctx, dtype):
    st = {k: (v if v.dtype == torch.int64 else v.to(dtype).requires_grad_(True)) for k, v in state.items()}
    lp = R.build_flow(spec, st, dtype).log_prob(x.to(dtype), _dt(ctx, dtype))
    keys = [k for k in st if st[k].requires_grad]
    return lp.detach(), dict(zip(keys, torch.autograd.grad(-lp.mean(), [st[k] for k in keys])))


@pytest.mark.parametrize("name", ["nsa", "nsc"])
def test_linear_flow_nll_gradient(name):
    from naz_amd.flows import io as fio
    spec, state, x, _, ctx = _flow_inputs(name)
    f = _product_flow(spec, state)
    lp = f.log_prob(_cuda(x), condition=_cuda(ctx))
    assert lp.requires_grad
    (-lp.mean()).backward()
    lp64, g64 = _ref_nll_grads(spec, state, x, ctx, torch.float64)
    lp32, g32 = _ref_nll_grads(spec, state, x, ctx, torch.float32)
    assert_parity(_np(lp), lp64.numpy(), lp32.numpy(), what=f"{name} graph-walk log_prob")
    params = fio.named_state_params(f)
    assert set(params) == set(g64), "canonical parameter sets differ"
    if name == "nsc":
        assert "layers.0.lower_spline.unnormalized_lambdas" in params
    missed = []
    for k, p in params.items():
        assert p.grad is not None, f"{k}: no gradient"
        r64 = g64[k].numpy()
        try:
            assert_parity(_np(p.grad), r64, g32[k].numpy(), what=f"{name} d/d{k}", floor=grad_floor(r64),
                          count_factor=None)
        except AssertionError as e:  # judge every parameter before failing
            missed.append(str(e))
    assert not missed, "\n".join(missed)


def test_linear_flow_trains_on_two_moons():
    from naz_amd.flows import NormalizingFlow
    from naz_amd.trainers.train_flows import DataParallel, nll_step
    torch.manual_seed(0)
    f = NormalizingFlow("nsa", None, 2, 0, [16, 16], 2, 5, order="linear")
    x = _cuda(O.two_moons(2048))
    params = list(f.parameters())
    opt = torch.optim.Adam(params, lr=1e-2)
    dp = DataParallel()
    losses = [float(nll_step(f, x, None, opt, params, dp, x.shape[0])) for _ in range(20)]
    print(losses)
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
