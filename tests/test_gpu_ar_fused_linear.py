"""GPU: the fused autoregressive kernels on order="linear" nsa flows (kind NAZ_AR_SPLINE_LINEAR,
csrc/made_ar_r16.h: rls_select_inv_quad in made_ar_r16_kernel, rls_select_fwd in
made_ar_fwd_kernel) at the two compiled shapes, D=4 | C=2 and D=8 | C=0 with H=[128,128], K=8.

log_prob and sample against the float64 restatement of pyro's linear-order spline flow
(tests/spline_linear_ref.py) under tests/parity.py's criterion with the float32 restatement as
yardstick, against the per-kernel chain on the same weights, and on the kernel's own edges: the
bounding map, one broadcast context vector, a ragged last tile, an empty batch, rows outside the
f16 split's range, all-tail batches, row position, the packed images' layout tags and the device
packer.  Under autograd the flow keeps the per-kernel walk.

The float32 restatement alone, on the log_prob inputs below (CPU): D=4 | C=2 median 2.4e-7, q99
1.7e-6, max 2.9e-6, 0 of 1200 rows above 1e-5; D=8 | C=0 1.1e-7 / 6.2e-7 / 3.9e-6, 0 of 1500.
13-14 % of the elements sit in the identity tails."""
import functools

import numpy as np
import pytest
import torch

from oracle import naz_oracle as O
from tests import spline_linear_ref as R
from tests.parity import assert_parity

pytestmark = pytest.mark.gpu

DEV = "cuda"

SPECS = {
    "D4C2": dict(flow_type="nsa", D=4, C=2, hidden=[128, 128], L=3, K=8, n=1200),  # naz's own nsa shape
    "D8C0": dict(flow_type="nsa", D=8, C=0, hidden=[128, 128], L=2, K=8, n=1500),  # no context, two dim groups
}
EDGE = dict(flow_type="nsa", D=4, C=2, hidden=[128, 128], L=2, K=8)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@functools.lru_cache(maxsize=None)
def _state(D, C, L):
    spec = dict(flow_type="nsa", D=D, C=C, hidden=[128, 128], L=L, K=8)
    return {k: v.float() for k, v in R.random_state(spec, seed=11).items()}


def _flow(spec, bounds=None, order="linear"):
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import io as fio
    f = NormalizingFlow("nsa", bounds, spec["D"], spec["C"], spec["hidden"], spec["L"], spec["K"], order=order)
    state = _state(spec["D"], spec["C"], spec["L"])
    if order == "linear":
        fio.load_state(f, {k: v.numpy() for k, v in state.items()})
    return f.to(DEV), state


def _np(t):
    return t.detach().double().cpu().numpy()


def _both(f, fn):
    """fn() on the fused launch and on the per-kernel chain."""
    with torch.no_grad():
        a = fn()
        f.set_fused(False)
        b = fn()
        f.set_fused(True)
    return a, b


@functools.lru_cache(maxsize=None)
def _log_prob_refs(name):
    spec = SPECS[name]
    n, D, C = spec["n"], spec["D"], spec["C"]
    state = _state(D, C, spec["L"])
    x = torch.as_tensor(O.gaussian_mixture(n, D, seed=5))
    c = torch.as_tensor(O.context_normal(n, C, seed=6)) if C else None
    lp64 = R.build_flow(spec, state, torch.float64).log_prob(x.double(), None if c is None else c.double()).numpy()
    lp32 = R.build_flow(spec, state, torch.float32).log_prob(x, c).numpy()
    return x, c, lp64, lp32


@pytest.mark.parametrize("name", list(SPECS))
def test_fused_linear_log_prob_vs_reference_and_chain(name):
    f, _ = _flow(SPECS[name])
    assert f.fused, "the fused autoregressive kernel must be selected for a linear-order nsa flow of this shape"
    x, c, lp64, lp32 = _log_prob_refs(name)
    cd = None if c is None else c.to(DEV)
    lp, lp_chain = _both(f, lambda: f.log_prob(x.to(DEV), condition=cd))
    lp, lp_chain = _np(lp), _np(lp_chain)
    print(name, "max |fused - chain|", float(np.abs(lp - lp_chain).max()))
    print(name, "fused", assert_parity(lp, lp64, lp32, what=f"fused linear {name}"))
    print(name, "chain", assert_parity(lp_chain, lp64, lp32, what=f"per-kernel linear {name}"))


@pytest.mark.parametrize("name", list(SPECS))
def test_fused_linear_sample_vs_reference_and_chain(name):
    """One naz_ar_flow_sample launch: y and the summed forward log-det (count_factor 3.0: the
    quadratic sampler's allowance, tests/test_gpu_ar_fused.py); the API takes the same launch.

    Measured on an MI355X (1500 rows; log-det's relative error against float64, floor 1; rows above
    1e-5: fused / float32 reference / allowance): D4C2 52 / 56 / 170 (q99 1.5e-5), D8C0 1 / 3 / 11
    (q99 6.1e-6).  The sampler forms the searched table's knots and θ in double (rls_select_fwd):
    with the all-float evaluator D8C0 had 20 rows above 1e-5 and failed the count."""
    from naz_amd import ops
    spec = SPECS[name]
    f, state = _flow(spec)
    assert f.fused
    g = torch.Generator().manual_seed(5)
    n, D, C = 1500, spec["D"], spec["C"]
    z = torch.randn(n, D, generator=g)
    c = torch.randn(n, C, generator=g) if C else None
    cd = None if c is None else c.to(DEV)
    plan = f._plan
    y, ld = ops.ar_flow_sample(plan.desc, plan.packed_fwd(), z.to(DEV), cd, with_logdet=True)
    y64, ld64 = R.build_flow(spec, state, torch.float64).forward_with_logdet(z.double(), None if c is None else c.double())
    y32, ld32 = R.build_flow(spec, state, torch.float32).forward_with_logdet(z, c)
    print(name, "y", assert_parity(_np(y), y64.numpy(), y32.numpy(), what=f"fused linear sample y {name}"))
    print(name, "ld", assert_parity(_np(ld), ld64.numpy(), ld32.numpy(), what=f"fused linear sample ld {name}",
                                    count_factor=3.0))
    y_api, y_chain = _both(f, lambda: f._pdf(cd)._transform_z(z.to(DEV)))
    assert torch.equal(y_api, y)
    np.testing.assert_allclose(_np(y), _np(y_chain), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("n", [777, 4096])
def test_fused_linear_bounds_one_context_vector(n):
    """The bounding map with one broadcast context vector: a ragged last tile (777), and the size
    from which the quadratic flows take the pass-0-constants path (4096; the linear kind has none
    and launches with ldc = 0)."""
    lo, hi = np.full(4, -9.0, np.float32), np.full(4, 9.5, np.float32)
    f, _ = _flow(EDGE, bounds={"low": lo, "high": hi})
    assert f.fused
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(n, 4, generator=g) * 17.0 - 8.0).to(DEV)
    c1 = torch.randn(2, generator=g).to(DEV)
    lp, ref = _both(f, lambda: f.log_prob(x, condition=c1))
    assert torch.isfinite(lp).all()
    np.testing.assert_allclose(_np(lp), _np(ref), rtol=2e-5, atol=2e-4)
    with torch.no_grad():
        assert f.log_prob(x[:0], condition=c1).shape == (0,)


def test_fused_linear_out_of_f16_range_routes_to_the_chain():
    f, _ = _flow(EDGE)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(300, 4, generator=g).to(DEV)
    x[7, 3] = 1e6  # outside the kernel's f16x3 input split: identity in every spline
    c = torch.randn(300, 2, generator=g).to(DEV)
    lp, ref = _both(f, lambda: f.log_prob(x, condition=c))
    assert torch.equal(lp, ref)


def test_fused_linear_sample_bounds_one_context_vector():
    lo, hi = np.full(4, -9.0, np.float32), np.full(4, 9.5, np.float32)
    f, _ = _flow(EDGE, bounds={"low": lo, "high": hi})
    c1 = torch.randn(2, generator=torch.Generator().manual_seed(8)).to(DEV)

    def draw(n):
        torch.manual_seed(0)
        return f.sample([n], condition=c1)

    s = draw(333)
    assert s.shape == (333, 4) and torch.isfinite(s).all()
    assert bool(((s > -9.0) & (s < 9.5)).all())
    a, b = _both(f, lambda: draw(333))
    np.testing.assert_allclose(_np(a), _np(b), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", list(SPECS))
def test_fused_linear_all_tail_batch_is_the_base_density(name):
    """Every |x_d| beyond the spline box: every layer is the identity with zero log-det."""
    spec = SPECS[name]
    f, _ = _flow(spec)
    bound = float(f.transforms[0].bound)
    g = torch.Generator().manual_seed(12)
    n, D, C = 500, spec["D"], spec["C"]
    sign = torch.where(torch.rand(n, D, generator=g) < 0.5, -1.0, 1.0)
    x = sign * (bound + 0.01 + 4.0 * torch.rand(n, D, generator=g))
    c = torch.randn(n, C, generator=g).to(DEV) if C else None
    with torch.no_grad():
        lp = f.log_prob(x.to(DEV), condition=c)
    want = (-0.5 * x.double() ** 2 - 0.5 * np.log(2.0 * np.pi)).sum(1).numpy()
    np.testing.assert_allclose(_np(lp), want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", list(SPECS))
def test_fused_linear_deterministic_and_row_position_free(name):
    spec = SPECS[name]
    f, _ = _flow(spec)
    g = torch.Generator().manual_seed(13)
    n, D, C = 400, spec["D"], spec["C"]
    x = (2.0 * torch.randn(n, D, generator=g)).to(DEV)
    c = torch.randn(n, C, generator=g).to(DEV) if C else None
    pm = torch.randperm(n, generator=g).to(DEV)
    with torch.no_grad():
        a = f.log_prob(x, condition=c)
        assert torch.equal(a, f.log_prob(x, condition=c))
        assert torch.equal(a[pm], f.log_prob(x[pm], condition=None if c is None else c[pm]))
        ya = f._pdf(c)._transform_z(x)
        assert torch.equal(ya, f._pdf(c)._transform_z(x))
        assert torch.equal(ya[pm], f._pdf(None if c is None else c[pm])._transform_z(x[pm]))


def test_fused_linear_images_tags_device_pack_and_batched_draws():
    """The linear and quadratic descriptors of one shape refuse each other's images by the layout
    tag (no launch); the device packer equals the host packer bit for bit; the batched log_prob
    equals the per-draw one bit for bit (after test_fused_ar_device_pack_and_batched_draws)."""
    from naz_amd import ops
    f, _ = _flow(EDGE)
    fq, _ = _flow(EDGE, order="quadratic")
    plan, qplan = f._plan, fq._plan
    assert plan.desc.kind == ops.AR_KIND["nsa_linear"] and qplan.desc.kind == ops.AR_KIND["nsa"]
    x = torch.as_tensor(O.gaussian_mixture(777, 4, seed=9)).to(DEV)
    c = torch.as_tensor(O.context_normal(777, 2, seed=3)).to(DEV)
    for d, inv, fwd in ((qplan.desc, plan.packed(), plan.packed_fwd()), (plan.desc, qplan.packed(), qplan.packed_fwd())):
        with pytest.raises(RuntimeError, match="another descriptor or layout"):
            ops.ar_flow_log_prob(d, inv, x, c)
        with pytest.raises(RuntimeError, match="another descriptor or layout"):
            ops.ar_flow_sample(d, fwd, x, c)
    flat = plan._flat().astype(np.float32)
    perm = np.stack([n.permutation.detach().cpu().numpy() for n in plan._nets()]).astype(np.int32)
    flats = [flat, flat * np.float32(1.03), flat * np.float32(0.97)]
    ft = torch.tensor(np.stack(flats), device=DEV)
    dev = ops.ar_flow_pack_batched(plan.desc, ft, perm)
    fwd = ops.ar_flow_pack_fwd_batched(plan.desc, ft)
    for p, fl in enumerate(flats):
        host = ops.ar_flow_pack(plan.desc, fl, perm, DEV)
        nbad = int((dev[p].view(torch.int32) != host.view(torch.int32)).sum())
        assert nbad == 0, f"draw {p} image: {nbad} words differ"
        assert torch.equal(fwd[p].view(torch.int32), ops.ar_flow_pack_fwd(plan.desc, fl, DEV).view(torch.int32))
    xs = torch.stack([x, 0.9 * x, 1.1 * x])
    c1 = c[0].contiguous()
    shared = ops.ar_flow_log_prob_batched(plan.desc, dev, x, c1)
    per = ops.ar_flow_log_prob_batched(plan.desc, dev, xs, c1)
    for p in range(3):
        assert torch.equal(shared[p], ops.ar_flow_log_prob(plan.desc, dev[p], x, c1))
        assert torch.equal(per[p], ops.ar_flow_log_prob(plan.desc, dev[p], xs[p], c1))
    # no pass-0-constants form for this kind: the packer and the launch say so
    assert ops.ar_flow_pass0_floats(plan.desc) < 0
    with pytest.raises(RuntimeError, match="pass-0"):
        ops.ar_flow_log_prob_batched(plan.desc, dev, x, c1, pass0_const=True)


def test_fused_linear_training_keeps_the_walk():
    f, _ = _flow(EDGE)
    assert f.fused
    g = torch.Generator().manual_seed(14)
    x = (1.5 * torch.randn(257, 4, generator=g)).to(DEV)
    c = torch.randn(257, 2, generator=g).to(DEV)
    assert not f._plan.train_ready(x, c)
    lp = f.log_prob(x, condition=c)
    assert lp.requires_grad
    f.set_fused(False)
    ref = f.log_prob(x, condition=c)
    f.set_fused(True)
    assert torch.equal(lp.detach(), ref.detach())
    (-lp.mean()).backward()
    params = list(f.parameters())
    assert params
    for p in params:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
