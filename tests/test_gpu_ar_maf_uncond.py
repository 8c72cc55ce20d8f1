"""GPU: the unconditional paper MAF (D=2 | C=0, H=[150]x3: naz's
examples/papers/2506.05657/train_mle_unsupervised.py) on the fused autoregressive kernels — log_prob
(made_ar_r16_kernel over a layout whose hidden sub-layers are cut into two ring stages each, and
whose pass 0 takes its output from the biases alone), sample, the device packers, the NLL step on
the fused maf backward, and the MC-dropout sampler.

References: the float64 oracle with the float32 oracle as yardstick (tests/parity.py), and this
library's per-layer path on the same weights.  The tolerances are the D=2 | C=2 tests' own."""
import numpy as np
import pytest
import torch

from oracle import naz_oracle as O
from tests.parity import assert_parity, grad_floor

pytestmark = pytest.mark.gpu

DEV = "cuda"
D, H3 = 2, [150, 150, 150]
LOW, HIGH = np.array([-2.0, 0.5], np.float32), np.array([3.0, 7.5], np.float32)


def _spec(L):
    return dict(flow_type="maf", D=D, C=0, hidden=list(H3), L=L)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


_FLOWS = {}


def _flow(L, bounds=False, p=None, cls=None, seed=11):
    """The flow (cached per configuration) with the oracle's random state loaded, and that state."""
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import io as fio
    key = (L, bounds, p, cls, seed)
    if key not in _FLOWS:
        state = {k: v.float() for k, v in O.random_state(_spec(L), seed=seed).items()}
        kw = {} if p is None else dict(dropout_p=p)
        b = {"low": LOW, "high": HIGH} if bounds else None
        f = (cls or NormalizingFlow)("maf", b, D, 0, list(H3), L, **kw)
        fio.load_state(f, {k: v.numpy() for k, v in state.items()})
        _FLOWS[key] = (f.to(DEV), state)
    f, state = _FLOWS[key]
    f.set_fused(True)
    f.train(p is not None)
    return f, state


def _box_rows(n, seed):
    """x uniform on the 1-99 % interior of the box [LOW, HIGH]."""
    u = torch.rand(n, D, generator=torch.Generator().manual_seed(seed)) * 0.98 + 0.01
    return torch.as_tensor(LOW) + u * torch.as_tensor(HIGH - LOW)


def _oracle_lp(spec, state, x, bounds):
    """(fp64, fp32) oracle log_prob; with bounds, naz's bounding_transform in the oracle's dtype first."""
    out = []
    for dt in (torch.float64, torch.float32):
        v, lj = x.to(dt), 0.0
        if bounds:
            lo, hi = torch.as_tensor(LOW).to(dt), torch.as_tensor(HIGH).to(dt)
            u = (v - lo) / (hi - lo)
            lj = -(torch.log(u) + torch.log1p(-u) + torch.log(hi - lo)).sum(-1)
            v = torch.log(u / (1 - u))
        out.append((O.build_flow(spec, state, dt).log_prob(v, None) + lj).numpy())
    return out


@pytest.mark.parametrize("L,n,bounds", [(3, 1000, False), (10, 600, False), (3, 1000, True)],
                         ids=["L3", "L10", "L3-bounds"])
def test_log_prob_vs_oracle_and_per_layer(L, n, bounds):
    f, state = _flow(L, bounds)
    assert f.fused and f._plan.inverse == 1, "the fused inverse kernel must be selected for this shape"
    x = _box_rows(n, 5) if bounds else torch.as_tensor(O.gaussian_mixture(n, D, seed=5))
    with torch.no_grad():
        lp = f.log_prob(x.to(DEV)).cpu().numpy()
        f.set_fused(False)
        lp_walk = f.log_prob(x.to(DEV)).cpu().numpy()
        f.set_fused(True)
    lp64, lp32 = _oracle_lp(_spec(L), state, x, bounds)
    st = assert_parity(lp, lp64, lp32, what=f"fused maf 2|0 L={L}")
    print(f"L={L} bounds={bounds}", st, "max |fused - walk|", float(np.abs(lp - lp_walk).max()))
    assert_parity(lp_walk, lp64, lp32, what=f"per-layer maf 2|0 L={L}")
    np.testing.assert_allclose(lp, lp_walk, rtol=2e-5, atol=2e-4)


def test_log_prob_ragged_and_empty_batches():
    """B = 1, 17, 129 (a ragged tile, one row past a 128-row one) and 0 are the leading rows of one
    batch: rows are independent, so each is bitwise the big batch's."""
    f, _ = _flow(3)
    x = torch.as_tensor(O.gaussian_mixture(777, D, seed=8)).to(DEV)
    with torch.no_grad():
        ref = f.log_prob(x)
        for B in (1, 17, 129, 0):
            lp = f.log_prob(x[:B])
            assert lp.shape == (B,) and torch.equal(lp, ref[:B]), B


def test_out_of_f16_range_routes_to_per_layer():
    f, _ = _flow(3)
    x = torch.randn(300, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    x[7, 1] = -40000.0  # |x| >= 2^15: outside the kernel's f16x3 input split
    assert not f._plan.log_prob_ready(x, None)
    with torch.no_grad():
        lp = f.log_prob(x)
        f.set_fused(False)
        ref = f.log_prob(x)
    np.testing.assert_allclose(lp.cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=0)


@pytest.mark.parametrize("L", [3, 10])
def test_sample_vs_oracle(L):
    from naz_amd import ops
    f, state = _flow(L)
    n = 1500
    z = torch.randn(n, D, generator=torch.Generator().manual_seed(5))
    plan = f._plan
    y, ld = ops.ar_flow_sample(plan.desc, plan.packed_fwd(), z.to(DEV), None, with_logdet=True)
    y64, ld64 = O.build_flow(_spec(L), state, torch.float64).forward_with_logdet(z.double(), None)
    y32, ld32 = O.build_flow(_spec(L), state, torch.float32).forward_with_logdet(z, None)
    assert_parity(y.double().cpu().numpy(), y64.numpy(), y32.numpy(), what=f"fused sample y L={L}")
    assert_parity(ld.double().cpu().numpy(), ld64.numpy(), ld32.numpy(), what=f"fused sample ld L={L}",
                  count_factor=3.0)
    with torch.no_grad():
        y_api = f._pdf(None)._transform_z(z.to(DEV))
        f.set_fused(False)
        y_walk = f._pdf(None)._transform_z(z.to(DEV))
        f.set_fused(True)
    assert torch.equal(y_api, y)
    np.testing.assert_allclose(y.cpu().numpy(), y_walk.cpu().numpy(), rtol=1e-4, atol=1e-4)
    # log_prob(sample) = base(z) - ld: the two fused directions invert each other
    with torch.no_grad():
        lpy = f.log_prob(y).cpu().numpy()
    ref64 = (ops.base_log_prob(z.to(DEV)).double().cpu() - ld64).numpy()
    ref32 = (ops.base_log_prob(z.to(DEV)).cpu() - ld32).numpy()
    assert_parity(lpy, ref64, ref32, what=f"log_prob(sample) L={L}")


def test_sample_with_bounds_lands_inside_the_box():
    f, _ = _flow(3, bounds=True)
    with torch.no_grad():
        s = f.sample([333])
        assert s.shape == (333, D) and bool(torch.isfinite(s).all())
        assert bool(((s > torch.as_tensor(LOW, device=DEV)) & (s < torch.as_tensor(HIGH, device=DEV))).all())
        torch.manual_seed(0)
        a = f.sample([1000])
        f.set_fused(False)
        torch.manual_seed(0)
        b = f.sample([1000])
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-4)


def test_device_packers_and_batched_draws():
    """The device packers give the host packers' images bit for bit (both directions; the inverse
    image's cut sub-layers included), and a batched launch over three weight draws gives every
    draw's single launch bit for bit."""
    from naz_amd import ops
    f, _ = _flow(3)
    plan = f._plan
    flat = plan._flat().astype(np.float32)
    perm = np.stack([n.permutation.detach().cpu().numpy() for n in plan._nets()]).astype(np.int32)
    flats = [flat, flat * np.float32(1.03), flat * np.float32(0.97)]
    ft = torch.tensor(np.stack(flats), device=DEV)
    dev = ops.ar_flow_pack_batched(plan.desc, ft, perm)
    fwd = ops.ar_flow_pack_fwd_batched(plan.desc, ft)
    for p, fl in enumerate(flats):
        host = ops.ar_flow_pack(plan.desc, fl, perm, DEV)
        nbad = int((dev[p].view(torch.int32) != host.view(torch.int32)).sum())
        assert nbad == 0, f"draw {p} inverse image: {nbad} words differ"
        assert torch.equal(fwd[p].view(torch.int32), ops.ar_flow_pack_fwd(plan.desc, fl, DEV).view(torch.int32))
    mask = (ft[0] != 0).float()
    noisy = ft + torch.rand_like(ft) * (1 - mask)
    assert torch.equal(ops.ar_flow_pack_batched(plan.desc, noisy, perm, mask=mask).view(torch.int32),
                       ops.ar_flow_pack_batched(plan.desc, noisy * mask, perm).view(torch.int32))
    assert torch.equal(ops.ar_flow_pack_fwd_batched(plan.desc, noisy, mask=mask).view(torch.int32),
                       ops.ar_flow_pack_fwd_batched(plan.desc, noisy * mask).view(torch.int32))
    x = torch.as_tensor(O.gaussian_mixture(777, D, seed=9)).to(DEV)
    xs = torch.stack([x, 0.9 * x, 1.1 * x])
    shared = ops.ar_flow_log_prob_batched(plan.desc, dev, x, None)
    per = ops.ar_flow_log_prob_batched(plan.desc, dev, xs, None)
    z = torch.randn(3, 500, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    ys, lds = ops.ar_flow_sample_batched(plan.desc, fwd, z, None, with_logdet=True)
    for p in range(3):
        assert torch.equal(shared[p], ops.ar_flow_log_prob(plan.desc, dev[p], x, None))
        assert torch.equal(per[p], ops.ar_flow_log_prob(plan.desc, dev[p], xs[p], None))
        y1, ld1 = ops.ar_flow_sample(plan.desc, fwd[p], z[p], None, with_logdet=True)
        assert torch.equal(ys[p], y1) and torch.equal(lds[p], ld1)


def _np(t):
    return t.detach().double().cpu().numpy()


@pytest.mark.parametrize("B,bounds", [(777, False), (130, False), (777, True)], ids=["B777", "B130", "B777-bounds"])
def test_fused_train_path_vs_oracle_and_walk(monkeypatch, B, bounds):
    """The NLL step on the fused maf backward (flows/maf_grad.py) with no context: gradients against
    the oracle's float64 autograd (tests/parity.py gradient criterion) and against the per-node walk."""
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import flow as flow_mod
    from naz_amd.flows import io as fio
    L = 3
    spec = _spec(L)
    state = {k: v.numpy() for k, v in O.random_state(spec, seed=23).items()}
    xh = _box_rows(B, 4) if bounds else torch.as_tensor(O.gaussian_mixture(B, D, seed=4))
    x = xh.to(DEV)
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setattr(flow_mod, "_TRAIN_FUSED", fused)
        f = NormalizingFlow("maf", {"low": LOW, "high": HIGH} if bounds else None, D, 0, list(H3), L)
        fio.load_state(f, state)
        assert f.fused and f._plan._train_kernels() and f._plan.train_ready(x, None) == (fused == "1")
        lp = f.log_prob(x)
        (-lp.mean()).backward()
        res[fused] = (lp.detach(), {k: p.grad.detach().clone() for k, p in fio.named_state_params(f).items()})
    st = {k: torch.as_tensor(np.asarray(v)) for k, v in state.items()}
    g64, g32 = {}, {}
    for dt, out in ((torch.float64, g64), (torch.float32, g32)):
        sd = {k: (v if v.dtype == torch.int64 else v.to(dt).requires_grad_(True)) for k, v in st.items()}
        v, lj = xh.to(dt), 0.0
        if bounds:
            lo, hi = torch.as_tensor(LOW).to(dt), torch.as_tensor(HIGH).to(dt)
            u = (v - lo) / (hi - lo)
            lj = -(torch.log(u) + torch.log1p(-u) + torch.log(hi - lo)).sum(-1)
            v = torch.log(u / (1 - u))
        lpo = O.build_flow(spec, sd, dt).log_prob(v, None) + lj
        keys = [k for k in sd if sd[k].requires_grad]
        out.update(zip(keys, torch.autograd.grad(-lpo.mean(), [sd[k] for k in keys])))
        out["lp"] = lpo.detach()
    assert_parity(_np(res["1"][0]), _np(g64["lp"]), _np(g32["lp"]), what="maf 2|0 train log_prob")
    for k, g in res["0"][1].items():
        a = res["1"][1][k]
        ref = _np(g64[k])
        if not np.any(ref):  # (a parameter no output depends on: both gradients are exact zeros)
            assert not bool(a.any()) and not bool(g.any()), k
            continue
        assert_parity(_np(a), ref, _np(g32[k]), what=f"maf 2|0 d/d{k}", floor=grad_floor(ref), count_factor=None)
        rel = float((a - g).norm() / g.norm().clamp_min(1e-30))
        assert rel < 5e-3, f"{k}: fused vs walk {rel:.2e}"


def test_adam_steps_decrease_the_loss_and_the_graphed_step_matches():
    """10 capturable-Adam steps at B = 2048 on the fused step: every loss finite, the last below the
    first; GraphedNllStep (1 eager step + 3 replays) reproduces the first 4."""
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import io as fio
    from naz_amd.trainers import DataParallel, GraphedNllStep, nll_step
    from naz_amd.trainers.train_flows import _flow_parameters
    L, B = 3, 2048
    state = {k: v.numpy() for k, v in O.random_state(_spec(L), seed=31).items()}
    x = torch.as_tensor(O.gaussian_mixture(B, D, seed=40), device=DEV)
    runs = {}
    for graphed in (False, True):
        f = NormalizingFlow("maf", None, D, 0, list(H3), L)
        fio.load_state(f, state)
        f = f.to(DEV)
        assert f._plan.train_ready(x, None)
        params = _flow_parameters(f)
        dp = DataParallel()
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        g = GraphedNllStep(f, opt, params, dp, B) if graphed else None
        steps = 4 if graphed else 10
        runs[graphed] = [float(g(x, None) if graphed else nll_step(f, x, None, opt, params, dp, B))
                         for _ in range(steps)]
        if graphed:
            assert not g.eager_only, g.capture_error
            assert g.replays == 3 and g.eager_steps == 1
    le, lg = runs[False], runs[True]
    assert np.isfinite(le).all() and le[-1] < le[0], le
    assert np.allclose(le[:4], lg, rtol=1e-5, atol=1e-5), (le[:4], lg)


def test_dropout_sampler_fused_vs_per_layer_and_p0(monkeypatch):
    from naz_amd import ops
    p, B = 0.25, 421
    f, _ = _flow(3, p=p)
    assert f._plan.dropout_sample_usable()
    torch.manual_seed(3)
    a = f.sample([B])
    torch.manual_seed(3)
    assert torch.equal(a, f.sample([B])) and bool(torch.isfinite(a).all())
    monkeypatch.setenv("NAZ_AR_DROPOUT_FUSED", "0")
    assert not f._plan.dropout_sample_usable()
    torch.manual_seed(3)
    w = f.sample([B])
    monkeypatch.delenv("NAZ_AR_DROPOUT_FUSED")
    torch.testing.assert_close(a, w, rtol=1e-3, atol=1e-3)  # test_gpu_ar_dropout.py's tolerance
    # p = 0: every unit kept at scale 1, bitwise the plain fused sampler
    plan = f._plan
    z = torch.randn(B, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    seeds = torch.randint(0, 2 ** 62, (3, 3), generator=torch.Generator().manual_seed(17), dtype=torch.int64)
    y, ld = ops.ar_flow_sample_dropout(plan.desc, plan.packed_fwd(), z, None, None, None, 0.0, seeds.to(DEV),
                                       with_logdet=True)
    y0, ld0 = ops.ar_flow_sample(plan.desc, plan.packed_fwd(), z, None, with_logdet=True)
    assert torch.equal(y, y0) and torch.equal(ld, ld0)
    yp, _ = ops.ar_flow_sample_dropout(plan.desc, plan.packed_fwd(), z, None, None, None, p, seeds.to(DEV),
                                       with_logdet=True)
    assert bool(torch.isfinite(yp).all()) and not torch.equal(yp, y0)


def test_sample_uncertain():
    from naz_amd.flows.mcdpflow import MCDPNormalizingFlow
    f, _ = _flow(3, bounds=True, p=0.25, cls=MCDPNormalizingFlow)
    assert f._plan.dropout_sample_usable()
    torch.manual_seed(5)
    s = np.asarray(f.sample_uncertain(3, [500]))
    assert s.shape == (3, 500, D) and np.isfinite(s).all()
    assert all(not np.array_equal(s[i], s[j]) for i in range(3) for j in range(i))
    assert ((s > LOW) & (s < HIGH)).all()
