"""GPU: the nsa NLL step on the fused spline backward (flows/maf_grad.py, NsaGrad: the saved-state inverse
kernel, made_ar_spline_bwd_kernel per layer, batched dW) at naz's own nsa shape D=4 | C=2,
H=[128,128], K=8 — against the oracle's float64 / float32 autograd (tests/parity.py) and the
autograd walk (NAZ_TRAIN_FUSED=0), identity tails, row independence, bounds, Adam steps, a captured
step, and the walk itself unchanged."""
import math

import numpy as np
import pytest
import torch

from oracle import naz_oracle as O
from tests.parity import assert_parity, grad_floor

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, C, HID, K = 4, 2, [128, 128], 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from naz_amd import _lib
    _lib.lib()


def _np(t):
    return t.detach().double().cpu().numpy()


def _spec(L, bounds=None):
    s = dict(flow_type="nsa", D=D, C=C, hidden=list(HID), L=L, K=K)
    if bounds is not None:
        s["bounds"] = bounds
    return s


def _flow(L, state, bounds=None):
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import io as fio
    b = None if bounds is None else {k: torch.as_tensor(v, device=DEV) for k, v in bounds.items()}
    f = NormalizingFlow("nsa", b, D, C, list(HID), L, K)
    fio.load_state(f, state)
    return f.to(DEV)


def _fused_and_walk(monkeypatch, L, state, x, c, bounds=None):
    """{"1": fused, "0": walk} -> (log_prob, {state key: gradient of -log_prob.mean()})."""
    from naz_amd.flows import flow as flow_mod
    from naz_amd.flows import io as fio
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setattr(flow_mod, "_TRAIN_FUSED", fused)
        f = _flow(L, state, bounds)
        assert f.fused and f._plan.train_ready(x, c) == (fused == "1")
        lp = f.log_prob(x, condition=c)
        (-lp.mean()).backward()
        res[fused] = (lp.detach(), {k: p.grad.detach().clone() for k, p in fio.named_state_params(f).items()})
    return res


def _oracle(spec, state, xh, cb):
    """float64 and float32 oracle autograd of -log_prob.mean(): {key: grad, "lp": log_prob}."""
    st = {k: torch.as_tensor(np.asarray(v)) for k, v in state.items()}
    g64, g32 = {}, {}
    for dt, out in ((torch.float64, g64), (torch.float32, g32)):
        sd = {k: (v if v.dtype == torch.int64 else v.to(dt).requires_grad_(True)) for k, v in st.items()}
        of = O.build_flow(spec, sd, dt)
        lpo = of.log_prob(torch.as_tensor(xh).to(dt), torch.as_tensor(np.ascontiguousarray(cb)).to(dt))
        keys = [k for k in sd if sd[k].requires_grad]
        out.update(zip(keys, torch.autograd.grad(-lpo.mean(), [sd[k] for k in keys])))
        out["lp"] = lpo.detach()
    return g64, g32


@pytest.mark.parametrize("ctx_rows,B", [(True, 777), (False, 130), (True, 2311)])
def test_fused_nsa_train_path_vs_oracle_and_walk(monkeypatch, ctx_rows, B):
    """Parity of the fused nsa NLL step at L=3: ragged batches against the 16-row wave and the
    128-row tile (777, 2311), one full tile plus two rows with ONE context vector (130).  The
    mixture data puts most rows' dims on both sides of the +-3 box inside every 16-row tile."""
    L = 3
    spec = _spec(L)
    state = {k: v.numpy() for k, v in O.random_state(spec, seed=23).items()}
    perms = [np.asarray(v) for k, v in state.items() if k.endswith("permutation")]
    assert len(perms) == L and any((p != np.arange(D)).any() for p in perms), "identity permutations only"
    xh = O.gaussian_mixture(B, D, seed=4)
    ch = O.context_normal(B if ctx_rows else 1, C, seed=5)
    outside = (np.abs(xh) > 3.0).any(1)
    assert 0 < outside.sum() < B
    x = torch.as_tensor(xh, device=DEV)
    c = torch.as_tensor(ch if ctx_rows else ch[0], device=DEV)
    res = _fused_and_walk(monkeypatch, L, state, x, c)
    cb = np.broadcast_to(ch, (B, C)) if not ctx_rows else ch
    g64, g32 = _oracle(spec, state, xh, cb)
    what = f"fused nsa B={B}"
    assert_parity(_np(res["1"][0]), _np(g64["lp"]), _np(g32["lp"]), what=f"{what} train log_prob")
    for k, g in res["0"][1].items():
        a = res["1"][1][k]
        ref = _np(g64[k])
        assert_parity(_np(a), ref, _np(g32[k]), what=f"{what} d/d{k}", floor=grad_floor(ref), count_factor=None)
        rel = float((a - g).norm() / g.norm().clamp_min(1e-30))
        assert rel < 5e-3, f"{k}: {what} vs walk {rel:.2e}"


def test_fused_nsa_tail_rows_are_the_identity(monkeypatch):
    """Every dim of every row outside the box: each layer is the identity, log p is the base density
    of x, and every parameter gradient is exactly zero (selected, never 0 x inf)."""
    from naz_amd.flows import flow as flow_mod
    from naz_amd.flows import io as fio
    L, B = 3, 203
    state = {k: v.numpy() for k, v in O.random_state(_spec(L), seed=23).items()}
    gen = torch.Generator().manual_seed(11)
    sign = torch.where(torch.rand(B, D, generator=gen) < 0.5, -1.0, 1.0)
    x = (sign * (3.5 + torch.rand(B, D, generator=gen))).to(DEV)
    c = torch.randn(B, C, generator=gen).to(DEV)
    monkeypatch.setattr(flow_mod, "_TRAIN_FUSED", "1")
    f = _flow(L, state)
    assert f.fused and f._plan.train_ready(x, c)
    lp = f.log_prob(x, condition=c)
    (-lp.mean()).backward()
    base = (-0.5 * x.double() ** 2 - 0.5 * math.log(2 * math.pi)).sum(1)
    assert torch.allclose(lp.double(), base, rtol=1e-6, atol=1e-6), float((lp.double() - base).abs().max())
    for k, p in fio.named_state_params(f).items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert float(p.grad.abs().max()) == 0.0, f"{k}: {float(p.grad.abs().max()):.3e}"


def test_fused_nsa_backward_rows_are_independent(monkeypatch):
    """NsaGrad.backward: dL/dx of rows inside the box is bitwise the same whether they are launched
    alone or interleaved with all-tail rows inside the 16-row tiles (first inside row at an odd
    index, total not a multiple of 16).  A spline maps the box to itself, so the inside rows stay
    inside through every layer."""
    from naz_amd.flows import flow as flow_mod
    L, n_in = 3, 150
    state = {k: v.numpy() for k, v in O.random_state(_spec(L), seed=23).items()}
    monkeypatch.setattr(flow_mod, "_TRAIN_FUSED", "1")
    f = _flow(L, state)
    plan = f._plan
    mg = plan.maf_grad()
    assert type(mg).__name__ == "NsaGrad"
    flat = torch.cat([p.detach().reshape(-1) for p in plan.train_params()])
    imgs = mg.images(flat)
    gen = torch.Generator().manual_seed(5)
    x_in = (0.8 * torch.randn(n_in, D, generator=gen)).clamp(-2.9, 2.9)
    c_in = torch.randn(n_in, C, generator=gen)
    total = 2 * n_in + 3
    assert total % 16 != 0
    pos = 1 + 2 * torch.arange(n_in)
    sign = torch.where(torch.rand(total, D, generator=gen) < 0.5, -1.0, 1.0)
    x_all = sign * (3.5 + torch.rand(total, D, generator=gen))
    c_all = torch.randn(total, C, generator=gen)
    x_all[pos], c_all[pos] = x_in, c_in
    out = {}
    for name, (xx, cc) in (("alone", (x_in, c_in)), ("mixed", (x_all, c_all))):
        xx, cc = xx.to(DEV).contiguous(), cc.to(DEV).contiguous()
        lp, states = mg.forward(imgs, xx, cc)
        lp, states = lp.clone(), states.clone()
        grad, g_x = mg.backward(imgs, states, cc, None)
        out[name] = (lp, g_x.clone(), grad.clone())
    pd = pos.to(DEV)
    assert bool(torch.isfinite(out["mixed"][1]).all()) and bool(torch.isfinite(out["mixed"][2]).all())
    assert torch.equal(out["alone"][0], out["mixed"][0][pd])
    assert torch.equal(out["alone"][1], out["mixed"][1][pd])
    # the tail rows pass their base-density gradient through every layer: dL/dx = -x
    tails = torch.ones(total, dtype=torch.bool)
    tails[pos] = False
    assert torch.equal(out["mixed"][1][tails.to(DEV)], -x_all[tails].to(DEV))
    # and add nothing to the parameter gradients beyond the reductions' summation order
    rel = float((out["alone"][2] - out["mixed"][2]).norm() / out["alone"][2].norm())
    assert rel < 1e-5, rel


def test_fused_nsa_train_with_bounds(monkeypatch):
    """bounds go through train_log_prob's bounding_fwd prologue: log_prob against the oracle with the
    same bounds, gradients against the walk."""
    L, B = 3, 300
    low, high = np.full(D, -5.0, np.float32), np.array([5.0, 4.0, 6.0, 5.0], np.float32)
    bounds = {"low": low, "high": high}
    spec = _spec(L)
    state = {k: v.numpy() for k, v in O.random_state(spec, seed=23).items()}
    rng = np.random.default_rng(9)
    xh = (low + (high - low) * rng.uniform(0.01, 0.99, size=(B, D))).astype(np.float32)
    ch = O.context_normal(B, C, seed=5)
    x, c = torch.as_tensor(xh, device=DEV), torch.as_tensor(ch, device=DEV)
    res = _fused_and_walk(monkeypatch, L, state, x, c, bounds)
    g64, g32 = _oracle(_spec(L, bounds), state, xh, ch)
    assert_parity(_np(res["1"][0]), _np(g64["lp"]), _np(g32["lp"]), what="fused nsa bounds log_prob")
    for k, g in res["0"][1].items():
        a = res["1"][1][k]
        rel = float((a - g).norm() / g.norm().clamp_min(1e-30))
        assert rel < 5e-3, f"{k}: fused nsa with bounds vs walk {rel:.2e}"


def test_fused_nsa_adam_steps_and_graphed_step(monkeypatch):
    """20 Adam steps of trainers.nll_step on L=4, B=4096: finite losses, the last below the first;
    GraphedNllStep (replayed, or eager where the step cannot be captured) takes the same steps, at
    test_graphed_nll_step_matches_eager_steps' tolerance.  Both runs use the capturable Adam: from
    this state (last conditioner layer x3, the loss falls from 10.9 to 8.2 in three steps) the
    rounding difference between torch's capturable and plain Adam arithmetic alone grows past that
    tolerance by the fourth step, and the comparison is about capture and replay, not about the
    optimizer's two code paths."""
    from naz_amd.flows import flow as flow_mod
    from naz_amd.trainers import DataParallel, GraphedNllStep, nll_step
    from naz_amd.trainers.train_flows import _flow_parameters
    monkeypatch.setattr(flow_mod, "_TRAIN_FUSED", "1")
    L, B = 4, 4096
    state = {k: v.numpy() for k, v in O.random_state(_spec(L), seed=31).items()}
    x = torch.as_tensor(O.gaussian_mixture(B, D, seed=40), device=DEV)
    c = torch.as_tensor(O.context_normal(B, C, seed=50), device=DEV)
    runs = {}
    for graphed, steps in ((False, 20), (True, 4)):
        f = _flow(L, state)
        assert f._plan.train_ready(x, c)
        params = _flow_parameters(f)
        dp = DataParallel()
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        g = GraphedNllStep(f, opt, params, dp, B) if graphed else None
        losses = [float(g(x, c) if graphed else nll_step(f, x, c, opt, params, dp, B)) for _ in range(steps)]
        runs[graphed] = losses
        if graphed:
            assert g.replays + g.eager_steps == steps
    le, lg = runs[False], runs[True]
    assert np.isfinite(le).all() and le[-1] < le[0], le
    assert np.allclose(le[:4], lg, rtol=1e-5, atol=1e-5), (le[:4], lg)


def test_nsa_walk_unchanged_at_the_fused_shape(monkeypatch):
    """NAZ_TRAIN_FUSED=0 at the 4|2|[128,128] shape: the degree-scheduled walk still gives the D-pass
    gradients (test_nsa_scheduled_differentiable_inverse_matches_d_pass's tolerances)."""
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import flow as flow_mod
    monkeypatch.setattr(flow_mod, "_TRAIN_FUSED", "0")
    torch.manual_seed(3)
    f = NormalizingFlow("nsa", None, D, C, list(HID), 2, K).to(DEV)
    x = torch.randn(1024, D, device=DEV) * 1.5
    c = torch.randn(1024, C, device=DEV)
    assert not f._plan.train_ready(x, c)
    out = {}
    for on in (True, False):
        for net in f.nets:
            net.degree_schedule = on
        f.zero_grad()
        lp = f.log_prob(x, condition=c)
        (-lp.mean()).backward()
        out[on] = (lp.detach(), [p.grad.detach().clone() for p in f.parameters() if p.grad is not None])
    assert torch.allclose(out[True][0], out[False][0], rtol=1e-5, atol=1e-5)
    assert len(out[True][1]) == len(out[False][1]) > 0
    for a, b in zip(out[True][1], out[False][1]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5 * float(b.abs().max()) + 1e-12), (a - b).abs().max()
