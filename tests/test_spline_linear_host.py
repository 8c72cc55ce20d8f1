"""CPU: order="linear" (pyro's rational-linear spline) — the reference restatement's own
properties, and everything of the feature that is decided on the host: symbols, argument checks,
construction, parameter shapes, the fused-plan decision, state I/O."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import naz_oracle as O
from tests import spline_linear_ref as R

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("naz_rls_fwd", "naz_rls_inv", "naz_rls_bwd")


# ------------------------------------------------------------------ the restatement (fp64)
def _one_spline(K, seed):
    """Unnormalised (w, h, d, l) of one spline, [1, K] / [1, K-1], fp64, ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(1, n, generator=g, dtype=torch.float64) for n in (K, K, K - 1, K))


def _knots(u, K, bound=3.0):
    frac = O.MIN_BIN_WIDTH + (1.0 - O.MIN_BIN_WIDTH * K) * F.softmax(u, dim=-1)
    return O._calculate_knots(frac, -bound, bound)[1]  # [1, K+1]


def _apply(x, p, inverse=False):
    """x [N] through the single spline p -> (y [N], ld [N])."""
    y, ld = R.monotonic_rls(x[:, None], *R.normalize4(*p), inverse=inverse)
    return y[:, 0], ld[:, 0]


@pytest.mark.parametrize("K", [5, 8])
def test_restatement_passes_through_the_knots_with_the_knot_slopes(K):
    p = _one_spline(K, 10 + K)
    xk, yk = _knots(p[0], K)[0], _knots(p[1], K)[0]
    y, _ = _apply(xk, p)
    torch.testing.assert_close(y, yk, rtol=0, atol=1e-12)
    x = xk[1:-1].clone().requires_grad_(True)
    y, _ = _apply(x, p)
    slope, = torch.autograd.grad(y.sum(), x)
    torch.testing.assert_close(slope, O.MIN_DERIVATIVE + F.softplus(p[2][0]), rtol=1e-10, atol=0)


@pytest.mark.parametrize("K", [5, 8])
@pytest.mark.parametrize("inverse", [False, True])
def test_restatement_logdet_is_the_log_derivative(K, inverse):
    p = _one_spline(K, 20 + K)
    x = (torch.rand(400, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 6 - 3).requires_grad_(True)
    y, ld = _apply(x, p, inverse)
    dydx, = torch.autograd.grad(y.sum(), x)
    assert bool((dydx > 0).all())
    torch.testing.assert_close(torch.exp(ld.detach()), dydx, rtol=1e-9, atol=0)


@pytest.mark.parametrize("K", [5, 8])
def test_restatement_round_trip_and_tails(K):
    g = torch.Generator().manual_seed(30 + K)
    Dt, B = 3, 500
    raw = torch.randn(B, Dt * (4 * K - 1), generator=g, dtype=torch.float64)
    x = 2 * torch.randn(B, Dt, generator=g, dtype=torch.float64)
    for layout in (R.LAYOUT_DENSE, R.LAYOUT_ARN):
        y, ld = R.rls_from_raw(x, raw, Dt, K, layout, False)
        xb, ldb = R.rls_from_raw(y, raw, Dt, K, layout, True)
        torch.testing.assert_close(xb, x, rtol=0, atol=1e-9)
        torch.testing.assert_close(ldb, -ld, rtol=0, atol=1e-8)
        tail = x.abs() > 3
        assert bool(tail.any()) and torch.equal(y[tail], x[tail]) and bool((ld[tail] == 0).all())


# ------------------------------------------------------------------ the feature, host side
def test_header_declares_and_library_exports_the_entries():
    from naz_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "naz_hip.h").read_text(), flags=re.S)
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared"
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert L.naz_abi_version() == 3


def test_host_side_argument_checks():
    from naz_amd import _lib
    L = _lib.lib()
    rc = L.naz_rls_fwd(None, 0, None, 0, None, 0, None, 0, 16, 0, 8, 0, 3.0, None)  # Dt = 0
    assert rc != 0 and b"bad shape" in L.naz_last_error()
    rc = L.naz_rls_inv(None, 0, None, 0, None, 0, None, 0, 0, 4, 2000, 0, 3.0, None)  # K*1e-3 > 1
    assert rc != 0 and b"Minimal bin width" in L.naz_last_error()
    rc = L.naz_rls_fwd(None, 0, None, 0, None, 0, None, 0, 4, 2, 8, 0, 3.0, None)
    assert rc != 0 and b"null x/y" in L.naz_last_error()
    rc = L.naz_rls_bwd(0, None, 0, None, 0, None, 0, None, 3, None, 0, None, 0, 0, 2, 8, 0, 3.0, None)
    assert rc != 0 and b"g_ld_mode" in L.naz_last_error()
    assert L.naz_rls_fwd(None, 0, None, 0, None, 0, None, 0, 0, 2, 8, 0, 3.0, None) == 0  # B = 0: no launch


def _flows():
    from naz_amd.flows import NormalizingFlow
    nsa = NormalizingFlow("nsa", None, 4, 2, [16, 16], 2, 5, order="linear")
    nsc = NormalizingFlow("nsc", None, 6, 3, [16, 16], 2, 8, 2, order="linear")
    return nsa, nsc


def test_linear_flows_construct_with_the_fourth_parameter_block():
    nsa, nsc = _flows()
    for net in nsa.nets:
        assert net.layers[-1].weight.shape[0] == 4 * (4 * 5 - 1)
        assert list(net.param_dims) == [5, 5, 4, 5]
    for t, net in zip(nsc.transforms, nsc.nets):
        assert net.layers[-1].weight.shape[0] == (6 - 2) * (4 * 8 - 1)
        low = t.lower_spline
        assert low.unnormalized_lambdas.shape == (2, 8)
        lam = low.unnormalized_lambdas.detach()
        assert 0.0 <= float(lam.min()) and float(lam.max()) < 1.0  # pyro's uniform init
        assert low.flat_raw().numel() == 2 * (4 * 8 - 1)
    assert not nsa.fused and not nsc.fused


def test_quadratic_stays_the_default_and_has_no_lambdas():
    from naz_amd.flows import NormalizingFlow
    f = NormalizingFlow("nsc", None, 6, 3, [16, 16], 2, 8, 2)
    for t, net in zip(f.transforms, f.nets):
        assert net.layers[-1].weight.shape[0] == (6 - 2) * (3 * 8 - 1)
        assert not hasattr(t.lower_spline, "unnormalized_lambdas")


def test_config3_shape_is_fused_only_for_the_quadratic_order():
    from naz_amd.flows import NormalizingFlow
    assert NormalizingFlow("nsc", None, 16, 32, [128, 128], 8, 8, 8).fused
    lin = NormalizingFlow("nsc", None, 16, 32, [128, 128], 8, 8, 8, order="linear")
    assert not lin.fused
    with pytest.raises(RuntimeError, match="no fused instantiation"):
        lin.set_fused(True)
    assert not NormalizingFlow("nsa", None, 16, 32, [128, 128], 2, 8, order="linear").fused


def test_state_round_trip_is_bitwise_lambdas_included():
    from naz_amd.flows import io as fio
    for f, g in zip(_flows(), _flows()):
        state = fio.export_state(f)
        if f.flow_type == "nsc":
            assert "layers.1.lower_spline.unnormalized_lambdas" in state
            assert "layers.0.lower_spline.unnormalized_lambdas" in fio.named_state_params(f)
        fio.load_state(g, state)
        back = fio.export_state(g)
        assert set(back) == set(state)
        for k in state:
            assert np.array_equal(back[k], state[k]), k


def test_reference_state_matches_the_product_flows():
    """The helper's random_state has exactly the product flow's canonical tensors and shapes."""
    from naz_amd.flows import io as fio
    nsa, nsc = _flows()
    specs = (dict(flow_type="nsa", D=4, C=2, hidden=[16, 16], L=2, K=5),
             dict(flow_type="nsc", D=6, C=3, hidden=[16, 16], L=2, K=8, split=2))
    for f, spec in zip((nsa, nsc), specs):
        st, ex = R.random_state(spec), fio.export_state(f)
        assert set(st) == set(ex)
        assert all(tuple(st[k].shape) == ex[k].shape for k in st)


def test_unknown_order_raises_value_error():
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows.transforms import Spline
    with pytest.raises(ValueError, match="order"):
        NormalizingFlow("nsa", None, 4, 2, [16, 16], 2, 5, order="cubic")
    with pytest.raises(ValueError, match="order"):
        NormalizingFlow("nsc", None, 6, 3, [16, 16], 2, 8, 2, order="cubic")
    with pytest.raises(ValueError, match="order"):
        Spline(2, 8, order="cubic")


def test_ops_reject_cpu_tensors_and_name_the_expected_width():
    from naz_amd import ops
    x, raw = torch.zeros(4, 2), torch.zeros(4, 2 * (4 * 8 - 1))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.rqs(x, raw, 8, order="linear")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.rqs_bwd(x, raw, 8, ops.LAYOUT_DENSE, False, 3.0, x, None, order="linear")
    with pytest.raises(ValueError, match="order"):
        ops.rqs(x, raw, 8, order="cubic")
