"""GPU: coupling_r16_kernel with GEMM1's pure-context B fragments resident across the layer loop.

The fp16 path splits the context k-steps once before the layer loop and forms only the last
k-step (the lane's x1 dims) per layer; the exact-FP32 fallback loads its context inside stage A.
Shapes are the smallest that reach every path: config 3 (D=16 | C=32, K=8, H=[128,128], split 8,
last conditioner layer x3 as bench.py::build_flow) with L = 3 on 2 * 128 + 5 rows (two full
workgroups and a ragged one), and the C = 0 shape (no pure-context step) with L = 2 on 133 rows.
Tolerance: tests/parity.py against the fp64 oracle, ref32 from the fp32 oracle; everything that
must not depend on the context's layout or on another workgroup's path is compared bitwise.
"""
import numpy as np
import pytest
import torch

from oracle import naz_oracle as O
from tests.parity import assert_parity

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2 * 128 + 5
R16_MODES = ["auto", "f16x3r16"]  # auto resolves to the r16 kernel at these shapes (asserted)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from naz_amd import _lib
    _lib.lib()


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


def _np(t):
    return t.detach().float().cpu().numpy()


def _flow(spec, state, mfma="f16x3r16"):
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import io as fio
    f = NormalizingFlow("nsc", None, spec["D"], spec["C"], spec["hidden"], spec["L"], spec["K"], spec["split"])
    fio.load_state(f, {k: v.numpy() for k, v in state.items()})
    assert f.fused
    f._plan.set_mfma(mfma)
    f._plan.packed()
    assert f._plan.mode == "f16x3r16", f"mfma={mfma} resolved to {f._plan.mode}: not the r16 kernel"
    return f


def _launch(f, x, c):
    """One naz_coupling_log_prob launch with the tensors as given (strides reach the kernel)."""
    from naz_amd import ops
    return ops.coupling_log_prob(f._plan.desc, f._plan.packed(), x, c)


def _oracle(spec, state, x, c):
    c64 = None if c is None else c.double()
    lp64 = O.build_flow(spec, state, torch.float64).log_prob(x.double(), c64).numpy()
    lp32 = O.build_flow(spec, state, torch.float32).log_prob(x, c).numpy()
    return lp64, lp32


@pytest.fixture(scope="module")
def case():
    """The config-3 L = 3 flow, its inputs and the oracle's log_prob (computed once, read-only)."""
    spec = dict(flow_type="nsc", D=16, C=32, hidden=[128, 128], L=3, K=8, split=8)
    state = {k: v.float() for k, v in O.random_state(spec, seed=1234).items()}
    x = torch.as_tensor(O.gaussian_mixture(B, 16, seed=3))
    c = torch.as_tensor(O.context_normal(B, 32, seed=4))
    lp64, lp32 = _oracle(spec, state, x, c)
    return dict(spec=spec, state=state, x=x, c=c, lp64=lp64, lp32=lp32)


@pytest.mark.parametrize("mfma", R16_MODES)
def test_oracle_parity(case, mfma):
    f = _flow(case["spec"], case["state"], mfma)
    lp = f.log_prob(case["x"].to(DEV), condition=case["c"].to(DEV))
    st = assert_parity(_np(lp), case["lp64"], case["lp32"], what=f"config3 L=3 {mfma}")
    print("resident ctx parity", mfma, st)


def test_both_gemm1_paths_in_one_launch(case):
    """One |ctx| >= 2^15 in a row of the middle workgroup: only that workgroup runs GEMM1 in exact
    FP32 (context loaded inside stage A, per layer); the others keep the resident fp16 fragments."""
    f = _flow(case["spec"], case["state"])
    x = case["x"].to(DEV)
    base = _np(_launch(f, x, case["c"].to(DEV)))
    c = case["c"].clone()
    c[200, 7] = 4.0e4
    lp = _np(_launch(f, x, c.to(DEV)))
    lp64, lp32 = _oracle(case["spec"], case["state"], case["x"], c)
    st = assert_parity(lp, lp64, lp32, what="config3 L=3, middle workgroup on exact-FP32 GEMM1")
    print("both gemm1 paths", st)
    others = np.r_[0:128, 256:B]
    assert np.array_equal(lp[others], base[others]), "rows of the fp16-path workgroups changed"
    assert lp[200] != base[200]


def test_noncontiguous_context(case):
    f = _flow(case["spec"], case["state"])
    x = case["x"].to(DEV)
    c = case["c"].to(DEV)
    wide = torch.full((B, 32 + 9), 7.0e4, device=DEV)  # out-of-range filler: must never be read as context
    wide[:, 5:37] = c
    view = wide[:, 5:37]
    assert view.stride(0) == 41 and not view.is_contiguous()
    assert np.array_equal(_np(_launch(f, x, view)), _np(_launch(f, x, c)))


def test_broadcast_context(case):
    f = _flow(case["spec"], case["state"])
    x = case["x"].to(DEV)
    c1 = case["c"][17].to(DEV)
    one = _np(_launch(f, x, c1))
    full = _np(_launch(f, x, c1.expand(B, 32).contiguous()))
    assert np.array_equal(one, full)
    c64 = case["c"][17].expand(B, 32)
    lp64, lp32 = _oracle(case["spec"], case["state"], case["x"], c64)
    assert_parity(one, lp64, lp32, what="config3 L=3 broadcast context")


def test_layer_dependence(case):
    """L = 1 and L = 3 flows with the same first layer: a fragment wrongly kept from one layer to
    the next (anything but the pure-context steps is layer-dependent) would break the L = 3 parity."""
    spec1 = dict(case["spec"], L=1)
    state1 = {k: v for k, v in case["state"].items() if k.startswith("layers.0.")}
    x, c = case["x"], case["c"]
    lp1 = _np(_flow(spec1, state1).log_prob(x.to(DEV), condition=c.to(DEV)))
    lp3 = _np(_flow(case["spec"], case["state"]).log_prob(x.to(DEV), condition=c.to(DEV)))
    lp64_1, lp32_1 = _oracle(spec1, state1, x, c)
    assert_parity(lp1, lp64_1, lp32_1, what="config3 L=1")
    assert_parity(lp3, case["lp64"], case["lp32"], what="config3 L=3")
    assert not np.any(lp1 == lp3)


@pytest.mark.parametrize("mfma", R16_MODES)
def test_c0_shape(mfma):
    """D=8 | C=0: GEMM1 is the x1 step alone (KS1 == 1), no resident fragment, no context load."""
    spec = dict(flow_type="nsc", D=8, C=0, hidden=[128, 128], L=2, K=8, split=4)
    state = {k: v.float() for k, v in O.random_state(spec, seed=77).items()}
    x = torch.as_tensor(O.gaussian_mixture(133, 8, seed=5))
    lp = _np(_flow(spec, state, mfma).log_prob(x.to(DEV)))
    lp64, lp32 = _oracle(spec, state, x, None)
    st = assert_parity(lp, lp64, lp32, what=f"D=8 C=0 L=2 {mfma}")
    print("c0 parity", mfma, st)
