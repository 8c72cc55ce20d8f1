"""GPU: GEMM1 of the 16-row coupling kernel after its last k-step became one concatenated MFMA
([Wh | Wh | Wl | 0] x [Xh | Xl | Xh | 0], coupling_r16.h CfgR16::CAT1) on a compacted stage-A image.

Config 3 takes the concatenated step (NR1 = 2 k-slots per quarter, one MFMA behind the context
step).  Config 2's single step is all of GEMM1 and keeps the three-MFMA form (CAT1 needs KS1 > 1),
now on the re-laid-out stage A: it is the old-path shape here.  Criterion: tests/parity.py against
the fp64 oracle with the fp32 oracle as ref32, as tests/test_gpu_parity.py.
The sample direction's input is standard normal (the base space): fed the data-space mixture, the
config-2 case has 3 elements of y above 1e-5 against a bound of 2 in every mode, exact fp32
included, before this kernel change as after it (the spline evaluator, not GEMM1).
"""
import numpy as np
import pytest
import torch

from oracle import naz_oracle as O
from tests.parity import assert_parity

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 133  # one full 128-row workgroup and one partial
SPEC3 = dict(flow_type="nsc", D=16, C=32, hidden=[128, 128], L=2, K=8, split=8)
SPEC2 = dict(flow_type="nsc", D=8, C=0, hidden=[128, 128], L=2, K=8, split=4)


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


def _flow(spec, state, mfma):
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import io as fio
    f = NormalizingFlow("nsc", None, spec["D"], spec["C"], spec["hidden"], spec["L"], spec["K"], spec["split"])
    fio.load_state(f, {k: v.numpy() for k, v in state.items()})
    assert f.fused
    f._plan.set_mfma(mfma)
    return f


def _state(spec, seed=1234):
    return {k: v.float() for k, v in O.random_state(spec, seed=seed).items()}


def _full_mantissa(t, seed):
    """t x (1 + 2^-12 x odd): every value keeps bits below its fp16 hi piece, so the hi x lo products
    of the f16x3 split carry ~2^-12 of the result."""
    g = torch.Generator().manual_seed(seed)
    odd = 2 * torch.randint(0, 8, t.shape, generator=g) + 1
    return (t.double() * (1.0 + odd.double() * 2.0 ** -12)).float()


def _inputs(spec, n=B):
    """x: the bench's mixture (log_prob's input, data space); c: a normal context; z: the sample
    direction's input, which lives in the base space, so standard normal draws."""
    x = torch.as_tensor(O.gaussian_mixture(n, spec["D"], seed=0))
    c = torch.as_tensor(O.context_normal(n, spec["C"], seed=1)) if spec["C"] else None
    z = torch.randn(n, spec["D"], generator=torch.Generator().manual_seed(2))
    return x, c, z


def _check_both_directions(spec, state, x, c, z, mfma, what):
    f = _flow(spec, state, mfma)
    o64 = O.build_flow(spec, state, torch.float64)
    o32 = O.build_flow(spec, state, torch.float32)
    cd = None if c is None else c.to(DEV)
    c64 = None if c is None else c.double()
    lp = f.log_prob(x.to(DEV), condition=cd)
    st = assert_parity(_np(lp), o64.log_prob(x.double(), c64).numpy(), o32.log_prob(x, c).numpy(),
                       what=f"{what} {mfma} log_prob")
    print(what, mfma, "log_prob", st)
    y, ld = f._plan.sample(z.to(DEV), cd, with_logdet=True)
    y64, ld64 = o64.forward_with_logdet(z.double(), c64)
    y32, ld32 = o32.forward_with_logdet(z, c)
    st = assert_parity(_np(y), y64.numpy(), y32.numpy(), what=f"{what} {mfma} sample y")
    print(what, mfma, "sample y", st)
    st = assert_parity(_np(ld), ld64.numpy(), ld32.numpy(), what=f"{what} {mfma} sample ld")
    print(what, mfma, "sample ld", st)


@pytest.mark.parametrize("mfma", ["f16x3r16", "f32"])
def test_small_config3_flow(mfma):
    x, c, z = _inputs(SPEC3)
    _check_both_directions(SPEC3, _state(SPEC3), x, c, z, mfma, "config3 L2 B133")


@pytest.mark.parametrize("mfma", ["f16x3r16", "f32"])
def test_product_terms(mfma):
    """W0's context columns zeroed and full 24-bit mantissas in W0's x1 columns and in x: GEMM1's
    result is the concatenated step alone, and a missing or misplaced Wh·Xl or Wl·Xh term is an
    error of about 1e-4 in the pre-activations."""
    state = _state(SPEC3)
    C = SPEC3["C"]
    for l in range(SPEC3["L"]):
        W = state[f"layers.{l}.nn.layers.0.weight"].clone()
        W[:, :C] = 0.0
        W[:, C:] = _full_mantissa(W[:, C:], seed=10 + l)
        state[f"layers.{l}.nn.layers.0.weight"] = W
    x, c, z = _inputs(SPEC3)
    _check_both_directions(SPEC3, state, _full_mantissa(x, seed=20), c, _full_mantissa(z, seed=21), mfma,
                           "config3 product terms")


@pytest.mark.parametrize("mfma", ["f16x3r16", "f32"])
def test_config2_shape(mfma):
    """D=8, C=0, S=4: one GEMM1 step, not concatenated (KS1 == 1): the three-MFMA path on the new
    stage-A layout."""
    x, c, z = _inputs(SPEC2)
    _check_both_directions(SPEC2, _state(SPEC2), x, c, z, mfma, "config2 L2 B133")


def test_mixed_range_launch():
    """Two workgroups in one launch: rows 128..255 carry a context value >= 2^15 (exact-fp32 GEMM1
    on the A32 image), rows 0..127 stay in range (fp16 image).  Both images share the bias and table
    offsets, so both workgroups must meet the criterion."""
    state = _state(SPEC3)
    x, c, _ = _inputs(SPEC3, 256)
    c[128:, 3] = 4.0e4
    f = _flow(SPEC3, state, "f16x3r16")
    lp = _np(f.log_prob(x.to(DEV), condition=c.to(DEV)))
    lp64 = O.build_flow(SPEC3, state, torch.float64).log_prob(x.double(), c.double()).numpy()
    lp32 = O.build_flow(SPEC3, state, torch.float32).log_prob(x, c).numpy()
    for name, sl in (("in range", slice(0, 128)), ("fp32 fallback", slice(128, 256))):
        st = assert_parity(lp[sl], lp64[sl], lp32[sl], what=f"mixed-range launch, {name} workgroup")
        print("mixed range", name, st)


def test_row_independence():
    """Rows 0..15 (one wave) of the 133-row launch are bitwise the 16-row launch of the same rows."""
    state = _state(SPEC3)
    x, c, z = _inputs(SPEC3)
    f = _flow(SPEC3, state, "f16x3r16")
    xd, cd, zd = x.to(DEV), c.to(DEV), z.to(DEV)
    lp = f.log_prob(xd, condition=cd)
    lp16 = f.log_prob(xd[:16].contiguous(), condition=cd[:16].contiguous())
    assert torch.equal(lp[:16], lp16)
    y, ld = f._plan.sample(zd, cd, with_logdet=True)
    y16, ld16 = f._plan.sample(zd[:16].contiguous(), cd[:16].contiguous(), with_logdet=True)
    assert torch.equal(y[:16], y16) and torch.equal(ld[:16], ld16)
