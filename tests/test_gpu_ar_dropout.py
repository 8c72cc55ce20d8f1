"""GPU: the fused sampler with MC dropout (naz_ar_flow_sample_dropout, csrc/made_ar_dropout.h) —
sample() of an nsa / maf flow built with dropout_p in train mode, and
MCDPNormalizingFlow.sample_uncertain, as one launch per flow (per chunk of iterations).

The reference is a float64 / float32 restatement of the forward direction with the kernel's own
masks multiplied in (tests/ar_dropout_ref.py; masks recovered by naz_dropout on ones, as
test_gpu_dropout.py does): a wrong row or column index in the fused hash gives O(1) errors.
B = 421 rows: three workgroup tiles (192 or 128 rows) with a ragged tail."""
import numpy as np
import pytest
import torch

from oracle import naz_oracle as O
from tests.ar_dropout_ref import dropout_flow, kernel_masks
from tests.parity import assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 421

MAF2 = dict(flow_type="maf", D=2, C=2, hidden=[150, 150, 150], L=3)
MAF4 = dict(flow_type="maf", D=4, C=2, hidden=[150, 150, 150], L=3)
NSA4 = dict(flow_type="nsa", D=4, C=2, hidden=[128, 128], L=3, K=8)
CASES = [(MAF2, "rows"), (MAF4, "one"), (NSA4, "rows")]  # context: one per row / a single vector


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _id(case):
    spec, ctx = case
    return f"{spec['flow_type']}D{spec['D']}C{spec['C']}-ctx_{ctx}"


_FLOWS = {}


def _flow(spec, p, bounds=None, cls=None):
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import io as fio
    key = (spec["flow_type"], spec["D"], p, bounds is not None, cls)
    if key not in _FLOWS:
        state = {k: v.float() for k, v in O.random_state(spec, seed=11).items()}
        extra = (spec["K"],) if spec["flow_type"] == "nsa" else ()
        kw = {} if p is None else dict(dropout_p=p)
        f = (cls or NormalizingFlow)(spec["flow_type"], bounds, spec["D"], spec["C"], spec["hidden"], spec["L"], *extra,
                                     **kw)
        fio.load_state(f, {k: v.numpy() for k, v in state.items()})
        _FLOWS[key] = (f.to(DEV), state)
    f, state = _FLOWS[key]
    f.train()
    return f, state


def _inputs(spec, ctx):
    g = torch.Generator().manual_seed(5)
    z = torch.randn(B, spec["D"], generator=g)
    c = torch.randn(B if ctx == "rows" else 1, spec["C"], generator=g)
    return z, (c if ctx == "rows" else c[0])


def _seeds(spec, draws=None, seed=17):
    g = torch.Generator().manual_seed(seed)
    shape = (spec["L"], len(spec["hidden"])) if draws is None else (draws, spec["L"], len(spec["hidden"]))
    return torch.randint(0, 2 ** 62, shape, generator=g, dtype=torch.int64)


def _fused(f, z, c, p, seeds, **kw):
    from naz_amd import ops
    plan = f._plan
    return ops.ar_flow_sample_dropout(plan.desc, plan.packed_fwd(), z.to(DEV), c.to(DEV), kw.pop("low", None),
                                      kw.pop("high", None), p, seeds.to(DEV), with_logdet=True, **kw)


@pytest.mark.parametrize("case,p", [(c, 0.25) for c in CASES] + [(CASES[0], 0.9)],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else f"p{v}")
def test_parity_fused_and_per_layer(case, p, monkeypatch):
    from naz_amd.nn import _DropoutMixin
    spec, ctx = case
    f, state = _flow(spec, p)
    assert f._plan is not None and f._plan.dropout_sample_usable()
    z, c = _inputs(spec, ctx)
    seeds = _seeds(spec)
    masks = kernel_masks(seeds.tolist(), p, B, spec["hidden"][0])
    keep = float(np.mean([float((m != 0).double().mean()) for lm in masks for m in lm]))
    assert abs(keep - (1 - p)) < 0.02, keep
    y64, ld64 = dropout_flow(spec, state, torch.float64, masks).forward_with_logdet(z.double(), c.double())
    y32, ld32 = dropout_flow(spec, state, torch.float32, masks).forward_with_logdet(z, c)
    y, ld = _fused(f, z, c, p, seeds)
    what = f"{_id(case)} p={p}"
    sy = assert_parity(y.double().cpu().numpy(), y64.numpy(), y32.numpy(), what=f"fused y {what}")
    # the summed log-det: test_gpu_ar_fused.py's bound for the same spline / affine arithmetic
    sl = assert_parity(ld.double().cpu().numpy(), ld64.numpy(), ld32.numpy(), what=f"fused ld {what}",
                       count_factor=3.0)
    print(what, "fused y", sy, "ld", sl)
    # the per-layer path under the same seeds, handed out in layer order
    it = iter(seeds.tolist())
    monkeypatch.setattr(_DropoutMixin, "_drop_args",
                        lambda self: (float(self.dropout_p), next(it)) if self.dropout_active() else None)
    with torch.no_grad():
        pdf = f._pdf(c.to(DEV))
        yw, ldw = z.to(DEV), torch.zeros(B, device=DEV)
        for t in pdf.transforms:
            yw = t._call_acc(yw, ldw)
    assert_parity(yw.double().cpu().numpy(), y64.numpy(), y32.numpy(), what=f"per-layer y {what}")
    assert_parity(ldw.double().cpu().numpy(), ld64.numpy(), ld32.numpy(), what=f"per-layer ld {what}",
                  count_factor=3.0)
    print(what, "max |fused - per-layer| y", float((y - yw).abs().max()), "ld", float((ld - ldw).abs().max()))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_p0_is_the_plain_sampler_bitwise(case):
    from naz_amd import ops
    spec, ctx = case
    f, _ = _flow(spec, 0.25)
    z, c = _inputs(spec, ctx)
    y, ld = _fused(f, z, c, 0.0, _seeds(spec))
    y0, ld0 = ops.ar_flow_sample(f._plan.desc, f._plan.packed_fwd(), z.to(DEV), c.to(DEV), with_logdet=True)
    assert torch.equal(y, y0) and torch.equal(ld, ld0)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_chunks_draws_determinism(case):
    spec, ctx = case
    p = 0.25
    f, _ = _flow(spec, p)
    z, c = _inputs(spec, ctx)
    seeds = _seeds(spec)
    y, ld = _fused(f, z, c, p, seeds)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(ld).all())
    # determinism
    y2, ld2 = _fused(f, z, c, p, seeds)
    assert torch.equal(y, y2) and torch.equal(ld, ld2)
    # chunking: rows [0, 200) and [200, 421) with their offsets
    rows = ctx == "rows"
    ya, lda = _fused(f, z[:200], c[:200] if rows else c, p, seeds, row_offset=0)
    yb, ldb = _fused(f, z[200:], c[200:] if rows else c, p, seeds, row_offset=200)
    assert torch.equal(torch.cat([ya, yb]), y) and torch.equal(torch.cat([lda, ldb]), ld)
    if rows:
        return  # draws share the context: the per-row contexts differ per draw only through z here
    # draws: [P = 3, B, D] in one launch == three single-draw launches with the seed rows
    g = torch.Generator().manual_seed(9)
    z3 = torch.randn(3, B, spec["D"], generator=g)
    s3 = _seeds(spec, draws=3, seed=23)
    y3, ld3 = _fused(f, z3, c, p, s3)
    assert y3.shape == (3, B, spec["D"]) and ld3.shape == (3, B)
    for i in range(3):
        yi, ldi = _fused(f, z3[i], c, p, s3[i])
        assert torch.equal(y3[i], yi) and torch.equal(ld3[i], ldi), i
    # two draws of the same z with different seeds differ
    zz = torch.stack([z, z])
    yy, _ = _fused(f, zz, c, p, s3[:2])
    assert not torch.equal(yy[0], yy[1])


def test_draws_with_per_row_contexts():
    """[P, B, D] with one context row per sample row (shared by the draws)."""
    spec, p = MAF2, 0.25
    f, _ = _flow(spec, p)
    z, c = _inputs(spec, "rows")
    s2 = _seeds(spec, draws=2, seed=29)
    y2, ld2 = _fused(f, torch.stack([z, z.flip(0)]), c, p, s2)
    for i, zi in enumerate((z, z.flip(0))):
        yi, ldi = _fused(f, zi, c, p, s2[i])
        assert torch.equal(y2[i], yi) and torch.equal(ld2[i], ldi)


def test_bounds_are_bounding_inv_of_the_unbounded_result():
    from naz_amd import ops
    spec, p = NSA4, 0.25
    f, _ = _flow(spec, p)
    z, c = _inputs(spec, "rows")
    seeds = _seeds(spec)
    low = torch.full((spec["D"],), -2.0, device=DEV)
    high = torch.tensor([3.0, 4.0, 5.0, 6.5], device=DEV)
    y, ld = _fused(f, z, c, p, seeds)
    yb, ldb = _fused(f, z, c, p, seeds, low=low, high=high)
    torch.testing.assert_close(yb, ops.bounding_inv(y, low, high), rtol=1e-6, atol=1e-6)
    assert torch.equal(ld, ldb)
    assert bool((yb > low).all()) and bool((yb < high).all())


def test_p_beyond_the_f16_pieces_is_refused():
    """1 / (1 - p) = 2^20 would push the scaled activation out of the f16 hi piece: an error, no launch."""
    spec = MAF2
    f, _ = _flow(spec, 0.25)
    z, c = _inputs(spec, "rows")
    with pytest.raises(RuntimeError, match="beyond the f16 pieces"):
        _fused(f, z, c, 1.0 - 2.0 ** -20, _seeds(spec))
    y, _ = _fused(f, z, c, 1.0 - 2.0 ** -16, _seeds(spec))  # scale 65536: the largest accepted
    assert bool(torch.isfinite(y).all())


def test_flow_sample_takes_the_fused_path_and_eval_is_untouched(monkeypatch):
    from naz_amd import ops
    spec, p = MAF4, 0.25
    f, _ = _flow(spec, p)
    f0, _ = _flow(spec, None)
    c = torch.randn(B, spec["C"], device=DEV)
    calls = dict(drop=0, fused=0)
    real_drop, real_fused = ops.dropout, ops.ar_flow_sample_dropout
    monkeypatch.setattr(ops, "dropout", lambda *a, **k: (calls.__setitem__("drop", calls["drop"] + 1), real_drop(*a, **k))[1])
    monkeypatch.setattr(ops, "ar_flow_sample_dropout",
                        lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), real_fused(*a, **k))[1])
    torch.manual_seed(3)
    a = f.sample([B], condition=c)
    torch.manual_seed(3)
    b = f.sample([B], condition=c)
    assert calls == dict(drop=0, fused=2) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    # the per-layer path draws the same z and the same seeds under the same torch seed
    monkeypatch.setenv("NAZ_AR_DROPOUT_FUSED", "0")
    torch.manual_seed(3)
    w = f.sample([B], condition=c)
    assert calls["drop"] == spec["L"] * len(spec["hidden"]) and calls["fused"] == 2
    torch.testing.assert_close(a, w, rtol=1e-3, atol=1e-3)
    monkeypatch.delenv("NAZ_AR_DROPOUT_FUSED")
    # eval mode: the flow built without dropout, bitwise (the plain fused sampler)
    f.eval()
    f0.eval()
    z = torch.randn(B, spec["D"], device=DEV)
    with torch.no_grad():
        ye = f._pdf(c)._transform_z(z)
        y0 = f0._pdf(c)._transform_z(z)
    assert torch.equal(ye, y0) and calls == dict(drop=spec["L"] * len(spec["hidden"]), fused=2)


def test_sample_uncertain(monkeypatch):
    from naz_amd import ops
    from naz_amd.flows.mcdpflow import MCDPNormalizingFlow
    spec, p = MAF2, 0.25
    f, _ = _flow(spec, p, cls=MCDPNormalizingFlow)
    c = torch.tensor([0.3, -0.7], device=DEV)
    calls = dict(drop=0, fused=0)
    real_drop, real_fused = ops.dropout, ops.ar_flow_sample_dropout
    monkeypatch.setattr(ops, "dropout", lambda *a, **k: (calls.__setitem__("drop", calls["drop"] + 1), real_drop(*a, **k))[1])
    monkeypatch.setattr(ops, "ar_flow_sample_dropout",
                        lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), real_fused(*a, **k))[1])

    def check(s):
        assert s.shape == (4, 2000, 2) and np.isfinite(s).all()
        assert all(not np.array_equal(s[i], s[j]) for i in range(4) for j in range(i))

    torch.manual_seed(5)
    s = f.sample_uncertain(4, [2000], condition=c)
    check(s)
    assert calls == dict(drop=0, fused=1), "one launch for the one chunk, no per-layer dropout launches"
    torch.manual_seed(5)
    assert np.array_equal(f.sample_uncertain(4, [2000], condition=c), s)
    # a row budget below two iterations: one launch per iteration
    monkeypatch.setattr(MCDPNormalizingFlow, "ROW_BUDGET", 3000)
    calls.update(drop=0, fused=0)
    check(f.sample_uncertain(4, [2000], condition=c))
    assert calls == dict(drop=0, fused=4)
    monkeypatch.setenv("NAZ_AR_DROPOUT_FUSED", "0")
    calls.update(drop=0, fused=0)
    torch.manual_seed(5)
    w = f.sample_uncertain(4, [2000], condition=c)
    check(w)
    assert calls["fused"] == 0 and calls["drop"] == 4 * spec["L"] * len(spec["hidden"])
    torch.manual_seed(5)
    assert np.array_equal(f.sample_uncertain(4, [2000], condition=c), w)
