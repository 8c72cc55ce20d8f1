"""GPU: the fused nsc kernels at tile edges and in the backward's persistent tile loop.

The three kernels (coupling_r16_kernel in its flow, one-layer and training-forward variants, and
coupling_bwd_r16_kernel) are row-independent by construction: a lane's results depend on its own
row only (the backward's f16x3 operand scale is per row, bwd_row_scale).  So a row's outputs must be
BITWISE equal between two launches that tile the rows differently, and the small launches are the
ones the other GPU files hold to the fp64 oracle.  The one workgroup-wide coupling by design is the
inference kernel's GEMM1 range flag (coupling_r16.h), off while every input is below 2^15.

Numbers used: exact equality; the 1e-5 norm bound of the atomically summed gradients
(test_gpu_train.py: test_fused_bwd_tail_rows_add_nothing, test_fused_train_dw_side_stream_matches);
tests/parity.py's gradient criterion against the oracle.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import naz_oracle as O
from tests.conftest import load_golden, spec_state
from tests.parity import assert_parity, grad_floor
from tests.test_gpu_train import CFG3, _bwd_layer, _cfg3_flow, _tail_layer_case

pytestmark = pytest.mark.gpu
DEV = "cuda"

# coupling.hip launches min(ntiles, BWD_GRID_CAP) backward workgroups of 16 * kBwdWaves rows: a
# workgroup takes a second tile only above BWD_ONE_PASS_ROWS rows (tests/test_nsc_tiles_host.py
# checks these against the sources)
BWD_GRID_CAP = 2048
BWD_TILE_ROWS = 64
BWD_ONE_PASS_ROWS = BWD_GRID_CAP * BWD_TILE_ROWS  # 131072
# workgroups 0 and 1 take three tiles, the rest two (both slot parities whatever the stage count);
# the last tile is ragged: 101 = 64 + 2 waves + 5 rows
B_TILE_LOOP = 2 * BWD_ONE_PASS_ROWS + 101
PER_ROW = ("h1", "h2", "dp1", "dp2", "dp3", "x0")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from naz_amd import _lib
    _lib.lib()


def _np(t):
    return t.detach().double().cpu().numpy()


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _assert_rows_equal(got, ref, what):
    """Bitwise equality of two [n, ...] tensors, naming the first rows that differ."""
    if not torch.equal(got, ref):
        bad = torch.nonzero((got != ref).reshape(got.shape[0], -1).any(dim=1)).reshape(-1)
        pytest.fail(f"{what}: {bad.numel()} of {got.shape[0]} rows differ, first {bad[:8].tolist()}")


# ------------------------------------------------------------------ A. the backward's tile loop
SHAPES = {"d16c32": dict(CFG3), "d8c0": dict(flow_type="nsc", D=8, C=0, hidden=[128, 128], L=6, K=8, split=4)}


def _flow(spec, state):
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import io as fio
    f = NormalizingFlow("nsc", None, spec["D"], spec["C"], spec["hidden"], spec["L"], spec["K"], spec["split"])
    fio.load_state(f, {k: np.asarray(v) for k, v in state.items()})
    return f


@pytest.fixture(scope="module", params=list(SHAPES))
def tile_loop(request):
    """One layer's backward on B_TILE_LOOP rows in one launch: states uniform in (-2.9, 2.9), about
    1 row in 16 (random positions) with every dim in the identity tails, about 1 in 16 with a few."""
    spec = SHAPES[request.param]
    D, C = spec["D"], spec["C"]
    state = {k: v.numpy() for k, v in O.random_state(spec, seed=1234).items()}
    f = _flow(spec, state)
    B = B_TILE_LOOP
    rng = np.random.default_rng(11)
    st = rng.uniform(-2.9, 2.9, size=(B, D)).astype(np.float32)
    kind = rng.random(B)
    tails = np.where(rng.random((B, D)) < 0.5, -1.0, 1.0) * (3.0 + rng.uniform(1e-3, 1.0, size=(B, D)))
    some = (kind[:, None] < 1 / 16) | ((kind[:, None] < 2 / 16) & (rng.random((B, D)) < 0.2))
    st = np.where(some, tails, st).astype(np.float32)
    state_rows = torch.as_tensor(st, device=DEV)
    ctx = torch.as_tensor(O.context_normal(B, C, seed=8), device=DEV) if C else None
    g_in = torch.randn(state_rows.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    bufs, g_out, g_low = _bwd_layer(f, state_rows, ctx, g_in)
    out = dict(spec=spec, state=state, f=f, st=state_rows, ctx=ctx, g_in=g_in, bufs=bufs, g_out=g_out, g_low=g_low)
    yield out
    out.clear()
    del bufs, g_out, state_rows, ctx, g_in
    torch.cuda.empty_cache()


def test_bwd_tile_loop_matches_one_pass_launches(tile_loop):
    """coupling_bwd_r16_kernel is persistent: above BWD_ONE_PASS_ROWS rows a workgroup loops over
    tiles (the has_next prefetch of the next tile's stage 0, the stage counter's slot parity carried
    across tiles, glow summed over tiles).  Every per-row output of the looping launch must be bitwise
    that of three launches of <= 100000 rows (one tile per workgroup; boundaries off the 64-row
    tile, so the row-to-lane mapping shifts too); g_low the sum of theirs to the atomics' rounding;
    rows wholly in the tails pass g_in through with a zero dPre3 row."""
    t = tile_loop
    B = t["st"].shape[0]
    assert B > BWD_ONE_PASS_ROWS
    g_low_sum = torch.zeros_like(t["g_low"])
    chunk = 99999  # odd: the second launch's rows change lane parity too, so no lane group stays together
    for lo in range(0, B, chunk):
        hi = min(lo + chunk, B)
        assert hi - lo <= BWD_ONE_PASS_ROWS
        ctx = None if t["ctx"] is None else t["ctx"][lo:hi]
        bufs, g_out, g_low = _bwd_layer(t["f"], t["st"][lo:hi], ctx, t["g_in"][lo:hi])
        _assert_rows_equal(t["g_out"][lo:hi], g_out, f"g_out rows [{lo}, {hi})")
        for k in PER_ROW:
            _assert_rows_equal(t["bufs"][k][lo:hi], bufs[k], f"{k} rows [{lo}, {hi})")
        g_low_sum += g_low
        del bufs, g_out, g_low
    assert bool(torch.isfinite(t["g_low"]).all())
    rel = _rel(t["g_low"], g_low_sum)
    print(f"g_low: tile loop vs the chunk launches' sum {rel:.2e}")
    assert rel < 1e-5, f"g_low: tile loop vs the chunk launches' sum {rel:.2e}"
    tail = (t["st"].abs() > 3.0).all(dim=1)
    assert int(tail.sum()) > B // 32 and int((~tail & (t["st"].abs() > 3.0).any(dim=1)).sum()) > B // 32
    _assert_rows_equal(t["g_out"][tail], t["g_in"][tail], "tail rows' g_out vs g_in")
    assert int(torch.count_nonzero(t["bufs"]["dp3"][tail])) == 0, "tail rows gave the conditioner a gradient"
    assert bool(torch.isfinite(t["g_out"]).all())
    for k in PER_ROW:
        assert bool(torch.isfinite(t["bufs"][k]).all()), f"{k} not finite"


def test_bwd_tile_loop_subsample_vs_oracle(tile_loop):
    """Every 127th row of the looping launch against autograd of the oracle's layer, float64 and
    float32, with the gradient criterion of tests/parity.py (rows are independent, so the
    subsample's oracle is the full batch's).

    Cotangent convention (flows/flow.py, _CouplingTrainFn.backward): the kernel takes g_in =
    dLoss/dP[l], the gradient on the layer's log_prob-direction OUTPUT x = T^-1(y), and g_lp =
    dLoss/dlog p per row, unscaled and unnegated; log p sums the log-dets of the inverse maps, i.e.
    MINUS the forward log-det that the oracle's layer.inverse returns per dim (Flow.log_prob: lp -=
    ld.sum(-1)).  So g_out = d/dy [ sum(x * g_in) - sum(g_lp * ld.sum(-1)) ]."""
    t = tile_loop
    spec, layer = t["spec"], 2
    idx = torch.arange(0, t["st"].shape[0], 127, device=DEV)
    y_h = t["st"][idx].cpu()
    c_h = None if t["ctx"] is None else t["ctx"][idx].cpu()
    g_h = t["g_in"][idx].cpu()
    g_lp = -1.0 / (1 << 16)  # _bwd_layer's constant
    ref = {}
    for dt in (torch.float64, torch.float32):
        ol = O.build_flow(spec, t["state"], dt).layers[layer]
        y = y_h.to(dt).requires_grad_(True)
        x, ld = ol.inverse(y, None if c_h is None else c_h.to(dt))
        s = (x * g_h.to(dt)).sum() - (g_lp * ld.sum(-1)).sum()
        ref[dt] = _np(torch.autograd.grad(s, y)[0])
    r64 = ref[torch.float64]
    st = assert_parity(_np(t["g_out"][idx]), r64, ref[torch.float32], what=f"{spec['D']}|{spec['C']} tile-loop g_out",
                       floor=grad_floor(r64), count_factor=None)
    print("tile-loop g_out vs oracle", st)


def test_fused_step_above_one_pass_matches_chunked_accumulation():
    """End to end through _CouplingTrainFn: the NLL gradient of an L=2 config-3-shaped flow at
    BWD_ONE_PASS_ROWS + 101 rows (every backward launch loops) against the gradient accumulated from
    the same rows in two chunks below the threshold, each chunk's loss weighted by its share of rows;
    per parameter tensor norm-wise within 1e-5 (the batch reductions' summation order)."""
    from naz_amd.flows import io as fio
    spec = dict(CFG3, L=2)
    state = {k: v.numpy() for k, v in O.random_state(spec, seed=33).items()}
    f = _flow(spec, state)
    B = BWD_ONE_PASS_ROWS + 101
    x = torch.as_tensor(O.gaussian_mixture(B, 16, seed=12), device=DEV)
    c = torch.as_tensor(O.context_normal(B, 32, seed=13), device=DEV)
    params = fio.named_state_params(f)
    assert f._plan.train_ready(x, c)
    (-f.log_prob(x, condition=c).mean()).backward()
    one = {k: p.grad.detach().clone() for k, p in params.items()}
    for p in params.values():
        p.grad = None
    h = 70001
    for rows in (slice(0, h), slice(h, B)):
        xs, cs = x[rows], c[rows]
        assert xs.shape[0] <= BWD_ONE_PASS_ROWS and f._plan.train_ready(xs, cs)
        (-f.log_prob(xs, condition=cs).mean() * (xs.shape[0] / B)).backward()
    for k, p in params.items():
        assert bool(torch.isfinite(one[k]).all()), f"d/d{k} not finite"
        rel = _rel(one[k], p.grad)
        assert rel < 1e-5, f"d/d{k}: one looping pass vs two one-pass chunks {rel:.2e}"


# ------------------------------------------------------------------ B. tails and inside rows in one wave
B_MIX = 4096 + 37


@functools.lru_cache(maxsize=None)
def _mixed_case(kind):
    """The r06 singular lower spline (_tail_layer_case) at B_MIX rows (a partial last tile).
    "interleaved": half the rows in the tails, then a fixed permutation, so tails and inside rows
    alternate inside every 16-row wave; "split": unpermuted with the first 2048 + 5 rows in the
    tails, a boundary off the tile (and the wave) edge.  Returns the flow, the state, context and
    g_in rows, and the tail mask."""
    B = B_MIX
    nt_want = B // 2 if kind == "interleaved" else 2048 + 5
    f, st, nt = _tail_layer_case(B, (nt_want + 0.5) / B)
    assert nt == nt_want
    ctx = torch.as_tensor(O.context_normal(B, 32, seed=8), device=DEV)
    g_in = torch.randn(st.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    tail = torch.arange(B, device=DEV) < nt
    if kind == "interleaved":
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(17)).to(DEV)
        st, ctx, g_in, tail = st[perm].contiguous(), ctx[perm].contiguous(), g_in[perm].contiguous(), tail[perm]
        waves = torch.nn.functional.pad(tail.float(), (0, -B % 16), value=0.5).reshape(-1, 16)
        assert bool(((waves == 1).any(dim=1) & (waves == 0).any(dim=1))[:B // 16].all()), "a wave is not mixed"
    else:
        assert nt % BWD_TILE_ROWS and nt % 16
    assert bool((st[tail].abs() > 3.0).all()) and bool((st[~tail].abs() < 3.0).all())
    return f, st, ctx, g_in, tail


@pytest.mark.parametrize("kind", ["interleaved", "split"])
def test_fused_bwd_inside_rows_unchanged_by_tail_rows_in_their_wave(kind):
    """VERDICT r06 Next #3: tail rows and inside rows mixed inside the 16-row waves and across a
    tile-misaligned boundary.  Every per-row output of the inside rows (g_out and the dW operands)
    is bitwise that of the inside rows launched alone in the same order; g_low agrees to the
    atomics' rounding; tail rows pass g_in through with a zero dPre3 row; everything finite."""
    f, st, ctx, g_in, tail = _mixed_case(kind)
    ins = torch.nonzero(~tail).reshape(-1)
    bufs, g_out, g_low = _bwd_layer(f, st, ctx, g_in)
    bufs_i, g_out_i, g_low_i = _bwd_layer(f, st[ins].contiguous(), ctx[ins].contiguous(), g_in[ins].contiguous())
    assert bool(torch.isfinite(g_low).all()) and bool(torch.isfinite(g_out).all())
    for k in PER_ROW:
        assert bool(torch.isfinite(bufs[k]).all()), f"{k} not finite"
    _assert_rows_equal(g_out[ins], g_out_i, "inside rows' g_out")
    for k in PER_ROW:
        _assert_rows_equal(bufs[k][ins], bufs_i[k], f"inside rows' {k}")
    rel = _rel(g_low, g_low_i)
    assert rel < 1e-5, f"tail rows changed the lower-spline gradient: {rel:.2e}"
    _assert_rows_equal(g_out[tail], g_in[tail], "tail rows' g_out vs g_in")
    assert int(torch.count_nonzero(bufs["dp3"][tail])) == 0


def test_train_forward_inside_rows_unchanged_by_tail_rows_in_their_wave():
    """The interleaved batch through the training forward (coupling_r16_kernel VAR = 1, all 8
    layers): log_prob and every saved state row of the inside rows are bitwise those of the
    inside-only launch, and everything is finite."""
    from naz_amd import ops
    f, st, ctx, _, tail = _mixed_case("interleaved")
    plan = f._plan
    assert plan.train_ready(st, ctx)
    packed, _, _ = plan.packed_bwd()
    d = plan.desc

    def fwd(xx, cc):
        states = torch.empty((d.L + 1, xx.shape[0], d.D), device=DEV)
        return ops.coupling_log_prob_train(d, packed, xx, cc, None, None, states), states

    ins = torch.nonzero(~tail).reshape(-1)
    lp, states = fwd(st, ctx)
    lp_i, states_i = fwd(st[ins].contiguous(), ctx[ins].contiguous())
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(states).all())
    _assert_rows_equal(lp[ins], lp_i, "inside rows' log_prob")
    _assert_rows_equal(states[:, ins].transpose(0, 1), states_i.transpose(0, 1), "inside rows' saved states")


# ------------------------------------------------------------------ C. ragged batches, every variant
NSC = ["nsc_d16c32_l2.npz", "nsc_d8c0_l6.npz", "nsc_d6c2_small.npz"]
RAGGED = [1, 15, 17, 127, 129, 255]


def _r16_ok(spec):
    return spec["split"] % 4 == 0 and (spec["D"] - spec["split"]) % 4 == 0


def _fixture_flow(name):
    fx = load_golden(name)
    spec, state = spec_state(fx)
    f = _flow(spec, state)
    assert f.fused, "the nsc fixture shapes must hit a fused instantiation"
    c = torch.as_tensor(fx["ctx"], dtype=torch.float32, device=DEV) if "ctx" in fx else None
    return fx, spec, f, c


def _head(t, n):
    return None if t is None else t[:n]


@pytest.mark.parametrize("name", NSC)
@pytest.mark.parametrize("direction", ["log_prob", "sample"])
def test_ragged_flow_kernel_rows_equal_full_launch(name, direction):
    """Partial waves and partial workgroups of the whole-flow kernel ("auto" mode), both directions:
    rows [:B] launched alone are bitwise rows [:B] of the whole fixture's launch (256 rows; 300 for
    nsc_d6c2_small), the one test_flow_log_prob_vs_golden / test_flow_sample_transform_vs_golden hold
    to the oracle."""
    fx, spec, f, c = _fixture_flow(name)
    v = torch.as_tensor(fx["x" if direction == "log_prob" else "z"], dtype=torch.float32, device=DEV)
    assert v.shape[0] > max(RAGGED)

    def run(n):
        with torch.no_grad():
            if direction == "log_prob":
                return (f.log_prob(v[:n], condition=_head(c, n)),)
            return f._plan.sample(v[:n], _head(c, n), with_logdet=True)

    full = run(v.shape[0])
    if _r16_ok(spec):
        assert f._plan.mode == "f16x3r16"
    for n in RAGGED:
        for a, b, what in zip(run(n), full, ("y / lp", "ld")):
            _assert_rows_equal(a, b[:n], f"{name} {direction} {what} at B = {n}")


@pytest.mark.parametrize("name", [n for n in NSC if n != "nsc_d6c2_small.npz"])
def test_ragged_layer_kernel_rows_equal_full_launch(name, monkeypatch):
    """The one-layer kernel (coupling_r16_kernel VAR = 2) through the per-Transform protocol, t(v)
    and t._inverse(y) with the cached log-det, every layer: ragged launches on the head of the
    256-row launch's own inputs give its rows bitwise."""
    from naz_amd import ops
    fx, spec, f, c = _fixture_flow(name)
    assert _r16_ok(spec)
    calls = []
    orig = ops.coupling_layer
    monkeypatch.setattr(ops, "coupling_layer", lambda *a, **k: calls.append(1) or orig(*a, **k))

    def layers(n):
        return [t for t in f._pdf(_head(c, n)).transforms if hasattr(t, "module")]

    def both(t, v):
        y = t(v)
        ld = t.log_abs_det_jacobian(v, y)
        xi = t._inverse(y)
        return y, ld, xi, t._cache_log_detJ

    with torch.no_grad():
        full, v = [], torch.as_tensor(fx["x"], dtype=torch.float32, device=DEV)
        for t in layers(256):
            full.append((v,) + both(t, v))
            v = full[-1][1]
        assert len(calls) >= 2 * len(full), "the per-layer fused kernel was not used"
        for n in RAGGED:
            for l, (t, ref) in enumerate(zip(layers(n), full)):
                for a, b, what in zip(both(t, ref[0][:n]), ref[1:], ("y", "ld", "inverse x", "inverse ld")):
                    _assert_rows_equal(a, b[:n], f"{name} layer {l} {what} at B = {n}")
        assert len(calls) >= 2 * len(full) * (1 + len(RAGGED))


@pytest.mark.parametrize("name", [n for n in NSC if n != "nsc_d6c2_small.npz"])
def test_ragged_train_forward_rows_equal_full_launch(name):
    """The training forward (coupling_r16_kernel VAR = 1) on ragged batches: log_prob and every
    saved state row are bitwise those of the 256-row launch."""
    from naz_amd import ops
    fx, spec, f, c = _fixture_flow(name)
    x = torch.as_tensor(fx["x"], dtype=torch.float32, device=DEV)
    plan = f._plan
    assert plan.train_ready(x, c)
    packed, _, _ = plan.packed_bwd()
    d = plan.desc

    def fwd(n):
        states = torch.empty((d.L + 1, n, d.D), device=DEV)
        return ops.coupling_log_prob_train(d, packed, x[:n], _head(c, n), None, None, states), states

    lp, states = fwd(256)
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(states).all())
    for n in RAGGED:
        lp_n, states_n = fwd(n)
        _assert_rows_equal(lp_n, lp[:n], f"{name} train log_prob at B = {n}")
        _assert_rows_equal(states_n.transpose(0, 1), states[:, :n].transpose(0, 1), f"{name} states at B = {n}")


@pytest.mark.parametrize("mfma", ["f16x3r16", "f16x3"])
def test_gemm1_range_flag_is_per_workgroup_in_ragged_batches(mfma):
    """The legitimate workgroup coupling: one row with context x 5e4 sends its 128-row workgroup's
    GEMM1 off the fp16 path (coupling_r16.h / coupling_w32.h: the range flag).  Config 3, B = 300
    (two full workgroups and a ragged one); the large row mid-workgroup and mid-wave (201), then in
    the ragged last workgroup (299): both runs match the live oracle over all rows, and the rows of
    the workgroups that hold no large row are bitwise those of the unscaled run.  (With the wave's
    vote taken inside a lane-0 branch, only a wave's first row could raise the flag: a single large
    row elsewhere took the fp16 path and came out NaN.)"""
    state = {k: v.numpy() for k, v in O.random_state(CFG3, seed=1234).items()}
    f = _cfg3_flow(state)
    f._plan.set_mfma(mfma)
    n = 300
    x = torch.as_tensor(O.gaussian_mixture(n, 16, seed=3))
    c0 = torch.as_tensor(O.context_normal(n, 32, seed=4))
    with torch.no_grad():
        base = f.log_prob(x.to(DEV), condition=c0.to(DEV))
    for big in (201, 299):
        c = c0.clone()
        c[big] *= 5e4
        with torch.no_grad():
            lp = f.log_prob(x.to(DEV), condition=c.to(DEV))
        lp64 = O.build_flow(CFG3, state, torch.float64).log_prob(x.double(), c.double()).numpy()
        lp32 = O.build_flow(CFG3, state, torch.float32).log_prob(x, c).numpy()
        assert_parity(_np(lp), lp64, lp32, what=f"config3 {mfma} B=300, row {big} context x 5e4")
        wg = big // 128
        other = torch.ones(n, dtype=torch.bool, device=DEV)
        other[128 * wg:128 * (wg + 1)] = False
        _assert_rows_equal(lp[other], base[other], f"rows outside workgroup {wg}")
