"""CPU: the fused MC-dropout sampler (include/naz_hip.h naz_ar_flow_sample_dropout*, csrc/
made_ar_dropout.h) — which descriptors have an instance, the host-side checks, and the plan's
decisions on CPU-constructed flows.  No GPU here: every call fails or returns before a launch."""
import pytest

SUPPORTED = [("maf", 2, 2, 150, 3), ("maf", 4, 2, 150, 3), ("nsa", 4, 2, 128, 2)]


def _lib_ops():
    from naz_amd import _lib, ops
    return _lib.lib(), ops


def _call(L, d, packed=16, z=16, ctx=16, ldc=2, low=None, high=None, y=16, B=128, P=1, p=0.25, seeds=16):
    return L.naz_ar_flow_sample_dropout(d, packed, z, d.D, B * d.D, ctx, ldc, low, high, y, d.D, B * d.D, None, B, B,
                                        P, p, seeds, 0, None)


def test_symbols_exported_and_bound():
    from naz_amd import _lib, ops
    L = _lib.lib()
    for name in ("naz_ar_flow_sample_dropout", "naz_ar_flow_sample_dropout_supported"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert callable(ops.ar_flow_sample_dropout) and callable(ops.ar_flow_sample_dropout_supported)
    assert L.naz_abi_version() == 3


def test_supported_shapes():
    L, ops = _lib_ops()
    for kind, D, C, H, nh in SUPPORTED:
        d = ops.ar_flow_desc(kind, D, C, H, 3, nh)
        assert L.naz_ar_flow_sample_dropout_supported(d) == 1 and ops.ar_flow_sample_dropout_supported(d)
    for bad in (ops.ar_flow_desc("nsa", 16, 32, 128, 3, 2), ops.ar_flow_desc("nsa", 8, 0, 128, 3, 2),
                ops.ar_flow_desc("nsa_linear", 4, 2, 128, 3, 2), ops.ar_flow_desc("maf", 4, 2, 512, 3, 5),
                ops.ar_flow_desc("maf", 2, 2, 150, 3, 2), ops.ar_flow_desc("maf", 2, 2, 150, 3, 3, act="relu"),
                ops.ar_flow_desc("nsa", 4, 2, 128, 3, 2, act="relu")):
        assert L.naz_ar_flow_sample_dropout_supported(bad) == 0 and not ops.ar_flow_sample_dropout_supported(bad)
    assert L.naz_ar_flow_sample_dropout_supported(None) == 0


@pytest.mark.parametrize("kind,D,C,H,nh", SUPPORTED)
def test_host_errors(kind, D, C, H, nh):
    L, ops = _lib_ops()
    d = ops.ar_flow_desc(kind, D, C, H, 3, nh)
    for kw in (dict(packed=None), dict(z=None), dict(y=None), dict(seeds=None)):
        assert _call(L, d, **kw) != 0 and b"null pointer" in L.naz_last_error(), kw
    assert _call(L, d, B=-1) != 0 and b"negative size" in L.naz_last_error()
    assert _call(L, d, P=-1) != 0 and b"negative size" in L.naz_last_error()
    assert _call(L, d, P=65536) != 0 and b"at most 65535 draws" in L.naz_last_error()
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert _call(L, d, p=p) != 0 and b"p must be in [0, 1)" in L.naz_last_error(), p
    assert _call(L, d, ctx=None, ldc=0) != 0 and b"needs ctx" in L.naz_last_error()
    assert _call(L, d, low=16) != 0 and b"low/high" in L.naz_last_error()
    # 16 is no packed image: refused by the image registry before any launch
    assert _call(L, d) != 0 and b"not a packed image" in L.naz_last_error()
    # no rows or no draws: no launch, no pointer read
    assert _call(L, d, packed=None, z=None, ctx=None, y=None, seeds=None, B=0) == 0
    assert _call(L, d, packed=None, z=None, ctx=None, y=None, seeds=None, P=0) == 0


def test_descriptor_without_instance_is_named():
    L, ops = _lib_ops()
    for bad, frag in ((ops.ar_flow_desc("nsa", 16, 32, 128, 3, 2), b"D=16 C=32 H=128 x 2"),
                      (ops.ar_flow_desc("maf", 4, 2, 512, 3, 5), b"D=4 C=2 H=512 x 5"),
                      (ops.ar_flow_desc("nsa_linear", 4, 2, 128, 3, 2), b"kind=2 D=4 C=2 H=128 x 2")):
        assert _call(L, bad) != 0
        msg = L.naz_last_error()
        assert b"no dropout sampler" in msg and frag in msg, msg
    assert L.naz_ar_flow_sample_dropout(None, 16, 16, 2, 0, 16, 2, None, None, 16, 2, 0, None, 0, 128, 1, 0.25, 16, 0,
                                        None) != 0
    assert b"null descriptor" in L.naz_last_error()


def test_p_beyond_the_f16_pieces_is_refused_not_overflowed():
    """1 / (1 - p) > 65536 would push the scaled activation out of the kernel's f16 hi piece: the
    entry says so (after the image resolves, so here the plan's routing is what is checked)."""
    from naz_amd import ops
    from naz_amd.flows import NormalizingFlow
    f = NormalizingFlow("maf", None, 2, 2, [150] * 3, 2, dropout_p=1.0 - 2.0 ** -20)
    f.train()
    assert f._plan is not None and f._plan.dropout_p() is not None
    assert 1.0 / (1.0 - f._plan.dropout_p()) > ops.AR_DROPOUT_MAX_SCALE
    assert not f._plan.dropout_sample_usable()  # the per-layer path


def _usable(f):
    return f._plan is not None and f._plan.dropout_sample_usable()


@pytest.mark.parametrize("ftype,args", [("maf", (2, 2, [150] * 3, 2)), ("maf", (4, 2, [150] * 3, 2)),
                                        ("nsa", (4, 2, [128, 128], 2, 8))])
def test_plan_decisions(ftype, args, monkeypatch):
    from naz_amd.flows import NormalizingFlow
    monkeypatch.delenv("NAZ_AR_DROPOUT_FUSED", raising=False)
    f = NormalizingFlow(ftype, None, *args, dropout_p=0.25)
    f.train()
    assert _usable(f)
    assert not f._plan.usable(), "the log_prob / no-dropout decisions are unchanged: False in train mode"
    monkeypatch.setenv("NAZ_AR_DROPOUT_FUSED", "0")
    assert not _usable(f), "the A/B switch keeps the per-layer path"
    monkeypatch.delenv("NAZ_AR_DROPOUT_FUSED")
    f.eval()
    assert not _usable(f) and f._plan.usable()
    # no dropout at all: never
    g = NormalizingFlow(ftype, None, *args)
    g.train()
    assert not _usable(g) and g._plan.usable()


def test_plan_decisions_elsewhere():
    from naz_amd.flows import NormalizingFlow
    f = NormalizingFlow("maf", None, 2, 2, [32, 32], 2, dropout_p=0.25)
    f.train()
    assert not _usable(f)
    f = NormalizingFlow("maf", None, 4, 2, [150] * 3, 2, dropout_p=0.25, random_perm=True)
    f.train()
    assert not _usable(f)
    f = NormalizingFlow("nsa", None, 4, 2, [128, 128], 2, 8, dropout_p=0.25, order="linear")
    f.train()
    assert not _usable(f)
    # conditioners with different p: not one common p
    f = NormalizingFlow("maf", None, 2, 2, [150] * 3, 2, dropout_p=0.25)
    f.train()
    f._plan._nets()[1].dropout_p = 0.5
    assert not _usable(f)
