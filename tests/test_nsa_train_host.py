"""CPU: the spline ("nsa") family of the fused autoregressive backward (include/naz_hip.h
naz_spline_ar_flow_*) — which descriptors have an instance, the operand widths, and the host-side
checks.  No GPU here: every call fails or returns before a launch."""
import ctypes


def _lib_ops():
    from naz_amd import _lib, ops
    return _lib.lib(), ops


def test_spline_bwd_packed_bytes_per_descriptor():
    L, ops = _lib_ops()
    one = int(L.naz_spline_ar_flow_bwd_packed_bytes(ops.ar_flow_desc("nsa", 4, 2, 128, 1, 2)))
    many = int(L.naz_spline_ar_flow_bwd_packed_bytes(ops.ar_flow_desc("nsa", 4, 2, 128, 16, 2)))
    assert one > 256
    assert many - 256 == 16 * (one - 256)  # a 256-byte header, then L equal layer images
    assert ops.spline_ar_flow_bwd_supported(ops.ar_flow_desc("nsa", 4, 2, 128, 8, 2))
    for bad in (ops.ar_flow_desc("nsa", 16, 32, 128, 4, 2), ops.ar_flow_desc("nsa", 8, 0, 128, 4, 2),
                ops.ar_flow_desc("nsa", 4, 2, 64, 4, 2), ops.ar_flow_desc("nsa", 4, 2, 128, 4, 2, K=6),
                ops.ar_flow_desc("maf", 4, 2, 150, 4, 3), ops.ar_flow_desc("maf", 2, 2, 150, 4, 3),
                ops.ar_flow_desc("maf", 4, 2, 512, 4, 5)):
        assert int(L.naz_spline_ar_flow_bwd_packed_bytes(bad)) < 0
        assert not ops.spline_ar_flow_bwd_supported(bad)
    # the affine family's answers are its own: no spline descriptor has an affine backward
    assert int(L.naz_ar_flow_bwd_packed_bytes(ops.ar_flow_desc("nsa", 4, 2, 128, 4, 2))) < 0


def test_spline_bwd_dims():
    L, ops = _lib_ops()
    d = ops.ar_flow_desc("nsa", 4, 2, 128, 3, 2)
    assert ops.spline_ar_flow_bwd_dims(d) == dict(n_hidden=2, HP=128, XA=128, XB=0, X0W=8, GOW=96, rows=128)
    assert L.naz_spline_ar_flow_bwd_dims(d, None) != 0 and b"null output" in L.naz_last_error()
    dims = (ctypes.c_int * 7)()
    rc = L.naz_spline_ar_flow_bwd_dims(ops.ar_flow_desc("nsa", 16, 32, 128, 3, 2), dims)
    assert rc != 0 and b"no fused backward" in L.naz_last_error()
    rc = L.naz_spline_ar_flow_bwd_dims(ops.ar_flow_desc("maf", 4, 2, 150, 3, 3), dims)
    assert rc != 0 and b"no fused backward" in L.naz_last_error()


def test_spline_bwd_layer_host_errors():
    L, ops = _lib_ops()
    d = ops.ar_flow_desc("nsa", 4, 2, 128, 4, 2)
    rc = L.naz_spline_ar_flow_bwd_layer(d, None, None, None, 0, None, None, None, 0, None, None, None, None, 128, None)
    assert rc != 0 and b"null pointer" in L.naz_last_error()
    bufs = (ctypes.c_void_p * 8)(*([16] * 8))
    # state_in (s_{l+1}) is required: the spline VJP is evaluated at the layer's input
    rc = L.naz_spline_ar_flow_bwd_layer(d, 16, 16, 16, 0, 16, None, 16, 2, 16, None, bufs, 16, 128, None)
    assert rc != 0 and b"null pointer" in L.naz_last_error()
    rc = L.naz_spline_ar_flow_bwd_layer(d, 16, 16, 16, 4, 16, 16, 16, 2, 16, None, bufs, 16, 128, None)  # layer == L
    assert rc != 0 and b"layer out of range" in L.naz_last_error()
    rc = L.naz_spline_ar_flow_bwd_layer(d, 16, 16, 16, 0, 16, 16, None, 0, 16, None, bufs, 16, 128, None)
    assert rc != 0 and b"needs ctx" in L.naz_last_error()
    rc = L.naz_spline_ar_flow_bwd_layer(d, 16, 16, 16, 0, 16, 16, 16, 2, 16, None, bufs, 16, -1, None)
    assert rc != 0 and b"negative batch" in L.naz_last_error()
    for bad in (ops.ar_flow_desc("nsa", 16, 32, 128, 4, 2), ops.ar_flow_desc("maf", 4, 2, 150, 4, 3)):
        rc = L.naz_spline_ar_flow_bwd_layer(bad, 16, 16, 16, 0, 16, 16, 16, 2, 16, None, bufs, 16, 128, None)
        assert rc != 0 and b"no fused backward" in L.naz_last_error()
    # 16 is no packed image: refused by the image registry before any launch
    rc = L.naz_spline_ar_flow_bwd_layer(d, 16, 16, 16, 0, 16, 16, 16, 2, 16, None, bufs, 16, 128, None)
    assert rc != 0 and b"not a packed image" in L.naz_last_error()
    assert L.naz_spline_ar_flow_bwd_layer(d, None, None, None, 0, None, None, None, 0, None, None, None, None, 0,
                                          None) == 0  # no rows: no launch


def test_spline_pack_bwd_and_train_forward_host_errors():
    L, ops = _lib_ops()
    d = ops.ar_flow_desc("nsa", 4, 2, 128, 4, 2)
    rc = L.naz_spline_ar_flow_pack_bwd(d, None, None, None, None)
    assert rc != 0 and b"null pointer" in L.naz_last_error()
    rc = L.naz_spline_ar_flow_pack_bwd(ops.ar_flow_desc("nsa", 8, 0, 128, 4, 2), 16, None, 16, None)
    assert rc != 0 and b"no fused backward" in L.naz_last_error()
    # the saved-state forward: a spline flow with a fused inverse; a maf descriptor belongs to the affine entry
    maf = ops.ar_flow_desc("maf", 4, 2, 150, 4, 3)
    rc = L.naz_spline_ar_flow_log_prob_train(maf, 16, 16, 4, 16, 2, 16, 16, 128, None)
    assert rc != 0 and b"no fused spline inverse" in L.naz_last_error()
    rc = L.naz_spline_ar_flow_log_prob_train(ops.ar_flow_desc("nsa", 5, 2, 128, 4, 2), 16, 16, 5, 16, 2, 16, 16, 128,
                                             None)
    assert rc != 0 and b"no fused spline inverse" in L.naz_last_error()
    rc = L.naz_spline_ar_flow_log_prob_train(d, 16, 16, 4, 16, 2, 16, None, 128, None)  # states
    assert rc != 0 and b"null pointer" in L.naz_last_error()
    rc = L.naz_spline_ar_flow_log_prob_train(d, 16, 16, 4, None, 0, 16, 16, 128, None)
    assert rc != 0 and b"needs ctx" in L.naz_last_error()
    rc = L.naz_spline_ar_flow_log_prob_train(d, 16, 16, 4, 16, 2, 16, 16, 128, None)
    assert rc != 0 and b"not a packed image" in L.naz_last_error()
    assert L.naz_spline_ar_flow_log_prob_train(d, None, None, 4, None, 2, None, None, 0, None) == 0  # no rows
    # every fused nsa shape has the saved-state forward, with or without a fused backward
    wide = ops.ar_flow_desc("nsa", 16, 32, 128, 4, 2)
    assert L.naz_spline_ar_flow_log_prob_train(wide, None, None, 16, None, 32, None, None, 0, None) == 0


def test_plan_reports_the_spline_backward():
    """NormalizingFlow's fused plan: the nsa NLL step has its kernels at naz's own nsa shape only."""
    from naz_amd.flows import NormalizingFlow
    f = NormalizingFlow("nsa", None, 4, 2, [128, 128], 3, 8)
    assert f._plan is not None and f._plan.kind == "nsa" and f._plan._train_kernels()
    for args, kw in (((4, 2, [64, 64], 3, 8), {}), ((16, 32, [128, 128], 3, 8), {}),
                     ((4, 2, [128, 128], 3, 8), dict(order="linear"))):
        g = NormalizingFlow("nsa", None, *args, **kw)
        assert g._plan is None or not g._plan._train_kernels()
    # the maf plans keep their answers
    m = NormalizingFlow("maf", None, 2, 2, [150] * 3, 2)
    assert m._plan is not None and m._plan._train_kernels()
