"""CPU: the host side of the fused autoregressive kernels for order="linear" nsa flows (kind
"nsa_linear" = NAZ_AR_SPLINE_LINEAR): which shapes are instantiated, the fused-plan decision, the
host packer's image (header, the λ rows, size), and the register / scratch budget of the new kernel
instances against the quadratic instances of the same shape and direction."""
import numpy as np
import pytest

from naz_amd import ops
from tests.isa_ring import code_objects
from tests.test_r16_resources import LIB, kernel_metadata

K = 8
SHAPES = [(4, 2), (8, 0)]


def test_supported_shapes():
    for D, C in SHAPES:
        assert ops.ar_flow_supported(ops.ar_flow_desc("nsa_linear", D, C, 128, 1))
    for bad in (ops.ar_flow_desc("nsa_linear", 16, 32, 128, 1), ops.ar_flow_desc("nsa_linear", 16, 0, 128, 1),
                ops.ar_flow_desc("nsa_linear", 4, 2, 128, 1, K=5), ops.ar_flow_desc("nsa_linear", 4, 2, 64, 1),
                ops.ar_flow_desc("nsa_linear", 4, 2, 128, 1, n_hidden=3)):
        assert not ops.ar_flow_supported(bad) and not ops.ar_flow_fwd_supported(bad)


def test_no_fused_backward_no_pass0_form_and_the_abi_stays():
    for D, C in SHAPES:
        d = ops.ar_flow_desc("nsa_linear", D, C, 128, 2)
        assert not ops.spline_ar_flow_bwd_supported(d)
        assert not ops.ar_flow_bwd_supported(d)
        assert ops.ar_flow_pass0_floats(d) < 0
    assert ops.spline_ar_flow_bwd_supported(ops.ar_flow_desc("nsa", 4, 2, 128, 2))
    assert int(ops.lib().naz_abi_version()) == 3


def test_fused_plan_decision():
    from naz_amd.flows import NormalizingFlow
    f = NormalizingFlow("nsa", None, 4, 2, [128, 128], 2, 8, order="linear")
    assert f.fused and f._plan.kind == "nsa_linear" and f._plan.P == 4 * K - 1
    assert f._plan.desc.kind == ops.AR_KIND["nsa_linear"]
    f.set_fused(False)
    assert not f.fused
    f.set_fused(True)
    assert f.fused
    assert NormalizingFlow("nsa", None, 8, 0, [128, 128], 2, 8, order="linear").fused
    assert not NormalizingFlow("nsa", None, 4, 2, [128, 128], 2, 8, order="linear", random_perm=True).fused
    assert not NormalizingFlow("nsa", None, 4, 2, [128, 128], 2, 5, order="linear").fused
    assert not NormalizingFlow("nsc", None, 4, 2, [128, 128], 2, 8, 2, order="linear").fused
    # the quadratic flow of the same shape keeps its own kind
    q = NormalizingFlow("nsa", None, 4, 2, [128, 128], 2, 8)
    assert q.fused and q._plan.kind == "nsa" and q._plan.P == 3 * K - 1


def _sizes(D, C, P, H=128):
    return [H * (C + D), H, H * H, H, D * P * H, D * P]


def _pack(d, flat, perm):
    nbytes = int(ops.lib().naz_ar_flow_packed_bytes(d))
    host = np.empty(nbytes // 4, dtype=np.float32)
    ops.check(ops.lib().naz_ar_flow_pack_host(d, np.ascontiguousarray(flat).ctypes.data, perm.ctypes.data,
                                              host.ctypes.data), "pack")
    return host.view(np.uint32), nbytes


@pytest.mark.parametrize("D,C", SHAPES)
def test_host_pack_of_the_linear_kind(D, C):
    L, H, P = 3, 128, 4 * K - 1
    d = ops.ar_flow_desc("nsa_linear", D, C, H, L)
    dq = ops.ar_flow_desc("nsa", D, C, H, L)
    rng = np.random.default_rng(0)
    sizes = _sizes(D, C, P)
    per = sum(sizes)
    flat = rng.standard_normal(L * per).astype(np.float32) * 0.1
    perm = np.stack([rng.permutation(D) for _ in range(L)]).astype(np.int32)
    img, nbytes = _pack(d, flat, perm)
    # the 256-byte image header (include/naz_hip.h "Packed images"), as tests/test_ar_pack.py reads it
    hdr = img[:64]
    assert hdr[0] == 0x495A414E and hdr[2] == 3 and hdr[4] == L and hdr[5] == 0
    assert int(hdr[6]) | (int(hdr[7]) << 32) == nbytes - 256 and not hdr[8:].any()
    # two output blocks per dim for either order: the same image size, another layout tag
    assert nbytes == int(ops.lib().naz_ar_flow_packed_bytes(dq))
    flat_q = rng.standard_normal(L * sum(_sizes(D, C, 3 * K - 1))).astype(np.float32) * 0.1
    assert _pack(dq, flat_q, perm)[0][3] != hdr[3]
    # bitwise stable
    assert np.array_equal(img, _pack(d, flat, perm)[0])
    # the λ rows of W_out (ARN rows pi D + i, pi >= 3K - 1) reach the image ...
    wout = sum(sizes[:4])
    pert = flat.copy()
    for layer in range(L):
        o = layer * per + wout + (3 * K - 1) * D * H
        pert[o:layer * per + wout + D * P * H] += 0.25
    assert not np.array_equal(img, _pack(d, pert, perm)[0])
    # ... and each λ bias lands in exactly one word: K per dim and layer (pass p holds dim perm[p]'s)
    pert = flat.copy()
    for layer in range(L):
        o = layer * per + wout + D * P * H
        pert[o + (3 * K - 1) * D:o + D * P] += 0.25
    changed = np.flatnonzero(img != _pack(d, pert, perm)[0])
    assert changed.size == L * D * K
    # the λ of one dim are 8 consecutive words, 24 words after the dim's first bias word (rows 0-22
    # hold widths, heights and slopes, row 23 stays zero)
    runs = changed.reshape(L * D, K)
    assert (np.diff(runs, axis=1) == 1).all()
    body = img[64:].view(np.float32)
    for run in runs:
        first = run[0] - 64 - 24
        assert body[first + 23] == 0.0 and np.count_nonzero(body[first:first + 23]) == 23


def _instances(kernel):
    """{(D, C): (linear metadata, quadratic metadata)} of one kernel template's nsa instances."""
    if not LIB.exists():
        from naz_amd import build
        build.build()
    found = {}
    for co in code_objects(LIB):
        for name, md in kernel_metadata(co).items():
            if kernel not in name:
                continue
            for D, C in SHAPES:
                quad = f"5CfgARILi{D}ELi{C}ELi128ELi8ELi2ELb0EEE"  # CfgAR<D, C, 128, 8, 2, false>
                if "8CfgARLinINS_" + quad in name:
                    found.setdefault((D, C), {})["lin"] = md
                elif quad in name:
                    found.setdefault((D, C), {})["quad"] = md
    return found


def _vgpr_class(n):
    """Waves per SIMD a VGPR count allows, among those these kernels are built for: their LDS ring
    leaves one workgroup per CU, so a SIMD holds the workgroup's 3, 2 or 1 waves and the budgets
    are the launch bounds' 168, 256 and 512 registers."""
    return next(w for w, lim in ((3, 168), (2, 256), (1, 512)) if n <= lim)


@pytest.mark.parametrize("kernel", ["made_ar_r16_kernel", "made_ar_fwd_kernel"])
def test_linear_instances_keep_the_quadratic_budget(kernel):
    found = _instances(kernel)
    assert sorted(found) == sorted(SHAPES), f"{kernel}: instances found for {sorted(found)}"
    for shape, md in found.items():
        lin, quad = md["lin"], md["quad"]
        print(kernel, shape, {k: (lin[k], quad[k]) for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size")})
        assert int(lin["private_segment_fixed_size"]) <= int(quad["private_segment_fixed_size"]), (shape, lin)
        assert _vgpr_class(int(lin["vgpr_count"])) >= _vgpr_class(int(quad["vgpr_count"])), (shape, lin, quad)
