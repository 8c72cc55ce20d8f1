"""CPU: the host side of the fused autoregressive kernels at the unconditional paper maf (D=2 | C=0,
H=[150]x3: naz examples/papers/2506.05657/train_mle_unsupervised.py) — which descriptors are
instantiated, the fused-plan decisions, the host packer's image (whose pass-1 hidden sub-layers are
cut over two ring stages each), the image sizes of every shape that was there before, and the
register / scratch budget of the new kernel instances against the D=2 | C=2 ones."""
import numpy as np
import pytest

from naz_amd import ops
from tests.isa_ring import code_objects
from tests.test_r16_resources import LIB, kernel_metadata

D, H, NH = 2, 150, 3


def _desc(L=1, D_=D, C=0, H_=H, nh=NH):
    return ops.ar_flow_desc("maf", D_, C, H_, L, nh)


def test_supported_shape_answers():
    d = _desc(3)
    assert ops.ar_flow_supported(d) == 1
    assert ops.ar_flow_fwd_supported(d) and ops.ar_flow_bwd_supported(d)
    assert ops.ar_flow_sample_dropout_supported(d)
    assert ops.ar_flow_pass0_floats(d) < 0
    dm = ops.ar_flow_bwd_dims(d)
    assert (dm["n_hidden"], dm["HP"], dm["XB"], dm["X0W"]) == (3, 160, 0, 8)
    for bad in (_desc(3, H_=64), _desc(3, D_=3), _desc(3, nh=2)):
        assert not ops.ar_flow_supported(bad) and not ops.ar_flow_fwd_supported(bad)
        assert not ops.ar_flow_bwd_supported(bad) and not ops.ar_flow_sample_dropout_supported(bad)
        assert ops.ar_flow_pass0_floats(bad) < 0


@pytest.mark.parametrize("bounds", [None, {"low": np.array([-2.0, 0.5], np.float32),
                                           "high": np.array([3.0, 7.5], np.float32)}], ids=["free", "bounds"])
def test_fused_plan_decisions(bounds, monkeypatch):
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows.flow import _FusedAR
    from naz_amd.flows.mcdpflow import MCDPNormalizingFlow
    f = NormalizingFlow("maf", bounds, 2, 0, [150, 150, 150], 10)
    assert f.fused and isinstance(f._plan, _FusedAR) and f._plan.kind == "maf" and f._plan.inverse == 1
    assert f._plan.masks_ok() and f._plan._train_kernels()
    assert f._plan.dropout_p() is None and not f._plan.dropout_sample_usable()
    f.set_fused(False)
    assert not f.fused
    f.set_fused(True)
    assert f.fused
    for cls in (NormalizingFlow, MCDPNormalizingFlow):
        g = cls("maf", bounds, 2, 0, [150, 150, 150], 3, dropout_p=0.2)
        g.train()
        assert g.fused and g._plan.dropout_sample_usable()
        monkeypatch.setenv("NAZ_AR_DROPOUT_FUSED", "0")
        assert not g._plan.dropout_sample_usable()
        monkeypatch.delenv("NAZ_AR_DROPOUT_FUSED")
        g.eval()
        assert not g._plan.dropout_sample_usable()
    # a random permutation puts Permute layers between the transforms: not fused; nor other shapes
    assert not NormalizingFlow("maf", bounds, 2, 0, [150, 150, 150], 3, random_perm=True).fused
    assert not NormalizingFlow("maf", bounds, 2, 0, [64, 64, 64], 3).fused
    assert not NormalizingFlow("maf", bounds, 3, 0, [150, 150, 150], 3).fused
    assert not NormalizingFlow("maf", bounds, 2, 0, [150, 150], 3).fused


def _sizes():
    return [H * D, H, H * H, H, H * H, H, 2 * D * H, 2 * D]  # W0, b0, W1, b1, W2, b2, W_out, b_out


def _pack(d, flat, perm):
    nbytes = int(ops.lib().naz_ar_flow_packed_bytes(d))
    host = np.empty(nbytes // 4, dtype=np.float32)
    ops.check(ops.lib().naz_ar_flow_pack_host(d, np.ascontiguousarray(flat).ctypes.data, perm.ctypes.data,
                                              host.ctypes.data), "pack")
    return host.view(np.uint32), nbytes


def _masks(perm):
    """The MADE masks of one layer in the flat layout (1 on biases): every hidden unit has degree 1."""
    order = np.empty(D, dtype=np.int64)
    order[perm] = np.arange(D)
    m0 = (1 >= (order + 1))[None, :].repeat(H, 0)
    mo = (np.tile(order + 1, 2) > 1)[:, None].repeat(H, 1)
    parts = [m0, np.ones(H), np.ones((H, H)), np.ones(H), np.ones((H, H)), np.ones(H), mo, np.ones(2 * D)]
    return np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in parts])


def test_host_pack():
    L = 3
    d = _desc(L)
    deg = ops.ar_flow_degrees(d)
    assert deg.shape == (H,) and (deg == 1).all()
    rng = np.random.default_rng(0)
    sizes = _sizes()
    per = sum(sizes)
    perm = np.array([[0, 1], [1, 0], [0, 1]], dtype=np.int32)
    mask = np.concatenate([_masks(p) for p in perm])
    flat = (rng.standard_normal(L * per).astype(np.float32) * 0.1 + np.float32(0.5)) * mask
    img, nbytes = _pack(d, flat, perm)
    # the 256-byte image header (include/naz_hip.h "Packed images"), as tests/test_ar_pack.py reads it
    hdr = img[:64]
    assert hdr[0] == 0x495A414E and hdr[2] == 3 and hdr[4] == L and hdr[5] == 0
    assert int(hdr[6]) | (int(hdr[7]) << 32) == nbytes - 256 and not hdr[8:].any()
    assert hdr[3] != _pack(ops.ar_flow_desc("maf", 2, 2, H, L, NH), np.zeros(L * (per + 2 * H), np.float32), perm)[0][3]
    assert (nbytes - 256) % L == 0  # body == L x layer
    layer = (nbytes - 256) // 4 // L
    # one 1 KB stage for pass 0 (the first dim's two biases), four for pass 1, in slots of the
    # largest (hidden layer 1 + half of hidden layer 2 = 5280 + 12880 floats, padded), + the perm row
    slot = (5280 + 12880 + 255) // 256 * 256
    assert layer == 5 * slot + 256
    assert np.array_equal(img, _pack(d, flat, perm)[0])  # bitwise stable
    body = img[64:].reshape(L, layer)
    for l in range(L):
        assert body[l, 5 * slot:5 * slot + D].tolist() == perm[l].tolist()
        # pass 0: nothing but the (mean, log_scale) biases of the dim of order 0
        bo = l * per + sum(sizes[:7])
        p0 = body[l, :slot].view(np.float32)
        assert p0[0] == flat[bo + perm[l, 0]] and p0[1] == flat[bo + D + perm[l, 0]] and not p0[2:].any()
    # each of the eight natural blocks reaches the image ...
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for k in range(8):
        pert = flat.copy()
        for l in range(L):
            sl = slice(l * per + offs[k], l * per + offs[k + 1])
            pert[sl] += np.float32(0.25) * mask[sl]
        assert not np.array_equal(img, _pack(d, pert, perm)[0]), f"block {k} does not reach the image"
    # ... and a masked-out weight does not: the packer reads rows with the masks applied, which is
    # what the plan hands it (weight * mask), whatever the masked entries of the parameter hold
    assert (mask == 0).sum() == L * (H + 2 * H)
    import torch
    from naz_amd.flows import NormalizingFlow
    f = NormalizingFlow("maf", None, D, 0, [H] * NH, L)
    plan = f._plan
    fperm = np.stack([n.permutation.detach().cpu().numpy() for n in plan._nets()]).astype(np.int32)
    before = _pack(d, plan._flat().astype(np.float32), fperm)[0]
    with torch.no_grad():
        for n in plan._nets():
            for layer in n.layers:
                layer.weight[layer.mask == 0] *= 7.0  # (the sign stays: w * 0 is a signed zero in the image)
    assert np.array_equal(before, _pack(d, plan._flat().astype(np.float32), fperm)[0])
    assert np.array_equal(np.concatenate([_masks(p) for p in fperm]) != 0, plan._flat() != 0)
    # the forward (sample) image and the backward image exist with whole-layer sizes
    assert int(ops.lib().naz_ar_flow_fwd_packed_bytes(d)) > 256
    assert int(ops.lib().naz_ar_flow_bwd_packed_bytes(d)) > 0


# (kind, D, C, H, n_hidden): naz_ar_flow_packed_bytes, naz_ar_flow_fwd_packed_bytes and
# naz_ar_flow_bwd_packed_bytes at L = 1, recorded from a build of the commit before the layout cut
BEFORE = {
    ("nsa", 16, 32, 128, 2): (673024, 394496, -1),
    ("nsa", 16, 0, 128, 2): (607488, 302336, -1),
    ("nsa", 8, 0, 128, 2): (304384, 181504, -1),
    ("nsa", 4, 2, 128, 2): (218368, 162048, -1),
    ("nsa_linear", 8, 0, 128, 2): (304384, 199936, -1),
    ("nsa_linear", 4, 2, 128, 2): (218368, 162048, -1),
    ("maf", 2, 2, 150, 3): (364800, 230656, 246016),
    ("maf", 4, 2, 150, 3): (449792, 236800, 246016),
    ("maf", 16, 32, 128, 2): (541952, 157952, -1),
    ("maf", 4, 2, 512, 5): (4261120, 3721472, -1),
}
PASS0_BEFORE = {("nsa", 16, 32): 64, ("nsa", 16, 0): 32, ("nsa", 8, 0): 32, ("nsa", 4, 2): 96, ("nsa_linear", 8, 0): -1,
                ("nsa_linear", 4, 2): -1, ("maf", 2, 2): 256, ("maf", 4, 2): 112, ("maf", 16, 32): 48, ("maf", 4, 2, 512): -1}


@pytest.mark.parametrize("shape", sorted(BEFORE), ids=lambda s: "-".join(map(str, s)))
def test_existing_shapes_keep_their_packed_bytes(shape):
    kind, D_, C, H_, nh = shape
    L = ops.lib()
    d = ops.ar_flow_desc(kind, D_, C, H_, 1, nh)
    got = (int(L.naz_ar_flow_packed_bytes(d)), int(L.naz_ar_flow_fwd_packed_bytes(d)),
           int(L.naz_ar_flow_bwd_packed_bytes(d)))
    assert got == BEFORE[shape]
    key = (kind, D_, C) + ((H_,) if H_ == 512 else ())
    assert ops.ar_flow_pass0_floats(d) == PASS0_BEFORE[key]
    d3 = ops.ar_flow_desc(kind, D_, C, H_, 3, nh)  # (the 256-byte header once, the body per layer)
    assert int(L.naz_ar_flow_packed_bytes(d3)) - 256 == 3 * (got[0] - 256)


def _vgpr_class(n):
    """Waves per SIMD a VGPR count allows, among those these kernels are built for (their LDS ring
    leaves one workgroup per CU): the launch bounds' 168, 256 and 512 registers."""
    return next(w for w, lim in ((3, 168), (2, 256), (1, 512)) if n <= lim)


KERNELS = ["made_ar_r16_kernel", "made_ar_fwd_kernel", "made_ar_bwd_kernel", "made_ar_fwd_drop_kernel"]


@pytest.fixture(scope="module")
def metadata():
    if not LIB.exists():
        from naz_amd import build
        build.build()
    md = {}
    for co in code_objects(LIB):
        md.update(kernel_metadata(co))
    return md


@pytest.mark.parametrize("kernel", KERNELS)
def test_new_instances_keep_the_conditional_siblings_budget(kernel, metadata):
    new_cfg, old_cfg = "5CfgARILi2ELi0ELi150ELi8ELi3ELb1EE", "5CfgARILi2ELi2ELi150ELi8ELi3ELb1EE"  # CfgAR<2, C, 150, 8, 3, true>
    pre = f"_ZN3naz{len(kernel)}{kernel}I"
    new = [m for n, m in metadata.items() if n.startswith(pre) and new_cfg in n]
    old = [m for n, m in metadata.items() if n.startswith(pre) and old_cfg in n]
    assert len(new) == 1 and len(old) == 1, f"{kernel}: {len(new)} new and {len(old)} sibling records"
    new, old = new[0], old[0]
    print(kernel, {k: (new[k], old[k]) for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size")})
    assert int(new["private_segment_fixed_size"]) == 0, new
    assert _vgpr_class(int(new["vgpr_count"])) >= _vgpr_class(int(old["vgpr_count"])), (new, old)
