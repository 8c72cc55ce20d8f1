"""GPU: the row-chunk loop of the fused maf / nsa NLL step (flows/maf_grad.py).  ``operand_bytes``
defaults to 4 GiB, where the chunk is the batch rounded down to the 128-row tile: no other test sets
it, so none runs more than one full chunk and a ragged rest.  Here a second grad object with
``operand_bytes=1`` runs the same step in chunks of one tile (300 rows: 128, 128 and a ragged 44)
against the default object (256 and 44): the context / g_lp slicing, the ragged last chunk, dW
accumulated across chunks, and the buffer dL/dx lands in at both parities of L."""
import numpy as np
import pytest
import torch

from oracle import naz_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 300


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from naz_amd import _lib
    _lib.lib()


def _flow(spec):
    from naz_amd.flows import NormalizingFlow
    from naz_amd.flows import io as fio
    state = {k: v.numpy() for k, v in O.random_state(spec, seed=23).items()}
    args = (spec["D"], spec["C"], list(spec["hidden"]), spec["L"]) + ((spec["K"],) if "K" in spec else ())
    f = NormalizingFlow(spec["flow_type"], None, *args)
    fio.load_state(f, state)
    return f.to(DEV)


@pytest.mark.parametrize("spec,ctx_form,weighted", [
    (dict(flow_type="nsa", D=4, C=2, hidden=[128, 128], L=3, K=8), "rows", True),
    (dict(flow_type="maf", D=2, C=2, hidden=[150] * 3, L=4), "one", False),
    (dict(flow_type="maf", D=2, C=0, hidden=[150] * 3, L=3), None, True),
], ids=["nsa-L3-ctx_rows-g_lp", "maf-L4-one_ctx", "maf_uncond-L3-g_lp"])
def test_chunked_step_matches_the_single_chunk_step(monkeypatch, spec, ctx_form, weighted):
    from naz_amd import ops
    from naz_amd.flows import flow as flow_mod
    monkeypatch.setattr(flow_mod, "_TRAIN_FUSED", "1")
    D, C = spec["D"], spec["C"]
    f = _flow(spec)
    plan = f._plan
    xh = O.gaussian_mixture(B, D, seed=4)
    if spec["flow_type"] == "nsa":
        outside = (np.abs(xh) > 3.0).any(1)
        assert 0 < outside.sum() < B
    x = torch.as_tensor(xh, device=DEV).float().contiguous()
    ctx = None
    if ctx_form is not None:
        ch = O.context_normal(B if ctx_form == "rows" else 1, C, seed=5)
        ctx = torch.as_tensor(ch, device=DEV).float().reshape(-1, C).contiguous()
        assert ctx.shape[0] == (B if ctx_form == "rows" else 1)
    assert f.fused and plan.train_ready(x, ctx)
    g_lp = None
    if weighted:
        g_lp = (0.25 + torch.rand(B, generator=torch.Generator().manual_seed(9))).to(DEV)

    mg = plan.maf_grad()
    assert type(mg).__name__ == ("NsaGrad" if spec["flow_type"] == "nsa" else "MafGrad")
    clip_zero = bool(mg.desc.flags & ops.AR_CLIP_ZERO_GRAD)
    chunked = type(mg)(mg.desc, mg.perms, mg.mask, operand_bytes=1, clip_zero=clip_zero)
    assert mg.dims["rows"] == 128
    flat = torch.cat([p.detach().reshape(-1) for p in plan.train_params()])

    out = {}
    for name, obj in (("whole", mg), ("chunked", chunked)):
        imgs = obj.images(flat)
        lp, states = obj.forward(imgs, x, ctx)
        lp, states = lp.clone(), states.clone()  # the buffers are reused
        grad, g_x = obj.backward(imgs, states, ctx, g_lp)
        out[name] = (lp, g_x.clone(), grad.clone())
        # the batched bf16x6 reduction had an instance for every width: no fp32 fallback was taken
        x6 = getattr(obj, "_x6", None)  # absent where the class has no fallback to take
        if x6 is not None:
            assert len(x6) > 0 and all(x6.values()), x6
    assert chunked._buffers(B)["chunk"] == 128 < B  # three chunks: 128, 128, 44

    (lp_a, gx_a, gr_a), (lp_b, gx_b, gr_b) = out["whole"], out["chunked"]
    assert torch.equal(lp_a, lp_b)
    # chunk edges are multiples of the 128-row tile: every workgroup sees the same rows
    assert bool(torch.isfinite(gx_a).all()) and torch.equal(gx_a, gx_b)
    for g in (gr_a, gr_b):
        assert bool(torch.isfinite(g).all()) and float(g.norm()) > 0.0
    # same terms, other summation order (test_fused_nsa_backward_rows_are_independent's bound)
    rel = float((gr_a - gr_b).norm() / gr_a.norm())
    print(f"d theta: chunked vs whole rel L2 {rel:.3e}")
    assert rel < 1e-5, rel
