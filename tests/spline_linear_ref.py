"""Reference restatement of pyro's rational-LINEAR spline (``_monotonic_rational_spline`` with
``lambdas``, i.e. order="linear") and of the nsa / nsc flows built on it.  Helper for
tests/test_spline_linear_host.py and tests/test_gpu_spline_linear.py, not a test module.

Everything up to the bin selection is oracle/naz_oracle.py::monotonic_rqs (constants,
_calculate_knots, the +1e-6 search, the clamped bin index, the padded derivatives, the identity
tails).  On the selected bin, with λ = (1 − 2·0.025)·sigmoid(u) + 0.025:
    wa = 1, wb = sqrt(d0/d1), wc = (λ·wa·d0 + (1−λ)·wb·d1)/δ,
    yc = ((1−λ)·wa·ya + λ·wb·yb) / ((1−λ)·wa + λ·wb)
and the two rational-linear pieces of pyro's literal num/den form.  pyro multiplies the pieces by
``(cond).float()``; here they are selected (torch.where), and the bin arithmetic runs on the input
clamped into the box so that autograd through the unselected tail stays finite.
"""
import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import naz_oracle as O

MIN_LAMBDA = 0.025
LAYOUT_DENSE, LAYOUT_ARN = O.LAYOUT_DENSE, O.LAYOUT_ARN


def monotonic_rls(inputs, widths, heights, derivatives, lambdas, inverse=False, bound=O.DEFAULT_BOUND):
    """inputs [..., Dt]; widths / heights [..., Dt, K] softmaxed; derivatives [..., Dt, K-1]
    softplus'ed; lambdas [..., Dt, K] sigmoid'ed.  Returns (outputs, logabsdet of the map applied)."""
    K = widths.shape[-1]
    outside = ~((inputs >= -bound) & (inputs <= bound))
    v = inputs.clamp(-bound, bound)

    widths = O.MIN_BIN_WIDTH + (1.0 - O.MIN_BIN_WIDTH * K) * widths
    heights = O.MIN_BIN_HEIGHT + (1.0 - O.MIN_BIN_HEIGHT * K) * heights
    derivatives = O.MIN_DERIVATIVE + derivatives
    widths, cumwidths = O._calculate_knots(widths, -bound, bound)
    heights, cumheights = O._calculate_knots(heights, -bound, bound)
    derivatives = F.pad(derivatives, pad=(1, 1), mode="constant", value=1.0 - O.MIN_DERIVATIVE)

    idx = O._searchsorted((cumheights if inverse else cumwidths) + O.SEARCH_EPS, v).unsqueeze(-1)
    W = O._select_bins(widths, idx)
    xk = O._select_bins(cumwidths, idx)
    ya = O._select_bins(cumheights, idx)
    H = O._select_bins(heights, idx)
    delta = O._select_bins(heights / widths, idx)
    d0 = O._select_bins(derivatives, idx)
    d1 = O._select_bins(derivatives[..., 1:], idx)
    lam = (1 - 2 * MIN_LAMBDA) * O._select_bins(lambdas, idx) + MIN_LAMBDA
    yb = ya + H

    wa = 1.0
    wb = torch.sqrt(d0 / d1) * wa
    wc = (lam * wa * d0 + (1 - lam) * wb * d1) / delta
    yc = ((1 - lam) * wa * ya + lam * wb * yb) / ((1 - lam) * wa + lam * wb)

    if inverse:
        left = v <= yc
        num = torch.where(left, lam * wa * (ya - v), (wc - lam * wb) * v + lam * wb * yb - wc * yc)
        den = torch.where(left, (wc - wa) * v + wa * ya - wc * yc, (wc - wb) * v + wb * yb - wc * yc)
        dnum = torch.where(left, wa * wc * lam * (yc - ya) * W, wb * wc * (1 - lam) * (yb - yc) * W)
        outputs = num / den * W + xk
    else:
        theta = (v - xk) / W
        left = theta <= lam
        num = torch.where(left, wa * ya * (lam - theta) + wc * yc * theta,
                          wc * yc * (1 - theta) + wb * yb * (theta - lam))
        den = torch.where(left, wa * (lam - theta) + wc * theta, wc * (1 - theta) + wb * (theta - lam))
        dnum = torch.where(left, wa * wc * lam * (yc - ya) / W, wb * wc * (1 - lam) * (yb - yc) / W)
        outputs = num / den
    logabsdet = torch.log(dnum) - 2 * torch.log(torch.abs(den))
    return torch.where(outside, inputs, outputs), torch.where(outside, torch.zeros_like(logabsdet), logabsdet)


def split_raw_params4(raw, Dt, K, layout):
    """raw [..., Dt*(4K-1)] -> unnormalised (w, h, d, l), pyro's param_dims order [K, K, K-1, K]."""
    lead = raw.shape[:-1]
    if layout == LAYOUT_DENSE:
        o = [0, Dt * K, 2 * Dt * K, Dt * (3 * K - 1), Dt * (4 * K - 1)]
        return tuple(raw[..., o[j]:o[j + 1]].reshape(lead + (Dt, n)) for j, n in enumerate((K, K, K - 1, K)))
    r = raw.reshape(lead + (4 * K - 1, Dt))
    o = [0, K, 2 * K, 3 * K - 1, 4 * K - 1]
    return tuple(r[..., o[j]:o[j + 1], :].transpose(-1, -2) for j in range(4))


def normalize4(w, h, d, l):
    return F.softmax(w, dim=-1), F.softmax(h, dim=-1), F.softplus(d), torch.sigmoid(l)


def rls_from_raw(x, raw, Dt, K, layout, inverse, bound=O.DEFAULT_BOUND):
    """The standalone primitive naz_rls_fwd / naz_rls_inv replace: (y, ld of the map applied)."""
    return monotonic_rls(x, *normalize4(*split_raw_params4(raw, Dt, K, layout)), inverse=inverse, bound=bound)


class SplineCouplingLinear(O.SplineCoupling):
    """O.SplineCoupling with the 4-block hypernet output and a 4-tuple lower spline."""

    def _upper(self, v2, x1, ctx, inverse):
        return rls_from_raw(v2, self.nn(x1, ctx), self.D - self.s, self.K, LAYOUT_DENSE, inverse, self.bound)

    def _lower(self, v1, inverse):
        return monotonic_rls(v1, *normalize4(*self.lower), inverse=inverse, bound=self.bound)

    def forward(self, x, ctx=None):
        x1, x2 = x[..., : self.s], x[..., self.s:]
        y1, ldk = self._lower(x1, False) if self.lower is not None else (x1, None)
        y2, ld = self._upper(x2, x1, ctx, False)
        if ldk is not None:
            ld = torch.cat([ld, ldk], dim=-1)
        return torch.cat([y1, y2], dim=-1), ld

    def inverse(self, y, ctx=None):
        y1, y2 = y[..., : self.s], y[..., self.s:]
        x1, ldk = self._lower(y1, True) if self.lower is not None else (y1, None)
        x2, ld = self._upper(y2, x1, ctx, True)
        ld = -ld
        if ldk is not None:
            ld = torch.cat([ld, -ldk], dim=-1)
        return torch.cat([x1, x2], dim=-1), ld


class SplineAutoregressiveLinear(O.SplineAutoregressive):
    def _apply(self, v, x, ctx, inverse):
        return rls_from_raw(v, self.nn(x, ctx), self.D, self.K, LAYOUT_ARN, inverse, self.bound)

    def forward(self, x, ctx=None):
        return self._apply(x, x, ctx, False)

    def inverse(self, y, ctx=None):
        x = torch.zeros_like(y)
        ld = None
        for _ in range(self.D):
            x, ld = self._apply(y, x, ctx, True)
        return x, -ld


_LOWER = ("widths", "heights", "derivatives", "lambdas")


def build_flow(spec: dict, state: Dict[str, torch.Tensor], dtype=torch.float64) -> O.Flow:
    """O.build_flow for an order="linear" nsa / nsc flow (canonical state plus
    ``lower_spline.unnormalized_lambdas``)."""
    t = {k: torch.as_tensor(v) for k, v in state.items()}
    ft, D, C, K = spec["flow_type"], spec["D"], spec["C"], spec["K"]
    hidden = list(spec["hidden"])
    layers = []
    for l in range(spec["L"]):
        p = f"layers.{l}."
        Ws = [t[p + f"nn.layers.{i}.weight"].to(dtype) for i in range(len(hidden) + 1)]
        bs = [t[p + f"nn.layers.{i}.bias"].to(dtype) for i in range(len(hidden) + 1)]
        if ft == "nsc":
            lower = None
            if (p + "lower_spline.unnormalized_widths") in t:
                lower = tuple(t[p + "lower_spline.unnormalized_" + n].to(dtype) for n in _LOWER)
            layers.append(SplineCouplingLinear(D, spec["split"], K, O.MLP(Ws, bs, "tanh"), lower))
        else:
            masks, _ = O.create_mask(D, C, hidden, t[p + "nn.permutation"].long(), 4 * K - 1)
            layers.append(SplineAutoregressiveLinear(D, K, O.MLP(Ws, bs, "tanh", masks=[m.to(dtype) for m in masks])))
    bounds = None
    if spec.get("bounds") is not None:
        bounds = {k: torch.as_tensor(v).to(dtype) for k, v in spec["bounds"].items()}
    return O.Flow(layers, D, bounds)


def random_state(spec: dict, seed: int = 1234, last_layer_scale: float = 3.0) -> Dict[str, torch.Tensor]:
    """O.random_state with the wider last layer (4K-1 per transformed dim) and the lower
    spline's lambdas ~ U(0, 1) (pyro's Spline init)."""
    g = torch.Generator().manual_seed(seed)
    ft, D, C, K = spec["flow_type"], spec["D"], spec["C"], spec["K"]
    hidden = list(spec["hidden"])
    out = {}
    for l in range(spec["L"]):
        p = f"layers.{l}."
        s = spec.get("split", 0)
        dims = ([s + C] + hidden + [(D - s) * (4 * K - 1)]) if ft == "nsc" else ([D + C] + hidden + [D * (4 * K - 1)])
        for i in range(len(dims) - 1):
            bnd = 1.0 / math.sqrt(dims[i])
            scale = last_layer_scale if i == len(dims) - 2 else 1.0
            out[p + f"nn.layers.{i}.weight"] = (torch.rand(dims[i + 1], dims[i], generator=g) * 2 - 1) * bnd * scale
            out[p + f"nn.layers.{i}.bias"] = (torch.rand(dims[i + 1], generator=g) * 2 - 1) * bnd * scale
        if ft == "nsc" and spec.get("lower", True):
            out[p + "lower_spline.unnormalized_widths"] = torch.randn(s, K, generator=g)
            out[p + "lower_spline.unnormalized_heights"] = torch.randn(s, K, generator=g)
            out[p + "lower_spline.unnormalized_derivatives"] = torch.randn(s, K - 1, generator=g)
            out[p + "lower_spline.unnormalized_lambdas"] = torch.rand(s, K, generator=g)
        if ft == "nsa":
            out[p + "nn.permutation"] = torch.randperm(D, generator=g)
    return out
