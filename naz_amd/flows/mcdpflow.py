"""naz's Monte-Carlo-dropout flow (naz/flows/mcdpflow.py:29-56) on the HIP kernels.

``MCDPNormalizingFlow(flow_type, bounds, *args, dropout_p=p, ...)`` is a NormalizingFlow whose
conditioners carry dropout (naz_dropout after every hidden activation).  ``sample_uncertain``
draws ``niter`` sample sets with dropout active (train mode), each from fresh base draws and
fresh dropout masks, through the flow's forward (sampling) direction — one conditioner pass
per layer per set, as the reference's ``sample_uncached`` does (mcdpflow.py:12-25; its
non-compose branch applies every transform to the base draws instead of chaining them, a bug;
the chained forward of its compose branch is what runs here).  Returns numpy
[niter, *shape, D], as the reference does."""
from __future__ import annotations

import numpy as np
import torch

from .flow import NormalizingFlow

__all__ = ["MCDPNormalizingFlow"]


class MCDPNormalizingFlow(NormalizingFlow):
    """Normalizing flow with Monte-Carlo dropout in its conditioners (mcdpflow.py:29-37)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.flow_maker = args[0]
        assert kwargs.get("dropout_p") not in [None, 0.0], "MCDPNormalizingFlow needs dropout_p > 0"

    # rows (iterations x sample rows) per fused launch: z and y of one chunk are 2 x ROW_BUDGET x D
    # floats on the device (64 MB each at D = 4)
    ROW_BUDGET = 1 << 22

    def sample_uncertain(self, niter, *args, condition=None, **kwargs):
        """mcdpflow.py:39-56: ``niter`` stochastic forward passes in train mode.

        Where the fused dropout sampler applies (a maf / nsa flow at a compiled shape,
        naz_ar_flow_sample_dropout), the base draws and dropout seeds of a chunk of iterations are
        drawn at once and the chunk is ONE launch, then copied to the host; a chunk holds as many
        iterations as keep iterations x rows at or below ROW_BUDGET = 2^22 rows (at least one).
        Otherwise one sample() per iteration on the per-layer kernels."""
        self.train()
        pdf = self._pdf(condition)
        bounds = self._bounds_dev(self._base_loc)
        shape = args[0] if args else kwargs.get("sample_shape", ())
        niter = int(niter)
        rows = max(int(torch.Size(shape).numel()), 1)
        chunk = max(1, self.ROW_BUDGET // rows)
        out = []
        with torch.no_grad():
            while len(out) < niter:
                n = min(chunk, niter - len(out))
                ys = pdf.sample_dropout_draws(n, shape, bounds=bounds) if hasattr(pdf, "sample_dropout_draws") else None
                if ys is None:
                    out.append(pdf.sample(shape, bounds=bounds).cpu().numpy())
                else:
                    out.extend(ys.cpu().numpy())
        return np.array(out)
