"""Reference of the forward (sampling) direction of an nsa / maf flow with MC dropout: the oracle
flow (oracle.build_flow) with every layer's conditioner replaced by an MLP that multiplies given
masks in after every hidden activation (nn.Dropout's train-mode arithmetic with the mask fixed).
The masks are the ones the kernels apply, recovered by running naz_dropout on ones."""
import torch
import torch.nn.functional as F

from oracle import naz_oracle as O


class DropMLP(O.MLP):
    """O.MLP with ``drop[i]`` ([B, H_i], 0 or 1 / (1 - p)) multiplied into hidden activation i."""

    def __init__(self, base: O.MLP, drop):
        self.weights, self.biases, self.masks, self.f = base.weights, base.biases, base.masks, base.f
        self.drop = drop

    def __call__(self, x, context=None):
        if context is not None:
            context = context.expand(x.shape[:-1] + (context.shape[-1],))
            h = torch.cat([context, x], dim=-1)
        else:
            h = x
        n = len(self.weights)
        for i in range(n):
            W = self.weights[i] if self.masks is None else self.masks[i].to(self.weights[i].dtype) * self.weights[i]
            h = F.linear(h, W, self.biases[i])
            if i < n - 1:
                h = self.f(h) * self.drop[i].to(h.dtype)
        return h


def kernel_masks(seeds, p, B, H, row_offset=0, device="cuda"):
    """masks[l][i] = naz_dropout(ones[B, H], p, seeds[l][i]) on the CPU in float64 (0 or 1 / (1 - p)),
    for rows row_offset .. row_offset + B - 1 of the call."""
    from naz_amd import ops
    ones = torch.ones((row_offset + B, H), device=device)
    return [[ops.dropout(ones, p, int(sd))[row_offset:].double().cpu() for sd in layer] for layer in seeds]


def dropout_flow(spec, state, dtype, masks):
    """oracle.build_flow(spec, state, dtype) whose layer l's conditioner applies masks[l]."""
    flow = O.build_flow(spec, state, dtype)
    assert len(flow.layers) == len(masks)
    for layer, m in zip(flow.layers, masks):
        layer.nn = DropMLP(layer.nn, m)
    return flow
