"""A/B of the nsa NLL step: the fused spline backward (flows/maf_grad.py, NsaGrad) against the autograd walk
(NAZ_TRAIN_FUSED=0, the path before it existed), same process, same weights and rows, interleaved.

    python scripts/nsa_train_bench.py [--rows 262144 10752] [--layers 8] [--reps 3] [--iters 5]
                                      [--out profiles/nsa_train_bench.json]

Times ``loss = -flow.log_prob(x, c).mean(); loss.backward()`` of NormalizingFlow("nsa", D=4 | C=2,
H=[128,128], K=8) with HIP events after warm-up: per repetition the median of ``iters`` steps, the
two paths alternating repetition by repetition.  Writes one JSON record with every repetition and the
FP32-equivalent FLOPs the fused step executes per row (a split f16x3 / bf16x6 product counted once).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from naz_amd import ops  # noqa: E402
from naz_amd.flows import NormalizingFlow  # noqa: E402
from naz_amd.flows import flow as flow_mod  # noqa: E402

D, C, HID, K = 4, 2, [128, 128], 8


def fused_flop_per_row(L: int) -> dict:
    """FLOPs per row of the fused step: the saved-state inverse, the per-layer backward kernel (dense
    MADE pass, D chains with their masked k-steps skipped, W_outᵀ g on the VALU) and the dW reductions
    over the padded operands."""
    d = ops.ar_flow_desc("nsa", D, C, HID[0], L, len(HID), K)
    dm = ops.spline_ar_flow_bwd_dims(d)
    HP, X0W, GOW = dm["HP"], dm["X0W"], dm["GOW"]
    HB, KSH, P = HP // 16, HP // 32, 3 * K - 1
    deg = ops.ar_flow_degrees(d)
    blk = 16 * 32 * 2
    kts = [int(((deg <= deg[min(16 * b + 15, len(deg) - 1)]).sum() + 31) // 32) for b in range(HB)]
    kt0 = [int((deg < deg[min(16 * b, len(deg) - 1)]).sum()) >> 5 for b in range(HB)]
    dense = (HB * ((C + 31) // 32 + 1) + sum(kts) + (P + 3) // 4 * KSH) * blk
    chain = 2 * P * HP + sum(KSH - t for t in kt0) * blk
    bwd = dense + D * chain + (D - 1) * KSH * blk
    dw = 2 * (HP * X0W + HP * HP + GOW * HP)
    inv = ops.ar_executed_flop_per_row(d)["inverse"]
    return dict(inverse=int(inv), backward=int(bwd * L), dw=int(dw * L), total=int(inv + (bwd + dw) * L))


def step_ms(f, x, c, iters: int) -> float:
    ts = []
    for _ in range(iters):
        f.zero_grad(set_to_none=False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = -f.log_prob(x, condition=c).mean()
        loss.backward()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 18, 10752])
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/nsa_train_bench.json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    f = NormalizingFlow("nsa", None, D, C, list(HID), a.layers, K).to(dev)
    rec = dict(shape=dict(D=D, C=C, hidden=HID, K=K, L=a.layers), device=torch.cuda.get_device_name(0),
               iters=a.iters, warmup=a.warmup, flop_per_row=fused_flop_per_row(a.layers), rows={})
    for B in a.rows:
        g = torch.Generator().manual_seed(B)
        x = (1.5 * torch.randn(B, D, generator=g)).to(dev)
        c = torch.randn(B, C, generator=g).to(dev)
        runs = {"fused": [], "walk": []}
        for path, flag in (("fused", "1"), ("walk", "0")):
            flow_mod._TRAIN_FUSED = flag
            assert f._plan.train_ready(x, c) == (flag == "1")
            step_ms(f, x, c, a.warmup)
        for _ in range(a.reps):
            for path, flag in (("fused", "1"), ("walk", "0")):
                flow_mod._TRAIN_FUSED = flag
                runs[path].append(step_ms(f, x, c, a.iters))
        flow_mod._TRAIN_FUSED = "1"
        fm, wm = float(np.median(runs["fused"])), float(np.median(runs["walk"]))
        spread = max(max(v) - min(v) for v in runs.values())
        rec["rows"][str(B)] = dict(fused_ms=runs["fused"], walk_ms=runs["walk"], fused_median_ms=fm, walk_median_ms=wm,
                                   speedup=wm / fm, spread_ms=spread,
                                   fused_tflops=rec["flop_per_row"]["total"] * B / fm * 1e-9)
        print(f"B={B}: fused {runs['fused']} ms, walk {runs['walk']} ms, x{wm / fm:.2f}", flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
