"""A/B/C of sampling with MC dropout active: the fused dropout sampler (naz_ar_flow_sample_dropout,
csrc/made_ar_dropout.h) against the per-layer path of the same flow (NAZ_AR_DROPOUT_FUSED=0: one
naz_linear_act + one naz_dropout launch per hidden layer per flow layer, then the maps) and against
the fused sampler without dropout (the same flow in eval mode), same process, same rows, interleaved.

    python scripts/mcdp_sample_bench.py [--rows 262144 10752] [--reps 3] [--iters 20]
                                        [--out profiles/mcdp_sample_bench.json]

Times ``flow._pdf(c)._transform_z(z)`` (sample without the draw of z; the dropout seeds are drawn
inside, as in production) with p = 0.25 for maf D=2|C=2 H=[150]x3 L=16 and nsa D=4|C=2 H=[128,128]
K=8 L=8, with HIP events after warm-up: per repetition the median of ``iters`` calls, the three
paths alternating repetition by repetition.  Then the wall time of
``MCDPNormalizingFlow.sample_uncertain(16, [65536])`` (host copies included; median of
``wall_iters`` calls per repetition), fused against per-layer.  Writes one JSON record with every
repetition; ``beats_per_layer`` = the per-layer median minus the fused median exceeds the largest
spread between repetitions of either; ``dropout_over_plain`` is the price of the hash.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from naz_amd.flows.mcdpflow import MCDPNormalizingFlow  # noqa: E402

P_DROP = 0.25
FLOWS = {"maf_2x2_L16": ("maf", (2, 2, [150, 150, 150], 16)), "nsa_4x2_L8": ("nsa", (4, 2, [128, 128], 8, 8))}
PATHS = ("fused_dropout", "per_layer", "no_dropout")


def call_ms(fn, iters: int) -> float:
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def wall_ms(fn, iters: int) -> float:
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def on(flow, path, fn):
    """fn() with the flow switched to ``path`` meanwhile."""
    os.environ["NAZ_AR_DROPOUT_FUSED"] = "0" if path == "per_layer" else "1"
    flow.train(path != "no_dropout")
    try:
        return fn()
    finally:
        os.environ.pop("NAZ_AR_DROPOUT_FUSED", None)
        flow.train()


def ab(runs, a, b):
    med = {p: float(np.median(v)) for p, v in runs.items()}
    spread = max(max(runs[p]) - min(runs[p]) for p in (a, b))
    return med, spread


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 18, 10752])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--wall-iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--niter", type=int, default=16)
    ap.add_argument("--set-rows", type=int, default=1 << 16)
    ap.add_argument("--out", default="profiles/mcdp_sample_bench.json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = dict(p=P_DROP, device=torch.cuda.get_device_name(0), iters=a.iters, wall_iters=a.wall_iters, warmup=a.warmup,
               reps=a.reps, transform_z={}, sample_uncertain={})
    ok = True
    with torch.no_grad():
        for name, (ftype, args) in FLOWS.items():
            torch.manual_seed(0)
            flow = MCDPNormalizingFlow(ftype, None, *args, dropout_p=P_DROP).to(dev)
            flow.train()
            assert flow._plan is not None and flow._plan.dropout_sample_usable(), name
            D, C = args[0], args[1]
            rec["transform_z"][name] = {}
            for B in a.rows:
                g = torch.Generator().manual_seed(B)
                z = torch.randn(B, D, generator=g).to(dev)
                c = torch.randn(B, C, generator=g).to(dev)
                call = lambda: flow._pdf(c)._transform_z(z)  # noqa: E731
                for p in PATHS:
                    on(flow, p, lambda: call_ms(call, a.warmup))
                runs = {p: [] for p in PATHS}
                for _ in range(a.reps):
                    for p in PATHS:
                        runs[p].append(on(flow, p, lambda: call_ms(call, a.iters)))
                med, spread = ab(runs, "fused_dropout", "per_layer")
                beats = bool(med["per_layer"] - med["fused_dropout"] > spread)
                ok = ok and beats
                rec["transform_z"][name][str(B)] = dict(
                    ms=runs, median_ms=med, spread_ms=spread, per_layer_over_fused=med["per_layer"] / med["fused_dropout"],
                    dropout_over_plain=med["fused_dropout"] / med["no_dropout"], beats_per_layer=beats)
                print(f"{name} B={B}: {runs} ms, per-layer/fused x{med['per_layer'] / med['fused_dropout']:.2f}, "
                      f"dropout/plain x{med['fused_dropout'] / med['no_dropout']:.2f}, spread {spread:.3f} ms", flush=True)
            cond = torch.randn(C, generator=torch.Generator().manual_seed(1)).to(dev)
            call = lambda: flow.sample_uncertain(a.niter, [a.set_rows], condition=cond)  # noqa: E731
            paths = PATHS[:2]
            for p in paths:
                on(flow, p, lambda: wall_ms(call, 1))
            runs = {p: [] for p in paths}
            for _ in range(a.reps):
                for p in paths:
                    runs[p].append(on(flow, p, lambda: wall_ms(call, a.wall_iters)))
            med, spread = ab(runs, *paths)
            beats = bool(med["per_layer"] - med["fused_dropout"] > spread)
            ok = ok and beats
            rec["sample_uncertain"][name] = dict(niter=a.niter, rows=a.set_rows, wall_ms=runs, median_ms=med,
                                                 spread_ms=spread, beats_per_layer=beats,
                                                 per_layer_over_fused=med["per_layer"] / med["fused_dropout"])
            print(f"{name} sample_uncertain({a.niter}, [{a.set_rows}]): {runs} ms wall, per-layer/fused "
                  f"x{med['per_layer'] / med['fused_dropout']:.2f}, spread {spread:.3f} ms", flush=True)
    rec["fused_beats_per_layer_everywhere"] = ok
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
