"""A/B/C of an order="linear" nsa flow's log_prob and sample: the fused launch (kind "nsa_linear",
csrc/made_ar_r16.h) against the per-kernel chain of the same flow (set_fused(False): the path before
the fused instances existed) and against the fused quadratic flow of the same shape, same process,
same rows, interleaved.

    python scripts/nsa_linear_bench.py [--rows 262144 10752] [--layers 8] [--reps 3] [--iters 20]
                                       [--out profiles/nsa_linear_bench.json]

Times ``flow.log_prob(x, condition=c)`` and ``flow._pdf(c)._transform_z(z)`` (sample without the
draw of z) of NormalizingFlow("nsa", D=4 | C=2, H=[128,128], K=8) with HIP events after warm-up: per
repetition the median of ``iters`` calls, the three paths alternating repetition by repetition.
Before timing, the fused results are compared with the chain's on the timed rows.  Writes one JSON
record with every repetition; ``beats_chain`` = the chain's median minus the fused median exceeds
the largest spread between repetitions of either.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from naz_amd.flows import NormalizingFlow  # noqa: E402

D, C, HID, K = 4, 2, [128, 128], 8


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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 18, 10752])
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/nsa_linear_bench.json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lin = NormalizingFlow("nsa", None, D, C, list(HID), a.layers, K, order="linear").to(dev)
    quad = NormalizingFlow("nsa", None, D, C, list(HID), a.layers, K).to(dev)
    assert lin.fused and lin._plan.kind == "nsa_linear" and quad.fused
    rec = dict(shape=dict(D=D, C=C, hidden=HID, K=K, L=a.layers), device=torch.cuda.get_device_name(0),
               iters=a.iters, warmup=a.warmup, reps=a.reps, rows={})
    with torch.no_grad():
        for B in a.rows:
            g = torch.Generator().manual_seed(B)
            x = (1.5 * torch.randn(B, D, generator=g)).to(dev)
            z = torch.randn(B, D, generator=g).to(dev)
            c = torch.randn(B, C, generator=g).to(dev)
            ops_ = {"log_prob": lambda f: f.log_prob(x, condition=c), "sample": lambda f: f._pdf(c)._transform_z(z)}

            def on(path, op, fn):
                """fn(call) with ``call`` = op on the flow of ``path``, switched to that path meanwhile."""
                f = quad if path == "quadratic_fused" else lin
                f.set_fused(path != "chain")
                try:
                    return fn(lambda: ops_[op](f))
                finally:
                    f.set_fused(True)

            rec["rows"][str(B)] = {}
            paths = ("fused", "chain", "quadratic_fused")
            for op in ops_:
                diff = float((on("fused", op, lambda call: call()) - on("chain", op, lambda call: call())).abs().max())
                for p in paths:
                    on(p, op, lambda call: call_ms(call, a.warmup))
                runs = {p: [] for p in paths}
                for _ in range(a.reps):
                    for p in paths:
                        runs[p].append(on(p, op, lambda call: call_ms(call, a.iters)))
                med = {p: float(np.median(v)) for p, v in runs.items()}
                spread = max(max(runs[p]) - min(runs[p]) for p in ("fused", "chain"))
                rec["rows"][str(B)][op] = dict(
                    ms=runs, median_ms=med, spread_ms=spread, max_abs_fused_minus_chain=diff,
                    chain_over_fused=med["chain"] / med["fused"], fused_over_quadratic=med["fused"] / med["quadratic_fused"],
                    beats_chain=bool(med["chain"] - med["fused"] > spread))
                print(f"B={B} {op}: {runs} ms, chain/fused x{med['chain'] / med['fused']:.2f}, "
                      f"fused/quadratic x{med['fused'] / med['quadratic_fused']:.2f}, |fused - chain| {diff:.2e}",
                      flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    return 0 if all(v[op]["beats_chain"] for v in rec["rows"].values() for op in v) else 1


if __name__ == "__main__":
    sys.exit(main())
