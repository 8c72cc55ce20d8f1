"""A/B of the unconditional paper maf (D=2 | C=0, H=[150]x3; naz examples/papers/2506.05657/
train_mle_unsupervised.py) on the fused autoregressive kernels against the per-layer path it took
before they had an instance at this shape, same process, same weights and rows, interleaved.

    python scripts/maf_uncond_bench.py [--rows 262144 10752] [--layers 10] [--reps 3] [--iters 5]
                                       [--out profiles/maf_uncond_bench.json]

Times, with HIP events after warm-up (per repetition the median of ``iters`` calls, the paths
alternating repetition by repetition):
  log_prob   flow.log_prob(x) under no_grad           fused vs set_fused(False)
  sample     flow.sample([B])                         fused vs set_fused(False)
  train      -log_prob(x).mean() and its backward     fused vs NAZ_TRAIN_FUSED=0 (the autograd walk)
  dropout    MCDP sample_uncertain(16, [2^16])        fused vs NAZ_AR_DROPOUT_FUSED=0
and, as a sanity line beside each, the fused conditional D=2 | C=2 flow of the same depth.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from naz_amd.flows import NormalizingFlow  # noqa: E402
from naz_amd.flows import flow as flow_mod  # noqa: E402
from naz_amd.flows.mcdpflow import MCDPNormalizingFlow  # noqa: E402

D, HID = 2, [150, 150, 150]


def timed(fn, iters: int) -> float:
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def ab(paths: dict, reps: int, iters: int, warmup: int) -> dict:
    """paths: name -> (enter, fn); enter() switches to the path.  Interleaved repetitions."""
    for enter, fn in paths.values():
        enter()
        timed(fn, warmup)
    runs = {k: [] for k in paths}
    for _ in range(reps):
        for k, (enter, fn) in paths.items():
            enter()
            runs[k].append(timed(fn, iters))
    out = {f"{k}_ms": v for k, v in runs.items()}
    out.update({f"{k}_median_ms": float(np.median(v)) for k, v in runs.items()})
    out["spread_ms"] = max(max(v) - min(v) for k, v in runs.items() if k != "cond_fused")
    if "fused" in runs and "before" in runs:
        out["gain_ms"] = out["before_median_ms"] - out["fused_median_ms"]
        out["speedup"] = out["before_median_ms"] / out["fused_median_ms"]
        out["fused_stays_default"] = bool(out["gain_ms"] > out["spread_ms"])
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 18, 10752])
    ap.add_argument("--layers", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dropout-iters", type=int, default=16)
    ap.add_argument("--dropout-rows", type=int, default=1 << 16)
    ap.add_argument("--out", default="profiles/maf_uncond_bench.json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    L = a.layers
    f = NormalizingFlow("maf", None, D, 0, list(HID), L).to(dev)
    fc = NormalizingFlow("maf", None, D, 2, list(HID), L).to(dev)
    assert f.fused and fc.fused
    rec = dict(shape=dict(D=D, C=0, hidden=HID, L=L), device=torch.cuda.get_device_name(0), iters=a.iters,
               warmup=a.warmup, reps=a.reps, rows={})

    def fused(on):
        return lambda: f.set_fused(on)

    def train_flag(flag):
        def enter():
            f.set_fused(True)
            flow_mod._TRAIN_FUSED = flag
        return enter

    def step(flow, x, c):
        def fn():
            flow.zero_grad(set_to_none=False)
            (-flow.log_prob(x, condition=c).mean()).backward()
        return fn

    def nograd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    for B in a.rows:
        g = torch.Generator().manual_seed(B)
        x = (1.5 * torch.randn(B, D, generator=g)).to(dev)
        c = torch.randn(B, 2, generator=g).to(dev)
        r = {}
        r["log_prob"] = ab({"fused": (fused(True), nograd(lambda: f.log_prob(x))),
                            "before": (fused(False), nograd(lambda: f.log_prob(x))),
                            "cond_fused": (lambda: None, nograd(lambda: fc.log_prob(x, condition=c)))},
                           a.reps, a.iters, a.warmup)
        r["sample"] = ab({"fused": (fused(True), lambda: f.sample([B])),
                          "before": (fused(False), lambda: f.sample([B])),
                          "cond_fused": (lambda: None, lambda: fc.sample([B], condition=c))},
                         a.reps, a.iters, a.warmup)
        r["train"] = ab({"fused": (train_flag("1"), step(f, x, None)),
                         "before": (train_flag("0"), step(f, x, None)),
                         "cond_fused": (train_flag("1"), step(fc, x, c))}, a.reps, a.iters, a.warmup)
        flow_mod._TRAIN_FUSED = "1"
        f.set_fused(True)
        rec["rows"][str(B)] = r
        for k, v in r.items():
            print(f"B={B} {k}: fused {v['fused_ms']} before {v['before_ms']} cond {v['cond_fused_ms']} ms "
                  f"x{v['speedup']:.2f} spread {v['spread_ms']:.3f}", flush=True)
    # MC dropout: sample_uncertain(iters, [rows]) (host copy of the samples included on both paths)
    m = MCDPNormalizingFlow("maf", None, D, 0, list(HID), L, dropout_p=0.1).to(dev)
    mc = MCDPNormalizingFlow("maf", None, D, 2, list(HID), L, dropout_p=0.1).to(dev)
    c1 = torch.tensor([0.3, -0.7], device=dev)
    n, rows = a.dropout_iters, a.dropout_rows

    def env(v):
        return lambda: os.environ.__setitem__("NAZ_AR_DROPOUT_FUSED", v)

    rec["dropout"] = dict(iters=n, rows=rows, **ab(
        {"fused": (env("1"), lambda: m.sample_uncertain(n, [rows])),
         "before": (env("0"), lambda: m.sample_uncertain(n, [rows])),
         "cond_fused": (env("1"), lambda: mc.sample_uncertain(n, [rows], condition=c1))}, a.reps, 1, 1))
    os.environ.pop("NAZ_AR_DROPOUT_FUSED", None)
    v = rec["dropout"]
    print(f"dropout {n} x {rows}: fused {v['fused_ms']} before {v['before_ms']} cond {v['cond_fused_ms']} ms "
          f"x{v['speedup']:.2f} spread {v['spread_ms']:.3f}", flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
