"""Time the rational-linear spline kernel (ops.rqs(order="linear", fast=True)) beside the quadratic
one (the yardstick, same run) at 2^20 rows, Dt = 8, K = 8, both directions, on one GPU.

One process, device events around every launch, a warm-up first, the two kernels alternating.
Prints ms and algorithmic TB/s per kernel (bytes from the shapes: per (row, dim) the raw block and
x in, y and the per-dim ld out) and writes one JSON file.
    python scripts/rls_bench.py [--rows N] [--reps N] [--out profiles/rls_bench.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from naz_amd import ops  # noqa: E402


def algorithmic_bytes(B, Dt, K, order):
    per_dim = 4 * K - 1 if order == "linear" else 3 * K - 1
    return B * Dt * (4 * per_dim + 4 + 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rls_bench: no GPU")
    dev = torch.device("cuda")
    B, Dt, K = args.rows, 8, 8
    g = torch.Generator(device=dev).manual_seed(0)
    x = 2 * torch.randn(B, Dt, device=dev, generator=g)
    raws = {o: torch.randn(B, Dt * ((4 if o == "linear" else 3) * K - 1), device=dev, generator=g)
            for o in ("quadratic", "linear")}
    y, ld = torch.empty_like(x), torch.empty_like(x)
    result = {"rows": B, "Dt": Dt, "K": K, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for inverse in (False, True):
        def launch(order):
            ops.rqs(x, raws[order], K, ops.LAYOUT_DENSE, inverse, 3.0, ops.LD_PERDIM, ld, out=y, fast=True,
                    order=order)
        for _ in range(args.warmup):
            launch("quadratic")
            launch("linear")
        torch.cuda.synchronize()
        events = {o: [] for o in raws}
        for _ in range(args.reps):
            for o in ("quadratic", "linear"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(o)
                e1.record()
                events[o].append((e0, e1))
        torch.cuda.synchronize()
        row = {}
        for o, ev in events.items():
            ms = sorted(a.elapsed_time(b) for a, b in ev)
            med = statistics.median(ms)
            row[o] = {"ms_median": med, "ms_min": ms[0], "ms_p90": ms[int(0.9 * len(ms))],
                      "algorithmic_TB_s": algorithmic_bytes(B, Dt, K, o) / (med * 1e-3) / 1e12}
        row["ratio_linear_over_quadratic"] = row["linear"]["ms_median"] / row["quadratic"]["ms_median"]
        row["bytes_ratio"] = algorithmic_bytes(B, Dt, K, "linear") / algorithmic_bytes(B, Dt, K, "quadratic")
        name = "inverse" if inverse else "forward"
        result[name] = row
        for o in ("quadratic", "linear"):
            print(f"{name:8s} {o:10s} {row[o]['ms_median']:.4f} ms (min {row[o]['ms_min']:.4f}, p90 "
                  f"{row[o]['ms_p90']:.4f})  {row[o]['algorithmic_TB_s']:.2f} TB/s algorithmic")
        print(f"{name:8s} linear / quadratic = {row['ratio_linear_over_quadratic']:.3f} "
              f"(bytes ratio {row['bytes_ratio']:.3f})")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
