#!/usr/bin/env python
"""Times the two-way nearest-neighbour search behind homan_amd.pointmetrics (hm_cloud_metrics) at evaluation sizes and
prints one JSON line per size: milliseconds per call (device events, after warm-up) and pair evaluations per second
(2 * B * N * M: both directions).  --host also times what the reference's stack does on the host for the same inputs:
scipy cKDTree queries in both directions (chamfer from the squared distances, ADD-S), single-threaded, float64.

usage: python tools/bench_pointmetrics.py [--reps R] [--host]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from homan_amd import ops  # noqa: E402

# (frames, N, M): a clip's hands, a clip's objects against dense ground truth, one dense scan, an evaluation batch of hands
SIZES = [(30, 778, 778), (30, 2000, 10000), (1, 50000, 50000), (2000, 778, 778)]


def host_metrics(x, y):
    from scipy.spatial import cKDTree
    out = []
    for xb, yb in zip(x.astype(np.float64), y.astype(np.float64)):
        dx, _ = cKDTree(yb).query(xb, k=1)
        dy, _ = cKDTree(xb).query(yb, k=1)
        out.append(((dx ** 2).mean() + (dy ** 2).mean(), dx.mean()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pointmetrics needs the MI355X"
    gen = torch.Generator(device="cuda").manual_seed(0)
    for B, N, M in SIZES:
        x = 0.1 * torch.randn(B, N, 3, device="cuda", generator=gen)
        y = 0.1 * torch.randn(B, M, 3, device="cuda", generator=gen)
        for _ in range(2):
            tab = ops.cloud_metrics(x, y)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            ops.cloud_metrics(x, y)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / a.reps
        pairs = 2.0 * B * N * M
        rec = {"frames": B, "N": N, "M": M, "ms": round(ms, 4), "pairs_per_s": float(f"{pairs / (ms * 1e-3):.4g}")}
        if a.host:
            xh, yh = x.cpu().numpy(), y.cpu().numpy()
            h0 = time.perf_counter()
            ref = host_metrics(xh, yh)
            rec["host_ckdtree_ms"] = round((time.perf_counter() - h0) * 1e3, 1)
            t = tab.cpu().numpy()
            rec["max_rel_diff_vs_host"] = float(max(max(abs(t[b, 0] + t[b, 1] - c) / c, abs(t[b, 2] - s) / s)
                                                    for b, (c, s) in enumerate(ref)))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
