#!/usr/bin/env python
"""Times the object-pose initialisation in soft silhouette mode (homan_amd.pose_optimization.find_optimal_pose with
sil_mode="soft") at the reference's size - 500 candidates against one 256 x 256 mask, the bottle of 3 000 faces, the scene of
bench.py --pose-init and tools/bench_poseinit_chamfer.py - through the loops that run it, with the hard fused loop as context:

  soft:fused   the fused launch sequence in a hipGraph, run by the resident fitter (hm_softsil_fwd, hm_softsil_pose_terms,
               hm_softsil_bwd, hm_rigid_bwd);
  soft:graph   PoseOptimizer.forward + autograd + torch Adam captured in a hipGraph (`_graph_loop`);
  nmr:fused    the default mode's fused loop (another image formation: context, not a comparison of like with like).

A fit is timed as a user makes it - find_optimal_pose, wall clock around a device synchronisation - at `--steps` and at twice
`--steps`; the two give the cost of a step and, by extrapolation to zero steps, the per-fit set-up.  The loops are timed
alternately, `--reps` rounds after `--warmup` untimed ones, and the medians are printed as one JSON line per loop (fields as
tools/bench_poseinit_chamfer.py).  The soft image's cost grows with the blur: `--sigma` is the one timed (with `--decay` < 1
the blur shrinks during a fit, so the step / set-up split of the two fit lengths means nothing; read fit_ms).  A last line
times hm_softsil_pose_terms alone at the same size.

usage: python tools/bench_poseinit_soft.py [--sigma 1e-4] [--decay 1.0] [--n 500] [--steps 50] [--size 256]
                                           [--loops soft:fused,soft:graph,nmr:fused] [--reps 5] [--warmup 2] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from homan_amd import pose_optimization as po  # noqa: E402
from bench_poseinit_chamfer import scene  # noqa: E402  (tools/ is the script's directory)


def terms_kernel_us(n, size, launches=200, repeats=5):
    """hm_softsil_pose_terms alone on n images of size x size: median over `repeats` of the device time of `launches` back-to-back
    launches (events around the batch, after a warm-up batch) -> (microseconds per launch, GB/s of alpha read + grad written)"""
    from homan_amd import lib as hlib, ops
    L, P = hlib.lib(), hlib.ptr
    alpha = torch.rand(n, size, size, device="cuda")
    keep, ref = torch.ones(size, size, device="cuda"), (torch.rand(size, size, device="cuda") < 0.3).float()
    terms, grad = torch.zeros(n, 2, device="cuda"), torch.zeros(n, size, size, device="cuda")
    ws = ops.softsil_pose_workspace(n, size, "cuda")
    call = lambda: hlib.check(L.hm_softsil_pose_terms(P(alpha), P(keep), P(ref), n, size, P(terms), P(grad), P(ws), hlib.stream()),
                              "hm_softsil_pose_terms")
    times = []
    for rep in range(repeats + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            call()
        end.record()
        torch.cuda.synchronize()
        if rep > 0:
            times.append(start.elapsed_time(end) * 1e3 / launches)
    us = statistics.median(times)
    return us, 2 * alpha.numel() * 4 / (us * 1e-6) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigma", type=float, default=1e-4)
    ap.add_argument("--decay", type=float, default=1.0)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--loops", default="soft:fused,soft:graph,nmr:fused")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_poseinit_soft needs the MI355X"
    verts, faces, mask, bbox, sq, K, rots = scene(a.n, a.size)
    loops = a.loops.split(",")
    soft = dict(sil_mode="soft", sil_sigma=a.sigma, sil_sigma_decay=a.decay)

    def fit_ms(loop, steps):
        sil, mode = loop.split(":")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        po.find_optimal_pose(verts, faces, mask, bbox, sq, (350, 350), K=K, num_iterations=steps, num_initializations=a.n,
                             rotations_init=rots, rend_size=a.size, mode=mode, **(soft if sil == "soft" else {}))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    times = {(loop, k): [] for loop in loops for k in (1, 2)}
    for rep in range(a.warmup + a.reps):
        for k in (1, 2):
            for loop in loops:                      # (alternating: every round sees the same machine)
                ms = fit_ms(loop, k * a.steps)
                if rep >= a.warmup:
                    times[(loop, k)].append(ms)
    records = []
    for loop in loops:
        t1, t2 = statistics.median(times[(loop, 1)]), statistics.median(times[(loop, 2)])
        step_ms = (t2 - t1) / a.steps
        rec = {"loop": loop, "sil_sigma": a.sigma, "sil_sigma_decay": a.decay, "candidates": a.n, "steps": a.steps, "size": a.size,
               "pose_steps_per_s": round(a.n * a.steps / (t1 * 1e-3)), "fit_ms": round(t1, 3),
               "fit_ms_min": round(min(times[(loop, 1)]), 3), "fit_ms_max": round(max(times[(loop, 1)]), 3),
               "fit_ms_2x_steps": round(t2, 3), "step_ms": round(step_ms, 4), "setup_ms": round(t1 - a.steps * step_ms, 3),
               "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
        records.append(rec)
        print(json.dumps(rec), flush=True)
    us, gbs = terms_kernel_us(a.n, a.size)
    rec = {"kernel": "hm_softsil_pose_terms", "candidates": a.n, "size": a.size, "us": round(us, 2), "GB_per_s": round(gbs, 1)}
    records.append(rec)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(records, fh, indent=1)


if __name__ == "__main__":
    main()
