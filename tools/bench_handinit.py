#!/usr/bin/env python
"""Times the hand initialisation from keypoints (homan_amd/handinit.py, csrc/handinit.hip) at 30 frames x 8 candidates on the
synthetic MANO model: keypoints of a known pose, the default candidate rotations, 2-D and 3-D targets.

Timed run (wall clock around synchronised runs of `--steps` steps on a resident fitter, graph replays; median of `--reps` after
one untimed fit): milliseconds per fit, fits per second, microseconds per step.  Kernel statistics are collected in a run of
their own, afterwards: `--profile-steps` un-captured steps under torch's profiler, every launch's mean duration and its share
of the step's summed kernel time - hm_keypoint_terms_clips (k_keypoint_terms) beside the MANO forward and backward.

usage: python tools/bench_handinit.py [--steps K] [--reps R] [--out profiles/handinit.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from homan_amd import handinit  # noqa: E402
from homan_amd.mano_assets import hand_models, synthetic_mano  # noqa: E402

B, F_PX, C_PX = 30, 351.0, 128.0


def targets(fit):
    """keypoints of a known pose under a known rigid motion, from the fitter's own kernels -> (kp2d, c2, K, kp3d, c3)"""
    dev = fit.device
    gen = torch.Generator().manual_seed(0)
    base = torch.randn(16, generator=gen) * 0.4
    with torch.no_grad():
        fit.pca.zero_()
        fit.pca[:B, :16] = (base[None] + torch.randn(B, 16, generator=gen) * 0.03).to(dev)
        a = 0.5 + 0.01 * torch.arange(B, dtype=torch.float32)
        R = torch.zeros(B, 3, 3)
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = a.cos(), a.sin(), -a.sin(), a.cos(), 1.0
        fit.rot6d[:B] = R[:, :, :2].to(dev)
        fit.trans[:B] = torch.tensor([0.02, -0.01, 0.5], device=dev)
    fit._forward()
    X = torch.einsum("kv,nvc->nkc", fit.W, fit.vh[:B]).cpu()
    kp2d = torch.stack([F_PX * X[..., 0] / X[..., 2] + C_PX, F_PX * X[..., 1] / X[..., 2] + C_PX], -1)
    K = torch.tensor([[F_PX, 0, C_PX], [0, F_PX, C_PX], [0, 0, 1.0]]).repeat(B, 1, 1)
    return kp2d, torch.ones(B, 21), K, X - X[:, :1], torch.ones(B, 21)


def kernel_stats(fit, steps):
    from torch.profiler import ProfilerActivity, profile
    fit._step_fused()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fit._step_fused()
        torch.cuda.synchronize()
    rows = {}
    for e in prof.key_averages():
        if "memcpy" in e.key.lower() or "memset" in e.key.lower() or e.key.startswith("hip"):     # (runtime calls are no kernels)
            continue
        total = getattr(e, "self_device_time_total", None)
        total = getattr(e, "self_cuda_time_total", 0.0) if total is None else total
        rows[e.key.split("(")[0]] = {"launches_per_step": e.count / steps, "us_per_launch": round(total / max(e.count, 1), 3),
                                     "us_per_step": round(total / steps, 3)}
    whole = sum(r["us_per_step"] for r in rows.values())
    for r in rows.values():
        r["share_of_step"] = round(r["us_per_step"] / whole, 4) if whole else None
    return {"kernels": rows, "kernel_us_per_step": round(whole, 3), "launches_per_step": sum(r["launches_per_step"] for r in rows.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_handinit needs the MI355X"
    cands = handinit.default_candidates()
    fit = handinit.HandKeypointFitter(hand_models(synthetic_mano(0))["right"], "right", B, cands.shape[0], max_steps=max(a.steps, 16))
    data = targets(fit)
    walls, res = [], None
    for _ in range(a.reps + 1):
        fit.load(data[0], data[1], data[2], cands, data[3], data[4])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit.run(a.steps)
        res = fit.result()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    timed = walls[1:]
    ms = float(np.median(timed))
    log = fit.loss_evolution()
    rec = {"frames": B, "candidates": int(cands.shape[0]), "steps": a.steps, "reps": a.reps,
           "fit_ms": {"median": round(ms, 3), "lowest": round(min(timed), 3), "highest": round(max(timed), 3)},
           "fits_per_second": round(1e3 / ms, 2), "us_per_step": round(1e3 * ms / a.steps, 2),
           "graph_steps_per_replay": handinit.GRAPH_STEPS, "selected_candidate": res["candidate"],
           "total_first": [float(v) for v in log[0, :, 7]], "total_final": [float(v) for v in res["vals"][:, 7]]}
    try:
        rec["kernel_stats"] = dict(kernel_stats(fit, a.profile_steps), steps=a.profile_steps, mode="un-captured launches")
    except Exception as exc:                                               # statistics, not a result: the timed record stands
        rec["kernel_stats"] = {"error": repr(exc)}
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
