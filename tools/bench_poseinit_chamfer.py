#!/usr/bin/env python
"""Times the object-pose initialisation with the edge-chamfer term on (homan_amd.pose_optimization.find_optimal_pose with
lw_chamfer != 0) at the reference's size - 500 candidates x 50 Adam steps against one 256 x 256 mask, the scene of
bench.py --pose-init - through the loops that can run that configuration:

  fused   the fused launch sequence in a hipGraph, run by the resident fitter (hm_pose_edge_terms + hm_sil_bwd mode 3);
  graph   PoseOptimizer.forward + autograd + torch Adam captured in a hipGraph (`_graph_loop`): the only way to run the
          configuration before the fused loop took the term.

A fit is timed as a user makes it - find_optimal_pose, wall clock around a device synchronisation - at `--steps` and at twice
`--steps`; the two give the cost of a step and, by extrapolation to zero steps, the per-fit set-up (mask upload, distance
transform, optimiser reset; for `graph` also the module's construction, the two un-captured steps and the capture).  The loops
are timed alternately, `--reps` rounds after `--warmup` untimed ones, and the medians are printed as one JSON line per loop:

  pose_steps_per_s   candidates * steps / median time of a `--steps` fit
  step_ms, setup_ms  as above;  fit_ms_min / fit_ms_max: the spread of the timed `--steps` fits

`--lw 0` times the reference's own configuration (no keyword is passed: the line also runs on a tree without the term).

usage: python tools/bench_poseinit_chamfer.py [--lw 0.5] [--n 500] [--steps 50] [--size 256] [--loops fused,graph] [--reps 5]
                                              [--warmup 2] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from homan_amd import ops, synth  # noqa: E402
from homan_amd import pose_optimization as po  # noqa: E402


def scene(n, size):
    """bench.py --pose-init's: the lathe bottle (3000 faces) rendered at a known pose as the mask, n random starting rotations"""
    ov, of = synth.bottle_mesh()
    verts, faces = torch.from_numpy(ov), torch.from_numpy(of).long()
    K = np.array([[480.0, 0, 175.0], [0, 480.0, 175.0], [0, 0, 1.0]], np.float32)
    sq = np.array([75.0, 60.0, 200.0, 200.0], np.float32)
    Rgt = torch.tensor(synth._rot_x(1.3) @ synth._rot_y(0.4), dtype=torch.float32)
    tgt_pose = (verts @ Rgt + torch.tensor([0.0, -0.02, 0.6]))[None]
    roi = po.get_K_crop_resize(torch.as_tensor(K)[None], torch.tensor([[sq[0], sq[1], sq[0] + sq[2], sq[1] + sq[2]]]), [size])
    roi[:, :2] /= size
    tgt = po.PoseOptimizer(ref_image=np.zeros((size, size), np.float32), vertices=verts, faces=faces,
                           rotation_init=po.matrix_to_rot6d(torch.eye(3)[None]), translation_init=torch.zeros(1, 1, 3), K=roi)
    with torch.no_grad():
        mask = ops.silhouette_render_noaa(tgt_pose.cuda(), tgt._K_all, tgt._sil_ctx).cpu().numpy()[0]
    ys, xs = np.nonzero(mask > 0)
    bbox = np.array([sq[0] + xs.min() * sq[2] / size, sq[1] + ys.min() * sq[2] / size,
                     (xs.max() - xs.min()) * sq[2] / size, (ys.max() - ys.min()) * sq[2] / size], np.float32)
    torch.manual_seed(0)
    return verts, faces, mask, bbox, sq, K, po.compute_random_rotations(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lw", type=float, default=0.5)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--loops", default="fused,graph")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_poseinit_chamfer needs the MI355X"
    verts, faces, mask, bbox, sq, K, rots = scene(a.n, a.size)
    term = dict(lw_chamfer=a.lw) if a.lw != 0 else {}
    loops = a.loops.split(",")

    def fit_ms(mode, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        po.find_optimal_pose(verts, faces, mask, bbox, sq, (350, 350), K=K, num_iterations=steps, num_initializations=a.n,
                             rotations_init=rots, rend_size=a.size, mode=mode, **term)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    times = {(mode, k): [] for mode in loops for k in (1, 2)}
    for rep in range(a.warmup + a.reps):
        for k in (1, 2):
            for mode in loops:                      # (alternating: every round sees the same machine)
                ms = fit_ms(mode, k * a.steps)
                if rep >= a.warmup:
                    times[(mode, k)].append(ms)
    records = []
    for mode in loops:
        t1, t2 = statistics.median(times[(mode, 1)]), statistics.median(times[(mode, 2)])
        step_ms = (t2 - t1) / a.steps
        rec = {"loop": mode, "lw_chamfer": a.lw, "candidates": a.n, "steps": a.steps, "size": a.size,
               "pose_steps_per_s": round(a.n * a.steps / (t1 * 1e-3)), "fit_ms": round(t1, 3), "fit_ms_min": round(min(times[(mode, 1)]), 3),
               "fit_ms_max": round(max(times[(mode, 1)]), 3), "fit_ms_2x_steps": round(t2, 3), "step_ms": round(step_ms, 4),
               "setup_ms": round(t1 - a.steps * step_ms, 3), "reps": a.reps, "warmup": a.warmup,
               "device": torch.cuda.get_device_name(0)}
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(records, fh, indent=1)


if __name__ == "__main__":
    main()
