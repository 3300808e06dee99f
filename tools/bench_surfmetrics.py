#!/usr/bin/env python
"""Times the surface metrics (homan_amd/pointmetrics.py get_surface_metrics, csrc/surfdist.hip) over a walk of the size of the
HO-3D evaluation split - the sequences and meshes of tools/bench_volmetrics.py: 13 sequences, 11 524 frames, a 778-vertex hand
(1552 closed faces) and a 3000-face object per frame - and prints one JSON line:

  surface_s / surface_fps   `get_surface_metrics` as a user calls it, sequence by sequence, on the interpolated frames already on
                            the device: both directions, chunks walked, lists returned (wall clock around device synchronises);
  kernel_ms                 `hm_point_mesh_distance` alone, called through ctypes on preallocated buffers (d2, face, inside; no
                            closest point), device events around `--windows` back-to-back calls on the frames of the first
                            sequence: hand vertices against the object's faces, object vertices against the hand's;
  tests_per_s               point-triangle tests per second those times imply (frames x points x faces / time) and
  fp32_share                the share of the fp32 vector peak at OPS_PER_TEST operations per test (see below);
  inter_s / inter_fps       for scale: `get_inter_metrics` (penetration depth off the 32^3 SDF) on the same frames, 512 at a time;
  grid_vs_exact             how far the grid's `pen_depths` lie from the exact `pen_depth` on the walk (information, no bar).
Every figure is the median of `--reps` timed windows after one untimed pass over every shape.

usage: python tools/bench_surfmetrics.py [--reps R] [--windows W] [--chunk C] [--out FILE.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from homan_amd import ho3deval, lib, pointmetrics, synth  # noqa: E402
from homan_amd.mano_assets import synthetic_mano  # noqa: E402
from bench_ho3deval import SEQ_LENS, make_sequence  # noqa: E402

# fp32 operations of one point-triangle test, counted off csrc/surfdist.hip (comparisons and selects not counted; contraction is
# off by definition, so none of them is half of an FMA): p - a, p - b, p - c 9; six dot products 30; va, vb, vc 9; d4 - d3 and
# d5 - d6 2; the closest point 8 (an edge region: one difference, one division, three multiply-adds as separate operations; a
# vertex region 0, the interior 16); p - q and its square 8; the ray test's six differences and three orientations 15 (most
# pairs leave it earlier).
OPS_PER_TEST = 81
PEAK_FP32_VECTOR = 157.3e12          # MI355X fp32 vector peak with every instruction an FMA (2 operations); without FMA: half


def median_wall(fn, reps):
    """median over `reps` calls, each ended by a device synchronise, after one untimed call -> (seconds, last result)"""
    fn()
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def median_events(fn, reps, windows):
    """median over `reps` of the device time of one call, from events around `windows` back-to-back calls -> milliseconds"""
    fn()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(windows):
            fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) / windows)
    return statistics.median(times)


def kernel_call(points, verts, faces):
    """a closure that enqueues hm_point_mesh_distance on preallocated outputs, and the number of point-triangle tests of a call"""
    h = lib.lib()
    B, N, V, F = points.shape[0], points.shape[1], verts.shape[1], faces.shape[0]
    dev = points.device
    d2 = torch.empty(B, N, device=dev)
    face, inside = torch.empty(B, N, dtype=torch.int32, device=dev), torch.empty(B, N, dtype=torch.int32, device=dev)
    nbytes = h.hm_point_mesh_workspace_bytes(B, N, F)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    args = (lib.ptr(points), lib.ptr(verts), lib.ptr(faces), B, N, V, F, lib.ptr(d2), lib.ptr(face), lib.ptr(inside), None,
            lib.ptr(ws) if nbytes else None)

    def call():
        lib.check(h.hm_point_mesh_distance(*args, lib.stream()), "hm_point_mesh_distance")
    call.keep = (d2, face, inside, ws)
    return call, B * N * F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_surfmetrics needs the MI355X"
    mano = synthetic_mano(0)
    hand = mano["v_template"].astype(np.float32)
    joints = np.ascontiguousarray(hand[np.linspace(0, 777, 21).astype(int)])
    obj, obj_faces = synth.bottle_mesh(segments=50, rings=30)
    obj = np.asarray(obj, np.float32) * np.float32(0.5)
    obj_faces = np.asarray(obj_faces)
    closed = np.asarray(mano["closed_faces"])
    rng = np.random.default_rng(0)
    walk = [make_sequence(rng, n, hand, joints, obj)[0] for n in SEQ_LENS]
    frames = sum(SEQ_LENS)
    clips = [(ho3deval.interpolate_sequence(seq, n, "hand_verts3d", ho3deval.CAMEXTR_SIGNS),
              ho3deval.interpolate_sequence(seq, n, "obj_verts3d", ho3deval.CAMEXTR_SIGNS)) for n, seq in zip(SEQ_LENS, walk)]
    hand_faces, object_faces = closed[None], obj_faces[None]
    tests_per_frame = hand.shape[0] * obj_faces.shape[0] + obj.shape[0] * closed.shape[0]

    def surface():
        return [pointmetrics.get_surface_metrics(h, o, hand_faces, object_faces) for h, o in clips]
    t_surf, res = median_wall(surface, a.reps)
    pen = np.concatenate([r["pen_depth"] for r in res])
    rec = {"sequences": len(SEQ_LENS), "frames": frames, "hand_verts": int(hand.shape[0]), "hand_faces": int(closed.shape[0]),
           "obj_verts": int(obj.shape[0]), "obj_faces": int(obj_faces.shape[0]), "reps": a.reps, "windows": a.windows,
           "chunk": a.chunk, "ops_per_test": OPS_PER_TEST, "tests_per_frame": tests_per_frame,
           "surface_s": round(t_surf, 4), "surface_fps": round(frames / t_surf, 1),
           "surface_tests_per_s": round(frames * tests_per_frame / t_surf, 1),
           "mean_pen_depth_mm": round(float(pen.mean()) * 1e3, 4),
           "mean_pen_depth_obj_mm": round(float(np.concatenate([r["pen_depth_obj"] for r in res]).mean()) * 1e3, 4),
           "mean_min_dist_mm": round(float(np.concatenate([r["min_dist"] for r in res]).mean()) * 1e3, 4),
           "mean_contact_share": round(float(np.concatenate([r["contact_share"] for r in res]).mean()), 5),
           "frames_in_contact": int(np.concatenate([r["has_contact"] for r in res]).sum()),
           "frames_penetrating": int((pen > 0).sum()), "kernel_ms": {}, "tests_per_s": {}, "fp32_share": {}}

    h0, o0 = clips[0]
    dev_obj_faces = torch.from_numpy(np.ascontiguousarray(obj_faces, dtype=np.int32)).to(h0.device)
    dev_hand_faces = torch.from_numpy(np.ascontiguousarray(closed, dtype=np.int32)).to(h0.device)
    total_ms, total_tests = 0.0, 0
    for key, (call, tests) in (("hand_to_object", kernel_call(h0, o0, dev_obj_faces)),
                               ("object_to_hand", kernel_call(o0, h0, dev_hand_faces))):
        ms = median_events(call, a.reps, a.windows)
        rate = tests / (ms * 1e-3)
        rec["kernel_ms"][key] = round(ms, 4)
        rec["tests_per_s"][key] = round(rate, 1)
        # operations over the peak WITH FMA (the guide's figure), and over what a stream without FMA can issue (half of it)
        rec["fp32_share"][key] = {"of_fma_peak": round(rate * OPS_PER_TEST / PEAK_FP32_VECTOR, 4),
                                  "of_issue_peak_without_fma": round(rate * OPS_PER_TEST / (PEAK_FP32_VECTOR / 2), 4)}
        total_ms, total_tests = total_ms + ms, total_tests + tests
    rec["kernel_frames"] = int(h0.shape[0])
    rec["kernel_walk_estimate_s"] = round(total_ms * 1e-3 * frames / h0.shape[0], 4)
    rec["tests_per_s"]["both"] = round(total_tests / (total_ms * 1e-3), 1)

    def depths():
        out = []
        for h, o in clips:
            for f0 in range(0, h.shape[0], a.chunk):
                out += pointmetrics.get_inter_metrics(h[f0:f0 + a.chunk], o[f0:f0 + a.chunk], torch.from_numpy(closed)[None],
                                                      torch.from_numpy(obj_faces)[None])["pen_depths"]
        return out
    t_inter, grid = median_wall(depths, max(a.reps // 2, 1))
    grid = np.asarray(grid, np.float64)
    diff = np.abs(grid - pen)
    rec.update({"inter_s": round(t_inter, 4), "inter_fps": round(frames / t_inter, 1),
                "grid_vs_exact": {"mean_grid_mm": round(float(grid.mean()) * 1e3, 4), "mean_exact_mm": round(float(pen.mean()) * 1e3, 4),
                                  "mean_abs_diff_mm": round(float(diff.mean()) * 1e3, 4), "max_abs_diff_mm": round(float(diff.max()) * 1e3, 4),
                                  "frames_grid_positive": int((grid > 0).sum()), "frames_exact_positive": int((pen > 0).sum())},
                "device": torch.cuda.get_device_name(0)})
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
