#!/usr/bin/env python
"""Times the volume metrics (homan_amd/pointmetrics.py get_volume_metrics, csrc/solidvox.hip) over a walk of the size of the
HO-3D evaluation split - 13 sequences, 11 524 frames, a 778-vertex hand (1552 closed faces) and a 3000-face object per frame -
at voxel pitches of 5 mm and 2 mm, and prints one JSON line:

  volume_fps[pitch]        frames / s of `get_volume_metrics` as a user calls it, sequence by sequence, on the interpolated
                           frames already on the device: boxes read back, chunks walked, lists returned (windows of 25 walks);
  launch_ms[pitch]         call time per entry point through its Python wrapper (checks, faces uploaded, boxes copied: not kernel
                           time) on the frames of the first sequence and their own boxes, device events around
                           200 back-to-back calls: `hm_mesh_volume` (hand, object), `hm_solid_voxels` (hand, object: clear,
                           mark pass, scan) and `hm_voxel_overlap`; region = launch dimensions (words per row, rows, slices);
  inter_fps                for scale: `get_inter_metrics` (penetration depth off the 32^3 SDF) on the same frames, 512 at a time;
  plausibility_fps         `ho3deval.evaluate_sequence_plausibility` over the walk from the host key frames (interpolation,
                           volume and depth), at 5 mm.
Every figure is the median of `--reps` timed windows after one untimed pass over every shape.

usage: python tools/bench_volmetrics.py [--reps R] [--chunk C] [--out FILE.json]"""
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
from homan_amd import ho3deval, ops, pointmetrics, synth  # noqa: E402
from homan_amd.mano_assets import synthetic_mano  # noqa: E402
from bench_ho3deval import SEQ_LENS, make_sequence  # noqa: E402

PITCHES = (0.005, 0.002)


def median_wall(fn, reps, inner=1):
    """median over `reps` windows of `inner` calls each, every window ended by a device synchronise, after one untimed call
    -> (seconds per call, last result): the millisecond walks are timed in windows long enough to be more than the clock"""
    fn()
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / inner)
    return statistics.median(times), out


def median_events(fn, reps, windows=200):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_volmetrics needs the MI355X"
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

    rec = {"sequences": len(SEQ_LENS), "frames": frames, "hand_faces": int(closed.shape[0]), "obj_faces": int(obj_faces.shape[0]),
           "reps": a.reps, "chunk": a.chunk, "volume_s": {}, "volume_fps": {}, "launch_ms": {}, "region": {},
           "mean_inter_volume_cm3": {}, "frames_in_contact": {}}
    for pitch in PITCHES:
        def volumes():
            return [pointmetrics.get_volume_metrics(h, o, hand_faces, object_faces, voxel=pitch) for h, o in clips]
        t, res = median_wall(volumes, a.reps, inner=25)
        inter = np.concatenate([r["inter_volumes"] for r in res])
        key = f"{round(pitch * 1000):d}mm"
        rec["volume_s"][key], rec["volume_fps"][key] = round(t, 4), round(frames / t, 1)
        rec["mean_inter_volume_cm3"][key] = round(float(inter.mean()) * 1e6, 4)
        rec["frames_in_contact"][key] = int((inter > 0).sum())
        # the entry points on the first sequence, with the boxes get_volume_metrics would hand them
        h, o = clips[0]
        hp = ops.voxel_pitch(pitch)
        boxes, _ = pointmetrics.common_boxes(h, o, hp)
        hw, ow = ops.solid_voxels(h, closed, hp, boxes), ops.solid_voxels(o, obj_faces, hp, boxes)
        rec["region"][key] = [int(hw.shape[3]), int(hw.shape[2]), int(hw.shape[1])]
        rec["launch_ms"][key] = {
            "frames": int(h.shape[0]),
            "mesh_volume_hand": round(median_events(lambda: ops.mesh_volume(h, closed), a.reps), 4),
            "mesh_volume_obj": round(median_events(lambda: ops.mesh_volume(o, obj_faces), a.reps), 4),
            "solid_voxels_hand": round(median_events(lambda: ops.solid_voxels(h, closed, hp, boxes, out=hw), a.reps), 4),
            "solid_voxels_obj": round(median_events(lambda: ops.solid_voxels(o, obj_faces, hp, boxes, out=ow), a.reps), 4),
            "voxel_overlap": round(median_events(lambda: ops.voxel_overlap(hw, ow), a.reps), 4)}

    def depths():
        out = []
        for h, o in clips:
            for f0 in range(0, h.shape[0], a.chunk):
                out += pointmetrics.get_inter_metrics(h[f0:f0 + a.chunk], o[f0:f0 + a.chunk], torch.from_numpy(closed)[None],
                                                      torch.from_numpy(obj_faces)[None])["pen_depths"]
        return out
    t_inter, pen = median_wall(depths, max(a.reps // 2, 1))
    t_plaus, plaus = median_wall(lambda: [ho3deval.evaluate_sequence_plausibility(seq, n, obj_faces, closed, chunk=a.chunk)
                                          for n, seq in zip(SEQ_LENS, walk)], max(a.reps // 2, 1))
    rec.update({"inter_s": round(t_inter, 4), "inter_fps": round(frames / t_inter, 1),
                "frames_with_depth": int((np.asarray(pen) > 0).sum()),
                "plausibility_s": round(t_plaus, 4), "plausibility_fps": round(frames / t_plaus, 1),
                "plausibility_mean_inter_volume_cm3": round(float(np.mean([p["inter_volume_mean"] for p in plaus])) * 1e6, 4),
                "device": torch.cuda.get_device_name(0)})
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
