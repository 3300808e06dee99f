#!/usr/bin/env python
"""Times the sequence evaluation (homan_amd/ho3deval.py) on a synthetic walk at the size of the HO-3D evaluation split - 13
sequences, 11 524 frames, one fitted key frame every ten, a 778-vertex hand and a 1 500-vertex object - and prints one JSON
line:

  interp_fps      frames / s of the three key-frame interpolations a sequence needs (object, hand vertices, joints: host key
                  arrays to device, hm_keyframe_interp, no copy back), wall clock around a device synchronisation;
  evaluate_fps    frames / s of `evaluate_sequence` as a user calls it: interpolation, object distance and ADD-S, penetration
                  depth and contact in chunks of `--chunk` frames, hand-root error, export arrays copied to the host;
  scoring_fps     frames / s of what evaluate_sequence does beyond the interpolation (the difference of the two times);
  baseline_fps    the walk of reference evalho3drecons.py:120-190 over the first `--baseline-frames` frames: one
                  `pointmetrics.get_point_metrics` and one `pointmetrics.get_inter_metrics` call per frame on the same
                  (already interpolated) arrays - the frame-by-frame scoring that was possible before this module.
The baseline's values are compared with evaluate_sequence's on the frames it covers (they must be identical).

usage: python tools/bench_ho3deval.py [--chunk C] [--baseline-frames N] [--reps R] [--out FILE.json]"""
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
from homan_amd import ho3deval, pointmetrics, synth  # noqa: E402
from homan_amd.mano_assets import synthetic_mano  # noqa: E402

SEQ_LENS = [886] * 12 + [892]          # 13 sequences, 11 524 frames (the HO-3D v2 evaluation split has 11 524)
KEY_STEP = 10


def make_sequence(rng, frame_nb, hand, joints, obj):
    """key-frame results every KEY_STEP frames: the hand next to the object, both drifting; ground truth = prediction + noise"""
    seq = {}
    for f in range(0, frame_nb, KEY_STEP):
        drift = np.array([0.0005 * f, 0.0002 * f, 0.5], np.float32) + rng.normal(size=3).astype(np.float32) * 0.002
        seq[f] = {"hand_verts3d": hand + drift, "hand_joints3d": joints + drift,
                  "obj_verts3d": (obj + drift + np.array([0.06, 0.0, 0.0], np.float32)).astype(np.float32),
                  "img_path": "seq/rgb/0000.png"}
    gt_obj = (rng.normal(size=(frame_nb,) + obj.shape) * 0.003 + obj + np.array([0.06, 0.0, -0.5])).astype(np.float32)
    gt_roots = rng.normal(size=(frame_nb, 1, 3)) * 0.01 + np.array([0.0, 0.0, -0.5])
    return seq, gt_obj, gt_roots


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def interpolate_all(seq, frame_nb):
    return (ho3deval.interpolate_sequence(seq, frame_nb, "obj_verts3d", ho3deval.CAMEXTR_SIGNS),
            ho3deval.interpolate_sequence(seq, frame_nb, "hand_verts3d", ho3deval.CAMEXTR_SIGNS),
            ho3deval.interpolate_sequence(seq, frame_nb, "hand_joints3d", ho3deval.CAMEXTR_SIGNS, ho3deval.UNORDER_IDXS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--baseline-frames", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ho3deval needs the MI355X"
    mano = synthetic_mano(0)
    hand = mano["v_template"].astype(np.float32)
    joints = np.ascontiguousarray(hand[np.linspace(0, 777, 21).astype(int)])
    obj, obj_faces = synth.bottle_mesh(segments=50, rings=30)
    obj = np.asarray(obj, np.float32) * np.float32(0.5)
    closed = np.asarray(mano["closed_faces"])
    rng = np.random.default_rng(0)
    walk = [make_sequence(rng, n, hand, joints, obj) for n in SEQ_LENS]
    frames = sum(SEQ_LENS)

    def evaluate_all():
        return [ho3deval.evaluate_sequence(seq, n, gt_obj, gt_roots, obj_faces, closed, chunk=a.chunk)
                for n, (seq, gt_obj, gt_roots) in zip(SEQ_LENS, walk)]

    interpolate_all(walk[0][0], SEQ_LENS[0])                      # warm-up: every kernel and shape of the timed windows
    ho3deval.evaluate_sequence(walk[0][0], SEQ_LENS[0], walk[0][1], walk[0][2], obj_faces, closed, chunk=a.chunk)
    ho3deval.evaluate_sequence(walk[-1][0], SEQ_LENS[-1], walk[-1][1], walk[-1][2], obj_faces, closed, chunk=a.chunk)
    t_interp, t_eval = [], []
    for _ in range(a.reps):
        t_interp.append(timed(lambda: [interpolate_all(seq, n) for n, (seq, _, _) in zip(SEQ_LENS, walk)])[0])
        dt, results = timed(evaluate_all)
        t_eval.append(dt)
    t_interp, t_eval = statistics.median(t_interp), statistics.median(t_eval)

    # ---- the frame-by-frame walk on the first sequence(s), on the arrays evaluate_sequence scored
    todo = min(a.baseline_frames, frames)
    hand_faces, object_faces = torch.from_numpy(closed)[None].cuda(), torch.as_tensor(np.asarray(obj_faces))[None].cuda()
    base = {"obj_dist": [], "obj_add-s": [], "pen_depths": [], "has_contact": []}
    t_base, done = 0.0, 0
    for n, (seq, gt_obj, _) in zip(SEQ_LENS, walk):
        if done >= todo:
            break
        pred_obj, pred_hand, _ = interpolate_all(seq, n)
        gt = torch.from_numpy(gt_obj)
        take = min(n, todo - done)
        if done == 0:                                              # warm-up of the per-frame shapes
            pointmetrics.get_point_metrics(pred_obj[:1], gt[:1])
            pointmetrics.get_inter_metrics(pred_hand[:1], pred_obj[:1], hand_faces, object_faces)

        def walk_frames():
            for f in range(take):
                point = pointmetrics.get_point_metrics(pred_obj[f:f + 1], gt[f:f + 1])
                inter = pointmetrics.get_inter_metrics(pred_hand[f:f + 1], pred_obj[f:f + 1], hand_faces, object_faces)
                base["obj_dist"].append(point["verts_dists"][0])
                base["obj_add-s"].append(point["add-s"][0])
                base["pen_depths"].extend(inter["pen_depths"])
                base["has_contact"].extend(float(v) for v in inter["has_contact"])
        t_base += timed(walk_frames)[0]
        done += take
    whole = {k: np.concatenate([r[k] for r in results])[:done] for k in base}
    same = all(np.array_equal(np.asarray(base[k], np.float64), whole[k]) for k in base)
    mean = ho3deval.summarise(results, unseen_from=ho3deval.UNSEEN_FROM_HO3D)[0]
    rec = {"sequences": len(SEQ_LENS), "frames": frames, "key_step": KEY_STEP, "hand_verts": 778, "obj_verts": int(obj.shape[0]),
           "chunk": a.chunk, "reps": a.reps, "interp_s": round(t_interp, 4), "evaluate_s": round(t_eval, 4),
           "interp_fps": round(frames / t_interp, 1), "evaluate_fps": round(frames / t_eval, 1),
           "scoring_fps": round(frames / max(t_eval - t_interp, 1e-9), 1), "baseline_frames": done,
           "baseline_s": round(t_base, 4), "baseline_fps": round(done / t_base, 1), "baseline_identical": bool(same),
           "contact_rate": round(mean["has_contact"], 4), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    assert same, "evaluate_sequence and the frame-by-frame walk differ"


if __name__ == "__main__":
    main()
