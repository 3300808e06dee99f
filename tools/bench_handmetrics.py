#!/usr/bin/env python
"""Times the hand protocol metrics (homan_amd/handmetrics.py, csrc/evalalign.hip) at the size of the HO-3D evaluation split -
13 sequences, 11 524 frames, 21 joints and a 778-vertex hand per frame - and prints one JSON line:

  align_joints_fps / align_mesh_fps   frames / s of `hm_procrustes_align` (mode 0, all three outputs) on device tensors;
  counts_mpts                         million distances / s of `hm_threshold_counts` on the mesh errors (float64, 100 steps);
  fscore_fps                          frames / s of the two-way nearest-neighbour search plus `hm_fscore` on the meshes
                                      (these three: back-to-back calls, 500 / 200 / 500 / 20 per timed window, outputs allocated
                                      by each call);
  protocol_fps                        frames / s of `get_hand_protocol_metrics` as a user calls it: host arrays in, the table and
                                      its per-point arrays back on the host;
  evaluate_fps / evaluate_protocol_fps  `ho3deval.evaluate_sequence` over the walk of tools/bench_ho3deval.py without and with the
                                      ground-truth hand (`evaluate_sequence_protocol`);
  baseline_fps                        the float64 NumPy / SciPy loop on the host over the first `--baseline-frames` frames: per
                                      frame `scipy.linalg.orthogonal_procrustes` on joints and mesh, the scale-and-translation
                                      alignment, and two `cKDTree` queries per F-score - what was possible before this module.
The baseline's table is compared with the device's on the frames it covers.

usage: python tools/bench_handmetrics.py [--baseline-frames N] [--reps R] [--chunk C] [--out FILE.json]"""
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
from homan_amd import handmetrics, ho3deval, ops, synth  # noqa: E402
from homan_amd.mano_assets import synthetic_mano  # noqa: E402
from bench_ho3deval import SEQ_LENS, make_sequence  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def median_time(fn, reps, inner=1):
    """median over `reps` windows of `inner` calls each (one synchronisation per window) -> (seconds per call, last result):
    the sub-millisecond calls are timed in windows long enough to be more than clock and scheduler"""
    fn()                                                              # warm-up of every kernel and shape
    times, out = [], None
    for _ in range(reps):
        def window():
            for _ in range(inner - 1):
                fn()
            return fn()
        dt, out = timed(window)
        times.append(dt / inner)
    return statistics.median(times), out


def host_align(pred, gt, anchors):
    """float64: (similarity-aligned points, their errors, scale-and-translation errors) with SciPy's orthogonal_procrustes"""
    from scipy.linalg import orthogonal_procrustes
    mu_g, mu_p = gt.mean(0), pred.mean(0)
    s1, s2 = np.linalg.norm(gt - mu_g) + 1e-8, np.linalg.norm(pred - mu_p) + 1e-8
    a, b = (gt - mu_g) / s1, (pred - mu_p) / s2
    Q, sigma = orthogonal_procrustes(b, a)
    aligned = (b @ Q) * sigma * s1 + mu_g
    ia, ib = anchors
    den = np.linalg.norm(pred[ib] - pred[ia])
    k = 1.0 if den == 0 else np.linalg.norm(gt[ib] - gt[ia]) / den
    sc_tr = k * (pred - pred[ia]) + gt[ia]
    return aligned, np.linalg.norm(aligned - gt, axis=-1), np.linalg.norm(sc_tr - gt, axis=-1)


def host_fscore(pred, gt, ths):
    from scipy.spatial import cKDTree
    d_pred, d_gt = cKDTree(gt).query(pred)[0], cKDTree(pred).query(gt)[0]
    out = []
    for th in ths:
        p, r = np.mean(d_pred < th), np.mean(d_gt < th)
        out.append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    return out


def host_protocol(gt_j, pred_j, gt_v, pred_v, ths=(0.005, 0.015), auc_max=0.05, steps=100, anchors=(0, 4)):
    errs = {k: [] for k in ("xyz", "xyz_al", "xyz_sc_tr", "mesh", "mesh_al", "mesh_sc_tr")}
    fs = {"f": [], "f_al": []}
    for f in range(gt_j.shape[0]):
        for name, gt, pred in (("xyz", gt_j[f].astype(np.float64), pred_j[f].astype(np.float64)),
                               ("mesh", gt_v[f].astype(np.float64), pred_v[f].astype(np.float64))):
            aligned, e_al, e_sc = host_align(pred, gt, anchors)
            errs[name].append(np.linalg.norm(pred - gt, axis=-1))
            errs[name + "_al"].append(e_al)
            errs[name + "_sc_tr"].append(e_sc)
        fs["f"].append(host_fscore(pred, gt, ths))
        fs["f_al"].append(host_fscore(aligned, gt, ths))
    table = {}
    t = np.linspace(0, auc_max, steps)
    for key, rows in errs.items():
        err = np.stack(rows)
        pck = np.array([np.mean(err <= th) for th in t])
        table[f"{key}_mean3d"] = float(err.mean())
        table[f"{key}_auc"] = float(np.sum((pck[1:] + pck[:-1]) * np.diff(t)) / 2.0 / auc_max)
    for prefix, rows in fs.items():
        rows = np.asarray(rows)
        for i, th in enumerate(ths):
            table[f"{prefix}@{round(th * 1000):d}"] = float(rows[:, i].mean())
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-frames", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_handmetrics needs the MI355X"
    mano = synthetic_mano(0)
    hand = mano["v_template"].astype(np.float32)
    joints = np.ascontiguousarray(hand[np.linspace(0, 777, 21).astype(int)])
    obj, obj_faces = synth.bottle_mesh(segments=50, rings=30)
    obj = np.asarray(obj, np.float32) * np.float32(0.5)
    closed = np.asarray(mano["closed_faces"])
    rng = np.random.default_rng(0)
    walk = [make_sequence(rng, n, hand, joints, obj) for n in SEQ_LENS]
    frames = sum(SEQ_LENS)

    # ---- the sequence evaluation without and with the ground-truth hand
    hand_gt = []
    for n, (seq, _, _) in zip(SEQ_LENS, walk):
        pj = ho3deval.interpolate_sequence(seq, n, "hand_joints3d", ho3deval.CAMEXTR_SIGNS, ho3deval.UNORDER_IDXS).cpu().numpy()
        pv = ho3deval.interpolate_sequence(seq, n, "hand_verts3d", ho3deval.CAMEXTR_SIGNS).cpu().numpy()
        hand_gt.append(((pj * 1.02 + rng.normal(size=pj.shape) * 0.004).astype(np.float32),
                        (pv * 1.02 + rng.normal(size=pv.shape) * 0.003).astype(np.float32), pj, pv))

    def evaluate_all(with_hand):
        out = []
        for n, (seq, gt_obj, gt_roots), (gj, gv, _, _) in zip(SEQ_LENS, walk, hand_gt):
            if with_hand:
                out.append(ho3deval.evaluate_sequence_protocol(seq, n, gt_obj, gt_roots, obj_faces, closed, chunk=a.chunk,
                                                               gt_hand_joints=gj, gt_hand_verts=gv))
            else:
                out.append(ho3deval.evaluate_sequence(seq, n, gt_obj, gt_roots, obj_faces, closed, chunk=a.chunk))
        return out
    t_eval, _ = median_time(lambda: evaluate_all(False), max(a.reps // 2, 1))
    t_eval_p, results = median_time(lambda: evaluate_all(True), max(a.reps // 2, 1))
    t_summary, table_seq = median_time(lambda: ho3deval.protocol_summary(results), max(a.reps // 2, 1))

    # ---- the module on the whole split at once
    gt_j, gt_v, pred_j, pred_v = (np.concatenate([h[i] for h in hand_gt]) for i in range(4))
    t_protocol, table = median_time(lambda: handmetrics.get_hand_protocol_metrics(gt_j, pred_j, gt_v, pred_v), a.reps)
    same_as_sequences = all(abs(table[k] - v) <= 1e-12 * max(abs(v), 1.0) for k, v in table_seq.items())
    dj, dv, dgj, dgv = (torch.from_numpy(x).cuda() for x in (pred_j, pred_v, gt_j, gt_v))
    t_align_j, _ = median_time(lambda: ops.procrustes_align(dj, dgj, 0), a.reps, inner=500)
    t_align_v, (_, err_v, _) = median_time(lambda: ops.procrustes_align(dv, dgv, 0), a.reps, inner=200)
    t_counts, _ = median_time(lambda: ops.threshold_counts(err_v, 0.05, 100), a.reps, inner=500)
    t_fscore, _ = median_time(lambda: handmetrics.frame_fscores(dgv, dv, handmetrics.F_THRESHOLDS), a.reps, inner=20)

    # ---- the host loop on the first frames, and its table against the device's on the same frames
    todo = min(a.baseline_frames, frames)
    t0 = time.perf_counter()
    base = host_protocol(gt_j[:todo], pred_j[:todo], gt_v[:todo], pred_v[:todo])
    t_base = time.perf_counter() - t0
    part = handmetrics.get_hand_protocol_metrics(gt_j[:todo], pred_j[:todo], gt_v[:todo], pred_v[:todo])
    worst = {k: abs(part[k] - v) for k, v in base.items()}
    rec = {"sequences": len(SEQ_LENS), "frames": frames, "joints": 21, "hand_verts": 778, "chunk": a.chunk, "reps": a.reps,
           "align_joints_s": round(t_align_j, 6), "align_joints_fps": round(frames / t_align_j, 1),
           "align_mesh_s": round(t_align_v, 6), "align_mesh_fps": round(frames / t_align_v, 1),
           "counts_s": round(t_counts, 6), "counts_mpts": round(err_v.numel() / t_counts / 1e6, 1),
           "fscore_s": round(t_fscore, 6), "fscore_fps": round(frames / t_fscore, 1),
           "protocol_s": round(t_protocol, 4), "protocol_fps": round(frames / t_protocol, 1),
           "evaluate_s": round(t_eval, 4), "evaluate_fps": round(frames / t_eval, 1),
           "evaluate_protocol_s": round(t_eval_p, 4), "evaluate_protocol_fps": round(frames / t_eval_p, 1),
           "protocol_summary_s": round(t_summary, 4), "summary_equals_whole_split": bool(same_as_sequences),
           "baseline_frames": todo, "baseline_s": round(t_base, 4), "baseline_fps": round(todo / t_base, 1),
           "baseline_worst_mean3d_diff": max(v for k, v in worst.items() if k.endswith("_mean3d")),
           "baseline_worst_auc_diff": max(v for k, v in worst.items() if k.endswith("_auc")),
           "baseline_worst_f_diff": max(v for k, v in worst.items() if "@" in k),
           "table": {k: round(v, 6) for k, v in table.items() if isinstance(v, float)},
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    assert same_as_sequences, "protocol_summary over the sequences and get_hand_protocol_metrics over the split differ"
    assert rec["baseline_worst_mean3d_diff"] < 1e-9 and rec["baseline_worst_auc_diff"] < 1e-3 and rec["baseline_worst_f_diff"] < 1e-3


if __name__ == "__main__":
    main()
