#!/usr/bin/env python
"""Golden vectors for the evaluation metrics (homan_amd/pointmetrics.py), produced by the REFERENCE's own
homan/eval/pointmetrics.py (get_point_metrics, get_align_metrics, imported in place) on CPU tensors, with scipy's real
cKDTree and a float64 restatement of pytorch3d's chamfer_distance.  Build container only; writes
tests/golden/pointmetrics_reference.npz (or the path given as the first argument)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import shims  # noqa: E402

# (not ref_*.npz: tests/util.py reads every ref_*.npz but the pose-initialisation one as a joint-fit golden)
OUT = os.path.join(ROOT, "tests", "golden", "pointmetrics_reference.npz")


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None,
                     batch_reduction="mean", point_reduction="mean", norm=2):
    """pytorch3d.loss.chamfer_distance as documented, for the calls the reference makes (no lengths, normals or weights):
    per frame mean_i min_j |x_i - y_j|^2 + mean_j min_i |y_j - x_i|^2 (squared Euclidean distances, norm=2,
    point_reduction="mean"); batch_reduction=None keeps the (B,) vector, "mean" averages it.  Returns (distance, None)
    like the library when no normals are given.  Computed in float64."""
    assert x_lengths is None and y_lengths is None and x_normals is None and y_normals is None and weights is None
    assert norm == 2 and point_reduction == "mean"
    d2 = ((x.double()[:, :, None, :] - y.double()[:, None, :, :]) ** 2).sum(-1)
    cham = d2.min(2)[0].mean(1) + d2.min(1)[0].mean(1)
    if batch_reduction == "mean":
        cham = cham.mean()
    elif batch_reduction == "sum":
        cham = cham.sum()
    return cham, None


def import_pointmetrics():
    shims.install()
    shims._module("pytorch3d")
    shims._module("pytorch3d.loss")
    shims._module("pytorch3d.loss.chamfer", chamfer_distance=chamfer_distance)
    cwd = os.getcwd()
    os.chdir(shims.REFERENCE_ROOT)
    sys.path.insert(0, shims.REFERENCE_ROOT)
    try:
        import homan.eval.pointmetrics as ref_pm
    finally:
        os.chdir(cwd)
        sys.path.remove(shims.REFERENCE_ROOT)
    return ref_pm


def _rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def resample(verts, faces, n, rng):
    """n points on the surface of the mesh: random faces, random barycentric coordinates."""
    f = faces[rng.integers(0, faces.shape[0], n)]
    w = rng.dirichlet(np.ones(3), n)
    return (verts[f] * w[:, :, None]).sum(1)


def clouds(seed):
    """(hand template, object mesh vertices, resampled object) and a seeded RNG"""
    from homan_amd import synth
    from homan_amd.mano_assets import synthetic_mano
    rng = np.random.default_rng(seed)
    ov, of = synth.bottle_mesh(segments=24, rings=16)
    return synthetic_mano(0)["v_template"].astype(np.float64), ov.astype(np.float64), resample(ov, of, 517, rng), rng


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def main(out=OUT):
    ref_pm = import_pointmetrics()
    hand, obj, obj_rs, rng = clouds(7)
    rec = {}
    # ---- get_point_metrics: N == M (prediction = ground truth + noise) and N != M (a resampled surface)
    for tag, pred_src in (("eq", obj), ("neq", obj_rs)):
        gt, pred = [], []
        for _ in range(3):
            R, t = _rot(rng), rng.normal(size=3) * 0.05 + np.array([0.0, 0.0, 0.5])
            gt.append(obj @ R.T + t)
            off = rng.normal(size=3) * 0.01
            pred.append((pred_src + rng.normal(size=pred_src.shape) * 0.003) @ R.T + t + off)
        gt, pred = f32(np.stack(gt)), f32(np.stack(pred))
        res = ref_pm.get_point_metrics(torch.from_numpy(gt), torch.from_numpy(pred))
        rec[f"point_{tag}_in_gt"], rec[f"point_{tag}_in_pred"] = gt, pred
        for k in ("chamfer_dists", "add-s", "verts_dists"):
            rec[f"point_{tag}_out_{k}"] = np.asarray(res[k], np.float64)
    # ---- get_align_metrics at 1 and 2 hands per frame: the prediction is the ground truth (hands and object) under one
    # per-frame map a * p + t (off in scale and translation) plus noise, the object prediction a resampled surface
    mirror = hand * np.array([-1.0, 1.0, 1.0]) + np.array([0.12, 0.0, 0.0])
    for hands, frames in ((1, 3), (2, 2)):
        gt_h, pred_h, gt_o, pred_o = [], [], [], []
        for _ in range(frames):
            R, t = _rot(rng), rng.normal(size=3) * 0.05 + np.array([0.0, 0.0, 0.5])
            a, t2 = 1.0 + rng.uniform(0.05, 0.25), rng.normal(size=3) * 0.04
            for h in range(hands):
                g = (hand if h == 0 else mirror) @ R.T + t
                gt_h.append(g)
                pred_h.append(a * (g + rng.normal(size=g.shape) * 0.002) + t2)
            og = obj @ R.T + t + np.array([0.05, 0.02, 0.0])
            gt_o.append(og)
            pred_o.append(a * ((obj_rs + rng.normal(size=obj_rs.shape) * 0.002) @ R.T + t + np.array([0.05, 0.02, 0.0])) + t2)
        arrs = [f32(np.stack(x)) for x in (gt_h, pred_h, gt_o, pred_o)]
        res = ref_pm.get_align_metrics(*[torch.from_numpy(x) for x in arrs])
        tag = f"align_h{hands}"
        for name, x in zip(("gt_hand", "pred_hand", "gt_obj", "pred_obj"), arrs):
            rec[f"{tag}_in_{name}"] = x
        for k in ("hand_mean_aligned", "obj_chamfer_aligned"):
            rec[f"{tag}_out_{k}"] = np.asarray(res[k], np.float64)
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
