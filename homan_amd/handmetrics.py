"""The hand evaluation protocol of FreiHAND / HO-3D and the ADD / ADD-S AUC of YCB objects, on the HIP kernels.

What the HO-3D server answers to the `pred.json` that `ho3deval.dump` writes: mean joint and mesh error raw, after a
Procrustes (similarity) alignment and after a scale-and-translation alignment, the AUC of the PCK curve over 0-50 mm, and
F-scores at 5 mm and 15 mm raw and aligned.  An extra beyond the reference, whose `get_align_metrics` only centres on a
centroid.  The protocol's script is not available to this project: the formulas are FIXED HERE (include/homan_amd.h, "hand
protocol metrics") and pinned by the float64 NumPy restatement of tests/handmetrics_ref.py, not by that script (DESIGN.md
section 7).  In particular the anchors of the scale-and-translation alignment default to rows (0, 4) of the set it is given
(wrist and, in HO-3D's joint order, the end of the first chain) and are UNPINNED: pass the pair your protocol uses.

The alignment (`hm_procrustes_align`), the threshold curves (`hm_threshold_counts`) and the F-scores (`hm_fscore`, off the
nearest-neighbour distances of `hm_cloud_metrics`) run on the device, one launch per kernel per call; raw errors are the
element-wise float64 norm of the fp32 inputs.  A frame's values do not depend on the other frames of the call.  There is no
CPU path: without a GPU these functions raise.
"""
import numpy as np
import torch

from . import lib, ops

ALIGN_MODES = ops.ALIGN_MODES
F_THRESHOLDS = (0.005, 0.015)


def _on_gpu(*tensors):
    """The inputs as contiguous fp32 tensors on ONE GPU (the first CUDA input's device, else the current one)."""
    if not torch.cuda.is_available():
        raise lib.HomanAmdError("homan_amd.handmetrics needs the GPU (there is no CPU fallback)")
    tensors = [t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t)) for t in tensors]
    dev = next((t.device for t in tensors if t.is_cuda), torch.device("cuda"))
    return [t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in tensors]


def _check_sets(**sets):
    """(name=(gt, pred)): float (B,N,3) of one shape, non-empty; checked before anything needs the device"""
    frames = None
    for name, (gt, pred) in sets.items():
        shapes = [tuple(np.shape(t)) for t in (gt, pred)]
        for shape in shapes:
            if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
                raise ValueError(f"{name}: expected non-empty (B, N, 3) arrays, got {shapes[0]} and {shapes[1]}")
        if shapes[0] != shapes[1]:
            raise ValueError(f"{name}: ground truth {shapes[0]} and prediction {shapes[1]} differ in shape")
        if frames is not None and shapes[0][0] != frames:
            raise ValueError(f"{name}: {shapes[0][0]} frames, the other set has {frames}")
        frames = shapes[0][0]


def _f_key(prefix, th):
    return f"{prefix}@{round(float(th) * 1000):d}"


def _check_thresholds(f_thresholds):
    ths = tuple(float(t) for t in f_thresholds)
    if not 1 <= len(ths) <= 8:
        raise ValueError(f"between 1 and 8 F-score thresholds, got {len(ths)}")
    if len({_f_key("f", t) for t in ths}) != len(ths):
        raise ValueError(f"F-score thresholds {ths} do not name distinct millimetres")
    return ths


def align(pred, gt, mode="similarity", anchors=(0, 4)):
    """pred, gt (B,N,3) -> (aligned (B,N,3) fp32, err (B,N) float64, xform (B,13) float64 {s, R row-major, t}) on the device,
    aligned = s * pred @ R.T + t.  mode "similarity": best similarity transform with an orthogonal factor (reflections
    allowed, the protocol's `align_w_scale`); "rigid_similarity": with a proper rotation (Kabsch / Umeyama); "scale_trans":
    scale and translation that map row anchors[0] onto the ground truth's and preserve the distance to row anchors[1]."""
    if mode not in ALIGN_MODES:
        raise ValueError(f"mode must be one of {sorted(ALIGN_MODES)}, got {mode!r}")
    _check_sets(points=(gt, pred))
    pred, gt = _on_gpu(pred, gt)
    with torch.cuda.device(pred.device):
        return ops.procrustes_align(pred, gt, ALIGN_MODES[mode], anchors)


def auc_from_counts(counts, n, val_max, steps):
    """PCK = counts / n over t = np.linspace(0, val_max, steps); AUC = trapezoid area under it over val_max (float64)"""
    if n == 0:
        return float("nan")
    pck = np.asarray(counts, np.float64) / float(n)
    t = np.linspace(0, val_max, steps)
    return float(np.sum((pck[1:] + pck[:-1]) * np.diff(t)) / 2.0 / val_max)


def auc(dist, val_max, steps=100):
    """AUC of the curve "share of `dist` at or below t", t over [0, val_max] in `steps` thresholds.  dist: tensor (moved to the
    GPU as it is when fp32 or float64) or array, any shape; NaN entries count as misses."""
    if not isinstance(dist, torch.Tensor):
        dist = torch.as_tensor(np.asarray(dist, np.float64))
    if not torch.cuda.is_available():
        raise lib.HomanAmdError("homan_amd.handmetrics needs the GPU (there is no CPU fallback)")
    if dist.dtype not in (torch.float32, torch.float64):
        dist = dist.double()
    dist = dist if dist.is_cuda else dist.cuda()
    with torch.cuda.device(dist.device):
        counts = ops.threshold_counts(dist, val_max, steps).cpu().numpy()
    return auc_from_counts(counts, dist.numel(), val_max, steps)


def frame_errors(gt, pred, anchors=(0, 4), scale_trans=True):
    """gt, pred (B,N,3) fp32 on the device -> {"": raw, "_al": similarity-aligned, "_sc_tr": scale-and-translation-aligned}
    per-point errors (B,N) float64 on the device, and the similarity-aligned points (B,N,3) fp32."""
    d = pred.double() - gt.double()
    errs = {"": ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).sqrt()}     # (element-wise: one order)
    aligned, errs["_al"], _ = ops.procrustes_align(pred, gt, 0)
    if scale_trans:
        errs["_sc_tr"] = ops.procrustes_align(pred, gt, 2, anchors)[1]
    return errs, aligned


def frame_fscores(gt, pred, thresholds):
    """gt (B,M,3), pred (B,N,3) fp32 on the device -> (B,T) float64 F-scores (prediction = x, ground truth = y)"""
    _, (x_d2, _, y_d2, _) = ops.cloud_metrics(pred, gt, per_point=True)
    return ops.fscore(x_d2, y_d2, thresholds)[:, :, 2]


def get_hand_protocol_metrics(gt_joints, pred_joints, gt_verts, pred_verts, f_thresholds=F_THRESHOLDS, auc_max=0.05, auc_steps=100,
                              anchors=(0, 4)):
    """gt_joints / pred_joints (B,21,3), gt_verts / pred_verts (B,778,3), metres, one frame and joint order -> dict:

      "{xyz|mesh}{|_al|_sc_tr}_mean3d"  mean error over all frames and points: raw, similarity-aligned, scale/translation-aligned
      "{xyz|mesh}{|_al|_sc_tr}_auc"     AUC of the PCK curve over [0, auc_max] in auc_steps thresholds
      "f@5", "f@15", "f_al@5", "f_al@15"  mean over the frames of the per-frame F-score of the meshes (per threshold in mm)
    and beside them the arrays they were formed from: "{...}_err" (B,N) float64 per-point errors, "f@5_frames" ... (B,) float64.
    `anchors` index the rows of the set that is aligned (joints and vertices alike); see the module's note on them."""
    ths = _check_thresholds(f_thresholds)
    _check_sets(joints=(gt_joints, pred_joints), verts=(gt_verts, pred_verts))
    gt_j, pred_j, gt_v, pred_v = _on_gpu(gt_joints, pred_joints, gt_verts, pred_verts)
    out, dev_errs, aligned = {}, {}, {}
    with torch.cuda.device(gt_j.device):
        for name, gt, pred in (("xyz", gt_j, pred_j), ("mesh", gt_v, pred_v)):
            errs, aligned[name] = frame_errors(gt, pred, anchors)
            for tag, err in errs.items():
                dev_errs[f"{name}{tag}"] = (err, ops.threshold_counts(err, auc_max, auc_steps))
        f_tabs = {"f": frame_fscores(gt_v, pred_v, ths), "f_al": frame_fscores(gt_v, aligned["mesh"], ths)}
        for key, (err, counts) in dev_errs.items():
            err = err.cpu().numpy()
            out[f"{key}_mean3d"] = float(err.mean())
            out[f"{key}_auc"] = auc_from_counts(counts.cpu().numpy(), err.size, auc_max, auc_steps)
            out[f"{key}_err"] = err
        for prefix, tab in f_tabs.items():
            tab = tab.cpu().numpy()
            for t, th in enumerate(ths):
                out[_f_key(prefix, th)] = float(tab[:, t].mean())
                out[_f_key(prefix, th) + "_frames"] = np.ascontiguousarray(tab[:, t])
    return out


def get_object_auc(gt_verts, pred_verts, max_dist=0.1, steps=100):
    """gt_verts (B,N,3), pred_verts (B,M,3) -> {"add_auc", "adds_auc", "add" (B,), "adds" (B,)}: per frame ADD = mean_i |g_i -
    p_i| (NaN when N != M, as `hm_cloud_metrics` gives it; its AUC is then NaN) and ADD-S = mean_i min_j |g_i - p_j|, as
    `pointmetrics.get_point_metrics` defines them; the AUC is the area under "share of frames at or below t", t over
    [0, max_dist] in `steps` thresholds, over max_dist."""
    for name, t in (("gt_verts", gt_verts), ("pred_verts", pred_verts)):
        shape = tuple(np.shape(t))
        if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"{name}: expected a non-empty (B, N, 3) array, got {shape}")
    if np.shape(gt_verts)[0] != np.shape(pred_verts)[0]:
        raise ValueError(f"batch sizes differ: {np.shape(gt_verts)[0]} vs {np.shape(pred_verts)[0]}")
    gt, pred = _on_gpu(gt_verts, pred_verts)
    with torch.cuda.device(gt.device):
        tab = ops.cloud_metrics(gt, pred)
        add, adds = tab[:, 3].contiguous(), tab[:, 2].contiguous()
        counts = torch.stack([ops.threshold_counts(add, max_dist, steps), ops.threshold_counts(adds, max_dist, steps)]).cpu().numpy()
        add, adds = add.cpu().numpy(), adds.cpu().numpy()
    paired = gt.shape[1] == pred.shape[1]
    return {"add_auc": auc_from_counts(counts[0], add.size, max_dist, steps) if paired else float("nan"),
            "adds_auc": auc_from_counts(counts[1], adds.size, max_dist, steps), "add": add, "adds": adds}
