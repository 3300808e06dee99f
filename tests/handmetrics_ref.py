"""The hand protocol's metrics (include/homan_amd.h, "hand protocol metrics") restated in float64 NumPy: the yardstick of
tests/test_handmetrics.py and tests/test_handmetrics_gpu.py.  The protocol's own script is not available to this project, so
these lines - not that script - are what the kernels of csrc/evalalign.hip are pinned to."""
import numpy as np

FSCORE_BAR = 1e-15          # F-scores are quotients of small integers formed in double: a last bit at most


def align(pred, gt, mode=0, anchors=(0, 4)):
    """pred, gt (N,3) -> (aligned (N,3) float64, err (N,) float64, (s, R (3,3), t (3,))) with aligned = s * pred @ R.T + t"""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    if mode == 2:
        a, b = anchors
        den = np.linalg.norm(pred[b] - pred[a])
        k = 1.0 if den == 0 else np.linalg.norm(gt[b] - gt[a]) / den
        aligned = k * (pred - pred[a]) + gt[a]
        s, R, t = k, np.eye(3), gt[a] - k * pred[a]
    else:
        mu_g, mu_p = gt.mean(0), pred.mean(0)
        s1, s2 = np.linalg.norm(gt - mu_g) + 1e-8, np.linalg.norm(pred - mu_p) + 1e-8
        a, b = (gt - mu_g) / s1, (pred - mu_p) / s2
        U, S, Vt = np.linalg.svd(b.T @ a)
        if mode == 0:
            try:
                from scipy.linalg import orthogonal_procrustes
            except ImportError:
                orthogonal_procrustes = None
            if orthogonal_procrustes is not None:      # scipy's (R, scale) maps its first argument onto its second
                Rs, ss = orthogonal_procrustes(b, a)
                resid = np.linalg.norm(b @ Rs - a)
                assert abs(np.linalg.norm(b @ (U @ Vt) - a) - resid) <= 1e-12 and abs(ss - S.sum()) <= 1e-12
        if mode == 1 and np.linalg.det(U @ Vt) < 0:
            U, S = U.copy(), S.copy()
            U[:, -1] = -U[:, -1]
            S[-1] = -S[-1]
        Q, sigma = U @ Vt, S.sum()
        aligned = (b @ Q) * sigma * s1 + mu_g
        s = sigma * s1 / s2
        R, t = Q.T, mu_g - s * (mu_p @ Q)
    return aligned, np.linalg.norm(aligned - gt, axis=-1), (s, R, t)


def thresholds(val_max, steps):
    return np.linspace(0, val_max, steps)


def threshold_counts(dist, val_max, steps):
    """counts[k] = #(dist_i <= t_k) by direct comparison; NaN compares false everywhere"""
    dist = np.asarray(dist, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return np.array([int(np.count_nonzero(dist <= t)) for t in thresholds(val_max, steps)], np.uint64)


def auc(counts, n, val_max, steps):
    """area under PCK = counts / n over the thresholds, over val_max"""
    pck = np.asarray(counts, np.float64) / float(n)
    t = thresholds(val_max, steps)
    return float(np.sum((pck[1:] + pck[:-1]) * np.diff(t)) / 2.0 / val_max)


def nn_d2(x, y):
    """brute-force squared fp32 nearest-neighbour distances x -> y, formed as hm_cloud_metrics states: (dx*dx + dy*dy) + dz*dz"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    d = x[:, None, :] - y[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    return d2.min(1)


def fscore_from_d2(x_d2, y_d2, ths):
    """(T,3) float64 {precision, recall, F}: strict <, distances sqrt of the fp32 squares in double, thresholds fp32"""
    dx, dy = np.sqrt(np.asarray(x_d2, np.float32).astype(np.float64)), np.sqrt(np.asarray(y_d2, np.float32).astype(np.float64))
    out = []
    for th in np.asarray(ths, np.float32).astype(np.float64):
        p, r = np.count_nonzero(dx < th) / float(dx.size), np.count_nonzero(dy < th) / float(dy.size)
        out.append((p, r, 2.0 * p * r / (p + r) if p + r > 0 else 0.0))
    return np.array(out, np.float64)


def fscore(pred, gt, ths):
    """pred (N,3) = x, gt (M,3) = y"""
    return fscore_from_d2(nn_d2(pred, gt), nn_d2(gt, pred), ths)


def hand_protocol_metrics(gt_joints, pred_joints, gt_verts, pred_verts, f_thresholds=(0.005, 0.015), auc_max=0.05, auc_steps=100,
                          anchors=(0, 4)):
    """the table of homan_amd.handmetrics.get_hand_protocol_metrics by a loop over the frames"""
    out = {}
    for name, gt, pred in (("xyz", gt_joints, pred_joints), ("mesh", gt_verts, pred_verts)):
        gt32, pred32 = np.asarray(gt, np.float32), np.asarray(pred, np.float32)
        raw = np.linalg.norm(pred32.astype(np.float64) - gt32.astype(np.float64), axis=-1)
        for tag, err in (("", raw), ("_al", np.stack([align(p, g, 0)[1] for p, g in zip(pred32, gt32)])),
                         ("_sc_tr", np.stack([align(p, g, 2, anchors)[1] for p, g in zip(pred32, gt32)]))):
            out[f"{name}{tag}_mean3d"] = float(err.mean())
            out[f"{name}{tag}_auc"] = auc(threshold_counts(err, auc_max, auc_steps), err.size, auc_max, auc_steps)
            out[f"{name}{tag}_err"] = err
    gt32, pred32 = np.asarray(gt_verts, np.float32), np.asarray(pred_verts, np.float32)
    al32 = np.stack([align(p, g, 0)[0] for p, g in zip(pred32, gt32)]).astype(np.float32)
    for tag, pr in (("f", pred32), ("f_al", al32)):
        tab = np.stack([fscore(p, g, f_thresholds) for p, g in zip(pr, gt32)])            # (B,T,3)
        for t, th in enumerate(f_thresholds):
            key = f"{tag}@{round(th * 1000):d}"
            out[f"{key}_frames"] = tab[:, t, 2]
            out[key] = float(tab[:, t, 2].mean())
    return out
