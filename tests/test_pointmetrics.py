"""Evaluation metrics (homan_amd/pointmetrics.py), CPU side: a torch restatement of reference homan/eval/pointmetrics.py
pinned to the reference's own outputs (tests/golden/pointmetrics_reference.npz, written by
tools/refharness/gen_goldens_pointmetrics.py), the public signatures, and the refusal to run without a GPU.
The GPU tests compare the kernels against this restatement."""
import importlib.util
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pointmetrics_reference.npz")
GENERATOR = os.path.join(ROOT, "tools", "refharness", "gen_goldens_pointmetrics.py")


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def chamfer64(x, y):
    """pytorch3d chamfer_distance(x, y, batch_reduction=None)[0] with its defaults, in float64 (as the generator's shim)"""
    d2 = ((x.double()[:, :, None, :] - y.double()[:, None, :, :]) ** 2).sum(-1)
    return d2.min(2)[0].mean(1) + d2.min(1)[0].mean(1)


def restate_point_metrics(gt, pred):
    """reference pointmetrics.py:17-44: chamfer (float64 shim), ADD-S (cKDTree: float64 distances), vertex error (fp32)"""
    gt, pred = torch.as_tensor(gt), torch.as_tensor(pred)
    adds = (gt.double()[:, :, None, :] - pred.double()[:, None, :, :]).norm(dim=-1).min(2)[0].mean(1)
    verts = (gt - pred).norm(2, -1).mean(-1) if gt.shape[1] == pred.shape[1] else adds
    return {"chamfer_dists": chamfer64(gt, pred).tolist(), "add-s": adds.tolist(), "verts_dists": verts.tolist()}


def restate_align_metrics(gt_hand, pred_hand, gt_obj, pred_obj, pred_centroid_from_gt=True):
    """reference pointmetrics.py:61-99 in fp32 (chamfer in float64); pred_centroid_from_gt=False centres the prediction on
    its own first hand"""
    gt_hand, pred_hand, gt_obj, pred_obj = [torch.as_tensor(t) for t in (gt_hand, pred_hand, gt_obj, pred_obj)]
    h = gt_hand.shape[0] // gt_obj.shape[0]
    gt_cent = gt_hand[::h].mean(1, keepdim=True)
    pred_cent = (gt_hand if pred_centroid_from_gt else pred_hand)[::h].mean(1, keepdim=True)
    rep = lambda t: t.repeat(1, h, 1).view(h * t.shape[0], -1, t.shape[-1])  # noqa: E731
    gt_hand_c, gt_obj_c = gt_hand - rep(gt_cent), gt_obj - gt_cent
    pred_hand_c, pred_obj_c = pred_hand - rep(pred_cent), pred_obj - pred_cent
    gt_scale = torch.sqrt((gt_hand_c[::h].norm(2, -1) ** 2).sum(1) / gt_hand.shape[1])
    pred_scale = torch.sqrt((pred_hand_c[::h].norm(2, -1) ** 2).sum(1) / pred_hand.shape[1])
    pred_hand_cs = pred_hand_c / rep(pred_scale[:, None, None]) * rep(gt_scale[:, None, None])
    pred_obj_cs = pred_obj_c / pred_scale[:, None, None] * gt_scale[:, None, None]
    return {"hand_mean_aligned": (gt_hand_c - pred_hand_cs).norm(2, -1).mean(-1).tolist(),
            "obj_chamfer_aligned": chamfer64(pred_obj_cs, gt_obj_c).tolist()}


def golden_cases(g):
    """[(function name, inputs, reference outputs)] of the golden file"""
    cases = []
    for tag in ("eq", "neq"):
        ins = [g[f"point_{tag}_in_{n}"] for n in ("gt", "pred")]
        cases.append(("point", tag, ins, {k: g[f"point_{tag}_out_{k}"] for k in ("chamfer_dists", "add-s", "verts_dists")}))
    for tag in ("align_h1", "align_h2"):
        ins = [g[f"{tag}_in_{n}"] for n in ("gt_hand", "pred_hand", "gt_obj", "pred_obj")]
        cases.append(("align", tag, ins, {k: g[f"{tag}_out_{k}"] for k in ("hand_mean_aligned", "obj_chamfer_aligned")}))
    return cases


def test_restatement_reproduces_reference_golden():
    g = load_golden()
    for kind, tag, ins, want in golden_cases(g):
        got = (restate_point_metrics if kind == "point" else restate_align_metrics)(*[torch.from_numpy(a) for a in ins])
        assert set(got) == set(want), tag
        for k, v in want.items():
            np.testing.assert_allclose(got[k], v, rtol=1e-6, atol=0, err_msg=f"{tag} {k}")
    assert g["point_neq_in_gt"].shape[1] != g["point_neq_in_pred"].shape[1]
    assert g["align_h2_in_gt_hand"].shape[0] == 2 * g["align_h2_in_gt_obj"].shape[0]


def _shims():
    spec = importlib.util.spec_from_file_location("_pm_shims", os.path.join(ROOT, "tools", "refharness", "shims.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_reproduces_committed_golden(tmp_path):
    if not os.path.isdir(os.path.join(_shims().REFERENCE_ROOT, "homan")):
        pytest.skip("the reference sources are not on this machine")
    out = str(tmp_path / "pm.npz")
    subprocess.run([sys.executable, GENERATOR, out], check=True, cwd=ROOT, capture_output=True, timeout=600)
    a, b = np.load(GOLDEN), np.load(out)
    assert a.files == b.files
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_signatures_mirror_the_reference():
    from homan_amd import pointmetrics
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(pointmetrics.get_point_metrics) == ["gt_points", "pred_points"]
    assert params(pointmetrics.get_align_metrics) == ["gt_hand_verts", "pred_hand_verts", "gt_obj_verts", "pred_obj_verts",
                                                      "pred_centroid_from_gt"]
    assert inspect.signature(pointmetrics.get_align_metrics).parameters["pred_centroid_from_gt"].default is True
    assert params(pointmetrics.repeat_hand_nb) == ["tens", "hand_nb"]
    assert params(pointmetrics.get_inter_metrics) == ["verts_person", "verts_object", "faces_person", "faces_object"]


def test_repeat_hand_nb_is_frame_major():
    from homan_amd.pointmetrics import repeat_hand_nb
    t = torch.arange(6.0).view(3, 2)
    r = repeat_hand_nb(t, 2)
    assert r.shape == (6, 2, 1)                     # (B, C) -> (B*h, C, 1), as the reference's unsqueeze(2) makes it
    assert torch.equal(r[:, :, 0], t.repeat_interleave(2, 0))
    c = torch.arange(9.0).view(3, 1, 3)
    assert torch.equal(repeat_hand_nb(c, 2), c.repeat_interleave(2, 0))
    assert repeat_hand_nb(torch.arange(3.0), 2).shape == (6, 1, 1)


def test_metrics_refuse_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the metrics run (tests/test_pointmetrics_gpu.py)")
    from homan_amd import pointmetrics
    g = load_golden()
    with pytest.raises(RuntimeError):
        pointmetrics.get_point_metrics(torch.from_numpy(g["point_eq_in_gt"]), torch.from_numpy(g["point_eq_in_pred"]))
    with pytest.raises(RuntimeError):
        pointmetrics.get_align_metrics(*[torch.from_numpy(g[f"align_h1_in_{n}"])
                                         for n in ("gt_hand", "pred_hand", "gt_obj", "pred_obj")])


def test_c_abi_rejects_bad_sizes_and_nulls():
    """hm_cloud_metrics / hm_align_stats check their arguments before any launch (HM_ERR_BAD_ARG = -1)"""
    from homan_amd import lib
    h = lib.lib()
    assert h.hm_cloud_metrics_workspace_bytes(0, 10, 10) == 0
    assert h.hm_cloud_metrics_workspace_bytes(2, 129, 1) == 2 * (2 + 1) * 3 * 8
    p = 1 << 20          # never dereferenced: every call below fails its argument check
    assert h.hm_cloud_metrics(None, p, 1, 4, 4, None, None, None, None, None, None, p, p, None) == -1
    assert h.hm_cloud_metrics(p, p, 1, 0, 4, None, None, None, None, None, None, p, p, None) == -1
    assert h.hm_cloud_metrics(p, p, 1, 4, 4, None, None, None, None, None, None, p, None, None) == -1
    assert h.hm_align_stats(p, p, 1, 0, 778, 1, p, p, p, None) == -1
    assert h.hm_align_stats(p, None, 1, 1, 778, 1, p, p, p, None) == -1
