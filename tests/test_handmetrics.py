"""CPU checks of the hand protocol metrics: the known answers of the float64 restatement (tests/handmetrics_ref.py) that the
kernels of csrc/evalalign.hip are pinned to, and the argument checks of the wrappers that need no device."""
import inspect

import numpy as np
import pytest
import torch

from tests import handmetrics_ref as ref


def _rotation(rng, proper=True):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if (np.linalg.det(q) < 0) == proper:
        q[:, 0] = -q[:, 0]
    return q


def _hand(rng, n=21):
    return rng.normal(size=(n, 3)) * 0.08 + np.array([0.05, -0.1, 0.6])


def test_similarity_transform_aligns_back_and_returns_its_scale():
    rng = np.random.default_rng(0)
    for mode in (0, 1):
        gt = _hand(rng)
        R, s, t = _rotation(rng), 1.7, np.array([0.3, -0.2, 0.1])
        pred = s * gt @ R.T + t
        aligned, err, (s_fit, R_fit, t_fit) = ref.align(pred, gt, mode)
        # the 1e-8 added to both norms leaves aligned - mu_g = (gt - mu_g) |b|^2 with |b| = 1 - 1e-8 / s2: err_i = |gt_i - mu_g|
        # (1 - |b|^2) <= s1 * 2e-8 / s2 = 2e-8 / s, and 1e-7 relative in the scale
        assert err.max() < 2.1e-8 / s and np.abs(aligned - gt).max() < 2.1e-8 / s
        assert abs(s_fit - 1 / s) < 1e-7
        np.testing.assert_allclose(R_fit, R.T, atol=1e-12)
        np.testing.assert_allclose(s_fit * pred @ R_fit.T + t_fit, aligned, atol=1e-15)


def test_mirrored_set_aligns_in_mode_0_and_not_in_mode_1():
    rng = np.random.default_rng(1)
    gt = _hand(rng)
    pred = 0.8 * gt @ _rotation(rng, proper=False).T + np.array([0.0, 0.1, -0.2])
    _, err0, (_, R0, _) = ref.align(pred, gt, 0)
    _, err1, (_, R1, _) = ref.align(pred, gt, 1)
    assert err0.max() < 2.1e-8 / 0.8 and np.linalg.det(R0) == pytest.approx(-1.0, abs=1e-12)
    assert err1.mean() > 1e-3 and np.linalg.det(R1) == pytest.approx(1.0, abs=1e-12)


def test_scale_trans_maps_the_anchor_and_keeps_the_anchor_distance():
    rng = np.random.default_rng(2)
    gt, pred = _hand(rng), _hand(rng) * 1.3
    for a, b in ((0, 4), (7, 2)):
        aligned, err, (k, R, t) = ref.align(pred, gt, 2, (a, b))
        np.testing.assert_allclose(aligned[a], gt[a], atol=1e-16)
        assert err[a] < 1e-16
        assert np.linalg.norm(aligned[b] - aligned[a]) == pytest.approx(np.linalg.norm(gt[b] - gt[a]), rel=1e-14)
        assert np.array_equal(R, np.eye(3)) and k == pytest.approx(np.linalg.norm(gt[b] - gt[a]) / np.linalg.norm(pred[b] - pred[a]))
    coincident = pred.copy()
    coincident[4] = coincident[0]
    assert ref.align(coincident, gt, 2, (0, 4))[2][0] == 1.0


def test_one_point_aligns_onto_the_ground_truth():
    aligned, err, _ = ref.align([[0.1, 0.2, 0.3]], [[-1.0, 0.5, 2.0]], 0)
    assert np.array_equal(aligned, [[-1.0, 0.5, 2.0]]) and err[0] == 0


def test_auc_of_zero_distances_is_one_and_of_far_distances_zero():
    for steps in (2, 100, 1024):
        counts = ref.threshold_counts(np.zeros(37), 0.05, steps)
        assert counts.tolist() == [37] * steps and ref.auc(counts, 37, 0.05, steps) == pytest.approx(1.0, abs=1e-15)
        far = np.full(37, np.nextafter(0.05, 1.0))
        counts = ref.threshold_counts(far, 0.05, steps)
        assert counts.tolist() == [0] * steps and ref.auc(counts, 37, 0.05, steps) == 0.0
    edge = ref.threshold_counts([0.05, np.nan, -0.0, 0.025], 0.05, 3)
    assert edge.tolist() == [1, 2, 3]
    from homan_amd import handmetrics
    assert handmetrics.auc_from_counts(edge, 4, 0.05, 3) == ref.auc(edge, 4, 0.05, 3) == pytest.approx((0.25 + 1.0 + 0.75) / 4)


def test_fscore_of_identical_clouds_is_one_and_of_far_clouds_zero():
    rng = np.random.default_rng(3)
    cloud = _hand(rng, 65)
    assert np.array_equal(ref.fscore(cloud, cloud, (0.005, 0.015)), np.ones((2, 3)))
    assert np.array_equal(ref.fscore(cloud, cloud + 10.0, (0.005, 0.015)), np.zeros((2, 3)))
    # strict <: a distance equal to the threshold does not count
    th = np.float32(0.25)
    tab = ref.fscore_from_d2(np.array([th * th, 0.0], np.float32), np.array([0.0], np.float32), [th])
    assert tab.tolist() == [[0.5, 1.0, 2.0 * 0.5 * 1.0 / 1.5]]


def test_wrappers_refuse_bad_arguments_before_they_need_the_device():
    from homan_amd import handmetrics, ho3deval, ops
    good = torch.zeros(2, 5, 3)
    for pred, gt in ((torch.zeros(2, 5, 2), good), (torch.zeros(5, 3), torch.zeros(5, 3)), (torch.zeros(2, 4, 3), good),
                     (torch.zeros(0, 5, 3), torch.zeros(0, 5, 3)), (torch.zeros(2, 0, 3), torch.zeros(2, 0, 3)),
                     (good.long(), good)):
        with pytest.raises(ValueError):
            ops.procrustes_align(pred, gt)
    with pytest.raises(ValueError):
        ops.procrustes_align(good, good, mode=3)
    with pytest.raises(ValueError):
        ops.procrustes_align(good, good, mode="affine")
    for anchors in ((0, 5), (-1, 4), (5, 0)):
        with pytest.raises(ValueError):
            ops.procrustes_align(good, good, mode=2, anchors=anchors)
    for steps in (1, 1025):
        with pytest.raises(ValueError):
            ops.threshold_counts(torch.zeros(4), 0.05, steps)
    for val_max in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.threshold_counts(torch.zeros(4), val_max, 100)
    with pytest.raises(ValueError):
        ops.threshold_counts(torch.zeros(4, dtype=torch.int32), 0.05, 100)
    d2 = torch.zeros(2, 5)
    for ths in ((), (0.001,) * 9):
        with pytest.raises(ValueError):
            ops.fscore(d2, d2, ths)
    for x, y in ((d2.double(), d2), (torch.zeros(5), d2), (d2, torch.zeros(3, 5)), (torch.zeros(2, 0), d2)):
        with pytest.raises(ValueError):
            ops.fscore(x, y, (0.005,))
    with pytest.raises(ValueError):
        handmetrics.align(good, good, mode="procrustes")
    with pytest.raises(ValueError):
        handmetrics.align(good, torch.zeros(2, 4, 3))
    joints, verts = np.zeros((2, 21, 3)), np.zeros((2, 778, 3))
    with pytest.raises(ValueError):
        handmetrics.get_hand_protocol_metrics(joints, joints, verts, np.zeros((2, 777, 3)))
    with pytest.raises(ValueError):
        handmetrics.get_hand_protocol_metrics(joints, joints, verts[:1], verts[:1])
    with pytest.raises(ValueError):
        handmetrics.get_hand_protocol_metrics(joints, joints, verts, verts, f_thresholds=())
    with pytest.raises(ValueError):
        handmetrics.get_object_auc(np.zeros((2, 8, 3)), np.zeros((3, 8, 3)))
    # the sequence evaluation keeps its signature; the protocol's arguments live on its sibling
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(ho3deval.evaluate_sequence_protocol) == params(ho3deval.evaluate_sequence) + ["gt_hand_joints", "gt_hand_verts",
                                                                                               "anchors"]
    assert params(handmetrics.get_hand_protocol_metrics) == ["gt_joints", "pred_joints", "gt_verts", "pred_verts", "f_thresholds",
                                                             "auc_max", "auc_steps", "anchors"]
    assert inspect.signature(handmetrics.align).parameters["anchors"].default == (0, 4)
    if not torch.cuda.is_available():            # no CPU path
        with pytest.raises(RuntimeError):
            handmetrics.align(good, good)


def test_library_refuses_bad_arguments_without_a_launch():
    """made-up device addresses: every call here must fail its host checks before anything is enqueued (HM_ERR_BAD_ARG = -1)"""
    import ctypes
    from homan_amd import lib
    h, p = lib.lib(), 1 << 20
    assert h.hm_procrustes_align(p, p, 0, 4, 0, 0, 0, p, p, p, None) == -1
    assert h.hm_procrustes_align(p, p, 1, 0, 0, 0, 0, p, p, p, None) == -1
    assert h.hm_procrustes_align(None, p, 1, 4, 0, 0, 0, p, p, p, None) == -1
    assert h.hm_procrustes_align(p, None, 1, 4, 0, 0, 0, p, p, p, None) == -1
    assert h.hm_procrustes_align(p, p, 1, 4, 3, 0, 0, p, p, p, None) == -1
    assert h.hm_procrustes_align(p, p, 1, 4, 2, 0, 4, p, p, p, None) == -1
    assert h.hm_procrustes_align(p, p, 1, 4, 2, -1, 3, p, p, p, None) == -1
    vmax = ctypes.c_double(0.05)
    for steps in (1, 1025):
        assert h.hm_threshold_counts(p, 4, 0, ctypes.addressof(vmax), steps, p, None) == -1
    assert h.hm_threshold_counts(None, 4, 0, ctypes.addressof(vmax), 100, p, None) == -1
    assert h.hm_threshold_counts(p, -1, 0, ctypes.addressof(vmax), 100, p, None) == -1
    assert h.hm_threshold_counts(p, 4, 0, None, 100, p, None) == -1
    zero = ctypes.c_double(0.0)
    assert h.hm_threshold_counts(p, 4, 0, ctypes.addressof(zero), 100, p, None) == -1
    ths = (ctypes.c_float * 9)(*([0.005] * 9))
    for T in (0, 9):
        assert h.hm_fscore(p, p, 1, 4, 4, ctypes.addressof(ths), T, p, None) == -1
    assert h.hm_fscore(p, p, 0, 4, 4, ctypes.addressof(ths), 2, p, None) == -1
    assert h.hm_fscore(p, p, 1, 0, 4, ctypes.addressof(ths), 2, p, None) == -1
    assert h.hm_fscore(p, None, 1, 4, 4, ctypes.addressof(ths), 2, p, None) == -1
    assert h.hm_fscore(p, p, 1, 4, 4, None, 2, p, None) == -1


_SVD_HOST = r'''
#include "evalalign.hip"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)            /* in.bin out.bin proper: 9 doubles per matrix in, Q (9) and trace S out */
{
    if (argc != 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    double m[9];
    while (fread(m, sizeof(double), 9, in) == 9) {
        double M[3][3], Q[3][3], sigma;
        for (int i = 0; i < 9; ++i) M[i / 3][i % 3] = m[i];
        ea_procrustes_q(M, atoi(argv[3]) != 0, Q, &sigma);
        fwrite(&Q[0][0], sizeof(double), 9, out);
        fwrite(&sigma, sizeof(double), 1, out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
'''


def test_written_out_svd_on_the_host_matches_numpy(tmp_path):
    """The 3x3 Jacobi SVD of csrc/evalalign.hip is a __host__ __device__ routine: built into a host program, its Q = U V^T must
    be orthogonal and reach trace(Q^T M) = sum of the singular values (mode 1: the smallest negated when det(U V^T) < 0) on full
    rank, graded, rank 2, rank 1 and zero matrices.  Bars: 1e-14, a few dozen roundings of 1.1e-16 on entries of modulus <= 1."""
    import subprocess
    from homan_amd import build
    rng = np.random.default_rng(0)
    mats = [rng.normal(size=(3, 3)) for _ in range(300)]
    mats += [rng.normal(size=(3, 3)) * np.array([1, 1e-3, 1e-9]) for _ in range(50)]
    for _ in range(50):
        mats.append(rng.normal(size=(3, 2)) @ rng.normal(size=(2, 3)))
        mats.append(rng.normal(size=(3, 1)) @ rng.normal(size=(1, 3)))
    mats += [np.zeros((3, 3)), np.eye(3), -np.eye(3), np.diag([1.0, 1.0, 0.0]), np.diag([0.0, 0.0, 1.0]), np.diag([2.0, 0.0, 0.0]),
             np.ones((3, 3)), np.diag([1.0, 1.0, -1.0]), np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, 1]]), np.diag([0.0, 3.0, 0.0])]
    mats = np.array(mats)
    (tmp_path / "svd_host.cpp").write_text(_SVD_HOST)
    mats.tofile(tmp_path / "in.bin")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([build.HIPCC] + flags + ["-I", build.CSRC, "-I", build.INCLUDE, "-x", "hip", str(tmp_path / "svd_host.cpp"),
                        "-o", str(tmp_path / "svd_host")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for proper in (0, 1):
        subprocess.run([str(tmp_path / "svd_host"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(proper)], check=True)
        out = np.fromfile(tmp_path / "out.bin").reshape(-1, 10)
        assert out.shape[0] == mats.shape[0] and np.isfinite(out).all()
        for M, row in zip(mats, out):
            Q, sigma = row[:9].reshape(3, 3), row[9]
            U, S, Vt = np.linalg.svd(M)
            if proper and np.linalg.det(U @ Vt) < 0:
                S[-1] = -S[-1]
            scale = max(S[0], 1.0)
            assert abs(np.trace(Q.T @ M) - S.sum()) <= 1e-14 * scale and abs(sigma - S.sum()) <= 1e-14 * scale
            assert np.abs(Q.T @ Q - np.eye(3)).max() <= 1e-14
            if proper:
                assert abs(np.linalg.det(Q) - 1) <= 1e-14
