"""CPU checks of the hand initialisation from keypoints: the float32 restatement of hm_keypoint_terms_clips against float64
autograd, the regressor's rows, the initial translation on a pinhole case, the new prototypes, the Python layer's argument
checks, and the restatement's whole fit on the scene the GPU tests share (tests/handinit_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

from homan_amd import handinit, lib
from homan_amd.mano_assets import hand_models, synthetic_mano
from homan_amd.postprocess import JOINT_ORDER, TIP_VERTS
from tests import handinit_ref as ref


@pytest.mark.parametrize("N,clip_len,with3d", [(3, 3, False), (6, 2, True)])
def test_restatement_gradient_matches_float64_autograd(N, clip_len, with3d):
    inp = ref.random_inputs(N, clip_len, seed=N, with3d=with3d)
    got = ref.keypoint_terms_f32(inp["verts"], inp["W"], inp["camintr"], inp["kp2d"], inp["c2"], inp["s"], inp["kp3d"], inp["c3"],
                                 ref.SIGMA, ref.ZNEAR, 1.0, 100.0, clip_len)
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))
    vh = t(inp["verts"]).requires_grad_(True)
    L2, L3, X = ref.terms_torch(vh, t(inp["W"]), t(inp["camintr"]), t(inp["kp2d"]), t(inp["c2"]), t(inp["s"]), t(inp["kp3d"]),
                                t(inp["c3"]), ref.SIGMA, ref.ZNEAR, clip_len)
    (1.0 * L2 + 100.0 * L3).sum().backward()
    g = vh.grad.numpy()
    assert np.isfinite(got["unit_grad"]).all() and np.isfinite(got["out"]).all()
    # float32 against float64: a few dozen roundings (2^-24 each) along each of the 63 dot products and the per-keypoint chain
    np.testing.assert_allclose(got["keypoints"], X.detach().numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(got["out"][:, 0], L2.detach().numpy(), rtol=2e-5)
    np.testing.assert_allclose(got["out"][:, 1], L3.detach().numpy(), rtol=2e-5, atol=1e-12)
    np.testing.assert_allclose(got["unit_grad"], g, rtol=0, atol=2e-5 * np.abs(g).max())


def test_regressor_rows():
    for side, m in hand_models(synthetic_mano(0)).items():
        W = handinit.keypoint_regressor(m)
        assert W.shape == (21, 778) and W.dtype == np.float32
        stacked = np.zeros((21, 778), np.float32)
        stacked[:16] = m["J_regressor"]
        for i, v in enumerate(TIP_VERTS):
            stacked[16 + i, v] = 1.0
        for k, src in enumerate(JOINT_ORDER):
            assert np.array_equal(W[k], stacked[src]), (side, k)
        tips = [k for k, src in enumerate(JOINT_ORDER) if src >= 16]
        assert tips == [4, 8, 12, 16, 20]
        for k in tips:
            assert W[k].sum() == 1.0 and (W[k] != 0).sum() == 1


def test_initial_translation_on_a_pinhole_case():
    """fronto-parallel keypoints at one depth: the translation is recovered exactly (up to float32 rounding)"""
    rng = np.random.default_rng(0)
    tmpl = torch.from_numpy(np.concatenate([rng.uniform(-0.08, 0.08, size=(21, 2)), np.zeros((21, 1))], 1).astype(np.float32))
    K = torch.tensor([[400.0, 0, 130.0], [0, 400.0, 110.0], [0, 0, 1.0]])
    t = torch.tensor([0.03, -0.02, 0.55])
    p = tmpl + t
    kp2d = torch.stack([K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]], -1)
    c2 = torch.ones(21)
    z, x, y = handinit.initial_translation(kp2d, c2, K, tmpl)
    np.testing.assert_allclose([float(x), float(y), float(z)], t.numpy(), rtol=0, atol=2e-6)
    # a missing detection with a NaN target changes nothing that it should not; no confident keypoint: the neutral start
    kp2d[3], c2[3] = float("nan"), 0.0
    z2, x2, y2 = handinit.initial_translation(kp2d, c2, K, tmpl)
    assert all(np.isfinite(float(v)) for v in (z2, x2, y2)) and abs(float(z2) - 0.55) < 0.05
    z0, x0, y0 = handinit.initial_translation(kp2d, torch.zeros(21), K, tmpl)
    assert (float(z0), float(x0), float(y0)) == (1.0, 0.0, 0.0)
    s = handinit.box_scales(kp2d[None], c2[None])
    ok = c2 > 0
    assert float(s) == float(max(kp2d[ok, 0].max() - kp2d[ok, 0].min(), kp2d[ok, 1].max() - kp2d[ok, 1].min()))
    assert float(handinit.box_scales(kp2d[None], torch.zeros(1, 21))) == 1.0


def test_new_prototypes_use_the_closed_type_tables():
    VP, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert lib._SIGNATURES["hm_keypoint_terms_clips"] == (I, [VP] * 8 + [Fl] * 4 + [I, I] + [VP] * 5 + [I, VP])
    assert lib._SIGNATURES["hm_handinit_finish_clips"] == (I, [VP, VP, I, I, VP, I] + [Fl] * 5 + [VP, I, VP, VP])
    text = open(lib._build.HEADER).read()
    for name in ("hm_keypoint_terms_clips", "hm_handinit_finish_clips"):
        params = text.split("int " + name + "(")[1].split(")")[0]
        for p in params.split(","):
            assert "workspace" not in p and not p.split()[-1].lstrip("*").startswith("ws_"), p


def test_python_layer_argument_checks():
    kp = np.zeros((3, 1, 21, 2), np.float32)
    K = np.eye(3, dtype=np.float32)
    with pytest.raises(ValueError):
        handinit.fit_hands_to_keypoints(kp[:, :, :20], K, ["right"])
    with pytest.raises(ValueError):
        handinit.fit_hands_to_keypoints(kp, K, ["right", "left"])
    with pytest.raises(ValueError):
        handinit.fit_hands_to_keypoints(kp, K, ["middle"])
    with pytest.raises(ValueError):
        handinit.fit_hands_to_keypoints(kp, K, ["right"], confidences=np.ones((3, 1, 20)))
    with pytest.raises(ValueError):
        handinit.fit_hands_to_keypoints(kp, K, ["right"], confidences3d=np.ones((3, 1, 21)))
    with pytest.raises(ValueError):
        handinit.fit_hands_to_keypoints(kp, K, ["right"], rotations_init=np.eye(3))
    with pytest.raises(ValueError):
        handinit.fit_hands_to_keypoints(kp, K, ["right"], loss_weights={"lw_nonsense": 1.0})
    with pytest.raises(ValueError):
        handinit.fit_hands_to_keypoints(kp, K, ["right"], loss_weights={"lw_kp2d": -1.0})
    if not torch.cuda.is_available():              # no fallback: valid arguments raise without a GPU
        with pytest.raises(lib.HomanAmdError):
            handinit.fit_hands_to_keypoints(kp, K, ["right"], mano_model=synthetic_mano(0))
        with pytest.raises(lib.HomanAmdError):
            handinit.HandKeypointFitter(synthetic_mano(0), "right", 3, 2)
    cands = handinit.default_candidates()
    assert cands.shape == (8, 3, 3)
    for R in cands:
        assert torch.equal(R @ R.T, torch.eye(3)) and float(torch.det(R)) == 1.0
    assert len({tuple(R.reshape(-1).tolist()) for R in cands}) == 8 and torch.equal(cands[0], torch.eye(3))


def test_linear_keypoints_against_posed_kinematic_joints():
    """The keypoints are a LINEAR map of the posed vertices, not the posed kinematic joints `postprocess` exports: the largest
    distance between the two on the synthetic model over the scene's poses and the kernel tests' random poses is measured
    here (printed; DESIGN.md section 7 quotes it).  The finger tips are vertices in both and agree exactly."""
    mano = ref.Mano(synthetic_mano(0), "right", torch.float64)
    rng = np.random.default_rng(5)
    pca = np.zeros((70, 45))
    pca[:, :16] = rng.normal(size=(70, 16)) * 0.5
    pca[:3] = ref.scene()["gt"]["pca"]
    with torch.no_grad():
        verts, joints = mano(torch.from_numpy(pca), torch.zeros(70, 10, dtype=torch.float64))
    X = torch.einsum("kv,nvc->nkc", mano.W, verts).numpy()
    J = torch.cat([joints, verts[:, list(TIP_VERTS)]], 1)[:, list(JOINT_ORDER)].numpy()
    d = np.linalg.norm(X - J, axis=-1)
    print("largest |linear keypoint - posed joint| = %.3f mm (mean %.3f mm)" % (1e3 * d.max(), 1e3 * d.mean()))
    assert np.array_equal(X[:, [4, 8, 12, 16, 20]], J[:, [4, 8, 12, 16, 20]])
    assert np.isfinite(d).all() and d.max() > 0          # a measurement, not a bound: the two are different points


def test_restatement_recovers_the_pose_and_separates_the_candidates():
    """the scene of the GPU tests (B = 3, C = 2, a start a quarter turn off, 30 steps): the fit works and the selection is not
    a coin toss at float32"""
    sc, r64, r32 = ref.scene_fits()
    first = ref.px_error(dict(keypoints=r64["keypoints0"]), sc, cand=r64["candidate"])
    last = ref.px_error(r64, sc)
    dev = np.abs(r64["vals"] - r32["vals"]).max()
    bar = 4 * dev + 1e-6
    totals = np.sort(r64["vals"][:, 7])
    print("2-D error (box units) %.4f -> %.4f; candidate %d; totals %s; float32 deviation %.3g, bar %.3g, margin %.3g"
          % (first, last, r64["candidate"], r64["vals"][:, 7], dev, bar, totals[1] - totals[0]))
    assert last < 0.5 * first
    assert totals[1] - totals[0] > 100 * bar
    assert r32["candidate"] == r64["candidate"]
    assert np.isfinite(r64["log"]).all() and r64["log"].shape == (ref.STEPS, sc["C"], 8)
