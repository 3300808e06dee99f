"""GPU checks of the hand initialisation from keypoints (csrc/handinit.hip, homan_amd/handinit.py): the kernel bit for bit
against the float32 restatement of tests/handinit_ref.py, its edge inputs and argument checks, the fused step against the
autograd step, the whole fit against the float64 restatement, and fit_hands_to_keypoints into build_model."""
import copy

import numpy as np
import pytest
import torch

from homan_amd import handinit, lib
from homan_amd.mano_assets import hand_models, synthetic_mano
from tests import handinit_ref as ref

pytestmark = pytest.mark.gpu
GUARD = -7.25
LW2, LW3 = 1.0, 100.0


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def run_kernel(inp, N, clip_len, sigma=ref.SIGMA, znear=ref.ZNEAR, drop=(), expect=0):
    """hm_keypoint_terms_clips on guard-filled outputs -> (return code, dict of numpy outputs)"""
    dev = torch.device("cuda")
    t = lambda k: None if (inp.get(k) is None or k in drop) else torch.from_numpy(np.ascontiguousarray(inp[k])).to(dev)
    a = {k: t(k) for k in ("verts", "W", "camintr", "kp2d", "c2", "s", "kp3d", "c3")}
    rows = inp["verts"].shape[0]
    C = max(rows // max(clip_len, 1), 1)
    out = dict(keypoints=torch.full((rows, 21, 3), GUARD, device=dev), unit_grad=torch.full((rows, 778, 3), GUARD, device=dev),
               row_parts=torch.full((rows, 2), GUARD, device=dev), out=torch.full((C, 2), GUARD, device=dev))
    tickets = torch.zeros(C, dtype=torch.int32, device=dev)
    P = lib.ptr
    rc = lib.lib().hm_keypoint_terms_clips(P(a["verts"]), P(a["W"]), P(a["camintr"]), P(a["kp2d"]), P(a["c2"]), P(a["s"]), P(a["kp3d"]),
                                           P(a["c3"]), sigma, znear, LW2, LW3, N, clip_len, P(out["keypoints"]), P(out["unit_grad"]),
                                           P(out["row_parts"]), P(tickets), P(out["out"]), 2, lib.stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert int(tickets.abs().sum()) == 0                    # the tickets reset themselves
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def restated(inp, clip_len, sigma=ref.SIGMA, znear=ref.ZNEAR):
    return ref.keypoint_terms_f32(inp["verts"], inp["W"], inp["camintr"], inp["kp2d"], inp["c2"], inp["s"], inp["kp3d"], inp["c3"],
                                  sigma, znear, LW2, LW3, clip_len)


def assert_same_bits(got, want):
    for k in ("keypoints", "row_parts", "out", "unit_grad"):
        diff = bits(got[k]) != bits(want[k])
        assert not diff.any(), (k, int(diff.sum()), np.abs(got[k] - want[k]).max())


@pytest.mark.parametrize("with3d", [False, True])
@pytest.mark.parametrize("N,clip_len", [(1, 1), (3, 3), (5, 1), (6, 2), (70, 7)])
def test_kernel_equals_the_restatement_bit_for_bit(N, clip_len, with3d):
    inp = ref.random_inputs(N, clip_len, seed=100 + N, with3d=with3d)
    _, got = run_kernel(inp, N, clip_len)
    assert np.isfinite(got["unit_grad"]).all() and np.isfinite(got["out"]).all()
    assert_same_bits(got, restated(inp, clip_len))


def test_left_hand_equals_the_restatement():
    inp = ref.random_inputs(6, 2, seed=7, with3d=True, side="left")
    right = handinit.keypoint_regressor(hand_models(synthetic_mano(0))["right"])
    assert np.array_equal(inp["W"], handinit.keypoint_regressor(hand_models(synthetic_mano(0))["left"]))
    assert inp["W"].shape == right.shape
    _, got = run_kernel(inp, 6, 2)
    assert_same_bits(got, restated(inp, 2))


def test_edge_inputs():
    inp = ref.random_inputs(4, 2, seed=3, with3d=True)
    # row 1: no detection at all, NaN targets; clip 1 (rows 2, 3): no confident keypoint in the whole clip
    for r in (1, 2, 3):
        inp["c2"][r], inp["kp2d"][r] = 0.0, np.nan
        inp["c3"][r], inp["kp3d"][r] = 0.0, np.nan
    _, got = run_kernel(inp, 4, 2)
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    assert (got["row_parts"][1:] == 0).all() and (got["unit_grad"][1:] == 0).all()
    assert (got["out"][1] == 0).all() and got["out"][0, 0] > 0 and got["out"][0, 1] > 0
    assert_same_bits(got, restated(inp, 2))
    # every keypoint at z <= znear: the constant cost c2 sigma^2, no 2-D gradient (2-D only: the gradient is zero)
    flat = ref.random_inputs(3, 3, seed=4, with3d=False)
    _, behind = run_kernel(flat, 3, 3, sigma=0.5, znear=10.0)
    assert (behind["unit_grad"] == 0).all()
    assert_same_bits(behind, restated(flat, 3, sigma=0.5, znear=10.0))
    np.testing.assert_allclose(behind["out"][0, 0], 0.25, rtol=1e-6)
    assert behind["out"][0, 1] == 0
    # znear between the keypoints' depths: both branches in one row
    z = restated(flat, 3)["keypoints"][..., 2]
    mid = float(np.median(z))
    _, mixed = run_kernel(flat, 3, 3, znear=mid)
    assert_same_bits(mixed, restated(flat, 3, znear=mid))
    assert (mixed["unit_grad"] != 0).any()


def test_a_clip_alone_equals_the_clip_in_a_batch_and_runs_repeat():
    inp = ref.random_inputs(6, 2, seed=11, with3d=True)
    _, a = run_kernel(inp, 6, 2)
    _, b = run_kernel(inp, 6, 2)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    alone = {k: (v if (v is None or k == "W") else v[2:4]) for k, v in inp.items()}
    _, c = run_kernel(alone, 2, 2)
    for k in ("keypoints", "unit_grad", "row_parts"):
        assert np.array_equal(bits(c[k]), bits(a[k][2:4])), k
    assert np.array_equal(bits(c["out"][0]), bits(a["out"][1]))


@pytest.mark.parametrize("case", ["null_W", "null_kp2d", "only_kp3d", "N_not_multiple", "sigma_zero", "sigma_negative", "N_zero",
                                  "clip_len_zero"])
def test_bad_arguments_leave_the_outputs_untouched(case):
    inp = ref.random_inputs(6, 2, seed=1, with3d=True)
    kw = dict(N=6, clip_len=2)
    drop = {"null_W": ("W",), "null_kp2d": ("kp2d",), "only_kp3d": ("c3",)}.get(case, ())
    if case == "N_not_multiple":
        kw = dict(N=5, clip_len=2)
    elif case == "sigma_zero":
        kw["sigma"] = 0.0
    elif case == "sigma_negative":
        kw["sigma"] = -1.0
    elif case == "N_zero":
        kw["N"] = 0
    elif case == "clip_len_zero":
        kw["clip_len"] = 0
    _, got = run_kernel(inp, drop=drop, expect=-1, **kw)
    for k, v in got.items():
        assert (v == GUARD).all(), k
    # the finishing entry point: same rule
    dev = torch.device("cuda")
    vals, g = torch.full((3, 8), GUARD, device=dev), torch.full((6, 10), GUARD, device=dev)
    betas = torch.zeros(6, 10, device=dev)
    L, P = lib.lib(), lib.ptr
    for args in ((None, P(g), 6, 2, P(vals), 8), (P(betas), P(g), 5, 2, P(vals), 8), (P(betas), P(g), 6, 2, None, 8),
                 (P(betas), P(g), 6, 2, P(vals), 7), (P(betas), P(g), 0, 2, P(vals), 8)):
        assert L.hm_handinit_finish_clips(*args, 1.0, 1.0, 1.0, 1.0, 1.0, None, 0, None, lib.stream()) == -1
    torch.cuda.synchronize()
    assert bool((vals == GUARD).all()) and bool((g == GUARD).all())


def _fitter(sc, mode, **kw):
    fit = handinit.HandKeypointFitter(hand_models(sc["mano"])[sc["side"]], sc["side"], sc["B"], sc["C"], lr=ref.LR, loss_weights=ref.LW,
                                      sigma=ref.SIGMA, znear=ref.ZNEAR, mode=mode, max_steps=64, **kw)
    _load(fit, sc)
    return fit


def _load(fit, sc):
    B, C, d, gt = sc["B"], sc["C"], sc["data"], sc["gt"]
    fit.load(d["kp2d"][:B], d["c2"][:B], d["camintr"][:B], sc["cands"], d["kp3d"][:B] if "kp3d" in d else None,
             d["c3"][:B] if "c3" in d else None)
    # the host start (initial_translation) computed on the device agrees with the CPU's; the fits then start from the SAME floats
    np.testing.assert_allclose(fit.trans.detach().cpu().numpy(), sc["trans0"], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(fit.s.cpu().numpy(), d["s"])
    with torch.no_grad():
        fit.trans.copy_(torch.from_numpy(sc["trans0"]))
        fit.rot6d.copy_(torch.from_numpy(sc["rot6d0"]))


def _params(fit):
    return {k: getattr(fit, k).detach().cpu().numpy().astype(np.float64) for k in ("rot6d", "trans", "pca", "betas")}


def test_one_fused_step_equals_one_autograd_step():
    """the project's one-step bars (tests/test_poseedge_gpu.py): rtol 2e-5 on the losses, atol 2e-5 on the parameters"""
    sc = ref.scene_fits()[0]
    fused, eager = _fitter(sc, "fused"), _fitter(sc, "eager")
    fused.run(1)
    eager.run(1)
    lf, le = fused.loss_evolution()[0], eager.loss_evolution()[0]
    print("fused", lf, "\neager", le)
    assert (lf[:, 7] > 0).all() and (lf[:, 1] > 0).all() and (lf[:, 5] > 0).all()
    np.testing.assert_allclose(lf, le, rtol=2e-5, atol=1e-12)
    pf, pe = _params(fused), _params(eager)
    for k in pf:
        print(k, np.abs(pf[k] - pe[k]).max())
        np.testing.assert_allclose(pf[k], pe[k], rtol=0, atol=2e-5, err_msg=k)
    assert np.abs(pf["pca"]).max() > 0 and np.abs(pf["betas"]).max() > 0


def test_whole_fit_against_the_float64_restatement():
    """30 steps, B = 3, C = 2, 2-D and 3-D targets.  Bar, the rule of tests/test_softsil_gpu.py: 4 x the deviation of the SAME
    restatement run in float32 from its float64 run, + 1e-6, per quantity.  Those deviations are measured here, on the CPU of the
    machine that runs the test (they move with the host's BLAS), largest absolute difference: final values 1.5e-07, step log
    8.1e-07, rot6d 3.2e-06, trans 1.4e-07, pca 6.5e-06, betas 4.4e-06 on the MI355X host (3.8e-07, 3.0e-07, 2.0e-06, 1.3e-07,
    2.1e-06, 2.8e-06 on another).  The fused loop's own distances from the float64 run there: 2.2e-07, 2.6e-07, 1.5e-06, 8.1e-08,
    1.2e-06, 1.2e-06; 2-D error 0.4299 -> 0.0584 box units, candidate 0 in both."""
    sc, r64, r32 = ref.scene_fits()
    fit = _fitter(sc, "fused")
    fit.run(ref.STEPS)
    res = fit.result()
    got = dict(_params(fit), vals=res["vals"].numpy().astype(np.float64), log=fit.loss_evolution().astype(np.float64))
    figures = {}
    for k in ("vals", "log", "rot6d", "trans", "pca", "betas"):
        dev = np.abs(r32[k] - r64[k]).max()
        figures[k] = (np.abs(got[k] - r64[k]).max(), 4 * dev + 1e-6)
        print("%-6s |kernel - float64| %.3g, bar %.3g (float32 restatement's deviation %.3g)" % (k, *figures[k], dev))
    first = ref.px_error(dict(keypoints=r64["keypoints0"]), sc, cand=res["candidate"])
    last = ref.px_error(dict(keypoints=fit.keypoints.cpu().numpy()), sc, cand=res["candidate"])
    print("2-D error (box units) %.4f -> %.4f; candidate %d (restatement %d)" % (first, last, res["candidate"], r64["candidate"]))
    for k, (err, bar) in figures.items():
        assert err <= bar, (k, err, bar)
    assert last < 0.5 * first
    assert res["candidate"] == r64["candidate"]


def test_second_fit_on_a_resident_fitter_repeats_a_fresh_one():
    sc = ref.scene_fits()[0]
    fit = _fitter(sc, "fused")
    fit.run(12)
    first = dict(_params(fit), log=fit.loss_evolution().copy(), vals=fit.result()["vals"].numpy())
    other = ref.scene(with3d=True, seed=5)
    _load(fit, other)
    fit.run(7)
    _load(fit, sc)
    fit.run(12)
    again = dict(_params(fit), log=fit.loss_evolution().copy(), vals=fit.result()["vals"].numpy())
    fresh = _fitter(sc, "fused")
    fresh.run(12)
    new = dict(_params(fresh), log=fresh.loss_evolution().copy(), vals=fresh.result()["vals"].numpy())
    for k in first:
        assert np.array_equal(first[k], again[k]), k
        assert np.array_equal(first[k], new[k]), k


@pytest.mark.parametrize("hands", [("right",), ("right", "left")])
def test_fit_hands_to_keypoints_end_to_end(hands):
    from homan_amd import synth
    from homan_amd.jointopt import build_model
    mano = synthetic_mano(0)
    sil_fn, hand_fn = synth.hip_clip_fns(mano)
    clip = synth.make_clip(seed=0, frames=3, rend_size=64, image_size=64, obj="cube", silhouette_fn=sil_fn, hand_verts_fn=hand_fn,
                           mano=mano, hands=hands)
    pp = clip["person_parameters"]
    B, h = len(pp), len(hands)
    K_px = torch.from_numpy(np.asarray(clip["camintr"], np.float32)).clone()
    K_px[:, :2] *= 64
    Ws = [torch.from_numpy(handinit.keypoint_regressor(hand_models(mano)[s])) for s in hands]
    X = torch.stack([torch.stack([Ws[i] @ pp[b]["verts"][i] for i in range(h)]) for b in range(B)])          # (B,h,21,3)
    hom = torch.einsum("bij,bhkj->bhki", K_px, X)
    kp2d = hom[..., :2] / hom[..., 2:]
    kw = dict(image_size=64, num_iterations=4, mano_model=mano)
    out = handinit.fit_hands_to_keypoints(kp2d, clip["camintr"], list(hands), keypoints3d=X - X[:, :, :1], **kw)
    eager = handinit.fit_hands_to_keypoints(kp2d, clip["camintr"], list(hands), keypoints3d=X - X[:, :, :1], mode="eager", **kw)
    assert len(out) == B
    for b in range(B):
        o, e = out[b], eager[b]
        assert o["translations"].shape == (h, 1, 3) and o["rotations"].shape == (h, 3, 3) and o["verts"].shape == (h, 778, 3)
        assert o["verts2d"].shape == (h, 778, 2) and o["faces"].shape == pp[b]["faces"].shape and o["hand_side"] == list(hands)
        assert o["mano_pca_pose"].shape == (h, 45) and o["mano_betas"].shape == (h, 10) and o["cams"].shape == (h, 3)
        assert not o["mano_trans"].any() and not o["mano_rot"].any() and not o["mano_betas"].any()
        assert o["keypoints3d"].shape == (h, 21, 3) and o["keypoint_loss"].shape == (h,) and o["candidate"].shape == (h,)
        assert torch.equal(o["faces"], pp[b]["faces"])
        assert torch.equal(o["candidate"], e["candidate"])
        np.testing.assert_allclose(o["keypoint_loss"].numpy(), e["keypoint_loss"].numpy(), rtol=2e-5)
        for k in ("translations", "rotations", "mano_pca_pose", "verts"):
            np.testing.assert_allclose(o[k].numpy(), e[k].numpy(), rtol=0, atol=2e-5, err_msg=k)
        cam = o["verts"] @ o["rotations"] + o["translations"]
        hom = torch.einsum("ij,hvj->hvi", K_px[b], cam)
        np.testing.assert_allclose(o["verts2d"].numpy(), (hom[..., :2] / hom[..., 2:]).numpy(), rtol=0, atol=5e-3)   # (2e-5 m at ~150 px per metre)
        np.testing.assert_allclose((torch.stack([Ws[i] @ cam[i] for i in range(h)])).numpy(), o["keypoints3d"].numpy(), rtol=0,
                                   atol=2e-5)
    # into the joint fit: masks and K_roi stay the clip's (maskutils' job), the hand is the fitted one
    person = []
    for b in range(B):
        d = {k: v for k, v in out[b].items() if k not in ("keypoints3d", "keypoint_loss", "candidate")}
        d.update({k: pp[b][k] for k in ("target_masks", "masks", "K_roi")})
        person.append(d)
    cam_all = torch.cat([o["verts"] @ o["rotations"] + o["translations"] for o in out])                      # frame-major rows
    for optimize_mano in (True, False):
        model = build_model(copy.deepcopy(person), copy.deepcopy(clip["object_parameters"]), objvertices=clip["objvertices"],
                            objfaces=clip["objfaces"], camintr=clip["camintr"], optimize_mano=optimize_mano, image_size=64,
                            mano_model=mano, rend_size=64, sync_metrics=False)
        with torch.no_grad():
            v = model.get_verts_hand()
        v = v[0] if isinstance(v, (tuple, list)) else v
        np.testing.assert_allclose(v.cpu().numpy(), cam_all.numpy(), rtol=0, atol=2e-5, err_msg=str(optimize_mano))
