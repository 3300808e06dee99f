"""Pose chain (MANO layer, rigid transform): the float64 references of tests/posechain_ref.py against the float32 CPU oracle
(oracle.lbs.ManoLayer, oracle.model.rot6d_to_matrix / transform_persp + autograd) on every case of the GPU grid, and the float32
noise floors the tolerances of tests/test_posechain_edges_gpu.py derive from.  CPU only.

A floor is the largest deviation (util.deviation: max |difference| / max |reference| per output tensor, no element exempt) of the
float32 oracle from the float64 reference over every case of the group.  The tests print every figure and pin each constant from
both sides; no constant was taken from a kernel.  The kernels add the same float32 terms in another order and get E32_FACTOR times
the floor (util.E32_FACTOR, the margin of the depth and pair-term suites).
"""
import numpy as np
import pytest
import torch

from tests import posechain_ref as pr
from tests import util

E32_MANO_VERTS = 2.9e-7          # (largest: rows, B = 3, the mirrored hand)
E32_MANO_JOINTS = 2.0e-7         # (the same case)
E32_MANO_G_PCA = 8.0e-7          # (largest: the wrist within 1e-3 of pi)
E32_MANO_G_ROT = 7.6e-7          # (largest: the wrist at 1e-6 rad)
E32_MANO_G_BETAS = 6.5e-7        # (largest: rows, B = 3, the right hand)
E32_MANO_G_TRANS = 1.9e-7        # (largest: betas of +-3; a plain sum of 778 upstream vectors)
E32_RIGID_VERTS = 9.3e-8         # (largest: backward grid, V = 513)
E32_RIGID_G_MESH = 1.7e-7        # (largest: V = 61441)
E32_RIGID_G_ROT6D = 1.8e-6       # (largest: exact grid, V = 4096 - nine sums over the vertices that nearly cancel in rot6d's backward)
E32_RIGID_G_TRANS = 3.0e-7       # (largest: the fused backward on the hand, two terms + g_frame)
E32_RIGID_G_SCALE = 6.7e-7       # (largest: smoothness grid, clips of one frame, V = 257; per-frame addends)
E32_FACTOR = util.E32_FACTOR
MANO_KEYS = ("verts", "joints", "g_pca", "g_rot", "g_betas", "g_trans")
RIGID_KEYS = ("verts", "g_mesh", "g_rot6d", "g_trans", "g_scale")


def _pinned(worst, bar):
    assert 0.5 * bar < worst <= bar, (worst, bar)


def _devs(got, want, keys):
    for k in keys:
        assert bool(torch.isfinite(got[k]).all()) and bool(torch.isfinite(want[k]).all()), k
    return [util.deviation(got[k].numpy(), want[k].numpy()) for k in keys]


def _fused_cases(models):
    """-> [(tag, float32 oracle, float64 reference)] of the fused rigid backward's grid (B = 4, two clips of two)"""
    out = []
    for parts in pr.FUSED_PARTS:
        p, rp, fi = pr.mano_params(4, seed=5), pr.rigid_pose(4, 2, seed=5), pr.fused_inputs(4, *parts)
        want = pr.mano_fused_ref(models["right"], p, rp, 2, fi)
        got = pr.mano_fused_ref(models["right"], p, rp, 2, fi, dtype=torch.float32, layer=pr.mano_oracle32_layer(models["right"]))
        out.append((f"fused n_terms={parts[0]} g_rigid={parts[1]} frame_stride={parts[2]}", got, want))
    return out


def test_mano_ref_matches_the_oracle_and_the_float32_floors():
    """posechain_ref.mano_layer (float64, from the raw model dictionary) against oracle.lbs.ManoLayer (float32) + autograd on every
    case of the GPU grid - frame counts, both hands' rows, clips, pca_dim 45, the five poses where the formulas turn (the oracle
    is finite on exactly those inputs) - and through the hand's rigid transform for the fused backward: E32_MANO_*."""
    models = pr.mano_models()
    worst = dict.fromkeys(MANO_KEYS, 0.0)
    for name, (side, p, flat) in pr.mano_cases().items():
        want = pr.mano_ref(models[side], p["pca"], p["rot"], p["betas"], p["trans"], p["gout"], flat)
        got = pr.mano_oracle32(models[side], p, flat)
        d = _devs(got, want, MANO_KEYS)
        print(f"mano {name}: " + " ".join(f"{k} {x:.3e}" for k, x in zip(MANO_KEYS, d)))
        if p["pca"].shape[1] > 16:
            assert not want["g_pca"][:, 16:].any() and not got["g_pca"][:, 16:].any()
        if name == "zero":                       # every joint exactly zero: identity rotations, the shaped template moved by trans
            m = models[side]
            shaped = torch.from_numpy(m["v_template"]).double()[None] + torch.einsum(
                "bl,vcl->bvc", torch.from_numpy(p["betas"]).double(), torch.from_numpy(m["shapedirs"]).double())
            rest = shaped + torch.from_numpy(p["trans"]).double()[:, None]
            assert util.deviation(want["verts"].numpy(), rest.numpy()) < 1e-6        # (float32 skinning weights sum to 1 +- 1e-7)
        for k, x in zip(MANO_KEYS, d):
            worst[k] = max(worst[k], x)
    for tag, got, want in _fused_cases(models):
        keys = ("g_pca", "g_rot", "g_betas", "g_trans")
        d = _devs(got, want, keys)
        print(f"mano {tag}: " + " ".join(f"{k} {x:.3e}" for k, x in zip(keys, d)))
        for k, x in zip(keys, d):
            worst[k] = max(worst[k], x)
    print("mano floors: " + " ".join(f"{k} {x:.3e}" for k, x in worst.items()))
    for k, bar in zip(MANO_KEYS, (E32_MANO_VERTS, E32_MANO_JOINTS, E32_MANO_G_PCA, E32_MANO_G_ROT, E32_MANO_G_BETAS, E32_MANO_G_TRANS)):
        _pinned(worst[k], bar)


def test_mano_ref_regresses_joints_from_the_raw_regressor():
    """The reference never sees kernel_layout: its rest joints are J_regressor @ shaped vertices, and they agree with the folded
    J_template + J_shapedirs @ betas of the kernels' layout to float32 rounding of the folded tables."""
    from homan_amd.mano_assets import kernel_layout
    m = pr.mano_models()["right"]
    lay = kernel_layout(m)
    betas = torch.from_numpy(pr.mano_params(5)["betas"]).double()
    folded = torch.from_numpy(lay[2]).double()[None] + torch.einsum("jcl,bl->bjc", torch.from_numpy(lay[3]).double(), betas)
    z = torch.zeros(5, 3, dtype=torch.float64)
    raw = pr.mano_layer(m, torch.zeros(5, 16, dtype=torch.float64), z, betas, None, flat_hand_mean=True)[1]
    dev = util.deviation(folded.numpy(), raw.numpy())
    print(f"folded joint regressor vs raw: {dev:.3e}")
    assert dev <= 2.0 ** -23                  # eleven float32 table entries per joint coordinate, each rounded once


def _rigid_cases():
    """-> [(tag, float32 oracle dict, float64 reference dict, keys)] of the rigid grids of the GPU test"""
    out = []
    for N in pr.RIGID_FWD_N:
        for V in pr.RIGID_FWD_V:
            d = pr.rigid_bwd_inputs(N, V, seed=1)
            a = (d["mesh"], d["rot6d"], d["trans"], d["scale"], 1, True)
            out.append((f"fwd N={N} V={V}", pr.rigid_oracle32(d, 1, True), pr.rigid_ref(*a), ("verts",)))
    for N, V in pr.RIGID_BWD:
        d = pr.rigid_bwd_inputs(N, V)
        want = pr.rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], 1, True, d["terms"], d["weights"], d["g_rigid"],
                            d["g_frame"], d["frame_scale"])
        out.append((f"bwd N={N} V={V}", pr.rigid_oracle32(d, 1, True), want, RIGID_KEYS))
    for V in pr.RIGID_EXACT_V:
        d = pr.exact_inputs(2, V)
        extra = pr.exact_extra(d)[0]
        want = pr.rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], 1, True, d["terms"], d["weights"], g_full_extra=extra)
        out.append((f"exact V={V}", pr.rigid_oracle32(d, 1, True, extra.float()), want, RIGID_KEYS[2:]))
    for N, cl, V in pr.SMOOTH_CASES:
        d = pr.exact_inputs(N, V, seed=2, clip_len=cl)
        extra = pr.exact_extra(d, cl, True)[0]
        want = pr.rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], cl, True, d["terms"], d["weights"], g_full_extra=extra)
        out.append((f"smooth N={N} clip_len={cl} V={V}", pr.rigid_oracle32(d, cl, True, extra.float()), want, RIGID_KEYS[2:]))
    return out


def test_rigid_ref_matches_the_oracle_and_the_float32_floors():
    """posechain_ref.rigid_ref (float64) against oracle.model.rot6d_to_matrix + transform_persp + autograd (float32) over the
    forward grid, the non-exact and exact backward grids (the silhouette gather and the smoothness term enter as a float64
    per-vertex gradient, rounded once for the oracle), the fused backward on the hand and the clips forward: E32_RIGID_*."""
    worst = dict.fromkeys(RIGID_KEYS, 0.0)
    cases = _rigid_cases()
    for tag, got, want in _fused_cases(pr.mano_models()):
        cases.append((tag, dict(verts=got["verts_world"], g_rot6d=got["g_rot6d"], g_trans=got["g_rigid_trans"]),
                      dict(verts=want["verts_world"], g_rot6d=want["g_rot6d"], g_trans=want["g_rigid_trans"]),
                      ("verts", "g_rot6d", "g_trans")))
    for kind in pr.DEGENERATE_ROT6D:
        d = pr.degenerate_inputs(kind)
        want = pr.rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], 1, True, d["terms"], d["weights"], d["g_rigid"],
                            d["g_frame"], d["frame_scale"])
        cases.append((f"degenerate {kind}", _degenerate_oracle32(d), want, RIGID_KEYS))
    for tag, got, want, keys in cases:
        d = _devs(got, want, keys)
        print(f"rigid {tag}: " + " ".join(f"{k} {x:.3e}" for k, x in zip(keys, d)))
        for k, x in zip(keys, d):
            worst[k] = max(worst[k], x)
    print("rigid floors: " + " ".join(f"{k} {x:.3e}" for k, x in worst.items()))
    for k, bar in zip(RIGID_KEYS, (E32_RIGID_VERTS, E32_RIGID_G_MESH, E32_RIGID_G_ROT6D, E32_RIGID_G_TRANS, E32_RIGID_G_SCALE)):
        _pinned(worst[k], bar)


def _degenerate_oracle32(d):
    """the float32 oracle at a degenerate rot6d: oracle.model in its reference form (F.normalize: x / clamp_min(|x|, 1e-12) with
    the norm's subgradient 0 at the zero vector)"""
    from oracle import model as om
    keep = om.REFERENCE_FORM
    om.REFERENCE_FORM = True
    try:
        return pr.rigid_oracle32(d, 1, True)
    finally:
        om.REFERENCE_FORM = keep


def test_degenerate_rot6d_on_the_oracle():
    """First column exactly zero; second column an exact multiple of the first (u = a2 - (b1.a2) b1 exactly zero).  The oracle's
    forward is finite in both of its forms and they agree bit for bit there (every vector involved is zero or exact).  Its
    gradient: the reference form (F.normalize) is finite and its clamp passes g / 1e-12 straight through - the Jacobian of
    x / clamp_min(|x|, 1e-12) at x = 0 is 1e12 I, what the kernels' `else` branches implement (du = db2 / nu, da1 = db1 / n1) -
    while the written-out form (sqrt of a sum of squares) back-propagates 0 / 0 into g_rot6d: the GPU test takes the reference
    form for the gradients and the written-out form for the forward's bits."""
    from oracle import model as om
    J = torch.autograd.functional.jacobian(lambda x: torch.nn.functional.normalize(x[None])[0], torch.zeros(3))
    assert torch.equal(J, torch.eye(3) * 1e12)
    for kind in pr.DEGENERATE_ROT6D:
        d = pr.degenerate_inputs(kind)
        written, ref_form = pr.rigid_oracle32(d, 1, True), _degenerate_oracle32(d)
        u_zero = kind == "parallel"
        R = written["rotmat"]
        assert bool(torch.isfinite(R).all()) and torch.equal(R, ref_form["rotmat"])
        assert not R[:, :, 2].any() and not R[:, :, 1 if u_zero else 0].any()            # b3 = 0 and the clamped column = 0
        for k in RIGID_KEYS:
            assert bool(torch.isfinite(ref_form[k]).all()), (kind, k)
        assert not bool(torch.isfinite(written["g_rot6d"]).all())                        # (0 / 0 in the sqrt's backward)
        for k in ("verts", "g_mesh", "g_trans", "g_scale"):
            assert bool(torch.isfinite(written[k]).all()), (kind, k)
        assert float(ref_form["g_rot6d"].abs().max()) > 1e11                             # the clamp's 1e12 is there


def test_rot6d_restatement_is_the_oracles():
    """posechain_ref.rot6d_to_matrix in float32 against oracle.model.rot6d_to_matrix (both forms) on random input: same
    mathematics, a few ulp apart"""
    from oracle import model as om
    r6 = torch.from_numpy(pr.rigid_pose(64, 1)[0])
    a, b = pr.rot6d_to_matrix(r6), om.rot6d_to_matrix(r6)
    assert util.deviation(a.numpy(), b.numpy()) <= 4 * 2.0 ** -23
    R = pr.rot6d_to_matrix(r6.double())
    assert util.deviation((R.transpose(1, 2) @ R).numpy(), np.tile(np.eye(3), (64, 1, 1))) < 1e-14       # a rotation


def test_gather_and_smoothness_refs():
    """sil_gather_ref against the closed form of k_bwd_gather evaluated in float64 numpy, smooth_grad_ref against
    oracle.objchain.smooth_unit_grad (float32, one clip) and zero across clip boundaries; fan_mesh has the valences it is for."""
    from oracle import objchain
    d = pr.exact_inputs(2, 257)
    g, (off, items) = pr.exact_extra(d)
    val = np.diff(off)
    assert val[0] == 0 and val[1] > 8 and val[-1] == 1 and val.sum() == 3 * len(d["faces"])
    assert not g[:, 0].any()                                                # the isolated vertex
    p = d["parts"].reshape(2, -1, 2)
    gn = np.zeros((2, 257, 2))
    for v in range(257):
        gn[:, v] = p[:, items[off[v]:off[v + 1]]].sum(1)
    cv, K = d["cam_verts"].astype(np.float64), d["K"].astype(np.float64)
    du0, dv0 = gn[..., 0] * 2.0, -gn[..., 1] * 2.0
    zz = cv[..., 2] + 1e-9
    dxn, dyn = K[:, None, 0, 0] * du0 + K[:, None, 1, 0] * dv0, K[:, None, 0, 1] * du0 + K[:, None, 1, 1] * dv0
    closed = np.stack([dxn / zz, dyn / zz, -(dxn * cv[..., 0] + dyn * cv[..., 1]) / (zz * zz)], -1)
    assert util.deviation(g.numpy(), closed) < 1e-13
    for N, cl, V in pr.SMOOTH_CASES:
        v = pr.exact_inputs(N, V, seed=2, clip_len=cl)["cam_verts"]
        got = pr.smooth_grad_ref(v, cl, pr.SMOOTH_WEIGHT).numpy()
        if cl == 1:
            assert not got.any()
            continue
        for c in range(N // cl):
            want = np.float32(pr.SMOOTH_WEIGHT) * objchain.smooth_unit_grad(v[c * cl:(c + 1) * cl]).astype(np.float64)
            assert util.deviation(got[c * cl:(c + 1) * cl], want) < 1e-6
