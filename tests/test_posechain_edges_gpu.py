"""Pose chain at the shapes and edges the rest of the suite does not reach: the MANO layer (csrc/mano.hip: k_mano_fwd,
k_mano_bwd<false>, k_mano_bwd<true>) and the rigid transform (csrc/geometry.hip: k_rigid_fwd, k_rigid_bwd<false>, k_rigid_bwd<true>,
k_rigid_bwd_x<1,1024>, k_rigid_bwd_x<2,768>) through the raw C ABI, on the synthetic hand model.

References: tests/posechain_ref.py (float64 torch + autograd, built from the raw model dictionary), checked against the float32 CPU
oracle in tests/test_posechain_refs.py, which also measures the float32 floors E32_*.  Whatever is stated as identical, untouched
or equal across paths is torch.equal / array_equal.  A comparison with a float64 reference allows E32_FACTOR times the floor of its
group (deviation = max |difference| / max |reference| per tensor, no element exempt).  The exact sums additionally get half a
quantum of 2^-44 per addend: V * 2^-45 absolute on g_trans and g_scale (V addends each), and that times the largest column sum of
|dR / drot6d| (posechain_ref.rot6d_gain) on g_rot6d, which is a linear map of nine such sums.

Every output buffer carries GUARD sentinel-filled rows after its last legitimate row (a strided call's other hand's rows are
guards as well); they must come back untouched, and so must the pad behind every workspace.
"""
import functools

import numpy as np
import pytest
import torch

from tests import posechain_ref as pr
from tests import test_posechain_refs as refs

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG = -1                    # HM_ERR_BAD_ARG of include/homan_amd.h
FACTOR = refs.E32_FACTOR
SENT, GUARD, PAD = -7.0, 2, 256
MANO_BAR = dict(verts=refs.E32_MANO_VERTS, joints=refs.E32_MANO_JOINTS, g_pca=refs.E32_MANO_G_PCA, g_rot=refs.E32_MANO_G_ROT,
                g_betas=refs.E32_MANO_G_BETAS, g_trans=refs.E32_MANO_G_TRANS)
RIGID_BAR = dict(verts=refs.E32_RIGID_VERTS, g_mesh=refs.E32_RIGID_G_MESH, g_rot6d=refs.E32_RIGID_G_ROT6D,
                 g_trans=refs.E32_RIGID_G_TRANS, g_scale=refs.E32_RIGID_G_SCALE)
GRADS = ("g_pca", "g_rot", "g_betas", "g_trans")


def _hl():
    from homan_amd import lib as hl
    return hl


def _dev(x, dtype=None):
    if x is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(x)) if not isinstance(x, torch.Tensor) else x
    return (t.to(device=DEV, dtype=dtype) if dtype is not None else t.to(DEV)).contiguous()


def _guarded(rows, *shape):
    return torch.full((rows + GUARD, *shape), SENT, device=DEV)


def _untouched(t, rows=0):
    return bool((t[rows:] == SENT).all())


def _same(a, b):
    """the same bits (the saved chain state holds integers too, parent -1 among them: a NaN pattern to a float comparison)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _zero_ws(nbytes):
    """zero-filled workspace of nbytes with a patterned pad behind it"""
    t = torch.zeros(nbytes + PAD, dtype=torch.uint8, device=DEV)
    t[nbytes:] = 0xA5
    return t


def _pad_ok(ws):
    return bool((ws[-PAD:] == 0xA5).all())


def _within(tag, got, want, bar, extra_abs=0.0):
    """|got - want| <= FACTOR * bar * max |want| + extra_abs, every element; prints the figure before it asserts"""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = want.detach().cpu().double().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"{tag}: error {err:.3e} scale {scale:.3e} deviation {err / scale if scale > 0 else err:.3e} "
          f"(bar {FACTOR * bar:.1e}, absolute part {extra_abs:.1e})")
    assert np.isfinite(got).all(), tag
    assert err <= FACTOR * bar * scale + extra_abs, tag


# ===================================================================== A. MANO
@functools.lru_cache(maxsize=None)
def _mctx(side, flat=False):
    from homan_amd import ops
    return ops.ManoContext(pr.mano_models()[side], DEV, flat_hand_mean=flat)


@functools.lru_cache(maxsize=None)
def _state_dw():
    return _hl().lib().hm_mano_state_bytes(1) // 4


@functools.lru_cache(maxsize=None)
def _case_ref(name):
    """float64 reference of a case of posechain_ref.mano_cases (computed once, shared, never modified)"""
    side, p, flat = pr.mano_cases()[name]
    return pr.mano_ref(pr.mano_models()[side], p["pca"], p["rot"], p["betas"], p["trans"], p["gout"], flat)


def _pdev(p):
    return {k: _dev(v) for k, v in p.items()}


def _fwd(mctx, p, B, joints=True, trans=True, state=True, world=None, entry="clips", clip_len=0, row0=0, row_stride=1, out=None,
         pca_dim=None):
    """hm_mano_fwd / _clips / _rows on device parameters p (arrays of B * row_stride rows) -> rc, dict of guarded outputs
    (verts, joints, state, world; None where not asked for).  world = (rot6d, trans, scale) device tensors."""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    rows = B * row_stride
    if out is None:
        out = dict(verts=_guarded(rows, 778, 3), joints=_guarded(rows, 16, 3) if joints else None,
                   state=_guarded(rows, _state_dw()) if state else None, world=_guarded(rows, 778, 3) if world else None)
    w = world or (None, None, None)
    a = (mctx.ptrs, P(p["pca"]), pca_dim if pca_dim is not None else p["pca"].shape[1], P(p["rot"]), P(p["betas"]),
         P(p["trans"]) if trans else None, B, P(out["verts"]), P(out["joints"]), P(w[0]), P(w[1]), P(w[2]), P(out["world"]),
         P(out["state"]))
    if entry == "plain":
        assert clip_len == 0
        rc = L.hm_mano_fwd(*a, hl.stream())
    elif entry == "clips":
        rc = L.hm_mano_fwd_clips(*a, clip_len, hl.stream())
    else:
        rc = L.hm_mano_fwd_rows(*a, clip_len, row0, row_stride, hl.stream())
    torch.cuda.synchronize()
    return rc, out


def _grad_bufs(rows, pca_dim):
    return dict(g_pca=_guarded(rows, pca_dim), g_rot=_guarded(rows, 3), g_betas=_guarded(rows, 10), g_trans=_guarded(rows, 3))


def _bwd(mctx, p, B, gout, state, ws=None, extra=None, w_extra=0.0, row0=0, row_stride=1, entry="plain", out=None, pca_dim=None):
    """hm_mano_bwd / _rows -> rc, dict of guarded gradients, workspace"""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    pd = pca_dim if pca_dim is not None else p["pca"].shape[1]
    out = out or _grad_bufs(B * row_stride, p["pca"].shape[1])
    ws = ws if ws is not None else _zero_ws(L.hm_mano_workspace_bytes(B))
    a = (mctx.ptrs, P(p["pca"]), pd, P(p["rot"]), P(p["betas"]), B, P(gout), P(extra), float(w_extra), P(out["g_pca"]),
         P(out["g_rot"]), P(out["g_betas"]), P(out["g_trans"]), P(state), P(ws))
    rc = L.hm_mano_bwd(*a, hl.stream()) if entry == "plain" else L.hm_mano_bwd_rows(*a, row0, row_stride, hl.stream())
    torch.cuda.synchronize()
    return rc, out, ws


def _bwd_fused(mctx, p, B, mesh, rot6d, scale, fi, clip_len, state, ws=None, n_terms=None, frame_stride=None, pca_dim=None):
    """hm_mano_bwd_rigid_clips -> rc, dict of the six guarded gradients (+ g_rot6d, g_rigid_trans), workspace"""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    out = _grad_bufs(B, p["pca"].shape[1])
    out.update(g_rot6d=_guarded(B, 3, 2), g_rigid_trans=_guarded(B, 3))
    ws = ws if ws is not None else _zero_ws(L.hm_mano_workspace_bytes(B))
    terms = [_dev(t) for t in fi["terms"]]
    tp, tw, tn = hl.terms(list(zip(terms, fi["weights"])))
    g_rigid, g_frame = _dev(fi["g_rigid"]), _dev(fi["g_frame"])
    stride = frame_stride if frame_stride is not None else (fi["g_frame"].shape[1] if fi["g_frame"] is not None else 0)
    rc = L.hm_mano_bwd_rigid_clips(mctx.ptrs, P(p["pca"]), pca_dim if pca_dim is not None else p["pca"].shape[1], P(p["rot"]),
                                   P(p["betas"]), B, None, 0.0, P(out["g_pca"]), P(out["g_rot"]), P(out["g_betas"]),
                                   P(out["g_trans"]), P(state), P(ws), P(mesh), P(rot6d), P(scale), tp, tw,
                                   tn if n_terms is None else n_terms, P(g_rigid), P(g_frame), stride, float(fi["frame_scale"]),
                                   P(out["g_rot6d"]), P(out["g_rigid_trans"]), clip_len, hl.stream())
    torch.cuda.synchronize()
    return rc, out, ws


def _check_mano_values(tag, out, want, B, keys):
    for k in keys:
        _within(f"{tag} {k}", out[k][:B], want[k], MANO_BAR[k])


def _world_bar(want_verts, want_world, scale):
    """verts_world composes the two groups: the model-space error, scaled by |s|, and the rigid transform's own"""
    s = float(np.abs(np.asarray(scale)).max())
    return refs.E32_MANO_VERTS * s * float(want_verts.abs().max()) / float(want_world.abs().max()) + refs.E32_RIGID_VERTS


@pytest.mark.parametrize("B", pr.MANO_B)
def test_mano_forward_does_not_depend_on_the_frame_grouping(B):
    """k_mano_fwd, four frames per workgroup, B on, below and above the group (the tail group's missing frames repeat the last
    one and store nothing): vertices, joints and verts_world against float64; frame i of the batch bit-equal - state included -
    to the same parameters run alone through hm_mano_fwd; guards untouched; every optional argument dropped alone leaves the
    other outputs as they were, and no translation is a translation of zeros."""
    _, p, _ = pr.mano_cases()[f"B{B}"]
    rp = pr.rigid_pose(B, 1, seed=B)
    mctx, pd, world = _mctx("right"), _pdev(p), tuple(_dev(x) for x in rp)
    rc, full = _fwd(mctx, pd, B, world=world)
    assert rc == 0
    for k, t in full.items():
        assert _untouched(t, B), k
    want = _case_ref(f"B{B}")
    _check_mano_values(f"B={B}", full, want, B, ("verts", "joints"))
    ww = pr.mano_fused_ref(pr.mano_models()["right"], p, rp, 0, pr.fused_inputs(B, 0, False, 0))["verts_world"]
    _within(f"B={B} verts_world", full["world"][:B], ww, _world_bar(want["verts"], ww, rp[2]))
    sw = (_state_dw() - 3 * 778 - 2, _state_dw() - 2)                    # the chain state's words are written up to its size
    for i in range(B):
        one_p = {k: v[i:i + 1].contiguous() for k, v in pd.items()}
        rc, one = _fwd(mctx, one_p, 1, world=tuple(x[i:i + 1].contiguous() for x in world[:2]) + (world[2],), entry="plain")
        assert rc == 0
        for k in ("verts", "joints", "world"):
            assert torch.equal(one[k][:1], full[k][i:i + 1]), (k, i)
        written = ~(one["state"][0] == SENT)
        assert bool(written[sw[0]:sw[1]].all())                          # (the posed vertices; the chain state has padding)
        assert _same(one["state"][0], full["state"][i]) and bool(written[:64].all()), i
    for drop in ("joints", "state", "world"):
        kw = dict(joints=drop != "joints", state=drop != "state", world=None if drop == "world" else world)
        rc, part = _fwd(mctx, pd, B, **kw)
        assert rc == 0 and part[drop] is None
        for k, t in part.items():
            assert t is None or _same(t, full[k]), (drop, k)
    rc, bare = _fwd(mctx, pd, B, joints=False, trans=False, state=False)
    zero_t = dict(pd, trans=torch.zeros_like(pd["trans"]))
    rc2, zt = _fwd(mctx, zero_t, B, joints=False, state=False)
    assert rc == 0 and rc2 == 0 and torch.equal(bare["verts"], zt["verts"]) and not torch.equal(bare["verts"], full["verts"])


@pytest.mark.parametrize("B", [1, 3])
def test_mano_rows_walk_one_hand_and_leave_the_other_alone(B):
    """hm_mano_fwd_rows / hm_mano_bwd_rows, two hands interleaved frame-major (row_stride 2, row0 0 and 1), the second through the
    mirrored model: each hand's rows are bit-equal to the contiguous call on the gathered rows (and within the floors of float64);
    the other hand's rows - vertices, joints, state, verts_world and all four gradients - are untouched, first as sentinels,
    then as the first hand's results."""
    both = pr.mano_params(2 * B, seed=3)
    rp = pr.rigid_pose(2 * B, B, seed=B)                                  # clip_len 2 rows: both hands of a frame share a scale
    pd, world = _pdev(both), tuple(_dev(x) for x in rp)
    gout = pd["gout"]
    out, grads = None, _grad_bufs(2 * B, 16)
    for h, side in enumerate(("right", "left")):
        mctx = _mctx(side)
        before = None if out is None else {k: t.clone() for k, t in out.items()}
        rc, out = _fwd(mctx, pd, B, world=world, entry="rows", clip_len=2, row0=h, row_stride=2, out=out)
        assert rc == 0
        g_before = {k: t.clone() for k, t in grads.items()}
        rc, grads, ws = _bwd(mctx, pd, B, gout, out["state"], row0=h, row_stride=2, entry="rows", out=grads)
        assert rc == 0 and _pad_ok(ws)
        for k, t in list(out.items()) + list(grads.items()):
            assert _untouched(t, 2 * B), k
            other = t[1 - h:2 * B:2]
            assert _untouched(other) if h == 0 else _same(other, (before[k] if k in before else g_before[k])[0:2 * B:2]), (k, h)
        gp = {k: v[h::2].contiguous() for k, v in pd.items()}
        gw = (world[0][h::2].contiguous(), world[1][h::2].contiguous(), world[2])
        rc, cont = _fwd(mctx, gp, B, world=gw, clip_len=1)
        assert rc == 0
        for k in ("verts", "joints", "world"):
            assert torch.equal(cont[k][:B], out[k][h:2 * B:2]), (k, h)
        rc, cg, _ = _bwd(mctx, gp, B, gp["gout"], cont["state"][:B].contiguous())
        assert rc == 0
        for k in GRADS:
            assert torch.equal(cg[k][:B], grads[k][h:2 * B:2]), (k, h)
        want = _case_ref(f"rows_B{B}_hand{h}")
        _check_mano_values(f"rows B={B} hand {h}", {k: t[h::2] for k, t in list(out.items()) + list(grads.items())}, want, B,
                           ("verts", "joints") + GRADS)
    assert not torch.equal(out["verts"][0], out["verts"][1])


def test_mano_clips_take_one_signed_scale_per_clip():
    """hm_mano_fwd_clips with verts_world, B = 9 as three clips of three with distinct hand scales, one negative (no absolute
    value on this path): against float64, and bit-equal to hm_rigid_fwd_clips on the forward's own vertices; clip_len = 0 is
    one clip (the first scale throughout)."""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    _, p, _ = pr.mano_cases()["clips"]
    rp = pr.rigid_pose(9, 3, seed=2)
    assert rp[2][-1] < 0 and len(set(np.abs(rp[2]).tolist())) == 3
    mctx, pd, world = _mctx("right"), _pdev(p), tuple(_dev(x) for x in rp)
    for cl in (3, 0):
        rc, out = _fwd(mctx, pd, 9, world=world, clip_len=cl)
        assert rc == 0 and all(_untouched(t, 9) for t in out.values())
        scale = rp[2] if cl else rp[2][:1]
        want = pr.mano_fused_ref(pr.mano_models()["right"], p, (rp[0], rp[1], scale), cl, pr.fused_inputs(9, 0, False, 0))
        _within(f"clips clip_len={cl} verts_world", out["world"][:9], want["verts_world"],
                _world_bar(want["verts"], want["verts_world"], scale))
        again = _guarded(9, 778, 3)
        verts = out["verts"][:9].contiguous()
        rc = L.hm_rigid_fwd_clips(P(verts), P(world[0]), P(world[1]), P(world[2]), 0, 9, 778, None, P(again), cl, hl.stream())
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(again, out["world"])
    _check_mano_values("clips", out, _case_ref("clips"), 9, ("verts", "joints"))


@pytest.mark.parametrize("pca_dim", [16, 45])
def test_mano_backward_saved_state_recompute_and_tickets(pca_dim):
    """k_mano_bwd<false>, B = 3: all four gradients against float64; the chain state the forward saved and state = NULL (chain
    recomputed) give the same bits; at pca_dim 45 the columns 16 .. 44 are exact zeros, or exactly w_extra * g_pca_extra with it;
    a second backward on the same workspace with another gout equals one on a fresh zeroed workspace (the tickets reset
    themselves)."""
    name = "pca45" if pca_dim == 45 else "B3"
    _, p, _ = pr.mano_cases()[name]
    mctx, pd = _mctx("right"), _pdev(p)
    rc, fw = _fwd(mctx, pd, 3)
    state = fw["state"][:3].contiguous()
    rc1, saved, ws = _bwd(mctx, pd, 3, pd["gout"], state)
    rc2, recomputed, ws2 = _bwd(mctx, pd, 3, pd["gout"], None)
    assert rc == 0 and rc1 == 0 and rc2 == 0 and _pad_ok(ws) and _pad_ok(ws2)
    want = _case_ref(name)
    for k in GRADS:
        assert _untouched(saved[k], 3) and torch.equal(saved[k], recomputed[k]), k
    _check_mano_values(f"pca_dim={pca_dim}", saved, want, 3, GRADS)
    if pca_dim == 45:
        assert not saved["g_pca"][:3, 16:].any()
    extra, w_extra = _dev(pr.rng(8).normal(size=(3, pca_dim)).astype(np.float32)), 1e-4
    rc, ex, _ = _bwd(mctx, pd, 3, pd["gout"], state, extra=extra, w_extra=w_extra)
    assert rc == 0
    wx = pr.mano_ref(pr.mano_models()["right"], p["pca"], p["rot"], p["betas"], p["trans"], p["gout"], g_pca_extra=extra.cpu().numpy(),
                     w_extra=w_extra)
    _within(f"pca_dim={pca_dim} g_pca with extra", ex["g_pca"][:3], wx["g_pca"], MANO_BAR["g_pca"])
    if pca_dim == 45:
        assert torch.equal(ex["g_pca"][:3, 16:], torch.tensor(w_extra, device=DEV) * extra[:, 16:])
    for k in GRADS[1:]:
        assert torch.equal(ex[k], saved[k]), k
    gout2 = _dev(pr.mano_params(3, pca_dim, seed=9)["gout"])
    rc, second, _ = _bwd(mctx, pd, 3, gout2, state, ws=ws)
    rc2, fresh, _ = _bwd(mctx, pd, 3, gout2, state)
    assert rc == 0 and rc2 == 0 and _pad_ok(ws)
    for k in GRADS:
        assert torch.equal(second[k], fresh[k]) and not torch.equal(second[k], saved[k]), k


@pytest.mark.parametrize("n_terms,g_rigid,frame_stride", pr.FUSED_PARTS)
def test_mano_backward_with_the_rigid_backward_inside(n_terms, g_rigid, frame_stride):
    """hm_mano_bwd_rigid_clips (k_mano_bwd<true>), B = 4 as two clips with two scales: all six gradients against float64; the four
    MANO gradients bit-equal to hm_rigid_bwd_clips (with g_mesh) followed by hm_mano_bwd, g_rot6d / g_trans within twice the
    allowance of those (both sides are within one of the truth; the header says the last bits differ); saved state and
    recomputed chain give the same bits."""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    B, cl = 4, 2
    p, rp, fi = pr.mano_params(B, seed=5), pr.rigid_pose(B, 2, seed=5), pr.fused_inputs(B, n_terms, g_rigid, frame_stride)
    mctx, pd = _mctx("right"), _pdev(p)
    r6, rt, rs = (_dev(x) for x in rp)
    rc, fw = _fwd(mctx, pd, B, world=(r6, rt, rs), clip_len=cl)
    assert rc == 0
    mesh, state = fw["verts"][:B].contiguous(), fw["state"][:B].contiguous()
    rc, got, ws = _bwd_fused(mctx, pd, B, mesh, r6, rs, fi, cl, state)
    assert rc == 0 and _pad_ok(ws) and all(_untouched(t, B) for t in got.values())
    want = pr.mano_fused_ref(pr.mano_models()["right"], p, rp, cl, fi)
    tag = f"fused n_terms={n_terms} g_rigid={g_rigid} frame_stride={frame_stride}"
    _check_mano_values(tag, got, want, B, GRADS)
    _within(f"{tag} g_rot6d", got["g_rot6d"][:B], want["g_rot6d"], RIGID_BAR["g_rot6d"])
    _within(f"{tag} g_rigid_trans", got["g_rigid_trans"][:B], want["g_rigid_trans"], RIGID_BAR["g_trans"])
    rc, again, _ = _bwd_fused(mctx, pd, B, mesh, r6, rs, fi, cl, None)
    assert rc == 0
    for k in got:
        assert torch.equal(again[k], got[k]), k
    # the two launches it replaces
    terms = [_dev(t) for t in fi["terms"]]
    tp, tw, tn = hl.terms(list(zip(terms, fi["weights"])))
    g_mesh, g6, gt = _guarded(B, 778, 3), _guarded(B, 3, 2), _guarded(B, 3)
    rws = _zero_ws(L.hm_rigid_workspace_bytes(B))
    gr, gf = _dev(fi["g_rigid"]), _dev(fi["g_frame"])
    rc = L.hm_rigid_bwd_clips(P(mesh), P(r6), P(rs), 0, tp, tw, tn, P(gr), P(gf), frame_stride, float(fi["frame_scale"]), B, 778,
                              P(g_mesh), P(g6), P(gt), None, P(rws), cl, hl.stream())
    torch.cuda.synchronize()
    assert rc == 0 and _pad_ok(rws) and _untouched(g_mesh, B)
    rc, two, _ = _bwd(mctx, pd, B, g_mesh[:B].contiguous(), state)
    assert rc == 0
    for k in GRADS:
        assert torch.equal(two[k], got[k]), k
    for k, a, b in (("g_rot6d", g6, got["g_rot6d"]), ("g_trans", gt, got["g_rigid_trans"])):
        scale = float(b[:B].abs().max())
        assert float((a[:B] - b[:B]).abs().max()) <= 2 * FACTOR * RIGID_BAR[k] * scale, k
    if n_terms == 0:
        assert all(not got[k][:B].any() for k in GRADS)                  # nothing reaches the mesh


@pytest.mark.parametrize("kind", pr.POSE_EDGES)
def test_mano_poses_where_the_formulas_turn(kind):
    """B = 4: every joint exactly zero (the |r + 1e-8| branch in all sixteen), the wrist at 1e-6 rad, within 1e-3 of pi, at 7.5 rad
    (beyond 2 pi), betas of +-3: values and gradients against float64, the forward bit-equal to the written-out CPU layer
    (orc_mano_forward).  tests/test_posechain_refs.py shows the float32 oracle finite and within its floor on these inputs."""
    from homan_amd.mano_assets import kernel_layout
    from oracle import clib
    side, p, flat = pr.mano_cases()[kind]
    mctx, pd = _mctx(side, flat), _pdev(p)
    rc, fw = _fwd(mctx, pd, 4)
    rc2, g, _ = _bwd(mctx, pd, 4, pd["gout"], fw["state"][:4].contiguous())
    assert rc == 0 and rc2 == 0
    _check_mano_values(kind, dict(fw, **g), _case_ref(kind), 4, ("verts", "joints") + GRADS)
    lay = kernel_layout(pr.mano_models()[side], flat_hand_mean=flat)
    exact = np.empty((4, 778, 3), np.float32)
    clib.lib().orc_mano_forward(*[clib.fptr(a) for a in lay[:7]], clib.iptr(lay[7]), clib.fptr(p["pca"]), 16, clib.fptr(p["rot"]),
                                clib.fptr(p["betas"]), 4, clib.fptr(exact))
    assert np.array_equal(fw["verts"][:4].cpu().numpy(), exact + p["trans"][:, None])


def test_mano_entry_points_refuse_bad_arguments():
    """HM_ERR_BAD_ARG and every output still at its sentinel, on real, correctly sized device buffers: pca_dim < 16, row0 >=
    row_stride, a clip_len that does not divide, verts_world without one of its three inputs, n_terms > 5, g_frame with
    frame_stride < 3."""
    B = 4
    p, rp, fi = pr.mano_params(2 * B, seed=5), pr.rigid_pose(2 * B, 2, seed=5), pr.fused_inputs(B, 5, True, 5)
    hl = _hl()
    P = hl.ptr
    mctx, pd = _mctx("right"), _pdev(p)
    world = tuple(_dev(x) for x in rp)

    def refused(rc, out):
        assert rc == BAD_ARG
        for k, t in out.items():
            assert t is None or _untouched(t), k

    for entry, kw in (("clips", {}), ("rows", dict(row_stride=2)), ("rows", dict(row_stride=2, row0=1))):
        refused(*_fwd(mctx, pd, B, world=world, entry=entry, pca_dim=15, **kw))
    refused(*_fwd(mctx, pd, B, world=world, entry="rows", row0=2, row_stride=2))
    refused(*_fwd(mctx, pd, B, world=world, entry="rows", row0=1, row_stride=1))
    refused(*_fwd(mctx, pd, B, world=world, entry="clips", clip_len=3))
    refused(*_fwd(mctx, pd, B, world=world, entry="rows", clip_len=3, row_stride=2))
    for missing in range(3):
        w = tuple(None if i == missing else x for i, x in enumerate(world))
        for entry, kw in (("clips", {}), ("rows", dict(row_stride=2))):
            out = dict(verts=_guarded(2 * B, 778, 3), joints=None, state=None, world=_guarded(2 * B, 778, 3))
            a = (mctx.ptrs, P(pd["pca"]), 16, P(pd["rot"]), P(pd["betas"]), P(pd["trans"]), B, P(out["verts"]), None, P(w[0]), P(w[1]),
                 P(w[2]), P(out["world"]), None)
            rc = (hl.lib().hm_mano_fwd_clips(*a, 0, hl.stream()) if entry == "clips" else
                  hl.lib().hm_mano_fwd_rows(*a, 0, 0, 2, hl.stream()))
            torch.cuda.synchronize()
            refused(rc, out)
    state = None
    gout = pd["gout"]
    for kw in (dict(pca_dim=15), dict(pca_dim=15, entry="rows", row_stride=2), dict(entry="rows", row0=2, row_stride=2),
               dict(entry="rows", row0=1, row_stride=1)):
        rc, out, ws = _bwd(mctx, pd, B, gout, state, **kw)
        refused(rc, out)
        assert not ws[:-PAD].any()
    mesh = gout                                                          # (any (B,778,3) floats will do: nothing is launched)
    for kw in (dict(pca_dim=15), dict(n_terms=6), dict(frame_stride=2), dict(clip_len=3)):
        cl = kw.pop("clip_len", 2)
        rc, out, ws = _bwd_fused(mctx, pd, B, mesh, world[0], world[2], fi, cl, None, **kw)
        refused(rc, out)
        assert not ws[:-PAD].any()
    rc, out, _ = _bwd_fused(mctx, pd, B, mesh, world[0], world[2], fi, 2, None)          # the same buffers are accepted as they are
    assert rc == 0 and not any(_untouched(t[:B]) for t in out.values())


# ===================================================================== B. rigid transform
def _rigid_fwd(d, clip_len, abs_scale, rotmat=True):
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    N, V = d["mesh"].shape[:2]
    verts, rm = _guarded(N, V, 3), _guarded(N, 3, 3) if rotmat else None
    keep = [_dev(d[k]) for k in ("mesh", "rot6d", "trans", "scale")]          # (alive until the launch has run)
    rc = L.hm_rigid_fwd_clips(P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), int(abs_scale), N, V, P(rm), P(verts), clip_len,
                              hl.stream())
    torch.cuda.synchronize()
    return rc, verts, rm


def _rigid_bwd(d, clip_len, abs_scale, workspace=True, ws=None, g_mesh=True, twin=True, weights=None, n_terms=None,
               frame_stride=None):
    """hm_rigid_bwd_clips -> rc, dict(g_mesh, g_rot6d, g_trans, g_scale) guarded, workspace (None without)"""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    N, V = d["mesh"].shape[:2]
    out = dict(g_mesh=_guarded(N, V, 3) if g_mesh else None, g_rot6d=_guarded(N, 3, 2), g_trans=_guarded(N, 3), g_scale=_guarded(N))
    if workspace and ws is None:
        ws = _zero_ws(L.hm_rigid_workspace_bytes(N))
    terms = [_dev(t) for t in d["terms"]]
    tp, tw, tn = hl.terms(list(zip(terms, d["weights"] if weights is None else weights)))
    gr, gf = (_dev(d["g_rigid"]), _dev(d["g_frame"])) if twin else (None, None)
    stride = frame_stride if frame_stride is not None else (d["g_frame"].shape[1] if twin else 0)
    keep = [_dev(d[k]) for k in ("mesh", "rot6d", "scale")]                    # (alive until the launch has run)
    rc = L.hm_rigid_bwd_clips(P(keep[0]), P(keep[1]), P(keep[2]), int(abs_scale), tp, tw,
                              tn if n_terms is None else n_terms, P(gr), P(gf), stride, float(d["frame_scale"]), N, V, P(out["g_mesh"]),
                              P(out["g_rot6d"]), P(out["g_trans"]), P(out["g_scale"]), P(ws) if workspace else None, clip_len, hl.stream())
    torch.cuda.synchronize()
    return rc, out, ws


@pytest.mark.parametrize("N", pr.RIGID_FWD_N)
@pytest.mark.parametrize("V", pr.RIGID_FWD_V)
def test_rigid_forward_is_the_oracles_floats(N, V):
    """k_rigid_fwd, V on and around the 256 vertices of a workgroup, one frame per clip with distinct scales, the last negative:
    vertices bit-equal to oracle.model.transform_persp in float32 with and without abs_scale, the rotation matrices bit-equal to
    oracle.model.rot6d_to_matrix, the same vertices with rotmat = NULL; within the float64 reference's floor; guards untouched."""
    d = pr.rigid_bwd_inputs(N, V, seed=1)
    assert d["scale"][-1] < 0
    for abs_scale in (True, False):
        want = pr.rigid_oracle32(dict(d, terms=(), weights=()), 1, abs_scale, with_twin=False)
        rc, verts, rm = _rigid_fwd(d, 1, abs_scale)
        assert rc == 0 and _untouched(verts, N) and _untouched(rm, N)
        assert np.array_equal(verts[:N].cpu().numpy(), want["verts"].numpy())
        assert np.array_equal(rm[:N].cpu().numpy(), want["rotmat"].numpy())
        rc, v2, _ = _rigid_fwd(d, 1, abs_scale, rotmat=False)
        assert rc == 0 and torch.equal(v2, verts)
        w64 = pr.rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], 1, abs_scale)
        _within(f"rigid fwd N={N} V={V} abs={abs_scale}", verts[:N], w64["verts"], RIGID_BAR["verts"])
    if N > 1:
        rc, one_clip, _ = _rigid_fwd(d, 0, True)                             # clip_len 0: one clip, the first scale throughout
        w = pr.rigid_oracle32(dict(d, scale=d["scale"][:1], terms=(), weights=()), 0, True, with_twin=False)
        assert rc == 0 and np.array_equal(one_clip[:N].cpu().numpy(), w["verts"].numpy())


def _check_rigid_grads(tag, out, want, N, keys=("g_mesh", "g_rot6d", "g_trans", "g_scale"), extra_abs=None):
    for k in keys:
        _within(f"{tag} {k}", out[k][:N], want[k], RIGID_BAR[k], (extra_abs or {}).get(k, 0.0))


@pytest.mark.parametrize("N,V", pr.RIGID_BWD)
def test_rigid_backward_at_every_launch_geometry(N, V):
    """k_rigid_bwd<false> through hm_rigid_bwd_clips where threads and chunks change: 256 threads up to V = 512, 1024 above; with
    a workspace one chunk up to V = 4096, two at 4097, sixteen at 61441; workspace = NULL is one workgroup per frame.  All four
    gradients against float64, with and without the workspace; g_mesh is element-wise, so the two runs give the same bits; a
    negative scale under abs_scale flips the sign of its scale gradient and nothing else; a second run on the same workspace
    with other weights equals one on a fresh workspace."""
    d = pr.rigid_bwd_inputs(N, V)
    want = pr.rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], 1, True, d["terms"], d["weights"], d["g_rigid"], d["g_frame"],
                        d["frame_scale"])
    rc, with_ws, ws = _rigid_bwd(d, 1, True)
    rc2, without, _ = _rigid_bwd(d, 1, True, workspace=False)
    assert rc == 0 and rc2 == 0 and _pad_ok(ws)
    for k, t in list(with_ws.items()) + list(without.items()):
        assert _untouched(t, N), k
    _check_rigid_grads(f"rigid bwd N={N} V={V} workspace", with_ws, want, N)
    _check_rigid_grads(f"rigid bwd N={N} V={V} no workspace", without, want, N)
    assert torch.equal(with_ws["g_mesh"], without["g_mesh"])
    assert d["scale"][-1] < 0
    rc, pos, _ = _rigid_bwd(dict(d, scale=np.abs(d["scale"])), 1, True)
    assert rc == 0 and torch.equal(pos["g_scale"][N - 1], -with_ws["g_scale"][N - 1]) and bool(pos["g_scale"][N - 1] != 0)
    assert torch.equal(pos["g_scale"][:N - 1], with_ws["g_scale"][:N - 1])
    for k in ("g_mesh", "g_rot6d", "g_trans"):
        assert torch.equal(pos[k], with_ws[k]), k
    rc, raw, _ = _rigid_bwd(d, 1, False)                                     # no abs: the signed scale itself
    wr = pr.rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], 1, False, d["terms"], d["weights"], d["g_rigid"], d["g_frame"],
                      d["frame_scale"])
    assert rc == 0
    _check_rigid_grads(f"rigid bwd N={N} V={V} signed scale", raw, wr, N)
    w2 = np.asarray([-0.4, 2.1], np.float32)
    rc, second, _ = _rigid_bwd(d, 1, True, ws=ws, weights=w2)
    rc2, fresh, _ = _rigid_bwd(d, 1, True, weights=w2)
    assert rc == 0 and rc2 == 0 and _pad_ok(ws)
    for k in second:
        assert torch.equal(second[k], fresh[k]) and not torch.equal(second[k], with_ws[k]), k


def _exact_bwd(d, clip_len, workspace=True, ws=None, smooth=None, extra_terms=()):
    """hm_rigid_bwd_sil_clips (abs_scale, default quantum) -> rc, dict(g_rot6d, g_trans, g_scale) guarded, workspace"""
    from oracle import objchain
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    N, V = d["mesh"].shape[:2]
    F = len(d["faces"])
    adj = objchain.build_adjacency(d["faces"], V)
    out = dict(g_rot6d=_guarded(N, 3, 2), g_trans=_guarded(N, 3), g_scale=_guarded(N))
    if workspace and ws is None:
        ws = _zero_ws(L.hm_rigid_workspace_bytes(N))
    terms = list(extra_terms) + [(_dev(t), w) for t, w in zip(d["terms"], d["weights"])]
    tp, tw, tn = hl.terms(terms)
    keep = [_dev(x) for x in (d["mesh"], d["rot6d"], d["scale"], d["parts"], adj[0], adj[1], d["cam_verts"], d["K"])]
    rc = L.hm_rigid_bwd_sil_clips(P(keep[0]), P(keep[1]), P(keep[2]), 1, tp, tw, tn, P(keep[3]), P(keep[4]), P(keep[5]), P(keep[6]),
                                  P(keep[7]), float(d["orig_size"]), F, N, V, P(out["g_rot6d"]), P(out["g_trans"]), P(out["g_scale"]),
                                  P(ws) if workspace else None, clip_len, 0, P(smooth), float(pr.SMOOTH_WEIGHT if smooth is not None else 0.0),
                                  hl.stream())
    torch.cuda.synchronize()
    return rc, out, ws


def _exact_abs(d, V):
    """the quantisation allowance: half a quantum per addend of each of the 13 sums"""
    q = V * 2.0 ** -45
    return dict(g_trans=q, g_scale=q, g_rot6d=q * float(pr.rot6d_gain(d["rot6d"]).max()))


@pytest.mark.parametrize("V", pr.RIGID_EXACT_V)
def test_rigid_backward_exact_sums_give_the_same_bits_on_every_path(V):
    """hm_rigid_bwd_sil_clips, N = 2, per-corner sums that are multiples of the quantum on a generated mesh with an isolated vertex
    and one of valence > 8.  With / without a workspace the sizes reach k_rigid_bwd_x<1,1024> with one chunk (256, both) and
    several (257 and 4096 with), k_rigid_bwd_x<2,768> (4097 and 24576 with), k_rigid_bwd<true> with one chunk (257 .. 24577
    without) and with sixteen strided chunks (24577 with): every path at one V gives the same bits, the bits of
    oracle.objchain.rigid_bwd_sil_exact (a plain loop over frames and vertices: no size limit of its own; one scale per call, so
    it is called per frame), within the float64 reference's allowance; a second run on the same workspace equals the first."""
    from oracle import objchain
    d = pr.exact_inputs(2, V)
    extra, adj = pr.exact_extra(d)
    val = np.diff(adj[0])
    assert val[0] == 0 and val.max() > 8 and d["scale"][-1] < 0
    assert not (np.round(d["parts"] / pr.QUANTUM) * pr.QUANTUM != d["parts"]).any()
    want = pr.rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], 1, True, d["terms"], d["weights"], g_full_extra=extra)
    rc, a, ws = _exact_bwd(d, 1)
    rc2, b, _ = _exact_bwd(d, 1, workspace=False)
    rc3, c, _ = _exact_bwd(d, 1, ws=ws)
    assert rc == 0 and rc2 == 0 and rc3 == 0 and _pad_ok(ws)
    for k in a:
        assert _untouched(a[k], 2) and torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    _check_rigid_grads(f"rigid exact V={V}", a, want, 2, ("g_rot6d", "g_trans", "g_scale"), _exact_abs(d, V))
    for n in range(2):
        sl = slice(n, n + 1)
        g6, gt, gs, _ = objchain.rigid_bwd_sil_exact(d["mesh"][sl], d["rot6d"][sl].reshape(1, 6), float(d["scale"][n]), 1,
                                                     [(t[sl], w) for t, w in zip(d["terms"], d["weights"])], d["parts"][sl], adj,
                                                     d["cam_verts"][sl], d["K"][sl], d["orig_size"], len(d["faces"]))
        assert np.array_equal(a["g_rot6d"][n].cpu().numpy().reshape(6), g6[0]), n
        assert np.array_equal(a["g_trans"][n].cpu().numpy(), gt[0]) and a["g_scale"][n].item() == gs[0], n


@pytest.mark.parametrize("N,clip_len,V", pr.SMOOTH_CASES)
def test_rigid_backward_forms_the_smoothness_term_itself(N, clip_len, V):
    """k_rigid_bwd_x with smooth_verts: a clip of one frame (no pair, zero term: the bits of a launch without it), one pair, three
    clips of three (no pair across a clip boundary), and the two-vertices-per-thread instantiation: against float64, and
    bit-equal to the same launch without smooth_verts when hm_smooth_fwd_clips' unit gradient is passed as the first weighted
    term.  A launch that falls through to k_rigid_bwd<true> (V = 257 without a workspace) refuses smooth_verts."""
    from homan_amd.clipbatch import ClipReduceWorkspace
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    d = pr.exact_inputs(N, V, seed=2, clip_len=clip_len)
    extra = pr.exact_extra(d, clip_len, True)[0]
    want = pr.rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], clip_len, True, d["terms"], d["weights"], g_full_extra=extra)
    cam = _dev(d["cam_verts"])
    rc, got, ws = _exact_bwd(d, clip_len, smooth=cam)
    assert rc == 0 and _pad_ok(ws) and all(_untouched(t, N) for t in got.values())
    _check_rigid_grads(f"smooth N={N} clip_len={clip_len} V={V}", got, want, N, ("g_rot6d", "g_trans", "g_scale"), _exact_abs(d, V))
    if clip_len == 1:
        rc, plain, _ = _exact_bwd(d, clip_len)
    else:
        clips = N // clip_len
        unit, val = torch.full((N, V, 3), SENT, device=DEV), torch.zeros(clips, device=DEV)
        rws = ClipReduceWorkspace(DEV, clips)
        rc = L.hm_smooth_fwd_clips(P(cam), N, V, 1, P(unit), P(val), P(rws.buf), clip_len, 1, hl.stream())
        torch.cuda.synchronize()
        assert rc == 0
        _within(f"smooth N={N} clip_len={clip_len} V={V} unit gradient", float(np.float32(pr.SMOOTH_WEIGHT)) * unit.double(),
                pr.smooth_grad_ref(d["cam_verts"], clip_len, pr.SMOOTH_WEIGHT), 2.0 ** -23)
        rc, plain, _ = _exact_bwd(d, clip_len, extra_terms=[(unit, pr.SMOOTH_WEIGHT)])
    assert rc == 0
    for k in got:
        assert torch.equal(plain[k], got[k]), k
    if V == 257:
        rc, out, _ = _exact_bwd(d, clip_len, workspace=False, smooth=cam)
        assert rc == BAD_ARG and all(_untouched(t) for t in out.values())


@pytest.mark.parametrize("kind", sorted(pr.DEGENERATE_ROT6D))
def test_rigid_degenerate_rot6d(kind):
    """First column exactly zero, and second column an exact multiple of the first ((1,0,0) and (2,0,0): u exactly zero): the
    forward bit-equal to the oracle's, the backward finite and equal to float32 torch autograd of the oracle's rot6d_to_matrix in
    its x / clamp_min(|x|, 1e-12) form (oracle.model.REFERENCE_FORM; tests/test_posechain_refs.py shows it finite there and its
    clamp gradient to be the kernels' `else` branches) within FACTOR + 1 floors - the kernel's FACTOR and the float32 reference's
    own one - and within FACTOR floors of the float64 reference."""
    d = pr.degenerate_inputs(kind)
    N = d["mesh"].shape[0]
    o32 = refs._degenerate_oracle32(d)
    written = pr.rigid_oracle32(d, 1, True)
    rc, verts, rm = _rigid_fwd(d, 1, True)
    assert rc == 0 and np.array_equal(verts[:N].cpu().numpy(), written["verts"].numpy())
    assert np.array_equal(rm[:N].cpu().numpy(), written["rotmat"].numpy())
    want = pr.rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], 1, True, d["terms"], d["weights"], d["g_rigid"], d["g_frame"],
                        d["frame_scale"])
    for workspace in (True, False):
        rc, got, _ = _rigid_bwd(d, 1, True, workspace=workspace)
        assert rc == 0
        for k in ("g_mesh", "g_rot6d", "g_trans", "g_scale"):
            g = got[k][:N].cpu().double().numpy()
            w = o32[k].double().numpy().reshape(g.shape)
            err, scale = np.abs(g - w).max(), np.abs(w).max()
            print(f"degenerate {kind} workspace={workspace} {k}: vs float32 autograd {err / scale:.3e} (bar {(FACTOR + 1) * RIGID_BAR[k]:.1e})")
            assert np.isfinite(g).all() and err <= (FACTOR + 1) * RIGID_BAR[k] * scale, k
        _check_rigid_grads(f"degenerate {kind} workspace={workspace}", got, want, N)
        assert float(got["g_rot6d"][:N].abs().max()) > 1e11


def test_rigid_entry_points_refuse_bad_arguments():
    """HM_ERR_BAD_ARG, outputs at their sentinel, workspace still zero: n_terms > 5, g_frame with frame_stride < 3, a clip_len
    that does not divide N (forward and backward)."""
    d = pr.rigid_bwd_inputs(3, 257)
    for kw, cl in ((dict(n_terms=6), 1), (dict(frame_stride=2), 1), ({}, 2)):
        rc, out, ws = _rigid_bwd(d, cl, True, **kw)
        assert rc == BAD_ARG and all(_untouched(t) for t in out.values()) and not ws[:-PAD].any()
    rc, verts, rm = _rigid_fwd(d, 2, True)
    assert rc == BAD_ARG and _untouched(verts) and _untouched(rm)
