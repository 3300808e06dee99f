"""The two gradient kernels on the tail of the fused iteration, bit for bit against the CPU oracle's written-out chains, at the
smallest shapes at which their finishing code can go wrong.

k_rigid_bwd_x (csrc/geometry.hip, through hm_rigid_bwd_sil_clips): wave 0 of a frame's last workgroup stores / reloads the chunk
records with 13 lanes and draws the ticket without a barrier.  V = 8 (one partly filled workgroup), 257 (two chunks), 1025 (five)
and 2049 (nine): one chunk, the smallest several and the sizes around 1024 and 2048 vertices where a launcher could switch to
one workgroup per frame; one and three frames, clips of one and of three frames, two clips; a mesh with an isolated vertex and one
of valence 12 (the corner tail behind the first eight); with and without the smoothness term formed inside the launch.  Mirror:
oracle.objchain.rigid_bwd_sil_exact (one scale per call: called per clip), the smoothness term as oracle.objchain.smooth_unit_grad
of the clip.

k_mano_bwd<false> / <true> (csrc/mano.hip, through hm_mano_bwd and hm_mano_bwd_rigid_clips): the frame's finishing workgroup
requests the chunk records, the PCA components and the joints' shape directions in one round trip and finishes on three waves.
B = 1, 3, 5 (the forward groups four frames), saved state and state = NULL, pca_dim 16 and 45 (the entry points refuse less than
the 16 components of the model, so the second width is the wider one: columns 16 .. 44 carry the prior's term alone), with and
without the PCA prior's term.  Mirrors: orc_mano_bwd_rows and orc_hand_chain (oracle/csrc/lbs_exact.c).

Every case runs twice on ONE workspace - the tickets re-arm themselves - and both runs must give the mirror's bits.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import posechain_ref as pr
from tests import test_posechain_edges_gpu as pe

pytestmark = pytest.mark.gpu
f32 = np.float32


# ===================================================================== k_rigid_bwd_x
def _mesh(V):
    """vertex 0 in no face, vertex 1 in a fan of 12 triangles over the pairs of vertices 2 .. 7 (valence 12 + the strip's), a strip
    (i, i+1, i+2) over 1 .. V-1 -> faces (F,3) int32"""
    assert V >= 8
    pairs = [(a, b) for a in range(2, 8) for b in range(a + 1, 8)][:12]
    fan = np.asarray([(1, a, b) for a, b in pairs])
    strip = np.stack([np.arange(1, V - 2), np.arange(2, V - 1), np.arange(3, V)], 1)
    return np.concatenate([strip, fan]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _rigid_inputs(N, V, clip_len):
    """pr.exact_inputs on the mesh above (computed once per shape, never modified)"""
    r = pr.rng(60, N, V, clip_len)
    faces = _mesh(V)
    rot6d, trans, scale = pr.rigid_pose(N, N // clip_len, seed=V)
    trans[:, 2] = (1.6 + 0.2 * r.random(N)).astype(f32)           # no vertex near the camera plane: 1 / z stays small (see below)
    mesh = (r.normal(size=(N, V, 3)) * 0.1).astype(f32)
    cam = pr.rigid_ref(mesh, rot6d, trans, scale, clip_len, True)["verts"].numpy().astype(f32)
    K = np.tile(np.array([[1.37, 0.02, 0.5], [0, 1.41, 0.48], [0, 0, 1.0]], f32), (N, 1, 1))
    parts = r.integers(-2 ** 34, 2 ** 34, size=(N, len(faces), 3, 2)).astype(np.float64) * pr.QUANTUM
    return dict(mesh=mesh, rot6d=rot6d, trans=trans, scale=scale, faces=faces, cam_verts=cam, K=K, parts=parts, orig_size=1.0,
                terms=[(r.normal(size=(N, V, 3)) * 1e-3).astype(f32) for _ in range(2)], weights=np.asarray([0.9, -1.7], f32))


def _rigid_mirror(d, clip_len, smooth):
    from oracle import objchain
    N, V = d["mesh"].shape[:2]
    adj = objchain.build_adjacency(d["faces"], V)
    g6, gt, gs = np.zeros((N, 6), f32), np.zeros((N, 3), f32), np.zeros(N, f32)
    for c in range(N // clip_len):
        sl = slice(c * clip_len, (c + 1) * clip_len)
        terms = [(t[sl], w) for t, w in zip(d["terms"], d["weights"])]
        if smooth:
            terms = [(objchain.smooth_unit_grad(d["cam_verts"][sl]), pr.SMOOTH_WEIGHT)] + terms
        g6[sl], gt[sl], gs[sl], gv = objchain.rigid_bwd_sil_exact(
            np.ascontiguousarray(d["mesh"][sl]), np.ascontiguousarray(d["rot6d"][sl].reshape(-1, 6)), float(d["scale"][c]), 1, terms,
            np.ascontiguousarray(d["parts"][sl]), adj, np.ascontiguousarray(d["cam_verts"][sl]), np.ascontiguousarray(d["K"][sl]),
            d["orig_size"], len(d["faces"]))
        # the sums are exact - the same bits in any order - while they stay below 2^53 quanta = 512.  gv = |s| R^T gf, so a component of
        # the vertex gradient gf is at most |gv|_1 / |s|, and every addend of the 13 sums is one times at most max(1, |s m|, |m|):
        # no partial sum, in any order, comes near the limit
        s, mmax = abs(float(d["scale"][c])), float(np.linalg.norm(d["mesh"][sl], axis=-1).max())
        assert np.abs(gv.astype(np.float64)).sum(axis=(1, 2)).max() / s * max(1.0, s * mmax, mmax) < 256.0
    return dict(g_rot6d=g6.reshape(N, 3, 2), g_trans=gt, g_scale=gs)


@pytest.mark.parametrize("N,clip_len", [(1, 1), (3, 1), (3, 3), (6, 3)])
@pytest.mark.parametrize("V", [8, 257, 1025, 2049])
def test_rigid_tail_gives_the_oracles_bits(V, N, clip_len):
    from oracle import objchain
    d = _rigid_inputs(N, V, clip_len)
    val = np.diff(objchain.build_adjacency(d["faces"], V)[0])
    assert val[0] == 0 and val[1] >= 12 and d["scale"][-1] < 0
    cam = pe._dev(d["cam_verts"])
    for smooth in (False, True):
        want = _rigid_mirror(d, clip_len, smooth)
        assert all(np.abs(w).max() > 0 for w in want.values())
        ws = None
        for run in range(2):
            rc, got, ws = pe._exact_bwd(d, clip_len, ws=ws, smooth=cam if smooth else None)
            assert rc == 0 and pe._pad_ok(ws)
            for k, w in want.items():
                assert pe._untouched(got[k], N), (k, smooth, run)
                assert np.array_equal(got[k][:N].cpu().numpy(), w), (k, smooth, run)
        if V <= 256:                                              # no workspace: one workgroup per frame, the same bits
            rc, lone, _ = pe._exact_bwd(d, clip_len, workspace=False, smooth=cam if smooth else None)
            assert rc == 0 and all(np.array_equal(lone[k][:N].cpu().numpy(), want[k]) for k in want)


# ===================================================================== k_mano_bwd
@functools.lru_cache(maxsize=None)
def _layout():
    from homan_amd.mano_assets import kernel_layout
    return kernel_layout(pr.mano_models()["right"], flat_hand_mean=False)


@functools.lru_cache(maxsize=None)
def _forward(B, pca_dim):
    """parameters, their device copies and the forward's mesh + saved state (once per shape)"""
    p = pr.mano_params(B, pca_dim, seed=11)
    pd = pe._pdev(p)
    rp = pr.rigid_pose(B, 1, seed=B, negative=False)
    rc, fw = pe._fwd(pe._mctx("right"), pd, B, world=tuple(pe._dev(x) for x in rp), clip_len=0)
    assert rc == 0
    return p, pd, rp, fw["verts"][:B].contiguous(), fw["state"][:B].contiguous()


def _extra(B, pca_dim):
    return pr.rng(12, B, pca_dim).normal(size=(B, pca_dim)).astype(f32)


def _mirror_outs(B, P):
    return dict(g_pca=np.zeros((B, P), f32), g_rot=np.zeros((B, 3), f32), g_betas=np.zeros((B, 10), f32), g_trans=np.zeros((B, 3), f32))


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("pca_dim", [16, 45])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_mano_backward_tail_gives_the_oracles_bits(B, pca_dim, prior):
    from oracle import clib
    p, pd, _, _, state = _forward(B, pca_dim)
    lay = _layout()
    extra, w_extra = (_extra(B, pca_dim), 1e-4) if prior else (None, 0.0)
    want = _mirror_outs(B, pca_dim)
    clib.lib().orc_mano_bwd_rows(*[clib.fptr(a) for a in lay[:7]], clib.iptr(lay[7]), clib.fptr(p["pca"]), pca_dim, clib.fptr(p["rot"]),
                                 clib.fptr(p["betas"]), clib.fptr(p["gout"]), clib.fptr(extra) if prior else None, float(w_extra), B,
                                 0, 1, *[clib.fptr(want[k]) for k in pe.GRADS])
    assert all(np.abs(w).max() > 0 for w in want.values())
    for st in (state, None):
        ws = None
        for run in range(2):
            rc, got, ws = pe._bwd(pe._mctx("right"), pd, B, pd["gout"], st, ws=ws, extra=pe._dev(extra), w_extra=w_extra)
            assert rc == 0 and pe._pad_ok(ws)
            for k in pe.GRADS:
                assert pe._untouched(got[k], B), (k, st is None, run)
                assert np.array_equal(got[k][:B].cpu().numpy(), want[k]), (k, st is None, run)


def _fused(B, pd, mesh, r6, rs, fi, state, ws, extra, w_extra):
    """hm_mano_bwd_rigid_clips with the PCA prior's term (pe._bwd_fused passes none)"""
    hl = pe._hl()
    L, P = hl.lib(), hl.ptr
    out = pe._grad_bufs(B, pd["pca"].shape[1])
    out.update(g_rot6d=pe._guarded(B, 3, 2), g_rigid_trans=pe._guarded(B, 3))
    ws = ws if ws is not None else pe._zero_ws(L.hm_mano_workspace_bytes(B))
    terms = [pe._dev(t) for t in fi["terms"]]
    tp, tw, tn = hl.terms(list(zip(terms, fi["weights"])))
    g_frame = pe._dev(fi["g_frame"])
    rc = L.hm_mano_bwd_rigid_clips(pe._mctx("right").ptrs, P(pd["pca"]), pd["pca"].shape[1], P(pd["rot"]), P(pd["betas"]), B, P(extra),
                                   float(w_extra), P(out["g_pca"]), P(out["g_rot"]), P(out["g_betas"]), P(out["g_trans"]), P(state),
                                   P(ws), P(mesh), P(r6), P(rs), tp, tw, tn, None, P(g_frame), fi["g_frame"].shape[1],
                                   float(fi["frame_scale"]), P(out["g_rot6d"]), P(out["g_rigid_trans"]), 0, hl.stream())
    torch.cuda.synchronize()
    return rc, out, ws


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("pca_dim", [16, 45])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_mano_backward_with_the_rigid_backward_tail_gives_the_oracles_bits(B, pca_dim, prior):
    from oracle import clib
    p, pd, rp, mesh, state = _forward(B, pca_dim)
    lay = _layout()
    fi = pr.fused_inputs(B, 2, False, 3, seed=pca_dim)
    extra, w_extra = (_extra(B, pca_dim), 1e-4) if prior else (None, 0.0)
    want = _mirror_outs(B, pca_dim)
    want.update(g_rot6d=np.zeros((B, 6), f32), g_rigid_trans=np.zeros((B, 3), f32))
    arrs = [np.ascontiguousarray(t, f32) for t in fi["terms"]]
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    mesh_h = np.ascontiguousarray(mesh.cpu().numpy())
    clib.lib().orc_hand_chain(*[clib.fptr(a) for a in lay[:7]], clib.iptr(lay[7]), clib.fptr(p["pca"]), pca_dim, clib.fptr(p["rot"]),
                              clib.fptr(p["betas"]), clib.fptr(mesh_h), clib.fptr(np.ascontiguousarray(rp[0].reshape(B, 6))),
                              float(rp[2][0]), ptrs, clib.fptr(np.ascontiguousarray(fi["weights"])), len(arrs), clib.fptr(fi["g_frame"]),
                              3, float(fi["frame_scale"]), clib.fptr(extra) if prior else None, float(w_extra), B,
                              *[clib.fptr(want[k]) for k in pe.GRADS], clib.fptr(want["g_rot6d"]), clib.fptr(want["g_rigid_trans"]))
    want["g_rot6d"] = want["g_rot6d"].reshape(B, 3, 2)
    assert all(np.abs(w).max() > 0 for w in want.values())
    r6, rs = pe._dev(rp[0]), pe._dev(rp[2])
    for st in (state, None):
        ws = None
        for run in range(2):
            rc, got, ws = _fused(B, pd, mesh, r6, rs, fi, st, ws, pe._dev(extra), w_extra)
            assert rc == 0 and pe._pad_ok(ws)
            for k, w in want.items():
                assert pe._untouched(got[k], B), (k, st is None, run)
                assert np.array_equal(got[k][:B].cpu().numpy(), w), (k, st is None, run)
