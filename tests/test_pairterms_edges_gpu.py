"""Hand-object pair terms at the shapes and edges the rest of the suite does not reach: the nearest-vertex search (nn_full_body /
nn_min_body, csrc/pair_bodies.h), the contact loss (csrc/contact.hip) and the SDF interpenetration loss (csrc/sdf.hip).

References: tests/util.py (float32 brute force for the search, float64 torch for contact and for the SDF sampling on the oracle's
grids), checked against the CPU oracle in tests/test_pairterms_refs.py, which also measures the float32 floors E32_*.  Whatever
is stated as identical (same float, same bits, exact zero, untouched) is torch.equal / array_equal; a comparison with a float64
reference allows E32_FACTOR times the floor of its group (deviation = max |difference| / max |reference| per tensor, no element
exempt), g_obj additionally Vh * 2^-45 absolute for its fixed-point accumulation (half a quantum of 2^-44 per addend).
"""
import numpy as np
import pytest
import torch

from tests import test_pairterms_refs as refs
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG, UNSUPPORTED = -1, -3          # HM_ERR_BAD_ARG, HM_ERR_UNSUPPORTED of include/homan_amd.h
FACTOR = refs.E32_FACTOR


def _dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x)) if not isinstance(x, torch.Tensor) else x
    return t.to(device=DEV, dtype=dtype).contiguous() if dtype is not None else t.to(DEV).contiguous()


# ===================================================================== A. nearest-vertex search
def _nn_raw(vh, vo, full=True, clip_len=0, stride=0, clips=1, order=None, sentinel=-7.0):
    """hm_nn_fwd_clips on device tensors -> rc, idx, d2, out (clips * max(stride, 1) floats, sentinel-filled)"""
    from homan_amd import lib as hl
    from homan_amd.clipbatch import ClipReduceWorkspace
    B, Vh, Vo = vh.shape[0], vh.shape[1], vo.shape[1]
    idx = torch.full((B, Vh), -5, dtype=torch.int32, device=DEV) if full else None
    d2 = torch.full((B, Vh), sentinel, device=DEV) if full else None
    out = torch.full((clips * max(stride, 1),), sentinel, device=DEV)
    ws = ClipReduceWorkspace(DEV, clips)
    rc = hl.lib().hm_nn_fwd_clips(hl.ptr(vh), hl.ptr(vo), B, Vh, Vo, hl.ptr(idx), hl.ptr(d2), hl.ptr(out), hl.ptr(ws.buf), clip_len,
                                  stride, hl.ptr(order), hl.stream())
    torch.cuda.synchronize()
    return rc, idx, d2, out


@pytest.mark.parametrize("Vh,Vo", util.NN_SHAPES)
def test_full_search_is_the_float32_brute_force(Vh, Vo):
    """k_nn at B = 3: nn_d2 has the bits of ((ox-hx)^2 + (oy-hy)^2) + (oz-hz)^2 in float32, nn_idx is the first argmin, the metric is
    max_b sqrt32(min d2); in float64 the picked pair is within 1e-6 (relative) of the true minimum.  Vh off and on the 128 of a
    workgroup, Vo below the wave count (empty shares), around a 64-group, one past 4096."""
    from homan_amd import ops
    vh, vo = util.nn_clouds(3, Vh, Vo)
    want_i, want_d, want_m = util.nn_bruteforce32(vh, vo)
    idx, d2, metric = ops.nearest_vertices(_dev(vh), _dev(vo), ops.ReduceWorkspace(DEV))
    assert np.array_equal(d2.cpu().numpy(), want_d)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), want_i)
    assert metric.cpu().numpy()[0] == want_m, (metric.item(), want_m)
    d64 = ((vh.astype(np.float64)[:, :, None] - vo.astype(np.float64)[:, None]) ** 2).sum(-1)
    picked = np.take_along_axis(d64, idx.cpu().numpy().astype(np.int64)[..., None], 2)[..., 0]
    assert (picked - d64.min(2) <= 1e-6 * d64.min(2) + 1e-12).all()


@pytest.mark.parametrize("Vo", [300, 1024])
def test_full_search_ties_keep_the_lowest_index(Vo):
    """Lattice clouds: every squared distance is exact and every object point is there many times over, so equal minima fall into
    different waves' shares and into different 64-groups of one share (util.nn_tie_spread) - the lowest index wins."""
    from homan_amd import ops
    vh, vo = util.nn_tie_clouds(3, 129, Vo)
    want_i, want_d, want_m = util.nn_bruteforce32(vh, vo)
    d64 = ((vh.astype(np.float64)[:, :, None] - vo.astype(np.float64)[:, None]) ** 2).sum(-1)
    assert np.array_equal(want_d.astype(np.float64), d64.min(2)) and np.array_equal(want_i, d64.argmin(2))      # exact
    across_waves, across_groups = util.nn_tie_spread(d64)
    assert across_waves > 100 and across_groups > 20
    idx, d2, metric = ops.nearest_vertices(_dev(vh), _dev(vo), ops.ReduceWorkspace(DEV))
    assert np.array_equal(d2.cpu().numpy(), want_d)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), want_i)
    assert metric.cpu().numpy()[0] == want_m


@pytest.mark.parametrize("Vo", [1, 63, 65, 4096])
def test_metric_only_search_returns_the_full_searchs_float(Vo):
    """k_nn_min (nn_idx = nn_d2 = NULL), with and without a random obj_order: the same float as the full search and as the brute
    force, for one group, a short one, one past a group, and all 64 groups."""
    Vh, B = 129, 3
    vh, vo = util.nn_clouds(B, Vh, Vo, seed=1)
    want_m = util.nn_bruteforce32(vh, vo)[2]
    vh_d, vo_d = _dev(vh), _dev(vo)
    rc, _, _, full = _nn_raw(vh_d, vo_d)
    assert rc == 0 and full.cpu().numpy()[0] == want_m
    perm = torch.from_numpy(np.random.default_rng(Vo).permutation(Vo).astype(np.int32)).to(DEV)
    for order in (None, perm):
        rc, _, _, out = _nn_raw(vh_d, vo_d, full=False, order=order)
        assert rc == 0 and torch.equal(out, full), (order is not None, out.item(), full.item())


def test_search_refuses_what_it_cannot_hold_before_any_launch():
    """HM_ERR_UNSUPPORTED, outputs untouched: a metric-only search over more than 4096 object vertices; clip frames x ceil(Vh / 128)
    = 513 (171 x 3) and 514 (257 x 2) block minima for the 512 slots of a clip - while 512 (256 x 2) runs and is right."""
    vh, vo = util.nn_clouds(3, 129, 4097)
    rc, _, _, out = _nn_raw(_dev(vh), _dev(vo), full=False)
    assert rc == UNSUPPORTED and bool((out == -7.0).all())
    for frames, Vh in ((171, 300), (257, 129)):
        vh, vo = util.nn_clouds(frames, Vh, 5)
        assert frames * ((Vh + 127) // 128) in (513, 514)
        for full in (True, False):
            rc, idx, d2, out = _nn_raw(_dev(vh), _dev(vo), full=full, clip_len=frames, stride=1)
            assert rc == UNSUPPORTED and bool((out == -7.0).all())
            if full:
                assert bool((idx == -5).all()) and bool((d2 == -7.0).all())
    vh, vo = util.nn_clouds(256, 256, 5)
    want_i, want_d, want_m = util.nn_bruteforce32(vh, vo)
    for full in (True, False):
        rc, idx, d2, out = _nn_raw(_dev(vh), _dev(vo), full=full, clip_len=256, stride=1)
        assert rc == 0 and out.cpu().numpy()[0] == want_m
        if full:
            assert np.array_equal(idx.cpu().numpy().astype(np.int64), want_i) and np.array_equal(d2.cpu().numpy(), want_d)


@pytest.mark.parametrize("full", [True, False])
def test_search_clips_are_single_clip_calls(full):
    """hm_nn_fwd_clips, C = 3 clips of 2 frames, out_stride 5: slot 5 c holds the metric of a single-clip call on clip c's frames (and
    the brute force's), every other slot is untouched."""
    C, CL, stride, Vh, Vo = 3, 2, 5, 129, 257
    vh, vo = util.nn_clouds(C * CL, Vh, Vo, seed=2)
    vh_d, vo_d = _dev(vh), _dev(vo)
    rc, idx, d2, out = _nn_raw(vh_d, vo_d, full=full, clip_len=CL, stride=stride, clips=C)
    assert rc == 0
    out = out.reshape(C, stride)
    assert bool((out[:, 1:] == -7.0).all())
    for c in range(C):
        sl = slice(c * CL, (c + 1) * CL)
        rc, idx1, d21, one = _nn_raw(vh_d[sl].contiguous(), vo_d[sl].contiguous(), full=full)
        assert rc == 0 and torch.equal(one[0], out[c, 0])
        assert out[c, 0].cpu().numpy() == util.nn_bruteforce32(vh[sl], vo[sl])[2]
        if full:
            assert torch.equal(idx[sl], idx1) and torch.equal(d2[sl], d21)
    assert len(set(out[:, 0].tolist())) == C


# ===================================================================== B. contact
def _contact_raw(vh, vo, nn, clip_len=0, stride=0, clips=1, thresh=util.CONTACT_THRESH):
    """hm_contact_fwd_clips -> rc, g_hand, g_obj, out (sentinel-filled before the call)"""
    from homan_amd import lib as hl
    from homan_amd.clipbatch import ClipReduceWorkspace
    B, Vh, Vo = vh.shape[0], vh.shape[1], vo.shape[1]
    gh, go = torch.full((B, Vh, 3), -7.0, device=DEV), torch.full((B, Vo, 3), -7.0, device=DEV)
    out = torch.full((clips * max(stride, 1),), -7.0, device=DEV)
    ws = ClipReduceWorkspace(DEV, clips)
    rc = hl.lib().hm_contact_fwd_clips(hl.ptr(vh), hl.ptr(vo), hl.ptr(nn), B, Vh, Vo, float(thresh), hl.ptr(gh), hl.ptr(go),
                                       hl.ptr(out), hl.ptr(ws.buf), clip_len, stride, hl.stream())
    torch.cuda.synchronize()
    return rc, gh, go, out


def _check_contact(tag, vh, vo, nn, got, want):
    """loss, g_hand, g_obj of the kernels against the float64 reference, at FACTOR x the float32 floors (+ the fixed-point bound)"""
    loss, gh, go = (t.cpu().double().numpy() for t in got)
    wl, wh, wo = (t.numpy() for t in want)
    Vh = vh.shape[1]
    d_l, d_h = util.deviation(loss, wl), util.deviation(gh, wh)
    err_o, scale_o = np.abs(go - wo).max(), np.abs(wo).max()
    print(f"contact {tag}: loss {loss.ravel()[0]:.9g} deviation {d_l:.3e} (bar {FACTOR * refs.E32_CONTACT:.1e}) g_hand {d_h:.3e} "
          f"g_obj {err_o / scale_o:.3e} (bar {FACTOR * refs.E32_CONTACT_GRAD:.1e})")
    assert np.isfinite(gh).all() and np.isfinite(go).all()
    assert d_l <= FACTOR * refs.E32_CONTACT, tag
    assert d_h <= FACTOR * refs.E32_CONTACT_GRAD, tag
    assert err_o <= FACTOR * refs.E32_CONTACT_GRAD * scale_o + Vh * 2.0 ** -45, tag
    picked = np.zeros(vo.shape[:2], bool)
    np.put_along_axis(picked, nn.astype(np.int64), True, 1)
    assert not go[~picked].any(), tag                                   # exact zeros on vertices nobody picked


@pytest.mark.parametrize("Vo", util.CONTACT_VO)
def test_contact_matches_the_float64_reference(Vo):
    """hm_contact_fwd for Vh in (1, 255, 257, 778) x B in (1, 3), picks given, a / thresh log-uniform over [1e-4, 20]: Vo = 1, 64 and
    4096 take the one-launch kernel (one range of object vertices), 4097 two ranges with a tail of one, 9000 three."""
    from homan_amd import ops
    rws = ops.ReduceWorkspace(DEV)
    for Vh in util.CONTACT_VH:
        for B in util.CONTACT_B:
            vh, vo, nn = util.contact_scene(B, Vh, Vo)
            want = util.contact_ref(vh, vo, nn)
            a, b = _dev(vh).requires_grad_(True), _dev(vo).requires_grad_(True)
            loss = ops.contact_loss(a, b, _dev(nn), rws)                 # (one workspace through all shapes: the ticket resets)
            loss.sum().backward()
            _check_contact(f"B={B} Vh={Vh} Vo={Vo}", vh, vo, nn, (loss.detach(), a.grad, b.grad), want)


@pytest.mark.parametrize("Vo,kind,zeros", [(4096, "same", 0), (9000, "same", 0), (9000, "last_range", 0), (64, "random", 5),
                                           (4097, "random", 5)])
def test_contact_skewed_picks_and_coincident_pairs(Vo, kind, zeros):
    """778 hand vertices that all pick ONE object vertex (778 fixed-point addends into one slot), picks in the last range only, and
    pairs at distance 0: the kernels' gradients are exactly 0 there (the reference's subgradient) and finite everywhere."""
    B, Vh = 3, 778
    vh, vo, nn = util.contact_scene(B, Vh, Vo, kind, zeros=zeros)
    want = util.contact_ref(vh, vo, nn)
    rc, gh, go, out = _contact_raw(_dev(vh), _dev(vo), _dev(nn))
    assert rc == 0
    _check_contact(f"B={B} Vh={Vh} Vo={Vo} {kind} zeros={zeros}", vh, vo, nn, (out, gh, go), want)
    if kind == "last_range":
        assert nn.min() >= 8192 and not go[:, :8192].any()
    if kind == "same":
        assert int((go.abs().sum(-1) != 0).sum()) == B
    if zeros:
        dead = torch.from_numpy((np.take_along_axis(vo, nn[..., None].astype(np.int64).repeat(3, -1), 1) == vh).all(-1))
        assert int(dead.sum()) == B * zeros and not gh.cpu()[dead].any() and not want[1][dead].any()


def test_contact_one_range_and_two_range_paths_agree():
    """The Vo = 4096 scene through k_contact_both, and with one far, unpicked vertex appended (Vo = 4097) through k_contact_hand +
    k_contact_obj: loss, g_hand and g_obj[:, :4096] bit for bit, g_obj[:, 4096] exactly 0."""
    vh, vo, nn = util.contact_scene(3, 778, 4096)
    vo2 = np.concatenate([vo, np.full((3, 1, 3), 50.0, np.float32)], 1)
    rc1, gh1, go1, out1 = _contact_raw(_dev(vh), _dev(vo), _dev(nn))
    rc2, gh2, go2, out2 = _contact_raw(_dev(vh), _dev(vo2), _dev(nn))
    assert rc1 == 0 and rc2 == 0 and float(out1) > 0
    assert torch.equal(out1, out2) and torch.equal(gh1, gh2) and torch.equal(go1, go2[:, :4096])
    assert not go2[:, 4096].any() and bool((go1 != 0).any())


@pytest.mark.parametrize("Vo", [64, 4097])
def test_contact_clips_are_single_clip_calls(Vo):
    """hm_contact_fwd_clips, C = 3 clips of 2 frames, out_stride 5, both launch shapes: per-clip loss and gradients are the bits of
    single-clip calls (the mean runs over clip_len * Vh, not over the batch), other slots untouched."""
    C, CL, stride, Vh = 3, 2, 5, 257
    vh, vo, nn = util.contact_scene(C * CL, Vh, Vo, seed=3)
    vh_d, vo_d, nn_d = _dev(vh), _dev(vo), _dev(nn)
    rc, gh, go, out = _contact_raw(vh_d, vo_d, nn_d, clip_len=CL, stride=stride, clips=C)
    assert rc == 0
    out = out.reshape(C, stride)
    assert bool((out[:, 1:] == -7.0).all())
    want = util.contact_ref(vh, vo, nn, clip_len=CL)
    for c in range(C):
        sl = slice(c * CL, (c + 1) * CL)
        rc, gh1, go1, one = _contact_raw(vh_d[sl].contiguous(), vo_d[sl].contiguous(), nn_d[sl].contiguous())
        assert rc == 0 and torch.equal(one[0], out[c, 0]) and torch.equal(gh1, gh[sl]) and torch.equal(go1, go[sl])
    _check_contact(f"clips Vo={Vo}", vh, vo, nn, (out[:, 0], gh, go), want)


def test_contact_refuses_a_clip_longer_than_its_partials():
    """clip_len = 513 frames for the 512 per-frame partial sums of a clip: HM_ERR_BAD_ARG, nothing written"""
    vh, vo, nn = util.contact_scene(513, 1, 1)
    rc, gh, go, out = _contact_raw(_dev(vh), _dev(vo), _dev(nn), clip_len=513, stride=1)
    assert rc == BAD_ARG and bool((gh == -7.0).all()) and bool((go == -7.0).all()) and bool((out == -7.0).all())
    rc, gh, go, out = _contact_raw(_dev(vh[:512]), _dev(vo[:512]), _dev(nn[:512]), clip_len=512, stride=1)
    assert rc == 0
    # (512 one-term partials added in float32: at most 512 roundings of 2^-24 each, in whatever order)
    np.testing.assert_allclose(out.item(), float(util.contact_ref(vh[:512], vo[:512], nn[:512])[0]), rtol=512 * 2.0 ** -24)


# ===================================================================== C. SDF interpenetration
def _unpack(words):
    """need-mask words (B,32,32) int32 [z][y] -> (B,32,32,32) bool [z][y][x]"""
    w = words.cpu().numpy().view(np.uint32)
    return ((w[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)


class _Run:
    """one hm_collision_fwd (+ dist_values, grids, lazy state) on a scene tuple"""

    def __init__(self, scene, scale_factor=0.2, cctx=None):
        from homan_amd import ops
        v0, f0, v1, f1 = scene
        self.B = len(v0)
        self.cctx = cctx if cctx is not None else ops.CollisionContext(f0, torch.from_numpy(f1), self.B, v0.shape[1], v1.shape[1], DEV)
        a, b = _dev(v0).requires_grad_(True), _dev(v1).requires_grad_(True)
        loss = ops.collision_loss(a, b, self.cctx, scale_factor)
        loss.backward()
        self.loss, self.g = loss.detach().clone(), [a.grad.clone(), b.grad.clone()]
        self.lazy = [tuple(t.clone() for t in self.cctx.needed(w)) for w in (0, 1)]      # before anything else touches the workspace
        self.grid = [self.cctx.grid(w).clone() for w in (0, 1)]
        dv = ops.collision_dist_values(a.detach(), b.detach(), self.cctx, scale_factor)
        self.dist = {k: v.clone() for k, v in dv.items()}
        self.lazy_after = [tuple(t.clone() for t in self.cctx.needed(w)) for w in (0, 1)]
        torch.cuda.synchronize()

    def bits(self):
        return [self.loss, *self.g, self.dist[(0, 1)], self.dist[(1, 0)]]


def _check_lazy(tag, run, scene, meta, scale_factor):
    """grids == the oracle's (brute-force debug kernel); the LAZY path (k_sdf_need + k_sdf_dist): need-mask == util.sdf_need_ref,
    list length == its popcount, and phi bit-equal to the full grid on every needed voxel"""
    verts = [scene[0], scene[2]]
    total = 0
    for w in (0, 1):
        ref = meta["sdfs"][w].float().clamp(min=0)
        assert torch.equal(run.grid[w].cpu(), ref), f"{tag}: full grid {w}"
        inside = (ref > 0).numpy()
        want = util.sdf_need_ref(verts[w], verts[1 - w], inside, scale_factor)
        for words, cnt, phi in (run.lazy[w], run.lazy_after[w]):
            need = _unpack(words)
            assert np.array_equal(need, want), f"{tag}: need-mask {w}: {need.sum()} vs {want.sum()}"
            assert np.array_equal(cnt.cpu().numpy(), want.reshape(run.B, -1).sum(1)), f"{tag}: list length {w}"
            sel = torch.from_numpy(need)
            assert torch.equal(phi.cpu()[sel], run.grid[w].cpu()[sel]), f"{tag}: lazy phi {w}"
        total += int(want.sum())
    return total


def _check_values(tag, run, scene, meta, scale_factor):
    want, gw, dist = util.sdf_scene_ref(meta["sdfs"], [scene[0], scene[2]], scale_factor)
    d_l = util.deviation(run.loss.cpu().double().numpy(), want.numpy())
    d_g = [util.deviation(g.cpu().double().numpy(), w.numpy()) for g, w in zip(run.g, gw)]
    d_v = [util.deviation(run.dist[k].cpu().double().numpy(), dist[k].numpy()) for k in ((0, 1), (1, 0))]
    print(f"sdf {tag}: loss {run.loss.item():.9g} deviation {d_l:.3e} (bar {FACTOR * refs.E32_SDF_LOSS:.1e}) gradients {d_g[0]:.3e} "
          f"{d_g[1]:.3e} (bar {FACTOR * refs.E32_SDF_GRAD:.1e}) values {d_v[0]:.3e} {d_v[1]:.3e} (bar {FACTOR * refs.E32_SDF_VALUES:.1e})")
    assert float(want) > 0
    assert d_l <= FACTOR * refs.E32_SDF_LOSS, tag
    assert max(d_g) <= FACTOR * refs.E32_SDF_GRAD, tag
    assert max(d_v) <= FACTOR * refs.E32_SDF_VALUES, tag
    for g, w in zip(run.g, gw):                                          # the same vertices carry a gradient
        assert torch.equal(g.cpu().abs().sum(-1) != 0, w.abs().sum(-1) != 0), tag
    return want, gw, dist


@pytest.mark.parametrize("name", util.SDF_SCENE_NAMES)
def test_collision_lazy_grid_and_values(name, mano_model):
    """Meshes of 4 / 8 vertices, F = 256 and 260, V0 > V1 with V1 < 256, the hand and the bottle in swapped slots, and the two
    scenes of test_ops_gpu: full grids == oracle, lazy evaluation == full grid where needed, need-mask and list length == numpy,
    loss / gradients / dist_values against the float64 reference."""
    scene = util.sdf_scenes(mano_model)[name]
    _, _, meta = util.oracle_sdf(scene)
    run = _Run(scene)
    assert _check_lazy(name, run, scene, meta, 0.2) > 0
    _check_values(name, run, scene, meta, 0.2)


def test_collision_octahedron_known_answer():
    """Unit octahedron at a power-of-two pose, scale_factor 0: voxel-centre rays run exactly through the edges of the projection.
    inside iff |x| + |y| + |z| < 1 (5440 voxels, exactly); phi = (1 - |x| - |y| - |z|) / sqrt 3 within FACTOR x E32_OCTA_PHI, on the
    full grid and on the lazily evaluated voxels."""
    scene = util.octahedron_scene()
    _, _, meta = util.oracle_sdf(scene, 0.0)
    run = _Run(scene, 0.0)
    inside, phi = util.octahedron_exact()
    for w in (0, 1):
        got = run.grid[w][0].cpu().numpy()
        assert np.array_equal(got > 0, inside) and int((got > 0).sum()) == util.OCTA_INSIDE
        err = np.abs(got - phi).max()
        print(f"octahedron grid {w}: |phi - exact| {err:.3e} (bar {FACTOR * refs.E32_OCTA_PHI:.1e})")
        assert err <= FACTOR * refs.E32_OCTA_PHI
    assert _check_lazy("octahedron", run, scene, meta, 0.0) > 0
    need = _unpack(run.lazy[0][0])[0]
    assert need.any() and np.abs(run.lazy[0][2][0].cpu().numpy() - phi)[need].max() <= FACTOR * refs.E32_OCTA_PHI
    _check_values("octahedron", run, scene, meta, 0.0)


def test_collision_disjoint_contained_and_far_frames():
    """B = 4: overlapping | disjoint | one mesh wholly inside the other | the second mesh 2^20 away (the index clamp before the
    int conversion).  Frames 1 and 3: exactly 0 loss, all-zero gradients, empty lists.  Every frame's gradients, dist_values,
    need-mask and list length are the bits of a B = 1 call on that frame alone."""
    scene = util.frames_scene()
    _, _, meta = util.oracle_sdf(scene)
    run = _Run(scene)
    _check_lazy("frames", run, scene, meta, 0.2)
    _check_values("frames", run, scene, meta, 0.2)
    v0, f0, v1, f1 = scene
    singles = []
    for f in range(4):
        one = _Run((v0[f:f + 1], f0, v1[f:f + 1], f1))
        singles.append(one)
        for k in (0, 1):
            assert torch.equal(one.g[k][0], run.g[k][f]), f
            assert torch.equal(one.lazy[k][0][0], run.lazy[k][0][f]) and torch.equal(one.lazy[k][1][0], run.lazy[k][1][f]), f
        for key in ((0, 1), (1, 0)):
            assert torch.equal(one.dist[key][0], run.dist[key][f]), f
    for f in (1, 3):
        assert singles[f].loss.item() == 0.0
        for k in (0, 1):
            assert not run.g[k][f].any() and int(run.lazy[k][1][f]) == 0 and not run.lazy[k][0][f].any()
    assert singles[0].loss.item() > 0 and singles[2].loss.item() > 0
    assert bool(run.g[1][2].any()) and not run.g[0][2].any()            # frame 2: only the contained mesh is pushed
    np.testing.assert_allclose(run.loss.item(), sum(s.loss.item() for s in singles), rtol=2 * FACTOR * refs.E32_SDF_LOSS)    # (either side within its bar of the float64 sum)


def test_collision_samples_in_the_border_shell():
    """Sample points at grid index -1, -0.5, -1e-3, 0, 30.999, 31, 31.5, 32 on each axis in turn, in an owner whose box fills its
    grid: values and gradients against float64 grid_sample (zeros padding, align_corners=False) on the oracle's grid - half
    weights in the shell, one-sided slopes at 0 and 31, nothing at -1 and 32."""
    scene, ix = util.shell_scene()
    _, _, meta = util.oracle_sdf(scene, 0.0)
    run = _Run(scene, 0.0)
    _check_lazy("shell", run, scene, meta, 0.0)
    want, gw, dist = _check_values("shell", run, scene, meta, 0.0)
    vals, grads = dist[(0, 1)][0, 4:].numpy(), gw[1][0, 4:].numpy()
    got_v, got_g = run.dist[(0, 1)][0, 4:].cpu().numpy(), run.g[1][0, 4:].cpu().numpy()
    for axis in range(3):
        v, g = vals[8 * axis:8 * axis + 8], grads[8 * axis:8 * axis + 8, axis]
        assert v[0] == 0 and v[7] == 0 and v[1] > 0 and v[6] > 0 and abs(v[1] / v[3] - 0.5) < 1e-12 and abs(v[6] / v[5] - 0.5) < 1e-12
        assert g[0] > 0 and g[3] == 2 * g[0] and g[5] == -g[0] and g[7] == 0        # one-sided at 0 and 31, slope phi[0] in the shell
        gv, gg = got_v[8 * axis:8 * axis + 8], got_g[8 * axis:8 * axis + 8, axis]
        assert gv[0] == 0 and gv[7] == 0 and gg[7] == 0 and not got_g[8 * axis + 7].any()      # exact zeros at -1 and 32
        assert gg[0] > 0 and gg[5] < 0 and gv[1] > 0 and gv[6] > 0       # (how close: _check_values above, no element exempt)


def test_collision_workspace_reuse(mano_model):
    """One CollisionContext: pose A, then pose B - loss, gradients, dist_values and the lazy phi on B's need-mask are the bits of a
    fresh context given B (masks, need-masks and the list are cleared, stale distances are never read); B twice in a row gives
    the same bits again (the ticket reset itself)."""
    scenes = util.sdf_scenes(mano_model)
    pose_a = scenes["hand_vs_box8"]
    v1 = (pose_a[2] * np.float32(0.8) + np.float32([0.01, -0.004, 0.125])).astype(np.float32)
    pose_b = (pose_a[0][::-1].copy(), pose_a[1], v1, pose_a[3])
    fresh = _Run(pose_b)
    first = _Run(pose_a)
    assert not torch.equal(first.lazy[0][0], fresh.lazy[0][0]) or not torch.equal(first.lazy[1][0], fresh.lazy[1][0])
    runs = [_Run(pose_b, cctx=first.cctx) for _ in range(2)]
    assert fresh.loss.item() > 0
    for r in runs:
        for x, y in zip(r.bits(), fresh.bits()):
            assert torch.equal(x, y)
        for w in (0, 1):
            assert torch.equal(r.lazy[w][0], fresh.lazy[w][0]) and torch.equal(r.lazy[w][1], fresh.lazy[w][1])
            sel = torch.from_numpy(_unpack(fresh.lazy[w][0]))
            assert sel.any() or w == 0
            assert torch.equal(r.lazy[w][2].cpu()[sel], fresh.lazy[w][2].cpu()[sel])


def test_collision_clips_are_single_clip_calls(mano_model):
    """hm_collision_fwd_clips, C = 3 clips of 2 frames, out_stride 5 (per-clip tickets, block records in (pair, frame, chunk) order,
    V0 = 778 / V1 = 252: four chunks): out[5 c] and the gradients are the bits of hm_collision_fwd on clip c's frames alone, every
    other slot is untouched."""
    from homan_amd import lib as hl
    from homan_amd import ops
    C, CL, stride = 3, 2, 5
    v0, f0, v1, f1 = util.sdf_scenes(mano_model)["ops_cube"]
    rng = np.random.default_rng(8)
    v0 = np.concatenate([v0, v0[::-1] + np.float32([0.004, 0.0, -0.003])]).astype(np.float32)
    v1 = np.concatenate([v1, v1 + rng.normal(size=(3, 1, 3)).astype(np.float32) * np.float32(0.006)]).astype(np.float32)
    B, V0, V1 = C * CL, v0.shape[1], v1.shape[1]
    cctx = ops.CollisionContext(f0, torch.from_numpy(f1), B, V0, V1, DEV)
    a, b = _dev(v0), _dev(v1)
    g0, g1 = torch.full_like(a, -7.0), torch.full_like(b, -7.0)
    out = torch.full((C * stride,), -7.0, device=DEV)
    for _ in range(2):                                                   # (twice: the per-clip tickets reset themselves)
        hl.check(hl.lib().hm_collision_fwd_clips(hl.ptr(a), hl.ptr(cctx.f0), V0, cctx.f0.shape[0], hl.ptr(b), hl.ptr(cctx.f1), V1,
                                                 cctx.f1.shape[0], B, 0.2, hl.ptr(g0), hl.ptr(g1), hl.ptr(out), hl.ptr(cctx.ws), CL,
                                                 stride, hl.stream()), "hm_collision_fwd_clips")
        torch.cuda.synchronize()
        res = out.reshape(C, stride)
        assert bool((res[:, 1:] == -7.0).all())
        for c in range(C):
            sl = slice(c * CL, (c + 1) * CL)
            one = _Run((v0[sl], f0, v1[sl], f1))
            assert one.loss.item() > 0 and torch.equal(one.loss, res[c, 0]), (c, one.loss.item(), res[c, 0].item())
            assert torch.equal(one.g[0], g0[sl]) and torch.equal(one.g[1], g1[sl])
        assert len(set(res[:, 0].tolist())) == C
