"""The kernels of csrc/surfcontact.hip (hm_surface_contact_fwd / _bwd), `ops.surface_contact_loss`, the term in `HOMan.forward`
and in the loops, against the NumPy restatement of tests/surfcontact_ref.py.

Bars.  The per-point detail, the two losses and all three gradients: equal, bit for bit - both sides perform the same fp32
operations in the same order and the sums are exact integer sums, so they do not depend on the order of the lanes.  A frame of
a batch against its call alone: the per-point detail outputs (value, bary, d2, face, inside) are compared directly - they carry
no 1 / (B N) - and the scaled outputs of the batch are held to the restatement, whose per-frame integer sums do not know of the
batch.  Against float64: util.E32_FACTOR times the floors the CPU file measured on the restatement (tests/test_surfcontact.py)."""
import numpy as np
import pytest
import torch

from tests import surfcontact_ref as cref
from tests import util
from tests.test_softsil_gpu import _clip, _close_as_the_two_loops, _fit, _model
from tests.test_surfcontact import E32, MESH_CASES
from tests.test_surfmetrics import DEGENERATE, comparison_cases, mesh, restated
from tests.test_surfmetrics_gpu import bits, cube_scene, three_poses

pytestmark = pytest.mark.gpu

F32 = np.float32
DETAIL = ("value", "bary", "d2", "face", "inside")
SCALED = (("loss", "out"), ("grad_points", "grad_points"), ("grad_verts_attr", "grad_verts_attr"),
          ("grad_verts_rep", "grad_verts_rep"))


def device(points, verts, faces, weights=None, **kw):
    """points (B,N,3) or (N,3), verts likewise -> the outputs of ops.surface_contact_terms as numpy arrays"""
    from homan_amd import ops
    points, verts = (np.array(a, F32).reshape((-1,) + np.shape(a)[-2:]) for a in (points, verts))
    ctx = ops.SurfaceContactContext(points.shape[0], points.shape[1], verts.shape[1], faces, "cuda")
    w = None if weights is None else torch.from_numpy(np.asarray(weights, F32)).cuda()
    out = ops.surface_contact_terms(torch.from_numpy(points).cuda(), torch.from_numpy(verts).cuda(), ctx, weights=w, **kw)
    assert all(t.is_cuda and t.is_contiguous() for t in out.values())
    assert out["face"].dtype == torch.int32 and out["inside"].dtype == torch.int32 and out["value"].dtype == torch.float32
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_equal(got, want, what):
    for key in DETAIL:
        assert np.array_equal(bits(got[key]), bits(want[key])), (what, key, int((bits(got[key]) != bits(want[key])).sum()))
    for key, ref_key in SCALED:
        assert np.array_equal(bits(got[key]), bits(want[ref_key])), (what, key, got[key].ravel()[:4], want[ref_key].ravel()[:4])


def check(points, verts, faces, what, weights=None, searches=None, **kw):
    points, verts = (np.array(a, F32).reshape((-1,) + np.shape(a)[-2:]) for a in (points, verts))
    got = device(points, verts, faces, weights, **kw)
    want = cref.loss_and_gradients(points, verts, faces, weights, searches=searches, **kw)
    assert_equal(got, want, what)
    return got, want


# =============================================================================================== one frame
@pytest.mark.parametrize("name", ("hand->box", "box->hand"))
def test_meshes_equal_the_restatement(name):
    p, v, f = comparison_cases()[name]
    got, want = check(p, v, f, name, searches=[restated(name)])
    assert got["loss"][0] > 0 and got["loss"][1] > 0 and 20 < got["inside"].sum() < len(p) - 20
    assert np.abs(got["grad_verts_attr"]).max() > 0 and np.abs(got["grad_verts_rep"]).max() > 0
    again = device(p, v, f)                                                           # two calls, the same bits
    for key in DETAIL + tuple(k for k, _ in SCALED):
        assert np.array_equal(bits(again[key]), bits(got[key])), key


@pytest.mark.parametrize("F", (1, 2, 12))
def test_few_faces(F):
    """F = 1: every point scatters into the same three vertices"""
    p, v, f = cube_scene()
    got, want = check(p, v, f[:F], F)
    if F == 1:
        assert (got["face"] == 0).all() and np.abs(got["grad_verts_attr"][0, f[0]]).max() > 0


@pytest.mark.parametrize("N", (1, 63, 64, 65, 257))
def test_point_counts_about_the_wave_and_the_workgroup(N):
    p, v, f = comparison_cases()["hand->box"]
    s = restated("hand->box")
    check(p[:N], v, f, N, searches=[{k: a[:N] for k, a in s.items()}])


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_face_counts_about_the_staging_chunk(delta):
    """one face short of a chunk, a full chunk, and one face in a second chunk (the search's split-merge path)"""
    from homan_amd import lib, ops
    p, v, f = comparison_cases()["hand->box"]
    F = ops.SURFDIST_CHUNK + delta
    faces = np.ascontiguousarray(f[np.linspace(0, len(f) - 1, F).astype(int)])
    assert (lib.lib().hm_point_mesh_workspace_bytes(1, len(p), F) > 0) == (delta > 0)
    check(p, v, faces, F)


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_faces(name):
    p, v, f = comparison_cases()[name]
    got, want = check(p, v, f, name, searches=[restated(name)], contact_thresh=0.5, collision_thresh=0.5)
    assert np.isfinite(got["grad_points"]).all() and np.isfinite(got["grad_verts_attr"]).all() and got["loss"][0] > 0


def test_special_points_faces_and_weights():
    """a point exactly on a vertex (D == 0), a non-finite point, a face naming a vertex >= V, non-unit weights with zeros"""
    p, v, f = cube_scene()
    points = p.copy()
    points[5] = v[f[3, 1]]
    points[9, 1] = np.nan
    points[11, 0] = np.inf
    faces = np.concatenate([f[:4], [[0, 1, len(v)]], f[4:]]).astype(np.int32)
    rng = np.random.default_rng(2)
    weights = np.where(rng.random(len(p)) < 0.3, 0.0, rng.uniform(0.25, 3.0, len(p))).astype(F32)
    assert (weights == 0).sum() > 5
    got, want = check(points, v, faces, "special", weights=weights)
    assert got["d2"][0, 5] == 0 and got["value"][0, 5] == 0 and not got["grad_points"][0, 5].any() and got["bary"][0, 5].max() == 1
    assert (got["face"][0, [9, 11]] == -1).all() and not got["value"][0, [9, 11]].any() and not got["bary"][0, [9, 11]].any()
    assert 4 not in set(got["face"].ravel().tolist())
    outside_zero = (weights == 0) & (got["inside"][0] == 0)
    inside_zero = (weights == 0) & (got["inside"][0] == 1) & (got["d2"][0] > 0)
    assert outside_zero.any() and not got["value"][0, outside_zero].any() and not got["grad_points"][0, outside_zero].any()
    assert inside_zero.any() and (got["value"][0, inside_zero] > 0).all()              # the weights are the attraction's
    plain = device(points, v, faces)                                                  # (another grid: the per-point values only)
    ins = got["inside"][0] == 1
    assert np.array_equal(bits(plain["value"][0, ins]), bits(got["value"][0, ins]))
    assert not np.array_equal(bits(plain["value"][0, ~ins]), bits(got["value"][0, ~ins]))


# =============================================================================================== batches
def test_a_batch_of_three_poses_and_a_frame_alone():
    hands, boxes, bf, searches = three_poses()
    got, want = check(hands, boxes, bf, "B=3", searches=list(searches))
    assert len({int(got["inside"][b].sum()) for b in range(3)}) > 1
    for b in range(3):                      # the detail outputs carry no 1 / (B N): a frame of the batch equals its call alone
        alone = device(hands[b], boxes[b], bf)
        for key in DETAIL:
            assert np.array_equal(bits(alone[key][0]), bits(got[key][b])), (b, key)
    # the other direction, other sizes: the box's vertices against the three hands
    check(boxes, hands, mesh("hand")[1], "B=3 back")


def test_more_frames_than_one_launch_dimension():
    """70 000 frames of two points against the 12-triangle cube (seven kinds of frame, repeated): the frame axis is split over
    launches of 65 535, and the loss adds more per-frame counts than fit 2^53 quanta - the hi / lo words and their one rounding"""
    import math
    B, kinds, c = 70000, 7, 0.05
    _, v, f = cube_scene()
    rng = np.random.default_rng(3)
    pts = (rng.random((kinds, 2, 3)) * [0.06, 0.06, 0.08] + [-0.03, -0.02, -0.015]).astype(F32)
    shifts = np.stack([np.array([0.0047 * s, -0.0011 * s, 0.0006 * s], F32) for s in range(kinds)])
    kind = np.arange(B) % kinds
    got = device(pts[kind], (v[None] + shifts[kind][:, None]).astype(F32), f, contact_thresh=c, collision_thresh=c)
    L = cref.log2q(2, 1.0, c, c)
    q, bn = math.ldexp(1.0, L), float(B * 2)
    frames = [cref.terms(pts[s], (v + shifts[s]).astype(F32), f, None, c, c) for s in range(kinds)]
    sums = [cref.frame_sums(t, f, len(v), L) for t in frames]
    for b in (0, 1, B // 2, 65534, 65535, 65536, B - 1):
        t, (acc, _) = frames[b % kinds], sums[b % kinds]
        for key in DETAIL:
            assert np.array_equal(bits(got[key][b]), bits(t[key])), (b, key)
        assert np.array_equal(bits(got["grad_points"][b]), bits((t["g"].astype(np.float64) / bn).astype(F32))), b
        for side, key in enumerate(("grad_verts_attr", "grad_verts_rep")):
            assert np.array_equal(bits(got[key][b]), bits(((acc[side].astype(np.float64) * q) / bn).astype(F32))), (b, key)
    for key in DETAIL + ("grad_points", "grad_verts_attr", "grad_verts_rep"):         # identical frames, identical bits
        assert np.array_equal(bits(got[key]), bits(got[key][:kinds])[kind]), key
    count = np.bincount(kind)
    for side in (0, 1):
        hi = sum(int(count[s]) * (sums[s][1][side] >> 32) for s in range(kinds))
        lo = sum(int(count[s]) * (sums[s][1][side] & 0xffffffff) for s in range(kinds))
        assert hi * 2 ** 32 + lo > 2 ** 53
        assert got["loss"][side] == F32(((float(hi) * 4294967296.0 + float(lo)) * q) / bn), side
    assert got["loss"][1] > 0 and 0 < got["inside"].sum() < 2 * B


# =============================================================================================== autograd
def test_autograd_scales_the_saved_unit_gradients():
    from homan_amd import ops
    hands, boxes, bf, _ = three_poses()
    ctx = ops.SurfaceContactContext(3, 778, boxes.shape[1], bf, "cuda")
    unit = ops.surface_contact_terms(torch.from_numpy(hands).cuda(), torch.from_numpy(boxes).cuda(), ctx)
    a, b = 0.75, -2.5
    P = torch.from_numpy(hands).cuda().requires_grad_()
    X = torch.from_numpy(boxes).cuda().requires_grad_()
    A, R = ops.surface_contact_loss(P, X, ctx)
    assert A.dim() == 0 and R.dim() == 0 and torch.equal(torch.stack([A, R]).detach(), unit["loss"])
    gp, gx = torch.autograd.grad(a * A + b * R, (P, X))
    inside = unit["inside"].bool()[..., None]
    assert torch.equal(gp, torch.where(inside, F32(b) * unit["grad_points"], F32(a) * unit["grad_points"]))
    assert torch.equal(gx, F32(a) * unit["grad_verts_attr"] + F32(b) * unit["grad_verts_rep"])
    # an input that does not require a gradient gets None
    A, R = ops.surface_contact_loss(P.detach(), X, ctx)
    (A + R).backward()
    assert torch.equal(X.grad, unit["grad_verts_attr"] + unit["grad_verts_rep"])
    P2 = P.detach().clone().requires_grad_()
    A, R = ops.surface_contact_loss(P2, X.detach(), ctx)
    assert torch.autograd.grad(A, P2, allow_unused=True)[0] is not None
    A, R = ops.surface_contact_loss(P.detach(), X.detach(), ctx)
    assert not A.requires_grad and not R.requires_grad
    # a context holds the unit gradients of its LAST forward: the backward of an earlier one is refused, not answered wrongly
    first, _ = ops.surface_contact_loss(P2, X, ctx)
    ops.surface_contact_loss(P2, X, ctx)
    with pytest.raises(RuntimeError, match="another forward"):
        first.backward()


@pytest.mark.parametrize("name", MESH_CASES)
def test_against_float64(name):
    p, v, f = comparison_cases()[name]
    got = device(p, v, f)
    want = cref.reference64(p[None], v[None], f, got["face"], got["inside"], skip=got["d2"] == 0)
    value = max(util.deviation(got["value"], want["value"]), util.deviation(got["loss"], want["out"]))
    points = util.deviation(got["grad_points"], want["grad_points"])
    verts = util.deviation(np.stack([got["grad_verts_attr"], got["grad_verts_rep"]]),
                           np.stack([want["grad_verts_attr"], want["grad_verts_rep"]]))
    print(f"{name}: values {value:.3e}  point gradient {points:.3e}  vertex gradient {verts:.3e}")
    assert value <= util.E32_FACTOR * E32[name][0]
    assert points <= util.E32_FACTOR * E32[name][1]
    assert verts <= util.E32_FACTOR * E32[name][2]


# =============================================================================================== the model
SURF = dict(surface_contact_thresh=0.05, surface_collision_thresh=0.05)       # (the synthetic grasp is loose: keep tanh unsaturated)


def _weights(**kw):
    from homan_amd import synth
    return dict({k: 0.0 for k in synth.STEP1_LOSS_WEIGHTS}, **kw)


def test_model_term_equals_the_op_and_reaches_the_parameters(mano_model):
    from homan_amd import ops, synth
    clip = _clip(mano_model, 61)
    model = _model(mano_model, clip, **SURF)
    lw = _weights(lw_surf_attr=1.5, lw_surf_rep=0.5)
    ld, md = model(loss_weights=lw)
    assert set(ld) == {"loss_surf_attr", "loss_surf_rep"} and set(md) == {"surf_inside_share"}
    vh, vo = model.get_verts_hand()[0], model.get_verts_object()[0]
    ctx = ops.SurfaceContactContext(vo.shape[0], 778, vo.shape[1], model.faces_object[0], vo.device)
    vh_leaf, vo_leaf = vh.detach().clone().requires_grad_(), vo.detach().clone().requires_grad_()
    A, R = ops.surface_contact_loss(vh_leaf, vo_leaf, ctx, contact_thresh=0.05, collision_thresh=0.05)
    assert torch.equal(ld["loss_surf_attr"], A) and torch.equal(ld["loss_surf_rep"], R) and float(A.detach()) > 0
    assert md["surf_inside_share"] == float(ctx.inside.float().mean())
    # gradients reach hand translation, MANO pose and the object's rotation and translation, and equal the op's vertex gradients
    # pushed through the vertices
    (1.5 * ld["loss_surf_attr"] + 0.5 * ld["loss_surf_rep"]).backward()
    g_h, g_o = torch.autograd.grad(1.5 * A + 0.5 * R, (vh_leaf, vo_leaf))
    names = ("translations_hand", "mano_pca_pose", "rotations_object", "translations_object")
    params = [getattr(model, n) for n in names]
    pushed = torch.autograd.grad((vh, vo), params, grad_outputs=(g_h, g_o))
    for n, p, want in zip(names, params, pushed):
        assert float(p.grad.abs().max()) > 0, n
        assert torch.equal(p.grad, want), n
    # one weight alone returns that term alone
    assert set(model(loss_weights=_weights(lw_surf_rep=1.0))[0]) == {"loss_surf_rep"}
    # without the keys, and with loss_weights=None, the keys are today's
    step1 = dict(synth.STEP1_LOSS_WEIGHTS)
    ld1, md1 = model(loss_weights=step1)
    ld0, md0 = model(loss_weights=dict(step1, lw_surf_attr=0.0, lw_surf_rep=0.0))
    assert set(ld1) == set(ld0) and set(md1) == set(md0) and not any("surf" in k for k in list(ld1) + list(md1))
    full = _model(mano_model, clip, ordinal_depth=True, **SURF)
    ld_none, md_none = full(loss_weights=None)
    ld_all, md_all = full(loss_weights={k: 1.0 for k in step1})                        # every term of the reference on
    assert set(ld_none) == set(ld_all) and set(md_none) == set(md_all) and "loss_contact" in ld_none
    assert not any("surf" in k for k in list(ld_none) + list(md_none)) and full._surf_ctxs is None


def _deepest_interior_point(verts, faces):
    """a point well inside the closed mesh verts (V,3): the deepest of the midpoints of random vertex pairs"""
    from homan_amd import ops
    rng = np.random.default_rng(0)
    pairs = rng.integers(0, verts.shape[0], (256, 2))
    mids = 0.5 * (verts[pairs[:, 0]] + verts[pairs[:, 1]])
    r = ops.point_mesh_distance(mids[None], verts[None], faces)
    depth = torch.where(r["inside"][0] == 1, r["d2"][0], torch.zeros_like(r["d2"][0]))
    assert float(depth.max()) > 0
    return mids[int(depth.argmax())]


def test_two_hands_two_way_and_tips(mano_model):
    from homan_amd import synth
    sil_fn, hand_fn = synth.hip_clip_fns(mano_model)
    clip = synth.make_clip(seed=62, frames=3, rend_size=32, image_size=64, obj="cube", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn, hands=("right", "left"))
    lw = _weights(lw_surf_attr=1.0, lw_surf_rep=1.0)
    one_way = _model(mano_model, clip, **SURF)
    two_way = _model(mano_model, clip, surface_two_way=True, **SURF)
    tips = _model(mano_model, clip, surface_contact_zones="tips", **SURF)
    assert one_way.hand_nb == 2
    # interpenetrating scene: hand 0 of every frame moved so that an interior point of it sits on an object vertex
    with torch.no_grad():
        vh, vo = one_way.get_verts_hand()[0], one_way.get_verts_object()[0]
        closed = torch.as_tensor(np.asarray(one_way.mano_model.closed_faces).astype(np.int32))
        for b in range(vo.shape[0]):
            shift = vo[b, 0] - _deepest_interior_point(vh[2 * b], closed)
            for m in (one_way, two_way, tips):
                m.translations_hand[2 * b] += shift
    ld1, md1 = one_way(loss_weights=lw)
    ld2, _ = two_way(loss_weights=lw)
    ldt, _ = tips(loss_weights=lw)
    assert ld1["loss_surf_attr"].dim() == 0 and float(ld1["loss_surf_attr"]) > 0 and float(ld1["loss_surf_rep"]) > 0
    assert 0 < md1["surf_inside_share"] < 1
    assert torch.equal(ld2["loss_surf_attr"], ld1["loss_surf_attr"])
    assert float(ld2["loss_surf_rep"]) > float(ld1["loss_surf_rep"])                  # the object -> hand share
    assert torch.equal(ldt["loss_surf_rep"], ld1["loss_surf_rep"])
    assert 0 < float(ldt["loss_surf_attr"]) < float(ld1["loss_surf_attr"])
    # tips: the attraction's gradient to the hand vertices is zero off the five tip vertices
    for ctx in tips._surf_ctxs["hand"]:
        off = torch.ones(778, dtype=torch.bool, device="cuda")
        off[list(cref.TIPS)] = False
        outside = ctx.inside == 0
        assert not bool(ctx.grad_points[outside & off[None]].any())
        assert bool(ctx.grad_points[outside & ~off[None]].any()) or not bool((outside & ~off[None]).any())
    ldt["loss_surf_attr"].backward()
    assert float(tips.translations_hand.grad.abs().max()) > 0


# =============================================================================================== the loops
def test_loops_take_the_term(mano_model):
    from homan_amd import synth
    from homan_amd.jointopt import FusedStepper, ShardStepper
    lw = dict(synth.STEP1_LOSS_WEIGHTS, lw_surf_attr=1.0, lw_surf_rep=5.0)
    clip = _clip(mano_model, 63)
    model = _model(mano_model, clip, sync=False, **SURF)
    with pytest.raises(NotImplementedError, match="mode='graph'"):
        FusedStepper(model, lw, 1e-2, 6)
    with pytest.raises(NotImplementedError):
        ShardStepper([model], lw, 1e-2, 6)
    _, auto = _fit(mano_model, clip, lw, 6, "auto", **SURF)
    _, eager = _fit(mano_model, clip, lw, 6, "eager", **SURF)
    _, graph = _fit(mano_model, clip, lw, 6, "graph", **SURF)
    _, plain = _fit(mano_model, clip, dict(synth.STEP1_LOSS_WEIGHTS), 6, "auto")
    assert len(auto["loss"]) == 6 and set(auto) == set(eager) == set(plain) | {"loss_surf_attr", "loss_surf_rep", "surf_inside_share"}
    _close_as_the_two_loops(auto["loss"], eager["loss"])
    _close_as_the_two_loops(auto["loss_surf_attr"], eager["loss_surf_attr"])
    for k in auto:                                                                     # two graph fits: identical bits
        np.testing.assert_array_equal(np.asarray(auto[k]), np.asarray(graph[k]), err_msg=k)
    assert auto["loss_surf_attr"][0] > 0 and auto["loss"][0] > plain["loss"][0]


def test_clip_fitter_walk_equals_solo_fits(mano_model):
    from homan_amd import synth
    from homan_amd.jointopt import ClipFitter
    lw = dict(synth.STEP1_LOSS_WEIGHTS, lw_surf_attr=1.0, lw_surf_rep=5.0)
    clips = [_clip(mano_model, s) for s in (64, 65)]
    fitter = ClipFitter(lw, num_iterations=6, optimize_mano=True, image_size=64, mano_model=mano_model, rend_size=32, **SURF)
    results = fitter.fit(clips)
    assert fitter.timing["built"] == 1 and fitter.timing["reused"] == 1 and len(fitter.resident_graph) == 1
    for clip, res in zip(clips, results):
        model, evo = _fit(mano_model, clip, lw, 6, "auto", **SURF)
        for k, v in res["state_dict"].items():
            assert torch.equal(v, getattr(model, k).detach().cpu()), k
        assert torch.equal(res["verts_object"], model.get_verts_object()[0].detach().cpu())
        assert "loss_surf_rep" in evo
        for k in evo:
            np.testing.assert_array_equal(np.asarray(res["loss_evolution"][k]), np.asarray(evo[k]), err_msg=k)


# =============================================================================================== the effect
def _descend(points, verts, faces, term, steps=30, lr=1e-3, **kw):
    """Adam on one translation per frame of `points` against the fixed mesh, on A (term 0) or R (term 1) alone -> (loss values,
    the moved points)"""
    from homan_amd import ops
    P, X = torch.from_numpy(points).cuda(), torch.from_numpy(verts).cuda()
    ctx = ops.SurfaceContactContext(P.shape[0], P.shape[1], X.shape[1], faces, "cuda")
    t = torch.zeros(P.shape[0], 1, 3, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([t], lr=lr)
    values = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = ops.surface_contact_loss(P + t, X, ctx, **kw)[term]
        values.append(float(loss))
        loss.backward()
        if len(values) <= steps:
            opt.step()
    return values, (P + t).detach()


def test_the_terms_do_what_they_are_for():
    from homan_amd import pointmetrics
    hands, boxes, bf, _ = three_poses()
    hands, boxes = hands[:2], boxes[:2]
    closed = mesh("hand")[1][None]
    metrics = lambda p: pointmetrics.get_surface_metrics(p, torch.from_numpy(boxes).cuda(), closed, bf[None])  # noqa: E731
    before = metrics(torch.from_numpy(hands).cuda())
    values, moved = _descend(hands, boxes, bf, term=1)
    after = metrics(moved)
    print("repulsion:", values[0], "->", values[-1], "pen_depth", before["pen_depth"], "->", after["pen_depth"])
    assert values[-1] < values[0] and all(a < b for a, b in zip(after["pen_depth"], before["pen_depth"]))
    # attraction alone, the hand moved off the box
    away = (hands + np.array([0.15, 0.0, 0.0], F32)).astype(F32)
    before = metrics(torch.from_numpy(away).cuda())
    assert min(before["min_dist"]) > 0.01 and max(before["pen_depth"]) == 0
    values, moved = _descend(away, boxes, bf, term=0, contact_thresh=0.1)
    after = metrics(moved)
    print("attraction:", values[0], "->", values[-1], "min_dist", before["min_dist"], "->", after["min_dist"])
    assert values[-1] < values[0] and all(a < b for a, b in zip(after["min_dist"], before["min_dist"]))
