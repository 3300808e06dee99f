"""The kernel of csrc/winding.hip (hm_point_mesh_winding), `ops.point_mesh_winding`, `ops.point_mesh_distance_signed`,
`pointmetrics.get_surface_metrics_signed` and `ho3deval.evaluate_sequence_surface_signed` against the NumPy restatement of
tests/winding_ref.py.

Bars.  count and inside: equal, bit for bit - both sides perform the same IEEE double operations in the same order, round every
angle to the same grid and add integers, whose sum depends neither on the order of the faces nor on how they are dealt to
workgroups.  winding: equal (count * 2^L / (4 pi), two correctly rounded operations on both sides).  The metrics: equal, as in
tests/test_surfmetrics_gpu.py.  What the flags mean on open meshes is the CPU file's subject (tests/test_winding.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import surfmetrics_ref as sref
from tests import winding_ref as wref
from tests.test_surfmetrics import DEGENERATE, comparison_cases, mesh, restated
from tests.test_surfmetrics_gpu import bits, cube_scene, three_poses
from tests.test_winding import SCENES, open_faces, winding

pytestmark = pytest.mark.gpu

F32 = np.float32
KEYS = ("count", "inside", "winding")


def device(points, verts, faces, log2q=None):
    """points (B,N,3) or (N,3), verts likewise -> the op's outputs as numpy arrays (B, ...)"""
    from homan_amd import ops
    points, verts = (np.array(a, F32).reshape((-1,) + a.shape[-2:]) for a in (points, verts))      # (writable copies)
    out = ops.point_mesh_winding(torch.from_numpy(points).cuda(), torch.from_numpy(verts).cuda(), faces, log2q)
    assert list(out) == ["count", "winding", "inside", "log2q"] and isinstance(out["log2q"], int)
    assert out["count"].dtype == torch.int64 and out["inside"].dtype == torch.int32 and out["winding"].dtype == torch.float64
    assert all(out[k].is_cuda and out[k].is_contiguous() and out[k].shape == points.shape[:2] for k in KEYS)
    return {k: (v.cpu().numpy() if k in KEYS else v) for k, v in out.items()}


def assert_frame(got, b, want, what):
    assert got["log2q"] == want["log2q"], what
    for key in KEYS:
        assert np.array_equal(bits(got[key][b]), bits(want[key])), (what, key, int((bits(got[key][b]) != bits(want[key])).sum()))


def check(points, verts, faces, what, log2q=None):
    got = device(points, verts, faces, log2q)
    want = wref.point_mesh_winding(points, verts, faces, log2q)
    assert_frame(got, 0, want, what)
    return got, want


# =============================================================================================== one frame
@pytest.mark.parametrize("F", (1, 2, 12))
def test_few_faces_and_points_on_the_surface(F):
    """the cube scene, and points exactly on a vertex, in a face's plane beside the face, on a face and on an edge: whatever the
    rules give, the same bits"""
    p, v, f = cube_scene()
    lo, hi = v.min(0), v.max(0)
    special = np.array([v[0], v[7], v[f[0, 1]],                                           # at vertices
                        [lo[0], hi[1] + 0.01, 0.07], [0.05, 0.0, lo[2]], [-0.03, lo[1], 0.02],   # in a face's plane, outside it
                        [lo[0], 0.0078125, 0.015625], [0.0, hi[1], 0.03125], [0.0, 0.0, hi[2]],  # on a face
                        [lo[0], lo[1], 0.025], [0.0, hi[1], hi[2]]], F32)                        # on an edge
    points = np.concatenate([p, special]).astype(F32)
    got, want = check(points, v, f[:F], F)
    if F == 12:
        assert 3 < want["inside"][:len(p)].sum() < 40
        assert np.array_equal(want["inside"][:len(p)], sref.point_mesh(p, v, f)["inside"])
    assert (wref.solid_angles(points[len(p):, None], v[f[None, :F, 0]], v[f[None, :F, 1]], v[f[None, :F, 2]]) == 0).any()


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_face_counts_about_the_staging_chunk(delta):
    """a sub-sample of the box's faces: one face short of a chunk, a full chunk, and one face in a second chunk (which, for a
    lone frame, a second workgroup takes: the counts cleared by the call and merged by the 64-bit atomicAdd)"""
    from homan_amd import lib, ops
    p, v, f = comparison_cases()["hand->box"]
    F = ops.SURFDIST_CHUNK + delta
    faces = np.ascontiguousarray(f[np.linspace(0, len(f) - 1, F).astype(int)])
    assert (lib.lib().hm_point_mesh_workspace_bytes(1, len(p), F) > 0) == (delta > 0)      # the search's split is this kernel's
    got, want = check(p, v, faces, F)
    assert np.abs(want["winding"]).max() > 0.05 and len(p) == 778
    check(p, v, np.ascontiguousarray(faces[::-1]), -F)
    assert np.array_equal(device(p, v, np.ascontiguousarray(faces[::-1]))["count"], got["count"])   # any order of the faces


@pytest.mark.parametrize("N", (1, 63, 64, 65, 257))
def test_point_counts_about_the_wave_and_the_workgroup(N):
    p, v, f = comparison_cases()["hand->box"]
    want = winding("hand->box")
    got = device(p[:N], v, f)
    assert_frame(got, 0, {k: (want[k][:N] if k in KEYS else want[k]) for k in want}, N)


def test_a_batch_of_three_poses_and_a_frame_alone():
    hands, boxes, bf, _ = three_poses()
    got = device(hands, boxes, bf)
    for b in range(3):
        assert_frame(got, b, wref.point_mesh_winding(hands[b], boxes[b], bf), b)
    assert len({int(got["inside"][b].sum()) for b in range(3)}) > 1
    for b in range(3):                                                                # each frame of B = 3 equals its B = 1 call
        alone = device(hands[b], boxes[b], bf)
        for key in KEYS:
            assert np.array_equal(bits(alone[key][0]), bits(got[key][b])), (key, b)
    again = device(hands, boxes, bf)                                                  # two calls, the same bits
    for key in KEYS:
        assert np.array_equal(bits(again[key]), bits(got[key])), key


def test_a_batch_large_enough_that_no_frame_is_split():
    """1100 frames of 65 points against 257 faces: two staging chunks walked by ONE workgroup per frame, which stores its counts
    and flags itself, against the same frames in a batch of three, whose faces are split"""
    from homan_amd import lib, ops
    B = 1100
    hands, boxes, bf, _ = three_poses()
    F = ops.SURFDIST_CHUNK + 1
    faces = np.ascontiguousarray(bf[np.linspace(0, len(bf) - 1, F).astype(int)])
    assert lib.lib().hm_point_mesh_workspace_bytes(B, 65, F) == 0 and lib.lib().hm_point_mesh_workspace_bytes(3, 65, F) > 0
    kind = np.arange(B) % 3
    got = device(hands[kind][:, 100:165], boxes[kind], faces)
    small = device(hands[:, 100:165], boxes, faces)
    for b in range(3):
        assert_frame(small, b, wref.point_mesh_winding(hands[b, 100:165], boxes[b], faces), b)
    for key in KEYS:
        assert np.array_equal(bits(got[key]), bits(small[key])[kind]), key


def test_more_frames_than_one_launch_dimension():
    """70 000 frames of two points against the 12-triangle cube: the frame axis is split over launches of 65 535"""
    B, kinds = 70000, 7
    _, v, f = cube_scene()
    rng = np.random.default_rng(3)
    pts = (rng.random((kinds, 2, 3)) * [0.06, 0.06, 0.08] + [-0.03, -0.02, -0.015]).astype(F32)
    shifts = np.stack([np.array([0.0047 * s, -0.0011 * s, 0.0006 * s], F32) for s in range(kinds)])
    kind = np.arange(B) % kinds
    got = device(pts[kind], (v[None] + shifts[kind][:, None]).astype(F32), f)
    want = [wref.point_mesh_winding(pts[s], (v + shifts[s]).astype(F32), f) for s in range(kinds)]
    for b in (0, 1, B // 2, 65534, 65535, 65536, B - 1):
        assert_frame(got, b, want[b % kinds], b)
    for key in KEYS:                                                                  # identical frames, identical bits
        assert np.array_equal(bits(got[key]), bits(got[key][:kinds])[kind]), key
    assert 0 < got["inside"].sum() < 2 * B


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_faces(name):
    p, v, f = comparison_cases()[name]
    got, want = check(p, v, f, name)
    assert not got["count"].any() and not got["inside"].any()


def test_skipped_faces_and_non_finite_points():
    """the cube with degenerate faces, faces that name a vertex outside [0, V), a NaN vertex, and NaN / inf points among them"""
    p, v, f = cube_scene()
    verts = np.concatenate([v, [[np.nan, 0.01, 0.01], [0.01, np.inf, 0.01], [0.03125, 0.0, 0.0625], [0.03125, 0.0, 0.0625],
                                [0.0625, 0.03125, 0.09375], [0.046875, 0.015625, 0.078125]]]).astype(F32)
    extra = [[0, 1, 99], [-1, 2, 3], [8, 0, 1], [0, 9, 2], [10, 11, 12], [10, 10, 10], [10, 12, 13], [2, 3, 14]]
    faces = np.concatenate([extra[:4], f[:6], extra[4:], f[6:]]).astype(np.int32)
    points = p.copy()
    points[3, 0], points[17, 1], points[40, 2] = np.nan, np.inf, -np.inf
    got, want = check(points, verts, faces, "mixed")
    assert not want["count"][[3, 17, 40]].any() and not want["inside"][[3, 17, 40]].any()
    plain = wref.point_mesh_winding(points, v, f)
    assert np.array_equal(want["count"], plain["count"])                              # none of the extra faces counts
    none = device(points, verts, np.asarray(extra[:4], np.int32))                     # every face skipped
    assert not none["count"].any() and not none["inside"].any()


def test_a_coarser_and_the_finest_grid():
    p, v, f = comparison_cases()["hand->box"]
    for L in (-47, -30, 0):
        got, want = check(p[:130], v, f, L, log2q=L)
        assert got["log2q"] == L
    assert np.array_equal(wref.point_mesh_winding(p[:130], v, f, -47)["inside"], winding("hand->box")["inside"][:130])
    from homan_amd import ops
    with pytest.raises(ValueError):
        ops.point_mesh_winding(torch.from_numpy(np.array(p[None])).cuda(), torch.from_numpy(np.array(v[None])).cuda(), f, log2q=-48)
    with pytest.raises(ValueError):
        ops.point_mesh_winding(torch.from_numpy(np.array(p[None])).cuda(), torch.from_numpy(np.array(v[None])).cuda(), f, log2q=1)


# =============================================================================================== scenes
@pytest.mark.parametrize("name", SCENES)
def test_open_scenes_equal_the_restatement(name):
    p, v, f = comparison_cases()[name]
    got = device(p, v, open_faces(f))
    assert_frame(got, 0, winding(name, True), name)


def test_a_full_closed_scene():
    p, v, f = comparison_cases()["hand->bottle"]
    assert (len(p), len(f)) == (778, 3000)
    got = device(p, v, f)
    assert_frame(got, 0, winding("hand->bottle"), "hand->bottle")
    assert np.array_equal(got["inside"][0], restated("hand->bottle")["inside"])


def test_null_flags_a_dirty_count_and_refusals():
    """through the raw C ABI: `inside` is optional, the count buffer may hold anything (the call clears it itself), and a refused
    call touches nothing"""
    from homan_amd import lib
    h = lib.lib()
    p, v, f = comparison_cases()["hand->box"]
    want = winding("hand->box")
    N, V, F = len(p), len(v), len(f)
    points, verts, faces = (torch.from_numpy(np.array(a)).cuda() for a in (p[None], v[None], f))
    for frames in (1, 256):                                                           # a lone frame's faces are split, those of 256 are not
        pts, vs = points.expand(frames, N, 3).contiguous(), verts.expand(frames, V, 3).contiguous()
        count = torch.full((frames, N), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
        inside = torch.full((frames, N), -7, dtype=torch.int32, device="cuda")
        assert h.hm_point_mesh_winding(lib.ptr(pts), lib.ptr(vs), lib.ptr(faces), frames, N, V, F, -44, lib.ptr(count), None,
                                       lib.stream()) == 0
        torch.cuda.synchronize()
        assert (inside == -7).all() and np.array_equal(count.cpu().numpy(), np.stack([want["count"]] * frames))
        for kw in (dict(F=0), dict(log2q=-48), dict(count=count.data_ptr() + 4)):
            args = dict(F=F, log2q=-44, count=lib.ptr(count))
            args.update(kw)
            count.fill_(3)
            assert h.hm_point_mesh_winding(lib.ptr(pts), lib.ptr(vs), lib.ptr(faces), frames, N, V, args["F"], args["log2q"],
                                           args["count"], lib.ptr(inside), lib.stream()) == -1, kw
            torch.cuda.synchronize()
            assert (count == 3).all() and (inside == -7).all()


# =============================================================================================== the signed distance op
def test_point_mesh_distance_signed():
    from homan_amd import ops
    p, v, f = comparison_cases()["hand->box"]
    fo = open_faces(f)
    P, X = torch.from_numpy(np.array(p[None])).cuda(), torch.from_numpy(np.array(v[None])).cuda()
    plain = ops.point_mesh_distance(P, X, fo, closest=True)
    assert list(plain) == ["d2", "face", "inside", "closest"]                          # the default call's keys are unchanged
    parity = ops.point_mesh_distance_signed(P, X, fo, closest=True)
    assert list(parity) == list(plain) and all(torch.equal(parity[k], plain[k]) for k in plain)
    assert list(ops.point_mesh_distance_signed(P, X, fo)) == ["d2", "face", "inside"]
    w = ops.point_mesh_winding(P, X, fo)
    for sign in ("winding", "auto"):                                                  # (the opened box is not closed)
        got = ops.point_mesh_distance_signed(P, X, fo, closest=True, sign=sign)
        assert list(got) == ["d2", "face", "inside", "closest", "winding"]
        for key in ("d2", "face", "closest"):
            assert np.array_equal(bits(got[key].cpu().numpy()), bits(plain[key].cpu().numpy())), key
        assert torch.equal(got["inside"], w["inside"]) and torch.equal(got["winding"], w["winding"])
        assert got["inside"].dtype == torch.int32
    assert np.array_equal(w["inside"].cpu().numpy()[0], winding("hand->box", True)["inside"])
    assert (w["inside"] != plain["inside"]).sum() >= 10                               # parity is wrong on the opened box
    auto_closed = ops.point_mesh_distance_signed(P, X, f, sign="auto")
    assert list(auto_closed) == ["d2", "face", "inside"]                              # closed: parity


# =============================================================================================== the metrics
METRIC_KEYS = ["pen_depth", "pen_depth_obj", "min_dist", "contact_share", "has_contact"]


def test_signed_metrics_equal_parity_on_a_closed_scene():
    from homan_amd import pointmetrics
    from tests.test_surfmetrics_gpu import scene
    person, obj, hf, bf = scene(2)
    args = (torch.from_numpy(person), torch.from_numpy(obj), np.stack([hf] * 2), bf[None])
    want = pointmetrics.get_surface_metrics(*args, per_vertex=True)
    assert max(want["pen_depth"]) > 0.001 and max(want["pen_depth_obj"]) > 0.001
    for sign in ("parity", "winding", "auto"):
        got = pointmetrics.get_surface_metrics_signed(*args, per_vertex=True, sign=sign)
        assert list(got) == METRIC_KEYS + ["signed_dist"] and {k: got[k] for k in METRIC_KEYS} == {k: want[k] for k in METRIC_KEYS}
        assert np.array_equal(bits(got["signed_dist"]), bits(want["signed_dist"])), sign
    # any chunking gives the same values
    frame_bytes = pointmetrics.surface_frame_bytes(2, 778, obj.shape[1], "winding")
    again = pointmetrics.get_surface_metrics_signed(*args, per_vertex=True, max_bytes=frame_bytes + 5, sign="winding")
    assert np.array_equal(bits(again["signed_dist"]), bits(want["signed_dist"]))
    with pytest.raises(ValueError):
        pointmetrics.get_surface_metrics_signed(*args, max_bytes=frame_bytes - 1, sign="winding")


@functools.lru_cache(maxsize=None)
def open_bottle_restated():
    p, v, f = comparison_cases()["hand->bottle"]
    return wref.surface_metrics([p], [mesh("hand")[1]], v, open_faces(f))


def test_signed_metrics_on_the_open_bottle_equal_the_restated_metrics():
    from homan_amd import pointmetrics
    p, v, f = comparison_cases()["hand->bottle"]
    fo, hf = open_faces(f), mesh("hand")[1]
    want = open_bottle_restated()
    args = (torch.from_numpy(np.array(p[None])), torch.from_numpy(np.array(v[None])), hf[None], fo[None])
    for sign in ("winding", "auto"):              # auto: the winding number for the bottle, parity for the closed hand - the same flags
        got = pointmetrics.get_surface_metrics_signed(*args, per_vertex=True, sign=sign)
        assert {k: got[k][0] for k in METRIC_KEYS} == {k: want[k] for k in METRIC_KEYS}, sign
        assert np.array_equal(bits(got["signed_dist"]), bits(want["signed_dist"])), sign
    parity = pointmetrics.get_surface_metrics(*args, per_vertex=True)
    assert ((parity["signed_dist"] < 0) != (want["signed_dist"] < 0)).sum() >= 10      # what the mode is for
    assert want["pen_depth"] > 0.001


def test_evaluate_sequence_surface_signed_passes_the_sign_through():
    from homan_amd import ho3deval, pointmetrics, synth
    hv, hf = mesh("hand")
    hand = (hv + np.array([0.0, 0.0, 0.5], F32)).astype(F32)
    box, faces = synth.box_mesh(2, 2, 2, scale=0.08)
    box = np.asarray(box, F32) - np.asarray(box, F32).mean(0)
    faces = open_faces(np.asarray(faces))
    joints = np.zeros((21, 3), F32) + hand.mean(0)
    seq = {f: {"hand_verts3d": (hand + F32(0.002 * f)).astype(F32), "hand_joints3d": joints,
               "obj_verts3d": (box + hand.mean(0) + F32(0.012 * f)).astype(F32), "img_path": "seq/rgb/0000.png"}
           for f in (0, 2, 6)}
    pred_hand = ho3deval.interpolate_sequence(seq, 7, "hand_verts3d", ho3deval.CAMEXTR_SIGNS)
    pred_obj = ho3deval.interpolate_sequence(seq, 7, "obj_verts3d", ho3deval.CAMEXTR_SIGNS)
    results = {}
    for sign in ("parity", "winding", "auto"):
        res = ho3deval.evaluate_sequence_surface_signed(seq, 7, faces, hf, chunk=3, sign=sign)
        direct = pointmetrics.get_surface_metrics_signed(pred_hand, pred_obj, hf[None], faces[None], sign=sign)
        assert list(res) == METRIC_KEYS + [k + "_mean" for k in METRIC_KEYS]
        for key in METRIC_KEYS:
            assert np.array_equal(res[key], np.asarray(direct[key], np.float64)), (sign, key)
        results[sign] = res
    default = ho3deval.evaluate_sequence_surface(seq, 7, faces, hf, chunk=3)
    assert all(np.array_equal(default[k], results["parity"][k]) for k in default)
    assert all(np.array_equal(results["auto"][k], results["winding"][k]) for k in default)
    assert any(not np.array_equal(results["parity"][k], results["winding"][k]) for k in METRIC_KEYS)
