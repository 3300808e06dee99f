"""The kernel of csrc/surfdist.hip (hm_point_mesh_distance), `pointmetrics.get_surface_metrics` and
`ho3deval.evaluate_sequence_surface` against the NumPy restatement of tests/surfmetrics_ref.py.

Bars.  d2, face, inside and closest: equal, bit for bit - both sides perform the same fp32 operations in the same order, and
the minimum and the parity do not depend on the order of the faces.  The metrics: equal - maxima, minima and counts of those
values, then sqrt((double)d2), which is correctly rounded on both sides (the device part ends at the fp32 squares).  How far
fp32 lies from float64 is the CPU file's subject (tests/test_surfmetrics.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import surfmetrics_ref as ref
from tests import volmetrics_ref as vref
from tests.test_surfmetrics import DEGENERATE, comparison_cases, mesh, posed_hand, restated

pytestmark = pytest.mark.gpu

F32 = np.float32
KEYS = ("d2", "face", "inside", "closest")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def device(points, verts, faces, closest=True):
    """points (B,N,3) or (N,3), verts likewise -> the op's outputs as numpy arrays (B, ...)"""
    from homan_amd import ops
    points, verts = (np.array(a, F32).reshape((-1,) + a.shape[-2:]) for a in (points, verts))      # (writable copies)
    out = ops.point_mesh_distance(torch.from_numpy(points).cuda(), torch.from_numpy(verts).cuda(), faces, closest=closest)
    assert out["d2"].dtype == torch.float32 and out["face"].dtype == torch.int32 and out["inside"].dtype == torch.int32
    assert all(t.is_cuda and t.is_contiguous() for t in out.values()) and ("closest" in out) == closest
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_frame(got, b, want, what):
    for key in KEYS:
        assert np.array_equal(bits(got[key][b]), bits(want[key])), (what, key, int((bits(got[key][b]) != bits(want[key])).sum()))


def check(points, verts, faces, what):
    got = device(points, verts, faces)
    want = ref.point_mesh(points, verts, faces)
    assert_frame(got, 0, want, what)
    return got, want


# =============================================================================================== one frame
@pytest.mark.parametrize("name", ("hand->box", "box->hand", "hand->bottle"))
def test_meshes_equal_the_restatement(name):
    p, v, f = comparison_cases()[name]
    assert len(f) == {"hand->box": 500, "box->hand": 1552, "hand->bottle": 3000}[name]
    want = restated(name)
    got = device(p, v, f)
    assert_frame(got, 0, want, name)
    assert 20 < got["inside"].sum() < len(p) - 20 and got["d2"].min() >= 0 and (got["face"] >= 0).all()
    again = device(p, v, f)                                                           # two calls, the same bits
    for key in KEYS:
        assert np.array_equal(bits(again[key]), bits(got[key])), key
    assert all(np.array_equal(bits(device(p, v, f, closest=False)[key]), bits(got[key])) for key in KEYS[:3])


@functools.lru_cache(maxsize=None)
def cube_scene():
    v, f = vref.cube_mesh([-0.02, -0.01, 0.0], [0.02, 0.03, 0.05])
    rng = np.random.default_rng(11)
    p = (rng.random((65, 3)) * [0.08, 0.08, 0.1] + [-0.04, -0.03, -0.025]).astype(F32)
    return p, v, f


@pytest.mark.parametrize("F", (1, 2, 12))
def test_few_faces(F):
    p, v, f = cube_scene()
    got, want = check(p, v, f[:F], F)
    if F == 12:
        assert 3 < want["inside"].sum() < 40


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_face_counts_about_the_staging_chunk(delta):
    """a sub-sample of the box's faces: one face short of a chunk, a full chunk, and one face in a second chunk (which, for a
    lone frame, a second workgroup takes: the merge through the integer atomics)"""
    from homan_amd import lib, ops
    p, v, f = comparison_cases()["hand->box"]
    F = ops.SURFDIST_CHUNK + delta
    faces = np.ascontiguousarray(f[np.linspace(0, len(f) - 1, F).astype(int)])
    assert (lib.lib().hm_point_mesh_workspace_bytes(1, len(p), F) > 0) == (delta > 0)
    check(p, v, faces, F)
    # the winning face may be the last one
    check(p, v, np.ascontiguousarray(faces[::-1]), -F)


@pytest.mark.parametrize("N", (1, 63, 64, 65, 257))
def test_point_counts_about_the_wave_and_the_workgroup(N):
    p, v, f = comparison_cases()["hand->box"]
    want = restated("hand->box")
    got = device(p[:N], v, f)
    assert_frame(got, 0, {k: want[k][:N] for k in KEYS}, N)


@functools.lru_cache(maxsize=None)
def three_poses():
    """the hand in three poses on the box, the box moved with it: (points (3,778,3), verts (3,Vb,3), faces, restated frames)"""
    bv, bf = mesh("box")
    hands = np.stack([posed_hand("box", angle=0.3 + 0.5 * b, shift=(0.004 - 0.003 * b, 0.006, 0.002 * b)) for b in range(3)])
    boxes = np.stack([(bv + F32(0.0021 * b)).astype(F32) for b in range(3)])
    want = tuple(ref.point_mesh(hands[b], boxes[b], bf) for b in range(3))
    return hands, boxes, bf, want


def test_a_batch_of_three_poses_and_a_frame_alone():
    hands, boxes, bf, want = three_poses()
    got = device(hands, boxes, bf)
    for b in range(3):
        assert_frame(got, b, want[b], b)
    assert len({want[b]["inside"].sum() for b in range(3)}) > 1
    alone = device(hands[1], boxes[1], bf)                                            # frame 1 of B = 3 equals its B = 1 call
    for key in KEYS:
        assert np.array_equal(bits(alone[key][0]), bits(got[key][1])), key
    # the other direction, other sizes: the box's vertices against the three hands
    back = device(boxes, hands, mesh("hand")[1])
    for b in (0, 2):
        assert_frame(back, b, ref.point_mesh(boxes[b], hands[b], mesh("hand")[1]), -b)


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_faces(name):
    p, v, f = comparison_cases()[name]
    got = device(p, v, f)
    assert_frame(got, 0, restated(name), name)
    assert np.isfinite(got["d2"]).all() and np.isfinite(got["closest"]).all()


def test_degenerate_and_skipped_faces_in_a_mesh():
    """the cube with degenerate faces, faces that name a vertex outside [0, V), a NaN vertex, and NaN / inf points among them"""
    p, v, f = cube_scene()
    verts = np.concatenate([v, [[np.nan, 0.01, 0.01], [0.01, np.inf, 0.01], [0.03125, 0.0, 0.0625], [0.03125, 0.0, 0.0625],
                                [0.0625, 0.03125, 0.09375], [0.046875, 0.015625, 0.078125]]]).astype(F32)
    extra = [[0, 1, 99], [-1, 2, 3], [8, 0, 1], [0, 9, 2], [10, 11, 12], [10, 10, 10], [10, 12, 13], [2, 3, 14]]        # (14: one past the last vertex)
    faces = np.concatenate([extra[:4], f[:6], extra[4:], f[6:]]).astype(np.int32)
    points = p.copy()
    points[3, 0], points[17, 1], points[40, 2] = np.nan, np.inf, -np.inf
    got, want = check(points, verts, faces, "mixed")
    assert (want["face"][[3, 17, 40]] == -1).all() and np.isinf(want["d2"][[3, 17, 40]]).all() and not want["closest"][[3, 17, 40]].any()
    assert set(want["face"].tolist()) & {10, 11, 12} and not set(want["face"].tolist()) & {0, 1, 2, 3}
    plain = ref.point_mesh(points, v, f)
    assert np.array_equal(want["inside"], plain["inside"])                            # degenerate faces cross no ray
    # every face skipped: nothing found, whatever the point
    none = device(points, verts, np.asarray(extra[:4], np.int32))
    assert np.isinf(none["d2"]).all() and (none["face"] == -1).all() and not none["inside"].any() and not none["closest"].any()


def test_a_scene_a_kilometre_from_the_origin():
    p, v, f = comparison_cases()["hand->box"]
    off = np.array([1000.0, -700.0, 300.0], F32)
    got, want = check((p + off).astype(F32), (v + off).astype(F32), f, "far")
    assert 5 < want["inside"].sum() < len(p) - 5


# =============================================================================================== batches
def test_more_frames_than_one_launch_dimension():
    """70 000 frames of two points against the 12-triangle cube: the frame axis is split over launches of 65 535"""
    B, kinds = 70000, 7
    _, v, f = cube_scene()
    rng = np.random.default_rng(3)
    pts = (rng.random((kinds, 2, 3)) * [0.06, 0.06, 0.08] + [-0.03, -0.02, -0.015]).astype(F32)
    shifts = np.stack([np.array([0.0047 * s, -0.0011 * s, 0.0006 * s], F32) for s in range(kinds)])
    kind = np.arange(B) % kinds
    points, verts = pts[kind], (v[None] + shifts[kind][:, None]).astype(F32)
    got = device(points, verts, f)
    want = [ref.point_mesh(pts[s], (v + shifts[s]).astype(F32), f) for s in range(kinds)]
    for b in (0, 1, B // 2, 65534, 65535, 65536, B - 1):
        assert_frame(got, b, want[b % kinds], b)
    for key in KEYS:                                                                  # identical frames, identical bits
        assert np.array_equal(bits(got[key]), bits(got[key][:kinds])[kind]), key
    assert 0 < got["inside"].sum() < 2 * B


def test_a_batch_large_enough_that_no_frame_is_split():
    """1100 frames of 65 points against 257 faces: two staging chunks walked by ONE workgroup per frame, outputs written by the
    lanes themselves (no workspace), against the same frames in a batch of three, whose faces are split"""
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
        assert_frame(small, b, ref.point_mesh(hands[b, 100:165], boxes[b], faces), b)
    for key in KEYS:
        assert np.array_equal(bits(got[key]), bits(small[key])[kind]), key


# =============================================================================================== call hygiene
def test_null_outputs_and_bad_arguments_leave_the_rest_untouched():
    from homan_amd import lib
    h = lib.lib()
    ptr, stream = lib.ptr, lib.stream()
    p, v, f = comparison_cases()["hand->box"]
    want = restated("hand->box")
    B, N, V, F = 1, len(p), len(v), len(f)
    points, verts, faces = (torch.from_numpy(np.array(a)).cuda() for a in (p[None], v[None], f))
    ws = torch.empty(h.hm_point_mesh_workspace_bytes(B, N, F), dtype=torch.uint8, device="cuda")
    assert ws.numel() == N * 12

    def fresh():
        return {"d2": torch.full((B, N), -7.0, device="cuda"), "face": torch.full((B, N), -7, dtype=torch.int32, device="cuda"),
                "inside": torch.full((B, N), -7, dtype=torch.int32, device="cuda"), "closest": torch.full((B, N, 3), -7.0, device="cuda")}

    def call(out, pp=points, vp=verts, fp=faces, B=B, N=N, V=V, F=F, w=ws):
        return h.hm_point_mesh_distance(*(None if t is None else ptr(t) for t in (pp, vp, fp)), B, N, V, F,
                                        *(None if out[k] is None else ptr(out[k]) for k in KEYS), None if w is None else ptr(w), stream)
    # every combination of NULL outputs but all four: the outputs asked for are the full call's, the buffers of the others
    # (kept aside) stay as they were
    for mask in range(1, 16):
        out = fresh()
        asked = {k: (out[k] if mask >> i & 1 else None) for i, k in enumerate(KEYS)}
        assert call(asked) == 0, mask
        torch.cuda.synchronize()
        for i, k in enumerate(KEYS):
            if mask >> i & 1:
                assert np.array_equal(bits(out[k].cpu().numpy()[0]), bits(want[k])), (mask, k)
            else:
                assert (out[k] == -7).all(), (mask, k)
    out = fresh()
    for kw in (dict(pp=None), dict(vp=None), dict(fp=None), dict(B=0), dict(B=-1), dict(N=0), dict(V=0), dict(F=0), dict(F=-2),
               dict(w=None)):
        assert call(out, **kw) == -1, kw
    assert call(dict.fromkeys(KEYS)) == -1
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in out.values())
    assert call(out) == 0                                                             # the buffers are still usable
    torch.cuda.synchronize()
    assert_frame({k: t.cpu().numpy() for k, t in out.items()}, 0, want, "after the refusals")
    # the workspace holds whatever the last call left: the next call initialises it itself
    ws.fill_(0x5a)
    out = fresh()
    assert call(out) == 0
    torch.cuda.synchronize()
    assert_frame({k: t.cpu().numpy() for k, t in out.items()}, 0, want, "dirty workspace")


def test_sign_at_the_voxel_centres_equals_the_voxeliser():
    from homan_amd import ops
    h = 0.005
    v, f = mesh("hand")
    box = vref.box_of(*vref.index_box(v, h))
    words = ops.solid_voxels(torch.from_numpy(v[None]).cuda(), f, h, box[None]).cpu().numpy().view(np.uint32)[0]
    occ = ((words[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(words.shape[:-1] + (-1,))[..., :box[3]].astype(bool)
    cx, cy, cz = (vref.centres(box[a], box[3 + a], h) for a in range(3))
    grid = np.ascontiguousarray(np.stack(np.meshgrid(cz, cy, cx, indexing="ij"), -1)[..., ::-1].reshape(-1, 3))
    got = device(grid, v, f, closest=False)
    assert np.array_equal(got["inside"][0].reshape(occ.shape) == 1, occ) and occ.sum() > 1000


# =============================================================================================== the metrics
@functools.lru_cache(maxsize=None)
def scene(hands):
    """4 frames of hand(s) on the box, in frame 2 far from it; (person (4*hands, 778, 3), object (4, Vb, 3), hand faces, box
    faces)"""
    bv, bf = mesh("box")
    person, obj = [], []
    for b in range(4):
        obj.append((bv + F32(0.0017 * b)).astype(F32))
        away = (0.4, 0.0, 0.0) if b == 2 else (0.0, 0.0, 0.0)
        for k in range(hands):
            shift = np.array([0.004 + 0.009 * k - 0.002 * b, 0.006 - 0.004 * k, 0.002 * b]) + away + 0.0017 * b
            person.append(posed_hand("box", angle=0.3 * b + 0.4 * k, shift=tuple(shift)))
    return np.stack(person), np.stack(obj), mesh("hand")[1], bf


@functools.lru_cache(maxsize=None)
def scene_restated(hands):
    person, obj, hf, bf = scene(hands)
    return tuple(ref.surface_metrics(list(person[b * hands:(b + 1) * hands]), [hf] * hands, obj[b], bf) for b in range(4))


@pytest.mark.parametrize("hands", (1, 2))
def test_get_surface_metrics_equals_the_restated_metrics(hands):
    from homan_amd import pointmetrics
    person, obj, hf, bf = scene(hands)
    want = scene_restated(hands)
    args = (torch.from_numpy(person), torch.from_numpy(obj), np.stack([hf] * hands), bf[None])
    got = pointmetrics.get_surface_metrics(*args)
    keys = ["pen_depth", "pen_depth_obj", "min_dist", "contact_share", "has_contact"]
    assert list(got) == keys and all(len(v) == 4 for v in got.values())
    print(f"{hands} hand(s): pen_depth (mm) {[round(x * 1e3, 3) for x in got['pen_depth']]}, pen_depth_obj "
          f"{[round(x * 1e3, 3) for x in got['pen_depth_obj']]}, min_dist {[round(x * 1e3, 3) for x in got['min_dist']]}, "
          f"share {[round(x, 3) for x in got['contact_share']]}")
    for key in keys:
        assert got[key] == [w[key] for w in want], key
    assert all(isinstance(x, float) for x in got["pen_depth"]) and all(isinstance(x, bool) for x in got["has_contact"])
    assert got["has_contact"] == [True, True, False, True] and got["pen_depth"][2] == 0.0 and got["contact_share"][2] == 0.0
    assert min(got["pen_depth"][:2]) > 0.001 and max(got["pen_depth_obj"]) > 0.001 and got["min_dist"][2] > 0.3
    full = pointmetrics.get_surface_metrics(*args, per_vertex=True)
    assert list(full) == keys + ["signed_dist"] and {k: full[k] for k in keys} == got
    signed = np.concatenate([w["signed_dist"] for w in want])
    assert full["signed_dist"].dtype == np.float64 and full["signed_dist"].shape == (4 * hands, 778)
    assert np.array_equal(bits(full["signed_dist"]), bits(signed))
    # any chunking, down to one frame per chunk, gives the same values; a frame alone gives the frame's values
    frame_bytes = pointmetrics.surface_frame_bytes(hands, 778, obj.shape[1])
    for frames_per_chunk in (3, 1):
        again = pointmetrics.get_surface_metrics(*args, per_vertex=True, max_bytes=frames_per_chunk * frame_bytes + 5)
        assert {k: again[k] for k in keys} == got and np.array_equal(bits(again["signed_dist"]), bits(signed)), frames_per_chunk
    with pytest.raises(ValueError):
        pointmetrics.get_surface_metrics(*args, max_bytes=frame_bytes - 1)
    alone = pointmetrics.get_surface_metrics(args[0][hands:2 * hands], args[1][1:2], args[2], args[3])
    assert {k: v[0] for k, v in alone.items()} == {k: v[1] for k, v in got.items()}
    # the threshold decides contact where nothing penetrates
    loose = pointmetrics.get_surface_metrics(*args, contact_thresh=0.5)
    assert loose["has_contact"] == [True] * 4 and loose["contact_share"][2] == 1.0 and loose["pen_depth"] == got["pen_depth"]


def test_known_depths_of_cubes():
    from homan_amd import pointmetrics
    from tests.test_surfmetrics import _cubes
    for gap, contact in ((-0.003, True), (0.002, True), (0.008, False)):
        (sv, sf), (bv, bf) = _cubes(gap)
        got = pointmetrics.get_surface_metrics(torch.from_numpy(sv[None]), torch.from_numpy(bv[None]), sf[None], bf[None])
        want = ref.surface_metrics([sv], [sf], bv, bf)
        assert {k: v[0] for k, v in got.items()} == {k: want[k] for k in got}
        assert got["has_contact"] == [contact] and abs(got["min_dist"][0] - abs(gap)) < 1e-7
        assert abs(got["pen_depth"][0] - max(-gap, 0.0)) < 1e-7


# =============================================================================================== sequences
def test_evaluate_sequence_surface_frame_by_frame():
    from homan_amd import ho3deval, pointmetrics, synth
    hv, hf = mesh("hand")
    hand = (hv + np.array([0.0, 0.0, 0.5], F32)).astype(F32)
    box, faces = synth.box_mesh(2, 2, 2, scale=0.08)
    box = np.asarray(box, F32) - np.asarray(box, F32).mean(0)
    faces = np.asarray(faces)
    joints = np.zeros((21, 3), F32) + hand.mean(0)
    seq = {f: {"hand_verts3d": (hand + F32(0.002 * f)).astype(F32), "hand_joints3d": joints,
               "obj_verts3d": (box + hand.mean(0) + F32(0.012 * f)).astype(F32), "img_path": "seq/rgb/0000.png"}
           for f in (0, 2, 6)}
    runs = {chunk: ho3deval.evaluate_sequence_surface(seq, 7, faces, hf, chunk=chunk) for chunk in (1, 3, 512)}
    res = runs[3]
    keys = ["pen_depth", "pen_depth_obj", "min_dist", "contact_share", "has_contact"]
    assert list(res) == keys + [k + "_mean" for k in keys]
    for chunk in (1, 512):
        for key in res:
            assert np.array_equal(res[key], runs[chunk][key]), (key, chunk)
    pred_hand = ho3deval.interpolate_sequence(seq, 7, "hand_verts3d", ho3deval.CAMEXTR_SIGNS)
    pred_obj = ho3deval.interpolate_sequence(seq, 7, "obj_verts3d", ho3deval.CAMEXTR_SIGNS)
    direct = pointmetrics.get_surface_metrics(pred_hand, pred_obj, hf[None], faces[None])
    for key in keys:
        assert res[key].dtype == np.float64 and res[key].shape == (7,)
        assert np.array_equal(res[key], np.asarray(direct[key], np.float64)), key
        assert res[key + "_mean"] == float(res[key].mean())
    ph, po = pred_hand.cpu().numpy(), pred_obj.cpu().numpy()
    for f in (0, 3, 6):                                                                # against the restatement itself
        want = ref.surface_metrics([ph[f]], [hf], po[f], faces)
        assert all(res[key][f] == float(want[key]) for key in keys), f
    assert res["has_contact"].max() == 1.0 and res["pen_depth"].max() > 0.001 and len(set(res["pen_depth"].tolist())) > 3
    # the neighbours are untouched: the plausibility walk on the same sequence gives the same values before and after
    before = ho3deval.evaluate_sequence_plausibility(seq, 7, faces, hf, chunk=4)
    ho3deval.evaluate_sequence_surface(seq, 7, faces, hf, chunk=4)
    after = ho3deval.evaluate_sequence_plausibility(seq, 7, faces, hf, chunk=4)
    assert all(np.array_equal(before[k], after[k]) for k in before)
