"""CPU side of the surface metrics (csrc/surfdist.hip, homan_amd/pointmetrics.py get_surface_metrics): known answers of the fp32
NumPy restatement tests/surfmetrics_ref.py, which the GPU tests hold the kernel to bit for bit, its distance against an
independently built float64 distance, and the argument checks of the wrappers and of the library that need no device.

The bar between the fp32 restatement and float64: |sqrt(d2_32) - dist_64| <= K * 2^-23 * S, S the largest of |p - a|, |p - b|,
|p - c| of the winning face.  K is not derived but measured over THIS file's inputs (`comparison_cases`: the synthetic hand
against the box and the bottle, both ways, the meshes interpenetrating, and the degenerate faces at unit scale).  Largest
ratios |error| / (2^-23 S) found on the CPU: hand->box 0.66, box->hand 6.2, hand->bottle 59.7, bottle->hand 93.8, degenerate
faces 0.56 / 0.61 / 0.39; K = 4 x 93.8, rounded up to a power of two = 512.  The large ratios are not lost digits of the region
walk: the closest point is formed in world coordinates, so the error has a floor of a few half-ulps of the COORDINATES (the
bottle sits 0.66 m from the origin as an object does in front of a camera: 3e-8 m per rounding, 5.6e-8 m observed) while S
is the few millimetres between a vertex and the surface it touches; in metres every error here is below 6e-8 on the meshes.
Every mesh used has height-to-edge ratios >= 1e-4 (asserted): below it the region walk does lose digits."""
import functools
import inspect

import numpy as np
import pytest
import torch

from tests import surfmetrics_ref as ref
from tests import volmetrics_ref as vref
from tests.test_volmetrics import rotated_bottle

F32 = np.float32
K_BAR = 512.0
EPS32 = 2.0 ** -23

# a right triangle with dyadic coordinates, and a point in each of the seven regions: (point, closest point, d2), all exact
TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], F32)
REGIONS = {"A": ([-1.0, -1.0, 0.5], [0.0, 0.0, 0.0], 2.25), "B": ([2.0, -0.5, 0.0], [1.0, 0.0, 0.0], 1.25),
           "AB": ([0.5, -1.0, 0.0], [0.5, 0.0, 0.0], 1.0), "C": ([-0.5, 2.0, 0.0], [0.0, 1.0, 0.0], 1.25),
           "AC": ([-1.0, 0.5, 0.0], [0.0, 0.5, 0.0], 1.0), "BC": ([1.0, 1.0, 0.0], [0.5, 0.5, 0.0], 0.5),
           "interior": ([0.25, 0.25, 2.0], [0.25, 0.25, 0.0], 4.0)}

# degenerate faces at unit scale: (vertices, faces)
DEGENERATE = {"a=b": ([[0.25, 0.5, -0.75], [0.25, 0.5, -0.75], [1.0, -0.25, 0.5]], [[0, 1, 2]]),
              "a=b=c": ([[0.25, 0.5, -0.75]], [[0, 0, 0]]),
              "collinear": ([[-0.5, 0.25, 1.0], [1.5, -0.75, 0.0], [0.0, 0.0, 0.75]], [[0, 1, 2]])}


@functools.lru_cache(maxsize=None)
def mesh(name):
    from homan_amd import synth
    from homan_amd.mano_assets import synthetic_mano
    if name == "hand":
        m = synthetic_mano(0)
        return m["v_template"].astype(F32), np.asarray(m["closed_faces"], np.int32)
    if name == "bottle":
        return rotated_bottle()
    if name == "box":
        v, f = synth.box_mesh()
        return (np.asarray(v, F32) + np.array([0.0137, -0.0291, 0.0453], F32)).astype(F32), np.asarray(f, np.int32)
    raise KeyError(name)


def posed_hand(target, angle=0.3, shift=(0.012, 0.03, 0.002)):
    """the hand turned about z and centred `shift` off the centroid of the mesh `target`: the two interpenetrate"""
    v, _ = mesh("hand")
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    centre = mesh(target)[0].astype(np.float64).mean(0)
    return ((v - v.mean(0)).astype(np.float64) @ rot.T + centre + np.asarray(shift)).astype(F32)


def degenerate_points():
    rng = np.random.default_rng(5)
    return (rng.random((64, 3)) * 3.0 - 1.0).astype(F32)


@functools.lru_cache(maxsize=None)
def comparison_cases():
    """{name: (points, verts, faces)}: every input of the fp32-against-float64 comparison, shared and left unchanged"""
    cases = {}
    for target, shift in (("box", (0.004, 0.006, 0.002)), ("bottle", (0.012, 0.03, 0.002))):
        hand = posed_hand(target, shift=shift)
        tv, tf = mesh(target)
        cases[f"hand->{target}"] = (hand, tv, tf)
        cases[f"{target}->hand"] = (tv, hand, mesh("hand")[1])
    for name, (v, f) in DEGENERATE.items():
        cases[name] = (degenerate_points(), np.asarray(v, F32), np.asarray(f, np.int32))
    for arrays in cases.values():
        for a in arrays:
            a.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def restated(name):
    """the fp32 restatement on a comparison case: computed once, shared, left unchanged"""
    out = ref.point_mesh(*comparison_cases()[name])
    for a in out.values():
        a.setflags(write=False)
    return out


# =============================================================================================== known answers
@pytest.mark.parametrize("region", sorted(REGIONS))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_the_seven_regions_of_a_right_triangle(region, dtype):
    p, q_want, d2_want = REGIONS[region]
    tri = TRI.astype(dtype)
    q, D = ref.face_distance(np.asarray([p], dtype), tri[None, 0], tri[None, 1], tri[None, 2])
    assert q[0].tolist() == q_want and D[0] == d2_want
    assert ref.independent_distance(np.asarray(p), *TRI) ** 2 == pytest.approx(d2_want, rel=1e-15)
    # every vertex order of the face gives the same point
    for order in ((1, 2, 0), (2, 0, 1), (0, 2, 1)):
        q2, D2 = ref.face_distance(np.asarray([p], dtype), *(tri[None, k] for k in order))
        assert q2[0].tolist() == q_want and D2[0] == d2_want


def test_points_on_a_vertex_an_edge_and_the_face():
    on = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.25, 0.0, 0.0], [0.0, 0.75, 0.0],
                   [0.25, 0.25, 0.0], [0.125, 0.5, 0.0]], F32)
    r = ref.point_mesh(on, TRI, [[0, 1, 2]])
    assert not r["d2"].any() and np.array_equal(r["closest"], on) and not r["face"].any()


def test_the_lower_face_wins_a_shared_edge():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, -1, 0.5], [5, 5, 5], [6, 5, 5], [5, 6, 5]], F32)
    faces = np.array([[4, 5, 6], [0, 1, 2], [1, 0, 3], [0, 1, 2]], np.int32)         # faces 1, 2 and 3 share the edge (0, 1)
    p = np.array([[0.5, -0.25, -1.0], [0.25, -0.5, -2.0]], F32)                      # nearest to that edge
    r = ref.point_mesh(p, verts, faces)
    assert r["face"].tolist() == [1, 1] and r["d2"].tolist() == [1.0625, 4.25]
    assert np.array_equal(r["closest"], np.array([[0.5, 0, 0], [0.25, 0, 0]], F32))
    swapped = ref.point_mesh(p, verts, faces[[0, 2, 1, 3]])
    assert swapped["face"].tolist() == [1, 1] and np.array_equal(swapped["d2"], r["d2"])
    assert ref.point_mesh(p, verts, faces[[1, 0, 2, 3]])["face"].tolist() == [0, 0]


def test_skipped_faces_and_points():
    v, f = vref.cube_mesh([0, 0, 0], [1, 1, 1])
    p = np.array([[0.5, 0.5, 0.25], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [2.0, 0.5, 0.5]], F32)
    want = ref.point_mesh(p, v, f)
    assert want["d2"].tolist() == [0.0625, np.inf, np.inf, 1.0] and want["inside"].tolist() == [1, 0, 0, 0]
    assert want["face"][1] == want["face"][2] == -1 and not want["closest"][1:3].any()
    # faces that name a vertex outside [0, V) or a non-finite one count nowhere: the results keep the numbering of the call
    more_v = np.concatenate([v, [[np.nan, 0.5, 0.5], [0.5, 0.5, np.inf]]]).astype(F32)
    more_f = np.concatenate([[[0, 1, 99], [-1, 2, 3], [8, 0, 1], [0, 9, 2]], f]).astype(np.int32)
    got = ref.point_mesh(p, more_v, more_f)
    assert np.array_equal(got["face"], np.where(want["face"] >= 0, want["face"] + 4, -1))
    for key in ("d2", "inside", "closest"):
        assert np.array_equal(got[key], want[key], equal_nan=True)
    none = ref.point_mesh(p, more_v, more_f[:4])
    assert np.isinf(none["d2"]).all() and (none["face"] == -1).all() and not none["inside"].any() and not none["closest"].any()


# =============================================================================================== fp32 against float64
@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_faces_are_finite(name):
    r = restated(name)
    assert np.isfinite(r["d2"]).all() and np.isfinite(r["closest"]).all() and (r["face"] == 0).all()
    p, v, f = comparison_cases()[name]
    q64, D64 = ref.face_distance(p.astype(np.float64)[:, None], *(v.astype(np.float64)[f[:, k]][None] for k in range(3)))
    assert np.abs(np.sqrt(D64[:, 0]) - ref.independent_mesh_distance(p, v, f)).max() < 1e-15 * 4
    if name == "a=b=c":
        assert np.array_equal(r["closest"], np.broadcast_to(v[0], (64, 3)))


def test_the_meshes_are_no_slivers():
    for name in ("hand", "box", "bottle"):
        ratio = ref.min_height_to_edge(*mesh(name))
        print(f"{name}: smallest height-to-edge ratio {ratio:.4f}")
        assert ratio >= 1e-4
    assert ref.min_height_to_edge(TRI, [[0, 1, 2]]) >= 1e-4 and ref.min_height_to_edge(*vref.cube_mesh([0, 0, 0], [1, 1, 1])) >= 1e-4


@pytest.mark.parametrize("name", ("hand->box", "box->hand", "hand->bottle", "bottle->hand", "a=b", "a=b=c", "collinear"))
def test_fp32_restatement_against_the_independent_float64_distance(name):
    p, v, f = comparison_cases()[name]
    r = restated(name)
    want = ref.independent_mesh_distance(p, v, f)
    err = np.abs(np.sqrt(r["d2"].astype(np.float64)) - want)
    ratio = err / (EPS32 * r["scale"])
    print(f"{name}: largest |sqrt(d2_32) - dist_64| {err.max():.3e} m, largest ratio to 2^-23 S {ratio.max():.3f} (K = {K_BAR})")
    assert (err <= K_BAR * EPS32 * r["scale"]).all()
    # the same rules in double agree with the independent distance to double precision
    r64 = ref.point_mesh(p, v, f, dtype=np.float64)
    assert np.abs(np.sqrt(r64["d2"]) - want).max() <= 64 * 2.0 ** -52 * r64["scale"].max()
    # the closest point lies at that distance and on the winning face's plane side of things: |p - closest| = sqrt(d2)
    gap = np.linalg.norm(p.astype(np.float64) - r["closest"].astype(np.float64), axis=1)
    assert np.abs(gap - want).max() <= 2 * K_BAR * EPS32 * r["scale"].max()
    if "->" in name:
        assert 20 < r["inside"].sum() < len(p) - 20                    # the meshes interpenetrate


def _sliver_error(ratio, trials=20, points=100):
    """largest |sqrt(d2_32) - dist_64| over random 5 cm triangles of the given height-to-edge ratio and points ~3 cm around"""
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(trials):
        a, e = rng.normal(size=3) * 0.02, rng.normal(size=3)
        e /= np.linalg.norm(e)
        n = np.cross(e, rng.normal(size=3))
        n /= np.linalg.norm(n)
        v = np.stack([a, a + 0.05 * e, a + 0.05 * rng.uniform(0.2, 0.8) * e + ratio * 0.05 * n]).astype(F32)
        pts = (a + rng.normal(size=(points, 3)) * 0.03).astype(F32)
        got = ref.point_mesh(pts, v, [[0, 1, 2]])
        worst = max(worst, float(np.abs(np.sqrt(got["d2"].astype(np.float64)) - ref.independent_mesh_distance(pts, v, [[0, 1, 2]])).max()))
    return worst


def test_slivers_keep_their_digits_down_to_a_ratio_of_1e_4():
    """the stated limit of the region walk: within 3e-8 m of float64 at 5 cm scale down to a height-to-edge
    ratio of 1e-4; thinner slivers that are not exactly degenerate lose digits (printed, not asserted)"""
    for ratio in (1e-2, 1e-4):
        assert _sliver_error(ratio, 40, 200) <= 3e-8, ratio
    for ratio in (1e-5, 1e-6, 1e-7):
        print(f"sliver of ratio {ratio:g}: largest error {_sliver_error(ratio, 40, 200):.3e} m")


# =============================================================================================== sign
def test_inside_and_outside_of_a_cube():
    v, f = vref.cube_mesh([-0.25, 0.0, 0.25], [0.5, 0.5, 1.0])
    rng = np.random.default_rng(2)
    p = (rng.random((400, 3)) * [1.25, 1.0, 1.25] + [-0.5, -0.25, 0.0]).astype(F32)
    within = ((p > v.min(0)) & (p < v.max(0))).all(1)
    assert 40 < within.sum() < 360
    r = ref.point_mesh(p, v, f)
    assert np.array_equal(r["inside"] == 1, within)
    for faces in (f[:, ::-1], np.roll(f, 1, axis=1), f[::-1]):                        # winding, vertex order, face order
        assert np.array_equal(ref.point_mesh(p, v, faces)["inside"], r["inside"])
    # in a box: the distance is that to the nearest wall
    wall = np.minimum(p - v.min(0), v.max(0) - p).min(1)[within]
    assert np.abs(np.sqrt(r["d2"][within]) - wall).max() < 1e-6


def test_points_on_the_face_planes_follow_the_half_open_rule():
    """a point ON a face whose plane is x = const is not in front of its own crossing (xhit > p_x is strict): on the low-x face
    it still sees the high-x face (inside), on the high-x face nothing (outside); a ray through an edge or a corner of the
    projected faces is given to exactly one of the triangles that share it (orient2), so such points get one crossing per wall"""
    v, f = vref.cube_mesh([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    p = np.array([[0.0, 0.5, 0.25], [1.0, 0.5, 0.25], [0.5, 0.5, 0.5], [0.5, 0.25, 0.25], [-1.0, 0.5, 0.5], [0.5, 0.0, 0.5],
                  [0.5, 1.0, 0.5], [-0.5, 0.0, 0.0], [0.5, 0.0, 0.0], [0.5, 1.0, 1.0]], F32)
    r = ref.point_mesh(p, v, f)
    assert r["inside"][:5].tolist() == [1, 0, 1, 1, 0]
    # the rows y = 0 / y = 1 and the corners: whatever the half-open rule gives them, it is what the voxeliser's rows get
    h = 0.25                                                           # centres at odd multiples of 1/8: none on a plane
    box = np.array([-2, -2, -2, 8, 8, 8])
    occ = vref.occupancy(v, f, h, box)
    cx = vref.centres(-2, 8, h)
    grid = np.stack(np.meshgrid(cx, cx, cx, indexing="ij"), -1).reshape(-1, 3)       # (x, y, z) major
    inside = ref.point_mesh(grid, v, f)["inside"].reshape(8, 8, 8)
    assert np.array_equal(inside.transpose(2, 1, 0) == 1, occ) and occ.sum() == 64
    # on-plane rows: a lattice whose centres lie ON the planes y = 0, z = 0.5 ...
    for pitch, first in ((0.5, -1), (1.0, -1)):
        cy = (np.arange(first, first + 4).astype(F32) + F32(0.5)) * F32(pitch)
        grid = np.stack(np.meshgrid(cy, cy, cy, indexing="ij"), -1).reshape(-1, 3)
        got = ref.point_mesh(grid, v, f)["inside"].reshape(4, 4, 4).transpose(2, 1, 0) == 1
        assert np.array_equal(got, vref.occupancy(v, f, pitch, np.array([first] * 3 + [4] * 3)))


def test_sign_at_voxel_centres_equals_the_voxeliser():
    h = 0.005
    for name in ("hand", "box"):
        v, f = mesh(name)
        first, last = vref.index_box(v, h)
        box = vref.box_of(first, last)
        occ = vref.occupancy(v, f, h, box)
        cx, cy, cz = (vref.centres(box[a], box[3 + a], h) for a in range(3))
        grid = np.stack(np.meshgrid(cz, cy, cx, indexing="ij"), -1)[..., ::-1].reshape(-1, 3)
        inside = ref.point_mesh(np.ascontiguousarray(grid), v, f)["inside"].reshape(occ.shape)
        assert np.array_equal(inside == 1, occ) and occ.sum() > 100, name


# =============================================================================================== metrics by hand
def _cubes(gap):
    """a 2 cm cube ("hand") whose +x face is `gap` short of (gap < 0: past) the -x face of a 10 cm cube at x = 0.25"""
    big = vref.cube_mesh([0.25, -0.05, -0.05], [0.35, 0.05, 0.05])
    hi = 0.25 - gap
    small = vref.cube_mesh([hi - 0.02, -0.01, -0.01], [hi, 0.01, 0.01])
    return small, big


def test_metrics_of_a_cube_pushed_into_a_cube():
    (sv, sf), (bv, bf) = _cubes(-0.003)
    m = ref.surface_metrics([sv], [sf], bv, bf)
    scale = 0.36
    assert abs(m["pen_depth"] - 0.003) <= K_BAR * EPS32 * scale and m["has_contact"] is True
    # four corners 3 mm inside, four 17 mm outside the wall: half the vertices are in contact
    assert m["contact_share"] == 0.5 and m["pen_depth_obj"] == 0.0 and m["min_dist"] == m["pen_depth"]
    assert (m["signed_dist"] < 0).sum() == 4 and abs(m["signed_dist"].max() - 0.017) < 1e-7
    assert m["signed_dist"].shape == (1, 8) and m["signed_dist"].dtype == np.float64


def test_contact_by_the_distance_threshold():
    for gap, contact in ((0.002, True), (0.008, False)):
        (sv, sf), (bv, bf) = _cubes(gap)
        m = ref.surface_metrics([sv], [sf], bv, bf)
        assert m["pen_depth"] == 0.0 and m["pen_depth_obj"] == 0.0 and abs(m["min_dist"] - gap) <= K_BAR * EPS32 * 0.36
        assert m["has_contact"] is contact and m["contact_share"] == (0.5 if contact else 0.0)
        assert ref.surface_metrics([sv], [sf], bv, bf, contact_thresh=0.01)["has_contact"] is True
        assert ref.surface_metrics([sv], [sf], bv, bf, contact_thresh=0.0)["has_contact"] is False


def test_an_object_vertex_inside_the_second_hand_only():
    """the object is a 2 cm cube; hand 0 is far away, hand 1 a 10 cm cube that holds one corner of the object 4 mm deep"""
    ov, of = vref.cube_mesh([0.0, 0.0, 0.0], [0.02, 0.02, 0.02])
    far, ff = vref.cube_mesh([0.5, 0.5, 0.5], [0.6, 0.6, 0.6])
    near, _ = vref.cube_mesh([0.016, 0.016, 0.016], [0.116, 0.116, 0.116])
    m = ref.surface_metrics([far, near], [ff, ff], ov, of)
    assert abs(m["pen_depth_obj"] - 0.004) <= K_BAR * EPS32 * 0.2 and m["has_contact"] is True
    # the near hand's corner (0.016,)*3 is inside the object too, 4 mm from its faces
    assert abs(m["pen_depth"] - 0.004) <= K_BAR * EPS32 * 0.2 and m["contact_share"] == 1.0 / 16.0
    alone = ref.surface_metrics([far], [ff], ov, of)
    assert alone["pen_depth_obj"] == 0.0 and alone["has_contact"] is False and alone["contact_share"] == 0.0
    # merged into one mesh, two overlapping hands would cancel: queried separately, they do not
    twice = ref.surface_metrics([near, near], [ff, ff], ov, of)
    assert twice["pen_depth_obj"] == m["pen_depth_obj"]
    merged = ref.point_mesh(ov, np.concatenate([near, near]), np.concatenate([ff, ff + 8]))
    assert not merged["inside"].any()


# =============================================================================================== arguments
def test_wrappers_check_their_arguments_before_any_device_work():
    from homan_amd import ho3deval, ops, pointmetrics
    v, f = vref.cube_mesh([0, 0, 0], [0.04, 0.04, 0.04])
    verts = torch.from_numpy(v)[None]
    for bad in (verts[0], verts[:, :, :2], verts[:0], verts.int(), v):
        with pytest.raises(ValueError):
            ops.point_mesh_distance(bad, verts, f)
        with pytest.raises(ValueError):
            ops.point_mesh_distance(verts, bad, f)
    for bad_faces in (f[:, :2], f[:0], f.astype(np.float32), f[0]):
        with pytest.raises(ValueError):
            ops.point_mesh_distance(verts, verts, bad_faces)
    with pytest.raises(ValueError):
        ops.point_mesh_distance(torch.cat([verts, verts]), verts, f)
    two = torch.cat([verts, verts])
    for kw in (dict(verts_person=torch.cat([two, verts])), dict(verts_person=verts[:, :, :2]), dict(max_bytes=0),
               dict(verts_object=two[:0]), dict(contact_thresh=-0.001), dict(contact_thresh=float("nan")),
               dict(contact_thresh=float("inf")), dict(max_bytes=pointmetrics.surface_frame_bytes(1, 8, 8) - 1),
               dict(verts_person=two.int())):
        args = dict(verts_person=two, verts_object=two, faces_person=f[None], faces_object=f[None])
        args.update(kw)
        with pytest.raises(ValueError):
            pointmetrics.get_surface_metrics(**args)
    with pytest.raises(ValueError):
        ho3deval.evaluate_sequence_surface({}, 4, f, f, chunk=0)
    with pytest.raises(ValueError):
        ho3deval.evaluate_sequence_surface({}, 4, f, f, contact_thresh=-1.0)
    params = lambda fn: list(inspect.signature(fn).parameters)  # noqa: E731
    assert params(ops.point_mesh_distance) == ["points", "verts", "faces", "closest"]
    assert params(pointmetrics.get_surface_metrics) == ["verts_person", "verts_object", "faces_person", "faces_object",
                                                        "contact_thresh", "per_vertex", "max_bytes"]
    defaults = inspect.signature(pointmetrics.get_surface_metrics).parameters
    assert (defaults["contact_thresh"].default, defaults["per_vertex"].default, defaults["max_bytes"].default) == (0.005, False, 256 << 20)
    assert params(ho3deval.evaluate_sequence_surface) == ["seq_res", "frame_nb", "obj_faces", "mano_faces_closed", "chunk",
                                                          "contact_thresh"]
    # the neighbours keep their signatures
    assert params(pointmetrics.get_inter_metrics) == ["verts_person", "verts_object", "faces_person", "faces_object"]
    assert params(ho3deval.evaluate_sequence_plausibility) == ["seq_res", "frame_nb", "obj_faces", "mano_faces_closed", "chunk",
                                                               "voxel"]
    if not torch.cuda.is_available():            # no CPU path
        with pytest.raises(RuntimeError):
            ops.point_mesh_distance(verts, verts, f)
        with pytest.raises(RuntimeError):
            pointmetrics.get_surface_metrics(verts, verts, f[None], f[None])


def test_the_contact_threshold_in_fp32_squares():
    """`d2 <= x` in fp32 with x = _d2_at_most(t) is the comparison sqrt((double)d2) <= t of the definition"""
    from homan_amd.pointmetrics import _d2_at_most
    for t in (0.005, 0.0, 0.002, 0.01, 1.0, 3.0e-23, 1e30):
        x = F32(_d2_at_most(t))
        assert float(x) == _d2_at_most(t) and np.sqrt(np.float64(x)) <= t
        if x < np.finfo(F32).max:
            assert np.sqrt(np.float64(np.nextafter(x, F32(np.inf)))) > t


def test_library_refuses_bad_arguments_without_a_launch():
    """made-up device addresses: every call here must fail its host checks before anything is enqueued (HM_ERR_BAD_ARG = -1)"""
    from homan_amd import lib, ops
    h, p = lib.lib(), 1 << 20

    def distance(points=p, verts=p, faces=p, B=1, N=8, V=8, F=3000, d2=p, face=p, inside=p, closest=p, ws=p):
        return h.hm_point_mesh_distance(points, verts, faces, B, N, V, F, d2, face, inside, closest, ws, None)
    assert h.hm_point_mesh_workspace_bytes(1, 8, 3000) == 8 * 12           # the faces of a lone frame are split
    for kw in (dict(points=None), dict(verts=None), dict(faces=None), dict(B=0), dict(B=-1), dict(N=0), dict(N=-5), dict(V=0),
               dict(V=-1), dict(F=0), dict(F=-3), dict(d2=None, face=None, inside=None, closest=None), dict(ws=None)):
        assert distance(**kw) == -1, kw
    for sizes in ((0, 8, 12), (1, 0, 12), (1, 8, 0), (-1, 8, 12)):
        assert h.hm_point_mesh_workspace_bytes(*sizes) == 0
    # one chunk of faces is never split, and a batch that fills the chip is not either: no workspace
    assert h.hm_point_mesh_workspace_bytes(1, 778, ops.SURFDIST_CHUNK) == 0
    assert h.hm_point_mesh_workspace_bytes(1, 778, ops.SURFDIST_CHUNK + 1) == 778 * 12
    assert h.hm_point_mesh_workspace_bytes(4096, 778, 3000) == 0
    assert h.hm_point_mesh_workspace_bytes(3, 5, 1552) == 3 * 5 * 12
