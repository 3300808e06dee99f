"""CPU side of the mesh preparation (csrc/remesh.hip, ops.lattice_signs / ops.surface_nets, homan_amd/meshprep.py): properties and
known answers of the rules on the NumPy restatement tests/meshprep_ref.py, which the GPU tests hold the kernels to bit for bit;
the budget search, the .obj / .off files, and the argument checks of the wrappers and of the library that need no device.

Bars, measured on the restatement (printed by the tests that assert them):
  snapped vertices   re-measured against the source, the distance of a snapped vertex is the rounding of the closest point's own
                     coordinates and of the second search: largest 1.5e-8 on the cubes, 3.3e-8 on the icosphere, 6.4e-8 on the
                     bottle.  Bar: 4 ulp of the largest source coordinate, 4 * 2^-23 * max|v| (5.4e-8, 2.1e-7, 3.1e-7 there): a
                     margin of 3.6 to 6.5 over the measured.
  unsnapped vertices keep their lattice position because d2 > (snap_limit h)^2 in fp32: re-measured, the same comparison, no margin.
  icosphere volume   relative error against the source's own volume 4.3e-2, 9.4e-3, 2.6e-3 at R = 6, 13, 24 (the lattice cuts
                     corners: second order in h).  Bars: strictly decreasing, and at R = 24 below 5.2e-3 (twice the measured)."""
import functools
import inspect
import pickle

import numpy as np
import pytest
import torch

from tests import meshprep_ref as mref
from tests import surfmetrics_ref as sref
from tests import volmetrics_ref as vref
from tests import winding_ref as wref
from tests.test_surfmetrics import mesh
from tests.test_winding import open_faces

F32 = np.float32
CUBE_LO, CUBE_SIDE = np.array([0.013, -0.021, 0.034]), 0.08
SCENE_R, SCENE_TIGHT, SCENE_WIDE = 16, 100, 500


@functools.lru_cache(maxsize=None)
def source(name):
    """the source meshes of both test files: (verts fp32, faces int32), shared and left unchanged"""
    if name in ("cube", "lidless"):
        v, f = vref.cube_mesh(CUBE_LO, CUBE_LO + CUBE_SIDE)
        if name == "lidless":
            lid = (v[f][:, :, 2] == v[:, 2].max()).all(1)
            assert lid.sum() == 2
            f = f[~lid]
    elif name == "two_cubes":
        v0, f0 = vref.cube_mesh(CUBE_LO, CUBE_LO + 0.04)
        v1, f1 = vref.cube_mesh(CUBE_LO + [0.04, 0.04, 0.0], CUBE_LO + [0.08, 0.08, 0.04])
        v, f = np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)])
    elif name == "icosphere":
        v, f = mref.icosphere(2, 0.05, (0.01, -0.02, 0.4))
    elif name == "bottle_open":
        v, f = mesh("bottle")
        f = open_faces(f)
    else:
        raise KeyError(name)
    v, f = np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


MESH_CASES = (("cube", 4), ("cube", 7), ("lidless", 4), ("lidless", 7), ("icosphere", 6), ("icosphere", 13), ("bottle_open", 8),
              ("two_cubes", 5))


@functools.lru_cache(maxsize=None)
def remeshed(name, R):
    """the restatement's make_watertight of a source at R cells: computed once, shared, left unchanged"""
    v, f = source(name)
    out = mref.make_watertight(v, f, resolution=R)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sign_field(name):
    """sign fields fed to the surface nets directly -> (inside (nz, ny, nx) int32, origin, pitch)"""
    if name == "noise13":                                                   # 13^3 cells, half the corners inside
        field = np.random.default_rng(13).integers(0, 2, (14, 14, 14))
    elif name == "one":
        field = np.zeros((3, 3, 3), int)
        field[1, 1, 1] = 1
    elif name == "empty":
        field = np.zeros((4, 5, 6), int)
    elif name == "full":                                                    # every corner flagged: the outer layer is cleared
        field = np.ones((5, 4, 7), int)
    elif name == "block":
        field = np.zeros((6, 7, 8), int)
        field[1:3, 2:5, 1:5] = 1                                            # a x b x c = 4 x 3 x 2 inside corners
    else:
        raise KeyError(name)
    field = field.astype(np.int32)
    field.setflags(write=False)
    return field, np.array([0.25, -1.5, 3.0], F32), F32(0.37)


def nets(name):
    return mref.surface_nets(*sign_field(name))


def assert_closed_oriented_positive(vertices, faces):
    from homan_amd import meshutils
    t = meshutils.mesh_topology(faces)
    assert t == {"closed": True, "oriented": True, "boundary_edges": 0, "nonmanifold_edges": 0}, t
    assert faces.min() >= 0 and faces.max() == len(vertices) - 1
    assert np.isfinite(vertices).all()
    assert mref.signed_volume(vertices, faces) > 0


# =============================================================================================== properties of the rules
@pytest.mark.parametrize("name,R", MESH_CASES)
def test_remeshed_sources_are_closed_oriented_and_of_positive_volume(name, R):
    v, f = source(name)
    out = remeshed(name, R)
    assert_closed_oriented_positive(out["vertices"], out["faces"])
    assert_closed_oriented_positive(out["lattice_vertices"], out["faces"])
    assert out["vertices"].dtype == F32 and out["faces"].dtype == np.int64
    print(name, R, "dims", out["dims"], "vertices", len(out["vertices"]), "snapped", int(out["snapped"].sum()),
          "repair", out["repair_passes"], out["repaired_corners"])
    # the outermost corner layer lies strictly outside the source's box
    lat = mref.lattice(v, f, R)
    pts = mref.corners(lat["origin"], lat["pitch"], lat["dims"]).reshape(lat["dims"][::-1] + (3,))
    first, last = pts[0, 0, 0], pts[-1, -1, -1]
    assert (first < lat["lo"]).all() and (last > lat["hi"]).all()
    assert (pts[1, 1, 1] < lat["lo"]).all() and (pts[-2, -2, -2] > lat["hi"]).all()      # and so does the layer next to it
    assert max(lat["dims"]) == R + 5


def test_two_cubes_meeting_along_an_edge_run_the_repair():
    out = remeshed("two_cubes", 5)
    assert out["repaired_corners"] > 0 and out["repair_passes"] >= 1
    v, f = source("two_cubes")
    raw = mref.clear_outer(mref.lattice_signs(v, f, 5)["inside"])
    assert int(mref.repair(raw)[0].sum() - raw.sum()) == out["repaired_corners"]


def test_noise_field_is_closed_after_the_repair_and_not_before():
    from homan_amd import meshutils
    out = nets("noise13")
    assert_closed_oriented_positive(out["vertices"], out["faces"])
    assert out["repair_passes"] >= 2 and out["repaired_corners"] > 100
    field = mref.clear_outer(sign_field("noise13")[0])
    assert not (out["field"][0].any() or out["field"][-1].any() or out["field"][:, 0].any() or out["field"][:, -1].any()
                or out["field"][:, :, 0].any() or out["field"][:, :, -1].any())
    assert (out["field"] | field == out["field"]).all()                     # the repair only sets corners
    # without the repair the same field has edges with four faces
    saved, mref.repair = mref.repair, lambda s: (s, 0, 0)
    try:
        raw = mref.surface_nets(*sign_field("noise13"))
    finally:
        mref.repair = saved
    assert meshutils.mesh_topology(raw["faces"])["nonmanifold_edges"] > 100


def test_known_answers():
    """One inside corner: the 8 cells around it and the 6 lattice edges that leave it, a cube of 12 triangles.  Nothing inside:
    nothing.  A solid block of a x b x c inside corners: the active cells are those that touch the block, (a + 1)(b + 1)(c + 1),
    less those with all 8 corners in it, (a - 1)(b - 1)(c - 1); the sign-changing edges leave the block through its six sides,
    one per corner of the side: 2 (ab + bc + ca) quads, twice as many triangles."""
    one = nets("one")
    assert one["vertices"].shape == (8, 3) and one["faces"].shape == (12, 3) and one["repair_passes"] == 0
    assert_closed_oriented_positive(one["vertices"], one["faces"])
    field, origin, h = sign_field("one")
    # each vertex is the mean of three edge midpoints of its cell, each half a cell off the corner along one axis: a sixth along every axis
    centre = origin + F32(1.0) * h
    # (coordinates up to 3.4, an fp32 ulp of 2.4e-7 there: three roundings on the way and one in this subtraction)
    assert np.allclose(np.abs(one["vertices"] - centre), h / 6, rtol=0, atol=4 * 2.4e-7)
    assert abs(mref.signed_volume(one["vertices"], one["faces"]) - (float(h) / 3) ** 3) < 1e-6
    # The order and the orientation, by hand.  The inside corner is (1, 1, 1); cell (ci, cj, ck) of the 2 x 2 x 2 cells has vertex
    # ci + 2 cj + 4 ck.  x-edges by base corner: (0, 1, 1), outside, then (1, 1, 1), inside; their cells, the base shifted by
    # (-1,-1), (0,-1), (0,0), (-1,0) along (y, z): (0,0,0), (0,1,0), (0,1,1), (0,0,1) = 0, 2, 6, 4, reversed for the outside base;
    # (1,0,0), (1,1,0), (1,1,1), (1,0,1) = 1, 3, 7, 5.  y-edges from (1, 0, 1) and (1, 1, 1), shifts along (z, x): 0, 4, 5, 1 reversed;
    # 2, 6, 7, 3.  z-edges from (1, 1, 0) and (1, 1, 1), shifts along (x, y): 0, 1, 3, 2 reversed; 4, 5, 7, 6.
    quads = [(4, 6, 2, 0), (1, 3, 7, 5), (1, 5, 4, 0), (2, 6, 7, 3), (2, 3, 1, 0), (4, 5, 7, 6)]
    assert one["faces"].tolist() == [list(t) for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    # vertex ci + 2 cj + 4 ck sits a sixth of a cell off the inside corner, towards its own cell
    signs = np.array([[2 * ((n >> a) & 1) - 1 for a in range(3)] for n in range(8)], F32)
    assert np.allclose(one["vertices"] - centre, signs * (h / 6), rtol=0, atol=4 * 2.4e-7)
    empty = nets("empty")
    assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3) and empty["cells"] == 0
    assert empty["vertices"].dtype == F32 and empty["faces"].dtype == np.int32
    a, b, c = 4, 3, 2
    block = nets("block")
    assert block["cells"] == len(block["vertices"]) == (a + 1) * (b + 1) * (c + 1) - (a - 1) * (b - 1) * (c - 1) == 54
    assert len(block["faces"]) == 4 * (a * b + b * c + c * a) == 104
    assert_closed_oriented_positive(block["vertices"], block["faces"])
    full = nets("full")                                                     # interior 3 x 2 x 5 corners
    assert full["cells"] == 4 * 3 * 6 - 2 * 1 * 4 and len(full["faces"]) == 4 * (6 + 10 + 15)
    assert_closed_oriented_positive(full["vertices"], full["faces"])
    # in the block, the first quad is the x-edge from the lowest base corner (0, 2, 1), outside: cells (0, 1..2, 0..1) reversed
    index = {c: n for n, c in enumerate(sorted(((ck, cj, ci) for ci in range(5) for cj in range(1, 5) for ck in range(0, 3)
                                                 if not (1 <= ci <= 3 and 2 <= cj <= 3 and ck == 1))))}
    assert len(index) == 54
    q = [index[(ck, cj, 0)] for cj, ck in ((1, 0), (2, 0), (2, 1), (1, 1))][::-1]
    assert block["faces"][:2].tolist() == [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    assert len(block["faces"]) // 2 == 2 * 3 * 2 + 2 * 4 * 2 + 2 * 4 * 3      # x-, y-, z-edges through the sides


# =============================================================================================== quality
@pytest.mark.parametrize("name,R", MESH_CASES)
def test_snapped_vertices_lie_on_the_source_and_the_others_beyond_the_limit(name, R):
    v, f = source(name)
    out = remeshed(name, R)
    again = sref.point_mesh(out["vertices"], v, f)
    snapped = out["snapped"]
    assert snapped.sum() >= len(snapped) // 2                               # the snap does its work on every case
    d = np.sqrt(again["d2"].astype(np.float64))
    bar = 4 * 2.0 ** -23 * float(np.abs(v).max())
    print(name, R, "largest distance of a snapped vertex", d[snapped].max(), "bar", bar, "unsnapped", int((~snapped).sum()))
    assert d[snapped].max() <= bar
    h = F32(out["pitch"])
    limit2 = (mref.SNAP_LIMIT * mref.SNAP_LIMIT) * (h * h)
    assert (again["d2"][~snapped] > limit2).all()
    assert np.array_equal(out["vertices"][~snapped], out["lattice_vertices"][~snapped])
    if name == "lidless":                                                   # the film over the missing lid stays where it is
        assert (~snapped).sum() >= 1 or R < 7


def test_icosphere_volume_converges_to_the_source():
    v, f = source("icosphere")
    want = mref.signed_volume(v, f)
    errs = [abs(mref.signed_volume(remeshed("icosphere", R)["vertices"], remeshed("icosphere", R)["faces"]) - want) / want
            for R in (6, 13, 24)]
    print("icosphere: relative volume error at R = 6, 13, 24", errs)
    assert errs[0] > errs[1] > errs[2]
    assert errs[2] < 5.2e-3


# =============================================================================================== the budget search
@functools.lru_cache(maxsize=None)
def cube_budget(target):
    v, f = source("cube")
    return mref.make_watertight(v, f, target_vertices=target, snap_limit=None)


def test_budget_search_follows_the_written_down_bisection():
    from homan_amd import meshprep
    out = cube_budget(1000)
    counts = dict(out["probes"])
    assert len(out["vertices"]) == counts[out["resolution"]] <= 1000
    # the probes, by hand: [4]; then a = 5, b = 128: the midpoints the counts steer to
    a, b, want = 5, 128, [4]
    while a <= b:
        m = (a + b) // 2
        want.append(m)
        a, b = (m + 1, b) if counts[m] <= 1000 else (a, m - 1)
    assert [R for R, _ in out["probes"]] == want and want[1] == 66 and len(want) == 8
    assert out["resolution"] == max(R for R, n in out["probes"] if n <= 1000)
    # the product's bisection is the restatement's, probe for probe
    got = meshprep.choose_resolution(lambda R: counts[R], 1000)
    assert got == (out["resolution"], out["probes"])
    assert meshprep.BUDGET_RESOLUTIONS == (mref.BUDGET_LO, mref.BUDGET_HI) == (4, 128)
    with pytest.raises(ValueError):
        meshprep.choose_resolution(lambda R: 99, 98)
    with pytest.raises(ValueError):
        mref.choose_resolution(lambda R: 99, 98)
    assert meshprep.choose_resolution(lambda R: 0, 1) == (128, [(4, 0), (66, 0), (97, 0), (113, 0), (121, 0), (125, 0), (127, 0), (128, 0)])


# =============================================================================================== the downstream scene
@functools.lru_cache(maxsize=None)
def scene():
    """the remeshed opened bottle at R = 16 and a cloud about it -> (points, remesh, signs against the opened source, distance
    to it): the GPU test compares the parity sign against the remesh with the winding sign against the source on these points"""
    v, f = source("bottle_open")
    lo, hi = v.min(0), v.max(0)
    rng = np.random.default_rng(16)
    tight = lo + rng.random((SCENE_TIGHT, 3)) * (hi - lo)                   # in the source's box, and in twice the box
    p = np.concatenate([tight, lo - 0.5 * (hi - lo) + rng.random((SCENE_WIDE, 3)) * 2.0 * (hi - lo)]).astype(F32)
    out = remeshed("bottle_open", SCENE_R)
    return p, out, wref.point_mesh_winding(p, v, f)["inside"], np.sqrt(sref.point_mesh(p, v, f)["d2"].astype(np.float64))


def test_remeshed_bottle_keeps_the_sign_of_the_open_source_outside_a_band_of_two_cells():
    p, out, want, dist = scene()
    assert_closed_oriented_positive(out["vertices"], out["faces"])
    far = dist > 2.0 * float(out["pitch"])
    got = sref.point_mesh(p, out["vertices"], out["faces"].astype(np.int32))["inside"]
    print("scene: points beyond 2h", int(far.sum()), "of", len(p), "inside among them", int(want[far].sum()),
          "disagreeing", int((got[far] != want[far]).sum()))
    assert far.sum() >= 0.7 * len(p)
    assert want[far].sum() >= 5 and (want[far] == 0).sum() >= 5             # both signs occur beyond the band
    assert np.array_equal(got[far], want[far])


# =============================================================================================== files
def test_obj_and_off_round_trips(tmp_path):
    from homan_amd import meshprep
    v, f = source("icosphere")
    for ext in (".obj", ".off"):
        path = str(tmp_path / ("m" + ext))
        meshprep.save_mesh(path, v, f)
        gv, gf = meshprep.load_mesh(path)
        assert gv.dtype == np.float64 and gf.dtype == np.int64
        assert np.array_equal(gv.astype(F32), v) and np.array_equal(gf, f)    # nine digits carry an fp32
    (tmp_path / "poly.obj").write_text(
        "# a square, a pentagon with texture / normal tokens, a triangle by negative indices\nmtllib x.mtl\no thing\n"
        "v 0 0 0\nv 1 0 0 0.5\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\nf 1 2 3 4\nv 2 0 0\nf 1/1/1 2/1/1 5/1/1 3//1 4/1\n"
        "v 0 0 1\nf -1 -2 -6\ns off\n")
    gv, gf = meshprep.load_obj(str(tmp_path / "poly.obj"))
    assert gv.shape == (6, 3) and gv[1].tolist() == [1.0, 0.0, 0.0]
    assert gf.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [0, 4, 2], [0, 2, 3], [5, 4, 0]]
    for head in ("OFF\n# comment\n5 2 0\n", "OFF 5 2 0\n"):
        (tmp_path / "poly.off").write_text(head + "0 0 0\n1 0 0\n1 1 0 # the third\n0 1 0\n0 0 1\n4 0 1 2 3\n3 0 1 4\n")
        gv, gf = meshprep.load_off(str(tmp_path / "poly.off"))
        assert gv.shape == (5, 3) and gv[2].tolist() == [1.0, 1.0, 0.0] and gf.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4]]
    (tmp_path / "bad.off").write_text("COFF 1 0 0\n0 0 0\n")
    with pytest.raises(ValueError):
        meshprep.load_off(str(tmp_path / "bad.off"))
    for bad in ("f 1 2\n", "v 0 0 0\nf 0 1 1\n"):
        (tmp_path / "bad.obj").write_text(bad)
        with pytest.raises(ValueError):
            meshprep.load_obj(str(tmp_path / "bad.obj"))
    with pytest.raises(ValueError):
        meshprep.load_mesh(str(tmp_path / "m.ply"))
    with pytest.raises(ValueError):
        meshprep.save_mesh(str(tmp_path / "m.ply"), v, f)


def test_prepare_meshes_skips_targets_whose_pickle_exists(tmp_path, monkeypatch):
    import importlib.util
    import os
    from homan_amd import meshprep
    spec = importlib.util.spec_from_file_location("prepare_meshes", os.path.join(os.path.dirname(__file__), "..", "tools",
                                                                                "prepare_meshes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    v, f = source("cube")
    for name in ("a", "b"):
        meshprep.save_obj(str(tmp_path / f"{name}.obj"), v, f)
    with open(tmp_path / "a_proc.pkl", "wb") as fh:
        pickle.dump({}, fh)
    (tmp_path / "list.txt").write_text(f"{tmp_path / 'b.obj'}\n{tmp_path / 'a.obj'}\n\n{tmp_path / 'b.obj'}\n")
    calls = []
    monkeypatch.setattr(meshprep, "simplify_mesh", lambda src, target, vert_nb: calls.append((src, target, vert_nb)) or
                        {"vertices": v, "faces": f, "resolution": 0})
    assert tool.main(["--file_path", str(tmp_path / "list.txt"), "--vertex_nb", "500"]) == 1
    assert calls == [(str(tmp_path / "b.obj"), str(tmp_path / "b_proc.obj"), 500)]


# =============================================================================================== arguments
def test_wrappers_check_their_arguments_before_any_device_work():
    from homan_amd import meshprep, ops
    v, f = source("cube")
    tv = torch.from_numpy(v.copy())
    for fn in (lambda *a, **k: ops.lattice_signs(*a, **k), lambda vv, ff, R, **k: meshprep.make_watertight(vv, ff, resolution=R, **k)):
        for bad in (v[None], v[:, :2], v[:0], v.astype(np.int32), tv[None], tv.int()):
            with pytest.raises(ValueError):
                fn(bad, f, 8)
        for bad in (f[:, :2], f[:0], f.astype(F32), f[0]):
            with pytest.raises(ValueError):
                fn(v, bad, 8)
        for R in (1, 0, -4, 257, 8.5):
            with pytest.raises(ValueError):
                fn(v, f, R)
        for sign in ("auto", "Winding", "", None):
            with pytest.raises(ValueError):
                fn(v, f, 8, sign=sign)
        with pytest.raises(ValueError):                                     # a degenerate box
            fn(np.zeros((8, 3), F32), f, 8)
        with pytest.raises(ValueError):                                     # no face names a finite vertex
            fn(np.full((8, 3), np.nan, F32), f, 8)
        with pytest.raises(ValueError):
            fn(v, f + 8, 8)
    for target in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            meshprep.make_watertight(v, f, target_vertices=target)
    for limit in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            meshprep.make_watertight(v, f, resolution=8, snap_limit=limit)
    field = sign_field("one")[0]
    for bad in (field.astype(F32), field[0], field[None], np.zeros((3, 3, 1), np.int32), np.zeros((2, 2, 513), np.int32),
                np.zeros((1025, 2, 2), np.int32), torch.zeros(3, 3, 3)):
        with pytest.raises(ValueError):
            ops.surface_nets(bad, (0, 0, 0), 1.0)
        with pytest.raises(ValueError):
            ops.surface_nets_count(bad)
    for origin in ((0, 0), (0, 0, 0, 0), (0, np.nan, 0), (np.inf, 0, 0), 1.0):
        with pytest.raises(ValueError):
            ops.surface_nets(field, origin, 1.0)
    for pitch in (0.0, -1.0, np.nan, np.inf, 1e-60, 1e60):
        with pytest.raises(ValueError):
            ops.surface_nets(field, (0, 0, 0), pitch)
    params = lambda fn: list(inspect.signature(fn).parameters)  # noqa: E731
    assert params(ops.lattice_signs) == ["verts", "faces", "resolution", "sign"]
    assert params(ops.surface_nets) == ["inside", "origin", "pitch"] and params(ops.surface_nets_count) == ["inside"]
    assert params(meshprep.make_watertight) == ["vertices", "faces", "resolution", "target_vertices", "snap_limit", "sign"]
    assert params(meshprep.simplify_mesh) == ["src_path", "target_path", "vert_nb", "save_pkl", "ignored"]
    d = inspect.signature(meshprep.make_watertight).parameters
    assert (d["resolution"].default, d["target_vertices"].default, d["sign"].default) == (None, 1000, "winding")
    assert d["snap_limit"].default == meshprep.SNAP_LIMIT == float(mref.SNAP_LIMIT) == float(F32(np.sqrt(F32(3.0))))
    assert ops.LATTICE_OFFSET == mref.OFFSET and ops.LATTICE_RESOLUTIONS == (mref.R_MIN, mref.R_MAX)
    origin, h, dims = ops.lattice_box(v, f, 7)                              # the host half of lattice_signs is the restatement's
    lat = mref.lattice(v, f, 7)
    assert np.array_equal(origin.view(np.uint32), lat["origin"].view(np.uint32)) and dims == lat["dims"]
    assert h.dtype == F32 and h == lat["pitch"]
    if not torch.cuda.is_available():            # no CPU path
        with pytest.raises(RuntimeError):
            ops.lattice_signs(v, f, 8)
        with pytest.raises(RuntimeError):
            ops.surface_nets(field, (0, 0, 0), 1.0)
        with pytest.raises(RuntimeError):
            ops.surface_nets_count(field)
        with pytest.raises(RuntimeError):
            meshprep.make_watertight(v, f, resolution=8)


def test_library_refuses_bad_arguments_without_a_launch():
    """made-up device addresses that are never dereferenced: every call here must fail its host checks before anything is enqueued
    (HM_ERR_BAD_ARG = -1)"""
    from homan_amd import lib
    h, p = lib.lib(), 1 << 20
    for name in ("hm_lattice_words", "hm_lattice_corners", "hm_lattice_repair", "hm_surface_nets_count", "hm_surface_nets_emit",
                 "hm_lattice_snap"):
        assert name in lib.exported_symbols()
    bad_dims = (dict(nx=1), dict(ny=1), dict(nz=0), dict(nx=-3), dict(nx=513), dict(nz=1025), dict(ny=1 << 20))
    inf, nan = float("inf"), float("nan")
    assert h.hm_lattice_words(64, 3, 5) == 15 and h.hm_lattice_words(65, 3, 5) == 30 and h.hm_lattice_words(2, 2, 2) == 4
    for kw in bad_dims:
        d = dict(dict(nx=4, ny=4, nz=4), **kw)
        assert h.hm_lattice_words(d["nx"], d["ny"], d["nz"]) == -1, kw

    def corners(nx=4, ny=4, nz=4, ox=0.0, oy=0.0, oz=0.0, hh=1.0, points=p):
        return h.hm_lattice_corners(nx, ny, nz, ox, oy, oz, hh, points, None)

    def repair(flags=p, nx=4, ny=4, nz=4, bits=p, report=p):
        return h.hm_lattice_repair(flags, nx, ny, nz, bits, report, None)

    def count(bits=p, nx=4, ny=4, nz=4, cell_bits=p, row_offsets=p, totals=p):
        return h.hm_surface_nets_count(bits, nx, ny, nz, cell_bits, row_offsets, totals, None)

    def emit(bits=p, cell_bits=p, row_offsets=p, totals=p, nx=4, ny=4, nz=4, ox=0.0, oy=0.0, oz=0.0, hh=1.0, max_vertices=8,
             max_triangles=12, vertices=p, triangles=p):
        return h.hm_surface_nets_emit(bits, cell_bits, row_offsets, totals, nx, ny, nz, ox, oy, oz, hh, max_vertices,
                                      max_triangles, vertices, triangles, None)

    def snap(lattice=p, closest=p, d2=p, n=8, snap_limit=1.0, hh=1.0, out=p, snapped=p):
        return h.hm_lattice_snap(lattice, closest, d2, n, snap_limit, hh, out, snapped, None)
    floats = (dict(hh=0.0), dict(hh=-1.0), dict(hh=inf), dict(hh=nan))
    origins = (dict(ox=nan), dict(oy=inf), dict(oz=-inf))
    misaligned = (p + 4, p + 1, p + 2)
    for kw in bad_dims + floats + origins + (dict(points=None),):
        assert corners(**kw) == -1, kw
    for kw in bad_dims + (dict(flags=None), dict(bits=None), dict(report=None)) + tuple(dict(bits=m) for m in misaligned):
        assert repair(**kw) == -1, kw
    for kw in (bad_dims + (dict(bits=None), dict(cell_bits=None), dict(row_offsets=None), dict(totals=None))
               + tuple(dict(bits=m) for m in misaligned) + tuple(dict(cell_bits=m) for m in misaligned)):
        assert count(**kw) == -1, kw
    for kw in (bad_dims + floats + origins + (dict(bits=None), dict(cell_bits=None), dict(row_offsets=None), dict(totals=None),
                                              dict(vertices=None), dict(triangles=None), dict(max_vertices=-1),
                                              dict(max_triangles=-2))
               + tuple(dict(bits=m) for m in misaligned) + tuple(dict(cell_bits=m) for m in misaligned)):
        assert emit(**kw) == -1, kw
    for kw in (dict(lattice=None), dict(closest=None), dict(d2=None), dict(out=None), dict(n=-1), dict(snap_limit=0.0),
               dict(snap_limit=-1.0), dict(snap_limit=nan), dict(snap_limit=inf)) + floats:
        assert snap(**kw) == -1, kw
    assert snap(n=0) == 0                                                   # nothing to do, nothing enqueued
    header = open(lib._build.HEADER).read()
    assert "ALIGNMENT: bits and cell_bits 8 bytes" in header
    assert "origin = lo - 1.381966f * h" in header and "1.7320508f" in header
