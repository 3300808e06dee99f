"""GPU side of the mesh preparation (csrc/remesh.hip): the kernels against the NumPy restatement tests/meshprep_ref.py.  The bar is
bit equality: faces and counts as integers, vertices as fp32 bit patterns - both sides do the same IEEE operations and the order
comes from the integer scan.  Shapes: the sign fields of tests/test_meshprep.py and lattices at the sizes where the kernels take
another path (an axis of 2 and of 3 corners; rows one short of, equal to and one beyond a 64-bit word of the packed field, which
is also the emit kernels' row tile, and beyond two words; a long thin lattice; more rows than one scan tile), then the sources of
that file end to end, the budget search, and the remeshed opened bottle through the consumers that assume a closed mesh."""
import functools
import pickle

import numpy as np
import pytest
import torch

from tests import meshprep_ref as mref
from tests.test_meshprep import (MESH_CASES, SCENE_R, assert_closed_oriented_positive, cube_budget, remeshed, scene, sign_field,
                                 source)

pytestmark = pytest.mark.gpu
F32 = np.float32
ORIGIN, PITCH = np.array([0.25, -1.5, 3.0], F32), F32(0.37)

# (nz, ny, nx) corners, share of inside corners
NOISE_SHAPES = {
    "axis2_x": ((5, 6, 2), 0.5), "axis2_y": ((5, 2, 6), 0.5), "axis2_z": ((2, 5, 6), 0.5), "axis3": ((3, 3, 3), 0.9),
    "axis3_x": ((6, 7, 3), 0.5), "word-1": ((5, 6, 63), 0.5), "word": ((6, 5, 64), 0.5), "word+1": ((5, 5, 65), 0.5),
    "word+2": ((4, 6, 66), 0.5), "two_words-1": ((4, 4, 127), 0.5), "two_words": ((4, 4, 128), 0.5), "two_words+2": ((4, 5, 130), 0.5),
    "thin_70x3x2": ((3, 4, 71), 0.5), "thin_dense": ((3, 4, 71), 0.85), "scan_tile+": ((46, 46, 4), 0.5),
    "scan_tiles_2+": ((70, 60, 5), 0.3),
}
FIELDS = ("noise13", "one", "empty", "full", "block") + tuple(NOISE_SHAPES)


@functools.lru_cache(maxsize=None)
def field(name):
    if name not in NOISE_SHAPES:
        return sign_field(name)
    shape, share = NOISE_SHAPES[name]
    rng = np.random.default_rng(sorted(NOISE_SHAPES).index(name))
    f = (rng.random(shape) < share).astype(np.int32)
    f.setflags(write=False)
    return f, ORIGIN, PITCH


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same_mesh(got, want):
    gv, gf = got["vertices"], got["faces"]
    gv = gv.cpu().numpy() if isinstance(gv, torch.Tensor) else gv
    gf = gf.cpu().numpy() if isinstance(gf, torch.Tensor) else gf
    assert (got["cells"] if "cells" in got else len(gv)) == len(want["vertices"])
    assert gv.shape == want["vertices"].shape and gf.shape == want["faces"].shape
    assert np.array_equal(gf, want["faces"])
    assert np.array_equal(bits(gv), bits(want["vertices"]))
    assert (got["repair_passes"], got["repaired_corners"]) == (want["repair_passes"], want["repaired_corners"])


@pytest.mark.parametrize("name", FIELDS)
def test_surface_nets_equal_the_restatement_bit_for_bit(name):
    from homan_amd import ops
    f, origin, pitch = field(name)
    want = mref.surface_nets(f, origin, pitch)
    got = ops.surface_nets(torch.from_numpy(f.copy()), origin, pitch)
    assert got["vertices"].dtype == torch.float32 and got["faces"].dtype == torch.int32 and got["vertices"].is_cuda
    print(name, f.shape, "vertices", got["cells"], "faces", len(got["faces"]), "repair", got["repair_passes"], got["repaired_corners"])
    assert_same_mesh(got, want)
    if name.startswith("axis2") or name == "empty":
        assert got["cells"] == 0 and got["faces"].shape == (0, 3)
    elif name != "axis3":
        assert got["cells"] > 0
        assert_closed_oriented_positive(got["vertices"].cpu().numpy(), got["faces"].cpu().numpy())
    if name in ("noise13", "scan_tile+", "word+2"):
        assert want["repair_passes"] >= 2 and want["repaired_corners"] > 0   # the repair's counts are compared on fields that need it
    again = ops.surface_nets(f.astype(bool), tuple(origin.tolist()), float(pitch))     # an array of booleans, a second call
    assert torch.equal(again["vertices"].view(torch.int32), got["vertices"].view(torch.int32))
    assert torch.equal(again["faces"], got["faces"])


def test_flags_of_any_integer_type_and_value_mean_inside():
    from homan_amd import ops
    f, origin, pitch = field("noise13")
    want = mref.surface_nets(f, origin, pitch)
    for flags in (torch.from_numpy(f * -7).long(), torch.from_numpy(f.astype(np.uint8) * 255).cuda(), torch.from_numpy(f != 0)):
        assert_same_mesh(ops.surface_nets(flags, origin, pitch), want)


@pytest.mark.parametrize("name,R", MESH_CASES)
def test_lattice_signs_and_make_watertight_equal_the_restatement(name, R):
    from homan_amd import meshprep, ops
    v, f = source(name)
    want = remeshed(name, R)
    lat = ops.lattice_signs(torch.from_numpy(v.copy()), f, R)
    ref_lat = mref.lattice_signs(v, f, R)
    assert lat["dims"] == ref_lat["dims"] == want["dims"] and lat["inside"].shape == ref_lat["inside"].shape
    assert np.array_equal(bits(lat["origin"]), bits(ref_lat["origin"])) and bits(lat["pitch"]) == bits(ref_lat["pitch"])
    assert np.array_equal(bits(lat["corners"].cpu().numpy()), bits(mref.corners(ref_lat["origin"], ref_lat["pitch"], ref_lat["dims"])))
    assert np.array_equal(lat["inside"].cpu().numpy(), ref_lat["inside"])
    got = meshprep.make_watertight(v, f, resolution=R)
    assert got["vertices"].dtype == F32 and got["faces"].dtype == np.int64 and got["probes"] is None
    assert_same_mesh(got, want)
    assert got["snapped"] == int(want["snapped"].sum()) and got["resolution"] == R and got["dims"] == want["dims"]
    assert bits(F32(got["pitch"])) == bits(want["pitch"]) and np.array_equal(bits(got["origin"]), bits(want["origin"]))
    assert got["topology"] == {"closed": True, "oriented": True, "boundary_edges": 0, "nonmanifold_edges": 0}
    assert got["source_topology"]["closed"] == (name in ("cube", "icosphere", "two_cubes"))
    unsnapped = meshprep.make_watertight(v, f, resolution=R, snap_limit=None)
    assert np.array_equal(bits(unsnapped["vertices"]), bits(want["lattice_vertices"])) and unsnapped["snapped"] == 0
    if name in ("cube", "icosphere"):                                        # a closed source: the parity sign gives the same lattice
        parity = ops.lattice_signs(v, f, R, sign="parity")
        assert np.array_equal(parity["inside"].cpu().numpy(), mref.lattice_signs(v, f, R, "parity")["inside"])
        assert np.array_equal(parity["inside"].cpu().numpy(), ref_lat["inside"])


def test_target_vertices_chooses_the_restatements_resolution():
    from homan_amd import meshprep
    v, f = source("cube")
    want = cube_budget(1000)
    got = meshprep.make_watertight(v, f, target_vertices=1000, snap_limit=None)
    assert got["resolution"] == want["resolution"] and got["probes"] == want["probes"]
    assert len(got["vertices"]) <= 1000
    assert np.array_equal(bits(got["vertices"]), bits(want["lattice_vertices"])) and np.array_equal(got["faces"], want["faces"])
    with pytest.raises(ValueError):
        meshprep.make_watertight(v, f, target_vertices=50)                  # R = 4 gives 98


def test_remeshed_open_bottle_serves_the_consumers_of_closed_meshes():
    from homan_amd import meshprep, ops, pointmetrics
    v, f = source("bottle_open")
    p, want, _, _ = scene()
    got = meshprep.make_watertight(v, f, resolution=SCENE_R)
    assert_same_mesh(got, want)
    assert got["topology"]["closed"] and got["topology"]["oriented"] and not got["source_topology"]["closed"]
    rv, rf = torch.from_numpy(got["vertices"]).cuda()[None], got["faces"].astype(np.int32)
    pts = torch.from_numpy(p).cuda()[None]
    src = torch.from_numpy(v.copy()).cuda()[None]
    parity = ops.point_mesh_distance(pts, rv, rf)["inside"][0].cpu().numpy()
    winding = ops.point_mesh_winding(pts, src, f)["inside"][0].cpu().numpy()
    dist = ops.point_mesh_distance(pts, src, f)["d2"][0].double().sqrt().cpu().numpy()
    far = dist > 2.0 * got["pitch"]
    print("points beyond 2h", int(far.sum()), "of", len(p), "inside among them", int(winding[far].sum()),
          "disagreeing", int((parity[far] != winding[far]).sum()))
    assert far.sum() >= 0.7 * len(p)
    assert np.array_equal(parity[far], winding[far])
    # the consumers that assume a closed mesh
    volume = ops.mesh_volume(rv, rf)
    assert torch.isfinite(volume).all() and abs(float(volume[0]) - mref.signed_volume(got["vertices"], got["faces"])) < 1e-9
    h = 0.005
    first, last = pointmetrics.index_boxes(got["vertices"].min(0), got["vertices"].max(0), h)
    boxes = np.concatenate([first, last - first + 1])[None]
    words = ops.solid_voxels(rv, rf, h, boxes)
    filled = ops.voxel_overlap(words, words)[0, 1].item() * h ** 3
    print("volume", float(volume[0]), "voxels", filled)
    assert 0.8 * float(volume[0]) < filled < 1.2 * float(volume[0])
    ctx = ops.SurfaceContactContext(1, pts.shape[1], rv.shape[1], rf, "cuda")
    A, R = ops.surface_contact_loss(pts.clone().requires_grad_(True), rv, ctx)
    assert torch.isfinite(A) and torch.isfinite(R) and float(A) > 0 and float(R) > 0


def test_simplify_mesh_writes_an_obj_and_a_pickle_that_load_back(tmp_path):
    from homan_amd import meshprep
    v, f = source("lidless")
    src, target = str(tmp_path / "raw.obj"), str(tmp_path / "out" / "raw_proc.obj")
    meshprep.save_obj(src, v, f)
    mesh = meshprep.simplify_mesh(src, target, vert_nb=300, manifold_path="unused", acvd_path="unused", tmp_folder="unused",
                                  verbose=False)
    assert len(mesh["vertices"]) <= 300 and mesh["topology"]["closed"] and mesh["topology"]["oriented"]
    gv, gf = meshprep.load_obj(target)
    assert np.array_equal(gv.astype(F32), mesh["vertices"]) and np.array_equal(gf, mesh["faces"])
    with open(str(tmp_path / "out" / "raw_proc.pkl"), "rb") as fh:
        pkl = pickle.load(fh)
    assert sorted(pkl) == ["faces", "vertices"]
    assert np.array_equal(pkl["vertices"], mesh["vertices"]) and np.array_equal(pkl["faces"], mesh["faces"])
    want = mref.make_watertight(v, f, target_vertices=300)
    assert mesh["resolution"] == want["resolution"] and np.array_equal(bits(mesh["vertices"]), bits(want["vertices"]))


def test_count_alone_gives_the_counts_of_the_whole_op():
    from homan_amd import ops
    for name in ("noise13", "empty", "scan_tile+"):
        f, origin, pitch = field(name)
        want = mref.surface_nets(f, origin, pitch)
        assert ops.surface_nets_count(f) == {"cells": want["cells"], "triangles": len(want["faces"]),
                                             "repair_passes": want["repair_passes"], "repaired_corners": want["repaired_corners"]}


def test_emit_writes_nothing_beyond_the_capacities():
    """hm_surface_nets_emit with capacities below the totals: every element below them is written as usual (a quad only if both
    its triangles fit), nothing at or beyond them is touched"""
    from homan_amd import lib
    f, origin, pitch = field("noise13")
    want = mref.surface_nets(f, origin, pitch)
    nz, ny, nx = f.shape
    h, dev = lib.lib(), torch.device("cuda")
    flags = torch.from_numpy(f.copy()).to(dev)
    words = h.hm_lattice_words(nx, ny, nz)
    packed = torch.empty(2 * words, dtype=torch.int64, device=dev)
    cell_bits = torch.empty(words, dtype=torch.int64, device=dev)
    offsets = torch.empty(4 * ny * nz, dtype=torch.int32, device=dev)
    report, totals = torch.empty(73, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
    lib.check(h.hm_lattice_repair(lib.ptr(flags), nx, ny, nz, lib.ptr(packed), lib.ptr(report), lib.stream()), "hm_lattice_repair")
    lib.check(h.hm_surface_nets_count(lib.ptr(packed), nx, ny, nz, lib.ptr(cell_bits), lib.ptr(offsets), lib.ptr(totals),
                                      lib.stream()), "hm_surface_nets_count")
    V, T = len(want["vertices"]), len(want["faces"])
    assert totals.tolist()[0] == V and 2 * sum(totals.tolist()[1:]) == T
    for cap_v, cap_t in ((V - 5, T - 3), (1, 2), (0, 0), (V, T)):
        vertices = torch.full((V, 3), -7.0, device=dev)
        tris = torch.full((T, 3), -7, dtype=torch.int32, device=dev)
        lib.check(h.hm_surface_nets_emit(lib.ptr(packed), lib.ptr(cell_bits), lib.ptr(offsets), lib.ptr(totals), nx, ny, nz,
                                         float(origin[0]), float(origin[1]), float(origin[2]), float(pitch), cap_v, cap_t,
                                         lib.ptr(vertices), lib.ptr(tris), lib.stream()), "hm_surface_nets_emit")
        gv, gt = vertices.cpu().numpy(), tris.cpu().numpy()
        whole = 2 * (cap_t // 2)
        assert np.array_equal(bits(gv[:cap_v]), bits(want["vertices"][:cap_v])) and (gv[cap_v:] == -7.0).all(), (cap_v, cap_t)
        assert np.array_equal(gt[:whole], want["faces"][:whole]) and (gt[whole:] == -7).all(), (cap_v, cap_t)
