"""GPU side of the edge-collapse decimation: csrc/decimate.hip behind ops.collapse_round / ops.decimate_mesh, meshprep.decimate,
make_watertight_detail and simplify_mesh(detail_resolution=...) against the NumPy restatement tests/decimate_ref.py, bit for bit:
integers equal, doubles and floats compared through their bit patterns."""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from tests import decimate_ref as dref
from tests import meshprep_ref as mref
from tests.test_decimate import CASES, assert_sound, decimated, shape
from tests.test_meshprep import source

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = tuple(dict.fromkeys(name for name, *_ in CASES))
RUNS = tuple((name, target) for name, target, *_ in CASES) + (("slab40", 300), ("mug32", 400))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def host(t):
    return t.cpu().numpy()


def assert_round_equal(got, want):
    assert np.array_equal(host(got["edges"]), want["edges"])
    assert np.array_equal(host(got["choice"]), want["choice"])
    assert np.array_equal(bits(host(got["cost"])), bits(want["cost"])) and np.array_equal(bits(host(got["l2"])), bits(want["l2"]))
    assert np.array_equal(host(got["valid"]) != 0, want["valid"])
    assert np.array_equal(host(got["rank"]), want["rank"])
    assert np.array_equal(host(got["selected"]) != 0, want["selected"])
    assert got["collapses"] == want["collapses"]
    assert got["vertices"].dtype == torch.float32 and got["faces"].dtype == torch.int32
    assert np.array_equal(bits(host(got["vertices"])), bits(want["vertices"]))
    assert np.array_equal(host(got["faces"]), want["faces"])


@functools.lru_cache(maxsize=None)
def mid_run(name):
    """the restatement's state half way through its longest run on a shape: (V, F, target)"""
    target = min(t for n, t, *_ in CASES if n == name)
    V, F = shape(name)
    for _ in range(decimated(name, target)["rounds"] // 2):
        r = dref.collapse_round(V, F, len(V) - target)
        V, F = r["vertices"], r["faces"]
    return V, F, target


@pytest.mark.parametrize("name", SHAPES)
def test_collapse_round_equals_the_restatement_bit_for_bit(name):
    from homan_amd import ops
    V, F = shape(name)
    target = min(t for n, t, *_ in CASES if n == name)
    for v, f in ((V, F), mid_run(name)[:2]):
        need = len(v) - target
        want = dref.collapse_round(v, f, need)
        got = ops.collapse_round(torch.from_numpy(v.copy()).cuda(), f, need)
        print(name, len(v), "edges", len(want["edges"]), "valid", int(want["valid"].sum()), "collapses", want["collapses"])
        assert_round_equal(got, want)
    few = ops.collapse_round(V, F, 1)                                       # the budget: only the lowest rank goes
    assert_round_equal(few, dref.collapse_round(V, F, 1))
    other = ops.collapse_round(V, F, 1, regularity=0.0)
    assert_round_equal(other, dref.collapse_round(V, F, 1, regularity=0.0))


@pytest.mark.parametrize("name,target", RUNS)
def test_decimate_mesh_equals_the_restatement_bit_for_bit(name, target):
    from homan_amd import meshprep, ops
    V, F = shape(name)
    want = decimated(name, target)
    got = ops.decimate_mesh(V, F, target)
    again = ops.decimate_mesh(torch.from_numpy(V.copy()).cuda(), torch.from_numpy(F.copy()).cuda(), target)
    for out in (got, again):
        assert (out["rounds"], out["reached"], out["collapses"]) == (want["rounds"], want["reached"], want["collapses"])
        assert np.array_equal(bits(host(out["vertices"])), bits(want["vertices"]))
        assert np.array_equal(host(out["faces"]), want["faces"]) and out["faces"].dtype == torch.int32
    if name == "icosphere2":                                                # the public entry, and the round limit
        pub = meshprep.decimate(V, F, target_vertices=target)
        assert pub["vertices"].dtype == F32 and pub["faces"].dtype == np.int64 and pub["topology"]["closed"]
        assert np.array_equal(bits(pub["vertices"]), bits(want["vertices"])) and np.array_equal(pub["faces"], want["faces"])
        assert (pub["rounds"], pub["reached"], pub["collapses"]) == (want["rounds"], want["reached"], want["collapses"])
        cut = meshprep.decimate(V, F, target_vertices=target, max_rounds=2)
        ref = dref.decimate(V, F, target, max_rounds=2)
        assert cut["rounds"] == 2 and not cut["reached"] and np.array_equal(bits(cut["vertices"]), bits(ref["vertices"]))
        same = meshprep.decimate(V, F, target_vertices=len(V))              # within the budget: unchanged
        assert same["rounds"] == 0 and same["reached"] and np.array_equal(same["vertices"], V) and np.array_equal(same["faces"], F)


def test_thin_slab_survives_where_the_budget_lattice_returns_nothing():
    from homan_amd import ops
    field, origin, pitch = dref.box_field(40, dref.slab)
    nets = ops.surface_nets(field, origin, pitch)
    out = ops.decimate_mesh(nets["vertices"], nets["faces"], 300)
    V, F = host(out["vertices"]), host(out["faces"]).astype(np.int64)
    nv, nf = host(nets["vertices"]), host(nets["faces"]).astype(np.int64)
    v0, v1 = mref.signed_volume(nv, nf), mref.signed_volume(V, F)
    print("slab:", len(nv), "->", len(V), "rounds", out["rounds"], "volume", v0, "->", v1, "relative", abs(v1 - v0) / v0)
    assert out["reached"] and len(V) == 300
    assert_sound(V, F, dref.euler(nv, nf))
    assert abs(v1 - v0) <= 0.02 * v0
    R, _ = mref.choose_resolution(lambda R: ops.surface_nets_count(dref.box_field(R, dref.slab)[0])["cells"], 300)
    assert ops.surface_nets_count(dref.box_field(R, dref.slab)[0])["cells"] == 0       # the old path: an empty mesh


def test_mug_keeps_its_handle_where_the_budget_lattice_fills_it():
    from homan_amd import ops
    field, origin, pitch = dref.box_field(32, dref.mug)
    nets = ops.surface_nets(field, origin, pitch)
    out = ops.decimate_mesh(nets["vertices"], nets["faces"], 400)
    V, F = host(out["vertices"]), host(out["faces"]).astype(np.int64)
    assert dref.euler(host(nets["vertices"]), host(nets["faces"])) == 0
    assert out["reached"] and len(V) == 400
    assert_sound(V, F, 0)
    R, _ = mref.choose_resolution(lambda R: ops.surface_nets_count(dref.box_field(R, dref.mug)[0])["cells"], 400)
    coarse = ops.surface_nets(*dref.box_field(R, dref.mug))
    print("mug: budget resolution", R, "vertices", coarse["cells"], "; 32 cells:", nets["cells"], "->", len(V), "rounds", out["rounds"])
    assert dref.euler(host(coarse["vertices"]), host(coarse["faces"])) == 2


def test_make_watertight_detail_from_the_mug_as_a_mesh():
    """End to end from the mug's 48-cell nets as a source mesh.  The restatement's second stage (tests/decimate_ref.py) runs on
    the first stage's device output, which test_meshprep_gpu.py holds to the restatement of the first stage: the NumPy sign and
    closest-point searches over 22 000 faces would take minutes."""
    from homan_amd import meshprep
    V, F = shape("mug48")
    assert dref.euler(V, F) == 0
    got = meshprep.make_watertight_detail(V, F, 32, target_vertices=400)
    first = meshprep.make_watertight(V, F, resolution=32)
    want = dref.finish_watertight(first["vertices"], first["faces"], first["vertices"], 400)
    print("mug as a mesh:", got["detail_vertices"], "->", len(got["vertices"]), "rounds", got["rounds"], "reached", got["reached"])
    assert got["detail_vertices"] == len(first["vertices"]) > 400 and got["probes"] is None and got["resolution"] == 32
    assert got["reached"] and len(got["vertices"]) == 400
    assert_sound(got["vertices"], got["faces"], 0)
    assert got["topology"]["closed"] and got["topology"]["oriented"] and got["faces"].dtype == np.int64
    assert np.array_equal(bits(got["vertices"]), bits(want["vertices"])) and np.array_equal(got["faces"], want["faces"])
    assert (got["rounds"], got["collapses"]) == (want["rounds"], want["collapses"])
    for key in ("pitch", "dims", "repair_passes", "repaired_corners", "snapped"):
        assert got[key] == first[key]
    small = meshprep.make_watertight_detail(V, F, 8, target_vertices=5000)  # nets within the budget: unchanged
    plain = meshprep.make_watertight(V, F, resolution=8)
    assert small["rounds"] == 0 and small["reached"] and small["detail_vertices"] == len(plain["vertices"])
    assert np.array_equal(bits(small["vertices"]), bits(plain["vertices"])) and np.array_equal(small["faces"], plain["faces"])


def test_default_call_on_the_mug_equals_the_parent_commits_output_bit_for_bit():
    """tests/golden/meshprep_mug48_default.npz is make_watertight(mug's 48-cell nets, target_vertices=400) as the commit BEFORE the
    decimation computed it on the device (the package of that commit, built on its own, same inputs).  The default path must still
    return those bits, that dict and nothing more: it bisects to a coarse lattice on which the mug's topology is lost."""
    from homan_amd import meshprep
    V, F = shape("mug48")
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "meshprep_mug48_default.npz")) as rec:
        want = {k: rec[k] for k in rec.files}
    got = meshprep.make_watertight(V, F, target_vertices=400)
    assert sorted(got) == want["keys"].tolist() == sorted(
        ["vertices", "faces", "resolution", "pitch", "origin", "dims", "repair_passes", "repaired_corners", "snapped", "probes",
         "source_topology", "topology"])
    assert got["vertices"].dtype == F32 and got["faces"].dtype == np.int64 == want["faces"].dtype
    assert np.array_equal(bits(got["vertices"]), bits(want["vertices"])) and np.array_equal(got["faces"], want["faces"])
    assert got["resolution"] == int(want["resolution"]) and [list(p) for p in got["probes"]] == want["probes"].tolist()
    assert np.array_equal(bits(got["origin"]), bits(want["origin"])) and bits(F32(got["pitch"])) == bits(want["pitch"])
    assert list(got["dims"]) == want["dims"].tolist() and got["snapped"] == int(want["snapped"])
    assert (got["repair_passes"], got["repaired_corners"]) == (int(want["repair_passes"]), int(want["repaired_corners"]))
    print("mug, default path: resolution", got["resolution"], "vertices", len(got["vertices"]), "euler",
          dref.euler(got["vertices"], got["faces"]))
    # the parent's own result: 400 vertices at 10 cells with Euler characteristic 12, i.e. several closed pieces where the source is
    # one surface with one handle (0) - on the analytic field the budget path gives 2 (test_mug_keeps_its_handle...), on the 0.04
    # wall as a MESH at 10 cells the winding sign breaks the wall up
    assert len(got["vertices"]) == 400 and dref.euler(got["vertices"], got["faces"]) == dref.euler(want["vertices"], want["faces"]) == 12


@pytest.mark.parametrize("name,R,target", (("cube", 7, 60), ("lidless", 7, 60), ("icosphere", 6, 40), ("cube", 4, 500)))
def test_make_watertight_detail_equals_the_restatements_two_stages(name, R, target):
    """both stages on the CPU (NumPy sign search, nets, snap, decimation) against the product, on sources small enough for that"""
    from homan_amd import meshprep
    v, f = source(name)
    want = dref.make_watertight_detail(v, f, R, target_vertices=target)
    got = meshprep.make_watertight_detail(v, f, R, target_vertices=target)
    print(name, R, want["detail_vertices"], "->", len(want["vertices"]), "rounds", want["rounds"])
    assert (got["detail_vertices"], got["rounds"], got["reached"], got["collapses"]) == (
        want["detail_vertices"], want["rounds"], want["reached"], want["collapses"])
    assert np.array_equal(bits(got["vertices"]), bits(want["vertices"])) and np.array_equal(got["faces"], want["faces"])
    assert (want["rounds"] == 0) == (want["detail_vertices"] <= target)


def test_vertices_that_no_face_names_are_dropped_before_the_rounds():
    from homan_amd import meshprep
    V, F = shape("icosphere1")
    stray = np.array([[7.0, 7.0, 7.0]], F32)
    more, renamed = np.concatenate([V[:5], stray, V[5:], stray]), np.where(F >= 5, F + 1, F)
    want, got = decimated("icosphere1", 12), meshprep.decimate(more, renamed, target_vertices=12)
    assert np.array_equal(bits(got["vertices"]), bits(want["vertices"])) and np.array_equal(got["faces"], want["faces"])
    same = meshprep.decimate(more, renamed, target_vertices=len(V))
    assert same["rounds"] == 0 and np.array_equal(same["vertices"], V) and np.array_equal(same["faces"], F)


def test_decimated_bottle_serves_the_consumers_of_closed_meshes():
    from homan_amd import meshprep, ops
    v, f = source("bottle_open")
    got = meshprep.make_watertight_detail(v, f, 24, target_vertices=300)
    assert got["reached"] and len(got["vertices"]) == 300 and got["detail_vertices"] > 300
    assert got["topology"]["closed"] and got["topology"]["oriented"] and not got["source_topology"]["closed"]
    rv, rf = torch.from_numpy(got["vertices"]).cuda()[None], got["faces"].astype(np.int32)
    volume = float(ops.mesh_volume(rv, rf)[0])
    print("bottle:", got["detail_vertices"], "-> 300 in", got["rounds"], "rounds; volume", volume)
    assert volume > 0 and abs(volume - mref.signed_volume(got["vertices"], got["faces"])) < 1e-9
    lo, hi = got["vertices"].min(0), got["vertices"].max(0)
    centre = got["vertices"].mean(0)
    pts = np.stack([centre, hi + (hi - lo), lo - (hi - lo)]).astype(F32)
    inside = ops.point_mesh_distance(torch.from_numpy(pts).cuda()[None], rv, rf)["inside"][0].cpu().numpy()
    assert inside.tolist() == [1, 0, 0]


def test_simplify_mesh_with_a_detail_resolution_writes_an_obj_and_a_pickle_that_load_back(tmp_path):
    from homan_amd import meshprep
    v, f = source("lidless")
    src, target = str(tmp_path / "raw.obj"), str(tmp_path / "out" / "raw_proc.obj")
    meshprep.save_obj(src, v, f)
    mesh = meshprep.simplify_mesh(src, target, vert_nb=100, detail_resolution=16, manifold_path="unused")
    assert len(mesh["vertices"]) == 100 and mesh["reached"] and mesh["topology"]["closed"] and mesh["topology"]["oriented"]
    assert mesh["detail_vertices"] > 100 and mesh["rounds"] >= 1
    gv, gf = meshprep.load_obj(target)
    assert np.array_equal(gv.astype(F32), mesh["vertices"]) and np.array_equal(gf, mesh["faces"])
    with open(str(tmp_path / "out" / "raw_proc.pkl"), "rb") as fh:
        pkl = pickle.load(fh)
    assert sorted(pkl) == ["faces", "vertices"]
    assert np.array_equal(pkl["vertices"], mesh["vertices"]) and np.array_equal(pkl["faces"], mesh["faces"])
    default = meshprep.simplify_mesh(src, target, vert_nb=100)              # without the argument: the budget lattice, as before
    want = mref.make_watertight(v, f, target_vertices=100)
    assert "rounds" not in default and default["resolution"] == want["resolution"]
    assert np.array_equal(bits(default["vertices"]), bits(want["vertices"])) and np.array_equal(default["faces"], want["faces"])


def test_compact_writes_nothing_beyond_the_capacities():
    """hm_decimate_compact with capacities below the survivors' counts: every element below them is written as usual, nothing at
    or beyond them is touched"""
    from homan_amd import lib, ops
    V, F = shape("icosphere2")
    want = dref.collapse_round(V, F, 1000)
    n, m, dev = len(V), len(F), torch.device("cuda")
    work = ops._Decimator(n, m, dev)
    work.verts[0].copy_(torch.from_numpy(V.copy()))
    work.faces[0].copy_(torch.from_numpy(F.astype(np.int32)))
    new_n, new_m, mid = work.round(work.verts[0], work.faces[0], n, m, 1000, 0.01, work.verts[1], work.faces[1])
    assert (new_n, new_m) == (len(want["vertices"]), len(want["faces"]))
    remap, vkeep, moved, vscan, fkeep, fscan = (mid[k] for k in ("remap", "vertex_keep", "moved", "vertex_scan", "face_keep",
                                                                 "face_scan"))
    assert int(vscan[-1]) == new_n and int(fscan[-1]) == new_m == m - 2 * want["collapses"]     # two faces go with every collapse
    for cap_v, cap_f in ((new_n - 5, new_m - 3), (1, 2), (0, 0), (new_n, new_m), (n, m)):
        out_v = torch.full((n, 3), -7.0, device=dev)
        out_f = torch.full((m, 3), -7, dtype=torch.int32, device=dev)
        lib.check(lib.lib().hm_decimate_compact(lib.ptr(work.verts[0]), lib.ptr(work.faces[0]), lib.ptr(mid["edges"]),
                                                lib.ptr(mid["choice"]), lib.ptr(remap), lib.ptr(moved), lib.ptr(vkeep),
                                                lib.ptr(vscan), lib.ptr(fkeep), lib.ptr(fscan), n, m, cap_v, cap_f,
                                                lib.ptr(out_v), lib.ptr(out_f), lib.stream()), "hm_decimate_compact")
        gv, gf = out_v.cpu().numpy(), out_f.cpu().numpy()
        cv, cf = min(cap_v, new_n), min(cap_f, new_m)
        assert np.array_equal(bits(gv[:cv]), bits(want["vertices"][:cv])) and (gv[cv:] == -7.0).all(), (cap_v, cap_f)
        assert np.array_equal(gf[:cf], want["faces"][:cf]) and (gf[cf:] == -7).all(), (cap_v, cap_f)
