"""CPU side of the winding-number sign (csrc/winding.hip, ops.point_mesh_winding, the sign="winding" mode of the surface metrics):
`hm_atan2` restated and compiled for the host, known answers of the NumPy restatement tests/winding_ref.py, which the GPU tests
hold the kernel to bit for bit, the restatement against an independently built float64 winding number, the host-only topology
check, and the argument checks of the wrappers and of the library that need no device.

Bars.  hm_atan2 against np.arctan2: 2^-44 rad (set by the rules; 4.5e-16 measured).  On a closed mesh w is an integer up to the
rounding of the sum, F * 2^(L-1) / (4 pi) = 7e-12 at 3000 faces, and the evaluation error: |w - rint(w)| <= 1e-9 (2.5e-13
measured).  The restatement against the independent winding number (spherical excess by l'Huilier's theorem, np.arccos /
np.arctan): not derived but measured over THIS file's inputs - the four scenes of tests.test_surfmetrics.comparison_cases(),
closed and with every seventh face removed, and the cube scene.  Largest |w - w_independent| found on the CPU: hand->box 1.7e-13,
box->hand 4.2e-12, hand->bottle 1.5e-12, bottle->hand 6.7e-11 (closed) and 1.4e-13, 3.6e-13, 1.5e-12, 2.8e-12 (open); the cube
1.3e-13.  The large figures are the independent side's: arccos loses digits on needle-thin spherical triangles.  Bar = 4 x
6.7e-11, rounded up to a power of two = 2^-31."""
import functools
import inspect
import subprocess

import numpy as np
import pytest
import torch

from tests import surfmetrics_ref as sref
from tests import volmetrics_ref as vref
from tests import winding_ref as wref
from tests.test_surfmetrics import DEGENERATE, comparison_cases, mesh, restated

F32 = np.float32
SCENES = ("hand->box", "box->hand", "hand->bottle", "bottle->hand")
INDEPENDENT_BAR = 2.0 ** -31


def open_faces(f):
    """the faces with every one whose index is a multiple of 7 removed: holes all over the mesh"""
    return np.ascontiguousarray(f[np.arange(len(f)) % 7 != 0])


@functools.lru_cache(maxsize=None)
def winding(name, opened=False):
    """the restatement on a scene, closed or opened: computed once, shared, left unchanged"""
    p, v, f = comparison_cases()[name]
    out = wref.point_mesh_winding(p, v, open_faces(f) if opened else f)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def cube_points():
    v, f = vref.cube_mesh([-0.02, -0.01, 0.0], [0.02, 0.03, 0.05])
    rng = np.random.default_rng(11)
    p = (rng.random((65, 3)) * [0.08, 0.08, 0.1] + [-0.04, -0.03, -0.025]).astype(F32)
    return p, v, f


# =============================================================================================== hm_atan2
def atan2_inputs(n=10 ** 6):
    rng = np.random.default_rng(0)
    yx = 10.0 ** rng.uniform(-18, 3, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    yx[:1000, 1] = 0.0                                                     # x = 0
    yx[1000:2000, 0] = yx[1000:2000, 1]                                    # the diagonals
    yx[2000:3000, 0] = -yx[2000:3000, 1]
    yx[3000:4000, 0] = wref.TAN_PI_8 * yx[3000:4000, 1]                    # about the fold
    return yx[:, 0].copy(), yx[:, 1].copy()


def test_hm_atan2_restated_is_within_2_to_the_minus_44_of_arctan2():
    y, x = atan2_inputs()
    assert all(((y > 0) == sy)[(x > 0) == sx].any() for sy in (0, 1) for sx in (0, 1)) and (x == 0).sum() >= 1000
    got = wref.hm_atan2(y, x)
    err = np.abs(got - np.arctan2(y, x)).max()
    print("hm_atan2: largest error", err)
    assert err <= 2.0 ** -44
    assert np.array_equal(wref.hm_atan2(-y, x), -got)                      # odd in y
    # the axes and the origin
    axes = wref.hm_atan2(np.array([0.0, 1.0, 0.0, -1.0, 0.0]), np.array([1.0, 0.0, -1.0, 0.0, 0.0]))
    assert axes.tolist() == [0.0, wref.PI_2, wref.PI, -wref.PI_2, 0.0]


def test_hm_atan2_compiled_for_the_host_is_the_restatement(tmp_path):
    """csrc/hm_common.h's function, compiled for the host with the project's contraction flag, on 200 000 pairs: the bits of the
    restatement (the device executes the same IEEE operations; the GPU tests hold the kernel's counts to them)"""
    from homan_amd import build
    (tmp_path / "host.cpp").write_text(
        '#include "hm_common.h"\n#include <cstdio>\nint main(int argc, char** argv) {\n    FILE* in = fopen(argv[1], "rb");\n'
        '    FILE* out = fopen(argv[2], "wb");\n    double yx[2];\n    if (argc != 3 || !in || !out) return 1;\n'
        '    while (fread(yx, sizeof(double), 2, in) == 2) {\n        const double r = hm_atan2(yx[0], yx[1]);\n'
        '        fwrite(&r, sizeof(double), 1, out);\n    }\n    fclose(in);\n    fclose(out);\n    return 0;\n}\n')
    r = subprocess.run([build.HIPCC, "-x", "hip", "--offload-host-only", "-O3", "-std=c++17", "-ffp-contract=off", "-I", build.CSRC,
                        "-I", build.INCLUDE, str(tmp_path / "host.cpp"), "-o", str(tmp_path / "host")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    y, x = atan2_inputs(200000)
    np.stack([y, x], 1).tofile(str(tmp_path / "yx.bin"))
    subprocess.run([str(tmp_path / "host"), str(tmp_path / "yx.bin"), str(tmp_path / "r.bin")], check=True)
    got = np.fromfile(str(tmp_path / "r.bin"))
    assert np.array_equal(got.view(np.uint64), wref.hm_atan2(y, x).view(np.uint64))


# =============================================================================================== closed and open scenes
@pytest.mark.parametrize("name", SCENES)
def test_closed_scene_equals_parity_and_w_is_an_integer(name):
    r = winding(name)
    assert np.array_equal(r["inside"], restated(name)["inside"])
    assert 20 < r["inside"].sum() < len(r["inside"]) - 20
    w = r["winding"]
    dev = np.abs(w - np.rint(w)).max()
    print(name, "largest |w - rint(w)|", dev, "rounding bound", len(comparison_cases()[name][2]) * 2.0 ** (r["log2q"] - 1) / (4 * np.pi))
    assert dev <= 1e-9
    assert set(np.rint(w).astype(int).tolist()) == {0, 1}                  # the project's meshes give +1 inside
    assert r["log2q"] == -44 and r["count"].dtype == np.int64


@pytest.mark.parametrize("name", SCENES)
def test_open_scene_winding_keeps_the_closed_flags_and_parity_does_not(name):
    p, v, f = comparison_cases()[name]
    closed = restated(name)["inside"]
    r = winding(name, True)
    parity = sref.point_mesh(p, v, open_faces(f))["inside"]
    wrong_w, wrong_p = int((r["inside"] != closed).sum()), int((parity != closed).sum())
    margin = np.abs(np.abs(r["winding"]) - 0.5).min()
    print(name, "faces left", len(open_faces(f)), "winding wrong", wrong_w, "parity wrong", wrong_p, "margin", margin)
    assert wrong_w <= 2
    assert wrong_p >= 10
    assert margin > 1e-6                                                   # no flag hangs on rounding


@pytest.mark.parametrize("name", SCENES + ("cube",))
def test_restatement_against_the_independent_winding_number(name):
    if name == "cube":
        p, v, f = cube_points()
        devs = [np.abs(wref.point_mesh_winding(p, v, f[:F])["winding"] - wref.independent_winding(p, v, f[:F])).max()
                for F in (1, 2, 12)]
    else:
        p, v, f = comparison_cases()[name]
        devs = [np.abs(winding(name)["winding"] - wref.independent_winding(p, v, f)).max(),
                np.abs(winding(name, True)["winding"] - wref.independent_winding(p, v, open_faces(f))).max()]
    print(name, "largest |w - w_independent|", devs)
    assert max(devs) <= INDEPENDENT_BAR


def test_a_mesh_wound_the_other_way_gives_the_same_flags():
    p, v, f = comparison_cases()["hand->box"]
    flipped = wref.point_mesh_winding(p, v, np.ascontiguousarray(f[:, ::-1]))
    # (c, b, a) runs the operations in another order: each angle is the negative up to its evaluation error, far below a
    # quantum, so each face's quanta differ by one at the most
    assert np.abs(flipped["count"] + winding("hand->box")["count"]).max() <= len(f)
    assert (flipped["count"] < 0).sum() > 20
    assert np.array_equal(flipped["inside"], winding("hand->box")["inside"])


# =============================================================================================== degenerate, skipped, split
@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_faces_count_for_nothing(name):
    p, v, f = comparison_cases()[name]
    r = wref.point_mesh_winding(p, v, f)
    assert not r["count"].any() and not r["inside"].any()


def test_skipped_faces_and_points():
    p, v, f = cube_points()
    want = wref.point_mesh_winding(p, v, f)
    assert 3 < want["inside"].sum() < 40
    verts = np.concatenate([v, [[np.nan, 0.01, 0.01], [0.01, np.inf, 0.01]]]).astype(F32)
    more = np.concatenate([f[:5], [[0, 1, 8]], [[0, 9, 2]], [[0, 1, 10]], [[-1, 2, 3]], f[5:], [[3, 3, 5]]]).astype(np.int32)
    got = wref.point_mesh_winding(p, verts, more)
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["inside"], want["inside"])
    points = p.copy()
    points[3, 1], points[7, 0], points[9, 2] = np.nan, np.inf, -np.inf
    bad = wref.point_mesh_winding(points, v, f)
    rows = [3, 7, 9]
    assert not bad["count"][rows].any() and not bad["inside"][rows].any()
    keep = np.setdiff1d(np.arange(len(p)), rows)
    assert np.array_equal(bad["count"][keep], want["count"][keep])
    # a point at a vertex and a point in a face's plane: every face that holds it gives exactly 0
    at_vertex = wref.solid_angles(v[None, 0], v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    assert not at_vertex[(f == 0).any(1)].any()


def test_any_split_of_the_faces_adds_up_to_the_same_count():
    p, v, f = comparison_cases()["hand->box"]
    whole = winding("hand->box")
    rng = np.random.default_rng(3)
    for cuts in ([256], [1, 2, 499], sorted(rng.choice(np.arange(1, len(f)), 7, replace=False).tolist())):
        total = np.zeros(len(p), np.int64)
        for part in np.split(np.arange(len(f)), cuts):
            total += wref.point_mesh_winding(p, v, f[part], log2q=whole["log2q"])["count"]
        assert np.array_equal(total, whole["count"]), cuts
    order = rng.permutation(len(f))
    assert np.array_equal(wref.point_mesh_winding(p, v, f[order])["count"], whole["count"])


def test_the_grid_and_the_threshold():
    from homan_amd import ops
    for F, want in ((1, -44), (2, -44), (3000, -44), (1 << 15, -44), ((1 << 15) + 1, -43), (1 << 20, -39), ((1 << 31) - 1, -28)):
        assert ops.winding_log2q(F) == want == wref.winding_log2q(F), F
        assert F * 8 * 2.0 ** -want <= 2.0 ** 62
    with pytest.raises(ValueError):
        ops.winding_log2q(0)
    assert wref.threshold(-44) == int(np.rint(2 * np.pi * 2.0 ** 44)) == 110534964875444
    # |count| > T is |w| > 0.5 up to the rounding of T itself (half a quantum)
    for L in (-47, -44, -30):
        assert abs(wref.threshold(L) * 2.0 ** L / (4 * np.pi) - 0.5) <= 2.0 ** (L - 1) / (4 * np.pi)


# =============================================================================================== topology
def test_mesh_topology_known_answers():
    from homan_amd import meshutils
    from homan_amd.mano_assets import synthetic_mano
    v, f = vref.cube_mesh([0, 0, 0], [1, 1, 1])
    assert meshutils.mesh_topology(f) == {"closed": True, "oriented": True, "boundary_edges": 0, "nonmanifold_edges": 0}
    assert meshutils.mesh_topology(torch.from_numpy(f)) == meshutils.mesh_topology(f)
    assert meshutils.mesh_topology(f[1:]) == {"closed": False, "oriented": True, "boundary_edges": 3, "nonmanifold_edges": 0}
    flipped = f.copy()
    flipped[4] = flipped[4, ::-1]
    t = meshutils.mesh_topology(flipped)
    assert t["closed"] and not t["oriented"] and t["boundary_edges"] == 0
    twice = meshutils.mesh_topology(np.concatenate([f, f[:1]]))
    assert not twice["closed"] and twice["nonmanifold_edges"] == 3 and twice["boundary_edges"] == 0
    for name in ("box", "bottle", "hand"):
        t = meshutils.mesh_topology(mesh(name)[1])
        assert t["closed"] and t["oriented"], name
        assert not meshutils.mesh_topology(open_faces(mesh(name)[1]))["closed"]
    assert not meshutils.mesh_topology(np.asarray(synthetic_mano(0)["faces"]))["closed"]      # the open hand: the wrist
    for bad in (f[:, :2], f[:0], f.astype(np.float32), f[0]):
        with pytest.raises(ValueError):
            meshutils.mesh_topology(bad)
    assert meshutils.resolve_sign("auto", f) == "parity" and meshutils.resolve_sign("auto", f[1:]) == "winding"
    assert meshutils.resolve_sign("parity", f[1:]) == "parity" and meshutils.resolve_sign("winding", f) == "winding"


# =============================================================================================== arguments
def test_wrappers_check_their_arguments_before_any_device_work():
    from homan_amd import ho3deval, ops, pointmetrics
    v, f = vref.cube_mesh([0, 0, 0], [0.04, 0.04, 0.04])
    verts = torch.from_numpy(v)[None]
    for fn in (ops.point_mesh_winding, ops.point_mesh_distance_signed):
        for bad in (verts[0], verts[:, :, :2], verts[:0], verts.int(), v):
            with pytest.raises(ValueError):
                fn(bad, verts, f)
            with pytest.raises(ValueError):
                fn(verts, bad, f)
        for bad_faces in (f[:, :2], f[:0], f.astype(np.float32), f[0]):
            with pytest.raises(ValueError):
                fn(verts, verts, bad_faces)
        with pytest.raises(ValueError):
            fn(torch.cat([verts, verts]), verts, f)
    two = torch.cat([verts, verts])
    for sign in ("Parity", "ray", "", None, 1):
        with pytest.raises(ValueError):
            ops.point_mesh_distance_signed(verts, verts, f, sign=sign)
        with pytest.raises(ValueError):
            pointmetrics.get_surface_metrics_signed(two, two, f[None], f[None], sign=sign)
        with pytest.raises(ValueError):
            pointmetrics.surface_frame_bytes(1, 8, 8, sign)
        with pytest.raises(ValueError):
            ho3deval.evaluate_sequence_surface_signed({}, 4, f, f, sign=sign)
    assert pointmetrics.surface_frame_bytes(2, 778, 1000) == pointmetrics.surface_frame_bytes(2, 778, 1000, "parity")
    for sign in ("winding", "auto"):                                       # + 12 bytes per point: the count and the flag
        assert pointmetrics.surface_frame_bytes(2, 778, 1000, sign) == pointmetrics.surface_frame_bytes(2, 778, 1000) + 2 * 1778 * 12
    with pytest.raises(ValueError):
        pointmetrics.get_surface_metrics_signed(two, two, f[None], f[None], sign="winding",
                                                max_bytes=pointmetrics.surface_frame_bytes(1, 8, 8, "winding") - 1)
    params = lambda fn: list(inspect.signature(fn).parameters)  # noqa: E731
    assert params(ops.point_mesh_winding) == ["points", "verts", "faces", "log2q"]
    assert params(ops.point_mesh_distance_signed) == params(ops.point_mesh_distance) + ["sign"]
    assert params(pointmetrics.get_surface_metrics_signed) == params(pointmetrics.get_surface_metrics) + ["sign"]
    assert params(ho3deval.evaluate_sequence_surface_signed) == params(ho3deval.evaluate_sequence_surface) + ["sign"]
    assert params(pointmetrics.surface_frame_bytes) == ["hands", "hand_verts", "obj_verts", "sign"]
    for fn in (ops.point_mesh_distance_signed, pointmetrics.get_surface_metrics_signed, ho3deval.evaluate_sequence_surface_signed,
               pointmetrics.surface_frame_bytes):
        assert inspect.signature(fn).parameters["sign"].default == "parity"
    for fn, twin in ((pointmetrics.get_surface_metrics_signed, pointmetrics.get_surface_metrics),
                     (ho3deval.evaluate_sequence_surface_signed, ho3deval.evaluate_sequence_surface)):
        shared = inspect.signature(twin).parameters
        assert all(inspect.signature(fn).parameters[k].default == shared[k].default for k in shared)
    if not torch.cuda.is_available():            # no CPU path
        with pytest.raises(RuntimeError):
            ops.point_mesh_winding(verts, verts, f)
        with pytest.raises(RuntimeError):
            pointmetrics.get_surface_metrics_signed(verts, verts, f[None], f[None], sign="winding")


def test_library_refuses_bad_arguments_without_a_launch():
    """made-up device addresses that are never dereferenced: every call here must fail its host checks before anything is enqueued
    (HM_ERR_BAD_ARG = -1)"""
    from homan_amd import lib
    h, p = lib.lib(), 1 << 20
    assert "hm_point_mesh_winding" in lib.exported_symbols()

    def call(points=p, verts=p, faces=p, B=1, N=8, V=8, F=3000, log2q=-44, count=p, inside=p):
        return h.hm_point_mesh_winding(points, verts, faces, B, N, V, F, log2q, count, inside, None)
    for kw in (dict(points=None), dict(verts=None), dict(faces=None), dict(B=0), dict(B=-1), dict(N=0), dict(N=-5), dict(V=0),
               dict(V=-1), dict(F=0), dict(F=-3), dict(count=None), dict(count=p + 4), dict(count=p + 1), dict(count=p + 12),
               dict(count=p + 4, inside=None), dict(log2q=-48), dict(log2q=-100), dict(log2q=1), dict(log2q=44),
               dict(F=(1 << 15) + 1, log2q=-44), dict(F=1 << 20, log2q=-40), dict(F=(1 << 31) - 1, log2q=-29)):
        assert call(**kw) == -1, kw
    header = open(lib._build.HEADER).read()
    assert "ALIGNMENT: count 8 bytes" in header
