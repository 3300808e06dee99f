"""Mesh preparation: from a raw object mesh (holes, missing caps, tens of thousands of faces) to the closed, oriented mesh of
about a thousand vertices that the fits, the collision grid, the voxeliser and the parity sign assume.

`simplify_mesh` has the call surface of the reference's meshprocess/simplifymesh.py, which shells out to two external
programs (ManifoldPlus for watertightness, ACVD for resampling to vert_nb vertices).  Here the stage is `make_watertight`:
the generalised winding number of the source at the corners of a lattice (`ops.lattice_signs`), a deterministic repair of the
sign field and surface nets on it (`ops.surface_nets`, csrc/remesh.hip), and a snap of the vertices onto the source surface
(`ops.point_mesh_distance`, `ops.lattice_snap`).  The rules are in include/homan_amd.h and DESIGN.md section 7.  The result is
closed and oriented by construction; it is not feature preserving (no sharp edges), decimates only through the lattice pitch,
loses components thinner than a cell, and may hold pinched vertices.

Opt-in second stage, for sources with parts thinner than a cell of the budget lattice: `make_watertight_detail` meshes at a fine
lattice and `decimate` brings the nets down to the budget by quadric edge collapses in deterministic parallel rounds
(`ops.decimate_mesh`, csrc/decimate.hip); `simplify_mesh(..., detail_resolution=R)` selects it.

Also here: a minimal reader and writer for .obj and .off files in plain Python and NumPy."""
import os
import pickle

import numpy as np

SNAP_LIMIT = float(np.float32(1.7320508))    # in cells: the cell diagonal
BUDGET_RESOLUTIONS = (4, 128)                # the bisection's range


# ---------------------------------------------------------------------------------------------- files
def _fan(poly, faces):
    for k in range(1, len(poly) - 1):
        faces.append((poly[0], poly[k], poly[k + 1]))


def load_obj(path):
    """-> (vertices (V,3) float64, faces (F,3) int64).  `v x y z [...]` and `f a b c [...]` lines; a token `a/b/c` names vertex a;
    negative indices count back from the vertices read so far; polygons are fanned from their first vertex; all else is ignored."""
    verts, faces = [], []
    with open(path) as fh:
        for line in fh:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                verts.append([float(x) for x in parts[1:4]])
            elif parts[0] == "f":
                poly = []
                for token in parts[1:]:
                    idx = int(token.split("/")[0])
                    if idx == 0:
                        raise ValueError(f"{path}: vertex index 0 in `{line.strip()}`")
                    poly.append(idx - 1 if idx > 0 else len(verts) + idx)
                if len(poly) < 3:
                    raise ValueError(f"{path}: a face of {len(poly)} vertices in `{line.strip()}`")
                _fan(poly, faces)
    return np.array(verts, np.float64).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3)


def save_obj(path, vertices, faces):
    """float32 coordinates survive the round trip: nine significant digits"""
    with open(path, "w") as fh:
        for v in np.asarray(vertices, np.float64):
            fh.write("v %.9g %.9g %.9g\n" % tuple(v))
        for f in np.asarray(faces, np.int64):
            fh.write("f %d %d %d\n" % tuple(f + 1))


def load_off(path):
    """-> (vertices (V,3) float64, faces (F,3) int64); polygons are fanned from their first vertex, comments (#) are skipped"""
    with open(path) as fh:
        tokens = []
        for line in fh:
            tokens.extend(line.split("#")[0].split())
    if not tokens or not tokens[0].startswith("OFF"):
        raise ValueError(f"{path}: not an OFF file")
    tokens[0] = tokens[0][3:]
    tokens = [t for t in tokens if t]
    nv, nf = int(tokens[0]), int(tokens[1])
    at = 3
    verts = np.array([float(t) for t in tokens[at:at + 3 * nv]], np.float64).reshape(nv, 3)
    at += 3 * nv
    faces = []
    for _ in range(nf):
        n = int(tokens[at])
        poly = [int(t) for t in tokens[at + 1:at + 1 + n]]
        if n < 3 or len(poly) != n:
            raise ValueError(f"{path}: a face of {n} vertices")
        _fan(poly, faces)
        at += 1 + n
    return verts, np.array(faces, np.int64).reshape(-1, 3)


def save_off(path, vertices, faces):
    vertices, faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    with open(path, "w") as fh:
        fh.write("OFF\n%d %d 0\n" % (len(vertices), len(faces)))
        for v in vertices:
            fh.write("%.9g %.9g %.9g\n" % tuple(v))
        for f in faces:
            fh.write("3 %d %d %d\n" % tuple(f))


def load_mesh(path):
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        return load_obj(path)
    if ext == ".off":
        return load_off(path)
    raise ValueError(f"{path}: only .obj and .off are read")


def save_mesh(path, vertices, faces):
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".obj", ".off"):
        raise ValueError(f"{path}: only .obj and .off are written")
    (save_obj if ext == ".obj" else save_off)(path, vertices, faces)


# ---------------------------------------------------------------------------------------------- the stage
def choose_resolution(count, target):
    """The budget rule: integer bisection over [4, 128] for the largest PROBED R with count(R) <= target (the count is not
    strictly monotonic in R; the probes as written here are the rule) -> (R, [(R, count), ...]).  ValueError when even R = 4
    exceeds the target."""
    lo, hi = BUDGET_RESOLUTIONS
    probes = []

    def probe(R):
        probes.append((R, int(count(R))))
        return probes[-1][1]
    if probe(lo) > target:
        raise ValueError(f"target_vertices {target}: even a resolution of {lo} gives {probes[-1][1]} vertices")
    best, a, b = lo, lo + 1, hi
    while a <= b:
        m = (a + b) // 2
        if probe(m) <= target:
            best, a = m, m + 1
        else:
            b = m - 1
    return best, probes


def _check_source(vertices, faces, resolution, target_vertices, snap_limit, sign):
    from . import ops
    if sign not in ("winding", "parity"):
        raise ValueError(f"sign {sign!r} not in [winding|parity]")
    v, f = ops._lattice_mesh(vertices, faces)
    if resolution is None:
        if isinstance(target_vertices, bool) or int(target_vertices) != target_vertices or target_vertices < 1:
            raise ValueError(f"target_vertices {target_vertices!r} is not a positive integer")
        ops.lattice_box(v, f, BUDGET_RESOLUTIONS[0])
    else:
        ops.lattice_box(v, f, resolution)
    if snap_limit is not None:
        with np.errstate(over="ignore"):
            sl = np.float32(snap_limit)
        if not (np.isfinite(sl) and sl >= 0):
            raise ValueError(f"snap_limit {snap_limit!r} is not finite and >= 0 in fp32")
    return v, f


def make_watertight(vertices, faces, resolution=None, target_vertices=1000, snap_limit=SNAP_LIMIT, sign="winding"):
    """vertices (V,3), faces (F,3) of a raw mesh -> {"vertices" (n,3) float32, "faces" (m,3) int64 (NumPy, on the host): a closed,
    oriented mesh with outward normals; "resolution", "pitch", "origin", "dims" of the lattice; "repair_passes",
    "repaired_corners"; "snapped" vertices moved onto the source; "probes" of the budget search (None with a given resolution);
    "source_topology", "topology": `meshutils.mesh_topology` of both}.
    resolution: cells along the longest extent, 2 ... 256; None = chosen by `choose_resolution` so that the vertex count is <=
    target_vertices.  snap_limit, in cells: a vertex within it of the source surface is moved onto the surface (0 or None:
    none is).  sign="winding" for sources with holes, "parity" for closed ones.  Arguments are checked before any device work;
    the work is HIP (no CPU path)."""
    import torch

    from . import meshutils, ops
    v, f = _check_source(vertices, faces, resolution, target_vertices, snap_limit, sign)
    probes = None
    if resolution is None:
        kept = {}                                    # the best probe's lattice: the bisection's answer is always its last best

        def count(R):
            probed = ops.lattice_signs(v, f, R, sign)
            n = ops.surface_nets_count(probed["inside"])["cells"]
            if n <= target_vertices:                 # (every later best is a larger R)
                kept.clear()
                kept[R] = probed
            return n
        resolution, probes = choose_resolution(count, int(target_vertices))
        lat = kept[resolution]
    else:
        lat = ops.lattice_signs(v, f, int(resolution), sign)
    nets = ops.surface_nets(lat["inside"], lat["origin"], lat["pitch"])
    out_v, snapped = nets["vertices"], 0
    if snap_limit is not None and float(np.float32(snap_limit)) > 0 and nets["cells"]:
        dev = out_v.device
        found = ops.point_mesh_distance(out_v[None], torch.from_numpy(v).to(dev)[None], f, closest=True)
        out_v, flags = ops.lattice_snap(out_v, found["closest"][0], found["d2"][0], lat["pitch"], snap_limit)
        snapped = int(flags.sum())
    out_f = nets["faces"].cpu().numpy().astype(np.int64)
    return {"vertices": out_v.cpu().numpy(), "faces": out_f, "resolution": int(resolution), "pitch": float(lat["pitch"]),
            "origin": lat["origin"].copy(), "dims": lat["dims"], "repair_passes": nets["repair_passes"],
            "repaired_corners": nets["repaired_corners"], "snapped": snapped, "probes": probes,
            "source_topology": meshutils.mesh_topology(f), "topology": meshutils.mesh_topology(out_f) if len(out_f) else None}


def _check_decimation(target_vertices, regularity, max_rounds):
    from . import ops
    return ops._decimate_numbers(target_vertices, regularity, max_rounds)


def decimate(vertices, faces, target_vertices=1000, regularity=0.01, max_rounds=4096):
    """A closed, oriented mesh brought down to target_vertices by quadric edge collapses in deterministic parallel rounds
    (`ops.decimate_mesh`, csrc/decimate.hip; the rules in include/homan_amd.h and DESIGN.md section 7) -> {"vertices" (n,3)
    float32, "faces" (m,3) int64 (NumPy, on the host), "rounds", "reached" (n <= target_vertices; False when the rounds got stuck
    or ran out), "collapses" per round, "topology"}.  The input must be closed and oriented, no face may repeat a vertex, indices
    in range, coordinates finite: checked on the host before any device work (`ops.closed_mesh`, ValueError); vertices that no
    face names are dropped there, the others keep their order.
    regularity >= 0 weighs the cube of the squared edge length against the quadric error: in flat regions it sends the shortest
    edge first.  The work is HIP (no CPU path)."""
    from . import meshutils, ops
    target_vertices, regularity, max_rounds = _check_decimation(target_vertices, regularity, max_rounds)
    out = ops.decimate_mesh(vertices, faces, target_vertices, regularity, max_rounds)
    out_f = out["faces"].cpu().numpy().astype(np.int64)
    return {"vertices": out["vertices"].cpu().numpy(), "faces": out_f, "rounds": out["rounds"], "reached": out["reached"],
            "collapses": out["collapses"], "topology": meshutils.mesh_topology(out_f)}


def make_watertight_detail(vertices, faces, detail_resolution, target_vertices=1000, snap_limit=SNAP_LIMIT, sign="winding",
                           regularity=0.01, max_rounds=4096):
    """The two-stage preparation: `make_watertight` at the FINE lattice detail_resolution (2 ... 256, no budget search), its snap,
    then `decimate` down to target_vertices -> `make_watertight`'s dict ("probes" is None; "vertices", "faces", "topology" are
    the decimated mesh's) with "detail_vertices" (the nets' vertex count), "rounds", "reached" and "collapses" added.  Nets that
    already meet the budget come back unchanged with rounds = 0.  Where the budget lattice loses parts thinner than its cell (a
    mug's wall and handle), the fine lattice keeps them and the collapses keep the topology.  Arguments are checked before any
    device work; the work is HIP (no CPU path)."""
    from . import meshutils, ops
    target_vertices, regularity, max_rounds = _check_decimation(target_vertices, regularity, max_rounds)
    if detail_resolution is None or isinstance(detail_resolution, bool):
        raise ValueError(f"detail_resolution {detail_resolution!r} is not an integer in [{ops.LATTICE_RESOLUTIONS[0]}, "
                         f"{ops.LATTICE_RESOLUTIONS[1]}]")
    out = make_watertight(vertices, faces, resolution=detail_resolution, snap_limit=snap_limit, sign=sign)
    out.update(detail_vertices=len(out["vertices"]), rounds=0, reached=len(out["vertices"]) <= target_vertices, collapses=[])
    if not out["reached"]:
        small = ops.decimate_mesh(out["vertices"], out["faces"], target_vertices, regularity, max_rounds)
        out_f = small["faces"].cpu().numpy().astype(np.int64)
        out.update(vertices=small["vertices"].cpu().numpy(), faces=out_f, rounds=small["rounds"], reached=small["reached"],
                   collapses=small["collapses"], topology=meshutils.mesh_topology(out_f))
    return out


def simplify_mesh(src_path, target_path, vert_nb=1000, save_pkl=True, **ignored):
    """The reference's meshprocess/simplifymesh.py simplify_mesh: reads src_path (.obj / .off), writes target_path (.obj / .off)
    with at most vert_nb vertices, watertight, and with save_pkl the pickle {"vertices", "faces"} next to it (the target's name
    with its extension replaced by .pkl) -> `make_watertight`'s dict.  manifold_path, acvd_path, tmp_folder and the like are accepted
    and unused: no external program runs.  The one keyword that is read: detail_resolution (default None = the budget lattice);
    an integer selects `make_watertight_detail`, the fine lattice followed by the edge-collapse decimation."""
    detail_resolution = ignored.get("detail_resolution")
    vertices, faces = load_mesh(src_path)
    if os.path.splitext(target_path)[1].lower() not in (".obj", ".off"):
        raise ValueError(f"{target_path}: only .obj and .off are written")
    if detail_resolution is None:
        mesh = make_watertight(vertices, faces, target_vertices=vert_nb)
    else:
        mesh = make_watertight_detail(vertices, faces, detail_resolution, target_vertices=vert_nb)
    folder = os.path.dirname(os.path.abspath(target_path))
    os.makedirs(folder, exist_ok=True)
    save_mesh(target_path, mesh["vertices"], mesh["faces"])
    if save_pkl:
        with open(os.path.splitext(target_path)[0] + ".pkl", "wb") as fh:
            pickle.dump({"vertices": mesh["vertices"], "faces": mesh["faces"]}, fh)
    return mesh
