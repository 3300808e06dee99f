"""NumPy restatement of the mesh preparation of csrc/remesh.hip, ops.lattice_signs / ops.surface_nets and homan_amd/meshprep.py
make_watertight; not product code, no device.  The rules are those of include/homan_amd.h / DESIGN.md section 7:

  lattice    lo, hi = the fp32 box of the vertices named by a face the search does not skip; h = max(hi - lo) / (float)R;
             origin = lo - 1.381966f * h; n = (int)floorf((hi - lo) / h) + 5 corners per axis; corner = origin + (float)index * h;
  signs      the winding number's |w| > 0.5 (tests/winding_ref.py) or the search's parity (tests/surfmetrics_ref.py); the outermost
             corner layer is forced outside;
  repair     Jacobi passes: all four corners of every unit face whose corners are a checkerboard are set, until nothing changes;
  vertices   one per cell whose 8 corners differ, ranked in row-major order, at origin + ((float)S / (float)n) * (0.5f * h) with S
             the integer sum of the midpoints of its sign-changing edges in half cells and n their count;
  faces      one quad per sign-changing lattice edge: x-edges, y-edges, z-edges, each in row-major order of the base corner p; the
             cells p + (-1,-1), (0,-1), (0,0), (-1,0) along the axes ((a+1)%3, (a+2)%3), reversed when p is outside; two triangles
             (q0, q1, q2), (q0, q2, q3);
  snap       the search's closest point iff d2 <= (snap_limit * snap_limit) * (h * h) in fp32, else the lattice position;
  budget     integer bisection over [4, 128] for the largest probed R whose vertex count is <= the target.
Arrays are indexed (k, j, i) so that C order is the rules' row-major order, i fastest.  Nothing here is tuned to the kernels' output."""
import numpy as np

from tests import surfmetrics_ref as sref
from tests import winding_ref as wref

F32 = np.float32
OFFSET = F32(1.381966)
SNAP_LIMIT = F32(1.7320508)
MAX_PASSES = 64
R_MIN, R_MAX = 2, 256
BUDGET_LO, BUDGET_HI = 4, 128


# ---------------------------------------------------------------------------------------------- lattice and signs
def lattice(verts, faces, resolution):
    """-> {"origin" (3,) fp32, "pitch" fp32, "dims" (nx, ny, nz) corners, "lo", "hi"}"""
    verts = np.ascontiguousarray(verts, F32)
    faces = np.asarray(faces).astype(np.int64)
    R = int(resolution)
    if not R_MIN <= R <= R_MAX:
        raise ValueError(f"resolution {resolution}")
    used = np.unique(faces[sref.valid_faces(verts, faces)])
    if not len(used):
        raise ValueError("no valid face")
    lo, hi = verts[used].min(0), verts[used].max(0)
    ext = hi - lo
    h = F32(ext.max()) / F32(R)
    if not (np.isfinite(h) and h > 0):
        raise ValueError("degenerate bounding box")
    origin = lo - OFFSET * h
    dims = tuple(int(n) + 5 for n in np.floor(ext / h))
    assert origin.dtype == F32 and h.dtype == F32
    return {"origin": origin, "pitch": h, "dims": dims, "lo": lo, "hi": hi}


def corners(origin, pitch, dims):
    """-> (nz * ny * nx, 3) fp32, corner (i, j, k) at row (k * ny + j) * nx + i"""
    nx, ny, nz = dims
    origin, h = np.asarray(origin, F32), F32(pitch)
    axes = [origin[a] + np.arange(n).astype(F32) * h for a, n in enumerate((nx, ny, nz))]
    out = np.empty((nz, ny, nx, 3), F32)
    out[..., 0], out[..., 1], out[..., 2] = axes[0][None, None, :], axes[1][None, :, None], axes[2][:, None, None]
    return out.reshape(-1, 3)


def lattice_signs(verts, faces, resolution, sign="winding", block=4096):
    """-> the lattice and "inside" (nz, ny, nx) int32: the flags as the sign search returns them (the outer layer not yet cleared)"""
    lat = lattice(verts, faces, resolution)
    pts = corners(lat["origin"], lat["pitch"], lat["dims"])
    if sign == "winding":
        flags = wref.point_mesh_winding(pts, verts, faces, block=block)["inside"]
    elif sign == "parity":
        flags = sref.point_mesh(pts, verts, faces)["inside"]
    else:
        raise ValueError(sign)
    nx, ny, nz = lat["dims"]
    lat["inside"] = flags.reshape(nz, ny, nx).astype(np.int32)
    return lat


def clear_outer(inside):
    s = np.asarray(inside) != 0
    assert s.ndim == 3 and min(s.shape) >= 2
    s = s.copy()
    s[0], s[-1], s[:, 0], s[:, -1], s[:, :, 0], s[:, :, -1] = False, False, False, False, False, False
    return s


def repair(s):
    """bool (nz, ny, nx) with a clear outer layer -> (the repaired field, passes that changed something, corners set)"""
    s = s.copy()
    passes = corners_set = 0
    for p in range(MAX_PASSES + 1):
        marks = np.zeros_like(s)
        for ax0, ax1 in ((1, 2), (0, 2), (0, 1)):                           # the two axes that span the face
            def part(d0, d1):
                idx = [slice(None)] * 3
                idx[ax0] = slice(d0, s.shape[ax0] - 1 + d0)
                idx[ax1] = slice(d1, s.shape[ax1] - 1 + d1)
                return tuple(idx)
            s00, s10, s01, s11 = s[part(0, 0)], s[part(1, 0)], s[part(0, 1)], s[part(1, 1)]
            checker = (s00 == s11) & (s10 == s01) & (s00 != s10)
            for d0 in (0, 1):
                for d1 in (0, 1):
                    marks[part(d0, d1)] |= checker
        new = s | marks
        changed = int((new & ~s).sum())
        if changed == 0:
            return s, passes, corners_set
        if p == MAX_PASSES:
            break
        s, passes, corners_set = new, passes + 1, corners_set + changed
    raise RuntimeError("the repair did not settle in 64 passes")


# ---------------------------------------------------------------------------------------------- surface nets
def surface_nets(inside, origin, pitch):
    """inside (nz, ny, nx) -> {"vertices" (V,3) fp32, "faces" (T,3) int32, "repair_passes", "repaired_corners", "cells", "field"}"""
    origin, h = np.asarray(origin, F32), F32(pitch)
    s, passes, corners_set = repair(clear_outer(inside))
    nz, ny, nx = s.shape
    cz, cy, cx = nz - 1, ny - 1, nx - 1

    def corner(dx, dy, dz):
        return s[dz:cz + dz, dy:cy + dy, dx:cx + dx]
    eight = np.stack([corner(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)])
    active = eight.any(0) & ~eight.all(0)
    count = int(active.sum())
    index = np.full(active.shape, -1, np.int64)
    index[active] = np.arange(count)
    K, J, I = np.indices(active.shape)
    S = np.zeros((3,) + active.shape, np.int64)
    n = np.zeros(active.shape, np.int64)
    for u in (0, 1):
        for v in (0, 1):
            e = corner(0, u, v) != corner(1, u, v)
            S[0] += e * (2 * I + 1); S[1] += e * (2 * (J + u)); S[2] += e * (2 * (K + v)); n += e
            e = corner(u, 0, v) != corner(u, 1, v)
            S[0] += e * (2 * (I + u)); S[1] += e * (2 * J + 1); S[2] += e * (2 * (K + v)); n += e
            e = corner(u, v, 0) != corner(u, v, 1)
            S[0] += e * (2 * (I + u)); S[1] += e * (2 * (J + v)); S[2] += e * (2 * K + 1); n += e
    half = F32(0.5) * h
    fn = n[active].astype(F32)
    vertices = np.stack([origin[a] + (S[a][active].astype(F32) / fn) * half for a in range(3)], 1).astype(F32)
    assert vertices.dtype == F32
    quads = []
    for a in range(3):
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        hi[2 - a], lo[2 - a] = slice(1, None), slice(None, -1)             # (array axis 2 is x)
        k, j, i = np.nonzero(s[tuple(lo)] != s[tuple(hi)])                  # base corners in row-major order
        base = np.stack([i, j, k], 1)
        cells = []
        for du, dv in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            c = base.copy()
            c[:, (a + 1) % 3] += du
            c[:, (a + 2) % 3] += dv
            assert (c >= 0).all() and (c < [cx, cy, cz]).all()
            cells.append(index[c[:, 2], c[:, 1], c[:, 0]])
        q = np.stack(cells, 1)
        assert (q >= 0).all()
        quads.append(np.where(s[k, j, i][:, None], q, q[:, ::-1]))
    q = np.concatenate(quads)
    faces = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    return {"vertices": vertices, "faces": faces, "repair_passes": passes, "repaired_corners": corners_set, "cells": count,
            "field": s}


def count_vertices(inside):
    return surface_nets(inside, np.zeros(3, F32), F32(1.0))["cells"]


def snap(lattice_vertices, verts, faces, pitch, snap_limit=SNAP_LIMIT):
    """-> (vertices (V,3) fp32, snapped (V,) bool, d2 (V,) fp32 of the lattice positions)"""
    if not len(lattice_vertices):
        return lattice_vertices.copy(), np.zeros(0, bool), np.zeros(0, F32)
    h, sl = F32(pitch), F32(snap_limit)
    found = sref.point_mesh(lattice_vertices, verts, faces)
    take = found["d2"] <= (sl * sl) * (h * h)
    return np.where(take[:, None], found["closest"], lattice_vertices).astype(F32), take, found["d2"]


# ---------------------------------------------------------------------------------------------- budget and the whole stage
def choose_resolution(count, target):
    """count(R) -> vertices after repair.  -> (R, [(R probed, count), ...]) by the written-down bisection"""
    probes = []

    def probe(R):
        probes.append((R, int(count(R))))
        return probes[-1][1]
    if probe(BUDGET_LO) > target:
        raise ValueError(f"target_vertices {target}: even R = {BUDGET_LO} gives {probes[-1][1]}")
    best, a, b = BUDGET_LO, BUDGET_LO + 1, BUDGET_HI
    while a <= b:
        m = (a + b) // 2
        if probe(m) <= target:
            best, a = m, m + 1
        else:
            b = m - 1
    return best, probes


def make_watertight(verts, faces, resolution=None, target_vertices=1000, snap_limit=SNAP_LIMIT, sign="winding"):
    verts = np.ascontiguousarray(verts, F32)
    cache = {}

    def signs(R):
        if R not in cache:
            cache[R] = lattice_signs(verts, faces, R, sign)
        return cache[R]
    probes = None
    if resolution is None:
        resolution, probes = choose_resolution(lambda R: count_vertices(signs(R)["inside"]), target_vertices)
    lat = signs(int(resolution))
    nets = surface_nets(lat["inside"], lat["origin"], lat["pitch"])
    out = {"lattice_vertices": nets["vertices"], "faces": nets["faces"].astype(np.int64), "resolution": int(resolution),
           "pitch": lat["pitch"], "origin": lat["origin"], "dims": lat["dims"], "repair_passes": nets["repair_passes"],
           "repaired_corners": nets["repaired_corners"], "probes": probes}
    if snap_limit is not None and snap_limit > 0:
        out["vertices"], out["snapped"], out["d2"] = snap(nets["vertices"], verts, faces, lat["pitch"], snap_limit)
    else:
        out["vertices"], out["snapped"] = nets["vertices"], np.zeros(len(nets["vertices"]), bool)
    return out


# ---------------------------------------------------------------------------------------------- helpers of the tests
def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def icosphere(subdivisions=2, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """an icosahedron subdivided `subdivisions` times (2 -> 162 vertices, 320 faces), outward normals"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius + np.asarray(centre)).astype(F32), np.array(f, np.int32)
