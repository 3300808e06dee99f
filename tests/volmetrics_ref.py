"""NumPy restatement of the solid voxeliser, the overlap counts and the mesh volume of csrc/solidvox.hip (not product code, no
device).  The definitions are those of include/homan_amd.h / DESIGN.md section 7:

  lattice   centre(i) = (float32(i) + 0.5f) * h, h rounded to fp32 once;
  inside    row (j, k) tests a triangle iff cy and cz lie in the closed fp32 [min, max] of its vertices' y and z; the crossing
            test is `ray_x_crosses` of csrc/inside_test.h, operation by operation in fp32 (arrays of float32 never promote, and
            NumPy rounds each operation once: no contraction); voxel i is inside iff the crossings with xhit > centre(i),
            strictly, are odd in number;
  layout    bit t of word w in row (k, j) <-> voxel (i0 + 32 w + t, j0 + j, k0 + k), zero outside the box's own extents.
All (triangle, row) pairs of a mesh are evaluated at once, vectorised; nothing here is tuned to the kernel's output."""
import numpy as np

F32 = np.float32


def centres(first, n, h):
    """fp32 centres of the voxel indices first .. first + n - 1"""
    return (np.arange(first, first + n).astype(F32) + F32(0.5)) * F32(h)


def _orient2(x1, y1, x2, y2):
    """the half-open orientation rule -> (sign in {-1, 0, 1}, twice the signed area), fp32"""
    tsa = y1 * x2 - x1 * y2
    tie = np.where(y2 > y1, 1, np.where(y2 < y1, -1, np.where(x1 > x2, 1, np.where(x1 < x2, -1, 0))))
    return np.where(tsa > 0, 1, np.where(tsa < 0, -1, tie)), tsa


def ray_x_crosses(cy, cz, v1, v2, v3):
    """cy, cz (P,) fp32; v1, v2, v3 (P,3) fp32 -> (crosses (P,) bool, xhit (P,) fp32, defined where crosses)"""
    assert all(a.dtype == F32 for a in (cy, cz, v1, v2, v3))
    y1, z1 = v1[:, 1] - cy, v1[:, 2] - cz
    y2, z2 = v2[:, 1] - cy, v2[:, 2] - cz
    y3, z3 = v3[:, 1] - cy, v3[:, 2] - cz
    sa, a = _orient2(y2, z2, y3, z3)
    sb, b = _orient2(y3, z3, y1, z1)
    sc, g = _orient2(y1, z1, y2, z2)
    total = a + b + g
    ok = (sa != 0) & (sb == sa) & (sc == sa) & (total != 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fa, fb, fc = a / total, b / total, g / total
        xhit = fa * v1[:, 0] + fb * v2[:, 0] + fc * v3[:, 0]
    assert xhit.dtype == F32
    return ok, xhit


def _ranges(lo, hi, c):
    """per triangle, the contiguous run [a, b) of the increasing centres c with lo <= c <= hi"""
    return np.searchsorted(c, lo, side="left"), np.searchsorted(c, hi, side="right")


def occupancy(verts, faces, h, box):
    """verts (V,3), faces (F,3), box = (i0, j0, k0, nx, ny, nz) -> bool (nz, ny, nx): voxel inside?"""
    verts, h = np.ascontiguousarray(verts, F32), F32(h)
    i0, j0, k0, nx, ny, nz = (int(x) for x in box)
    occ = np.zeros((nz, ny, nx), bool)
    if nx <= 0 or ny <= 0 or nz <= 0:
        return occ
    cx, cy, cz = centres(i0, nx, h), centres(j0, ny, h), centres(k0, nz, h)
    assert (np.diff(cx) > 0).all() and (np.diff(cy) > 0).all() and (np.diff(cz) > 0).all()
    tri = verts[np.asarray(faces)]                                   # (F,3,3)
    ja, jb = _ranges(tri[:, :, 1].min(1), tri[:, :, 1].max(1), cy)
    ka, kb = _ranges(tri[:, :, 2].min(1), tri[:, :, 2].max(1), cz)
    nj, nk = np.maximum(jb - ja, 0), np.maximum(kb - ka, 0)
    per = nj * nk
    total = int(per.sum())
    if total == 0:
        return occ
    f = np.repeat(np.arange(len(per)), per)
    local = np.arange(total) - np.repeat(np.cumsum(per) - per, per)
    j = ja[f] + local % nj[f]
    k = ka[f] + local // nj[f]
    ok, xhit = ray_x_crosses(cy[j], cz[k], tri[f, 0], tri[f, 1], tri[f, 2])
    ok &= ~np.isnan(xhit)                                            # (NaN > c is false: no voxel in front)
    m = np.searchsorted(cx, xhit[ok], side="left")                   # number of centres with centre < xhit
    j, k = j[ok], k[ok]
    toggles = np.zeros((nz, ny, nx + 1), np.int64)                   # a crossing toggles the voxels 0 .. m - 1 of its row
    np.add.at(toggles, (k, j, m), 1)
    behind = np.cumsum(toggles[:, :, ::-1], axis=2)[:, :, ::-1]      # crossings with m >= i, for i = 0 .. nx
    return (behind[:, :, 1:] % 2).astype(bool)                       # voxel i is toggled by the crossings with m >= i + 1


def pack(occ, dims=None):
    """bool (nz, ny, nx) -> uint32 words (NZ, NY, NWX), dims = (NWX, NY, NZ) (default: the smallest that hold it)"""
    nz, ny, nx = occ.shape
    nwx, NY, NZ = (-(-nx // 32), ny, nz) if dims is None else dims
    assert nx <= 32 * nwx and ny <= NY and nz <= NZ
    bits = np.zeros((NZ, NY, 32 * nwx), np.uint64)
    bits[:nz, :ny, :nx] = occ
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (bits.reshape(NZ, NY, nwx, 32) * weights).sum(-1).astype(np.uint32)


def solid_voxels(verts, faces, h, boxes, dims=None):
    """verts (B,V,3), boxes (B,6) -> uint32 (B, NZ, NY, NWX): what hm_solid_voxels writes"""
    boxes = np.asarray(boxes).reshape(len(verts), 6)
    if dims is None:
        dims = (int(-(-boxes[:, 3].max() // 32)), int(boxes[:, 4].max()), int(boxes[:, 5].max()))
    return np.stack([pack(occupancy(v, faces, h, b), dims) for v, b in zip(verts, boxes)])


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def overlap_counts(a, b):
    """uint32 a (B,...) or (S,B,...), b (B,...) -> (B,3) uint64 {popcount(A & b), popcount(A), popcount(b)}, A = OR over S"""
    if a.ndim == b.ndim + 1:
        a = np.bitwise_or.reduce(a, axis=0)
    return np.array([[popcount(x & y), popcount(x), popcount(y)] for x, y in zip(a, b)], np.uint64)


def index_box(verts, h):
    """a mesh's inclusive index box (first (3,), last (3,)): floor(min / h) - 1 .. floor(max / h) + 1, the division in double"""
    verts, h = np.asarray(verts, F32).reshape(-1, 3).astype(np.float64), float(F32(h))
    return (np.floor(verts.min(0) / h) - 1).astype(np.int64), (np.floor(verts.max(0) / h) + 1).astype(np.int64)


def box_of(first, last):
    n = np.asarray(last) - np.asarray(first) + 1
    return np.concatenate([first, n if (n > 0).all() else np.zeros(3, np.int64)]).astype(np.int64)


def cell_volume(h):
    """(double)h^3 of the fp32 pitch, multiplied left to right"""
    hd = float(F32(h))
    return (hd * hd) * hd


def inter_volume(hands, hand_faces, obj, obj_faces, h):
    """hands: list of (Vh,3) meshes of one frame, each voxelised alone and OR-ed; obj (Vo,3) -> popcount(hand & obj) * h^3 over
    the intersection of the index box of all hand vertices with the object's"""
    hf, hl = index_box(np.concatenate(hands), h)
    of, ol = index_box(obj, h)
    box = box_of(np.maximum(hf, of), np.minimum(hl, ol))
    occ = np.zeros((box[5], box[4], box[3]), bool)
    for v in hands:
        occ |= occupancy(v, hand_faces, h, box)
    common = int((occ & occupancy(obj, obj_faces, h, box)).sum())
    return common * cell_volume(h)


def mesh_volume(verts, faces):
    """float64 |sum of signed tetrahedra about vertex 0| / 6 from the fp32 vertices, and sum |det| (for the error bound)"""
    v = np.asarray(verts, F32).astype(np.float64)
    e = v[np.asarray(faces)] - v[0]
    det = np.einsum("fi,fi->f", e[:, 0], np.cross(e[:, 1], e[:, 2]))
    return abs(det.sum()) / 6.0, np.abs(det).sum()


def surface_area(verts, faces):
    v = np.asarray(verts, np.float64)
    t = v[np.asarray(faces)]
    return 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum()


def cube_mesh(lo, hi):
    """12-triangle box [lo, hi] (3-vectors), outward winding, fp32 vertices"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)]).astype(F32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    faces = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.asarray(faces, np.int32)
