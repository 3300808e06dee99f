"""NumPy restatement of the generalised winding number of csrc/winding.hip (hm_point_mesh_winding) and of `hm_atan2`
(csrc/hm_common.h); not product code, no device.  The rules are those of include/homan_amd.h / DESIGN.md section 7:

  per pair   A = (double)a - (double)p, B, C likewise; dot products (x*x + y*y) + z*z; la = sqrt(A.A), lb, lc;
             num = (A_x (B x C)_x + A_y (B x C)_y) + A_z (B x C)_z with B x C = (B_y C_z - B_z C_y, B_z C_x - B_x C_z,
             B_x C_y - B_y C_x); den = ((((la lb) lc + (A.B) lc) + (B.C) la) + (C.A) lb);
             omega = 0 when num == 0, else 2 hm_atan2(num, den);
  hm_atan2   mx = max(|x|, |y|), mn = min(|x|, |y|); 0 when mx == 0; u = (mn - mx) / (mn + mx) and base pi/4 when
             mn > tan(pi/8) mx, else u = mn / mx and base 0; z = u u, q = the alternating series c_19 ... c_1 by Horner,
             r = base + (u + (u z) q); r = pi/2 - r when |y| > |x|; r = pi - r when x < 0; r = -r when y < 0;
  exact sum  every omega is rounded to the grid 2^L, ties to even ((omega + magic) - magic in the kernel, np.rint(omega / 2^L)
             here: the same value while |omega| < 2^(L + 51)), and the quanta are added as signed 64-bit integers;
  sign       inside iff |count| > T, T = rint(2 pi / 2^L): |w| > 0.5 decided in integers;
  skipped    a face that names a vertex outside [0, V), has a non-finite coordinate, or has zero area as the search defines it
             (the fp32 cross product (b - a) x (c - a) is exactly (0, 0, 0)); a non-finite point gets (0, 0).
Arrays of float64 are combined one IEEE operation at a time (NumPy contracts nothing), in the kernel's order, all (point, face)
pairs of a block at once.  `independent_winding` is a second, differently built float64 winding number: the spherical excess
of the face's three unit directions by l'Huilier's theorem with np.arctan / np.arccos, signed by the determinant.  Nothing here
is tuned to the kernel's output."""
import math

import numpy as np

from tests.surfmetrics_ref import valid_faces

F32, F64 = np.float32, np.float64
TAN_PI_8 = 0.41421356237309503
PI_4, PI_2, PI, TWO_PI = 0.7853981633974483, 1.5707963267948966, 3.141592653589793, 6.283185307179586
# c_k = (-1)^k / (2k + 1), k = 1 ... 19, as the doubles nearest to them (the literals of csrc/hm_common.h)
ATAN_C = tuple(F64((-1.0) ** k) / F64(2 * k + 1) for k in range(1, 20))
LOG2Q_MIN = -47


def hm_atan2(y, x):
    """hm_atan2 of csrc/hm_common.h, operation by operation: float64 arrays (broadcastable) -> float64"""
    y, x = np.broadcast_arrays(np.asarray(y, F64), np.asarray(x, F64))
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.where(ay > ax, ay, ax), np.where(ay > ax, ax, ay)
    fold = mn > TAN_PI_8 * mx
    top, bottom = np.where(fold, mn - mx, mn), np.where(fold, mn + mx, mx)
    zero = mx == 0
    u = top / np.where(zero, 1.0, bottom)
    z = u * u
    q = np.full(u.shape, ATAN_C[18])
    for k in range(17, -1, -1):
        q = ATAN_C[k] + z * q
    r = np.where(fold, PI_4, 0.0) + (u + (u * z) * q)
    r = np.where(ay > ax, PI_2 - r, r)
    r = np.where(x < 0, PI - r, r)
    r = np.where(y < 0, -r, r)
    return np.where(zero, 0.0, r)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def solid_angles(p, a, b, c):
    """p, a, b, c broadcastable (..., 3) float32 -> omega (...) float64: the signed solid angle of each pair by the rules above"""
    assert p.dtype == a.dtype == b.dtype == c.dtype == F32
    p = p.astype(F64)
    A, B, C = a.astype(F64) - p, b.astype(F64) - p, c.astype(F64) - p
    la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
    cx = B[..., 1] * C[..., 2] - B[..., 2] * C[..., 1]
    cy = B[..., 2] * C[..., 0] - B[..., 0] * C[..., 2]
    cz = B[..., 0] * C[..., 1] - B[..., 1] * C[..., 0]
    num = (A[..., 0] * cx + A[..., 1] * cy) + A[..., 2] * cz
    den = (((la * lb) * lc + _dot(A, B) * lc) + _dot(B, C) * la) + _dot(C, A) * lb
    return np.where(num == 0, 0.0, 2.0 * hm_atan2(num, den))


def counted_faces(verts, faces):
    """the faces that count: valid by the search's rules and not of zero area in fp32 -> bool (F,)"""
    verts = np.ascontiguousarray(verts, F32)
    faces = np.asarray(faces).astype(np.int64)
    ok = valid_faces(verts, faces)
    t = verts[np.where(ok[:, None], faces, 0)]
    with np.errstate(over="ignore", invalid="ignore"):
        ab, ac = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    return ok & ~((nx == 0) & (ny == 0) & (nz == 0))


def winding_log2q(F):
    """ops.winding_log2q restated: max(-44, ceil(log2 F) - 59)"""
    return max(-44, (int(F) - 1).bit_length() - 59)


def threshold(log2q):
    return int(np.rint(math.ldexp(TWO_PI, -log2q)))


def point_mesh_winding(points, verts, faces, log2q=None, block=96):
    """points (N,3), verts (V,3), faces (F,3) -> {"count" (N,) int64, "inside" (N,) int32, "winding" (N,) float64 =
    count * 2^L / (4 pi), "log2q"}: what hm_point_mesh_winding returns for one frame, bit for bit"""
    points, verts = np.ascontiguousarray(points, F32), np.ascontiguousarray(verts, F32)
    faces = np.asarray(faces).astype(np.int64)
    L = winding_log2q(len(faces)) if log2q is None else int(log2q)
    count = np.zeros(len(points), np.int64)
    keep = np.flatnonzero(counted_faces(verts, faces))
    rows = np.flatnonzero(np.isfinite(points).all(1))
    if len(keep) and len(rows):
        tri = verts[faces[keep]]
        scale = math.ldexp(1.0, -L)
        for r0 in range(0, len(rows), block):
            sel = rows[r0:r0 + block]
            omega = solid_angles(points[sel][:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
            count[sel] = np.rint(omega * scale).astype(np.int64).sum(1)
    inside = (np.abs(count) > threshold(L)).astype(np.int32)
    return {"count": count, "inside": inside, "winding": count.astype(F64) * math.ldexp(1.0, L) / (4.0 * PI), "log2q": L}


# ---------------------------------------------------------------------------------------------- the independent winding number
def independent_winding(points, verts, faces, block=256):
    """float64 winding number built differently: per face the spherical excess E of the unit directions to a, b, c by
    l'Huilier's theorem, tan(E/4) = sqrt(tan(s/2) tan((s-x)/2) tan((s-y)/2) tan((s-z)/2)) with x, y, z the arcs between the
    directions (np.arccos of clipped dot products, s their half sum), signed by det(A, B, C); w = sum / (4 pi).  Loses digits
    for needle-thin spherical triangles, which is the measured part of the bar (tests/test_winding.py)."""
    points, verts = np.asarray(points, F64), np.asarray(verts, F64)
    tri = verts[np.asarray(faces)[counted_faces(verts.astype(F32), faces)]]
    out = np.zeros(len(points))
    for r0 in range(0, len(points), block):
        p = points[r0:r0 + block, None, None, :]
        d = tri[None] - p                                               # (P, K, 3, 3)
        length = np.linalg.norm(d, axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            n = d / length
        arcs = [np.arccos(np.clip((n[:, :, i] * n[:, :, j]).sum(-1), -1.0, 1.0)) for i, j in ((1, 2), (2, 0), (0, 1))]
        s = 0.5 * (arcs[0] + arcs[1] + arcs[2])
        prod = np.tan(0.5 * s) * np.tan(0.5 * (s - arcs[0])) * np.tan(0.5 * (s - arcs[1])) * np.tan(0.5 * (s - arcs[2]))
        excess = 4.0 * np.arctan(np.sqrt(np.maximum(prod, 0.0)))
        det = np.linalg.det(d)
        omega = np.where(np.isfinite(excess) & (det != 0), np.sign(det) * excess, 0.0)
        out[r0:r0 + block] = omega.sum(1) / (4.0 * np.pi)
    return out


# ---------------------------------------------------------------------------------------------- the metrics
def surface_metrics(hands, hand_faces, obj, obj_faces, contact_thresh=0.005):
    """tests/surfmetrics_ref.surface_metrics with the sign of the winding number: distances from the fp32 search, `inside`
    from `point_mesh_winding`"""
    from tests.surfmetrics_ref import point_mesh
    dists, insides, depth_obj = [], [], 0.0
    for v, f in zip(hands, hand_faces):
        dists.append(np.sqrt(point_mesh(v, obj, obj_faces)["d2"].astype(F64)))
        insides.append(point_mesh_winding(v, obj, obj_faces)["inside"] == 1)
        back = np.sqrt(point_mesh(obj, v, f)["d2"].astype(F64))
        in_hand = point_mesh_winding(obj, v, f)["inside"] == 1
        if in_hand.any():
            depth_obj = max(depth_obj, float(back[in_hand].max()))
    dist, inside = np.stack(dists), np.stack(insides)
    pen = float(dist[inside].max()) if inside.any() else 0.0
    min_dist = float(dist.min())
    share = float(F64((inside | (dist <= contact_thresh)).sum()) / F64(dist.size))
    return {"pen_depth": pen, "pen_depth_obj": depth_obj, "min_dist": min_dist, "contact_share": share,
            "has_contact": bool(pen > 0 or depth_obj > 0 or min_dist <= contact_thresh),
            "signed_dist": np.where(inside, -dist, dist)}
