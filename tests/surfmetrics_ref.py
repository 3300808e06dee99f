"""NumPy restatement of the point-to-mesh distance of csrc/surfdist.hip and of the surface metrics built on it (not product
code, no device).  The rules are those of include/homan_amd.h / DESIGN.md section 7:

  distance   Ericson's region walk on ab, ac, ap, bp, cp with dot products formed as (x*x + y*y) + z*z, the first region that
             holds wins (A, B, AB, C, AC, BC, interior); a face whose cross product ab x ac is exactly (0, 0, 0) is its three
             segments ab, bc, ca (clamped projection, ties in that order);
  per point  d2 = the minimum over the faces, face = the lowest index that attains it, closest = that face's point;
  sign       inside iff the faces with `ray_x_crosses` (tests/volmetrics_ref.py, the rule of csrc/inside_test.h) and
             xhit > p_x, strictly, are odd in number;
  skipped    a face that names a vertex outside [0, V) or has a non-finite coordinate; a non-finite point gets (+inf, -1, 0, 0).
Arrays of float32 never promote and NumPy rounds each operation once (no contraction): in fp32 (the default) this performs the
kernel's operations in the kernel's order, all (point, face) pairs at once.  `dtype=np.float64` runs the same rules in double.
`independent_distance` is a second, differently built float64 distance: the plane distance where the projection falls inside
the triangle, else the minimum over the three segments.  Nothing here is tuned to the kernel's output."""
import numpy as np

from tests.volmetrics_ref import ray_x_crosses

F32 = np.float32


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _segment(p, u, v):
    """clamped projection of p on u -> v: (q, |p - q|^2)"""
    e, w = v - u, p - u
    len2 = _dot(e, e)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = _dot(w, e) / len2
    t = np.where(t < 0, 0, np.where(t > 1, 1, t)).astype(p.dtype)
    t = np.where(len2 > 0, t, 0).astype(p.dtype)
    q = u + t[..., None] * e
    d = p - q
    return q, _dot(d, d)


def face_distance(p, a, b, c):
    """p, a, b, c broadcastable (..., 3) of one float dtype -> (q (..., 3), D (...)) by the rules above"""
    assert p.dtype == a.dtype == b.dtype == c.dtype and p.dtype in (np.float32, np.float64)
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        q_in = (a + (vb / s)[..., None] * ab) + (vc / s)[..., None] * ac
        q_bc = b + (e1 / (e1 + e2))[..., None] * (c - b)
        q_ac = a + (d2 / (d2 - d6))[..., None] * ac
        q_ab = a + (d1 / (d1 - d3))[..., None] * ab
    regions = (((d1 <= 0) & (d2 <= 0), a), ((d3 >= 0) & (d4 <= d3), b), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), q_ab),
               ((d6 >= 0) & (d5 <= d6), c), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), q_ac), ((va <= 0) & (e1 >= 0) & (e2 >= 0), q_bc))
    q = q_in
    for holds, point in reversed(regions):                  # the first region that holds wins
        q = np.where(holds[..., None], point, q)
    d = p - q
    D = _dot(d, d)
    # degenerate faces: the three segments, ties in the order ab, bc, ca
    nx, ny, nz = ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2], \
        ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]
    flat = (nx == 0) & (ny == 0) & (nz == 0)
    if flat.any():
        qs, Ds = _segment(p, a, b)
        for u, v in ((b, c), (c, a)):
            q2, D2 = _segment(p, u, v)
            less = D2 < Ds
            qs, Ds = np.where(less[..., None], q2, qs), np.where(less, D2, Ds)
        q, D = np.where(flat[..., None], qs, q), np.where(flat, Ds, D)
    assert q.dtype == p.dtype and D.dtype == p.dtype
    return q, D


def valid_faces(verts, faces):
    """faces that name vertices of [0, V) with finite coordinates -> bool (F,)"""
    faces = np.asarray(faces).astype(np.int64)
    in_range = ((faces >= 0) & (faces < len(verts))).all(1)
    finite = np.isfinite(np.asarray(verts)[np.where(in_range[:, None], faces, 0)]).all((1, 2))
    return in_range & finite


def point_mesh(points, verts, faces, dtype=F32, block=96):
    """points (N,3), verts (V,3), faces (F,3) -> {"d2" (N,), "face" (N,) int32, "inside" (N,) int32, "closest" (N,3), "scale"
    (N,): the largest of |p - a|, |p - b|, |p - c| of the winning face in float64, for the error bars}"""
    points, verts = np.ascontiguousarray(points, dtype), np.ascontiguousarray(verts, dtype)
    faces = np.asarray(faces).astype(np.int64)
    keep = np.flatnonzero(valid_faces(verts, faces))
    n = len(points)
    out = {"d2": np.full(n, np.inf, dtype), "face": np.full(n, -1, np.int32), "inside": np.zeros(n, np.int32),
           "closest": np.zeros((n, 3), dtype), "scale": np.zeros(n)}
    ok = np.isfinite(points).all(1)
    if not len(keep) or not ok.any():
        return out
    tri = verts[faces[keep]]                                          # (K,3,3)
    rows = np.flatnonzero(ok)
    for r0 in range(0, len(rows), block):
        sel = rows[r0:r0 + block]
        p = points[sel]
        q, D = face_distance(p[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        D = np.where(np.isnan(D), np.inf, D)                          # (a NaN is never less than the best so far)
        best = D.min(1)
        k = np.argmax(D == best[:, None], axis=1)                     # the lowest index that attains the minimum
        found = best < np.inf
        pick = np.arange(len(sel))
        out["d2"][sel] = np.where(found, best, np.inf)
        out["face"][sel] = np.where(found, keep[k], -1)
        out["closest"][sel] = np.where(found[:, None], q[pick, k], 0)
        corner = tri[k].astype(np.float64) - p[:, None, :].astype(np.float64)
        out["scale"][sel] = np.where(found, np.linalg.norm(corner, axis=2).max(1), 0.0)
        P, K = len(sel), len(keep)
        if dtype == F32:
            flat = lambda x: np.ascontiguousarray(np.broadcast_to(x, (P, K) + x.shape[2:])).reshape((P * K,) + x.shape[2:])  # noqa: E731
            crosses, xhit = ray_x_crosses(flat(p[:, None, 1]), flat(p[:, None, 2]), flat(tri[None, :, 0]), flat(tri[None, :, 1]),
                                          flat(tri[None, :, 2]))
            hits = (crosses & (xhit > flat(p[:, None, 0]))).reshape(P, K)
            out["inside"][sel] = hits.sum(1) % 2
    return out


# ---------------------------------------------------------------------------------------------- the independent float64 distance
def _segment_distance64(p, u, v):
    e, w = v - u, p - u
    len2 = (e * e).sum(-1)
    t = np.clip(np.divide((w * e).sum(-1), len2, out=np.zeros_like(len2), where=len2 > 0), 0.0, 1.0)
    return np.linalg.norm(p - (u + t[..., None] * e), axis=-1)


def independent_distance(p, a, b, c):
    """float64 distance of p to the triangle (a, b, c), built differently from the region walk: the plane distance where the
    orthogonal projection falls inside the triangle, else the minimum over the three segments.  Broadcasts over (..., 3)."""
    p, a, b, c = (np.asarray(x, np.float64) for x in np.broadcast_arrays(p, a, b, c))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    safe = np.where(nn > 0, nn, 1.0)
    h = ((p - a) * n).sum(-1) / safe                                  # p = foot + h n
    foot = p - h[..., None] * n
    within = np.ones(nn.shape, bool)
    for u, v in ((a, b), (b, c), (c, a)):
        within &= (np.cross(v - u, foot - u) * n).sum(-1) >= 0
    within &= nn > 0
    edges = np.minimum(np.minimum(_segment_distance64(p, a, b), _segment_distance64(p, b, c)), _segment_distance64(p, c, a))
    return np.where(within, np.abs(h) * np.sqrt(safe), edges)


def independent_mesh_distance(points, verts, faces, block=256):
    """float64 distance of every point to the mesh (valid faces only) -> (N,)"""
    points, verts = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    tri = verts[np.asarray(faces)[valid_faces(verts, faces)]]
    out = np.empty(len(points))
    for r0 in range(0, len(points), block):
        p = points[r0:r0 + block, None, :]
        out[r0:r0 + block] = independent_distance(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]).min(1)
    return out


def min_height_to_edge(verts, faces):
    """the smallest ratio (height over its longest edge) of the non-degenerate faces of a mesh, float64"""
    t = np.asarray(verts, np.float64)[np.asarray(faces)]
    edges = np.stack([np.linalg.norm(t[:, (k + 1) % 3] - t[:, k], axis=1) for k in range(3)], 1)
    area2 = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    longest = edges.max(1)
    ratio = area2[longest > 0] / longest[longest > 0] ** 2
    return float(ratio[ratio > 0].min())


# ---------------------------------------------------------------------------------------------- the metrics
def surface_metrics(hands, hand_faces, obj, obj_faces, contact_thresh=0.005):
    """One frame.  hands: list of (Vh,3) meshes, hand_faces: one (Fh,3) array per hand, obj (Vo,3) ->
    {"pen_depth", "pen_depth_obj", "min_dist", "contact_share", "has_contact", "signed_dist" (hands, Vh) float64}"""
    dists, insides, depth_obj = [], [], 0.0
    for v, f in zip(hands, hand_faces):
        r = point_mesh(v, obj, obj_faces)
        dists.append(np.sqrt(r["d2"].astype(np.float64)))
        insides.append(r["inside"] == 1)
        back = point_mesh(obj, v, f)                                   # each hand queried as its own mesh
        in_hand = back["inside"] == 1
        if in_hand.any():
            depth_obj = max(depth_obj, float(np.sqrt(back["d2"].astype(np.float64))[in_hand].max()))
    dist, inside = np.stack(dists), np.stack(insides)
    signed = np.where(inside, -dist, dist)
    pen = float(dist[inside].max()) if inside.any() else 0.0
    min_dist = float(dist.min())
    share = float(np.float64((inside | (dist <= contact_thresh)).sum()) / np.float64(dist.size))
    return {"pen_depth": pen, "pen_depth_obj": depth_obj, "min_dist": min_dist, "contact_share": share,
            "has_contact": bool(pen > 0 or depth_obj > 0 or min_dist <= contact_thresh), "signed_dist": signed}
