"""NumPy restatement of the surface contact loss of csrc/surfcontact.hip (not product code, no device), on the search of
tests/surfmetrics_ref.py.  The rules are those of include/homan_amd.h / DESIGN.md section 7:

  walk       the winning face is walked again by the search's own rules (`walk`, the operations of csrc/surfdist_walk.h in their
             order), which gives q, D, the barycentric weights and dv = p - q in world space;
  terms      d = sqrt(D), c = inside ? c_r : c_a, t = hm_tanh(d / c), om = inside ? 1 : weights[i], u = om (c t),
             phi = om (1 - t t), g = (phi dv) / d; u = g = 0 when face < 0 or D == 0, weights 0 when face < 0;
  sums       every fp32 addend rounded to the grid 2^L as (x + magic) - magic in double, counted in quanta as integers and
             summed exactly; a total is (float)((double)count * 2^L / (B N)); the loss adds its per-frame counts as hi / lo words.
Arrays of float32 never promote and NumPy rounds each operation once: in fp32 this performs the kernel's operations in the
kernel's order.  `hm_tanh` restates csrc/hm_common.h in float64.  `reference64` is the float64 loss with torch autograd through
d = |p - sum_k w_k.detach() x_k|, given the fp32 search's face and inside flag (teacher forcing).  Nothing here is tuned to the
kernel's output."""
import math

import numpy as np

from tests import surfmetrics_ref as sref

F32, F64 = np.float32, np.float64
CONTACT_THRESH, COLLISION_THRESH = 0.010, 0.020
TIPS = (745, 317, 444, 556, 673)


def hm_tanh(x):
    """csrc/hm_common.h hm_tanh: fp32 in, IEEE double operations, fp32 out"""
    x = np.asarray(x, F32)
    ax = np.abs(x.astype(F64))
    q = ax * ax
    small = ax * (1.0 + q * (-3.33333333333333314830e-01 + q * (1.33333333333333331483e-01 + q * -5.39682539682539708542e-02)))
    t = -2.0 * np.minimum(ax, 20.0)                        # (beyond 20 the result is replaced below)
    k = np.rint(t * 1.44269504088896338700e+00)
    r = (t - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
    z = r * r
    p = np.full_like(z, 4.13813679705723846039e-08)
    for coef in (-1.65339022054652515390e-06, 6.61375632143793436117e-05, -2.77777777770155933842e-03, 1.66666666666666019037e-01):
        p = coef + z * p
    c = r - z * p
    er = 1.0 - ((r * c) / (c - 2.0) - r)
    e = np.ldexp(er, k.astype(np.int64))
    th = (1.0 - e) / (1.0 + e)
    th = np.where(ax > 20.0, 1.0, np.where(ax < 0.01, small, th))
    return np.where(x < 0, -th, th).astype(F32)


def _segment(p, u, v):
    e, w = v - u, p - u
    len2 = sref._dot(e, e)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = sref._dot(w, e) / len2
    t = np.where(t < 0, 0, np.where(t > 1, 1, t)).astype(p.dtype)
    t = np.where(len2 > 0, t, 0).astype(p.dtype)
    q = u + t[..., None] * e
    d = p - q
    return q, sref._dot(d, d), t


def walk(p, a, b, c):
    """p, a, b, c (n,3) of one float dtype: one face per point -> (q (n,3), D (n,), w (n,3), dv (n,3)): the rules of
    surfmetrics_ref.face_distance with the weights each region implies"""
    dt = p.dtype
    assert a.dtype == b.dtype == c.dtype == dt and dt in (F32, F64)
    one, zero = np.ones(len(p), dt), np.zeros(len(p), dt)
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    dot = sref._dot
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        tv, tw = vb / s, vc / s
        t_bc, t_ac, t_ab = e1 / (e1 + e2), d2 / (d2 - d6), d1 / (d1 - d3)
        q_in = (a + tv[:, None] * ab) + tw[:, None] * ac
        q_bc = b + t_bc[:, None] * (c - b)
        q_ac = a + t_ac[:, None] * ac
        q_ab = a + t_ab[:, None] * ab
        stack = lambda *cols: np.stack(cols, 1).astype(dt)  # noqa: E731
        regions = (((d1 <= 0) & (d2 <= 0), a, stack(one, zero, zero)),
                   ((d3 >= 0) & (d4 <= d3), b, stack(zero, one, zero)),
                   ((vc <= 0) & (d1 >= 0) & (d3 <= 0), q_ab, stack(one - t_ab, t_ab, zero)),
                   ((d6 >= 0) & (d5 <= d6), c, stack(zero, zero, one)),
                   ((vb <= 0) & (d2 >= 0) & (d6 <= 0), q_ac, stack(one - t_ac, zero, t_ac)),
                   ((va <= 0) & (e1 >= 0) & (e2 >= 0), q_bc, stack(zero, one - t_bc, t_bc)))
        q, w = q_in, stack((one - tv) - tw, tv, tw)
    for holds, point, weights in reversed(regions):                 # the first region that holds wins
        q, w = np.where(holds[:, None], point, q), np.where(holds[:, None], weights, w)
    nx, ny, nz = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], \
        ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    flat = (nx == 0) & (ny == 0) & (nz == 0)
    if flat.any():                                                   # the three segments, ties in the order ab, bc, ca
        qs, Ds, t = _segment(p, a, b)
        ws = stack(one - t, t, zero)
        for (u, v), place in (((b, c), lambda t: stack(zero, one - t, t)), ((c, a), lambda t: stack(t, zero, one - t))):
            q2, D2, t2 = _segment(p, u, v)
            less = D2 < Ds
            qs, Ds, ws = np.where(less[:, None], q2, qs), np.where(less, D2, Ds), np.where(less[:, None], place(t2), ws)
        q, w = np.where(flat[:, None], qs, q), np.where(flat[:, None], ws, w)
    dv = p - q
    D = dot(dv, dv)
    assert q.dtype == dt and w.dtype == dt and D.dtype == dt
    return q, D, w, dv


def terms(points, verts, faces, weights=None, contact_thresh=CONTACT_THRESH, collision_thresh=COLLISION_THRESH, search=None):
    """One frame: points (N,3), verts (V,3), faces (F,3), weights (N,) or None -> {"value" u, "g" (N,3) (not yet / (B N)), "bary"
    (N,3), "d2", "face", "inside"}, all fp32 / int32.  search: the result of surfmetrics_ref.point_mesh, if already known."""
    points, verts = np.ascontiguousarray(points, F32), np.ascontiguousarray(verts, F32)
    faces = np.asarray(faces).astype(np.int64)
    s = sref.point_mesh(points, verts, faces) if search is None else search
    n = len(points)
    face, inside = s["face"], s["inside"] != 0
    found = face >= 0
    tri = verts[np.clip(faces[np.where(found, face, 0)], 0, len(verts) - 1)]     # (N,3,3); a placeholder where none was found
    p = np.where(found[:, None], points, 0).astype(F32)
    tri = np.where(found[:, None, None], tri, 0).astype(F32)
    q, D, w, dv = walk(p, tri[:, 0], tri[:, 1], tri[:, 2])
    assert np.array_equal(D[found].view(np.uint32), s["d2"][found].view(np.uint32)), "the walk is not the search's"
    assert np.array_equal(q[found].view(np.uint32), s["closest"][found].view(np.uint32))
    valid = found & (D != 0)
    c = np.where(inside, F32(collision_thresh), F32(contact_thresh)).astype(F32)
    om = np.ones(n, F32) if weights is None else np.where(inside, F32(1), np.asarray(weights, F32)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.sqrt(D)
        t = hm_tanh(d / c)
        u = om * (c * t)
        phi = om * (F32(1) - t * t)
        g = (phi[:, None] * dv) / d[:, None]
    u, g = np.where(valid, u, 0).astype(F32), np.where(valid[:, None], g, 0).astype(F32)
    w = np.where(found[:, None], w, 0).astype(F32)
    return {"value": u, "g": g, "bary": w, "d2": s["d2"], "face": face, "inside": s["inside"], "valid": valid}


def log2q(N, weight_max=1.0, contact_thresh=CONTACT_THRESH, collision_thresh=COLLISION_THRESH):
    """the grid of the exact sums: ceil(log2(N M)) - 50 with M = max(weight_max, 1) * max(c_a, c_r, 1)"""
    M = max(float(weight_max), 1.0) * max(float(contact_thresh), float(collision_thresh), 1.0)
    return math.ceil(math.log2(N * M)) - 50


def quanta(x, L):
    """fp32 x rounded to the grid 2^L as hm_quant does, as an integer count (int64)"""
    magic = 6755399441055744.0 * math.ldexp(1.0, L)
    r = (np.asarray(x, F32).astype(F64) + magic) - magic
    n = r * math.ldexp(1.0, -L)
    assert (np.abs(n) < 2.0 ** 51).all(), "an addend outside the exact range"
    return n.astype(np.int64)


def frame_sums(t, faces, V, L):
    """per-point terms of one frame -> (vertex counts (2,V,3) int64: attraction, repulsion; loss counts (2,) Python ints)"""
    faces = np.asarray(faces).astype(np.int64)
    acc = np.zeros((2, V, 3), np.int64)
    loss = [0, 0]
    for side in (0, 1):
        sel = np.flatnonzero(t["valid"] & ((t["inside"] != 0) == bool(side)))
        for k in range(3):
            add = quanta(-(t["bary"][sel, k][:, None] * t["g"][sel]), L)          # the fp32 product, negated, then rounded
            add[t["bary"][sel, k] == 0] = 0
            np.add.at(acc[side], faces[t["face"][sel], k], add)
        loss[side] = int(quanta(t["value"][sel], L).sum())
        assert np.abs(acc[side]).max(initial=0) < 2 ** 53 and abs(loss[side]) < 2 ** 53
    return acc, loss


def loss_and_gradients(points, verts, faces, weights=None, contact_thresh=CONTACT_THRESH, collision_thresh=COLLISION_THRESH,
                       L=None, searches=None):
    """points (B,N,3), verts (B,V,3) -> {"out" (2,) = (A, R), "grad_points" (B,N,3), "grad_verts_attr", "grad_verts_rep" (B,V,3),
    and the per-point detail "value", "bary", "d2", "face", "inside" (B, ...)}: what hm_surface_contact_fwd returns, bit for bit"""
    points, verts = np.asarray(points, F32), np.asarray(verts, F32)
    B, N, V = points.shape[0], points.shape[1], verts.shape[1]
    if L is None:
        L = log2q(N, 1.0 if weights is None else float(np.max(weights)), contact_thresh, collision_thresh)
    bn, q = float(B * N), math.ldexp(1.0, L)
    frames = [terms(points[b], verts[b], faces, weights, contact_thresh, collision_thresh,
                    None if searches is None else searches[b]) for b in range(B)]
    sums = [frame_sums(t, faces, V, L) for t in frames]
    out = {k: np.stack([t[k] for t in frames]) for k in ("value", "bary", "d2", "face", "inside")}
    out["g"] = np.stack([t["g"] for t in frames])
    out["grad_points"] = (out["g"].astype(F64) / bn).astype(F32)
    verts_grad = np.stack([acc for acc, _ in sums], 1)                                     # (2,B,V,3)
    conv = ((verts_grad.astype(F64) * q) / bn).astype(F32)
    out["grad_verts_attr"], out["grad_verts_rep"] = conv[0], conv[1]
    total = []
    for side in (0, 1):
        hi = sum(loss[side] >> 32 for _, loss in sums)
        lo = sum(loss[side] & 0xffffffff for _, loss in sums)
        total.append(F32(((float(hi) * 4294967296.0 + float(lo)) * q) / bn))
    out["out"] = np.array(total, F32)
    out["L"] = L
    return out


def reference64(points, verts, faces, face, inside, weights=None, contact_thresh=CONTACT_THRESH,
                collision_thresh=COLLISION_THRESH, skip=None):
    """float64, torch autograd: points (B,N,3), verts (B,V,3), the fp32 search's face and inside (B,N) -> {"out" (2,), "value"
    (B,N), "grad_points" (B,N,3): of A where outside and of R where inside, "grad_verts_attr", "grad_verts_rep" (B,V,3)}.
    skip (B,N) bool: points the fp32 side gives no term (its D == 0)."""
    import torch
    faces = np.asarray(faces).astype(np.int64)
    face, inside = np.asarray(face), np.asarray(inside) != 0
    B, N = face.shape
    found = face >= 0
    P = torch.tensor(np.where(found[..., None], np.asarray(points, F64), 0.0), requires_grad=True)
    X = torch.tensor(np.asarray(verts, F64), requires_grad=True)
    idx = np.clip(faces[np.where(found, face, 0)], 0, X.shape[1] - 1)                      # (B,N,3)
    tri = X[torch.arange(B)[:, None, None], torch.from_numpy(idx)]                         # (B,N,3 corners,3)
    flat = lambda x: x.detach().numpy().reshape(B * N, 3)  # noqa: E731
    _, _, w, _ = walk(flat(P), flat(tri[:, :, 0]), flat(tri[:, :, 1]), flat(tri[:, :, 2]))
    w = torch.from_numpy(w.reshape(B, N, 3))
    diff = P - (w[..., None] * tri).sum(2)
    valid = torch.from_numpy(found) & (diff.detach() != 0).any(2)
    if skip is not None:
        valid = valid & ~torch.from_numpy(np.asarray(skip, bool))
    d = torch.where(valid[..., None], diff, torch.ones_like(diff)).norm(dim=2)       # (no norm of a zero vector on the tape)
    c = torch.from_numpy(np.where(inside, float(F32(collision_thresh)), float(F32(contact_thresh))))
    om = torch.ones(B, N, dtype=torch.float64) if weights is None else \
        torch.from_numpy(np.where(inside, 1.0, np.asarray(weights, F64)[None, :]))
    u = torch.where(valid, om * c * torch.tanh(d / c), torch.zeros_like(d))
    ins = torch.from_numpy(inside)
    A, R = (u * ~ins).sum() / (B * N), (u * ins).sum() / (B * N)
    gpa, gva = torch.autograd.grad(A, (P, X), retain_graph=True)
    gpr, gvr = torch.autograd.grad(R, (P, X))
    return {"out": np.array([A.item(), R.item()]), "value": u.detach().numpy(),
            "grad_points": torch.where(ins[..., None], gpr, gpa).numpy(),
            "grad_verts_attr": gva.numpy(), "grad_verts_rep": gvr.numpy()}
