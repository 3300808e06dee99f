"""NumPy restatement of the edge-collapse decimation of csrc/decimate.hip, ops.collapse_round / ops.decimate_mesh,
meshprep.decimate and meshprep.make_watertight_detail; not product code, no device.  The rules are those of include/homan_amd.h / DESIGN.md section 7.  The state is
V (n,3) fp32 and F (m,3) integers, closed and oriented, n > target; one round:

  1 face quadric    in double from the fp32 coordinates: N = (b - a) x (c - a), d = -((Nx ax + Ny ay) + Nz az); the 10 numbers
                    (NxNx, NxNy, NxNz, NyNy, NyNz, NzNz, Nx d, Ny d, Nz d, d d); no normalisation (weight: squared doubled area);
  2 vertex quadric  the sum over the incident faces in ascending face index, sequential double adds from 0;
  3 edges           undirected, a < b, in ascending (a, b); c = the third vertex of the face that runs a -> b, d = of the face that
                    runs b -> a;
  4 placement       three fp32 candidates V[a], V[b], (V[a] + V[b]) * 0.5f; err_k = the form of Q_a + Q_b at candidate k:
                    ((((((((q0 x) x + (q3 y) y) + (q5 z) z) + 2 ((q1 x) y)) + 2 ((q2 x) z)) + 2 ((q4 y) z)) + 2 (q6 x)) + 2 (q7 y))
                    + 2 (q8 z)) + q9; choice = the first minimum in the order a, b, mid; l2 = (dx dx + dy dy) + dz dz in double;
                    cost = err + (double)regularity * ((l2 l2) l2); a non-finite cost makes the edge invalid;
  5 validity        m > 4; |N(a) & N(b)| == 2; valence(c) > 3 and valence(d) > 3; for every face that holds exactly one of a, b:
                    with that corner moved to p, (Nox Nnx + Noy Nny) + Noz Nnz > 0 for the normals of rule 1 before and after;
  6 rank            the valid edges sorted by (cost, l2, edge index) get 0, 1, ...; an invalid edge has RANK_NONE;
  7 selection       m1[v] = the least rank of a valid edge at v; m2[w] = min(m1[w], m1[v] for v in N(w)); e is selected iff
                    m2[a] == m2[b] == rank(e);
  8 budget          of the selected edges only the need = n - target of lowest rank are kept (`selected` is what is kept);
  9 apply           V[a] = p; b -> a in every face; faces that now repeat a vertex and the vertices b are dropped; both lists
                    are compacted in their order;
 10 stop            n <= target, a round that selects nothing (stuck), or max_rounds.
Nothing here is tuned to the kernels' output."""
import numpy as np

from tests import meshprep_ref as mref

F32, F64 = np.float32, np.float64
RANK_NONE = 2 ** 31 - 1
REGULARITY, MAX_ROUNDS = 0.01, 4096


# ---------------------------------------------------------------------------------------------- checks
def check_mesh(vertices, faces):
    """-> (V fp32, F int64); ValueError unless closed, oriented, no face repeats a vertex, indices in range, coordinates finite.
    Vertices that no face names are dropped first (the others keep their order)."""
    V = np.ascontiguousarray(vertices, F32)
    F = np.asarray(faces).astype(np.int64)
    if V.ndim != 2 or V.shape[1] != 3 or F.ndim != 2 or F.shape[1] != 3 or len(F) < 1:
        raise ValueError("shapes")
    if F.min() < 0 or F.max() >= len(V):
        raise ValueError("indices out of range")
    used = np.unique(F)
    V, F = V[used], np.searchsorted(used, F)
    if not np.isfinite(V).all():
        raise ValueError("a coordinate is not finite")
    if (F[:, 0] == F[:, 1]).any() or (F[:, 1] == F[:, 2]).any() or (F[:, 2] == F[:, 0]).any():
        raise ValueError("a face repeats a vertex")
    tails, heads = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1)
    n = len(V)
    directed = np.unique(tails * n + heads, return_counts=True)
    if (directed[1] != 1).any() or not np.array_equal(directed[0], np.unique(heads * n + tails)):
        raise ValueError("not closed and oriented: every edge must be run once in each direction")
    return V, F


# ---------------------------------------------------------------------------------------------- structure
def _ranges(start, count):
    """concatenated aranges start[i] ... start[i] + count[i] - 1 -> (the owner i of every element, the element)"""
    owner = np.repeat(np.arange(len(start)), count)
    first = np.repeat(np.cumsum(count) - count, count)
    return owner, np.repeat(start, count) + (np.arange(len(owner)) - first)


def structure(F, n):
    F = np.asarray(F, np.int64)
    u, w, c = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1), F[:, [2, 0, 1]].reshape(-1)
    key = u * n + w
    order = np.argsort(key, kind="stable")
    su, sw, sc, skey = u[order], w[order], c[order], key[order]
    voff = np.concatenate([[0], np.cumsum(np.bincount(su, minlength=n))])
    fwd = su < sw
    a, b, cc = su[fwd], sw[fwd], sc[fwd]
    back = np.searchsorted(skey, b * n + a)
    assert np.array_equal(skey[back], b * n + a)
    corners = np.argsort(u, kind="stable")                  # per vertex its corners in ascending corner = face index
    return {"nbr": sw, "voff": voff, "valence": np.diff(voff), "keys": skey, "edges": np.stack([a, b, cc, sc[back]], 1),
            "corners": corners, "he_u": su, "he_w": sw}


def normals(a, b, c):
    e1, e2 = b - a, c - a
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)


def face_quadrics(P, F):
    a, b, c = P[F[:, 0]], P[F[:, 1]], P[F[:, 2]]
    N = normals(a, b, c)
    d = -((N[:, 0] * a[:, 0] + N[:, 1] * a[:, 1]) + N[:, 2] * a[:, 2])
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    return np.stack([x * x, x * y, x * z, y * y, y * z, z * z, x * d, y * d, z * d, d * d], 1)


def vertex_quadrics(q, st, n):
    Q = np.zeros((n, 10), F64)
    val, first = st["valence"], st["voff"][:-1]
    for j in range(int(val.max())):
        sel = np.nonzero(val > j)[0]
        Q[sel] = Q[sel] + q[st["corners"][first[sel] + j] // 3]
    return Q


def quadric_form(Q, p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    s = (Q[:, 0] * x) * x + (Q[:, 3] * y) * y
    s = s + (Q[:, 5] * z) * z
    s = s + 2.0 * ((Q[:, 1] * x) * y)
    s = s + 2.0 * ((Q[:, 2] * x) * z)
    s = s + 2.0 * ((Q[:, 4] * y) * z)
    s = s + 2.0 * (Q[:, 6] * x)
    s = s + 2.0 * (Q[:, 7] * y)
    s = s + 2.0 * (Q[:, 8] * z)
    return s + Q[:, 9]


# ---------------------------------------------------------------------------------------------- one round
def collapse_round(vertices, faces, need, regularity=REGULARITY):
    """-> {"vertices", "faces" after the round, "edges" (E,4) a b c d, "choice", "cost", "l2", "valid", "rank", "selected",
    "collapses"}"""
    V, F = np.ascontiguousarray(vertices, F32), np.asarray(faces).astype(np.int64)
    n, m = len(V), len(F)
    reg = F64(F32(regularity))
    st = structure(F, n)
    P = V.astype(F64)
    Q = vertex_quadrics(face_quadrics(P, F), st, n)
    ed = st["edges"]
    a, b, c, d = ed.T
    E = len(ed)
    with np.errstate(all="ignore"):
        cand = np.stack([V[a], V[b], (V[a] + V[b]) * F32(0.5)], 1)
        assert cand.dtype == F32
        Qe = Q[a] + Q[b]
        errs = np.stack([quadric_form(Qe, cand[:, k].astype(F64)) for k in range(3)], 1)
        choice = np.zeros(E, np.int32)
        best = errs[:, 0].copy()
        for k in (1, 2):
            less = errs[:, k] < best
            choice[less], best[less] = k, errs[less, k]
        dlt = P[b] - P[a]
        l2 = (dlt[:, 0] * dlt[:, 0] + dlt[:, 1] * dlt[:, 1]) + dlt[:, 2] * dlt[:, 2]
        cost = best + reg * ((l2 * l2) * l2)
        p32 = cand[np.arange(E), choice]
        p = p32.astype(F64)
        val, voff = st["valence"], st["voff"]
        owner, slot = _ranges(voff[a], val[a])              # the link condition: common neighbours of a and b
        want = b[owner] * n + st["nbr"][slot]
        at = np.minimum(np.searchsorted(st["keys"], want), len(st["keys"]) - 1)
        common = np.bincount(owner, weights=st["keys"][at] == want, minlength=E)
        valid = np.isfinite(cost) & (common == 2) & (val[c] > 3) & (val[d] > 3) & (m > 4)
        for end, other in ((a, b), (b, a)):                 # the faces around each endpoint, that endpoint moved to p
            owner, slot = _ranges(voff[end], val[end])
            corner = st["corners"][slot]
            f, k = corner // 3, corner % 3
            skip = (F[f] == other[owner][:, None]).any(1)
            old = P[F[f]]
            new = old.copy()
            new[np.arange(len(f)), k] = p[owner]
            No, Nn = normals(old[:, 0], old[:, 1], old[:, 2]), normals(new[:, 0], new[:, 1], new[:, 2])
            dot = (No[:, 0] * Nn[:, 0] + No[:, 1] * Nn[:, 1]) + No[:, 2] * Nn[:, 2]
            valid &= np.bincount(owner, weights=~(dot > 0) & ~skip, minlength=E) == 0
    idx = np.nonzero(valid)[0]
    rank = np.full(E, RANK_NONE, np.int64)
    rank[idx[np.lexsort((idx, l2[idx], cost[idx]))]] = np.arange(len(idx))
    m1 = np.full(n, RANK_NONE, np.int64)
    np.minimum.at(m1, a[idx], rank[idx])
    np.minimum.at(m1, b[idx], rank[idx])
    m2 = m1.copy()
    np.minimum.at(m2, st["he_u"], m1[st["he_w"]])
    selected = valid & (m2[a] == rank) & (m2[b] == rank)
    chosen = np.nonzero(selected)[0]
    chosen = chosen[np.argsort(rank[chosen])][:max(int(need), 0)]
    selected = np.zeros(E, bool)
    selected[chosen] = True
    newV, remap, keep = V.copy(), np.arange(n), np.ones(n, bool)
    newV[a[chosen]] = p32[chosen]
    remap[b[chosen]] = a[chosen]
    keep[b[chosen]] = False
    G = remap[F]
    fkeep = (G[:, 0] != G[:, 1]) & (G[:, 1] != G[:, 2]) & (G[:, 2] != G[:, 0])
    assert (~fkeep).sum() == 2 * len(chosen)
    index = np.cumsum(keep) - 1
    return {"vertices": newV[keep], "faces": index[G[fkeep]], "edges": ed, "choice": choice, "cost": cost, "l2": l2,
            "valid": valid, "rank": rank, "selected": selected, "collapses": len(chosen)}


# ---------------------------------------------------------------------------------------------- the loop and the stage
def decimate(vertices, faces, target_vertices=1000, regularity=REGULARITY, max_rounds=MAX_ROUNDS, each_round=None):
    """-> {"vertices" fp32, "faces" int64, "rounds", "reached", "collapses"}; each_round(V, F) is called after every round"""
    V, F = check_mesh(vertices, faces)
    collapses = []
    while len(V) > target_vertices and len(collapses) < max_rounds:
        r = collapse_round(V, F, len(V) - target_vertices, regularity)
        collapses.append(r["collapses"])
        V, F = r["vertices"], r["faces"]
        if each_round is not None:
            each_round(V, F)
        if r["collapses"] == 0:
            break
    return {"vertices": V, "faces": F, "rounds": len(collapses), "reached": len(V) <= target_vertices, "collapses": collapses}


def finish_watertight(nets_vertices, nets_faces, snapped_vertices, target_vertices, regularity=REGULARITY, max_rounds=MAX_ROUNDS):
    """the second stage of make_watertight_detail: the snapped nets, decimated unless they meet the budget"""
    if len(nets_vertices) <= target_vertices:
        return {"vertices": snapped_vertices, "faces": np.asarray(nets_faces).astype(np.int64), "rounds": 0, "reached": True,
                "collapses": []}
    return decimate(snapped_vertices, nets_faces, target_vertices, regularity, max_rounds)


def make_watertight_detail(verts, faces, detail_resolution, target_vertices=1000, snap_limit=mref.SNAP_LIMIT, sign="winding"):
    """both stages on the CPU (the NumPy sign search: small sources only)"""
    first = mref.make_watertight(verts, faces, resolution=detail_resolution, snap_limit=snap_limit, sign=sign)
    out = finish_watertight(first["lattice_vertices"], first["faces"], first["vertices"], target_vertices)
    out["detail_vertices"] = len(first["lattice_vertices"])
    return out


# ---------------------------------------------------------------------------------------------- helpers of the tests
def euler(vertices, faces):
    return len(vertices) - 3 * len(faces) // 2 + len(faces)


def min_doubled_area2(vertices, faces):
    P = np.asarray(vertices, F64)
    N = normals(P[faces[:, 0]], P[faces[:, 1]], P[faces[:, 2]])
    return float((N * N).sum(1).min())


def box_field(R, inside):
    """the sign field of `inside(x, y, z)` over the unit box at R cells: corners at (index - 2) / R, R + 5 per axis ->
    (field (nz, ny, nx) int32, origin, pitch)"""
    t = (np.arange(R + 5) - 2.0) / R
    z, y, x = np.meshgrid(t, t, t, indexing="ij")
    return inside(x, y, z).astype(np.int32), np.full(3, -2.0 / R, F32), F32(1.0 / R)


def slab(x, y, z):
    return (np.abs(z - 0.5) < 0.03) & (x > 0) & (x < 1) & (y > 0) & (y < 1)


def mug(x, y, z):
    r = np.hypot(x - 0.4, y - 0.5)
    body = (r < 0.3) & (z > 0.05) & (z < 0.95) & ~((r < 0.26) & (z > 0.1))
    handle = (np.hypot(np.hypot(x - 0.7, z - 0.5) - 0.22, y - 0.5) < 0.035) & (x > 0.68)
    return body | handle


def solid(name):
    """the small closed meshes of the tests -> (V fp32, F int64), outward normals"""
    if name == "tetrahedron":
        v = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]
        f = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]
    elif name == "octahedron":
        v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
        f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    elif name == "cube":
        from tests import volmetrics_ref as vref
        v, f = vref.cube_mesh(np.array([0.013, -0.021, 0.034]), np.array([0.093, 0.059, 0.114]))
    elif name.startswith("icosphere"):
        v, f = mref.icosphere(int(name[-1]))
    else:
        raise KeyError(name)
    V, F = np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int64)
    assert mref.signed_volume(V, F) > 0
    return V, F
