"""Hard silhouette rasteriser (csrc/raster_setup.hip, raster_fwd.hip, raster_lines.hip, raster_sweep.hip): the edge scenes, upstream
gradients and CPU-side helpers shared by tests/test_raster_refs.py (every scene has the property it is there for, on the oracle
alone) and tests/test_raster_edges_gpu.py (kernels against the oracle, exactly).

The reference is the written-out CPU oracle: oracle/csrc/nmr_raster.c (orc_nmr_face_index_map) for coverage and depth,
oracle/csrc/objchain.c (orc_nmr_grad_faces_alpha_exact) for the per-(face, corner) sums `parts`, which include/homan_amd.h
("ORDER-INDEPENDENT SUMS") promises bit for bit.  For the lattice scenes a second reference in integer arithmetic decides the
exact ties without a float.  Numpy restatements of the kernels' bookkeeping (sample boxes, line families, unit composition,
vertex gather) live here as well: they state WHICH path a scene takes, never what a kernel computes on it.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

f32 = np.float32

NEAR, FAR, EPS = 0.1, 100.0, 1e-3              # neural_renderer defaults (homan_amd.ops.NMR_*)
CAND_CAP = 512                                 # csrc/raster_fwd.hip: faces scanned per binning round
RB_PASS = 128                                  # csrc/raster_fwd.hip: candidates per record pass (half per winding class)
SWEEP_UNIT = 256                               # csrc/raster_common.h: items per sweep unit
SWEEP_PASS_FACES = 16                          # csrc/raster_common.h: faces of a unit staged at a time
COMPACT_FACES = 256                            # csrc/raster_lines.hip: face slots per work-list block (one face per thread)
MAX_QUANTA_LOG2 = 45                           # the largest |parts| a case may reach, in quanta: 2^8 inside the header's 2^53

# float32 noise floor of the fused silhouette loss and IoU: the largest relative deviation of the expression
#     loss = sum((keep * img - ref)^2) / sum(keep) / B,   iou = mean_b sum(img_b ref_b) / (sum(clamp(img_b + ref_b, 0, 1)) + 1e-6)
# evaluated with float32 torch on the CPU from its float64 value, over the fused-loss cases FUSED_CASES below (oracle images, both
# upstream weights share them).  Measured by
#     pytest -s tests/test_raster_refs.py -k noise_floor
# which prints every figure and pins this constant from both sides; never taken from a kernel.  The kernel sums the same terms in
# float32 in another order (tile partials, block sums): tests/test_raster_edges_gpu.py allows it util.E32_FACTOR times the floor.
E32_SIL_LOSS = 2.0e-8

Scene = namedtuple("Scene", "name verts faces K S znear zfar")          # verts (B,V,3), faces (F,3) int64, K (B,3,3): torch, CPU

_EYE = torch.eye(3)
_K_ROI = torch.tensor([[2.6, 0, 0.5], [0, 2.6, 0.5], [0, 0, 1.0]])     # tests/test_raster_gpu.py _scene: the object fills ~60 %


def _scene(name, verts, faces, K, S, znear=NEAR, zfar=FAR):
    verts = verts.float().contiguous()
    B = verts.shape[0]
    K = (K[None].expand(B, 3, 3) if K.dim() == 2 else K).float().contiguous()
    return Scene(name, verts, torch.as_tensor(faces).long().contiguous(), K, int(S), float(znear), float(zfar))


@functools.lru_cache(maxsize=None)
def _bottle():
    """the 3000-face bottle, turned as in the scratch poses of the issue -> verts (V,3) float32 torch, faces (F,3) int64 numpy"""
    from homan_amd import synth
    ov, of = synth.bottle_mesh()
    R = torch.tensor(synth._rot_x(1.1) @ synth._rot_y(0.4), dtype=torch.float32)
    return torch.from_numpy(ov).float() @ R, np.asarray(of, np.int64)


# ===================================================================== scenes
LATTICE_ORDERS = ("natural", "permuted", "doubled")
LATTICE_S, LATTICE_STEP = 32, 4


def lattice_nodes():
    """sample indices of the lattice nodes on both axes: 4, 8, .., 60"""
    return np.arange(LATTICE_STEP, 2 * LATTICE_S - LATTICE_STEP + 1, LATTICE_STEP)


def lattice(order="natural"):
    """A planar lattice at z = 1 under K = identity whose nodes lie EXACTLY on sample centres (x = (2 i + 1) / 128 is sample
    column i; image y runs down, so it is sample row 63 - i): every node, edge and diagonal sample is an exact tie of an edge
    function, and vertices sit on integer pixel coordinates.  14 x 14 quads split along one diagonal, F = 392.  `permuted`: a
    seeded permutation of the faces; `doubled`: every face twice, permuted, so every covered sample is an exact depth tie."""
    assert order in LATTICE_ORDERS
    is_ = 2 * LATTICE_S
    n = lattice_nodes()
    x = ((2 * n + 1) / (2.0 * is_)).astype(f32)                     # exact in float32
    X, Y = np.meshgrid(x, x)
    v = np.stack([X.ravel(), Y.ravel(), np.ones(X.size, f32)], 1).astype(f32)
    m, q = len(n), len(n) - 1
    fs = []
    for r in range(q):
        for c in range(q):
            a, b, c_, d = r * m + c, r * m + c + 1, (r + 1) * m + c, (r + 1) * m + c + 1
            fs += [[a, b, d], [a, d, c_]]
    fs = np.array(fs, np.int64)
    if order == "doubled":
        fs = np.concatenate([fs, fs])
    if order != "natural":
        fs = fs[np.random.default_rng(LATTICE_ORDERS.index(order)).permutation(len(fs))]
    return _scene(f"lattice-{order}", torch.from_numpy(v)[None], fs, _EYE, LATTICE_S)


def lattice_integer_index_map(faces):
    """The index map of a lattice scene in integer arithmetic.  A node at sample (column i, row j) has NDC * is = (2 i + 1 - is,
    2 j + 1 - is): the rasteriser's edge functions on those doubled integer coordinates, a sample inside iff none is negative
    (inclusive), back-facing windings skipped, all depths equal: the lowest index of (faces, then their reversed copies) wins."""
    is_ = 2 * LATTICE_S
    n = lattice_nodes()
    m = len(n)
    faces = np.asarray(faces, np.int64)
    F = len(faces)
    col, row = n[faces % m], (is_ - 1) - n[faces // m]              # (F,3) sample column / row of the corners
    X, Y = 2 * col + 1 - is_, 2 * row + 1 - is_
    s = 2 * np.arange(is_) + 1 - is_
    SX, SY = s[None, :], s[:, None]
    idx = np.full((is_, is_), -1, np.int64)
    for fn in range(2 * F - 1, -1, -1):                             # descending: the lowest index is written last
        k = fn % F
        x, y = (X[k], Y[k]) if fn < F else (X[k, ::-1], Y[k, ::-1])
        if (y[2] - y[0]) * (x[1] - x[0]) < (y[1] - y[0]) * (x[2] - x[0]):
            continue
        inside = np.ones((is_, is_), bool)
        for e in range(3):
            e1 = (e + 1) % 3
            inside &= ~((SY - y[e]) * (x[e1] - x[e]) < (SX - x[e]) * (y[e1] - y[e]))
        idx[inside] = fn
    return idx.astype(np.int32)[None]


def triangle_identity(idx, faces):
    """index map -> per sample a key of the owning TRIANGLE (its sorted vertices), whatever its position in the face list"""
    faces = np.asarray(faces, np.int64)
    key = np.sort(faces, 1)
    key = (key[:, 0] * 10 ** 4 + key[:, 1]) * 10 ** 4 + key[:, 2]
    out = idx.astype(np.int64)
    w = out >= 0
    out[w] = key[out[w] % len(faces)]
    return out


def quad_and_cube(S):
    """Two triangles of a slightly skewed quad over ~90 % of the raster at z = 2 with a turned 12-face box in front, F = 14: faces
    over every super-region (the `nloc >= 4` bins of the face setup) and over three or more sweep units (double atomics)."""
    from homan_amd import synth
    q = torch.tensor([[0.05, 0.04, 1.0], [0.97, 0.06, 1.0], [0.95, 0.96, 1.0], [0.03, 0.93, 1.0]]) * 2.0
    cv, cf = synth.box_mesh(1, 1, 1, scale=0.5)
    R = torch.tensor(synth._rot_x(0.5) @ synth._rot_y(0.7), dtype=torch.float32)
    cvt = torch.from_numpy(cv).float() @ R + torch.tensor([0.45, 0.55, 1.0])
    faces = np.concatenate([np.array([[0, 1, 2], [0, 2, 3]], np.int64), np.asarray(cf, np.int64) + 4])
    return _scene(f"quad_and_cube-{S}", torch.cat([q, cvt])[None], faces, _EYE, S)


def crowded(fx):
    """The whole bottle inside one 32 x 32-sample region of a 128^2-sample raster: one bin of 3000 faces (several binning rounds of
    CAND_CAP, several record passes), most faces smaller than a sample, dozens of faces per sweep unit."""
    vb, of = _bottle()
    K = torch.tensor([[fx, 0, 0.37], [0, fx, 0.62], [0, 0, 1.0]])
    return _scene(f"crowded-{fx}", (vb + torch.tensor([0.0, 0.0, 0.6]))[None], of, K, 64)


def border():
    """the bottle over the raster's left and top border"""
    vb, of = _bottle()
    return _scene("border", (vb + torch.tensor([-0.09, 0.08, 0.6]))[None], of, _K_ROI, 32)


NEAR_TZ = (0.11, 0.06)


def near(tz):
    """The bottle through the near plane (tz = 0.11: faces cross znear, none reaches z = 0) and through the camera plane (0.06:
    vertices behind the camera, |NDC| of hundreds)."""
    vb, of = _bottle()
    K = torch.tensor([[0.35, 0, 0.5], [0, 0.35, 0.5], [0, 0, 1.0]])
    return _scene(f"near-{tz}", (vb + torch.tensor([0.03, -0.02, tz]))[None], of, K, 32)


def slab():
    """the centred bottle cut by znear = 0.58 and zfar = 0.63 (per-sample depth test on both sides)"""
    vb, of = _bottle()
    return _scene("slab", (vb + torch.tensor([0.0, 0.0, 0.6]))[None], of, _K_ROI, 32, znear=0.58, zfar=0.63)


def centred():
    vb, of = _bottle()
    return _scene("centred", (vb + torch.tensor([0.0, 0.0, 0.6]))[None], of, _K_ROI, 32)


INSANE_VERTS = {100: [0.01, 0.02, 0.0], 900: [0.0, 0.0, -1e-9], 1300: [0.3, 0.2, 1e-30], 400: [float("nan"), 0.0, 0.6],
                1200: [float("inf"), 0.0, 0.6], 700: [1e20, 0.0, 0.6]}


def insane():
    """The centred bottle with six vertices overwritten: z = 0, z = -1e-9 (z + 1e-9 = 0: projects to inf), z = 1e-30, x = NaN,
    x = inf, x = 1e20.  nr.projection turns every one of them into NaN (its zero distortion coefficients meet an r^6 that
    overflows: 0 * inf), the faces touching them are culled, and the rest of the mesh must come out as if they were not there."""
    sc = centred()
    v = sc.verts.clone()
    for k, p in INSANE_VERTS.items():
        v[0, k] = torch.tensor(p)
    return _scene("insane", v, sc.faces, _K_ROI, 32)


def insane_kept_faces():
    """mask (F,) of the faces that touch none of the overwritten vertices"""
    return ~np.isin(centred().faces.numpy(), list(INSANE_VERTS)).any(1)


NONPOW2_SIZES = (96, 160, 352)


def nonpow2(S):
    """two frames of the bottle as tests/test_raster_gpu.py poses it, at a raster size that is no power of two (the IEEE-division
    paths of unit_body and sweep_item_scale; 3, 5, 11 mask words per line; ragged super-region grids)"""
    from homan_amd import synth
    ov, of = synth.bottle_mesh()
    g = torch.Generator().manual_seed(S)
    B = 2
    ang = torch.rand(B, generator=g) * 6.28
    R = torch.stack([torch.tensor(synth._rot_x(1.1 + 0.1 * i) @ synth._rot_y(float(a)), dtype=torch.float32)
                     for i, a in enumerate(ang)])
    t = torch.tensor([[0.0, 0.0, 0.6]]) + torch.randn(B, 3, generator=g) * 0.01
    verts = torch.from_numpy(ov).float()[None].repeat(B, 1, 1) @ R + t[:, None]
    return _scene(f"nonpow2-{S}", verts, np.asarray(of, np.int64), _K_ROI, S)


MIXED_FRAMES = ("border", "offscreen", "near-0.11", "centred")


def mixed():
    """four frames with a camera each: over the border, everything off screen, through the near plane, plain"""
    off = centred()
    frames = [border(), off._replace(verts=off.verts + torch.tensor([5.0, 0.0, 0.0])), near(0.11), centred()]
    return _scene("mixed", torch.cat([f.verts for f in frames]), frames[0].faces, torch.cat([f.K for f in frames]), 32)


def frame_of(sc, b):
    """frame b of a scene as a scene of its own (B = 1)"""
    return sc._replace(name=f"{sc.name}[{b}]", verts=sc.verts[b:b + 1].contiguous(), K=sc.K[b:b + 1].contiguous())


_BUILDERS = {}
for _o in LATTICE_ORDERS:
    _BUILDERS[f"lattice-{_o}"] = functools.partial(lattice, _o)
for _s in (256, 512):
    _BUILDERS[f"quad_and_cube-{_s}"] = functools.partial(quad_and_cube, _s)
for _f in (0.3, 0.6):
    _BUILDERS[f"crowded-{_f}"] = functools.partial(crowded, _f)
_BUILDERS["border"] = border
for _t in NEAR_TZ:
    _BUILDERS[f"near-{_t}"] = functools.partial(near, _t)
_BUILDERS["slab"] = slab
_BUILDERS["insane"] = insane
for _s in NONPOW2_SIZES:
    _BUILDERS[f"nonpow2-{_s}"] = functools.partial(nonpow2, _s)
_BUILDERS["mixed"] = mixed
SCENES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def scene(name):
    return _BUILDERS[name]()


# ===================================================================== upstream gradients (generic backward, mode 0)
PATTERNS = ("dense", "zero", "negative", "positive", "rim")
ALL_PATTERN_SCENES = ("lattice-natural", "border", "nonpow2-96")          # every pattern; the other scenes run `dense`
COARSE_CASE = ("border", -24)                                             # unscaled randn on the grid 2^-24
FUSED_CASES = ("border", "nonpow2-96")
FUSED_WEIGHTS = (3.0, -0.7)


# log2 of the scale of `dense` and its kin: 2^-10, smaller where long sweeps (large faces, large rasters) or the lattice's many
# exact zero distances (|term| = |g| / eps) would take max |parts| beyond MAX_QUANTA_LOG2 - tests/test_raster_refs.py prints every
# case's figure.  Powers of two: the terms scale exactly.
SCALE_LOG2 = {"quad_and_cube-256": -14, "quad_and_cube-512": -16, "nonpow2-352": -13,
              "lattice-natural": -12, "lattice-permuted": -12, "lattice-doubled": -12}


def upstream(pattern, B, S, scale_log2=-10, seed=5):
    """dL/d silhouette (B,S,S) float32.  dense: randn * 2^scale_log2 (the scale keeps every exact sum far inside its range, see
    MAX_QUANTA_LOG2); negative / positive: -|dense| / +|dense| (one sweep plane stays empty); rim: non-zero in the outer pixel
    ring only, corners included (sources at bit 0 and bit is - 1 of the line words); coarse: unscaled randn."""
    g = torch.randn(B, S, S, generator=torch.Generator().manual_seed(seed))
    if pattern == "coarse":
        return g
    g = g * 2.0 ** scale_log2
    if pattern == "dense":
        return g
    if pattern == "zero":
        return torch.zeros(B, S, S)
    if pattern == "negative":
        return -g.abs()
    if pattern == "positive":
        return g.abs()
    if pattern == "rim":
        ring = torch.zeros(S, S, dtype=torch.bool)
        ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
        return g * ring
    raise ValueError(pattern)


def upstream_for(name, pattern):
    """the upstream gradient of (scene, pattern) as both test files use it"""
    sc = scene(name)
    return upstream(pattern, sc.verts.shape[0], sc.S, SCALE_LOG2.get(name, -10))


def patterns_of(name):
    return PATTERNS if name in ALL_PATTERN_SCENES else ("dense",)


def sample_gradient_generic(gimg):
    """(B,S,S) dL/d pooled -> (B,2S,2S) dL/d alpha on the rasteriser's unflipped sample grid: 0.25 * g (2x2 average pool), flipped"""
    g = np.asarray(gimg, f32) * f32(0.25)
    return np.ascontiguousarray(np.repeat(np.repeat(g, 2, 1), 2, 2)[:, ::-1], f32)


# ===================================================================== the oracle side
def project(sc):
    """oracle projection of a scene -> (B,F,9) float32 NDC faces (mesh faces only)"""
    from oracle import nmr
    B = sc.verts.shape[0]
    with np.errstate(all="ignore"):
        ndc = nmr.projection(sc.verts, sc.K, _EYE[None], torch.zeros(1, 3), torch.zeros(1, 5), 1)
        return nmr.vertices_to_faces(ndc, sc.faces[None].expand(B, -1, -1)).reshape(B, -1, 9).numpy()


def fill_back(faces9):
    """(B,F,9) -> (B,2F,9): the mesh faces, then their reversed copies"""
    B, F = faces9.shape[:2]
    f = faces9.reshape(B, F, 3, 3)
    return np.ascontiguousarray(np.concatenate([f, f[:, :, ::-1]], 1).reshape(B, 2 * F, 9), f32)


def oracle_maps(faces9, S, znear=NEAR, zfar=FAR):
    """-> (both (B,2F,9), idx (B,2S,2S) int32, depth (B,2S,2S) float32 [zfar where empty])"""
    from oracle import clib
    both = fill_back(faces9)
    B, NF = both.shape[:2]
    idx = np.empty((B, 2 * S, 2 * S), np.int32)
    dep = np.empty((B, 2 * S, 2 * S), f32)
    clib.lib().orc_nmr_face_index_map(clib.fptr(both), B, NF, 2 * S, znear, zfar, clib.iptr(idx), clib.fptr(dep))
    return both, idx, dep


def oracle_parts(both, idx, grad_alpha, eps=EPS, log2q=0):
    from oracle import objchain
    return objchain.pseudo_gradient_exact(both, idx, np.ascontiguousarray(grad_alpha, f32), both.shape[1] // 2, eps, log2q)


def pool_alpha(idx):
    """flip + 2x2 average pool of the coverage (exact: quarters) -> (B,S,S) float32"""
    a = (idx >= 0).astype(f32)[:, ::-1]
    n = a.shape[1] // 2
    a4 = a.reshape(a.shape[0], n, 2, n, 2)
    return f32(0.25) * (((a4[:, :, 0, :, 0] + a4[:, :, 0, :, 1]) + a4[:, :, 1, :, 0]) + a4[:, :, 1, :, 1])


def pool_depth(dep):
    """flip + 2x2 pool of the depth map in the epilogue's order (((z0 + z1) + z2) + z3) / 4 -> (B,S,S) float32"""
    d = np.ascontiguousarray(dep[:, ::-1], f32)
    n = d.shape[1] // 2
    d4 = d.reshape(d.shape[0], n, 2, n, 2)
    return (((d4[:, :, 0, :, 0] + d4[:, :, 0, :, 1]) + d4[:, :, 1, :, 0]) + d4[:, :, 1, :, 1]) / f32(4.0)


def quanta_log2(parts, log2q):
    """log2 of max |parts| in quanta of 2^log2q (0 = the default grid 2^-44); -inf for all-zero sums"""
    m = float(np.abs(parts).max())
    return float(np.log2(m)) - (log2q if log2q else -44) if m > 0 else -np.inf


def gather_ref(parts, faces, verts, K, orig_size=1.0):
    """k_bwd_gather restated: per vertex the (exact, float64) sum of its corners' parts, rounded to float32 -> grad_ndc (B,V,3);
    then the projection backward in float32, operation by operation in the kernel's order -> grad_verts (B,V,3).  Vertices whose
    projection backward overflows or is undefined come out non-finite here: the caller compares the finite ones."""
    B, V = verts.shape[:2]
    flat = np.asarray(faces, np.int64).reshape(-1)
    s = np.zeros((B, V, 2), np.float64)
    for b in range(B):
        np.add.at(s[b], flat, parts[b].reshape(-1, 2))              # exact: multiples of the quantum far inside 2^53
    gu, gv = s[..., 0].astype(f32), s[..., 1].astype(f32)
    ndc = np.stack([gu, gv, np.zeros_like(gu)], -1)
    v, k = np.asarray(verts, f32), np.asarray(K, f32)
    two = f32(2.0) / f32(orig_size)
    with np.errstate(all="ignore"):
        zz = v[..., 2] + f32(1e-9)
        du0, dv0 = gu * two, (-gv) * two
        dxn = k[:, None, 0, 0] * du0 + k[:, None, 1, 0] * dv0
        dyn = k[:, None, 0, 1] * du0 + k[:, None, 1, 1] * dv0
        gverts = np.stack([dxn / zz, dyn / zz, -(dxn * v[..., 0] + dyn * v[..., 1]) / (zz * zz)], -1).astype(f32)
    return ndc, gverts


# ===================================================================== which path a scene takes (restated bookkeeping)
def topix(v, is_):
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        return f32(0.5) * ((v * f32(is_) + f32(is_)) - f32(1.0))


def sample_boxes(faces9, S):
    """the face setup's sample boxes -> (x0, y0, x1, y1, live) per (B,F): live = some winding faces the camera, the box is on
    screen, finite and not empty"""
    is_ = 2 * S
    f = faces9.reshape(*faces9.shape[:2], 3, 3)
    with np.errstate(all="ignore"):
        px, py = topix(f[..., 0], is_), topix(f[..., 1], is_)
        xmin, xmax, ymin, ymax = px.min(-1), px.max(-1), py.min(-1), py.max(-1)
        ok = (xmax >= -2) & (ymax >= -2) & (xmin <= is_ + 1) & (ymin <= is_ + 1)
        ok &= (np.abs(f[..., :2]) <= f32(1e15)).all((-1, -2))
        lo =lambda a: np.maximum(0, np.ceil(np.maximum(np.nan_to_num(a, nan=0.0), f32(-2.0)) - f32(0.01))).astype(np.int64)
        hi = lambda a: np.minimum(is_ - 1, np.floor(np.minimum(np.nan_to_num(a, nan=0.0), f32(is_ + 1.0)) + f32(0.01))).astype(np.int64)
        x0, x1, y0, y1 = lo(xmin), hi(xmax), lo(ymin), hi(ymax)
    live = ok & (x1 >= x0) & (y1 >= y0)          # (one winding of every face faces the camera; both, if its area is zero)
    return x0, y0, x1, y1, live


def sr_shift(is_):
    return 6 if is_ <= 512 else 7


def family_counts(both, S):
    """sweep_family restated: items of the twelve (winding, edge, axis) line families -> (B,2F) int64 items per winding"""
    is_ = 2 * S
    f = both.reshape(*both.shape[:2], 3, 3)
    px, py = topix(f[..., 0], is_), topix(f[..., 1], is_)
    n = np.zeros(both.shape[:2], np.int64)
    with np.errstate(all="ignore"):
        for e in range(3):
            for a in (px, py):
                a0, a1 = a[..., e], a[..., (e + 1) % 3]
                lo = np.maximum(np.ceil(np.minimum(a0, a1)), f32(0.0))
                hi = np.trunc(np.minimum(np.maximum(a0, a1), f32(is_ - 1.0)))
                c = np.where(a0 != a1, np.maximum(0, hi - lo + 1), 0)
                n += np.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64)
    return n


def face_items(both, idx, S):
    """items of every mesh face in the sweep work list: the families of its windings that own a sample -> (B,F) int64"""
    B, NF = both.shape[:2]
    own = np.zeros((B, NF), bool)
    for b in range(B):
        u = np.unique(idx[b])
        own[b, u[u >= 0]] = True
    items = np.where(own, family_counts(both, S), 0)
    return items[:, :NF // 2] + items[:, NF // 2:], own


def unit_face_counts(items):
    """The compaction restated: face slots in order, COMPACT_FACES per block, a block's items laid end to end from a unit
    boundary (its total padded to SWEEP_UNIT) -> number of faces with an item in every unit, over all blocks."""
    flat = items.reshape(-1)
    counts = []
    for s in range(0, len(flat), COMPACT_FACES):
        n = flat[s:s + COMPACT_FACES]
        n = n[n > 0]
        if not len(n):
            continue
        end = np.cumsum(n)
        first, last = (end - n) // SWEEP_UNIT, (end - 1) // SWEEP_UNIT
        for u in range(int(last[-1]) + 1):
            counts.append(int(((first <= u) & (last >= u)).sum()))
    return np.asarray(counts, np.int64)


# ===================================================================== fused loss (ops.silhouette_loss)
def fused_masks(sc):
    """keep / ref masks of a fused-loss case: the oracle's silhouette of the scene shifted by a few millimetres, thresholded, with
    two ignore bands (keep = 0) through the object: columns [S/8, S/8 + S/16) and rows [S/2, S/2 + S/16) -> keep, ref (B,S,S)
    float32 torch"""
    shifted = sc._replace(verts=sc.verts + torch.tensor([0.006, -0.004, 0.0]))
    _, idx, _ = oracle_maps(project(shifted), sc.S, sc.znear, sc.zfar)
    tm = (torch.from_numpy(pool_alpha(idx)) > 0.5).float()
    S = sc.S
    tm[:, :, S // 8:S // 8 + S // 16] = -1
    tm[:, S // 2:S // 2 + S // 16] = -1
    return (tm >= 0).float(), (tm > 0).float()


def fused_loss_ref(pooled, keep, ref, dtype=torch.float64):
    """loss and IoU of homan/losses.py:183-197 on a pooled image, in `dtype` -> (loss, iou) python floats"""
    img, keep, ref = (torch.as_tensor(x).to(dtype) for x in (pooled, keep, ref))
    B = img.shape[0]
    image = keep * img
    loss = (((image - ref) ** 2).sum() / keep.sum()) / B
    inter = (image * ref).sum((1, 2))
    union = (image + ref).clamp(0, 1).sum((1, 2))
    return float(loss), float((inter / (union + 1e-6)).mean())
