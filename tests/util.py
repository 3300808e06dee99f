"""Shared helpers for the test-suite (golden loading, oracle-backed clip generation)."""
import glob
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_names():
    """Joint-optimisation goldens (the pose-initialisation golden has its own schema, tests/test_poseinit.py)."""
    names = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "ref_*.npz")))
    return [n for n in names if not n.startswith("ref_poseinit")]


def load_golden(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    rec = {k: z[k] for k in z.files}
    inputs = {k[3:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("in_") and k != "in_camintr"}
    weights = {"lw_" + k[3:]: float(v) for k, v in rec.items() if k.startswith("lw_")}
    meta = dict(image_size=int(rec["meta_image_size"]), steps=int(rec["meta_steps"]),
                optimize_object_scale=bool(rec["meta_optimize_object_scale"]),
                optimize_mano=bool(rec["meta_optimize_mano"]), lr=float(rec["meta_lr"]),
                hand_sides=[str(x) for x in rec["meta_hand_sides"]] if "meta_hand_sides" in rec else ["right"],
                inter_type=str(rec["meta_inter_type"]) if "meta_inter_type" in rec else "centroid",
                has_trajectory="evo_loss" in rec)
    return rec, inputs, rec["in_camintr"], weights, meta


def model_kwargs(inputs, camintr, meta):
    kw = dict(inputs)
    kw.update(hand_sides=list(meta["hand_sides"]), camintr=camintr, class_name="default", int_scale_init=1,
              hand_proj_mode="persp", optimize_mano=meta["optimize_mano"], optimize_mano_beta=True,
              optimize_object_scale=meta["optimize_object_scale"], image_size=meta["image_size"],
              inter_type=meta["inter_type"])
    return kw


def oracle_clip_fns(mano_model):
    """(silhouette_fn, hand_verts_fn) backed by the CPU oracle, for homan_amd.synth.make_clip."""
    from homan_amd.mano_assets import hand_models
    from oracle import lbs, nmr
    layers = {side: lbs.ManoLayer(m, num_pca_comps=16, flat_hand_mean=False) for side, m in hand_models(mano_model).items()}

    def hand_fn(pca, rot, betas, side="right"):
        layer = layers[side]
        hp = pca[:, :16] @ layer.hand_components
        if side == "left":          # homan/manomodel.py:131-132, applied before the mean pose is added
            hp = hp.clone()
            hp[:, 1::3] *= -1
            hp[:, 2::3] *= -1
        return layer(betas=betas, global_orient=rot, hand_pose=hp, transl=torch.zeros(len(rot), 3))[0]

    def sil_fn(verts, faces, K, size):
        r = nmr.Renderer(image_size=size, K=K, R=torch.eye(3)[None], t=torch.zeros(1, 3), orig_size=1)
        return r(verts, faces, mode="silhouettes")

    return sil_fn, hand_fn


# ===================================================================== depth term: float64 references and shared inputs
# (tests/test_depth_oracle.py checks the references against the CPU oracle; tests/test_depth_edges_gpu.py the kernels against them)
def ordinal_depth_ref(masks, sils, depths):
    """Ordinal depth term (reference homan/lossutils.py:133-169 as oracle/model.py words it: n layers, every ordered pair, one
    normaliser) in float64 torch.  masks (B,n,H,W) bool; sils: n x (B,S,S) bool ("fully covered"); depths: n x (B,S,S), any float
    type, differentiable: the clamp's backward (inclusive bounds) is torch's own.  -> 0-d float64 (NaN for a clip without pairs)."""
    depths = [d.double() for d in depths]
    loss = torch.zeros((), dtype=torch.float64, device=depths[0].device)
    num_pairs = 0
    for i in range(len(sils)):
        for j in range(len(sils)):
            has_pred = sils[i] & sils[j]
            pairs = int((has_pred.flatten(1).sum(1) > 0).sum())
            if pairs == 0:
                continue
            num_pairs += pairs
            mask = masks[:, i] & ~masks[:, j] & (depths[j] < depths[i]) & has_pred
            n = int(mask.sum())
            if n == 0:
                continue
            dists = torch.clamp(depths[i] - depths[j], min=0.0, max=2.0)
            loss = loss + torch.log(1 + torch.exp(dists))[mask].sum() / n
    return loss / num_pairs


def depth_backward_ref(faces9, idx_map, grad_depth, faces, verts, K, orig_size):
    """Backward of the pooled depth image (NMR backward_depth_map, the formula that heads csrc/raster_depth.hip) in float64 numpy.
    faces9 (B,F,9) NDC face vertices and idx_map (B,2S,2S) sample owners (face, F + face = reversed winding, -1 = none) as the
    forward left them; grad_depth (B,S,S); faces (F,3) mesh topology; verts (B,V,3) camera space; K (B,3,3).  Per owned sample
    with zp its depth and w_k its clamped, renormalised barycentrics: A_k += g zp^2 w_k; per (face, winding)
    d(x,y)_k = -A_k tmp[l] is / 2, dz_k = A_k / z_k^2, tmp[l] = -sum_m inv[m][l] / z_m; then the gather to mesh vertices and the
    projection backward.  -> (B,V,3) float64.  NOT the derivative of the forward depth (see tests/test_depth_oracle.py)."""
    f9 = np.asarray(faces9, np.float64)
    idx = np.asarray(idx_map)
    g = np.asarray(grad_depth, np.float64)
    faces = np.asarray(faces, np.int64)
    verts, K = np.asarray(verts, np.float64), np.asarray(K, np.float64)
    B, F = f9.shape[:2]
    V, is_ = verts.shape[1], idx.shape[1]
    f9 = f9.reshape(B, F, 3, 3)
    fd = np.concatenate([f9, f9[:, :, ::-1]], 1)                    # (B,2F,3,3): both windings, corners in winding order
    p = 0.5 * (fd[..., :2] * is_ + is_ - 1)
    z = fd[..., 2]
    (x0, y0), (x1, y1), (x2, y2) = [(p[..., k, 0], p[..., k, 1]) for k in range(3)]
    inv = np.stack([np.stack([y1 - y2, x2 - x1, x1 * y2 - x2 * y1], -1),
                    np.stack([y2 - y0, x0 - x2, x2 * y0 - x0 * y2], -1),
                    np.stack([y0 - y1, x1 - x0, x0 * y1 - x1 * y0], -1)], -2)            # (B,2F,3,3)
    den = x2 * (y0 - y1) + x0 * (y1 - y2) + x1 * (y2 - y0)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = inv / den[..., None, None]
    bi, yi, xi = np.nonzero(idx >= 0)
    gs = 0.25 * g[bi, (is_ - 1 - yi) >> 1, xi >> 1]                 # vertical flip + 2x2 average pool, backwards
    keep = gs != 0
    bi, yi, xi, gs = bi[keep], yi[keep], xi[keep], gs[keep]
    fn = idx[bi, yi, xi]
    I = inv[bi, fn]
    w = np.clip(I[:, :, 0] * xi[:, None] + I[:, :, 1] * yi[:, None] + I[:, :, 2], 0.0, 1.0)
    ws = w.sum(1)
    zp = ws / (w / z[bi, fn]).sum(1)
    contrib = (gs * zp * zp / ws)[:, None] * w
    slot = bi * 2 * F + fn
    A = np.stack([np.bincount(slot, contrib[:, k], minlength=B * 2 * F) for k in range(3)], -1).reshape(B, 2 * F, 3)
    with np.errstate(invalid="ignore"):
        tmp = -(inv[..., :2] / z[..., None]).sum(-2)                # (B,2F,2)
        gf = np.concatenate([-A[..., None] * tmp[..., None, :] * (is_ / 2.0), (A / (z * z))[..., None]], -1)     # (B,2F,3,3)
    gf[A == 0] = 0.0                                                # (windings that own nothing, degenerate ones included)
    gc = gf[:, :F] + gf[:, F:, ::-1]                                # winding order -> mesh corners
    gn = np.zeros((B, V, 3))
    np.add.at(gn, (np.arange(B)[:, None, None], faces[None]), gc)
    du0, dv0 = gn[..., 0] * (2.0 / orig_size), -gn[..., 1] * (2.0 / orig_size)
    zz = verts[..., 2] + 1e-9
    dxn = K[:, None, 0, 0] * du0 + K[:, None, 1, 0] * dv0
    dyn = K[:, None, 0, 1] * du0 + K[:, None, 1, 1] * dv0
    return np.stack([dxn / zz, dyn / zz, -(dxn * verts[..., 0] + dyn * verts[..., 1]) / (zz * zz) + gn[..., 2]], -1)


def deviation(got, want):
    """max |got - want| / max |want| (0 if both are zero throughout)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max()
    diff = np.abs(got - want).max()
    return diff / scale if scale > 0 else diff


# Meshes x frames x sizes of the depth-backward grid: synth.box_mesh dims -> (V, frames).  Frames are chosen by the 256-thread
# workgroups of the vertex gather: V = 8 and 26 put nine or more frames into a workgroup, 44 five to six, 98 two to three.
DEPTH_BWD_MESHES = {(1, 1, 1): (8, 40), (2, 2, 2): (26, 24), (3, 3, 2): (44, 12), (4, 4, 4): (98, 6), (5, 5, 10): (252, 4)}
DEPTH_BWD_SIZES = (64, 128, 256)


def depth_bwd_scene(dims, frames, near=False):
    """A box turning in front of the camera, right of the image centre (it reaches the last 64-pixel segment of its rows) -> verts (B,V,3) float32, faces (F,3) int32, K (B,3,3) float32 (orig_size 1).
    near: large and close, its long faces upright - taller than half the image."""
    from homan_amd import synth
    v, f = synth.box_mesh(*dims, scale=0.3 if near else 0.16)
    t = np.arange(frames)
    R = np.stack([synth._rot_x(1.3 + (0.0 if near else 0.07 * ti)) @ synth._rot_y(0.45 + 0.11 * ti) for ti in t])
    tr = np.stack([0.12 + 0.01 * np.sin(0.9 * t), 0.02 * np.cos(0.7 * t), np.full(frames, 0.5 if near else 0.6) + 0.01 * (t % 3)], 1)
    verts = np.einsum("vj,bjk->bvk", v.astype(np.float64), R) + tr[:, None]
    fl = 480.0 / 350.0
    K = np.tile(np.array([[fl, 0, 0.5], [0, fl, 0.5], [0, 0, 1.0]], np.float32), (frames, 1, 1))
    return torch.from_numpy(verts.astype(np.float32)), f, torch.from_numpy(K)


def depth_bwd_upstream(pattern, B, S, V, seed=0):
    """Upstream images (B,S,S) float32 of the depth-backward grid, by name (None: the pattern does not exist at this shape)."""
    rng = np.random.default_rng([seed, B, S, V])
    g = np.zeros((B, S, S), np.float32)
    if pattern == "zero":
        pass
    elif pattern == "dense":
        g[:] = rng.normal(size=g.shape)
    elif pattern == "last_frame_pixel":
        g[B - 1, S // 2, int(0.774 * S)] = 0.7             # (the box sits right of the centre: depth_bwd_scene)
    elif pattern == "late_frames":          # frames that are the ninth or later of a gather workgroup
        late = set()
        for w in range((B * V + 255) // 256):
            b_lo, b_hi = 256 * w // V, min(256 * w + 255, B * V - 1) // V
            late.update(range(b_lo + 8, b_hi + 1))
        if not late:
            return None
        for b in sorted(late):
            g[b] = rng.normal(size=(S, S))
    elif pattern == "last_segment":
        g[:, :, S - 64:] = rng.normal(size=(B, S, 64))
    elif pattern == "band":
        g[::2, S // 2 - 2:S // 2 + 1] = rng.normal(size=g[::2, :3].shape)
    else:
        raise ValueError(pattern)
    return g


DEPTH_BWD_PATTERNS = ("zero", "dense", "last_frame_pixel", "late_frames", "last_segment", "band")


# ---- synthetic layer images of the ordinal term
ORD_BOUND_X = (1e-6, 1.0, float(np.nextafter(np.float32(2), np.float32(0))), 2.0, float(np.nextafter(np.float32(2), np.float32(3))),
               5.0, 0.0)


def ordinal_scene(B, S, kind="mixed", seed=0):
    """-> dict(d=[d0, d1] float32 depth images, a=[a0, a1] float32 silhouette values (1 = covered), m=[m0, m1] uint8 masks), numpy.
    kind: "mixed" - both layers cover most pixels, annotation and depth order random per pixel, so both directions occur; rows
          0-1 of every frame hold the depth differences of ORD_BOUND_X (front depth 0, so the difference is exact in float32);
          frames 1 / 2 / 3 (where they exist) lack layer 0 / layer 1 / both; a quarter of the pixels has silhouette 0.75 or 0;
          "one_direction" - as mixed, but layer 1 is annotated nowhere (no pixel of the second kind);
          "no_pairs" - no pixel fully covered in either layer;
          "full_clamped" - every pixel covered by both, annotated layer 0, layer 1 in front by 3 (clamped to 2)."""
    rng = np.random.default_rng([seed, B, S])
    shp = (B, S, S)
    if kind == "full_clamped":
        one = np.ones(shp, np.float32)
        return dict(d=[4.0 * one, one.copy()], a=[one.copy(), one.copy()], m=[np.ones(shp, np.uint8), np.zeros(shp, np.uint8)])
    base = rng.uniform(0.5, 3.0, shp)
    x = np.where(rng.random(shp) < 0.7, rng.uniform(0.01, 1.98, shp), rng.uniform(2.02, 4.0, shp))
    sign = np.where(rng.random(shp) < 0.5, -1.0, 1.0)
    d0 = base.astype(np.float32)
    d1 = (base + sign * x).astype(np.float32)
    nb = len(ORD_BOUND_X)
    cols = np.arange(S)
    for r, (back, front) in enumerate(((d0, d1), (d1, d0))):      # row 0: layer 0 behind by x ; row 1: layer 1 behind by x
        back[:, r, :] = np.asarray(ORD_BOUND_X, np.float32)[cols % nb]
        front[:, r, :] = 0.0
    a = [np.where(rng.random(shp) < 0.75, 1.0, np.where(rng.random(shp) < 0.5, 0.75, 0.0)).astype(np.float32) for _ in range(2)]
    for l in range(2):
        a[l][:, :2] = 1.0
    m0 = (rng.random(shp) < 0.5).astype(np.uint8)
    m1 = np.where(rng.random(shp) < 0.8, 1 - m0, m0).astype(np.uint8)     # mostly exclusive; some pixels both or neither
    m0[:, 0], m1[:, 0] = 1, 0                                      # bound rows: annotated in front = rendered behind
    m0[:, 1], m1[:, 1] = 0, 1
    if kind == "one_direction":
        m1[:] = 0
    elif kind == "no_pairs":
        a = [np.minimum(ai, 0.75) for ai in a]
    elif kind != "mixed":
        raise ValueError(kind)
    if kind != "no_pairs":
        if B > 1:
            a[0][1] = np.minimum(a[0][1], 0.75)
        if B > 2:
            a[1][2] = 0.0
        if B > 3:
            a[0][3], a[1][3] = 0.0, np.minimum(a[1][3], 0.75)
    return dict(d=[d0, d1], a=a, m=[m0, m1])


def assert_ordinal_scene_has_no_near_ties(sc):
    """away from the deliberate bound rows (0-1), every depth difference is >= 1e-3 from 0 and from the clamp's 2 (float64)"""
    d0, d1 = sc["d"][0].astype(np.float64), sc["d"][1].astype(np.float64)
    x = np.abs(d0 - d1)[:, 2:]
    for d2 in sc["d"][2:]:                                          # a third layer is compared with layer 0 only (it never meets 1)
        x = np.concatenate([x, np.abs(d0 - d2.astype(np.float64))[:, 2:]])
    if x.size:
        assert x.min() >= 1e-3 and np.abs(x - 2.0).min() >= 1e-3
    xb = np.abs(d0 - d1)[:, :2]
    assert np.isin(xb.astype(np.float32), np.asarray(ORD_BOUND_X, np.float32)).all()       # the bound rows hold exactly those


def ordinal_ref_on_scene(sc):
    """float64 reference on an `ordinal_scene`: -> (loss (0-d, float64), [g0, g1] float64 gradients w.r.t. the depth images,
    zeros where the loss is NaN / has no gradient)"""
    d = [torch.from_numpy(x).double().requires_grad_(True) for x in sc["d"]]
    sils = [torch.from_numpy(x) == 1 for x in sc["a"]]
    masks = torch.stack([torch.from_numpy(x) != 0 for x in sc["m"]], 1)
    loss = ordinal_depth_ref(masks, sils, d)
    if loss.requires_grad and bool(torch.isfinite(loss)):
        loss.backward()
    return loss.detach(), [x.grad if x.grad is not None else torch.zeros_like(x) for x in d]


# (B, S, kind) of the ordinal-term cases, CPU (reference vs oracle) and GPU (kernels vs reference) alike
ORDINAL_CASES = [(1, 64, "mixed"), (5, 64, "mixed"), (5, 64, "one_direction"), (256, 64, "mixed"), (257, 64, "mixed"),
                 (300, 64, "mixed"), (300, 64, "one_direction"), (3, 96, "mixed"), (2, 350, "mixed"), (2, 1024, "full_clamped")]


def oracle_depth_backward(verts, faces, K, size, grad_depth):
    """The CPU oracle (float32) on a depth-backward scene -> (vertex gradients (B,V,3), faces9 (B,F,9), idx_map (B,2S,2S))."""
    from oracle import nmr
    B, F = verts.shape[0], faces.shape[0]
    r = nmr.Renderer(image_size=size, K=K, R=torch.eye(3)[None], t=torch.zeros(1, 3), orig_size=1)
    vo = verts.clone().requires_grad_(True)
    f = r._ndc_faces(vo, torch.from_numpy(faces)[None].repeat(B, 1, 1), None, None, None, None, None)
    _, depth, idx = nmr.rasterize_alpha_depth(f, size, True, r.near, r.far, r.rasterizer_eps)
    (depth * torch.from_numpy(grad_depth)).sum().backward()
    return vo.grad.numpy(), f[:, :F].detach().reshape(B, F, 9).numpy(), idx.numpy()


# float32 noise floors: the largest deviation (max |difference| / max |reference|) of the float32 CPU oracle from the float64
# references above, over every case of tests/test_depth_oracle.py::test_ordinal_depth_ref_matches_the_oracle (loss value and both
# gradient images; largest: the gradients of the 257-frame clip, 2.34e-7) and ::test_depth_backward_ref_matches_the_oracle
# (largest: 252-vertex box, S = 128, dense upstream image, 1.25e-3 - the oracle adds a face's samples one by one in float32 and
# a dense random image makes them cancel; images with few non-zero pixels give 5e-7 .. 2.5e-4).  Measured with those two tests
# (they print every figure and pin these constants from both sides); never taken from a kernel.  The kernels sum the same terms
# in float32 in another order: tests/test_depth_edges_gpu.py allows them E32_FACTOR times the floor.
E32_ORDINAL = 2.4e-7
E32_DEPTH_BWD = 1.25e-3
E32_FACTOR = 4.0


def ordinal_scene3(B=6, S=64, seed=1):
    """Three layers: 0 and 1 as in a mixed `ordinal_scene`; layer 2 covers only pixels layer 1 does not cover (the two never meet),
    is absent from the odd frames, and lies in front of or behind layer 0 at random with random annotation.  -> as ordinal_scene"""
    sc = ordinal_scene(B, S, "mixed", seed)
    rng = np.random.default_rng([seed, B, S, 3])
    shp = (B, S, S)
    x = np.where(rng.random(shp) < 0.7, rng.uniform(0.01, 1.98, shp), rng.uniform(2.02, 4.0, shp))
    d2 = (sc["d"][0].astype(np.float64) + np.where(rng.random(shp) < 0.5, -1.0, 1.0) * x).astype(np.float32)
    a2 = np.where((sc["a"][1] != 1) & (rng.random(shp) < 0.8), 1.0, 0.5).astype(np.float32)
    a2[1::2] = 0.0
    m2 = (rng.random(shp) < 0.3).astype(np.uint8)
    return dict(d=sc["d"] + [d2], a=sc["a"] + [a2], m=sc["m"] + [m2])


# ===================================================================== pair terms: references and shared scenes
# (tests/test_pairterms_refs.py checks the references against the CPU oracle and measures the float32 floors;
#  tests/test_pairterms_edges_gpu.py holds the kernels of csrc/pair_bodies.h, contact.hip and sdf.hip against them)
NN_SHAPES = [(1, 1), (1, 64), (1, 4097), (64, 3), (64, 65), (64, 4096), (127, 63), (127, 257), (128, 64), (128, 4097), (129, 1),
             (129, 65), (129, 257), (778, 3), (778, 4096), (778, 4097)]          # (Vh, Vo): every value of either axis of the grid


def nn_bruteforce32(vh, vo):
    """Nearest object vertex of every hand vertex in float32, d2 = ((ox-hx)^2 + (oy-hy)^2) + (oz-hz)^2 with every operation
    rounded (numpy does not contract), first argmin.  vh (B,Vh,3), vo (B,Vo,3) float32 numpy -> idx (B,Vh) int64, d2 (B,Vh)
    float32, metric = max_b sqrt32(min_i d2) float32."""
    vh, vo = np.asarray(vh, np.float32), np.asarray(vo, np.float32)
    d = [vo[:, None, :, c] - vh[:, :, None, c] for c in range(3)]
    d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    assert d2.dtype == np.float32
    idx = d2.argmin(2)
    best = np.take_along_axis(d2, idx[..., None], 2)[..., 0]
    return idx, best, np.sqrt(best.min(1)).max()


def nn_clouds(B, Vh, Vo, seed=0):
    """random float32 clouds, the object's next to the hand's (some hand vertices inside it)"""
    rng = np.random.default_rng([seed, B, Vh, Vo])
    vh = (rng.normal(size=(B, Vh, 3)) * 0.04 + [0.02, 0.0, 0.6]).astype(np.float32)
    vo = (rng.normal(size=(B, Vo, 3)) * 0.05 + [0.0, 0.0, 0.62]).astype(np.float32)
    return vh, vo


def nn_tie_clouds(B, Vh, Vo, seed=0):
    """Coordinates on multiples of 1/4 in [0, 1] (a lattice of 125 points, every squared distance exact in float32): an object
    of several hundred vertices holds each point many times over and every hand vertex has its minimum at many indices."""
    rng = np.random.default_rng([seed, B, Vh, Vo, 7])
    vh = (rng.integers(0, 5, size=(B, Vh, 3)) / 4.0 + 1.0 / 64.0).astype(np.float32)      # (off the object's lattice by 1/64)
    vo = (rng.integers(0, 5, size=(B, Vo, 3)) / 4.0).astype(np.float32)
    return vh, vo


def nn_tie_spread(d2, waves=4):
    """How the equal minima of exact squared distances d2 (B,Vh,Vo) fall on the full search's layout (csrc/pair_bodies.h: wave q
    scans the contiguous share [q s, (q+1) s), s = ceil(Vo / waves), 64 at a time) -> (hand vertices whose minimum lies in more
    than one wave's share, hand vertices with it in more than one 64-group of a single share)"""
    Vo = d2.shape[2]
    share = -(-Vo // waves)
    at_min = d2 == d2.min(2, keepdims=True)
    j = np.arange(Vo)
    wave, group = j // share, (j % share) // 64
    in_wave = np.stack([(at_min & (wave == q)).any(2) for q in range(waves)])
    two_groups = np.zeros(d2.shape[:2], bool)
    for q in range(waves):
        two_groups |= np.stack([(at_min & (wave == q) & (group == g)).any(2) for g in range(group.max() + 1)]).sum(0) >= 2
    return int((in_wave.sum(0) >= 2).sum()), int(two_groups.sum())


# ---- contact
CONTACT_THRESH = 0.02
CONTACT_VO = (1, 64, 4096, 4097, 9000)       # one range | one range, full | two ranges with a tail of one | three ranges
CONTACT_VH = (1, 255, 257, 778)
CONTACT_B = (1, 3)


def contact_scene(B, Vh, Vo, kind="random", seed=0, zeros=0):
    """-> vh (B,Vh,3), vo (B,Vo,3) float32, nn (B,Vh) int32.  The picks are GIVEN (no search, no near-tie ambiguity) and the hand
    vertex sits at distance thresh * 10^U(-4, log10 20) from its pick: a / thresh log-uniform over [1e-4, 20], the linear end and
    full saturation.  kind: "random" picks | "same" every vertex picks one object vertex | "last_range" picks >= 4096 * (ranges - 1).
    zeros: that many hand vertices per frame coincide with their pick (a == 0)."""
    rng = np.random.default_rng([seed, B, Vh, Vo, len(kind)])
    vo = (rng.normal(size=(B, Vo, 3)) * 0.05 + [0.0, 0.0, 0.6]).astype(np.float32)
    if kind == "random":
        nn = rng.integers(0, Vo, size=(B, Vh))
    elif kind == "same":
        nn = np.full((B, Vh), min(17, Vo - 1))
    elif kind == "last_range":
        nn = rng.integers(4096 * ((Vo - 1) // 4096), Vo, size=(B, Vh))
    else:
        raise ValueError(kind)
    u = rng.normal(size=(B, Vh, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    r = CONTACT_THRESH * 10.0 ** rng.uniform(-4.0, np.log10(20.0), size=(B, Vh, 1))
    if Vh >= 2:
        r[:, 0], r[:, 1] = CONTACT_THRESH * 1e-4, CONTACT_THRESH * 20.0         # both ends are there
    picked = np.take_along_axis(vo, nn[..., None].repeat(3, -1), 1)
    vh = (picked.astype(np.float64) + r * u).astype(np.float32)
    for z in range(zeros):
        vh[:, (3 + 5 * z) % Vh] = picked[:, (3 + 5 * z) % Vh]
    return vh, vo, nn.astype(np.int32)


def contact_ref(vh, vo, nn, thresh=CONTACT_THRESH, dtype=torch.float64, clip_len=None):
    """mean_{b,i} thresh tanh(|o_nn - h| / thresh) (reference contactloss.py as executed, csrc/contact.hip) with torch autograd
    for both gradients -> (loss (C,), g_hand, g_obj).  A pair at distance 0 has value 0 and subgradient 0 (the kernels'
    convention; autograd through the norm alone gives NaN there).  clip_len: one mean per clip of that many frames."""
    h = torch.as_tensor(vh).to(dtype).requires_grad_(True)
    o = torch.as_tensor(vo).to(dtype).requires_grad_(True)
    idx = torch.as_tensor(nn).long()
    d = torch.gather(o, 1, idx[..., None].expand(-1, -1, 3)) - h
    a2 = (d * d).sum(-1)
    live = a2 > 0
    a = torch.sqrt(torch.where(live, a2, torch.ones_like(a2)))
    val = torch.where(live, thresh * torch.tanh(a / thresh), torch.zeros_like(a))
    B, Vh = val.shape
    loss = val.reshape(-1, clip_len or B, Vh).mean((1, 2))
    loss.sum().backward()
    return loss.detach(), h.grad, o.grad


# ---- SDF interpenetration
def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32) * 0.0125
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)          # outward


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)      # outward
    return v, f


def _posed(v, B, shift, seed, turn=0.35, wobble=0.004):
    """(V,3) -> (B,V,3) float32: turned by a frame-dependent angle about x and y, moved by `shift` plus a small seeded wobble"""
    from homan_amd import synth
    rng = np.random.default_rng([seed, B, len(v)])
    out = []
    for b in range(B):
        R = synth._rot_x(turn * (b + 1) * 0.7) @ synth._rot_y(turn * (b + 1))
        out.append(v.astype(np.float64) @ R.T + np.asarray(shift) + rng.normal(size=3) * wobble)
    return np.stack(out).astype(np.float32)


def sdf_scenes(mano):
    """name -> (verts0 (B,V0,3), faces0, verts1 (B,V1,3), faces1), float32 / int32 numpy: the closed meshes of the pair-term edge
    tests (each mesh reaches into the other unless said otherwise), and the two scenes of test_ops_gpu.test_collision_vs_oracle."""
    from homan_amd import synth
    hv, hf = mano["v_template"].astype(np.float32), mano["closed_faces"].astype(np.int32)
    tv, tf = tetrahedron()
    b1v, b1f = synth.box_mesh(1, 1, 1)
    bav, baf = synth.box_mesh(4, 4, 6)
    bbv, bbf = synth.box_mesh(1, 1, 32)
    btv, btf = synth.bottle_mesh()
    assert (len(tv), len(tf), len(b1v), len(b1f)) == (4, 4, 8, 12) and len(baf) == 256 and len(bbf) == 260
    ctr = np.array([0.02, -0.01, 0.6])
    sc = {}
    tet, box = _posed(tv, 2, ctr + [0.004, 0.003, 0.01], 1), _posed(b1v, 2, ctr, 2)
    sc["tet_in_box"] = (tet, tf, box, b1f)
    sc["box_around_tet"] = (box, b1f, tet, tf)
    sc["F256_vs_F260"] = (_posed(bav, 2, ctr, 3), baf, _posed(bbv * [0.5, 0.5, 1.0], 2, ctr + [0.006, -0.004, 0.02], 4, turn=0.2), bbf)
    hand = _posed(hv, 2, ctr - [0.02, 0.0, 0.0], 5, turn=0.1)
    sc["hand_vs_box8"] = (hand, hf, _posed(b1v * 1.6, 2, ctr + [0.012, 0.0, 0.0], 6), b1f)
    sc["bottle_vs_hand"] = (_posed(btv, 2, ctr + [0.05, 0.0, 0.01], 7, turn=0.05), btf, hand, hf)
    # tests/test_ops_gpu.py::test_collision_vs_oracle, written out
    g = torch.Generator().manual_seed(4)
    B = 3
    vh = torch.from_numpy(hv)[None].repeat(B, 1, 1) + torch.randn(B, 1, 3, generator=g) * 0.01 + torch.tensor([0.0, 0.0, 0.55])
    vo = torch.from_numpy(btv)[None].repeat(B, 1, 1) + torch.tensor([0.02, 0.0, 0.56]) + torch.randn(B, 1, 3, generator=g) * 0.01
    vh = vh + torch.tensor([0.03, 0.0, 0.0])
    sc["ops_bottle"] = (vh.numpy(), hf, vo.numpy(), btf)
    cv, cf = synth.box_mesh()
    vc = torch.from_numpy(cv)[None].repeat(B, 1, 1) * 1.5 + vh.mean(1, keepdim=True) + torch.tensor([0.01, 0.0, 0.0])
    sc["ops_cube"] = (vh.numpy(), hf, vc.numpy(), cf)
    return {k: tuple(np.ascontiguousarray(x) for x in v) for k, v in sc.items()}


SDF_SCENE_NAMES = ("tet_in_box", "box_around_tet", "F256_vs_F260", "hand_vs_box8", "bottle_vs_hand", "ops_bottle", "ops_cube")
OCTA_SCALE, OCTA_OFFSET, OCTA_INSIDE = 0.125, (0.5, -0.25, 2.0), 5440


def octahedron_scene():
    """Unit octahedron at a power-of-two scale and offset (scale_factor 0: its normalised box is the unit octahedron exactly, the
    voxel centres (odd / 32) sit ON the projected edges |y| + |z| = 1) and a half-size copy inside it.  -> scene tuple, B = 1."""
    v, f = octahedron()
    big = (v * OCTA_SCALE + np.asarray(OCTA_OFFSET, np.float32))[None].astype(np.float32)
    small = (v * (OCTA_SCALE / 2) + np.asarray(OCTA_OFFSET, np.float32))[None].astype(np.float32)
    return big, f, small, f


def octahedron_exact():
    """-> inside (32,32,32) bool [z][y][x], phi (32,32,32) float64 = (1 - |x| - |y| - |z|) / sqrt 3 inside, 0 outside"""
    c = -1.0 + (np.arange(32) + 0.5) / 16.0
    s = np.abs(c)[:, None, None] + np.abs(c)[None, :, None] + np.abs(c)[None, None, :]
    assert not (s == 1).any()
    return s < 1, np.where(s < 1, (1 - s) / np.sqrt(3.0), 0.0)


def frames_scene():
    """B = 4, boxes of 44 and 26 vertices about one unit across: frame 0 overlapping, 1 disjoint, 2 the second wholly inside the
    first, 3 the second 2^20 away (its coordinates stay exact there: multiples of 1/8)."""
    from homan_amd import synth
    av, af = synth.box_mesh(3, 3, 2, scale=2.0)
    bv, bf = synth.box_mesh(2, 2, 2, scale=2.0)
    a = _posed(av, 4, [0.1, -0.2, 3.0], 11, turn=0.1, wobble=0.02)
    b = _posed(bv, 4, [0.1, -0.2, 3.0], 12, turn=0.15, wobble=0.02)
    b[0] += np.float32([0.3, 0.2, 0.25])
    b[1] += np.float32([3.0, 0.0, 0.0])
    b[2] = (0.3 * (b[2] - b[2].mean(0)) + a[2].mean(0)).astype(np.float32)
    cube = np.sign(bv) * np.float32(0.5) * (bv != 0)                   # 26 vertices on {-0.5, 0, 0.5}^3
    b[3] = (cube + np.float32([2.0 ** 20, 0.0, 3.0])).astype(np.float32)
    return a, af, b, bf


SHELL_IX = (-1.0, -0.5, -1e-3, 0.0, 30.999, 31.0, 31.5, 32.0)


def shell_scene():
    """Owner (slot 0): a cube of half-side 1/4 about (0.5, -0.25, 2.0); with scale_factor 0 its normalised box fills the grid
    exactly (every voxel inside, centre and scale powers of two).  Sampled (slot 1): a tetrahedron inside it, plus 24 loose
    vertices (no face uses them) at grid index SHELL_IX on each axis in turn, the other two indices at 10.25 and 17.5 - in the
    zero-padded border shell, on it, and beyond it.  The integer indices are exact in float32.  -> scene tuple (B = 1), and
    the (24, 3) grid indices of the loose vertices."""
    from homan_amd import synth
    bv, bf = synth.box_mesh(1, 1, 1)
    c, s = np.asarray(OCTA_OFFSET, np.float64), 0.25
    owner = (np.sign(bv) * s + c).astype(np.float32)
    tv, tf = tetrahedron()
    ix = []
    for axis in range(3):
        for x in SHELL_IX:
            p = [10.25, 17.5, 10.25]
            p[(axis + 1) % 3], p[axis] = 17.5, x
            ix.append(p)
    ix = np.asarray(ix, np.float64)
    loose = c + s * ((2.0 * ix + 1.0) / 32.0 - 1.0)
    sampled = np.concatenate([tv * 4.0 + c + [0.03, -0.02, 0.05], loose]).astype(np.float32)
    return (owner[None], bf, sampled[None], tf), ix


def sdf_need_ref(verts_owner, verts_sampled, inside, scale_factor):
    """The voxels the lazy evaluation must list, per frame: the 8 trilinear corners of every sample point, inside the grid and
    inside the owner's mesh - from the float32 index arithmetic of sdf_sample_setup (csrc/sdf.hip), operation by operation.
    verts_* (B,V,3) float32, inside (B,32,32,32) bool [z][y][x] -> (B,32,32,32) bool."""
    f32 = np.float32
    vo, vs = np.asarray(verts_owner, f32), np.asarray(verts_sampled, f32)
    lo, hi = vo.min(1), vo.max(1)
    ctr = (lo + hi) / f32(2.0)
    sc = ((hi - lo) * ((f32(1.0) + f32(scale_factor)) * f32(0.5))).max(1)
    need = np.zeros(inside.shape, bool)
    for b in range(len(vs)):
        l = (vs[b] - ctr[b]) / sc[b]
        ix = ((l + f32(1.0)) * f32(32.0) - f32(1.0)) / f32(2.0)
        assert ix.dtype == f32
        i0 = np.floor(np.minimum(np.maximum(ix, f32(-4.0)), f32(36.0))).astype(np.int64)
        for corner in range(8):
            x, y, z = i0[:, 0] + (corner & 1), i0[:, 1] + ((corner >> 1) & 1), i0[:, 2] + (corner >> 2)
            ok = (x >= 0) & (x < 32) & (y >= 0) & (y < 32) & (z >= 0) & (z < 32)
            need[b, z[ok], y[ok], x[ok]] = True
    return need & inside


def sdf_scene_ref(phis, verts, scale_factor=0.2, dtype=torch.float64):
    """SDFSceneLoss (reference scenesdf.py:77-148) on GIVEN grids: phis = the oracle's float32 clamp(SDF, 0) of both meshes
    (B,32,32,32); box centre and scale, normalisation, trilinear sampling (grid_sample, zeros padding, align_corners=False) in
    `dtype`; loss = sum over both ordered pairs; gradients by autograd to the sampled vertices only (boxes and grids are
    constants, as in the reference).  -> loss (0-d), [g0, g1], {(k, l): (B,V_l) sample x owner scale}."""
    v = [torch.as_tensor(x).to(dtype).requires_grad_(True) for x in verts]
    loss, dist = torch.zeros((), dtype=dtype), {}
    for k, l in ((0, 1), (1, 0)):
        with torch.no_grad():
            lo, hi = v[k].min(1)[0], v[k].max(1)[0]
            ctr = ((lo + hi) / 2)[:, None]
            sc = ((hi - lo) * ((1 + scale_factor) * 0.5)).max(-1)[0]
        local = (v[l] - ctr) / sc.view(-1, 1, 1)
        d = torch.nn.functional.grid_sample(torch.as_tensor(phis[k]).to(dtype)[:, None], local.view(local.shape[0], -1, 1, 1, 3),
                                            mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0, :, 0, 0]
        dist[(k, l)] = (d * sc[:, None]).detach()
        loss = loss + d.sum()
    if loss.requires_grad:
        loss.backward()
    return loss.detach(), [x.grad if x.grad is not None else torch.zeros_like(x) for x in v], dist


def oracle_sdf(scene, scale_factor=0.2):
    """the CPU oracle (float32) on a scene tuple -> loss, [g0, g1], meta (sdfs, dist_values)"""
    from oracle import model as om
    v0, f0, v1, f1 = scene
    a, b = torch.from_numpy(v0).clone().requires_grad_(True), torch.from_numpy(v1).clone().requires_grad_(True)
    loss, meta = om.sdf_scene_loss([torch.from_numpy(f0), torch.from_numpy(f1)], [a, b], scale_factor=scale_factor)
    if loss.requires_grad:
        loss.backward()
    g = [x.grad if x.grad is not None else torch.zeros_like(x) for x in (a, b)]
    return loss.detach(), g, meta
