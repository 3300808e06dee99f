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
