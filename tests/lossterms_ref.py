"""References and input builders for the frame-loss terms (csrc/losses.hip), Adam and the log kernels (csrc/adam.hip) and the two
helpers at the end of csrc/geometry.hip (k_scale_by, k_sum_small).  CPU only: torch and numpy, no homan_amd.lib.

Every reference is a torch function on CPU tensors, float64 unless `dtype=torch.float32` asks for the same formulas in float32
(tests/test_lossterms_refs.py measures the float32 floors that way and checks the references against the CPU oracle;
tests/test_lossterms_edges_gpu.py holds the kernels against them).  Gradients are autograd of the value unless stated.
A gate (the coarse interaction term's boxes, IoU and z distance) is a decision, not a number with a tolerance: it is restated in
float32 numpy in the oracle's operation order, whatever `dtype` says.
"""
import numpy as np
import torch

F32 = np.float32
IMAGE_SIZE = 256.0
# (N = frames x hand_nb, V, hand_nb) of the hand-term grid: one element | one below, at and above a block of 256 | the scene of
# test_ops_gpu | two hands, three cameras | N V = 65 700 > 256 * 256 (k_v2d's cap) and N V 3 > 256 * 1024 (k_smooth's) |
# N V 3 = 88 800 > 170 * 512 (k_hand_terms' cap), two hands, four cameras
HAND_SHAPES = [(1, 1, 1), (1, 255, 1), (1, 256, 1), (1, 257, 1), (5, 778, 1), (6, 778, 2), (9, 7300, 1), (8, 3700, 2)]
PRIOR_NPCA = (1, 45, 256, 257, 7 * 45)
INTER_SHAPES = [(1, 1), (3, 63), (64, 65), (255, 257), (778, 1500), (1500, 778)]          # (Vh, Vo)
INTER_EXPANSION, INTER_ZTHRESH = 0.2, 3.0          # reference homan/losses.py:90,95
OFFSCREEN_V = (1, 255, 256, 257, 1000)
OFFSCREEN_WEIGHTS = (1.0, 0.37)
ZFAR = 100.0
SUM_SMALL_N = (1, 63, 64, 65, 1000)
GATE_K = ((1.0, 0.0, 0.5), (0.0, 1.0, 0.5), (0.0, 0.0, 1.0))
GATE_EXPANSIONS = (0.0, 0.25)


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).detach().to(dtype)


# ===================================================================== builders
def cameras(n, general=True):
    """(n,3,3) float32, every one different from every other (for n <= 105).  general: skew 0.03 and bottom row
    (0.01, -0.02, 1.1); otherwise a pinhole camera with bottom row (0, 0, 1)."""
    i = np.arange(n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 0], K[:, 0, 2] = 1.37 + 0.05 * (i % 7), 0.5 + 0.01 * (i % 3)
    K[:, 1, 1], K[:, 1, 2] = 1.41 - 0.04 * (i % 5), 0.5 - 0.015 * (i % 3)
    K[:, 0, 1] = 0.03 if general else 0.0
    K[:, 2] = (0.01, -0.02, 1.1) if general else (0.0, 0.0, 1.0)
    return torch.from_numpy(K.astype(F32))


def hand_scene(N, V, hand_nb, seed=0):
    """-> verts (N,V,3), camintr (N / hand_nb, 3, 3) general and distinct, ref2d (N,V,2) in pixels of IMAGE_SIZE; float32, every
    frame's data its own."""
    rng = np.random.default_rng([seed, N, V, hand_nb])
    verts = rng.normal(size=(N, V, 3)) * 0.05 + [0.0, 0.0, 0.6] + rng.normal(size=(N, 1, 3)) * 0.01
    ref2d = rng.uniform(0.0, IMAGE_SIZE, size=(N, V, 2))
    return torch.from_numpy(verts.astype(F32)), cameras(N // hand_nb), torch.from_numpy(ref2d.astype(F32))


def ops_scene(hand_nb=1):
    """The scene of tests/test_ops_gpu.py::test_v2d_smooth_priors, written out (B = 5, V = 778, one pinhole camera for every
    frame); hand_nb = 2: ten hand frames, frame n under camera n // 2 of five distinct general cameras (`cameras`).
    -> verts, camintr (5,3,3), ref2d, verts_obj (5,1500,3), pca"""
    g = torch.Generator().manual_seed(2)
    B, V = 5 * hand_nb, 778
    verts = torch.randn(B, V, 3, generator=g) * 0.05 + torch.tensor([0.0, 0.0, 0.6])
    camintr = torch.tensor([[1.37, 0, 0.5], [0, 1.37, 0.5], [0, 0, 1.0]]).repeat(5, 1, 1)
    if hand_nb > 1:
        camintr = cameras(5)
    ref2d = torch.rand(B, V, 2, generator=g) * 256
    vob = torch.randn(5, 1500, 3, generator=g)
    pca = torch.randn(B, 45, generator=g)
    return verts, camintr, ref2d, vob, pca


def priors_scene(npca, clips, seed=0):
    """-> pca (clips, npca), s_obj, m_obj, s_hand, m_hand (clips,) float32, every clip's own"""
    rng = np.random.default_rng([seed, npca, clips])
    f = lambda x: torch.from_numpy(np.asarray(x, F32))
    c = np.arange(clips)
    return (f(rng.normal(size=(clips, npca))), f(1.2 + 0.3 * c), f(1.0 - 0.1 * c), f(0.9 - 0.2 * c), f(1.0 + 0.05 * c))


def inter_scene(B, Vh, Vo, seed=0, z_off_every=0, box_off=()):
    """Random hand and object clouds next to each other, per-frame distinct cameras -> vh (B,Vh,3), vo (B,Vo,3), camintr (B,3,3)
    float32.  Frames b with b % z_off_every == z_off_every - 1 have the hand 5 further away (z gap > 3); frames in `box_off`
    have it 2 to the right (boxes apart).  Every gated-off frame is far from its gate's edge."""
    rng = np.random.default_rng([seed, B, Vh, Vo])
    vh = rng.normal(size=(B, Vh, 3)) * 0.04 + [0.02, 0.0, 0.6] + rng.normal(size=(B, 1, 3)) * 0.01
    vo = rng.normal(size=(B, Vo, 3)) * 0.05 + [0.0, 0.0, 0.62] + rng.normal(size=(B, 1, 3)) * 0.01
    for b in range(B):
        if z_off_every and b % z_off_every == z_off_every - 1:
            vh[b, :, 2] += 5.0
        if b in box_off:
            vh[b, :, 0] += 2.0
    return torch.from_numpy(vh.astype(F32)), torch.from_numpy(vo.astype(F32)), cameras(B)


def _exact32(a):
    a = np.asarray(a, np.float64)
    assert np.array_equal(a.astype(F32).astype(np.float64), a), "not exact in float32"
    return a.astype(F32)


def _rect(u0, u1, v0, v1, zs, extra=()):
    """four vertices whose NDC coordinates under GATE_K are the corners of [u0,u1] x [v0,v1] (NDC = 2 (x, y) / z there), at
    depths zs, plus `extra` vertices; padded to five vertices with copies of the first (which move neither box nor z range)"""
    pts = [(u * z / 2.0, v * z / 2.0, z) for (u, v), z in zip(((u0, v0), (u1, v0), (u1, v1), (u0, v1)), zs)] + list(extra)
    pts += [pts[0]] * (5 - len(pts))
    return _exact32(pts)[None]


def gate_scenes(expansion):
    """The exact gate scenes for `expansion` in GATE_EXPANSIONS under K = GATE_K: dyadic coordinates, z in {1, 4} (and one vertex
    on the optical axis at 4 - 2^-21), so every projected coordinate and every (expanded) box edge is exact in float32.
    -> [(name, vh (1,V,3), vo (1,V,3), flag, z distance)], V = 5 (1 for "point"), float32 numpy.
      touch     the (expanded) boxes share the edge u = 0 resp. meet at one abscissa: w = 0, IoU = 0         -> 0
      quantum   the hand's (expanded) box reaches 2^-24 over the object's edge at u = 0                     -> 1
      zgap3     boxes overlapping, object at z = 1, hand at z = 4: gap exactly 3.0 (the threshold)         -> 0
      zgap3m    the same with one hand vertex at 4 - 2^-21: gap 3 - 2^-21                                  -> 1
      point     each mesh one vertex, both at one point: areas 0, IoU = 0 / 0                              -> 0
      zoverlap  object z in [1, 4], hand at z = 4: ranges overlap, z distance 0                            -> 1"""
    q = 2.0 ** -24
    if expansion == 0.0:
        obj_u, touch_u, quant_u = (-1.0, 0.0), (0.0, 1.0), (-q, 1.0)
    elif expansion == 0.25:             # centre +- 1.25 x half extent: object -> [0, 1.25], hand -> [-0.625 (+ q), 0 (+ q)]; the
        # hand on the left, where u + 0.5 < 0.5 carries the 2^-25 that the quantum needs
        obj_u, touch_u, quant_u = (0.125, 1.125), (-0.5625, -0.0625), (-0.5625 + q, -0.0625 + q)
    else:
        raise ValueError(expansion)
    za, zb = (1.0, 4.0, 1.0, 4.0), (4.0, 1.0, 4.0, 1.0)
    obj = _rect(*obj_u, -0.5, 0.5, za)
    sq_o, sq_h = _rect(-0.5, 0.5, -0.5, 0.5, (1.0,) * 4), (-0.25, 0.75, -0.25, 0.75)
    pt = _exact32([[0.25, -0.125, 1.0]])[None]
    return [("touch", _rect(*touch_u, -0.5, 0.5, zb), obj, 0, 0.0),
            ("quantum", _rect(*quant_u, -0.5, 0.5, zb), obj, 1, 0.0),
            ("zgap3", _rect(*sq_h, (4.0,) * 4), sq_o, 0, 3.0),
            ("zgap3m", _rect(*sq_h, (4.0,) * 4, extra=[(0.0, 0.0, 4.0 - 2.0 ** -21)]), sq_o, 1, 3.0 - 2.0 ** -21),
            ("point", pt, pt.copy(), 0, 0.0),
            ("zoverlap", _rect(*sq_h, (4.0,) * 4), _rect(-0.5, 0.5, -0.5, 0.5, (1.0, 1.0, 4.0, 4.0)), 1, 0.0)]


def gate_clip(expansion):
    """the five-vertex gate scenes as frames of three clips of two: (touch, zgap3) - all gated off -, (quantum, zgap3m),
    (zoverlap, touch) -> vh (6,5,3), vo (6,5,3), camintr (6,3,3) float32 torch, flags (6,) int"""
    sc = {n: (h, o, f) for n, h, o, f, _ in gate_scenes(expansion)}
    order = ("touch", "zgap3", "quantum", "zgap3m", "zoverlap", "touch")
    vh, vo = np.concatenate([sc[n][0] for n in order]), np.concatenate([sc[n][1] for n in order])
    K = torch.tensor(GATE_K).repeat(len(order), 1, 1)
    return torch.from_numpy(vh), torch.from_numpy(vo), K, np.array([sc[n][2] for n in order])


def offscreen_cloud(N, V, seed=0):
    """N candidates with vertices of their own straddling all six planes under `offscreen_K()` -> (N,V,3) float32"""
    rng = np.random.default_rng([seed, N, V])
    z = np.where(rng.random((N, V)) < 0.8, rng.uniform(0.3, 3.0, (N, V)), rng.uniform(-2.0, 140.0, (N, V)))
    xy = rng.uniform(-0.6, 0.6, (N, V, 2)) * np.abs(z)[..., None]          # NDC in about [-1.7, 1.7]
    return torch.from_numpy(np.concatenate([xy, z[..., None]], -1).astype(F32))


def offscreen_K():
    return torch.tensor([[1.37, 0.03, 0.52], [-0.02, 1.41, 0.47], [0.0, 0.0, 1.0]])


OFFSCREEN_EXACT_Z = 16.0


def offscreen_exact_scene():
    """Under GATE_K (NDC = 2 (x, y) / z) at z = OFFSCREEN_EXACT_Z: per NDC plane (u = 1, v = 1, u = -1, v = -1) one vertex on the
    plane, one a float32 step inside and one a step outside (the step of u + 0.5 next to 1 resp. of u - 0.5 next to -1.5: the
    smallest change of the NDC coordinate the float32 formula can show), then the depth cases on the optical axis:
    z = 2^-20, z = -0.5, z = zfar, z = the float32 after zfar.  -> verts (1,16,3) float32, names (16)"""
    z, pts, names = OFFSCREEN_EXACT_Z, [], []
    step = 2.0 ** -22                 # NDC = 2 (u - 0.5), u = xn + 0.5 in [1, 2) (quantum 2^-23) resp. [-1, -0.5] ...
    for axis, sign in ((0, 1.0), (1, 1.0), (0, -1.0), (1, -1.0)):
        for where, d in (("on", 0.0), ("inside", -step), ("outside", step)):
            p = [0.0, 0.0, z]
            p[axis] = sign * (1.0 + d) * z / 2.0
            pts.append(p)
            names.append(("u", "v")[axis] + ("+" if sign > 0 else "-") + where)
    pts += [[0.0, 0.0, 2.0 ** -20], [0.0, 0.0, -0.5], [0.0, 0.0, ZFAR], [0.0, 0.0, float(np.nextafter(F32(ZFAR), F32(1e9)))]]
    names += ["z0+", "z<0", "zfar", "zfar+"]
    return torch.from_numpy(_exact32(pts))[None], names


def adam_inputs(sizes, steps, seed=0):
    """-> params [float32 (n,)], grads [step][tensor] float32.  Tensor 1 (where it exists) has an all-zero gradient at every step;
    the others hold exact zeros (a fifth of the entries), 1e-20 and 1e+15 among ordinary values."""
    rng = np.random.default_rng([seed, len(sizes), steps])
    params = [torch.from_numpy(rng.normal(size=n).astype(F32)) for n in sizes]
    grads = []
    for t in range(steps):
        row = []
        for k, n in enumerate(sizes):
            g = rng.normal(size=n) * 10.0 ** rng.integers(-3, 2)
            g[rng.random(n) < 0.2] = 0.0
            if n >= 3:
                g[(t + 1) % n], g[(t + 2) % n] = 1e-20, 1e15
            elif t % 3 == 1:
                g[0] = 1e-20 if t % 2 else 1e15
            row.append(torch.from_numpy((np.zeros(n) if k == 1 else g).astype(F32)))
        grads.append(row)
    return params, grads


def adam_oracle_run(params, grads, lrs, t0=0):
    """oracle.adam.Adam (the bit-exact statement of k_adam) driven with given gradients: params [tensor], grads [step][tensor],
    lrs [float per tensor], step counter preset to t0 -> [step][(p, m, v) per tensor] float32 numpy copies"""
    from oracle import adam as o_adam
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    opt = o_adam.Adam([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)])
    opt.t = t0
    out = []
    for row in grads:
        for p, g in zip(ps, row):
            p.grad = g.clone()
        opt.step()
        out.append([(p.detach().numpy().copy(), opt.state[id(p)]["m"].copy(), opt.state[id(p)]["v"].copy()) for p in ps])
    return out


def log_scene(nclips, n, seed=0):
    """-> vals (nclips, n + 1) float32 (last column a sentinel the kernel overwrites), weights (n,) float32; for n > 1 the weight
    at index n // 2 is 0 and every clip's value there is NaN"""
    rng = np.random.default_rng([seed, nclips, n])
    vals = rng.normal(size=(nclips, n + 1)).astype(F32)
    w = rng.uniform(0.1, 3.0, size=n).astype(F32)
    if n > 1:
        w[n // 2] = 0.0
        vals[:, n // 2] = np.nan
    vals[:, n] = -7.0
    return torch.from_numpy(vals), torch.from_numpy(w)


def sum_small_scene(n, clips, exact, seed=0):
    """-> parts (clips, n), extra (clips,) float32.  exact: multiples of 2^-10 below 2^3 in magnitude (up to 2^10 of them: every
    partial sum in any order is a multiple of 2^-10 below 2^13, exact in float32, and so is SUM_SMALL_W's combination with
    `extra`); otherwise uniform in [-0.3, 1)."""
    rng = np.random.default_rng([seed, n, clips, int(exact)])
    if exact:
        parts, extra = rng.integers(-2 ** 13 + 1, 2 ** 13, size=(clips, n)) / 1024.0, rng.integers(-2 ** 10, 2 ** 10, size=clips) / 1024.0
        assert n <= 2 ** 10
    else:
        parts, extra = rng.uniform(-0.3, 1.0, size=(clips, n)), rng.normal(size=clips)
    return torch.from_numpy(parts.astype(F32)), torch.from_numpy(extra.astype(F32))


# ===================================================================== references
def v2d_ref(verts, camintr, hand_nb, ref2d, image_size, dtype=torch.float64):
    """2-D reprojection term (reference homan/losses.py:141-164) for a general 3 x 3 K per frame, frame n under camera
    n // hand_nb: p = (K x)_{0,1} / (K x)_2; loss = mean_{n,v} |p - ref / size|^2; metric = mean |p size - ref|.
    -> loss (0-d), metric (0-d), d loss / d verts (N,V,3)"""
    v = _t(verts, dtype).clone().requires_grad_(True)
    K = _t(camintr, dtype)[torch.arange(v.shape[0]) // hand_nb][:, None]            # (N,1,3,3)
    r = _t(ref2d, dtype)
    x, y, z = v.unbind(-1)
    hx = K[..., 0, 0] * x + K[..., 0, 1] * y + K[..., 0, 2] * z
    hy = K[..., 1, 0] * x + K[..., 1, 1] * y + K[..., 1, 2] * z
    hz = K[..., 2, 0] * x + K[..., 2, 1] * y + K[..., 2, 2] * z
    p = torch.stack([hx / hz, hy / hz], -1)
    loss = ((p - r / image_size) ** 2).sum(-1).mean()
    metric = (p.detach() * image_size - r).norm(2, -1).mean()
    loss.backward()
    return loss.detach(), metric, v.grad


def smooth_ref(verts, hand_nb, dtype=torch.float64):
    """Temporal smoothness (reference homan/lossutils.py:18-36): mean over the pairs (n, n + hand_nb) and all coordinates of the
    squared difference -> value (0-d), gradient (N,V,3).  Without a pair (N <= hand_nb) value and gradient are 0: the project's
    convention (the rigid backward's smoothness term states the same); the oracle's mean() of an empty tensor is NaN."""
    v = _t(verts, dtype).clone().requires_grad_(True)
    if v.shape[0] <= hand_nb:
        return torch.zeros((), dtype=dtype), torch.zeros_like(v)
    loss = ((v[hand_nb:] - v[:-hand_nb]) ** 2).mean()
    loss.backward()
    return loss.detach(), v.grad


def priors_ref(pca, s_obj, m_obj, s_hand, m_hand, dtype=torch.float64):
    """PCA prior mean(pca^2) (reference homan/lossutils.py:39-40) and the two intrinsic-scale priors (s - m)^2 (:107-109) of ONE
    clip -> (l_pca, l_sobj, l_shand) 0-d, (g_pca like pca, g_sobj 0-d, g_shand 0-d)"""
    p = _t(pca, dtype).clone().requires_grad_(True)
    so, sh = _t(s_obj, dtype).reshape(()).clone().requires_grad_(True), _t(s_hand, dtype).reshape(()).clone().requires_grad_(True)
    l0, l1, l2 = (p ** 2).mean(), (so - _t(m_obj, dtype).reshape(())) ** 2, (sh - _t(m_hand, dtype).reshape(())) ** 2
    (l0 + l1 + l2).backward()
    return (l0.detach(), l1.detach(), l2.detach()), (p.grad, so.grad, sh.grad)


def inter_boxes32(verts, K, expansion):
    """oracle.model.project_bbox in float32 numpy, operation by operation (oracle.nmr.projection with R = I, t = 0, no distortion,
    orig_size 1 leaves x / (z + 1e-9), (y * -1) / (z + 1e-9); then (xn k00 + yn k01) + k02, 1 - (...), 2 (u - 0.5); the boxes'
    expansion about their centre with the factor float32(1 + expansion), skipped when expansion == 0) -> (B,4) float32"""
    v, K = np.asarray(verts, F32), np.asarray(K, F32)
    zz = v[..., 2] + F32(1e-9)
    xn, yn = v[..., 0] / zz, (v[..., 1] * F32(-1.0)) / zz
    u = (xn * K[:, None, 0, 0] + yn * K[:, None, 0, 1]) + K[:, None, 0, 2]
    w = (xn * K[:, None, 1, 0] + yn * K[:, None, 1, 1]) + K[:, None, 1, 2]
    w = F32(1.0) - w
    u, w = F32(2.0) * (u - F32(0.5)), F32(2.0) * (w - F32(0.5))
    lo, hi = np.stack([u.min(1), w.min(1)], 1), np.stack([u.max(1), w.max(1)], 1)
    if expansion:
        c, e = (lo + hi) / F32(2.0), (hi - lo) / F32(2.0) * F32(1.0 + expansion)
        lo, hi = c - e, c + e
    box = np.concatenate([lo, hi], 1)
    assert box.dtype == F32
    return box


def inter_boxes64(verts, K, expansion):
    """the same boxes in exact terms: float64, and without the 1e-9 under the division (which float32 absorbs for |z| >= 2^-5:
    z + 1e-9 == z there) - on the exact gate scenes every operation is exact in float64, so these ARE the boxes"""
    v, K = np.asarray(verts, np.float64), np.asarray(K, np.float64)
    xn, yn = v[..., 0] / v[..., 2], -v[..., 1] / v[..., 2]
    u = 2.0 * (xn * K[:, None, 0, 0] + yn * K[:, None, 0, 1] + K[:, None, 0, 2] - 0.5)
    w = 2.0 * (1.0 - (xn * K[:, None, 1, 0] + yn * K[:, None, 1, 1] + K[:, None, 1, 2]) - 0.5)
    lo, hi = np.stack([u.min(1), w.min(1)], 1), np.stack([u.max(1), w.max(1)], 1)
    c, e = (lo + hi) / 2.0, (hi - lo) / 2.0 * (1.0 + expansion)
    return np.concatenate([c - e, c + e], 1)


def inter_gate32(vh, vo, camintr, expansion, zthresh):
    """The gate of the coarse interaction term (reference homan/losses.py:98-139) in float32 numpy in the oracle's operation order:
    oracle.model.project_bbox of object and hand, compute_iou(box_obj, box_hand), compute_dist_z(object, hand),
    flag = IoU > 0 and z distance < zthresh (an IoU of 0 / 0 is NaN: not > 0).
    -> dict(flag (B,) int64, iou (B,) float32, zd (B,) float32, box_obj, box_hand (B,4) float32)"""
    vh, vo = np.asarray(vh, F32), np.asarray(vo, F32)
    b1, b2 = inter_boxes32(vo, camintr, expansion), inter_boxes32(vh, camintr, expansion)
    with np.errstate(invalid="ignore", divide="ignore"):
        a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
        a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
        wh = np.maximum(np.minimum(b1[:, 2:], b2[:, 2:]) - np.maximum(b1[:, :2], b2[:, :2]), F32(0.0))
        inter = wh[:, 0] * wh[:, 1]
        iou = inter / (a1 + a2 - inter)
    a, b, c, d = vo[..., 2].min(1), vo[..., 2].max(1), vh[..., 2].min(1), vh[..., 2].max(1)
    zd = np.where((d >= a) & (b >= c), F32(0.0), np.minimum(np.abs(c - b), np.abs(a - d)))
    assert iou.dtype == F32 and zd.dtype == F32
    with np.errstate(invalid="ignore"):
        flag = (iou > 0) & (zd < F32(zthresh))
    return dict(flag=flag.astype(np.int64), iou=iou, zd=zd, box_obj=b1, box_hand=b2)


def inter_ref(vh, vo, camintr, expansion, zthresh, clip_len=None, upstream=1.0, dtype=torch.float64):
    """Coarse interaction term (reference homan/losses.py:199-242, centroid mode): per frame the gate's flag (inter_gate32), the
    MSE of the two centroids and the record's gradient vector flag * 2 (c_h - c_o) / 3; per clip of clip_len frames (None: one
    clip) the sum of the flagged frames' MSE; and the gradients of `upstream` x (sum over all clips) to both meshes (autograd).
    -> dict(flag (B,) int64, mse (B,), gvec (B,3), total (C,), g_hand (B,Vh,3), g_obj (B,Vo,3), gate = inter_gate32's dict)"""
    gate = inter_gate32(vh, vo, camintr, expansion, zthresh)
    on = torch.from_numpy(gate["flag"]) != 0
    h, o = _t(vh, dtype).clone().requires_grad_(True), _t(vo, dtype).clone().requires_grad_(True)
    ch, co = h.mean(1), o.mean(1)
    mse = ((ch - co) ** 2).mean(-1)
    total = torch.where(on, mse, torch.zeros_like(mse)).reshape(-1, clip_len or len(mse)).sum(1)
    (total.sum() * upstream).backward()
    gvec = on.to(dtype)[:, None] * 2 * (ch - co).detach() / 3
    return dict(flag=gate["flag"], mse=mse.detach(), gvec=gvec, total=total.detach(), g_hand=h.grad, g_obj=o.grad, gate=gate)


def offscreen_ref(verts, K, zfar, weight, dtype=torch.float64):
    """Off-screen penalty of the pose initialisation (reference homan/pose_optimization.py:112-135 as
    oracle.poseopt.PoseOptimizer.compute_offscreen_loss words it): NDC (u, v) of oracle.nmr.projection under ONE camera K (its
    first two rows; R = I, t = 0, orig_size 1), hinges relu(u - 1) + relu(v - 1) + relu(-1 - u) + relu(-1 - v) + relu(-z) +
    relu(z - zfar) summed over a candidate's vertices, times weight.  relu has subgradient 0 at 0 (torch.relu; the kernel's
    strict `> 0`).  verts (N,V,3) -> out (N,), d sum(out) / d verts (N,V,3)"""
    v, k = _t(verts, dtype).clone().requires_grad_(True), _t(K, dtype)
    x, y, z = v.unbind(-1)
    zz = z + 1e-9
    xn, yn = x / zz, y / zz
    u = (xn * k[0, 0] + yn * k[0, 1]) + k[0, 2]
    w = 1 - ((xn * k[1, 0] + yn * k[1, 1]) + k[1, 2])
    nu, nv = 2 * (u - 0.5), 2 * (w - 0.5)
    relu = torch.relu
    val = relu(nu - 1) + relu(nv - 1) + relu(-1 - nu) + relu(-1 - nv) + relu(-z) + relu(z - zfar)
    out = weight * val.sum(1)
    out.sum().backward()
    return out.detach(), v.grad


def log_total_ref(vals, w):
    """t = 0; for i: if w[i] != 0: t += w[i] * vals[i] - float32, in that order, every operation rounded: bit-exact.  A zero
    weight skips its value (a NaN there does not reach the total).  vals (n,), w (n,) -> numpy float32 scalar"""
    vals, w = np.asarray(vals, F32), np.asarray(w, F32)
    t = F32(0.0)
    for i in range(len(w)):
        if w[i] != 0:
            t = F32(t + F32(w[i] * vals[i]))
    return t


def sum_small_ref(parts, w0, extra, w1, dtype=torch.float64):
    """out[c] = w0 sum(parts[c]) + w1 extra[c] (extra None: no second term).  parts (C,n) -> (C,)"""
    out = float(w0) * _t(parts, dtype).sum(1)
    return out if extra is None else out + float(w1) * _t(extra, dtype)


# ===================================================================== the cases of the GPU grid (shared with the floors)
CLIP_C, CLIP_LEN, CLIP_V = 3, 4, 300
SMOOTH_ONLY = [(1, 300, 1), (2, 300, 2), (2, 300, 1), (3, 300, 2)]          # (N, V, hand_nb): N = hand_nb twice, N = hand_nb + 1 twice


def clip_batch(hand_nb):
    """3 clips of 4 frames back to back (V = 300) -> verts (12,300,3), camintr (12 / hand_nb,3,3), ref2d (12,300,2)"""
    return hand_scene(CLIP_C * CLIP_LEN, CLIP_V, hand_nb, seed=5)


def clip_slice(batch, hand_nb, c):
    verts, K, ref2d = batch
    kc = CLIP_LEN // hand_nb
    return verts[c * CLIP_LEN:(c + 1) * CLIP_LEN], K[c * kc:(c + 1) * kc], ref2d[c * CLIP_LEN:(c + 1) * CLIP_LEN]


def hand_cases():
    """name -> (verts, camintr, ref2d, hand_nb): HAND_SHAPES and every clip of the two clip batches"""
    out = {f"N{N}_V{V}_nb{nb}": hand_scene(N, V, nb) + (nb,) for N, V, nb in HAND_SHAPES}
    for nb in (1, 2):
        for c in range(CLIP_C):
            out[f"clip{c}_nb{nb}"] = clip_slice(clip_batch(nb), nb, c) + (nb,)
    return out


def smooth_only_cases():
    return {f"N{N}_V{V}_nb{nb}": (hand_scene(N * nb, V, nb, seed=3)[0][:N], nb) for N, V, nb in SMOOTH_ONLY}


def inter_cases():
    """name -> (vh, vo, camintr, expansion, zthresh, clip_len or None), torch float32"""
    out = {}
    for Vh, Vo in INTER_SHAPES:
        out[f"Vh{Vh}_Vo{Vo}"] = inter_scene(4, Vh, Vo, z_off_every=4, box_off=(1,)) + (INTER_EXPANSION, INTER_ZTHRESH, None)
    out["long300"] = inter_scene(300, 8, 8, z_off_every=3) + (INTER_EXPANSION, INTER_ZTHRESH, None)
    out["clips3x4"] = inter_scene(12, 8, 8, z_off_every=3, box_off=(4,)) + (INTER_EXPANSION, INTER_ZTHRESH, 4)
    for e in GATE_EXPANSIONS:
        vh, vo, K, _ = gate_clip(e)
        out[f"gate_e{e}"] = (vh, vo, K, e, INTER_ZTHRESH, 2)
        pt = [s for s in gate_scenes(e) if s[0] == "point"][0]
        out[f"point_e{e}"] = (torch.from_numpy(pt[1]), torch.from_numpy(pt[2]), torch.tensor(GATE_K)[None], e, INTER_ZTHRESH, None)
    return out


INTER_UPSTREAMS = (1.0, -2.5, 0.0)


def offscreen_cases():
    """name -> (verts (N,V,3), K (3,3), weight): random clouds x weights, the exact scene, and each of its vertices alone
    (names "hinge_*")"""
    out = {}
    for V in OFFSCREEN_V:
        for w in OFFSCREEN_WEIGHTS:
            out[f"cloud_V{V}_w{w}"] = (offscreen_cloud(3, V), offscreen_K(), w)
    ex, names = offscreen_exact_scene()
    for w in OFFSCREEN_WEIGHTS:
        out[f"exact_w{w}"] = (ex, torch.tensor(GATE_K), w)
    for i, n in enumerate(names):
        out[f"hinge_{n}"] = (ex[:, i:i + 1].contiguous(), torch.tensor(GATE_K), 1.0)
    return out


SUM_SMALL_W = (0.5, -2.0)            # (w0, w1): powers of two, so the exact data stay exact
