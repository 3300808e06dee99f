"""Restatements for the hand initialisation from keypoints (homan_amd/handinit.py, csrc/handinit.hip).

`keypoint_terms_f32`: hm_keypoint_terms_clips in NumPy float32, in the operation order include/homan_amd.h states - every
product and sum is one NumPy operation on float32 arrays, so it rounds once, as the kernel's does (-ffp-contract=off).  The
kernel is held to it bit for bit.

`terms_torch` / `fit`: the same mathematics in differentiable torch, in the dtype asked for, MANO from oracle/lbs.py, torch's
Adam with the three learning-rate groups, the candidates and the selection of HandKeypointFitter.  The float64 run is the
reference of the whole fit; the float32 run of the SAME code measures what float32 rounding alone does to a fit.

`scene`: the inputs the CPU and the GPU tests share.
"""
import numpy as np
import torch

from homan_amd import handinit
from homan_amd.mano_assets import hand_models, synthetic_mano
from oracle import lbs as olbs

F = np.float32
V, K21 = 778, 21


# ---------------------------------------------------------------------------------------------- fp32, the kernel's order
def tree64(a):
    """(..., 64) -> (...): a_l += a_(l ^ o), o = 32 .. 1"""
    a = np.asarray(a, F)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lanes ^ o]
    return a[..., 0]


def blocksum(x):
    x = np.asarray(x, F).reshape(-1)
    acc = np.zeros(256, F)
    for j in range(0, x.size, 256):
        chunk = x[j:j + 256]
        acc[:chunk.size] = acc[:chunk.size] + chunk
    w = tree64(acc.reshape(4, 64))
    return ((w[0] + w[1]) + w[2]) + w[3]


def _pad64(a, axis):
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, (-a.shape[axis]) % 64)
    return np.pad(a, pad)


def keypoint_terms_f32(verts, W, camintr, kp2d, c2, s, kp3d, c3, sigma, znear, lw2, lw3, clip_len):
    """-> dict(keypoints (N,21,3), unit_grad (N,778,3), row_parts (N,2), out (C,2)), all float32"""
    verts, W, camintr, kp2d, c2, s = (np.asarray(a, F) for a in (verts, W, camintr, kp2d, c2, s))
    N, C = verts.shape[0], verts.shape[0] // clip_len
    has3 = kp3d is not None
    sigma, znear, lw2, lw3, two = F(sigma), F(znear), F(lw2), F(lw3), F(2)
    # regression: lane l adds vertices l, l + 64, ... from 0, then TREE64
    Wp, Vp = _pad64(W, 1), _pad64(verts, 1)                     # (21,832), (N,832,3): +0 products change nothing
    acc = np.zeros((N, K21, 64, 3), F)
    for j in range(Wp.shape[1] // 64):
        sl = slice(64 * j, 64 * j + 64)
        acc = acc + Wp[None, :, sl, None] * Vp[:, None, sl, :]
    X = tree64(np.moveaxis(acc, 2, -1))                          # (N,21,3)
    S2 = np.array([blocksum(c2[c * clip_len:(c + 1) * clip_len]) for c in range(C)], F)
    S3 = np.array([blocksum(np.asarray(c3, F)[c * clip_len:(c + 1) * clip_len]) if has3 else F(0) for c in range(C)], F)
    with np.errstate(all="ignore"):
        coef2 = np.where(S2 > 0, lw2 / S2, F(0)).astype(F).repeat(clip_len)[:, None]
        coef3 = np.where(S3 > 0, lw3 / S3, F(0)).astype(F).repeat(clip_len)[:, None]
        x, y, z = X[..., 0], X[..., 1], X[..., 2]
        fx, cx, fy, cy = (camintr[:, i, j][:, None] for i, j in ((0, 0), (0, 2), (1, 1), (1, 2)))
        sc, s2 = s[:, None], sigma * sigma
        fxx, fyy = fx * x, fy * y
        px, py = fxx / z + cx, fyy / z + cy
        rx, ry = (px - kp2d[..., 0]) / sc, (py - kp2d[..., 1]) / sc
        u = rx * rx + ry * ry
        den = s2 + u
        q = s2 / den
        g = (c2 * (q * q)) * coef2
        gpx, gpy = g * ((two * rx) / sc), g * ((two * ry) / sc)
        on, front = c2 > 0, z > znear
        live = on & front
        cost2 = np.where(live, c2 * ((s2 * u) / den), np.where(on, c2 * s2, F(0))).astype(F)
        dX = np.stack([gpx * (fx / z), gpy * (fy / z), -((gpx * fxx + gpy * fyy) / (z * z))], -1)
        G = np.where(live[..., None], dX, F(0)).astype(F)
        cost3 = np.zeros((N, K21), F)
        if has3:
            kp3d, c3 = np.asarray(kp3d, F), np.asarray(c3, F)
            d = (X - X[:, :1]) - kp3d
            on3 = c3 > 0
            cost3 = np.where(on3, c3 * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]), F(0)).astype(F)
            h = np.where(on3[..., None], (((two * c3) * coef3)[..., None]) * d, F(0)).astype(F)
            G = G + h
            tot = np.zeros((N, 3), F)
            for k in range(K21):
                tot = tot + h[:, k]
            G[:, 0] = G[:, 0] - tot
    unit = np.zeros((N, V, 3), F)
    for k in range(K21):
        unit = unit + W[k][None, :, None] * G[:, k][:, None, :]
    row_parts = np.stack([tree64(_pad64(cost2, 1)), tree64(_pad64(cost3, 1))], -1)
    out = np.zeros((C, 2), F)
    for c in range(C):
        rows = slice(c * clip_len, (c + 1) * clip_len)
        b2, b3 = blocksum(row_parts[rows, 0]), blocksum(row_parts[rows, 1])
        out[c, 0] = b2 / S2[c] if S2[c] > 0 else 0
        out[c, 1] = b3 / S3[c] if S3[c] > 0 else 0
    return dict(keypoints=X, unit_grad=unit, row_parts=row_parts, out=out)


# ---------------------------------------------------------------------------------------------- differentiable torch
def rot6d_to_matrix(r6):
    a1, a2 = r6[:, :, 0], r6[:, :, 1]
    b1 = a1 / torch.linalg.vector_norm(a1, dim=1, keepdim=True).clamp_min(1e-12)
    u = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    b2 = u / torch.linalg.vector_norm(u, dim=1, keepdim=True).clamp_min(1e-12)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-1)


def terms_torch(vh, W, camintr, kp2d, c2, s, kp3d, c3, sigma, znear, clip_len):
    """-> (L2d (C,), L3d (C,), X (N,21,3)) in vh's dtype; targets with zero confidence never enter the arithmetic"""
    N, C = vh.shape[0], vh.shape[0] // clip_len
    X = torch.einsum("kv,nvc->nkc", W, vh)
    on, z = c2 > 0, X[..., 2]
    front = z > znear
    zs = torch.where(front, z, torch.ones_like(z))
    px = camintr[:, 0, 0, None] * X[..., 0] / zs + camintr[:, 0, 2, None]
    py = camintr[:, 1, 1, None] * X[..., 1] / zs + camintr[:, 1, 2, None]
    tgt = torch.where(on[..., None], kp2d, torch.zeros_like(kp2d))
    rx, ry = (px - tgt[..., 0]) / s[:, None], (py - tgt[..., 1]) / s[:, None]
    u = rx * rx + ry * ry
    s2 = sigma * sigma
    cost2 = torch.where(on, torch.where(front, c2 * (s2 * u / (s2 + u)), c2 * s2), torch.zeros_like(u))
    S2 = c2.reshape(C, -1).sum(1)
    L2 = torch.where(S2 > 0, cost2.reshape(C, -1).sum(1) / S2.clamp_min(1e-30), torch.zeros_like(S2))
    if kp3d is None:
        return L2, torch.zeros_like(L2), X
    on3 = c3 > 0
    d = (X - X[:, :1]) - torch.where(on3[..., None], kp3d, torch.zeros_like(kp3d))
    cost3 = torch.where(on3, c3 * (d * d).sum(-1), torch.zeros_like(c3))
    S3 = c3.reshape(C, -1).sum(1)
    L3 = torch.where(S3 > 0, cost3.reshape(C, -1).sum(1) / S3.clamp_min(1e-30), torch.zeros_like(S3))
    return L2, L3, X


class Mano:
    """MANO of one side in `dtype` from oracle/lbs.py (the left hand: the mirrored model, and the sign flip of the PCA basis that
    homan_amd.manomodel folds into it)"""

    def __init__(self, mano_model, side, dtype):
        m = dict(hand_models(mano_model)[side])
        comps = np.array(m["hand_components"], np.float64, copy=True)[:16]
        if side == "left":
            comps[:, 1::3] *= -1.0
            comps[:, 2::3] *= -1.0
        self.dtype = dtype
        self.model = {k: torch.as_tensor(np.asarray(m[k])).to(dtype) for k in
                      ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")}
        self.model["parents"] = torch.as_tensor(np.asarray(m["parents"])).long()
        self.comps, self.mean = torch.from_numpy(comps).to(dtype), torch.as_tensor(np.asarray(m["hand_mean"])).to(dtype)
        self.W = torch.from_numpy(handinit.keypoint_regressor(m)).to(dtype)
        self.model_np = m

    def __call__(self, pca, betas):
        """-> (verts (N,778,3), posed kinematic joints (N,16,3)), zero global rotation"""
        was = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)
        try:
            pose = pca[:, :16] @ self.comps + self.mean[None]
            full = torch.cat([torch.zeros(pca.shape[0], 3, dtype=self.dtype), pose], 1)
            return olbs.lbs(betas, full, self.model)
        finally:
            torch.set_default_dtype(was)


def all_terms(mano, p, data, lw, sigma, znear, B):
    """p = (rot6d, trans, pca, betas) -> vals (C,8) = {L2d, L3d, Lpca, 0, 0, Lsmooth, Lbeta, total}, vh, X"""
    rot6d, trans, pca, betas = p
    C = rot6d.shape[0] // B
    vm = mano(pca, betas)[0]
    vh = vm @ rot6d_to_matrix(rot6d) + trans[:, None]
    L2, L3, X = terms_torch(vh, mano.W, data["camintr"], data["kp2d"], data["c2"], data["s"], data.get("kp3d"), data.get("c3"),
                            sigma, znear, B)
    lp = (pca ** 2).reshape(C, -1).mean(1)
    lb = (betas ** 2).reshape(C, -1).mean(1)
    v = vh.reshape(C, B, -1)
    sm = ((v[:, 1:] - v[:, :-1]) ** 2).reshape(C, -1).mean(1) if B > 1 else torch.zeros_like(lp)
    total = lw["lw_kp2d"] * L2 + lw["lw_kp3d"] * L3 + lw["lw_pca"] * lp + lw["lw_beta"] * lb + lw["lw_smooth"] * sm
    zero = torch.zeros_like(lp)
    return torch.stack([L2, L3, lp, zero, zero, sm, lb, total], 1), vh, X


def fit(mano_model, side, data, rot6d0, trans0, steps, lr, lw, sigma, znear, B, dtype, pca_dim=45, optimize_betas=True):
    """The whole fit in `dtype`: -> dict(log (steps,C,8) the values before every update, vals (C,8) at the final parameters,
    candidate, rot6d, trans, pca, betas, verts_world, keypoints), numpy float64"""
    mano = Mano(mano_model, side, dtype)
    cast = lambda t: None if t is None else torch.as_tensor(np.asarray(t)).to(dtype)
    data = {k: cast(v) for k, v in data.items()}
    N = rot6d0.shape[0]
    rot6d, trans = cast(rot6d0).clone().requires_grad_(True), cast(trans0).clone().requires_grad_(True)
    pca = torch.zeros(N, pca_dim, dtype=dtype, requires_grad=True)
    betas = torch.zeros(N, 10, dtype=dtype, requires_grad=True)
    p = (rot6d, trans, pca, betas)
    opt = torch.optim.Adam([{"params": [trans], "lr": lr}, {"params": [rot6d], "lr": lr * 10},
                            {"params": [pca] + ([betas] if optimize_betas else []), "lr": lr * 10}])
    log, X0 = [], None
    for _ in range(steps):
        opt.zero_grad()
        vals, _, X = all_terms(mano, p, data, lw, sigma, znear, B)
        X0 = X.detach().numpy().astype(np.float64) if X0 is None else X0
        log.append(vals.detach().numpy().astype(np.float64))
        vals[:, 7].sum().backward()
        opt.step()
    with torch.no_grad():
        vals, vh, X = all_terms(mano, p, data, lw, sigma, znear, B)
    n64 = lambda t: t.detach().numpy().astype(np.float64)
    totals = np.nan_to_num(n64(vals[:, 7]), nan=np.inf)
    return dict(log=np.stack(log) if log else np.zeros((0, N // B, 8)), vals=n64(vals), candidate=int(np.argmin(totals)),
                rot6d=n64(rot6d), trans=n64(trans), pca=n64(pca), betas=n64(betas), verts_world=n64(vh), keypoints=n64(X),
                keypoints0=n64(X) if X0 is None else X0)


# ---------------------------------------------------------------------------------------------- the shared scene
LW = dict(lw_kp2d=1.0, lw_kp3d=100.0, lw_pca=0.004, lw_beta=0.01, lw_smooth=10.0)
SIGMA, ZNEAR, LR, STEPS = 1.0, 0.01, 1e-2, 30


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    m = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}
    return np.array(m[axis], np.float64)


def scene(side="right", B=3, seed=0, with3d=False):
    """Keypoints of a known pose of the synthetic model, B = 3 frames; C = 2 candidate starts: the true rotation turned by a
    quarter turn about the camera's z axis, and the same start turned by a further half turn about the camera's y axis (the hand
    seen from behind).  One keypoint of frame 1 is a missing detection (confidence 0, NaN target).
    -> dict(mano, side, data (per-row float32 arrays tiled over the candidates), rot6d0, trans0, gt)"""
    mano_model = synthetic_mano(0)
    rng = np.random.default_rng(seed)
    m32 = Mano(mano_model, side, torch.float64)
    pca = np.zeros((B, 45))
    pca[:, :16] = rng.normal(size=16)[None] * 0.4 + rng.normal(size=(B, 16)) * 0.03
    R_col = np.stack([_rot("z", 0.3 + 0.02 * b) @ _rot("y", 0.4) @ _rot("x", -0.3) for b in range(B)])
    R = np.transpose(R_col, (0, 2, 1))                                   # row-vector convention: verts @ R
    t = np.stack([[0.02 + 0.004 * b, -0.01, 0.5] for b in range(B)])
    with torch.no_grad():
        vm, _ = m32(torch.from_numpy(pca), torch.zeros(B, 10, dtype=torch.float64))
        vh = vm @ torch.from_numpy(R) + torch.from_numpy(t)[:, None]
        X = torch.einsum("kv,nvc->nkc", m32.W, vh).numpy()
        tmpl = torch.einsum("kv,vc->kc", m32.W, m32(torch.zeros(1, 45, dtype=torch.float64), torch.zeros(1, 10, dtype=torch.float64))[0][0])
    f, c0 = 480.0 * 256 / 350.0, 128.0
    K = np.tile(np.array([[f, 0, c0], [0, f, c0], [0, 0, 1.0]]), (B, 1, 1))
    kp2d = np.stack([f * X[..., 0] / X[..., 2] + c0, f * X[..., 1] / X[..., 2] + c0], -1)
    c2 = np.ones((B, 21))
    kp2d[1 % B, 7] = np.nan
    c2[1 % B, 7] = 0.0
    kp3d = X - X[:, :1]
    quarter, half = _rot("z", np.pi / 2).T, _rot("y", np.pi).T          # applied after R, in camera space (row vectors)
    cands = np.stack([R @ quarter, R @ quarter @ half])                   # (C,B,3,3)
    C = cands.shape[0]
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    tk = torch.einsum("kc,nbcd->nbkd", tmpl.float(), f32(cands))
    z, x, y = handinit.initial_translation(f32(kp2d)[None].expand(C, B, 21, 2), f32(c2)[None].expand(C, B, 21),
                                           f32(K)[None].expand(C, B, 3, 3), tk)
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32)[None], (C,) + np.asarray(a).shape)
                                          .reshape((C * B,) + np.asarray(a).shape[1:]))
    data = dict(camintr=tile(K), kp2d=tile(kp2d), c2=tile(c2), s=tile(handinit.box_scales(f32(kp2d), f32(c2)).numpy()))
    if with3d:
        data.update(kp3d=tile(kp3d), c3=tile(np.ones((B, 21))))
    return dict(mano=mano_model, side=side, B=B, C=C, data=data, cands=cands.astype(np.float32),
                rot6d0=np.ascontiguousarray(cands[..., :2].reshape(C * B, 3, 2).astype(np.float32)),
                trans0=torch.stack([x, y, z], -1).reshape(C * B, 3).numpy().astype(np.float32),
                gt=dict(pca=pca, R=R, t=t, keypoints=X, kp2d=kp2d, K=K, c2=c2, kp3d=kp3d))


_FITS = {}


def scene_fits(with3d=True):
    """the shared scene with the restatement's float64 and float32 fits (computed once per process)"""
    if with3d not in _FITS:
        sc = scene(with3d=with3d)
        run = lambda dt: fit(sc["mano"], sc["side"], sc["data"], sc["rot6d0"], sc["trans0"], STEPS, LR, LW, SIGMA, ZNEAR, sc["B"], dt)
        _FITS[with3d] = (sc, run(torch.float64), run(torch.float32))
    return _FITS[with3d]


def px_error(res, sc, cand=None):
    """mean 2-D keypoint error in box units of candidate `cand` (default: the selected one) of a fit result / of `keypoints`"""
    c = res["candidate"] if cand is None else cand
    B, gt = sc["B"], sc["gt"]
    X = np.asarray(res["keypoints"], np.float64)[c * B:(c + 1) * B]
    f, c0 = gt["K"][0, 0, 0], gt["K"][0, 0, 2]
    p = np.stack([f * X[..., 0] / X[..., 2] + c0, f * X[..., 1] / X[..., 2] + c0], -1)
    e = np.linalg.norm(p - np.nan_to_num(gt["kp2d"]), axis=-1) / sc["data"]["s"][:B, None]
    return float((e * (gt["c2"] > 0)).sum() / (gt["c2"] > 0).sum())


def random_inputs(N, clip_len, seed, with3d, mano_model=None, side="right"):
    """kernel-level inputs: camera-space vertices of random poses, noisy targets, a few zero confidences with NaN targets"""
    rng = np.random.default_rng(seed)
    m = Mano(synthetic_mano(0) if mano_model is None else mano_model, side, torch.float64)
    pca = np.zeros((N, 45))
    pca[:, :16] = rng.normal(size=(N, 16)) * 0.5
    with torch.no_grad():
        vm = m(torch.from_numpy(pca), torch.from_numpy(rng.normal(size=(N, 10)) * 0.3))[0].numpy()
    verts = (vm + np.array([0.0, 0.0, 0.5]) + rng.normal(size=(N, 1, 3)) * 0.03).astype(F)
    W = m.W.numpy().astype(F)
    f = 351.0
    K = np.tile(np.array([[f, 0, 128.0], [0, f * 1.01, 120.0], [0, 0, 1.0]], F), (N, 1, 1))
    X = np.einsum("kv,nvc->nkc", W.astype(np.float64), verts.astype(np.float64))
    kp2d = np.stack([f * X[..., 0] / X[..., 2] + 128, f * 1.01 * X[..., 1] / X[..., 2] + 120], -1) + rng.normal(size=(N, 21, 2)) * 6
    c2 = rng.uniform(0.2, 1.0, size=(N, 21))
    miss = rng.uniform(size=(N, 21)) < 0.15
    c2[miss] = 0
    kp2d[miss] = np.nan
    out = dict(verts=verts, W=W, camintr=K, kp2d=kp2d.astype(F), c2=c2.astype(F),
               s=handinit.box_scales(torch.from_numpy(kp2d.astype(F)), torch.from_numpy(c2.astype(F))).numpy().astype(F),
               kp3d=None, c3=None)
    if with3d:
        kp3d = (X - X[:, :1]) + rng.normal(size=(N, 21, 3)) * 0.01
        c3 = rng.uniform(0.2, 1.0, size=(N, 21))
        miss3 = rng.uniform(size=(N, 21)) < 0.1
        c3[miss3] = 0
        kp3d[miss3] = np.nan
        out.update(kp3d=kp3d.astype(F), c3=c3.astype(F))
    return out
