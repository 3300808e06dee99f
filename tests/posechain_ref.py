"""Pose chain (csrc/mano.hip, csrc/geometry.hip): float64 references and the shared case grids of tests/test_posechain_refs.py
(references against the float32 CPU oracle, float32 floors) and tests/test_posechain_edges_gpu.py (kernels against the references).

Plain float64 torch with autograd.  No kernel and none of the written-out C oracles (oracle/csrc) is involved: the MANO layer is
built from the RAW model dictionary (v_template, shapedirs, posedirs, J_regressor, lbs_weights, parents), so the host-side folding
of the joint regressor into J_template / J_shapedirs (homan_amd.mano_assets.kernel_layout) is under test as well.
"""
import numpy as np
import torch

F64 = torch.float64


def _t64(x):
    return x.detach().to(F64) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(F64)


# ===================================================================== MANO layer
def rodrigues(r):
    """(n,3) axis-angle -> (n,3,3): angle = |r + 1e-8|, dir = r / angle, R = I + sin K + (1 - cos) K K (smplx.lbs.batch_rodrigues)"""
    angle = torch.sqrt(((r + 1e-8) ** 2).sum(1, keepdim=True))
    d = r / angle
    zero = torch.zeros_like(d[:, 0])
    K = torch.stack([zero, -d[:, 2], d[:, 1], d[:, 2], zero, -d[:, 0], -d[:, 1], d[:, 0], zero], 1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=r.dtype)[None]
    return eye + torch.sin(angle)[:, None] * K + (1 - torch.cos(angle))[:, None] * (K @ K)


def mano_layer(model, pca, rot, betas, trans=None, flat_hand_mean=False):
    """pose = pca[:, :16] @ comps + hand_mean; shape and pose blend shapes, joint regression, kinematic chain over `parents`,
    rest-pose removal, skinning -> (vertices + trans (B,778,3), posed joints + trans (B,16,3)).  dtype: that of `pca`."""
    dt = pca.dtype
    g = lambda k: torch.as_tensor(np.asarray(model[k])).to(dt)
    vt, sd, pd, jreg, W = g("v_template"), g("shapedirs"), g("posedirs"), g("J_regressor"), g("lbs_weights")
    parents = [int(p) for p in np.asarray(model["parents"])]
    comps = g("hand_components")[:16]
    mean = torch.zeros(45, dtype=dt) if flat_hand_mean else g("hand_mean")
    B = pca.shape[0]
    pose = torch.cat([rot, pca[:, :16] @ comps + mean[None]], 1)
    v_shaped = vt[None] + torch.einsum("bl,vcl->bvc", betas, sd)
    J = torch.einsum("jv,bvc->bjc", jreg, v_shaped)
    R = rodrigues(pose.reshape(-1, 3)).view(B, 16, 3, 3)
    feat = (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(B, 135)
    v_posed = v_shaped + (feat @ pd).view(B, -1, 3)
    Rw, tw = [None] * 16, [None] * 16
    for j, p in enumerate(parents):
        if p < 0:
            Rw[j], tw[j] = R[:, j], J[:, j]
        else:
            Rw[j] = Rw[p] @ R[:, j]
            tw[j] = (Rw[p] @ (J[:, j] - J[:, p])[..., None])[..., 0] + tw[p]
    Rw, tw = torch.stack(Rw, 1), torch.stack(tw, 1)
    At = tw - (Rw @ J[..., None])[..., 0]                              # rest pose removed
    TR, Tt = torch.einsum("vj,bjik->bvik", W, Rw), torch.einsum("vj,bji->bvi", W, At)
    verts = torch.einsum("bvik,bvk->bvi", TR, v_posed) + Tt
    if trans is not None:
        verts, tw = verts + trans[:, None], tw + trans[:, None]
    return verts, tw


def mano_ref(model, pca, rot, betas, trans, gout=None, flat_hand_mean=False, g_pca_extra=None, w_extra=0.0, dtype=F64):
    """-> dict(verts, joints[, g_pca (B,pca_dim), g_rot, g_betas, g_trans]) for the upstream gradient `gout` (B,778,3) on the
    vertices; g_pca additionally gets w_extra * g_pca_extra (columns >= 16 receive nothing else)."""
    ins = [torch.as_tensor(np.asarray(x)).to(dtype).requires_grad_(True) for x in (pca, rot, betas, trans)]
    v, j = mano_layer(model, *ins, flat_hand_mean=flat_hand_mean)
    out = dict(verts=v.detach(), joints=j.detach())
    if gout is not None:
        (v * torch.as_tensor(np.asarray(gout)).to(dtype)).sum().backward()
        gp = ins[0].grad
        if g_pca_extra is not None:
            gp = gp + float(np.float32(w_extra)) * torch.as_tensor(np.asarray(g_pca_extra)).to(dtype)
        out.update(g_pca=gp, g_rot=ins[1].grad, g_betas=ins[2].grad, g_trans=ins[3].grad)
    return out


# ===================================================================== rigid transform
def rot6d_to_matrix(r6):
    """reference homan/utils/geometry.py:9-27 in the dtype of `r6`: b1 = a1 / max(|a1|, 1e-12), u = a2 - (b1.a2) b1, b2 = u / max(|u|,
    1e-12), b3 = b1 x b2, columns of R.  (oracle.model.rot6d_to_matrix rounds its norms to float32: restated.)  The norm's
    gradient at the zero vector is torch's subgradient 0, so a clamped normalisation passes g / 1e-12 straight through."""
    r = r6.reshape(-1, 3, 2)
    a1, a2 = r[:, :, 0], r[:, :, 1]
    b1 = a1 / torch.linalg.vector_norm(a1, dim=1, keepdim=True).clamp_min(1e-12)
    u = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    b2 = u / torch.linalg.vector_norm(u, dim=1, keepdim=True).clamp_min(1e-12)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-1)


def frame_scales(scale, N, clip_len):
    """one scale per clip -> one per frame"""
    return scale.reshape(-1).repeat_interleave(clip_len if clip_len else N)


def rigid_ref(mesh, rot6d, trans, scale, clip_len=0, abs_scale=False, terms=(), weights=(), g_rigid=None, g_frame=None,
              frame_scale=1.0, g_full_extra=None, dtype=F64, rot_fn=None):
    """(s mesh) @ R(rot6d) + t with one scale per clip (|s| if abs_scale) and the gradients of
        sum(verts * g_full) + sum(twin * (g_rigid + frame_scale * g_frame[:, None, :3]))
    g_full = sum_k weights[k] terms[k] (+ g_full_extra, already in `dtype`), twin = the mesh-detached vertices (their gradient
    reaches R and t only).  -> dict(verts, rotmat, g_mesh, g_rot6d (N,3,2), g_trans (N,3), g_scale (N,): per FRAME, the addends of
    the clip's scale gradient, w.r.t. the raw scale)."""
    from oracle import model as om
    c = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)
    N, V = mesh.shape[:2]
    m, r6, t = c(mesh).requires_grad_(True), c(rot6d).requires_grad_(True), c(trans).reshape(N, 3).requires_grad_(True)
    sf = frame_scales(c(scale), N, clip_len).clone().requires_grad_(True)
    R = (rot_fn or rot6d_to_matrix)(r6)
    v, vd = om.transform_persp(m, t[:, None], R, sf.abs() if abs_scale else sf)
    out = dict(verts=v.detach(), rotmat=R.detach())
    g_full = torch.zeros(N, V, 3, dtype=dtype)
    for tk, wk in zip(terms, weights):
        g_full = g_full + float(np.float32(wk)) * c(tk)
    if g_full_extra is not None:
        g_full = g_full + g_full_extra.to(dtype)
    g_tw = torch.zeros(N, V, 3, dtype=dtype)
    if g_rigid is not None:
        g_tw = g_tw + c(g_rigid)
    if g_frame is not None:
        g_tw = g_tw + float(np.float32(frame_scale)) * c(g_frame)[:, None, :3]
    ((v * g_full).sum() + (vd * g_tw).sum()).backward()
    out.update(g_mesh=m.grad, g_rot6d=r6.grad, g_trans=t.grad, g_scale=sf.grad, g_full=g_full)
    return out


# ===================================================================== silhouette gather and smoothness inside the rigid backward
def sil_gather_ref(parts, adj_off, adj_items, cam_verts, K, orig_size):
    """The work of k_bwd_gather in float64: per-corner NDC gradients (B,F,3,2) summed onto their vertices through the CSR adjacency
    (item = face * 3 + corner), then the backward of the projection  u = 2 (K00 x/z' + K01 y/z' + K02) / orig - 1,
    v = -(2 (K10 x/z' + K11 y/z' + K12) / orig - 1), z' = z + 1e-9, by autograd.  -> (B,V,3) float64"""
    p = _t64(parts).reshape(parts.shape[0], -1, 2)
    off, items = np.asarray(adj_off, np.int64), torch.as_tensor(np.asarray(adj_items, np.int64))
    B, V = cam_verts.shape[:2]
    owner = torch.as_tensor(np.repeat(np.arange(V), np.diff(off)))
    g_ndc = torch.zeros(B, V, 2, dtype=F64)
    g_ndc.index_add_(1, owner, p[:, items])
    cv, K = _t64(cam_verts).requires_grad_(True), _t64(K)
    zz = cv[..., 2] + 1e-9
    xn, yn = cv[..., 0] / zz, cv[..., 1] / zz
    u = 2.0 * (K[:, None, 0, 0] * xn + K[:, None, 0, 1] * yn + K[:, None, 0, 2]) / orig_size - 1.0
    v = -(2.0 * (K[:, None, 1, 0] * xn + K[:, None, 1, 1] * yn + K[:, None, 1, 2]) / orig_size - 1.0)
    ((u * g_ndc[..., 0]).sum() + (v * g_ndc[..., 1]).sum()).backward()
    return cv.grad


def smooth_grad_ref(verts, clip_len, weight):
    """weight * d mean((v[t+1] - v[t])^2) / dv per clip of clip_len frames (reference homan/lossutils.py:18-36; a clip of one frame
    has no pair and no term) -> (N,V,3) float64"""
    v = _t64(verts).requires_grad_(True)
    N = v.shape[0]
    cl = clip_len if clip_len else N
    if cl < 2:
        return torch.zeros_like(v).detach()
    c = v.reshape(N // cl, cl, *v.shape[1:])
    (float(np.float32(weight)) * ((c[:, 1:] - c[:, :-1]) ** 2).mean((1, 2, 3)).sum()).backward()
    return v.grad


# ===================================================================== shared inputs
def rng(*key):
    return np.random.default_rng([20240, *key])


def mano_params(B, pca_dim=16, seed=0):
    """random float32 hand parameters of B rows: dict(pca (B,pca_dim), rot, betas, trans, gout (B,778,3))"""
    r = rng(1, B, pca_dim, seed)
    f = np.float32
    return dict(pca=(r.normal(size=(B, pca_dim)) * 0.4).astype(f), rot=(r.normal(size=(B, 3)) * 0.5).astype(f),
                betas=(r.normal(size=(B, 10)) * 0.5).astype(f), trans=(r.normal(size=(B, 3)) * 0.05).astype(f),
                gout=r.normal(size=(B, 778, 3)).astype(f))


POSE_EDGES = ("zero", "tiny", "near_pi", "beyond_2pi", "betas3")


def pose_edge_params(kind):
    """B = 4 rows where the formulas turn -> (params, flat_hand_mean).  The wrist carries the special angle, about x, y, -z and
    the diagonal in the four rows (a finger joint's angle is pca @ comps + mean and cannot be set exactly through 16 components);
    "zero": pca = 0 on the flat_hand_mean layout and rot = 0 - every one of the sixteen joints is exactly zero."""
    p = mano_params(4, 16, seed=len(kind))
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, -1], [3 ** -0.5] * 3], np.float64)
    flat = False
    if kind == "zero":
        p["pca"][:], p["rot"][:], flat = 0.0, 0.0, True
    elif kind == "tiny":
        p["rot"] = (axes * 1e-6).astype(np.float32)
    elif kind == "near_pi":
        p["rot"] = (axes * (np.pi - np.array([1e-3, 1e-4, -1e-3, 5e-4]))[:, None]).astype(np.float32)
    elif kind == "beyond_2pi":
        p["rot"] = (axes * 7.5).astype(np.float32)
    elif kind == "betas3":
        p["betas"] = np.where(rng(2).random((4, 10)) < 0.5, -3.0, 3.0).astype(np.float32)
    else:
        raise ValueError(kind)
    return p, flat


MANO_B = (1, 3, 4, 5, 9)
# fused rigid backward: (n_terms, g_rigid, frame_stride or 0 = no g_frame); every value of each of the three parts
FUSED_PARTS = ((0, True, 0), (2, False, 3), (5, True, 5))


def rigid_pose(N, nclips, seed=0, negative=True):
    """rot6d (N,3,2), trans (N,3), one scale per clip (distinct; the last negative if asked) float32"""
    r = rng(3, N, nclips, seed)
    scale = (0.7 + 0.45 * np.arange(nclips) + 0.1 * r.random(nclips)).astype(np.float32)
    if negative:
        scale[-1] = -scale[-1]
    return (r.normal(size=(N, 3, 2)).astype(np.float32), (r.normal(size=(N, 3)) * 0.3 + [0.0, 0.0, 0.6]).astype(np.float32), scale)


def fused_inputs(B, n_terms, g_rigid, frame_stride, seed=0):
    """per-vertex inputs of the fused rigid backward on the hand's 778 vertices"""
    r = rng(4, B, n_terms, frame_stride, seed)
    f = np.float32
    return dict(terms=[r.normal(size=(B, 778, 3)).astype(f) for _ in range(n_terms)],
                weights=(r.uniform(0.3, 2.0, size=n_terms) * np.where(np.arange(n_terms) % 2, -1, 1)).astype(f),
                g_rigid=r.normal(size=(B, 778, 3)).astype(f) if g_rigid else None,
                g_frame=r.normal(size=(B, frame_stride)).astype(f) if frame_stride else None, frame_scale=f(0.37))


def mano_fused_ref(model, p, rp, clip_len, fi, dtype=F64, layer=None):
    """MANO layer -> hand rigid transform (no abs on the scale) -> the fused backward's six gradients, by autograd through both.
    p: mano_params, rp: rigid_pose, fi: fused_inputs.  layer(pca, rot, betas, trans) -> verts replaces the float64 layer (the
    float32 oracle)."""
    from oracle import model as om
    c = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)
    ins = [c(p[k]).requires_grad_(True) for k in ("pca", "rot", "betas", "trans")]
    vm = layer(*ins) if layer else mano_layer(model, *ins)[0]
    B = vm.shape[0]
    r6, t = c(rp[0]).requires_grad_(True), c(rp[1]).requires_grad_(True)
    sf = frame_scales(c(rp[2]), B, clip_len)
    R = rot6d_to_matrix(r6) if dtype == F64 else om.rot6d_to_matrix(r6)
    v, vd = om.transform_persp(vm, t[:, None], R, sf)
    g_full, g_tw = torch.zeros(B, 778, 3, dtype=dtype), torch.zeros(B, 778, 3, dtype=dtype)
    for tk, wk in zip(fi["terms"], fi["weights"]):
        g_full = g_full + c(wk) * c(tk)
    if fi["g_rigid"] is not None:
        g_tw = g_tw + c(fi["g_rigid"])
    if fi["g_frame"] is not None:
        g_tw = g_tw + c(fi["frame_scale"]) * c(fi["g_frame"])[:, None, :3]
    ((v * g_full).sum() + (vd * g_tw).sum()).backward()
    z = lambda x: x.grad if x.grad is not None else torch.zeros_like(x)
    return dict(verts=vm.detach(), verts_world=v.detach(), g_pca=z(ins[0]), g_rot=z(ins[1]), g_betas=z(ins[2]), g_trans=z(ins[3]),
                g_rot6d=z(r6), g_rigid_trans=z(t))


# ---- rigid transform grids
RIGID_FWD_V = (1, 255, 256, 257)
RIGID_FWD_N = (1, 3)
# non-exact backward: (N, V).  threads = 256 up to V = 512, 1024 above; chunks = ceil(V / (4 threads)) with a workspace: one up to
# 4096 (1024 threads), two at 4097, sixteen first at 15 * 4096 + 1 = 61441
RIGID_BWD = ((3, 1), (3, 512), (3, 513), (3, 4096), (3, 4097), (2, 61441))
RIGID_EXACT_V = (256, 257, 4096, 4097, 24576, 24577)          # N = 2


def rigid_bwd_inputs(N, V, seed=0):
    """mesh, pose (clips of one frame for N = 3 -> three scales, the last negative; N = 2 -> two), two weighted terms, g_rigid,
    g_frame (stride 4)"""
    r = rng(5, N, V, seed)
    f = np.float32
    rot6d, trans, scale = rigid_pose(N, N, seed)
    return dict(mesh=(r.normal(size=(N, V, 3)) * 0.1).astype(f), rot6d=rot6d, trans=trans, scale=scale,
                terms=[r.normal(size=(N, V, 3)).astype(f) for _ in range(2)], weights=np.asarray([1.3, -0.6], f),
                g_rigid=r.normal(size=(N, V, 3)).astype(f), g_frame=r.normal(size=(N, 4)).astype(f), frame_scale=f(0.81))


DEGENERATE_ROT6D = {"first_zero": [[0, 0.3], [0, -1.1], [0, 0.7]], "parallel": [[1, 2], [0, 0], [0, 0]]}


def degenerate_inputs(kind, N=2, V=257):
    d = rigid_bwd_inputs(N, V, seed=7)
    d["rot6d"] = np.tile(np.asarray(DEGENERATE_ROT6D[kind], np.float32)[None], (N, 1, 1))
    return d


# ---- the exact backward's synthetic silhouette sums
QUANTUM = 2.0 ** -44


def fan_mesh(V):
    """A small generated topology over V vertices: a strip of triangles (i, i+1, i+2) over vertices 1 .. V-2 plus a fan of 12
    triangles around vertex 1; vertex 0 is in no face (valence 0), vertex 1 has valence > 8, the last vertex valence 1.
    -> faces (F,3) int32"""
    assert V >= 16
    strip = np.stack([np.arange(1, V - 2), np.arange(2, V - 1), np.arange(3, V)], 1)
    fan = np.stack([np.full(12, 1), np.arange(2, 14), np.arange(3, 15)], 1)
    return np.concatenate([strip, fan]).astype(np.int32)


def exact_inputs(N, V, seed=0, clip_len=1):
    """mesh in front of the camera, its pose, camera-space vertices (float32 of the float64 transform: any float32 will do, they
    are an INPUT of the backward), K, per-corner sums that are multiples of the quantum 2^-44 (|value| < 2^-10), two terms."""
    r = rng(6, N, V, seed)
    f = np.float32
    faces = fan_mesh(V)
    nclips = N // clip_len
    rot6d, trans, scale = rigid_pose(N, nclips, seed)
    mesh = (r.normal(size=(N, V, 3)) * 0.1).astype(f)
    cam = rigid_ref(mesh, rot6d, trans, scale, clip_len, True)["verts"].numpy().astype(f)
    K = np.tile(np.array([[1.37, 0.02, 0.5], [0, 1.41, 0.48], [0, 0, 1.0]], f), (N, 1, 1))
    parts = r.integers(-2 ** 34, 2 ** 34, size=(N, len(faces), 3, 2)).astype(np.float64) * QUANTUM
    return dict(mesh=mesh, rot6d=rot6d, trans=trans, scale=scale, faces=faces, cam_verts=cam, K=K, parts=parts, orig_size=1.0,
                terms=[(r.normal(size=(N, V, 3)) * 1e-3).astype(f) for _ in range(2)], weights=np.asarray([0.9, -1.7], f))


def rigid_oracle32(d, clip_len, abs_scale, g_full_extra=None, with_twin=True, rot_fn=None):
    """the float32 CPU oracle of the rigid backward: oracle.model.rot6d_to_matrix + transform_persp + autograd"""
    from oracle import model as om
    return rigid_ref(d["mesh"], d["rot6d"], d["trans"], d["scale"], clip_len, abs_scale, d.get("terms", ()), d.get("weights", ()),
                     d.get("g_rigid") if with_twin else None, d.get("g_frame") if with_twin else None, d.get("frame_scale", 1.0),
                     g_full_extra, dtype=torch.float32, rot_fn=rot_fn or om.rot6d_to_matrix)


def rot6d_gain(rot6d):
    """max_i sum_k |dR_k / dr6_i| per frame (float64 autograd): an error of e in each of the nine sums dR moves a component of
    g_rot6d = J^T dR by at most gain * e.  -> (N,) numpy"""
    out = []
    for r in np.asarray(rot6d, np.float64).reshape(-1, 6):
        J = torch.autograd.functional.jacobian(lambda x: rot6d_to_matrix(x).reshape(9), torch.from_numpy(r))
        out.append(float(J.abs().sum(0).max()))
    return np.asarray(out)


# ---- the MANO grid: name -> (model key "right" / "left", params, flat_hand_mean)
def mano_cases():
    cases = {f"B{B}": ("right", mano_params(B), False) for B in MANO_B}
    for B in (1, 3):                                                  # two hands interleaved frame-major: row = 2 frame + hand
        both = mano_params(2 * B, seed=3)
        for h, side in enumerate(("right", "left")):
            cases[f"rows_B{B}_hand{h}"] = (side, {k: np.ascontiguousarray(v[h::2]) for k, v in both.items()}, False)
    cases["clips"] = ("right", mano_params(9, seed=1), False)
    cases["pca45"] = ("right", mano_params(3, 45), False)
    for kind in POSE_EDGES:
        p, flat = pose_edge_params(kind)
        cases[kind] = ("right", p, flat)
    return cases


def mano_models():
    from homan_amd.mano_assets import mirrored, synthetic_mano
    right = synthetic_mano(0)
    return {"right": right, "left": mirrored(right)}


def mano_oracle32(model, p, flat_hand_mean=False):
    """the float32 CPU oracle: oracle.lbs.ManoLayer + autograd -> the outputs of mano_ref"""
    from oracle import lbs
    layer = lbs.ManoLayer(model, num_pca_comps=16, flat_hand_mean=flat_hand_mean)
    ins = [torch.from_numpy(np.asarray(p[k], np.float32)).clone().requires_grad_(True) for k in ("pca", "rot", "betas", "trans")]
    v, j = layer(betas=ins[2], global_orient=ins[1], hand_pose=ins[0][:, :16] @ layer.hand_components, transl=ins[3])[:2]
    (v * torch.from_numpy(p["gout"])).sum().backward()
    return dict(verts=v.detach(), joints=j.detach(), g_pca=ins[0].grad, g_rot=ins[1].grad, g_betas=ins[2].grad, g_trans=ins[3].grad)


def mano_oracle32_layer(model):
    """(pca, rot, betas, trans) -> vertices through oracle.lbs.ManoLayer, for mano_fused_ref(dtype=float32)"""
    from oracle import lbs
    layer = lbs.ManoLayer(model, num_pca_comps=16, flat_hand_mean=False)
    return lambda pca, rot, betas, trans: layer(betas=betas, global_orient=rot, hand_pose=pca[:, :16] @ layer.hand_components,
                                                transl=trans)[0]


# (N, clip_len, V) of the smoothness-inside-the-backward cases: no pair | one pair | three clips of three, no pair across a clip
# boundary (k_rigid_bwd_x<1,1024>, two chunks) | the two-vertices-per-thread instantiation
SMOOTH_CASES = ((2, 1, 257), (2, 2, 257), (9, 3, 257), (2, 2, 4097))
SMOOTH_WEIGHT = 0.6


def exact_extra(d, clip_len=1, smooth=False):
    """float64 per-vertex gradient the exact backward forms itself: silhouette gather (+ smoothness of the camera-space vertices)"""
    from oracle import objchain
    adj = objchain.build_adjacency(d["faces"], d["mesh"].shape[1])
    g = sil_gather_ref(d["parts"], adj[0], adj[1], d["cam_verts"], d["K"], d["orig_size"])
    if smooth:
        g = g + smooth_grad_ref(d["cam_verts"], clip_len, SMOOTH_WEIGHT)
    return g, adj
