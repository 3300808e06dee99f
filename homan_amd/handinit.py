"""Hand initialisation: MANO fitted to 21 2-D (and optionally 3-D) keypoints per frame, on HIP (csrc/handinit.hip).

The reference has no counterpart: its `person_parameters` come from a hand-pose network (homan/mocap.py:34-113,
homan/prepare/frameinfos.py:90-184), which is out of scope here.  This is the optimisation-based start for a user who has
keypoints - a 2-D detector's, HO-3D's annotation, a 3-D lifter's: the rules are DESIGN.md section 7 ("Hand initialisation from
keypoints") and include/homan_amd.h; `fit_hands_to_keypoints` returns what `optimize_hand_object` / `build_model` take.

A row is one frame of one candidate start, a clip of B rows one candidate track; the C candidates of a hand are fitted side by
side as a clip batch (N = C * B rows), each step being
    hm_mano_fwd_clips -> hm_keypoint_terms_clips -> hm_smooth_fwd_clips -> hm_priors_fwd_clips -> hm_mano_bwd_rigid_clips
    -> hm_handinit_finish_clips -> hm_adam_step
on ONE stream, captured in a hipGraph of several steps.  There is no CPU path.
"""
import math

import numpy as np
import torch

from . import lib as _lib
from . import ops
from .loopcommon import HmAdam
from .mano_assets import hand_models
from .postprocess import JOINT_ORDER, TIP_VERTS

NS = 8                       # a clip's row of values: {L2d, L3d, Lpca, -, -, Lsmooth, Lbeta, total} (include/homan_amd.h)
SLOTS = ("kp2d", "kp3d", "pca", None, None, "smooth", "beta", "total")
GRAPH_STEPS = 5              # steps per replay of the captured loop
# Not tuned on real detections: the 2-D term is a mean over keypoints of squared residuals in box units,
# the 3-D term a mean of squared metres, the priors as in the joint fit (lw_pca) or weak (lw_beta).
DEFAULT_LOSS_WEIGHTS = dict(lw_kp2d=1.0, lw_kp3d=100.0, lw_pca=0.004, lw_beta=0.01, lw_smooth=10.0)
DEFAULT_SIGMA, DEFAULT_ZNEAR = 1.0, 0.01


def keypoint_regressor(mano_model_np):
    """W (21,778) fp32: the 16 rows of the model's J_regressor, five one-hot rows at TIP_VERTS, permuted by JOINT_ORDER - the
    21 joints in the order of `postprocess`, as a LINEAR map of the posed vertices (not the posed kinematic joints)."""
    jreg = np.asarray(mano_model_np["J_regressor"], np.float32)
    if jreg.shape != (16, 778):
        raise ValueError(f"J_regressor has shape {jreg.shape}, expected (16, 778)")
    tips = np.zeros((len(TIP_VERTS), 778), np.float32)
    tips[np.arange(len(TIP_VERTS)), list(TIP_VERTS)] = 1.0
    return np.ascontiguousarray(np.concatenate([jreg, tips])[list(JOINT_ORDER)])


def box_scales(kp2d, c2):
    """s (...,) in pixels: the larger extent of each frame's confident 2-D keypoints, floored at 1 (1 without any)."""
    ext = _extent(kp2d, c2 > 0)
    return ext.clamp_min(1.0)


def _extent(pts, ok):
    """larger of the per-axis extents of the first two coordinates of pts (...,K,>=2) over the points `ok`; 0 without any"""
    big = torch.finfo(pts.dtype).max
    p = torch.nan_to_num(pts[..., :2], nan=0.0)
    hi = torch.where(ok[..., None], p, torch.full_like(p, -big)).amax(-2)
    lo = torch.where(ok[..., None], p, torch.full_like(p, big)).amin(-2)
    return torch.where(ok.any(-1), (hi - lo).amax(-1), torch.zeros_like(hi[..., 0]))


def initial_translation(kp2d, c2, camintr, template_keypoints):
    """-> (z, x, y), each (...,): the translation that puts the rotated template's keypoints (...,21,3) on the 2-D keypoints
    (...,21,2; pixels; confidences c2 (...,21)) under camintr (...,3,3; pixels).  z = focal length (the mean of fx and fy) times the
    metric extent of the template's confident keypoints over their 2-D extent; x, y put the keypoints' centroid on the 2-D
    centroid at that depth.  Host-side torch, run once per fit, like the object's TCO_init.  A frame without confident
    keypoints gets z = 1, x = y = 0."""
    ok = c2 > 0
    has = ok.any(-1)
    f = 0.5 * (camintr[..., 0, 0] + camintr[..., 1, 1])
    e2, e3 = _extent(kp2d, ok).clamp_min(1.0), _extent(template_keypoints, ok)
    z = torch.where(has & (e3 > 0), f * e3 / e2, torch.ones_like(f))
    w = ok.to(kp2d.dtype)
    cnt = w.sum(-1).clamp_min(1.0)
    m2 = (torch.nan_to_num(kp2d, nan=0.0) * w[..., None]).sum(-2) / cnt[..., None]
    m3 = (template_keypoints * w[..., None]).sum(-2) / cnt[..., None]
    depth = z + m3[..., 2]
    x = (m2[..., 0] - camintr[..., 0, 2]) / camintr[..., 0, 0] * depth - m3[..., 0]
    y = (m2[..., 1] - camintr[..., 1, 2]) / camintr[..., 1, 1] * depth - m3[..., 1]
    zero = torch.zeros_like(x)
    return z, torch.where(has, x, zero), torch.where(has, y, zero)


def default_candidates():
    """(8,3,3): {identity, half turn about the camera's y axis} x quarter turns about its z axis, as the row-vector rotations
    of the rigid transform (verts = mesh @ R + t).  Not tuned: a coarse cover of the palm's facing and in-plane direction."""
    out = []
    for half in (0.0, math.pi):
        ry = np.array([[math.cos(half), 0, math.sin(half)], [0, 1, 0], [-math.sin(half), 0, math.cos(half)]])
        for q in range(4):
            a = q * math.pi / 2
            rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
            out.append(np.round(rz @ ry).T)
    return torch.from_numpy(np.stack(out).astype(np.float32))


def rot6d_to_matrix(r6):
    """(n,3,2) -> (n,3,3): Gram-Schmidt, columns b1 b2 b3 (result formatting; the kernels convert in csrc/hm_common.h)"""
    a1, a2 = r6[:, :, 0], r6[:, :, 1]
    b1 = a1 / a1.norm(dim=1, keepdim=True).clamp_min(1e-12)
    u = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    b2 = u / u.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=1)), dim=-1)


def _check_weights(loss_weights):
    lw = dict(DEFAULT_LOSS_WEIGHTS)
    for k, v in (loss_weights or {}).items():
        if k not in lw:
            raise ValueError(f"unknown loss weight {k!r}; known: {sorted(lw)}")
        if not (float(v) >= 0 and math.isfinite(float(v))):
            raise ValueError(f"loss weight {k} = {v!r} must be finite and >= 0")
        lw[k] = float(v)
    return lw


class HandKeypointFitter:
    """The resident loop of one (side, B, C): buffers, Adam state and the captured graph outlive a fit; `load` installs another
    hand's keypoints and starts, `run` steps.  mode "fused": the launch sequence of the module docstring; "eager": the same terms
    through the autograd wrappers of homan_amd.ops (the fused step's check), same Adam launch."""

    def __init__(self, model_np, side, B, C, lr=1e-2, loss_weights=None, sigma=DEFAULT_SIGMA, znear=DEFAULT_ZNEAR, pca_dim=45,
                 max_steps=1024, mode="fused", optimize_betas=True, device="cuda"):
        if not torch.cuda.is_available():
            raise _lib.HomanAmdError("homan_amd.handinit needs the GPU (there is no CPU fallback)")
        if mode not in ("fused", "eager"):
            raise ValueError(f"mode {mode!r} not in [fused|eager]")
        if side not in ("right", "left"):
            raise ValueError(f"{side} not in [left|right]")
        if B < 1 or C < 1 or pca_dim < 16 or max_steps < 1:
            raise ValueError("B, C, max_steps must be >= 1 and pca_dim >= 16")
        if not (sigma > 0 and math.isfinite(sigma)):
            raise ValueError(f"sigma = {sigma!r} must be finite and > 0")
        self.side, self.B, self.C, self.N, self.P, self.mode = side, B, C, B * C, pca_dim, mode
        self.lr, self.lw, self.sigma, self.znear, self.max_steps = float(lr), _check_weights(loss_weights), float(sigma), float(znear), max_steps
        self.optimize_betas = bool(optimize_betas)
        self.L = _lib.lib()
        dev = self.device = torch.device(device)
        m = dict(model_np)
        if side == "left":             # the left path's sign flip of the PCA basis, as ManoModel._left_ctx folds it
            comps = np.array(m["hand_components"], np.float32, copy=True)
            comps[:, 1::3] *= -1.0
            comps[:, 2::3] *= -1.0
            m["hand_components"] = comps
        self.mctx = ops.ManoContext(m, dev, num_pca_comps=16, flat_hand_mean=False)
        self.W = torch.from_numpy(keypoint_regressor(model_np)).to(dev)
        self.faces = torch.from_numpy(np.asarray(model_np["faces"]).astype(np.int32))
        N, P = self.N, pca_dim
        z = lambda *s: torch.zeros(*s, device=dev)
        par = lambda *s: torch.nn.Parameter(z(*s))
        self.rot6d, self.trans, self.pca, self.betas = par(N, 3, 2), par(N, 3), par(N, P), par(N, 10)
        for p in (self.rot6d, self.trans, self.pca, self.betas):
            p.grad = torch.zeros_like(p)
        self.mano_rot, self.g_mano_rot, self.g_mano_trans = z(N, 3), z(N, 3), z(N, 3)
        self.ones_c, self.g_sc = torch.ones(C, device=dev), z(2, C)
        self.vm, self.vh = z(N, 778, 3), z(N, 778, 3)
        self.state = torch.empty(self.L.hm_mano_state_bytes(N), dtype=torch.uint8, device=dev)
        self.kp2d, self.c2, self.s, self.kp3d, self.c3 = z(N, 21, 2), z(N, 21), torch.ones(N, device=dev), z(N, 21, 3), z(N, 21)
        self.camintr = z(N, 3, 3)
        self.keypoints, self.U_kp, self.U_sm, self.U_pca = z(N, 21, 3), z(N, 778, 3), z(N, 778, 3), z(N, P)
        self.row_parts = z(N, 2)
        self.tickets = torch.zeros(C, dtype=torch.int32, device=dev)
        self.rws = torch.zeros(C * self.L.hm_reduce_workspace_bytes(), dtype=torch.uint8, device=dev)
        self.vals, self.log = z(C, NS), z(max_steps, C, NS)
        groups = [{"params": [self.trans], "lr": self.lr},
                  {"params": [self.rot6d, self.pca] + ([self.betas] if self.optimize_betas else []), "lr": self.lr * 10}]
        self.opt = HmAdam(groups)
        self.graph_k = self.graph_1 = None
        self.steps_done = 0
        # the template: keypoints of the zero pose, zero shape (initial_translation reads them)
        with torch.no_grad():
            self.rot6d[:, 0, 0] = 1.0
            self.rot6d[:, 1, 1] = 1.0
        self._forward()
        self.template_keypoints = torch.einsum("kv,vc->kc", self.W, self.vm[0]).clone()

    # ---------------------------------------------------------------- one fit's inputs
    def load(self, kp2d, c2, camintr, rotations, kp3d=None, c3=None):
        """kp2d (B,21,2) pixels, c2 (B,21), camintr (B,3,3) pixels, rotations (C,3,3) the candidates' starts, (or (C,B,3,3): per
        frame), kp3d (B,21,3) / c3 (B,21) optional.  Every candidate starts at the zero pose and shape under its rotation, placed by initial_translation."""
        B, C, dev = self.B, self.C, self.device
        f = lambda t: torch.as_tensor(t, dtype=torch.float32).to(dev)
        kp2d, c2, camintr, rotations = f(kp2d), f(c2), f(camintr), f(rotations)
        if rotations.dim() == 3:
            rotations = rotations[:, None].expand(rotations.shape[0], B, 3, 3)
        if kp2d.shape != (B, 21, 2) or c2.shape != (B, 21) or camintr.shape != (B, 3, 3) or rotations.shape != (C, B, 3, 3):
            raise ValueError(f"expected kp2d ({B},21,2), c2 ({B},21), camintr ({B},3,3), rotations ({C},3,3) or ({C},{B},3,3); got "
                             f"{tuple(kp2d.shape)}, {tuple(c2.shape)}, {tuple(camintr.shape)}, {tuple(rotations.shape)}")
        if (kp3d is None) != (c3 is None):
            raise ValueError("kp3d and c3 come together")
        if bool((c2 < 0).any()) or bool(torch.isnan(c2).any()):
            raise ValueError("confidences must be >= 0")
        tile = lambda t: t[None].expand(C, *t.shape).reshape(C * B, *t.shape[1:])
        self.kp2d.copy_(tile(kp2d))
        self.c2.copy_(tile(c2))
        self.camintr.copy_(tile(camintr))
        self.s.copy_(tile(box_scales(kp2d, c2)))
        if kp3d is not None:
            kp3d, c3 = f(kp3d), f(c3)
            if kp3d.shape != (B, 21, 3) or c3.shape != (B, 21) or bool((c3 < 0).any()) or bool(torch.isnan(c3).any()):
                raise ValueError(f"expected kp3d ({B},21,3) and c3 ({B},21) >= 0")
            self.kp3d.copy_(tile(kp3d))
            self.c3.copy_(tile(c3))
        else:
            self.kp3d.zero_()
            self.c3.zero_()
        tk = torch.einsum("kc,nbcd->nbkd", self.template_keypoints, rotations)              # (C,B,21,3)
        z, x, y = initial_translation(kp2d[None].expand(C, B, 21, 2), c2[None].expand(C, B, 21),
                                      camintr[None].expand(C, B, 3, 3), tk)
        with torch.no_grad():
            self.rot6d.copy_(rotations[..., :2].reshape(C * B, 3, 2))
            self.trans.copy_(torch.stack([x, y, z], -1).reshape(C * B, 3))
            self.pca.zero_()
            self.betas.zero_()
        for p in (self.rot6d, self.trans, self.pca, self.betas):
            p.grad.zero_()
        self.opt.reset()
        self.log.zero_()
        self.steps_done = 0

    # ---------------------------------------------------------------- the launches
    def _forward(self):
        P, ck, sb = _lib.ptr, _lib.check, _lib.stream()
        ck(self.L.hm_mano_fwd_clips(self.mctx.ptrs, P(self.pca), self.P, P(self.mano_rot), P(self.betas), None, self.N, P(self.vm),
                                    None, P(self.rot6d), P(self.trans), P(self.ones_c), P(self.vh), P(self.state), self.B, sb),
           "mano_fwd + rigid")

    def _terms(self):
        P, ck, sb, lw, vals = _lib.ptr, _lib.check, _lib.stream(), self.lw, self.vals.data_ptr()
        ck(self.L.hm_keypoint_terms_clips(P(self.vh), P(self.W), P(self.camintr), P(self.kp2d), P(self.c2), P(self.s), P(self.kp3d),
                                          P(self.c3), self.sigma, self.znear, lw["lw_kp2d"], lw["lw_kp3d"], self.N, self.B,
                                          P(self.keypoints), P(self.U_kp), P(self.row_parts), P(self.tickets), vals, NS, sb),
           "keypoint terms")
        if self.B > 1:                 # (a clip of one frame has no smoothness term: its slot stays 0)
            ck(self.L.hm_smooth_fwd_clips(P(self.vh), self.N, 778, 1, P(self.U_sm), vals + 4 * 5, P(self.rws), self.B, NS, sb), "smooth")
        ck(self.L.hm_priors_fwd_clips(P(self.pca), self.P * self.B, P(self.ones_c), P(self.ones_c), P(self.ones_c), P(self.ones_c),
                                      P(self.U_pca), P(self.g_sc[0]), P(self.g_sc[1]), vals + 4 * 2, self.C, NS, sb), "priors")

    def _finish(self, grads):
        P, ck, sb, lw = _lib.ptr, _lib.check, _lib.stream(), self.lw
        ck(self.L.hm_handinit_finish_clips(P(self.betas), P(self.betas.grad) if grads else None, self.N, self.B, P(self.vals), NS,
                                           lw["lw_kp2d"], lw["lw_kp3d"], lw["lw_pca"], lw["lw_beta"], lw["lw_smooth"],
                                           P(self.opt.step_t) if grads else None, self.max_steps, P(self.log) if grads else None,
                                           sb), "finish")

    def _step_fused(self):
        P, ck, sb, lw = _lib.ptr, _lib.check, _lib.stream(), self.lw
        self._forward()
        self._terms()
        tp, tw, tn = _lib.terms([(self.U_kp, 1.0), (self.U_sm if self.B > 1 else None, lw["lw_smooth"])])
        ck(self.L.hm_mano_bwd_rigid_clips(self.mctx.ptrs, P(self.pca), self.P, P(self.mano_rot), P(self.betas), self.N,
                                          P(self.U_pca), lw["lw_pca"], P(self.pca.grad), P(self.g_mano_rot), P(self.betas.grad),
                                          P(self.g_mano_trans), P(self.state), P(self.mctx.workspace(self.N)), P(self.vm),
                                          P(self.rot6d), P(self.ones_c), tp, tw, tn, None, None, 8, 0.0, P(self.rot6d.grad),
                                          P(self.trans.grad), self.B, sb), "mano_bwd + rigid_bwd")
        self._finish(True)
        self.opt.step(zero_grad=False)

    def eager_terms(self):
        """the step's terms through autograd (homan_amd.ops): -> (totals (C,), vals (C,8)) with the graph attached to the
        parameters; the clips' smoothness and priors one clip at a time, the betas prior in torch"""
        lw, B, C = self.lw, self.B, self.C
        vm = ops.mano_lbs(self.pca, self.mano_rot, self.betas, None, self.mctx)
        vh = ops.rigid_transform(vm, self.rot6d, self.trans, self.ones_c[:1], False)[0]
        kp, l2, l3, _ = ops.keypoint_terms(vh, self.W, self.camintr, self.kp2d, self.c2, self.s, self.kp3d, self.c3, sigma=self.sigma,
                                           znear=self.znear, clip_len=B, lw_kp2d=lw["lw_kp2d"], lw_kp3d=lw["lw_kp3d"])
        rws = ops.ReduceWorkspace(self.device)
        rows = []
        for c in range(C):
            sl = slice(c * B, (c + 1) * B)
            sm = ops.smooth_loss(vh[sl], 1, rws) if B > 1 else torch.zeros((), device=self.device)
            lp = ops.priors(self.pca[sl], self.ones_c[:1], self.ones_c[:1], self.ones_c[:1], self.ones_c[:1])[0]
            lb = (self.betas[sl] ** 2).mean()
            total = kp[c] + lw["lw_pca"] * lp + lw["lw_beta"] * lb + lw["lw_smooth"] * sm
            zero = torch.zeros((), device=self.device)
            rows.append(torch.stack([l2[c], l3[c], lp.detach(), zero, zero, sm.detach(), lb.detach(), total]))
        vals = torch.stack(rows)
        return vals[:, 7], vals

    def _step_eager(self):
        params = (self.rot6d, self.trans, self.pca, self.betas)
        totals, vals = self.eager_terms()
        grads = torch.autograd.grad(totals.sum(), params)
        for p, g in zip(params, grads):
            p.grad.copy_(g)
        self.vals.copy_(vals.detach())
        self.log[min(self.steps_done, self.max_steps - 1)].copy_(self.vals)
        self.opt.step(zero_grad=False)

    # ---------------------------------------------------------------- running
    def run(self, steps):
        """`steps` more steps.  The first two steps of a fused loop's life run un-captured (lazy initialisation of the library; the
        same launches), then GRAPH_STEPS steps and one step are captured and every further step is a replay."""
        if self.steps_done + steps > self.max_steps:
            raise ValueError(f"{self.steps_done + steps} steps exceed max_steps = {self.max_steps}")
        left = steps
        if self.mode == "eager":
            for _ in range(left):
                self._step_eager()
                self.steps_done += 1
            return
        if self.graph_1 is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(min(2, left)):
                    self._step_fused()
                    left -= 1
                    self.steps_done += 1
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            if left:
                self.graph_1, self.graph_k = _lib.new_graph(), _lib.new_graph()
                # (a capture only records: the captured launches run at the replays)
                with torch.cuda.graph(self.graph_1):
                    self._step_fused()
                with torch.cuda.graph(self.graph_k):
                    for _ in range(GRAPH_STEPS):
                        self._step_fused()
        while left >= GRAPH_STEPS:
            self.graph_k.replay()
            left -= GRAPH_STEPS
            self.steps_done += GRAPH_STEPS
        for _ in range(left):
            self.graph_1.replay()
            self.steps_done += 1

    def evaluate(self):
        """the terms at the CURRENT parameters, no gradient, no step -> vals (C,8) on the device"""
        with torch.no_grad():
            if self.mode == "eager":
                return self.eager_terms()[1].detach().clone()
            self._forward()
            self._terms()
            self._finish(False)
            return self.vals.clone()

    def loss_evolution(self):
        """(steps, C, 8) numpy: every step's values BEFORE its update"""
        torch.cuda.synchronize()
        return self.log[:self.steps_done].cpu().numpy()

    def result(self):
        """after the last step: the terms once more at the final parameters, the candidate with the lowest total (the first
        minimum; a NaN total never wins) -> dict of host tensors for that candidate's B frames"""
        vals = self.evaluate()
        if self.mode == "eager":              # (the autograd path leaves nothing in the fitter's vertex buffers)
            self._forward()
        totals = torch.nan_to_num(vals[:, 7], nan=float("inf")).cpu()
        best = int(torch.argmin(totals))
        sl = slice(best * self.B, (best + 1) * self.B)
        with torch.no_grad():
            kp = torch.einsum("kv,nvc->nkc", self.W, self.vh[sl]) if self.mode == "eager" else self.keypoints[sl]
            out = dict(candidate=best, totals=vals[:, 7].cpu(), vals=vals.cpu(), rot6d=self.rot6d[sl].cpu(), trans=self.trans[sl].cpu(),
                       pca=self.pca[sl].cpu(), betas=self.betas[sl].cpu(), verts=self.vm[sl].cpu(), verts_world=self.vh[sl].cpu(),
                       keypoints=kp.cpu())
        return out


_FITTERS = {}


def _resident_fitter(model_np, source, side, B, C, **kw):
    """source: what the models were made from (the caller's mano_model object, or the mano_root string)"""
    key = (source if isinstance(source, str) else id(source), side, B, C, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _FITTERS:
        if len(_FITTERS) >= 4:
            _FITTERS.pop(next(iter(_FITTERS)))
        _FITTERS[key] = (HandKeypointFitter(model_np, side, B, C, **kw), source)         # (the source is kept: its id is the key)
    return _FITTERS[key][0]


def release_hand_fitters():
    _FITTERS.clear()


def fit_hands_to_keypoints(keypoints2d, camintr, hand_sides, confidences=None, keypoints3d=None, confidences3d=None,
                           image_size=640, rotations_init=None, num_iterations=100, lr=1e-2, loss_weights=None,
                           mano_root="extra_data/mano", mano_model=None, mode="fused", sigma=DEFAULT_SIGMA, znear=DEFAULT_ZNEAR,
                           optimize_betas=False, pca_dim=45):
    """keypoints2d (B,h,21,2) in pixels, in the joint order of `postprocess.JOINT_ORDER`; camintr (3,3) or (B,3,3) as
    `build_model` takes it (divided by image_size); hand_sides: h of "right" / "left"; confidences (B,h,21) >= 0 (missing
    detections: 0, their targets may be NaN); keypoints3d (B,h,21,3) metres relative to keypoint 0 with confidences3d, optional;
    rotations_init (C,3,3) or (h,C,3,3) candidate starts as row-vector rotations (default: `default_candidates`).
    -> list of B person_parameters dicts (the keys `loopcommon.collate_inputs` reads, as `synth.make_clip` shows them, except
    masks / K_roi / target_masks, which are `maskutils`' job), plus keypoints3d (h,21,3) camera space, keypoint_loss (h,) and
    candidate (h,).  `verts` are the MANO-space vertices: verts @ rotations + translations is the camera-space hand.
    optimize_betas=False keeps the shape at zero: the joint fit starts betas at zero whatever it is given (reference
    homan/homan.py:108), so only then is the returned hand the one `optimize_mano=True` starts from.  `cams` is the perspective
    mode's placeholder: hand_proj_mode="ortho" is not served."""
    kp = torch.as_tensor(keypoints2d, dtype=torch.float32)
    hand_sides = list(hand_sides)
    if kp.dim() != 4 or kp.shape[1:] != (len(hand_sides), 21, 2) or kp.shape[0] < 1:
        raise ValueError(f"keypoints2d must be (B, {len(hand_sides)}, 21, 2), got {tuple(kp.shape)}")
    for side in hand_sides:
        if side not in ("right", "left"):
            raise ValueError(f"{side} not in [left|right]")
    if num_iterations < 0:
        raise ValueError("num_iterations must be >= 0")
    B, h = kp.shape[:2]
    c2 = torch.ones(B, h, 21) if confidences is None else torch.as_tensor(confidences, dtype=torch.float32)
    if c2.shape != (B, h, 21):
        raise ValueError(f"confidences must be ({B}, {h}, 21), got {tuple(c2.shape)}")
    if (keypoints3d is None) != (confidences3d is None) and keypoints3d is None:
        raise ValueError("confidences3d without keypoints3d")
    kp3 = c3 = None
    if keypoints3d is not None:
        kp3 = torch.as_tensor(keypoints3d, dtype=torch.float32)
        c3 = torch.ones(B, h, 21) if confidences3d is None else torch.as_tensor(confidences3d, dtype=torch.float32)
        if kp3.shape != (B, h, 21, 3) or c3.shape != (B, h, 21):
            raise ValueError(f"keypoints3d must be ({B}, {h}, 21, 3) and confidences3d ({B}, {h}, 21)")
    K = torch.as_tensor(camintr, dtype=torch.float32).clone()
    K = (K[None] if K.dim() == 2 else K).expand(B, 3, 3).clone()
    if K.shape != (B, 3, 3):
        raise ValueError(f"camintr must be (3,3) or ({B},3,3)")
    K[:, :2] *= float(image_size)                                     # pixels
    cands = default_candidates() if rotations_init is None else torch.as_tensor(rotations_init, dtype=torch.float32)
    if cands.dim() == 3:
        cands = cands[None].expand(h, *cands.shape)
    if cands.dim() != 4 or cands.shape[0] != h or cands.shape[2:] != (3, 3):
        raise ValueError("rotations_init must be (C,3,3) or (h,C,3,3)")
    lw = _check_weights(loss_weights)
    if not torch.cuda.is_available():
        raise _lib.HomanAmdError("homan_amd.handinit needs the GPU (there is no CPU fallback)")
    models = hand_models(mano_model, mano_root)
    per_hand = []
    for i, side in enumerate(hand_sides):
        fit = _resident_fitter(models[side], mano_root if mano_model is None else mano_model, side, B, cands.shape[1], lr=lr, loss_weights=lw, sigma=sigma,
                               znear=znear, pca_dim=pca_dim, mode=mode, optimize_betas=optimize_betas,
                               max_steps=max(1024, num_iterations))
        fit.load(kp[:, i], c2[:, i], K, cands[i], None if kp3 is None else kp3[:, i], None if kp3 is None else c3[:, i])
        fit.run(num_iterations)
        res = fit.result()
        res["faces"], res["rotations"] = fit.faces, rot6d_to_matrix(res["rot6d"])
        per_hand.append(res)
    out = []
    for b in range(B):
        st = lambda key: torch.stack([r[key][b] for r in per_hand])
        vw = st("verts_world")
        hom = torch.einsum("ij,hvj->hvi", K[b], vw)
        out.append(dict(
            translations=st("trans")[:, None].clone(), rotations=st("rotations").clone(), hand_side=list(hand_sides),
            faces=torch.stack([r["faces"] for r in per_hand]).clone(), mano_trans=torch.zeros(h, 3), mano_rot=torch.zeros(h, 3),
            mano_betas=st("betas").clone(), mano_pca_pose=st("pca").clone(), verts=st("verts").clone(),
            verts2d=(hom[..., :2] / hom[..., 2:]).contiguous(), cams=torch.tensor([[1.0, 0.0, 0.0]]).repeat(h, 1),
            keypoints3d=st("keypoints").clone(), keypoint_loss=torch.stack([r["totals"][r["candidate"]] for r in per_hand]),
            candidate=torch.tensor([r["candidate"] for r in per_hand])))
    return out
