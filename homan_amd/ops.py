"""Autograd-facing wrappers over the HIP kernels (C ABI via ctypes).

Each op mirrors one leaf the reference calls (file:line in the docstrings).  Forward and
backward arithmetic is entirely in libhoman_amd.so; torch supplies memory, streams and the
autograd graph.
"""
import numpy as np
import torch

from . import lib as _lib

NMR_NEAR, NMR_FAR, NMR_EPS = 0.1, 100.0, 1e-3   # neural_renderer ctor defaults used at reference losses.py:73-77


def _f32(t):
    return t.contiguous().float()


def _p(v):
    """what a C argument takes: a tensor's device address; None, numbers and raw addresses as they are"""
    return _lib.ptr(v) if isinstance(v, torch.Tensor) else v


_RENDER_FIELDS = {name for name, _ in _lib.SilRender._fields_}


def build_adjacency(faces_np, num_verts):
    """CSR vertex -> (face*3 + corner) lists for a (F,3) face array (host, once per topology)."""
    faces_np = np.asarray(faces_np).astype(np.int64)
    flat = faces_np.reshape(-1)
    order = np.argsort(flat, kind="stable")
    counts = np.bincount(flat, minlength=num_verts)
    off = np.zeros(num_verts + 1, np.int32)
    off[1:] = np.cumsum(counts)
    return torch.from_numpy(off), torch.from_numpy(order.astype(np.int32))


class SilhouetteContext:
    """Per-call-site state of the silhouette op: topology adjacency + the workspace that carries
    the forward intermediates (packed faces, index map, bit planes) to the backward."""

    def __init__(self, faces, num_verts, batch, size, device):
        assert faces.dim() == 3 and faces.shape[0] == batch
        f0 = faces[0].detach().cpu().numpy()
        if batch > 1:
            assert bool((faces == faces[:1]).all()), "per-frame topologies must be identical"
        # The kernels tile the image in 32x32-pixel blocks (64-sample mask words of the edge sweeps).  Any other image size
        # (the reference's Core50 setting renders at 350, homan/getdataset.py:35) is rendered on the next multiple of 32
        # with the first two rows of K scaled by size / padded size: the top-left size x size block of that render shows
        # exactly the rays of the requested image (same pinhole, coarser normalisation), the rest is cropped away.  Sample
        # positions then round differently from a native render of that size: coverage agrees up to projection rounding
        # (tests/test_render_gpu.py), where multiples of 32 are bit-exact against the oracle.
        self.size = int(size)
        size = (self.size + 31) // 32 * 32
        self.padded = size != self.size
        self.B, self.V, self.F, self.S = batch, num_verts, f0.shape[0], size
        self.faces = faces[0].to(device=device, dtype=torch.int32).contiguous()
        off, items = build_adjacency(f0, num_verts)
        self.adj_off, self.adj_items = off.to(device), items.to(device)
        # dispatch order of the forward raster's (frame, 32x32-sample region) workgroups: default = regions from the
        # ROI centre outwards, frame fastest; `calibrate()` replaces it by a cost-sorted order
        n = size // 16
        ry, rx = np.divmod(np.arange(n * n), n)
        ring = np.maximum(np.abs(2 * rx + 1 - n), np.abs(2 * ry + 1 - n))
        regions = np.argsort(ring, kind="stable").astype(np.int64)
        wo = (np.arange(batch, dtype=np.int64)[None, :] << 16) | regions[:, None]
        self.work_order = torch.from_numpy(wo.reshape(-1).astype(np.int32)).to(device)
        # grid of the backward's order-independent sums (include/homan_amd.h, "ORDER-INDEPENDENT SUMS"): 0 = the default
        # 2^-44, right for the normalised silhouette loss of the joint fit; the pose initialisation's unnormalised sums of
        # squares set a coarser one
        self.sum_log2q = 0
        nbytes = _lib.lib().hm_sil_workspace_bytes(self.B, self.V, self.F, self.S)
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=device)   # holds a self-resetting ticket

    # ---- image sizes that are not a multiple of 32 (see __init__)
    def K_eff(self, K):
        if not self.padded:
            return K
        K = K.clone()
        K[:, :2, :] *= self.size / self.S
        return K.contiguous()

    def crop(self, img):
        return img[..., :self.size, :self.size].contiguous() if self.padded else img

    def pad(self, img, value=0.0):
        if not self.padded:
            return img
        d = self.S - self.size
        return torch.nn.functional.pad(img, (0, d, 0, d), value=value).contiguous()

    def eps(self):
        """the rasteriser's eps (NDC units, added to every pseudo-distance of the backward) in the units of the grid the
        kernels render on: a padded render's NDC is the requested image's times size / S, and d loss / d NDC is carried
        back through that factor, so eps scales with it (otherwise the gradient is off by ~eps / pixel pitch: 1-2 %)"""
        return NMR_EPS * self.size / self.S if self.padded else NMR_EPS

    def crop_samples(self, img):
        """(.., 2S, 2S) sample-resolution image -> the (.., 2 size, 2 size) block the caller asked for (no-AA renders)"""
        n = 2 * self.size
        return img[..., :n, :n].contiguous() if self.padded else img

    def pad_samples(self, img, value=0.0):
        if not self.padded:
            return img
        d = 2 * (self.S - self.size)
        return torch.nn.functional.pad(img, (0, d, 0, d), value=value).contiguous()

    def calibrate(self):
        """Cost-sorted launch orders from the screen boxes of the last forward (poses move little during an
        optimisation, so the statistics of the current state predict the cost of the next iterations):
        forward raster workgroups by descending candidate count.
        Pure scheduling: results do not depend on the order."""
        raw = torch.empty(self.B * self.F * 8, dtype=torch.uint8, device=self.workspace.device)
        _lib.check(_lib.lib().hm_sil_read_boxes(_lib.ptr(self.workspace), self.B, self.V, self.F, self.S, _lib.ptr(raw),
                                                _lib.stream()), "hm_sil_read_boxes")
        bx = raw.cpu().numpy().view(np.uint16).reshape(self.B, self.F, 4).astype(np.int64)
        valid = (bx[..., 0] >> 14) != 0
        x0, y0, x1, y1 = bx[..., 0] & 0x3fff, bx[..., 1], bx[..., 2], bx[..., 3]
        n, is_ = self.S // 16, 2 * self.S
        # region index of a sample: columns x // 32 ; rows are flipped (tile row 0 holds the largest yi)
        rx0, rx1 = x0 // 32, x1 // 32
        ry0, ry1 = (is_ - 1 - y1) // 32, (is_ - 1 - y0) // 32
        cnt = np.zeros((self.B, n + 1, n + 1), np.int64)
        bi = np.broadcast_to(np.arange(self.B)[:, None], x0.shape)[valid]
        a0, a1, c0, c1 = ry0[valid], ry1[valid] + 1, rx0[valid], rx1[valid] + 1
        np.add.at(cnt, (bi, a0, c0), 1)
        np.add.at(cnt, (bi, a1, c1), 1)
        np.add.at(cnt, (bi, a0, c1), -1)
        np.add.at(cnt, (bi, a1, c0), -1)
        cnt = cnt.cumsum(1).cumsum(2)[:, :n, :n].reshape(self.B, n * n)
        order = np.argsort(-cnt.reshape(-1), kind="stable")
        b_idx, region = np.divmod(order, n * n)
        self.work_order = torch.from_numpy(((b_idx << 16) | region).astype(np.int32)).to(self.workspace.device)
        # winding class that owns the samples (the camera-facing surface of a closed mesh): rasterised first, the other
        # class is then rejected block-wise behind it
        idx = self.idx_map()
        near = int(((idx >= self.F).sum() > ((idx >= 0) & (idx < self.F)).sum()).item())
        _lib.check(_lib.lib().hm_sil_hint_near_winding(_lib.ptr(self.workspace), near, _lib.stream()),
                   "hm_sil_hint_near_winding")
        self.near_winding = near
        # (the edge sweeps keep the natural face order: sorting faces by box perimeter was measured slower -- it scatters
        #  neighbouring faces, and with them the cache lines of the index map and the mask planes they share)

    # ---- the rasteriser's launches (include/homan_amd.h; keywords = the header's parameter names = HmSilRender's fields).  A launch
    # layer only: K, masks and gradient images arrive as the kernels take them (K_eff / pad / crop stay with the caller), and the
    # library's return code goes back to the caller, who hands it to lib.check under its own label
    def render_fields(self, **given):
        """the HmSilRender fields of one render on this context (lib.sil_renders): the context's own state + `given`"""
        unknown = set(given) - _RENDER_FIELDS
        if unknown:
            raise TypeError(f"render_fields: unknown field(s) {sorted(unknown)}")
        return dict(faces=self.faces, faces_bstride=0, B=self.B, V=self.V, F=self.F, S=self.S, znear=NMR_NEAR, zfar=NMR_FAR,
                    orig_size=1.0, work_order=self.work_order, workspace=self.workspace) | given

    def forward(self, *, keep_sum=None, loss_out=None, alpha_full=None, out_stride=0, phases=3, stream=None, **render):
        """one hm_sil_fwd_phase_clips: `render` as render_fields takes it (verts, K, pooled required)"""
        r = {k: _p(v) for k, v in self.render_fields(**render).items()}
        g = r.get
        return _lib.lib().hm_sil_fwd_phase_clips(
            r["verts"], r["faces"], r["faces_bstride"], r["K"], r["B"], r["V"], r["F"], r["S"], float(r["orig_size"]), r["znear"],
            r["zfar"], g("keep"), g("ref"), _p(keep_sum), r["pooled"], _p(loss_out), r["work_order"], g("pooled_depth"),
            _p(alpha_full), g("mask_shared", 0), g("rigid_rot6d"), g("rigid_trans"), g("rigid_scale"), g("rigid_abs", 0),
            g("persistent_outputs", 0), r["workspace"], g("clip_len", 0), out_stride, g("cam_verts_out"), phases,
            _lib.stream() if stream is None else stream)

    def backward(self, verts, K, mode, *, upstream=None, grad_pooled=None, keep_sum=None, grad_verts=None, grad_ndc=None,
                 clip_len=0, loss_out=None, out_stride=0, phases=3, eps=None, sum_log2q=None, orig_size=1.0, stream=None):
        """one hm_sil_bwd_phase_clips on the state the last forward left in the workspace"""
        return _lib.lib().hm_sil_bwd_phase_clips(
            _p(verts), _p(K), self.B, self.V, self.F, self.S, float(orig_size), self.eps() if eps is None else eps, mode,
            _p(upstream), _p(grad_pooled), _p(keep_sum), _p(self.adj_off), _p(self.adj_items), _p(grad_verts), _p(grad_ndc),
            _p(self.workspace), clip_len, _p(loss_out), out_stride, phases, self.sum_log2q if sum_log2q is None else sum_log2q,
            _lib.stream() if stream is None else stream)

    def reduce(self, *, keep_sum=None, loss_out=None, frame_out=None, clip_len=0, out_stride=0, stream=None):
        """one hm_sil_reduce_clips"""
        return _lib.lib().hm_sil_reduce_clips(self.B, self.V, self.F, self.S, _p(keep_sum), _p(loss_out), _p(frame_out),
                                              _p(self.workspace), clip_len, out_stride,
                                              _lib.stream() if stream is None else stream)

    def parts_ptr(self):
        """device address of the (B,F,3,2) doubles of the last backward: the `sil_parts` of hm_rigid_bwd_sil*"""
        return _lib.lib().hm_sil_parts(_p(self.workspace), self.B, self.V, self.F, self.S)

    def idx_map(self):
        out = torch.empty(self.B, 2 * self.S, 2 * self.S, dtype=torch.int32, device=self.workspace.device)
        _lib.check(_lib.lib().hm_sil_read_idx_map(_lib.ptr(self.workspace), self.B, self.V, self.F, self.S,
                                                  _lib.ptr(out), _lib.stream()), "hm_sil_read_idx_map")
        return out

    def invalidate_outputs(self):
        """the loss inputs (keep / ref masks) in the caller's buffers changed: see hm_sil_invalidate_outputs"""
        _lib.check(_lib.lib().hm_sil_invalidate_outputs(_lib.ptr(self.workspace), self.B, self.V, self.F, self.S,
                                                        _lib.stream()), "hm_sil_invalidate_outputs")

    # ---- the non-zero flags of a depth-gradient image (hm_depth_bwd_sparse), handed from the loss term that wrote image and flags
    # in one launch to the depth backward of this context's render: no second copy of the image, the flags ride beside it
    _gflags = None
    last_depth_bwd = None        # "sparse" / "dense": the path the last depth backward on this context took

    def offer_gflags(self, grad_image, flags):
        """`flags` describe `grad_image` as it is NOW; they are taken (once) only by a depth backward that receives that very
        tensor, unmodified - a gradient autograd has summed with another term's is a different or a re-versioned tensor"""
        self._gflags = (grad_image, grad_image._version, flags)

    def take_gflags(self, grad_image):
        held, self._gflags = self._gflags, None
        if held is None or self.padded or self.S % 64 != 0:
            return None
        img, version, flags = held
        same = (img.data_ptr() == grad_image.data_ptr() and img.shape == grad_image.shape and grad_image.is_contiguous() and
                grad_image.dtype == torch.float32 and grad_image._version == version)
        return flags if same else None

    def parts(self):
        """(B,F,3,2) float64: per-(face, corner) NDC gradients of the last backward (exact sums, see include/homan_amd.h)"""
        out = torch.empty(self.B, self.F, 3, 2, dtype=torch.float64, device=self.workspace.device)
        _lib.check(_lib.lib().hm_sil_read_parts(_lib.ptr(self.workspace), self.B, self.V, self.F, self.S,
                                                _lib.ptr(out), _lib.stream()), "hm_sil_read_parts")
        return out

    def faces9(self):
        out = torch.empty(self.B, self.F, 9, device=self.workspace.device)
        _lib.check(_lib.lib().hm_sil_read_faces9(_lib.ptr(self.workspace), self.B, self.V, self.F, self.S,
                                                 _lib.ptr(out), _lib.stream()), "hm_sil_read_faces9")
        return out


class _SilhouetteLoss(torch.autograd.Function):
    """reference homan/losses.py:183-197 (render @ ROI intrinsics, keep-masked MSE, /sum(keep), /B, IoU metric)."""

    @staticmethod
    def forward(ctx, verts, K, keep, ref, keep_sum, sctx, orig_size):
        verts, K = _f32(verts), sctx.K_eff(_f32(K))
        keep, ref = sctx.pad(keep), sctx.pad(ref)          # (padding: keep = 0, so it counts for nothing)
        pooled = torch.empty(sctx.B, sctx.S, sctx.S, device=verts.device)
        out = torch.empty(2, device=verts.device)
        _lib.check(sctx.forward(verts=verts, K=K, orig_size=orig_size, keep=keep, ref=ref, keep_sum=keep_sum, pooled=pooled,
                                loss_out=out), "hm_sil_fwd")
        ctx.save_for_backward(verts, K, keep_sum)
        ctx.sctx, ctx.orig_size = sctx, orig_size
        pooled = sctx.crop(pooled)
        ctx.mark_non_differentiable(pooled)
        return out[0:1], out[1], pooled

    @staticmethod
    def backward(ctx, g_loss, _g_iou, _g_img):
        verts, K, keep_sum = ctx.saved_tensors
        sctx = ctx.sctx
        g_loss = _f32(g_loss).reshape(1)
        grad_verts = torch.empty_like(verts)
        _lib.check(sctx.backward(verts, K, 1, upstream=g_loss, keep_sum=keep_sum, grad_verts=grad_verts,
                                 orig_size=ctx.orig_size), "hm_sil_bwd")
        return grad_verts, None, None, None, None, None, None


class _SilhouetteRender(torch.autograd.Function):
    """reference homan/losses.py:187: renderer(verts, faces, K=, mode='silhouettes') -> (B,S,S)."""

    @staticmethod
    def forward(ctx, verts, K, sctx, orig_size):
        verts, K = _f32(verts), sctx.K_eff(_f32(K))
        pooled = torch.empty(sctx.B, sctx.S, sctx.S, device=verts.device)
        _lib.check(sctx.forward(verts=verts, K=K, orig_size=orig_size, pooled=pooled), "hm_sil_fwd")
        ctx.save_for_backward(verts, K)
        ctx.sctx, ctx.orig_size = sctx, orig_size
        return sctx.crop(pooled)

    @staticmethod
    def backward(ctx, g_img, grad_ndc_out=None):
        verts, K = ctx.saved_tensors
        sctx = ctx.sctx
        g_img = sctx.pad(_f32(g_img))
        grad_verts = torch.empty_like(verts)
        _lib.check(sctx.backward(verts, K, 0, grad_pooled=g_img, grad_verts=grad_verts, grad_ndc=getattr(sctx, "grad_ndc", None),
                                 orig_size=ctx.orig_size), "hm_sil_bwd")
        return grad_verts, None, None, None


class _SilhouetteRenderNoAA(torch.autograd.Function):
    """reference homan/pose_optimization.py:89-96,140-141: nr.Renderer(image_size, anti_aliasing=False)(verts, faces,
    mode='silhouettes') -> (B,image_size,image_size) hard 0/1 coverage.  `sctx` is built with size = image_size // 2
    (its sample grid IS the image); the backward is the same edge-sweep pseudo-gradient, fed per sample."""

    @staticmethod
    def forward(ctx, verts, K, sctx, orig_size):
        verts, K = _f32(verts), sctx.K_eff(_f32(K))       # (sizes off the 64-sample grid: padded render, cropped below)
        n = 2 * sctx.S
        pooled = torch.empty(sctx.B, sctx.S, sctx.S, device=verts.device)
        alpha = torch.empty(sctx.B, n, n, device=verts.device)
        _lib.check(sctx.forward(verts=verts, K=K, orig_size=orig_size, pooled=pooled, alpha_full=alpha), "hm_sil_fwd")
        ctx.save_for_backward(verts, K)
        ctx.sctx, ctx.orig_size = sctx, orig_size
        return sctx.crop_samples(alpha)

    @staticmethod
    def backward(ctx, g_img):
        verts, K = ctx.saved_tensors
        sctx = ctx.sctx
        g_img = _lib.aligned(sctx.pad_samples(_f32(g_img)), 8)         # (mode 3 reads it as float2)
        grad_verts = torch.empty_like(verts)
        _lib.check(sctx.backward(verts, K, 3, grad_pooled=g_img, grad_verts=grad_verts, orig_size=ctx.orig_size), "hm_sil_bwd")
        return grad_verts, None, None, None


def silhouette_render_noaa(verts, K, sctx, orig_size=1.0):
    """Hard silhouettes without anti-aliasing, (B, 2*sctx.S, 2*sctx.S)."""
    return _SilhouetteRenderNoAA.apply(verts, K, sctx, orig_size)


class _MaskedSilhouetteL2NoAA(torch.autograd.Function):
    """reference homan/pose_optimization.py:138-143 in one pass: image = keep * Renderer(anti_aliasing=False)(verts) ;
    loss_b = sum((image_b - ref)^2) ; iou_b.  keep / ref: one (n,n) mask shared by all poses.  The backward reuses the
    sweep planes the forward emitted, which is valid for POSITIVE upstream gradients only (a sum of per-pose losses)."""

    @staticmethod
    def forward(ctx, verts, K, keep, ref, sctx, orig_size):
        verts, K = _f32(verts), sctx.K_eff(_f32(K))
        n = 2 * sctx.S
        keep, ref = sctx.pad_samples(keep), sctx.pad_samples(ref)      # (padding: keep = 0, it counts for nothing)
        assert keep.shape == (n, n) and ref.shape == (n, n) and keep.is_contiguous() and ref.is_contiguous()
        keep, ref = _lib.aligned(keep, 8), _lib.aligned(ref, 8)        # (the per-sample loss reads them as float2)
        pooled = torch.empty(sctx.B, sctx.S, sctx.S, device=verts.device)
        alpha = torch.empty(sctx.B, n, n, device=verts.device)
        frame = torch.empty(sctx.B, 2, device=verts.device)
        _lib.check(sctx.forward(verts=verts, K=K, orig_size=orig_size, keep=keep, ref=ref, mask_shared=1, pooled=pooled,
                                alpha_full=alpha), "hm_sil_fwd")
        _lib.check(sctx.reduce(frame_out=frame), "hm_sil_reduce")
        ctx.save_for_backward(verts, K)
        ctx.sctx, ctx.orig_size = sctx, orig_size
        alpha = sctx.crop_samples(alpha)
        ctx.mark_non_differentiable(alpha)
        return frame[:, 0], frame[:, 1], alpha

    @staticmethod
    def backward(ctx, g_loss, _g_iou, _g_alpha):
        verts, K = ctx.saved_tensors
        sctx = ctx.sctx
        g_loss = _f32(g_loss).contiguous()
        grad_verts = torch.empty_like(verts)
        _lib.check(sctx.backward(verts, K, 4, upstream=g_loss, grad_verts=grad_verts, orig_size=ctx.orig_size), "hm_sil_bwd")
        return grad_verts, None, None, None, None, None


def masked_silhouette_l2_noaa(verts, K, keep, ref, sctx, orig_size=1.0):
    """-> (per-pose sum of squares (B,), per-pose IoU (B,), coverage image (B,n,n) [no gradient])."""
    return _MaskedSilhouetteL2NoAA.apply(verts, K, keep, ref, sctx, orig_size)


def silhouette_loss(verts, K, keep, ref, keep_sum, sctx, orig_size=1.0):
    """-> (loss_sil (1,), mean IoU (0-d), silhouettes (B,S,S))."""
    return _SilhouetteLoss.apply(verts, K, keep, ref, keep_sum, sctx, orig_size)


def silhouette_render(verts, K, sctx, orig_size=1.0):
    return _SilhouetteRender.apply(verts, K, sctx, orig_size)


class SoftSilhouetteContext:
    """Per-call-site state of the soft silhouette op (csrc/softsil.hip; a non-parity extra, see include/homan_amd.h): topology,
    CSR adjacency and the workspace, allocated once.  Any image size from 1 to 4096: the 32-pixel grid of the hard path does not
    apply, so nothing is padded and K is used as given."""

    def __init__(self, faces, num_verts, batch, size, device):
        assert faces.dim() == 3 and faces.shape[0] == batch
        f0 = faces[0].detach().cpu().numpy()
        if batch > 1:
            assert bool((faces == faces[:1]).all()), "per-frame topologies must be identical"
        self.B, self.V, self.F, self.S = batch, num_verts, f0.shape[0], int(size)
        self.size = self.S
        self.faces = faces[0].to(device=device, dtype=torch.int32).contiguous()
        off, items = build_adjacency(f0, num_verts)
        self.adj_off, self.adj_items = off.to(device), items.to(device)
        nbytes = _lib.lib().hm_softsil_workspace_bytes(self.B, self.V, self.F, self.S)
        if nbytes == 0:
            raise _lib.HomanAmdError(f"soft silhouettes: unsupported shape B={self.B} V={self.V} F={self.F} S={self.S}")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)

    def invalidate_outputs(self):
        """(the hard context's hook for new masks in resident buffers, HOMan.load_clip: every soft render writes every pixel)"""


class _SoftSilhouetteRender(torch.autograd.Function):
    """Soft Rasterizer silhouettes (Liu et al. 2019) with their true gradient; stands beside reference homan/losses.py:187."""

    @staticmethod
    def forward(ctx, verts, K, sctx, sigma, orig_size):
        verts, K = _f32(verts), _f32(K)
        assert sigma.dtype == torch.float32 and sigma.numel() == 1 and sigma.device == verts.device
        alpha = torch.empty(sctx.B, sctx.S, sctx.S, device=verts.device)
        _lib.check(_lib.lib().hm_softsil_fwd(
            _lib.ptr(verts), _lib.ptr(sctx.faces), _lib.ptr(K), sctx.B, sctx.V, sctx.F, sctx.S, float(orig_size),
            NMR_NEAR, NMR_FAR, _lib.ptr(sigma), _lib.ptr(alpha), _lib.ptr(sctx.workspace), _lib.stream()), "hm_softsil_fwd")
        ctx.save_for_backward(verts, K, alpha)
        ctx.sctx, ctx.sigma, ctx.orig_size = sctx, sigma, orig_size        # (sigma: the live tensor, read again by the backward)
        return alpha

    @staticmethod
    def backward(ctx, g_img):
        verts, K, alpha = ctx.saved_tensors
        sctx = ctx.sctx
        g_img = _f32(g_img)
        grad_verts = torch.empty_like(verts)
        _lib.check(_lib.lib().hm_softsil_bwd(
            _lib.ptr(verts), _lib.ptr(sctx.faces), _lib.ptr(K), sctx.B, sctx.V, sctx.F, sctx.S, float(ctx.orig_size),
            NMR_NEAR, NMR_FAR, _lib.ptr(ctx.sigma), _lib.ptr(alpha), _lib.ptr(g_img), _lib.ptr(sctx.adj_off),
            _lib.ptr(sctx.adj_items), _lib.ptr(grad_verts), _lib.ptr(sctx.workspace), _lib.stream()), "hm_softsil_bwd")
        return grad_verts, None, None, None, None


def soft_silhouette_render(verts, K, sctx, sigma, orig_size=1.0):
    """-> (B,S,S) soft coverage.  sigma: 1-element float32 device tensor (NDC^2), read by the kernels when they run - a value
    changed in place is followed by a captured graph; not differentiable."""
    return _SoftSilhouetteRender.apply(verts, K, sctx, sigma, orig_size)


def softsil_pose_workspace(n, size, device):
    """zero-filled ticket / partials buffer of hm_softsil_pose_terms for n candidates at mask size `size`"""
    nbytes = _lib.lib().hm_softsil_pose_workspace_bytes(int(n), int(size))
    if nbytes == 0:
        raise _lib.HomanAmdError(f"soft pose terms: unsupported shape N={n} S={size}")
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)


class _SoftSilPoseTerms(torch.autograd.Function):
    """The masked L2 and the IoU of the pose initialisation on the soft image (csrc/softpose.hip, hm_softsil_pose_terms): the
    expressions of reference homan/pose_optimization.py:138-147 on image = keep * alpha, one shared mask for every candidate."""

    @staticmethod
    def forward(ctx, alpha, keep, ref, workspace):
        alpha = _f32(alpha).contiguous()
        n, size = alpha.shape[0], alpha.shape[1]
        assert alpha.shape == (n, size, size) and keep.shape == (size, size) and ref.shape == (size, size)
        terms = torch.empty(n, 2, device=alpha.device)
        grad = torch.empty_like(alpha)
        _lib.check(_lib.lib().hm_softsil_pose_terms(_lib.ptr(alpha), _lib.ptr(keep), _lib.ptr(ref), n, size, _lib.ptr(terms),
                                                    _lib.ptr(grad), _lib.ptr(workspace), _lib.stream()), "hm_softsil_pose_terms")
        ctx.save_for_backward(grad)
        mask, iou = terms[:, 0], terms[:, 1]
        ctx.mark_non_differentiable(iou)
        return mask, iou

    @staticmethod
    def backward(ctx, g_mask, _g_iou):
        grad, = ctx.saved_tensors
        return _f32(g_mask)[:, None, None] * grad, None, None, None


def softsil_pose_terms(alpha, keep, ref, workspace):
    """alpha (n,S,S) soft images, keep / ref (S,S) 0 / 1 -> (per-candidate sum of squares (n,), per-candidate IoU (n,) [no
    gradient]); workspace: softsil_pose_workspace(n, S, device)."""
    return _SoftSilPoseTerms.apply(alpha, keep, ref, workspace)


class _DepthRender(torch.autograd.Function):
    """reference homan/homan.py:391,406: `_, depths, sils = renderer.render(verts, faces, textures, K=)`.
    -> (silhouettes (B,S,S), depths (B,S,S)); only the depth image is differentiable here (the ordinal depth loss uses
    the silhouettes as a mask only: lossutils.py:146-149 compares them with ==)."""

    @staticmethod
    def forward(ctx, verts, K, sctx, orig_size):
        verts, K = _f32(verts), sctx.K_eff(_f32(K))
        pooled = torch.empty(sctx.B, sctx.S, sctx.S, device=verts.device)
        depth = torch.empty(sctx.B, sctx.S, sctx.S, device=verts.device)
        _lib.check(sctx.forward(verts=verts, K=K, orig_size=orig_size, pooled=pooled, pooled_depth=depth), "hm_sil_fwd")
        ctx.save_for_backward(verts, K)
        ctx.sctx, ctx.orig_size = sctx, orig_size
        pooled, depth = sctx.crop(pooled), sctx.crop(depth)
        ctx.mark_non_differentiable(pooled)
        return pooled, depth

    @staticmethod
    def backward(ctx, _g_sil, g_depth):
        verts, K = ctx.saved_tensors
        sctx = ctx.sctx
        grad_verts = torch.empty_like(verts)
        # a gradient image that arrives exactly as a loss term's backward left it, with that term's non-zero flags
        # (offer_gflags), takes the sparse backward: same result, faces and frames off the flagged segments are not walked
        gflags = sctx.take_gflags(g_depth)
        sctx.last_depth_bwd = "dense" if gflags is None else "sparse"
        if gflags is not None:
            _lib.check(_lib.lib().hm_depth_bwd_sparse(
                _lib.ptr(verts), _lib.ptr(K), sctx.B, sctx.V, sctx.F, sctx.S, float(ctx.orig_size), _lib.ptr(g_depth),
                _lib.ptr(sctx.adj_off), _lib.ptr(sctx.adj_items), _lib.ptr(grad_verts), _lib.ptr(gflags),
                _lib.ptr(sctx.workspace), _lib.stream()), "hm_depth_bwd_sparse")
            return grad_verts, None, None, None
        _lib.check(_lib.lib().hm_depth_bwd(
            _lib.ptr(verts), _lib.ptr(K), sctx.B, sctx.V, sctx.F, sctx.S, float(ctx.orig_size),
            _lib.ptr(sctx.pad(_f32(g_depth))),
            _lib.ptr(sctx.adj_off), _lib.ptr(sctx.adj_items), _lib.ptr(grad_verts), _lib.ptr(sctx.workspace),
            _lib.stream()), "hm_depth_bwd")
        return grad_verts, None, None, None


def depth_render(verts, K, sctx, orig_size):
    """-> (silhouettes, depths), both (B,S,S).  One SilhouetteContext per rendered mesh (the backward reads the
    forward's index map from its workspace)."""
    return _DepthRender.apply(verts, K, sctx, orig_size)


def render_rgbd(verts, K, sctx, textures, light_direction=(0, 1, 0), intensity_ambient=0.5, intensity_directional=0.5,
                background_color=(0, 0, 0), orig_size=1.0):
    """`renderer.render(vertices, faces, textures, K=)` -> (rgb (B,3,S,S), depth (B,S,S), alpha (B,S,S)) for the
    reference's per-face colour textures (B,F,1,1,1,3) (reference homan/homan.py:510-545).  Visualisation only: no
    gradient.  Rasterises with csrc/raster_*.hip (hm_sil_fwd) and shades its index map (hm_shade_rgb)."""
    import ctypes
    with torch.no_grad():
        verts, K = _f32(verts.detach()), _f32(K)
        alpha, depth = _DepthRender.apply(verts, K, sctx, orig_size)      # (cropped to the requested size)
        tex = _f32(textures.reshape(sctx.B, sctx.F, 3))
        rgb = torch.empty(sctx.B, 3, sctx.S, sctx.S, device=verts.device)
        ld = (ctypes.c_float * 3)(*[float(x) for x in light_direction])
        bg = (ctypes.c_float * 3)(*[float(x) for x in background_color])
        _lib.check(_lib.lib().hm_shade_rgb(_lib.ptr(verts), _lib.ptr(sctx.faces), 0, _lib.ptr(tex), sctx.B, sctx.V,
                                           sctx.F, sctx.S, ctypes.cast(ld, ctypes.c_void_p),
                                           float(intensity_ambient), float(intensity_directional),
                                           ctypes.cast(bg, ctypes.c_void_p), _lib.ptr(rgb), _lib.ptr(sctx.workspace),
                                           _lib.stream()), "hm_shade_rgb")
    return sctx.crop(rgb), depth, alpha


class _OrdinalDepthLoss(torch.autograd.Function):
    """reference homan/lossutils.py:133-169 for the two layers (object, hand) of homan/homan.py:384-419."""

    @staticmethod
    def forward(ctx, d0, d1, a0, a1, m0, m1, rws):
        d0, d1, a0, a1 = _f32(d0), _f32(d1), _f32(a0), _f32(a1)
        B, S = d0.shape[0], d0.shape[1]
        assert d0.shape == d1.shape == a0.shape == a1.shape == m0.shape == m1.shape == (B, S, S)
        assert m0.dtype == torch.uint8 and m1.dtype == torch.uint8 and m0.is_contiguous() and m1.is_contiguous()
        part = torch.zeros(B * 8, device=d0.device)          # (per-frame records: zero on entry, see the header)
        rec = torch.empty(5, device=d0.device)
        out = torch.empty(1, device=d0.device)
        _lib.check(_lib.lib().hm_ordinal_depth_fwd(
            _lib.ptr(d0), _lib.ptr(d1), _lib.ptr(a0), _lib.ptr(a1), _lib.ptr(m0), _lib.ptr(m1), B, S, _lib.ptr(part),
            _lib.ptr(rec), _lib.ptr(out), _lib.ptr(rws.buf), _lib.stream()), "hm_ordinal_depth_fwd")
        ctx.save_for_backward(d0, d1, a0, a1, m0, m1, rec)
        pairs = rec[:1].clone()             # the normaliser of this pair of layers (a count of frames: no gradient)
        ctx.mark_non_differentiable(pairs)
        return out.reshape(()), pairs

    @staticmethod
    def backward(ctx, g, _g_pairs=None):
        d0, d1, a0, a1, m0, m1, rec = ctx.saved_tensors
        g0, g1 = torch.empty_like(d0), torch.empty_like(d1)
        _lib.check(_lib.lib().hm_ordinal_depth_bwd(
            _lib.ptr(d0), _lib.ptr(d1), _lib.ptr(a0), _lib.ptr(a1), _lib.ptr(m0), _lib.ptr(m1), d0.shape[0], d0.shape[1],
            _lib.ptr(rec), _lib.ptr(_f32(g).reshape(1)), _lib.ptr(g0), _lib.ptr(g1), _lib.stream()), "hm_ordinal_depth_bwd")
        return g0, g1, None, None, None, None, None


def ordinal_depth_loss(d_obj, d_hand, sil_obj, sil_hand, mask_obj, mask_hand, rws):
    """0-d loss.  mask_*: (B,S,S) uint8 instance masks."""
    return _OrdinalDepthLoss.apply(d_obj, d_hand, sil_obj, sil_hand, mask_obj, mask_hand, rws)[0]


def ordinal_depth_loss_layers(depths, sils, masks, rws):
    """The ordinal depth term over n >= 2 layers (reference homan/lossutils.py:133-169: every ordered pair of layers, one
    normaliser for all - the number of (pair, frame) combinations whose two silhouettes meet, a layer with itself included).
    Every unordered pair goes through the two-layer kernels, which normalise by the pair's OWN count; the pair's value times
    (its count / the scene's count) is its share of the scene's loss, and autograd carries the same factor into the gradients.
    depths / sils: n x (B,S,S) float renders, masks: n x (B,S,S) uint8."""
    n = len(depths)
    if n == 2:
        return ordinal_depth_loss(depths[0], depths[1], sils[0], sils[1], masks[0], masks[1], rws)
    with torch.no_grad():
        present = [(s == 1).flatten(1).any(1).sum().float() for s in sils]          # frames in which layer i covers a pixel fully
    terms, counts = [], []
    for a in range(n):
        for b in range(a + 1, n):
            val, pairs = _OrdinalDepthLoss.apply(depths[a], depths[b], sils[a], sils[b], masks[a], masks[b], rws)
            terms.append((val, pairs[0]))
            counts.append(pairs[0] - present[a] - present[b])                       # = 2 x frames in which a and b meet
    total = sum(present) + sum(counts)
    loss = torch.zeros((), device=depths[0].device)
    for val, pairs in terms:
        loss = loss + torch.where(pairs > 0, val * (pairs / total), torch.zeros_like(val))
    return loss


class DepthObsScratch:
    """The caller's scratch of hm_depth_obs_fwd for L layers of B frames: the records' integer words and the ticket, zero-filled
    once (every call leaves them zero).  Allocated outside any stream capture and kept by whoever calls the term repeatedly."""

    def __init__(self, layers, batch, device):
        nbytes = _lib.lib().hm_depth_obs_acc_bytes(int(layers), int(batch))
        if nbytes == 0:
            raise _lib.HomanAmdError(f"observed-depth term: unsupported shape L={layers} B={batch}")
        self.L, self.B = int(layers), int(batch)
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)


class _DepthObsLoss(torch.autograd.Function):
    """The observed-depth term (csrc/depthobs.hip; the rule is in include/homan_amd.h): one forward launch over all layers, which
    also leaves the un-scaled clamped residuals; the backward scales them into the layers' gradient images in one launch."""

    @staticmethod
    def forward(ctx, depth_map, delta, scratch, sctxs, L, *images):
        depths, sils, masks = images[:L], images[L:2 * L], images[2 * L:]
        depths = [_lib.aligned(_f32(t), 16) for t in depths]
        sils = [_lib.aligned(_f32(t), 16) for t in sils]
        masks = [_lib.aligned(t.contiguous(), 4) for t in masks]
        depth_map = _lib.aligned(_f32(depth_map), 16)
        B, S = depths[0].shape[0], depths[0].shape[1]
        for t in depths + sils + masks + [depth_map]:
            assert tuple(t.shape) == (B, S, S), f"observed-depth term: image of shape {tuple(t.shape)}, expected {(B, S, S)}"
        assert all(m.dtype == torch.uint8 for m in masks) and (scratch.L, scratch.B) == (L, B)
        dev = depths[0].device
        clamped = [torch.empty(B, S, S, device=dev) for _ in range(L)]
        records = torch.empty(L, B, 2, device=dev)
        out = torch.empty(4, device=dev)
        p3 = lambda ts: [_lib.ptr(ts[i]) if i < L else None for i in range(3)]
        _lib.check(_lib.lib().hm_depth_obs_fwd(*p3(depths), *p3(sils), *p3(masks), _lib.ptr(depth_map), L, B, S, float(delta),
                                               NMR_NEAR, NMR_FAR, *p3(clamped), _lib.ptr(scratch.buf), _lib.ptr(records),
                                               _lib.ptr(out), _lib.stream()), "hm_depth_obs_fwd")
        ctx.save_for_backward(records, out, *clamped)
        ctx.sctxs, ctx.L = sctxs, L
        loss, stats = out[0].clone(), out[1:].clone()        # (stats: mean |r|, valid share, N - no gradient)
        ctx.mark_non_differentiable(stats, records)
        return loss, stats, records

    @staticmethod
    def backward(ctx, g_loss, *_unused):
        records, out, *clamped = ctx.saved_tensors
        L, (B, S) = ctx.L, clamped[0].shape[:2]
        grads = [torch.empty_like(c) for c in clamped]
        # the non-zero flags of hm_depth_bwd_sparse, when the caller named the renders' contexts (the masks cover a small part of
        # the image) and the size has whole 64-pixel segments
        flags = ([torch.empty(B * S * (S // 64), dtype=torch.uint8, device=records.device) for _ in range(L)]
                 if ctx.sctxs is not None and S % 64 == 0 else [])
        p3 = lambda ts: [_lib.ptr(ts[i]) if i < len(ts) else None for i in range(3)]
        _lib.check(_lib.lib().hm_depth_obs_bwd(*p3(clamped), L, B, S, _lib.ptr(records), _lib.ptr(out),
                                               _lib.ptr(_f32(g_loss).reshape(1)), *p3(grads), *p3(flags), _lib.stream()),
                   "hm_depth_obs_bwd")
        for sctx, g, f in zip(ctx.sctxs or [], grads, flags):
            sctx.offer_gflags(g, f)
        return (None, None, None, None, None) + tuple(grads) + (None,) * (2 * L)


def depth_obs_loss(depths, sils, masks, depth_map, delta, scratch=None, sctxs=None, detail=False):
    """The observed-depth term over 1..3 layers -> (0-d loss, mean |residual| over the valid pixels [m], valid pixels / mask
    pixels with a usable sensor value); the two metrics carry no gradient.  depths / sils: the layers' (B,S,S) renders
    (depth_render), masks: their (B,S,S) uint8 instance masks, depth_map (B,S,S) fp32 metres at the masks' resolution and in the
    renders' camera (NaN, infinite, zero, negative and out-of-range values are ignored), 0 < delta <= 1 the Huber threshold [m].
    scratch: a DepthObsScratch(L, B) kept by the caller (required under stream capture; else one is made for the call).
    sctxs: the renders' SilhouetteContexts, ONLY when this term is the sole consumer of their depth images - their depth backward
    then takes the sparse path on the flags this term's backward writes (image sizes that are multiples of 64).
    detail=True appends (number of (layer, frame) with a valid pixel, records (L,B,2) = valid pixels, sum of rho)."""
    L = len(depths)
    if not (1 <= L <= 3 and len(sils) == L and len(masks) == L):
        raise ValueError(f"observed-depth term: 1 to 3 layers with a silhouette and a mask each, got {L}/{len(sils)}/{len(masks)}")
    if not 0 < float(delta) <= 1:
        raise ValueError(f"observed-depth term: delta {delta} must lie in (0, 1] (metres)")
    if sctxs is not None and len(sctxs) != L:
        raise ValueError("observed-depth term: one raster context per layer")
    if scratch is None:
        scratch = DepthObsScratch(L, depths[0].shape[0], depths[0].device)
    loss, stats, records = _DepthObsLoss.apply(depth_map, float(delta), scratch, sctxs, L, *depths, *sils, *masks)
    return (loss, stats[0], stats[1]) + ((stats[2], records) if detail else ())


def register_depth(frames, depth_scale, Kd, T, Kc, size, znear=NMR_NEAR, zfar=NMR_FAR, edge_radius=1, edge_jump_abs=0.02,
                   edge_jump_rel=0.0, max_splat=8, out=None, stats=None):
    """hm_depth_register (csrc/depthprep.hip; the rule is in include/homan_amd.h): raw sensor frames (B,Hd,Wd), uint16 or fp32
    device tensor, -> ((B,size,size) fp32 metres in the colour camera with 0 = no measurement, stats (B,4) int32 = valid source
    pixels, dropped by the edge filter, dropped by the range / splat rules, valid target pixels).  Kd (3,3) or (B,3,3) pixel
    intrinsics of the depth camera, T (3,4) or (B,3,4) depth -> colour, Kc (3,3) or (B,3,3) normalised `camintr`: fp32 device
    tensors.  Three launches on the current stream, nothing else: with `out` / `stats` given the call can be captured."""
    if frames.dtype not in (torch.uint16, torch.float32) or frames.dim() != 3:
        raise ValueError(f"register_depth: frames must be (B, Hd, Wd) uint16 or float32, got {tuple(frames.shape)} {frames.dtype}")
    B, Hd, Wd = frames.shape
    mats = []
    for name, m, shape in (("Kd", Kd, (3, 3)), ("T", T, (3, 4)), ("Kc", Kc, (3, 3))):
        if m.dtype != torch.float32 or tuple(m.shape) not in (shape, (B,) + shape):
            raise ValueError(f"register_depth: {name} must be fp32 {shape} or {(B,) + shape}, got {tuple(m.shape)} {m.dtype}")
        mats.append((m.contiguous(), int(m.dim() == 3)))
    size = int(size)
    frames = frames.contiguous()
    out = torch.empty(B, size, size, dtype=torch.float32, device=frames.device) if out is None else out
    stats = torch.empty(B, 4, dtype=torch.int32, device=frames.device) if stats is None else stats
    assert tuple(out.shape) == (B, size, size) and out.dtype == torch.float32 and tuple(stats.shape) == (B, 4)
    assert stats.dtype == torch.int32
    (kd, kd_s), (t, t_s), (kc, kc_s) = mats
    _lib.check(_lib.lib().hm_depth_register(_lib.ptr(frames), int(frames.dtype == torch.float32), B, Hd, Wd, float(depth_scale),
                                            _lib.ptr(kd), kd_s, _lib.ptr(t), t_s, _lib.ptr(kc), kc_s, size, float(znear),
                                            float(zfar), int(edge_radius), float(edge_jump_abs), float(edge_jump_rel),
                                            int(max_splat), _lib.ptr(out), _lib.ptr(stats), _lib.stream()), "hm_depth_register")
    return out, stats


# =============================================================================== shared small state
class ReduceWorkspace:
    """Zero-initialised scratch for the single-launch grid reductions (partials + self-resetting ticket)."""

    def __init__(self, device):
        self.buf = torch.zeros(_lib.lib().hm_reduce_workspace_bytes(), dtype=torch.uint8, device=device)


def _scale_by(unit, g):
    """g (scalar tensor) * unit, in a HIP kernel."""
    out = torch.empty_like(unit)
    g = _f32(g).reshape(1)
    _lib.check(_lib.lib().hm_scale_by(_lib.ptr(unit), _lib.ptr(g), unit.numel(), _lib.ptr(out), _lib.stream()),
               "hm_scale_by")
    return out


# =============================================================================== rigid transform
_RIGID_WS = {}


def _rigid_workspace(N, device):
    """Zero-initialised ticket / partials buffer of hm_rigid_bwd, one per (frames, device, stream)."""
    key = (N, str(device), torch.cuda.current_stream().cuda_stream)
    if key not in _RIGID_WS:
        _RIGID_WS[key] = torch.zeros(_lib.lib().hm_rigid_workspace_bytes(N), dtype=torch.uint8, device=device)
    return _RIGID_WS[key]


class _RigidTransform(torch.autograd.Function):
    """reference homan/utils/geometry.py:9-27 + homan/utils/camera.py:108-139:
    verts = (s * mesh) @ rot6d_to_matrix(rot6d) + t, and the mesh-detached twin (same values; its gradient
    reaches rotation and translation only)."""

    @staticmethod
    def forward(ctx, mesh, rot6d, trans, scale, abs_scale):
        mesh, rot6d, trans, scale = _f32(mesh), _f32(rot6d), _f32(trans), _f32(scale)
        N, V = mesh.shape[0], mesh.shape[1]
        verts = torch.empty_like(mesh)
        _lib.check(_lib.lib().hm_rigid_fwd(_lib.ptr(mesh), _lib.ptr(rot6d), _lib.ptr(trans), _lib.ptr(scale),
                                           int(abs_scale), N, V, None, _lib.ptr(verts), _lib.stream()), "hm_rigid_fwd")
        ctx.save_for_backward(mesh, rot6d, scale)
        ctx.abs_scale = int(abs_scale)
        ctx.trans_shape = trans.shape
        return verts, verts.clone()

    @staticmethod
    def backward(ctx, g_full, g_det):
        mesh, rot6d, scale = ctx.saved_tensors
        N, V = mesh.shape[0], mesh.shape[1]
        need_mesh, need_scale = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        g_full = None if g_full is None else _f32(g_full)
        g_det = None if g_det is None else _f32(g_det)
        g_mesh = torch.empty_like(mesh) if need_mesh else None
        g_rot = torch.empty_like(rot6d)
        g_trans = torch.empty(N, 3, device=mesh.device)
        g_sp = torch.empty(N, device=mesh.device) if need_scale else None
        tp, tw, tn = _lib.terms([(g_full, 1.0)])
        _lib.check(_lib.lib().hm_rigid_bwd(_lib.ptr(mesh), _lib.ptr(rot6d), _lib.ptr(scale), ctx.abs_scale, tp, tw, tn,
                                           _lib.ptr(g_det), None, 0, 0.0, N, V, _lib.ptr(g_mesh), _lib.ptr(g_rot),
                                           _lib.ptr(g_trans), _lib.ptr(g_sp), _lib.ptr(_rigid_workspace(N, mesh.device)),
                                           _lib.stream()), "hm_rigid_bwd")
        g_scale = g_sp.sum().reshape(scale.shape) if need_scale else None
        return g_mesh, g_rot, g_trans.view(ctx.trans_shape), g_scale, None


def rigid_transform(mesh, rot6d, trans, scale, abs_scale=False):
    return _RigidTransform.apply(mesh, rot6d, trans, scale, abs_scale)


# =============================================================================== MANO
class ManoContext:
    """Device copy of the MANO model in the kernel layout (see csrc/mano.hip) + backward workspace."""

    def __init__(self, model_np, device, num_pca_comps=16, flat_hand_mean=False):
        import ctypes
        assert num_pca_comps == 16, "the reference builds ManoModel(pca_comps=16) (homan/homan.py:70)"
        from .mano_assets import kernel_layout
        self.tensors = [torch.from_numpy(a).to(device) for a in kernel_layout(model_np, flat_hand_mean)]
        self.ptrs = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in self.tensors])
        self.device = device
        self._ws = {}

    def workspace(self, B):
        if B not in self._ws:
            self._ws[B] = torch.zeros(_lib.lib().hm_mano_workspace_bytes(B), dtype=torch.uint8, device=self.device)
        return self._ws[B]


class _ManoLBS(torch.autograd.Function):
    """reference homan/manomodel.py:84-151 (forward_pca, right hand) + the `mano` layer + homan/homan.py:356 (+mano_trans)."""

    @staticmethod
    def forward(ctx, pca, rot, betas, trans, mctx):
        pca, rot, betas = _f32(pca), _f32(rot), _f32(betas)
        trans = None if trans is None else _f32(trans)
        B, P = pca.shape
        verts = torch.empty(B, 778, 3, device=pca.device)
        state = torch.empty(_lib.lib().hm_mano_state_bytes(B), dtype=torch.uint8, device=pca.device)
        _lib.check(_lib.lib().hm_mano_fwd(mctx.ptrs, _lib.ptr(pca), P, _lib.ptr(rot), _lib.ptr(betas), _lib.ptr(trans), B,
                                          _lib.ptr(verts), None, None, None, None, None, _lib.ptr(state), _lib.stream()),
                   "hm_mano_fwd")
        ctx.save_for_backward(pca, rot, betas, state)
        ctx.mctx, ctx.has_trans = mctx, trans is not None
        return verts

    @staticmethod
    def backward(ctx, g_verts):
        pca, rot, betas, state = ctx.saved_tensors
        B, P = pca.shape
        g_verts = _f32(g_verts)
        g_pca, g_rot, g_betas = torch.empty_like(pca), torch.empty_like(rot), torch.empty_like(betas)
        g_trans = torch.empty(B, 3, device=pca.device)
        _lib.check(_lib.lib().hm_mano_bwd(ctx.mctx.ptrs, _lib.ptr(pca), P, _lib.ptr(rot), _lib.ptr(betas), B,
                                          _lib.ptr(g_verts), None, 0.0, _lib.ptr(g_pca), _lib.ptr(g_rot), _lib.ptr(g_betas),
                                          _lib.ptr(g_trans), _lib.ptr(state), _lib.ptr(ctx.mctx.workspace(B)),
                                          _lib.stream()), "hm_mano_bwd")
        return g_pca, g_rot, g_betas, (g_trans if ctx.has_trans else None), None


def mano_lbs(pca, rot, betas, trans, mctx):
    return _ManoLBS.apply(pca, rot, betas, trans, mctx)


def mano_joints(pca, rot, betas, trans, mctx):
    """Posed joints (B,16,3), no gradient (reference homan/homan.py:309-339 is off the optimisation path)."""
    pca, rot, betas = _f32(pca.detach()), _f32(rot.detach()), _f32(betas.detach())
    B, P = pca.shape
    verts = torch.empty(B, 778, 3, device=pca.device)
    joints = torch.empty(B, 16, 3, device=pca.device)
    tr = None if trans is None else _f32(trans.detach())
    _lib.check(_lib.lib().hm_mano_fwd(mctx.ptrs, _lib.ptr(pca), P, _lib.ptr(rot), _lib.ptr(betas), _lib.ptr(tr), B,
                                      _lib.ptr(verts), _lib.ptr(joints), None, None, None, None, None, _lib.stream()),
               "hm_mano_fwd")
    return verts, joints


# =============================================================================== vertex losses
class _V2dLoss(torch.autograd.Function):
    """reference homan/losses.py:141-164."""

    @staticmethod
    def forward(ctx, verts, camintr, ref2d, image_size, hand_nb, rws):
        verts = _f32(verts)
        N, V = verts.shape[:2]
        unit = torch.empty_like(verts)
        out = torch.empty(2, device=verts.device)
        _lib.check(_lib.lib().hm_v2d_fwd(_lib.ptr(verts), _lib.ptr(camintr), int(hand_nb), _lib.ptr(ref2d),
                                         float(image_size), N, V, _lib.ptr(unit), _lib.ptr(out), _lib.ptr(rws.buf),
                                         _lib.stream()), "hm_v2d_fwd")
        ctx.save_for_backward(unit)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_loss, _g_metric):
        (unit,) = ctx.saved_tensors
        return _scale_by(unit, g_loss), None, None, None, None, None


def v2d_loss(verts, camintr, ref2d, image_size, hand_nb, rws):
    return _V2dLoss.apply(verts, camintr, ref2d, image_size, hand_nb, rws)


class _SmoothLoss(torch.autograd.Function):
    """reference homan/lossutils.py:18-36 (one term: hand or object)."""

    @staticmethod
    def forward(ctx, verts, hand_nb, rws):
        verts = _f32(verts)
        N, V = verts.shape[:2]
        unit = torch.empty_like(verts)
        out = torch.empty(1, device=verts.device)
        _lib.check(_lib.lib().hm_smooth_fwd(_lib.ptr(verts), N, V, int(hand_nb), _lib.ptr(unit), _lib.ptr(out),
                                            _lib.ptr(rws.buf), _lib.stream()), "hm_smooth_fwd")
        ctx.save_for_backward(unit)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (unit,) = ctx.saved_tensors
        return _scale_by(unit, g), None, None


def smooth_loss(verts, hand_nb, rws):
    return _SmoothLoss.apply(verts, hand_nb, rws)


class _Priors(torch.autograd.Function):
    """reference homan/lossutils.py:39-40 (mean(pca^2)) and :107-109 (scale priors)."""

    @staticmethod
    def forward(ctx, pca, s_obj, m_obj, s_hand, m_hand):
        pca, s_obj, s_hand = _f32(pca), _f32(s_obj), _f32(s_hand)
        g_pca = torch.empty_like(pca)
        g_so, g_sh = torch.empty_like(s_obj), torch.empty_like(s_hand)
        out = torch.empty(3, device=pca.device)
        _lib.check(_lib.lib().hm_priors_fwd(_lib.ptr(pca), pca.numel(), _lib.ptr(s_obj), _lib.ptr(m_obj),
                                            _lib.ptr(s_hand), _lib.ptr(m_hand), _lib.ptr(g_pca), _lib.ptr(g_so),
                                            _lib.ptr(g_sh), _lib.ptr(out), _lib.stream()), "hm_priors_fwd")
        ctx.save_for_backward(g_pca, g_so, g_sh)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g0, g1, g2):
        g_pca, g_so, g_sh = ctx.saved_tensors
        return (_scale_by(g_pca, g0) if ctx.needs_input_grad[0] else None,
                _scale_by(g_so, g1) if ctx.needs_input_grad[1] else None, None,
                _scale_by(g_sh, g2) if ctx.needs_input_grad[3] else None, None)


def priors(pca, s_obj, m_obj, s_hand, m_hand):
    return _Priors.apply(pca, s_obj, m_obj, s_hand, m_hand)


class _KeypointTerms(torch.autograd.Function):
    """hm_keypoint_terms_clips (csrc/handinit.hip; no reference counterpart): the 21 regressed keypoints of camera-space MANO
    vertices against 2-D / 3-D targets.  Differentiable output: total (C,) = lw_kp2d L2d + lw_kp3d L3d per clip."""

    @staticmethod
    def forward(ctx, verts, W, camintr, kp2d, c2, s, kp3d, c3, sigma, znear, clip_len, lw_kp2d, lw_kp3d):
        verts = _f32(verts)
        N = verts.shape[0]
        C = N // clip_len if clip_len > 0 else 0
        dev = verts.device
        keypoints, unit = torch.empty(N, 21, 3, device=dev), torch.empty_like(verts)
        row_parts, tickets = torch.empty(N, 2, device=dev), torch.zeros(max(C, 1), dtype=torch.int32, device=dev)
        out = torch.empty(max(C, 1), 2, device=dev)
        _lib.check(_lib.lib().hm_keypoint_terms_clips(_p(verts), _p(W), _p(camintr), _p(kp2d), _p(c2), _p(s), _p(kp3d), _p(c3),
                                                      float(sigma), float(znear), float(lw_kp2d), float(lw_kp3d), N, int(clip_len),
                                                      _p(keypoints), _p(unit), _p(row_parts), _p(tickets), _p(out), 2,
                                                      _lib.stream()), "hm_keypoint_terms_clips")
        ctx.save_for_backward(unit)
        ctx.clip_len = int(clip_len)
        l2, l3 = out[:, 0], out[:, 1]
        total = float(lw_kp2d) * l2 + float(lw_kp3d) * l3
        ctx.mark_non_differentiable(l2, l3, keypoints)
        return total, l2, l3, keypoints

    @staticmethod
    def backward(ctx, g_total, _g2, _g3, _gk):
        (unit,) = ctx.saved_tensors
        B = ctx.clip_len
        g_total = _f32(g_total)
        g = torch.cat([_scale_by(unit[c * B:(c + 1) * B], g_total[c]) for c in range(unit.shape[0] // B)])
        return (g,) + (None,) * 12


def keypoint_terms(verts_world, W, camintr, kp2d, c2, s, kp3d=None, c3=None, sigma=1.0, znear=0.01, clip_len=1, lw_kp2d=1.0,
                   lw_kp3d=1.0):
    """verts_world (N,778,3) camera-space MANO vertices, W (21,778) (handinit.keypoint_regressor), camintr (N,3,3) pixels, kp2d
    (N,21,2) pixels, c2 (N,21) >= 0, s (N) box scales in pixels, kp3d (N,21,3) / c3 (N,21) optional, clips of clip_len rows
    -> (total (C,), L2d (C,), L3d (C,), keypoints (N,21,3)); the gradient flows through `total` = lw_kp2d L2d + lw_kp3d L3d
    (the rules: include/homan_amd.h)."""
    f = lambda t: None if t is None else _f32(t)
    return _KeypointTerms.apply(verts_world, f(W), f(camintr), f(kp2d), f(c2), f(s), f(kp3d), f(c3), sigma, znear, clip_len,
                                lw_kp2d, lw_kp3d)


class _InterLoss(torch.autograd.Function):
    """reference homan/losses.py:199-242 ('centroid'), gating :98-139; returns the un-normalised sum, shape (1,)."""

    @staticmethod
    def forward(ctx, vh, vo, camintr, expansion, zthresh, rws):
        vh, vo = _f32(vh), _f32(vo)
        B, Vh, Vo = vo.shape[0], vh.shape[1], vo.shape[1]
        assert vh.shape[0] == B, "one hand per frame"
        rec = torch.empty(B, 8, device=vh.device)
        out = torch.empty(1, device=vh.device)
        _lib.check(_lib.lib().hm_inter_fwd(_lib.ptr(vh), _lib.ptr(vo), _lib.ptr(camintr), B, Vh, Vo, float(expansion),
                                           float(zthresh), _lib.ptr(rec), _lib.ptr(out), _lib.ptr(rws.buf),
                                           _lib.stream()), "hm_inter_fwd")
        ctx.save_for_backward(rec)
        ctx.dims = (B, Vh, Vo)
        return out

    @staticmethod
    def backward(ctx, g):
        (rec,) = ctx.saved_tensors
        B, Vh, Vo = ctx.dims
        g = _f32(g).reshape(1)
        gh = torch.empty(B, Vh, 3, device=rec.device) if ctx.needs_input_grad[0] else None
        go = torch.empty(B, Vo, 3, device=rec.device) if ctx.needs_input_grad[1] else None
        if gh is not None or go is not None:
            _lib.check(_lib.lib().hm_inter_bwd(_lib.ptr(rec), _lib.ptr(g), B, Vh, Vo, _lib.ptr(gh), _lib.ptr(go),
                                               _lib.stream()), "hm_inter_bwd")
        return gh, go, None, None, None, None


def inter_loss(vh, vo, camintr, rws, expansion=0.2, zthresh=3.0):
    return _InterLoss.apply(vh, vo, camintr, expansion, zthresh, rws)


def interaction_flags(vh, vo, camintr, rws, expansion=0.2, zthresh=3.0):
    """(B,) bool, no grad: which frames the coarse interaction term applies to (expanded 2-D boxes overlap and the depth ranges
    are closer than `zthresh`; reference homan/losses.py:98-139), from the frame records of hm_inter_fwd."""
    with torch.no_grad():
        vh, vo = _f32(vh.detach()), _f32(vo.detach())
        B = vo.shape[0]
        rec = torch.empty(B, 8, device=vh.device)
        out = torch.empty(1, device=vh.device)
        _lib.check(_lib.lib().hm_inter_fwd(_lib.ptr(vh), _lib.ptr(vo), _lib.ptr(camintr), B, vh.shape[1], vo.shape[1],
                                           float(expansion), float(zthresh), _lib.ptr(rec), _lib.ptr(out), _lib.ptr(rws.buf),
                                           _lib.stream()), "hm_inter_fwd")
        return rec[:, 0] != 0


def nearest_vertices(vh, vo, rws, metric_only=False):
    """hand -> object nearest vertex (no grad): idx (B,Vh) int32, squared distance, and the metric
    max_b min_{i,j} |h_i - o_j| of reference homan/losses.py:225-241.  metric_only: (None, None, metric) - the same exact
    value from the pruned search."""
    vh, vo = _f32(vh.detach()), _f32(vo.detach())
    B, Vh, Vo = vo.shape[0], vh.shape[1], vo.shape[1]
    idx = None if metric_only else torch.empty(B, Vh, dtype=torch.int32, device=vh.device)
    d2 = None if metric_only else torch.empty(B, Vh, device=vh.device)
    metric = torch.empty(1, device=vh.device)
    _lib.check(_lib.lib().hm_nn_fwd(_lib.ptr(vh), _lib.ptr(vo), B, Vh, Vo, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(metric),
                                    _lib.ptr(rws.buf), _lib.stream()), "hm_nn_fwd")
    return idx, d2, metric


class _ContactLoss(torch.autograd.Function):
    """reference homan/lossutils.py:112-130 -> interactions/contactloss.py:149-309 as executed (appendix B.1)."""

    @staticmethod
    def forward(ctx, vh, vo, nn_idx, thresh, rws):
        vh, vo = _f32(vh), _f32(vo)
        B, Vh, Vo = vo.shape[0], vh.shape[1], vo.shape[1]
        gh, go = torch.empty_like(vh), torch.empty_like(vo)
        out = torch.empty(1, device=vh.device)
        _lib.check(_lib.lib().hm_contact_fwd(_lib.ptr(vh), _lib.ptr(vo), _lib.ptr(nn_idx), B, Vh, Vo, float(thresh),
                                             _lib.ptr(gh), _lib.ptr(go), _lib.ptr(out), _lib.ptr(rws.buf),
                                             _lib.stream()), "hm_contact_fwd")
        ctx.save_for_backward(gh, go)
        return out

    @staticmethod
    def backward(ctx, g):
        gh, go = ctx.saved_tensors
        return (_scale_by(gh, g) if ctx.needs_input_grad[0] else None,
                _scale_by(go, g) if ctx.needs_input_grad[1] else None, None, None, None)


def contact_loss(vh, vo, nn_idx, rws, thresh=0.020):
    return _ContactLoss.apply(vh, vo, nn_idx, thresh, rws)


class CollisionContext:
    def __init__(self, faces_hand_closed, faces_obj, B, Vh, Vo, device):
        self.f0 = torch.as_tensor(np.asarray(faces_hand_closed), dtype=torch.int32).to(device).contiguous()
        self.f1 = faces_obj.to(device=device, dtype=torch.int32).contiguous()
        self.B, self.V0, self.V1 = B, Vh, Vo
        self.ws = torch.zeros(_lib.lib().hm_collision_workspace_bytes(B, Vh, Vo, self.f0.shape[0], self.f1.shape[0]),
                              dtype=torch.uint8, device=device)

    def grid(self, which):
        """clamp(SDF,0) (B,32,32,32) of mesh `which` from the last forward (debug / API completeness)."""
        f = self.f0 if which == 0 else self.f1
        V = self.V0 if which == 0 else self.V1
        phi = torch.empty(self.B, 32, 32, 32, device=self.ws.device)
        _lib.check(_lib.lib().hm_collision_read_grid(_lib.ptr(f), V, f.shape[0], self.B, which, self.V0, self.V1,
                                                     self.f0.shape[0], self.f1.shape[0], _lib.ptr(phi),
                                                     _lib.ptr(self.ws), _lib.stream()),
                   "hm_collision_read_grid")
        return phi

    def needed(self, which):
        """The lazy evaluation of the last forward for mesh `which` (debug): need-mask (B,32,32) int32 words (bit i of word
        [z][y] <-> voxel (z,y,i) is inside and touched by a sample), list length (B) int32, and phi (B,32,32,32) as the
        workspace holds it - defined only where the need bit is set."""
        dev = self.ws.device
        mask = torch.empty(self.B, 32, 32, dtype=torch.int32, device=dev)
        cnt = torch.empty(self.B, dtype=torch.int32, device=dev)
        phi = torch.empty(self.B, 32, 32, 32, device=dev)
        _lib.check(_lib.lib().hm_collision_read_needed(self.B, which, self.V0, self.V1, self.f0.shape[0], self.f1.shape[0],
                                                       _lib.ptr(mask), _lib.ptr(cnt), _lib.ptr(phi), _lib.ptr(self.ws),
                                                       _lib.stream()), "hm_collision_read_needed")
        return mask, cnt, phi


class _CollisionLoss(torch.autograd.Function):
    """reference homan/lossutils.py:43-64 (sdf branch) -> interactions/scenesdf.py:77-148."""

    @staticmethod
    def forward(ctx, vh, vo, cctx, scale_factor):
        vh, vo = _f32(vh), _f32(vo)
        g0, g1 = torch.empty_like(vh), torch.empty_like(vo)
        out = torch.empty(1, device=vh.device)
        _lib.check(_lib.lib().hm_collision_fwd(_lib.ptr(vh), _lib.ptr(cctx.f0), cctx.V0, cctx.f0.shape[0], _lib.ptr(vo),
                                               _lib.ptr(cctx.f1), cctx.V1, cctx.f1.shape[0], cctx.B, float(scale_factor),
                                               _lib.ptr(g0), _lib.ptr(g1), _lib.ptr(out), _lib.ptr(cctx.ws),
                                               _lib.stream()), "hm_collision_fwd")
        ctx.save_for_backward(g0, g1)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        g0, g1 = ctx.saved_tensors
        return (_scale_by(g0, g) if ctx.needs_input_grad[0] else None,
                _scale_by(g1, g) if ctx.needs_input_grad[1] else None, None, None)


def collision_loss(vh, vo, cctx, scale_factor=0.2):
    return _CollisionLoss.apply(vh, vo, cctx, scale_factor)


def collision_dist_values(vh, vo, cctx, scale_factor=0.2):
    """`sdf_meta["dist_values"]` of reference homan/interactions/scenesdf.py:141-146 for the two-mesh scene
    [hand, object]: {(1, 0): (B,Vh) depth of the hand vertices inside the object, (0, 1): (B,Vo) the reverse}, world
    units, no gradient.  Runs the SDF forward on (vh, vo) and samples its grids (csrc/sdf.hip)."""
    with torch.no_grad():
        vh, vo = _f32(vh.detach()), _f32(vo.detach())
        collision_loss(vh, vo, cctx, scale_factor)
        dv0 = torch.empty(vh.shape[:2], device=vh.device)
        dv1 = torch.empty(vo.shape[:2], device=vo.device)
        _lib.check(_lib.lib().hm_collision_dist_values(_lib.ptr(vh), cctx.V0, _lib.ptr(vo), cctx.V1, cctx.f0.shape[0],
                                                       cctx.f1.shape[0], cctx.B, _lib.ptr(dv0), _lib.ptr(dv1),
                                                       _lib.ptr(cctx.ws), _lib.stream()), "hm_collision_dist_values")
    return {(1, 0): dv0, (0, 1): dv1}


def cloud_metrics(x, y, aff_x=None, aff_y=None, per_point=False):
    """Exact nearest neighbours between x (B,N,3) and y (B,M,3) in both directions (no grad; csrc/pointmetrics.hip) ->
    (B,4) float64 {mean d2 x->y, mean d2 y->x, mean distance x->y, mean |x_i - y_i| (NaN when N != M)} and, per_point,
    (x_d2 (B,N), x_idx (B,N) int32, y_d2 (B,M), y_idx (B,M) int32).  aff_x / aff_y (B,5) optional per-frame affine on load,
    rows (cx, cy, cz, div, mul): p' = ((p - c) / div) * mul."""
    x, y = _f32(x.detach()), _f32(y.detach())
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    dev = x.device
    out4 = torch.empty(B, 4, dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.lib().hm_cloud_metrics_workspace_bytes(B, N, M), dtype=torch.uint8, device=dev)
    pp = (torch.empty(B, N, device=dev), torch.empty(B, N, dtype=torch.int32, device=dev),
          torch.empty(B, M, device=dev), torch.empty(B, M, dtype=torch.int32, device=dev)) if per_point else (None,) * 4
    _lib.check(_lib.lib().hm_cloud_metrics(_lib.ptr(x), _lib.ptr(y), B, N, M, _lib.ptr(aff_x), _lib.ptr(aff_y),
                                           *[_lib.ptr(t) for t in pp], _lib.ptr(out4), _lib.ptr(ws), _lib.stream()),
               "hm_cloud_metrics")
    return (out4, pp) if per_point else out4


def align_stats(gt_hand, pred_hand, frames, pred_centroid_from_gt=True):
    """Hand alignment of reference homan/eval/pointmetrics.py:61-90 (no grad): hands (frames*hands, V, 3), frame-major ->
    aff_gt (frames,5), aff_pred (frames,5) (the cloud_metrics affines of the object search) and hand_mean (frames*hands)
    float64, the mean vertex distance of the aligned hands."""
    gt_hand, pred_hand = _f32(gt_hand.detach()), _f32(pred_hand.detach())
    hands, V = gt_hand.shape[0] // frames, gt_hand.shape[1]
    dev = gt_hand.device
    aff_gt, aff_pred = torch.empty(frames, 5, device=dev), torch.empty(frames, 5, device=dev)
    hand_mean = torch.empty(frames * hands, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().hm_align_stats(_lib.ptr(gt_hand), _lib.ptr(pred_hand), frames, hands, V, int(bool(pred_centroid_from_gt)),
                                         _lib.ptr(aff_gt), _lib.ptr(aff_pred), _lib.ptr(hand_mean), _lib.stream()),
               "hm_align_stats")
    return aff_gt, aff_pred, hand_mean


def keyframe_interp(key_vals, key_frames, frame_nb, gather=None, signs=(1.0, 1.0, 1.0), out_dtype=torch.float32):
    """Key-frame values (K,N,3) at the sorted host frame numbers `key_frames` -> every frame of the sequence, (frame_nb, M, 3)
    fp32 or fp64 (no grad; csrc/seqinterp.hip): the blend of reference homan/eval/ho3devalutils.py:53-96, then per-coordinate
    `signs` (+-1) and the row `gather` (M host indices into N, repeats allowed).  The library checks the host arrays before it
    enqueues anything; a refused call raises ValueError."""
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError(f"out_dtype must be float32 or float64, got {out_dtype}")
    key_vals = _f32(key_vals.detach())
    if key_vals.dim() != 3 or key_vals.shape[2] != 3:
        raise ValueError(f"key_vals: expected (K, N, 3), got {tuple(key_vals.shape)}")
    K, N = key_vals.shape[0], key_vals.shape[1]
    kf = np.ascontiguousarray(np.asarray(key_frames).reshape(-1), dtype=np.int32)
    if kf.shape[0] != K:
        raise ValueError(f"{kf.shape[0]} key frames for {K} key values")
    ga = None if gather is None else np.ascontiguousarray(np.asarray(gather).reshape(-1), dtype=np.int32)
    M = N if ga is None else ga.shape[0]
    sg = np.ascontiguousarray(np.asarray(signs, dtype=np.float32).reshape(-1))
    if sg.shape[0] != 3:
        raise ValueError("signs: three values, each +1 or -1")
    dev = key_vals.device
    kf_dev = torch.empty(max(K, 1), dtype=torch.int32, device=dev)
    ga_dev = None if ga is None else torch.empty(max(M, 1), dtype=torch.int32, device=dev)
    out = torch.empty(max(int(frame_nb), 0), M, 3, dtype=out_dtype, device=dev)
    rc = _lib.lib().hm_keyframe_interp(_lib.ptr(key_vals), kf.ctypes.data, K, N, int(frame_nb),
                                       None if ga is None else ga.ctypes.data, M, sg.ctypes.data,
                                       int(out_dtype == torch.float64), _lib.ptr(kf_dev), _lib.ptr(ga_dev), _lib.ptr(out),
                                       _lib.stream())
    if rc == -1:
        raise ValueError(f"hm_keyframe_interp refused its arguments: key frames {kf.tolist()[:8]}... must start at 0, increase "
                         f"strictly and end at or before frame_nb = {frame_nb}; gather must index [0, {N}); signs must be +-1")
    _lib.check(rc, "hm_keyframe_interp")
    return out


ALIGN_MODES = {"similarity": 0, "rigid_similarity": 1, "scale_trans": 2}


def _check_pair(pred, gt):
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"{name}: expected a float tensor, got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name}: expected a non-empty (B, N, 3) tensor, got {tuple(t.shape)}")
    if pred.shape != gt.shape:
        raise ValueError(f"pred and gt differ in shape: {tuple(pred.shape)} vs {tuple(gt.shape)}")


def procrustes_align(pred, gt, mode=0, anchors=(0, 4)):
    """Per-frame alignment of pred (B,N,3) onto gt (B,N,3) (no grad; csrc/evalalign.hip, formulas in include/homan_amd.h) ->
    aligned (B,N,3) fp32, err (B,N) float64 = |aligned_i - gt_i| before `aligned` is rounded, xform (B,13) float64
    {s, R row-major, t} with aligned = s * pred @ R.T + t.  mode 0 / "similarity": orthogonal factor, reflections allowed;
    1 / "rigid_similarity": proper rotation; 2 / "scale_trans": scale and translation off the two `anchors` (rows of N)."""
    mode = ALIGN_MODES.get(mode, mode)
    if mode not in (0, 1, 2):
        raise ValueError(f"mode must be one of {sorted(ALIGN_MODES)} or 0 / 1 / 2, got {mode!r}")
    _check_pair(pred, gt)
    B, N = pred.shape[0], pred.shape[1]
    a, b = (int(v) for v in anchors)
    if mode == 2 and not (0 <= a < N and 0 <= b < N):
        raise ValueError(f"anchors {(a, b)} out of range for {N} points")
    pred, gt = _f32(pred.detach()), _f32(gt.detach())
    dev = pred.device
    aligned = torch.empty(B, N, 3, device=dev)
    err = torch.empty(B, N, dtype=torch.float64, device=dev)
    xform = torch.empty(B, 13, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().hm_procrustes_align(_lib.ptr(pred), _lib.ptr(gt), B, N, mode, a, b, _lib.ptr(aligned), _lib.ptr(err),
                                              _lib.ptr(xform), _lib.stream()), "hm_procrustes_align")
    return aligned, err, xform


def threshold_counts(dist, val_max, steps=100):
    """Exact counts[k] = #(dist_i <= t_k) over t = np.linspace(0, val_max, steps) (no grad; csrc/evalalign.hip) -> (steps,)
    int64 on the device of `dist` (any shape, fp32 or float64; NaN counts nowhere)."""
    if not isinstance(dist, torch.Tensor) or dist.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"dist: expected a float32 or float64 tensor, got {getattr(dist, 'dtype', type(dist))}")
    steps = int(steps)
    if not 2 <= steps <= 1024:
        raise ValueError(f"steps must lie in [2, 1024], got {steps}")
    vmax = np.array([val_max], dtype=np.float64)
    if not (np.isfinite(vmax[0]) and vmax[0] > 0):
        raise ValueError(f"val_max must be positive and finite, got {val_max}")
    dist = dist.detach().contiguous()
    counts = torch.empty(steps, dtype=torch.int64, device=dist.device)
    _lib.check(_lib.lib().hm_threshold_counts(_lib.ptr(dist) if dist.numel() else None, dist.numel(),
                                              int(dist.dtype == torch.float64), vmax.ctypes.data, steps, _lib.ptr(counts),
                                              _lib.stream()), "hm_threshold_counts")
    return counts


def fscore(x_d2, y_d2, thresholds):
    """x_d2 (B,N), y_d2 (B,M): the squared fp32 nearest-neighbour distances of `cloud_metrics(pred, gt, per_point=True)`;
    thresholds: 1 to 8 floats -> (B,T,3) float64 {precision, recall, F}, strict < (no grad; csrc/evalalign.hip)."""
    ths = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
    if not 1 <= ths.shape[0] <= 8:
        raise ValueError(f"between 1 and 8 thresholds, got {ths.shape[0]}")
    for name, t in (("x_d2", x_d2), ("y_d2", y_d2)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name}: expected a non-empty (B, N) float32 tensor, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if x_d2.shape[0] != y_d2.shape[0]:
        raise ValueError(f"batch sizes differ: {x_d2.shape[0]} vs {y_d2.shape[0]}")
    x_d2, y_d2 = x_d2.detach().contiguous(), y_d2.detach().contiguous()
    B, T = x_d2.shape[0], ths.shape[0]
    out = torch.empty(B, T, 3, dtype=torch.float64, device=x_d2.device)
    _lib.check(_lib.lib().hm_fscore(_lib.ptr(x_d2), _lib.ptr(y_d2), B, x_d2.shape[1], y_d2.shape[1], ths.ctypes.data, T,
                                    _lib.ptr(out), _lib.stream()), "hm_fscore")
    return out


VOXEL_MAX_INDEX = 1 << 22        # beyond it ((float)i + 0.5f) * pitch is no longer a clean fp32 lattice (csrc/solidvox.hip)


def _check_mesh(verts, faces):
    """verts: non-empty float (B,V,3) tensor; faces: (F,3) integers in [0, V), host array or tensor -> int32 numpy (F,3)"""
    if not isinstance(verts, torch.Tensor) or not verts.is_floating_point():
        raise ValueError(f"verts: expected a float tensor, got {getattr(verts, 'dtype', type(verts))}")
    if verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[0] < 1 or verts.shape[1] < 1:
        raise ValueError(f"verts: expected a non-empty (B, V, 3) tensor, got {tuple(verts.shape)}")
    faces = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.dtype.kind not in "iu":
        raise ValueError(f"faces: expected a non-empty integer (F, 3) array, got {faces.dtype} {faces.shape}")
    if faces.min() < 0 or faces.max() >= verts.shape[1]:
        raise ValueError(f"faces index [{faces.min()}, {faces.max()}], outside the {verts.shape[1]} vertices")
    return np.ascontiguousarray(faces, dtype=np.int32)


def voxel_pitch(pitch):
    """the pitch rounded to fp32 once: that value is h everywhere (ValueError unless it is finite and positive)"""
    with np.errstate(over="ignore"):
        h = np.float32(pitch)
    if not (np.isfinite(h) and h > 0):
        raise ValueError(f"pitch must be positive and finite in fp32, got {pitch}")
    return h


def mesh_volume(verts, faces):
    """Exact volume of B closed meshes of one topology (no grad; csrc/solidvox.hip): verts (B,V,3), faces (F,3) -> (B,) float64
    |sum_f det(p1 - r, p2 - r, p3 - r)| / 6 about each frame's vertex 0, in double, summed in one fixed order."""
    faces = _check_mesh(verts, faces)
    verts = _f32(verts.detach())
    B, V = verts.shape[0], verts.shape[1]
    out = torch.empty(B, dtype=torch.float64, device=verts.device)
    fdev = torch.from_numpy(faces).to(verts.device)
    _lib.check(_lib.lib().hm_mesh_volume(_lib.ptr(verts), _lib.ptr(fdev), B, V, faces.shape[0], _lib.ptr(out), _lib.stream()),
               "hm_mesh_volume")
    return out


def solid_voxels(verts, faces, pitch, boxes, dims=None, out=None):
    """Solid voxelisation of B closed meshes on the world-anchored lattice of `pitch` (no grad; csrc/solidvox.hip, the rules in
    include/homan_amd.h): verts (B,V,3), faces (F,3), boxes (B,6) host integers {i0, j0, k0, nx, ny, nz} per frame, dims =
    (NWX, NY, NZ) launch-wide (default: the smallest that hold every box) -> words (B, NZ, NY, NWX) int32 holding the 32-bit
    patterns: bit t of word w in row (k, j) is voxel (i0 + 32w + t, j0 + j, k0 + k), centre ((float)i + 0.5f) * pitch.  out:
    a contiguous int32 device tensor of that shape to fill instead of a new one."""
    faces = _check_mesh(verts, faces)
    h = voxel_pitch(pitch)
    B, V = verts.shape[0], verts.shape[1]
    boxes = np.asarray(boxes)
    if boxes.shape != (B, 6) or boxes.dtype.kind not in "iu":
        raise ValueError(f"boxes: expected integers of shape ({B}, 6), got {boxes.dtype} {boxes.shape}")
    boxes = boxes.astype(np.int64)
    if (boxes[:, 3:] < 0).any():
        raise ValueError("boxes: negative extent")
    if (boxes[:, :3] < -VOXEL_MAX_INDEX).any() or (boxes[:, :3] + boxes[:, 3:] > VOXEL_MAX_INDEX).any():
        raise ValueError(f"boxes: voxel index beyond +-{VOXEL_MAX_INDEX}")
    need = (int(-(-boxes[:, 3].max() // 32)), int(boxes[:, 4].max()), int(boxes[:, 5].max()))
    nwx, ny, nz = need if dims is None else (int(d) for d in dims)
    if nwx < need[0] or ny < need[1] or nz < need[2]:
        raise ValueError(f"dims {(nwx, ny, nz)} do not hold the boxes, which need {need}")
    boxes = np.ascontiguousarray(boxes, dtype=np.int32)
    verts = _f32(verts.detach())
    dev = verts.device
    if out is not None and (out.dtype != torch.int32 or tuple(out.shape) != (B, nz, ny, nwx) or not out.is_contiguous()
                            or out.device != dev):
        raise ValueError(f"out: expected a contiguous int32 tensor of shape {(B, nz, ny, nwx)} on {dev}")
    words = torch.empty(B, nz, ny, nwx, dtype=torch.int32, device=dev) if out is None else out
    boxes_dev = torch.empty(B, 6, dtype=torch.int32, device=dev)
    fdev = torch.from_numpy(faces).to(dev)
    _lib.check(_lib.lib().hm_solid_voxels(_lib.ptr(verts), _lib.ptr(fdev), B, V, faces.shape[0], float(h), boxes.ctypes.data,
                                          nwx, ny, nz, _lib.ptr(boxes_dev), _lib.ptr(words) if words.numel() else None,
                                          _lib.stream()), "hm_solid_voxels")
    return words


def voxel_overlap(a, b):
    """Words of two voxelisations of one region -> (B,3) int64 {popcount(a & b), popcount(a), popcount(b)} per frame (no grad;
    csrc/solidvox.hip).  b (B, ...) int32; a of the same shape, or (S, B, ...): S voxelisations that are OR-ed first."""
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise ValueError(f"{name}: expected an int32 tensor of words, got {getattr(t, 'dtype', type(t))}")
    if b.dim() < 1 or b.shape[0] < 1:
        raise ValueError(f"b: expected (B, ...) with B >= 1, got {tuple(b.shape)}")
    if a.shape == b.shape:
        sets = 1
    elif a.dim() == b.dim() + 1 and a.shape[1:] == b.shape and a.shape[0] >= 1:
        sets = a.shape[0]
    else:
        raise ValueError(f"a {tuple(a.shape)} is neither b's shape {tuple(b.shape)} nor (S,) + it")
    a, b = a.detach().contiguous(), b.detach().contiguous()
    B = b.shape[0]
    counts = torch.empty(B, 3, dtype=torch.int64, device=b.device)
    per_frame = b.numel() // B
    _lib.check(_lib.lib().hm_voxel_overlap(_lib.ptr(a) if per_frame else None, sets, _lib.ptr(b) if per_frame else None, B,
                                           per_frame, _lib.ptr(counts), _lib.stream()), "hm_voxel_overlap")
    return counts


SURFDIST_CHUNK = 256             # faces staged through LDS per pass (SD_CHUNK of csrc/surfdist.hip)


def _point_mesh_inputs(points, verts, faces, who):
    """the argument checks shared by the point-against-mesh ops -> (device, points, verts, faces) as contiguous fp32 / int32"""
    for name, t in (("points", points), ("verts", verts)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"{name}: expected a float tensor, got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name}: expected a non-empty (B, N, 3) tensor, got {tuple(t.shape)}")
    if points.shape[0] != verts.shape[0]:
        raise ValueError(f"batch sizes differ: {points.shape[0]} vs {verts.shape[0]}")
    faces = faces.detach() if isinstance(faces, torch.Tensor) else torch.from_numpy(np.array(faces))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.is_floating_point() or faces.dtype == torch.bool:
        raise ValueError(f"faces: expected a non-empty integer (F, 3) array, got {faces.dtype} {tuple(faces.shape)}")
    if not torch.cuda.is_available():
        raise _lib.HomanAmdError(f"homan_amd.ops.{who} needs the GPU (there is no CPU fallback)")
    dev = next((t.device for t in (points, verts) if t.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    points = points.detach().to(device=dev, dtype=torch.float32).contiguous()
    verts = verts.detach().to(device=dev, dtype=torch.float32).contiguous()
    return dev, points, verts, faces.to(device=dev, dtype=torch.int32).contiguous()


def point_mesh_distance(points, verts, faces, closest=False):
    """Exact distance of points (B,N,3) to the triangle meshes verts (B,V,3), faces (F,3) - one topology for all frames - and
    the inside-outside sign (no grad; csrc/surfdist.hip, the rules in include/homan_amd.h) -> {"d2" (B,N) fp32 squared
    distance to the nearest face, "face" (B,N) int32 the lowest face that attains it, "inside" (B,N) int32 0 / 1: odd number of
    faces crossed by the +x ray (meaningful for a closed mesh)} and, with closest, {"closest" (B,N,3) fp32}.  A face that
    names a vertex outside [0, V) or has a non-finite coordinate is skipped; a non-finite point gets (+inf, -1, 0, 0).  The
    inputs are moved to the GPU as contiguous fp32 / int32; there is no CPU path.  `point_mesh_distance_signed` is this op with
    a choice of the sign's rule."""
    dev, points, verts, faces = _point_mesh_inputs(points, verts, faces, "point_mesh_distance")
    B, N, V, F = points.shape[0], points.shape[1], verts.shape[1], faces.shape[0]
    with torch.cuda.device(dev):
        out = {"d2": torch.empty(B, N, device=dev), "face": torch.empty(B, N, dtype=torch.int32, device=dev),
               "inside": torch.empty(B, N, dtype=torch.int32, device=dev)}
        if closest:
            out["closest"] = torch.empty(B, N, 3, device=dev)
        nbytes = _lib.lib().hm_point_mesh_workspace_bytes(B, N, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        _lib.check(_lib.lib().hm_point_mesh_distance(_lib.ptr(points), _lib.ptr(verts), _lib.ptr(faces), B, N, V, F,
                                                     _lib.ptr(out["d2"]), _lib.ptr(out["face"]), _lib.ptr(out["inside"]),
                                                     _lib.ptr(out.get("closest")), _lib.ptr(ws), _lib.stream()),
                   "hm_point_mesh_distance")
    return out


WINDING_LOG2Q_MIN = -47          # WN_LOG2Q_MIN of csrc/winding.hip


def winding_log2q(F):
    """The grid 2^L of the exact sum of hm_point_mesh_winding (include/homan_amd.h): L = max(-44, ceil(log2(F)) - 59).  Every
    solid angle is below 8 in magnitude, so F addends stay below 2^62 quanta of a signed 64-bit count."""
    if int(F) < 1:
        raise ValueError(f"winding_log2q: F {F}")
    return max(-44, (int(F) - 1).bit_length() - 59)


def _winding_run(points, verts, faces, log2q):
    """one hm_point_mesh_winding -> (count (B,N) int64, inside (B,N) int32, log2q), new tensors"""
    L = None if log2q is None else int(log2q)
    dev, points, verts, faces = _point_mesh_inputs(points, verts, faces, "point_mesh_winding")
    B, N, V, F = points.shape[0], points.shape[1], verts.shape[1], faces.shape[0]
    L = winding_log2q(F) if L is None else L
    lowest = max(WINDING_LOG2Q_MIN, (F - 1).bit_length() - 59)
    if not lowest <= L <= 0:
        raise ValueError(f"log2q {L} outside [{lowest}, 0] for {F} faces")
    with torch.cuda.device(dev):
        count = torch.empty(B, N, dtype=torch.int64, device=dev)
        inside = torch.empty(B, N, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().hm_point_mesh_winding(_lib.ptr(points), _lib.ptr(verts), _lib.ptr(faces), B, N, V, F, L,
                                                    _lib.ptr(count), _lib.ptr(inside), _lib.stream()), "hm_point_mesh_winding")
    return count, inside, L


def point_mesh_winding(points, verts, faces, log2q=None):
    """Generalised winding number of points (B,N,3) against the triangle meshes verts (B,V,3), faces (F,3): the inside-outside
    sign for meshes that need not be closed (no grad; csrc/winding.hip, the rules in include/homan_amd.h) -> {"count" (B,N)
    int64 the signed solid angle of all faces in quanta of 2^log2q, summed exactly, "winding" (B,N) float64 = count * 2^log2q /
    (4 pi), "inside" (B,N) int32 0 / 1: |winding| > 0.5, decided on the integers, "log2q"}.  log2q None = winding_log2q(F).
    Skipped faces as `point_mesh_distance`, and faces of zero area; a non-finite point gets (0, 0).  For a point exactly on the
    surface the values are deterministic but not meaningful.  Inputs are checked and moved as by `point_mesh_distance`; nothing
    synchronises with the host; there is no CPU path."""
    import math
    count, inside, L = _winding_run(points, verts, faces, log2q)
    with torch.cuda.device(count.device):
        # (a true division: by a Python scalar torch multiplies with the reciprocal, which rounds differently)
        winding = (count.double() * math.ldexp(1.0, L)) / torch.full((), 4.0 * math.pi, dtype=torch.float64, device=count.device)
    return {"count": count, "winding": winding, "inside": inside, "log2q": L}


def point_mesh_distance_signed(points, verts, faces, closest=False, sign="parity"):
    """`point_mesh_distance` with a choice of the inside-outside rule.  sign="parity": that op, its keys and bits.
    sign="winding": d2, face and closest are the search's bits unchanged, "inside" is `point_mesh_winding`'s (|w| > 0.5: meaningful
    for open meshes too), and a key "winding" (B,N) float64 is added.  sign="auto": parity where `meshutils.mesh_topology` finds
    the faces closed, else winding.  Any other string is a ValueError."""
    from . import meshutils
    rule = meshutils.resolve_sign(sign, faces)
    out = point_mesh_distance(points, verts, faces, closest=closest)
    if rule == "winding":
        w = point_mesh_winding(points, verts, faces)
        out["inside"], out["winding"] = w["inside"], w["winding"]
    return out


# =============================================================================== surface contact loss
def surface_contact_log2q(N, weight_max=1.0, contact_thresh=0.010, collision_thresh=0.020):
    """The grid 2^L of the exact sums of hm_surface_contact_fwd (include/homan_amd.h): L = ceil(log2(N M)) - 50 with
    M = max(weight_max, 1) * max(contact_thresh, collision_thresh, 1), which bounds every addend: N addends of one frame - all
    the points on one face is a legal input - stay below 2^51 quanta.  N = 778 at unit weights gives -40."""
    import math
    M = max(float(weight_max), 1.0) * max(float(contact_thresh), float(collision_thresh), 1.0)
    if not (N >= 1 and math.isfinite(M)):
        raise ValueError(f"surface_contact_log2q: N {N}, bound {M}")
    return math.ceil(math.log2(N * M)) - 50


def _check_surface_thresholds(contact_thresh, collision_thresh):
    for name, c in (("contact_thresh", contact_thresh), ("collision_thresh", collision_thresh)):
        with np.errstate(over="ignore"):
            c32 = np.float32(c)
        if not (np.isfinite(c32) and c32 > 0):
            raise ValueError(f"{name} must be positive and finite in fp32, got {c}")
    return float(contact_thresh), float(collision_thresh)


class SurfaceContactContext:
    """Workspace and static unit-gradient buffers of `surface_contact_loss` for points (B,N,3) against meshes (B,V,3) of the
    topology faces (F,3) (host array or tensor of integers in [0, V)).  A context serves one forward at a time: the backward
    of a forward reads the context's buffers, so it has to run before the context's next forward (one context per call site)."""

    def __init__(self, B, N, V, faces, device):
        B, N, V = int(B), int(N), int(V)
        if B < 1 or N < 1 or V < 1:
            raise ValueError(f"SurfaceContactContext: B, N, V must be positive, got {(B, N, V)}")
        faces = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces)
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.dtype.kind not in "iu":
            raise ValueError(f"faces: expected a non-empty integer (F, 3) array, got {faces.dtype} {faces.shape}")
        if not torch.cuda.is_available():
            raise _lib.HomanAmdError("homan_amd.ops.SurfaceContactContext needs the GPU (there is no CPU fallback)")
        dev = torch.device(device)
        self.B, self.N, self.V, self.F, self.device = B, N, V, int(faces.shape[0]), dev
        self.faces = torch.from_numpy(np.array(faces, dtype=np.int32)).to(dev)             # (a writable, contiguous copy)
        self.ws = torch.zeros(_lib.lib().hm_surface_contact_workspace_bytes(B, N, V, self.F), dtype=torch.uint8, device=dev)
        self.grad_points = torch.zeros(B, N, 3, device=dev)
        self.inside = torch.zeros(B, N, dtype=torch.int32, device=dev)
        self.grad_verts_attr = torch.zeros(B, V, 3, device=dev)
        self.grad_verts_rep = torch.zeros(B, V, 3, device=dev)
        self._weights = (None, None, 1.0)              # (key of the caller's tensor, fp32 device copy, its maximum)
        self.calls = 0                                 # forwards run on these buffers

    def weights(self, weights, weight_max=None):
        """the caller's per-point weights as (fp32 device tensor or None, maximum).  The maximum is read on the host once per
        tensor (and version of it); pass `weight_max` to skip that read - it synchronises, which a stream capture forbids."""
        if weights is None:
            return None, 1.0
        if not isinstance(weights, torch.Tensor) or not weights.is_floating_point() or tuple(weights.shape) != (self.N,):
            raise ValueError(f"weights: expected a float tensor of shape ({self.N},), got "
                             f"{getattr(weights, 'dtype', type(weights))} {tuple(getattr(weights, 'shape', ()))}")
        key = (weights.data_ptr(), weights._version, weights.device, weight_max)
        if self._weights[0] != key:
            w = weights.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if weight_max is None:
                lo, hi = float(w.min()), float(w.max())
                if not (lo >= 0 and np.isfinite(hi)):
                    raise ValueError(f"weights must be finite and >= 0, got [{lo}, {hi}]")
                weight_max = hi
            self._weights = (key, w, float(weight_max))
        return self._weights[1], self._weights[2]


def _check_surface_inputs(points, verts, sctx):
    if not isinstance(sctx, SurfaceContactContext):
        raise ValueError(f"ctx: expected a SurfaceContactContext, got {type(sctx)}")
    for name, t, n in (("points", points, sctx.N), ("verts", verts, sctx.V)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"{name}: expected a float tensor, got {getattr(t, 'dtype', type(t))}")
        if tuple(t.shape) != (sctx.B, n, 3):
            raise ValueError(f"{name}: expected {(sctx.B, n, 3)} (the context's sizes), got {tuple(t.shape)}")


def _surface_contact_run(points, verts, sctx, wdev, c_a, c_r, log2q, detail=None):
    """one hm_surface_contact_fwd on the context's buffers -> out (2,) = (A, R), a new tensor"""
    out = torch.empty(2, device=sctx.device)
    d = detail or {}
    _lib.check(_lib.lib().hm_surface_contact_fwd(_lib.ptr(points), _lib.ptr(verts), _lib.ptr(sctx.faces), _lib.ptr(wdev), sctx.B,
                                                 sctx.N, sctx.V, sctx.F, c_a, c_r, log2q, _lib.ptr(out),
                                                 _lib.ptr(sctx.grad_points), _lib.ptr(sctx.inside),
                                                 _lib.ptr(sctx.grad_verts_attr), _lib.ptr(sctx.grad_verts_rep),
                                                 _lib.ptr(d.get("value")), _lib.ptr(d.get("bary")), _lib.ptr(d.get("d2")),
                                                 _lib.ptr(d.get("face")), _lib.ptr(sctx.ws), _lib.stream()),
               "hm_surface_contact_fwd")
    sctx.calls += 1                    # (whose unit gradients the buffers hold: the backward checks it)
    return out


class _SurfaceContactLoss(torch.autograd.Function):
    """hm_surface_contact_fwd / _bwd (csrc/surfcontact.hip): the forward leaves the unit gradients in the context, the backward
    scales them by the two upstreams."""

    @staticmethod
    def forward(ctx, points, verts, sctx, wdev, c_a, c_r, log2q):
        out = _surface_contact_run(_f32(points.detach()), _f32(verts.detach()), sctx, wdev, c_a, c_r, log2q)
        ctx.sctx, ctx.call = sctx, sctx.calls
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_attr, g_rep):
        s = ctx.sctx
        if ctx.call != s.calls:
            raise RuntimeError("surface_contact_loss: the context has run another forward since this one; its unit gradients are "
                               "gone (one SurfaceContactContext per call site, backward before the next forward)")
        want_p, want_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_p or want_v):
            return (None,) * 7
        up = torch.stack([_f32(g_attr).reshape(()), _f32(g_rep).reshape(())])
        gp = torch.empty_like(s.grad_points) if want_p else None
        gv = torch.empty_like(s.grad_verts_attr) if want_v else None
        _lib.check(_lib.lib().hm_surface_contact_bwd(_lib.ptr(s.grad_points), _lib.ptr(s.inside), _lib.ptr(s.grad_verts_attr),
                                                     _lib.ptr(s.grad_verts_rep), _lib.ptr(up), s.B * s.N, s.B * s.V,
                                                     _lib.ptr(gp), _lib.ptr(gv), _lib.stream()), "hm_surface_contact_bwd")
        return gp, gv, None, None, None, None, None


def surface_contact_loss(points, verts, ctx, weights=None, contact_thresh=0.010, collision_thresh=0.020, weight_max=None):
    """Surface contact loss (csrc/surfcontact.hip, the rules in include/homan_amd.h; beyond the reference): points (B,N,3)
    against the meshes verts (B,V,3) of ctx's topology -> (A, R), 0-d tensors: attraction = sum over the points OUTSIDE the
    mesh of w c_a tanh(d / c_a), repulsion = sum over the points INSIDE of c_r tanh(d / c_r), d the exact distance to the
    surface, both over B N.  weights (N,) fp32 >= 0 weigh the attraction only.  Both `points` and `verts` receive gradients
    (through the closest point, envelope theorem); results are the same bits from run to run and at any batch position."""
    _check_surface_inputs(points, verts, ctx)
    c_a, c_r = _check_surface_thresholds(contact_thresh, collision_thresh)
    wdev, wmax = ctx.weights(weights, weight_max)
    return _SurfaceContactLoss.apply(points, verts, ctx, wdev, c_a, c_r, surface_contact_log2q(ctx.N, wmax, c_a, c_r))


def surface_contact_terms(points, verts, ctx, weights=None, contact_thresh=0.010, collision_thresh=0.020, weight_max=None):
    """The per-point detail of `surface_contact_loss`, no gradient -> {"value" (B,N) the point's term u, "bary" (B,N,3) the
    barycentric weights of its closest point on "face" (B,N) int32, "d2" (B,N), "inside" (B,N) int32, and the call's results
    "loss" (2,) = (A, R), "grad_points" (B,N,3), "grad_verts_attr", "grad_verts_rep" (B,V,3) at unit upstream}, new tensors."""
    _check_surface_inputs(points, verts, ctx)
    c_a, c_r = _check_surface_thresholds(contact_thresh, collision_thresh)
    wdev, wmax = ctx.weights(weights, weight_max)
    dev, B, N = ctx.device, ctx.B, ctx.N
    with torch.no_grad():
        detail = {"value": torch.empty(B, N, device=dev), "bary": torch.empty(B, N, 3, device=dev),
                  "d2": torch.empty(B, N, device=dev), "face": torch.empty(B, N, dtype=torch.int32, device=dev)}
        points = points.detach().to(device=dev, dtype=torch.float32).contiguous()
        verts = verts.detach().to(device=dev, dtype=torch.float32).contiguous()
        out = _surface_contact_run(points, verts, ctx, wdev, c_a, c_r, surface_contact_log2q(N, wmax, c_a, c_r), detail)
        detail.update(inside=ctx.inside.clone(), loss=out, grad_points=ctx.grad_points.clone(),
                      grad_verts_attr=ctx.grad_verts_attr.clone(), grad_verts_rep=ctx.grad_verts_rep.clone())
    return detail


# =============================================================================== mesh preparation (csrc/remesh.hip)
LATTICE_OFFSET = np.float32(1.381966)        # cells between the lattice's origin and the box's lower corner
LATTICE_RESOLUTIONS = (2, 256)               # admitted cells along the longest extent
LATTICE_MAX_AXIS = 512                       # RM_MAX_AXIS of csrc/remesh.hip
LATTICE_WORD, LATTICE_SCAN_TILE = 64, 2048   # corners per word of the packed field (= the emit kernels' row tile); rows per scan tile
_LATTICE_REPORT_INTS = 73


def _lattice_mesh(verts, faces):
    """one mesh as host arrays -> (verts (V,3) fp32, faces (F,3) int64), checked"""
    v = verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else np.asarray(verts)
    if v.dtype.kind != "f" or v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError(f"verts: expected a non-empty float (V, 3) array, got {v.dtype} {v.shape}")
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in "iu":
        raise ValueError(f"faces: expected a non-empty integer (F, 3) array, got {f.dtype} {f.shape}")
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int64)


def lattice_box(verts, faces, resolution):
    """The lattice of include/homan_amd.h for a source mesh, on the host -> (origin (3,) fp32, pitch fp32, dims (nx, ny, nz)
    corners): h = max(hi - lo) / (float)R over the box of the vertices named by a face the search does not skip, origin =
    lo - 1.381966f * h, floor((hi - lo) / h) + 5 corners per axis.  ValueError for R outside [2, 256], no valid face, a box
    whose longest extent is not positive and finite."""
    v, f = _lattice_mesh(verts, faces)
    R = int(resolution)
    if R != resolution or not LATTICE_RESOLUTIONS[0] <= R <= LATTICE_RESOLUTIONS[1]:
        raise ValueError(f"resolution {resolution!r} not an integer in [{LATTICE_RESOLUTIONS[0]}, {LATTICE_RESOLUTIONS[1]}]")
    in_range = ((f >= 0) & (f < len(v))).all(1)
    ok = in_range & np.isfinite(v[np.where(in_range[:, None], f, 0)]).all((1, 2))
    if not ok.any():
        raise ValueError("the mesh has no face with in-range, finite vertices")
    used = v[np.unique(f[ok])]
    lo, hi = used.min(0), used.max(0)
    with np.errstate(over="ignore", invalid="ignore"):
        ext = hi - lo
        h = np.float32(ext.max()) / np.float32(R)
        if not (np.isfinite(h) and h > 0):
            raise ValueError(f"degenerate bounding box: extents {ext.tolist()}")
        origin = lo - LATTICE_OFFSET * h
        dims = tuple(int(n) + 5 for n in np.floor(ext / h))
    if not np.isfinite(origin).all():
        raise ValueError("the lattice's origin is not finite")
    return origin, h, dims


def _lattice_args(origin, pitch):
    o = np.asarray(origin, dtype=np.float64).reshape(-1)
    with np.errstate(over="ignore"):
        o32, h = o.astype(np.float32), np.float32(pitch)
    if o.shape != (3,) or not np.isfinite(o32).all():
        raise ValueError(f"origin: expected three finite numbers, got {origin!r}")
    if not (np.isfinite(h) and h > 0):
        raise ValueError(f"pitch {pitch!r} is not positive and finite in fp32")
    return o32, h


def lattice_signs(verts, faces, resolution, sign="winding"):
    """The sign lattice of a source mesh (csrc/remesh.hip, csrc/winding.hip; the rules in include/homan_amd.h): verts (V,3),
    faces (F,3) of ONE mesh, `resolution` cells along its longest extent -> {"inside" (nz, ny, nx) int32 on the device: the flag
    of every corner by sign="winding" (|w| > 0.5: sources that need not be closed) or "parity" (closed sources), "origin" (3,)
    fp32 and "pitch" fp32 on the host, "dims" (nx, ny, nz), "corners" (nz ny nx, 3) fp32 the positions}.  The box is formed
    on the host (`lattice_box`); the search is brute force over every corner.  No grad, no CPU path."""
    if sign not in ("winding", "parity"):
        raise ValueError(f"sign {sign!r} not in [winding|parity]")
    v, f = _lattice_mesh(verts, faces)
    origin, h, (nx, ny, nz) = lattice_box(v, f, resolution)
    if not torch.cuda.is_available():
        raise _lib.HomanAmdError("homan_amd.ops.lattice_signs needs the GPU (there is no CPU fallback)")
    dev = verts.device if isinstance(verts, torch.Tensor) and verts.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        pts = torch.empty(nz * ny * nx, 3, device=dev)
        _lib.check(_lib.lib().hm_lattice_corners(nx, ny, nz, float(origin[0]), float(origin[1]), float(origin[2]), float(h),
                                                 _lib.ptr(pts), _lib.stream()), "hm_lattice_corners")
        vt = torch.from_numpy(v).to(dev)[None]
        if sign == "winding":
            inside = _winding_run(pts[None], vt, f, None)[1]
        else:
            inside = point_mesh_distance(pts[None], vt, f)["inside"]
    return {"inside": inside.view(nz, ny, nx), "origin": origin, "pitch": h, "dims": (nx, ny, nz), "corners": pts}


def _lattice_field(inside, who):
    """the argument checks shared by the sign-field ops -> (the field as a tensor, (nx, ny, nz))"""
    t = inside if isinstance(inside, torch.Tensor) else torch.from_numpy(np.array(inside))
    if t.dim() != 3 or t.is_floating_point() or t.is_complex():
        raise ValueError(f"inside: expected (nz, ny, nx) integers or booleans, got {t.dtype} {tuple(t.shape)}")
    nz, ny, nx = (int(n) for n in t.shape)
    if min(nx, ny, nz) < 2 or max(nx, ny, nz) > LATTICE_MAX_AXIS:
        raise ValueError(f"inside: every axis must have 2 ... {LATTICE_MAX_AXIS} corners, got {(nz, ny, nx)}")
    return t, (nx, ny, nz)


def _surface_nets_counted(t, dims, who):
    """hm_lattice_repair and hm_surface_nets_count on a checked field, and the ONE host read -> (the device buffers for
    hm_surface_nets_emit, host = [passes, corners, status, ..., cells, x-, y-, z-edges])"""
    if not torch.cuda.is_available():
        raise _lib.HomanAmdError(f"homan_amd.ops.{who} needs the GPU (there is no CPU fallback)")
    nx, ny, nz = dims
    dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    handle = _lib.lib()
    with torch.cuda.device(dev):
        flags = (t.detach() != 0).to(device=dev, dtype=torch.int32).contiguous()
        words = handle.hm_lattice_words(nx, ny, nz)
        bits = torch.empty(2 * words, dtype=torch.int64, device=dev)
        cell_bits = torch.empty(words, dtype=torch.int64, device=dev)
        offsets = torch.empty(4 * ny * nz, dtype=torch.int32, device=dev)
        report = torch.empty(_LATTICE_REPORT_INTS + 4, dtype=torch.int32, device=dev)
        totals = report[_LATTICE_REPORT_INTS:]
        _lib.check(handle.hm_lattice_repair(_lib.ptr(flags), nx, ny, nz, _lib.ptr(bits), _lib.ptr(report), _lib.stream()),
                   "hm_lattice_repair")
        _lib.check(handle.hm_surface_nets_count(_lib.ptr(bits), nx, ny, nz, _lib.ptr(cell_bits), _lib.ptr(offsets),
                                                _lib.ptr(totals), _lib.stream()), "hm_surface_nets_count")
        host = report.cpu().tolist()                                       # the one host read
    if host[2]:
        raise _lib.HomanAmdError(f"{who}: the checkerboard repair did not settle in 64 passes")
    return (dev, bits, cell_bits, offsets, totals), host


def surface_nets_count(inside):
    """The counts of `surface_nets` without its outputs (hm_lattice_repair + hm_surface_nets_count, one host read): what the
    budget search of `meshprep.make_watertight` probes with -> {"cells": vertices the field would give, "triangles",
    "repair_passes", "repaired_corners"}.  Arguments and errors as `surface_nets`."""
    t, dims = _lattice_field(inside, "surface_nets_count")
    _, host = _surface_nets_counted(t, dims, "surface_nets_count")
    return {"cells": host[-4], "triangles": 2 * sum(host[-3:]), "repair_passes": host[0], "repaired_corners": host[1]}


def surface_nets(inside, origin, pitch):
    """Surface nets on a lattice of signs (csrc/remesh.hip, the rules in include/homan_amd.h): inside (nz, ny, nx) integers or
    booleans, non-zero = inside (tensor or array; the outermost layer is forced outside), corner (i, j, k) at origin +
    (float)index * pitch -> {"vertices" (V,3) fp32, "faces" (T,3) int32 on the device: closed, oriented, normals outward,
    "repair_passes", "repaired_corners": the checkerboard repair's counts, "cells" = V}.  The output is a function of the field
    alone, the same bits on every call.  ONE host read (the repair's report and the counts) sizes the outputs.  No grad, no CPU
    path; a field the repair cannot settle in 64 passes raises HomanAmdError."""
    t, (nx, ny, nz) = _lattice_field(inside, "surface_nets")
    o, h = _lattice_args(origin, pitch)
    (dev, bits, cell_bits, offsets, totals), host = _surface_nets_counted(t, (nx, ny, nz), "surface_nets")
    n_vertices, n_faces = host[-4], 2 * sum(host[-3:])
    with torch.cuda.device(dev):
        vertices = torch.empty(n_vertices, 3, device=dev)
        faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().hm_surface_nets_emit(_lib.ptr(bits), _lib.ptr(cell_bits), _lib.ptr(offsets), _lib.ptr(totals), nx,
                                                   ny, nz, float(o[0]), float(o[1]), float(o[2]), float(h), n_vertices, n_faces,
                                                   _lib.ptr(vertices) if n_vertices else None,
                                                   _lib.ptr(faces) if n_faces else None, _lib.stream()), "hm_surface_nets_emit")
    return {"vertices": vertices, "faces": faces, "repair_passes": host[0], "repaired_corners": host[1], "cells": n_vertices}


def lattice_snap(lattice_vertices, closest, d2, pitch, snap_limit):
    """The snap of include/homan_amd.h: per vertex `closest` iff d2 <= (snap_limit * snap_limit) * (pitch * pitch) in fp32, else
    its lattice position -> (vertices (n,3) fp32, snapped (n,) int32); device tensors in, new device tensors out."""
    _, h = _lattice_args((0.0, 0.0, 0.0), pitch)
    with np.errstate(over="ignore"):
        sl = np.float32(snap_limit)
    if not (np.isfinite(sl) and sl > 0):
        raise ValueError(f"snap_limit {snap_limit!r} is not positive and finite in fp32")
    n = lattice_vertices.shape[0] if isinstance(lattice_vertices, torch.Tensor) and lattice_vertices.dim() == 2 else -1
    for name, x, shape in (("lattice_vertices", lattice_vertices, (n, 3)), ("closest", closest, (n, 3)), ("d2", d2, (n,))):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or tuple(x.shape) != shape or n < 0:
            raise ValueError(f"{name}: expected an fp32 tensor of shape {shape}, got {getattr(x, 'dtype', type(x))} "
                             f"{tuple(getattr(x, 'shape', ()))}")
    if not lattice_vertices.is_cuda:
        raise _lib.HomanAmdError("homan_amd.ops.lattice_snap needs device tensors (there is no CPU fallback)")
    dev = lattice_vertices.device
    with torch.cuda.device(dev):
        out = torch.empty(n, 3, device=dev)
        snapped = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            _lib.check(_lib.lib().hm_lattice_snap(_lib.ptr(lattice_vertices.contiguous()), _lib.ptr(closest.contiguous()),
                                                  _lib.ptr(d2.contiguous()), n, float(sl), float(h), _lib.ptr(out),
                                                  _lib.ptr(snapped), _lib.stream()), "hm_lattice_snap")
    return out, snapped


# =============================================================================== edge-collapse decimation (csrc/decimate.hip)
DECIMATE_MAX_VERTS, DECIMATE_MAX_FACES = 1 << 20, 1 << 22     # DC_MAX_VERTS, DC_MAX_FACES of csrc/decimate.hip
DECIMATE_RANK_NONE = 2 ** 31 - 1                              # the rank of an invalid edge
DECIMATE_REGULARITY, DECIMATE_MAX_ROUNDS = 0.01, 4096


def closed_mesh(verts, faces):
    """The input contract of the decimation (include/homan_amd.h), checked on the host -> (verts (n,3) fp32, faces (m,3) int64) as
    NumPy arrays.  ValueError unless: closed and oriented (`meshutils.mesh_topology`), no face repeats a vertex, every index in
    range, every coordinate of a vertex that a face names finite, 4 <= n <= 2^20, 4 <= m <= 2^22.  Vertices that no face names
    (raw scans carry them) are DROPPED here, the others keep their order and the faces are renumbered: the rounds' contract is
    that every vertex is named."""
    from . import meshutils
    v, f = _lattice_mesh(verts, faces)
    if f.min() < 0 or f.max() >= len(v):
        raise ValueError(f"faces: an index outside [0, {len(v)})")
    used = np.unique(f)
    if len(used) != len(v):
        v, f = np.ascontiguousarray(v[used]), np.searchsorted(used, f)
    n, m = len(v), len(f)
    if not (4 <= n <= DECIMATE_MAX_VERTS and 4 <= m <= DECIMATE_MAX_FACES):
        raise ValueError(f"a closed mesh of 4 ... 2^20 vertices and 4 ... 2^22 faces is expected, got {n} and {m}")
    if not np.isfinite(v).all():
        raise ValueError("verts: a coordinate is not finite")
    if (f[:, 0] == f[:, 1]).any() or (f[:, 1] == f[:, 2]).any() or (f[:, 2] == f[:, 0]).any():
        raise ValueError("faces: a face repeats a vertex")
    topology = meshutils.mesh_topology(f)
    if not (topology["closed"] and topology["oriented"]):
        raise ValueError(f"the mesh is not closed and oriented: {topology}")
    return v, f


def _decimate_numbers(target, regularity, max_rounds):
    for name, x in (("target_vertices", target), ("max_rounds", max_rounds)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
            raise ValueError(f"{name} {x!r} is not a positive integer")
    with np.errstate(over="ignore"):
        reg = np.float32(regularity) if isinstance(regularity, (int, float, np.floating, np.integer)) and not isinstance(
            regularity, bool) else np.float32(np.nan)
    if not (np.isfinite(reg) and reg >= 0):
        raise ValueError(f"regularity {regularity!r} is not finite and >= 0 in fp32")
    return int(target), float(reg), int(max_rounds)


class _Decimator:
    """Every buffer of the rounds, sized once from the input (n0 vertices, m0 faces): the library's outputs and the outputs of
    the sorts, scans and gathers between its entry points, which are torch's (plumbing) and write into these buffers (`out=`).
    `round` issues one round's launches and makes its one host read.  What torch's sorts and scans need as temporaries of their
    own comes from its caching allocator."""

    def __init__(self, n0, m0, dev):
        E0, C0 = 3 * m0 // 2, 3 * m0
        i32 = dict(dtype=torch.int32, device=dev)
        self.corner_words = torch.empty(5, C0, dtype=torch.int64, device=dev)     # he, ck, both sorted, the sorts' indices
        self.edge_words = torch.empty(7, E0, dtype=torch.int64, device=dev)       # keys, orders and what the rank's sorts write
        self.doubles = torch.empty(10 * n0 + 2 * E0, dtype=torch.float64, device=dev)
        self.voff, self.corner_ints = torch.empty(n0 + 1, **i32), torch.empty(2, C0, **i32)
        self.edges, self.per_edge = torch.empty(E0, 4, **i32), torch.empty(6, E0, **i32)
        self.per_vertex, self.per_face = torch.empty(6, n0, **i32), torch.empty(2, m0, **i32)
        self.verts = [torch.empty(n0, 3, device=dev) for _ in range(2)]
        self.faces = [torch.empty(m0, 3, **i32) for _ in range(2)]
        self.n0, self.m0 = n0, m0

    def round(self, V, F, n, m, need, reg, out_v, out_f):
        """V (>= n, 3), F (>= m, 3) contiguous device buffers -> (new n, new m, the round's intermediates as views)"""
        h, p, s = _lib.lib(), _lib.ptr, _lib.stream()
        E, C = 3 * m // 2, 3 * m
        E0 = 3 * self.m0 // 2
        he, ck, he_sorted, corner_sorted, corner_idx = (self.corner_words[k, :C] for k in range(5))
        cost_keys, l2_keys, by_l2, keys_by_l2, sorted_keys, by_cost, order = (self.edge_words[k, :E] for k in range(7))
        quadrics = self.doubles[:10 * n]
        cost, l2 = self.doubles[10 * self.n0:10 * self.n0 + E], self.doubles[10 * self.n0 + E0:10 * self.n0 + E0 + E]
        voff, edges = self.voff[:n + 1], self.edges[:E]
        is_edge, edge_scan = self.corner_ints[0, :C], self.corner_ints[1, :C]
        choice, valid, rank, selected, by_rank, selected_scan = (self.per_edge[k, :E] for k in range(6))
        m1, m2, remap, vkeep, moved, vertex_scan = (self.per_vertex[k, :n] for k in range(6))
        fkeep, face_scan = self.per_face[0, :m], self.per_face[1, :m]
        _lib.check(h.hm_decimate_keys(p(F), n, m, p(he), p(ck), s), "hm_decimate_keys")
        torch.sort(he, out=(he_sorted, corner_idx))
        torch.sort(ck, out=(corner_sorted, corner_idx))
        _lib.check(h.hm_decimate_offsets(p(he_sorted), n, m, p(voff), p(is_edge), s), "hm_decimate_offsets")
        torch.cumsum(is_edge, 0, dtype=torch.int32, out=edge_scan)
        _lib.check(h.hm_decimate_costs(p(V), p(F), p(he_sorted), p(corner_sorted), p(voff), p(edge_scan), n, m, reg, p(quadrics),
                                       p(edges), p(choice), p(cost), p(l2), p(valid), p(cost_keys), p(l2_keys), s),
                   "hm_decimate_costs")
        torch.sort(l2_keys, stable=True, out=(sorted_keys, by_l2))
        torch.index_select(cost_keys, 0, by_l2, out=keys_by_l2)
        torch.sort(keys_by_l2, stable=True, out=(sorted_keys, by_cost))
        torch.index_select(by_l2, 0, by_cost, out=order)
        _lib.check(h.hm_decimate_select(p(edges), p(valid), p(order), p(he_sorted), p(voff), n, m, p(rank), p(m1), p(m2),
                                        p(selected), p(by_rank), p(remap), p(vkeep), p(moved), s), "hm_decimate_select")
        torch.cumsum(by_rank, 0, dtype=torch.int32, out=selected_scan)
        _lib.check(h.hm_decimate_mark(p(F), p(edges), p(rank), p(selected_scan), need, n, m, p(selected), p(remap), p(vkeep),
                                      p(moved), p(fkeep), s), "hm_decimate_mark")
        torch.cumsum(vkeep, 0, dtype=torch.int32, out=vertex_scan)
        torch.cumsum(fkeep, 0, dtype=torch.int32, out=face_scan)
        _lib.check(h.hm_decimate_compact(p(V), p(F), p(edges), p(choice), p(remap), p(moved), p(vkeep), p(vertex_scan), p(fkeep),
                                         p(face_scan), n, m, n, m, p(out_v), p(out_f), s), "hm_decimate_compact")
        new_n = int(vertex_scan[-1])                                       # the round's one host read
        # two faces go with every collapse (rule 5's link condition); `collapse_round` checks the face scan against it
        return new_n, m - 2 * (n - new_n), {"edges": edges, "choice": choice, "cost": cost, "l2": l2, "valid": valid, "rank": rank,
                                            "selected": selected, "vertex_keep": vkeep, "remap": remap, "moved": moved,
                                            "vertex_scan": vertex_scan, "face_keep": fkeep, "face_scan": face_scan}


def _decimate_start(verts, faces, who):
    v, f = closed_mesh(verts, faces)
    if not torch.cuda.is_available():
        raise _lib.HomanAmdError(f"homan_amd.ops.{who} needs the GPU (there is no CPU fallback)")
    dev = verts.device if isinstance(verts, torch.Tensor) and verts.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return v, f, dev


def collapse_round(verts, faces, need, regularity=DECIMATE_REGULARITY):
    """ONE round of the decimation (csrc/decimate.hip, the rules in include/homan_amd.h): verts (n,3), faces (m,3) of a closed,
    oriented mesh (checked on the host: `closed_mesh`), `need` = the most collapses wanted -> {"vertices" (n',3) fp32, "faces"
    (m',3) int32 after the round, on the device; the round's intermediates per edge in ascending (a, b): "edges" (E,4) a b c d,
    "choice" 0 / 1 / 2, "cost", "l2" fp64, "valid", "rank" (2^31 - 1 for an invalid edge), "selected" (after the budget);
    "collapses"}.  No grad, no CPU path."""
    if isinstance(need, bool) or not isinstance(need, (int, np.integer)) or need < 0:
        raise ValueError(f"need {need!r} is not an integer >= 0")
    _, reg, _ = _decimate_numbers(1, regularity, 1)
    v, f, dev = _decimate_start(verts, faces, "collapse_round")
    n, m = len(v), len(f)
    with torch.cuda.device(dev):
        work = _Decimator(n, m, dev)
        work.verts[0].copy_(torch.tensor(v))
        work.faces[0].copy_(torch.from_numpy(f.astype(np.int32)))
        new_n, new_m, mid = work.round(work.verts[0], work.faces[0], n, m, int(need), reg, work.verts[1], work.faces[1])
        kept_faces = int(mid["face_scan"][-1])                             # (a second host read: this entry is the tests')
    if kept_faces != new_m:
        raise _lib.HomanAmdError(f"collapse_round: {n - new_n} collapses dropped {m - kept_faces} faces, not two each")
    out = {k: t.clone() for k, t in mid.items()}
    out.update(vertices=work.verts[1][:new_n].clone(), faces=work.faces[1][:new_m].clone(), collapses=n - new_n)
    return out


def decimate_mesh(verts, faces, target, regularity=DECIMATE_REGULARITY, max_rounds=DECIMATE_MAX_ROUNDS):
    """The decimation loop: rounds of `collapse_round` with need = n - target until n <= target, a round collapses nothing
    (stuck), or max_rounds -> {"vertices" (n,3) fp32, "faces" (m,3) int32 on the device, "rounds", "reached" (n <= target),
    "collapses" per round}.  Buffers are sized once from the input; a round makes ONE host read (its new vertex count).  The
    input is checked on the host first (`closed_mesh`); a mesh within the target comes back unchanged, rounds = 0.  The output is
    a function of the input alone.  No grad, no CPU path."""
    target, reg, max_rounds = _decimate_numbers(target, regularity, max_rounds)
    v, f, dev = _decimate_start(verts, faces, "decimate_mesh")
    n, m = len(v), len(f)
    collapses = []
    with torch.cuda.device(dev):
        work = _Decimator(n, m, dev)
        work.verts[0].copy_(torch.tensor(v))
        work.faces[0].copy_(torch.from_numpy(f.astype(np.int32)))
        at = 0
        while n > target and len(collapses) < max_rounds:
            new_n, m, _ = work.round(work.verts[at], work.faces[at], n, m, n - target, reg, work.verts[1 - at], work.faces[1 - at])
            collapses.append(n - new_n)
            n, at = new_n, 1 - at
            if collapses[-1] == 0:
                break
        vertices, out_faces = work.verts[at][:n].clone(), work.faces[at][:m].clone()
    return {"vertices": vertices, "faces": out_faces, "rounds": len(collapses), "reached": n <= target, "collapses": collapses}
