"""HOMan -- the hand-object model of the reference (reference homan/homan.py:26-508), MI355X-native.

Same constructor keywords, same Parameter / buffer names (so `named_parameters()` filtering by "mano" /
"rotation" in reference homan/jointopt.py:128-151 and `load_state_dict(strict=False)` of a reference
`joint_fit.pt` behave identically), same `forward(loss_weights) -> (loss_dict, metric_dict)`,
`get_verts_object()` and `get_verts_hand(detach_scale=False)`.  All arithmetic runs in the hand-written HIP kernels
of libhoman_amd.so through `homan_amd.ops`; there is no CPU path.

Visualisation (off the optimisation path, no gradients): `model.renderer` (homan_amd.nmr.Renderer with the reference's
light, homan.py:168-176), the combined scene topology / colour buffers (:177-219) and render / render_gt /
render_with_gt / render_limem / save_obj (:510-628) on the same rasteriser.  Not mirrored: assign_human_masks (:239-296,
never called by the reference).
"""
import numpy as np
import torch
from torch import nn

from . import constants, lossutils, nmr, ops, trans3d
from .depthprep import SensorDepth
from .losses import Losses
from .manomodel import ManoModel
from .meshutils import get_faces_and_textures


def combine_verts(verts_list):
    """reference homan/utils/geometry.py:43-47."""
    batch_size = verts_list[0].shape[0]
    return torch.cat([v.reshape(batch_size, -1, 3) for v in verts_list], 1)


def matrix_to_rot6d(rotmat):
    """reference homan/utils/geometry.py:30-40."""
    return rotmat.view(-1, 3, 3)[:, :, :2]


def weakcam_persp_trans(cams, K, image_size=640, reference_depth=1.0):
    """Camera-space translation (B,1,3) of the scaled-orthographic hand cameras `cams` = [s, tx, ty] (reference
    homan/utils/camera.py:85-97: the camera goes to pixel units of a 640-pixel image - `compute_transformation_ortho`'s default
    `image_size`, which HOMan.get_verts_hand does not override - and through `libyana.camutils.camconvs.
    batch_weakcam2persptrans(cams_px, K_px, 1)`).  libyana is not in /root/reference: the conversion is the first-order
    identity between the two camera models (u = s X + t  vs  u = f (X + T) / (Z + T_z) + c  =>  T_z = f / s,
    T_xy = (t - c) T_z / f_xy), restated from the model, not from its source (parity unpinned; oracle/yana.py states the
    same)."""
    persp_scale = cams[:, :1] / 2 * image_size
    persp_trans = (cams[:, 1:] + 1 / cams[:, :1]) * persp_scale
    fx, fy = K[:, 0, 0] * image_size, K[:, 1, 1] * image_size
    cx, cy = K[:, 0, 2] * image_size, K[:, 1, 2] * image_size
    tz = reference_depth * fx / persp_scale[:, 0]
    tx = (persp_trans[:, 0] - cx) * tz / fx
    ty = (persp_trans[:, 1] - cy) * tz / fy
    return torch.stack([tx, ty, tz.expand_as(tx)], 1).unsqueeze(1)


def clip_tensors(translations_object, rotations_object, verts_object_og, translations_hand, rotations_hand, verts_hand_og,
                 ref_verts2d_hand, mano_trans, mano_rot, mano_betas, mano_pca_pose, masks_object, masks_hand,
                 camintr_rois_object, camintr_rois_hand, target_masks_object, target_masks_hand, cams_hand=None, camintr=None,
                 int_scale_init=1.0, hand_proj_mode="persp", device=None, depth_maps=None, **_not_clip_data):
    """The data arguments of the constructor (reference homan/homan.py:27-60) -> ordered {name: tensor} of everything in a
    model that depends on the clip, in the form the model stores it (:62-166; in the constructor's registration order).  The ONE
    place where raw clip inputs are converted: HOMan.__init__ registers these, HOMan.load_clip copies them in place.  Raises
    the ortho refusals on the host input (forward may run inside a stream capture).  Without `device` nothing touches a
    device; with it, what is DERIVED (mask comparisons, constants) is formed there - the clip's own arrays stay where the
    caller has them, so that the consumer's copy is their one transfer.
    depth_maps (optional, a homan_amd extra: the observed-depth term): (B, S, S) sensor depth in METRES, in
    the camera of `camintr` and registered pixel for pixel with the instance masks, i.e. at THEIR resolution - raw sensor frames
    (another resolution, millimetres, uint16, a depth camera of its own) are brought to that grid by depthprep.prepare_depth_maps,
    or handed to HOMan / load_clip as a depthprep.SensorDepth, which they prepare with their own camintr before this function.
    NaN, infinite, zero, negative and out-of-range values mark pixels without a measurement.  Adds the buffer `depth_maps`."""
    f32 = lambda t: torch.as_tensor(t).detach().float()
    rot6d = lambda r: (matrix_to_rot6d(r) if r.shape[-1] == 3 else r).contiguous()
    const = lambda shape, value: torch.full(tuple(shape), float(value), device=device)
    if cams_hand is None:
        if hand_proj_mode == "ortho":
            raise ValueError("hand_proj_mode='ortho' needs cams_hand (scaled-orthographic [s, tx, ty] per hand, s != 0)")
        cams_hand = torch.zeros(translations_hand.shape[0], 3)
    elif hand_proj_mode == "ortho" and bool((f32(cams_hand).reshape(-1, 3)[:, 0] == 0).any()):
        raise ValueError("hand_proj_mode='ortho': cams_hand holds a zero scale (the translation is f / s)")
    tmo, tmh = (f32(t) if device is None else f32(t).to(device, non_blocking=True)
                for t in (target_masks_object, target_masks_hand))
    # (no intrinsics = the reference's default, homan.py:156-158 - for a clip loaded into a resident model too, NOT the previous
    #  clip's; one matrix serves every frame)
    camintr = f32([[[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]]] if camintr is None else camintr)
    camintr = camintr.unsqueeze(0) if camintr.dim() == 2 else camintr
    if camintr.shape[0] == 1:
        camintr = camintr.expand(translations_object.shape[0], 3, 3)
    masks_object = torch.as_tensor(masks_object).detach()
    out = dict(
        translations_object=f32(translations_object), rotations_object=rot6d(f32(rotations_object)),
        verts_object_og=f32(verts_object_og), translations_hand=f32(translations_hand),
        rotations_hand=rot6d(f32(rotations_hand)), cams_hand=f32(cams_hand), mano_pca_pose=f32(mano_pca_pose),
        mano_rot=f32(mano_rot), mano_trans=f32(mano_trans), mano_betas=const(f32(mano_betas).shape, 0),      # (betas start at zero, :108)
        int_scales_hand=const((1,), int_scale_init), verts_hand_og=f32(verts_hand_og), ref_verts2d_hand=f32(ref_verts2d_hand),
        # (reference :122 wraps the argument in torch.Tensor(...), which raises for its own float default 1.0 - callers pass the
        #  int 1, jointopt.py:118; any real number is accepted here)
        int_scales_object=const((1,), int_scale_init), int_scale_object_mean=const((1,), 1), int_scale_hand_mean=const((1,), 1),
        ref_mask_object=(tmo > 0).float(), keep_mask_object=(tmo >= 0).float(), ref_mask_hand=(tmh > 0).float(),
        keep_mask_hand=(tmh >= 0).float(), camintr_rois_object=f32(camintr_rois_object),
        camintr_rois_hand=f32(camintr_rois_hand), camintr=camintr.contiguous())
    if masks_hand is not None:
        out["masks_human"] = torch.as_tensor(masks_hand).detach()
    out["masks_object"] = masks_object.unsqueeze(0) if masks_object.dim() == 2 else masks_object
    if depth_maps is not None:
        depth_maps = f32(depth_maps)
        want = (translations_object.shape[0],) + tuple(out["masks_object"].shape[-2:])
        if tuple(depth_maps.shape) != want:
            raise ValueError(f"depth_maps of shape {tuple(depth_maps.shape)}: expected {want} (one map per frame, at the "
                             "instance masks' resolution)")
        out["depth_maps"] = depth_maps.contiguous()
    return out


class HOMan(nn.Module):
    def __init__(self, translations_object, rotations_object, verts_object_og, faces_object, translations_hand,
                 rotations_hand, verts_hand_og, ref_verts2d_hand, hand_sides, mano_trans, mano_rot, mano_betas,
                 mano_pca_pose, faces_hand, masks_object, masks_hand, camintr_rois_object, camintr_rois_hand,
                 target_masks_object, target_masks_hand, class_name, cams_hand=None, int_scale_init=1.0, camintr=None,
                 optimize_object_scale=False, optimize_ortho_cam=True, hand_proj_mode="persp", optimize_mano=True,
                 optimize_mano_beta=True, inter_type="centroid", image_size=640,
                 # homan_amd extensions (keyword-only use)
                 mano_model=None, mano_root="extra_data/mano", rend_size=constants.REND_SIZE, sync_metrics=True,
                 ordinal_depth=False, sil_mode="nmr", sil_sigma=1e-4, surface_contact_thresh=constants.CONTACT_THRESH,
                 surface_collision_thresh=constants.COLLISION_THRESH, surface_two_way=False, surface_contact_zones="all",
                 depth_maps=None, depth_obs_delta=0.03, depth_obs_layers="all"):
        # (host-side checks of the options first: no device is touched before they pass)
        if depth_obs_layers not in ("all", "object", "hand"):
            raise ValueError(f"depth_obs_layers {depth_obs_layers} not in [all|object|hand]")
        if not 0 < float(depth_obs_delta) <= 1:
            raise ValueError(f"depth_obs_delta {depth_obs_delta} must lie in (0, 1] (metres; the kernel's exact sums are sized for it)")
        if isinstance(depth_maps, SensorDepth):           # (raw sensor frames: registered below, against THIS model's camera)
            depth_maps.check(translations_object.shape[0], image_size)
        elif depth_maps is not None:
            want = (translations_object.shape[0], int(image_size), int(image_size))
            if tuple(torch.as_tensor(depth_maps).shape) != want:
                raise ValueError(f"depth_maps of shape {tuple(torch.as_tensor(depth_maps).shape)}: expected (B, image_size, "
                                 f"image_size) = {want}")
            if int(image_size) > 1024:
                # hm_depth_obs_fwd keeps a frame's pixel counts in 21-bit fields, like the ordinal depth term's kernel
                raise NotImplementedError(f"depth_maps: image_size {image_size} > 1024 (scale maps, masks and intrinsics down)")
        if surface_contact_zones not in ("all", "tips"):
            raise ValueError(f"surface_contact_zones {surface_contact_zones} not in [all|tips]")
        for name, c in (("surface_contact_thresh", surface_contact_thresh), ("surface_collision_thresh", surface_collision_thresh)):
            if not 0 < float(c) < float("inf"):
                raise ValueError(f"{name} {c} must be a positive number (metres)")
        if sil_mode not in ("nmr", "soft"):
            raise ValueError(f"sil_mode {sil_mode} not in [nmr|soft]")
        if not float(sil_sigma) > 0 or float(sil_sigma) == float("inf"):
            raise ValueError(f"sil_sigma {sil_sigma} must be a positive number (NDC^2)")
        super().__init__()
        if not torch.cuda.is_available():
            raise RuntimeError("homan_amd.HOMan needs an MI355X (ROCm) device; there is no CPU path")
        dev = torch.device("cuda")
        if isinstance(depth_maps, SensorDepth):
            depth_maps = depth_maps.prepare(camintr, int(image_size))
        self.hand_proj_mode = hand_proj_mode
        self.hand_sides = hand_sides
        self.hand_nb = len(hand_sides)
        for side in hand_sides:
            if side not in ("right", "left"):
                raise ValueError(f"{side} not in [left|right]")           # reference manomodel.py:141
        if self.hand_nb not in (1, 2):      # the reference's collision term de-interleaves with a stride of 2 (lossutils.py:58)
            raise NotImplementedError("one or two hands per frame; got %d" % self.hand_nb)
        self.optimize_mano, self.optimize_object_scale = optimize_mano, optimize_object_scale
        # everything clip-dependent, from the one preprocessing (clip_tensors); the options decide Parameter or buffer
        free = {"translations_object", "rotations_object", "translations_hand", "rotations_hand"}
        free |= {"cams_hand"} if optimize_ortho_cam else set()
        free |= {"mano_pca_pose", "mano_rot", "mano_trans"} if optimize_mano else set()
        free |= {"mano_betas"} if optimize_mano_beta else {"int_scales_hand"}
        free |= {"int_scales_object"} if optimize_object_scale else set()
        for name, t in clip_tensors(translations_object, rotations_object, verts_object_og, translations_hand, rotations_hand,
                                    verts_hand_og, ref_verts2d_hand, mano_trans, mano_rot, mano_betas, mano_pca_pose,
                                    masks_object, masks_hand, camintr_rois_object, camintr_rois_hand, target_masks_object,
                                    target_masks_hand, cams_hand, camintr, int_scale_init, hand_proj_mode,
                                    depth_maps=depth_maps).items():
            if name == "camintr":       # (the topology's place in the reference's registration order, homan.py:144-151)
                self.register_buffer("faces_object", faces_object.detach().clone())
                # white per-face textures of the single-mesh depth renders (state_dict keys)
                self.register_buffer("textures_object", torch.ones(faces_object.shape[0], faces_object.shape[1], 1, 1, 1, 3))
                self.register_buffer("textures_hand", torch.ones(faces_hand.shape[0], faces_hand.shape[1], 1, 1, 1, 3))
                self.register_buffer("faces_hand", faces_hand.detach().clone())
            t = torch.empty_like(t, device=dev).copy_(t)      # (the model's own storage, wherever the caller's tensor lives)
            if name in free:
                setattr(self, name, nn.Parameter(t, requires_grad=True))
            elif name != "mano_trans":   # reference homan.py:104-106: no mano_trans at all without optimize_mano
                self.register_buffer(name, t)
        batch = translations_object.shape[0]
        self.image_size = image_size
        self.cuda()

        # leaves: MANO layer (kept out of saved checkpoints by its "mano_model" prefix, fit_vid_dataset.py:366-371)
        self.mano_model = ManoModel(mano_root, pca_comps=16, mano_model=mano_model, device=dev)
        self.sync_metrics = sync_metrics
        self.reduce_ws = ops.ReduceWorkspace(dev)
        # sil_mode="soft" (a homan_amd extra, NOT the reference's image formation: DESIGN.md section 7): the object silhouette term
        # renders with the Soft Rasterizer op, whose gradient is a true derivative, all three coordinates included.  Its blur
        # `sil_sigma` (NDC^2) is a plain device tensor - no buffer, no Parameter: the state_dict keys stay the reference's - that
        # the kernels read when they run, so `model.sil_sigma.mul_(0.5)` between steps anneals it, captured graphs included.
        self.sil_mode = sil_mode
        self.sil_sigma = torch.full((1,), float(sil_sigma), dtype=torch.float32, device=dev)
        num_verts_object = self.verts_object_og.shape[1]
        self.losses = Losses(renderer=None, ref_mask_object=self.ref_mask_object,
                             keep_mask_object=self.keep_mask_object, ref_mask_hand=self.ref_mask_hand,
                             ref_verts2d_hand=self.ref_verts2d_hand, keep_mask_hand=self.keep_mask_hand,
                             camintr_rois_object=self.camintr_rois_object, camintr_rois_hand=self.camintr_rois_hand,
                             camintr=self.camintr, class_name=class_name, hand_nb=self.hand_nb, inter_type=inter_type,
                             faces_object=self.faces_object, num_verts_object=num_verts_object, rend_size=rend_size,
                             reduce_ws=self.reduce_ws, sync_metrics=sync_metrics, sil_mode=sil_mode,
                             sil_sigma=self.sil_sigma)
        closed = np.asarray(self.mano_model.closed_faces)
        if self.hand_nb == 1:
            self.collision_ctx = ops.CollisionContext(closed, self.faces_object[0], batch, 778, num_verts_object, dev)
        else:
            # scene [hand 0, hand 1, object], both hands with the closed topology in reversed winding (lossutils.py:53-59).
            # Every mesh's SDF depends on its own vertices only and the loss is a sum over ordered pairs of meshes
            # (scenesdf.py:131-146): three two-mesh launches give the same sum and the same gradients.
            rev = np.ascontiguousarray(closed[:, ::-1])
            rev_t = torch.as_tensor(rev.astype(np.int32))
            self.collision_ctx = (ops.CollisionContext(rev, rev_t, batch, 778, 778, dev),
                                  ops.CollisionContext(rev, self.faces_object[0], batch, 778, num_verts_object, dev),
                                  ops.CollisionContext(rev, self.faces_object[0], batch, 778, num_verts_object, dev))
        self._mano_cache = None
        # surface contact loss (a homan_amd extra): on when forward() is given lw_surf_attr / lw_surf_rep;
        # its contexts are built at the first forward that needs them (before any capture: GraphStepper's warm-up forwards)
        self.surface_contact_thresh, self.surface_collision_thresh = float(surface_contact_thresh), float(surface_collision_thresh)
        self.surface_two_way, self.surface_contact_zones = bool(surface_two_way), surface_contact_zones
        self._surf_ctxs = None
        # ordinal depth term: the reference's own call site cannot run (see forward()); `ordinal_depth=True` opts into the
        # loss the method describes (homan.py:384-419 + lossutils.py:133-169) instead of reproducing that TypeError
        self.ordinal_depth = bool(ordinal_depth)
        if self.ordinal_depth and int(image_size) > 1024:
            # hm_ordinal_depth_fwd packs a frame's three pixel counts into 21-bit fields of one 64-bit atomic: 1024^2 = 2^20
            # pixels per frame is its limit (the term is rendered at image_size, reference homan.py:168-172)
            raise NotImplementedError(f"ordinal depth term: image_size {image_size} > 1024 (rendered at image_size; scale the "
                                      "instance masks and intrinsics down, or leave ordinal_depth off)")
        self._depth_state = None
        # observed-depth term (a homan_amd extra): on when forward() is given lw_depth_obs > 0; needs the
        # buffer `depth_maps`.  delta = 0.03 m is an UNTUNED default.
        self.depth_obs_delta, self.depth_obs_layers = float(depth_obs_delta), depth_obs_layers
        self._depth_obs_scratch = None
        with torch.no_grad():
            self.verts_hand_init = self.get_verts_hand()[0].detach().clone()
            self.verts_object_init = self.get_verts_object()[0].detach().clone()
        self._setup_visualisation(batch)

    # ------------------------------------------------------------------ another clip into the same model
    def load_clip(self, faces_object=None, hand_sides=None, **clip):
        """The data arguments of the constructor (reference homan/homan.py:27-60) for ANOTHER clip of the same shapes, through
        the constructor's preprocessing (clip_tensors), copied IN PLACE into this model's Parameters and buffers: every context,
        workspace and captured graph built on them stays valid (a resident stepper fits a stream of clips without rebuilding
        anything, jointopt.ClipFitter).  Topologies and hand sides are the model's own (checked when given).  Every check comes
        before the first copy: a clip that is refused leaves the model as it was."""
        if hand_sides is not None and list(hand_sides) != list(self.hand_sides):
            raise ValueError("load_clip: other hand sides")
        if faces_object is not None and not torch.equal(torch.as_tensor(faces_object)[0].cpu(), self.faces_object[0].cpu()):
            raise ValueError("load_clip: other object topology")
        if isinstance(clip.get("depth_maps"), SensorDepth):
            clip["depth_maps"].check(torch.as_tensor(clip["translations_object"]).shape[0], self.image_size)
            clip = dict(clip, depth_maps=clip["depth_maps"].prepare(clip.get("camintr"), int(self.image_size)))
        new = clip_tensors(**dict(clip, hand_proj_mode=self.hand_proj_mode, device=self.translations_object.device))
        if hasattr(self, "depth_maps") and "depth_maps" not in new:
            raise ValueError("load_clip: the model was built with depth_maps; every later clip must bring depth_maps too")
        if "depth_maps" in new and not hasattr(self, "depth_maps"):
            raise ValueError("load_clip: the clip brings depth_maps, the model was built without (build it with depth_maps)")
        pairs = [(name, getattr(self, name), src) for name, src in new.items() if hasattr(self, name)]
        for name, dst, src in pairs:
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"load_clip: {name} of shape {tuple(src.shape)} does not fit the model's {tuple(dst.shape)}")
        with torch.no_grad():
            for name, dst, src in pairs:     # (the instance masks come in the caller's dtype and are converted on the way)
                dst.data.copy_(src, non_blocking=not name.startswith("masks_"))
            self._refresh_derived()

    def _refresh_derived(self):
        """Everything in the model that FOLLOWS its clip-dependent Parameters and buffers, brought up to them - the complete
        list (anything new that is computed from a clip's data and kept belongs here)."""
        self.losses.keep_sum.copy_(self.keep_mask_object.sum().reshape(1))
        self.losses.sil_ctx.invalidate_outputs()         # the raster's region state: outputs it skipped as unchanged
        if self._depth_state is not None:
            for dst, src in zip(self._depth_state[1], self._depth_masks()):
                dst.copy_(src)
        self._mano_cache = None
        self.verts_hand_init.copy_(self.get_verts_hand()[0].detach())
        self.verts_object_init.copy_(self.get_verts_object()[0].detach())
        self.renderer.K.copy_(self.camintr)

    # ------------------------------------------------------------------ visualisation (reference homan.py:168-219, 510-628)
    def _setup_visualisation(self, batch_size):
        """Renderer with the reference's light and the combined [object, hand...] scene meshes in prediction colours
        (gold / grey), ground-truth colours (green / blue) and both (:177-219).  Buffers are plain attributes, as in
        the reference (they are not part of the state_dict)."""
        self.renderer = nmr.Renderer(image_size=self.image_size, K=self.camintr.clone(), orig_size=1)
        self.renderer.light_direction = [1, 0.5, 1]
        self.renderer.light_intensity_direction = 0.3
        self.renderer.light_intensity_ambient = 0.5
        self.renderer.background_color = [1.0, 1.0, 1.0]
        # one scene = object first, then the hands (first frame's meshes give the per-mesh face counts).  Three colourings
        # of it, each stored as `faces<suffix>` / `textures<suffix>` replicated over the frames (:177-219): the fit
        # (gold object, grey hands), the ground truth (green, blue), and both in one scene (fit meshes, then truth meshes).
        scene = [(self.verts_object_init[:1], self.faces_object[:1])]
        scene += [(self.verts_hand_init[h:h + 1], self.faces_hand[h:h + 1]) for h in range(self.hand_nb)]
        fit_palette = ["gold"] + ["grey"] * self.hand_nb
        truth_palette = ["green"] + ["blue"] * self.hand_nb
        for suffix, meshes, palette in (("", scene, fit_palette), ("_gt", scene, truth_palette),
                                        ("_with_gt", scene + scene, fit_palette + truth_palette)):
            f, tex = get_faces_and_textures([v for v, _ in meshes], [t for _, t in meshes], color_names=palette)
            setattr(self, "faces" + suffix, f.repeat(batch_size, 1, 1))
            setattr(self, "textures" + suffix, tex.repeat(batch_size, 1, 1, 1, 1, 1))

    def render_limem(self, renderer, verts, faces, textures, K, max_in_batch=5):
        """:510-544: render in chunks, -> images (N,S,S,3) float in [0,1] (numpy), masks (N,S,S) bool."""
        sample_nb = verts.shape[0]
        assert verts.dim() == 3 and verts.shape[2] == 3
        assert tuple(faces.shape[::2]) == (sample_nb, 3) and tuple(textures.shape[2:]) == (1, 1, 1, 3)
        assert tuple(K.shape) == (sample_nb, 3, 3)
        chunk_nb = (sample_nb + 1) // min(max_in_batch, sample_nb) if max_in_batch is not None else 1
        all_images, all_masks = [], []
        for vert, face, tex, camintr in zip(verts.chunk(chunk_nb, 0), faces.chunk(chunk_nb, 0),
                                            textures.chunk(chunk_nb, 0), K.chunk(chunk_nb, 0)):
            chunk_images, _, chunk_masks = renderer.render(vertices=vert.contiguous(), faces=face.contiguous(),
                                                           textures=tex.contiguous(), K=camintr.contiguous())
            all_images.append(np.clip(chunk_images.cpu().numpy().transpose(0, 2, 3, 1), 0, 1))
            all_masks.append(chunk_masks.cpu().numpy().astype(bool))
        return np.concatenate(all_images), np.concatenate(all_masks)

    def _viz_K(self, renderer, n):
        K = renderer.K
        return (K.repeat(n, 1, 1) if K.shape[0] == 1 else K)[:n]

    def render(self, renderer, rotate=False, viz_len=10, max_in_batch=None):
        """:546-562."""
        with torch.no_grad():
            verts_object = self.get_verts_object()[0]
            verts_hands = self.get_verts_hand()[0]
            verts_hands = [verts_hands[i::self.hand_nb] for i in range(self.hand_nb)]
            verts_combined = combine_verts([verts_object] + verts_hands)
            if rotate:
                verts_combined = trans3d.rot_points(verts_combined)
            n = min(viz_len, verts_combined.shape[0])
            return self.render_limem(renderer, verts_combined[:viz_len], self.faces[:viz_len], self.textures[:viz_len],
                                     K=self._viz_K(renderer, n), max_in_batch=max_in_batch)

    def render_gt(self, renderer, verts_hand_gt=None, verts_object_gt=None, rotate=False, viz_len=10, max_in_batch=None):
        """:564-581."""
        with torch.no_grad():
            verts_combined = combine_verts([verts_object_gt, verts_hand_gt])
            if rotate:
                verts_combined = trans3d.rot_points(verts_combined)
            n = min(viz_len, verts_combined.shape[0])
            return self.render_limem(renderer, verts_combined[:viz_len], self.faces[:viz_len], self.textures_gt[:viz_len],
                                     K=self._viz_K(renderer, n), max_in_batch=max_in_batch)

    def render_with_gt(self, renderer, verts_hand_gt=None, verts_object_gt=None, rotate=False, viz_len=10, init=False,
                       max_in_batch=None):
        """:583-613."""
        with torch.no_grad():
            if init:
                verts_object_pred, verts_hands = self.verts_object_init, self.verts_hand_init
            else:
                verts_object_pred, verts_hands = self.get_verts_object()[0], self.get_verts_hand()[0]
            verts_hands_pred = [verts_hands[i::self.hand_nb] for i in range(self.hand_nb)]
            verts_list = [verts_object_pred] + verts_hands_pred + [verts_object_gt] + [v for v in verts_hand_gt]
            verts_combined = combine_verts(verts_list)
            if rotate:
                verts_combined = trans3d.rot_points(verts_combined)
            n = min(viz_len, verts_combined.shape[0])
            return self.render_limem(renderer, verts_combined[:viz_len], self.faces_with_gt[:viz_len],
                                     self.textures_with_gt[:viz_len], K=self._viz_K(renderer, n),
                                     max_in_batch=max_in_batch)

    def save_obj(self, fname):
        """:615-628: first scene of the clip as a Wavefront OBJ (combined object + hand mesh)."""
        with torch.no_grad():
            verts_combined = combine_verts([self.get_verts_object()[0], self.get_verts_hand()[0]])
        with open(fname, "w") as fp:
            for v in verts_combined[0].cpu().numpy():
                fp.write(f"v {v[0]:f} {v[1]:f} {v[2]:f}\n")
            for face in self.faces[0].cpu().numpy():
                fp.write(f"f {face[0] + 1:d} {face[1] + 1:d} {face[2] + 1:d}\n")

    # ------------------------------------------------------------------ vertices
    def get_verts_object(self):
        """reference homan.py:298-307."""
        return ops.rigid_transform(self.verts_object_og, self.rotations_object, self.translations_object,
                                   self.int_scales_object, abs_scale=True)

    def _mano_verts(self):
        if self._mano_cache is not None:
            return self._mano_cache
        h = self.hand_nb
        if h == 1:
            return self.mano_model.forward_pca(self.mano_pca_pose, rot=self.mano_rot, betas=self.mano_betas,
                                               side=self.hand_sides[0], trans=self.mano_trans)["verts"]
        # hands interleaved frame-major [h0_t0, h1_t0, h0_t1, ...] (homan.py:62-63): hand i is the strided slice i::h through
        # ITS side's layer (:343-358), re-interleaved
        per_hand = [self.mano_model.forward_pca(self.mano_pca_pose[i::h].contiguous(), rot=self.mano_rot[i::h].contiguous(),
                                                betas=self.mano_betas[i::h].contiguous(), side=side,
                                                trans=self.mano_trans[i::h].contiguous())["verts"]
                    for i, side in enumerate(self.hand_sides)]
        return torch.stack(per_hand, 1).reshape(-1, 778, 3)

    def get_verts_hand(self, detach_scale=False):
        """reference homan.py:341-382 (persp)."""
        verts_hand_og = self._mano_verts() if self.optimize_mano else self.verts_hand_og
        scale = self.int_scales_hand.detach() if detach_scale else self.int_scales_hand
        if self.hand_proj_mode == "persp":
            return ops.rigid_transform(verts_hand_og, self.rotations_hand, self.translations_hand, scale,
                                       abs_scale=False)
        if self.hand_proj_mode == "ortho":
            # reference homan.py:364-371 -> utils/camera.py:59-105: no rotation, the translation follows from the weak camera
            # `cams_hand` (a Parameter with `optimize_ortho_cam`), vertices = s * (v + trans).  On the kernels' rigid
            # transform that is (s * v) @ I + (s * trans); the twin detaches the MESH only (scale and camera keep their gradient
            # there, unlike the perspective twin), hence the second call on the detached mesh.  Eager / graph loops only.
            h = len(self.hand_sides)          # (cams_hand holds B * hand_nb rows, frame-major: K once per hand)
            K = self.camintr if h == 1 else self.camintr.repeat_interleave(h, dim=0)
            trans = weakcam_persp_trans(self.cams_hand, K)
            ident = torch.eye(3, device=trans.device)[:, :2].expand(trans.shape[0], 3, 2).contiguous()
            st = scale.view(-1, 1, 1) * trans
            full = ops.rigid_transform(verts_hand_og, ident, st, scale, abs_scale=False)[0]
            twin = ops.rigid_transform(verts_hand_og.detach(), ident, st, scale, abs_scale=False)[0]
            return full, twin
        raise ValueError(f"Expected hand_proj_mode {self.hand_proj_mode} to be in [ortho|persp]")

    def get_joints_hand(self):
        """reference homan.py:309-339 (21 joints incl. finger tips, camera space); no gradient."""
        with torch.no_grad():
            h = self.hand_nb
            joints = torch.stack([self.mano_model.joints(self.mano_pca_pose[i::h].contiguous(), self.mano_rot[i::h].contiguous(),
                                                         self.mano_betas[i::h].contiguous(), side=side)
                                  for i, side in enumerate(self.hand_sides)], 1).reshape(-1, 16, 3)
            verts = self._mano_verts() - self.mano_trans.unsqueeze(1)
            tips = verts[:, [745, 317, 444, 556, 673]]
            full = torch.cat([joints, tips], 1)[:, [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8,
                                                    9, 20]]
            full = full + self.mano_trans.unsqueeze(1)
            return ops.rigid_transform(full.contiguous(), self.rotations_hand, self.translations_hand,
                                       self.int_scales_hand, abs_scale=False)

    # ------------------------------------------------------------------ losses
    def _depth_masks(self):
        """the u8 instance masks of the ordinal depth term's layers [object, hand 0, (hand 1)], from the model's buffers"""
        size = int(self.image_size)
        if tuple(self.masks_object.shape[1:]) != (size, size) or tuple(self.masks_human.shape[1:]) != (size, size):
            raise NotImplementedError("ordinal depth: instance masks must be (B, image_size, image_size), got "
                                      f"{tuple(self.masks_object.shape)} / image_size {size}")
        return [(m != 0).to(torch.uint8).contiguous()
                for m in [self.masks_object] + [self.masks_human[h::self.hand_nb] for h in range(self.hand_nb)]]

    def depth_layers(self):
        """([raster context], [instance mask u8]) of the ordinal depth term, one of each per layer [object, hand 0, (hand 1)], at
        the full-image size (built once) - a context carries ONE render's intermediates to its backward, so every layer has its own"""
        if self._depth_state is None:
            masks = self._depth_masks()
            batch, dev = self.translations_object.shape[0], self.translations_object.device
            faces = [self.faces_object] + [self.faces_hand[h:h + 1].expand(batch, -1, -1) for h in range(self.hand_nb)]
            self._depth_state = ([ops.SilhouetteContext(f, m.shape[1], batch, int(self.image_size), dev)
                                  for f, m in zip(faces, [self.verts_object_og] + [self.verts_hand_og] * self.hand_nb)], masks)
        return self._depth_state

    def depth_contexts(self):
        """the one-hand view of depth_layers(): (object context, hand context, object mask u8, hand mask u8)"""
        ctxs, masks = self.depth_layers()
        return ctxs[0], ctxs[1], masks[0], masks[1]

    def render_depth_layers(self, verts_object, verts_hand, layers=None):
        """{layer: (silhouette, depth)} of the layers [object, hand 0, (hand 1)] named in `layers` (default: all), each rendered
        ONCE at the full-image intrinsics on its own context of depth_layers() (reference homan.py:391,403-417: one render per
        hand over its strided rows).  Every depth term of a forward consumes these renders; autograd sums their gradient images
        into one depth backward per layer."""
        ctxs, _ = self.depth_layers()
        verts = [verts_object] + ([verts_hand] if self.hand_nb == 1 else
                                  [verts_hand[h::self.hand_nb].contiguous() for h in range(self.hand_nb)])
        return {l: ops.depth_render(verts[l], self.camintr, ctxs[l], 1.0)
                for l in (range(len(ctxs)) if layers is None else layers)}

    def compute_ordinal_depth_loss(self, verts_object=None, verts_hand=None, renders=None):
        """reference homan/homan.py:384-419: render object and hand depth at the full-image intrinsics, compare their
        ordering with the instance masks (lossutils.py:133-169); with two hands the three layers pair-wise.
        renders: render_depth_layers() of this forward, when another depth term shares them."""
        if renders is None:
            if verts_object is None:
                verts_object, _ = self.get_verts_object()
            if verts_hand is None:
                verts_hand, _ = self.get_verts_hand()
            renders = self.render_depth_layers(verts_object, verts_hand)
        _, masks = self.depth_layers()
        sils, deps = [renders[l][0] for l in range(len(masks))], [renders[l][1] for l in range(len(masks))]
        # (two layers: the object-hand pair of the two-layer kernels; three: every pair of them)
        return {"loss_depth": ops.ordinal_depth_loss_layers(deps, sils, masks, self.reduce_ws)}

    def depth_obs_layer_ids(self):
        """the layers of depth_layers() the observed-depth term compares, by the option depth_obs_layers"""
        return {"all": list(range(1 + self.hand_nb)), "object": [0], "hand": list(range(1, 1 + self.hand_nb))}[self.depth_obs_layers]

    def compute_depth_obs_loss(self, renders, sole_consumer):
        """({"loss_depth_obs"}, {"depth_obs_mae", "depth_obs_valid_share"}): the observed-depth term (ops.depth_obs_loss; the rule is
        in include/homan_amd.h and DESIGN.md section 7) on the layers of depth_obs_layers, against the buffer `depth_maps`.
        sole_consumer: no other term reads these renders' depth images, so their backward may take the sparse path."""
        ids = self.depth_obs_layer_ids()
        ctxs, masks = self.depth_layers()
        if self._depth_obs_scratch is None:
            self._depth_obs_scratch = ops.DepthObsScratch(len(ids), self.depth_maps.shape[0], self.depth_maps.device)
        loss, mae, share = ops.depth_obs_loss([renders[l][1] for l in ids], [renders[l][0] for l in ids], [masks[l] for l in ids],
                                              self.depth_maps, self.depth_obs_delta, self._depth_obs_scratch,
                                              [ctxs[l] for l in ids] if sole_consumer else None)
        return {"loss_depth_obs": loss}, {"depth_obs_mae": mae, "depth_obs_valid_share": share}

    def compute_surface_contact_loss(self, verts_hand, verts_object):
        """({"loss_surf_attr", "loss_surf_rep"}, {"surf_inside_share"}) on the model's options (lossutils)"""
        if self._surf_ctxs is None:
            self._surf_ctxs = lossutils.surface_contact_contexts(
                verts_object.shape[0], self.hand_nb, np.asarray(self.mano_model.closed_faces), self.faces_object[0],
                verts_object.shape[1], verts_object.device, self.surface_two_way, self.surface_contact_zones)
        return lossutils.compute_surface_contact_loss(verts_hand, verts_object, self._surf_ctxs, self.surface_contact_thresh,
                                                      self.surface_collision_thresh)

    def forward(self, loss_weights=None):
        """reference homan.py:421-508: a loss whose weight is zero is not computed.  The one exception to "None computes
        everything" is the surface contact loss, an extra: it runs only when loss_weights holds a positive lw_surf_attr or
        lw_surf_rep (the term with a positive weight is returned), so forward(None) and weight sets without those keys
        return the reference's keys.  The observed-depth term, the other extra, follows the same rule on lw_depth_obs (and needs
        the model's depth_maps)."""
        lw = loss_weights
        on = lambda key: lw is None or lw[key] > 0
        want_obs = lw is not None and lw.get("lw_depth_obs", 0) > 0
        if want_obs and not hasattr(self, "depth_maps"):
            raise ValueError("lw_depth_obs > 0: the model has no sensor depth; build it with depth_maps=(B, image_size, image_size)")
        loss_dict, metric_dict = {}, {}
        if self.optimize_mano:      # MANO is evaluated once and shared by the reference's two get_verts_hand calls
            self._mano_cache = None
            self._mano_cache = self._mano_verts()
        try:
            verts_object, _ = self.get_verts_object()
            verts_hand, verts_hand_det = self.get_verts_hand()
            if self.int_scales_hand.requires_grad:
                verts_hand_det_scale, _ = self.get_verts_hand(detach_scale=True)
            else:       # the scale is a buffer: detaching it changes nothing
                verts_hand_det_scale = verts_hand
        finally:
            self._mano_cache = None
        want_pca, want_so, want_sh = on("lw_pca"), on("lw_scale_obj"), on("lw_scale_hand")
        if want_pca or want_so or want_sh:
            l_pca, l_so, l_sh = ops.priors(self.mano_pca_pose, self.int_scales_object, self.int_scale_object_mean,
                                           self.int_scales_hand, self.int_scale_hand_mean)
            if want_pca:
                loss_dict["loss_pca"] = l_pca
        if lw is None or lw["lw_smooth_hand"] > 0 or lw["lw_smooth_obj"] > 0:
            loss_dict.update(lossutils.compute_smooth_loss(verts_hand, verts_object, self.reduce_ws))
        if on("lw_collision"):
            loss_dict.update(lossutils.compute_collision_loss(verts_hand_det_scale, verts_object.detach(),
                                                              self.collision_ctx))
        nn_cache = None
        if on("lw_contact"):
            l_contact, nn_cache = lossutils.compute_contact_loss(verts_hand_det_scale, verts_object, self.reduce_ws)
            loss_dict.update(l_contact)
        if lw is not None and (lw.get("lw_surf_attr", 0) > 0 or lw.get("lw_surf_rep", 0) > 0):
            l, m = self.compute_surface_contact_loss(verts_hand_det_scale, verts_object)
            loss_dict.update({k: v for k, v in l.items() if lw.get(k.replace("loss", "lw"), 0) > 0})
            metric_dict.update({k: v.item() if self.sync_metrics else v.detach() for k, v in m.items()})
        if on("lw_v2d_hand"):
            l, m = self.losses.compute_verts2d_loss_hand(verts_hand, image_size=self.image_size,
                                                         min_hand_size=70 if self.optimize_object_scale else 1000)
            loss_dict.update(l)
            metric_dict.update(m)
        if on("lw_sil_obj"):
            l, m = self.losses.compute_sil_loss_object(verts_object, self.faces_object)
            loss_dict.update(l)
            metric_dict.update(m)
        if on("lw_inter"):
            inter_obj = verts_object.unsqueeze(1) if self.optimize_object_scale else verts_object.unsqueeze(1).detach()
            l, m = self.losses.compute_interaction_loss(verts_hand_det.view(-1, self.hand_nb, 778, 3), inter_obj,
                                                        nn=nn_cache)
            loss_dict.update(l)
            metric_dict.update(m)
        if want_so:
            loss_dict["loss_scale_obj"] = l_so
        if want_sh:
            loss_dict["loss_scale_hand"] = l_sh
        want_ord = lw is None or lw["lw_depth"] > 0
        if want_ord and not self.ordinal_depth:
            # reference homan.py:506-507 calls lossutils.compute_ordinal_depth_loss() without its arguments
            raise TypeError("compute_ordinal_depth_loss() missing 3 required positional arguments: "
                            "'masks', 'silhouettes', and 'depths'")
        # both depth terms consume ONE render per layer (a context holds one render's intermediates)
        renders = None
        if want_ord or want_obs:
            renders = self.render_depth_layers(verts_object, verts_hand, None if want_ord else self.depth_obs_layer_ids())
        if want_ord:
            loss_dict.update(self.compute_ordinal_depth_loss(renders=renders))
        if want_obs:
            l, m = self.compute_depth_obs_loss(renders, sole_consumer=not want_ord)
            loss_dict.update(l)
            metric_dict.update({k: v.item() if self.sync_metrics else v.detach() for k, v in m.items()})
        return loss_dict, metric_dict
