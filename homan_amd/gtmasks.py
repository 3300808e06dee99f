"""Ground-truth instance masks (the `--gt_masks` ablation) of reference homan/prepare/gtmasks.py:14-123 on the project's
rasteriser: the annotated hand and object meshes of every frame are rendered as ONE mesh at the full-image camera, the
front-most instance of every sample is read off the rasteriser's face-index map (`hm_instance_masks`, csrc/maskcrop.hip)
instead of a one-hot colour render, and the crops come from the HIP crop-and-resize (homan_amd/maskutils.py).
There is no CPU path: without a GPU this raises."""
import numpy as np
import torch

from . import lib, maskutils, ops
from .bbox import bbox_wh_to_xy
from .constants import REND_SIZE


def instance_sample_counts(verts, faces, face_start, K, image_size):
    """verts (B,V,3) camera space, faces (F,3) of the concatenated instances, instance i = faces
    [face_start[i], face_start[i+1]), K (B,3,3) pixel intrinsics -> (B,I,image_size,image_size) uint8: how many of the
    pixel's 2x2 samples show instance i in front (count / 4 = `renders[:, i]` of reference gtmasks.py:77, count > 0 = mask)."""
    if not torch.cuda.is_available():
        raise lib.HomanAmdError("homan_amd.gtmasks needs the GPU (there is no CPU fallback)")
    dev = verts.device if verts.is_cuda else torch.device("cuda")
    import ctypes
    with torch.cuda.device(dev), torch.no_grad():
        verts = verts.detach().to(device=dev, dtype=torch.float32).contiguous()
        B, I = verts.shape[0], len(face_start) - 1
        K_nc = torch.as_tensor(K, dtype=torch.float32).to(dev).reshape(-1, 3, 3).clone()
        K_nc[:, :2] = 1 / image_size * K_nc[:, :2]
        faces = torch.as_tensor(np.asarray(faces).astype(np.int32))[None].repeat(B, 1, 1)
        sctx = ops.SilhouetteContext(faces, verts.shape[1], B, image_size, dev)
        ops.silhouette_render(verts, K_nc.contiguous(), sctx)
        starts = (ctypes.c_int * (I + 1))(*[int(s) for s in face_start])
        out = torch.empty(B, I, sctx.S, sctx.S, dtype=torch.uint8, device=dev)
        lib.check(lib.lib().hm_instance_masks(lib.ptr(sctx.idx_map()), B, sctx.S, sctx.F, ctypes.cast(starts, ctypes.c_void_p), I,
                                              lib.ptr(out), lib.stream()), "hm_instance_masks")
        return out[:, :, :image_size, :image_size].contiguous()


def _assign(dst, src):
    """dst[:] = src for a numpy or a torch destination"""
    if isinstance(dst, np.ndarray):
        dst[:] = src.cpu().numpy()
    else:
        dst[:] = src.to(dst.device)


def render_gt_masks(annots, obj_infos, person_parameters, sample_folder="", debug=False, image_size=640, rend_size=REND_SIZE):
    """Replace object and hand masks with ground truth (reference prepare/gtmasks.py:14-123).  annots: {"camera": {"K":
    (B,3,3) pixels}, "hands": [{"verts3d": (B,V,3), "faces": (B,F,3)}], "objects": [...]}; obj_infos: per-frame dicts with
    `square_bbox` (xywh), `target_crop_mask`, `crop_mask`, `full_mask`; person_parameters: per-frame dicts with `bboxes`.
    Overwrites in place: `target_crop_mask` = object crop minus the union of the hands' crops (values in {-1, 0, 1}),
    `crop_mask`, `full_mask` (the first object's) and person_parameters[t]["masks"] (the hands' anti-aliased renders)."""
    hand_nb = len(annots["hands"])
    all_verts, all_faces, face_start, verts_off = [], [], [0], 0
    for inst in list(annots["hands"]) + list(annots["objects"]):
        verts3d = torch.as_tensor(np.asarray(inst["verts3d"]), dtype=torch.float32)
        faces = np.asarray(inst["faces"])
        faces = faces[0] if faces.ndim == 3 else faces
        all_faces.append(faces.astype(np.int64) + verts_off)
        all_verts.append(verts3d)
        verts_off += verts3d.shape[1]
        face_start.append(face_start[-1] + faces.shape[0])
    counts = instance_sample_counts(torch.cat(all_verts, 1), np.concatenate(all_faces), face_start,
                                    np.asarray(annots["camera"]["K"], dtype=np.float32), image_size)
    B, I = counts.shape[:2]
    if len(obj_infos) != B or len(person_parameters) != B:
        raise ValueError(f"{B} annotated frames for {len(obj_infos)} obj_infos and {len(person_parameters)} person_parameters")
    obj_square_bboxes = bbox_wh_to_xy(torch.Tensor(np.stack([obj_info["square_bbox"] for obj_info in obj_infos])))
    flat = counts.view(B * I, image_size, image_size)                  # instance i of frame b = mask b * I + i
    frames = torch.arange(B)
    obj_crops = maskutils.crop_and_resize(flat, obj_square_bboxes, rend_size, index=frames * I + hand_nb)
    hands_of = frames[:, None] * I + torch.arange(hand_nb)[None] if hand_nb else torch.full((B, 1), -1)
    gt_obj_occlusions = maskutils.target_masks(maskutils.MODE_MINUS, flat, flat, obj_square_bboxes, rend_size,
                                               target_index=frames * I + hand_nb, occluder_index=hands_of)
    if debug and sample_folder:
        import os
        from PIL import Image
        row = np.concatenate(list((counts[0].cpu().numpy() * 63).astype(np.uint8)), axis=1)
        Image.fromarray(row).save(os.path.join(sample_folder, "rendered_gt.png"))
    for time_idx, obj_info in enumerate(obj_infos):
        h, w = obj_info["full_mask"].shape[:2]
        _assign(obj_info["target_crop_mask"], gt_obj_occlusions[time_idx])
        _assign(obj_info["crop_mask"], obj_crops[time_idx])
        _assign(obj_info["full_mask"], counts[time_idx, hand_nb, :h, :w] > 0)
    for time_idx, person_param in enumerate(person_parameters):
        hand_render_mask = counts[time_idx, :hand_nb, :h, :w].float() * 0.25
        if "masks" in person_param:
            _assign(person_param["masks"], hand_render_mask)
        else:
            person_param["masks"] = hand_render_mask
