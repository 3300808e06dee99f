"""Target masks, occlusions and ROI intrinsics of reference homan/lib2d/maskutils.py on the HIP crop-and-resize.

`add_occlusions` (:16-38) and `add_target_hand_occlusions` (:41-81) keep the reference's names and arguments; detectron2's
`BitMasks.crop_and_resize`, which both rest on, is `crop_and_resize` here (csrc/maskcrop.hip: ROIAlign of the binarised
mask, >= 0.5), and each function is ONE `hm_target_masks` launch.  `add_target_hand_occlusions_clip` does the per-frame loop
of reference fit_vid_dataset.py:300-308 as one launch over every hand of every frame.  Masks may be bool, byte or float,
tensors (any device) or arrays; the results live where the inputs did.  There is no CPU path: without a GPU these functions
raise.
"""
import os

import numpy as np
import torch

from . import lib
from .bbox import bbox_wh_to_xy, bbox_xy_to_wh, make_bbox_square
from .constants import REND_SIZE
from .pose_optimization import get_K_crop_resize

MODE_HAND, MODE_OBJECT, MODE_MINUS = 0, 1, 2


def _device(*tensors):
    if not torch.cuda.is_available():
        raise lib.HomanAmdError("homan_amd.maskutils needs the GPU (there is no CPU fallback)")
    return next((t.device for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda), torch.device("cuda"))


def _masks_arg(masks, dev):
    """(N,H,W) masks of any dtype -> (contiguous device tensor of bytes or fp32, is_fp32)"""
    m = torch.as_tensor(masks)
    if m.dim() != 3 or 0 in m.shape:
        raise ValueError(f"expected non-empty (N, H, W) masks, got {tuple(m.shape)}")
    m = m.detach().to(dev)
    if m.dtype == torch.bool:
        m = m.contiguous().view(torch.uint8)
    elif m.dtype not in (torch.uint8, torch.float32):
        m = (m != 0).to(torch.uint8)
    return m.contiguous(), int(m.dtype == torch.float32)


def _boxes_arg(boxes, dev):
    b = torch.as_tensor(boxes).detach().to(device=dev, dtype=torch.float32).reshape(-1, 4).contiguous()
    return b


def _index_arg(index, shape, limit, dev):
    """host-checked int32 index tensor on the device (negative entries = none, where the kernel allows them)"""
    idx = torch.as_tensor(index).detach().reshape(shape)
    if idx.numel() and int(idx.max()) >= limit:
        raise ValueError(f"mask index {int(idx.max())} out of range for {limit} masks")
    return idx.to(device=dev, dtype=torch.int32).contiguous()


def crop_and_resize(masks, boxes, size, index=None):
    """detectron2 `BitMasks(masks).crop_and_resize(boxes, size)`: masks (N,H,W), boxes (R,4) x1 y1 x2 y2 in pixels ->
    bool (R,size,size).  index (R) names the mask of each box (default: box r crops mask r, R == N)."""
    dev = _device(masks, boxes)
    m, f32 = _masks_arg(masks, dev)
    b = _boxes_arg(boxes, dev)
    R, (N, H, W) = b.shape[0], m.shape
    if index is None:
        if R != N:
            raise ValueError(f"{R} boxes for {N} masks: pass `index`")
        idx = None
    else:
        idx = _index_arg(index, (R,), N, dev)
        if R and int(idx.min()) < 0:
            raise ValueError("negative mask index")
    out = torch.empty(R, int(size), int(size), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        lib.check(lib.lib().hm_mask_crop_resize(lib.ptr(m), f32, N, H, W, lib.ptr(idx), lib.ptr(b), R, int(size), lib.ptr(out),
                                                lib.stream()), "hm_mask_crop_resize")
    out = out.view(torch.bool)
    src = masks if isinstance(masks, torch.Tensor) else None
    return out if src is None or src.is_cuda else out.cpu()


def target_masks(mode, target, occluders, boxes, size, target_index=None, occluder_index=None):
    """hm_target_masks (include/homan_amd.h): the fp32 -1 / 0 / 1 targets (R,size,size) of R boxes in one launch, on the GPU.
    target (Nt,H,W) - (Nt,size,size) in MODE_OBJECT -, occluders (No,H,W), occluder_index (R,K) with negative = none."""
    dev = _device(target, occluders, boxes)
    t, t_f32 = _masks_arg(target, dev)
    o, o_f32 = _masks_arg(occluders, dev)
    b = _boxes_arg(boxes, dev)
    R, size = b.shape[0], int(size)
    No, H, W = o.shape
    if mode == MODE_OBJECT:
        if tuple(t.shape[1:]) != (size, size):
            raise ValueError(f"object targets must be ({size}, {size}) crops, got {tuple(t.shape[1:])}")
    elif tuple(t.shape[1:]) != (H, W):
        raise ValueError(f"target masks {tuple(t.shape[1:])} and occluders {(H, W)} differ in size")
    if target_index is None and t.shape[0] != R:
        raise ValueError(f"{R} boxes for {t.shape[0]} targets: pass `target_index`")
    ti = None if target_index is None else _index_arg(target_index, (R,), t.shape[0], dev)
    oi = torch.arange(No, dtype=torch.int32).repeat(R, 1) if occluder_index is None else occluder_index
    oi = _index_arg(oi, (R, -1), No, dev)
    out = torch.empty(R, size, size, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        lib.check(lib.lib().hm_target_masks(int(mode), lib.ptr(t), t_f32, t.shape[0], lib.ptr(ti), lib.ptr(o), o_f32, No,
                                            lib.ptr(oi), oi.shape[1], H, W, lib.ptr(b), R, size, lib.ptr(out), lib.stream()),
                  "hm_target_masks")
    return out


def add_occlusions(masks, occluder_mask, mask_bboxes, rend_size=REND_SIZE):
    """reference maskutils.py:16-38.  masks: list of (rend_size, rend_size) boolean object crops; mask_bboxes: matching
    list of square xywh boxes; occluder_mask (B,H,W): the occluders' full-image masks.  -> list of float32 arrays: the
    object crop with -1 wherever ANY occluder, cropped to the object's box, is set and 1 wherever the object is."""
    if len(masks) == 0:
        return []
    boxes = bbox_wh_to_xy(torch.Tensor(np.stack([np.asarray(b, dtype=np.float64) for b in mask_bboxes])))
    crops = np.stack([np.asarray(m) for m in masks]) != 0
    out = target_masks(MODE_OBJECT, torch.from_numpy(crops), occluder_mask, boxes, rend_size)
    return list(out.cpu().numpy())


def _square_boxes(tight_boxes, square_expand):
    """xyxy boxes -> squared, expanded xyxy boxes, as a tensor like `tight_boxes` (reference maskutils.py:55-60)"""
    tight_boxes = torch.as_tensor(tight_boxes)
    person_boxes = bbox_wh_to_xy(make_bbox_square(bbox_xy_to_wh(tight_boxes), bbox_expansion=square_expand))
    return torch.as_tensor(person_boxes, dtype=tight_boxes.dtype, device=tight_boxes.device)


def _k_roi(K, person_boxes, rend_size):
    """reference maskutils.py:67-77: crop-resize intrinsics of every box, rows :2 brought to the NC rendering space"""
    n = person_boxes.shape[0]
    K = (K if isinstance(K, torch.Tensor) else torch.as_tensor(np.asarray(K))).to(person_boxes)
    K_roi = get_K_crop_resize(K.reshape(1, 3, 3).repeat(n, 1, 1), person_boxes, [rend_size] * n)
    K_roi[:, :2] = K_roi[:, :2] / rend_size
    return K_roi


def _save_debug(target, sample_folder):
    """the row of occlusion masks the reference draws with libyana's imagify (-1 black, 0 grey, 1 white), with PIL"""
    if not sample_folder:
        return
    from PIL import Image
    row = np.concatenate(list(target.detach().cpu().numpy()), axis=1)
    path = os.path.join(sample_folder, "tmpoccl.png")
    Image.fromarray(((row + 1.0) * 127.5).astype(np.uint8)).save(path)
    print(f"Saving occlusion masks to {path}")


def add_target_hand_occlusions(person_parameters, object_parameters, K, square_expand=0, sample_folder=None, debug=False,
                               rend_size=REND_SIZE):
    """reference maskutils.py:41-81.  person_parameters {"bboxes": (h,4) xyxy, "masks": (h,H,W)}, object_parameters
    {"full_mask": (H,W)}, K (3,3) pixel intrinsics.  Writes `target_masks` (h,rend_size,rend_size) float in {-1, 0, 1}
    (hand crop, -1 where the object's crop is set), `K_roi` (h,3,3) and `square_bboxes` (h,4) in place; returns the dict."""
    return add_target_hand_occlusions_clip([person_parameters], [object_parameters], [K], square_expand=square_expand,
                                           sample_folder=sample_folder, debug=debug, rend_size=rend_size)[0]


def add_target_hand_occlusions_clip(person_parameters, object_parameters, camintr, square_expand=0, sample_folder=None,
                                    debug=False, rend_size=REND_SIZE):
    """The loop of reference fit_vid_dataset.py:300-308 over a clip - lists of per-frame dicts and per-frame (3,3) pixel
    intrinsics (or one (3,3) for all) - as ONE launch over every hand of every frame.  Writes the three keys into every
    frame's person_parameters exactly as the per-frame calls do; returns the list."""
    frames = len(person_parameters)
    if len(object_parameters) != frames:
        raise ValueError(f"{frames} person_parameters for {len(object_parameters)} object_parameters")
    if frames == 0:
        return person_parameters
    if not isinstance(camintr, (list, tuple)):
        camintr = list(camintr) if len(np.shape(camintr)) == 3 else [camintr] * frames
    if len(camintr) != frames:
        raise ValueError(f"{len(camintr)} intrinsics for {frames} frames")
    hand_masks = [torch.as_tensor(p["masks"]) for p in person_parameters]
    obj_masks = [torch.as_tensor(o["full_mask"]) for o in object_parameters]
    dev = _device(*hand_masks, *obj_masks)
    counts = [m.shape[0] for m in hand_masks]
    boxes = [_square_boxes(p["bboxes"], square_expand) for p in person_parameters]
    frame_of = torch.repeat_interleave(torch.arange(frames), torch.tensor(counts))
    out = target_masks(MODE_HAND, torch.cat([m.to(dev) for m in hand_masks]), torch.stack([m.to(dev) for m in obj_masks]),
                       torch.cat([b.to(dev, torch.float32) for b in boxes]), rend_size, occluder_index=frame_of[:, None])
    at = 0
    for p, m, b, K, n in zip(person_parameters, hand_masks, boxes, camintr, counts):
        t = out[at:at + n]
        at += n
        p["K_roi"] = _k_roi(K, b, rend_size)
        p["target_masks"] = t if m.is_cuda else t.cpu()
        p["square_bboxes"] = b
        if debug:
            _save_debug(t, sample_folder)
    return person_parameters
