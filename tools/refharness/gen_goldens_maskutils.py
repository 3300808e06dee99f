#!/usr/bin/env python
"""Golden vectors for the target masks (homan_amd/maskutils.py, homan_amd/bbox.py), produced by the REFERENCE's own
homan/lib2d/maskutils.py (add_occlusions, add_target_hand_occlusions) and homan/utils/bbox.py, imported in place, over the
CPU restatement of detectron2's BitMasks.crop_and_resize (tests/maskcrop_ref.py) and the two BoxMode conversions the
reference uses.  Build container only; writes tests/golden/maskutils_reference.npz (or the path given as the first
argument): inputs and outputs only, masks as uint8 / int8."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import shims  # noqa: E402

# (not ref_*.npz: tests/util.py reads every ref_*.npz but the pose-initialisation one as a joint-fit golden)
OUT = os.path.join(ROOT, "tests", "golden", "maskutils_reference.npz")


class BoxMode:
    """detectron2.structures.BoxMode for the conversions of homan/utils/bbox.py:70-86 (XYXY_ABS <-> XYWH_ABS): a copy of the
    boxes with columns 2, 3 shifted by columns 0, 1; the type of the input (tensor, array, list, tuple) is kept."""
    XYXY_ABS, XYWH_ABS = 0, 1

    @staticmethod
    def convert(box, from_mode, to_mode):
        assert {from_mode, to_mode} == {BoxMode.XYXY_ABS, BoxMode.XYWH_ABS}
        single = isinstance(box, (list, tuple))
        if single:
            arr = torch.tensor(box)[None, :]
        elif isinstance(box, np.ndarray):
            arr = torch.from_numpy(np.asarray(box)).clone()
        else:
            arr = box.clone()
        if to_mode == BoxMode.XYXY_ABS:
            arr[:, 2] += arr[:, 0]
            arr[:, 3] += arr[:, 1]
        else:
            arr[:, 2] -= arr[:, 0]
            arr[:, 3] -= arr[:, 1]
        if single:
            return type(box)(arr.flatten().tolist())
        return arr.numpy() if isinstance(box, np.ndarray) else arr


def import_maskutils():
    from tests.maskcrop_ref import BitMasks
    shims.install()
    shims._module("detectron2")
    shims._module("detectron2.structures", BitMasks=BitMasks, BoxMode=BoxMode)
    shims._module("detectron2.structures.boxes", BoxMode=BoxMode)
    shims._module("libyana.visutils.imagify", viz_imgrow=lambda *a, **k: None)
    cwd = os.getcwd()
    os.chdir(shims.REFERENCE_ROOT)
    sys.path.insert(0, shims.REFERENCE_ROOT)
    try:
        import homan.lib2d.maskutils as ref_mu
        import homan.utils.bbox as ref_bbox
    finally:
        os.chdir(cwd)
        sys.path.remove(shims.REFERENCE_ROOT)
    # shims.install() has imported homan.utils.bbox already (through homan.homan), over its placeholder detectron2
    ref_bbox.BoxMode = BoxMode
    ref_mu.BitMasks = BitMasks
    return ref_mu, ref_bbox


def instance_masks(image_size, hands, seed, rows=None):
    """full-image instance masks of frame 0 of a synthetic clip: hands (h,H,W) and object (H,W), uint8; rows = (r0, r1)
    keeps that band of image rows (a non-square image)"""
    from homan_amd import synth
    from homan_amd.mano_assets import synthetic_mano
    from tests import util
    sil_fn, hand_fn = util.oracle_clip_fns(synthetic_mano(0))
    clip = synth.make_clip(seed=seed, frames=1, rend_size=32, image_size=image_size, obj="bottle", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn, hands=hands)
    hm = clip["person_parameters"][0]["masks"].numpy() > 0
    om = clip["object_parameters"][0]["full_mask"].numpy() > 0
    if rows is not None:
        hm, om = hm[:, rows[0]:rows[1]], om[rows[0]:rows[1]]
    K = clip["camintr"][0].copy()
    K[:2] *= image_size
    if rows is not None:
        K[1, 2] -= rows[0]
    return hm.astype(np.uint8), om.astype(np.uint8), K.astype(np.float32)


def tight_box(mask):
    """x1 y1 x2 y2 around the set pixels of a mask (the detector's box), float32"""
    ys, xs = np.nonzero(mask)
    return np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float32)


def hand_cases():
    """name -> (hand masks (h,H,W), tight xyxy boxes (h,4), object mask (H,W), K, square_expand)"""
    cases = {}
    hm, om, K = instance_masks(128, ("right",), 11, rows=(16, 112))                      # 96 x 128, one hand
    cases["h1_96x128_e0"] = (hm, np.stack([tight_box(m) for m in hm]), om, K, 0)         # small box: up-sampling, grid 1
    cases["h1_96x128_e03"] = (hm, np.stack([tight_box(m) for m in hm]) + np.float32(0.37), om, K, 0.3)   # fractional
    hm2, om2, K2 = instance_masks(128, ("right", "left"), 12, rows=(16, 112))            # 96 x 128, two hands
    b2 = np.stack([tight_box(m) for m in hm2])
    b2[0] += np.array([-30.25, -40.5, -30.25, -20.5], np.float32)                        # partly outside the image
    cases["h2_96x128_e03"] = (hm2, b2, om2, K2, 0.3)
    hm3, om3, K3 = instance_masks(640, ("right",), 13)                                   # 640 x 640, one hand
    t = tight_box(hm3[0])
    cx, cy = (t[0] + t[2]) / 2, (t[1] + t[3]) / 2
    boxes = np.array([t,                                                                  # as detected
                      [cx - 150.3, cy - 140.1, cx + 150.4, cy + 120.2],                   # grid 2, fractional
                      [cx - 330.0, cy - 200.0, cx + 330.5, cy + 330.0],                   # grid 3, partly outside
                      [cx - 10.5, cy - 9.25, cx + 12.0, cy + 11.5]], np.float32)          # 22 pixels: strong up-sampling
    cases["h1_640_boxes_e0"] = (np.repeat(hm3, 4, 0), boxes, om3, K3, 0)
    hm4, om4, K4 = instance_masks(640, ("right", "left"), 14)                            # 640 x 640, two hands + an empty mask
    m4 = np.concatenate([hm4, np.zeros_like(hm4[:1])])
    b4 = np.concatenate([np.stack([tight_box(m) for m in hm4]), np.array([[200.0, 180.0, 420.0, 400.0]], np.float32)])
    cases["h2_640_empty_e03"] = (m4, b4, om4, K4, 0.3)
    return cases


def main(out=OUT):
    ref_mu, ref_bbox = import_maskutils()
    from tests.maskcrop_ref import crop_and_resize
    S = ref_mu.REND_SIZE
    rec = {"meta_rend_size": np.array(S)}
    cases = hand_cases()
    rec["meta_hand_cases"] = np.array(sorted(cases))
    for name, (hm, boxes, om, K, expand) in sorted(cases.items()):
        person = {"masks": torch.from_numpy(hm.astype(np.float32)), "bboxes": torch.from_numpy(boxes.copy())}
        obj = {"full_mask": torch.from_numpy(om.astype(np.float32))}
        res = ref_mu.add_target_hand_occlusions(person, obj, K.copy(), square_expand=expand, debug=False)
        rec.update({f"{name}_in_masks": hm, f"{name}_in_bboxes": boxes, f"{name}_in_full_mask": om, f"{name}_in_K": K,
                    f"{name}_in_square_expand": np.array(expand, np.float64),
                    f"{name}_out_target_masks": res["target_masks"].numpy().astype(np.int8),
                    f"{name}_out_K_roi": res["K_roi"].numpy(), f"{name}_out_square_bboxes": res["square_bboxes"].numpy()})
        assert res["target_masks"].dtype == torch.float32 and res["K_roi"].dtype == torch.float32
    # ---- add_occlusions: object crops (cut with the restatement: they are inputs here) occluded by the hands' masks
    occ = {"o_96x128": cases["h2_96x128_e03"], "o_640": cases["h2_640_empty_e03"]}
    rec["meta_object_cases"] = np.array(sorted(occ))
    for name, (hm, _, om, _, _) in sorted(occ.items()):
        t = tight_box(om)
        xywh = ref_bbox.make_bbox_square(ref_bbox.bbox_xy_to_wh(t), 0.3)
        shifted = xywh + np.array([7.3, -4.6, 0.0, 0.0], np.float32)                      # a second, off-centre box
        bbs = [xywh.astype(np.float32), shifted.astype(np.float32)]
        crops = [crop_and_resize(om[None], ref_bbox.bbox_wh_to_xy(b)[None], S)[0] for b in bbs]
        res = ref_mu.add_occlusions(crops, torch.from_numpy(hm.astype(np.float32)), bbs)
        rec.update({f"{name}_in_masks": np.stack(crops).astype(np.uint8), f"{name}_in_mask_bboxes": np.stack(bbs),
                    f"{name}_in_occluder_mask": hm, f"{name}_out_occluded": np.stack(res).astype(np.int8)})
        assert all(r.dtype == np.float32 for r in res)
    # ---- the bbox helpers on arrays, a tensor and a list
    rng = np.random.default_rng(5)
    xyxy = (rng.uniform(0, 300, (5, 2)).astype(np.float32))
    xyxy = np.concatenate([xyxy, xyxy + rng.uniform(5, 200, (5, 2)).astype(np.float32)], 1)
    wh = ref_bbox.bbox_xy_to_wh(xyxy)
    rec.update(bbox_in_xyxy=xyxy, bbox_out_wh=wh, bbox_out_xy_again=ref_bbox.bbox_wh_to_xy(wh),
               bbox_out_square_e0=ref_bbox.make_bbox_square(wh, 0.0), bbox_out_square_e03=ref_bbox.make_bbox_square(wh, 0.3),
               bbox_out_square_single=ref_bbox.make_bbox_square(wh[2], 0.3),
               bbox_out_wh_tensor=ref_bbox.bbox_xy_to_wh(torch.from_numpy(xyxy)).numpy(),
               bbox_out_wh_list=np.array(ref_bbox.bbox_xy_to_wh([float(v) for v in xyxy[1]]), np.float64))
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
