"""Target masks (homan_amd/maskutils.py, bbox.py, gtmasks.py), CPU side: known answers of the crop-and-resize restatement
(tests/maskcrop_ref.py), the reference's own outputs (tests/golden/maskutils_reference.npz, written by
tools/refharness/gen_goldens_maskutils.py) against that restatement and the bbox helpers, the public signatures, the C ABI's
argument checks and the refusal to run without a GPU.  The GPU tests compare the kernels with the restatement."""
import importlib.util
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import maskcrop_ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "maskutils_reference.npz")
GENERATOR = os.path.join(ROOT, "tools", "refharness", "gen_goldens_maskutils.py")


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def hand_cases(g):
    """[(name, inputs dict, outputs dict)] of add_target_hand_occlusions in the golden file"""
    return [(str(n), {k: g[f"{n}_in_{k}"] for k in ("masks", "bboxes", "full_mask", "K", "square_expand")},
             {k: g[f"{n}_out_{k}"] for k in ("target_masks", "K_roi", "square_bboxes")}) for n in g["meta_hand_cases"]]


def object_cases(g):
    return [(str(n), {k: g[f"{n}_in_{k}"] for k in ("masks", "mask_bboxes", "occluder_mask")}, g[f"{n}_out_occluded"])
            for n in g["meta_object_cases"]]


def compose_hand(masks, full_mask, boxes, size):
    """reference maskutils.py:61-65 over the restatement: hand crops, -1 where the object's crop is set"""
    t = maskcrop_ref.crop_and_resize(masks, boxes, size).astype(np.float32)
    t[maskcrop_ref.crop_and_resize(np.repeat(full_mask[None], len(boxes), 0), boxes, size)] = -1
    return t


def compose_object(crops, occluder_mask, boxes_xyxy, size):
    """reference maskutils.py:29-36 over the restatement"""
    out = []
    for crop, box in zip(crops, boxes_xyxy):
        occ = maskcrop_ref.crop_and_resize(occluder_mask, np.repeat(box[None], len(occluder_mask), 0), size)
        t = (crop != 0).astype(np.float32)
        t[occ.sum(0) > 0] = -1
        t[crop != 0] = 1
        out.append(t)
    return np.stack(out)


# ------------------------------------------------------------------ known answers of the restatement
def test_full_image_box_at_native_size_returns_the_mask():
    rng = np.random.default_rng(0)
    m = rng.random((2, 48, 48)) < 0.4
    out = maskcrop_ref.crop_and_resize(m, np.array([[0, 0, 48, 48]] * 2, np.float32), 48)
    np.testing.assert_array_equal(out, m)


def test_half_size_crop_is_two_of_four_with_ties_kept():
    """box (0, 0, 2S, 2S): the 2x2 samples of an output fall on the four pixels of its block; >= 0.5 keeps the exact ties"""
    rng = np.random.default_rng(1)
    m = rng.random((1, 48, 48)) < 0.5
    out = maskcrop_ref.crop_and_resize(m, np.array([[0, 0, 48, 48]], np.float32), 24)
    blocks = m[0].reshape(24, 2, 24, 2).sum((1, 3))
    assert (blocks == 2).sum() > 100                    # exact 0.5 ties are common: the >= decides them
    np.testing.assert_array_equal(out[0], blocks >= 2)


def test_box_outside_the_image_returns_zeros():
    m = np.ones((1, 20, 30), bool)
    for box in ([40, 5, 60, 15], [-50, -50, -10, -10], [5, 30, 25, 55]):
        assert not maskcrop_ref.crop_and_resize(m, np.array([box], np.float32), 16).any()


def test_bins_wider_than_four_images_are_empty():
    """the kernel answers such boxes without walking their samples (csrc/maskcrop.hip): the restatement, which walks them,
    agrees"""
    m = np.ones((1, 6, 5), bool)
    for box in ([-100, -3, 100, 9], [-2, -300, 7, 300], [0, 0, 5 * 4 * 7 * 4 + 8, 6]):
        assert not maskcrop_ref.crop_and_resize(m, np.array([box], np.float32), 4).any()
    assert maskcrop_ref.crop_and_resize(m, np.array([[0, 0, 5, 6]], np.float32), 4).all()


def test_torch_form_of_the_restatement_is_the_same_function():
    rng = np.random.default_rng(2)
    m = rng.random((3, 40, 56)) < 0.5
    boxes = np.array([[3.3, 2.1, 30.7, 36.2], [-8.5, 10.0, 70.0, 90.5], [10.25, 10.5, 14.0, 15.75], [0, 0, 56, 40]], np.float32)
    index = np.array([2, 0, 1, 1])
    for size in (8, 16):
        a = maskcrop_ref.crop_and_resize(m, boxes, size, index)
        b = maskcrop_ref.crop_and_resize_torch(torch.from_numpy(m), torch.from_numpy(boxes), size, index)
        np.testing.assert_array_equal(a, b.numpy())
    bm = maskcrop_ref.BitMasks(torch.from_numpy(m[index].astype(np.float32)))
    np.testing.assert_array_equal(bm.crop_and_resize(torch.from_numpy(boxes), 16).numpy(), a)


# ------------------------------------------------------------------ the reference's outputs
def test_golden_is_the_composition_over_the_restatement():
    """the reference's add_target_hand_occlusions / add_occlusions outputs = the compositions written out above on the
    boxes homan_amd.bbox makes; K_roi = get_K_crop_resize of those boxes, rows :2 over the render size"""
    from homan_amd import bbox
    from homan_amd.pose_optimization import get_K_crop_resize
    g = load_golden()
    S = int(g["meta_rend_size"])
    grids = set()
    for name, ins, want in hand_cases(g):
        boxes = bbox.bbox_wh_to_xy(bbox.make_bbox_square(bbox.bbox_xy_to_wh(ins["bboxes"]), float(ins["square_expand"])))
        assert boxes.dtype == np.float32
        np.testing.assert_array_equal(boxes, want["square_bboxes"], err_msg=name)
        np.testing.assert_array_equal(compose_hand(ins["masks"], ins["full_mask"], boxes, S), want["target_masks"], err_msg=name)
        n = len(boxes)
        K_roi = get_K_crop_resize(torch.from_numpy(ins["K"])[None].repeat(n, 1, 1), torch.from_numpy(boxes), [S] * n)
        K_roi[:, :2] = K_roi[:, :2] / S
        torch.testing.assert_close(K_roi, torch.from_numpy(want["K_roi"]))
        grids |= {int(max(np.ceil((b[2] - b[0]) / S), 1)) for b in boxes}
        assert set(np.unique(want["target_masks"])) <= {-1, 0, 1}
    assert grids == {1, 2, 3}                                   # up-sampling and both down-sampling grids are covered
    assert any(ins["masks"].shape[1] != ins["masks"].shape[2] for _, ins, _ in hand_cases(g))
    assert any((ins["masks"].reshape(len(ins["masks"]), -1).sum(1) == 0).any() for _, ins, _ in hand_cases(g))
    for name, ins, want in object_cases(g):
        got = compose_object(ins["masks"], ins["occluder_mask"], bbox.bbox_wh_to_xy(ins["mask_bboxes"]), S)
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert (want == -1).any() and (want == 1).any()


def _shims():
    spec = importlib.util.spec_from_file_location("_mu_shims", os.path.join(ROOT, "tools", "refharness", "shims.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_golden_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(_shims().REFERENCE_ROOT, "homan")):
        pytest.skip("the reference sources are not on this machine")
    out = str(tmp_path / "mu.npz")
    subprocess.run([sys.executable, GENERATOR, out], check=True, cwd=ROOT, capture_output=True, timeout=900)
    a, b = np.load(GOLDEN), np.load(out)
    assert a.files == b.files
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_bbox_helpers_match_the_reference():
    from homan_amd import bbox
    g = load_golden()
    xyxy = g["bbox_in_xyxy"]
    wh = bbox.bbox_xy_to_wh(xyxy)
    assert isinstance(wh, np.ndarray) and wh.dtype == np.float32
    np.testing.assert_array_equal(wh, g["bbox_out_wh"])
    np.testing.assert_array_equal(xyxy, g["bbox_in_xyxy"])                       # the input is not written to
    np.testing.assert_array_equal(bbox.bbox_wh_to_xy(wh), g["bbox_out_xy_again"])
    np.testing.assert_array_equal(bbox.make_bbox_square(wh, 0.0), g["bbox_out_square_e0"])
    np.testing.assert_array_equal(bbox.make_bbox_square(wh, 0.3), g["bbox_out_square_e03"])
    np.testing.assert_array_equal(bbox.make_bbox_square(wh[2], 0.3), g["bbox_out_square_single"])
    t = bbox.bbox_xy_to_wh(torch.from_numpy(xyxy))
    assert isinstance(t, torch.Tensor)
    np.testing.assert_array_equal(t.numpy(), g["bbox_out_wh_tensor"])
    as_list = bbox.bbox_xy_to_wh([float(v) for v in xyxy[1]])
    assert isinstance(as_list, list)
    np.testing.assert_array_equal(np.array(as_list, np.float64), g["bbox_out_wh_list"])
    assert isinstance(bbox.bbox_wh_to_xy((1.0, 2.0, 3.0, 4.0)), tuple) and bbox.bbox_wh_to_xy((1.0, 2.0, 3.0, 4.0)) == (1, 2, 4, 6)


def test_signatures_mirror_the_reference():
    from homan_amd import bbox, gtmasks, maskutils
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(maskutils.add_occlusions) == ["masks", "occluder_mask", "mask_bboxes", "rend_size"]
    assert params(maskutils.add_target_hand_occlusions) == ["person_parameters", "object_parameters", "K", "square_expand",
                                                            "sample_folder", "debug", "rend_size"]
    assert params(maskutils.add_target_hand_occlusions_clip)[:4] == ["person_parameters", "object_parameters", "camintr",
                                                                     "square_expand"]
    assert params(maskutils.crop_and_resize) == ["masks", "boxes", "size", "index"]
    sig = inspect.signature(maskutils.add_target_hand_occlusions).parameters
    assert sig["square_expand"].default == 0 and sig["sample_folder"].default is None and sig["rend_size"].default == 256
    assert params(gtmasks.render_gt_masks)[:6] == ["annots", "obj_infos", "person_parameters", "sample_folder", "debug",
                                                   "image_size"]
    assert inspect.signature(gtmasks.render_gt_masks).parameters["image_size"].default == 640
    assert params(bbox.make_bbox_square) == ["bbox", "bbox_expansion"]
    assert params(bbox.bbox_xy_to_wh) == ["bbox"] and params(bbox.bbox_wh_to_xy) == ["bbox"]


def test_maskutils_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the functions run (tests/test_maskutils_gpu.py)")
    from homan_amd import gtmasks, maskutils
    g = load_golden()
    _, ins, _ = hand_cases(g)[0]
    with pytest.raises(RuntimeError):
        maskutils.crop_and_resize(ins["masks"], ins["bboxes"], 64)
    with pytest.raises(RuntimeError):
        maskutils.add_target_hand_occlusions({"masks": torch.from_numpy(ins["masks"]), "bboxes": torch.from_numpy(ins["bboxes"])},
                                             {"full_mask": torch.from_numpy(ins["full_mask"])}, ins["K"])
    with pytest.raises(RuntimeError):
        maskutils.add_occlusions([np.zeros((256, 256), bool)], torch.zeros(1, 8, 8), [np.array([0, 0, 4, 4.0])])
    with pytest.raises(RuntimeError):
        gtmasks.instance_sample_counts(torch.zeros(1, 3, 3), np.array([[0, 1, 2]]), [0, 1], np.eye(3, dtype=np.float32)[None], 32)


def test_c_abi_rejects_bad_sizes_and_nulls():
    """the three entry points check their arguments before any launch (HM_ERR_BAD_ARG = -1, HM_ERR_UNSUPPORTED = -3);
    R == 0 is not an error and launches nothing"""
    import ctypes
    from homan_amd import lib
    h = lib.lib()
    p = 1 << 20          # never dereferenced: every call below returns before a launch
    assert h.hm_mask_crop_resize(p, 0, 1, 8, 8, None, p, 0, 16, p, None) == 0
    assert h.hm_mask_crop_resize(None, 0, 1, 8, 8, None, None, 0, 16, None, None) == 0
    assert h.hm_mask_crop_resize(p, 0, 1, 8, 8, None, p, 1, 0, p, None) == -1           # S <= 0
    assert h.hm_mask_crop_resize(p, 0, 1, 8, 8, None, p, 1, -4, p, None) == -1
    assert h.hm_mask_crop_resize(p, 0, 1, 8, 8, None, p, -1, 16, p, None) == -1
    assert h.hm_mask_crop_resize(p, 0, 0, 8, 8, None, p, 1, 16, p, None) == -1
    assert h.hm_mask_crop_resize(p, 1, 1, 0, 8, None, p, 1, 16, p, None) == -1
    assert h.hm_mask_crop_resize(None, 0, 1, 8, 8, None, p, 1, 16, p, None) == -1
    assert h.hm_mask_crop_resize(p, 0, 1, 8, 8, None, None, 1, 16, p, None) == -1
    assert h.hm_mask_crop_resize(p, 0, 1, 8, 8, None, p, 1, 16, None, None) == -1
    ok = (0, p, 0, 1, None, p, 0, 1, p, 1, 8, 8, p, 1, 16, p, None)
    bad = {0: 3, 1: None, 3: 0, 5: None, 8: None, 9: -1, 10: 0, 12: None, 13: -2, 14: 0, 15: None}
    for at, value in bad.items():
        args = list(ok)
        args[at] = value
        assert h.hm_target_masks(*args) == -1, at
    no_occluder = list(ok)
    no_occluder[13] = 0                                                                   # R == 0
    assert h.hm_target_masks(*no_occluder) == 0
    starts = (ctypes.c_int * 10)(*range(10))
    sp = ctypes.cast(starts, ctypes.c_void_p)
    assert h.hm_instance_masks(None, 1, 32, 9, sp, 2, p, None) == -1
    assert h.hm_instance_masks(p, 1, 32, 9, None, 2, p, None) == -1
    assert h.hm_instance_masks(p, 0, 32, 9, sp, 2, p, None) == -1
    assert h.hm_instance_masks(p, 1, 0, 9, sp, 2, p, None) == -1
    assert h.hm_instance_masks(p, 1, 32, 9, sp, 0, p, None) == -1
    assert h.hm_instance_masks(p, 1, 32, 9, sp, 9, p, None) == -3                        # more than 8 instances
    assert h.hm_instance_masks(p, 1, 32, 1, sp, 2, p, None) == -1                        # a face range past F
