"""Target masks on the GPU (csrc/maskcrop.hip through homan_amd/maskutils.py and gtmasks.py): the crop-and-resize against
its CPU restatement with ZERO differing pixels, the fused target masks against the composition of separate crops and against
the reference's golden outputs, the clip-level call against the per-frame calls, the ground-truth instance masks against the
oracle renderer, and the rebuilt dicts through the model builder and a short fused fit."""
import copy

import numpy as np
import pytest
import torch

from homan_amd import bbox, gtmasks, maskutils, synth
from homan_amd.pose_optimization import get_K_crop_resize
from tests import maskcrop_ref
from tests.test_maskutils import hand_cases, load_golden, object_cases

pytestmark = pytest.mark.gpu


def check_crops(masks, boxes, size, index=None):
    """byte and fp32 inputs, host and device inputs: all equal to the restatement, no pixel apart"""
    want = maskcrop_ref.crop_and_resize(masks, boxes, size, index)
    m = torch.from_numpy(np.ascontiguousarray(masks))
    for given in (m.to(torch.uint8), m.to(torch.float32) * 0.25, m.to(torch.bool).cuda()):
        got = maskutils.crop_and_resize(given, torch.from_numpy(boxes), size, index)
        assert got.dtype == torch.bool and got.is_cuda == given.is_cuda
        diff = int((got.cpu().numpy() != want).sum())
        assert diff == 0, f"{diff} pixels differ"
    return want


def random_boxes(rng, n, H, W):
    """boxes at fractional coordinates: small (up-sampling), large (grids 2 and 3), partly and wholly outside"""
    c = rng.uniform([-0.2 * W, -0.2 * H], [1.2 * W, 1.2 * H], (n, 2))
    half = rng.uniform(1.0, 1.3 * max(H, W), (n, 2)) * rng.choice([0.05, 0.3, 1.0], (n, 1))
    return np.concatenate([c - half, c + half], 1).astype(np.float32)


@pytest.mark.parametrize("size", [64, 256])
def test_crop_and_resize_equals_the_restatement_on_random_masks(size):
    rng = np.random.default_rng(size)
    for H, W, n in ((96, 128, 5), (301, 277, 3)):
        masks = rng.random((n, H, W)) < 0.5                         # noise: the most ties and flips per pixel there can be
        boxes = random_boxes(rng, 12, H, W)
        boxes[0] = (0, 0, W, H)
        boxes[1] = (0, 0, 2 * size, 2 * size)                       # exact 0.5 ties
        index = rng.permutation(np.arange(12) % n)                  # several masks per launch, shuffled
        check_crops(masks, boxes, size, index)
    one = check_crops(masks[:1], boxes[2:3], size)                  # R = 1, no index
    assert one.shape == (1, size, size)
    empty = maskutils.crop_and_resize(torch.from_numpy(masks), torch.zeros(0, 4), size, index=torch.zeros(0, dtype=torch.long))
    assert empty.shape == (0, size, size) and empty.dtype == torch.bool      # R = 0


def test_crop_and_resize_ties_and_far_boxes():
    rng = np.random.default_rng(3)
    m = rng.random((1, 48, 48)) < 0.5
    want = check_crops(m, np.array([[0, 0, 48, 48]], np.float32), 24)
    blocks = m[0].reshape(24, 2, 24, 2).sum((1, 3))
    assert (blocks == 2).sum() > 100
    np.testing.assert_array_equal(want[0], blocks >= 2)
    np.testing.assert_array_equal(check_crops(m, np.array([[0, 0, 48, 48]], np.float32), 48), m)
    small = np.ones((1, 6, 5), bool)                                 # bins wider than four images: answered without the walk
    far = np.array([[-100, -3, 100, 9], [-2, -300, 7, 300], [0, 0, 568, 6], [60, 60, 90, 90], [0, 0, 5, 6]], np.float32)
    got = check_crops(small, far, 4, index=np.zeros(5, int))
    assert not got[:4].any() and got[4].all()


@pytest.mark.parametrize("size", [64, 256])
def test_crop_and_resize_on_the_golden_silhouettes(size):
    g = load_golden()
    rng = np.random.default_rng(7)
    for name, ins, want in hand_cases(g):
        masks = np.concatenate([ins["masks"], ins["full_mask"][None]])
        n, (H, W) = len(want["square_bboxes"]), masks.shape[1:]
        boxes = np.concatenate([want["square_bboxes"], want["square_bboxes"], random_boxes(rng, 4, H, W)])
        index = np.concatenate([np.arange(n), np.full(n, len(masks) - 1), rng.integers(0, len(masks), 4)])
        check_crops(masks, boxes, size, index)


def test_target_masks_are_the_composition_of_crops_and_the_golden():
    g = load_golden()
    S = int(g["meta_rend_size"])
    for name, ins, want in hand_cases(g):
        boxes = torch.from_numpy(want["square_bboxes"])
        n = len(boxes)
        for dt in (torch.uint8, torch.float32):
            hm, om = torch.from_numpy(ins["masks"]).to(dt), torch.from_numpy(ins["full_mask"]).to(dt)
            t = maskutils.crop_and_resize(hm, boxes, S).float()
            t[maskutils.crop_and_resize(om[None], boxes, S, index=torch.zeros(n, dtype=torch.long))] = -1
            fused = maskutils.target_masks(maskutils.MODE_HAND, hm, om[None], boxes, S).cpu()
            assert torch.equal(fused, t), name
            assert torch.equal(fused, torch.from_numpy(want["target_masks"]).float()), name
            # ... and through the reference's entry point
            person = {"masks": hm, "bboxes": torch.from_numpy(ins["bboxes"].copy())}
            out = maskutils.add_target_hand_occlusions(person, {"full_mask": om}, ins["K"], square_expand=float(ins["square_expand"]))
            assert out is person and out["target_masks"].dtype == torch.float32
            assert torch.equal(out["target_masks"], torch.from_numpy(want["target_masks"]).float()), name
            assert torch.equal(out["square_bboxes"], boxes), name
            torch.testing.assert_close(out["K_roi"], torch.from_numpy(want["K_roi"]))
    for name, ins, want in object_cases(g):
        boxes = torch.from_numpy(bbox.bbox_wh_to_xy(ins["mask_bboxes"]))
        occ = torch.from_numpy(ins["occluder_mask"])
        for r in range(len(boxes)):                                  # composition, maskutils.py:29-36
            o = maskutils.crop_and_resize(occ, boxes[r:r + 1].repeat(len(occ), 1), S)
            t = torch.from_numpy(ins["masks"][r] != 0).float()
            t[o.sum(0) > 0] = -1
            t[torch.from_numpy(ins["masks"][r] != 0)] = 1
            assert torch.equal(t, torch.from_numpy(want[r]).float()), name
        got = maskutils.add_occlusions([m != 0 for m in ins["masks"]], occ.float(), list(ins["mask_bboxes"]))
        assert len(got) == len(want) and all(a.dtype == np.float32 and a.shape == (S, S) for a in got)
        np.testing.assert_array_equal(np.stack(got), want.astype(np.float32), err_msg=name)
    # the third mode: crop(target) - (any cropped occluder), values in {-1, 0, 1}
    name, ins, want = hand_cases(g)[-1]
    hm, boxes = torch.from_numpy(ins["masks"]), torch.from_numpy(want["square_bboxes"])
    om = torch.from_numpy(ins["full_mask"])[None]
    minus = maskutils.target_masks(maskutils.MODE_MINUS, om, hm, boxes[:1], S, target_index=[0],
                                   occluder_index=[[0, -1, 1]]).cpu()
    sep = maskutils.crop_and_resize(om, boxes[:1], S).float() \
        - (maskutils.crop_and_resize(hm[:2], boxes[:1].repeat(2, 1), S).sum(0, keepdim=True) > 0).float()
    assert torch.equal(minus, sep) and set(minus.unique().tolist()) <= {-1.0, 0.0, 1.0}


def _clip_dicts(hands, image_size=64, rend_size=64, frames=4, seed=3):
    """a synthetic clip and the inputs of the mask stage made from it: per-frame `bboxes` of the hands (tight boxes of their
    instance masks) and the object's square box"""
    sil_fn, hand_fn = synth.hip_clip_fns()
    clip = synth.make_clip(seed=seed, frames=frames, rend_size=rend_size, image_size=image_size, obj="cube", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn, hands=hands)

    def tight(mask):
        ys, xs = np.nonzero(mask.numpy())
        return [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1] if len(xs) else [4, 4, 20, 20]
    for p in clip["person_parameters"]:
        p["bboxes"] = torch.tensor([tight(m) for m in p["masks"]], dtype=torch.float32)
    K_px = torch.from_numpy(clip["camintr"]).clone()
    K_px[:, :2] *= image_size
    return clip, K_px


@pytest.mark.parametrize("hands", [("right",), ("right", "left")])
def test_clip_call_equals_the_per_frame_calls(hands):
    clip, K_px = _clip_dicts(hands)
    per_frame = copy.deepcopy(clip["person_parameters"])
    for p, o, K in zip(per_frame, clip["object_parameters"], K_px):
        maskutils.add_target_hand_occlusions(p, o, K.numpy(), square_expand=0.3, rend_size=64)
    whole = copy.deepcopy(clip["person_parameters"])
    maskutils.add_target_hand_occlusions_clip(whole, clip["object_parameters"], K_px, square_expand=0.3, rend_size=64)
    resident = [{k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in p.items()} for p in clip["person_parameters"]]
    maskutils.add_target_hand_occlusions_clip(resident, [{"full_mask": o["full_mask"].cuda()} for o in clip["object_parameters"]],
                                              K_px.cuda(), square_expand=0.3, rend_size=64)
    for a, b, c in zip(per_frame, whole, resident):
        for k in ("target_masks", "K_roi", "square_bboxes"):
            assert a[k].shape[0] == len(hands) and a[k].dtype == torch.float32
            assert torch.equal(a[k], b[k]), k
            assert c[k].is_cuda and torch.equal(a[k], c[k].cpu()), k
        want = maskcrop_ref.crop_and_resize(a["masks"].numpy(), a["square_bboxes"].numpy(), 64)
        assert ((a["target_masks"] == 1).numpy() <= want).all() and (a["target_masks"] >= -1).all()


def _gt_scene(hands, image_size, frames=2):
    """annotations in the reference's layout (camera K in pixels, hands then objects as camera-space meshes) from a
    synthetic clip; a second hand = the first one's mesh moved to the other side of the object"""
    clip, K_px = _clip_dicts(("right",), image_size=image_size, rend_size=64, frames=frames)
    hv = clip["gt"]["verts_hand"]
    hf = clip["person_parameters"][0]["faces"][0].numpy()
    hand_list = [{"verts3d": hv.numpy(), "faces": np.repeat(hf[None], frames, 0)}]
    if len(hands) == 2:
        mirrored = hv * torch.tensor([-1.0, 1.0, 1.0]) + torch.tensor([0.0, 0.01, 0.03])
        hand_list.append({"verts3d": mirrored.numpy(), "faces": np.repeat(hf[None, :, ::-1].copy(), frames, 0)})
    annots = {"camera": {"K": K_px.numpy()}, "hands": hand_list,
              "objects": [{"verts3d": clip["gt"]["verts_object"].numpy(), "faces": clip["objfaces"].numpy()}]}
    return clip, K_px, annots


def _oracle_instances(annots, image_size):
    """`renders` of reference gtmasks.py:32-77 with the oracle renderer: one-hot colour per instance, ambient 1, directional 0"""
    from oracle import nmr
    insts = annots["hands"] + annots["objects"]
    verts = torch.cat([torch.from_numpy(i["verts3d"]) for i in insts], 1)
    off = np.cumsum([0] + [i["verts3d"].shape[1] for i in insts])
    faces = torch.cat([torch.from_numpy(i["faces"].astype(np.int64)) + int(o) for i, o in zip(insts, off)], 1)
    tex = torch.cat([torch.eye(3)[k].view(1, 1, 1, 1, 1, 3).repeat(verts.shape[0], i["faces"].shape[1], 1, 1, 1, 1)
                     for k, i in enumerate(insts)], 1)
    K_nc = torch.from_numpy(annots["camera"]["K"]).clone()
    K_nc[:, :2] = 1 / image_size * K_nc[:, :2]
    r = nmr.Renderer(image_size=image_size, K=K_nc, R=torch.eye(3)[None], t=torch.zeros(1, 3), orig_size=1)
    r.light_intensity_direction, r.light_intensity_ambient = 0, 1
    return r(verts, faces, tex, K=K_nc)[0][:, :len(insts)]


@pytest.mark.parametrize("hands,image_size", [(("right",), 64), (("right", "left"), 96)])
def test_render_gt_masks_equals_the_oracle_and_keeps_the_dict_layout(hands, image_size):
    clip, K_px, annots = _gt_scene(hands, image_size)
    B, h, S = len(clip["person_parameters"]), len(hands), 64
    renders = _oracle_instances(annots, image_size)
    obj_infos, persons = [], []
    for b in range(B):
        ys, xs = np.nonzero(renders[b, h].numpy() > 0)
        tight = np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float32)
        obj_infos.append({"square_bbox": bbox.make_bbox_square(bbox.bbox_xy_to_wh(tight), 0.3),
                          "target_crop_mask": np.full((S, S), 7, np.float32), "crop_mask": np.zeros((S, S), bool),
                          "full_mask": np.zeros((image_size, image_size), bool)})
        boxes = torch.tensor([[10, 10, 50, 50.0]] * h)
        persons.append({"bboxes": boxes, "masks": torch.full((h, image_size, image_size), 7.0)} if b else {"bboxes": boxes})
    assert gtmasks.render_gt_masks(annots, obj_infos, persons, image_size=image_size, rend_size=S) is None
    for b in range(B):
        got_h, got_o = persons[b]["masks"], obj_infos[b]["full_mask"]
        assert got_h.shape == (h, image_size, image_size) and got_h.dtype == torch.float32
        assert got_o.shape == (image_size, image_size) and got_o.dtype == np.bool_
        assert torch.equal(got_h.cpu(), renders[b, :h])                        # the anti-aliased values, not only > 0
        np.testing.assert_array_equal(got_o, renders[b, h].numpy() > 0)
        assert (got_h.cpu() > 0).any() and got_o.any()
        # the crops: the restatement on the masks that were written
        box = bbox.bbox_wh_to_xy(obj_infos[b]["square_bbox"].astype(np.float32))[None]
        oc = maskcrop_ref.crop_and_resize(got_o[None], box, S)[0]
        hc = maskcrop_ref.crop_and_resize((got_h.cpu() > 0).numpy(), np.repeat(box, h, 0), S)
        tcm = obj_infos[b]["target_crop_mask"]
        assert tcm.shape == (S, S) and tcm.dtype == np.float32 and obj_infos[b]["crop_mask"].dtype == np.bool_
        np.testing.assert_array_equal(obj_infos[b]["crop_mask"], oc)
        np.testing.assert_array_equal(tcm, oc.astype(np.float32) - (hc.sum(0) > 0).astype(np.float32))
        assert set(np.unique(tcm).tolist()) <= {-1.0, 0.0, 1.0}


def test_rebuilt_dicts_fit_end_to_end():
    """ground-truth meshes -> render_gt_masks -> add_target_hand_occlusions_clip -> build_model -> 4 fused steps: the stage's
    output is what the built stages accept, with the shapes and dtypes of the clip's own dicts"""
    from homan_amd.jointopt import FusedStepper, build_model
    from homan_amd.mano_assets import synthetic_mano
    image_size = S = 64
    clip, K_px, annots = _gt_scene(("right",), image_size, frames=4)
    persons, objects = copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"])
    obj_infos = []
    for o in objects:
        ys, xs = np.nonzero(o["full_mask"].numpy())
        tight = np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float32)
        obj_infos.append({"square_bbox": bbox.make_bbox_square(bbox.bbox_xy_to_wh(tight), 0.3),
                          "target_crop_mask": np.zeros((S, S), np.float32), "crop_mask": np.zeros((S, S), bool),
                          "full_mask": np.zeros((image_size, image_size), bool)})
    for p in persons:
        del p["target_masks"], p["K_roi"]
    gtmasks.render_gt_masks(annots, obj_infos, persons, image_size=image_size, rend_size=S)
    maskutils.add_target_hand_occlusions_clip(persons, [{"full_mask": torch.from_numpy(i["full_mask"]).float()} for i in obj_infos],
                                              K_px, square_expand=0.3, rend_size=S)
    for o, info, K in zip(objects, obj_infos, K_px):
        box = torch.from_numpy(bbox.bbox_wh_to_xy(info["square_bbox"].astype(np.float32)))[None]
        K_roi = get_K_crop_resize(K[None], box, [S])
        K_roi[:, :2] = K_roi[:, :2] / S
        o.update(target_masks=torch.from_numpy(info["target_crop_mask"])[None], K_roi=K_roi[:, None],
                 full_mask=torch.from_numpy(info["full_mask"]).float())
    for mine, theirs in ((persons, clip["person_parameters"]), (objects, clip["object_parameters"])):
        for a, b in zip(mine, theirs):
            for k in ("target_masks", "K_roi", "masks", "full_mask"):
                if k in b:
                    assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].device == b[k].device, k
            assert set(a["target_masks"].unique().tolist()) <= {-1.0, 0.0, 1.0}
    # the rebuilt hand target covers the clip's own (both are the same hand seen through a box around it)
    assert all((p["target_masks"] == 1).any() for p in persons)
    mano = synthetic_mano(0)
    model = build_model(persons, objects, objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"],
                        optimize_mano=True, image_size=image_size, mano_model=mano, rend_size=S, sync_metrics=False)
    stepper = FusedStepper([model], dict(synth.STEP2_LOSS_WEIGHTS), 1e-2, 4)
    stepper.run(4)
    evo = stepper.loss_evolution(4, clip=0)
    assert np.isfinite(evo["loss"]).all() and len(evo["loss"]) == 4
