"""homan_amd.homan.clip_tensors: the one conversion of a clip's raw inputs into the tensors a model stores (what HOMan.__init__
registers and HOMan.load_clip copies in place), against the CPU oracle's constructor.  No device."""
import copy

import pytest
import torch

from tests import util

DEFAULT_K = [[[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]]]       # reference homan/homan.py:156-158


@pytest.fixture(scope="module")
def clips(mano_model):
    from homan_amd import synth
    sil_fn, hand_fn = util.oracle_clip_fns(mano_model)
    make = lambda **kw: synth.make_clip(seed=5, frames=3, rend_size=32, image_size=32, obj="cube", silhouette_fn=sil_fn,
                                        hand_verts_fn=hand_fn, **kw)
    return {"one": make(), "two": make(hands=("right", "left"))}


def _inputs(clip):
    from homan_amd.jointopt import collate_inputs
    return collate_inputs(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]), clip["objvertices"],
                          clip["objfaces"])


def _as_6d(kw):
    from homan_amd.homan import matrix_to_rot6d
    return dict(kw, rotations_object=matrix_to_rot6d(kw["rotations_object"]).clone(),
                rotations_hand=matrix_to_rot6d(kw["rotations_hand"]).clone())


VARIANTS = {
    "matrices": lambda kw, K: dict(kw, camintr=K),
    "rot6d": lambda kw, K: dict(_as_6d(kw), camintr=K),
    "camintr_none": lambda kw, K: dict(kw, camintr=None),
    "camintr_3x3": lambda kw, K: dict(kw, camintr=K[0]),
    "camintr_1x3x3": lambda kw, K: dict(kw, camintr=K[:1]),
    "camintr_Bx3x3": lambda kw, K: dict(kw, camintr=K * torch.linspace(1.0, 1.2, K.shape[0])[:, None, None]),
    "mask_2d": lambda kw, K: dict(kw, camintr=K, masks_object=kw["masks_object"][0]),
}


@pytest.mark.parametrize("hands", ["one", "two"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_clip_tensors_match_the_oracle_model(variant, hands, clips, mano_model):
    """every name both hold is torch.equal (the oracle stores the instance masks as bool: compared as != 0).  Two things the
    oracle's constructor does differently are bridged HERE, not in the code under test: it cannot take camintr=None (it is given
    the reference's default), and like the reference it leaves one intrinsic matrix as (1,3,3) where the model stores it per
    frame (compared expanded; clip_tensors' own shape is asserted)."""
    from homan_amd.homan import clip_tensors
    from oracle.model import OracleHOMan
    clip = clips[hands]
    kw = VARIANTS[variant](_inputs(clip), torch.as_tensor(clip["camintr"]).clone())
    frames = kw["translations_object"].shape[0]
    if variant == "mask_2d":      # (one frame's mask for a whole clip is no real input: what is checked is the unsqueeze)
        assert kw["masks_object"].dim() == 2
    got = clip_tensors(**copy.deepcopy(kw))
    assert all(t.device.type == "cpu" for t in got.values())
    okw = copy.deepcopy(kw)
    if okw["camintr"] is None:
        okw["camintr"] = torch.tensor(DEFAULT_K)
    om = OracleHOMan(**okw, optimize_mano=True, image_size=32, mano_model=mano_model, rend_size=32)
    want = dict(list(om.named_parameters()) + list(om.named_buffers()))
    shared = sorted(set(got) & set(want))
    assert set(shared) >= {"rotations_object", "rotations_hand", "cams_hand", "mano_betas", "mano_trans", "int_scales_object",
                           "int_scales_hand", "int_scale_object_mean", "int_scale_hand_mean", "ref_mask_object", "keep_mask_hand",
                           "camintr_rois_object", "camintr_rois_hand", "camintr", "masks_object", "masks_human"}
    assert tuple(got["camintr"].shape) == (frames, 3, 3) and got["masks_object"].dim() == 3
    assert got["masks_object"].dtype == kw["masks_object"].dtype
    assert got["rotations_object"].is_contiguous() and got["rotations_hand"].is_contiguous()
    for name in shared:
        a, b = got[name], want[name].detach()
        if name.startswith("masks_"):
            a = a != 0
        elif name == "camintr":
            b = b.expand_as(a)
        assert a.dtype == b.dtype and torch.equal(a, b), name


def test_ortho_refusals_and_persp_default(clips):
    from homan_amd.homan import clip_tensors
    kw = _inputs(clips["one"])
    with pytest.raises(ValueError, match="needs cams_hand"):
        clip_tensors(**dict(kw, cams_hand=None), hand_proj_mode="ortho")
    cams = kw["cams_hand"].clone() + 1.0
    clip_tensors(**dict(kw, cams_hand=cams), hand_proj_mode="ortho")
    cams[1, 0] = 0.0
    with pytest.raises(ValueError, match="zero scale"):
        clip_tensors(**dict(kw, cams_hand=cams), hand_proj_mode="ortho")
    assert torch.equal(clip_tensors(**dict(kw, cams_hand=cams))["cams_hand"], cams)         # persp: any camera is stored
    got = clip_tensors(**dict(kw, cams_hand=None))["cams_hand"]
    assert got.shape == (kw["translations_hand"].shape[0], 3) and not got.any()


def test_every_batched_name_is_a_clip_tensor(clips):
    from homan_amd import clipbatch
    from homan_amd.homan import clip_tensors
    got = clip_tensors(**_inputs(clips["one"]))
    assert set(clipbatch._PER_FRAME + clipbatch._PER_CLIP) <= set(got)
