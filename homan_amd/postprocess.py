"""`joint_fit.pt` -> camera-space hand vertices, 21 joints and the object pose: reference homan/postprocess.py:16-136 as
executed, on the MANO and rigid kernels for all frames and hands of a sample at once, with one host sync.

What the reference does and this keeps: hand `i` owns rows `i::hand_nb` of every per-row tensor; a two-hand sample is
relabelled ["left", "right"] (:30-31); the 16 posed joints go through the hand's rigid transform, the five finger tips are
read off the TRANSFORMED vertices (745, 317, 444, 556, 673) and the 21 are put in the order of `HOMan.get_joints_hand`
(:66-70); `hand_verts3d` / `hand_joints3d` / `side` are those of the LAST hand (the loop variables after :33-70);
`obj_scale = scale * int_scales_object.item()` with `scale` the first element of a list / tuple / array, 1 when absent.
Divergence: the reference's `isinstance(scale, (..., torch.tensor, ...))` (:105) raises a TypeError on a bare float, since
`torch.tensor` is a function; a plain number is accepted here and used as it is.  There is no CPU path.
"""
import numpy as np
import torch

from . import lib, ops

TIP_VERTS = (745, 317, 444, 556, 673)
JOINT_ORDER = (0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20)


def _rigid(mesh, rot6d, trans, scale, abs_scale, want_rot=False):
    """hm_rigid_fwd without autograd: (s * mesh) @ R(rot6d) + trans, and R (N,3,3) when asked for"""
    N, V = mesh.shape[0], mesh.shape[1]
    verts = torch.empty_like(mesh)
    rotmat = torch.empty(N, 3, 3, device=mesh.device) if want_rot else None
    lib.check(lib.lib().hm_rigid_fwd(lib.ptr(mesh), lib.ptr(rot6d), lib.ptr(trans), lib.ptr(scale), int(abs_scale), N, V,
                                     lib.ptr(rotmat), lib.ptr(verts), lib.stream()), "hm_rigid_fwd")
    return verts, rotmat


def _mano_context(mano_model, side):
    if side not in ("right", "left"):
        raise ValueError(f"{side} not in [left|right]")
    return mano_model.ctx_mean if side == "right" else mano_model._left_ctx(False)


def fit_geometry(state_dict, hand_sides, mano_model=None):
    """The geometry of a fit as DEVICE tensors (no host sync): {"hand_verts" (hand_nb, B, 778, 3), "hand_joints"
    (hand_nb, B, 21, 3), "obj_rot" (B,3,3), "obj_trans" (B,1,3), "obj_verts" (B,Vo,3) - the state's own mesh under the object's
    pose, as HOMan.get_verts_object -, "int_scales_object" (1), "hand_sides"}.  B = frames; hand i is rows i::hand_nb."""
    if not torch.cuda.is_available():
        raise lib.HomanAmdError("homan_amd.postprocess needs the GPU (there is no CPU fallback)")
    if mano_model is None:
        from .manomodel import ManoModel
        mano_model = ManoModel("extra_data/mano", pca_comps=16)
    hand_sides = list(hand_sides)
    hand_nb = len(hand_sides)
    if hand_nb == 2:
        hand_sides = ["left", "right"]
    dev = torch.device(mano_model.device)
    sd = {k: state_dict[k].detach().to(device=dev, dtype=torch.float32)
          for k in ("mano_pca_pose", "mano_rot", "mano_betas", "mano_trans", "rotations_hand", "translations_hand",
                    "int_scales_hand", "int_scales_object", "translations_object", "rotations_object", "verts_object_og")}
    tips, order = list(TIP_VERTS), list(JOINT_ORDER)
    with torch.no_grad(), torch.cuda.device(dev):
        hand_scale = sd["int_scales_hand"].reshape(-1)[:1].contiguous()
        all_verts, all_joints = [], []
        for i, side in enumerate(hand_sides):
            rows = lambda key: sd[key][i::hand_nb].contiguous()         # noqa: E731
            verts_og, joints_og = ops.mano_joints(rows("mano_pca_pose"), rows("mano_rot"), rows("mano_betas"),
                                                  rows("mano_trans").reshape(-1, 3), _mano_context(mano_model, side))
            rot6d, trans = rows("rotations_hand").reshape(-1, 3, 2), rows("translations_hand").reshape(-1, 3)
            verts = _rigid(verts_og, rot6d, trans, hand_scale, False)[0]
            joints = _rigid(joints_og, rot6d, trans, hand_scale, False)[0]
            all_verts.append(verts)
            all_joints.append(torch.cat([joints, verts[:, tips]], 1)[:, order])
        obj_trans = sd["translations_object"].contiguous()
        obj_scale = sd["int_scales_object"].reshape(-1)[:1].contiguous()
        obj_verts, obj_rot = _rigid(sd["verts_object_og"].contiguous(), sd["rotations_object"].reshape(-1, 3, 2).contiguous(),
                                    obj_trans.reshape(-1, 3), obj_scale, True, want_rot=True)
    return {"hand_verts": torch.stack(all_verts), "hand_joints": torch.stack(all_joints), "obj_rot": obj_rot,
            "obj_trans": obj_trans, "obj_verts": obj_verts, "int_scales_object": obj_scale, "hand_sides": hand_sides}


def _numpify(value):
    return value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)


def post_process(sample_info, state_dict, frame_nb=10, mano_model=None):
    """reference postprocess.py:16-136 -> (train_infos, seq_idx, frame_idxs): one dict per frame with the reference's keys
    (numpy fp32 arrays): all_hand_verts3d [hand_nb x (778,3)], hand_verts3d (778,3) and hand_joints3d (21,3) of the LAST hand,
    camintr, img_path, side, obj_path, obj_rot (3,3), obj_trans (1,3), obj_scale (float), hand_sides."""
    hand_sides = [hand["label"].split("_")[0] for hand in sample_info["hands"]]
    geo = fit_geometry(state_dict, hand_sides, mano_model)
    parts = [geo[k] for k in ("hand_verts", "hand_joints", "obj_rot", "obj_trans", "int_scales_object")]
    flat = torch.cat([p.reshape(-1) for p in parts]).cpu().numpy()                 # the one host sync
    host, at = [], 0
    for p in parts:
        host.append(flat[at:at + p.numel()].reshape(tuple(p.shape)))
        at += p.numel()
    all_verts, all_joints, obj_rot, obj_trans, obj_scales = host
    hand_sides = geo["hand_sides"]
    camintrs = _numpify(sample_info["camera"]["K"])
    obj = sample_info["objects"][0]
    scale = obj["scale"] if "scale" in obj else 1
    if isinstance(scale, (list, tuple, torch.Tensor, np.ndarray)):
        scale = scale[0]
    obj_scale = scale * obj_scales.item()
    img_path, obj_path = sample_info["images"], obj["path"]
    train_infos = []
    for f in range(frame_nb):
        train_infos.append({
            "all_hand_verts3d": [hand_v[f].copy() for hand_v in all_verts],
            "hand_verts3d": all_verts[-1][f].copy(),
            "hand_joints3d": all_joints[-1][f].copy(),
            "camintr": camintrs[f],
            "img_path": img_path[f],
            "side": hand_sides[-1],
            "obj_path": obj_path[f],
            "obj_rot": obj_rot[f].copy(),
            "obj_trans": obj_trans[f].copy(),
            "obj_scale": obj_scale,
            "hand_sides": hand_sides,
        })
    return train_infos, sample_info["seq_idx"], sample_info["frame_idxs"]
