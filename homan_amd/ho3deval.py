"""Sequence evaluation and HO-3D export of fitted key frames: what reference evalho3drecons.py does after `post_process`
(:99-239, :310-311) with homan/eval/ho3devalutils.py, along the time axis on the GPU.

The reference script runs at import and needs the datasets; its behaviour is restated here from its line numbers:
  - `interpolate_res` (ho3devalutils.py:53-96) blends the key-frame results of a sequence over every frame: one launch of
    `hm_keyframe_interp` per key instead of a Python walk (csrc/seqinterp.hip, bit-equal on fp32 keys);
  - every frame is scored (evalho3drecons.py:120-190): object vertex distance and ADD-S through `ops.cloud_metrics`
    (prediction first, ground truth second, :131-133), hand-root error (:160), penetration depth and contact of the hand in
    the object's SDF (:176-188) - in chunks of frames, one SDF scene per chunk size instead of two grids per frame;
  - `dump` (ho3devalutils.py:16-33) writes the `pred.json` / zip of the HO-3D server;
  - beyond the reference: with the ground-truth hand, `evaluate_sequence_protocol` adds what that server scores (aligned
    joint and mesh errors, F-scores; homan_amd/handmetrics.py) and `protocol_summary` forms its table;
    `evaluate_sequence_plausibility` scores what needs no ground truth: intersection volume, penetration depth, contact.
Predictions are moved to the HO-3D frame by right-multiplying with camextr = diag(1, -1, -1) (:101), a sign flip of y and z;
the 21 joints go from this project's order to HO-3D's with `UNORDER_IDXS` (:105-107, row 12 is named twice).
Divergences: a sequence with ONE key frame holds that key over all frames (the reference raises a NameError); a zero
coordinate keeps (x) or flips (y, z) its sign, where numpy's `.dot` gives it the sign the other coordinates' zero products
leave - equal as numbers; `dump` copies to `copy_to` only when given (the reference always writes ./pred.zip) and writes the
zip with `zipfile` instead of calling the `zip` program.  There is no CPU path for the interpolation and the scores.
"""
import json
import os
import shutil
import zipfile
from collections import defaultdict

import numpy as np
import torch

from . import constants, handmetrics, lib, meshutils, ops, pointmetrics

CAMEXTR_SIGNS = (1.0, -1.0, -1.0)                # diagonal of evalho3drecons.py:101
UNORDER_IDXS = (0, 5, 6, 7, 10, 11, 12, 17, 18, 19, 13, 14, 15, 1, 2, 3, 4, 8, 12, 16, 20)       # ours -> HO-3D (:105-107)
INTERP_KEYS = ("hand_verts3d", "hand_joints3d", "obj_verts3d", "hand_roots")
UNSEEN_FROM_HO3D = 7694                          # "AP objects start at index 7694" (:140-141)


def dump(pred_out_path, xyz_pred_list, verts_pred_list, codalab=True, copy_to=None):
    """ho3devalutils.py:16-33: [joints, vertices] rounded to 4 decimals as JSON; codalab: a zip beside it that holds exactly
    that file (as `zip -j`), copied to `copy_to` when given.  Returns the zip's path (None without codalab)."""
    xyz_pred_list = [np.asarray(x).round(4).tolist() for x in xyz_pred_list]
    verts_pred_list = [np.asarray(x).round(4).tolist() for x in verts_pred_list]
    with open(pred_out_path, "w") as fo:
        json.dump([xyz_pred_list, verts_pred_list], fo)
    if not codalab:
        return None
    save_zip_path = pred_out_path.replace(".json", ".zip")
    with zipfile.ZipFile(save_zip_path, "w", zipfile.ZIP_DEFLATED) as zf:
        zf.write(pred_out_path, arcname=os.path.basename(pred_out_path))
    if copy_to is not None:
        shutil.copy(save_zip_path, copy_to)
    return save_zip_path


def extend_res(seq_res, frame_nb, keys=("hand_verts3d", "hand_joints3d", "obj_verts3d", "hand_roots", "obj_faces")):
    """ho3devalutils.py:36-50: a sequence fitted at EVERY frame, regrouped per key (img_paths gains one entry per key and
    frame, as the reference builds it)."""
    img_root = os.path.dirname(seq_res[0]["img_path"])
    full_res = defaultdict(list)
    for frame_idx in range(frame_nb):
        for key in keys:
            full_res[key].append(seq_res[frame_idx][key])
            full_res["img_paths"].append(os.path.join(img_root, f"{frame_idx:04d}.png"))
    return dict(full_res)


def _keys_on_device(seq_res, key):
    """(sorted key frames, (K,N,3) fp32 device tensor of seq_res[frame][key])"""
    if not torch.cuda.is_available():
        raise lib.HomanAmdError("homan_amd.ho3deval needs the GPU (there is no CPU fallback)")
    seq_keys = sorted(seq_res.keys())
    vals = []
    for frame in seq_keys:
        val = seq_res[frame][key]
        val = val.detach().cpu().numpy() if isinstance(val, torch.Tensor) else np.asarray(val)
        if val.dtype != np.float32:
            # (the reference blends whatever dtype it is given; its own results are fp32 and the kernel is pinned to those)
            raise ValueError(f"{key} at key frame {frame}: expected float32 (the reference's results), got {val.dtype}")
        if val.ndim != 2 or val.shape[1] != 3:
            raise ValueError(f"{key} at key frame {frame}: expected (N, 3), got {val.shape}")
        vals.append(val)
    return seq_keys, torch.from_numpy(np.stack(vals)).cuda()


def interpolate_sequence(seq_res, frame_nb, key, signs=(1.0, 1.0, 1.0), gather=None):
    """seq_res {key frame: {key: (N,3) fp32}} -> device tensor (frame_nb, M, 3) fp32 = the reference's
    `interpolate_res(...)[key][f].dot(diag(signs))[gather].astype(np.float32)` for every frame f."""
    seq_keys, vals = _keys_on_device(seq_res, key)
    return ops.keyframe_interp(vals, seq_keys, frame_nb, gather=gather, signs=signs, out_dtype=torch.float32)


def interpolate_res(seq_res, frame_nb, keys=INTERP_KEYS):
    """ho3devalutils.py:53-96 -> {key: [frame_nb arrays (N,3) float64], "img_paths": [...]}.  img_paths as the reference
    builds it: one entry per frame before the last key frame, then ONE more (so last key frame + 1 entries)."""
    interp_res = {}
    img_root = os.path.dirname(seq_res[0]["img_path"])
    outs = []
    for key in keys:
        seq_keys, vals = _keys_on_device(seq_res, key)
        outs.append(ops.keyframe_interp(vals, seq_keys, frame_nb, out_dtype=torch.float64))
    for key_idx, (key, out) in enumerate(zip(keys, outs)):
        interp_res[key] = list(out.cpu().numpy())
        if key_idx == 0:
            interp_res["img_paths"] = [os.path.join(img_root, f"{f:04d}.png") for f in range(seq_keys[-1] + 1)]
    return interp_res


def _faces(faces):
    """(F,3) or (1,F,3) faces -> (1,F,3) int64 CPU tensor"""
    faces = torch.as_tensor(np.asarray(faces.cpu() if isinstance(faces, torch.Tensor) else faces)).long()
    return faces.reshape(1, -1, 3)


def _hand_gt(gt, name, pred):
    """ground-truth joints / vertices of every frame -> fp32 on the prediction's device, shaped like it (None stays None)"""
    if gt is None:
        return None
    gt = torch.as_tensor(np.asarray(gt.cpu() if isinstance(gt, torch.Tensor) else gt))
    if tuple(gt.shape) != tuple(pred.shape):
        raise ValueError(f"{name}: expected {tuple(pred.shape)}, got {tuple(gt.shape)}")
    return gt.to(device=pred.device, dtype=torch.float32).contiguous()


def _evaluate_sequence(seq_res, frame_nb, gt_obj_verts, gt_hand_roots, obj_faces, mano_faces_closed, chunk, hand_gt=None):
    """evaluate_sequence; hand_gt = (gt_hand_joints or None, gt_hand_verts or None, anchors) adds the protocol's per-frame arrays"""
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    obj = interpolate_sequence(seq_res, frame_nb, "obj_verts3d", CAMEXTR_SIGNS)
    verts = interpolate_sequence(seq_res, frame_nb, "hand_verts3d", CAMEXTR_SIGNS)
    joints = interpolate_sequence(seq_res, frame_nb, "hand_joints3d", CAMEXTR_SIGNS, UNORDER_IDXS)
    dev = obj.device
    gt_obj = torch.as_tensor(np.asarray(gt_obj_verts.cpu() if isinstance(gt_obj_verts, torch.Tensor) else gt_obj_verts))
    if gt_obj.dim() != 3 or gt_obj.shape[0] != frame_nb or gt_obj.shape[2] != 3:
        raise ValueError(f"gt_obj_verts: expected ({frame_nb}, Vg, 3), got {tuple(gt_obj.shape)}")
    gt_obj = gt_obj.to(device=dev, dtype=torch.float32).contiguous()       # (`torch.Tensor(gt_objverts).float()`, :133)
    hand_faces, object_faces = _faces(mano_faces_closed)[0], _faces(obj_faces)[0]
    gt_joints, gt_verts, anchors = hand_gt if hand_gt is not None else (None, None, None)
    gt_joints = _hand_gt(gt_joints, "gt_hand_joints", joints)
    gt_verts = _hand_gt(gt_verts, "gt_hand_verts", verts)
    scenes, tabs, deepest, protocol = {}, [], [], defaultdict(list)
    with torch.cuda.device(dev):
        for f0 in range(0, frame_nb, chunk):
            n = min(chunk, frame_nb - f0)
            tabs.append(ops.cloud_metrics(obj[f0:f0 + n], gt_obj[f0:f0 + n]))
            if n not in scenes:
                scenes[n] = ops.CollisionContext(hand_faces.numpy(), object_faces, n, verts.shape[1], obj.shape[1], dev)
            depth = ops.collision_dist_values(verts[f0:f0 + n], obj[f0:f0 + n], scenes[n], constants.SDF_SCALE_FACTOR)[(1, 0)]
            deepest.append(depth.amax(dim=1))
            if gt_joints is not None:
                errs, _ = handmetrics.frame_errors(gt_joints[f0:f0 + n], joints[f0:f0 + n], anchors)
                for tag, err in errs.items():
                    protocol[f"joint_err{tag}"].append(err)
            if gt_verts is not None:
                errs, aligned = handmetrics.frame_errors(gt_verts[f0:f0 + n], verts[f0:f0 + n], scale_trans=False)
                for tag, err in errs.items():
                    protocol[f"mesh_err{tag}"].append(err)
                for prefix, pred in (("f", verts[f0:f0 + n]), ("f_al", aligned)):
                    tab = handmetrics.frame_fscores(gt_verts[f0:f0 + n], pred, handmetrics.F_THRESHOLDS)
                    for t, th in enumerate(handmetrics.F_THRESHOLDS):
                        protocol[f"{prefix}@{round(th * 1000):d}"].append(tab[:, t])
        tab = torch.cat(tabs)
        same_size = obj.shape[1] == gt_obj.shape[1]
        scores = torch.stack([tab[:, 3] if same_size else tab[:, 2], tab[:, 2], torch.cat(deepest).double()]).cpu().numpy()
        export_joints, export_verts = joints.cpu().numpy(), verts.cpu().numpy()
        protocol = {key: torch.cat(parts).cpu().numpy() for key, parts in protocol.items()}
    roots = np.asarray(gt_hand_roots.cpu() if isinstance(gt_hand_roots, torch.Tensor) else gt_hand_roots).reshape(frame_nb, -1, 3)
    hand_root = np.linalg.norm(export_joints[:, 0] - roots[:, 0], axis=-1).astype(np.float64)
    res = {"obj_dist": scores[0], "obj_add-s": scores[1], "hand_root": hand_root, "pen_depths": scores[2],
            "has_contact": (scores[2] > 0).astype(np.float64), "export_joints": export_joints, "export_verts": export_verts}
    res.update(protocol)
    return res


def evaluate_sequence(seq_res, frame_nb, gt_obj_verts, gt_hand_roots, obj_faces, mano_faces_closed, chunk=512):
    """Scores of every frame of one sequence (evalho3drecons.py:120-190) and its export arrays.

    seq_res: {key frame: {"hand_verts3d" (778,3), "hand_joints3d" (21,3), "obj_verts3d" (Vo,3)}} fp32, camera frame;
    gt_obj_verts (frame_nb, Vg, 3) and gt_hand_roots (frame_nb, 1, 3) or (frame_nb, 3): ground truth in the HO-3D frame,
    i.e. after the script's `.dot(camextr)` (:122, :150); obj_faces (Fo,3), mano_faces_closed (Fh,3): topology of the
    predicted object mesh and of the closed hand.  Frames are scored `chunk` at a time; a frame's values do not depend on
    the chunk size.  Returns per-frame float64 arrays "obj_dist", "obj_add-s", "hand_root", "pen_depths", "has_contact"
    (0 / 1) and fp32 "export_joints" (frame_nb, 21, 3) in HO-3D order, "export_verts" (frame_nb, 778, 3), both flipped:
    the lists `dump` takes."""
    return _evaluate_sequence(seq_res, frame_nb, gt_obj_verts, gt_hand_roots, obj_faces, mano_faces_closed, chunk)


def evaluate_sequence_plausibility(seq_res, frame_nb, obj_faces, mano_faces_closed, chunk=512, voxel=0.005):
    """Physical-plausibility scores of every interpolated frame of one sequence; no ground truth is needed.  seq_res, obj_faces,
    mano_faces_closed and chunk as `evaluate_sequence` (the frames are interpolated and flipped the same way) ->
    "inter_volume" (frame_nb,) float64, m^3: hand-object intersection volume on the world-anchored lattice of pitch `voxel`
    (`pointmetrics.get_volume_metrics`); "pen_depth" and "has_contact" (0 / 1), float64: what `pointmetrics.get_inter_metrics`
    gives, the "pen_depths" / "has_contact" of `evaluate_sequence`; and their means over the frames, "inter_volume_mean",
    "pen_depth_mean", "has_contact_mean".  A frame's values do not depend on the chunk size."""
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    ops.voxel_pitch(voxel)
    obj = interpolate_sequence(seq_res, frame_nb, "obj_verts3d", CAMEXTR_SIGNS)
    verts = interpolate_sequence(seq_res, frame_nb, "hand_verts3d", CAMEXTR_SIGNS)
    hand_faces, object_faces = _faces(mano_faces_closed), _faces(obj_faces)
    volumes, depths, contacts = [], [], []
    for f0 in range(0, frame_nb, chunk):
        hand, thing = verts[f0:f0 + chunk], obj[f0:f0 + chunk]
        volumes += pointmetrics.get_volume_metrics(hand, thing, hand_faces, object_faces, voxel=voxel)["inter_volumes"]
        inter = pointmetrics.get_inter_metrics(hand, thing, hand_faces, object_faces)
        depths += inter["pen_depths"]
        contacts += inter["has_contact"]
    res = {"inter_volume": np.asarray(volumes, np.float64), "pen_depth": np.asarray(depths, np.float64),
           "has_contact": np.asarray(contacts, np.float64)}
    res.update({f"{key}_mean": float(vals.mean()) for key, vals in list(res.items())})
    return res


def evaluate_sequence_surface(seq_res, frame_nb, obj_faces, mano_faces_closed, chunk=512, contact_thresh=0.005):
    """`evaluate_sequence_surface_signed` with the ray-parity sign, which needs closed meshes: see there."""
    return evaluate_sequence_surface_signed(seq_res, frame_nb, obj_faces, mano_faces_closed, chunk, contact_thresh, "parity")


def evaluate_sequence_surface_signed(seq_res, frame_nb, obj_faces, mano_faces_closed, chunk=512, contact_thresh=0.005,
                                     sign="parity"):
    """Surface-distance plausibility of every interpolated frame of one sequence (`pointmetrics.get_surface_metrics_signed`,
    which `sign` is passed to: "parity", "winding" for meshes that are not closed, or "auto"); no ground truth is needed.
    seq_res, obj_faces, mano_faces_closed and chunk as `evaluate_sequence_plausibility` (the frames are
    interpolated and flipped the same way) -> per-frame float64 arrays "pen_depth" (hand into object, to the object's surface),
    "pen_depth_obj" (object vertices inside the hand), "min_dist", "contact_share" (hand vertices within `contact_thresh` of
    the surface or inside it) and "has_contact" (0 / 1), and their means over the frames under the same names with "_mean".
    A frame's values do not depend on the chunk size."""
    if sign not in meshutils.SIGN_MODES:
        raise ValueError(f"sign {sign!r} not in [parity|winding|auto]")
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    if not (np.isfinite(float(contact_thresh)) and float(contact_thresh) >= 0):
        raise ValueError(f"contact_thresh must be finite and not negative, got {contact_thresh}")
    obj = interpolate_sequence(seq_res, frame_nb, "obj_verts3d", CAMEXTR_SIGNS)
    verts = interpolate_sequence(seq_res, frame_nb, "hand_verts3d", CAMEXTR_SIGNS)
    hand_faces, object_faces = _faces(mano_faces_closed), _faces(obj_faces)
    keys = ("pen_depth", "pen_depth_obj", "min_dist", "contact_share", "has_contact")
    lists = {key: [] for key in keys}
    for f0 in range(0, frame_nb, chunk):
        part = pointmetrics.get_surface_metrics_signed(verts[f0:f0 + chunk], obj[f0:f0 + chunk], hand_faces, object_faces,
                                                       contact_thresh=contact_thresh, sign=sign)
        for key in keys:
            lists[key] += part[key]
    res = {key: np.asarray(lists[key], np.float64) for key in keys}
    res.update({f"{key}_mean": float(vals.mean()) for key, vals in list(res.items())})
    return res


PROTOCOL_KEYS = ("joint_err", "joint_err_al", "joint_err_sc_tr", "mesh_err", "mesh_err_al", "f@5", "f@15", "f_al@5", "f_al@15")


def evaluate_sequence_protocol(seq_res, frame_nb, gt_obj_verts, gt_hand_roots, obj_faces, mano_faces_closed, chunk=512,
                               gt_hand_joints=None, gt_hand_verts=None, anchors=(0, 4)):
    """`evaluate_sequence` with the hand protocol's per-frame arrays (homan_amd/handmetrics.py) added, computed chunk by chunk
    from the interpolated frames already on the device.  gt_hand_joints (frame_nb, 21, 3): HO-3D frame, HO-3D joint order (that
    of "export_joints") -> "joint_err", "joint_err_al", "joint_err_sc_tr" (frame_nb, 21) float64 per-joint errors raw,
    similarity-aligned and scale-and-translation-aligned on the joint rows `anchors`.  gt_hand_verts (frame_nb, 778, 3) ->
    "mesh_err", "mesh_err_al" (frame_nb, 778) and the per-frame F-scores "f@5", "f@15", "f_al@5", "f_al@15" (frame_nb,).
    Either may be None; with both None the result is `evaluate_sequence`'s: same keys, same bits.  A frame's values do not
    depend on the chunk size.  `protocol_summary` turns the arrays into the protocol's table."""
    return _evaluate_sequence(seq_res, frame_nb, gt_obj_verts, gt_hand_roots, obj_faces, mano_faces_closed, chunk,
                              (gt_hand_joints, gt_hand_verts, anchors))


def protocol_summary(per_frame, auc_max=0.05, auc_steps=100):
    """The protocol's table from the arrays of `evaluate_sequence_protocol` (a dict, or a list of them in sequence order):
    "xyz_mean3d", "xyz_auc", "xyz_al_mean3d", "xyz_al_auc", "xyz_sc_tr_mean3d", "xyz_sc_tr_auc", "mesh_mean3d", "mesh_auc",
    "mesh_al_mean3d", "mesh_al_auc" (means over all frames and points; AUC of the PCK curve over [0, auc_max], counted exactly
    on the device) and "f@5", "f@15", "f_al@5", "f_al@15" (means over the frames); only what the arrays hold."""
    if isinstance(per_frame, dict):
        per_frame = [per_frame]
    table = {}
    for key, name in (("joint_err", "xyz"), ("joint_err_al", "xyz_al"), ("joint_err_sc_tr", "xyz_sc_tr"), ("mesh_err", "mesh"),
                      ("mesh_err_al", "mesh_al")):
        if all(key in seq for seq in per_frame):
            err = np.concatenate([np.asarray(seq[key], np.float64).reshape(-1) for seq in per_frame])
            table[f"{name}_mean3d"] = float(err.mean())
            table[f"{name}_auc"] = handmetrics.auc(err, auc_max, auc_steps)
    for key in ("f@5", "f@15", "f_al@5", "f_al@15"):
        if all(key in seq for seq in per_frame):
            table[key] = float(np.concatenate([np.asarray(seq[key], np.float64).reshape(-1) for seq in per_frame]).mean())
    return table


def summarise(per_frame, unseen_from=None):
    """evalho3drecons.py:227-238: ({key: mean}, {key: median}, {key: max}) over all frames.  per_frame: the dict of
    `evaluate_sequence`, or a list of them in sequence order (concatenated).  unseen_from: global frame index at which the
    unseen objects start (`UNSEEN_FROM_HO3D` for the test split, :140-146); the object errors are then reported for both
    sides as well: "obj_dist_seen" / "add-s_seen" below it, "obj_dist_unseen" / "add-s_unseen" from it on."""
    if isinstance(per_frame, dict):
        per_frame = [per_frame]
    errors = {key: np.concatenate([np.asarray(seq[key], np.float64).reshape(-1) for seq in per_frame])
              for key in ("obj_dist", "obj_add-s", "hand_root", "has_contact", "pen_depths")}
    if unseen_from is not None:
        for name, key in (("obj_dist", "obj_dist"), ("add-s", "obj_add-s")):
            for side, part in (("seen", errors[key][:unseen_from]), ("unseen", errors[key][unseen_from:])):
                if part.size:
                    errors[f"{name}_{side}"] = part
    return ({key: float(np.mean(vals)) for key, vals in errors.items()},
            {key: float(np.median(vals)) for key, vals in errors.items()},
            {key: float(np.max(vals)) for key, vals in errors.items()})
