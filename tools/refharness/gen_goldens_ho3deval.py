#!/usr/bin/env python
"""Golden vectors for the sequence evaluation (homan_amd/postprocess.py, homan_amd/ho3deval.py), produced by the REFERENCE's
own homan/postprocess.py (post_process) and homan/eval/ho3devalutils.py (interpolate_res, dump), imported in place on CPU
tensors over the repo's CPU oracle leaves.  Build container only; writes tests/golden/ho3deval_reference.npz (or the path
given as the first argument).

Contents: two synthetic fits of 4 frames (one right hand; two hands labelled right, left - the reference relabels them) with
their sample_info and the reference's post_process outputs; a sequence whose key frames 0, 3, 7 ARE the first three results
of the one-hand sample (as evalho3drecons.py:84-97 collects them, plus a small object and a hand root), its interpolate_res output at
frame_nb = 10, that output after `.dot(camextr)[unorder_idxs].astype(np.float32)` (evalho3drecons.py:126-127,154-158), and
the rounded lists dump writes.  hand_verts3d / hand_joints3d / side of a sample are recorded as the INDEX of the hand whose
arrays they equal (the file stays below the joint-fit goldens' size).

Why 4 frames and not 3: rot6d_to_matrix (homan/utils/geometry.py:26) calls `torch.cross(b1, b2)` without `dim`, which takes the
FIRST dimension of size 3 - with exactly 3 rows that is the batch axis, and the reference then returns matrices that are no
rotations (determinant ~0.1).  An accident of that batch size, never met at the script's frame_nb = 10; no golden here has
3 rows per hand or object."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import shims  # noqa: E402

# (not ref_*.npz: tests/util.py reads every ref_*.npz but the pose-initialisation one as a joint-fit golden)
OUT = os.path.join(ROOT, "tests", "golden", "ho3deval_reference.npz")
STATE_KEYS = ("mano_pca_pose", "mano_rot", "mano_betas", "mano_trans", "rotations_hand", "translations_hand",
              "int_scales_hand", "int_scales_object", "translations_object", "rotations_object", "verts_object_og")
INTERP_KEYS = ("hand_verts3d", "hand_joints3d", "obj_verts3d", "hand_roots")
FRAME_NB = 10
CAMEXTR = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]])                      # evalho3drecons.py:101
UNORDER_IDXS = [0, 5, 6, 7, 10, 11, 12, 17, 18, 19, 13, 14, 15, 1, 2, 3, 4, 8, 12, 16, 20]       # :105-107


def import_reference():
    shims.install()
    shims._module("manopth")
    shims._module("manopth.manolayer")
    shims._module("manopth.rodrigues_layer")
    shims._module("libyana.renderutils")
    shims._module("libyana.renderutils.py3drendutils")
    cwd = os.getcwd()
    os.chdir(shims.REFERENCE_ROOT)
    sys.path.insert(0, shims.REFERENCE_ROOT)
    try:
        import homan.postprocess as ref_pp
        import homan.eval.ho3devalutils as ref_ev
    finally:
        os.chdir(cwd)
        sys.path.remove(shims.REFERENCE_ROOT)
    return ref_pp, ref_ev


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def synthetic_fit(rng, labels, frames, obj_verts):
    """A state_dict with the keys post_process reads (shapes of a joint_fit.pt: hands interleaved frame-major)"""
    rows = frames * len(labels)
    rot6d = lambda n: np.eye(3)[None, :, :2] + rng.normal(size=(n, 3, 2)) * 0.3          # noqa: E731
    sd = {
        "mano_pca_pose": rng.normal(size=(rows, 45)) * 0.4,
        "mano_rot": rng.normal(size=(rows, 3)) * 0.5,
        "mano_betas": rng.normal(size=(rows, 10)) * 0.5,
        "mano_trans": rng.normal(size=(rows, 3)) * 0.02,
        "rotations_hand": rot6d(rows),
        "translations_hand": rng.normal(size=(rows, 1, 3)) * 0.03 + np.array([0.0, 0.0, 0.5]),
        "int_scales_hand": np.array([1.0 + rng.uniform(0.02, 0.2)]),
        "int_scales_object": np.array([1.0 + rng.uniform(0.02, 0.2)]),
        "translations_object": rng.normal(size=(frames, 1, 3)) * 0.03 + np.array([0.05, 0.0, 0.55]),
        "rotations_object": rot6d(frames),
        "verts_object_og": np.repeat(obj_verts[None], frames, 0),
    }
    return {k: torch.from_numpy(f32(v)) for k, v in sd.items()}


def main(out=OUT):
    ref_pp, ref_ev = import_reference()
    from homan_amd import synth
    rng = np.random.default_rng(11)
    obj_verts, obj_faces = synth.box_mesh(2, 2, 2, scale=0.08)
    obj_verts = f32(obj_verts)
    rec = {"obj_verts": obj_verts, "obj_faces": np.asarray(obj_faces, np.int32)}
    results = {}
    for tag, labels, frame_idxs, scale in (("pp1", ["right_hand"], [0, 3, 7, 9], [1.25]),
                                          ("pp2", ["right_hand", "left_hand"], [0, 1, 2, 3], None)):
        frames = len(frame_idxs)
        assert frames != 3          # (see the module docstring)
        sd = synthetic_fit(rng, labels, frames, obj_verts)
        K = f32(np.array([[480.0, 0.0, 128.0], [0.0, 480.0, 128.0], [0.0, 0.0, 1.0]])[None].repeat(frames, 0))
        K[:, 0, 2] += np.arange(frames, dtype=np.float32)
        seq = "SM1" if tag == "pp1" else "MPM10"
        obj_info = {"path": [f"models/box_{tag}/textured_simple.obj"] * frames}
        if scale is not None:
            obj_info["scale"] = scale
        sample_info = {"hands": [{"label": label} for label in labels], "camera": {"K": torch.from_numpy(K)},
                       "images": [f"HO3D/evaluation/{seq}/rgb/{f:04d}.png" for f in frame_idxs], "objects": [obj_info],
                       "seq_idx": seq, "frame_idxs": frame_idxs}
        infos, seq_idx, got_idxs = ref_pp.post_process(sample_info, sd, frame_nb=frames)
        assert seq_idx == seq and list(got_idxs) == frame_idxs and len(infos) == frames
        results[tag] = infos
        for k in STATE_KEYS:
            rec[f"{tag}_sd_{k}"] = sd[k].numpy()
        rec[f"{tag}_in_labels"] = np.array(labels)
        rec[f"{tag}_in_K"] = K
        rec[f"{tag}_in_images"] = np.array(sample_info["images"])
        rec[f"{tag}_in_obj_path"] = np.array(obj_info["path"])
        rec[f"{tag}_in_scale"] = f32(scale if scale is not None else [])
        rec[f"{tag}_in_frame_idxs"] = np.asarray(frame_idxs, np.int32)
        rec[f"{tag}_in_seq_idx"] = np.array(seq)
        all_verts = np.stack([np.stack(info["all_hand_verts3d"]) for info in infos])          # (frames, hands, 778, 3)
        rec[f"{tag}_out_all_hand_verts3d"] = all_verts
        assert all_verts.dtype == np.float32
        # the single-hand entries are one of the hands': which one is what the golden records
        owner = [h for h in range(len(labels)) if all(np.array_equal(info["hand_verts3d"], info["all_hand_verts3d"][h])
                                                      for info in infos)]
        assert len(owner) == 1
        rec[f"{tag}_out_hand_verts3d_hand"] = np.int32(owner[0])
        rec[f"{tag}_out_hand_joints3d"] = np.stack([info["hand_joints3d"] for info in infos])
        for k in ("camintr", "obj_rot", "obj_trans"):
            rec[f"{tag}_out_{k}"] = np.stack([info[k] for info in infos])
        rec[f"{tag}_out_obj_scale"] = np.asarray([info["obj_scale"] for info in infos], np.float64)
        for k in ("img_path", "side", "obj_path"):
            rec[f"{tag}_out_{k}"] = np.array([info[k] for info in infos])
        rec[f"{tag}_out_hand_sides"] = np.array(infos[0]["hand_sides"])
        assert all(info["hand_sides"] == infos[0]["hand_sides"] for info in infos)

    # ---- the sequence: key frames = the one-hand sample's results, as evalho3drecons.py:84-97 collects them
    scan = obj_verts - obj_verts.mean(0)
    seq_res = {}
    for frame_idx, info in zip(rec["pp1_in_frame_idxs"].tolist()[:3], results["pp1"]):
        res = dict(info)
        res["obj_verts3d"] = scan.dot(info["obj_rot"]) * info["obj_scale"] + info["obj_trans"]          # (:91-93)
        res["hand_roots"] = f32(info["hand_joints3d"][:1] + rng.normal(size=(1, 3)) * 0.01)
        assert res["obj_verts3d"].dtype == np.float32
        seq_res[frame_idx] = res
    rec["seq_in_obj_verts3d"] = np.stack([seq_res[f]["obj_verts3d"] for f in sorted(seq_res)])
    rec["seq_in_hand_roots"] = np.stack([seq_res[f]["hand_roots"] for f in sorted(seq_res)])
    interp = ref_ev.interpolate_res(seq_res, FRAME_NB)
    rec["seq_out_img_paths"] = np.array(interp["img_paths"])
    for k in INTERP_KEYS:
        assert len(interp[k]) == FRAME_NB
        rec[f"seq_out_{k}"] = np.stack([np.asarray(v, np.float64) for v in interp[k]])
        idx = UNORDER_IDXS if k == "hand_joints3d" else slice(None)
        rec[f"seq_flip_{k}"] = np.stack([v.dot(CAMEXTR)[idx].astype(np.float32) for v in interp[k]])
    # ---- dump (codalab=False: no `zip` call, no ./pred.zip): the joints and, to keep the file small, the object's vertices
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "pred.json")
        ref_ev.dump(path, list(rec["seq_flip_hand_joints3d"]), list(rec["seq_flip_obj_verts3d"]), codalab=False)
        with open(path) as fh:
            xyz, verts = json.load(fh)
    rec["dump_out_xyz"], rec["dump_out_verts"] = np.asarray(xyz, np.float64), np.asarray(verts, np.float64)
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
