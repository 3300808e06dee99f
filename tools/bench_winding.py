#!/usr/bin/env python
"""Times the generalised winding number (`hm_point_mesh_winding`, csrc/winding.hip) and, in the same run and at the same shapes,
the parity search beside it (`hm_point_mesh_distance`: d2, face, inside; no closest point), both alone through ctypes on
preallocated buffers, device events around `--windows` back-to-back calls.  Shapes:

  evaluation   the frames of the first sequence of the HO-3D evaluation walk of tools/bench_surfmetrics.py (886 frames): the
               778 hand vertices against the 3000-face object, and the object's vertices against the hand's 1552 closed faces;
               no frame's faces are split;
  fit          30 frames of the hand against the 3000-face bottle, the size of a fit (tools/bench_surfcontact.py): the faces of
               a frame are dealt to several workgroups, which merge through the 64-bit integer atomicAdd.
Prints one JSON line: per shape `winding_ms`, `parity_ms`, the pairs per second each implies, and their ratio.  Every figure is
the median of `--reps` timed windows after one untimed call.

usage: python tools/bench_winding.py [--reps R] [--windows W] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from homan_amd import ho3deval, lib, ops, synth  # noqa: E402
from homan_amd.mano_assets import synthetic_mano  # noqa: E402
from bench_ho3deval import SEQ_LENS, make_sequence  # noqa: E402
from bench_surfmetrics import kernel_call, median_events  # noqa: E402


def winding_call(points, verts, faces):
    """a closure that enqueues hm_point_mesh_winding on preallocated outputs (count and inside)"""
    h = lib.lib()
    B, N, V, F = points.shape[0], points.shape[1], verts.shape[1], faces.shape[0]
    count = torch.empty(B, N, dtype=torch.int64, device=points.device)
    inside = torch.empty(B, N, dtype=torch.int32, device=points.device)
    args = (lib.ptr(points), lib.ptr(verts), lib.ptr(faces), B, N, V, F, ops.winding_log2q(F), lib.ptr(count), lib.ptr(inside))

    def call():
        lib.check(h.hm_point_mesh_winding(*args, lib.stream()), "hm_point_mesh_winding")
    call.keep = (count, inside)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_winding needs the MI355X"
    mano = synthetic_mano(0)
    hand = mano["v_template"].astype(np.float32)
    joints = np.ascontiguousarray(hand[np.linspace(0, 777, 21).astype(int)])
    obj, obj_faces = synth.bottle_mesh(segments=50, rings=30)
    obj = np.asarray(obj, np.float32) * np.float32(0.5)
    closed = np.asarray(mano["closed_faces"])
    seq = make_sequence(np.random.default_rng(0), SEQ_LENS[0], hand, joints, obj)[0]
    h0 = ho3deval.interpolate_sequence(seq, SEQ_LENS[0], "hand_verts3d", ho3deval.CAMEXTR_SIGNS)
    o0 = ho3deval.interpolate_sequence(seq, SEQ_LENS[0], "obj_verts3d", ho3deval.CAMEXTR_SIGNS)
    dev_obj_faces = torch.from_numpy(np.ascontiguousarray(obj_faces, dtype=np.int32)).to(h0.device)
    dev_hand_faces = torch.from_numpy(np.ascontiguousarray(closed, dtype=np.int32)).to(h0.device)
    shapes = (("evaluation_hand_to_object", h0, o0, dev_obj_faces), ("evaluation_object_to_hand", o0, h0, dev_hand_faces),
              ("fit_hand_to_object", h0[:30].contiguous(), o0[:30].contiguous(), dev_obj_faces))
    rec = {"reps": a.reps, "windows": a.windows, "shapes": {}}
    for key, points, verts, faces in shapes:
        parity, pairs = kernel_call(points, verts, faces)
        winding = winding_call(points, verts, faces)
        ms_w, ms_p = median_events(winding, a.reps, a.windows), median_events(parity, a.reps, a.windows)
        rec["shapes"][key] = {"frames": int(points.shape[0]), "points": int(points.shape[1]), "faces": int(faces.shape[0]),
                              "log2q": ops.winding_log2q(faces.shape[0]), "winding_ms": round(ms_w, 4), "parity_ms": round(ms_p, 4),
                              "winding_pairs_per_s": round(pairs / (ms_w * 1e-3), 1),
                              "parity_pairs_per_s": round(pairs / (ms_p * 1e-3), 1), "winding_over_parity": round(ms_w / ms_p, 3)}
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
