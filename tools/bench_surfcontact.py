#!/usr/bin/env python
"""Times the surface contact loss (ops.surface_contact_loss, csrc/surfcontact.hip) at the size of a fit - B = 30 frames, the
778-vertex hand against the 3 000-face bottle - and prints one JSON line:

  forward_ms     `hm_surface_contact_fwd` alone (search + terms + finish), through ctypes on a context's buffers;
  search_ms      `hm_point_mesh_distance` alone on the same inputs (d2, face and inside; no closest point);
  terms_ms       forward_ms - search_ms: memset, k_surface_terms, k_surface_finish, k_surface_loss;
  backward_ms    `hm_surface_contact_bwd` alone (both gradients);
  step_ms        forward plus backward as a user calls them: `surface_contact_loss` and `torch.autograd.grad` of A + R with respect to
                 points and vertices,
each for the hand's vertices against the bottle ("hand_to_object") and the bottle's vertices against the closed hand
("object_to_hand"; one-way is the first, two-way the sum of both), device events around `--windows` back-to-back calls, median of
`--reps`; and
  graph_its_per_s   the iteration rate of jointopt.GraphStepper (HOMan.forward + autograd in a hipGraph) on bench.py's clip with the
                    cfg3 weight set (synth.STEP2_LOSS_WEIGHTS): without the term, with it one-way, with it two-way - same process,
                    alternating, median of `--reps` windows of `--steps` iterations.

usage: python tools/bench_surfcontact.py [--frames B] [--reps R] [--windows W] [--steps K] [--size S] [--out FILE.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from homan_amd import lib, ops, synth  # noqa: E402
from homan_amd.mano_assets import synthetic_mano  # noqa: E402
from bench_surfmetrics import kernel_call, median_events  # noqa: E402


def scene(B, mano):
    """the hand gripping the bottle, turned and shifted a little from frame to frame -> (hand (B,778,3), bottle (B,V,3), faces)"""
    hand = mano["v_template"].astype(np.float64)
    obj, obj_faces = synth.bottle_mesh(segments=50, rings=30)
    obj = np.asarray(obj, np.float64) * 0.5
    centre = obj.mean(0) + np.array([0.0, 0.0, 0.66])
    hands, objs = [], []
    for b in range(B):
        ang = 0.3 + 0.02 * b
        c, s = np.cos(ang), np.sin(ang)
        rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        hands.append((hand - hand.mean(0)) @ rot.T + centre + np.array([0.012 + 0.0005 * b, 0.03, 0.002]))
        objs.append(obj - obj.mean(0) + centre)
    return np.stack(hands).astype(np.float32), np.stack(objs).astype(np.float32), np.asarray(obj_faces, np.int32)


def direction(points, verts, faces, reps, windows):
    """the five figures of one direction, in milliseconds, and the share of the points inside"""
    P, X = torch.from_numpy(points).cuda(), torch.from_numpy(verts).cuda()
    ctx = ops.SurfaceContactContext(P.shape[0], P.shape[1], X.shape[1], faces, "cuda")
    L = ops.surface_contact_log2q(P.shape[1])

    def forward():
        return ops._surface_contact_run(P, X, ctx, None, 0.010, 0.020, L)
    up = torch.ones(2, device="cuda")
    gp, gv = torch.empty_like(ctx.grad_points), torch.empty_like(ctx.grad_verts_attr)

    def backward():
        lib.check(lib.lib().hm_surface_contact_bwd(lib.ptr(ctx.grad_points), lib.ptr(ctx.inside), lib.ptr(ctx.grad_verts_attr),
                                                   lib.ptr(ctx.grad_verts_rep), lib.ptr(up), ctx.B * ctx.N, ctx.B * ctx.V, lib.ptr(gp),
                                                   lib.ptr(gv), lib.stream()), "hm_surface_contact_bwd")
    Pg, Xg = P.clone().requires_grad_(), X.clone().requires_grad_()

    def step():
        A, R = ops.surface_contact_loss(Pg, Xg, ctx)
        return torch.autograd.grad(A + R, (Pg, Xg))
    search, _ = kernel_call(P, X, ctx.faces)
    out = {"forward_ms": median_events(forward, reps, windows), "search_ms": median_events(search, reps, windows),
           "backward_ms": median_events(backward, reps, windows), "step_ms": median_events(step, reps, windows)}
    out["terms_ms"] = out["forward_ms"] - out["search_ms"]
    out = {k: round(v, 4) for k, v in out.items()}
    out["inside_share"] = round(float(ctx.inside.float().mean()), 4)
    out["loss"] = [float(x) for x in forward()]
    return out


def graph_rates(a, mano):
    from homan_amd.jointopt import GraphStepper, build_model
    sil_fn, hand_fn = synth.hip_clip_fns(mano)
    clip = synth.make_clip(seed=0, frames=a.frames, rend_size=a.size, image_size=a.size, obj="bottle", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn)
    base = dict(synth.STEP2_LOSS_WEIGHTS)
    with_term = dict(base, lw_surf_attr=1.0, lw_surf_rep=1.0)
    total = a.warmup + a.reps * a.steps
    steppers = {}
    for name, lw, kw in (("without", base, {}), ("one_way", with_term, {}), ("two_way", with_term, dict(surface_two_way=True))):
        model = build_model(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                            objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"], optimize_mano=True,
                            image_size=a.size, mano_model=mano, rend_size=a.size, sync_metrics=False, **kw)
        steppers[name] = GraphStepper(model, lw, 1e-2, total)
        steppers[name].run(a.warmup)
    rates = {name: [] for name in steppers}
    for _ in range(a.reps):                                  # alternating: the three see the same machine
        for name, st in steppers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.run(a.steps)
            torch.cuda.synchronize()
            rates[name].append(a.steps / (time.perf_counter() - t0))
    out = {name: round(statistics.median(r), 1) for name, r in rates.items()}
    out["ms_per_iteration"] = {name: round(1e3 / out[name], 4) for name in steppers}
    out["spread"] = {name: [round(min(r), 1), round(max(r), 1)] for name, r in rates.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--no-graph", action="store_true", help="skip the graph-mode iteration rates")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_surfcontact needs the MI355X"
    mano = synthetic_mano(0)
    hands, objs, obj_faces = scene(a.frames, mano)
    closed = np.asarray(mano["closed_faces"], np.int32)
    rec = {"frames": a.frames, "hand_verts": 778, "hand_faces": int(closed.shape[0]), "obj_verts": int(objs.shape[1]),
           "obj_faces": int(obj_faces.shape[0]), "reps": a.reps, "windows": a.windows,
           "hand_to_object": direction(hands, objs, obj_faces, a.reps, a.windows),
           "object_to_hand": direction(objs, hands, closed, a.reps, a.windows)}
    rec["one_way_step_ms"] = rec["hand_to_object"]["step_ms"]
    rec["two_way_step_ms"] = round(rec["hand_to_object"]["step_ms"] + rec["object_to_hand"]["step_ms"], 4)
    if not a.no_graph:
        rec["graph_its_per_s"] = dict(graph_rates(a, mano), steps=a.steps, size=a.size, weights="STEP2 (cfg3)")
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
