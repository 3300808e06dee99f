#!/usr/bin/env python
"""Times the observed-depth term (ops.depth_obs_loss, csrc/depthobs.hip) and prints one JSON line:

  kernels        at `--frames` frames of `--image`^2 pixels with two and three layers: `hm_depth_obs_fwd` and `hm_depth_obs_bwd`
                 (with the sparse-backward flags) alone, through ctypes on preallocated buffers, device events around `--windows`
                 back-to-back calls, median of `--reps`; beside each the bytes the launch must move (computed from the shapes,
                 below) and the ratio of the measured time to those bytes over the HBM bandwidth (8 TB/s peak and 6.3 TB/s
                 achievable, the figures of the MI355X microarchitecture notes).  The layers' masks cover discs of about a tenth
                 of the image, like a hand and an object in a frame.
                   forward bytes / (pixel, layer): 4 (depth) + 4 (silhouette) + 1 (mask) read, 4 (clamped residual) written,
                   + 4 per pixel for the depth map (counted ONCE: the layers' re-reads can be served from cache; 13 read per
                   pixel and layer when they are not); backward: 4 read + 4 written (+ the flags, 1/64 byte).
  graph_its_per_s   the iteration rate of jointopt.GraphStepper (HOMan.forward + autograd in a hipGraph) on bench.py's cfg2 clip
                    (30 frames, 256^2, bottle, synth.STEP1_LOSS_WEIGHTS): without the term - the path a caller without
                    lw_depth_obs runs, unchanged from before the term existed - and with it (all layers, lw_depth_obs = 100,
                    an untuned weight) - same process, alternating, median of `--reps` windows of `--steps` iterations.  The depth
                    maps are composed from the clip's own starting renders (nearest fully covered layer per pixel).

usage: python tools/bench_depthobs.py [--frames B] [--image S] [--reps R] [--windows W] [--steps K] [--size S] [--out FILE.json]"""
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
from bench_surfmetrics import median_events  # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def model_bytes(B, S, L):
    """bytes one launch must move, from the shapes alone -> (forward, forward with the map re-read per layer, backward)"""
    px = B * S * S
    return px * (L * (4 + 4 + 1 + 4) + 4), px * L * (13 + 4), px * L * 8 + L * px // 64


def layers(B, S, L, seed=0):
    """L layers of renders whose masks are discs of about a tenth of the image, and a sensor map with holes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:S, :S]
    D = rng.uniform(0.4, 0.9, (B, S, S)).astype(np.float32)
    D[rng.uniform(size=D.shape) < 0.02] = 0.0                                   # sensor holes
    d, a, m = [], [], []
    for l in range(L):
        cx, cy = S * (0.35 + 0.15 * l), S * (0.45 + 0.05 * l)
        disc = (xx - cx) ** 2 + (yy - cy) ** 2 < (0.18 * S) ** 2
        a.append(np.broadcast_to(disc, D.shape).astype(np.float32))
        m.append(np.broadcast_to(disc, D.shape).astype(np.uint8))
        d.append(np.where(disc, D + rng.normal(0, 0.03, D.shape), 100.0).astype(np.float32))
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return [cu(x) for x in d], [cu(x) for x in a], [cu(x) for x in m], cu(D)


def kernels(B, S, L, reps, windows):
    d, a, m, D = layers(B, S, L)
    h, P = lib.lib(), lib.ptr
    scratch = ops.DepthObsScratch(L, B, "cuda")
    c = [torch.empty_like(x) for x in d]
    g = [torch.empty_like(x) for x in d]
    f = [torch.empty(B * S * (S // 64), dtype=torch.uint8, device="cuda") for _ in range(L)]
    rec, out, up = torch.empty(L, B, 2, device="cuda"), torch.empty(4, device="cuda"), torch.ones(1, device="cuda")
    p3 = lambda ts: [P(ts[i]) if i < L else None for i in range(3)]

    def forward():
        lib.check(h.hm_depth_obs_fwd(*p3(d), *p3(a), *p3(m), P(D), L, B, S, 0.03, ops.NMR_NEAR, ops.NMR_FAR, *p3(c), P(scratch.buf),
                                     P(rec), P(out), lib.stream()), "hm_depth_obs_fwd")

    def backward():
        lib.check(h.hm_depth_obs_bwd(*p3(c), L, B, S, P(rec), P(out), P(up), *p3(g), *p3(f), lib.stream()), "hm_depth_obs_bwd")
    fwd_ms, bwd_ms = median_events(forward, reps, windows), median_events(backward, reps, windows)
    bf, bf_reread, bb = model_bytes(B, S, L)
    return {"layers": L, "forward_ms": round(fwd_ms, 4), "backward_ms": round(bwd_ms, 4), "forward_bytes": bf,
            "forward_bytes_map_reread": bf_reread, "backward_bytes": bb,
            "forward_time_over_bytes_at_peak": round(fwd_ms * 1e-3 / (bf / HBM_PEAK), 2),
            "forward_time_over_bytes_at_achievable": round(fwd_ms * 1e-3 / (bf / HBM_ACHIEVABLE), 2),
            "backward_time_over_bytes_at_peak": round(bwd_ms * 1e-3 / (bb / HBM_PEAK), 2),
            "forward_TBps": round(bf / (fwd_ms * 1e-3) / 1e12, 3), "backward_TBps": round(bb / (bwd_ms * 1e-3) / 1e12, 3),
            "valid_share": round(float(out[2]), 4), "flag_share": round(float(torch.stack(f).float().mean()), 4)}


def compose(model):
    """(depth maps, instance masks per layer) from the model's own per-layer renders at its current parameters"""
    with torch.no_grad():
        renders = model.render_depth_layers(model.get_verts_object()[0], model.get_verts_hand()[0])
        sils = torch.stack([renders[l][0] for l in sorted(renders)])
        deps = torch.stack([renders[l][1] for l in sorted(renders)])
        near, arg = torch.where(sils == 1, deps, torch.full_like(deps, float("inf"))).min(0)
        hit = torch.isfinite(near)
        return torch.where(hit, near, torch.zeros_like(near)).cpu(), [((arg == l) & hit).cpu() for l in range(sils.shape[0])]


def graph_rates(a, mano):
    from homan_amd.jointopt import GraphStepper, build_model
    sil_fn, hand_fn = synth.hip_clip_fns(mano)
    clip = synth.make_clip(seed=0, frames=a.frames, rend_size=a.size, image_size=a.size, obj="bottle", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn)

    def build(clip, **kw):
        return build_model(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                           objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"], optimize_mano=True,
                           image_size=a.size, mano_model=mano, rend_size=a.size, sync_metrics=False, **kw)
    D, masks = compose(build(clip))
    for b, (pp, op) in enumerate(zip(clip["person_parameters"], clip["object_parameters"])):
        op["full_mask"] = masks[0][b].float()
        pp["masks"] = torch.stack([m[b] for m in masks[1:]]).float()
    D = D + (D > 0) * 0.01                                   # (a centimetre off: the term has work to do)
    base = dict(synth.STEP1_LOSS_WEIGHTS)
    total = a.warmup + a.reps * a.steps
    steppers = {}
    for name, lw in (("without", base), ("with_depth_obs", dict(base, lw_depth_obs=100.0))):
        steppers[name] = GraphStepper(build(clip, depth_maps=D), lw, 1e-2, total)
        steppers[name].run(a.warmup)
    rates = {name: [] for name in steppers}
    for _ in range(a.reps):                                  # alternating: both see the same machine
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
    ap.add_argument("--image", type=int, default=640, help="image size of the kernel timings")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--size", type=int, default=256, help="raster and image size of the graph-loop clip (cfg2: 256)")
    ap.add_argument("--no-graph", action="store_true", help="skip the graph-mode iteration rates")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depthobs needs the MI355X"
    rec = {"frames": a.frames, "image": a.image, "reps": a.reps, "windows": a.windows, "delta": 0.03,
           "hbm_TBps": {"peak": HBM_PEAK / 1e12, "achievable": HBM_ACHIEVABLE / 1e12},
           "kernels": [kernels(a.frames, a.image, L, a.reps, a.windows) for L in (2, 3)]}
    if not a.no_graph:
        rec["graph_its_per_s"] = dict(graph_rates(a, synthetic_mano(0)), steps=a.steps, size=a.size, weights="STEP1 (cfg2)",
                                      lw_depth_obs=100.0)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
