#!/usr/bin/env python
"""Times the soft silhouette op (hm_softsil_fwd + hm_softsil_bwd, csrc/softsil.hip) at cfg2's size - one clip of 30 frames at
256 x 256, the bottle - for sigma in {1e-5, 1e-4, 1e-3}, and, in the same process on the same clip, the hard path's three
heavy kernels (raster, edge sweep, line sources) through hm_bench_sil_kernels.  Warm-up first, device events, repetitions
sized for a window of about half a second.  Prints one JSON record and writes it to profiles/softsil.json.

The two are different image formations (the soft mode is a non-parity extra): the numbers stand side by side, neither is a bar
for the other.

usage: python tools/bench_softsil.py [--window 0.5] [--out profiles/softsil.json]"""
import argparse
import copy
import json
import math
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from homan_amd import lib as hlib, ops, synth  # noqa: E402
from homan_amd.jointopt import build_model  # noqa: E402
from homan_amd.mano_assets import synthetic_mano  # noqa: E402

SIGMAS = [1e-5, 1e-4, 1e-3]


def timed(fn, window):
    """ms per call of fn(): three warm-up calls, one timed call to size the series, then a series of about `window` seconds"""
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    reps = max(10, min(20000, int(math.ceil(window * 1e3 / max(t0.elapsed_time(t1), 1e-3)))))
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softsil.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_softsil needs the MI355X"
    mano = synthetic_mano(0)
    sil_fn, hand_fn = synth.hip_clip_fns(mano)
    clip = synth.make_clip(seed=0, frames=30, rend_size=256, image_size=256, obj="bottle", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn)
    model = build_model(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                        objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"], optimize_mano=True,
                        image_size=256, mano_model=mano, rend_size=256, sync_metrics=False)
    L, P = hlib.lib(), hlib.ptr
    with torch.no_grad():
        verts = model.get_verts_object()[0].detach().contiguous()
    K, hard = model.camintr_rois_object.contiguous(), model.losses.sil_ctx
    B, V, F, S = hard.B, hard.V, hard.F, 256
    rec = {"frames": B, "size": S, "faces": F, "verts": V, "window_s": a.window, "soft": []}

    soft = ops.SoftSilhouetteContext(model.faces_object, V, B, S, verts.device)
    alpha, gverts = torch.empty(B, S, S, device="cuda"), torch.empty(B, V, 3, device="cuda")
    # the upstream image of the silhouette term: d loss / d alpha = 2 keep (keep alpha - ref) / sum(keep) / B
    keep, ref = model.keep_mask_object, model.ref_mask_object
    sigma = torch.zeros(1, device="cuda")
    args = (P(verts), P(hard.faces), P(K), B, V, F, S, 1.0, ops.NMR_NEAR, ops.NMR_FAR, P(sigma))

    def fwd():
        hlib.check(L.hm_softsil_fwd(*args, P(alpha), P(soft.workspace), hlib.stream()), "hm_softsil_fwd")

    for s in SIGMAS:
        sigma.fill_(s)
        fwd()
        up = (2 * keep * (keep * alpha - ref) / keep.sum() / B).contiguous()

        def bwd():
            hlib.check(L.hm_softsil_bwd(*args, P(alpha), P(up), P(soft.adj_off), P(soft.adj_items), P(gverts), P(soft.workspace),
                                        hlib.stream()), "hm_softsil_bwd")

        def both():
            fwd()
            bwd()

        f_ms, f_reps = timed(fwd, a.window)
        b_ms, _ = timed(bwd, a.window)
        t_ms, t_reps = timed(both, a.window)
        rec["soft"].append({"sigma": s, "cutoff_radius_px": round(math.sqrt(16 * s) * S / 2, 2), "fwd_ms": round(f_ms, 4),
                            "bwd_ms": round(b_ms, 4), "fwd_bwd_ms": round(t_ms, 4), "reps": t_reps,
                            "coverage": round(float(alpha.mean()), 4)})

    # the hard path on the same clip: one forward + backward to populate its workspace, then each heavy kernel back to back
    pooled, out2, one = torch.empty(B, S, S, device="cuda"), torch.empty(2, device="cuda"), torch.ones(1, device="cuda")
    ms = torch.zeros(3)
    reps = 200
    for _ in range(2):       # (the first series warms up; a series of 200 launches is 10-60 ms per kernel: ten of them below)
        hlib.check(L.hm_bench_sil_kernels(P(verts), P(hard.faces), P(K), B, V, F, S, P(keep), P(ref), P(model.losses.keep_sum),
                                          P(pooled), P(out2), P(hard.work_order), P(hard.adj_off), P(hard.adj_items), P(one),
                                          P(gverts), P(hard.workspace), reps, ms.data_ptr(), hlib.stream()), "hm_bench_sil_kernels")
    acc, series = [0.0, 0.0, 0.0], 10
    for _ in range(series):
        hlib.check(L.hm_bench_sil_kernels(P(verts), P(hard.faces), P(K), B, V, F, S, P(keep), P(ref), P(model.losses.keep_sum),
                                          P(pooled), P(out2), P(hard.work_order), P(hard.adj_off), P(hard.adj_items), P(one),
                                          P(gverts), P(hard.workspace), reps, ms.data_ptr(), hlib.stream()), "hm_bench_sil_kernels")
        acc = [x + float(y) for x, y in zip(acc, ms)]
    r, sw, ln = (x / series for x in acc)
    rec["hard_kernels"] = {"raster_ms": round(r, 4), "sweep_ms": round(sw, 4), "lines_ms": round(ln, 4),
                           "sum_ms": round(r + sw + ln, 4), "reps": reps * series,
                           "note": "standalone launches of the three heavy kernels only (no face setup, reduction or gather)"}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
