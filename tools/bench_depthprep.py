#!/usr/bin/env python
"""Times the depth registration (ops.register_depth, csrc/depthprep.hip: fill, splat, finish) and prints one JSON line.

  cases     `--frames` uint16 frames of 640x480 and of 1280x720 onto `--image`^2 (default 640), each with the identity and with a
            baseline transform (25 mm and a degree about y).  The call is captured in a hipGraph on preallocated buffers; the time
            is the median of `--reps` windows of `--windows` back-to-back replays between device events.  Beside it:
              bytes      what the three launches must move, from the shapes and the call's own statistics:
                           source   every tile (64x16) with its halo of r pixels, 2 bytes per pixel, read once
                           fill     4 bytes per target pixel written
                           atomics  4 bytes per atomicMin: surviving source pixels x the mean footprint (target pixels per
                                    source pixel in x times in y: the expected number of pixel centres inside it)
                           finish   4 bytes read and 4 written per target pixel
              the time those bytes take at the HBM bandwidth (8 TB/s peak, 6.3 TB/s achievable: the MI355X microarchitecture
              notes) and the ratio of the measured time to it;
              numpy_ms   the NumPy restatement of the same rule (tests/depthprep_ref.py) on the host, once: what a caller did
                         before - and the check that the timed call computed the rule (maps and statistics bit-equal).
  None of these is a pass criterion.

usage: python tools/bench_depthprep.py [--frames B] [--image S] [--reps R] [--windows W] [--no-numpy] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from homan_amd import depthprep, lib, ops  # noqa: E402
from bench_surfmetrics import median_events  # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12
TILE_W, TILE_H = 64, 16


def sensor_frames(B, Hd, Wd, seed=0):
    """a sloped background between 1 and 1.6 m, a nearer box that moves from frame to frame, 2 % holes; uint16 millimetres"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:Hd, :Wd]
    out = np.empty((B, Hd, Wd), np.uint16)
    for b in range(B):
        z = 1.0 + 0.6 * xx / Wd + 0.1 * yy / Hd
        x0, y0 = int(Wd * (0.3 + 0.005 * b)), int(Hd * 0.35)
        z[y0:y0 + Hd // 3, x0:x0 + Wd // 4] = 0.55 + 0.05 * yy[y0:y0 + Hd // 3, x0:x0 + Wd // 4] / Hd
        z += rng.normal(0, 0.001, z.shape)
        raw = np.rint(z * 1000).astype(np.uint16)
        raw[rng.random(z.shape) < 0.02] = 0
        out[b] = raw
    return out


def model_bytes(B, Hd, Wd, S, r, stats, fx_ratio, fy_ratio):
    tiles = -(-Wd // TILE_W) * -(-Hd // TILE_H) * B
    source = tiles * (TILE_W + 2 * r) * (TILE_H + 2 * r) * 2
    survivors = int((stats[:, 0] - stats[:, 1] - stats[:, 2]).sum())
    atomics = int(survivors * fx_ratio * fy_ratio) * 4
    px = B * S * S
    return {"source": source, "fill": 4 * px, "atomics": atomics, "finish": 8 * px, "total": source + 12 * px + atomics}


def case(name, B, Hd, Wd, S, f_px, T, a):
    frames = sensor_frames(B, Hd, Wd)
    Kd = np.array([[f_px, 0, Wd / 2.0], [0, f_px, Hd / 2.0], [0, 0, 1]], np.float64)
    ratio = S / Wd                                               # the colour image shows the sensor's width in S pixels
    Kc = np.array([[f_px * ratio / S, 0, 0.5], [0, f_px * ratio / S, 0.5], [0, 0, 1]], np.float64)
    opt = {k: v for k, v in depthprep.DEFAULTS.items() if k != "pixel_center"}
    cu = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    f, mats = cu(frames, np.uint16), [cu(m, np.float32) for m in (Kd, T, Kc)]
    out = torch.empty(B, S, S, device="cuda")
    stats = torch.empty(B, 4, dtype=torch.int32, device="cuda")
    call = lambda: ops.register_depth(f, 0.001, *mats, S, out=out, stats=stats, **opt)
    call()
    torch.cuda.synchronize()
    g = lib.new_graph()
    with torch.cuda.graph(g):
        call()
    ms = median_events(g.replay, a.reps, a.windows)
    st = stats.cpu().numpy()
    nbytes = model_bytes(B, Hd, Wd, S, opt["edge_radius"], st, ratio, ratio)
    rec = {"case": name, "source": [Wd, Hd], "frames": B, "image": S, "ms": round(ms, 4), "us_per_frame": round(1e3 * ms / B, 3),
           "bytes": nbytes, "ms_of_bytes_at_peak": round(1e3 * nbytes["total"] / HBM_PEAK, 4),
           "ms_of_bytes_at_achievable": round(1e3 * nbytes["total"] / HBM_ACHIEVABLE, 4),
           "time_over_bytes_at_achievable": round(ms * 1e-3 / (nbytes["total"] / HBM_ACHIEVABLE), 2),
           "stats_sum": st.sum(0).tolist(), "valid_target_share": round(float(st[:, 3].sum()) / (B * S * S), 4)}
    if not a.no_numpy:
        from tests import depthprep_ref
        t0 = time.perf_counter()
        want, want_stats = depthprep_ref.register32(frames, 0.001, Kd, T, Kc, S, **opt)
        rec["numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        rec["numpy_over_device"] = round(rec["numpy_ms"] / ms, 1)
        rec["bit_equal_to_numpy"] = bool(out.cpu().numpy().tobytes() == want.tobytes() and st.tolist() == want_stats.tolist())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--image", type=int, default=640)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--no-numpy", action="store_true", help="skip the NumPy restatement on the host")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depthprep needs the MI355X"
    c, s = np.cos(np.radians(1.0)), np.sin(np.radians(1.0))
    identity = np.eye(3, 4)
    baseline = np.array([[c, 0, s, 0.025], [0, 1, 0, 0.0], [-s, 0, c, 0.0]])
    rec = {"frames": a.frames, "image": a.image, "reps": a.reps, "windows": a.windows,
           "options": {k: v for k, v in depthprep.DEFAULTS.items()},
           "hbm_TBps": {"peak": HBM_PEAK / 1e12, "achievable": HBM_ACHIEVABLE / 1e12}, "cases": []}
    for Wd, Hd, f_px in ((640, 480, 580.0), (1280, 720, 920.0)):
        for tname, T in (("identity", identity), ("baseline", baseline)):
            rec["cases"].append(case(f"{Wd}x{Hd}_{tname}", a.frames, Hd, Wd, a.image, f_px, T, a))
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
