#!/usr/bin/env python
"""Times the two-stage mesh preparation (meshprep.make_watertight_detail: surface nets at a fine lattice, then the edge-collapse
decimation of csrc/decimate.hip) beside the budget-lattice path (meshprep.make_watertight) on the inputs of tools/bench_meshprep.py:
the 3 000-face bottle and the same bottle subdivided twice (48 000 faces), target_vertices=1000, detail_resolution 64 and 96.

Per source: the default path's wall clock (median, and lowest / highest of the timed runs: the session's run-to-run spread); per
detail resolution the whole call (wall clock, synchronised), the stages alone through the ops (device events: winding search,
nets, snap; the decimation by wall clock, since it reads the host once per round), the detail vertex count, the rounds, ms per
round, and the launches of one round (kernels counted by torch's profiler: the library's and torch's sorts, scans and gathers).
Quality: the two-way surface distance between each path's output and the source (`ops.point_mesh_distance` from the vertices of
one to the surface of the other, mean and largest, in units of the source's longest extent).
Every timing is the median of `--reps` runs after one untimed run.

usage: python tools/bench_decimate.py [--reps R] [--out profiles/decimate.json]"""
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
from homan_amd import meshprep, ops, synth  # noqa: E402
from bench_meshprep import median_ms, subdivide  # noqa: E402


def wall_ms(fn, reps):
    out, result = [], None
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    timed = out[1:]
    return {"median_ms": round(float(np.median(timed)), 3), "lowest_ms": round(min(timed), 3), "highest_ms": round(max(timed), 3)}, result


def two_way(out_v, out_f, src_v, src_f):
    """vertex-sampled surface distance in both directions, in units of the source's longest extent"""
    dev = torch.device("cuda")
    extent = float((src_v.max(0) - src_v.min(0)).max())
    a = torch.from_numpy(np.ascontiguousarray(out_v, np.float32)).to(dev)[None]
    b = torch.from_numpy(np.ascontiguousarray(src_v, np.float32)).to(dev)[None]
    to_src = ops.point_mesh_distance(a, b, np.asarray(src_f, np.int64))["d2"][0].double().sqrt() / extent
    to_out = ops.point_mesh_distance(b, a, np.asarray(out_f, np.int64))["d2"][0].double().sqrt() / extent
    return {"output_to_source_mean": float(to_src.mean()), "output_to_source_max": float(to_src.max()),
            "source_to_output_mean": float(to_out.mean()), "source_to_output_max": float(to_out.max())}


def launches_of_one_round(v, f):
    try:
        from torch.profiler import ProfilerActivity, profile
        ops.collapse_round(v, f, 1)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            ops.collapse_round(v, f, 1)
            torch.cuda.synchronize()
        names = [e.key for e in prof.key_averages() for _ in range(e.count) if "memcpy" not in e.key.lower()
                 and "memset" not in e.key.lower()]
        return {"kernels": len(names), "of_the_library": sum(n.startswith("k_dc_") for n in names)}
    except Exception as exc:                                               # a count, not a result: the rest of the record stands
        return {"kernels": None, "error": repr(exc)}


def detail_row(v, f, R, reps):
    whole, mesh = wall_ms(lambda: meshprep.make_watertight_detail(v, f, R, target_vertices=1000), reps)
    lat = ops.lattice_signs(v, f, R)
    nets = ops.surface_nets(lat["inside"], lat["origin"], lat["pitch"])
    src = torch.from_numpy(v).to(nets["vertices"].device)[None]

    def snap():
        found = ops.point_mesh_distance(nets["vertices"][None], src, f, closest=True)
        return ops.lattice_snap(nets["vertices"], found["closest"][0], found["d2"][0], lat["pitch"], meshprep.SNAP_LIMIT)[0]
    row = {"whole": whole, "detail_vertices": mesh["detail_vertices"], "out_vertices": int(len(mesh["vertices"])),
           "reached": mesh["reached"], "rounds": mesh["rounds"], "closed": mesh["topology"]["closed"],
           "oriented": mesh["topology"]["oriented"],
           "winding_search_ms": round(median_ms(lambda: ops.lattice_signs(v, f, R), reps), 3),
           "nets_ms": round(median_ms(lambda: ops.surface_nets(lat["inside"], lat["origin"], lat["pitch"]), reps), 3),
           "snap_ms": round(median_ms(snap, reps), 3)}
    snapped = snap()
    row["decimation"], small = wall_ms(lambda: ops.decimate_mesh(snapped, nets["faces"], 1000), reps)
    row["ms_per_round"] = round(row["decimation"]["median_ms"] / max(small["rounds"], 1), 4)
    row["launches_per_round"] = launches_of_one_round(snapped, nets["faces"])
    row["distance"] = two_way(mesh["vertices"], mesh["faces"], v, f)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decimate needs the MI355X"
    bv, bf = synth.bottle_mesh(segments=50, rings=30)
    bv, bf = np.asarray(bv, np.float32), np.asarray(bf, np.int64)
    fv, ff = subdivide(*subdivide(bv, bf))
    rec = {"reps": a.reps, "target_vertices": 1000, "sources": {}}
    for name, v, f in (("bottle_3000", bv, bf), ("bottle_48000", fv, ff)):
        default, mesh = wall_ms(lambda: meshprep.make_watertight(v, f, target_vertices=1000), a.reps)
        row = {"faces": int(len(f)), "default_path": dict(default, resolution=mesh["resolution"], out_vertices=int(len(mesh["vertices"])),
                                                           distance=two_way(mesh["vertices"], mesh["faces"], v, f))}
        for R in (64, 96):
            row[f"detail_resolution_{R}"] = detail_row(v, f, R, a.reps)
        row["default_path_again"] = wall_ms(lambda: meshprep.make_watertight(v, f, target_vertices=1000), a.reps)[0]
        rec["sources"][name] = row
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
