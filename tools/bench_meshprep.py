#!/usr/bin/env python
"""Times the mesh preparation (homan_amd/meshprep.py make_watertight, csrc/remesh.hip) at target_vertices=1000 for two sources:
the 3 000-face bottle, and the same bottle subdivided twice (48 000 faces).  Per source: the whole `make_watertight` (wall clock,
the budget search's probes included, synchronised), and at the resolution it chose the stages alone through the ops, device
events around each: signs (corner positions + winding number), repair (pack + Jacobi passes), count (popcounts + scan), emit
(vertices + faces), snap (closest point + select).  Every figure is the median of `--reps` runs after one untimed run.

usage: python tools/bench_meshprep.py [--reps R] [--out profiles/meshprep.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from homan_amd import lib, meshprep, ops, synth  # noqa: E402


def subdivide(v, f):
    """every triangle into four through its edge midpoints"""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    uniq, inverse = np.unique(edges, axis=0, return_inverse=True)
    mid = len(v) + inverse.reshape(3, -1)
    ab, bc, ca = mid[0], mid[1], mid[2]
    nv = np.concatenate([v, 0.5 * (v[uniq[:, 0]] + v[uniq[:, 1]])])
    nf = np.concatenate([np.stack([f[:, 0], ab, ca], 1), np.stack([f[:, 1], bc, ab], 1), np.stack([f[:, 2], ca, bc], 1),
                         np.stack([ab, bc, ca], 1)])
    return nv.astype(np.float32), nf


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def stages(v, f, R, reps):
    h = lib.lib()
    lat = ops.lattice_signs(v, f, R)
    nx, ny, nz = lat["dims"]
    o, pitch = lat["origin"], float(lat["pitch"])
    dev = lat["inside"].device
    flags = lat["inside"].contiguous()
    words = h.hm_lattice_words(nx, ny, nz)
    bits = torch.empty(2 * words, dtype=torch.int64, device=dev)
    cell_bits = torch.empty(words, dtype=torch.int64, device=dev)
    offsets = torch.empty(4 * ny * nz, dtype=torch.int32, device=dev)
    report = torch.empty(ops._LATTICE_REPORT_INTS + 4, dtype=torch.int32, device=dev)     # as ops._surface_nets_counted
    totals = report[ops._LATTICE_REPORT_INTS:]

    def repair():
        lib.check(h.hm_lattice_repair(lib.ptr(flags), nx, ny, nz, lib.ptr(bits), lib.ptr(report), lib.stream()), "repair")

    def count():
        lib.check(h.hm_surface_nets_count(lib.ptr(bits), nx, ny, nz, lib.ptr(cell_bits), lib.ptr(offsets), lib.ptr(totals),
                                          lib.stream()), "count")
    out = {"signs_ms": median_ms(lambda: ops.lattice_signs(v, f, R), reps), "repair_ms": median_ms(repair, reps),
           "count_ms": median_ms(count, reps)}
    host = report.cpu().tolist()
    nv, nt = host[-4], 2 * sum(host[-3:])
    vertices = torch.empty(nv, 3, device=dev)
    tris = torch.empty(nt, 3, dtype=torch.int32, device=dev)

    def emit():
        lib.check(h.hm_surface_nets_emit(lib.ptr(bits), lib.ptr(cell_bits), lib.ptr(offsets), lib.ptr(totals), nx, ny, nz,
                                         float(o[0]), float(o[1]), float(o[2]), pitch, nv, nt, lib.ptr(vertices), lib.ptr(tris),
                                         lib.stream()), "emit")
    out["emit_ms"] = median_ms(emit, reps)
    src = torch.from_numpy(v).to(dev)[None]

    def snap():
        found = ops.point_mesh_distance(vertices[None], src, f, closest=True)
        ops.lattice_snap(vertices, found["closest"][0], found["d2"][0], pitch, meshprep.SNAP_LIMIT)
    out["snap_ms"] = median_ms(snap, reps)
    out.update(corners=nx * ny * nz, dims=[nx, ny, nz], vertices=nv, triangles=nt, repair_passes=host[0])
    return {k: round(x, 4) if isinstance(x, float) else x for k, x in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_meshprep needs the MI355X"
    bv, bf = synth.bottle_mesh(segments=50, rings=30)
    bv, bf = np.asarray(bv, np.float32), np.asarray(bf, np.int64)
    fv, ff = subdivide(*subdivide(bv, bf))
    rec = {"reps": a.reps, "target_vertices": 1000, "sources": {}}
    for name, v, f in (("bottle_3000", bv, bf), ("bottle_48000", fv, ff)):
        walls, mesh = [], None
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh = meshprep.make_watertight(v, f, target_vertices=1000)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        row = {"faces": int(len(f)), "make_watertight_ms": round(float(np.median(walls[1:])), 3), "resolution": mesh["resolution"],
               "probes": mesh["probes"], "out_vertices": int(len(mesh["vertices"])), "snapped": mesh["snapped"],
               "closed": mesh["topology"]["closed"], "oriented": mesh["topology"]["oriented"]}
        row["stages_at_chosen_resolution"] = stages(v, f, mesh["resolution"], a.reps)
        row["stages_at_resolution_64"] = stages(v, f, 64, a.reps)
        rec["sources"][name] = row
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
