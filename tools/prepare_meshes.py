#!/usr/bin/env python
"""Prepares a list of object meshes for the fits: each `X.obj` (or `.off`) named in a text file, one path per line, becomes the
watertight `X_proc.obj` of at most `--vertex_nb` vertices and the pickle `X_proc.pkl` {"vertices", "faces"} beside it
(homan_amd/meshprep.py simplify_mesh; the walk of the reference's shapemeshprocess.py, without its two external programs).
A source whose pickle already exists is skipped.

usage: python tools/prepare_meshes.py [--file_path extra_data/objmodels.txt] [--vertex_nb 1000] [--detail_resolution 64]"""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from homan_amd import meshprep  # noqa: E402


def targets(src):
    stem, ext = os.path.splitext(src)
    return stem + "_proc" + ext, stem + "_proc.pkl"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--file_path", default="extra_data/objmodels.txt", help="text file with one mesh path per line")
    ap.add_argument("--vertex_nb", type=int, default=1000, help="vertex budget of the prepared mesh")
    ap.add_argument("--detail_resolution", type=int, default=None,
                    help="off by default; an integer in [2, 256]: surface nets at that fine lattice, then edge-collapse "
                         "decimation to --vertex_nb (keeps parts thinner than a cell of the budget lattice)")
    ap.add_argument("--manifold_path", default=None, help="accepted for the reference's command line; unused")
    ap.add_argument("--acvd_path", default=None, help="accepted for the reference's command line; unused")
    a = ap.parse_args(argv)
    with open(a.file_path) as fh:
        sources = sorted({line.strip() for line in fh if line.strip()})
    done = 0
    for src in sources:
        target, pkl = targets(src)
        if os.path.exists(pkl):
            print(f"{src}: {pkl} exists, skipped")
            continue
        if not os.path.exists(src):
            raise FileNotFoundError(src)
        extra = {} if a.detail_resolution is None else {"detail_resolution": a.detail_resolution}
        mesh = meshprep.simplify_mesh(src, target, vert_nb=a.vertex_nb, **extra)
        if "rounds" in mesh:
            print(f"{src}: {mesh['detail_vertices']} vertices off the fine lattice, {mesh['rounds']} rounds of collapses, "
                  f"budget {'met' if mesh['reached'] else 'NOT met'}")
        print(f"{src}: {len(mesh['vertices'])} vertices, {len(mesh['faces'])} faces at resolution {mesh['resolution']} -> {target}")
        done += 1
    return done


if __name__ == "__main__":
    main()
