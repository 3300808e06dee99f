#!/usr/bin/env python
"""Times the hand target masks of a clip (homan_amd.maskutils.add_target_hand_occlusions_clip -> hm_target_masks) at the
dataset walk's size - 30 frames of 640 x 640 float instance masks, one and two hands, REND_SIZE 256 - with device-resident
inputs, and prints one JSON line per configuration:

  call_ms     the clip-level call as a user makes it (box arithmetic on the host, stacking of the per-frame masks, ONE launch,
              K_roi), wall clock around a device synchronisation;
  kernel_ms   the hm_target_masks launch alone on already stacked masks (device events);
  model_bytes the traffic model - every mask read once plus the targets written - and model_GBps = model_bytes / kernel_ms;
  host_ms     (--host) the same crops and composition through the CPU restatement's torch form (tests/maskcrop_ref.py) on
              `--threads` threads, masks already on the host.

Each figure is the median of `--reps` timed runs after `--warmup` untimed ones, in one process.

usage: python tools/bench_maskutils.py [--reps R] [--warmup W] [--host] [--threads T] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from homan_amd import maskutils  # noqa: E402
from homan_amd.constants import REND_SIZE  # noqa: E402

FRAMES, IMAGE = 30, 640


def blob(cx, cy, rx, ry, device):
    """an elliptic instance mask (IMAGE, IMAGE), float 0 / 1"""
    y, x = torch.meshgrid(torch.arange(IMAGE, device=device), torch.arange(IMAGE, device=device), indexing="ij")
    return ((((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2) <= 1.0).float()


def make_clip(hands, device):
    """per-frame dicts of a clip: hands of ~150 pixels next to an object of ~250, drifting over the frames"""
    persons, objects = [], []
    for t in range(FRAMES):
        ox, oy = 320 + 2.0 * t, 330 - 1.5 * t
        obj = blob(ox, oy, 90, 125, device)
        centres = [(ox - 110, oy + 10), (ox + 115, oy - 20)][:hands]
        masks = torch.stack([blob(cx, cy, 75, 60, device) * (1 - obj) for cx, cy in centres])
        boxes = torch.tensor([[cx - 75, cy - 60, cx + 76, cy + 61] for cx, cy in centres], dtype=torch.float32)
        persons.append({"masks": masks, "bboxes": boxes})
        objects.append({"full_mask": obj})
    K = torch.tensor([[877.7, 0, 320.0], [0, 877.7, 320.0], [0, 0, 1.0]])
    return persons, objects, K


def median_ms(fn, warmup, reps, events):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        if events:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1))
        else:
            h0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - h0) * 1e3)
    return statistics.median(times)


def host_form(persons, objects, boxes):
    from tests.maskcrop_ref import crop_and_resize_torch
    out = []
    for p, o, b in zip(persons, objects, boxes):
        t = crop_and_resize_torch(p["masks"], b, REND_SIZE).float()
        t[crop_and_resize_torch(o["full_mask"][None].repeat(len(b), 1, 1), b, REND_SIZE)] = -1
        out.append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_maskutils needs the MI355X"
    dev = torch.device("cuda")
    records = []
    for hands in (1, 2):
        persons, objects, K = make_clip(hands, dev)
        call_ms = median_ms(lambda: maskutils.add_target_hand_occlusions_clip(persons, objects, K, square_expand=0.3),
                            a.warmup, a.reps, events=False)
        hm = torch.cat([p["masks"] for p in persons])
        om = torch.stack([o["full_mask"] for o in objects])
        boxes = torch.cat([p["square_bboxes"] for p in persons]).to(dev)
        frame_of = torch.arange(FRAMES).repeat_interleave(hands)[:, None]
        kernel_ms = median_ms(lambda: maskutils.target_masks(maskutils.MODE_HAND, hm, om, boxes, REND_SIZE, occluder_index=frame_of),
                              a.warmup, a.reps, events=True)
        model = hm.numel() * 4 + om.numel() * 4 + len(boxes) * REND_SIZE * REND_SIZE * 4
        rec = {"frames": FRAMES, "image": IMAGE, "hands": hands, "rois": len(boxes), "rend_size": REND_SIZE,
               "call_ms": round(call_ms, 4), "kernel_ms": round(kernel_ms, 4), "model_bytes": model,
               "model_GBps": float(f"{model / (kernel_ms * 1e-3) / 1e9:.4g}"), "reps": a.reps, "warmup": a.warmup,
               "device": torch.cuda.get_device_name(0)}
        if a.host:
            torch.set_num_threads(a.threads)
            hp = [{"masks": p["masks"].cpu()} for p in persons]
            ho = [{"full_mask": o["full_mask"].cpu()} for o in objects]
            hb = [p["square_bboxes"].cpu() for p in persons]
            want = host_form(hp, ho, hb)
            assert all(torch.equal(w, p["target_masks"].cpu()) for w, p in zip(want, persons)), "kernel and host form differ"
            times = []
            for _ in range(max(3, a.reps // 5)):
                h0 = time.perf_counter()
                host_form(hp, ho, hb)
                times.append((time.perf_counter() - h0) * 1e3)
            rec.update(host_ms=round(statistics.median(times), 2), host_threads=a.threads)
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(records, fh, indent=1)


if __name__ == "__main__":
    main()
