"""CPU restatement of detectron2's `BitMasks.crop_and_resize` (ROIAlign, output (S,S), spatial_scale 1, sampling_ratio 0,
aligned, on the binarised mask as fp32, then >= 0.5) - what csrc/maskcrop.hip is compared with, pixel for pixel.

detectron2 is a third-party leaf without source in the reference tree: this is written from the published algorithm and is
PARITY-UNPINNED.  Every operation is rounded to fp32 and the samples of an output pixel are added one by one,
rows (iy) outside, columns (ix) inside:

    sx = x1 - 0.5 ; sy = y1 - 0.5 ; rw = x2 - x1 ; rh = y2 - y1
    bw = rw / S ; bh = rh / S ; gw = max(ceil(rw / S), 1) ; gh = max(ceil(rh / S), 1)
    sample (iy, ix) of output (ph, pw):  y = (sy + ph*bh) + ((iy + .5)*bh) / gh ,  x likewise
    bilinear(y, x): 0 if y < -1 or y > H or x < -1 or x > W; clamp y, x to >= 0;
                    yl = (int)y; if yl >= H-1 { yl = yh = H-1; y = yl } else yh = yl+1; same in x;
                    ly = y-yl, lx = x-xl, hy = 1-ly, hx = 1-lx;
                    v = ((hy*hx)*m[yl,xl] + (hy*lx)*m[yl,xh]) + ((ly*hx)*m[yh,xl] + (ly*lx)*m[yh,xh])
    out = (sum over iy then ix of v) / (gh*gw) >= 0.5

`crop_and_resize` is the numpy form (vectorised over the pixels of one box), `crop_and_resize_torch` the same operations on
torch CPU tensors (tools/bench_maskutils.py times it as the host alternative).
"""
import math

import numpy as np
import torch

F = np.float32


def _axis(c, n):
    """sample coordinates c (S,) along an axis of n pixels -> (inside, low index, high index, low weight l, high weight h)"""
    inside = (c >= F(-1.0)) & (c <= F(n))
    c = np.where(inside, np.maximum(c, F(0.0)), F(0.0)).astype(F)
    lo = c.astype(np.int64)
    top = lo >= n - 1
    lo = np.where(top, n - 1, lo)
    hi = np.where(top, n - 1, lo + 1)
    c = np.where(top, lo.astype(F), c)
    l = (c - lo.astype(F)).astype(F)
    return inside, lo, hi, l, (F(1.0) - l).astype(F)


def crop_one(mask, box, size):
    """mask (H,W) of any dtype (binarised as != 0), box x1 y1 x2 y2 -> bool (size, size)"""
    m = (np.asarray(mask) != 0).astype(F)
    H, W = m.shape
    x1, y1, x2, y2 = [F(v) for v in np.asarray(box, dtype=F)]
    S = F(size)
    sx, sy, rw, rh = F(x1 - F(0.5)), F(y1 - F(0.5)), F(x2 - x1), F(y2 - y1)
    bw, bh = F(rw / S), F(rh / S)
    gw, gh = int(max(math.ceil(F(rw / S)), 1)), int(max(math.ceil(F(rh / S)), 1))
    p = np.arange(size, dtype=F)
    y0, x0 = (sy + p * bh).astype(F), (sx + p * bw).astype(F)
    acc = np.zeros((size, size), F)
    for iy in range(gh):
        in_y, yl, yh, ly, hy = _axis((y0 + F(F(F(iy) + F(0.5)) * bh) / F(gh)).astype(F), H)
        for ix in range(gw):
            in_x, xl, xh, lx, hx = _axis((x0 + F(F(F(ix) + F(0.5)) * bw) / F(gw)).astype(F), W)
            v = ((hy[:, None] * hx[None, :]) * m[np.ix_(yl, xl)] + (hy[:, None] * lx[None, :]) * m[np.ix_(yl, xh)]) \
                + ((ly[:, None] * hx[None, :]) * m[np.ix_(yh, xl)] + (ly[:, None] * lx[None, :]) * m[np.ix_(yh, xh)])
            assert v.dtype == F
            acc = acc + np.where(in_y[:, None] & in_x[None, :], v, F(0.0))
    return (acc / F(gh * gw)) >= F(0.5)


def crop_and_resize(masks, boxes, size, index=None):
    """masks (N,H,W), boxes (R,4), index (R) (default: box r crops mask r) -> bool (R,size,size), numpy"""
    masks = np.asarray(masks)
    boxes = np.asarray(boxes, dtype=F).reshape(-1, 4)
    index = np.arange(len(boxes)) if index is None else np.asarray(index)
    assert len(index) == len(boxes)
    out = np.zeros((len(boxes), size, size), bool)
    for r, (n, box) in enumerate(zip(index, boxes)):
        out[r] = crop_one(masks[n], box, size)
    return out


def _axis_t(c, n):
    inside = (c >= -1.0) & (c <= float(n))
    c = torch.where(inside, c.clamp(min=0.0), torch.zeros_like(c))
    lo = c.long()
    top = lo >= n - 1
    lo = torch.where(top, torch.full_like(lo, n - 1), lo)
    hi = torch.where(top, lo, lo + 1)
    c = torch.where(top, lo.float(), c)
    l = c - lo.float()
    return inside, lo, hi, l, 1.0 - l


def crop_and_resize_torch(masks, boxes, size, index=None):
    """`crop_and_resize` on torch CPU tensors (fp32, the same operations in the same order) -> bool (R,size,size)"""
    masks = torch.as_tensor(masks)
    boxes = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    index = range(len(boxes)) if index is None else torch.as_tensor(index).tolist()
    out = torch.zeros(len(boxes), size, size, dtype=torch.bool)
    p = torch.arange(size, dtype=torch.float32)
    one = torch.ones((), dtype=torch.float32)
    for r, n in enumerate(index):
        m = (masks[n] != 0).float()
        H, W = m.shape
        x1, y1, x2, y2 = boxes[r]
        sx, sy, rw, rh = x1 - 0.5, y1 - 0.5, x2 - x1, y2 - y1
        bw, bh = rw / size, rh / size
        gw, gh = int(max(math.ceil(float(bw)), 1)), int(max(math.ceil(float(bh)), 1))
        y0, x0 = sy + p * bh, sx + p * bw
        acc = torch.zeros(size, size)
        for iy in range(gh):
            in_y, yl, yh, ly, hy = _axis_t(y0 + ((iy + 0.5) * one * bh) / gh, H)
            for ix in range(gw):
                in_x, xl, xh, lx, hx = _axis_t(x0 + ((ix + 0.5) * one * bw) / gw, W)
                top, bot = m[yl], m[yh]
                v = ((hy[:, None] * hx[None, :]) * top[:, xl] + (hy[:, None] * lx[None, :]) * top[:, xh]) \
                    + ((ly[:, None] * hx[None, :]) * bot[:, xl] + (ly[:, None] * lx[None, :]) * bot[:, xh])
                acc = acc + torch.where(in_y[:, None] & in_x[None, :], v, torch.zeros_like(v))
        out[r] = (acc / float(gh * gw)) >= 0.5
    return out


class BitMasks:
    """The part of detectron2.structures.BitMasks the reference uses: a (N,H,W) tensor binarised on construction and
    `crop_and_resize(boxes, mask_size)`, one box per mask, -> bool tensor (N, mask_size, mask_size)."""

    def __init__(self, tensor):
        tensor = torch.as_tensor(tensor).to(torch.bool)
        assert tensor.dim() == 3, tensor.size()
        self.tensor = tensor
        self.image_size = tensor.shape[1:]

    def __len__(self):
        return self.tensor.shape[0]

    def crop_and_resize(self, boxes, mask_size):
        assert len(boxes) == len(self), "{} != {}".format(len(boxes), len(self))
        boxes = torch.as_tensor(boxes).detach().cpu().float().numpy()
        return torch.from_numpy(crop_and_resize(self.tensor.cpu().numpy(), boxes, mask_size))
