"""Bounding-box helpers of reference homan/utils/bbox.py:42-89 (`make_bbox_square`, `bbox_xy_to_wh`, `bbox_wh_to_xy`) in
numpy, on the host.  The two conversions are what the reference asks of detectron2's `BoxMode.convert` (XYXY_ABS <->
XYWH_ABS): they keep the type (tensor, array, list, tuple), the dtype and the shape of what they are given."""
import numpy as np
import torch


def _numpify(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def make_bbox_square(bbox, bbox_expansion=0.0):
    """bbox (4 or B x 4) in xywh -> the square box of side max(w, h) * (1 + bbox_expansion) around the same centre, as a
    numpy array of the same shape (reference bbox.py:42-61, same operations in the same order and dtype)."""
    bbox = _numpify(bbox)
    original_shape = bbox.shape
    bbox = bbox.reshape(-1, 4)
    center = np.stack((bbox[:, 0] + bbox[:, 2] / 2, bbox[:, 1] + bbox[:, 3] / 2), axis=1)
    b = np.expand_dims(np.maximum(bbox[:, 2], bbox[:, 3]), 1)
    b *= 1 + bbox_expansion
    square_bboxes = np.hstack((center - b / 2, b, b))
    return square_bboxes.reshape(original_shape)


def _convert(bbox, sign):
    """columns 2:4 += sign * columns 0:2, on a copy, type preserved (BoxMode.convert for the two modes used)"""
    if isinstance(bbox, (tuple, list)):
        assert len(bbox) == 4, "a box given as a list or tuple has 4 entries"
        arr = torch.tensor(bbox)[None, :]
        arr[:, 2:] += sign * arr[:, :2]
        return type(bbox)(arr.flatten().tolist())
    original_shape = bbox.shape
    arr = torch.from_numpy(np.asarray(bbox)).clone() if isinstance(bbox, np.ndarray) else bbox.clone()
    arr = arr.reshape((-1, 4))
    if sign > 0:
        arr[:, 2] += arr[:, 0]
        arr[:, 3] += arr[:, 1]
    else:
        arr[:, 2] -= arr[:, 0]
        arr[:, 3] -= arr[:, 1]
    arr = arr.reshape(original_shape)
    return arr.numpy() if isinstance(bbox, np.ndarray) else arr


def bbox_xy_to_wh(bbox):
    """x1 y1 x2 y2 -> x1 y1 w h (reference bbox.py:64-75)"""
    return _convert(bbox, -1)


def bbox_wh_to_xy(bbox):
    """x1 y1 w h -> x1 y1 x2 y2 (reference bbox.py:78-89)"""
    return _convert(bbox, +1)
