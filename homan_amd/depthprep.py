"""Raw sensor depth onto the fit's pixel grid: what `depth_maps=` of HOMan / build_model / optimize_hand_object takes, made from
what an RGB-D camera delivers - uint16 (or float) frames at the sensor's own resolution, in its own units, seen from a depth
camera with its own intrinsics and a baseline to the colour camera.

`prepare_depth_maps` is ONE call of hm_depth_register (csrc/depthprep.hip; the rule - validity, the edge filter that removes
flying pixels on the source grid, the footprint splat, the minimum merge - is in include/homan_amd.h and DESIGN.md section 7).
`SensorDepth` carries frames and their camera to wherever `depth_maps` is accepted, so that they are registered against the
intrinsics and size the fit itself uses.  A homan_amd extra, not in the reference tree.  Frames and matrices may be tensors on
any device or arrays; the result lives on the GPU.  There is no CPU path: without a GPU these functions raise, after every
check of their arguments."""
import numpy as np
import torch

from . import lib, ops

# UNTUNED defaults: no real sensor has been registered with them yet
DEFAULTS = dict(pixel_center=0.5, znear=ops.NMR_NEAR, zfar=ops.NMR_FAR, edge_radius=1, edge_jump_abs=0.02, edge_jump_rel=0.0,
                max_splat=8)
MAX_SIZE = 1024                                   # the depth term's limit (hm_depth_obs_fwd)
DEFAULT_CAMINTR = ((1.0, 0.0, 0.5), (0.0, 1.0, 0.5), (0.0, 0.0, 1.0))        # HOMan's camintr=None


def _device(*tensors):
    if not torch.cuda.is_available():
        raise lib.HomanAmdError("homan_amd.depthprep needs the GPU (there is no CPU fallback)")
    return next((t.device for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda), torch.device("cuda"))


def _frames_arg(frames, depth_scale):
    """(B,Hd,Wd) frames -> (tensor of uint16 or a float type, where the caller has it; metres per unit)"""
    f = frames.detach() if isinstance(frames, torch.Tensor) else torch.as_tensor(np.asarray(frames))
    if f.dim() != 3 or 0 in f.shape:
        raise ValueError(f"depth frames: expected non-empty (B, Hd, Wd), got {tuple(f.shape)}")
    if f.dtype != torch.uint16 and not f.dtype.is_floating_point:
        raise ValueError(f"depth frames of dtype {f.dtype}: uint16 (sensor units) or a float type (packed encodings are combined "
                         "into uint16 by the caller)")
    scale = (0.001 if f.dtype == torch.uint16 else 1.0) if depth_scale is None else float(depth_scale)
    if not 0 < scale < float("inf"):
        raise ValueError(f"depth_scale {depth_scale} must be a positive number (metres per unit)")
    return f, scale


def _host(m):
    return np.asarray(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m, dtype=np.float64)


def _intrinsics_arg(name, K, frames):
    """(3,3) or (frames,3,3) -> float64 host array of that shape, checked: finite, no skew, last row 0 0 1, non-zero focal lengths"""
    k = _host(K)
    if k.shape == (1, 3, 3):
        k = k[0]
    if k.shape not in ((3, 3), (frames, 3, 3)):
        raise ValueError(f"{name} of shape {k.shape}: expected (3, 3) or ({frames}, 3, 3)")
    if not np.isfinite(k).all():
        raise ValueError(f"{name} holds a non-finite entry")
    if (k[..., 0, 1] != 0).any() or (k[..., 1, 0] != 0).any() or (k[..., 2, :] != np.array([0.0, 0.0, 1.0])).any():
        raise ValueError(f"{name}: only fx, fy, cx, cy are read - skew, and a last row other than 0 0 1, are refused")
    if (k[..., 0, 0] == 0).any() or (k[..., 1, 1] == 0).any():
        raise ValueError(f"{name}: zero focal length")
    return k


def _transform_arg(T, frames):
    """None, (3,4) / (4,4) or per frame -> float64 host (3,4) or (frames,3,4), finite"""
    if T is None:
        return np.eye(3, 4)
    t = _host(T)
    if t.shape[-2:] == (4, 4):
        if (t[..., 3, :] != np.array([0.0, 0.0, 0.0, 1.0])).any():
            raise ValueError("depth_to_color (4, 4): the last row must be 0 0 0 1")
        t = t[..., :3, :]
    if t.shape == (1, 3, 4):
        t = t[0]
    if t.shape not in ((3, 4), (frames, 3, 4)):
        raise ValueError(f"depth_to_color of shape {t.shape}: expected (3, 4), (4, 4) or one per frame ({frames})")
    if not np.isfinite(t).all():
        raise ValueError("depth_to_color holds a non-finite entry")
    return np.ascontiguousarray(t)


def check_options(pixel_center=0.5, znear=ops.NMR_NEAR, zfar=ops.NMR_FAR, edge_radius=1, edge_jump_abs=0.02, edge_jump_rel=0.0,
                  max_splat=8):
    """the options of prepare_depth_maps, checked on the host -> dict"""
    if float(pixel_center) not in (0.0, 0.5):
        raise ValueError(f"pixel_center {pixel_center} not in [0.5|0.0] (where the intrinsics put the centre of pixel 0)")
    if not 0 < float(znear) < float(zfar) <= 100:
        raise ValueError(f"znear {znear} / zfar {zfar}: need 0 < znear < zfar <= 100 (metres)")
    if int(edge_radius) != edge_radius or not 0 <= int(edge_radius) <= 3:
        raise ValueError(f"edge_radius {edge_radius} not in 0..3 (pixels of the source grid; 0 turns the filter off)")
    for name, v in (("edge_jump_abs", edge_jump_abs), ("edge_jump_rel", edge_jump_rel)):
        if not 0 <= float(v) < float("inf"):
            raise ValueError(f"{name} {v} must be a non-negative number")
    if int(max_splat) != max_splat or int(max_splat) < 1:
        raise ValueError(f"max_splat {max_splat} must be a positive integer (target pixels per source pixel and direction)")
    return dict(pixel_center=float(pixel_center), znear=float(znear), zfar=float(zfar), edge_radius=int(edge_radius),
                edge_jump_abs=float(edge_jump_abs), edge_jump_rel=float(edge_jump_rel), max_splat=int(max_splat))


def _check_size(image_size):
    if int(image_size) != image_size or not 1 <= int(image_size) <= MAX_SIZE:
        raise ValueError(f"image_size {image_size} not in 1..{MAX_SIZE} (the observed-depth term's limit)")
    return int(image_size)


def prepare_depth_maps(frames, depth_camintr, camintr, image_size, depth_to_color=None, depth_scale=None, pixel_center=0.5,
                       znear=ops.NMR_NEAR, zfar=ops.NMR_FAR, edge_radius=1, edge_jump_abs=0.02, edge_jump_rel=0.0, max_splat=8,
                       return_stats=False):
    """Sensor frames -> the (B, image_size, image_size) fp32 device tensor `depth_maps=` takes: metres in the colour camera,
    registered with the pixels ops.depth_render draws under `camintr`, exactly 0 where nothing was measured.
    frames (B,Hd,Wd): uint16 or float; depth_scale: metres per unit (default 0.001 for uint16, 1 for floats).
    depth_camintr: the depth camera's PIXEL intrinsics, (3,3) or (B,3,3); pixel_center=0.5 means pixel (row v, column u) covers
    [u, u+1) x [v, v+1) in their units, 0.0 that they were calibrated with integer pixel centres (the principal point is shifted
    by half a pixel on the host).  depth_to_color: (3,4) / (4,4) rigid transform from the depth to the colour camera, or one per
    frame; default identity.  camintr: the model's intrinsics, normalised by image_size exactly as HOMan takes them, (3,3) or
    (B,3,3); None = HOMan's default.  The other options are those of the rule (include/homan_amd.h); their defaults are UNTUNED.
    return_stats=True appends the (B,4) int32 counts: valid source pixels, dropped by the edge filter, dropped by the range /
    splat rules, valid target pixels."""
    f, scale = _frames_arg(frames, depth_scale)
    B = f.shape[0]
    opt = check_options(pixel_center, znear, zfar, edge_radius, edge_jump_abs, edge_jump_rel, max_splat)
    size = _check_size(image_size)
    kd = _intrinsics_arg("depth_camintr", depth_camintr, B).copy()
    kd[..., :2, 2] += 0.5 - opt.pop("pixel_center")
    t = _transform_arg(depth_to_color, B)
    kc = _intrinsics_arg("camintr", DEFAULT_CAMINTR if camintr is None else camintr, B)
    dev = _device(f)
    f = f.to(dev)
    if f.dtype != torch.uint16:
        f = f.float()
    with torch.cuda.device(dev):
        mats = [torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(dev) for m in (kd, t, kc)]
        out, stats = ops.register_depth(f, scale, *mats, size, **opt)
    return (out, stats) if return_stats else out


class SensorDepth:
    """Raw depth frames with their camera, for every place that takes `depth_maps`: HOMan, build_model, optimize_hand_object and
    HOMan.load_clip register them with the model's OWN `camintr` and `image_size` (prepare_depth_maps), so the maps cannot be made
    for other intrinsics than the fit uses.  frames (B,Hd,Wd) uint16 or float, camintr: the depth camera's pixel intrinsics,
    to_color: depth -> colour transform (default identity), scale: metres per unit, options: those of prepare_depth_maps."""

    def __init__(self, frames, camintr, to_color=None, scale=None, **options):
        unknown = set(options) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"SensorDepth: unknown option(s) {sorted(unknown)}; known: {sorted(DEFAULTS)}")
        f, _ = _frames_arg(frames, scale)
        check_options(**options)
        _intrinsics_arg("SensorDepth camintr", camintr, f.shape[0])
        _transform_arg(to_color, f.shape[0])
        self.frames, self.camintr, self.to_color, self.scale, self.options = frames, camintr, to_color, scale, dict(options)
        self.shape = tuple(f.shape)

    def check(self, frames, image_size):
        """host-side: one depth frame per frame of the clip, a size the depth term takes"""
        if self.shape[0] != int(frames):
            raise ValueError(f"SensorDepth holds {self.shape[0]} frames, the clip has {int(frames)}")
        _check_size(image_size)

    def prepare(self, camintr, image_size, return_stats=False):
        return prepare_depth_maps(self.frames, self.camintr, camintr, image_size, depth_to_color=self.to_color,
                                  depth_scale=self.scale, return_stats=return_stats, **self.options)


def clip_sensor_depth(clip):
    """The SensorDepth of a clip dictionary that brings raw frames - clip["depth_frames"] with clip["depth_camintr"], optionally
    clip["depth_to_color"], clip["depth_scale"] and clip["depth_options"] - or None.  A clip that brings both raw frames and
    prepared clip["depth_maps"] is refused."""
    if clip.get("depth_frames") is None:
        return None
    if clip.get("depth_maps") is not None:
        raise ValueError("the clip brings both depth_frames and depth_maps: pass the raw frames or the prepared maps, not both")
    if clip.get("depth_camintr") is None:
        raise ValueError("clip['depth_frames'] needs clip['depth_camintr'] (the depth camera's pixel intrinsics)")
    return SensorDepth(clip["depth_frames"], clip["depth_camintr"], clip.get("depth_to_color"), clip.get("depth_scale"),
                       **(clip.get("depth_options") or {}))
