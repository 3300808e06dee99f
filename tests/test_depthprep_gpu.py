"""The kernels of csrc/depthprep.hip (hm_depth_register), `ops.register_depth`, `depthprep.prepare_depth_maps` / `SensorDepth`
and their wiring into HOMan, optimize_hand_object and ClipFitter.

Kernel against the fp32 NumPy restatement of tests/depthprep_ref.py: BIT FOR BIT, maps and statistics.  The pixel convention is
pinned against `ops.depth_render` on analytic scenes (ray-plane intersection in float64)."""
import numpy as np
import pytest
import torch

from tests import depthprep_ref as pref
from tests.test_softsil_gpu import _clip, _fit

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MM = F32(0.001)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(frames, scale, Kd, T, Kc, S, **opt):
    from homan_amd import ops
    f = frames if isinstance(frames, torch.Tensor) else _cu(frames)
    out, stats = ops.register_depth(f, scale, *[_cu(np.asarray(m, F32)) for m in (Kd, T, Kc)], S, **opt)
    return out.cpu().numpy(), stats.cpu().numpy()


def _same_bits(got, want, what=""):
    assert got[1].tolist() == want[1].tolist(), f"{what} stats {got[1].tolist()} / {want[1].tolist()}"
    diff = got[0].view(np.uint32) != want[0].view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} pixels differ, first at {np.argwhere(diff)[0].tolist()}"


def _scene(B, Hd, Wd, seed, dtype=np.uint16):
    """two surfaces, ramps and noise; depth steps EXACTLY on the kernel's tile borders (column 64, rows 16 and 32) and on the
    frame's border; every kind of invalid source value"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:Hd, :Wd]
    z = np.empty((B, Hd, Wd), F64)
    for b in range(B):
        far = 1.8 + 0.002 * xx + 0.001 * yy + 0.1 * b
        near = (yy >= Hd // 4) & (yy < 3 * Hd // 4) & (xx >= Wd // 3) & (xx < 2 * Wd // 3)
        z[b] = np.where(near, 0.9 + 0.001 * yy, far)
        z[b][:, 64:] += 0.3
        z[b][16:32] += 0.25
        z[b][0, :] -= 0.2
        z[b][:, -1] -= 0.2
        z[b][-1, :] += 0.15
        z[b] += rng.normal(0, 0.002, (Hd, Wd))
    bad = rng.random((B, Hd, Wd))
    if dtype == np.uint16:
        raw = np.rint(z * 1000).astype(np.uint16)
        raw[bad < 0.02] = 0
        raw[(bad >= 0.02) & (bad < 0.03)] = 65535
        raw[(bad >= 0.03) & (bad < 0.04)] = 50                      # 5 cm: below znear
        return raw
    raw = z.astype(F32)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -1.0, 0.0, 150.0, 0.05)):
        raw[(bad >= 0.006 * k) & (bad < 0.006 * (k + 1))] = v
    return raw


def _rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F64)


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], F64)


def _rigid(R=np.eye(3), t=(0, 0, 0)):
    return np.concatenate([np.asarray(R, F64), np.asarray(t, F64).reshape(3, 1)], 1)


# =============================================================================================== 1. identity
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("S", [1, 4, 16])
def test_identity_returns_the_scaled_frame(S, dtype):
    """same size, Kd = S * Kc, T = identity, no edge filter: frame * depth_scale where that is in range, 0 elsewhere"""
    frames = _scene(2, S, S, seed=S, dtype=dtype)
    scale = 0.001 if dtype == np.uint16 else 0.5
    Kc = pref.intrinsics(1.3, 0.5, 0.5)
    Kd = pref.intrinsics(1.3 * S, 0.5 * S, 0.5 * S)
    out, stats = _run(frames, scale, Kd, pref.IDENTITY, Kc, S, edge_radius=0)
    with np.errstate(invalid="ignore"):
        z = frames.astype(F32) * F32(scale)
        want = np.where((z >= F32(pref.NEAR)) & (z <= F32(pref.FAR)), z, F32(0)).astype(F32)
    assert out.tobytes() == want.tobytes()
    n = (want != 0).reshape(2, -1).sum(1)
    assert stats.tolist() == [[int(k), 0, 0, int(k)] for k in n]


# =============================================================================================== 2. kernel == restatement
_TX = _rigid(t=(0.03, -0.004, 0.002))
CASES = {
    # name: (B, Wd, Hd, S, ratio, dtype, T, per-frame matrices, options)
    "tiny_S1": (1, 7, 5, 1, 1.0, np.uint16, pref.IDENTITY, False, dict(edge_radius=0)),
    "tiny_S15_f32": (3, 7, 5, 15, 2.5, np.float32, pref.IDENTITY, False, dict()),
    "down_0.4": (1, 64, 48, 16, 0.4, np.uint16, pref.IDENTITY, False, dict()),
    "cap_bites": (3, 64, 48, 128, 2.5, np.uint16, _TX, False, dict(max_splat=2)),
    "parallax": (1, 64, 48, 128, 2.5, np.uint16, _rigid(t=(0.12, 0.02, 0.0)), False, dict(edge_radius=0)),
    "rotation_per_frame": (3, 97, 65, 128, 1.0, np.uint16, _rigid(_rot_y(0.05) @ _rot_z(0.03), (0.03, 0, 0.01)), True,
                           dict(edge_radius=3)),
    "rot180_f32": (1, 97, 65, 16, 0.4, np.float32, _rigid(_rot_z(np.pi)), False, dict()),
    "leaves_every_side": (1, 64, 48, 128, 7.9, np.uint16, pref.IDENTITY, False, dict(edge_radius=0)),
    "behind_znear_f32": (3, 64, 48, 15, 1.0, np.float32, _rigid(t=(0, 0, -0.9)), False, dict()),
    "tile_border_steps_r3": (1, 97, 65, 128, 1.0, np.uint16, pref.IDENTITY, False, dict(edge_radius=3, edge_jump_abs=0.05)),
    "tile_border_steps_r1_rel": (1, 97, 65, 128, 1.0, np.uint16, _TX, False, dict(edge_radius=1, edge_jump_abs=0.0, edge_jump_rel=0.02)),
    "f32_rows_of_four": (3, 64, 48, 16, 1.0, np.float32, _TX, True, dict(edge_radius=1)),
    "up_7.9": (1, 7, 5, 128, 7.9, np.uint16, _TX, False, dict(edge_radius=0)),
}


def _case(name):
    B, Wd, Hd, S, ratio, dtype, T, per_frame, opt = CASES[name]
    frames = _scene(B, Hd, Wd, seed=len(name) + S, dtype=dtype)
    Kd, Kc = pref.scaled_cameras(Hd, Wd, S, ratio)
    if per_frame:                              # another camera and another transform for every frame
        Kd = np.stack([Kd + np.array([[b, 0, 0.5 * b], [0, 2 * b, -0.25 * b], [0, 0, 0]]) for b in range(B)])
        Kc = np.stack([Kc + np.array([[0.01 * b, 0, 0.02 * b], [0, 0, -0.01 * b], [0, 0, 0]]) for b in range(B)])
        T = np.stack([T + _rigid(np.zeros((3, 3)), (0.01 * b, -0.005 * b, 0.0)) for b in range(B)])
    return frames, (0.001 if dtype == np.uint16 else 1.0), Kd, T, Kc, S, opt


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_restatement_bit_for_bit(name):
    frames, scale, Kd, T, Kc, S, opt = _case(name)
    want = pref.register32(frames, scale, Kd, T, Kc, S, **opt)
    got = _run(frames, scale, Kd, T, Kc, S, **opt)
    print(f"{name}: stats {got[1].tolist()}")
    _same_bits(got, want, name)
    st = want[1].sum(0)
    assert st[0] > 0
    if name in ("cap_bites", "behind_znear_f32"):
        assert st[2] > 0                        # the splat cap, the range rule
    if opt.get("edge_radius", 1) > 0 and frames.shape[2] > 7:
        assert st[1] > 0                        # the edge filter had something to remove
    if name != "tiny_S1":
        assert st[3] > 0


def test_shared_matrices_equal_per_frame_copies():
    frames, scale, Kd, T, Kc, S, opt = _case("cap_bites")
    B = frames.shape[0]
    shared = _run(frames, scale, Kd, T, Kc, S, **opt)
    copies = _run(frames, scale, np.stack([Kd] * B), np.stack([T] * B), np.stack([Kc] * B), S, **opt)
    _same_bits(copies, shared)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_a_view_one_element_off_an_aligned_base(dtype):
    """a contiguous view that is only element-aligned takes the element loads: the same bits as the 16-byte loads"""
    frames, scale, Kd, T, Kc, S, opt = _case("down_0.4" if dtype == np.uint16 else "f32_rows_of_four")
    Kd, T, Kc = (m[0] if m.ndim == 3 else m for m in (Kd, T, Kc))
    dev = _cu(frames)
    flat = torch.zeros(frames.size + 8, dtype=torch.int16 if dtype == np.uint16 else torch.float32, device="cuda").view(dev.dtype)
    assert dev.data_ptr() % 16 == 0 and flat.data_ptr() % 16 == 0
    view = flat[1:1 + frames.size].view(frames.shape)
    view.copy_(dev)
    assert view.is_contiguous() and view.data_ptr() % 16 == frames.itemsize
    want = pref.register32(frames, scale, Kd, T, Kc, S, **opt)
    _same_bits(_run(view, scale, Kd, T, Kc, S, **opt), want, "view")
    _same_bits(_run(dev, scale, Kd, T, Kc, S, **opt), want, "aligned")


# =============================================================================================== 3. determinism
def test_a_frame_has_the_same_bits_alone_first_and_last_and_twice():
    frames, scale, Kd, T, Kc, S, opt = _case("cap_bites")
    both = _run(frames, scale, Kd, T, Kc, S, **opt)
    again = _run(frames, scale, Kd, T, Kc, S, **opt)
    _same_bits(again, both, "second call")
    alone = _run(frames[:1], scale, Kd, T, Kc, S, **opt)
    last = _run(frames[[1, 2, 0]], scale, Kd, T, Kc, S, **opt)
    for name, (m, s) in (("alone", (alone[0][0], alone[1][0])), ("last", (last[0][2], last[1][2]))):
        assert m.tobytes() == both[0][0].tobytes() and s.tolist() == both[1][0].tolist(), name


# =============================================================================================== 4. against the renderer
def _hexahedron(front, back):
    """closed 8-vertex mesh: front = (x0, x1, y0, y1, z), back likewise -> (verts (8,3) float64, faces (12,3))"""
    def ring(x0, x1, y0, y1, z):
        return [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
    quads = [(0, 1, 2, 3), (4, 7, 6, 5), (0, 3, 7, 4), (1, 5, 6, 2), (0, 4, 5, 1), (3, 2, 6, 7)]
    faces = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return np.array(ring(*front) + ring(*back), F64), np.array(faces, np.int32)


def _render(verts, faces, Kc, S):
    from homan_amd import ops
    ctx = ops.SilhouetteContext(_cu(faces)[None], verts.shape[0], 1, S, torch.device("cuda"))
    sil, dep = ops.depth_render(_cu(verts.astype(F32))[None], _cu(np.asarray(Kc, F32))[None], ctx, 1.0)
    return sil[0].cpu().numpy(), dep[0].cpu().numpy()


# the round-trip scene, in the colour camera: a fronto-parallel face at z = 0.8 and a tilted one x = 0.02 + 1.5 (z - 0.8) up to
# z = 0.9; asymmetric in y and off-centre principal points, so that a flipped axis cannot hide
_FRONT, _BACK = (-0.12, 0.02, -0.10, 0.06, 0.8), (-0.12, 0.17, -0.10, 0.06, 0.9)


def _analytic_depth(K_px, centre, H, W):
    """depth along z (of a camera at `centre`, axes as the colour camera's) of the scene's two visible faces through the pixel
    centres of K_px, by ray-plane intersection in float64 -> (depth (H,W), 0 = no hit; face label 0 / 1 / 2)"""
    v, u = np.mgrid[:H, :W] + 0.5
    d = np.stack([(u - K_px[0, 2]) / K_px[0, 0], (v - K_px[1, 2]) / K_px[1, 1], np.ones_like(u)], -1)
    c = np.asarray(centre, F64)
    x0, x1, y0, y1, zf = _FRONT
    depth, label = np.full((H, W), np.inf), np.zeros((H, W), int)
    s = zf - c[2]                                                     # front: z = zf
    p = c + s * d
    hit = (p[..., 0] >= x0) & (p[..., 0] <= x1) & (p[..., 1] >= y0) & (p[..., 1] <= y1)
    depth, label = np.where(hit, s, depth), np.where(hit, 1, label)
    n, off = np.array([1.0, 0.0, -1.5]), x1 - 1.5 * zf                # tilted: x - 1.5 z = x1 - 1.5 zf
    s = (off - n @ c) / (d @ n)
    p = c + s[..., None] * d
    hit = (s > 0) & (p[..., 2] >= zf) & (p[..., 2] <= _BACK[4]) & (p[..., 1] >= y0) & (p[..., 1] <= y1) & (s < depth)
    depth, label = np.where(hit, s, depth), np.where(hit, 2, label)
    return np.where(label > 0, depth, 0.0), label


def test_round_trip_against_the_renderer():
    """A sensor frame of the box synthesised for a depth camera of another resolution (80 x 60) 3 cm aside, in uint16 millimetres,
    prepared onto the 64^2 grid of the colour camera and compared with ops.depth_render of the same box.
    Bound per pixel: half a millimetre of quantisation, plus the surface's depth slope per target pixel times (one target pixel:
    the render averages 2 x 2 samples inside it; plus one source pixel of footprint: the value written is the depth at the source
    pixel's centre, which projects anywhere inside the footprint that covers the target centre), plus 8 fp32 roundings of z."""
    from homan_amd import depthprep
    S, Wd, Hd = 64, 80, 60
    Kc = pref.intrinsics(2.0, 0.48, 0.53)
    Kc_px = Kc * np.array([[S], [S], [1]])
    Kd = pref.intrinsics(100.0, 40.0, 30.0)
    centre = np.array([0.03, 0.004, 0.002])                           # the depth camera, in the colour camera's frame
    T = _rigid(t=centre)
    sensor, _ = _analytic_depth(Kd, centre, Hd, Wd)
    frames = np.rint(sensor * 1000).astype(np.uint16)[None]
    assert (frames > 0).sum() > 500
    prepared, stats = depthprep.prepare_depth_maps(frames, Kd, Kc, S, depth_to_color=T, return_stats=True)
    prepared = prepared.cpu().numpy()[0]
    sil, dep = _render(*_hexahedron(_FRONT, _BACK), Kc, S)
    truth, label = _analytic_depth(Kc_px, np.zeros(3), S, S)
    # pixels at least two pixels off every edge: the same face in the whole 5 x 5 window
    pad = np.pad(label, 2)
    flat = np.ones((S, S), bool)
    for dy in range(5):
        for dx in range(5):
            flat &= pad[dy:dy + S, dx:dx + S] == label
    use = flat & (label > 0) & (sil == 1.0) & (prepared > 0)
    assert (use & (label == 1)).sum() >= 60 and (use & (label == 2)).sum() >= 60, ((use & (label == 1)).sum(), (use & (label == 2)).sum())
    assert use.sum() >= 0.9 * (flat & (label > 0)).sum()             # (nearly) every such pixel was measured and rendered
    ratio = Kc_px[0, 0] / Kd[0, 0]                                    # target pixels per source pixel
    for face in (1, 2):
        m = use & (label == face)
        t = np.where(label == face, truth, np.nan)
        with np.errstate(invalid="ignore"):
            slope = max(np.nanmax(np.abs(np.diff(t, axis=0))), np.nanmax(np.abs(np.diff(t, axis=1))))
        bound = 0.0005 + slope * (1.0 + ratio) + 8 * 2.0 ** -24 * 1.0
        err = np.abs(prepared.astype(F64) - dep.astype(F64))[m]
        err_truth = np.abs(prepared.astype(F64) - truth)[m]
        print(f"face {face}: {int(m.sum())} pixels, slope {slope:.5f} m / pixel, bound {bound:.5f} m, "
              f"max |prepared - render| {err.max():.5f} m, max |prepared - analytic| {err_truth.max():.5f} m")
        assert err.max() <= bound
    print("stats", stats.cpu().numpy().tolist())


@pytest.mark.parametrize("axis", ["column", "row"])
def test_a_depth_step_lands_on_its_column_and_on_the_renderers(axis):
    """Two fronto-parallel planes, the near one (0.7 m) from x* = 0.035 m on, the far one (1.0 m) everywhere, seen by a depth
    camera 3 cm to the left: the edge lies exactly on source column 46 (0.065 / 0.7 * 70 + 39.5) and on target column 37
    (0.035 / 0.7 * 128 + 30.6).  Prepared with the edge filter off, the near plane must start at column 37: half a pixel or a
    flipped axis moves it.  A box with its edge there, rendered by ops.depth_render, starts at the same column.  `row`: the same
    scene transposed."""
    from homan_amd import depthprep
    S, long_, short = 64, 80, 60
    swap = axis == "row"
    cut_src, cut_dst = 46, 37
    u = np.arange(long_)
    line = np.where(u >= cut_src, 700, 1000).astype(np.uint16)
    frames = (np.tile(line[:, None], (1, short)) if swap else np.tile(line[None, :], (short, 1)))[None]
    k_long, k_short = (70.0, 39.5), (70.0, 30.0)
    Kd = np.array([[k_short[0], 0, k_short[1]], [0, k_long[0], k_long[1]], [0, 0, 1]] if swap else
                  [[k_long[0], 0, k_long[1]], [0, k_short[0], k_short[1]], [0, 0, 1]], F64)
    c_long, c_short = 30.6 / S, 0.5
    Kc = pref.intrinsics(2.0, c_short, c_long) if swap else pref.intrinsics(2.0, c_long, c_short)
    t = (0.0, -0.03, 0.0) if swap else (-0.03, 0.0, 0.0)
    out = depthprep.prepare_depth_maps(frames, Kd, Kc, S, depth_to_color=_rigid(t=t), edge_radius=0).cpu().numpy()[0]
    out = out.T if swap else out
    near, far = F32(700) * MM, F32(1000) * MM
    assert (out[:, cut_dst:] == near).all() and (out[:, :cut_dst] == far).all(), np.unique(out, return_counts=True)
    # the renderer draws a box whose edge is at x* from the same column on
    front = (-0.3, 0.3, 0.035, 0.6, 0.7) if swap else (0.035, 0.6, -0.3, 0.3, 0.7)
    back = (-0.3, 0.3, 0.04, 0.6, 0.75) if swap else (0.04, 0.6, -0.3, 0.3, 0.75)      # (its edge projects inside the front's)
    sil, dep = _render(*_hexahedron(front, back), Kc, S)
    sil, dep = (sil.T, dep.T) if swap else (sil, dep)
    lo, hi = 32 - 15, 32 + 15                                         # rows well inside the box's +-0.3 m (+-55 pixels)
    assert (sil[lo:hi, cut_dst:] == 1.0).all() and (sil[lo:hi, :cut_dst] == 0.0).all()
    assert np.abs(dep[lo:hi, cut_dst:] - 0.7).max() < 1e-5


# =============================================================================================== 5. tiling
@pytest.mark.parametrize("Hd, Wd, S, ratio", pref.TILING_CASES)
def test_a_constant_frame_leaves_no_hole_on_the_device(Hd, Wd, S, ratio):
    Kd, Kc = pref.scaled_cameras(Hd, Wd, S, ratio)
    inside = pref.inside_source(Hd, Wd, S, Kd, Kc)
    for z in (0.7, 1.0, 3.3):
        frames = np.full((1, Hd, Wd), z, F32)
        out, stats = _run(frames, 1.0, Kd, pref.IDENTITY, Kc, S)
        assert (out[0][inside] == F32(z)).all(), f"{int((out[0][inside] == 0).sum())} holes"
        assert stats[0, 1] == 0 and stats[0, 2] == 0 and stats[0, 3] >= inside.sum()
        _same_bits((out, stats), pref.register32(frames, 1.0, Kd, pref.IDENTITY, Kc, S))


# =============================================================================================== 6. capture
def test_captured_call_follows_the_frames():
    from homan_amd import lib, ops
    frames, scale, Kd, T, Kc, S, opt = _case("cap_bites")
    other = _scene(*frames.shape, seed=99)
    assert (other != frames).any()
    f = _cu(frames)
    mats = [_cu(np.asarray(m, F32)) for m in (Kd, T, Kc)]
    out = torch.full((frames.shape[0], S, S), -1.0, device="cuda")
    stats = torch.full((frames.shape[0], 4), -1, dtype=torch.int32, device="cuda")
    first = _run(frames, scale, Kd, T, Kc, S, **opt)                 # (eager: the kernels are loaded before the capture)
    torch.cuda.synchronize()
    g = lib.new_graph()
    with torch.cuda.graph(g):
        ops.register_depth(f, scale, *mats, S, out=out, stats=stats, **opt)
    g.replay()
    _same_bits((out.cpu().numpy(), stats.cpu().numpy()), first, "first replay")
    f.copy_(_cu(other))
    g.replay()
    eager = _run(other, scale, Kd, T, Kc, S, **opt)
    _same_bits((out.cpu().numpy(), stats.cpu().numpy()), eager, "replay after the frames changed")
    _same_bits(eager, pref.register32(other, scale, Kd, T, Kc, S, **opt))


# =============================================================================================== 7. misaligned pointers
def test_misaligned_pointers_are_refused_and_nothing_is_launched():
    from homan_amd import lib
    B, Hd, Wd, S = 1, 8, 8, 4
    f16 = torch.full((B * Hd * Wd + 8,), 1000, dtype=torch.int16, device="cuda").view(torch.uint16)
    f32 = torch.full((B * Hd * Wd + 8,), 1.0, device="cuda")
    out = torch.full((B * S * S + 8,), -7.0, device="cuda")
    stats = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    Kd, Kc = pref.scaled_cameras(Hd, Wd, S, 0.5)
    kd, t, kc = (_cu(np.asarray(m, F32)) for m in (Kd, pref.IDENTITY, Kc))
    h = lib.lib()

    def call(frames, is_f32, o, st, k=kd.data_ptr(), size=S):
        return h.hm_depth_register(frames, is_f32, B, Hd, Wd, 0.001, k, 0, t.data_ptr(), 0, kc.data_ptr(), 0, size, 0.1, 100.0, 1, 0.02,
                                   0.0, 8, o, st, lib.stream())
    P = lambda x: x.data_ptr()
    bad = [call(P(f16) + 1, 0, P(out), P(stats)),                     # uint16 frames at an odd address
           call(P(f32) + 2, 1, P(out), P(stats)),                     # fp32 frames off their element
           call(P(f16), 0, P(out) + 4, P(stats)),                     # S * S % 4 == 0: out moves four pixels at a time
           call(P(f16), 0, P(out) + 8, P(stats)),
           call(P(f16), 0, P(out) + 2, P(stats), size=3),             # other sizes: element alignment
           call(P(f16), 0, P(out), P(stats) + 2),
           call(P(f16), 0, P(out), P(stats), k=P(kd) + 2)]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    assert (out == -7.0).all() and (stats == -7).all()
    # element-aligned views pass: frames one element off, out one float off at an odd size
    assert call(P(f16) + 2, 0, P(out) + 4, P(stats), size=3) == 0
    torch.cuda.synchronize()
    assert (out[:1] == -7.0).all() and (out[1:10] != -7.0).all() and (out[10:] == -7.0).all()
    assert (stats[:4] != -7).all() and (stats[4:] == -7).all()


# =============================================================================================== 8. end to end
def _sensor_of(mano, clip, Wd=80, Hd=60):
    """raw uint16 frames for a clip: the scene's own composed depth (tests/test_depthobs_gpu.py) seen as a sensor image of
    another resolution - resampled by nearest pixel on the host, which is all this test needs: both paths get the same frames"""
    from tests.test_depthobs_gpu import _with_depth
    clip, D = _with_depth(mano, clip)
    S = D.shape[-1]
    Kc = np.asarray(clip["camintr"], F64).reshape(-1, 3, 3)[0]
    Kd = np.array([[Kc[0, 0] * Wd, 0, Kc[0, 2] * Wd], [0, Kc[1, 1] * Hd, Kc[1, 2] * Hd], [0, 0, 1]], F64)
    rows = np.minimum(((np.arange(Hd) + 0.5) / Hd * S).astype(int), S - 1)
    cols = np.minimum(((np.arange(Wd) + 0.5) / Wd * S).astype(int), S - 1)
    frames = np.rint(D.numpy()[:, rows][:, :, cols] * 1000).astype(np.uint16)
    return clip, frames, Kd


def _weights():
    from homan_amd import synth
    return dict(synth.STEP1_LOSS_WEIGHTS, lw_depth_obs=100.0)


def test_sensor_depth_through_the_fit_equals_prepared_maps(mano_model):
    from homan_amd import depthprep
    clip, frames, Kd = _sensor_of(mano_model, _clip(mano_model, 91))
    T = _rigid(t=(0.01, 0.0, 0.0))
    maps = depthprep.prepare_depth_maps(frames, Kd, clip["camintr"], 64, depth_to_color=T)
    assert tuple(maps.shape) == (3, 64, 64) and maps.is_cuda and float((maps > 0).float().mean()) > 0.02
    sensor = depthprep.SensorDepth(frames, Kd, to_color=T)
    m_a, evo_a = _fit(mano_model, clip, _weights(), 4, "auto", depth_maps=sensor)
    m_b, evo_b = _fit(mano_model, clip, _weights(), 4, "auto", depth_maps=maps)
    assert torch.equal(m_a.depth_maps, maps) and torch.equal(m_b.depth_maps, maps)
    assert evo_a["loss_depth_obs"][0] > 0 and len(evo_a["loss"]) == 4
    for k in evo_b:
        np.testing.assert_array_equal(np.asarray(evo_a[k]), np.asarray(evo_b[k]), err_msg=k)
    for (k, a), (_, b) in zip(m_a.state_dict().items(), m_b.state_dict().items()):
        assert torch.equal(a, b), k
    # registered against the MODEL's intrinsics: other options reach the kernel, the wrong number of frames does not
    with pytest.raises(ValueError, match="holds 2 frames"):
        _fit(mano_model, clip, _weights(), 1, "auto", depth_maps=depthprep.SensorDepth(frames[:2], Kd))
    wide = depthprep.SensorDepth(frames, Kd, to_color=T, edge_radius=0)
    m_c, _ = _fit(mano_model, clip, _weights(), 1, "auto", depth_maps=wide)
    assert torch.equal(m_c.depth_maps, depthprep.prepare_depth_maps(frames, Kd, clip["camintr"], 64, depth_to_color=T, edge_radius=0))
    assert not torch.equal(m_c.depth_maps, maps)


def test_clip_fitter_takes_raw_frames(mano_model):
    from homan_amd import depthprep
    from homan_amd.jointopt import ClipFitter
    raw, prepared = [], []
    for seed in (92, 93):
        clip, frames, Kd = _sensor_of(mano_model, _clip(mano_model, seed))
        raw.append(dict(clip, depth_frames=torch.from_numpy(frames), depth_camintr=Kd, depth_scale=0.001))
        prepared.append(dict(clip, depth_maps=depthprep.prepare_depth_maps(frames, Kd, clip["camintr"], 64)))
    kw = dict(num_iterations=4, optimize_mano=True, image_size=64, mano_model=mano_model, rend_size=32)
    fit_raw, fit_prepared = ClipFitter(_weights(), **kw), ClipFitter(_weights(), **kw)
    got, want = fit_raw.fit(raw), fit_prepared.fit(prepared)
    # the second clip of the shape reuses the resident stepper: raw frames do not change the shape signature
    assert fit_raw.timing["built"] == 1 and fit_raw.timing["reused"] == 1
    more = fit_raw.fit(raw[:1])
    assert fit_raw.timing["built"] == 1 and fit_raw.timing["reused"] == 2
    for a, b in list(zip(got, want)) + [(more[0], want[0])]:
        assert a["loss_evolution"]["loss_depth_obs"][0] > 0
        for k in b["loss_evolution"]:
            np.testing.assert_array_equal(np.asarray(a["loss_evolution"][k]), np.asarray(b["loss_evolution"][k]), err_msg=k)
        for k in b["state_dict"]:
            assert torch.equal(a["state_dict"][k], b["state_dict"][k]), k
        assert torch.equal(a["verts_object"], b["verts_object"]) and torch.equal(a["verts_hand"], b["verts_hand"])
    with pytest.raises(ValueError, match="both depth_frames and depth_maps"):
        fit_raw.fit([dict(raw[0], depth_maps=prepared[0]["depth_maps"])])
