"""CPU side of the depth registration (csrc/depthprep.hip, ops.register_depth, homan_amd/depthprep.py): the fp32 NumPy restatement
tests/depthprep_ref.py - which the GPU tests hold the kernels to bit for bit - against known answers worked out in float64, the
tiling property of the footprint splat, and every refusal that needs no device."""
import numpy as np
import pytest
import torch

from tests import depthprep_ref as pref

F32, F64 = np.float32, np.float64


def _same_camera(S, f=1.0):
    """(Kd, Kc) of ONE camera at size S: Kd = S * Kc"""
    return pref.intrinsics(f * S, S / 2.0, S / 2.0), pref.intrinsics(f, 0.5, 0.5)


# =============================================================================================== known answers
def test_a_shifted_camera_moves_a_fronto_parallel_plane_by_f_t_over_z():
    S, z, tx, ty = 32, 2.0, 0.25, -0.125                     # f t / z = 32 * 0.25 / 2 = 4 columns, 32 * -0.125 / 2 = -2 rows
    Kd, Kc = _same_camera(S)
    frame = np.zeros((1, S, S), F32)
    frame[0, 6:20, 5:17] = z
    T = np.array([[1, 0, 0, tx], [0, 1, 0, ty], [0, 0, 1, 0]], F64)
    px, py, zc = pref.project64(5.0, 6.0, z, Kd, T, Kc, S)   # the float64 geometry: the patch's corner lands 4 right, 2 up
    assert (px, py, zc) == (9.0, 4.0, z)
    out, stats = pref.register32(frame, 1.0, Kd, T, Kc, S, edge_radius=0)
    want = np.zeros((S, S), F32)
    want[4:18, 9:21] = z
    assert np.array_equal(out[0], want)
    assert stats.tolist() == [[14 * 12, 0, 0, 14 * 12]]
    # a shift along the axis changes the depth written, not only the place: zc is the depth in the COLOUR camera
    T[2, 3] = 0.5
    out, _ = pref.register32(frame, 1.0, Kd, T, Kc, S, edge_radius=0)
    assert set(np.unique(out)) == {F32(0.0), F32(2.5)}


def test_invalid_source_values():
    S = 4
    Kd, Kc = _same_camera(S)
    u16 = np.array([[[0, 65535, 1000, 99], [100, 100, 100, 100], [100, 100, 100, 100], [100, 100, 100, 100]]], np.uint16)
    out, stats = pref.register32(u16, 0.001, Kd, pref.IDENTITY, Kc, S, edge_radius=0)
    # 0 is no measurement, 65535 * 0.001 = 65.5 m is in range (znear 0.1, zfar 100), 99 * 0.001 is below znear
    assert out[0, 0].tolist() == [0.0, float(F32(65535) * F32(0.001)), float(F32(1000) * F32(0.001)), 0.0]
    assert stats[0, 0] == 14 and stats[0, 3] == 14
    out, stats = pref.register32(u16, 0.01, Kd, pref.IDENTITY, Kc, S, edge_radius=0)          # 655.35 m: beyond zfar
    assert out[0, 0, 1] == 0.0 and stats[0, 0] == 14
    f32 = np.full((1, S, S), 1.5, F32)
    f32[0, 0] = [np.nan, np.inf, -np.inf, -1.5]
    f32[0, 1, :2] = [0.0, 100.5]
    out, stats = pref.register32(f32, 1.0, Kd, pref.IDENTITY, Kc, S, edge_radius=0)
    assert not out[0, 0].any() and not out[0, 1, :2].any() and (out[0, 1, 2:] == 1.5).all() and (out[0, 2:] == 1.5).all()
    assert stats.tolist() == [[10, 0, 0, 10]]
    # depth_scale multiplies float frames too
    out, _ = pref.register32(f32, 2.0, Kd, pref.IDENTITY, Kc, S, edge_radius=0)
    assert (out[0, 2:] == 3.0).all()


@pytest.mark.parametrize("r", [1, 2, 3])
def test_edge_filter_removes_exactly_the_pixels_within_r_of_a_step(r):
    S, col = 16, 9
    Kd, Kc = _same_camera(S)
    frame = np.full((1, S, S), 1.0, F32)
    frame[0, :, col:] = 1.0 + 0.0625                        # a step of 6.25 cm between columns 8 and 9 (exact in fp32)
    out, stats = pref.register32(frame, 1.0, Kd, pref.IDENTITY, Kc, S, edge_radius=r, edge_jump_abs=0.05)
    gone = np.zeros((S, S), bool)
    gone[:, col - r:col + r] = True
    assert np.array_equal(out[0] == 0, gone) and np.array_equal(out[0][~gone], frame[0][~gone])
    assert stats.tolist() == [[S * S, 2 * r * S, 0, S * S - 2 * r * S]]
    # a step below the threshold removes nothing; neither does one AT it (the comparison is strict)
    for thr in (0.07, 0.0625):
        out, stats = pref.register32(frame, 1.0, Kd, pref.IDENTITY, Kc, S, edge_radius=r, edge_jump_abs=thr)
        assert np.array_equal(out, frame) and stats[0, 1] == 0
    # the relative part scales with the pixel's own depth: 0.06 * 1.0 < 0.0625 < 0.06 * 1.0625, so only the near side goes
    out, stats = pref.register32(frame, 1.0, Kd, pref.IDENTITY, Kc, S, edge_radius=r, edge_jump_abs=0.0, edge_jump_rel=0.06)
    near = np.zeros((S, S), bool)
    near[:, col - r:col] = True
    assert np.array_equal(out[0] == 0, near)
    # invalid neighbours and the frame's border do not vote: a hole next to a flat surface removes nothing
    frame = np.full((1, S, S), 1.0, F32)
    frame[0, 5, 5] = 0.0
    out, stats = pref.register32(frame, 1.0, Kd, pref.IDENTITY, Kc, S, edge_radius=r, edge_jump_abs=0.05)
    assert stats.tolist() == [[S * S - 1, 0, 0, S * S - 1]]


def test_a_footprint_larger_than_max_splat_is_dropped_and_counted():
    S = 16
    Kd = pref.intrinsics(1.0, 0.5, 0.5)                                # ONE source pixel ...
    Kc = pref.intrinsics(5.0 / S, 0.5, 0.5)                              # ... that covers 5 x 5 target pixels around the centre
    frame = np.full((1, 1, 1), 2.0, F32)
    out, stats = pref.register32(frame, 1.0, Kd, pref.IDENTITY, Kc, S, edge_radius=0, max_splat=5)
    assert int((out != 0).sum()) == 25 and stats.tolist() == [[1, 0, 0, 25]]
    lo, hi = pref.project64([0.0, 1.0], [0.0, 1.0], 2.0, Kd, pref.IDENTITY, Kc, S)[0]
    assert (lo, hi) == (5.5, 10.5) and (out[0, 5:10, 5:10] == 2.0).all()       # centres 5.5 .. 9.5 lie in [5.5, 10.5)
    out, stats = pref.register32(frame, 1.0, Kd, pref.IDENTITY, Kc, S, edge_radius=0, max_splat=4)
    assert not out.any() and stats.tolist() == [[1, 0, 1, 0]]           # dropped, not clamped to 4 x 4
    # clipped to the image first: the same pixel hanging over the corner covers 3 x 3 pixels and passes a cap of 3
    Kc = pref.intrinsics(5.0 / S, 0.5 / S, 0.5 / S)
    out, stats = pref.register32(frame, 1.0, Kd, pref.IDENTITY, Kc, S, edge_radius=0, max_splat=3)
    assert (out[0, :3, :3] == 2.0).all() and stats.tolist() == [[1, 0, 0, 9]]


def test_the_nearer_surface_wins_and_the_result_ignores_the_order():
    S = 16
    Kd, Kc = _same_camera(S)
    src = np.full((1, S, S), 2.0, F32)
    src[0, :, 4:8] = 1.0                                   # a near strip in front of a far plane
    T = np.array([[1, 0, 0, 0.25], [0, 1, 0, 0], [0, 0, 1, 0]], F64)         # parallax: near moves 16 * .25 / 1 = 4, far 2 columns
    out, stats = pref.register32(src, 1.0, Kd, T, Kc, S, edge_radius=0)
    # far columns 0..3 land on 2..5, the strip on 8..11 - where the far columns 8, 9 land too and lose -, far 10..13 on 12..15;
    # columns 6, 7 see what the depth camera could not: a hole, not an interpolation
    row = [0, 0, 2, 2, 2, 2, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    assert np.array_equal(out[0], np.tile(np.array(row, F32), (S, 1)))
    assert stats.tolist() == [[S * S, 0, 0, 12 * S]]
    flipped, _ = pref.register32(src[:, ::-1, ::-1].copy(), 1.0, pref.intrinsics(-S, S / 2.0, S / 2.0, -S), T, Kc, S, edge_radius=0)
    assert np.array_equal(out, flipped)                                 # mirrored intrinsics swap the interval ends


# =============================================================================================== tiling
@pytest.mark.parametrize("Hd, Wd, S, ratio", pref.TILING_CASES)
def test_a_constant_frame_leaves_no_hole_inside_the_field_of_view(Hd, Wd, S, ratio):
    """T = identity and constant depth: neighbouring source pixels share their corners bit for bit, so their footprints tile the
    target - every target pixel whose centre is inside the source frame is valid; the cap on holes is zero."""
    Kd, Kc = pref.scaled_cameras(Hd, Wd, S, ratio)
    for z in (0.7, 1.0, 3.3):
        out, stats = pref.register32(np.full((1, Hd, Wd), z, F32), 1.0, Kd, pref.IDENTITY, Kc, S, edge_radius=1)
        inside = pref.inside_source(Hd, Wd, S, Kd, Kc)
        assert inside.any() and not inside.all()
        assert (out[0][inside] == F32(z)).all(), f"{int((out[0][inside] == 0).sum())} holes"
        assert stats[0, 1] == 0 and stats[0, 2] == 0
        outside = ~pref.inside_source(Hd, Wd, S, Kd, Kc, margin=-1e-3)
        assert not out[0][outside].any()


# =============================================================================================== refusals on the host
def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    """hm_depth_register with addresses that are never dereferenced: every check returns HM_ERR_BAD_ARG on the host (a call that got
    past them would fault on this machine, which has no device)"""
    from homan_amd import lib
    h = lib.lib()
    base = 0x7f0000000000
    good = dict(frames=base, frames_f32=0, B=2, Hd=6, Wd=8, depth_scale=0.001, Kd=base + 0x1000, Kd_stride=0, T=base + 0x2000,
                T_stride=1, Kc=base + 0x3000, Kc_stride=0, S=16, znear=0.1, zfar=100.0, edge_radius=1, edge_jump_abs=0.02,
                edge_jump_rel=0.0, max_splat=8, out=base + 0x4000, stats=base + 0x5000, stream=None)
    nan, inf = float("nan"), float("inf")
    bad = [dict(frames=None), dict(Kd=None), dict(T=None), dict(Kc=None), dict(out=None), dict(stats=None),
           dict(B=0), dict(B=65536), dict(Hd=0), dict(Wd=-1), dict(S=0), dict(S=1025),
           dict(edge_radius=-1), dict(edge_radius=4), dict(max_splat=0), dict(max_splat=-3),
           dict(depth_scale=0.0), dict(depth_scale=-0.001), dict(depth_scale=nan), dict(depth_scale=inf),
           dict(znear=0.0), dict(znear=nan), dict(znear=2.0, zfar=1.0), dict(zfar=100.5), dict(zfar=nan),
           dict(edge_jump_abs=-0.01), dict(edge_jump_abs=nan), dict(edge_jump_rel=-1.0), dict(edge_jump_rel=inf),
           dict(Kd_stride=2), dict(T_stride=-1), dict(Kc_stride=9),
           dict(frames=base + 1), dict(frames=base + 2, frames_f32=1), dict(out=base + 0x4004), dict(out=base + 0x4008),
           dict(out=base + 0x4002, S=15), dict(stats=base + 0x5002), dict(Kd=base + 0x1002), dict(T=base + 0x2001),
           dict(Kc=base + 0x3002)]
    for change in bad:
        assert h.hm_depth_register(*dict(good, **change).values()) == -1, change


def _args(B=2, Hd=6, Wd=8, S=16):
    return (np.full((B, Hd, Wd), 1000, np.uint16), pref.intrinsics(10.0, Wd / 2.0, Hd / 2.0), pref.intrinsics(1.0, 0.5, 0.5), S)


@pytest.fixture
def no_device(monkeypatch):
    """every refusal below comes before a device is asked for: a call that reached one would raise this instead"""
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", boom)


def test_prepare_depth_maps_refuses_on_the_host(no_device):
    from homan_amd import depthprep
    frames, Kd, Kc, S = _args()
    bad = [
        (dict(frames=frames[0]), "expected non-empty"),
        (dict(frames=frames.astype(np.int32)), "dtype"),
        (dict(frames=frames[:, :0]), "expected non-empty"),
        (dict(depth_scale=0.0), "depth_scale"),
        (dict(depth_scale=float("nan")), "depth_scale"),
        (dict(depth_camintr=np.eye(4)), "depth_camintr of shape"),
        (dict(depth_camintr=np.stack([Kd] * 3)), "depth_camintr of shape"),
        (dict(depth_camintr=Kd * np.array([[1, 1, 1], [1, 1, 1], [1, 1, np.nan]])), "non-finite"),
        (dict(depth_camintr=Kd + np.array([[0, 0.1, 0], [0, 0, 0], [0, 0, 0]])), "skew"),
        (dict(depth_camintr=Kd * np.array([[0, 1, 1], [1, 1, 1], [1, 1, 1]])), "zero focal"),
        (dict(camintr=np.full((3, 3), np.inf)), "non-finite"),
        (dict(depth_to_color=np.eye(3)), "depth_to_color of shape"),
        (dict(depth_to_color=np.full((3, 4), np.nan)), "non-finite"),
        (dict(depth_to_color=np.ones((4, 4))), "last row"),
        (dict(image_size=0), "image_size"),
        (dict(image_size=1025), "image_size"),
        (dict(pixel_center=0.25), "pixel_center"),
        (dict(znear=0.0), "znear"),
        (dict(znear=2.0, zfar=1.0), "znear"),
        (dict(zfar=101.0), "znear"),
        (dict(edge_radius=4), "edge_radius"),
        (dict(edge_radius=-1), "edge_radius"),
        (dict(edge_radius=1.5), "edge_radius"),
        (dict(edge_jump_abs=-0.01), "edge_jump_abs"),
        (dict(edge_jump_rel=float("inf")), "edge_jump_rel"),
        (dict(max_splat=0), "max_splat"),
    ]
    for change, needle in bad:
        kw = dict(frames=frames, depth_camintr=Kd, camintr=Kc, image_size=S)
        kw.update(change)
        with pytest.raises(ValueError, match=needle):
            depthprep.prepare_depth_maps(**kw)


def test_sensor_depth_refuses_on_the_host(no_device):
    from homan_amd import depthprep
    frames, Kd, _, S = _args()
    with pytest.raises(TypeError, match="unknown option"):
        depthprep.SensorDepth(frames, Kd, edge_radios=1)
    with pytest.raises(ValueError, match="edge_radius"):
        depthprep.SensorDepth(frames, Kd, edge_radius=7)
    with pytest.raises(ValueError, match="expected non-empty"):
        depthprep.SensorDepth(frames[0], Kd)
    with pytest.raises(ValueError, match="SensorDepth camintr"):
        depthprep.SensorDepth(frames, np.eye(2))
    with pytest.raises(ValueError, match="depth_scale"):
        depthprep.SensorDepth(frames, Kd, scale=-1.0)
    sd = depthprep.SensorDepth(frames, Kd, to_color=np.eye(4), scale=0.001, max_splat=4)
    assert sd.shape == frames.shape and sd.options == {"max_splat": 4}
    with pytest.raises(ValueError, match="holds 2 frames"):
        sd.check(3, S)
    with pytest.raises(ValueError, match="image_size"):
        sd.check(2, 2048)
    sd.check(2, S)


def test_a_clip_with_raw_frames_and_prepared_maps_is_refused(no_device):
    from homan_amd import depthprep
    frames, Kd, _, S = _args()
    assert depthprep.clip_sensor_depth({"depth_maps": np.zeros((2, S, S), F32)}) is None
    assert depthprep.clip_sensor_depth({}) is None
    with pytest.raises(ValueError, match="both depth_frames and depth_maps"):
        depthprep.clip_sensor_depth({"depth_frames": frames, "depth_camintr": Kd, "depth_maps": np.zeros((2, S, S), F32)})
    with pytest.raises(ValueError, match="depth_camintr"):
        depthprep.clip_sensor_depth({"depth_frames": frames})
    sd = depthprep.clip_sensor_depth({"depth_frames": frames, "depth_camintr": Kd, "depth_scale": 0.002,
                                      "depth_options": {"edge_radius": 2}})
    assert sd.scale == 0.002 and sd.options == {"edge_radius": 2}


def test_clip_fitter_refuses_both_keys_before_any_copy(no_device):
    """ClipFitter._inputs looks at the depth keys first: nothing of the clip is collated, let alone copied"""
    from homan_amd.shard import ClipFitter
    frames, Kd, _, S = _args()
    fitter = ClipFitter.__new__(ClipFitter)                    # (no device, no model: _inputs must refuse before it needs either)
    with pytest.raises(ValueError, match="both depth_frames and depth_maps"):
        fitter._inputs({"depth_frames": frames, "depth_camintr": Kd, "depth_maps": np.zeros((2, S, S), F32)})


def test_without_a_gpu_the_module_raises_like_maskutils(monkeypatch):
    from homan_amd import depthprep, lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    frames, Kd, Kc, S = _args()
    with pytest.raises(lib.HomanAmdError, match="no CPU fallback"):
        depthprep.prepare_depth_maps(frames, Kd, Kc, S)


def test_pixel_center_shifts_the_principal_point_on_the_host(monkeypatch):
    """pixel_center=0.0: intrinsics calibrated with integer pixel centres - the kernel's convention is reached by cx, cy + 0.5"""
    from homan_amd import depthprep, ops
    seen = {}

    def fake(frames, scale, Kd, T, Kc, size, **opt):
        seen.update(Kd=Kd.cpu().numpy(), scale=scale, opt=opt, T=T.cpu().numpy())
        return "maps", "stats"
    monkeypatch.setattr(ops, "register_depth", fake)
    monkeypatch.setattr(depthprep, "_device", lambda *a: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    frames, Kd, Kc, S = _args()
    assert depthprep.prepare_depth_maps(frames, Kd, Kc, S, pixel_center=0.0) == "maps"
    assert seen["Kd"][0, 2] == Kd[0, 2] + 0.5 and seen["Kd"][1, 2] == Kd[1, 2] + 0.5 and seen["Kd"][0, 0] == Kd[0, 0]
    assert seen["scale"] == 0.001 and np.array_equal(seen["T"], np.eye(3, 4, dtype=F32)) and "pixel_center" not in seen["opt"]
    assert depthprep.prepare_depth_maps(frames.astype(F32), Kd, Kc, S, return_stats=True) == ("maps", "stats")
    assert seen["Kd"][0, 2] == Kd[0, 2] and seen["scale"] == 1.0
    assert seen["opt"] == dict(znear=ops.NMR_NEAR, zfar=ops.NMR_FAR, edge_radius=1, edge_jump_abs=0.02, edge_jump_rel=0.0, max_splat=8)
