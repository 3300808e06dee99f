"""CPU side of the observed-depth term (csrc/depthobs.hip, ops.depth_obs_loss, HOMan's lw_depth_obs): the fp32 NumPy restatement
tests/depthobs_ref.py - which the GPU tests hold the kernels to bit for bit - against its float64 closed form, known answers by
hand, and every refusal that needs no device.

Bound of the fp32 restatement against float64 (u = 2^-24, the unit roundoff of fp32; validity is decided on the same fp32
inputs on both sides, so both sum over the same pixels):
  r32 = fl(d - D): |r32 - r| <= u |r|.
  quadratic branch, rho32 = fl(fl(0.5 r32) r32): the halving is exact, the product rounds once, r32 enters twice:
      |rho32 - rho| <= (2u + u) rho + O(u^2) = 3u rho.
  linear branch, rho32 = fl(delta fl(|r32| - fl(0.5 delta))): |r32| is off by u |r|, the difference and the product round once each
      and fl(0.5 delta) is exact: |rho32 - rho| <= delta u |r| + 2u rho <= 4u rho, because rho = delta (|r| - delta / 2) >= delta |r| / 2
      wherever |r| >= delta.  A pixel within u |r| of the threshold may take the other branch: both forms and their first derivatives
      agree at |r| = delta, so the forms differ by (|r| - delta)^2 / 2 <= (u delta)^2 / 2 there, far below u rho.
  grid: each addend moves by at most 2^-33 (half a quantum), so a record's mean by at most 2^-33; the mean's own rounding to the
      grid adds 2^-33; the mean over the N records keeps both.
  the final rounding of the loss to fp32: u loss.
  |loss32 - loss64| <= 4u loss64 + u loss64 + 2^-32 = 5u loss64 + 2^-32.
The same steps for the mean |r| (one rounding of r32, grid, final rounding): |mae32 - mae64| <= 2u mae64 + 2^-33.
Gradient images: c32 = clamp(r32) is off by at most u |c|, w32 = fl(fl(up / N) / n) by 2u, the product rounds once:
  |g32 - g64| <= 4u |g64|  (+ the smallest normal for underflow)."""
import numpy as np
import pytest
import torch

from tests import depthobs_ref as dref
from tests import util

F32, F64 = np.float32, np.float64
U = dref.U32


def _one_pixel(d, D, a=1.0, m=1, S=2, B=1):
    """a (B,S,S) case whose only candidate pixel is (0, 0, 0)"""
    dep, sil, msk, Dm = (np.zeros((B, S, S), F32), np.zeros((B, S, S), F32), np.zeros((B, S, S), np.uint8),
                         np.full((B, S, S), 0.5, F32))
    dep[0, 0, 0], sil[0, 0, 0], msk[0, 0, 0], Dm[0, 0, 0] = d, a, m, D
    return [dep], [sil], [msk], Dm


DELTA = 0.03125          # 2^-5: the hand-made values below are exact in fp32


@pytest.mark.parametrize("r, rho, g", [
    (1 / 64, 1 / 8192, 1 / 64),                    # |r| < delta: r^2 / 2, gradient r
    (-1 / 64, 1 / 8192, -1 / 64),
    (1 / 16, 3 / 2048, 1 / 32),                    # |r| > delta: delta (|r| - delta / 2), gradient delta
    (-1 / 16, 3 / 2048, -1 / 32),
    (1 / 32, 1 / 2048, 1 / 32),                    # r = +-delta exactly: both forms give delta^2 / 2
    (-1 / 32, 1 / 2048, -1 / 32),
])
def test_one_valid_pixel_by_hand(r, rho, g):
    case = _one_pixel(1.0 + r, 1.0)
    f = dref.forward32(*case, DELTA)
    assert float(f["loss"]) == rho and float(f["N"]) == 1.0 and float(f["mae"]) == abs(r) and float(f["share"]) == 1.0
    assert f["records"][0, 0].tolist() == [1.0, rho]
    grads, _ = dref.backward32(f, upstream=1.0)
    assert float(grads[0][0, 0, 0]) == g and np.count_nonzero(grads[0]) == 1
    r64 = dref.reference64(*case, DELTA)
    assert r64["loss"] == rho and r64["grads"][0][0, 0, 0] == g
    grads2, _ = dref.backward32(f, upstream=0.5)
    assert float(grads2[0][0, 0, 0]) == 0.5 * g


@pytest.mark.parametrize("case", [
    _one_pixel(1.0, np.nan), _one_pixel(1.0, np.inf), _one_pixel(1.0, -1.0), _one_pixel(1.0, 0.0), _one_pixel(1.0, 0.05),
    _one_pixel(1.0, 150.0), _one_pixel(1.0, 1.01, a=0.75), _one_pixel(1.0, 1.01, m=0),
], ids=["nan", "inf", "negative", "zero", "below-near", "above-far", "sil<1", "mask0"])
def test_no_valid_pixel_gives_zero_everything(case):
    f = dref.forward32(*case, DELTA)
    assert float(f["loss"]) == 0.0 and float(f["N"]) == 0.0 and float(f["mae"]) == 0.0 and not f["records"].any()
    grads, _ = dref.backward32(f)
    assert not grads[0].any() and np.isfinite(grads[0]).all()
    r64 = dref.reference64(*case, DELTA)
    assert r64["loss"] == 0.0 and not r64["grads"][0].any()


def test_two_frames_two_layers_by_hand():
    """N counts the (layer, frame) records that hold a valid pixel; each is a mean over ITS valid pixels"""
    dep = np.zeros((2, 2, 2), F32); sil = np.ones((2, 2, 2), F32); msk = np.ones((2, 2, 2), np.uint8)
    D = np.ones((2, 2, 2), F32)
    dep[0] = 1.0 + 1 / 64                     # frame 0: four pixels of r = 1/64 -> mean 2^-13
    dep[1] = 1.0 + 1 / 16                     # frame 1: one valid pixel (three masked out) of r = 1/16 -> 3/2048
    msk[1].reshape(-1)[1:] = 0
    lay1 = (np.ones((2, 2, 2), F32), np.ones((2, 2, 2), F32), np.zeros((2, 2, 2), np.uint8))     # a layer the sensor never sees
    f = dref.forward32([dep, lay1[0]], [sil, lay1[1]], [msk, lay1[2]], D, DELTA)
    assert float(f["N"]) == 2.0 and float(f["loss"]) == (1 / 8192 + 3 / 2048) / 2
    assert f["n"].tolist() == [[4, 1], [0, 0]]
    assert float(f["mae"]) == F32((4 / 64 + 1 / 16) / 5) and float(f["share"]) == 1.0
    grads, _ = dref.backward32(f)
    assert float(grads[0][0, 0, 0]) == (1 / 64) / (4 * 2) and float(grads[0][1, 0, 0]) == (1 / 32) / (1 * 2)
    assert not grads[1].any()


@pytest.mark.parametrize("B, S, L, delta, seed", [(1, 16, 2, 0.03125, 0), (3, 48, 3, 0.03, 1), (2, 64, 3, 0.03125, 2),
                                                  (2, 64, 1, 1.0, 3), (4, 33, 2, 0.005, 4)])
def test_fp32_restatement_against_float64(B, S, L, delta, seed):
    case = dref.random_case(B, S, L, delta, seed, rows=(S // 4, S // 2))
    f, r = dref.forward32(*case, delta), dref.reference64(*case, delta)
    assert float(f["N"]) == r["N"] > 0
    print(f"loss {float(f['loss']):.9e} / {r['loss']:.9e}  mae {float(f['mae']):.9e} / {r['mae']:.9e}")
    assert abs(float(f["loss"]) - r["loss"]) <= 5 * U * r["loss"] + 2.0 ** -32
    assert abs(float(f["mae"]) - r["mae"]) <= 2 * U * r["mae"] + 2.0 ** -33
    assert abs(float(f["share"]) - r["share"]) <= U * r["share"]
    grads, flags = dref.backward32(f, upstream=0.7)
    r = dref.reference64(*case, delta, upstream=float(F32(0.7)))
    for g32, g64 in zip(grads, r["grads"]):
        assert np.all(np.abs(g32.astype(F64) - g64) <= 4 * U * np.abs(g64) + 1.2e-38)
        assert np.array_equal(g32 != 0, g64 != 0)
    if S % 64 == 0:
        assert all(fl.shape == (B, S, S // 64) and fl.any() and not fl.all() for fl in flags)


def test_residuals_at_plus_and_minus_delta_are_in_the_random_case():
    delta = 0.03125
    depths, sils, masks, D = dref.random_case(2, 16, 2, delta, 0)
    valid, _ = dref.valid_masks(depths, sils, masks, D)
    for l in range(2):
        r = (depths[l] - D)[valid[l]]
        assert (r == F32(delta)).any() and (r == -F32(delta)).any()
    assert np.isnan(D).any() and np.isinf(D).any() and (D < 0).any() and (D == 0).any() and (D > 100).any()
    assert not valid[1][1].any() and valid[0][1].any()                     # one (layer, frame) without a valid pixel
    empty = dref.random_case(2, 16, 2, delta, 0, empty_clip=True)
    f = dref.forward32(*empty, delta)
    assert float(f["loss"]) == 0.0 and float(f["N"]) == 0.0
    assert all(not g.any() for g in dref.backward32(f)[0])


def test_sums_do_not_depend_on_the_order_of_the_frames():
    delta = 0.03
    depths, sils, masks, D = dref.random_case(3, 48, 3, delta, 5)
    a = dref.forward32(depths, sils, masks, D, delta)
    perm = [2, 0, 1]
    b = dref.forward32([d[perm] for d in depths], [s[perm] for s in sils], [m[perm] for m in masks], D[perm], delta)
    for k in ("loss", "mae", "share", "N"):
        assert a[k].tobytes() == b[k].tobytes()
    assert a["records"][:, perm].tobytes() == b["records"].tobytes()
    ga, gb = dref.backward32(a)[0], dref.backward32(b)[0]
    assert all(x[perm].tobytes() == y.tobytes() for x, y in zip(ga, gb))


def test_the_grid_holds_a_frame_of_1024_squared():
    """every addend is at most 100 (|r| <= zfar = 100; rho <= delta |r| <= 100 with delta <= 1): 2^20 of them at 2^32 quanta each"""
    assert 1024 * 1024 * 100 * 2 ** 32 < 2 ** 63


# =============================================================================================== refusals, no device
def _golden_kwargs():
    rec, inputs, camintr, weights, meta = util.load_golden(util.golden_names()[0])
    return util.model_kwargs(inputs, camintr, meta), meta


def test_clip_tensors_takes_and_checks_depth_maps():
    from homan_amd.homan import clip_tensors
    kw, meta = _golden_kwargs()
    B, size = kw["translations_object"].shape[0], kw["masks_object"].shape[-1]
    assert "depth_maps" not in clip_tensors(**kw)
    dm = np.full((B, size, size), 0.6, np.float64)
    out = clip_tensors(**kw, depth_maps=dm)
    assert out["depth_maps"].dtype == torch.float32 and tuple(out["depth_maps"].shape) == (B, size, size)
    assert list(out)[-1] == "depth_maps"
    for bad in (dm[:-1], dm[:, :-1], dm[0]):
        with pytest.raises(ValueError, match="depth_maps"):
            clip_tensors(**kw, depth_maps=bad)


def test_model_options_are_checked_on_the_host():
    import homan_amd
    kw, meta = _golden_kwargs()
    B, size = kw["translations_object"].shape[0], int(meta["image_size"])
    dm = torch.full((B, size, size), 0.6)
    for bad in (dict(depth_obs_layers="hands"), dict(depth_obs_delta=0.0), dict(depth_obs_delta=1.5), dict(depth_obs_delta=-0.03),
                dict(depth_obs_delta=float("nan")), dict(depth_maps=dm[1:]), dict(depth_maps=dm[:, :, :-1])):
        with pytest.raises(ValueError, match="depth_"):
            homan_amd.HOMan(**kw, **bad)
    big = dict(kw, image_size=2048)
    with pytest.raises(NotImplementedError, match="1024"):
        homan_amd.HOMan(**big, depth_maps=torch.zeros(B, 2048, 2048))


def test_build_model_passes_the_options_through():
    """on host inputs: the refusal comes from HOMan's own checks, reached through build_model's new keywords"""
    from homan_amd import synth
    from homan_amd.loopcommon import build_model
    from homan_amd.mano_assets import synthetic_mano
    mano = synthetic_mano(0)
    sil_fn, hand_fn = util.oracle_clip_fns(mano)
    clip = synth.make_clip(seed=0, frames=2, rend_size=32, image_size=32, obj="cube", silhouette_fn=sil_fn, hand_verts_fn=hand_fn,
                           mano=mano)
    common = dict(objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"], image_size=32,
                  mano_model=mano, rend_size=32)
    with pytest.raises(ValueError, match="depth_maps"):
        build_model(clip["person_parameters"], clip["object_parameters"], depth_maps=torch.zeros(2, 16, 16), **common)
    with pytest.raises(ValueError, match="depth_obs_layers"):
        build_model(clip["person_parameters"], clip["object_parameters"], depth_maps=torch.zeros(2, 32, 32),
                    depth_obs_layers="none", **common)
    with pytest.raises(ValueError, match="depth_obs_delta"):
        build_model(clip["person_parameters"], clip["object_parameters"], depth_obs_delta=2.0, **common)


def test_wrapper_checks_its_arguments_before_any_device_work():
    from homan_amd import ops
    img = torch.zeros(1, 16, 16)
    m = torch.zeros(1, 16, 16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="layers"):
        ops.depth_obs_loss([], [], [], img, 0.03)
    with pytest.raises(ValueError, match="layers"):
        ops.depth_obs_loss([img] * 4, [img] * 4, [m] * 4, img, 0.03)
    with pytest.raises(ValueError, match="layers"):
        ops.depth_obs_loss([img, img], [img], [m, m], img, 0.03)
    for delta in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="delta"):
            ops.depth_obs_loss([img], [img], [m], img, delta)
    with pytest.raises(ValueError, match="context"):
        ops.depth_obs_loss([img], [img], [m], img, 0.03, sctxs=[None, None])


def test_fused_steppers_refuse_the_term():
    """before anything is built, so without a device: the message names the mode that covers the term"""
    from homan_amd import jointopt
    from homan_amd.fused import FusedStepper
    lw = {"lw_depth_obs": 1.0}
    with pytest.raises(NotImplementedError, match="mode='graph'"):
        FusedStepper(None, lw, 1e-2, 4)
    with pytest.raises(NotImplementedError, match="mode='graph'"):
        FusedStepper([None, None], lw, 1e-2, 4)               # a clip batch refuses it the same way
    with pytest.raises(NotImplementedError, match="mode='graph'"):
        jointopt.ShardStepper([], lw, 1e-2, 4)


def test_weighted_total_maps_the_new_key():
    from homan_amd.loopcommon import _weighted_total
    total = _weighted_total({"loss_pca": torch.tensor([3.0]), "loss_depth_obs": torch.tensor(0.5)},
                            {"lw_pca": 2.0, "lw_depth_obs": 4.0})
    assert float(total) == 8.0 and tuple(total.shape) == (1,)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """fake addresses, never dereferenced: every refusal is decided on the host (HM_ERR_BAD_ARG = -1)"""
    from homan_amd import lib as hlib
    L = hlib.lib()
    A = 0x7f0000000000
    img = lambda k: A + 0x100000 * k
    ok_fwd = dict(d=[img(1), img(2), None], a=[img(3), img(4), None], m=[img(5), img(6), None], D=img(7), L=2, B=2, S=16,
                  delta=0.03, c=[img(8), img(9), None], acc=img(10), rec=img(11), out=img(12))

    def fwd(**kw):
        a = dict(ok_fwd, **kw)
        return L.hm_depth_obs_fwd(*a["d"], *a["a"], *a["m"], a["D"], a["L"], a["B"], a["S"], a["delta"], 0.1, 100.0, *a["c"],
                                  a["acc"], a["rec"], a["out"], None)
    for bad in (dict(L=0), dict(L=4), dict(B=0), dict(S=0), dict(S=1040), dict(delta=0.0), dict(delta=1.5), dict(delta=float("nan")),
                dict(D=None), dict(acc=None), dict(rec=None), dict(out=None), dict(d=[img(1), None, None]),
                dict(m=[img(5), None, None]), dict(c=[None, img(9), None]),
                dict(d=[img(1) + 4, img(2), None]), dict(a=[img(3), img(4) + 8, None]), dict(m=[img(5) + 2, img(6), None]),
                dict(D=img(7) + 4), dict(c=[img(8) + 4, img(9), None]), dict(acc=img(10) + 4)):
        assert fwd(**bad) == -1, bad
    assert L.hm_depth_obs_acc_bytes(2, 3) == (2 * 3 * 4 + 2) * 8 and L.hm_depth_obs_acc_bytes(4, 3) == 0

    def bwd(c=(img(1), img(2), None), g=(img(3), img(4), None), f=(None, None, None), Ln=2, B=2, S=64, rec=img(5), out=img(6),
            up=img(7)):
        return L.hm_depth_obs_bwd(*c, Ln, B, S, rec, out, up, *g, *f, None)
    for bad in (dict(Ln=0), dict(B=0), dict(S=2048), dict(rec=None), dict(out=None), dict(up=None), dict(c=(img(1), None, None)),
                dict(g=(img(3), None, None)), dict(g=(img(3) + 4, img(4), None)), dict(c=(img(1) + 8, img(2), None)),
                dict(f=(img(8), None, None)), dict(f=(img(8), img(9), None), S=48)):
        assert bwd(**bad) == -1, bad
