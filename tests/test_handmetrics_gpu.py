"""The kernels of csrc/evalalign.hip (hm_procrustes_align, hm_threshold_counts, hm_fscore), homan_amd/handmetrics.py and the
protocol arrays of homan_amd/ho3deval.py against the float64 NumPy restatement of tests/handmetrics_ref.py.

Bars.  err: 2^-27 * max|coordinate| of the frame, about 1/16 of a float32 ulp of the inputs - what the data can resolve; the
restatement's own scatter under a reversal of the point order is <= 6e-16 m on such inputs, and a double-precision kernel sits
orders below the bar (the tests print what they measure).  aligned: one fp32 ulp of the restatement's value.  Counts are
integers and F-scores ratios of the same integers (1e-15).  AUCs: 1e-12.
Measured on the MI355X: max |err - restatement| 1.0e-14 m over all shapes and modes (bar >= 4.2e-9 m)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import handmetrics_ref as ref

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 21, 63, 64, 65, 778)        # one wave per frame up to 64 points, four above
SHAPES = [(3, n) for n in SIZES] + [(1, 21), (70, 21), (70, 778)]
ERR_BAR_REL = 2.0 ** -27


def _rotation(rng, proper):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if (np.linalg.det(q) < 0) == proper:
        q[:, 0] = -q[:, 0]
    return q


def _anchors(n):
    return (0, 4) if n > 4 else (0, n - 1)


@functools.lru_cache(maxsize=None)
def hand_sets(B, N, noise=0.01, seed=0):
    """gt (B,N,3) fp32: 0.08 m spread at 0.6 m; pred: a random similarity transform of it, frames alternating in handedness,
    plus `noise` metres -> (pred fp32, gt fp32, [(s, R)] of the transforms)"""
    rng = np.random.default_rng(1000 * seed + 10 * N + B)
    gt = (rng.normal(size=(B, N, 3)) * 0.08 + np.array([0.05, -0.1, 0.6])).astype(np.float32)
    pred, xf = [], []
    for f in range(B):
        R, s, t = _rotation(rng, proper=f % 2 == 0), rng.uniform(0.7, 1.4), rng.normal(size=3) * 0.05
        pred.append(s * gt[f].astype(np.float64) @ R.T + t + rng.normal(size=(N, 3)) * noise)
        xf.append((s, R))
    return np.stack(pred).astype(np.float32), gt, xf


@functools.lru_cache(maxsize=None)
def restated(B, N, mode, noise=0.01):
    pred, gt, _ = hand_sets(B, N, noise)
    rows = [ref.align(p, g, mode, _anchors(N)) for p, g in zip(pred, gt)]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), [r[2] for r in rows])


def device_align(pred, gt, mode, anchors):
    from homan_amd import ops
    aligned, err, xform = ops.procrustes_align(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), mode, anchors)
    assert aligned.dtype == torch.float32 and err.dtype == torch.float64 and xform.dtype == torch.float64
    return aligned.cpu().numpy(), err.cpu().numpy(), xform.cpu().numpy()


def err_bar(pred, gt):
    """(B,1): 2^-27 * max|coordinate| of each frame"""
    return ERR_BAR_REL * np.maximum(np.abs(pred).max((1, 2)), np.abs(gt).max((1, 2))).astype(np.float64)[:, None]


def apply_xform(xform, pred):
    s, R, t = xform[:, 0], xform[:, 1:10].reshape(-1, 3, 3), xform[:, 10:13]
    return s[:, None, None] * np.einsum("bnj,bij->bni", pred.astype(np.float64), R) + t[:, None, :]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# =============================================================================================== alignment
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,N", SHAPES)
def test_alignment_matches_the_restatement(B, N, mode):
    pred, gt, _ = hand_sets(B, N)
    want_al, want_err, want_xf = restated(B, N, mode)
    aligned, err, xform = device_align(pred, gt, mode, _anchors(N))
    bar = err_bar(pred, gt)
    worst = np.abs(err - want_err).max()
    print(f"align mode {mode} B {B} N {N}: max |err - restatement| {worst:.3e} m (bar {bar.min():.3e}), "
          f"max |aligned - restatement| {np.abs(aligned - want_al).max():.3e} m")
    assert np.isfinite(aligned).all() and np.isfinite(err).all() and np.isfinite(xform).all()
    assert (np.abs(err - want_err) <= bar).all()
    ulp = np.spacing(np.abs(want_al).astype(np.float32)).astype(np.float64)
    assert (np.abs(aligned.astype(np.float64) - want_al) <= ulp).all()
    assert (np.abs(aligned.astype(np.float64) - apply_xform(xform, pred)) <= ulp).all()
    R = xform[:, 1:10].reshape(-1, 3, 3)
    np.testing.assert_allclose(np.abs(np.linalg.det(R)), 1.0, rtol=0, atol=1e-12)
    if mode == 2:
        assert (R == np.eye(3)).all()
        np.testing.assert_allclose(xform[:, 0], [x[0] for x in want_xf], rtol=1e-14)
    if N == 1:
        assert np.array_equal(aligned, gt) and (err == 0).all()
    if N >= 4 and mode != 2:         # (below four points the orthogonal factor is not unique)
        np.testing.assert_allclose(xform[:, 0], [x[0] for x in want_xf], rtol=1e-12)
        np.testing.assert_allclose(R, np.stack([x[1] for x in want_xf]), rtol=0, atol=1e-11)
        np.testing.assert_allclose(xform[:, 10:], np.stack([x[2] for x in want_xf]), rtol=0, atol=1e-11)


@pytest.mark.parametrize("N", [4, 21, 778])
def test_alignment_recovers_a_noise_free_transform(N):
    """pred = s * gt @ R.T + t rounded to fp32, frames alternating in handedness.  Mode 0 returns the inverse transform, mirrored
    or not; mode 1 returns it on the proper frames and a proper rotation with a residual on the mirrored ones.  Bar on R and on
    the relative scale, 1e-5: the rounding of pred moves a coordinate by at most 2^-24 * 1.5 = 9e-8 m, an angle of 1e-6 at the
    0.08 m spread of the set (and 1e-6 relative in its size); ten times that.  (The 1e-8 the formula adds to the norms is 3e-8
    relative.)"""
    B = 6
    pred, gt, xf = hand_sets(B, N, noise=0.0)
    mirrored = np.array([f % 2 == 1 for f in range(B)])
    s_true, R_true = np.array([x[0] for x in xf]), np.stack([x[1] for x in xf])
    assert ((np.linalg.det(R_true) < 0) == mirrored).all()
    _, err0, x0 = device_align(pred, gt, 0, (0, 0))
    _, err1, x1 = device_align(pred, gt, 1, (0, 0))
    R0, R1 = x0[:, 1:10].reshape(-1, 3, 3), x1[:, 1:10].reshape(-1, 3, 3)
    print(f"recover N {N}: max |R0 - R^T| {np.abs(R0 - R_true.transpose(0, 2, 1)).max():.3e}, "
          f"max |s0 s - 1| {np.abs(x0[:, 0] * s_true - 1).max():.3e}, max err0 {err0.max():.3e} m, "
          f"mean err1 on the mirrored frames {err1[mirrored].mean():.3e} m")
    np.testing.assert_allclose(R0, R_true.transpose(0, 2, 1), rtol=0, atol=1e-5)
    np.testing.assert_allclose(x0[:, 0] * s_true, 1.0, rtol=0, atol=1e-5)
    assert err0.max() < 1e-6                                        # (9e-8 m of rounding, through a scale of at most 1 / 0.7)
    np.testing.assert_allclose(np.linalg.det(R0), np.where(mirrored, -1.0, 1.0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.linalg.det(R1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(R1[~mirrored], R_true.transpose(0, 2, 1)[~mirrored], rtol=0, atol=1e-5)
    assert err1[~mirrored].max() < 1e-6 and err1[mirrored].mean(1).min() > 1e-3
    # the restatement agrees on both
    for mode, xd in ((0, x0), (1, x1)):
        want = [ref.align(p, g, mode)[2] for p, g in zip(pred, gt)]
        np.testing.assert_allclose(xd[:, 1:10].reshape(-1, 3, 3), np.stack([w[1] for w in want]), rtol=0, atol=1e-11)


def _degenerate_sets():
    rng = np.random.default_rng(5)
    sets = {}
    for name, N in (("one point", 1), ("two points", 2)):
        sets[name] = ((rng.normal(size=(N, 3)) * 0.08 + 0.5).astype(np.float32), (rng.normal(size=(N, 3)) * 0.08 + 0.6).astype(np.float32))
    N = 21
    flat = (rng.normal(size=(N, 3)) * 0.08 + np.array([0.05, -0.1, 0.6])).astype(np.float32)
    flat[:, 2] = np.float32(0.625)                      # exactly coplanar: M has a zero row, rank 2 to the bit
    line = flat.copy()
    line[:, 1] = np.float32(-0.125)                     # exactly collinear: rank 1
    for name, pred in (("coplanar", flat), ("collinear", line)):
        R = _rotation(rng, proper=True)
        gt = (1.2 * pred.astype(np.float64) @ R.T + np.array([0.02, 0.01, -0.03]) + rng.normal(size=(N, 3)) * 0.01).astype(np.float32)
        sets[name] = (pred, gt)
        sets[name + ", exact match"] = (pred, (1.2 * pred.astype(np.float64) @ R.T).astype(np.float32))
    sets["all equal"] = (np.full((N, 3), 0.375, np.float32), flat)
    sets["both all equal"] = (np.full((N, 3), 0.375, np.float32), np.full((N, 3), -0.25, np.float32))
    return sets


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_degenerate_sets_give_finite_outputs_and_the_minimum(mode):
    """rank-deficient M: the minimiser is not unique, its residual is.  R is not compared."""
    for name, (pred, gt) in _degenerate_sets().items():
        N = pred.shape[0]
        anchors = (0, N - 1) if N < 5 else (0, 4)
        aligned, err, xform = device_align(pred[None], gt[None], mode, anchors)
        want_al, want_err, _ = ref.align(pred, gt, mode, anchors)
        assert np.isfinite(aligned).all() and np.isfinite(err).all() and np.isfinite(xform).all(), name
        bar = err_bar(pred[None], gt[None])[0, 0]
        got, want = np.sqrt((err[0] ** 2).sum()), np.sqrt((want_err ** 2).sum())
        print(f"degenerate mode {mode} {name}: residual {got:.9e} vs restatement {want:.9e}, difference {abs(got - want):.3e} (bar {bar:.3e})")
        assert abs(got - want) <= bar, name
        np.testing.assert_allclose(abs(np.linalg.det(xform[0, 1:10].reshape(3, 3))), 1.0, rtol=0, atol=1e-12, err_msg=name)
        ulp = np.spacing(np.abs(aligned[0])).astype(np.float64)
        assert (np.abs(aligned[0].astype(np.float64) - apply_xform(xform, pred[None])[0]) <= ulp).all(), name
        if N == 1:
            assert np.array_equal(aligned[0], gt), name


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N", [21, 778])
def test_alignment_is_deterministic_and_independent_of_the_batch(N, mode):
    pred, gt, _ = hand_sets(70, N)
    first, second = device_align(pred, gt, mode, (0, 4)), device_align(pred, gt, mode, (0, 4))
    for a, b in zip(first, second):
        assert np.array_equal(bits(a), bits(b))
    for f in (0, 33, 69):
        alone = device_align(pred[f:f + 1], gt[f:f + 1], mode, (0, 4))
        for a, b in zip(first, alone):
            assert np.array_equal(bits(a[f]), bits(b[0])), f


def test_frame_axis_beyond_one_launch():
    """65537 frames of three points: the frame axis goes out in launches of at most 65535 frames.  The frames repeat seven
    distinct ones, so every row must carry the bits of its frame computed in a call of seven."""
    B, N = 65537, 3
    pred7, gt7, _ = hand_sets(7, N)
    want_err = restated(7, N, 0)[1]
    reps = -(-B // 7)
    pred, gt = np.tile(pred7, (reps, 1, 1))[:B], np.tile(gt7, (reps, 1, 1))[:B]
    base = device_align(pred7, gt7, 0, (0, 2))
    assert (np.abs(base[1] - want_err) <= err_bar(pred7, gt7)).all()
    full = device_align(pred, gt, 0, (0, 2))
    for a, b in zip(full, base):
        assert np.array_equal(bits(a), bits(np.tile(b, (reps,) + (1,) * (b.ndim - 1))[:B]))


# =============================================================================================== threshold counts
def _distances(n, val_max, steps, dtype, seed):
    """values exactly on thresholds, their neighbours in `dtype`, above val_max, NaN, zero, and a uniform fill"""
    rng = np.random.default_rng(seed)
    t = np.linspace(0, val_max, steps).astype(dtype)
    on = np.concatenate([t, np.nextafter(t, dtype(np.inf)), np.nextafter(t[1:], dtype(-np.inf))])
    rng.shuffle(on)
    special = np.concatenate([np.array([np.nan, val_max * 1.5, np.inf, 0.0, -0.0, val_max], dtype), on])
    take = special[:max(n // 2, min(n, 1))]
    fill = rng.uniform(0, 1.2 * val_max, size=n - take.shape[0]).astype(dtype)
    vals = np.concatenate([take, fill])
    rng.shuffle(vals)
    return vals


@pytest.mark.parametrize("steps", [2, 100, 1024])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 21 * 70, 778 * 70])
def test_threshold_counts_are_exact(n, steps):
    from homan_amd import ops
    val_max = 0.05
    for dtype in (np.float32, np.float64):
        vals = _distances(n, val_max, steps, dtype, seed=n + steps)
        assert vals.shape == (n,) and vals.dtype == dtype
        want = ref.threshold_counts(vals, val_max, steps)
        got = ops.threshold_counts(torch.from_numpy(vals).cuda(), val_max, steps)
        assert got.dtype == torch.int64 and got.shape == (steps,)
        assert np.array_equal(got.cpu().numpy().astype(np.uint64), want), (dtype, np.flatnonzero(got.cpu().numpy() != want.astype(np.int64))[:8])
        if n >= 63:
            assert 0 < want[0] and want[-1] < n and np.isnan(vals).any()        # (the edge values are in the sample)
        again = ops.threshold_counts(torch.from_numpy(vals).cuda(), val_max, steps)
        assert torch.equal(got, again)


def test_threshold_counts_on_every_threshold_and_its_neighbours():
    """all of linspace itself: value k sits exactly on t_k, so counts[k] = k + 1; one ulp up shifts every count by one"""
    from homan_amd import ops
    for val_max, steps in ((0.05, 100), (0.1, 1024), (0.05, 2), (1.0, 7)):
        t = np.linspace(0, val_max, steps)
        assert ref.threshold_counts(t, val_max, steps).tolist() == list(range(1, steps + 1))
        for vals in (t, np.nextafter(t, np.inf), np.nextafter(t[1:], -np.inf)):
            want = ref.threshold_counts(vals, val_max, steps)
            got = ops.threshold_counts(torch.from_numpy(np.ascontiguousarray(vals)).cuda(), val_max, steps).cpu().numpy()
            assert np.array_equal(got.astype(np.uint64), want), (val_max, steps)
    from homan_amd import handmetrics
    assert handmetrics.auc(np.zeros(50), 0.05) == pytest.approx(1.0, abs=1e-15)
    assert handmetrics.auc(np.full(50, 0.0500001), 0.05) == 0.0


# =============================================================================================== F-scores
@functools.lru_cache(maxsize=None)
def _clouds(N, M):
    rng = np.random.default_rng(N + 7 * M)
    gt = (rng.normal(size=(3, M, 3)) * 0.04 + np.array([0.05, -0.1, 0.6])).astype(np.float32)
    if N == M:           # paired clouds a few millimetres apart, else two samples of one distribution
        pred = (gt + rng.normal(size=(3, N, 3)) * 0.005).astype(np.float32)
    else:
        pred = (rng.normal(size=(3, N, 3)) * 0.04 + np.array([0.05, -0.1, 0.6]) + 0.004).astype(np.float32)
    return pred, gt


def _assert_clear_of_thresholds(d2, ths):
    d = np.sqrt(np.asarray(d2, np.float32).astype(np.float64))
    for th in np.asarray(ths, np.float32).astype(np.float64):
        assert (np.abs(d - th) > 1e-9 * th).all()


@pytest.mark.parametrize("N,M", [(1, 1), (65, 64), (778, 778), (130, 4097)])
def test_fscore_matches_the_restatement(N, M):
    from homan_amd import ops
    ths = (0.005, 0.015)
    pred, gt = _clouds(N, M)
    _, (x_d2, _, y_d2, _) = ops.cloud_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), per_point=True)
    got = ops.fscore(x_d2, y_d2, ths).cpu().numpy()
    assert got.shape == (3, 2, 3) and got.dtype == np.float64
    for f in range(3):
        dx, dy = ref.nn_d2(pred[f], gt[f]), ref.nn_d2(gt[f], pred[f])
        _assert_clear_of_thresholds(dx, ths)
        _assert_clear_of_thresholds(dy, ths)
        want = ref.fscore_from_d2(dx, dy, ths)
        assert np.abs(got[f] - want).max() <= ref.FSCORE_BAR, (f, got[f], want)
    print(f"fscore N {N} M {M}: F@5 {got[:, 0, 2].tolist()}, F@15 {got[:, 1, 2].tolist()}")
    assert (got[:, 0] <= got[:, 1]).all() and (got >= 0).all() and (got <= 1).all()
    single = ops.fscore(x_d2[1:2].contiguous(), y_d2[1:2].contiguous(), ths[1:]).cpu().numpy()
    assert np.array_equal(bits(single[0, 0]), bits(got[1, 1]))


def test_fscore_just_under_and_just_over_a_threshold_and_none_under():
    """64 pairs x_i = y_i + (d_i, 0, 0), the pairs 0.125 m apart on another axis: d_i = th * (1 -+ 2^-20), a part in a million
    under or over the fp32 threshold (fp32 resolves 6e-8).  A second frame is 1 m away from everything: p + r = 0, F = 0."""
    from homan_amd import ops
    ths = np.array([0.005, 0.015], np.float32)
    rng = np.random.default_rng(9)
    y = np.zeros((2, 64, 3), np.float32)
    y[:, :, 1] = np.arange(64, dtype=np.float32) * np.float32(0.125)
    x = y.copy()
    under = rng.random(64) < 0.4
    which = rng.integers(0, 2, size=64)
    d = (ths[which].astype(np.float64) * np.where(under, 1 - 2.0 ** -20, 1 + 2.0 ** -20)).astype(np.float32)
    x[0, :, 0] = d
    x[1, :, 2] = np.float32(1.0)
    dx, dy = ref.nn_d2(x[0], y[0]), ref.nn_d2(y[0], x[0])
    assert np.array_equal(dx, d * d) and np.array_equal(dy, dx)
    _assert_clear_of_thresholds(dx, ths)
    rel = np.abs(np.sqrt(dx.astype(np.float64)) / ths[which].astype(np.float64) - 1)
    assert rel.max() < 2e-6                                           # just under, just over
    want = ref.fscore_from_d2(dx, dy, ths)
    assert want[0, 0] == np.count_nonzero(under & (which == 0)) / 64 and 0 < want[0, 0] < want[1, 0] < 1
    _, (x_d2, _, y_d2, _) = ops.cloud_metrics(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), per_point=True)
    got = ops.fscore(x_d2, y_d2, ths).cpu().numpy()
    assert np.abs(got[0] - want).max() <= ref.FSCORE_BAR
    assert np.array_equal(got[1], np.zeros((2, 3)))


# =============================================================================================== bad arguments
def test_bad_arguments_leave_the_outputs_untouched_and_the_buffers_usable():
    from homan_amd import lib
    h = lib.lib()
    ptr, stream = lib.ptr, lib.stream()
    pred_np, gt_np, _ = hand_sets(3, 21)
    pred, gt = torch.from_numpy(pred_np).cuda(), torch.from_numpy(gt_np).cuda()
    aligned = torch.full((3, 21, 3), 7.0, device="cuda")
    err = torch.full((3, 21), 7.0, dtype=torch.float64, device="cuda")
    xform = torch.full((3, 13), 7.0, dtype=torch.float64, device="cuda")

    def call_align(p=pred, g=gt, B=3, N=21, mode=0, a=0, b=4):
        return h.hm_procrustes_align(None if p is None else ptr(p), None if g is None else ptr(g), B, N, mode, a, b, ptr(aligned),
                                     ptr(err), ptr(xform), stream)
    for kw in (dict(B=0), dict(N=0), dict(p=None), dict(g=None), dict(mode=2, b=21), dict(mode=2, a=-1), dict(mode=3), dict(B=-1)):
        assert call_align(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (aligned == 7).all() and (err == 7).all() and (xform == 7).all()
    assert call_align() == 0
    torch.cuda.synchronize()
    assert (np.abs(err.cpu().numpy() - restated(3, 21, 0)[1]) <= err_bar(pred_np, gt_np)).all() and not (aligned == 7).any()

    dist = torch.rand(500, device="cuda") * 0.06
    counts = torch.full((100,), -7, dtype=torch.int64, device="cuda")
    vmax, zero = ctypes.c_double(0.05), ctypes.c_double(0.0)

    def call_counts(d=dist, n=500, vm=vmax, steps=100):
        return h.hm_threshold_counts(None if d is None else ptr(d), n, 0, None if vm is None else ctypes.addressof(vm), steps,
                                     ptr(counts), stream)
    for kw in (dict(steps=1), dict(steps=1025), dict(d=None), dict(n=-1), dict(vm=None), dict(vm=zero)):
        assert call_counts(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (counts == -7).all()
    assert call_counts() == 0
    assert np.array_equal(counts.cpu().numpy().astype(np.uint64), ref.threshold_counts(dist.cpu().numpy(), 0.05, 100))

    d2 = torch.rand(3, 21, device="cuda") * 1e-4
    out = torch.full((3, 2, 3), 7.0, dtype=torch.float64, device="cuda")
    ths = (ctypes.c_float * 9)(*([0.005, 0.015] + [0.02] * 7))

    def call_f(x=d2, y=d2, B=3, N=21, M=21, th=ths, T=2):
        return h.hm_fscore(None if x is None else ptr(x), None if y is None else ptr(y), B, N, M,
                           None if th is None else ctypes.addressof(th), T, ptr(out), stream)
    for kw in (dict(T=0), dict(T=9), dict(B=0), dict(N=0), dict(M=0), dict(x=None), dict(y=None), dict(th=None)):
        assert call_f(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out == 7).all()
    assert call_f() == 0
    want = np.stack([ref.fscore_from_d2(r, r, [0.005, 0.015]) for r in d2.cpu().numpy()])
    assert np.abs(out.cpu().numpy() - want).max() <= ref.FSCORE_BAR


# =============================================================================================== the protocol's table
def test_hand_protocol_metrics_against_the_restatement_loop():
    from homan_amd import handmetrics
    B = 5
    pred_j, gt_j, _ = hand_sets(B, 21, noise=0.008, seed=1)
    pred_v, gt_v, _ = hand_sets(B, 778, noise=0.004, seed=1)
    # (the transforms of hand_sets would put every raw error far past 50 mm: the raw sets are the aligned ones, moved a little)
    al_j, al_v = restated_for(pred_j, gt_j), restated_for(pred_v, gt_v)
    shift = np.array([0.004, -0.003, 0.002])
    pred_j, pred_v = (1.05 * al_j + shift).astype(np.float32), (1.05 * al_v + shift).astype(np.float32)
    got = handmetrics.get_hand_protocol_metrics(gt_j, pred_j, gt_v, pred_v)
    want = ref.hand_protocol_metrics(gt_j, pred_j, gt_v, pred_v)
    bars = {"xyz": err_bar(pred_j, gt_j), "mesh": err_bar(pred_v, gt_v)}
    for name in ("xyz", "mesh"):
        for tag in ("", "_al", "_sc_tr"):
            key = f"{name}{tag}"
            diff = np.abs(got[f"{key}_err"] - want[f"{key}_err"])
            print(f"protocol {key}: mean3d {got[f'{key}_mean3d']:.6e} (restatement {want[f'{key}_mean3d']:.6e}), auc "
                  f"{got[f'{key}_auc']:.12f} (restatement {want[f'{key}_auc']:.12f}), max per-point difference {diff.max():.3e} m")
            assert (diff <= bars[name]).all(), key
            assert abs(got[f"{key}_mean3d"] - want[f"{key}_mean3d"]) <= bars[name].max(), key
            assert abs(got[f"{key}_auc"] - want[f"{key}_auc"]) <= 1e-12, key
            assert 0.05 < got[f"{key}_auc"] < 0.999, key                 # (the curve is neither empty nor saturated)
    # F of the aligned meshes: the restatement's F on the device's aligned fp32 points (themselves held to one ulp of the
    # restatement's above), so that a vertex a rounding away from 5 mm cannot decide the comparison
    aligned = handmetrics.align(pred_v, gt_v)[0].cpu().numpy()
    for prefix, pts in (("f", pred_v), ("f_al", aligned)):
        tab = np.stack([ref.fscore(p, g, (0.005, 0.015)) for p, g in zip(pts, gt_v)])
        for t, mm in enumerate((5, 15)):
            key = f"{prefix}@{mm}"
            assert np.abs(got[f"{key}_frames"] - tab[:, t, 2]).max() <= ref.FSCORE_BAR, key
            assert abs(got[key] - tab[:, t, 2].mean()) <= ref.FSCORE_BAR, key
            assert abs(got[key] - want[key]) <= 0.01 and 0 < got[key] < 1, key      # (and the all-restatement table is next to it)
    assert set(got) == set(want)
    alone = handmetrics.get_hand_protocol_metrics(gt_j[2:3], pred_j[2:3], gt_v[2:3], pred_v[2:3])
    for key in ("xyz_err", "xyz_al_err", "xyz_sc_tr_err", "mesh_err", "mesh_al_err", "mesh_sc_tr_err", "f@5_frames", "f_al@15_frames"):
        assert np.array_equal(bits(alone[key][0]), bits(got[key][2])), key


def restated_for(pred, gt):
    return np.stack([ref.align(p, g, 0)[0] for p, g in zip(pred, gt)])


def test_object_auc_against_the_restatement_loop():
    from homan_amd import handmetrics
    rng = np.random.default_rng(11)
    gt = (rng.normal(size=(5, 26, 3)) * 0.05 + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    pred = (gt + rng.normal(size=(5, 26, 3)) * 0.01 + np.linspace(0, 0.09, 5)[:, None, None]).astype(np.float32)
    got = handmetrics.get_object_auc(gt, pred)
    d = gt - pred                                  # as hm_cloud_metrics states its paired distance: fp32 differences and square
    add = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float64)).mean(1)
    assert d.dtype == np.float32
    adds = np.stack([np.sqrt(ref.nn_d2(g, p).astype(np.float64)).mean() for g, p in zip(gt, pred)])
    np.testing.assert_allclose(got["add"], add, rtol=1e-14)
    np.testing.assert_allclose(got["adds"], adds, rtol=1e-14)
    for key, vals in (("add_auc", add), ("adds_auc", adds)):
        want = ref.auc(ref.threshold_counts(vals, 0.1, 100), 5, 0.1, 100)
        print(f"object {key}: {got[key]:.12f} (restatement {want:.12f})")
        assert abs(got[key] - want) <= 1e-12 and 0 < got[key] < 1
    other = handmetrics.get_object_auc(gt, pred[:, :20])
    assert np.isnan(other["add_auc"]) and np.isnan(other["add"]).all()
    adds = np.stack([np.sqrt(ref.nn_d2(g, p).astype(np.float64)).mean() for g, p in zip(gt, pred[:, :20])])
    assert abs(other["adds_auc"] - ref.auc(ref.threshold_counts(adds, 0.1, 100), 5, 0.1, 100)) <= 1e-12


# =============================================================================================== evaluate_sequence
def test_evaluate_sequence_protocol_arrays(mano_model):
    from homan_amd import handmetrics, ho3deval
    from tests.test_ho3deval import _ground_truth, golden, golden_seq_res
    g = golden()
    gt_obj, gt_roots = _ground_truth()
    closed = np.asarray(mano_model["closed_faces"])
    args = (golden_seq_res(), 10, gt_obj, gt_roots, g["obj_faces"], closed)
    plain = ho3deval.evaluate_sequence(*args, chunk=4)
    same = ho3deval.evaluate_sequence_protocol(*args, chunk=4)
    assert list(same) == list(plain)
    for key in plain:
        assert plain[key].dtype == same[key].dtype and np.array_equal(bits(plain[key]), bits(same[key])), key
    rng = np.random.default_rng(31)
    gt_j = (g["seq_flip_hand_joints3d"].astype(np.float64) * 1.03 + rng.normal(size=(10, 21, 3)) * 0.004).astype(np.float32)
    gt_v = (g["seq_flip_hand_verts3d"].astype(np.float64) * 1.03 + rng.normal(size=(10, 778, 3)) * 0.003).astype(np.float32)
    want = handmetrics.get_hand_protocol_metrics(gt_j, g["seq_flip_hand_joints3d"], gt_v, g["seq_flip_hand_verts3d"])
    pairs = {"joint_err": "xyz_err", "joint_err_al": "xyz_al_err", "joint_err_sc_tr": "xyz_sc_tr_err", "mesh_err": "mesh_err",
             "mesh_err_al": "mesh_al_err", "f@5": "f@5_frames", "f@15": "f@15_frames", "f_al@5": "f_al@5_frames",
             "f_al@15": "f_al@15_frames"}
    assert tuple(pairs) == ho3deval.PROTOCOL_KEYS
    for chunk in (1, 3, 512):
        res = ho3deval.evaluate_sequence_protocol(*args, chunk=chunk, gt_hand_joints=gt_j, gt_hand_verts=gt_v)
        assert list(res) == list(plain) + list(pairs)
        for key in plain:
            assert np.array_equal(bits(plain[key]), bits(res[key])), (key, chunk)
        for key, name in pairs.items():
            assert res[key].dtype == np.float64 and np.array_equal(bits(res[key]), bits(want[name])), (key, chunk)
    table = ho3deval.protocol_summary([res, res])
    assert set(table) == {"xyz_mean3d", "xyz_auc", "xyz_al_mean3d", "xyz_al_auc", "xyz_sc_tr_mean3d", "xyz_sc_tr_auc", "mesh_mean3d",
                          "mesh_auc", "mesh_al_mean3d", "mesh_al_auc", "f@5", "f@15", "f_al@5", "f_al@15"}
    for key, value in table.items():
        np.testing.assert_allclose(value, want[key], rtol=1e-13, err_msg=key)
        if key.endswith("_auc"):
            assert value == want[key], key                                # (the same integers, doubled)
    only_joints = ho3deval.evaluate_sequence_protocol(*args, gt_hand_joints=gt_j)
    assert list(only_joints) == list(plain) + ["joint_err", "joint_err_al", "joint_err_sc_tr"]
    assert set(ho3deval.protocol_summary(only_joints)) == {"xyz_mean3d", "xyz_auc", "xyz_al_mean3d", "xyz_al_auc", "xyz_sc_tr_mean3d",
                                                           "xyz_sc_tr_auc"}
    with pytest.raises(ValueError):
        ho3deval.evaluate_sequence_protocol(*args, gt_hand_joints=gt_j[:9])
    assert ho3deval.summarise(res)[0] == ho3deval.summarise(plain)[0]
