"""Evaluation metrics on the GPU (csrc/pointmetrics.hip through homan_amd/pointmetrics.py): per-point nearest neighbours
bit-equal to a float32 brute force, per-frame means, the reference's golden values, properties of the alignment, and
independence from the batch a frame is computed in."""
import math

import numpy as np
import pytest
import torch

from homan_amd import ops, pointmetrics
from homan_amd.mano_assets import synthetic_mano
from tests.test_pointmetrics import golden_cases, load_golden, restate_align_metrics

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 778, 4097, 20000)
PAIRS = ([(n, m) for n in SIZES[:5] for m in SIZES[:5]]
         + [(4097, 63), (63, 4097), (4097, 4097), (20000, 1), (1, 20000), (20000, 65), (778, 20000), (20000, 4097)])
ALIGN_RTOL, ALIGN_ATOL = 1e-5, 1e-7          # aligned metrics against the reference golden and the restatement


def affine_np(p, aff):
    """((p - c) / div) * mul in float32, in that order"""
    if aff is None:
        return p
    c, div, mul = aff[:3], aff[3], aff[4]
    return ((p - c) / div) * mul


def brute(q, t):
    """float32 brute force: d2 = (dx*dx + dy*dy) + dz*dz, ties to the lowest index (argmin)"""
    d2, idx = np.empty(len(q), np.float32), np.empty(len(q), np.int64)
    step = max(1, 4_000_000 // len(t))
    for s in range(0, len(q), step):
        qc = q[s:s + step]
        dx, dy, dz = [t[None, :, k] - qc[:, None, k] for k in range(3)]
        d = (dx * dx + dy * dy) + dz * dz
        i = d.argmin(1)
        idx[s:s + step], d2[s:s + step] = i, d[np.arange(len(qc)), i]
    return d2, idx


def run(x, y, aff_x=None, aff_y=None):
    dev = torch.device("cuda")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out4, (xd, xi, yd, yi) = ops.cloud_metrics(t(x), t(y), t(aff_x), t(aff_y), per_point=True)
    return out4.cpu().numpy(), xd.cpu().numpy(), xi.cpu().numpy(), yd.cpu().numpy(), yi.cpu().numpy()


def check_frame(x, y, out4, xd, xi, yd, yi, ax=None, ay=None):
    xa, ya = affine_np(x, ax), affine_np(y, ay)
    bxd, bxi = brute(xa, ya)
    byd, byi = brute(ya, xa)
    np.testing.assert_array_equal(xd.view(np.uint32), bxd.view(np.uint32))
    np.testing.assert_array_equal(xi, bxi)
    np.testing.assert_array_equal(yd.view(np.uint32), byd.view(np.uint32))
    np.testing.assert_array_equal(yi, byi)
    want = [bxd.astype(np.float64).sum() / len(x), byd.astype(np.float64).sum() / len(y),
            np.sqrt(bxd.astype(np.float64)).sum() / len(x)]
    np.testing.assert_allclose(out4[:3], want, rtol=1e-12, atol=0)
    if len(x) == len(y):
        d = xa - ya
        pd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        np.testing.assert_allclose(out4[3], np.sqrt(pd.astype(np.float64)).sum() / len(x), rtol=1e-12, atol=0)
    else:
        assert np.isnan(out4[3])


def cloud(rng, B, n, grid=False):
    if grid:        # coordinates on a coarse lattice: many equal distances
        return (rng.integers(-3, 4, size=(B, n, 3)) * 0.125).astype(np.float32)
    return (rng.normal(size=(B, n, 3)) * 0.1 + np.array([0.0, 0.0, 0.5])).astype(np.float32)


@pytest.mark.parametrize("n,m", PAIRS)
def test_nn_bit_equal_to_float32_brute_force(n, m):
    rng = np.random.default_rng(n * 100003 + m)
    x, y = cloud(rng, 1, n), cloud(rng, 1, m)
    out4, xd, xi, yd, yi = run(x, y)
    check_frame(x[0], y[0], out4[0], xd[0], xi[0], yd[0], yi[0])


@pytest.mark.parametrize("B,n,m", [(3, 778, 65), (70, 778, 778), (3, 4097, 64)])
def test_nn_batches(B, n, m):
    rng = np.random.default_rng(B)
    x, y = cloud(rng, B, n), cloud(rng, B, m)
    res = run(x, y)
    for b in range(B):
        check_frame(x[b], y[b], *[r[b] for r in res])


@pytest.mark.parametrize("n,m", [(778, 778), (130, 4097), (65, 64)])
def test_nn_ties_keep_lowest_index(n, m):
    rng = np.random.default_rng(11)
    x = cloud(rng, 2, n, grid=True)
    y = cloud(rng, 2, m, grid=True)
    y[:, m // 2:] = y[:, :m - m // 2]                # duplicated targets
    x[:, :5] = y[:, 7:12]                            # queries exactly on targets
    res = run(x, y)
    assert (res[1] == 0).any()
    for b in range(2):
        check_frame(x[b], y[b], *[r[b] for r in res])


@pytest.mark.parametrize("side", ["x", "y", "both"])
def test_nn_affine_on_load(side):
    rng = np.random.default_rng(5)
    B, n, m = 3, 778, 1000
    x, y = cloud(rng, B, n), cloud(rng, B, m)
    aff = lambda: np.concatenate([rng.normal(size=(B, 3)) * 0.1, rng.uniform(0.5, 2.0, (B, 2))], 1).astype(np.float32)  # noqa
    ax = aff() if side in ("x", "both") else None
    ay = aff() if side in ("y", "both") else None
    res = run(x, y, ax, ay)
    for b in range(B):
        check_frame(x[b], y[b], *[r[b] for r in res], ax=None if ax is None else ax[b], ay=None if ay is None else ay[b])


def _close(got, want, rel, abs_=0.0, what=""):
    np.testing.assert_allclose(got, want, rtol=rel, atol=abs_, err_msg=what)


def test_against_reference_golden():
    g = load_golden()
    for kind, tag, ins, want in golden_cases(g):
        t = [torch.from_numpy(a) for a in ins]
        if kind == "point":
            got = pointmetrics.get_point_metrics(*t)
            _close(got["chamfer_dists"], want["chamfer_dists"], ALIGN_RTOL, ALIGN_ATOL, tag)
            _close(got["add-s"], want["add-s"], 1e-6, 0, tag)
            _close(got["verts_dists"], want["verts_dists"], 1e-6, 0, tag)
            assert all(type(v) is float for vs in got.values() for v in vs)
        else:
            got = pointmetrics.get_align_metrics(*t)
            for k in ("hand_mean_aligned", "obj_chamfer_aligned"):
                _close(got[k], want[k], ALIGN_RTOL, ALIGN_ATOL, f"{tag} {k}")
            own = pointmetrics.get_align_metrics(*t, pred_centroid_from_gt=False)
            ref_own = restate_align_metrics(*t, pred_centroid_from_gt=False)
            for k in ("hand_mean_aligned", "obj_chamfer_aligned"):
                _close(own[k], ref_own[k], ALIGN_RTOL, ALIGN_ATOL, f"{tag} own centroid {k}")
                assert len(own[k]) == len(want[k])


def test_identical_clouds_give_zero():
    rng = np.random.default_rng(1)
    x = torch.from_numpy(cloud(rng, 4, 500)).cuda()
    r = pointmetrics.get_point_metrics(x, x.clone())
    assert r == {"chamfer_dists": [0.0] * 4, "add-s": [0.0] * 4, "verts_dists": [0.0] * 4}


def test_one_point_chamfer():
    a = torch.zeros(1, 1, 3)
    b = torch.tensor([[[0.5, 0.25, -1.0]]])
    r = pointmetrics.get_point_metrics(a, b)
    assert r["chamfer_dists"] == [2 * 1.3125] and r["add-s"] == [math.sqrt(1.3125)] == r["verts_dists"]


def _similar_scene(hands):
    """ground truth (hands of the synthetic template, an object) and a prediction a * gt + t (the same map for all)"""
    rng = np.random.default_rng(hands)
    tpl = synthetic_mano(0)["v_template"].astype(np.float32)
    frames = 3
    gt_h = np.stack([tpl + rng.normal(size=3).astype(np.float32) * 0.01 for _ in range(frames * hands)])
    gt_o = (rng.normal(size=(frames, 300, 3)) * 0.03).astype(np.float32)
    a, t = np.float32(2.0), np.array([0.125, -0.0625, 0.25], np.float32)
    return [torch.from_numpy(v) for v in (gt_h, a * gt_h + t, gt_o, a * gt_o + t)], gt_h


@pytest.mark.parametrize("hands", [1, 2])
def test_similarity_invariance_with_own_centroid(hands):
    ins, gt_h = _similar_scene(hands)
    scale = float(np.sqrt(((gt_h[0] - gt_h[0].mean(0)) ** 2).sum(1).mean()))
    own = pointmetrics.get_align_metrics(*ins, pred_centroid_from_gt=False)
    assert max(own["hand_mean_aligned"]) <= 1e-6 * scale
    assert max(own["obj_chamfer_aligned"]) ** 0.5 <= 1e-6 * scale
    ref = pointmetrics.get_align_metrics(*ins)          # the reference's centring: not invariant
    assert min(ref["hand_mean_aligned"]) > 1e-3 * scale
    assert min(ref["obj_chamfer_aligned"]) > 0


def test_deterministic_and_batch_independent():
    rng = np.random.default_rng(3)
    B = 70
    x, y = cloud(rng, B, 778), cloud(rng, B, 2000)
    full = run(x, y)
    again = run(x, y)
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()
    for b in (0, 31, 69):
        one = run(x[b:b + 1], y[b:b + 1])
        for a, o in zip(full, one):
            assert a[b].tobytes() == o[0].tobytes()
    gm = pointmetrics.get_point_metrics(torch.from_numpy(x), torch.from_numpy(y))
    g1 = pointmetrics.get_point_metrics(torch.from_numpy(x[31:32]), torch.from_numpy(y[31:32]))
    assert all(gm[k][31] == g1[k][0] for k in gm)


def test_frame_axis_beyond_grid_limit():
    B, V = 70000, 778
    gen = torch.Generator(device="cuda").manual_seed(0)
    tpl = torch.from_numpy(synthetic_mano(0)["v_template"].astype(np.float32)).cuda()
    x = tpl + 0.01 * torch.randn(B, V, 3, device="cuda", generator=gen)
    y = tpl + 0.01 * torch.randn(B, V, 3, device="cuda", generator=gen)
    out4, (xd, xi, yd, yi) = ops.cloud_metrics(x, y, per_point=True)
    assert torch.isfinite(out4).all()
    for b in (0, 65534, 65535, 69999):
        check_frame(x[b].cpu().numpy(), y[b].cpu().numpy(), out4[b].cpu().numpy(), xd[b].cpu().numpy(),
                    xi[b].cpu().numpy(), yd[b].cpu().numpy(), yi[b].cpu().numpy())


def test_bad_shapes_raise_value_error():
    a, b = torch.zeros(2, 10, 3), torch.zeros(3, 10, 3)
    with pytest.raises(ValueError):
        pointmetrics.get_point_metrics(a, b)
    with pytest.raises(ValueError):
        pointmetrics.get_point_metrics(torch.zeros(2, 0, 3), a)
    with pytest.raises(ValueError):
        pointmetrics.get_point_metrics(a, torch.zeros(2, 10, 2))
    h = torch.zeros(4, 778, 3)
    with pytest.raises(ValueError):
        pointmetrics.get_align_metrics(h, h, torch.zeros(3, 10, 3), torch.zeros(3, 12, 3))       # 4 hands for 3 frames
    with pytest.raises(ValueError):
        pointmetrics.get_align_metrics(h, h[:, :700], torch.zeros(2, 10, 3), torch.zeros(2, 12, 3))
    with pytest.raises(ValueError):
        pointmetrics.get_align_metrics(h, h, torch.zeros(2, 10, 3), torch.zeros(1, 12, 3))
