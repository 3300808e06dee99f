"""Pair terms (nearest-vertex search, contact, SDF interpenetration): the references of tests/util.py against the CPU oracle, and the
float32 noise floors the GPU tolerances of tests/test_pairterms_edges_gpu.py derive from.  CPU only.

A floor is the largest deviation (util.deviation: max |difference| / max |reference|, per output tensor) of the SAME formulas
evaluated in float32 on the CPU - torch float32 for the contact term, the oracle (float32 torch + its C grid) for the SDF term -
from the float64 reference, over every case of the group.  The tests below print every figure and pin each constant from both
sides; no constant was taken from a kernel.  The kernels add the same float32 terms in another order and get E32_FACTOR times
the floor, the margin of the depth term (util.E32_FACTOR).
"""
import numpy as np
import pytest
import torch

from tests import util

E32_CONTACT = 1.2e-7          # contact loss (largest: Vo = 1, Vh = 1, one frame - a single rounded tanh)
E32_CONTACT_GRAD = 5.8e-7     # both contact gradients (largest: the object's, float32 scatter-add of up to 778 picks)
E32_SDF_LOSS = 8.5e-7         # sum of all samples (largest: F256_vs_F260)
E32_SDF_GRAD = 7.6e-6         # gradients to the sampled vertices (largest: F256_vs_F260; a difference of grid values x 16 / scale)
E32_SDF_VALUES = 3.0e-6       # dist_values (largest: ops_cube)
E32_OCTA_PHI = 4.3e-8         # |oracle phi - (1 - |x| - |y| - |z|) / sqrt 3| on the octahedron, absolute, normalised units
E32_FACTOR = util.E32_FACTOR


def _pinned(worst, bar):
    assert 0.5 * bar < worst <= bar, (worst, bar)


def test_nn_bruteforce32_is_the_float64_minimum():
    """util.nn_bruteforce32: its pick is within 1e-6 (relative) of the float64 minimum on every shape of the GPU grid, and on the
    lattice clouds - where every squared distance is exact - it IS the first float64 argmin."""
    for Vh, Vo in util.NN_SHAPES:
        vh, vo = util.nn_clouds(3, Vh, Vo)
        idx, d2, metric = util.nn_bruteforce32(vh, vo)
        d64 = ((vh.astype(np.float64)[:, :, None] - vo.astype(np.float64)[:, None]) ** 2).sum(-1)
        picked = np.take_along_axis(d64, idx[..., None], 2)[..., 0]
        assert (picked - d64.min(2) <= 1e-6 * d64.min(2) + 1e-12).all(), (Vh, Vo)
        assert d2.dtype == np.float32 and metric.dtype == np.float32
        np.testing.assert_allclose(metric, np.sqrt(d64.min((1, 2))).max(), rtol=1e-6)
    for Vo in (300, 1024):
        vh, vo = util.nn_tie_clouds(3, 129, Vo)
        idx, d2, _ = util.nn_bruteforce32(vh, vo)
        d64 = ((vh.astype(np.float64)[:, :, None] - vo.astype(np.float64)[:, None]) ** 2).sum(-1)
        assert np.array_equal(idx, d64.argmin(2)) and np.array_equal(d2.astype(np.float64), d64.min(2))
        across_waves, across_groups = util.nn_tie_spread(d64)
        print(f"nn ties Vo={Vo}: minimum in several waves' shares for {across_waves} hand vertices, in several groups of a share for {across_groups}")
        assert across_waves > 100 and across_groups > 20                 # of 3 x 129


def test_contact_ref_matches_the_oracle_and_the_float32_floor():
    """util.contact_ref against oracle.model.compute_contact_loss with the oracle's own neighbour choice passed in (hand against
    bottle, the scene of test_ops_gpu), then float32 against float64 over every shape of the GPU test: E32_CONTACT*."""
    from homan_amd.mano_assets import synthetic_mano
    from oracle import model as om
    from oracle import yana
    m = synthetic_mano(0)
    v0, f0, v1, f1 = util.sdf_scenes(m)["ops_bottle"]
    a, b = torch.from_numpy(v0).clone().requires_grad_(True), torch.from_numpy(v1).clone().requires_grad_(True)
    B = len(v0)
    co = om.compute_contact_loss(a, b, torch.from_numpy(f1).long()[None].repeat(B, 1, 1), torch.from_numpy(f0).long())["loss_contact"]
    co.sum().backward()
    idx_o = yana.batch_pairwise_dist(torch.from_numpy(v0), torch.from_numpy(v1)).min(2)[1]
    want, gh, go = util.contact_ref(v0, v1, idx_o)
    devs = (util.deviation(co.detach().numpy(), want.numpy()), util.deviation(a.grad.numpy(), gh.numpy()),
            util.deviation(b.grad.numpy(), go.numpy()))
    print("contact oracle vs float64 reference: loss %.3e g_hand %.3e g_obj %.3e" % devs)
    assert float(want) > 0 and devs[0] <= E32_CONTACT and max(devs[1:]) <= E32_CONTACT_GRAD
    worst_l = worst_g = 0.0
    cases = [(B, Vh, Vo, "random", 0) for Vo in util.CONTACT_VO for Vh in util.CONTACT_VH for B in util.CONTACT_B]
    cases += [(3, 778, 4096, "same", 0), (3, 778, 9000, "last_range", 0), (3, 778, 64, "random", 5), (3, 257, 4097, "random", 5)]
    for B, Vh, Vo, kind, zeros in cases:
        vh, vo, nn = util.contact_scene(B, Vh, Vo, kind, zeros=zeros)
        want = util.contact_ref(vh, vo, nn)
        got = util.contact_ref(vh, vo, nn, dtype=torch.float32)
        d = [util.deviation(x.numpy(), y.numpy()) for x, y in zip(got, want)]
        print(f"contact B={B} Vh={Vh} Vo={Vo} {kind} zeros={zeros}: e32 loss {d[0]:.3e} g_hand {d[1]:.3e} g_obj {d[2]:.3e}")
        assert all(torch.isfinite(x).all() for x in want)
        if Vh >= 2:
            ratio = np.linalg.norm(np.take_along_axis(vo, nn[..., None].astype(np.int64).repeat(3, -1), 1).astype(np.float64) - vh,
                                   axis=-1) / util.CONTACT_THRESH
            assert ratio[ratio > 0].min() < 1.2e-4 and ratio.max() > 19.0             # the linear end and full saturation
        if zeros:
            dead = (np.take_along_axis(vo, nn[..., None].astype(np.int64).repeat(3, -1), 1) == vh).all(-1)
            assert dead.sum() == B * zeros and not want[1][torch.from_numpy(dead)].any()       # subgradient 0
        worst_l, worst_g = max(worst_l, d[0]), max(worst_g, d[1], d[2])
    print(f"contact floors: loss {worst_l:.3e} gradients {worst_g:.3e}")
    _pinned(worst_l, E32_CONTACT)
    _pinned(worst_g, E32_CONTACT_GRAD)


def _sdf_cases(mano_model):
    scenes = util.sdf_scenes(mano_model)
    cases = [(n, scenes[n], 0.2) for n in util.SDF_SCENE_NAMES]
    return cases + [("octahedron", util.octahedron_scene(), 0.0), ("frames", util.frames_scene(), 0.2),
                    ("shell", util.shell_scene()[0], 0.0)]


def test_sdf_scene_ref_matches_the_oracle_and_the_float32_floor(mano_model):
    """util.sdf_scene_ref (float64 on the oracle's grids) against oracle.model.sdf_scene_loss (float32) on every scene of the GPU
    test: loss, both gradients, both dist_values.  The largest deviations are E32_SDF_*."""
    worst = [0.0, 0.0, 0.0]
    for name, scene, sf in _sdf_cases(mano_model):
        lo, go, meta = util.oracle_sdf(scene, sf)
        want, gw, dist = util.sdf_scene_ref(meta["sdfs"], [scene[0], scene[2]], sf)
        d = [util.deviation(lo.numpy(), want.numpy()), max(util.deviation(a.numpy(), b.numpy()) for a, b in zip(go, gw)),
             max(util.deviation(meta["dist_values"][k].detach().numpy(), dist[k].numpy()) for k in dist)]
        print(f"sdf {name}: loss {float(want):.9g} e32 loss {d[0]:.3e} gradients {d[1]:.3e} values {d[2]:.3e}")
        assert float(want) > 0
        for a, b in zip(go, gw):                                         # the same vertices carry a gradient
            assert torch.equal(a.abs().sum(-1) != 0, b.abs().sum(-1) != 0), name
        worst = [max(w, x) for w, x in zip(worst, d)]
    print("sdf floors: loss %.3e gradients %.3e values %.3e" % tuple(worst))
    _pinned(worst[0], E32_SDF_LOSS)
    _pinned(worst[1], E32_SDF_GRAD)
    _pinned(worst[2], E32_SDF_VALUES)


def test_octahedron_known_answer_on_the_oracle():
    """The oracle's grid of the unit octahedron: voxel-centre rays pass exactly through the projected edges |y| + |z| = 1 and the
    half-open rule still gives inside iff |x| + |y| + |z| < 1 (5440 voxels); phi = (1 - |x| - |y| - |z|) / sqrt 3 to E32_OCTA_PHI."""
    scene = util.octahedron_scene()
    _, _, meta = util.oracle_sdf(scene, 0.0)
    inside, phi = util.octahedron_exact()
    assert inside.sum() == util.OCTA_INSIDE
    c = -1.0 + (np.arange(32) + 0.5) / 16.0
    assert (np.abs(c)[:, None] + np.abs(c)[None] == 1).sum() == 64       # rows whose ray runs along an edge of the projection
    worst = 0.0
    for k in (0, 1):                                                     # the half-size copy normalises to the same grid
        got = meta["sdfs"][k][0].numpy()
        assert np.array_equal(got > 0, inside)
        worst = max(worst, np.abs(got - phi).max())
    print(f"octahedron: |phi - exact| {worst:.3e}")
    _pinned(worst, E32_OCTA_PHI)


def test_scene_builders_reach_the_edges_they_are_for(mano_model):
    """frames_scene: frames 1 and 3 sample nothing, frame 2 one way only; shell_scene: the owner fills its grid, and the loose
    vertices' float32 grid indices are SHELL_IX exactly where those are multiples of 1/4; sdf_need_ref lists nothing outside."""
    a, af, b, bf = util.frames_scene()
    _, _, meta = util.oracle_sdf((a, af, b, bf))
    _, gw, dist = util.sdf_scene_ref(meta["sdfs"], [a, b])
    live = [[bool(dist[k][f].max() > 0) for k in ((0, 1), (1, 0))] for f in range(4)]
    assert live == [[True, True], [False, False], [True, False], [False, False]], live
    inside = [(p > 0).numpy() for p in meta["sdfs"]]
    for f in range(4):
        n0 = util.sdf_need_ref(a[f:f + 1], b[f:f + 1], inside[0][f:f + 1], 0.2).sum()
        n1 = util.sdf_need_ref(b[f:f + 1], a[f:f + 1], inside[1][f:f + 1], 0.2).sum()
        assert [n0 > 0, n1 > 0] == live[f]
        assert not gw[0][f].any() == (not live[f][1]) and (not gw[1][f].any()) == (not live[f][0])
    (owner, _, sampled, _), ix = util.shell_scene()
    _, _, meta = util.oracle_sdf((owner, util.shell_scene()[0][1], sampled, util.shell_scene()[0][3]), 0.0)
    assert bool((meta["sdfs"][0] > 0).all())
    f32 = np.float32
    lo, hi = owner[0].min(0), owner[0].max(0)
    ctr, sc = (lo + hi) / f32(2), ((hi - lo) * f32(0.5)).max()
    got = (((sampled[0, 4:] - ctr) / sc + f32(1)) * f32(32) - f32(1)) / f32(2)
    exact = ix == np.round(ix * 4) / 4
    assert np.array_equal(got[exact].astype(np.float64), ix[exact])
    np.testing.assert_allclose(got, ix, atol=2e-5)
    assert exact.sum() == 72 - 6 and (~exact).sum() == 3 * 2
