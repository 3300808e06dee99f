"""The references of tests/lossterms_ref.py against the CPU oracle, the exact gate scenes decided by the oracle itself, and the
float32 floors E32_* of the frame-loss terms: the reference in float32 against the reference in float64, `util.deviation` per
output tensor, over every case of the GPU grid (tests/test_lossterms_edges_gpu.py).  Every figure is printed (pytest -s) and every
constant is pinned from both sides; none is taken from a kernel.  The kernels sum the same float32 terms in another order: the
GPU test allows them E32_FACTOR times the floor.  CPU only."""
import types

import numpy as np
import torch

from tests import lossterms_ref as lr
from tests import util

E32_V2D_LOSS = 1.1e-7         # v2d loss (largest: one frame of 257 vertices)
E32_V2D_METRIC = 1.0e-7       # v2d pixel metric
E32_V2D_GRAD = 2.6e-7         # d v2d / d verts (a quotient rule's difference per element)
E32_SMOOTH = 1.6e-7           # smoothness value
E32_SMOOTH_GRAD = 1.2e-7      # smoothness gradient
E32_PCA = 1.8e-7              # PCA prior and the two scale priors
E32_PCA_GRAD = 7.5e-8         # their gradients
E32_INTER_SUM = 3.2e-6        # interaction: per-frame centroid MSE and the per-clip sum (largest: Vh 1500, Vo 778 - the centroids
#                               are 0.6 from the origin and 0.02 apart: the difference of two float32 means cancels five bits)
E32_INTER_GRAD = 4.0e-6       # interaction: record vector and both mesh gradients (the same difference)
E32_OFFSCREEN = 1.3e-7        # off-screen value (clouds, the whole exact scene, each of its vertices alone but the four below)
E32_OFFSCREEN_GRAD = 1.5e-7   # off-screen gradient (every case, single vertices included)
E32_OFFSCREEN_HINGE = 2.7e-4  # off-screen value of ONE vertex a float32 step (2^-22) beyond an NDC plane at z = 16: float32
#                               absorbs the 1e-9 under the division, float64 does not - 2 * 0.5 * 1e-9 / 16 of 2^-22
E32_SUM_SMALL = 1.2e-7        # hm_sum_small_clips on random data
E32_FACTOR = util.E32_FACTOR


def _pinned(worst, bar):
    assert 0.5 * bar < worst <= bar, (worst, bar)


def _dev(got, want):
    return util.deviation(torch.as_tensor(got).detach().numpy(), torch.as_tensor(want).detach().numpy())


def _ops_hand_obj(B=5, seed=0):
    """the scene of tests/test_ops_gpu.py::test_inter_and_contact, written out: frame 4 gated off by z, frame 3 by the boxes"""
    from homan_amd import synth
    from homan_amd.mano_assets import synthetic_mano
    g = torch.Generator().manual_seed(seed)
    m = synthetic_mano(0)
    vh = torch.from_numpy(m["v_template"])[None].repeat(B, 1, 1) + torch.randn(B, 1, 3, generator=g) * 0.01
    vh = vh + torch.tensor([0.0, 0.0, 0.55])
    ov, _ = synth.bottle_mesh()
    vo = torch.from_numpy(ov)[None].repeat(B, 1, 1) + torch.tensor([0.02, 0.0, 0.56]) + torch.randn(B, 1, 3, generator=g) * 0.01
    vh[4] += torch.tensor([0.0, 0.0, 5.0])
    vh[3] += torch.tensor([2.0, 0.0, 0.0])
    return vh, vo


def test_hand_term_refs_match_the_oracle():
    """v2d_ref, smooth_ref, priors_ref against OracleLosses.compute_verts2d_loss_hand, compute_smooth_loss, compute_pca_loss and
    compute_intrinsic_scale_prior at the scene of test_ops_gpu (B = 5, V = 778) and with two hands per frame under five distinct
    general cameras (skew, bottom row other than (0, 0, 1): the lookup n // hand_nb and the general K against the oracle): values,
    the metric and every gradient within E32_FACTOR floors (the oracle is float32 and sums in its own order)."""
    from oracle import model as om
    for nb in (1, 2):
        verts, camintr, ref2d, vob, pca = lr.ops_scene(nb)
        losses = om.OracleLosses(camintr, None, None, ref2d, None, nb, "centroid", 32)
        vo = verts.clone().requires_grad_(True)
        lo, mo = losses.compute_verts2d_loss_hand(vo, 256)
        lo["loss_v2d_hand"].backward()
        loss, metric, grad = lr.v2d_ref(verts, camintr, nb, ref2d, 256.0)
        if nb == 2:                  # the lookup is observable: every frame under camera 0 is another loss
            assert not torch.equal(camintr[0], camintr[1]) and camintr[0, 0, 1] != 0 and camintr[0, 2, 0] != 0
            assert abs(float(lr.v2d_ref(verts, camintr[:1].repeat(5, 1, 1), nb, ref2d, 256.0)[0]) - float(loss)) > 1e-3 * float(loss)
        d = (_dev(lo["loss_v2d_hand"], loss), abs(mo["v2d_hand"] - float(metric)) / float(metric), _dev(vo.grad, grad))
        print(f"oracle vs v2d_ref hand_nb={nb}: loss {d[0]:.3e} metric {d[1]:.3e} gradient {d[2]:.3e}")
        assert float(loss) > 0 and d[0] <= E32_FACTOR * E32_V2D_LOSS and d[1] <= E32_FACTOR * E32_V2D_METRIC
        assert d[2] <= E32_FACTOR * E32_V2D_GRAD
        a, b = verts.clone().requires_grad_(True), vob.clone().requires_grad_(True)
        sm = om.compute_smooth_loss(a, b)
        (sm["loss_smooth_hand"] + sm["loss_smooth_obj"]).backward()
        for name, x, got, k in (("hand", a, sm["loss_smooth_hand"], nb), ("obj", b, sm["loss_smooth_obj"], 1)):
            val, g = lr.smooth_ref(x.detach(), k)
            d = (_dev(got, val), _dev(x.grad, g))
            print(f"oracle vs smooth_ref {name} hand_nb={k}: value {d[0]:.3e} gradient {d[1]:.3e}")
            assert float(val) > 0 and d[0] <= E32_FACTOR * E32_SMOOTH and d[1] <= E32_FACTOR * E32_SMOOTH_GRAD
        po = pca.clone().requires_grad_(True)
        so, sh = torch.tensor([1.2], requires_grad=True), torch.tensor([0.9], requires_grad=True)
        l0 = om.compute_pca_loss(po)["loss_pca"]
        l1, l2 = om.compute_intrinsic_scale_prior(so, torch.ones(1)), om.compute_intrinsic_scale_prior(sh, torch.ones(1))
        (l0 + l1 + l2).backward()
        vals, grads = lr.priors_ref(pca, so.detach(), torch.ones(1), sh.detach(), torch.ones(1))
        d = [_dev(x, y) for x, y in zip((l0, l1, l2), vals)] + [_dev(x.grad.reshape(y.shape), y) for x, y in zip((po, so, sh), grads)]
        print("oracle vs priors_ref: values %.3e %.3e %.3e gradients %.3e %.3e %.3e" % tuple(d))
        assert max(d[:3]) <= E32_FACTOR * E32_PCA and max(d[3:]) <= E32_FACTOR * E32_PCA_GRAD
    # no pair: the project's convention against the oracle's NaN
    val, g = lr.smooth_ref(torch.randn(2, 7, 3), 2)
    assert float(val) == 0.0 and not g.any()
    assert torch.isnan(om.compute_smooth_loss(torch.randn(1, 7, 3), torch.randn(1, 9, 3))["loss_smooth_hand"])


def test_inter_ref_matches_the_oracle_and_its_flags():
    """inter_ref against OracleLosses.compute_interaction_loss (one and two hands) with both gradients, and the float32 restatement
    of the gate against assign_interaction_pairs on EVERY frame of every random scene of the GPU grid: no frame may disagree."""
    from oracle import model as om
    vh, vo = _ops_hand_obj()
    B = len(vh)
    camintr = torch.tensor([[1.37, 0, 0.5], [0, 1.37, 0.5], [0, 0, 1.0]]).repeat(B, 1, 1)
    losses = om.OracleLosses(camintr, None, None, None, None, 1, "centroid", 32)
    vh2 = vh + torch.tensor([0.01, -0.02, 0.03])                  # a second hand per frame
    for hands in ([vh], [vh, vh2]):
        hs = [h.clone().requires_grad_(True) for h in hands]
        b = vo.clone().requires_grad_(True)
        lo, _ = losses.compute_interaction_loss(torch.stack(hs, 1), b.unsqueeze(1))
        (lo["loss_inter"] * 2).sum().backward()
        refs = [lr.inter_ref(h, vo, camintr, lr.INTER_EXPANSION, lr.INTER_ZTHRESH, upstream=2.0) for h in hands]
        want, g_obj = sum(r["total"] for r in refs), sum(r["g_obj"] for r in refs)
        d = [_dev(lo["loss_inter"], want), _dev(b.grad, g_obj)] + [_dev(h.grad, r["g_hand"]) for h, r in zip(hs, refs)]
        print(f"oracle vs inter_ref, {len(hands)} hand(s): sum {d[0]:.3e} g_obj {d[1]:.3e} g_hand " + " ".join(f"{x:.3e}" for x in d[2:]))
        assert float(want) > 0 and d[0] <= E32_FACTOR * E32_INTER_SUM and max(d[1:]) <= E32_FACTOR * E32_INTER_GRAD
        for h, r in zip(hands, refs):
            assert list(r["flag"]) == losses.assign_interaction_pairs(h, vo) == [1, 1, 1, 0, 0]
            # the record's vector is the gradient of the frame's MSE to either centroid
            np.testing.assert_allclose((r["g_hand"].sum(1) / 2.0).numpy(), r["gvec"].numpy(), rtol=1e-12, atol=1e-18)
    assert np.float32(1.0 + lr.INTER_EXPANSION) == np.float32(1.0) + np.float32(lr.INTER_EXPANSION)      # (the kernel's factor)
    frames = 0
    for name, (h, o, K, e, zt, _) in lr.inter_cases().items():
        if name.startswith(("gate", "point")):
            continue                                    # (expansions the oracle's method does not take: the next test)
        assert (e, zt) == (om.INTERACTION_BBOX_EXPANSION, float(om.INTERACTION_Z_THRESH))
        want = om.OracleLosses(K, None, None, None, None, 1, "centroid", 32).assign_interaction_pairs(h, o)
        got = lr.inter_gate32(h, o, K, e, zt)
        wrong = int((np.asarray(want) != got["flag"]).sum())
        frames += len(want)
        print(f"flags {name}: {sum(want)} of {len(want)} frames interact, {wrong} differ from the oracle")
        assert wrong == 0, name
        np.testing.assert_array_equal(got["box_hand"], om.project_bbox(h, K, e).numpy())          # the boxes themselves: the same bits
        np.testing.assert_array_equal(got["box_obj"], om.project_bbox(o, K, e).numpy())
    assert frames > 300


def test_exact_gate_scenes_are_decided_by_the_oracle_as_listed():
    """On the exact scenes the oracle's own functions (project_bbox, compute_iou, compute_dist_z) decide as lossterms_ref lists,
    the float32 restatement decides the same from the same boxes, and float32 and float64 box edges are identical."""
    from oracle import model as om
    K = torch.tensor(lr.GATE_K)[None]
    for e in lr.GATE_EXPANSIONS:
        assert np.float32(1.0 + e) == np.float32(1.0) + np.float32(e)
        for name, vh, vo, flag, zd in lr.gate_scenes(e):
            h, o = torch.from_numpy(vh), torch.from_numpy(vo)
            bo, bh = om.project_bbox(o, K, e), om.project_bbox(h, K, e)
            iou = om.compute_iou(bo[0], bh[0])
            z = om.compute_dist_z(o[0], h[0])
            oracle_flag = 1 if (iou > 0) and (z < om.INTERACTION_Z_THRESH) else 0
            g = lr.inter_gate32(vh, vo, K.numpy(), e, lr.INTER_ZTHRESH)
            print(f"gate scene e={e} {name}: oracle IoU {float(iou):.9g} z distance {float(z):.9g} flag {oracle_flag}")
            assert oracle_flag == flag == int(g["flag"][0]), name
            assert float(z) == zd == float(g["zd"][0]), name
            for b32, b_or, v in ((g["box_obj"], bo, vo), (g["box_hand"], bh, vh)):
                np.testing.assert_array_equal(b32, b_or.numpy())
                np.testing.assert_array_equal(b32.astype(np.float64), lr.inter_boxes64(v, K.numpy(), e))
            np.testing.assert_array_equal(g["iou"], np.float32(float(iou)))                       # (NaN == NaN here)
            if name == "touch":
                assert float(iou) == 0.0 and (bo[0, 2] == bh[0, 0] or bo[0, 0] == bh[0, 2])
            if name == "quantum":
                assert min(float(bo[0, 2] - bh[0, 0]), float(bh[0, 2] - bo[0, 0])) == 2.0 ** -24
            if name == "point":
                assert torch.isnan(iou)


def test_offscreen_ref_matches_the_oracle():
    """offscreen_ref against PoseOptimizer.compute_offscreen_loss (float32) on every cloud of the GPU grid, value and gradient
    (clouds: no vertex on a plane, where torch.max's subgradient 1/2 would differ from relu's 0)."""
    from oracle import poseopt
    for name, (v, K, w) in lr.offscreen_cases().items():
        if not name.startswith("cloud"):
            continue
        me = types.SimpleNamespace(K=K[None], far=lr.ZFAR)
        x = v.clone().requires_grad_(True)
        lo = w * poseopt.PoseOptimizer.compute_offscreen_loss(me, x)
        lo.sum().backward()
        out, g = lr.offscreen_ref(v, K, lr.ZFAR, w)
        d = (_dev(lo, out), _dev(x.grad, g))
        print(f"oracle vs offscreen_ref {name}: value {d[0]:.3e} gradient {d[1]:.3e}")
        assert (float(out.max()) > 0 or v.shape[1] == 1) and d[0] <= E32_FACTOR * E32_OFFSCREEN and d[1] <= E32_FACTOR * E32_OFFSCREEN_GRAD
    ex, names = lr.offscreen_exact_scene()
    out, g = lr.offscreen_ref(ex, torch.tensor(lr.GATE_K), lr.ZFAR, 1.0, dtype=torch.float32)
    for i, n in enumerate(names):           # float32: on a plane and inside exactly nothing, outside exactly the step
        o1, g1 = lr.offscreen_ref(ex[:, i:i + 1], torch.tensor(lr.GATE_K), lr.ZFAR, 1.0, dtype=torch.float32)
        if n.endswith(("on", "inside")) or n in ("z0+", "zfar"):
            assert float(o1) == 0.0 and not g1.any(), n
        elif n.endswith("outside"):
            assert float(o1) == 2.0 ** -22 and g1.any(), n
    assert bool(torch.equal(g[0, 13], torch.tensor([0.0, 0.0, -1.0]))) and bool(torch.equal(g[0, 15], torch.tensor([0.0, 0.0, 1.0])))


def test_log_total_ref_and_adam_helper():
    """log_total_ref skips a NaN under a zero weight and adds in index order; adam_oracle_run drives oracle.adam.Adam: a tensor whose
    gradient is zero from the first step does not move, and a preset step counter changes the bias corrections."""
    vals, w = lr.log_scene(3, 13)
    for c in range(3):
        t = lr.log_total_ref(vals[c, :13], w)
        assert np.isfinite(t) and t.dtype == np.float32
        keep = [i for i in range(13) if i != 6]
        np.testing.assert_allclose(t, float((vals[c, keep].double() * w[keep].double()).sum()), rtol=1e-5)
    assert np.isnan(lr.log_total_ref([np.nan, 1.0], [1.0, 1.0])) and lr.log_total_ref([np.nan, 1.0], [0.0, 2.0]) == 2.0
    params, grads = lr.adam_inputs((5, 4, 1), 3)
    a, b = lr.adam_oracle_run(params, grads, (1e-2, 1e-1, 1e-3)), lr.adam_oracle_run(params, grads, (1e-2, 1e-1, 1e-3), t0=999)
    assert np.array_equal(a[-1][1][0], params[1].numpy()) and not a[-1][1][2].any()
    assert not np.array_equal(a[0][0][0], b[0][0][0]) and np.array_equal(a[0][0][1], b[0][0][1])
    assert all(np.isfinite(x).all() for step in a + b for ts in step for x in ts)


def test_float32_floors():
    """Each reference in float32 against itself in float64 over every case of the GPU grid; the worst deviation per group is the
    floor E32_*, pinned from both sides."""
    worst = dict(v2d=0.0, metric=0.0, v2d_g=0.0, smooth=0.0, smooth_g=0.0, pca=0.0, pca_g=0.0, inter=0.0, inter_g=0.0, off=0.0,
                 off_g=0.0, hinge=0.0, sum_small=0.0)

    def note(key, got, want, tag):
        d = _dev(got, want)
        worst[key] = max(worst[key], d)
        return f"{tag} {d:.3e}"

    f32 = torch.float32
    for name, (verts, K, ref2d, nb) in lr.hand_cases().items():
        a, b = lr.v2d_ref(verts, K, nb, ref2d, lr.IMAGE_SIZE), lr.v2d_ref(verts, K, nb, ref2d, lr.IMAGE_SIZE, dtype=f32)
        s, t = lr.smooth_ref(verts, nb), lr.smooth_ref(verts, nb, dtype=f32)
        print(f"e32 hand terms {name}:", note("v2d", b[0], a[0], "loss"), note("metric", b[1], a[1], "metric"),
              note("v2d_g", b[2], a[2], "gradient"), note("smooth", t[0], s[0], "smooth"), note("smooth_g", t[1], s[1], "gradient"))
    for name, (verts, nb) in lr.smooth_only_cases().items():
        s, t = lr.smooth_ref(verts, nb), lr.smooth_ref(verts, nb, dtype=f32)
        print(f"e32 smoothness {name}:", note("smooth", t[0], s[0], "value"), note("smooth_g", t[1], s[1], "gradient"))
    for npca in lr.PRIOR_NPCA:
        sc = lr.priors_scene(npca, 3)
        for c in range(3):
            a, b = lr.priors_ref(*[x[c] for x in sc]), lr.priors_ref(*[x[c] for x in sc], dtype=f32)
            print(f"e32 priors npca={npca} clip {c}:", *[note("pca", y, x, "value") for x, y in zip(a[0], b[0])],
                  *[note("pca_g", y, x, "gradient") for x, y in zip(a[1], b[1])])
    for name, (h, o, K, e, zt, cl) in lr.inter_cases().items():
        for up in lr.INTER_UPSTREAMS:
            a, b = lr.inter_ref(h, o, K, e, zt, cl, up), lr.inter_ref(h, o, K, e, zt, cl, up, dtype=f32)
            print(f"e32 interaction {name} upstream {up}:", note("inter", b["mse"], a["mse"], "mse"), note("inter", b["total"], a["total"], "sum"),
                  note("inter_g", b["gvec"], a["gvec"], "record"), note("inter_g", b["g_hand"], a["g_hand"], "g_hand"),
                  note("inter_g", b["g_obj"], a["g_obj"], "g_obj"))
    for name, (v, K, w) in lr.offscreen_cases().items():
        a, b = lr.offscreen_ref(v, K, lr.ZFAR, w), lr.offscreen_ref(v, K, lr.ZFAR, w, dtype=f32)
        key = "hinge" if name.endswith("outside") else "off"
        print(f"e32 off-screen {name}:", note(key, b[0], a[0], "value"), note("off_g", b[1], a[1], "gradient"))
    for n in lr.SUM_SMALL_N:
        parts, extra = lr.sum_small_scene(n, 3, exact=False)
        for ex in (None, extra):
            a, b = lr.sum_small_ref(parts, lr.SUM_SMALL_W[0], ex, lr.SUM_SMALL_W[1]), lr.sum_small_ref(parts, lr.SUM_SMALL_W[0], ex, lr.SUM_SMALL_W[1], dtype=f32)
            print(f"e32 sum_small n={n} extra={'yes' if ex is not None else 'no'}:", note("sum_small", b, a, "sum"))
        pe, ee = lr.sum_small_scene(n, 3, exact=True)
        assert torch.equal(lr.sum_small_ref(pe, lr.SUM_SMALL_W[0], ee, lr.SUM_SMALL_W[1], dtype=f32).double(),
                           lr.sum_small_ref(pe, lr.SUM_SMALL_W[0], ee, lr.SUM_SMALL_W[1]))
    print("floors: " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for key, bar in (("v2d", E32_V2D_LOSS), ("metric", E32_V2D_METRIC), ("v2d_g", E32_V2D_GRAD), ("smooth", E32_SMOOTH),
                     ("smooth_g", E32_SMOOTH_GRAD), ("pca", E32_PCA), ("pca_g", E32_PCA_GRAD), ("inter", E32_INTER_SUM),
                     ("inter_g", E32_INTER_GRAD), ("off", E32_OFFSCREEN), ("off_g", E32_OFFSCREEN_GRAD),
                     ("hinge", E32_OFFSCREEN_HINGE), ("sum_small", E32_SUM_SMALL)):
        _pinned(worst[key], bar)
