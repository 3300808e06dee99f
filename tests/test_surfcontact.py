"""CPU side of the surface contact loss (csrc/surfcontact.hip, ops.surface_contact_loss): known answers of the fp32 NumPy
restatement tests/surfcontact_ref.py, which the GPU tests hold the kernel to bit for bit; the envelope gradient against central
differences of an independently built float64 distance; hm_tanh restated; the range of the exact sums; how far the fp32
restatement lies from float64; and the argument checks that need no device.

Floors (fp32 restatement against the float64 reference of surfcontact_ref.reference64, which is given the fp32 search's face and
inside flag; `util.deviation` = max |difference| / max |reference|), measured on the CPU over `comparison_cases()` and pinned
from both sides - the constants below come from this measurement, never from the kernel:
                 values     point gradient   vertex gradient (attraction, repulsion together)
  hand->box      5.623e-08  2.250e-06        6.076e-07
  box->hand      4.813e-07  2.764e-04        4.628e-05
  hand->bottle   1.897e-06  1.642e-04        5.628e-05
  bottle->hand   4.016e-06  4.679e-04        3.291e-05
The gradient floors are set by the world-space form of p - q: the closest point is formed in world coordinates (the bottle sits
0.66 m from the origin: half an ulp of a coordinate is 3e-8 m) and the worst points lie 1e-5 to 1e-4 m from the surface, where
(p - q) / d turns that rounding into up to a few 1e-4 of a unit vector."""
import math

import numpy as np
import pytest
import torch

from tests import surfcontact_ref as cref
from tests import surfmetrics_ref as sref
from tests import util
from tests.test_surfmetrics import REGIONS, TRI, comparison_cases, restated

F32, F64 = np.float32, np.float64
MESH_CASES = ("hand->box", "box->hand", "hand->bottle", "bottle->hand")
# name -> (values, point gradient, vertex gradients): the floors measured by test_floors_of_the_fp32_restatement
E32 = {"hand->box": (5.7e-8, 2.3e-6, 6.1e-7), "box->hand": (4.9e-7, 2.8e-4, 4.7e-5), "hand->bottle": (1.9e-6, 1.7e-4, 5.7e-5),
       "bottle->hand": (4.1e-6, 4.7e-4, 3.3e-5)}


def _pinned(worst, bar):
    assert 0.5 * bar < worst <= bar, (worst, bar)


# =============================================================================================== known answers
REGION_WEIGHTS = {"A": [1.0, 0.0, 0.0], "B": [0.0, 1.0, 0.0], "C": [0.0, 0.0, 1.0], "AB": [0.5, 0.5, 0.0], "AC": [0.5, 0.0, 0.5],
                  "BC": [0.0, 0.5, 0.5], "interior": [0.5, 0.25, 0.25]}


@pytest.mark.parametrize("region", sorted(REGIONS))
@pytest.mark.parametrize("dtype", (F32, F64))
def test_weights_on_the_seven_regions_of_a_right_triangle(region, dtype):
    p, q_want, d2_want = REGIONS[region]
    tri = TRI.astype(dtype)
    q, D, w, dv = cref.walk(np.asarray([p], dtype), tri[None, 0], tri[None, 1], tri[None, 2])
    assert q[0].tolist() == q_want and D[0] == d2_want and w[0].tolist() == REGION_WEIGHTS[region]
    assert dv[0].tolist() == (np.asarray(p) - np.asarray(q_want)).tolist()
    assert ((w[0][:, None] * tri).sum(0)).tolist() == q_want                 # the weights reproduce q


@pytest.mark.parametrize("region", sorted(REGIONS))
def test_gradients_on_the_seven_regions(region):
    """dd/dp = n = (p - q) / d and dd/dx_k = -w_k n: with c large against d, tanh is linear to fp32 (t = d / c up to (d/c)^2 / 3)
    and the term's g is phi n, its vertex gradient -w_k phi n"""
    p, q_want, d2_want = REGIONS[region]
    t = cref.terms(np.asarray([p], F32), TRI, np.array([[0, 1, 2]]), contact_thresh=1.0, collision_thresh=1.0)
    d = math.sqrt(d2_want)
    n = (np.asarray(p) - np.asarray(q_want)) / d
    th = math.tanh(d)
    assert t["face"][0] == 0 and t["inside"][0] == 0 and t["bary"][0].tolist() == REGION_WEIGHTS[region]
    assert t["value"][0] == pytest.approx(th, rel=2e-7)
    np.testing.assert_allclose(t["g"][0], (1 - th * th) * n, rtol=0, atol=3e-7)
    full = cref.loss_and_gradients(np.asarray([[p]], F32), TRI[None], np.array([[0, 1, 2]]), contact_thresh=1.0,
                                   collision_thresh=1.0)
    want = -np.asarray(REGION_WEIGHTS[region])[:, None] * ((1 - th * th) * n)[None]
    np.testing.assert_allclose(full["grad_verts_attr"][0], want, rtol=0, atol=3e-7)
    assert not full["grad_verts_rep"].any() and full["out"][1] == 0 and full["out"][0] == t["value"][0]
    np.testing.assert_array_equal(full["grad_points"][0, 0], t["g"][0])     # B N = 1


def test_degenerate_faces_give_the_segment_weights():
    # ab collapsed: the face is its segments; the point projects on bc (= ac) at t = 0.5
    a = np.array([[0.0, 0.0, 0.0]], F32)
    c = np.array([[2.0, 0.0, 0.0]], F32)
    p = np.array([[1.0, 1.0, 0.0]], F32)
    q, D, w, _ = cref.walk(p, a, a.copy(), c)
    assert q[0].tolist() == [1.0, 0.0, 0.0] and D[0] == 1.0 and w[0].tolist() == [0.0, 0.5, 0.5]       # bc before ca
    q, D, w, _ = cref.walk(p, a, c, c.copy())                                    # ab first
    assert w[0].tolist() == [0.5, 0.5, 0.0]
    q, D, w, _ = cref.walk(p, c, c.copy(), a)                                    # a = b: ab is a point (D = 2), bc wins
    assert w[0].tolist() == [0.0, 0.5, 0.5] and D[0] == 1.0
    q, D, w, _ = cref.walk(np.array([[3.0, 1.0, 0.0]], F32), a, np.array([[1.0, 0.0, 0.0]], F32), c)   # collinear, beyond c
    assert q[0].tolist() == [2.0, 0.0, 0.0] and w[0].tolist() == [0.0, 0.0, 1.0]


def test_zero_distance_no_face_and_weights():
    tri = TRI
    pts = np.array([[1.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.25, 0.25, 0.5], [0.25, 0.25, 0.5]], F32)
    t = cref.terms(pts, tri, np.array([[0, 1, 2]]), weights=np.array([1.0, 1.0, 0.0, 2.5], F32))
    assert t["value"][0] == 0 and not t["g"][0].any() and t["bary"][0].tolist() == [0.0, 1.0, 0.0]    # D == 0: on vertex b
    assert t["face"][1] == -1 and t["value"][1] == 0 and not t["g"][1].any() and not t["bary"][1].any()
    assert t["value"][2] == 0 and not t["g"][2].any()                                                   # zero weight
    one = cref.terms(pts[3:], tri, np.array([[0, 1, 2]]))
    assert t["value"][3] == F32(2.5) * one["value"][0]
    np.testing.assert_allclose(t["g"][3], F32(2.5) * one["g"][0], rtol=3e-7)
    # a face naming a vertex >= V is skipped by the search
    t = cref.terms(pts[2:3], tri, np.array([[0, 1, 3]]))
    assert t["face"][0] == -1 and t["value"][0] == 0


# =============================================================================================== the envelope gradient
def _u64(p, tri, c):
    d = sref.independent_distance(p, tri[0], tri[1], tri[2])
    return c * np.tanh(d / c)


@pytest.mark.parametrize("name", ("hand->box", "box->hand"))
def test_envelope_gradient_against_central_differences(name):
    """float64: u(p, x) = c tanh(dist(p, face) / c) with `independent_distance` (a differently built distance) differentiated by
    central differences in p and in the face's vertices, against g and -w_k g of the float64 walk.  Points away from region
    borders (their weights are not within 0.05 of a border of their region) and 1 mm or more from the surface, both signs."""
    p_all, v, f = comparison_cases()[name]
    s = restated(name)
    rng = np.random.default_rng(3)
    checked = {0: 0, 1: 0}
    for i in rng.permutation(len(p_all)):
        inside = int(s["inside"][i])
        if checked[inside] >= 12:
            continue
        tri = v[f[s["face"][i]]].astype(F64)
        p = p_all[i].astype(F64)
        q, D, w, dv = cref.walk(p[None], tri[None, 0], tri[None, 1], tri[None, 2])
        w, d = w[0], math.sqrt(D[0])
        if d < 1e-3 or np.any((w > 0) & (w < 0.05)) or np.any((w < 1) & (w > 0.95)):
            continue
        c = cref.COLLISION_THRESH if inside else cref.CONTACT_THRESH
        th = math.tanh(d / c)
        g = (1 - th * th) * dv[0] / d
        h = 1e-7
        num_p = np.array([(_u64(p + h * e, tri, c) - _u64(p - h * e, tri, c)) / (2 * h) for e in np.eye(3)])
        np.testing.assert_allclose(num_p, g, rtol=0, atol=2e-6)
        for k in range(3):
            num_x = np.empty(3)
            for a in range(3):
                tp, tm = tri.copy(), tri.copy()
                tp[k, a] += h
                tm[k, a] -= h
                num_x[a] = (_u64(p, tp, c) - _u64(p, tm, c)) / (2 * h)
            np.testing.assert_allclose(num_x, -w[k] * g, rtol=0, atol=2e-6)
        checked[inside] += 1
    assert checked == {0: 12, 1: 12}


# =============================================================================================== tanh, the grid
def test_hm_tanh_restated_is_within_half_an_ulp_of_tanh():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-25, 25, 20000), rng.uniform(-0.02, 0.02, 5000), 10.0 ** rng.uniform(-30, 1.3, 5000),
                        [0.0, 0.01, 20.0, 21.0, -20.0, 1e-38, 0.00999999977648258209228515625]]).astype(F32)
    got = cref.hm_tanh(x)
    want = np.tanh(x.astype(F64))
    ulp = np.spacing(np.abs(want).astype(F32)).astype(F64)
    assert got.dtype == F32 and (np.abs(got.astype(F64) - want) <= 0.5 * ulp * (1 + 1e-6)).all()
    assert (cref.hm_tanh(-x) == -got).all() and cref.hm_tanh(F32(0)) == 0


def test_the_grid_holds_every_point_on_one_face():
    """L = ceil(log2(N M)) - 50: 778 addends of the largest magnitude an addend can have stay below 2^51 quanta, and the default
    grid of the object chain (2^-44) would not: 778 * 2^44 > 2^53"""
    from homan_amd import ops
    L = cref.log2q(778)
    assert L == -40 == ops.surface_contact_log2q(778)
    assert 778 * int(cref.quanta(F32(1.0 + 2.0 ** -20), L)) < 2 ** 51 and 778 * 2 ** 44 > 2 ** 53
    for N, wmax, c in ((1, 1.0, 0.02), (778, 7.5, 0.02), (3000, 1.0, 3.0), (100000, 1000.0, 0.5)):
        L = cref.log2q(N, wmax, c, c)
        assert L == ops.surface_contact_log2q(N, wmax, c, c)
        M = max(wmax, 1.0) * max(c, 1.0)
        assert N * M * 2.0 ** -L <= 2.0 ** 50
    # every point of the hand on ONE face of the box: the sums of the restatement stay exact (frame_sums asserts the range)
    p, v, f = comparison_cases()["hand->box"]
    out = cref.loss_and_gradients(p[None], v[None], f[:1])
    assert (out["face"] == 0).all() and np.abs(out["grad_verts_attr"]).max() > 0
    touched = np.flatnonzero(np.abs(out["grad_verts_attr"][0]).sum(1) + np.abs(out["grad_verts_rep"][0]).sum(1))
    assert set(touched) <= set(f[0].tolist())


def test_sums_do_not_depend_on_the_order_of_the_points():
    p, v, f = comparison_cases()["hand->box"]
    a = cref.loss_and_gradients(p[None], v[None], f, searches=[restated("hand->box")])
    order = np.random.default_rng(1).permutation(len(p))
    b = cref.loss_and_gradients(p[order][None], v[None], f)
    for key in ("out", "grad_verts_attr", "grad_verts_rep"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    assert np.array_equal(a["grad_points"][0][order].view(np.uint32), b["grad_points"][0].view(np.uint32))


# =============================================================================================== fp32 against float64
@pytest.fixture(scope="module")
def floors():
    out = {}
    for name in MESH_CASES:
        p, v, f = comparison_cases()[name]
        s = restated(name)
        got = cref.loss_and_gradients(p[None], v[None], f, searches=[s])
        want = cref.reference64(p[None], v[None], f, s["face"][None], s["inside"][None], skip=(s["d2"] == 0)[None])
        verts = util.deviation(np.stack([got["grad_verts_attr"], got["grad_verts_rep"]]),
                               np.stack([want["grad_verts_attr"], want["grad_verts_rep"]]))
        out[name] = (max(util.deviation(got["value"], want["value"]), util.deviation(got["out"], want["out"])),
                     util.deviation(got["grad_points"], want["grad_points"]), verts)
    return out


@pytest.mark.parametrize("name", MESH_CASES)
def test_floors_of_the_fp32_restatement(name, floors):
    value, points, verts = floors[name]
    print(f"{name}: values {value:.3e}  point gradient {points:.3e}  vertex gradient {verts:.3e}")
    _pinned(value, E32[name][0])
    _pinned(points, E32[name][1])
    _pinned(verts, E32[name][2])


# =============================================================================================== arguments
def test_wrappers_check_their_arguments_before_any_device_work():
    from homan_amd import lossutils, ops
    faces = np.array([[0, 1, 2]], np.int32)
    for bad in (dict(B=0, N=4, V=3), dict(B=1, N=0, V=3), dict(B=1, N=4, V=-1)):
        with pytest.raises(ValueError):
            ops.SurfaceContactContext(faces=faces, device="cpu", **bad)
    for bad_faces in (np.zeros((0, 3), np.int32), np.zeros((2, 4), np.int32), np.zeros((2, 3), np.float32)):
        with pytest.raises(ValueError):
            ops.SurfaceContactContext(1, 4, 3, bad_faces, "cpu")
    with pytest.raises(ValueError):
        ops.surface_contact_loss(torch.zeros(1, 4, 3), torch.zeros(1, 3, 3), None)
    with pytest.raises(ValueError):
        ops.surface_contact_terms(torch.zeros(1, 4, 3), torch.zeros(1, 3, 3), "ctx")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError):
            ops._check_surface_thresholds(bad, 0.02)
        with pytest.raises(ValueError):
            ops._check_surface_thresholds(0.01, bad)
    with pytest.raises(ValueError):
        ops.surface_contact_log2q(0)
    with pytest.raises(ValueError):
        lossutils.surface_contact_contexts(1, 1, faces, faces, 3, "cpu", contact_zones="palm")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ops.SurfaceContactContext(1, 4, 3, faces, "cpu")


def test_context_checks_shapes_and_weights():
    """the checks of points, verts and weights against a context, on a stand-in that carries the context's sizes (no device)"""
    from homan_amd import ops
    ctx = object.__new__(ops.SurfaceContactContext)
    ctx.B, ctx.N, ctx.V, ctx.F, ctx.device, ctx._weights = 2, 4, 3, 1, torch.device("cpu"), (None, None, 1.0)
    good_p, good_v = torch.zeros(2, 4, 3), torch.zeros(2, 3, 3)
    ops._check_surface_inputs(good_p, good_v, ctx)
    for p, v in ((torch.zeros(1, 4, 3), good_v), (good_p, torch.zeros(2, 4, 3)), (good_p.int(), good_v), (good_p.numpy(), good_v),
                 (good_p, torch.zeros(2, 3))):
        with pytest.raises(ValueError):
            ops._check_surface_inputs(p, v, ctx)
    assert ctx.weights(None) == (None, 1.0)
    for w in (torch.zeros(3), torch.zeros(4, 1), torch.zeros(4, dtype=torch.int32), [1.0] * 4, torch.tensor([1.0, -1.0, 0.0, 0.0]),
              torch.tensor([1.0, float("inf"), 0.0, 0.0]), torch.tensor([1.0, float("nan"), 0.0, 0.0])):
        with pytest.raises(ValueError):
            ctx.weights(w)
    w, wmax = ctx.weights(torch.tensor([0.0, 2.5, 1.0, 0.0], dtype=torch.float64))
    assert w.dtype == torch.float32 and wmax == 2.5


def test_model_options_are_checked_on_the_host():
    import homan_amd
    rec, inputs, camintr, weights, meta = util.load_golden(util.golden_names()[0])
    kw = util.model_kwargs(inputs, camintr, meta)
    for bad in (dict(surface_contact_zones="palm"), dict(surface_contact_thresh=0.0), dict(surface_collision_thresh=float("inf"))):
        with pytest.raises(ValueError):
            homan_amd.HOMan(**kw, **bad)


def test_fused_steppers_refuse_the_term():
    """before anything is built, so without a device: the message names the mode that covers the term"""
    from homan_amd import jointopt
    from homan_amd.fused import FusedStepper
    for lw in ({"lw_surf_attr": 1.0}, {"lw_surf_rep": 0.5, "lw_surf_attr": 0.0}):
        with pytest.raises(NotImplementedError, match="mode='graph'"):
            FusedStepper(None, lw, 1e-2, 4)
        with pytest.raises(NotImplementedError, match="mode='graph'"):
            jointopt.ShardStepper([], lw, 1e-2, 4)


def test_weighted_total_takes_weight_sets_without_the_new_keys():
    from homan_amd.loopcommon import _weighted_total
    lw = {"lw_pca": 2.0, "lw_contact": 0.0}
    total = _weighted_total({"loss_pca": torch.tensor([3.0])}, lw)
    assert float(total) == 6.0
    lw = {"lw_pca": 2.0, "lw_surf_rep": 4.0}
    total = _weighted_total({"loss_pca": torch.tensor([3.0]), "loss_surf_rep": torch.tensor(0.5)}, lw)
    assert float(total) == 8.0 and tuple(total.shape) == (1,)
