"""Frame-loss terms, Adam and the log kernels at the shapes and edges the rest of the suite does not reach, through the raw C ABI:
csrc/losses.hip (k_v2d, k_smooth, k_priors, k_hand_terms, k_inter, k_inter_bwd, k_offscreen), csrc/adam.hip (k_adam, k_log,
k_log_total) and the two helpers at the end of csrc/geometry.hip (k_scale_by, k_sum_small).

References: tests/lossterms_ref.py (float64 torch + autograd; the interaction gate, the log total and Adam are bit-exact
restatements), checked against the float32 CPU oracle in tests/test_lossterms_refs.py, which also measures the float32 floors
E32_*.  Whatever is stated as identical, untouched or exact is torch.equal on the bits.  A comparison with a float64 reference
allows E32_FACTOR times the floor of its group (deviation = max |difference| / max |reference| per tensor, no element exempt) and
prints its figure first.  Every output buffer is filled with -7.0 and carries GUARD rows behind its last legitimate row; every
reduction runs twice on one workspace: the second run returns the first's bits and the ticket word of every clip's slice is 0
after each.
"""
import functools

import numpy as np
import pytest
import torch

from tests import lossterms_ref as lr
from tests import test_lossterms_refs as refs
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG = -1                    # HM_ERR_BAD_ARG of include/homan_amd.h
FACTOR = refs.E32_FACTOR
SENT, GUARD, PAD = -7.0, 2, 256
WS_FLOATS, TICKET = 576, 512    # HM_RED_WS_FLOATS, the ticket word's float offset (csrc/hm_common.h)
STRIDE = 5


def _hl():
    from homan_amd import lib as hl
    return hl


def _dev(x):
    if x is None:
        return None
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
    return t.to(DEV).contiguous()


def _guarded(rows, *shape):
    return torch.full((rows + GUARD, *shape), SENT, device=DEV)


def _untouched(t, rows=0):
    return bool((t[rows:] == SENT).all())


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ws(clips=1):
    """zero-filled reduce workspace of `clips` slices with a patterned pad behind it"""
    n = clips * _hl().lib().hm_reduce_workspace_bytes()
    assert n == clips * WS_FLOATS * 4
    t = torch.zeros(n + PAD, dtype=torch.uint8, device=DEV)
    t[n:] = 0xA5
    return t


def _ws_idle(ws):
    """pad untouched and every slice's ticket word back at 0"""
    words = ws[:-PAD].view(torch.int32).reshape(-1, WS_FLOATS)
    return bool((ws[-PAD:] == 0xA5).all()) and bool((words[:, TICKET] == 0).all())


def _twice(run, clips=1):
    """run(ws) -> (rc, dict of tensors) two times on ONE workspace: same bits, idle workspace after each -> the first's dict"""
    ws = _ws(clips)
    rc, a = run(ws)
    torch.cuda.synchronize()
    assert rc == 0 and _ws_idle(ws)
    rc, b = run(ws)
    torch.cuda.synchronize()
    assert rc == 0 and _ws_idle(ws)
    for k in a:
        assert _same(a[k], b[k]), k
    return a


def _within(tag, got, want, bar):
    """util.deviation(got, want) <= FACTOR * bar (a reference that is zero throughout allows nothing); prints the figure first"""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = want.detach().cpu().double().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    dev = util.deviation(got, want)
    print(f"{tag}: scale {np.abs(want).max():.3e} deviation {dev:.3e} (bar {FACTOR * bar:.1e})")
    assert np.isfinite(got).all(), tag
    assert dev <= (FACTOR * bar if np.abs(want).max() > 0 else 0.0), tag


# ===================================================================== A. v2d, smoothness, priors, hand terms
def _v2d(verts, K, nb, ref2d, ws, clip_len=0, stride=0):
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    N, V = verts.shape[:2]
    C = N // clip_len if clip_len else 1
    o = dict(unit=_guarded(N, V, 3), out=_guarded(C, max(stride, 2)))
    a = (P(verts), P(K), nb, P(ref2d), lr.IMAGE_SIZE, N, V, P(o["unit"]), P(o["out"]), P(ws))
    if clip_len == 0 and stride == 0:              # (the single-clip entry point)
        return L.hm_v2d_fwd(*a, hl.stream()), o
    return L.hm_v2d_fwd_clips(*a, clip_len, stride, hl.stream()), o


def _smooth(verts, nb, ws, clip_len=0, stride=0):
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    N, V = verts.shape[:2]
    C = N // clip_len if clip_len else 1
    o = dict(unit=_guarded(N, V, 3), out=_guarded(C, max(stride, 1)))
    a = (P(verts), N, V, nb, P(o["unit"]), P(o["out"]), P(ws))
    if clip_len == 0 and stride == 0:
        return L.hm_smooth_fwd(*a, hl.stream()), o
    return L.hm_smooth_fwd_clips(*a, clip_len, stride, hl.stream()), o


def _priors(sc, clips, stride=0):
    """sc = (pca (clips, npca), s_obj, m_obj, s_hand, m_hand) device tensors"""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    npca = sc[0].shape[1]
    o = dict(g_pca=_guarded(clips, npca), g_so=_guarded(clips), g_sh=_guarded(clips), out=_guarded(clips, max(stride, 3)))
    a = (P(sc[0]), npca, *[P(x) for x in sc[1:]], P(o["g_pca"]), P(o["g_so"]), P(o["g_sh"]), P(o["out"]))
    rc = L.hm_priors_fwd(*a, hl.stream()) if clips == 1 and stride == 0 else L.hm_priors_fwd_clips(*a, clips, stride, hl.stream())
    torch.cuda.synchronize()
    return rc, o


def _hand_terms(verts, K, nb, ref2d, sc, ws, clip_len=0, stride=0, s_obj=True):
    """sc: priors tuple (per-clip pca (C, npca), scales) or None (pca = NULL)"""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    N, V = verts.shape[:2]
    C = N // clip_len if clip_len else 1
    npca = sc[0].shape[1] if sc else 45
    o = dict(u_v2d=_guarded(N, V, 3), u_sm=_guarded(N, V, 3), v2d=_guarded(C, max(stride, 2)), sm=_guarded(C, max(stride, 1)),
             g_pca=_guarded(C, npca), g_so=_guarded(C), g_sh=_guarded(C), pri=_guarded(C, max(stride, 3)))
    pr = [P(x) for x in sc] if sc else [None] * 5
    if not s_obj:
        pr[1] = None
    rc = L.hm_hand_terms_fwd_clips(P(verts), P(K), nb, P(ref2d), lr.IMAGE_SIZE, N, V, P(o["u_v2d"]), P(o["v2d"]), P(o["u_sm"]),
                                   P(o["sm"]), pr[0], npca, *pr[1:], P(o["g_pca"]), P(o["g_so"]), P(o["g_sh"]), P(o["pri"]), P(ws),
                                   clip_len, stride, hl.stream())
    return rc, o


@functools.lru_cache(maxsize=None)
def _hand_case(name):
    """a case of lossterms_ref.hand_cases with its float64 references (computed once, shared, never modified)"""
    verts, K, ref2d, nb = lr.hand_cases()[name]
    return dict(verts=verts, K=K, ref2d=ref2d, nb=nb, v2d=lr.v2d_ref(verts, K, nb, ref2d, lr.IMAGE_SIZE), sm=lr.smooth_ref(verts, nb))


def _hand_pca(N, seed=1):
    """one clip's priors for a hand case of N frames: pca (1, N * 45) and the four scales, on the device"""
    return tuple(_dev(x) for x in lr.priors_scene(N * 45, 1, seed))


HAND_NAMES = [f"N{N}_V{V}_nb{nb}" for N, V, nb in lr.HAND_SHAPES]


@pytest.mark.parametrize("name", HAND_NAMES)
def test_v2d_and_smoothness_against_float64(name):
    """hm_v2d_fwd and hm_smooth_fwd: loss, pixel metric, smoothness value and every gradient element within the allowance of the
    float64 references - cameras general and distinct per frame, frame n under camera n // hand_nb."""
    c = _hand_case(name)
    verts, K, ref2d, nb = _dev(c["verts"]), _dev(c["K"]), _dev(c["ref2d"]), c["nb"]
    N = verts.shape[0]
    o = _twice(lambda ws: _v2d(verts, K, nb, ref2d, ws))
    loss, metric, grad = c["v2d"]
    _within(f"v2d {name} loss", o["out"][0, 0], loss, refs.E32_V2D_LOSS)
    _within(f"v2d {name} metric", o["out"][0, 1], metric, refs.E32_V2D_METRIC)
    _within(f"v2d {name} gradient", o["unit"][:N], grad, refs.E32_V2D_GRAD)
    assert _untouched(o["unit"], N) and _untouched(o["out"], 1)
    s = _twice(lambda ws: _smooth(verts, nb, ws))
    _within(f"smooth {name} value", s["out"][0, 0], c["sm"][0], refs.E32_SMOOTH)
    _within(f"smooth {name} gradient", s["unit"][:N], c["sm"][1], refs.E32_SMOOTH_GRAD)
    assert _untouched(s["unit"], N) and _untouched(s["out"], 1)
    if N <= nb:
        assert float(s["out"][0, 0]) == 0.0 and not s["unit"][:N].any()


@pytest.mark.parametrize("N,V,nb", lr.SMOOTH_ONLY)
def test_smoothness_without_a_pair_and_with_one(N, V, nb):
    """N = hand_nb: value exactly 0, gradient exactly 0.  N = hand_nb + 1: one pair (frames 0 and hand_nb); those two frames get
    exactly their one-sided gradient -/+ 2 d / count, the frames in between (no partner) exactly 0."""
    verts_c, _ = lr.smooth_only_cases()[f"N{N}_V{V}_nb{nb}"]
    verts = _dev(verts_c)
    s = _twice(lambda ws: _smooth(verts, nb, ws))
    val, grad = lr.smooth_ref(verts_c, nb)
    assert _untouched(s["unit"], N) and _untouched(s["out"], 1)
    if N == nb:
        assert float(s["out"][0, 0]) == 0.0 and bool((s["unit"][:N] == 0).all()) and float(val) == 0.0
        return
    _within(f"smooth N={N} hand_nb={nb} value", s["out"][0, 0], val, refs.E32_SMOOTH)
    _within(f"smooth N={N} hand_nb={nb} gradient", s["unit"][:N], grad, refs.E32_SMOOTH_GRAD)
    d = verts[nb] - verts[0]
    inv = torch.tensor(1.0, device=DEV) / float(V * 3)             # count = (N - hand_nb) V 3 = V 3, 1 / count rounded once
    one_sided = 2.0 * d * inv
    assert torch.equal(s["unit"][nb], one_sided) and torch.equal(s["unit"][0], 2.0 * (0.0 - d) * inv)
    assert bool((s["unit"][1:nb] == 0).all())


@pytest.mark.parametrize("npca", lr.PRIOR_NPCA)
def test_priors_clips_against_float64(npca):
    """hm_priors_fwd_clips, 3 clips with scales and means of their own, out_stride 5: values and gradients within the allowance,
    the other floats of the rows untouched; hm_priors_fwd on clip 1 alone returns that clip's bits."""
    sc_c = lr.priors_scene(npca, 3)
    sc = tuple(_dev(x) for x in sc_c)
    rc, o = _priors(sc, 3, STRIDE)
    assert rc == 0
    for c in range(3):
        vals, grads = lr.priors_ref(*[x[c] for x in sc_c])
        for k in range(3):
            _within(f"priors npca={npca} clip {c} value {k}", o["out"][c, k], vals[k], refs.E32_PCA)
        _within(f"priors npca={npca} clip {c} g_pca", o["g_pca"][c], grads[0], refs.E32_PCA_GRAD)
        _within(f"priors npca={npca} clip {c} g_sobj", o["g_so"][c], grads[1], refs.E32_PCA_GRAD)
        _within(f"priors npca={npca} clip {c} g_shand", o["g_sh"][c], grads[2], refs.E32_PCA_GRAD)
    assert bool((o["out"][:3, 3:] == SENT).all()) and all(_untouched(o[k], 3) for k in o)
    rc, one = _priors(tuple(x[1:2].contiguous() for x in sc), 1)
    assert rc == 0 and _same(one["out"][0, :3], o["out"][1, :3]) and _same(one["g_pca"][0], o["g_pca"][1])
    assert _same(one["g_so"][:1], o["g_so"][1:2]) and _same(one["g_sh"][:1], o["g_sh"][1:2]) and all(_untouched(one[k], 1) for k in one)


@pytest.mark.parametrize("nb", [1, 2])
def test_clip_batches_equal_single_clip_calls(nb):
    """3 clips of 4 frames, out_stride 5: hm_v2d_fwd_clips, hm_smooth_fwd_clips and hm_hand_terms_fwd_clips return for each clip,
    bit for bit, what a single-clip call on that clip's slice with that clip's cameras returns; the rows' other floats stay
    untouched; and each clip is within the allowance of ITS float64 reference (no smoothness pair crosses a clip boundary, no
    clip reads another's cameras)."""
    C, CL = lr.CLIP_C, lr.CLIP_LEN
    batch = lr.clip_batch(nb)
    verts, K, ref2d = (_dev(x) for x in batch)
    sc_c = lr.priors_scene(CL * 45, C, seed=2)
    sc = tuple(_dev(x) for x in sc_c)
    v = _twice(lambda ws: _v2d(verts, K, nb, ref2d, ws, CL, STRIDE), C)
    s = _twice(lambda ws: _smooth(verts, nb, ws, CL, STRIDE), C)
    h = _twice(lambda ws: _hand_terms(verts, K, nb, ref2d, sc, ws, CL, STRIDE), C)
    assert bool((v["out"][:C, 2:] == SENT).all()) and bool((s["out"][:C, 1:] == SENT).all())
    assert bool((h["v2d"][:C, 2:] == SENT).all()) and bool((h["sm"][:C, 1:] == SENT).all()) and bool((h["pri"][:C, 3:] == SENT).all())
    assert all(_untouched(x[k], C * CL if k.startswith("u") else C) for x in (v, s, h) for k in x)
    assert _same(h["u_v2d"], v["unit"]) and _same(h["u_sm"], s["unit"])
    for c in range(C):
        case = _hand_case(f"clip{c}_nb{nb}")
        cv, cK, cr = (_dev(x) for x in lr.clip_slice(batch, nb, c))
        v1 = _twice(lambda ws: _v2d(cv, cK, nb, cr, ws))
        s1 = _twice(lambda ws: _smooth(cv, nb, ws))
        rows = slice(c * CL, (c + 1) * CL)
        assert _same(v1["out"][0, :2], v["out"][c, :2]) and _same(v1["unit"][:CL], v["unit"][rows]), c
        assert _same(s1["out"][0, :1], s["out"][c, :1]) and _same(s1["unit"][:CL], s["unit"][rows]), c
        h1 = _twice(lambda ws: _hand_terms(cv, cK, nb, cr, tuple(x[c:c + 1].contiguous() for x in sc), ws))
        for k, n in (("v2d", 2), ("sm", 1), ("pri", 3)):
            assert _same(h1[k][0, :n], h[k][c, :n]), (k, c)
        assert _same(h1["u_v2d"][:CL], h["u_v2d"][rows]) and _same(h1["u_sm"][:CL], h["u_sm"][rows]) and _same(h1["g_pca"][0], h["g_pca"][c])
        assert _same(h1["g_so"][:1], h["g_so"][c:c + 1]) and _same(h1["g_sh"][:1], h["g_sh"][c:c + 1]), c
        loss, metric, grad = case["v2d"]
        for tag, o_v2d, o_sm in (("clips", v["out"][c], s["out"][c]), ("hand terms", h["v2d"][c], h["sm"][c])):
            _within(f"{tag} nb={nb} clip {c} v2d loss", o_v2d[0], loss, refs.E32_V2D_LOSS)
            _within(f"{tag} nb={nb} clip {c} v2d metric", o_v2d[1], metric, refs.E32_V2D_METRIC)
            _within(f"{tag} nb={nb} clip {c} smoothness", o_sm[0], case["sm"][0], refs.E32_SMOOTH)
        _within(f"clips nb={nb} clip {c} v2d gradient", v["unit"][rows], grad, refs.E32_V2D_GRAD)
        _within(f"clips nb={nb} clip {c} smoothness gradient", s["unit"][rows], case["sm"][1], refs.E32_SMOOTH_GRAD)
        vals, grads = lr.priors_ref(*[x[c] for x in sc_c])
        for k in range(3):
            _within(f"hand terms nb={nb} clip {c} prior {k}", h["pri"][c, k], vals[k], refs.E32_PCA)
        _within(f"hand terms nb={nb} clip {c} g_pca", h["g_pca"][c], grads[0], refs.E32_PCA_GRAD)
        _within(f"hand terms nb={nb} clip {c} g_sobj", h["g_so"][c], grads[1], refs.E32_PCA_GRAD)
        _within(f"hand terms nb={nb} clip {c} g_shand", h["g_sh"][c], grads[2], refs.E32_PCA_GRAD)


@pytest.mark.parametrize("name", HAND_NAMES)
def test_hand_terms_launch_against_its_entry_points_and_float64(name):
    """hm_hand_terms_fwd_clips: unit gradients, prior gradients and the three prior values are the bits of hm_v2d_fwd,
    hm_smooth_fwd and hm_priors_fwd (the same per-element arithmetic); the three summed outputs (other block counts, another
    order) are within the allowance of float64; with pca = NULL the prior outputs and gradients stay untouched."""
    c = _hand_case(name)
    verts, K, ref2d, nb = _dev(c["verts"]), _dev(c["K"]), _dev(c["ref2d"]), c["nb"]
    N = verts.shape[0]
    sc = _hand_pca(N)
    h = _twice(lambda ws: _hand_terms(verts, K, nb, ref2d, sc, ws))
    v = _twice(lambda ws: _v2d(verts, K, nb, ref2d, ws))
    s = _twice(lambda ws: _smooth(verts, nb, ws))
    rc, p = _priors(sc, 1)
    assert rc == 0
    assert _same(h["u_v2d"], v["unit"]) and _same(h["u_sm"], s["unit"])
    assert _same(h["g_pca"], p["g_pca"]) and _same(h["g_so"], p["g_so"]) and _same(h["g_sh"], p["g_sh"]) and _same(h["pri"], p["out"])
    loss, metric, _ = c["v2d"]
    _within(f"hand terms {name} v2d loss", h["v2d"][0, 0], loss, refs.E32_V2D_LOSS)
    _within(f"hand terms {name} v2d metric", h["v2d"][0, 1], metric, refs.E32_V2D_METRIC)
    _within(f"hand terms {name} smoothness", h["sm"][0, 0], c["sm"][0], refs.E32_SMOOTH)
    assert _untouched(h["v2d"], 1) and _untouched(h["sm"], 1) and _untouched(h["pri"], 1)
    n = _twice(lambda ws: _hand_terms(verts, K, nb, ref2d, None, ws))
    assert all(_untouched(n[k]) for k in ("g_pca", "g_so", "g_sh", "pri"))
    assert all(_same(n[k], h[k]) for k in ("u_v2d", "u_sm", "v2d", "sm"))


def test_hand_term_entry_points_refuse_bad_arguments():
    """hand_nb = 0, a clip_len that does not divide N, pca without s_obj: HM_ERR_BAD_ARG before any launch, outputs untouched"""
    verts, K, ref2d = (_dev(x) for x in lr.clip_batch(1))
    sc = tuple(_dev(x) for x in lr.priors_scene(lr.CLIP_LEN * 45, lr.CLIP_C, seed=2))
    ws = _ws(lr.CLIP_C)
    calls = [_v2d(verts, K, 0, ref2d, ws), _smooth(verts, 0, ws), _hand_terms(verts, K, 0, ref2d, sc, ws, lr.CLIP_LEN, STRIDE),
             _v2d(verts, K, 1, ref2d, ws, 5, STRIDE), _smooth(verts, 1, ws, 5, STRIDE), _hand_terms(verts, K, 1, ref2d, sc, ws, 5, STRIDE),
             _hand_terms(verts, K, 1, ref2d, sc, ws, lr.CLIP_LEN, STRIDE, s_obj=False)]
    torch.cuda.synchronize()
    for i, (rc, o) in enumerate(calls):
        assert rc == BAD_ARG, i
        assert all(_untouched(t) for t in o.values()), i
    assert _ws_idle(ws) and not ws[:-PAD].any()


# ===================================================================== B. coarse interaction
def _inter(vh, vo, K, e, zt, ws, clip_len=0, stride=0):
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    B, Vh, Vo = vh.shape[0], vh.shape[1], vo.shape[1]
    C = B // clip_len if clip_len else 1
    o = dict(rec=_guarded(B, 8), out=_guarded(C, max(stride, 1)))
    a = (P(vh), P(vo), P(K), B, Vh, Vo, e, zt, P(o["rec"]), P(o["out"]), P(ws))
    if clip_len == 0 and stride == 0:
        return L.hm_inter_fwd(*a, hl.stream()), o
    return L.hm_inter_fwd_clips(*a, clip_len, stride, hl.stream()), o


def _inter_bwd(rec, up, B, Vh, Vo, hand=True, obj=True):
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    o = dict(g_hand=_guarded(B, Vh, 3), g_obj=_guarded(B, Vo, 3))
    rc = L.hm_inter_bwd(P(rec), P(torch.tensor([up], device=DEV)), B, Vh, Vo, P(o["g_hand"]) if hand else None,
                        P(o["g_obj"]) if obj else None, hl.stream())
    torch.cuda.synchronize()
    return rc, o


@functools.lru_cache(maxsize=None)
def _inter_case(name):
    h, o, K, e, zt, cl = lr.inter_cases()[name]
    return dict(vh=h, vo=o, K=K, e=e, zt=zt, cl=cl, ref={up: lr.inter_ref(h, o, K, e, zt, cl, up) for up in lr.INTER_UPSTREAMS})


@pytest.mark.parametrize("name", list(lr.inter_cases()))
def test_interaction_against_the_gate_and_float64(name):
    """hm_inter_fwd_clips + hm_inter_bwd on every case of lossterms_ref.inter_cases (the exact gate scenes; meshes from 1 to 1500
    vertices, whole waves without a vertex; 300 frames in one clip; 3 clips of 4 with out_stride 5): the flags are the float32
    gate's exactly, the record's vector is exactly 0 where the flag is, a clip of gated-off frames sums to exactly 0; MSE, sums
    and both gradients (upstream 1, -2.5, 0) within the allowance; record pads, guard rows, other floats of the rows untouched."""
    c = _inter_case(name)
    vh, vo, K = _dev(c["vh"]), _dev(c["vo"]), _dev(c["K"])
    B, Vh, Vo = vh.shape[0], vh.shape[1], vo.shape[1]
    cl = c["cl"] or 0
    C = B // cl if cl else 1
    stride = STRIDE if cl else 0
    o = _twice(lambda ws: _inter(vh, vo, K, c["e"], c["zt"], ws, cl, stride), C)
    r = c["ref"][1.0]
    rec = o["rec"][:B]
    flags = rec[:, 0].cpu().numpy()
    print(f"inter {name}: {int(flags.sum())} of {B} frames interact (reference {int(r['flag'].sum())})")
    assert np.array_equal(flags, r["flag"].astype(np.float32))
    off = torch.from_numpy(r["flag"] == 0).to(DEV)
    assert bool((rec[off][:, 2:5] == 0).all())
    assert bool((rec[:, 5:] == SENT).all()) and _untouched(o["rec"], B) and _untouched(o["out"], C) and bool((o["out"][:C, 1:] == SENT).all())
    _within(f"inter {name} mse", rec[:, 1], r["mse"], refs.E32_INTER_SUM)
    _within(f"inter {name} record vector", rec[:, 2:5], r["gvec"], refs.E32_INTER_GRAD)
    _within(f"inter {name} sum", o["out"][:C, 0], r["total"], refs.E32_INTER_SUM)
    per_clip = r["flag"].reshape(C, -1).sum(1)
    for k in np.nonzero(per_clip == 0)[0]:
        assert float(o["out"][k, 0]) == 0.0, k
    if name.startswith("gate"):
        assert per_clip[0] == 0 and per_clip[1:].all()
    for up in lr.INTER_UPSTREAMS:
        rc, g = _inter_bwd(rec, up, B, Vh, Vo)
        assert rc == 0 and _untouched(g["g_hand"], B) and _untouched(g["g_obj"], B)
        _within(f"inter {name} upstream {up} g_hand", g["g_hand"][:B], c["ref"][up]["g_hand"], refs.E32_INTER_GRAD)
        _within(f"inter {name} upstream {up} g_obj", g["g_obj"][:B], c["ref"][up]["g_obj"], refs.E32_INTER_GRAD)


@pytest.mark.parametrize("name", ["Vh778_Vo1500", "Vh1500_Vo778"])
def test_interaction_backward_with_one_output(name):
    """hm_inter_bwd with g_hand NULL, with g_obj NULL (the given output holds the two-output call's bits, the other stays
    untouched), with both NULL (refused), for Vo > Vh and Vo < Vh"""
    c = _inter_case(name)
    vh, vo, K = _dev(c["vh"]), _dev(c["vo"]), _dev(c["K"])
    B, Vh, Vo = vh.shape[0], vh.shape[1], vo.shape[1]
    rec = _twice(lambda ws: _inter(vh, vo, K, c["e"], c["zt"], ws))["rec"]
    for up in lr.INTER_UPSTREAMS:
        rc, both = _inter_bwd(rec, up, B, Vh, Vo)
        rc_h, only_h = _inter_bwd(rec, up, B, Vh, Vo, obj=False)
        rc_o, only_o = _inter_bwd(rec, up, B, Vh, Vo, hand=False)
        rc_n, none = _inter_bwd(rec, up, B, Vh, Vo, hand=False, obj=False)
        assert (rc, rc_h, rc_o, rc_n) == (0, 0, 0, BAD_ARG)
        assert _same(only_h["g_hand"], both["g_hand"]) and _untouched(only_h["g_obj"])
        assert _same(only_o["g_obj"], both["g_obj"]) and _untouched(only_o["g_hand"])
        assert _untouched(none["g_hand"]) and _untouched(none["g_obj"])
        assert _untouched(both["g_hand"], B) and _untouched(both["g_obj"], B)


# ===================================================================== C. off-screen penalty
def _offscreen(verts, K, w):
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    N, V = verts.shape[:2]
    o = dict(out=_guarded(N), grad=_guarded(N, V, 3))
    rc = L.hm_offscreen_fwd(P(verts), P(K), N, V, lr.ZFAR, w, P(o["out"]), P(o["grad"]), hl.stream())
    torch.cuda.synchronize()
    assert rc == 0 and _untouched(o["out"], N) and _untouched(o["grad"], N)
    return o["out"][:N], o["grad"][:N]


@pytest.mark.parametrize("name", list(lr.offscreen_cases()))
def test_offscreen_against_float64(name):
    """hm_offscreen_fwd on random clouds straddling all six planes (V from 1 to 1000, weights 1 and 0.37), on the exact scene and
    on each of its vertices alone: value and gradient within the allowance; a candidate's value and gradient do not depend on
    the other candidates (bit for bit); a vertex on a plane, a step inside, at z = 0+ or at z = zfar contributes exactly
    nothing; a vertex a step outside contributes what float64 says, with its sign."""
    verts_c, K_c, w = lr.offscreen_cases()[name]
    verts, K = _dev(verts_c), _dev(K_c)
    out, grad = _offscreen(verts, K, w)
    want, gwant = lr.offscreen_ref(verts_c, K_c, lr.ZFAR, w)
    hinge = name.startswith("hinge")
    # (the loose floor belongs to the four vertices a step beyond an NDC plane alone: the depth cases have no 1e-9 in them)
    _within(f"offscreen {name} value", out, want, refs.E32_OFFSCREEN_HINGE if name.endswith("outside") else refs.E32_OFFSCREEN)
    _within(f"offscreen {name} gradient", grad, gwant, refs.E32_OFFSCREEN_GRAD)
    if hinge:
        if name.endswith(("on", "inside")) or name in ("hinge_z0+", "hinge_zfar"):
            assert float(out[0]) == 0.0 and bool((grad == 0).all()) and float(want[0]) == 0.0
        else:
            assert float(out[0]) > 0.0 and bool(grad.any())
    if name.startswith("exact"):
        _, names = lr.offscreen_exact_scene()
        for i, n in enumerate(names):
            if n.endswith(("on", "inside")) or n in ("z0+", "zfar"):
                assert bool((grad[0, i] == 0).all()), n
            else:
                assert bool(grad[0, i].any()), n
    if name.startswith("cloud"):
        assert float(want.min()) > 0 or verts.shape[1] == 1
        for n in range(verts.shape[0]):
            o1, g1 = _offscreen(verts[n:n + 1].contiguous(), K, w)
            assert _same(o1, out[n:n + 1]) and _same(g1, grad[n:n + 1]), n


# ===================================================================== D. Adam and the log kernels
ADAM_SIZES = (1, 255, 256, 257, 3000, 16384, 16385)         # 16 385 > 64 blocks x 256 threads: the stride loop runs
ADAM_LRS = (1e-2, 1e-1, 1e-3)
ADAM_STEPS = 12


def _hm_adam(params_c, lrs, t0=0):
    from homan_amd.loopcommon import HmAdam
    ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in params_c]
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt = HmAdam([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)])
    opt.step_t[0] = t0
    return ps, opt


def _np_same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


@pytest.mark.parametrize("t0", [0, 999])
def test_adam_equals_the_oracle_bit_for_bit(t0):
    """HmAdam (k_adam) against oracle.adam.Adam: parameters, m and v after every one of 12 steps, seven tensors from 1 to 16 385
    elements in one launch (grid capped at 64 blocks), three learning rates, gradients with exact zeros, 1e-20 and 1e+15, one
    tensor with an all-zero gradient throughout (it must not move), the step counter preset to 0 and to 999; the counter grows
    by exactly one per launch, its ticket word is 0, and zero_grad zeroes the gradients or leaves their bits."""
    lrs = [ADAM_LRS[i % 3] for i in range(len(ADAM_SIZES))]
    params_c, grads_c = lr.adam_inputs(ADAM_SIZES, ADAM_STEPS)
    want = lr.adam_oracle_run(params_c, grads_c, lrs, t0)
    ps, opt = _hm_adam(params_c, lrs, t0)
    assert opt.blocks == 64 and len(opt.items) == len(ADAM_SIZES)
    for t in range(ADAM_STEPS):
        for p, g in zip(ps, grads_c[t]):
            p.grad.copy_(g)
        zero = t % 2 == 0
        opt.step(zero_grad=zero)
        torch.cuda.synchronize()
        assert opt.step_t.tolist() == [t0 + t + 1, 0], t
        for k, (p, (m, v)) in enumerate(zip(ps, opt.state)):
            for tag, got, ref in (("p", p, want[t][k][0]), ("m", m, want[t][k][1]), ("v", v, want[t][k][2])):
                assert _np_same(got.detach().cpu().numpy(), ref), (t, ADAM_SIZES[k], tag)
            if zero:
                assert bool((p.grad == 0).all()), (t, k)
            else:
                assert _same(p.grad, grads_c[t][k].to(DEV)), (t, k)
    assert _np_same(ps[1].detach().cpu().numpy(), params_c[1].numpy())            # all-zero gradient: 0 / eps, never moved
    assert any(not _np_same(p.detach().cpu().numpy(), q.numpy()) for p, q in zip(ps, params_c))


def _log_want(vals_c, w_c, n):
    tot = np.array([lr.log_total_ref(vals_c[c, :n].numpy(), w_c.numpy()) for c in range(vals_c.shape[0])], np.float32)
    row = vals_c.numpy().copy()
    row[:, n] = tot
    return row


@pytest.mark.parametrize("n", [1, 13])
@pytest.mark.parametrize("nclips", [1, 3, 70])
def test_log_total_and_adam_log_row(nclips, n):
    """hm_log_total_clips and the log row of hm_adam_step_log (64 blocks: 70 clips are more than one per log block) against
    log_total_ref, bit for bit: a zero weight skips its NaN value, the row lands at the step being taken, the rest of the log
    stays untouched; with the counter at max_steps or beyond no row is written and the totals still are.  The Adam half of
    the fused launch still equals the oracle."""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    vals_c, w_c = lr.log_scene(nclips, n)
    want = _log_want(vals_c, w_c, n)
    assert np.isfinite(want[:, n]).all() and (n == 1 or np.isnan(want[:, n // 2]).all()) and want[:, n].any()
    max_steps = 4
    params_c, grads_c = lr.adam_inputs((16385, 7), 1, seed=4)
    for s in (0, 2, 3, 4, 9):
        for fused in (False, True):
            vals, w, log = _dev(vals_c.clone()), _dev(w_c), _guarded(max_steps, nclips, n + 1)
            if fused:
                ps, opt = _hm_adam(params_c, ADAM_LRS[:2], s)
                assert opt.blocks == 64
                for p, g in zip(ps, grads_c[0]):
                    p.grad.copy_(g)
                opt.step(zero_grad=False, log=(vals, w, n, max_steps, log, nclips))
                torch.cuda.synchronize()
                ref = lr.adam_oracle_run(params_c, grads_c, ADAM_LRS[:2], s)[0]
                assert opt.step_t.tolist() == [s + 1, 0]
                assert all(_np_same(p.detach().cpu().numpy(), r[0]) for p, r in zip(ps, ref))
            else:
                step = torch.tensor([s, 0], dtype=torch.int32, device=DEV)
                assert L.hm_log_total_clips(P(vals), P(w), n, P(step), max_steps, P(log), nclips, hl.stream()) == 0
                torch.cuda.synchronize()
                assert step.tolist() == [s, 0]
            assert _np_same(vals.cpu().numpy(), want), (s, fused)
            lg = log.cpu().numpy()
            for row in range(max_steps + GUARD):
                if row == s and s < max_steps:
                    assert _np_same(lg[row], want), (s, fused, row)
                else:
                    assert (lg[row] == SENT).all(), (s, fused, row)


@pytest.mark.parametrize("n", [1, 13, 65])
def test_log_scalars(n):
    """hm_log_scalars: row step[0] of the log = src (plain indexing), every other float untouched; at max_steps or beyond nothing
    is written"""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    src = _dev(np.random.default_rng(n).normal(size=n).astype(np.float32))
    max_steps = 3
    for s in (0, 2, 3, 7):
        log = _guarded(max_steps, n)
        step = torch.tensor([s, 0], dtype=torch.int32, device=DEV)
        assert L.hm_log_scalars(P(src), n, P(step), max_steps, P(log), hl.stream()) == 0
        torch.cuda.synchronize()
        for row in range(max_steps + GUARD):
            if row == s and s < max_steps:
                assert _same(log[row], src), (s, row)
            else:
                assert bool((log[row] == SENT).all()), (s, row)
        assert step.tolist() == [s, 0]


# ===================================================================== E. hm_scale_by and hm_sum_small_clips
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100000])
def test_scale_by(n):
    """out = s[0] * in: the float32 product's bits for s = 0, -1.5 and 1e-30; guard rows untouched"""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    x_c = torch.from_numpy(np.random.default_rng(n).normal(size=n).astype(np.float32))
    x = _dev(x_c)
    for s in (0.0, -1.5, 1e-30):
        out = _guarded(n)
        sc = torch.tensor([s], dtype=torch.float32)
        assert L.hm_scale_by(P(x), P(sc.to(DEV)), n, P(out), hl.stream()) == 0
        torch.cuda.synchronize()
        want = (sc.numpy()[0] * x_c.numpy()).astype(np.float32)
        assert want.dtype == np.float32 and _np_same(out[:n].cpu().numpy(), want), s
        assert _untouched(out, n)


@pytest.mark.parametrize("n", lr.SUM_SMALL_N)
def test_sum_small_clips(n):
    """hm_sum_small_clips, 3 clips, extra NULL and given: exact on exactly summable data, within the allowance on random data"""
    hl = _hl()
    L, P = hl.lib(), hl.ptr
    w0, w1 = lr.SUM_SMALL_W
    for exact in (True, False):
        parts_c, extra_c = lr.sum_small_scene(n, 3, exact)
        parts, extra = _dev(parts_c), _dev(extra_c)
        for ex_c, ex in ((None, None), (extra_c, extra)):
            out = _guarded(3)
            assert L.hm_sum_small_clips(P(parts), n, w0, P(ex), w1, P(out), 3, hl.stream()) == 0
            torch.cuda.synchronize()
            want = lr.sum_small_ref(parts_c, w0, ex_c, w1)
            assert _untouched(out, 3)
            if exact:
                assert torch.equal(out[:3].cpu().double(), want), (n, ex is not None)
            else:
                _within(f"sum_small n={n} extra={'yes' if ex is not None else 'no'}", out[:3], want, refs.E32_SUM_SMALL)
