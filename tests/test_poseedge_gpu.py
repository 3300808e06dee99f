"""The edge-chamfer term of the object-pose initialisation in the fused loop (csrc/poseedge.hip: hm_edge_edt,
hm_pose_edge_terms; homan_amd.pose_optimization._FusedPoseLoop with lw_chamfer != 0, PoseFitter, find_optimal_pose(s)).

Every figure a test compares is printed before it is asserted."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy.ndimage import distance_transform_edt

from tests import util

GOLD = os.path.join(util.GOLDEN_DIR, "ref_poseinit_cube_n6_s64.npz")
FUSED_STEP_KERNEL_NODES = 10         # kernel nodes of one captured step at lw_chamfer = 0, counted on the parent commit
EDGE_STEP_KERNEL_NODES = 11          # ... of the step with the term: hm_pose_edge_terms for hm_sil_reduce, mode 3's mask pass
EDGE_REL = 1e-5                     # chamfer sum and gradient samples: of the sum of the magnitudes of their addends
MAX_LOOP_SIZE = 1024                 # largest mask the loop accepts: the edge sweeps take S <= 512 pixels of 2 x 2 samples


def _load():
    z = np.load(GOLD, allow_pickle=False)
    return {k: z[k] for k in z.files}


def _scene():
    rec = _load()
    return dict(rec=rec, n=int(rec["meta_n"]), size=int(rec["meta_size"]), verts=torch.from_numpy(rec["in_vertices"]),
                faces=torch.from_numpy(rec["in_faces"]), rots=torch.from_numpy(rec["in_rotations_init"]),
                trans0=torch.from_numpy(rec["init_translations"]).clone(), K=torch.from_numpy(rec["init_camintr_roi"]))


def _band(ref, k):
    """maxpool_k(ref) - ref > 0 on the CPU (reference pose_optimization.py:84-85)"""
    t = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32))[None, None]
    return (torch.nn.functional.max_pool2d(t, k, 1, k // 2)[0, 0] - t[0, 0] > 0).numpy()


def _edge_edt(ref, k, power, stride=None):
    """hm_edge_edt on the (size, size) 0 / 1 image `ref`, held with `stride` floats per row -> (buffer (stride, stride), count)"""
    from homan_amd import lib as hlib
    size = ref.shape[0]
    stride = stride or size
    buf = torch.zeros(stride, stride)
    buf[:size, :size] = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32))
    buf = buf.cuda()
    out = torch.full((stride, stride), -7.0, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hlib.check(hlib.lib().hm_edge_edt(hlib.ptr(buf), size, stride, k, power, hlib.ptr(out), hlib.ptr(count), hlib.stream()),
               "hm_edge_edt")
    return out.cpu().numpy(), int(count.item())


def _masks(size, rng):
    """target masks in the -1 / 0 / 1 convention: random blobs, one foreground sample, a target on the border, occluded regions"""
    y, x = np.mgrid[:size, :size]
    blobs = np.zeros((size, size), np.float32)
    for _ in range(5):
        cy, cx, ry, rx = rng.uniform(0, size, 2).tolist() + rng.uniform(size / 16, size / 4, 2).tolist()
        blobs[((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1] = 1
    single = np.zeros((size, size), np.float32)
    single[size // 3, size // 2 + 1] = 1
    border = np.zeros((size, size), np.float32)
    border[: size // 3, size // 2:] = 1
    border[-1, :5] = 1
    occluded = blobs.copy()
    occluded[size // 2:, : size // 3] = -1
    occluded[: size // 8] = -1
    return {"blobs": blobs, "single": single, "border": border, "occluded": occluded}


@pytest.mark.gpu
def test_edge_edt_equals_the_references_own_output():
    """hm_edge_edt on the golden's mask against `edt_ref_edge` as the reference computed it (scipy on the host, float64,
    ** (2 * power), float32).  The bar is the oracle test's rtol 1e-6; the values are in fact equal."""
    rec = _load()
    ref = (rec["in_mask"] > 0).astype(np.float32)
    out, count = _edge_edt(ref, 7, 0.25)
    print("band samples", count, "max |diff|", np.abs(out - rec["edt_ref_edge"]).max(), "equal", np.array_equal(out, rec["edt_ref_edge"]))
    assert count == int(_band(ref, 7).sum())
    np.testing.assert_allclose(out, rec["edt_ref_edge"], rtol=1e-6)
    assert np.array_equal(out, rec["edt_ref_edge"])


@pytest.mark.gpu
@pytest.mark.parametrize("size", [64, 100, 256, MAX_LOOP_SIZE])
def test_edge_edt_is_the_exact_squared_distance(size):
    """The transform is integer arithmetic: with power 1 the output IS d2 = the squared Euclidean distance to the nearest sample of
    the edge band, equal to rint(scipy_edt(~band) ** 2) at every sample; with power 0.5 it is float32(sqrt(float64(d2))), the
    correctly rounded distance.  (The entry point returns d2 ** power, as the reference's `edt ** (power * 2)` does; the exponent
    at which the output is d2 itself is therefore 1, not 0.5.)  Masks without a band - empty, full - give count 0 and zeros.  A
    row stride larger than the size (the loop's padded copies) leaves everything outside the image untouched."""
    rng = np.random.default_rng(size)
    for name, mask in _masks(size, rng).items():
        ref = (mask > 0).astype(np.float32)
        for k in (3, 5, 7):
            band = _band(ref, k)
            want = np.rint(distance_transform_edt(~band) ** 2).astype(np.int64)
            stride = size if size % 64 == 0 else (size + 63) // 64 * 64
            d2, count = _edge_edt(ref, k, 1.0, stride)
            dist, _ = _edge_edt(ref, k, 0.5, stride)
            bad = int((d2[:size, :size] != want).sum())
            print(size, name, k, "band", count, "samples off", bad, "max d2", int(want.max()))
            assert count == int(band.sum()) and count > 0
            assert np.array_equal(d2[:size, :size], want.astype(np.float32))
            assert np.array_equal(dist[:size, :size], np.sqrt(want.astype(np.float64)).astype(np.float32))
            assert (d2[size:] == -7.0).all() and (d2[:, size:] == -7.0).all()
    for fill in (0.0, 1.0):
        out, count = _edge_edt(np.full((size, size), fill, np.float32), 7, 0.25)
        assert count == 0 and not out.any()


def _edge_terms(alpha, keep, ref, edt, k, lw):
    """hm_pose_edge_terms on (n, size, size) `alpha` and (size, size) keep / ref / edt, all padded to the 64-sample grid ->
    (terms (n,4), grad (n, stride, stride)) as numpy"""
    from homan_amd import lib as hlib
    L, P = hlib.lib(), hlib.ptr
    n, size = alpha.shape[0], alpha.shape[1]
    stride = (size + 63) // 64 * 64
    pad = lambda t, v=0.0: torch.nn.functional.pad(torch.as_tensor(t).float(), (0, stride - size, 0, stride - size), value=v).contiguous().cuda()
    a, kp, rf, ed = pad(alpha, 1.0), pad(keep, 1.0), pad(ref, 1.0), pad(edt, 5.0)       # (padding the kernel must not look at)
    terms, grad = torch.full((n, 4), -7.0, device="cuda"), torch.full((n, stride, stride), -7.0, device="cuda")
    ws = torch.zeros(L.hm_pose_edge_workspace_bytes(n, stride), dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        hlib.check(L.hm_pose_edge_terms(P(a), P(kp), P(rf), P(ed), n, size, stride, k, lw, P(terms), P(grad), P(ws), hlib.stream()),
                   "hm_pose_edge_terms")
        outs.append((terms.cpu().numpy().copy(), grad.cpu().numpy().copy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])       # two calls: the same bits
    return outs[0]


def _edge_case_images(size, rng):
    y, x = np.mgrid[:size, :size]
    zero, one = np.zeros((size, size)), np.ones((size, size))
    frame = ((y == 0) | (x == 0) | (y == size - 1) | (x == size - 1)).astype(np.float64)         # every border and corner
    corners = np.zeros((size, size))
    for cy in (0, size - 1):
        for cx in (0, size - 1):
            corners[cy, cx] = 1
    corners[size // 2 - 4: size // 2 + 5, size // 3: size // 3 + 9] = 1                            # a block: ties in every window on it
    dense, sparse = (rng.random((size, size)) < 0.5).astype(np.float64), (rng.random((size, size)) < 0.02).astype(np.float64)
    stripes = ((x // 3 + y // 5) % 2).astype(np.float64)
    alpha = np.stack([zero, one, frame, corners, dense, sparse, stripes])
    keep = np.ones((size, size))
    keep[size // 4: size // 4 + 6] = 0                                                            # an occluded band and holes
    keep[rng.random((size, size)) < 0.03] = 0
    ref = (((y - size * 0.45) / (size * 0.3)) ** 2 + ((x - size * 0.55) / (size * 0.25)) ** 2 <= 1).astype(np.float64)
    return alpha, keep, ref


def _torch_edge_terms(alpha, keep, ref, edt, k, lw, device, dtype):
    """lw * sum (pool(img) - img) * edt + sum (img - ref)^2 through torch autograd -> (mask, chamfer sum, d / d alpha, the sum of
    the magnitudes of each gradient sample's addends, of each chamfer sum's addends)"""
    to = lambda t: torch.as_tensor(t, dtype=dtype, device=device)
    a, kp, rf, ed = to(alpha).requires_grad_(True), to(keep), to(ref), to(edt)
    pool = torch.nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)
    img = kp * a
    img.retain_grad()
    mask = ((img - rf) ** 2).sum((1, 2))
    edges = pool(img) - img
    cham = (edges * ed).sum((1, 2))
    (lw * cham + mask).sum().backward(retain_graph=True)
    g_total = a.grad.clone()
    g_cham = torch.autograd.grad(cham.sum(), img)[0]                 # sum over the windows that name p of edt[q], minus edt[p]
    mag = kp * (2 * (img - rf).abs() + lw * (g_cham + 2 * ed))
    return (mask.detach().cpu().numpy(), cham.detach().cpu().numpy(), g_total.cpu().numpy(), mag.detach().cpu().numpy(),
            (edges * ed).abs().sum((1, 2)).detach().cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("size", [64, 100, 96, 256])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_edge_terms_against_torch_autograd(size, k):
    """hm_pose_edge_terms against float64 CPU autograd of lw * sum (pool(img) - img) * edt + sum (img - ref)^2, img = keep * alpha, on
    binary images with ties, all-zero windows, foreground on every border and corner; sizes on and off the 64-sample tile grid.
    The L2 sum and the IoU (counts) are exact; the chamfer sum and every gradient sample lie within 1e-5 of the sum of the
    magnitudes of their addends (<= 50 float32 additions per gradient sample: 50 * 2^-24 = 3e-6).  The same holds against torch on
    the GPU - the path users have had - whose max-pool tie rule is thereby shown to be the CPU's."""
    rng = np.random.default_rng(100 * size + k)
    lw = 0.5
    alpha, keep, ref = _edge_case_images(size, rng)
    edt = distance_transform_edt(~_band(ref, k)) ** 0.5
    terms, grad = _edge_terms(alpha, keep, ref, edt, k, lw)
    n = alpha.shape[0]
    assert not grad[:, size:].any() and not grad[:, :, size:].any()               # outside the image: zeros, not left-overs
    img = keep[None] * alpha
    inter, union = (img * ref).sum((1, 2)), np.clip(img + ref, 0, 1).sum((1, 2))
    want_iou = inter.astype(np.float32) / (union.astype(np.float32) + np.float32(1e-6))
    for where, dtype in (("cpu", torch.float64), ("cuda", torch.float32)):
        mask, cham, g, mag, cham_mag = _torch_edge_terms(alpha, keep, ref, edt.astype(np.float32), k, lw, where, dtype)
        err_c = np.abs(terms[:, 3] - cham) / np.maximum(cham_mag, 1e-30)
        err_g = np.abs(grad[:, :size, :size] - g) / np.maximum(mag, 1e-30)
        print(size, k, where, "chamfer rel err", err_c.max(), "gradient rel err", err_g.max(), "chamfer", cham)
        assert np.array_equal(terms[:, 2], mask.astype(np.float32))
        assert np.array_equal(terms[:, 1], want_iou)
        assert (np.abs(terms[:, 3] - cham) <= EDGE_REL * cham_mag).all()
        assert (np.abs(grad[:, :size, :size] - g) <= EDGE_REL * mag).all()
    assert float(terms[:, 3].max()) > 0
    assert np.array_equal(terms[:, 0], terms[:, 2] + np.float32(lw) * terms[:, 3])            # (float32: rounded like the sum of the dict)


@pytest.mark.gpu
def test_edge_terms_all_zero_window_names_its_top_left_sample():
    """torch's rule in the degenerate case: an all-zero 12 x 12 image under a 7-window sends gradient to 81 positions."""
    z = np.zeros((1, 12, 12))
    one = np.ones((12, 12))
    _, grad = _edge_terms(z, one, np.zeros((12, 12)), one, 7, 1.0)
    named = grad[0, :12, :12] + 1.0                   # (keep = 1, img = ref: the gradient is named - edt)
    print("positions named", int((named > 0).sum()), "total", named.sum())
    assert int((named > 0).sum()) == 81 and named.sum() == 144.0


@pytest.mark.gpu
def test_edge_terms_refuse_other_window_sizes():
    from homan_amd import lib as hlib
    L, P = hlib.lib(), hlib.ptr
    t = torch.zeros(1, 64, 64, device="cuda")
    ws = torch.zeros(L.hm_pose_edge_workspace_bytes(1, 64), dtype=torch.uint8, device="cuda")
    out = torch.zeros(4, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in (1, 4, 9):
        assert L.hm_pose_edge_terms(P(t), P(t[0]), P(t[0]), P(t[0]), 1, 64, 64, k, 0.5, P(out), P(t.clone()), P(ws), hlib.stream()) == -3
    for k in (4, 9):
        assert L.hm_edge_edt(P(t[0]), 64, 64, k, 0.25, P(t[0].clone()), P(cnt), hlib.stream()) == -3


def _autograd_step(po, sc, rots6, trans, lw_chamfer):
    """one step of PoseOptimizer.forward + autograd + torch Adam from the given poses -> (per-candidate losses, loss_dict, module)"""
    m = po.PoseOptimizer(ref_image=sc["rec"]["in_mask"], vertices=sc["verts"], faces=sc["faces"], rotation_init=rots6,
                         translation_init=trans, num_initializations=sc["n"], K=sc["K"], lw_chamfer=lw_chamfer)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    ld, _, _ = m()
    per_pose = sum(ld.values())
    per_pose.sum().backward()
    opt.step()
    return per_pose.detach(), ld, m


def _fused_step(po, sc, rots6, trans, lw_chamfer):
    m = po.PoseOptimizer(ref_image=sc["rec"]["in_mask"], vertices=sc["verts"], faces=sc["faces"], rotation_init=rots6,
                         translation_init=trans, num_initializations=sc["n"], K=sc["K"], lw_chamfer=lw_chamfer)
    losses, _, _ = po._fused_loop(m, 1e-2, 1)
    return losses.clone(), m


def _same_step(a_losses, a, b_losses, b, tag):
    dl = (np.abs(b_losses.cpu().numpy() - a_losses.cpu().numpy()) / np.abs(a_losses.cpu().numpy())).max()
    dr = (b.rotations - a.rotations).abs().max().item()
    dt = (b.translations - a.translations).abs().max().item()
    print(tag, "loss rel diff", dl, "rotation diff", dr, "translation diff", dt)
    np.testing.assert_allclose(b_losses.cpu().numpy(), a_losses.cpu().numpy(), rtol=2e-5)
    np.testing.assert_allclose(b.rotations.detach().cpu().numpy(), a.rotations.detach().cpu().numpy(), atol=2e-5)
    np.testing.assert_allclose(b.translations.detach().cpu().numpy(), a.translations.detach().cpu().numpy(), atol=2e-5)


@pytest.mark.gpu
def test_fused_step_with_the_edge_term_equals_the_autograd_step():
    """test_fused_poseinit_step_equals_the_autograd_step with lw_chamfer = 0.5: the fused launch sequence (hm_pose_edge_terms,
    hm_sil_bwd mode 3) against PoseOptimizer.forward + autograd (max-pool through torch, scipy distance transform) + torch Adam,
    after ONE step from the same start, two candidates pushed half out of the image (by 0.08: they keep half of their ~2 000
    covered samples, so their chamfer sums stay positive; the 0.25 of that test leaves nothing of them on screen).  That test's tolerances: rtol 2e-5 on the
    losses, atol 2e-5 on the poses.  The term is positive and it acts: some candidate's step differs from its lw_chamfer = 0
    step by far more than the tolerance.  Measured on an MI355X: losses equal, rotations within 1e-9, translations within 2e-9; the
    step with the term differs from the step without it by 0.02 (two Adam steps of opposite sign)."""
    from homan_amd import pose_optimization as po
    sc = _scene()
    sc["trans0"][:2, :, 0] += 0.08
    r6 = po.matrix_to_rot6d(sc["rots"])
    a_losses, ld, a = _autograd_step(po, sc, r6, sc["trans0"], 0.5)
    assert float(ld["offscreen"].max()) > 0
    print("chamfer", ld["chamfer"].detach().cpu().numpy())
    assert float(ld["chamfer"].min()) > 0
    b_losses, b = _fused_step(po, sc, r6, sc["trans0"], 0.5)
    _same_step(a_losses, a, b_losses, b, "lw 0.5")
    _, c = _fused_step(po, sc, r6, sc["trans0"], 0)
    moved = max((b.rotations - c.rotations).abs().max().item(), (b.translations - c.translations).abs().max().item())
    print("step with the term vs without", moved)
    assert moved > 100 * 2e-5


@pytest.mark.gpu
def test_whole_fits_with_the_edge_term(monkeypatch):
    """find_optimal_pose(..., lw_chamfer=0.5), mode "fused" against the autograd modes, 8 steps on the golden scene.  Free runs of a
    piecewise-constant loss separate once a sample flips, so the comparison is teacher-forced: from every pose the autograd
    trajectory visits, one fused step equals one autograd step (the tolerances of the one-step test).  Free-running, both loops end
    with a best-ever loss no worse than their first step's; the fused result is the same bits in a second run, through a resident
    fitter that fitted another mask in between, and with the candidates walked as two or three groups."""
    from homan_amd import pose_optimization as po
    sc = _scene()
    rec, n, size = sc["rec"], sc["n"], sc["size"]
    r6 = po.matrix_to_rot6d(sc["rots"])
    # the autograd trajectory (reference loop, :330-357) and its best-ever loss
    m = po.PoseOptimizer(ref_image=rec["in_mask"], vertices=sc["verts"], faces=sc["faces"], rotation_init=r6,
                         translation_init=sc["trans0"], num_initializations=n, K=sc["K"], lw_chamfer=0.5)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    visited, minima = [], []
    for _ in range(8):
        visited.append((m.rotations.detach().clone().cpu(), m.translations.detach().clone().cpu()))
        opt.zero_grad()
        per_pose = sum(m()[0].values())
        per_pose.sum().backward()
        opt.step()
        minima.append(float(per_pose.min()))
    print("autograd per-step minima", minima)
    assert np.isfinite(minima).all() and min(minima) <= minima[0]
    for t, (rot_t, trans_t) in enumerate(visited):
        a_losses, _, a = _autograd_step(po, sc, rot_t, trans_t, 0.5)
        b_losses, b = _fused_step(po, sc, rot_t, trans_t, 0.5)
        _same_step(a_losses, a, b_losses, b, f"step {t}")
    # free runs
    first = po.PoseOptimizer(ref_image=rec["in_mask"], vertices=sc["verts"], faces=sc["faces"], rotation_init=r6,
                             translation_init=sc["trans0"], num_initializations=n, K=sc["K"], lw_chamfer=0.5)
    first_min = float(po._fused_loop(first, 1e-2, 1)[0].min())
    loop = po._FusedPoseLoop(po.PoseOptimizer(ref_image=rec["in_mask"], vertices=sc["verts"], faces=sc["faces"], rotation_init=r6,
                                              translation_init=sc["trans0"], num_initializations=n, K=sc["K"], lw_chamfer=0.5), 1e-2)
    loop.run(8)
    torch.cuda.synchronize()
    print("fused first-step minimum", first_min, "best ever", float(loop.best_loss), "band samples", int(loop.edge.band_samples))
    assert np.isfinite(float(loop.best_loss)) and float(loop.best_loss) <= first_min
    assert int(loop.edge.band_samples) == int(_band((rec["in_mask"] > 0).astype(np.float32), 7).sum())
    loop.release()

    mask_a = rec["in_mask"]
    mask_b = np.roll(mask_a, (3, -2), axis=(0, 1)).copy()
    mask_b[: size // 4] = -1

    def fit(mask, mode="fused", steps=8):
        return po.find_optimal_pose(sc["verts"], sc["faces"], mask, rec["in_bbox"], rec["in_square_bbox"], (350, 350), K=rec["in_K"],
                                    num_iterations=steps, num_initializations=n, rotations_init=sc["rots"], rend_size=size,
                                    sort_best=True, mode=mode, lw_chamfer=0.5)

    same = lambda x, y: torch.equal(x.rotations, y.rotations) and torch.equal(x.translations, y.translations)
    graph = fit(mask_a, "graph")
    assert torch.isfinite(sum(graph()[0].values())).all()
    monkeypatch.setenv("HOMAN_POSE_PARTS", "1")
    monkeypatch.setenv("HOMAN_POSE_FITTER", "0")
    alone, again = fit(mask_a), fit(mask_a)
    alone_b = fit(mask_b, steps=5)
    assert same(alone, again)
    monkeypatch.setenv("HOMAN_POSE_FITTER", "1")
    po._FITTERS.clear()
    res_a, res_b, res_a2 = fit(mask_a), fit(mask_b, steps=5), fit(mask_a)
    assert len(po._FITTERS) == 1 and next(iter(po._FITTERS.values())).fits == 3
    assert same(res_a, alone) and same(res_b, alone_b) and same(res_a2, alone)
    assert not same(res_a, res_b)
    for parts in (2, 3):
        monkeypatch.setenv("HOMAN_POSE_PARTS", str(parts))
        po._FITTERS.clear()
        g_a, g_b, g_a2 = fit(mask_a), fit(mask_b, steps=5), fit(mask_a)
        assert next(iter(po._FITTERS.values())).parts == parts
        assert same(g_a, alone) and same(g_b, alone_b) and same(g_a2, alone)
        la, ia, _ = g_a()
        lb, ib, _ = alone()
        assert torch.equal(ia, ib) and all(torch.equal(la[key], lb[key]) for key in la)
    po._FITTERS.clear()


_KEPT = []


def _kernel_nodes(step):
    """kernel nodes of `step` captured in a hipGraph"""
    g = torch.cuda.CUDAGraph(keep_graph=True)
    _KEPT.append(g)                          # (graphs are never destroyed in this process: homan_amd.lib.new_graph)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        step()
    hip = ctypes.CDLL("libamdhip64.so")
    raw = ctypes.c_void_p(g.raw_cuda_graph())
    count = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(count)) == 0
    nodes = (ctypes.c_void_p * count.value)()
    assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(count)) == 0
    kinds = []
    for node in nodes:
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) == 0
        kinds.append(kind.value)
    return sum(1 for kind in kinds if kind == 0), len(kinds)              # hipGraphNodeTypeKernel = 0


@pytest.mark.gpu
def test_weight_zero_is_untouched(monkeypatch):
    """find_optimal_pose(...) and find_optimal_pose(..., lw_chamfer=0) return the same bits, resident and standalone, and a step
    captured with weight 0 holds FUSED_STEP_KERNEL_NODES = 10 kernel nodes - the count of the commit before the term existed - and
    nothing else; the step with the term holds one more (hm_pose_edge_terms in hm_sil_reduce's place, plus the mask pass of
    hm_sil_bwd mode 3 that mode 5 does without)."""
    from homan_amd import pose_optimization as po
    sc = _scene()
    rec, n, size = sc["rec"], sc["n"], sc["size"]

    def fit(**kw):
        po._FITTERS.clear()
        return po.find_optimal_pose(sc["verts"], sc["faces"], rec["in_mask"], rec["in_bbox"], rec["in_square_bbox"], (350, 350),
                                    K=rec["in_K"], num_iterations=8, num_initializations=n, rotations_init=sc["rots"],
                                    rend_size=size, **kw)

    for resident in ("1", "0"):
        monkeypatch.setenv("HOMAN_POSE_FITTER", resident)
        plain, zero = fit(), fit(lw_chamfer=0)
        assert torch.equal(plain.rotations, zero.rotations) and torch.equal(plain.translations, zero.translations)
        lp, ip, _ = plain()
        lz, iz, _ = zero()
        assert torch.equal(ip, iz) and all(torch.equal(lp[key], lz[key]) for key in lp)
    po._FITTERS.clear()
    counts = {}
    for lw in (0, 0.5):
        m = po.PoseOptimizer(ref_image=rec["in_mask"], vertices=sc["verts"], faces=sc["faces"], rotation_init=po.matrix_to_rot6d(sc["rots"]),
                             translation_init=sc["trans0"], num_initializations=n, K=sc["K"], lw_chamfer=lw)
        loop = po._FusedPoseLoop(m, 1e-2)
        counts[lw] = _kernel_nodes(loop._step)
        loop.release()
    print("(kernel nodes, all nodes) of a captured step", counts)
    assert counts[0] == (FUSED_STEP_KERNEL_NODES, FUSED_STEP_KERNEL_NODES)
    assert counts[0.5] == (EDGE_STEP_KERNEL_NODES, EDGE_STEP_KERNEL_NODES)


@pytest.mark.gpu
def test_find_optimal_poses_passes_the_edge_term_through():
    """The clip wrapper with lw_chamfer = 0.5: the reference's dict keys and shapes, orthonormal rotations, and the fitters it
    went through were built for that weight."""
    from homan_amd import pose_optimization as po
    rec = _load()
    size, n = int(rec["meta_size"]), int(rec["meta_n"])
    verts, faces, K = rec["in_vertices"], rec["in_faces"], rec["in_K"]
    ann = {"target_crop_mask": rec["in_mask"], "bbox": rec["in_bbox"], "square_bbox": rec["in_square_bbox"], "full_mask": torch.zeros(8, 8)}
    rots0 = torch.from_numpy(rec["in_rotations_init"])
    sampler = po.compute_random_rotations
    po.compute_random_rotations = lambda B=10, *a, **k: rots0.clone().to("cuda")
    po._FITTERS.clear()
    try:
        out = po.find_optimal_poses((350, 350), faces=faces, vertices=verts, annotations=[ann, ann], Ks=[K, K], num_iterations=4,
                                    num_initializations=n, rend_size=size, lw_chamfer=0.5)
    finally:
        po.compute_random_rotations = sampler
    assert len(po._FITTERS) == 1
    fitter = next(iter(po._FITTERS.values()))
    assert fitter.fits == 2 and fitter.shell.lw_chamfer == 0.5 and (fitter.loop or fitter.loops[0]).edge is not None
    po._FITTERS.clear()
    V = verts.shape[0]
    assert len(out) == 2
    for h in out:
        assert set(h) == {"rotations", "translations", "verts_trans", "target_masks", "K_roi", "masks", "verts", "full_mask"}
        assert tuple(h["rotations"].shape) == (1, 3, 3) and tuple(h["translations"].shape) == (1, 1, 3)
        assert tuple(h["verts_trans"].shape) == (1, V, 3) and tuple(h["target_masks"].shape) == (1, size, size)
        assert tuple(h["K_roi"].shape) == (1, 1, 3, 3)
        R = h["rotations"][0].cpu()
        np.testing.assert_allclose((R.T @ R).numpy(), np.eye(3), atol=1e-5)
        assert torch.isfinite(h["translations"]).all()
