"""The pose initialisation's soft silhouette mode on the GPU: hm_softsil_pose_terms / hm_sigma_anneal (csrc/softpose.hip) on their
own, PoseOptimizer(sil_mode="soft") and the fused loop against the float64 restatement (tests/softpose_ref.py), the whole
free-running fit against the restatement's loop with torch Adam, the three loop modes, the resident fitter and its candidate
groups, the blur schedule, and find_optimal_poses.

Bars.  Sums of exactly representable addends are compared exactly; sums of random addends with the worst-case bound of a float32
sum of S^2 non-negative addends in any order, (S^2 + 2) 2^-24 relative.  Module against restatement: the rule of
tests/test_softsil_gpu.py - both get the SAME float32 inputs; values within 4 x the deviation of the restatement run in float32
from the one run in float64, + 1e-6; gradients within 4 x that deviation, relative to the largest entry.  Steps and fits: the
project's one-step bars, rtol 2e-5 on losses and atol 2e-5 on poses (tests/test_poseedge_gpu.py).  Every figure is printed
before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from tests import softpose_ref as ref

pytestmark = pytest.mark.gpu

# (N, S): one sample; fewer samples than a wave, odd count; odd count over many lanes; the 16-byte path with a partial chunk;
# many candidates; several partial sums per candidate through the ticket
SHAPES = [(1, 1), (3, 3), (2, 37), (5, 40), (70, 64), (3, 130)]
SIGMAS = [1e-3, 4e-3]
EPS24 = 2.0 ** -24


def _masks(S, gen):
    """-1 / 0 / 1 masks: a target with an occluded band, everything occluded, everything kept"""
    target = (torch.rand(S, S, generator=gen) < 0.4).float()
    banded = target.clone()
    banded[:, : max(1, S // 8)] = -1
    banded[S // 2: S // 2 + max(1, S // 6), S // 3:] = -1
    return {"banded": banded, "occluded": torch.full((S, S), -1.0), "kept": target}


def _call(alpha, mask, terms=None, grad=None, ws=None):
    """hm_softsil_pose_terms on host tensors alpha (N,S,S), mask (S,S) -> (terms (N,2), grad (N,S,S)) on the host"""
    from homan_amd import lib as hlib, ops
    N, S = alpha.shape[0], alpha.shape[1]
    a, keep, tgt = alpha.cuda().contiguous(), (mask >= 0).float().cuda(), (mask > 0).float().cuda()
    terms = torch.full((N, 2), -7.5, device="cuda") if terms is None else terms
    grad = torch.full((N, S, S), -7.5, device="cuda") if grad is None else grad
    ws = ops.softsil_pose_workspace(N, S, "cuda") if ws is None else ws
    hlib.check(hlib.lib().hm_softsil_pose_terms(hlib.ptr(a), hlib.ptr(keep), hlib.ptr(tgt), N, S, hlib.ptr(terms), hlib.ptr(grad),
                                                hlib.ptr(ws), hlib.stream()), "hm_softsil_pose_terms")
    return terms.cpu(), grad.cpu()


def _sums64(alpha, mask):
    keep, tgt = (mask >= 0).double(), (mask > 0).double()
    image = keep * alpha.double()
    return (((image - tgt) ** 2).sum((1, 2)), (image * tgt).sum((1, 2)), (image + tgt).clamp(0, 1).sum((1, 2)))


def _grad32(alpha, mask):
    keep, tgt = (mask >= 0).float(), (mask > 0).float()
    return 2 * keep * (keep * alpha - tgt)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_terms_on_exact_inputs(shape):
    """alpha in {0, 1/8, .., 1}: every addend is a multiple of 1/64 and every sum stays below 2^24 / 64, so any summation order is
    exact - the mask term equals the float64 value, the IoU is one add and one divide away (3e-7), the gradient image equals the
    float32 expression (keep is 0 / 1: every operation in it is exact)."""
    N, S = shape
    gen = torch.Generator().manual_seed(1000 * N + S)
    alpha = torch.randint(0, 9, (N, S, S), generator=gen).float() / 8
    for name, mask in _masks(S, gen).items():
        terms, grad = _call(alpha, mask)
        sq, inter, union = _sums64(alpha, mask)
        iou = inter / (union + 1e-6)
        err = float(((terms[:, 1].double() - iou).abs() / iou.clamp_min(1e-30)).max())
        print(shape, name, "mask equal", torch.equal(terms[:, 0].double(), sq), "IoU rel err", err)
        assert torch.equal(terms[:, 0].double(), sq)
        assert ((terms[:, 1].double() - iou).abs() <= ref.IOU_REL * iou).all()
        assert torch.equal(grad, _grad32(alpha, mask))
        assert name != "occluded" or (not terms.any() and not grad.any())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_terms_on_random_inputs(shape):
    """alpha in [0, 1).  The sum of squares, and each of the IoU's two sums, within (S^2 + 2) 2^-24 relative of float64.  The two
    sums reach the caller only as their quotient, so each is isolated by a mask: target everywhere -> the union is S^2 exactly
    and IoU (S^2 + 1e-6) is the intersection; target on ONE sample p -> the intersection is alpha_p exactly and alpha_p / IoU -
    1e-6 is the union; both through one add and one divide (3e-7, as above).  On the general masks the quotient is held to the
    sum of its parts' bounds.  The gradient image is bit-equal as on exact inputs."""
    N, S = shape
    gen = torch.Generator().manual_seed(2000 * N + S)
    alpha = torch.rand(N, S, S, generator=gen)
    bound = (S * S + 2) * EPS24
    for name, mask in _masks(S, gen).items():
        terms, grad = _call(alpha, mask)
        sq, inter, union = _sums64(alpha, mask)
        iou = inter / (union + 1e-6)
        e_sq = float(((terms[:, 0].double() - sq).abs() / sq.clamp_min(1e-30)).max())
        e_iou = float(((terms[:, 1].double() - iou).abs() / iou.clamp_min(1e-30)).max())
        print(shape, name, "sum of squares rel err", e_sq, "IoU rel err", e_iou, "bound", bound)
        assert ((terms[:, 0].double() - sq).abs() <= bound * sq).all()
        assert ((terms[:, 1].double() - iou).abs() <= (2 * bound + ref.IOU_REL) * iou).all()
        assert torch.equal(grad, _grad32(alpha, mask))
    full = torch.ones(S, S)
    terms, _ = _call(alpha, full)
    _, inter, _ = _sums64(alpha, full)
    got = terms[:, 1].double() * (S * S + 1e-6)
    print(shape, "intersection rel err", float(((got - inter).abs() / inter).max()))
    assert ((got - inter).abs() <= (bound + ref.IOU_REL) * inter).all()
    one = torch.zeros(S, S)
    one[S // 2, S // 3] = 1
    terms, _ = _call(alpha + 0.01, one)                       # (alpha_p > 0)
    _, inter, union = _sums64(alpha + 0.01, one)
    got = inter / terms[:, 1].double() - 1e-6
    print(shape, "union rel err", float(((got - union).abs() / union).max()))
    assert ((got - union).abs() <= (bound + ref.IOU_REL) * union).all()


def test_a_candidates_results_do_not_depend_on_the_batch():
    """the 70 rows of one call at N = 70 equal, bit for bit, 70 calls at N = 1; two calls agree bit for bit"""
    from homan_amd import ops
    N, S = 70, 64
    gen = torch.Generator().manual_seed(3)
    alpha = torch.rand(N, S, S, generator=gen)
    mask = _masks(S, gen)["banded"]
    terms, grad = _call(alpha, mask)
    again_t, again_g = _call(alpha, mask)
    assert torch.equal(terms, again_t) and torch.equal(grad, again_g)
    ws = ops.softsil_pose_workspace(1, S, "cuda")
    rows = [_call(alpha[i: i + 1], mask, ws=ws) for i in range(N)]
    assert torch.equal(torch.cat([t for t, _ in rows]), terms) and torch.equal(torch.cat([g for _, g in rows]), grad)
    # an odd size (the scalar path) the same way
    alpha, mask = torch.rand(5, 37, 37, generator=gen), _masks(37, gen)["banded"]
    terms, grad = _call(alpha, mask)
    rows = [_call(alpha[i: i + 1], mask) for i in range(5)]
    assert torch.equal(torch.cat([t for t, _ in rows]), terms) and torch.equal(torch.cat([g for _, g in rows]), grad)


def test_bad_arguments_leave_the_outputs_untouched():
    from homan_amd import lib as hlib, ops
    L, P = hlib.lib(), hlib.ptr
    N, S = 3, 16
    gen = torch.Generator().manual_seed(4)
    alpha = torch.rand(N, S, S, generator=gen).cuda()
    mask = _masks(S, gen)["banded"]
    keep, tgt = (mask >= 0).float().cuda(), (mask > 0).float().cuda()
    terms, grad = torch.full((N, 2), -7.5, device="cuda"), torch.full((N, S, S), -7.5, device="cuda")
    ws = ops.softsil_pose_workspace(N, S, "cuda")
    tensors = dict(alpha=alpha, keep=keep, ref=tgt, terms=terms, grad=grad, ws=ws)

    def call(N=N, S=S, **null):
        t = {k: (None if k in null else P(v)) for k, v in tensors.items()}
        return L.hm_softsil_pose_terms(t["alpha"], t["keep"], t["ref"], N, S, t["terms"], t["grad"], t["ws"], hlib.stream())

    assert call(N=0) == -1 and call(S=0) == -1 and call(S=4097) == -1 and call(N=65536) == -1
    for name in tensors:
        assert call(**{name: None}) == -1, name
    sigma = torch.tensor([1e-3], device="cuda")
    for bad in ((None, 0.9, 0.0), (P(sigma), 0.0, 0.0), (P(sigma), 1.5, 0.0), (P(sigma), 0.9, -1.0), (P(sigma), float("nan"), 0.0)):
        assert L.hm_sigma_anneal(*bad, hlib.stream()) == -1, bad
    torch.cuda.synchronize()
    assert bool((terms == -7.5).all()) and bool((grad == -7.5).all()) and float(sigma) == float(np.float32(1e-3))
    assert call() == 0 and L.hm_sigma_anneal(P(sigma), 0.5, 0.0, hlib.stream()) == 0
    torch.cuda.synchronize()
    assert not bool((terms == -7.5).any()) and not bool((grad == -7.5).any())
    assert float(sigma) == float(np.float32(1e-3) * np.float32(0.5))


# ---------------------------------------------------------------- module and loops against the restatement
def _start(S, offscreen=False):
    sc = ref.scene(S)
    trans = sc["trans"].clone()
    if offscreen:
        trans[0, 0, 0] += 0.25                 # candidate 0 half out of the image: the off-screen gradient joins
    return sc, sc["rot6d"], trans


@functools.lru_cache(maxsize=None)
def _restated(S, sigma, offscreen):
    """the restatement in float64 and float32 on the start's float32 inputs, once per case"""
    sc, r6, trans = _start(S, offscreen)
    s = float(np.float32(sigma))
    args = (r6, trans, sc["mesh"], sc["faces"], sc["K"], sc["mask"], s)
    return ref.forward_and_grads(*args, torch.float64), ref.forward_and_grads(*args, torch.float32)


def _module(S, sigma, offscreen=False, **kw):
    from homan_amd.pose_optimization import PoseOptimizer
    sc, r6, trans = _start(S, offscreen)
    return PoseOptimizer(ref_image=sc["mask"].numpy(), vertices=sc["mesh"], faces=sc["faces"], rotation_init=r6,
                         translation_init=trans, num_initializations=4, K=sc["K"][None], sil_mode="soft", sil_sigma=sigma, **kw)


def _check_values(tag, got, w64, w32):
    """the 4 x rule on values: images per sample, absolute; per-candidate terms relative to the float64 value"""
    for key in ("image", "mask", "iou", "offscreen"):
        g, a, b = got[key].detach().cpu().double(), w64[key], w32[key].double()
        scale = 1.0 if key == "image" else a.abs().clamp_min(1e-30)
        if key == "offscreen":
            scale = torch.where(a > 0, a, torch.ones_like(a))
        dev, err = float(((b - a).abs() / scale).max()), float(((g - a).abs() / scale).max())
        print(tag, key, "restatement f32-f64", dev, "module", err)
        assert torch.isfinite(g).all() and err <= ref.RULE_FACTOR * dev + ref.VALUE_ABS, key


def _check_grads(tag, g_rot, g_trans, r64, r32):
    (_, gr64, gt64), (_, gr32, gt32) = r64, r32
    for key, g, a, b in (("rotations", g_rot, gr64, gr32), ("translations", g_trans, gt64, gt32)):
        g, b = g.detach().cpu().double().reshape(a.shape), b.double()
        top = float(a.abs().max())
        dev, err = float((b - a).abs().max()) / top, float((g - a).abs().max()) / top
        print(tag, key, "gradient (of max %.3e): restatement f32-f64" % top, dev, "module", err)
        assert top > 0 and torch.isfinite(g).all() and err <= ref.RULE_FACTOR * dev, key


@pytest.mark.parametrize("case", [(32, 1e-3, False), (32, 4e-3, False), (37, 1e-3, False), (37, 4e-3, False), (32, 1e-3, True)], ids=str)
def test_forward_and_backward_match_the_restatement(case):
    """PoseOptimizer(sil_mode="soft").forward() + backward on the cube scene against the float64 restatement: image, mask term,
    IoU, off-screen term and the gradients of rotations / translations, depth included, under the 4 x rule."""
    S, sigma, offscreen = case
    r64, r32 = _restated(S, sigma, offscreen)
    m = _module(S, sigma, offscreen)
    ld, iou, image = m()
    assert set(ld) == {"mask", "chamfer", "offscreen"} and not ld["chamfer"].any() and not iou.requires_grad
    sum(ld.values()).sum().backward()
    _check_values(case, dict(image=image, mask=ld["mask"], iou=iou, offscreen=ld["offscreen"]), r64[0], r32[0])
    assert (float(r64[0]["offscreen"].max()) > 0) == offscreen
    assert float(m.translations.grad[..., 2].abs().max()) > 0
    _check_grads(case, m.rotations.grad, m.translations.grad, r64, r32)


def _same_step(a_losses, a, b_losses, b, tag):
    """tests/test_poseedge_gpu.py::_same_step"""
    dl = (np.abs(b_losses.cpu().numpy() - a_losses.cpu().numpy()) / np.abs(a_losses.cpu().numpy())).max()
    dr = (b.rotations - a.rotations).abs().max().item()
    dt = (b.translations - a.translations).abs().max().item()
    print(tag, "loss rel diff", dl, "rotation diff", dr, "translation diff", dt)
    np.testing.assert_allclose(b_losses.cpu().numpy(), a_losses.cpu().numpy(), rtol=2e-5)
    np.testing.assert_allclose(b.rotations.detach().cpu().numpy(), a.rotations.detach().cpu().numpy(), atol=2e-5)
    np.testing.assert_allclose(b.translations.detach().cpu().numpy(), a.translations.detach().cpu().numpy(), atol=2e-5)


@pytest.mark.parametrize("offscreen", [False, True])
def test_fused_step_equals_the_autograd_step(offscreen):
    """One _FusedPoseLoop step from the same start: its gradients obey the 4 x rule against float64; losses and poses after the step
    equal one autograd + torch Adam step of the same module at the one-step bars."""
    from homan_amd import pose_optimization as po
    S, sigma = 32, 1e-3
    a = _module(S, sigma, offscreen)
    opt = torch.optim.Adam(a.parameters(), lr=1e-2)
    a_losses = sum(a()[0].values())
    a_losses.sum().backward()
    opt.step()
    b = _module(S, sigma, offscreen)
    loop = po._FusedPoseLoop(b, 1e-2)
    b_losses = loop.run(1)[0].clone()
    torch.cuda.synchronize()
    g_rot, g_trans = b.rotations.grad.clone(), b.translations.grad.clone()
    assert loop.stamped_replays(3) is None
    loop.release()
    _check_grads(("fused", offscreen), g_rot, g_trans, *_restated(S, sigma, offscreen))
    _same_step(a_losses.detach(), a, b_losses, b, ("fused vs autograd", offscreen))
    assert float(np.float32(b.sil_sigma.item())) == float(np.float32(sigma))


@functools.lru_cache(maxsize=None)
def _cpu_fit(sigma, steps=30):
    sc, r6, trans = _start(32)
    return ref.fit(r6, trans, sc["mesh"], sc["faces"], sc["K"], sc["mask"], float(np.float32(sigma)), steps, 1e-2, torch.float64)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_whole_fit_against_the_cpu(sigma):
    """30 free-running fused steps at S = 32, lr 1e-2, against the float64 restatement's loop with torch Adam: final poses within
    2e-5, final losses within 2e-5 relative (the float32 restatement loop ends 4.3e-7 / 2.2e-6 from the float64 one), and the fit
    works: the smallest final loss is below half the smallest first loss (the CPU loops reach 0.10 / 0.13 of it).  Measured on an
    MI355X: sigma 1e-3: rotations 5.3e-7, translations 1.3e-7, losses 9.7e-7, smallest loss 30.47 -> 3.095; sigma 4e-3: 3.9e-7,
    8.1e-8, 1.2e-6, 36.68 -> 4.861."""
    from homan_amd import pose_optimization as po
    r, t, losses = _cpu_fit(sigma)
    m = _module(32, sigma)
    loop = po._FusedPoseLoop(m, 1e-2)
    first = loop.run(1)[0].clone()
    final = loop.run(29)[0].clone()
    torch.cuda.synchronize()
    loop.release()
    d_rot = float((m.rotations.detach().cpu().double() - r).abs().max())
    d_trans = float((m.translations.detach().cpu().double() - t).abs().max())
    d_loss = float(((final.cpu().double() - losses[-1]).abs() / losses[-1]).max())
    print("sigma", sigma, "fit vs CPU float64: rotations", d_rot, "translations", d_trans, "losses (relative)", d_loss,
          "| smallest loss", float(first.min()), "->", float(final.min()), "CPU", float(losses[0].min()), "->", float(losses[-1].min()))
    np.testing.assert_allclose(first.cpu().numpy(), losses[0].numpy(), rtol=2e-5)
    assert float(final.min()) < 0.5 * float(first.min())
    assert d_rot <= 2e-5 and d_trans <= 2e-5 and d_loss <= 2e-5


# ---------------------------------------------------------------- find_optimal_pose(s), fitter, schedule
def _fop_args(S, pad=0):
    """find_optimal_pose's arguments for the scene: the crop is the whole image, K in pixels"""
    sc = ref.scene(S)
    rows, cols = np.nonzero(sc["mask"].numpy() > 0)
    bbox = [float(cols.min()), float(rows.min()), float(cols.max() - cols.min() + 1), float(rows.max() - rows.min() + 1)]
    K = sc["K"].clone()
    K[:2] *= S
    rots = torch.cat([sc["rots"], sc["rots"][:pad]])
    return sc, dict(vertices=sc["mesh"], faces=sc["faces"], bbox=bbox, square_bbox=[0.0, 0.0, float(S), float(S)], image_size=(S, S),
                    K=K, num_initializations=4 + pad, rotations_init=rots, rend_size=S, sort_best=False, sil_mode="soft")


def _same_bits(x, y):
    return torch.equal(x.rotations, y.rotations) and torch.equal(x.translations, y.translations)


def test_modes_and_residency(monkeypatch):
    """find_optimal_pose(sil_mode="soft"), 8 steps: "fused", "graph" and "eager" agree at the bars of the whole fit; the fused
    result through a resident fitter that fitted another mask and another blur in between equals a standalone fit bit for bit,
    also with the candidates padded to 6 and walked as 2 and 3 groups; an odd mask size goes through the fitter."""
    from homan_amd import pose_optimization as po
    sc, kw = _fop_args(32)
    mask_a = sc["mask"].numpy()
    mask_b = np.roll(mask_a, (2, -3), axis=(0, 1)).copy()
    mask_b[:6] = -1
    fit = lambda mask, steps=8, **more: po.find_optimal_pose(mask=mask, num_iterations=steps, **{**kw, "sil_sigma": 1e-3, **more})
    monkeypatch.setenv("HOMAN_POSE_FITTER", "0")
    monkeypatch.setenv("HOMAN_POSE_PARTS", "1")
    alone, alone_b = fit(mask_a), fit(mask_b, steps=5)
    assert not _same_bits(alone, alone_b) and torch.isfinite(alone.rotations).all()
    losses = lambda m: sum(m()[0].values()).detach()
    for mode in ("graph", "eager"):
        other = fit(mask_a, mode=mode)
        _same_step(losses(alone), alone, losses(other), other, ("fused vs " + mode))
    monkeypatch.setenv("HOMAN_POSE_FITTER", "1")
    po._FITTERS.clear()
    res_a, res_b, res_c, res_a2 = fit(mask_a), fit(mask_b, steps=5), fit(mask_b, sil_sigma=4e-3), fit(mask_a)
    assert len(po._FITTERS) == 2 and sorted(f.fits for f in po._FITTERS.values()) == [1, 3]
    assert _same_bits(res_a, alone) and _same_bits(res_b, alone_b) and _same_bits(res_a2, alone) and not _same_bits(res_c, res_b)
    _, kw6 = _fop_args(32, pad=2)
    fit6 = lambda mask, steps=8: po.find_optimal_pose(mask=mask, num_iterations=steps, **{**kw6, "sil_sigma": 1e-3})
    monkeypatch.setenv("HOMAN_POSE_FITTER", "0")
    alone6, alone6_b = fit6(mask_a), fit6(mask_b, 5)
    assert torch.equal(alone6.rotations[:4], alone.rotations) and torch.equal(alone6.rotations[4:], alone.rotations[:2])
    monkeypatch.setenv("HOMAN_POSE_FITTER", "1")
    for parts in (2, 3):
        monkeypatch.setenv("HOMAN_POSE_PARTS", str(parts))
        po._FITTERS.clear()
        g_a, g_b, g_a2 = fit6(mask_a), fit6(mask_b, 5), fit6(mask_a)
        fitter = next(iter(po._FITTERS.values()))
        assert fitter.parts == parts and fitter.fits == 3
        assert _same_bits(g_a, alone6) and _same_bits(g_b, alone6_b) and _same_bits(g_a2, alone6)
        la, ia, _ = g_a()
        lb, ib, _ = alone6()
        assert torch.equal(ia, ib) and all(torch.equal(la[k], lb[k]) for k in la)
    monkeypatch.setenv("HOMAN_POSE_PARTS", "1")
    po._FITTERS.clear()
    sc37, kw37 = _fop_args(37)
    odd = po.find_optimal_pose(mask=sc37["mask"].numpy(), num_iterations=4, **kw37)
    fitter = next(iter(po._FITTERS.values()))
    assert fitter.size == 37 and fitter.fits == 1 and odd.image_size == 37
    assert torch.isfinite(odd.rotations).all() and torch.isfinite(sum(odd()[0].values())).all()
    po._FITTERS.clear()


def test_sigma_schedule(monkeypatch):
    """decay 0.9, floor 3e-4 from 1e-3: after 5 and 20 fused steps the device sigma equals the float32 sequence of the host bit for
    bit; restart() restores the start; the graph and eager loops end at the same bits; the schedule changes the fit; the module
    find_optimal_pose returns carries the blur its fit ended with."""
    from homan_amd import pose_optimization as po
    sched = dict(sil_sigma_decay=0.9, sil_sigma_min=3e-4)
    seq = ref.anneal_sequence(1e-3, 0.9, 3e-4, 20)
    assert seq[20] == np.float32(3e-4) and seq[5] > np.float32(3e-4)
    bits = lambda m: np.float32(m.sil_sigma.item())
    m = _module(32, 1e-3, **sched)
    loop = po._FusedPoseLoop(m, 1e-2)
    loop.run(5)
    assert bits(m) == seq[5]
    loop.run(15)
    assert bits(m) == seq[20]
    loop.restart()
    assert bits(m) == np.float32(1e-3)
    loop.release()
    fused5 = _module(32, 1e-3, **sched)
    po._fused_loop(fused5, 1e-2, 5)
    for run in (po._graph_loop, po._host_loop):
        other = _module(32, 1e-3, **sched)
        run(other, 1e-2, 5)
        assert bits(other) == seq[5], run.__name__
        _same_step(sum(fused5()[0].values()).detach(), fused5, sum(other()[0].values()).detach(), other, run.__name__)
    still = _module(32, 1e-3)
    po._fused_loop(still, 1e-2, 5)
    assert bits(still) == np.float32(1e-3) and not torch.equal(still.rotations, fused5.rotations)
    sc, kw = _fop_args(32)
    for resident in ("1", "0"):
        monkeypatch.setenv("HOMAN_POSE_FITTER", resident)
        po._FITTERS.clear()
        for _ in range(2):                       # (a resident fitter's second fit starts from sil_sigma again)
            out = po.find_optimal_pose(mask=sc["mask"].numpy(), num_iterations=5, sil_sigma=1e-3, **sched, **kw)
            assert bits(out) == seq[5]
    po._FITTERS.clear()


def test_find_optimal_poses_in_soft_mode():
    """the clip wrapper over 2 frames in soft mode: the documented keys and shapes, finite; with the default keywords its outputs
    equal a call that names sil_mode="nmr", bit for bit"""
    from homan_amd import pose_optimization as po
    S = 64
    sc, kw = _fop_args(S)
    ann = {"target_crop_mask": sc["mask"].numpy(), "bbox": kw["bbox"], "square_bbox": kw["square_bbox"], "full_mask": torch.zeros(8, 8)}
    sampler = po.compute_random_rotations
    po.compute_random_rotations = lambda B=10, *a, **k: sc["rots"].clone().to("cuda")
    po._FITTERS.clear()
    call = lambda **more: po.find_optimal_poses((S, S), faces=sc["faces"], vertices=sc["mesh"], annotations=[ann, ann],
                                                Ks=[kw["K"], kw["K"]], num_iterations=4, num_initializations=4, rend_size=S, **more)
    try:
        soft = call(sil_mode="soft", sil_sigma=1e-3, sil_sigma_decay=0.8)
        fitter = next(iter(po._FITTERS.values()))
        assert len(po._FITTERS) == 1 and fitter.fits == 2 and fitter.shell.sil_mode == "soft"
        plain, named = call(), call(sil_mode="nmr")
    finally:
        po.compute_random_rotations = sampler
        po._FITTERS.clear()
    V = sc["mesh"].shape[0]
    for h in soft:
        assert set(h) == {"rotations", "translations", "verts_trans", "target_masks", "K_roi", "masks", "verts", "full_mask"}
        assert tuple(h["rotations"].shape) == (1, 3, 3) and tuple(h["translations"].shape) == (1, 1, 3)
        assert tuple(h["verts_trans"].shape) == (1, V, 3) and tuple(h["target_masks"].shape) == (1, S, S)
        assert tuple(h["K_roi"].shape) == (1, 1, 3, 3)
        assert all(torch.isfinite(h[k]).all() for k in ("rotations", "translations", "verts_trans"))
    for p, q in zip(plain, named):
        assert all(torch.equal(p[k], q[k]) for k in p)
