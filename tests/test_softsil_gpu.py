"""Soft silhouette mode on the GPU: the kernels of csrc/softsil.hip against the float64 restatement (tests/softsil_ref.py), their
determinism and argument checks, and the mode through model, loops and ClipFitter.

Bars.  Kernel and restatement get the SAME float32 vertices, K and sigma.  Forward: 4 x the largest difference between the
restatement run in float32 and in float64 on those inputs (projection included; the factor allows for another operation order)
+ 1e-6 (8 ulp of 1.0: pixel-face pairs that rounding puts on either side of the cutoff, 1.13e-7 each).  Backward: 4 x the
float32-vs-float64 difference of the restatement's gradient, relative to the largest gradient entry.  Every case prints its
figures before it asserts."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import softsil_ref as ref

pytestmark = pytest.mark.gpu

# (S, F, B, sigma): S 16 = one tile, 40 = off every power-of-two grid (edge tiles masked), 64 = several tiles; F across the
# 64-lane and the 256-entry chunk; sigma 1e-4 sub-pixel, 4e-3 = cutoff radius 0.25 NDC (footprints span tiles)
CASES = [(16, 1, 1, 1e-4), (16, 12, 3, 4e-3), (40, 12, 1, 1e-4), (40, 65, 3, 4e-3), (64, 65, 1, 1e-4), (40, 300, 3, 4e-3),
         (64, 300, 1, 1e-4), (64, 12, 3, 4e-3), ("soup", 40, 1e-4), ("soup", 40, 4e-3), ("soup", 64, 4e-3)]


def _mesh(F):
    from homan_amd import synth
    if F <= 12:
        v, f = synth.box_mesh(1, 1, 1, scale=0.2)           # the cube: 12 faces
    else:
        v, f = synth.bottle_mesh(segments=10, rings=15, scale=0.2)      # 300 faces
    return torch.from_numpy(v).float(), torch.from_numpy(f[:F].astype(np.int64))


def _rot(gen):
    q = torch.randn(4, generator=gen, dtype=torch.float64)
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def _soup():
    """hand-made faces, two frames: a plain face; an off-screen face; a face across the near plane; an exactly degenerate face;
    a face covering the whole image in frame 0, behind the near plane in frame 1 - where the top-right tile is then reached by
    no face (the plain face stays 0.7 NDC away, beyond either cutoff radius)"""
    uv = torch.tensor([[-0.6, -0.5], [-0.1, -0.4], [-0.4, 0.1],                  # 0-2 plain
                       [3.0, 3.0], [4.0, 3.0], [3.0, 4.0],                       # 3-5 off-screen
                       [0.2, -0.8], [0.7, -0.7], [0.5, -0.2],                    # 6-8 across the near plane (vertex 6)
                       [0.3, 0.3], [0.3, 0.3], [0.6, 0.5],                       # 9-11 degenerate (two corners on one point)
                       [-3.0, -3.0], [9.0, -3.0], [-3.0, 9.0]])                  # 12-14 covers the image
    z = torch.ones(2, 15)
    z[:, 6] = 0.05
    z[1, 12:] = 0.01
    verts = torch.stack([uv[None, :, 0] * z / 2, -uv[None, :, 1] * z / 2, z], -1).float()
    K = torch.tensor([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]).expand(2, 3, 3).contiguous()
    return verts, torch.arange(15).reshape(5, 3), K


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs (float32, host) and the restatement's float64 / float32 images and gradients, computed once per case"""
    gen = torch.Generator().manual_seed(100 + CASES.index(case))
    if case[0] == "soup":
        _, S, sigma = case
        verts, faces, K = _soup()
    else:
        S, F, B, sigma = case
        mesh, faces = _mesh(F)
        verts = torch.stack([(mesh.double() @ _rot(gen).T + torch.tensor([0.03 * b, -0.02 * b, 0.6 + 0.05 * b])).float()
                             for b in range(B)])
        K = torch.tensor([[1.2, 0.02, 0.5], [0.0, 1.15, 0.52], [0.0, 0.0, 1.0]]).expand(B, 3, 3).contiguous()
    sigma = float(np.float32(sigma))                   # the value the kernel reads, for the float64 run too
    up = torch.randn(verts.shape[0], S, S, generator=gen)
    a64, g64 = ref.alpha_and_grad(verts, faces, K, S, sigma, up, torch.float64)
    a32, g32 = ref.alpha_and_grad(verts, faces, K, S, sigma, up, torch.float32)
    return dict(verts=verts, faces=faces, K=K, S=S, sigma=sigma, up=up, a64=a64, g64=g64, a32=a32, g32=g32)


def _run(c, twice=False):
    from homan_amd import ops
    dev = torch.device("cuda")
    verts = c["verts"].to(dev).requires_grad_(True)
    B, V = verts.shape[:2]
    sctx = ops.SoftSilhouetteContext(c["faces"][None].expand(B, -1, -1).to(dev), V, B, c["S"], dev)
    sigma = torch.tensor([c["sigma"]], device=dev)
    out = []
    for _ in range(2 if twice else 1):
        verts.grad = None
        alpha = ops.soft_silhouette_render(verts, c["K"].to(dev), sctx, sigma)
        (alpha * c["up"].to(dev)).sum().backward()
        out.append((alpha.detach().cpu(), verts.grad.detach().cpu()))
    return out


@pytest.mark.parametrize("case", CASES, ids=str)
def test_forward_and_backward_match_the_restatement(case):
    c = _case(case)
    (alpha, grad), = _run(c)
    ref_diff = float((c["a32"].double() - c["a64"]).abs().max())
    err = float((alpha.double() - c["a64"]).abs().max())
    gmax = float(c["g64"].abs().max())
    gref_diff = float((c["g32"].double() - c["g64"]).abs().max()) / gmax
    gerr = float((grad.double() - c["g64"]).abs().max()) / gmax
    print(f"softsil {case}: image restatement f32-f64 {ref_diff:.3e} kernel {err:.3e} | gradient (of max {gmax:.3e}) "
          f"restatement {gref_diff:.3e} kernel {gerr:.3e}")
    assert gmax > 0 and float(c["g64"][..., 2].abs().max()) > 0           # the z components are part of the check
    assert torch.isfinite(alpha).all() and torch.isfinite(grad).all()
    assert err <= ref.RULE_FACTOR * ref_diff + ref.IMAGE_ABS
    assert gerr <= ref.RULE_FACTOR * gref_diff


def test_soup_edge_faces():
    """what the hand-made faces are there for, stated on the kernel's own output"""
    c = _case(("soup", 40, 4e-3))
    (alpha, grad), = _run(c)
    assert float(alpha[0].min()) == 1.0                      # frame 0: the covering face, deep inside everywhere
    assert float(alpha[1, :16, 32:].abs().max()) == 0.0      # frame 1: the tile no face reaches
    assert float(alpha[1].max()) > 0.99                      # ... while the plain face is there
    assert float(grad[:, 3:12].abs().max()) == 0.0           # off-screen, near-plane and degenerate faces: zero gradient
    assert float(grad[1, 12:].abs().max()) == 0.0 and float(grad[1, :3].abs().max()) > 0


@pytest.mark.parametrize("case", [(40, 65, 3, 4e-3), (64, 300, 1, 1e-4), ("soup", 40, 4e-3)], ids=str)
def test_two_calls_agree_bit_for_bit(case):
    (a0, g0), (a1, g1) = _run(_case(case), twice=True)
    assert torch.equal(a0, a1) and torch.equal(g0, g1)


def test_bad_arguments_leave_the_outputs_untouched():
    from homan_amd import lib, ops
    L, P, dev = lib.lib(), lib.ptr, torch.device("cuda")
    c = _case((16, 12, 3, 4e-3))
    B, V, F, S = 3, c["verts"].shape[1], 12, 16
    verts, K, faces = c["verts"].to(dev), c["K"].to(dev), c["faces"].to(dev, torch.int32).contiguous()
    sctx = ops.SoftSilhouetteContext(c["faces"][None].expand(B, -1, -1).to(dev), V, B, S, dev)
    sigma = torch.tensor([c["sigma"]], device=dev)
    alpha = torch.full((B, S, S), 7.5, device=dev)
    gverts = torch.full((B, V, 3), 7.5, device=dev)
    up = c["up"].to(dev)
    fwd = lambda B=B, F=F, S=S, out=alpha: L.hm_softsil_fwd(P(verts), P(faces), P(K), B, V, F, S, 1.0, ops.NMR_NEAR, ops.NMR_FAR,
                                                            P(sigma), P(out), P(sctx.workspace), lib.stream())
    bwd = lambda B=B, F=F, S=S, out=gverts: L.hm_softsil_bwd(P(verts), P(faces), P(K), B, V, F, S, 1.0, ops.NMR_NEAR, ops.NMR_FAR,
                                                             P(sigma), P(alpha), P(up), P(sctx.adj_off), P(sctx.adj_items),
                                                             P(out), P(sctx.workspace), lib.stream())
    for call in (fwd, bwd):
        assert call(S=0) == -1 and call(F=0) == -1 and call(out=None) == -1 and call(B=0) == -1 and call(S=4097) == -1
    torch.cuda.synchronize()
    assert bool((alpha == 7.5).all()) and bool((gverts == 7.5).all())
    assert fwd() == 0 and bwd() == 0                        # (and the same arguments, unspoilt, are accepted)
    torch.cuda.synchronize()
    assert not bool((alpha == 7.5).any()) and not bool((gverts == 7.5).any())


# ---------------------------------------------------------------- model, loops, ClipFitter
def _clip(mano, seed, frames=3, rend=32, image=64):
    from homan_amd import synth
    sil_fn, hand_fn = synth.hip_clip_fns(mano)
    return synth.make_clip(seed=seed, frames=frames, rend_size=rend, image_size=image, obj="cube", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn)


def _model(mano, clip, rend=32, image=64, sync=True, **kw):
    from homan_amd.jointopt import build_model
    return build_model(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                       objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"], optimize_mano=True,
                       image_size=image, mano_model=mano, rend_size=rend, sync_metrics=sync, **kw)


def test_model_forward_uses_the_soft_image(mano_model):
    from homan_amd import synth
    lw = dict(synth.STEP1_LOSS_WEIGHTS)
    clip = _clip(mano_model, 51)
    soft, hard = _model(mano_model, clip, sil_mode="soft"), _model(mano_model, clip)
    assert soft.sil_mode == "soft" and hard.sil_mode == "nmr" and abs(float(soft.sil_sigma) - 1e-4) < 1e-10
    ld, md = soft(loss_weights=lw)
    ld_h, md_h = hard(loss_weights=lw)
    assert set(ld) == set(ld_h) and set(md) == set(md_h) and set(soft.state_dict()) == set(hard.state_dict())
    assert tuple(ld["loss_sil_obj"].shape) == (1,) and tuple(soft.losses.last_silhouettes.shape) == (3, 32, 32)
    # the expression of homan_amd.losses (reference losses.py:189-196) on the restatement's image, in float64
    verts = soft.get_verts_object()[0].detach().cpu()
    faces, K = soft.faces_object[0].cpu().long(), soft.camintr_rois_object.cpu()
    sigma = float(soft.sil_sigma)
    a64 = ref.soft_silhouette(verts.double(), faces, K, 32, sigma)
    a32 = ref.soft_silhouette(verts, faces, K, 32, sigma)
    e = 4 * float((a32.double() - a64).abs().max()) + 1e-6            # the forward bar, per pixel
    keep, tgt = soft.keep_mask_object.cpu().double(), soft.ref_mask_object.cpu().double()
    image = keep * a64
    loss = ((image - tgt) ** 2).sum() / keep.sum() / 3
    # |d (i - t)^2| <= 2 |i - t| e + e^2 per kept pixel; the float32 evaluation of the expression itself: 1e-6 relative
    loss_bar = float((keep * (2 * (image - tgt).abs() * e + e * e)).sum() / keep.sum() / 3) + 1e-6 * float(loss)
    inter, union = (image * tgt).sum((1, 2)), (image + tgt).clamp(0, 1).sum((1, 2))
    iou = inter / (union + 1e-6)
    # inter moves by at most e sum(t), union by at most e sum(keep): first-order quotient bound with the smaller denominator
    d_iou = (e * tgt.sum((1, 2)) + iou * e * keep.sum((1, 2))) / (union - e * keep.sum((1, 2)))
    iou_bar = float(d_iou.mean()) + 1e-6
    got_loss, got_iou = float(ld["loss_sil_obj"]), float(md["iou_object"])
    print(f"softsil model: loss {got_loss:.9e} vs {float(loss):.9e} (bar {loss_bar:.3e}); iou {got_iou:.9e} vs "
          f"{float(iou.mean()):.9e} (bar {iou_bar:.3e})")
    assert abs(got_loss - float(loss)) <= loss_bar
    assert abs(got_iou - float(iou.mean())) <= iou_bar
    np.testing.assert_allclose(soft.losses.last_silhouettes.cpu().double().numpy(), a64.numpy(), atol=e, rtol=0)
    # ... and the term reaches the object's depth: the translation's z gets a silhouette gradient
    only_sil = dict({k: 0.0 for k in lw}, lw_sil_obj=1.0)
    ld, _ = soft(loss_weights=only_sil)
    ld["loss_sil_obj"].sum().backward()
    assert float(soft.translations_object.grad[..., 2].abs().max()) > 0


def _fit(mano, clip, lw, steps, mode, **kw):
    from homan_amd.jointopt import optimize_hand_object
    return optimize_hand_object(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                                objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"],
                                loss_weights=lw, num_iterations=steps, optimize_mano=True, image_size=64, mano_model=mano,
                                rend_size=32, mode=mode, **kw)[:2]


def _close_as_the_two_loops(evo, want):
    """the comparison of tests/test_model_gpu.py::test_short_trajectory_eager_and_graph, with its tolerances"""
    np.testing.assert_allclose(evo[0], want[0], rtol=1e-6)
    np.testing.assert_allclose(evo[:3], want[:3], rtol=2e-5)
    np.testing.assert_allclose(evo, want, rtol=0.01)


def test_loops_take_the_soft_mode(mano_model):
    from homan_amd import synth
    from homan_amd.jointopt import FusedStepper, ShardStepper
    lw = dict(synth.STEP1_LOSS_WEIGHTS)
    clip = _clip(mano_model, 52)
    model = _model(mano_model, clip, sync=False, sil_mode="soft", sil_sigma=1e-3)
    with pytest.raises(NotImplementedError):
        FusedStepper(model, lw, 1e-2, 6)
    with pytest.raises(NotImplementedError):
        ShardStepper([model], lw, 1e-2, 6)
    _, auto = _fit(mano_model, clip, lw, 6, "auto", sil_mode="soft", sil_sigma=1e-3)
    _, eager = _fit(mano_model, clip, lw, 6, "eager", sil_mode="soft", sil_sigma=1e-3)
    _, hard = _fit(mano_model, clip, lw, 6, "auto")
    assert len(auto["loss"]) == 6 and set(auto) == set(eager)
    _close_as_the_two_loops(auto["loss"], eager["loss"])
    assert abs(auto["loss_sil_obj"][0] - hard["loss_sil_obj"][0]) > 1e-6 * abs(hard["loss_sil_obj"][0])      # another image


def test_clip_fitter_walk_equals_solo_fits(mano_model):
    from homan_amd import synth
    from homan_amd.jointopt import ClipFitter
    lw = dict(synth.STEP1_LOSS_WEIGHTS)
    clips = [_clip(mano_model, s) for s in (53, 54)]
    fitter = ClipFitter(lw, num_iterations=6, optimize_mano=True, image_size=64, mano_model=mano_model, rend_size=32,
                        sil_mode="soft", sil_sigma=1e-3)
    results = fitter.fit(clips)
    assert fitter.timing["built"] == 1 and fitter.timing["reused"] == 1 and len(fitter.resident_graph) == 1
    for clip, res in zip(clips, results):
        model, evo = _fit(mano_model, clip, lw, 6, "auto", sil_mode="soft", sil_sigma=1e-3)
        for k, v in res["state_dict"].items():
            assert torch.equal(v, getattr(model, k).detach().cpu()), k
        assert torch.equal(res["verts_object"], model.get_verts_object()[0].detach().cpu())
        for k in evo:
            np.testing.assert_array_equal(np.asarray(res["loss_evolution"][k]), np.asarray(evo[k]), err_msg=k)


def test_sigma_changed_in_place_follows_the_replay(mano_model):
    from homan_amd import synth
    from homan_amd.jointopt import GraphStepper, parameter_groups
    lw = dict(synth.STEP1_LOSS_WEIGHTS)
    clip = _clip(mano_model, 55)
    kw = dict(sil_mode="soft", sil_sigma=2.5e-4)
    stepper = GraphStepper(_model(mano_model, clip, sync=False, **kw), lw, 1e-2, 4)
    stepper.run(2)
    stepper.model.sil_sigma.mul_(4)
    stepper.run(2)
    graph = stepper.loss_evolution(4)["loss"]
    model = _model(mano_model, clip, **kw)
    opt = torch.optim.Adam(parameter_groups(model, 1e-2))
    eager = []
    for step in range(4):
        if step == 2:
            model.sil_sigma.mul_(4)
        opt.zero_grad()
        ld, _ = model(loss_weights=lw)
        tot = sum(ld[k] * lw[k.replace("loss", "lw")] for k in ld)
        eager.append(tot.item())
        tot.sum().backward()
        opt.step()
    _close_as_the_two_loops(graph, eager)
    still = GraphStepper(_model(mano_model, clip, sync=False, **kw), lw, 1e-2, 4)      # the same fit with sigma left alone
    still.run(4)
    unchanged = still.loss_evolution(4)["loss"]
    np.testing.assert_array_equal(unchanged[:2], graph[:2])
    assert abs(unchanged[2] - graph[2]) > 1e-4 * abs(graph[2])
