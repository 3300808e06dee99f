"""Ordinal-depth row: the oracle's depth image and its backward, checked on the CPU.

The depth backward restates the NMR kernel from its published formula; here it is checked against torch autograd
(float64) of the forward depth formula on the samples the hard rasteriser assigned to each face.
"""
import numpy as np
import torch

from oracle import model as o_model
from oracle import nmr
from tests import util


def _two_triangles():
    # NDC faces (B=1, NF=2, 3, 3): a large slanted triangle and a smaller one in front of part of it
    f = torch.tensor([[[[-0.8, -0.7, 0.9], [0.7, -0.6, 0.5], [-0.1, 0.8, 0.7]],
                       [[-0.3, -0.2, 0.45], [0.5, -0.3, 0.40], [0.1, 0.5, 0.42]]]], dtype=torch.float32)
    return f


def _depth_f64(faces, idx, size):
    """depth image recomputed in float64 from the (differentiable) faces, ownership fixed to `idx`."""
    B, NF = faces.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(size, dtype=torch.float64), torch.arange(size, dtype=torch.float64),
                            indexing="ij")
    out = torch.full((B, size, size), 100.0, dtype=torch.float64)
    for b in range(B):
        for fn in range(NF):
            sel = idx[b] == fn
            if not sel.any():
                continue
            p = 0.5 * (faces[b, fn, :, :2] * size + size - 1)
            M = torch.cat([p, torch.ones(3, 1, dtype=torch.float64)], 1).T            # columns = vertices
            w = torch.linalg.solve(M, torch.stack([xs[sel], ys[sel], torch.ones_like(xs[sel])]))   # (3, n)
            zp = 1.0 / (w / faces[b, fn, :, 2:3]).sum(0)
            out[b][sel] = zp
    return out


def test_depth_backward_matches_autograd_of_forward_formula():
    size = 32
    faces = _two_triangles().requires_grad_(True)
    alpha, depth, idx = nmr._RasterizeAlphaDepth.apply(faces, size, 0.1, 100.0, 1e-3)
    g = torch.from_numpy(np.random.default_rng(0).normal(size=tuple(depth.shape)).astype(np.float32))
    (depth * g).sum().backward()
    got = faces.grad.clone()

    f64 = faces.detach().double().requires_grad_(True)
    d64 = _depth_f64(f64, idx, size)
    assert torch.allclose(d64.float(), depth.detach(), rtol=1e-5, atol=1e-6)
    (d64 * g.double()).sum().backward()
    want = f64.grad.float()
    # interior samples only enter (both triangles lie inside the image, clamps inactive away from edges): the
    # analytic backward equals the true derivative up to the edge samples whose barycentrics were clamped
    assert torch.allclose(got, want, rtol=2e-2, atol=2e-2 * want.abs().max()), (got, want)


def test_ordinal_depth_loss_counts_pairs_like_the_reference():
    B, S = 3, 8
    d0 = torch.full((B, S, S), 100.0)
    d1 = torch.full((B, S, S), 100.0)
    s0 = torch.zeros(B, S, S, dtype=torch.bool)
    s1 = torch.zeros(B, S, S, dtype=torch.bool)
    s0[:2, 2:6, 2:6] = True
    s1[1:, 4:8, 4:8] = True
    d0[s0] = 0.6
    d1[s1] = 0.5                                   # layer 1 in front where both render
    masks = torch.zeros(B, 2, S, S, dtype=torch.bool)
    masks[:, 0, 2:6, 2:6] = True                   # annotation: layer 0 owns the overlap
    out = o_model.compute_ordinal_depth_loss(masks, [s0, s1], [d0, d1])["loss_depth"]
    # pairs: (0,0): 2 frames, (1,1): 2 frames, (0,1) and (1,0): frame 1 only -> 6
    want = np.log1p(np.exp(0.1)) / 6.0
    assert abs(float(out) - want) < 1e-6


# ------------------------------------------------------------------ the float64 references of tests/util.py vs the oracle
def _oracle_ordinal(sc):
    d = [torch.from_numpy(x).clone().requires_grad_(True) for x in sc["d"]]
    masks = torch.stack([torch.from_numpy(x) != 0 for x in sc["m"]], 1)
    loss = o_model.compute_ordinal_depth_loss(masks, [torch.from_numpy(x) == 1 for x in sc["a"]], d)["loss_depth"]
    if loss.requires_grad and bool(torch.isfinite(loss)):
        loss.backward()
    return loss.detach(), [x.grad if x.grad is not None else torch.zeros_like(x) for x in d]


def test_ordinal_depth_ref_matches_the_oracle():
    """util.ordinal_depth_ref (float64) against oracle.model.compute_ordinal_depth_loss (float32) on every synthetic clip the
    GPU tests use: value and both gradient images.  The largest deviation is the float32 noise floor util.E32_ORDINAL."""
    worst = 0.0
    for B, S, kind in util.ORDINAL_CASES + [(6, 64, "three_layers")]:
        sc = util.ordinal_scene3(B, S) if kind == "three_layers" else util.ordinal_scene(B, S, kind)
        if kind != "full_clamped":
            util.assert_ordinal_scene_has_no_near_ties(sc)
        want, gw = util.ordinal_ref_on_scene(sc)
        got, gg = _oracle_ordinal(sc)
        assert float(want) > 0
        devs = [util.deviation(got.numpy(), want.numpy())] + [util.deviation(a.numpy(), b.numpy()) for a, b in zip(gg, gw)]
        print(f"ordinal B={B} S={S} {kind}: loss {float(want):.9g} e32 value {devs[0]:.3e} gradients", *(f"{x:.3e}" for x in devs[1:]))
        assert (kind == "full_clamped") == (not gw[0].any())          # clamped everywhere: no gradient at all
        for a, b in zip(gg, gw):                                       # the same pixels carry a gradient (the bounds included)
            assert torch.equal(a != 0, b != 0)
        worst = max(worst, *devs)
    assert 0.5 * util.E32_ORDINAL < worst <= util.E32_ORDINAL, worst


def test_ordinal_depth_ref_at_the_clamp_bounds_and_without_pairs():
    """Row 0 of a mixed scene holds x = ORD_BOUND_X in turn: torch's clamp passes the gradient for 0 < x <= 2 (bounds inclusive,
    x = 0 is not wrongly ordered), reference and oracle alike; a clip without a covered pixel gives 0 / 0 in both."""
    sc = util.ordinal_scene(1, 64, "mixed")
    _, gw = util.ordinal_ref_on_scene(sc)
    _, gg = _oracle_ordinal(sc)
    x = np.asarray(util.ORD_BOUND_X, np.float32)[np.arange(64) % len(util.ORD_BOUND_X)]
    want_nz = torch.from_numpy((x > 0) & (x <= 2))
    assert want_nz[3] and x[3] == 2.0                                  # x == 2.0 exactly carries a gradient
    for g in (gw, gg):
        assert torch.equal(g[0][0, 0] > 0, want_nz) and torch.equal(g[1][0, 0] < 0, want_nz)
        assert torch.equal(g[1][0, 1] > 0, want_nz) and torch.equal(g[0][0, 1] < 0, want_nz)
    sc = util.ordinal_scene(4, 64, "no_pairs")
    assert torch.isnan(util.ordinal_ref_on_scene(sc)[0]) and torch.isnan(_oracle_ordinal(sc)[0])


def test_depth_backward_ref_matches_the_oracle():
    """util.depth_backward_ref (float64) against the oracle's depth-image backward (projection + _RasterizeAlphaDepth, float32)
    over the mesh x size grid of the GPU test, for a dense, a banded and (small meshes) a late-frames upstream image.  The largest
    deviation is the float32 noise floor util.E32_DEPTH_BWD."""
    worst = 0.0
    for dims, (V, B) in util.DEPTH_BWD_MESHES.items():
        for S in util.DEPTH_BWD_SIZES:
            for near in ((False, True) if V == 8 and S > 64 else (False,)):
                verts, faces, K = util.depth_bwd_scene(dims, B, near)
                assert verts.shape[1] == V
                for pat in ("dense", "band", "late_frames"):
                    g = util.depth_bwd_upstream(pat, B, S, V)
                    if g is None or (pat == "late_frames" and S == 256):
                        continue
                    got, f9, idx = util.oracle_depth_backward(verts, faces, K, S, g)
                    want = util.depth_backward_ref(f9, idx, g, faces, verts.numpy(), K.numpy(), 1.0)
                    assert np.abs(want).max() > 0
                    dev = util.deviation(got, want)
                    print(f"depth bwd V={V} B={B} S={S} near={near} {pat}: e32 {dev:.3e}")
                    worst = max(worst, dev)
    assert 0.5 * util.E32_DEPTH_BWD < worst <= util.E32_DEPTH_BWD, worst
