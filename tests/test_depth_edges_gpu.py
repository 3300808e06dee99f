"""Depth term, the kernels of csrc/raster_depth.hip at the shapes and edges the rest of the suite does not reach: small meshes
(a gather workgroup over many frames), long clips, sizes off the 64 grid, absent layers, the clamp's bounds, three layers.

Every comparison is against the float64 references of tests/util.py (checked against the CPU oracle in
tests/test_depth_oracle.py), at util.E32_FACTOR times the float32 noise floor measured there (util.E32_ORDINAL,
util.E32_DEPTH_BWD): deviation = max |difference| / max |reference| per output tensor, no element exempt.  Claims of identity
(sparse == dense, second call == first call, flags) are torch.equal.
"""
import copy

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG = -1          # HM_ERR_BAD_ARG of csrc/hm_common.h


def _box_rows(sctx):
    """pixel rows spanned by the sample box of every face with a box (hm_sil_read_boxes, layout as SilhouetteContext.calibrate)"""
    from homan_amd import lib as hlib
    raw = torch.empty(sctx.B * sctx.F * 8, dtype=torch.uint8, device=DEV)
    hlib.check(hlib.lib().hm_sil_read_boxes(hlib.ptr(sctx.workspace), sctx.B, sctx.V, sctx.F, sctx.S, hlib.ptr(raw), hlib.stream()),
               "hm_sil_read_boxes")
    bx = raw.cpu().numpy().view(np.uint16).reshape(sctx.B, sctx.F, 4).astype(np.int64)
    valid = (bx[..., 0] >> 14) != 0
    is_ = 2 * sctx.S
    return (((is_ - 1 - bx[..., 1]) >> 1) - ((is_ - 1 - bx[..., 3]) >> 1))[valid]


def _depth_bwd(sctx, verts, K, g, flags):
    from homan_amd import lib as hlib
    out = torch.full((sctx.B, sctx.V, 3), 7.0, device=DEV)           # sentinel: every element must be written
    hlib.check(hlib.lib().hm_depth_bwd_sparse(hlib.ptr(verts), hlib.ptr(K), sctx.B, sctx.V, sctx.F, sctx.S, 1.0, hlib.ptr(g),
                                              hlib.ptr(sctx.adj_off), hlib.ptr(sctx.adj_items), hlib.ptr(out),
                                              hlib.ptr(flags) if flags is not None else None, hlib.ptr(sctx.workspace),
                                              hlib.stream()), "depth bwd")
    return out


_A_CASES = [(dims, S, False) for dims in util.DEPTH_BWD_MESHES for S in util.DEPTH_BWD_SIZES] + [((1, 1, 1), 128, True),
                                                                                               ((1, 1, 1), 256, True)]


@pytest.mark.parametrize("dims,S,near", _A_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_depth_backward_sparse_dense_and_reference(dims, S, near):
    """A. hm_depth_bwd_sparse with the flags of the upstream image == without them (hm_depth_bwd) == util.depth_backward_ref, for
    boxes of 8 .. 252 vertices (a 256-thread gather workgroup over 1 .. 32 frames), S = 64 / 128 / 256 (1 / 2 / 4 flag segments a
    row), faces lower and taller than 64 pixel rows, and upstream images that are zero, dense, one pixel of the last frame, only
    frames that are the ninth or later of a workgroup, only the last segment of the rows, a band of rows."""
    from homan_amd import ops
    V, B = util.DEPTH_BWD_MESHES[dims]
    verts, faces, K = util.depth_bwd_scene(dims, B, near)
    assert verts.shape == (B, V, 3)
    vd, Kd = verts.to(DEV).contiguous(), K.to(DEV).contiguous()
    sctx = ops.SilhouetteContext(torch.from_numpy(faces)[None].repeat(B, 1, 1).to(DEV), V, B, S, DEV)
    with torch.no_grad():
        sil, _ = ops.depth_render(vd, Kd, sctx, 1.0)
    assert bool((sil == 1).flatten(1).any(1).all())                  # the box is in every frame
    f9, idx = sctx.faces9().cpu().numpy(), sctx.idx_map().cpu().numpy()
    # the branches this case is here for
    spans = [min(256 * w + 255, B * V - 1) // V - 256 * w // V + 1 for w in range((B * V + 255) // 256)]     # frames per workgroup
    assert len(spans) >= 2
    if V <= 26:
        assert 255 // V >= 8 and max(spans) >= 9                     # no per-frame scan: every vertex is gathered
    elif V < 252:
        assert 2 <= min(spans[:-1]) and max(spans) <= 8 and (V != 44 or max(spans) >= 5)      # the per-frame scan, 2 .. 8 frames
    rows = _box_rows(sctx)
    if near:
        assert rows.max() >= 64                                      # boxes too tall for the flag test: walked regardless
    elif S == 64:
        assert rows.max() < 64
    rng = np.random.default_rng(7)
    seen = 0
    for pattern in util.DEPTH_BWD_PATTERNS:
        g_np = util.depth_bwd_upstream(pattern, B, S, V)
        if g_np is None:
            assert V > 26 and pattern == "late_frames"
            continue
        seen += 1
        g = torch.from_numpy(g_np).to(DEV)
        flags = (g.reshape(B, S, S // 64, 64) != 0).any(-1).to(torch.uint8).contiguous()      # as hm_ordinal_depth_bwd_flags does
        extra = torch.maximum(flags, torch.from_numpy((rng.random(tuple(flags.shape)) < 0.1).astype(np.uint8)).to(DEV))
        dense = _depth_bwd(sctx, vd, Kd, g, None)
        for fl in (flags, extra.contiguous()):                       # (a byte may be set over an all-zero segment)
            assert torch.equal(_depth_bwd(sctx, vd, Kd, g, fl), dense), pattern
        zero_frames = torch.from_numpy(~g_np.reshape(B, -1).any(1)).to(DEV)
        assert not dense[zero_frames].any(), pattern                 # exact zeros
        want = util.depth_backward_ref(f9, idx, g_np, faces, verts.numpy(), K.numpy(), 1.0)
        live = np.abs(want).reshape(B, -1).max(1) > 0
        if pattern == "zero":
            assert not live.any() and not dense.any()
            continue
        assert live.any() and (pattern != "dense" or live.all()), pattern
        if pattern == "late_frames":
            assert live[8:].any() and not live[:8].any()
        if pattern == "last_frame_pixel":
            assert live[B - 1] and live.sum() == 1
        got = dense.cpu().numpy()
        assert ((np.abs(got).reshape(B, -1).max(1) > 0) == live).all(), pattern            # no frame dropped, none invented
        dev = util.deviation(got, want)
        print(f"depth bwd V={V} B={B} S={S} near={near} {pattern}: deviation {dev:.3e} (bar {util.E32_FACTOR * util.E32_DEPTH_BWD:.1e})")
        assert dev <= util.E32_FACTOR * util.E32_DEPTH_BWD, pattern
    assert seen == len(util.DEPTH_BWD_PATTERNS) - (V > 26)


def _to_dev(sc):
    return ([torch.from_numpy(x).to(DEV) for x in sc["d"]], [torch.from_numpy(x).to(DEV) for x in sc["a"]],
            [torch.from_numpy(x).to(DEV).contiguous() for x in sc["m"]])


def _ordinal_raw(d, a, m, rws):
    """the C entry points themselves: forward -> (loss, rec), backward with upstream 1 and flags -> (rc, g0, g1, f0, f1)"""
    from homan_amd import lib as hlib
    L, P = hlib.lib(), hlib.ptr
    B, S = d[0].shape[:2]
    part, rec, out = torch.zeros(B * 8, device=DEV), torch.empty(5, device=DEV), torch.empty(1, device=DEV)
    hlib.check(L.hm_ordinal_depth_fwd(P(d[0]), P(d[1]), P(a[0]), P(a[1]), P(m[0]), P(m[1]), B, S, P(part), P(rec), P(out),
                                      P(rws.buf), hlib.stream()), "hm_ordinal_depth_fwd")
    assert not part.any()                                            # the frame records are re-armed
    up = torch.ones(1, device=DEV)
    g0, g1 = torch.full_like(d[0], 7.0), torch.full_like(d[1], 7.0)
    nseg = (S + 63) // 64
    f0 = torch.full((B, S, nseg), 9, dtype=torch.uint8, device=DEV)
    f1 = torch.full_like(f0, 9)
    rc = L.hm_ordinal_depth_bwd_flags(P(d[0]), P(d[1]), P(a[0]), P(a[1]), P(m[0]), P(m[1]), B, S, P(rec), P(up), P(g0), P(g1),
                                      P(f0), P(f1), hlib.stream())
    return out[0], rec, rc, g0, g1, f0, f1


@pytest.mark.parametrize("B,S,kind", util.ORDINAL_CASES)
def test_ordinal_loss_and_gradients_match_the_float64_reference(B, S, kind):
    """B. k_ordinal_depth / k_ordinal_depth_bwd vs util.ordinal_depth_ref: one frame, clips up to and beyond the 256 staged frame
    records, S = 1024 fully covered and clamped (the packed counts and the fixed-point sum at their largest), sizes off the 64
    grid, frames without one or both layers, silhouette values below 1, one direction empty, x on and around the clamp's bounds."""
    from homan_amd import ops
    sc = util.ordinal_scene(B, S, kind)
    if kind != "full_clamped":
        util.assert_ordinal_scene_has_no_near_ties(sc)
    want, gw = util.ordinal_ref_on_scene(sc)
    assert float(want) > 0
    d, a, m = _to_dev(sc)
    bar = util.E32_FACTOR * util.E32_ORDINAL
    rws = ops.ReduceWorkspace(DEV)
    results = []
    for _ in range(2):                                               # twice through the same workspace: self-resetting records
        dh = [x.clone().requires_grad_(True) for x in d]
        got = ops.ordinal_depth_loss(dh[0], dh[1], a[0], a[1], m[0], m[1], rws)
        got.backward()
        results.append((got.detach(), dh[0].grad, dh[1].grad))
    for x, y in zip(*results):
        assert torch.equal(x, y)
    got, g0, g1 = results[0]
    dev_v = util.deviation(got.cpu().numpy(), want.numpy())
    devs = [util.deviation(g.cpu().numpy(), w.numpy()) for g, w in zip((g0, g1), gw)]
    print(f"ordinal B={B} S={S} {kind}: loss {got.item():.9g} deviation value {dev_v:.3e} gradients {devs[0]:.3e} {devs[1]:.3e} (bar {bar:.1e})")
    # not vacuous, and the branch in question taken
    loss_raw, rec, rc, r0, r1, f0, f1 = _ordinal_raw(d, a, m, rws)
    assert loss_raw.item() == got.item()
    rec = rec.cpu().numpy()
    if kind == "mixed":
        assert rec[1] > 0 and rec[3] > 0 and gw[0].any() and gw[1].any()
        if B > 3:                                                    # frames 1 / 2 / 3 lack layer 0 / layer 1 / both
            frame_pairs = [4.0] * B
            frame_pairs[1], frame_pairs[2], frame_pairs[3] = 1.0, 1.0, 0.0
            assert rec[0] == sum(frame_pairs)
    elif kind == "one_direction":
        assert rec[1] > 0 and rec[3] == 0 and gw[0].any()
    else:
        assert rec[0] == 4 * B and rec[1] == B * S * S and rec[3] == 0 and not gw[0].any()      # 2^20 pixels a frame at S = 1024
    assert dev_v <= bar
    for g, w, dv in zip((g0, g1), gw, devs):
        assert torch.equal((g != 0).cpu(), w != 0)                   # the same pixels carry a gradient: the bounds included
        assert dv <= bar
    # the flags entry point: the same gradients, and flags == any(g != 0) per 64-pixel segment; off the 64 grid it refuses
    if S % 64 == 0:
        assert rc == 0 and torch.equal(r0, g0) and torch.equal(r1, g1)
        for gi, fi in ((r0, f0), (r1, f1)):
            assert torch.equal(fi, (gi.reshape(B, S, S // 64, 64) != 0).any(-1).to(torch.uint8))
    else:
        assert rc == BAD_ARG
        torch.cuda.synchronize()
        assert bool((r0 == 7.0).all()) and bool((f0 == 9).all())     # nothing was launched
        _, faces, _ = util.depth_bwd_scene((1, 1, 1), B)
        sctx = ops.SilhouetteContext(torch.from_numpy(faces)[None].repeat(B, 1, 1).to(DEV), 8, B, S, DEV)
        assert sctx.S % 64 != 0
        from homan_amd import lib as hlib
        P = hlib.ptr
        verts, K = torch.zeros(B, 8, 3, device=DEV), torch.zeros(B, 3, 3, device=DEV)
        gpd, out = torch.zeros(B, sctx.S, sctx.S, device=DEV), torch.full((B, 8, 3), 7.0, device=DEV)
        fl = torch.zeros(B, sctx.S, sctx.S // 64 + 1, dtype=torch.uint8, device=DEV)
        assert hlib.lib().hm_depth_bwd_sparse(P(verts), P(K), B, 8, sctx.F, sctx.S, 1.0, P(gpd), P(sctx.adj_off), P(sctx.adj_items),
                                              P(out), P(fl), P(sctx.workspace), hlib.stream()) == BAD_ARG
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())


def test_ordinal_gradient_at_the_clamp_bounds():
    """Rows 0 / 1 of a mixed scene hold x = util.ORD_BOUND_X in turn, layer 0 / layer 1 behind: the gradient passes for
    0 < x <= 2 - at x == 2.0 exactly too (torch.clamp's backward is inclusive), not at x = 0 and not beyond 2."""
    from homan_amd import ops
    sc = util.ordinal_scene(1, 64, "mixed")
    want, gw = util.ordinal_ref_on_scene(sc)
    d, a, m = _to_dev(sc)
    dh = [x.clone().requires_grad_(True) for x in d]
    ops.ordinal_depth_loss(dh[0], dh[1], a[0], a[1], m[0], m[1], ops.ReduceWorkspace(DEV)).backward()
    x = np.asarray(util.ORD_BOUND_X, np.float32)[np.arange(64) % len(util.ORD_BOUND_X)]
    passes = torch.from_numpy((x > 0) & (x <= 2))
    assert x[3] == 2.0 and passes[3] and not passes[4] and not passes[6]
    for r, (back, front) in enumerate(((0, 1), (1, 0))):
        assert torch.equal(gw[back][0, r] > 0, passes) and torch.equal(gw[front][0, r] < 0, passes)          # the reference itself
        assert torch.equal(dh[back].grad[0, r].cpu() > 0, passes), (r, dh[back].grad[0, r, :7])
        assert torch.equal(dh[front].grad[0, r].cpu() < 0, passes)
        np.testing.assert_allclose(dh[back].grad[0, r].cpu().numpy(), gw[back][0, r].numpy(), rtol=util.E32_FACTOR * util.E32_ORDINAL,
                                   atol=0)


def test_ordinal_loss_of_a_clip_without_pairs_is_the_references_nan():
    """no pixel fully covered in any frame: 0 / 0 in the reference and in the oracle (oracle/model.py) - and in the kernel"""
    from homan_amd import ops
    sc = util.ordinal_scene(4, 64, "no_pairs")
    want, _ = util.ordinal_ref_on_scene(sc)
    d, a, m = _to_dev(sc)
    rws = ops.ReduceWorkspace(DEV)
    for _ in range(2):
        got = ops.ordinal_depth_loss(d[0], d[1], a[0], a[1], m[0], m[1], rws)
        assert bool(torch.isnan(want)) and bool(torch.isnan(got))


def test_three_layers_match_the_float64_reference():
    """C. ops.ordinal_depth_loss_layers, n = 3: layers 1 and 2 never meet (that pair has no wrongly ordered pixel, and counts only
    its layers' own frames), layer 2 is absent from every other frame.  Value and the gradients of all three depth images."""
    from homan_amd import ops
    B, S = 6, 64
    sc = util.ordinal_scene3(B, S)
    util.assert_ordinal_scene_has_no_near_ties(sc)
    assert not ((sc["a"][1] == 1) & (sc["a"][2] == 1)).any() and not sc["a"][2][1::2].any() and (sc["a"][2][0::2] == 1).any()
    want, gw = util.ordinal_ref_on_scene(sc)
    assert float(want) > 0 and all(g.any() for g in gw)
    d, a, m = _to_dev(sc)
    dh = [x.clone().requires_grad_(True) for x in d]
    got = ops.ordinal_depth_loss_layers(dh, a, m, ops.ReduceWorkspace(DEV))
    got.backward()
    bar = util.E32_FACTOR * util.E32_ORDINAL
    devs = [util.deviation(got.detach().cpu().numpy(), want.numpy())] + [util.deviation(x.grad.cpu().numpy(), w.numpy())
                                                                          for x, w in zip(dh, gw)]
    print("ordinal three layers: deviation value %.3e gradients %.3e %.3e %.3e (bar %.1e)" % (*devs, bar))
    for x, w in zip(dh, gw):
        assert torch.equal((x.grad != 0).cpu(), w != 0)
    assert max(devs) <= bar, devs


def test_fused_loop_on_a_small_box_in_a_long_clip(mano_model):
    """D. An 8-vertex box over 12 frames, silhouette and depth term on: the object's depth backward is the flagged (sparse) call
    and one gather workgroup holds all 12 frames.  FusedStepper's iteration == HOMan.forward + autograd (dense depth backward):
    logged losses and every parameter gradient; the object's pose gradients of frames 8 .. 11 are not zero."""
    from homan_amd import HOMan, synth
    from homan_amd.jointopt import FusedStepper
    from oracle.jointopt import collate_inputs
    size, frames = 64, 12
    sil_fn, hand_fn = synth.hip_clip_fns(mano_model)
    ov, of = synth.box_mesh(1, 1, 1)
    assert ov.shape[0] == 8 and frames * 8 <= 256 and frames >= 9
    clip = synth.make_clip(seed=5, frames=frames, rend_size=size, image_size=size, obj=(ov, of), silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn)
    for pp, op in zip(clip["person_parameters"], clip["object_parameters"]):
        full = ((pp["masks"][0] > 0) | (op["full_mask"] > 0))
        op["full_mask"] = full.float()
        pp["masks"] = torch.zeros_like(pp["masks"])
        pp["translations"] = pp["translations"] + torch.tensor([0.06, 0.0, -0.02])    # hand over the object
    kw = collate_inputs(clip["person_parameters"], clip["object_parameters"], clip["objvertices"], clip["objfaces"])
    common = dict(camintr=clip["camintr"], class_name="default", int_scale_init=1, optimize_mano=True, image_size=size,
                  mano_model=mano_model, rend_size=size, sync_metrics=False)
    lw = dict(synth.STEP1_LOSS_WEIGHTS, lw_depth=2.0)
    assert lw["lw_sil_obj"] > 0
    # the depth term alone, through autograd: which frames of the object it reaches
    probe = HOMan(**copy.deepcopy(kw), ordinal_depth=True, **common)
    ld, _ = probe(loss_weights=dict({k: 0.0 for k in lw}, lw_depth=1.0))
    assert float(ld["loss_depth"].detach()) > 0
    ld["loss_depth"].sum().backward()
    for name in ("rotations_object", "translations_object"):
        rows = getattr(probe, name).grad.reshape(frames, -1).abs().max(1)[0]
        assert bool((rows[8:] > 0).all()), (name, rows)
    model = HOMan(**copy.deepcopy(kw), ordinal_depth=True, **common)
    loss_dict, _ = model(loss_weights=lw)
    assert float(loss_dict["loss_depth"].detach()) > 0
    total = sum(loss_dict[k] * lw[k.replace("loss", "lw")] for k in loss_dict)
    total.sum().backward()
    ref_grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    ref_losses = {k: float(v.detach().reshape(-1)[0]) for k, v in loss_dict.items()}
    for name in ("rotations_object", "translations_object"):
        assert bool((ref_grads[name].reshape(frames, -1).abs().max(1)[0][8:] > 0).all()), name
    st = FusedStepper(model, lw, 1e-2, 4, capture=False)
    assert st.d_flags is not None                                    # the sparse path
    st.forward_backward(log=True)
    torch.cuda.synchronize()
    for k, v in ref_losses.items():
        np.testing.assert_allclose(st.log_buf[0, 0, st.SLOTS.index(k)].item(), v, rtol=2e-6, atol=1e-9, err_msg=k)
    np.testing.assert_allclose(st.log_buf[0, 0, len(st.SLOTS)].item(), float(total.detach().reshape(-1)[0]), rtol=2e-6)
    for k, p in model.named_parameters():
        if k in ref_grads:
            scale = max(ref_grads[k].abs().max().item(), 1e-20)
            assert ((p.grad - ref_grads[k]).abs().max() / scale).item() < 2e-5, k
