"""The kernels of csrc/depthobs.hip (hm_depth_obs_fwd / _bwd), `ops.depth_obs_loss`, the term in `HOMan.forward` and in the loops.

Kernel against the fp32 NumPy restatement of tests/depthobs_ref.py: BIT FOR BIT (loss, records, metrics, gradient images, flags).
Model against the float64 closed form on the model's own renders: the bounds derived in tests/test_depthobs.py for values and
gradient images; for parameter gradients see _PARAM_BAR."""
import copy

import numpy as np
import pytest
import torch

from tests import depthobs_ref as dref
from tests import util
from tests.test_softsil_gpu import _clip, _close_as_the_two_loops, _fit, _model

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
U = dref.U32


def _dev(case):
    depths, sils, masks, D = case
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return [cu(d) for d in depths], [cu(a) for a in sils], [cu(m) for m in masks], cu(D)


def _run(case, delta, upstream=1.0):
    """-> dict like depthobs_ref.forward32 + grads, from ops.depth_obs_loss and its autograd backward"""
    from homan_amd import ops
    depths, sils, masks, D = _dev(case)
    depths = [d.requires_grad_() for d in depths]
    loss, mae, share, count, records = ops.depth_obs_loss(depths, sils, masks, D, delta, detail=True)
    assert loss.dim() == 0 and not mae.requires_grad and not share.requires_grad
    (loss * upstream).backward()
    return dict(loss=loss.detach().cpu().numpy(), mae=mae.cpu().numpy(), share=share.cpu().numpy(), N=count.cpu().numpy(),
                records=records.cpu().numpy(), grads=[d.grad.cpu().numpy() for d in depths])


def _same_bits(got, want, grads):
    for k in ("loss", "mae", "share", "N", "records"):
        assert np.asarray(got[k], F32).tobytes() == np.asarray(want[k], F32).tobytes(), (k, got[k], want[k])
    for l, (g, w) in enumerate(zip(got["grads"], grads)):
        assert g.tobytes() == w.tobytes(), f"gradient image of layer {l}"


# =============================================================================================== 1. kernel against the restatement
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("B, S", [(1, 16), (3, 48), (2, 64)])
def test_kernel_equals_the_restatement_bit_for_bit(B, S, L):
    delta = 0.03125                                   # (2^-5: the case holds residuals at exactly +-delta)
    case = dref.random_case(B, S, L, delta, seed=10 * S + L, empty_layer_frame=B * L > 1, rows=(S // 4, S // 2) if S == 64 else None)
    valid, _ = dref.valid_masks(*case)
    r0 = (case[0][0] - case[3])[valid[0]]
    assert (r0 == F32(delta)).any() and (r0 == -F32(delta)).any()
    assert B * L == 1 or not valid[L - 1][B - 1].any()                              # a (layer, frame) with no valid pixel
    want = dref.forward32(*case, delta)
    for up in (1.0, 0.7):
        got = _run(case, delta, up)
        _same_bits(got, want, dref.backward32(want, up)[0])
        assert all(np.isfinite(g).all() for g in got["grads"])
    again = _run(case, delta, 0.7)                                                    # two runs: the same bits
    _same_bits(again, got, got["grads"])
    print(f"B {B} S {S} L {L}: loss {float(got['loss']):.6e} mae {float(got['mae']):.6e} share {float(got['share']):.4f}")


def test_untuned_default_delta_and_odd_size():
    """delta = 0.03 (not a power of two) and an odd image size (element loads, a partial last group)"""
    for B, S, L, delta in ((2, 48, 2, 0.03), (2, 33, 3, 0.03), (1, 16, 3, 1.0)):
        case = dref.random_case(B, S, L, delta, seed=7)
        want = dref.forward32(*case, delta)
        _same_bits(_run(case, delta), want, dref.backward32(want)[0])


def test_a_clip_without_a_valid_pixel():
    case = dref.random_case(2, 48, 3, 0.03125, seed=3, empty_clip=True)
    got = _run(case, 0.03125)
    assert float(got["loss"]) == 0.0 and float(got["N"]) == 0.0 and float(got["mae"]) == 0.0 and not got["records"].any()
    assert all(not g.any() and np.isfinite(g).all() for g in got["grads"])
    want = dref.forward32(*case, 0.03125)
    _same_bits(got, want, dref.backward32(want)[0])


def test_a_frame_gives_the_same_bits_first_and_last():
    delta = 0.03
    depths, sils, masks, D = dref.random_case(3, 48, 2, delta, seed=11)
    a = _run((depths, sils, masks, D), delta)
    perm = [1, 2, 0]                                   # frame 0 goes last
    b = _run(([d[perm] for d in depths], [s[perm] for s in sils], [m[perm] for m in masks], D[perm]), delta)
    for k in ("loss", "mae", "share", "N"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["records"][:, perm].tobytes() == b["records"].tobytes()
    assert all(x[perm].tobytes() == y.tobytes() for x, y in zip(a["grads"], b["grads"]))


def test_backward_flags_equal_the_restatement():
    """hm_depth_obs_bwd with flags (S % 64 == 0): images as without, one byte per 64-pixel row segment"""
    from homan_amd import lib as hlib
    B, S, L, delta = 2, 64, 3, 0.03125
    case = dref.random_case(B, S, L, delta, seed=21, rows=(16, 32))
    want = dref.forward32(*case, delta)
    grads, flags = dref.backward32(want, 0.7)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    c = [cu(x) for x in want["clamped"]]
    rec, out, up = cu(want["records"]), cu(np.array([want["loss"], want["mae"], want["share"], want["N"]], F32)), cu(np.array([0.7], F32))
    g = [torch.full((B, S, S), float("nan"), device="cuda") for _ in range(L)]
    f = [torch.full((B * S * (S // 64),), 255, dtype=torch.uint8, device="cuda") for _ in range(L)]
    P = hlib.ptr
    hlib.check(hlib.lib().hm_depth_obs_bwd(P(c[0]), P(c[1]), P(c[2]), L, B, S, P(rec), P(out), P(up), P(g[0]), P(g[1]), P(g[2]),
                                           P(f[0]), P(f[1]), P(f[2]), hlib.stream()), "hm_depth_obs_bwd")
    for l in range(L):
        assert g[l].cpu().numpy().tobytes() == grads[l].tobytes()
        got = f[l].cpu().numpy().reshape(B, S, S // 64)
        assert np.array_equal(got, flags[l]) and got.any() and not got.all()


# =============================================================================================== scenes
def _compose(model):
    """(depth map (B,S,S), [instance mask per layer] bool) from the model's OWN per-layer renders: per pixel the nearest fully
    covered layer and its depth, 0 where no layer covers the pixel fully"""
    with torch.no_grad():
        renders = model.render_depth_layers(model.get_verts_object()[0], model.get_verts_hand()[0])
        sils = torch.stack([renders[l][0] for l in sorted(renders)])
        deps = torch.stack([renders[l][1] for l in sorted(renders)])
        cand = torch.where(sils == 1, deps, torch.full_like(deps, float("inf")))
        near, arg = cand.min(0)
        hit = torch.isfinite(near)
        return torch.where(hit, near, torch.zeros_like(near)).cpu(), [((arg == l) & hit).cpu() for l in range(sils.shape[0])]


def _with_depth(mano, clip, image=64, **kw):
    """the clip with instance masks and a depth map composed at its starting parameters -> (clip, depth_maps)"""
    D, masks = _compose(_model(mano, clip, image=image, **kw))
    clip = copy.deepcopy(clip)
    for b, (pp, op) in enumerate(zip(clip["person_parameters"], clip["object_parameters"])):
        op["full_mask"] = masks[0][b].float()
        pp["masks"] = torch.stack([m[b] for m in masks[1:]]).float()
    return clip, D


def _weights(**kw):
    from homan_amd import synth
    return dict({k: 0.0 for k in synth.STEP1_LOSS_WEIGHTS}, **kw)


def _param_grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


# per-pixel gradient images differ from float64 by at most 4u relative (tests/test_depthobs.py) + u for the cast of the float64
# image to the fp32 the depth backward takes = 5u; the depth backward and the pose chain behind it are LINEAR in the image and the
# same kernels on both sides, so the parameter gradients differ by that map applied to a per-pixel perturbation of relative size
# 5u and independent sign: it accumulates as sqrt(n) over the n valid pixels of a frame (n <= 64^2 here, taken at its bound, so
# sqrt(n) = 64), relative to the largest entry of the parameter's gradient; util.E32_FACTOR is the suite's margin on fp32 floors.
_PARAM_BAR = 5 * U * 64 * util.E32_FACTOR


def _model_against_float64(model, also=None):
    """loss, gradient images and every parameter's gradient of HOMan's term against depthobs_ref.reference64 on the model's own
    renders, pushed through the existing depth backward"""
    lw = _weights(lw_depth_obs=1.0)
    ids = model.depth_obs_layer_ids()
    # the reference: renders under autograd, float64 gradient images pushed through _DepthRender's backward
    model.zero_grad()
    vo, vh = model.get_verts_object()[0], model.get_verts_hand()[0]
    renders = model.render_depth_layers(vo, vh, ids)
    _, masks = model.depth_layers()
    host = lambda t: t.detach().cpu().numpy()
    r64 = dref.reference64([host(renders[l][1]) for l in ids], [host(renders[l][0]) for l in ids], [host(masks[l]) for l in ids],
                           host(model.depth_maps), model.depth_obs_delta)
    torch.autograd.backward([renders[l][1] for l in ids], [torch.from_numpy(g.astype(F32)).cuda() for g in r64["grads"]])
    want = _param_grads(model)
    model.zero_grad()
    ld, md = model(loss_weights=lw)
    assert set(ld) == {"loss_depth_obs"} and set(md) == {"depth_obs_mae", "depth_obs_valid_share"}
    loss = float(ld["loss_depth_obs"].detach())
    print(f"loss {loss:.9e} / {r64['loss']:.9e}  mae {md['depth_obs_mae']:.6e} / {r64['mae']:.6e}  share {md['depth_obs_valid_share']:.4f}")
    assert abs(loss - r64["loss"]) <= 5 * U * r64["loss"] + 2.0 ** -32
    assert abs(md["depth_obs_mae"] - r64["mae"]) <= 2 * U * r64["mae"] + 2.0 ** -33
    assert abs(md["depth_obs_valid_share"] - r64["share"]) <= U * r64["share"]
    ld["loss_depth_obs"].backward()
    got = _param_grads(model)
    assert set(got) == set(want)
    for k in want:
        ref = float(want[k].abs().max())
        print(f"  {k}: max |grad| {ref:.4e}  deviation {float((got[k] - want[k]).abs().max()) / max(ref, 1e-30):.3e}")
        assert float((got[k] - want[k]).abs().max()) <= _PARAM_BAR * ref, k
    return r64, got


@pytest.mark.parametrize("hands, layers", [(("right",), "all"), (("right",), "object"), (("right",), "hand"),
                                           (("right", "left"), "all"), (("right", "left"), "hand")])
def test_model_on_a_synthetic_scene(mano_model, hands, layers):
    from homan_amd import synth
    sil_fn, hand_fn = synth.hip_clip_fns(mano_model)
    clip = synth.make_clip(seed=71, frames=3, rend_size=32, image_size=64, obj="cube", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn, hands=hands)
    clip, D = _with_depth(mano_model, clip)
    model = _model(mano_model, clip, depth_maps=D, depth_obs_layers=layers)
    assert model.hand_nb == len(hands) and "depth_maps" in dict(model.named_buffers())
    # at the parameters the map was composed from: zero loss, zero gradients
    ld, md = model(loss_weights=_weights(lw_depth_obs=1.0))
    assert float(ld["loss_depth_obs"].detach()) == 0.0 and md["depth_obs_mae"] == 0.0 and md["depth_obs_valid_share"] > 0.5
    ld["loss_depth_obs"].backward()
    grads = _param_grads(model)
    assert grads and all(not bool(g.any()) for g in grads.values())
    # the object pushed away and aside: against float64
    with torch.no_grad():
        model.translations_object += torch.tensor([0.004, -0.003, 0.02], device="cuda")
        model.translations_hand += torch.tensor([-0.002, 0.001, -0.012], device="cuda")
    r64, got = _model_against_float64(model)
    assert r64["loss"] > 0
    moved = "translations_hand" if layers == "hand" else "translations_object"
    assert float(got[moved].abs().max()) > 0


def test_both_depth_terms_share_the_renders(mano_model):
    """ordinal term on as well: its value is bit-equal to a model without lw_depth_obs; the gradients add up"""
    clip, D = _with_depth(mano_model, _clip(mano_model, 72), ordinal_depth=True)
    shift = torch.tensor([0.004, -0.003, 0.02], device="cuda")
    models = [_model(mano_model, clip, depth_maps=D, ordinal_depth=True) for _ in range(3)]
    plain = _model(mano_model, clip, ordinal_depth=True)
    with torch.no_grad():
        for m in models + [plain]:
            m.translations_object += shift
            # a non-zero ordinal term: the hand moved in front of the object (x and y only: it stays the nearer one), the
            # annotation saying the object owns every pixel
            over = m.get_verts_object()[0].mean((0, 1)) - m.get_verts_hand()[0].mean((0, 1))
            over[2] = 0
            m.translations_hand += over
            m.masks_object.fill_(1)
            m.masks_human.zero_()
            m._refresh_derived()
    both, only_obs, only_ord = models
    ld, _ = both(loss_weights=_weights(lw_depth=1.0, lw_depth_obs=1.0))
    assert list(ld) == ["loss_depth", "loss_depth_obs"]
    (ld["loss_depth"] + ld["loss_depth_obs"]).sum().backward()
    assert [c.last_depth_bwd for c in both.depth_layers()[0]] == ["dense", "dense"]
    ld_obs, _ = only_obs(loss_weights=_weights(lw_depth_obs=1.0))
    ld_obs["loss_depth_obs"].backward()
    assert [c.last_depth_bwd for c in only_obs.depth_layers()[0]] == ["sparse", "sparse"]
    ld_ord, _ = only_ord(loss_weights=_weights(lw_depth=1.0))
    ld_ord["loss_depth"].sum().backward()
    ld_plain, _ = plain(loss_weights=_weights(lw_depth=1.0))
    assert float(ld_plain["loss_depth"].detach()) > 0
    assert torch.equal(ld["loss_depth"], ld_plain["loss_depth"]) and torch.equal(ld_ord["loss_depth"], ld_plain["loss_depth"])
    assert torch.equal(ld["loss_depth_obs"], ld_obs["loss_depth_obs"])
    g_both, g_obs, g_ord = _param_grads(both), _param_grads(only_obs), _param_grads(only_ord)
    for k in ("translations_object", "rotations_object"):
        want = g_obs[k] + g_ord[k]
        ref = float(want.abs().max())
        print(f"{k}: max |grad| {ref:.4e} deviation {float((g_both[k] - want).abs().max()) / ref:.3e}")
        # the same two gradient images, added per pixel before the (linear) depth backward instead of after it: one fp32 rounding
        # per pixel in place of one per vertex - the accumulation of _PARAM_BAR with u for 5u
        assert ref > 0 and float((g_both[k] - want).abs().max()) <= _PARAM_BAR / 5 * ref, k


# =============================================================================================== 2. backward paths
def test_sparse_and_dense_depth_backward_give_the_same_bits(mano_model):
    clip, D = _with_depth(mano_model, _clip(mano_model, 73))
    model = _model(mano_model, clip, depth_maps=D + (D > 0) * 0.02)
    out = {}
    for sole in (True, False):
        vo = model.get_verts_object()[0].detach().clone().requires_grad_()
        vh = model.get_verts_hand()[0].detach().clone().requires_grad_()
        l, _ = model.compute_depth_obs_loss(model.render_depth_layers(vo, vh), sole_consumer=sole)
        assert float(l["loss_depth_obs"].detach()) > 0
        l["loss_depth_obs"].backward()
        out[sole] = (vo.grad.clone(), vh.grad.clone(), [c.last_depth_bwd for c in model.depth_layers()[0]])
    assert out[True][2] == ["sparse", "sparse"] and out[False][2] == ["dense", "dense"]
    assert bool(out[True][0].any()) and bool(out[True][1].any())
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


def test_other_sizes_take_the_dense_backward(mano_model):
    clip = _clip(mano_model, 74, image=48)
    clip, D = _with_depth(mano_model, clip, image=48)
    model = _model(mano_model, clip, image=48, depth_maps=D + (D > 0) * 0.02)
    ld, _ = model(loss_weights=_weights(lw_depth_obs=1.0))
    assert float(ld["loss_depth_obs"].detach()) > 0
    ld["loss_depth_obs"].backward()
    assert [c.last_depth_bwd for c in model.depth_layers()[0]] == ["dense", "dense"]
    assert float(model.translations_object.grad.abs().max()) > 0


# =============================================================================================== 4. what the term is for
K_SCALE, STEPS = 1.15, 150


def test_depth_resolves_the_scale_and_distance_ambiguity(mano_model):
    """The object scaled by k and moved k times further away shows the same silhouette: the silhouette term alone leaves it there,
    the observed depth pulls it back.  Measured end errors are recorded in DESIGN.md section 5."""
    from homan_amd.jointopt import GraphStepper
    clip, D = _with_depth(mano_model, _clip(mano_model, 75), optimize_object_scale=True)
    err = {}
    for name, lw in (("depth", _weights(lw_sil_obj=1.0, lw_depth_obs=100.0)), ("control", _weights(lw_sil_obj=1.0))):
        model = _model(mano_model, clip, sync=False, depth_maps=D, optimize_object_scale=True)
        tz_true = model.translations_object.detach()[:, 0, 2].clone()
        with torch.no_grad():
            model.translations_object *= K_SCALE
            model.int_scales_object.fill_(K_SCALE)
        start = float((model.translations_object.detach()[:, 0, 2] - tz_true).abs().mean())
        stepper = GraphStepper(model, lw, 1e-2, STEPS)
        stepper.run(STEPS)
        torch.cuda.synchronize()
        err[name] = (start, float((model.translations_object.detach()[:, 0, 2] - tz_true).abs().mean()),
                     float(model.int_scales_object.detach()[0]))
        print(f"{name}: |t_z - t_z*| {start:.4f} -> {err[name][1]:.4f} m, scale {K_SCALE} -> {err[name][2]:.4f} in {STEPS} steps")
    assert err["depth"][1] < 0.5 * err["depth"][0]
    assert err["control"][1] > 0.9 * err["control"][0]


# =============================================================================================== 5. loops
def test_loops_take_the_term(mano_model):
    from homan_amd import synth
    from homan_amd.jointopt import FusedStepper, ShardStepper
    lw = dict(synth.STEP1_LOSS_WEIGHTS, lw_depth_obs=100.0)
    clip, D = _with_depth(mano_model, _clip(mano_model, 76))
    D = D + (D > 0) * 0.01
    model = _model(mano_model, clip, sync=False, depth_maps=D)
    with pytest.raises(NotImplementedError, match="mode='graph'"):
        FusedStepper(model, lw, 1e-2, 5)
    with pytest.raises(NotImplementedError, match="mode='graph'"):
        ShardStepper([model], lw, 1e-2, 5)
    with pytest.raises(NotImplementedError, match="mode='graph'"):
        _fit(mano_model, clip, lw, 5, "fused", depth_maps=D)
    with pytest.raises(ValueError, match="depth_maps"):
        _model(mano_model, clip)(loss_weights=lw)                       # a positive weight on a model without maps
    _, auto = _fit(mano_model, clip, lw, 5, "auto", depth_maps=D)
    _, eager = _fit(mano_model, clip, lw, 5, "eager", depth_maps=D)
    _, graph = _fit(mano_model, clip, lw, 5, "graph", depth_maps=D)
    _, plain = _fit(mano_model, clip, dict(synth.STEP1_LOSS_WEIGHTS), 5, "auto", depth_maps=D)
    new = {"loss_depth_obs", "depth_obs_mae", "depth_obs_valid_share"}
    assert len(auto["loss"]) == 5 and set(auto) == set(eager) == set(plain) | new
    for k in ("loss", "loss_depth_obs", "depth_obs_mae"):
        _close_as_the_two_loops(graph[k], eager[k])
    for k in auto:                                                       # auto fell to the graph loop: identical bits
        np.testing.assert_array_equal(np.asarray(auto[k]), np.asarray(graph[k]), err_msg=k)
    assert auto["loss_depth_obs"][0] > 0 and auto["loss"][0] > plain["loss"][0]


def test_clip_fitter_walk_equals_solo_fits(mano_model):
    from homan_amd import synth
    from homan_amd.jointopt import ClipFitter
    lw = dict(synth.STEP1_LOSS_WEIGHTS, lw_depth_obs=100.0)
    clips = []
    for seed in (77, 78):
        clip, D = _with_depth(mano_model, _clip(mano_model, seed))
        clips.append(dict(clip, depth_maps=D + (D > 0) * 0.01))
    fitter = ClipFitter(lw, num_iterations=5, optimize_mano=True, image_size=64, mano_model=mano_model, rend_size=32)
    results = fitter.fit(clips)
    assert fitter.timing["built"] == 1 and fitter.timing["reused"] == 1 and len(fitter.resident_graph) == 1
    for clip, res in zip(clips, results):
        model, evo = _fit(mano_model, clip, lw, 5, "auto", depth_maps=clip["depth_maps"])
        for k, v in res["state_dict"].items():
            assert torch.equal(v, getattr(model, k).detach().cpu()), k
        assert torch.equal(res["verts_object"], model.get_verts_object()[0].detach().cpu())
        assert evo["loss_depth_obs"][0] > 0
        for k in evo:
            np.testing.assert_array_equal(np.asarray(res["loss_evolution"][k]), np.asarray(evo[k]), err_msg=k)


def test_load_clip_refusals_leave_the_model_untouched(mano_model):
    from homan_amd.loopcommon import collate_inputs
    clip, D = _with_depth(mano_model, _clip(mano_model, 79))
    other, D2 = _with_depth(mano_model, _clip(mano_model, 80))
    kw = lambda c: dict(collate_inputs(c["person_parameters"], c["object_parameters"], c["objvertices"], c["objfaces"]),
                        camintr=c["camintr"])
    with_maps, without = _model(mano_model, clip, depth_maps=D), _model(mano_model, clip)
    for model, bad, msg in ((with_maps, kw(other), "depth_maps"), (with_maps, dict(kw(other), depth_maps=D2[:, :32, :32]), "depth_maps"),
                            (with_maps, dict(kw(other), depth_maps=D2[:2]), "depth_maps"),
                            (without, dict(kw(other), depth_maps=D2), "depth_maps")):
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        with pytest.raises(ValueError, match=msg):
            model.load_clip(**bad)
        after = model.state_dict()
        assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)
    with_maps.load_clip(**dict(kw(other), depth_maps=D2))
    assert torch.equal(with_maps.depth_maps.cpu(), D2)
    fresh = _model(mano_model, other, depth_maps=D2)
    lw = _weights(lw_depth_obs=1.0, lw_sil_obj=1.0)
    a, b = with_maps(loss_weights=lw)[0], fresh(loss_weights=lw)[0]
    assert all(torch.equal(a[k], b[k]) for k in b)
