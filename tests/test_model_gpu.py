"""End-to-end: homan_amd.HOMan (HIP) vs the CPU oracle and vs the reference-generated goldens.  GPU box."""
import copy

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
NAMES = util.golden_names()
# handobj_maxdist: the reference takes its distances from |a|^2 + |b|^2 - 2ab in fp32 (libyana batch_pairwise_dist,
# losses.py:227): at |a|^2 ~ 0.36 m^2 the rounding of that expansion is eps * 0.72 / (2 d) ~ 4e-6 m at d = 6 mm.  The kernel
# differences the coordinates first; the reference's own rounding error is the tolerance (absolute, 1e-5 m).
METRIC_ATOL = {"handobj_maxdist": 1e-5}
GRAD_ATOL = 5e-5      # parameter gradients vs the reference goldens, as a fraction of the tensor's largest entry


def _build_hip(name, mano_model, sync=True):
    from homan_amd import HOMan
    rec, inputs, camintr, weights, meta = util.load_golden(name)
    model = HOMan(mano_model=mano_model, rend_size=meta["image_size"], sync_metrics=sync,
                  **util.model_kwargs(inputs, camintr, meta))
    return rec, model, weights, meta


@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_reference_goldens(name, mano_model):
    """loss_dict / metric_dict / parameter gradients of the HIP model vs the REFERENCE composition's outputs
    (tolerance: 1e-4 relative on losses, BASELINE.json north_star)."""
    rec, model, weights, meta = _build_hip(name, mano_model)
    loss_dict, metric_dict = model(loss_weights=weights)
    fwd_keys = [k[4:] for k in rec if k.startswith("fwd_")]
    assert sorted(loss_dict) == sorted(fwd_keys)
    for k in fwd_keys:
        ref, got = rec["fwd_" + k], loss_dict[k].detach().cpu().numpy()
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-9, err_msg=k)
    for k in (k[7:] for k in rec if k.startswith("metric_")):
        np.testing.assert_allclose(metric_dict[k], float(rec["metric_" + k]), rtol=2e-4, atol=METRIC_ATOL.get(k, 0), err_msg=k)
    total = sum(loss_dict[k] * weights[k.replace("loss", "lw")] for k in loss_dict)
    total.sum().backward()
    for k, p in model.named_parameters():
        ref = rec["grad_" + k]
        if ref.size == 0:
            assert p.grad is None, k
            continue
        scale = max(np.abs(ref).max(), 1e-12)
        got = p.grad.cpu().numpy()
        # rotation, rigid transform and projection follow the oracle's operation order (bit-equal vertices and coverage,
        # tests/test_lockstep_gpu.py), what is left is the summation order of the gradients: 5e-5 of the largest entry
        np.testing.assert_allclose(got / scale, ref / scale, atol=GRAD_ATOL, err_msg=k)
    # (the golden's vertices come from the reference's own torch.matmul on the generating host - an MKL FMA chain, 2 ulp
    #  from the written-out products at ~1 m, see tests/test_oracle_golden.py)
    np.testing.assert_allclose(model.get_verts_object()[0].detach().cpu().numpy(), rec["verts_object"], atol=3e-7)
    np.testing.assert_allclose(model.get_verts_hand()[0].detach().cpu().numpy(), rec["verts_hand"], atol=2e-6)
    sd = set(model.state_dict().keys())
    viz_only = set()      # every reference key exists, the white depth-render textures included
    assert not (set(rec["state_dict_keys"].tolist()) - sd - viz_only)


@pytest.mark.parametrize("name", NAMES)
def test_pinned_step_matches_reference(name, mano_model):
    """Per-step pin: the HIP model at the reference loop's parameters after `pin_step` Adam steps vs the reference's own
    forward / backward there (losses 1e-4 relative = north_star, gradients 5e-5 of the largest entry)."""
    rec, model, weights, meta = _build_hip(name, mano_model)
    if not meta["has_trajectory"]:
        pytest.skip("forward / backward golden only")
    pinned = {k[4:]: torch.from_numpy(rec[k]).cuda() for k in rec if k.startswith("pin_")}
    _, unexpected = model.load_state_dict(pinned, strict=False)
    assert not unexpected
    loss_dict, metric_dict = model(loss_weights=weights)
    for k in (k[7:] for k in rec if k.startswith("pinfwd_")):
        np.testing.assert_allclose(loss_dict[k].detach().cpu().numpy(), rec["pinfwd_" + k], rtol=1e-4, atol=1e-9, err_msg=k)
    for k in (k[10:] for k in rec if k.startswith("pinmetric_")):
        np.testing.assert_allclose(metric_dict[k], float(rec["pinmetric_" + k]), rtol=2e-4, atol=METRIC_ATOL.get(k, 0),
                                   err_msg=k)
    sum(loss_dict[k] * weights[k.replace("loss", "lw")] for k in loss_dict).sum().backward()
    for k, p in model.named_parameters():
        ref = rec["pingrad_" + k]
        if ref.size == 0:
            assert p.grad is None, k
            continue
        scale = max(np.abs(ref).max(), 1e-12)
        np.testing.assert_allclose(p.grad.cpu().numpy() / scale, ref / scale, atol=GRAD_ATOL, err_msg=k)


@pytest.mark.parametrize("name", ["ref_step1_cube_b4_s64", "ref_step2_cube_b4_s64", "ref_step2_twohands_cube_b4_s64",
                                  "ref_step1_lefthand_cube_b4_s64"])
def test_short_trajectory_eager_and_graph(name, mano_model):
    """First optimisation steps against the reference loop's loss_evolution, in both loop modes.  The hard
    rasteriser makes long trajectories chaotic (a 1e-7 perturbation flips samples), so the comparison is tight on
    the first steps and loose after."""
    from homan_amd.jointopt import GraphStepper, parameter_groups
    steps = 6
    for mode in ("eager", "graph"):
        rec, model, weights, meta = _build_hip(name, mano_model, sync=(mode == "eager"))
        if mode == "eager":
            opt = torch.optim.Adam(parameter_groups(model, meta["lr"]))
            evo = []
            for _ in range(steps):
                opt.zero_grad()
                ld, _ = model(loss_weights=weights)
                tot = sum(ld[k] * weights[k.replace("loss", "lw")] for k in ld)
                evo.append(tot.item())
                tot.sum().backward()
                opt.step()
        else:
            st = GraphStepper(model, weights, meta["lr"], steps)
            st.run(steps)
            evo = st.loss_evolution(steps)["loss"]
        ref = rec["evo_loss"][:steps]
        # bars = what tools/measure_test_bars.py measures on the MI355X (profiles/r06_test_bars.json) x ~1.5-2: first step 7.9e-8,
        # first three 8.1e-6, all six 5.6e-3 (a flipped sample by then)
        np.testing.assert_allclose(evo[0], ref[0], rtol=1e-6, err_msg=mode)
        np.testing.assert_allclose(evo[:3], ref[:3], rtol=2e-5, err_msg=mode)
        np.testing.assert_allclose(evo, ref, rtol=0.01, err_msg=mode)
        sd = model.state_dict()
        np.testing.assert_array_equal(sd["mano_rot"].cpu().numpy(), rec["in_mano_rot"])      # never stepped


def test_two_hands_through_optimize_hand_object(mano_model):
    """hand_nb = 2 (right + left) through the public entry: `mode="auto"` leaves the fused loop (one right hand only) for
    the graph-captured HOMan.forward iteration and follows the reference loop's loss_evolution of the golden."""
    from homan_amd import synth
    from homan_amd.jointopt import optimize_hand_object
    sil_fn, hand_fn = synth.hip_clip_fns(mano_model)
    clip = synth.make_clip(seed=4, frames=4, rend_size=64, image_size=64, obj="cube", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn, hands=("right", "left"))
    rec, _, _, weights, meta = util.load_golden("ref_step2_twohands_cube_b4_s64")
    np.testing.assert_allclose(clip["person_parameters"][0]["verts"].numpy(), rec["in_verts_hand_og"][:2], atol=2e-6)
    model, evo, _ = optimize_hand_object(clip["person_parameters"], clip["object_parameters"], objvertices=clip["objvertices"],
                                         objfaces=clip["objfaces"], loss_weights=weights, num_iterations=4, lr=meta["lr"],
                                         camintr=clip["camintr"], optimize_mano=True, image_size=64, mano_model=mano_model,
                                         rend_size=64)
    assert model.hand_nb == 2 and model.get_verts_hand()[0].shape == (8, 778, 3)
    # right + left hands through their own side's model: vertices bit-equal with the oracle's written-out layer at the fitted
    # parameters
    from oracle.jointopt import collate_inputs
    from oracle.model import OracleHOMan
    kw = collate_inputs(clip["person_parameters"], clip["object_parameters"], clip["objvertices"], clip["objfaces"])
    om = OracleHOMan(**kw, camintr=clip["camintr"], class_name="default", int_scale_init=1, optimize_mano=True, image_size=64,
                     mano_model=mano_model, rend_size=64)
    with torch.no_grad():
        for k, p in om.named_parameters():
            p.copy_(dict(model.named_parameters())[k].detach().cpu())
    assert torch.equal(model.get_verts_hand()[0].detach().cpu(), om.get_verts_hand()[0].detach())
    np.testing.assert_allclose(evo["loss"][0], rec["evo_loss"][0], rtol=1e-4)
    np.testing.assert_allclose(evo["loss"][:3], rec["evo_loss"][:3], rtol=5e-3)


def test_hip_vs_oracle_cfg_sized_clip(mano_model):
    """A fresh synthetic clip (not a golden): HIP model vs oracle model, losses + vertex outputs."""
    from homan_amd import HOMan, synth
    from oracle.jointopt import collate_inputs
    from oracle.model import OracleHOMan
    sil_fn, hand_fn = util.oracle_clip_fns(mano_model)
    clip = synth.make_clip(seed=7, frames=6, rend_size=128, image_size=128, obj="bottle", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn)
    kw = collate_inputs(clip["person_parameters"], clip["object_parameters"], clip["objvertices"], clip["objfaces"])
    common = dict(camintr=clip["camintr"], class_name="default", int_scale_init=1, optimize_mano=True,
                  image_size=128, mano_model=mano_model, rend_size=128)
    lw = dict(synth.STEP2_LOSS_WEIGHTS)
    om = OracleHOMan(**copy.deepcopy(kw), **common)
    hm = HOMan(**copy.deepcopy(kw), **common)
    lo, mo = om(loss_weights=lw)
    lh, mh = hm(loss_weights=lw)
    for k in lo:
        np.testing.assert_allclose(lh[k].detach().cpu().numpy(), lo[k].detach().numpy(), rtol=1e-4, atol=1e-9,
                                   err_msg=k)
    for k in mo:
        np.testing.assert_allclose(mh[k], mo[k], rtol=2e-4, err_msg=k)
    # 1e-3 mm on vertices (BASELINE.json north_star) at identical parameters
    dv = (hm.get_verts_hand()[0].detach().cpu() - om.get_verts_hand()[0].detach()).abs().max().item()
    do = (hm.get_verts_object()[0].detach().cpu() - om.get_verts_object()[0].detach()).abs().max().item()
    assert dv < 1e-6 and do < 1e-6, (dv, do)     # metres
    # ... and, since both sides evaluate ONE written-out operation order (oracle/csrc/lbs_exact.c <-> csrc/mano.hip for the MANO
    # layer, oracle.model.transform_persp <-> the rigid kernels), bit for bit:
    assert dv == 0.0 and do == 0.0, (dv, do)
    # hand silhouette term (reference losses.py:166-181, present but disabled upstream): value + NMR pseudo-gradient
    vo_h = om.get_verts_hand()[0].detach().requires_grad_(True)
    lo_h = om.losses.compute_sil_loss_hand(vo_h, om.faces_hand)["loss_sil_hand"]
    lo_h.sum().backward()
    vh_h = hm.get_verts_hand()[0].detach().requires_grad_(True)
    lh_h = hm.losses.compute_sil_loss_hand(vh_h, hm.faces_hand)["loss_sil_hand"]
    lh_h.sum().backward()
    assert float(lo_h) > 0
    np.testing.assert_allclose(lh_h.detach().cpu().numpy(), lo_h.detach().numpy(), rtol=1e-5)
    scale = vo_h.grad.abs().max().item()
    assert scale > 0
    np.testing.assert_allclose(vh_h.grad.cpu().numpy(), vo_h.grad.numpy(), rtol=1e-3, atol=1e-3 * scale)


@pytest.mark.parametrize("name", NAMES)
def test_fused_step_equals_autograd_path(name, mano_model):
    """FusedStepper (no autograd tape) vs HOMan.forward + autograd: same losses, same parameter gradients."""
    from homan_amd.jointopt import FusedStepper
    rec, model, weights, meta = _build_hip(name, mano_model, sync=False)
    loss_dict, metric_dict = model(loss_weights=weights)
    total = sum(loss_dict[k] * weights[k.replace("loss", "lw")] for k in loss_dict)
    total.sum().backward()
    ref_grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    ref_losses = {k: float(v.detach().reshape(-1)[0]) for k, v in loss_dict.items()}
    ref_losses.update({k: float(v) for k, v in metric_dict.items()})
    ref_losses["loss"] = float(total.detach().reshape(-1)[0])
    st = FusedStepper(model, weights, meta["lr"], 4, capture=False)
    st.forward_backward(log=True)
    torch.cuda.synchronize()
    evo = {k: st.log_buf[0, 0, st.SLOTS.index(k)].item() for k in st.keys}      # log rows are (step, clip, slot)
    evo["loss"] = st.log_buf[0, 0, len(st.SLOTS)].item()
    assert sorted(evo) == sorted(ref_losses)
    for k, v in ref_losses.items():
        np.testing.assert_allclose(evo[k], v, rtol=2e-6, atol=1e-9, err_msg=k)
    for k, p in model.named_parameters():
        if k in ref_grads:
            scale = max(ref_grads[k].abs().max().item(), 1e-20)
            err = ((p.grad - ref_grads[k]).abs().max() / scale).item()
            assert err < 2e-5, (k, err)
        else:
            assert p.grad is None or k in ("cams_hand",), k
    # ... and a few captured steps follow the autograd loop (left hands and optimize_mano=False included)
    rec2, fresh, _, _ = _build_hip(name, mano_model, sync=False)
    from homan_amd.jointopt import GraphStepper
    gs = GraphStepper(fresh, weights, meta["lr"], 3)
    gs.run(3)
    rec3, again, _, _ = _build_hip(name, mano_model, sync=False)
    fs = FusedStepper(again, weights, meta["lr"], 3)
    fs.run(3)
    np.testing.assert_allclose(fs.loss_evolution(3)["loss"][:2], gs.loss_evolution(3)["loss"][:2], rtol=1e-5)
    np.testing.assert_allclose(fs.loss_evolution(3)["loss"], gs.loss_evolution(3)["loss"], rtol=2e-2)


@pytest.mark.parametrize("weights_name", ["STEP1_LOSS_WEIGHTS", "STEP2_LOSS_WEIGHTS"])
def test_fused_loop_on_a_mesh_over_4096_vertices(weights_name, mano_model):
    """Object meshes beyond the metric-only search's group table (4096 vertices, e.g. un-decimated YCB models): the fused
    loop takes the full search for the logged distance, the contact scatter walks the object in ranges of 4096 vertices -
    same losses and gradients as HOMan.forward + autograd, and `mode="auto"` runs it."""
    from homan_amd import synth
    from homan_amd.jointopt import FusedStepper, build_model, optimize_hand_object
    ov, of = synth.bottle_mesh(segments=90, rings=50)
    assert ov.shape[0] > 4096
    sil_fn, hand_fn = synth.hip_clip_fns(mano_model)
    clip = synth.make_clip(seed=3, frames=4, rend_size=64, image_size=64, obj=(ov, of), silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn)
    weights = dict(getattr(synth, weights_name))
    common = dict(objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"], optimize_mano=True,
                  image_size=64, mano_model=mano_model, rend_size=64)
    model = build_model(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                        sync_metrics=False, **common)
    loss_dict, metric_dict = model(loss_weights=weights)
    total = sum(loss_dict[k] * weights[k.replace("loss", "lw")] for k in loss_dict)
    total.sum().backward()
    ref_grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    ref = {k: float(v.detach().reshape(-1)[0]) for k, v in loss_dict.items()}
    ref.update({k: float(v) for k, v in metric_dict.items()})
    st = FusedStepper(model, weights, 1e-2, 4, capture=False)
    st.forward_backward(log=True)
    torch.cuda.synchronize()
    for k, v in ref.items():
        np.testing.assert_allclose(st.log_buf[0, 0, st.SLOTS.index(k)].item(), v, rtol=2e-6, atol=1e-9, err_msg=k)
    for k, p in model.named_parameters():
        if k in ref_grads:
            scale = max(ref_grads[k].abs().max().item(), 1e-20)
            assert ((p.grad - ref_grads[k]).abs().max() / scale).item() < 2e-5, k
    _, evo, _ = optimize_hand_object(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                                     loss_weights=weights, num_iterations=3, **common)
    assert np.isfinite(evo["loss"]).all() and abs(evo["loss"][0] - float(total.detach().reshape(-1)[0])) < 1e-5 * abs(evo["loss"][0])


def test_fused_loop_without_the_silhouette_term(mano_model):
    """lw_sil_obj = 0 at one clip, one hand, no depth / collision / contact term: there is no face setup, the side stream's
    own transform writes the object's vertices and every pair-wise launch must read THAT buffer (launch_plan: side_own_vo needs
    the silhouette term) - same losses and gradients as HOMan.forward + autograd, at the bars of
    test_fused_step_equals_autograd_path."""
    from homan_amd import synth
    from homan_amd.jointopt import FusedStepper, build_model
    sil_fn, hand_fn = synth.hip_clip_fns(mano_model)
    clip = synth.make_clip(seed=0, frames=2, rend_size=64, image_size=64, obj="cube", silhouette_fn=sil_fn, hand_verts_fn=hand_fn)
    weights = dict(synth.STEP1_LOSS_WEIGHTS, lw_sil_obj=0.0)
    model = build_model(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                        objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"], optimize_mano=True,
                        image_size=64, mano_model=mano_model, rend_size=64, sync_metrics=False)
    loss_dict, metric_dict = model(loss_weights=weights)
    total = sum(loss_dict[k] * weights[k.replace("loss", "lw")] for k in loss_dict)
    total.sum().backward()
    ref_grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    ref = {k: float(v.detach().reshape(-1)[0]) for k, v in loss_dict.items()}
    ref.update({k: float(v) for k, v in metric_dict.items()})
    assert "loss_sil_obj" not in ref and ref["loss_smooth_obj"] > 0 and ref["handobj_maxdist"] > 0
    st = FusedStepper(model, weights, 1e-2, 4, capture=False)
    st.forward_backward(log=True)
    torch.cuda.synchronize()
    assert sorted(st.keys) == sorted(ref)
    for k, v in ref.items():
        got = st.log_buf[0, 0, st.SLOTS.index(k)].item()
        print(k, got, v, abs(got - v) / max(abs(v), 1e-30))
        np.testing.assert_allclose(got, v, rtol=2e-6, atol=1e-9, err_msg=k)
    np.testing.assert_allclose(st.log_buf[0, 0, len(st.SLOTS)].item(), float(total.detach().reshape(-1)[0]), rtol=2e-6, atol=1e-9)
    for k, p in model.named_parameters():
        if k in ref_grads:
            scale = max(ref_grads[k].abs().max().item(), 1e-20)
            err = ((p.grad - ref_grads[k]).abs().max() / scale).item()
            print(k, "gradient error", err)
            assert err < 2e-5, (k, err)


def test_fused_loop_at_a_render_size_off_the_tile_grid(mano_model):
    """rend_size % 32 != 0 (the reference's REND_SIZE is 256, but the silhouette size is the caller's): the fused loop renders
    on the padded grid with rescaled intrinsics, padded masks and eps in the padded grid's units - same losses and gradients
    as HOMan.forward + autograd, alone and in a clip batch."""
    from homan_amd import synth
    from homan_amd.jointopt import FusedStepper, build_model
    size = 80
    sil_fn, hand_fn = synth.hip_clip_fns(mano_model)
    weights = dict(synth.STEP2_LOSS_WEIGHTS)

    def make(seed):
        clip = synth.make_clip(seed=seed, frames=4, rend_size=size, image_size=size, obj="cube", silhouette_fn=sil_fn,
                               hand_verts_fn=hand_fn)
        return build_model(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                           objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"],
                           optimize_mano=True, image_size=size, mano_model=mano_model, rend_size=size, sync_metrics=False)
    model = make(2)
    assert model.losses.sil_ctx.padded
    loss_dict, metric_dict = model(loss_weights=weights)
    total = sum(loss_dict[k] * weights[k.replace("loss", "lw")] for k in loss_dict)
    total.sum().backward()
    ref_grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    ref = {k: float(v.detach().reshape(-1)[0]) for k, v in loss_dict.items()}
    ref.update({k: float(v) for k, v in metric_dict.items()})
    st = FusedStepper(model, weights, 1e-2, 4, capture=False)
    st.forward_backward(log=True)
    torch.cuda.synchronize()
    for k, v in ref.items():
        np.testing.assert_allclose(st.log_buf[0, 0, st.SLOTS.index(k)].item(), v, rtol=2e-6, atol=1e-9, err_msg=k)
    for k, p in model.named_parameters():
        if k in ref_grads:
            scale = max(ref_grads[k].abs().max().item(), 1e-20)
            assert ((p.grad - ref_grads[k]).abs().max() / scale).item() < 2e-5, k
    # a batch of two such clips == the clips alone, bit for bit
    solo = []
    for seed in (2, 3):
        one = FusedStepper(make(seed), weights, 1e-2, 4)
        one.run(4)
        solo.append(one.loss_evolution(4)["loss"])
    both = FusedStepper([make(2), make(3)], weights, 1e-2, 4)
    both.run(4)
    for e, want in zip(both.loss_evolution(4), solo):
        np.testing.assert_array_equal(e["loss"], want)


def test_fused_trajectory_matches_reference_loop(mano_model):
    from homan_amd.jointopt import FusedStepper
    rec, model, weights, meta = _build_hip("ref_step2_cube_b4_s64", mano_model, sync=False)
    st = FusedStepper(model, weights, meta["lr"], 6)
    st.run(6)
    evo = st.loss_evolution(6)
    ref = rec["evo_loss"][:6]
    np.testing.assert_allclose(evo["loss"][0], ref[0], rtol=1e-4)
    np.testing.assert_allclose(evo["loss"][:3], ref[:3], rtol=5e-3)
    np.testing.assert_allclose(evo["loss"], ref, rtol=0.1)
    for k in ("loss_sil_obj", "loss_contact", "loss_collision", "iou_object"):
        np.testing.assert_allclose(evo[k][0], rec["evo_" + k][0], rtol=2e-4, atol=1e-9, err_msg=k)
    np.testing.assert_array_equal(model.mano_rot.detach().cpu().numpy(), rec["in_mano_rot"])


def test_joint_fit_resume_roundtrip(mano_model, tmp_path):
    """reference fit_vid_dataset.py:365-372 / :322-338: a fit saved as joint_fit.pt and resumed through
    `state_dict=` (jointopt.py:126-127, strict=False) continues from the very same parameters."""
    from homan_amd import checkpoint, synth
    from homan_amd.jointopt import FusedStepper, build_model
    sil_fn, hand_fn = util.oracle_clip_fns(mano_model)
    clip = synth.make_clip(seed=11, frames=4, rend_size=64, image_size=64, obj="bottle", silhouette_fn=sil_fn,
                           hand_verts_fn=hand_fn)

    def make(state_dict=None):
        return build_model(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                           objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"],
                           optimize_mano=True, image_size=64, mano_model=mano_model, rend_size=64, state_dict=state_dict,
                           sync_metrics=False)
    lw = dict(synth.STEP2_LOSS_WEIGHTS)
    model = make()
    FusedStepper(model, lw, 1e-2, 5).run(5)
    path = tmp_path / "joint_fit.pt"
    checkpoint.save_joint_fit(model, path)
    resumed = make(checkpoint.load_joint_fit(path))
    fresh = make()
    with torch.no_grad():
        assert torch.equal(resumed.get_verts_object()[0], model.get_verts_object()[0])
        assert torch.equal(resumed.get_verts_hand()[0], model.get_verts_hand()[0])
        assert not torch.equal(fresh.get_verts_object()[0], model.get_verts_object()[0])
        la, _ = model(loss_weights=lw)
        lb, _ = resumed(loss_weights=lw)
    for k in la:
        assert torch.equal(la[k], lb[k]), k


def test_adaptive_raster_order_is_invisible_to_the_results(mano_model, monkeypatch):
    """hm_tune_raster_reorder: the rasteriser's workgroups record what they cost and the backward's first launch re-sorts the
    launch order for the next forward (a scheduling hint captured with the iteration).  Ten iterations with the hint forced on
    and forced off give bit-identical loss rows and parameters: the order kept in the workspace stays a permutation of the
    (frame, region) entries - a region rendered twice or not at all would show in the moving silhouettes."""
    from homan_amd import lib as hl
    from homan_amd.jointopt import FusedStepper
    name, steps = "ref_step2_cube_b4_s64", 10
    outs = []
    for on in (0, 1):
        monkeypatch.setattr(FusedStepper, "raster_reorder", on)
        rec, model, weights, meta = _build_hip(name, mano_model, sync=False)
        st = FusedStepper(model, weights, meta["lr"], steps)
        assert hl.lib().hm_tune_raster_reorder(-1) == 0          # (the hint is restored after the capture)
        st.run(steps)
        outs.append((st.loss_evolution(steps), {k: v.detach().clone() for k, v in model.named_parameters()}))
    (evo_a, par_a), (evo_b, par_b) = outs
    for k in evo_a:
        np.testing.assert_array_equal(np.asarray(evo_a[k]), np.asarray(evo_b[k]), err_msg=k)
    for k in par_a:
        assert torch.equal(par_a[k], par_b[k]), k


def test_in_graph_timestamps_are_invisible_to_the_results(mano_model):
    """hm_sil_timestamps: the three heavy kernels of the silhouette chain stamp the device wall clock while they are replayed
    from the captured hipGraph (bench.py's roofline timing).  The durations are positive and sane, and the optimisation - loss
    rows and parameters - is bit for bit the one of an untimed twin."""
    import ctypes
    from homan_amd import lib as hl
    from homan_amd.jointopt import FusedStepper
    name, steps = "ref_step2_cube_b4_s64", 4
    outs = []
    for timed in (False, True):
        rec, model, weights, meta = _build_hip(name, mano_model, sync=False)
        st = FusedStepper(model, weights, meta["lr"], steps)
        sctx = model.losses.sil_ctx
        ws, us3, dims = hl.ptr(sctx.workspace), (ctypes.c_float * 3)(), (sctx.B, sctx.V, sctx.F, sctx.S)
        for _ in range(steps):
            if timed:
                hl.check(hl.lib().hm_sil_timestamps(ws, *dims, 1, hl.stream()), "hm_sil_timestamps")
            st.run(1)
            if timed:
                hl.check(hl.lib().hm_sil_timestamps_read(ws, *dims, None, ctypes.cast(us3, ctypes.c_void_p), hl.stream()), "read")
                assert all(0.5 < us3[i] < 5e3 for i in range(3)), list(us3)
        outs.append((st.loss_evolution(steps), {k: v.detach().clone() for k, v in model.named_parameters()}))
    (evo_a, par_a), (evo_b, par_b) = outs
    for k in evo_a:
        np.testing.assert_array_equal(np.asarray(evo_a[k]), np.asarray(evo_b[k]), err_msg=k)
    for k in par_a:
        assert torch.equal(par_a[k], par_b[k]), k


def test_cfg1_full_fit_follows_the_reference_loop(mano_model):
    """BASELINE cfg1 at full size (10 frames 128^2, cube, silhouette + 2-D keypoints, 100 Adam steps): the fused loop against
    the `loss_evolution` the REFERENCE's own loop produced on these inputs (tests/golden/ref_cfg1_cube_b10_s128.npz, generated
    by tools/refharness/gen_goldens.py from /root/reference).  Tight while the two runs see the same coverage (the hard
    rasteriser makes the loss piecewise constant in the pose: a last-bit difference flips a sample within a few steps,
    DESIGN.md section 2), then the same optimisation.  Bars = measured (tools/measure_test_bars.py, profiles/r06_test_bars.json)
    x 1.5: the total within 8 % at every step (measured 5.5 %), the silhouette term within 6.5 % of its FIRST value (measured
    4.3 %: late in the fit the term is small and its relative deviation means nothing), the final total within 3.5 % (2.2 %),
    the hand's 2-D term - which does not see the object on this loss set - within 1e-5 throughout (1.4e-6)."""
    from homan_amd.jointopt import FusedStepper
    rec, model, weights, meta = _build_hip("ref_cfg1_cube_b10_s128", mano_model, sync=False)
    steps = meta["steps"]
    assert steps == 100
    st = FusedStepper(model, weights, meta["lr"], steps)
    st.run(steps)
    evo = st.loss_evolution(steps)
    split = steps
    for k in ("loss", "loss_sil_obj", "loss_v2d_hand"):
        got, ref = np.asarray(evo[k]), rec["evo_" + k]
        bad = np.nonzero(np.abs(got - ref) > 5e-4 * np.abs(ref) + 1e-7)[0]
        if len(bad):
            split = min(split, int(bad[0]))
    assert split >= 3, split
    for k in ("loss", "loss_sil_obj", "loss_v2d_hand"):
        got, ref = np.asarray(evo[k]), rec["evo_" + k]
        np.testing.assert_allclose(got[0], ref[0], rtol=1e-4, err_msg=k)
        np.testing.assert_allclose(got[:split], ref[:split], rtol=5e-4, atol=1e-7, err_msg=k)
        if k == "loss_sil_obj":
            np.testing.assert_allclose(got[split:], ref[split:], rtol=0, atol=0.065 * abs(float(ref[0])), err_msg=k)
        else:
            np.testing.assert_allclose(got[split:], ref[split:], rtol=0.08, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(evo["loss_v2d_hand"], rec["evo_loss_v2d_hand"], rtol=1e-5)
    np.testing.assert_allclose(evo["loss"][-1], rec["evo_loss"][-1], rtol=0.035)
    np.testing.assert_array_equal(model.mano_rot.detach().cpu().numpy(), rec["in_mano_rot"])      # never stepped


@pytest.mark.parametrize("frames,obj", [(2, "cube"), (2, "bottle")])
def test_shortest_clip_matches_oracle_and_fits(frames, obj, mano_model):
    """The shortest clip the reference's loss set is defined on: TWO frames (one frame makes the temporal smoothness a mean over
    nothing; three frames trigger the reference's dim-less torch.cross).  HIP forward vs the CPU oracle
    (losses 1e-4), the fused loop a few steps: finite, the objective falls, and a batch of two such clips equals the solo fits."""
    from homan_amd import HOMan, synth
    from homan_amd.jointopt import FusedStepper
    from oracle.jointopt import collate_inputs
    from oracle.model import OracleHOMan
    size = 64
    sil_fn, hand_fn = util.oracle_clip_fns(mano_model)
    lw = dict(synth.STEP2_LOSS_WEIGHTS)

    def make(seed):
        clip = synth.make_clip(seed=seed, frames=frames, rend_size=size, image_size=size, obj=obj, silhouette_fn=sil_fn,
                               hand_verts_fn=hand_fn)
        kw = collate_inputs(clip["person_parameters"], clip["object_parameters"], clip["objvertices"], clip["objfaces"])
        return kw, dict(camintr=clip["camintr"], class_name="default", int_scale_init=1, optimize_mano=True, image_size=size,
                        mano_model=mano_model, rend_size=size)
    kw, common = make(71)
    lo, _ = OracleHOMan(**copy.deepcopy(kw), **common)(loss_weights=lw)
    lh, _ = HOMan(**copy.deepcopy(kw), **common)(loss_weights=lw)
    assert sorted(lo) == sorted(lh)
    for k in lo:
        np.testing.assert_allclose(lh[k].detach().cpu().numpy().reshape(-1), lo[k].detach().numpy().reshape(-1), rtol=1e-4,
                                   atol=1e-9, err_msg=k)
    solo = []
    for seed in (71, 72):
        kw_s, common_s = make(seed)
        st = FusedStepper(HOMan(**kw_s, **common_s, sync_metrics=False), lw, 1e-2, 8)
        st.run(8)
        evo = st.loss_evolution(8)
        assert np.isfinite(evo["loss"]).all() and evo["loss"][-1] < evo["loss"][0]
        solo.append(evo["loss"])
    both = FusedStepper([HOMan(**make(s)[0], **make(s)[1], sync_metrics=False) for s in (71, 72)], lw, 1e-2, 8)
    both.run(8)
    for e, want in zip(both.loss_evolution(8), solo):
        np.testing.assert_array_equal(e["loss"], want)
