"""homan_amd.fused.launch_plan on the CPU: every admissible input passes the assertions the launch code relies on, and the plans
of the configurations people run are pinned.  The pinned values are those of the expressions that stood in FusedStepper's
constructor and builders before they moved into launch_plan; the one deliberate difference is the last row (`side_own_vo`
without the silhouette term)."""
import itertools

import pytest

SWITCHES = ["pca", "so", "sh", "smooth", "col", "con", "v2d", "sil", "inter", "depth"]


def _switches(weights):
    from homan_amd.fused import TERMS
    on = dict.fromkeys(SWITCHES, False)
    for _, key, switch in TERMS:
        on[switch] = on[switch] or (key is not None and weights.get(key, 0.0) > 0)
    return on


def test_every_admissible_input_has_a_consistent_plan():
    """all 1024 switch sets x clips x hands x shared scale x inter_min x free scale x mesh sizes on both sides of the two vertex
    thresholds, restricted to what FusedStepper's constructor admits: launch_plan's own assertions hold for each"""
    from homan_amd.fused import LaunchPlan, launch_plan
    n = 0
    for bits in itertools.product([False, True], repeat=10):
        on = dict(zip(SWITCHES, bits))
        for C, h, shared, inter_min, free_scale, Vo in itertools.product((1, 2, 8), (1, 2), (False, True), (False, True),
                                                                         (False, True), (8, 4096, 4097, 24576, 24577)):
            if (h > 1 and (C > 1 or shared)) or (inter_min and (h > 1 or C > 1)) or (shared and not free_scale):
                continue
            plan = launch_plan(C, h, Vo, on, shared, inter_min, free_scale)
            assert isinstance(plan, LaunchPlan)
            n += 1
    assert n == 71680


COLUMNS = ["use_aux", "log_in_adam", "side_own_vo", "merge_renders", "pairs_after_lines", "mano_bwd_rigid", "fuse", "nn_fused",
           "nn_full_fused", "ht_fused", "nn_separate", "sm_in", "side_terms", "graph_iters", "sweep_blocks", "raster_lds_pad",
           "nn_lds_pad"]
# (weights, overrides of the weights, clips, object vertices, shared scale) -> the columns above
PINNED = {
    "cfg1, 1 clip": (("CFG1", {}, 1, 252, False), (0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 4, 1280, 0, 0)),
    "step-1, 1 clip": (("STEP1", {}, 1, 252, False), (0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 0, 4, 1280, 0, 0)),
    "step-2, 1 clip": (("STEP2", {}, 1, 252, False), (0, 1, 0, 0, 0, 1, 1, 0, 1, 1, 0, 1, 1, 4, 768, 4096, 0)),
    "step-1 + depth, 1 clip": (("STEP1", dict(lw_depth=2.0), 1, 252, False), (0, 1, 0, 1, 0, 1, 1, 1, 0, 1, 0, 1, 0, 4, 1280, 0, 0)),
    "step-1, 2 clips": (("STEP1", {}, 2, 252, False), (1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1024, 0, 34816)),
    "step-2, 2 clips": (("STEP2", {}, 2, 252, False), (1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1024, 0, 0)),
    "step-2, 2 clips, shared scale": (("STEP2", {}, 2, 252, True), (1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1024, 0, 0)),
    "step-1 + depth, 2 clips": (("STEP1", dict(lw_depth=2.0), 2, 252, False), (0, 1, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1024, 0, 34816)),
    "step-1, 1 clip, Vo = 4502": (("STEP1", {}, 1, 4502, False), (0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 4, 1280, 0, 0)),
    "step-1, 1 clip, Vo = 25002": (("STEP1", {}, 1, 25002, False), (0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 4, 1280, 0, 0)),
    # before launch_plan: side_own_vo = 1 here, with `vo_b` a buffer nothing wrote
    "step-1 without the silhouette term, 1 clip": (("STEP1", dict(lw_sil_obj=0.0), 1, 252, False),
                                                   (0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 4, 1280, 0, 0)),
}


@pytest.mark.parametrize("name", list(PINNED))
def test_pinned_plans(name):
    from homan_amd import synth
    from homan_amd.fused import launch_plan
    (weights, override, C, Vo, shared), want = PINNED[name]
    on = _switches(dict(getattr(synth, weights + "_LOSS_WEIGHTS"), **override))
    plan = launch_plan(C, 1, Vo, on, shared_scale=shared, inter_min=False, optimize_object_scale=shared)
    got = {k: getattr(plan, k) for k in COLUMNS}
    assert got == dict(zip(COLUMNS, want)), name
    assert plan.sil_reduce_in_bwd == (not plan.use_aux) and plan.pair_fused == (C == 1)
