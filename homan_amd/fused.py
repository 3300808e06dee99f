"""FusedStepper: the whole optimisation iteration (reference homan/jointopt.py:158-192 over homan/homan.py:421-508) as a fixed
sequence of C-ABI kernel launches on two or three HIP streams, captured in hipGraphs - the benchmark path.  One clip, a batch
of equal-shaped clips (homan_amd.clipbatch), or - through homan_amd.shard - a shard of clips of any shapes."""
from dataclasses import dataclass

import numpy as np
import torch

from . import lib as _lib
from .loopcommon import HmAdam, parameter_groups

# the loss terms and logged metrics, in slot order: (slot of `vals` / name in loss_evolution, key of its weight - None: a metric,
# logged only -, switch of FusedStepper.on).  A switch is on when one of its weights is positive.
TERMS = (("loss_pca", "lw_pca", "pca"), ("loss_scale_obj", "lw_scale_obj", "so"), ("loss_scale_hand", "lw_scale_hand", "sh"),
         ("loss_smooth_obj", "lw_smooth_obj", "smooth"), ("loss_smooth_hand", "lw_smooth_hand", "smooth"),
         ("loss_collision", "lw_collision", "col"), ("loss_contact", "lw_contact", "con"),
         ("loss_v2d_hand", "lw_v2d_hand", "v2d"), ("v2d_hand", None, "v2d"), ("loss_sil_obj", "lw_sil_obj", "sil"),
         ("iou_object", None, "sil"), ("loss_inter", "lw_inter", "inter"), ("handobj_maxdist", None, "inter"),
         ("loss_depth", "lw_depth", "depth"))


@dataclass(frozen=True)
class LaunchPlan:
    """every scheduling decision of the fused iteration, taken once by `launch_plan` (which says what each one is for)"""
    use_aux: bool
    log_in_adam: bool
    side_own_vo: bool
    merge_renders: bool
    sil_reduce_in_bwd: bool
    pairs_after_lines: bool
    mano_bwd_rigid: bool
    pair_fused: bool
    fuse: bool
    nn_fused: bool
    nn_full_fused: bool
    ht_fused: bool
    nn_separate: bool
    sm_in: bool
    side_terms: bool
    graph_iters: int
    sweep_blocks: int
    raster_lds_pad: int
    nn_lds_pad: int


def launch_plan(C, h, Vo, on, shared_scale=False, inter_min=False, optimize_object_scale=False):
    """The LaunchPlan of a fit of C clips with h hands per frame and Vo object vertices; `on`: the ten term switches of
    FusedStepper.on.  Pure (no device, no library): the one place where a launch is placed, merged, split or hinted, and where
    what must hold between those decisions is checked (tests/test_fused_plan.py walks every admissible input)."""
    # third stream for the silhouette reduction + log row: it pays on a clip batch (+1.5 %); at one clip the graph executor
    # spends two cross-queue hops (~10 us each) on it, and two streams are 5-6 % faster (same-box A/B, cfg2 and cfg3)
    # (with the depth launches on the side stream the three-stream graph dies at replay in the HIP runtime, like the other
    #  patterns listed at _loop_streams: two streams)
    use_aux = C > 1 and not on["depth"]
    # two streams, no shared scale: the log row of a step is written by the Adam launch itself (one launch less)
    log_in_adam = not use_aux and not shared_scale
    # the side stream forms the camera-space object vertices ITSELF (hm_rigid_fwd_clips into a buffer of its own: the face
    # setup's arithmetic, the same floats) instead of waiting for the face setup's copy: the silhouette chain then has no
    # successor on another queue between the iteration's fork and its join - the rasteriser follows the face setup without
    # the few microseconds a node with a cross-queue successor costs its own queue (EXPERIMENTS r6)
    # (not on the step-2 sets: there the hand-side chain is the longer one, and one more launch on it costs what the
    #  silhouette chain gains - cfg3 5 457 -> 5 221 it/s with it)
    # (only with the silhouette term: without it there is no face setup, the side stream's own transform writes `vo` and
    #  every reader of `vo_b` must find it there)
    side_own_vo = h == 1 and C == 1 and on["sil"] and not on["depth"] and not on["col"] and not on["con"]
    # with the ordinal depth term the object's two renders of an iteration - ROI silhouette, full-image depth - are ONE launch
    # pair (hm_sil_fwd_multi; see _issue_silhouette_chain)
    merge_renders = h == 1 and on["depth"] and on["sil"]
    # the silhouette loss / IoU values (log only) come out of the backward's first launch: one launch less on the chain
    # (two streams only: with the third stream the reduction and the log row stay there, behind the raster's event)
    sil_reduce_in_bwd = not use_aux
    # iterations per replay of the second graph (run()): one clip, no collective between the halves of an iteration.  The
    # turnaround between two replays is ~5 us of a 160 us iteration (same-box A/B: +2-3 % at 4, no more at 8 / 16)
    graph_iters = 4 if C == 1 else 1
    # a clip batch: the pair-wise terms of the side stream wait for the END of the line expansion (the backward in two
    # calls) - that kernel is latency-bound and takes 200 us instead of 150 next to neighbours that hold its wave slots -
    # and the sweeps run 1024 persistent workgroups instead of 1280 so that the hand's gradient launches find registers
    # next to them (same-box A/B, 8 clips: step-1 8 650 -> 8 865 it/s, step-2 7 142 -> 7 332; either change alone loses).
    # (Started next to the raster instead, the search / smoothness / interaction launches cost it more - 362 -> 433 us -
    #  than they gain next to the line expansion - 230 -> 162 us.)
    pairs_after_lines = C > 1 and on["sil"]
    # the hand's rigid backward inside the MANO backward's launch (hm_mano_bwd_rigid_clips): one launch less on the hand-side
    # chain.  One clip: cfg2 +1.3 %, cfg3 +1.4 %; a clip batch hides that chain under the silhouette chain and loses 1-1.6 %
    # (round 6: a clip batch too, +0.5 % - the separate hand launch was a 1024-thread workgroup per frame that found no room
    #  next to the persistent sweeps: 106 us on average, up to 365 us in the 8-clip profile of round 5)
    #  (a step-2 batch keeps the separate launch: 7 715 against 7 647 it/s)
    mano_bwd_rigid = C == 1 or not (on["col"] or on["con"])
    # the pair-wise terms in one launch (csrc/pairterms.hip) at one clip: the hand-side chain is the iteration's critical
    # path, -6 %; a batch hides that chain under the silhouette chain and the fused launch only adds contention there, +1.6 %
    pair_fused = C == 1
    # pair terms that feed nothing to each other go in ONE launch (csrc/pairterms.hip): the interaction term, the
    # object's smoothness, the metric-only search (no contact term) and the hand-only reductions
    fuse = pair_fused and on["inter"] and Vo <= 4096 and not inter_min
    nn_fused = fuse and not on["con"]
    # with the contact term the FULL search (nearest object vertex of every hand vertex) is the launch's first block
    # range instead, and the contact launches follow it: one launch less on the hand-side chain of the step-2 sets
    nn_full_fused = fuse and on["con"]
    ht_fused = fuse and on["smooth"] and on["v2d"]
    # ... and otherwise the search is a launch of its own (_issue_pair_terms)
    nn_separate = (on["con"] or on["inter"]) and not nn_fused and not nn_full_fused
    # the object's smoothness gradient is formed INSIDE the rigid backward from the camera-space vertices the face setup
    # wrote (same floats as the unit gradient of the smoothness launch times its weight): on the step-1 sets this chain
    # then needs nothing from the side stream before the join - one cross-queue edge less on the iteration's tail
    sm_in = on["smooth"] and on["sil"] and Vo <= 24576
    side_terms = on["con"] or (on["inter"] and optimize_object_scale) or (on["smooth"] and not sm_in) or not on["sil"]
    # scheduling hint baked into the captured launches: with the collision / contact terms the hand-side stream is
    # the longer chain and the persistent edge sweeps should leave it more of the GPU (same results either way;
    # same-box A/B on cfg3, round 2 before the launch fusions: 1280 -> 4030, 768 -> 4130, 512 -> 4194 it/s; after them,
    # with the raster ballast below: 512 -> 4408, 768 -> 4552, 1024 -> 4537, 1280 -> 4512)
    sweep_blocks = 768 if (on["col"] or on["con"]) and C == 1 else 1024 if pairs_after_lines else 1280
    # same idea for the rasteriser: 8 KB of LDS ballast = 4 workgroups per CU instead of 6 leaves registers for the
    # hand-side kernels (cfg3 one clip: 4347 -> 4500 it/s; cfg2, where that chain is short: 5820 -> 5500, so not there)
    raster_lds_pad = 4096 if (on["col"] or on["con"]) and C == 1 else 0
    # and for the metric-only search of a clip batch: its 1680 small, latency-bound workgroups otherwise take every wave
    # slot of the CUs next to the line expansion (lines 250 -> 226 us, iteration -4.4 % at 3 search workgroups per CU;
    # 2 per CU make the search itself the tail)
    # (34 KB: with the sweep's 30.5 KB workgroups a CU then holds 4 sweeps + 1 search, 2 + 2 or 1 + 3 - the mixes the
    #  40 KB ballast gave next to the 28.9 KB workgroups of the float sweeps; at 40 KB the search found room only
    #  next to THREE sweep workgroups and took 297 instead of 137 us, same-box profile)
    nn_lds_pad = 34816 if C > 1 and not on["con"] else 0
    # ---- what the launch code relies on between these
    # the aux block waits for ev_ras, which only the split forward records (_issue_silhouette_chain)
    assert not (use_aux and (side_own_vo or merge_renders))
    # the silhouette reduction runs exactly once: in the backward's first launch or in the aux block
    assert sil_reduce_in_bwd != use_aux
    # the log row is written exactly once: by Adam, by the aux block, or by the join (_issue_join, _iteration)
    assert log_in_adam == (not use_aux and not shared_scale)
    # one search where the contact or the interaction term needs one, none otherwise (_issue_pair_terms)
    assert nn_fused + nn_full_fused + nn_separate == (1 if on["con"] or on["inter"] else 0)
    # ev_lines is recorded on the silhouette chain only
    assert on["sil"] or not pairs_after_lines
    # `vo_b` has one writer per iteration: the face setup (sil, vo_b is vo), the side copy (sil, side_own_vo) or the side's own
    # transform into `vo` (no sil: vo_b must be vo)
    assert on["sil"] or not side_own_vo
    # the main chain skips the wait for ev_pair only when it reads nothing of the side stream's before the join
    assert side_terms or (on["sil"] and not on["con"] and not (on["inter"] and optimize_object_scale) and
                          (sm_in or not on["smooth"]))
    return LaunchPlan(use_aux, log_in_adam, side_own_vo, merge_renders, sil_reduce_in_bwd, pairs_after_lines, mano_bwd_rigid,
                      pair_fused, fuse, nn_fused, nn_full_fused, ht_fused, nn_separate, sm_in, side_terms, graph_iters,
                      sweep_blocks, raster_lds_pad, nn_lds_pad)


def _morton_order(verts):
    """permutation of the (V,3) vertices along a 3-D Morton curve (10 bits per axis): consecutive vertices are neighbours"""
    v = verts.detach().float().cpu().numpy()
    lo, hi = v.min(0), v.max(0)
    q = np.clip(((v - lo) / np.maximum(hi - lo, 1e-12) * 1023.0).astype(np.int64), 0, 1023)
    code = np.zeros(len(v), np.int64)
    for bit in range(10):
        for ax in range(3):
            code |= ((q[:, ax] >> bit) & 1) << (3 * bit + ax)
    return torch.from_numpy(np.argsort(code, kind="stable").astype(np.int32))


_LOOP_STREAMS = {}


def _loop_streams(device):
    """(capture, side, aux, warm-up) HIP streams of the fused loop, one set per device, pairwise distinct.
    torch hands streams out of a pool of 32 per device, round-robin: a process that builds many steppers eventually draws
    a side stream that IS the capture stream, and a capture in which two 'streams' wait on each other both ways crashes
    the HIP graph runtime at replay.  Steppers replay in stream order anyway, so they share one verified set."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _LOOP_STREAMS:
        got, seen = [], {torch.cuda.current_stream(key).cuda_stream, torch.cuda.default_stream(key).cuda_stream}
        for _ in range(256):
            st = torch.cuda.Stream(device=key)
            if st.cuda_stream not in seen:
                seen.add(st.cuda_stream)
                got.append(st)
            if len(got) == 4:
                break
        assert len(got) == 4, "could not obtain four distinct HIP streams"
        _LOOP_STREAMS[key] = tuple(got)
    return _LOOP_STREAMS[key]


class FusedStepper:
    """The whole optimisation iteration as a fixed sequence of C-ABI kernel launches (no autograd tape, no torch
    arithmetic kernels), captured in a hipGraph:

        forward   rigid(obj) . mano . rigid(hand) . priors . smooth x2 . [collision] . [nn] . [contact] . v2d .
                  silhouettes(project, setup, raster, reduce) . inter . log(total + loss_evolution row)
        backward  sil(masks, sweeps, gather) . inter . weighted sums of the per-loss vertex gradients .
                  rigid_bwd(obj) . rigid_bwd(hand) . mano_bwd . prior terms . Adam

    Same kernels, same detach structure and same weighting as HOMan.forward + autograd (reference homan/homan.py:421-508,
    jointopt.py:178-192); tests/test_model_gpu.py checks the two paths produce the same gradients.  Supports the
    configurations of BASELINE.json (one right hand, optimize_mano=True, optimize_mano_beta=True, persp); anything
    else should use mode="graph".

    `model` is one HOMan, or a list of HOMan of identical shapes = a CLIP BATCH (homan_amd.clipbatch): the C clips are
    then optimised together, every kernel launched once over the C * B frames through the `*_clips` entry points
    (per-clip normalisers, sums, scales, Adam state and log rows; BASELINE cfg4).  Per clip the arithmetic - including
    the order of every floating-point sum - is the single-clip one, so a batched step equals C single steps bit for bit.
    With `shared_scale` (BASELINE cfg5) the object scale is ONE scalar for all clips of all ranks: each clip keeps a
    replica, the replicas' gradients are summed over the local clips and all-reduced over `group` once per iteration
    (one 4-byte RCCL all-reduce on the compute stream between the two captured halves of the iteration), and every
    replica takes the identical Adam step."""

    SLOTS = [slot for slot, _, _ in TERMS]
    # the raster's launch order follows the measured cost of its workgroups from iteration to iteration (hm_tune_raster_reorder,
    # captured with the iteration; same-box A/B: raster 57 -> 45 us inside the graph at one clip, 356 -> 298 us at eight; the
    # iteration: clip batches and the step-2 sets +0.3..1 %, one-clip step-1 fits +4 % in the steady state and over iterations
    # 5-25 - but only since the metric-only search got shorter: while the hand-side chain was as long as the silhouette chain
    # it had been running in the raster's tail and a shorter raster pushed it under the sweeps, -4 %)
    raster_reorder = 1

    def __init__(self, model, loss_weights, lr, max_steps, capture=True, shared_scale=False, group=None, collectives=True):
        from . import constants, ops
        from .clipbatch import ClipBatch, ClipReduceWorkspace
        if float(loss_weights.get("lw_surf_attr", 0)) > 0 or float(loss_weights.get("lw_surf_rep", 0)) > 0:
            # (checked before anything is built: mode="auto" and ClipFitter fall back as they do for sil_mode="soft")
            raise NotImplementedError("lw_surf_attr / lw_surf_rep: the surface contact loss is not in the fused launch sequence "
                                      "(mode='graph' or 'eager')")
        if float(loss_weights.get("lw_depth_obs", 0)) > 0:
            # (one clip or a batch of clips alike: the term lives in HOMan.forward only)
            raise NotImplementedError("lw_depth_obs: the observed-depth term is not in the fused launch sequence "
                                      "(mode='graph' or 'eager')")
        for one in (model.models if isinstance(model, ClipBatch) else model if isinstance(model, (list, tuple)) else [model]):
            if len(one.hand_sides) not in (1, 2):
                raise NotImplementedError("one or two hands per frame")
            if getattr(one, "sil_mode", "nmr") != "nmr":
                # the launch sequence below renders with the hard rasteriser whatever the model says: refuse, so that
                # mode="auto" and ClipFitter fall back to HOMan.forward + autograd in a hipGraph, which honours the mode
                raise NotImplementedError("sil_mode='soft': the fused loop renders hard silhouettes only (mode='graph' or 'eager')")
        m = self.model = model if isinstance(model, ClipBatch) else ClipBatch(model if isinstance(model, (list, tuple))
                                                                             else [model])
        if len({tuple(one.hand_sides) for one in m.models}) != 1:
            raise NotImplementedError("the clips of a batch share the hand side (one MANO model per launch)")
        if m.int_scales_hand.requires_grad or m.hand_proj_mode != "persp":
            raise NotImplementedError("FusedStepper covers optimize_mano_beta=True (the hand scale a buffer) and persp")
        self.h = h = len(m.models[0].hand_sides)
        kinds = {one.losses.inter_type for one in m.models}
        # inter_type "min" (reference losses.py:219-221, a HOMan option its loop cannot select): one hand, one clip
        self.inter_min = kinds == {"min"}
        if len(kinds) != 1 or (self.inter_min and (h > 1 or m.C > 1)):
            raise NotImplementedError("inter_type='min' in the fused loop: one hand, one clip (else mode='graph' or 'eager')")
        if h > 1 and (m.C > 1 or shared_scale):
            raise NotImplementedError("two hands per frame: the fused loop takes one clip at a time (a batch of two-hand "
                                      "clips: one stepper per clip, or mode='graph')")
        lw = self.lw = {k: float(v) for k, v in loss_weights.items()}
        on = self.on = {switch: any(key is not None and lw.get(key, 0.0) > 0 for _, key, sw in TERMS if sw == switch)
                        for _, _, switch in TERMS}
        if on["depth"] and not getattr(m, "ordinal_depth", False):
            # reference homan.py:506-507 calls lossutils.compute_ordinal_depth_loss() without its arguments
            raise TypeError("compute_ordinal_depth_loss() missing 3 required positional arguments: "
                            "'masks', 'silhouettes', and 'depths'")
        self.shared_scale, self.group = bool(shared_scale), group
        # collectives=False: the caller (ShardStepper: several steppers of one rank) issues the broadcast / all-reduce of the
        # tied scale itself - every rank must issue the same number of collectives whatever its number of steppers
        self.collectives = bool(collectives)
        if self.shared_scale and not m.optimize_object_scale:
            raise ValueError("shared_scale needs models built with optimize_object_scale=True")
        self.L, self.c, self.ops = _lib.lib(), constants, ops
        dev = m.translations_object.device
        B, Vo, Vh = m.B, m.verts_object_og.shape[1], 778          # B = frames of the whole batch
        C, NS = m.C, len(self.SLOTS) + 1
        self.B, self.C, self.clip_len, self.NS = B, C, m.clip_len, NS
        self.plan = launch_plan(C, h, Vo, on, self.shared_scale, self.inter_min, m.optimize_object_scale)
        self.Vo, self.Vh, self.P = Vo, Vh, m.mano_pca_pose.shape[1]
        f = lambda *shape: torch.zeros(*shape, device=dev)
        N = self.N = B * h                                        # hand rows (hands interleaved frame-major, homan.py:62-63)
        self.vo, self.vm, self.vh = f(B, Vo, 3), f(N, Vh, 3), f(N, Vh, 3)
        # the side stream's view of the object's vertices (see side_own_vo)
        self.vo_b = torch.zeros_like(self.vo) if self.plan.side_own_vo else self.vo
        self.vals = f(C, NS)                                      # row c: the loss / metric slots of clip c + its total
        w = self.w = {slot: lw[key] if on[switch] else 0 for slot, key, switch in TERMS if key is not None}
        self.weights = torch.tensor([w.get(k, 0.0) for k in self.SLOTS], device=dev)
        self.keys = [slot for slot, _, switch in TERMS if on[switch]]
        # the object's smoothness VALUE (its gradient is formed inside the rigid backward) rides the pair-terms launch of the side
        # stream as a block range.  Until round 6 the step-2 sets launched it on the silhouette chain instead, behind the sweeps
        # (round 3: cfg3 +5 % while the hand side was by far the longer chain); since the hand side's launches were fused the
        # silhouette chain is the longer one there too and an 8 us launch on its tail costs what it lasts: cfg3 5 405 -> 5 510
        # it/s over iterations 20-420, 5 246 -> 5 304 in the steady state (same box, alternated; on a clip batch the old placement
        # lost 4 %).
        # unit gradients / scratch
        self.U_pca, self.U_so, self.U_sh = f(N, self.P), f(C), f(C)
        self.U_smo, self.U_smh, self.U_v2d = f(B, Vo, 3), f(N, Vh, 3), f(N, Vh, 3)
        self.U_colh, self.U_colo, self.U_conh, self.U_cono = f(N, Vh, 3), f(B, Vo, 3), f(N, Vh, 3), f(B, Vo, 3)
        self.G_sil, self.G_int_h, self.G_int_o = f(B, Vo, 3), f(N, Vh, 3), f(B, Vo, 3)
        self.G_o, self.G_h, self.G_mesh = f(B, Vo, 3), f(N, Vh, 3), f(N, Vh, 3)
        self.g_pca_mano, self.g_so_part = f(N, self.P), f(B)
        self.rec = f(N, 8)
        if self.inter_min:
            self.G_min_h, self.tmp_inter, self.rows = f(N, Vh, 3), f(2), torch.arange(B, device=dev)
        if h > 1:
            # two hands: the pair-wise terms see one hand at a time as a dense (B,778,3) array (hand i = rows i::h)
            self.vh_d = [f(B, Vh, 3) for _ in range(h)]
            self.nn_idx_d = [torch.zeros(B, Vh, dtype=torch.int32, device=dev) for _ in range(h)]
            self.nn_d2_d = [f(B, Vh) for _ in range(h)]
            self.U_conh_d, self.U_cono_d = [f(B, Vh, 3) for _ in range(h)], [f(B, Vo, 3) for _ in range(h)]
            self.U_colh2, self.U_col_d = f(N, Vh, 3), [f(B, Vh, 3) for _ in range(4)]      # (h0|h1), (h0|obj), (h1|obj): hand sides
            self.U_colo_d = f(B, Vo, 3)
            self.rec_d, self.G_int_o_d = [f(B, 8) for _ in range(h)], [f(B, Vo, 3) for _ in range(h)]
            self.tmp_h, self.tmp_col = f(h, 4), f(3)
            self.rws_h = [ClipReduceWorkspace(dev, 1) for _ in range(h)]
            self.hand_ctx = [m.mano_model.ctx_mean if sd == "right" else m.mano_model._left_ctx(False)
                             for sd in m.models[0].hand_sides]
        self.nn_idx = torch.zeros(B, Vh, dtype=torch.int32, device=dev)
        # the metric-only search's seed pairs (per frame the vertex pair that held the minimum at the last iteration: its distance
        # now bounds this iteration's minimum before anything is scanned; hm_nn_fwd_rigid_clips).  Scheduling data only.
        self.nn_seed = torch.zeros((2 + (Vh + 127) // 128) * B, dtype=torch.int32, device=dev)
        self.nn_d2 = f(B, Vh)
        self.obj_order = _morton_order(m.verts_object_og[0]).to(dev)      # spatial sort of the rigid mesh (metric-only search)
        # ... and of the hand: its template's vertices in the same kind of order, so that the 128 hand vertices of a search
        # workgroup are a patch of the hand, not a sample of all of it (articulation moves the patches, it does not mix them)
        side = m.models[0].hand_sides[0]
        self.mctx = m.mano_model.ctx_mean if side == "right" else m.mano_model._left_ctx(False)      # (see ManoModel)
        self.hand_order = _morton_order(self.mctx.tensors[0]).to(dev)
        self._install_clip_constants()       # sil_K / sil_keep / sil_ref, obj_spheres
        self.pooled = f(B, m.sil_ctx.S, m.sil_ctx.S)
        self.up_sil, self.up_inter = torch.tensor([w["loss_sil_obj"]], device=dev), torch.tensor([w["loss_inter"]], device=dev)
        if self.on["depth"] and h > 1:
            # two hands per frame: the three layers [object, hand 0, hand 1] of reference homan.py:384-419, every unordered pair
            # through the two-layer kernels, one normaliser for the scene (lossutils.py:133-169; ops.ordinal_depth_loss_layers is
            # the autograd form of what _forward_backward_hands issues)
            ctxs, masks = m.models[0].depth_layers()
            if ctxs[0].padded:
                raise NotImplementedError("the fused loop renders the depth images at image_size % 32 == 0; other sizes: "
                                          "mode='graph' or 'eager'")
            self.dlayers = list(zip(ctxs, [Vo] + [Vh] * h, masks))
            self.dpairs = [(a, b) for a in range(h + 1) for b in range(a + 1, h + 1)]
            Sd = ctxs[0].S
            self.dl_sil, self.dl_dep = [f(B, Sd, Sd) for _ in self.dlayers], [f(B, Sd, Sd) for _ in self.dlayers]
            self.dl_g = [f(B, Sd, Sd) for _ in self.dlayers]
            self.dp_part, self.dp_rec = [f(B * 8) for _ in self.dpairs], [f(8) for _ in self.dpairs]
            self.dp_out, self.dp_up = [f(1) for _ in self.dpairs], [f(1) for _ in self.dpairs]
            self.dp_g = [(f(B, Sd, Sd), f(B, Sd, Sd)) for _ in self.dpairs]
            self.rws_dp = [ClipReduceWorkspace(dev, 1) for _ in self.dpairs]
            self.G_dep_o, self.G_dep_h_d, self.G_dep_h = f(B, Vo, 3), [f(B, Vh, 3) for _ in range(h)], f(N, Vh, 3)
        elif self.on["depth"]:
            # ordinal depth term (reference homan.py:384-419, opt-in): object and hand rendered with depth at the full-image
            # camera, the pair-wise ordinal loss, and its gradient back through both depth images to the camera-space vertices
            self.dctx = m.depth_contexts()
            ctx_o, ctx_h = self.dctx[0], self.dctx[1]
            if ctx_o.padded:
                raise NotImplementedError("the fused loop renders the depth images at image_size % 32 == 0; other sizes: "
                                          "mode='graph' or 'eager'")
            Sd = ctx_o.S
            self.d_sil_o, self.d_dep_o, self.d_sil_h, self.d_dep_h = f(B, Sd, Sd), f(B, Sd, Sd), f(B, Sd, Sd), f(B, Sd, Sd)
            self.d_go, self.d_gh, self.d_part, self.d_rec = f(B, Sd, Sd), f(B, Sd, Sd), f(B * 8), f(C, 8)
            # non-zero structure of the two gradient images, one byte per (frame, pixel row, 64-pixel segment): the depth-map
            # backward skips faces and frames that touch no flagged segment (the term is zero wherever render and annotation
            # agree on the order); ones = "walk everything" until the first backward has written them
            self.d_flags = torch.ones(2, B * Sd * (Sd // 64), dtype=torch.uint8, device=dev) if Sd % 64 == 0 else None
            self.rws_depth = ClipReduceWorkspace(dev, C)
            self.G_dep_o, self.G_dep_h = f(B, Vo, 3), f(B, Vh, 3)
            self.up_depth = torch.tensor([w["loss_depth"]], device=dev)
        # static gradient buffers for exactly the parameters that receive gradients in this configuration
        for p in m.parameters():
            p.grad = None
        gp = [m.translations_object, m.rotations_object, m.translations_hand, m.rotations_hand]
        if m.optimize_mano:          # (optimize_mano=False, the reference function's own default: the hand mesh is the
            gp += [m.mano_pca_pose, m.mano_rot, m.mano_trans, m.mano_betas]      # constant `verts_hand_og`, homan.py:357-358)
        if m.optimize_object_scale:
            gp.append(m.int_scales_object)
        for p in gp:
            p.grad = torch.zeros_like(p)
        self._build_optimizers(lr)
        self.log_buf = torch.zeros(max_steps, C, NS, device=dev)
        self.max_steps = max_steps
        self.rigid_ws_h, self.rigid_ws_o = (torch.zeros(self.L.hm_rigid_workspace_bytes(n), dtype=torch.uint8, device=dev)
                                            for n in (N, B))
        self.mano_state = torch.empty(self.L.hm_mano_state_bytes(N), dtype=torch.uint8, device=dev)
        self.graph = self.graph_b = self.graph_k = None
        self.cap_stream, self.side, self.aux, side = _loop_streams(dev)
        self.ev_vo, self.ev_pair, self.ev_sil, self.ev_fwd, self.ev_ras = (torch.cuda.Event() for _ in range(5))
        self.ev_dep, self.ev_dgrad, self.ev_lines = (torch.cuda.Event() for _ in range(3))
        self.reduce_ws_b = ClipReduceWorkspace(dev, C)
        # (the terms of the fused pair-terms launch run side by side: a reduce workspace each)
        self.reduce_ws_c, self.reduce_ws_d, self.reduce_ws_e = (ClipReduceWorkspace(dev, C) for _ in range(3))
        if self.shared_scale:
            self._sync_shared_scale_start()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.forward_backward()              # warm-up, no optimiser step
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if self.on["sil"]:
            m.sil_ctx.calibrate()                # cost-sorted launch orders from the current state (scheduling only)
        if self.on["depth"] and self.h == 1:
            # the HAND's depth render gets a cost-sorted launch order and its near-winding hint too (its active workgroups started
            # up to 32 us late behind background regions of the static order, profiles/r06_raster_trace_depth.txt; with the
            # object's two renders in one launch the hand side is the longer chain: cfg2 + depth 4 151 -> 4 215 it/s, same box);
            # the object's depth render keeps the static order (sorted: +-0 alone, -1 % with the hand's)
            self.dctx[1].calibrate()
        if capture:
            # the hints are per-thread values read when a launch is issued (= captured): set, capture, restore - whatever
            # happens in between (a capture that raises must not leave them changed for the next stepper)
            tune, p, prev = _lib.lib(), self.plan, []
            try:
                for name, value in (("hm_tune_sweep_blocks", p.sweep_blocks), ("hm_tune_raster_lds_pad", p.raster_lds_pad),
                                    ("hm_tune_raster_reorder", self.raster_reorder), ("hm_tune_nn_lds_pad", p.nn_lds_pad)):
                    prev.append((name, getattr(tune, name)(value)))
                self.graph = _lib.new_graph()
                with torch.cuda.graph(self.graph, stream=self.cap_stream):
                    self.forward_backward(log=not p.log_in_adam)
                    if not self.shared_scale:
                        self._capture_step()
                if self.shared_scale:        # the all-reduce of the scale gradient runs between two captured halves
                    self.graph_b = _lib.new_graph()
                    with torch.cuda.graph(self.graph_b, stream=self.cap_stream):
                        self._spread_shared_scale_grad()
                        self.opt.step(zero_grad=False)
                elif p.graph_iters > 1:
                    # K iterations in ONE graph: the boundary between two replays (the executor's own start-up, a few
                    # microseconds of an iteration that lasts 160) is paid once per K iterations; run() replays this graph
                    # for every full K and the one-iteration graph for the rest - the same launches either way
                    self.graph_k = _lib.new_graph()
                    with torch.cuda.graph(self.graph_k, stream=self.cap_stream):
                        self._capture_iterations(p.graph_iters)
            finally:
                for name, value in reversed(prev):
                    getattr(tune, name)(value)

    # ---- other clips into the resident stepper
    def reload(self, clip_inputs):
        """`clip_inputs`: one dict of HOMan data arguments per clip of the batch (what `collate_inputs` returns, + camintr),
        clips of exactly the shapes and topology this stepper was built for.  Everything that depends on the clip is copied in
        place (ClipBatch.load_clips, then the stepper's own constants) and everything that depends on the FIT is reset;
        buffers, workspaces, streams and the captured hipGraph are reused as they are.  The next `run(steps)` is the fit of the
        new clips, bit-identical to the fit a freshly built stepper would make (tests/test_clip_fitter_gpu.py).
        Carried across clips on purpose, none of it able to change a result:
          nn_seed   per frame the vertex pair that held the minimum at the last launch.  The search evaluates that pair's
                    distance at the CURRENT vertices: the distance of a real pair, so an upper bound of the minimum it then finds
                    exactly (nn_min_body, csrc/pair_bodies.h); indices out of range are ignored.  Any pair prunes correctly.
          d_flags   written in full (1 or 0 per segment) by hm_ordinal_depth_bwd_flags of an iteration BEFORE that iteration's
                    hm_depth_bwd_sparse reads them (csrc/raster_depth.hip): the previous clip's are never read.
          the raster's cost order (calibrate(), hm_tune_raster_reorder)   a permutation of the (frame, region) workgroups of
                    k_raster_fwd, each of which writes its own region's pixels only (csrc/raster_fwd.hip): any order, same image."""
        self.model.load_clips(clip_inputs)
        self._install_clip_constants()
        self._reset_fit()
        if self.shared_scale:
            self._sync_shared_scale_start()

    def _install_clip_constants(self):
        """What the stepper itself derives from the clips' data: assigned at construction, copied in place on reload.
        sil_K / sil_keep / sil_ref: silhouettes at a size off the kernels' 32-pixel tile grid (the reference's REND_SIZE is 256)
        are rendered on the next multiple, with the first two rows of K rescaled and the masks padded with keep = 0
        (ops.SilhouetteContext); on the grid they ARE the batch's tensors.  obj_spheres: see _group_spheres."""
        m, sx = self.model, self.model.sil_ctx
        with torch.no_grad():
            new = dict(sil_K=sx.K_eff(m.camintr_rois_object).contiguous(), sil_keep=sx.pad(m.keep_mask_object),
                       sil_ref=sx.pad(m.ref_mask_object), obj_spheres=self._group_spheres())
            for name, t in new.items():
                own = getattr(self, name, None)
                if own is None:
                    setattr(self, name, t)
                elif own.data_ptr() != t.data_ptr():
                    own.copy_(t)

    def _reset_fit(self):
        """everything that belongs to the fit, not to the clip: Adam moments and step counter, loss slots, gradients"""
        self.opt.reset()
        self.vals.zero_()
        for p in self.model.parameters():
            if p.grad is not None:
                p.grad.zero_()

    def _group_spheres(self):
        """Bounding spheres, in MESH space, of the groups of 64 object vertices in `obj_order`, per frame (a clip's frames share
        one mesh, the clips of a batch need not): (B, groups, 4), centre = mean, radius = farthest vertex.  The search carries
        them into camera space with the frame's rigid transform instead of reducing the transformed vertices of every group in
        every workgroup.  (Repeats of a real vertex pad the last group: masked out of the mean, they change nothing.)"""
        m, Vo, B = self.model, self.Vo, self.B
        ng = (Vo + 63) // 64
        vs = m.verts_object_og.detach()[:, self.obj_order.long()]
        pad = ng * 64 - Vo
        valid = torch.ones(Vo + pad, dtype=torch.bool, device=vs.device)
        if pad:
            vs = torch.cat([vs, vs[:, -1:].expand(-1, pad, -1)], 1)
            valid[Vo:] = False
        grp = vs.reshape(B, ng, 64, 3)
        wgt = valid.reshape(1, ng, 64, 1).float()
        ctr = (grp * wgt).sum(2) / wgt.sum(2)
        rad = ((grp - ctr[:, :, None]) ** 2).sum(-1).sqrt().amax(2)
        return torch.cat([ctr, rad[..., None]], -1).contiguous()

    # ---- shared object scale (BASELINE cfg5): C local replicas of one scalar, kept identical on every rank
    def _dist_on(self):
        import torch.distributed as dist
        return (self.collectives and dist.is_available() and dist.is_initialized() and
                dist.get_world_size(self.group) > 1)

    def _sync_shared_scale_start(self):
        import torch.distributed as dist
        s = self.model.int_scales_object
        with torch.no_grad():
            s0 = s.data[:1].clone()              # one element on the wire whatever the number of local clips
            if self._dist_on():
                from .dist import broadcast_shared_scalar, group_src
                broadcast_shared_scalar(s0, group_src(self.group), self.group)
            s.copy_(s0.expand_as(s))
        self.g_shared = torch.zeros(1, device=s.device)

    def _reduce_shared_scale_grad(self):
        """One fp32 per step over xGMI: sum over ranks of (sum over local clips of d loss / d scale), on the compute
        stream, no host synchronisation."""
        if self._dist_on():
            from .dist import sync_shared_scalar_grad
            sync_shared_scalar_grad(self.g_shared, self.group)

    def _spread_shared_scale_grad(self):
        # every replica receives the global sum (identical Adam steps keep the replicas bit-identical)
        g = self.model.int_scales_object.grad
        g.copy_(self.g_shared.expand_as(g))

    def _slot(self, name):
        """device address of slot `name` of clip 0; clip c is `self.NS` floats further (the kernels' out_stride)"""
        i = self.SLOTS.index(name)
        return self.vals.data_ptr() + 4 * i

    def forward_backward(self, log=False):
        """Two concurrent branches (fork/join on HIP streams, captured as parallel branches of the hipGraph):
        A (calling stream): object transform, silhouettes forward/backward, object gradients;
        B (side stream):    MANO, hand transform, priors, 2-D / smoothness / collision / contact / interaction losses,
                            hand gradients, MANO backward.
        B waits for the object vertices before the pair-wise losses, A waits for B's object-side gradient terms, both
        join before the log row and the Adam step.  Every launch covers all the clips of the batch (clip_len frames
        each, per-clip scalars NS floats apart in `vals`).  The launches are ISSUED in the order of the builders below - the order
        is part of the design: the graph executor maps the captured branches onto its queues by it (EXPERIMENTS.md)."""
        if self.h > 1:
            return self._forward_backward_hands(log)
        self.side.wait_stream(torch.cuda.current_stream())
        self._issue_silhouette_chain()
        with torch.cuda.stream(self.side):
            self._issue_hand_forward()
            # (issued in this order on purpose - with the depth term too: its renders BEFORE the pair-wise terms put the hand's
            #  raster next to the silhouette raster, cfg2 + depth 4 000 -> 3 790 it/s, EXPERIMENTS r6)
            self._issue_pair_terms()
            if self.on["depth"]:
                self._issue_depth_terms()
            self._issue_hand_backward(log)
        self._issue_object_backward()
        self._issue_join(log)

    # ---- hooks of the capture (tools/chain_only.py overrides them for its measurement-only launch graphs)
    def _build_optimizers(self, lr):
        self.opt = HmAdam(parameter_groups(self.model, lr))

    def _capture_step(self):
        """the optimiser step behind one captured iteration"""
        self.opt.step(zero_grad=False, log=self._adam_log())

    def _capture_iterations(self, K):
        """K iterations of the second graph"""
        for _ in range(K):
            self.forward_backward(log=not self.plan.log_in_adam)
            self._capture_step()

    def _aux_block(self, log):
        """the silhouette reduction and the log row on the third stream (clip batches)"""
        m, L, P, ck = self.model, self.L, _lib.ptr, _lib.check
        if not self.plan.use_aux:
            return
        # the silhouette reduction and the log row run on a third stream, off both chains.  (Only this: HIP stream
        # capture crashes when two captured streams wait for each other's events in both directions, and the hipGraph
        # executor maps richer fork patterns onto its hardware queues in orders that serialise the branches -- both
        # measured.  WHERE this block is issued matters too: issued after the hand-side backward, the executor runs it
        # behind that chain, +20 us on the iteration.)
        with torch.cuda.stream(self.aux):
            self.aux.wait_event(self.ev_fwd)
            if self.on["sil"]:
                self.aux.wait_event(self.ev_ras)
                ck(m.sil_ctx.reduce(keep_sum=m.keep_sum, loss_out=self._slot("loss_sil_obj"), clip_len=self.clip_len,
                                    out_stride=self.NS, stream=self.aux.cuda_stream), "sil_reduce")
            if log:
                ck(L.hm_log_total_clips(P(self.vals), P(self.weights), len(self.SLOTS), P(self.opt.step_t),
                                        self.max_steps, P(self.log_buf), self.C, self.aux.cuda_stream), "log")

    def _issue_silhouette_chain(self):
        """A, first half: face setup (+ camera-space vertices), fork point, rasteriser, [object depth render], line expansion + sweeps"""
        m, L, ck, on, plan = self.model, self.L, _lib.check, self.on, self.plan
        CL, NS, sctx, main = self.clip_len, self.NS, m.sil_ctx, torch.cuda.current_stream()
        sa = main.cuda_stream
        # ---------------- A: silhouettes forward + backward (the critical chain: nothing else rides it; the object's rigid
        # transform is applied inside the face setup, the other losses get the vertices from the side stream)
        if on["sil"]:
            # the render: the object's rigid pose applied in the face setup, which also writes the camera-space vertices self.vo
            render = dict(verts=m.verts_object_og, K=self.sil_K, keep=self.sil_keep, ref=self.sil_ref, pooled=self.pooled,
                          rigid_rot6d=m.rotations_object, rigid_trans=m.translations_object, rigid_scale=m.int_scales_object,
                          rigid_abs=1, persistent_outputs=1, clip_len=CL, cam_verts_out=self.vo)
            fwd_args = dict(render, out_stride=NS, stream=sa)
            if plan.merge_renders:
                # with the ordinal depth term: the silhouette render and the OBJECT's depth render (the same mesh and pose at the
                # full-image camera) as ONE face-setup launch and ONE raster launch (hm_sil_fwd_multi: per render the arguments
                # of the two calls below, the depth render forming its vertices from the pose like the silhouette render does -
                # the same floats as self.vo); each render keeps its workspace, the backward passes are unchanged
                # the DEPTH render's workgroups first: it lasts as long as its slowest workgroup (37 us: one region with 240
                # candidates, profiles/r06_raster_trace_depth.txt), which then runs under the silhouette render's two rounds
                # instead of behind them (cfg2 + depth 4 208 -> 4 303 it/s, same box; results do not depend on the order)
                arr = _lib.sil_renders([
                    self.dctx[0].render_fields(verts=m.verts_object_og, K=m.camintr, pooled=self.d_sil_o, pooled_depth=self.d_dep_o,
                                               rigid_rot6d=m.rotations_object, rigid_trans=m.translations_object,
                                               rigid_scale=m.int_scales_object, rigid_abs=1, persistent_outputs=1, clip_len=CL),
                    sctx.render_fields(**render)])
                ck(L.hm_sil_fwd_multi(arr, 2, 1, sa), "sil_fwd_multi(setup)")
                self.ev_sil.record(main)
                ck(L.hm_sil_fwd_multi(arr, 2, 2, sa), "sil_fwd_multi(raster)")
                self.ev_dep.record(main)
            elif plan.side_own_vo:
                ck(sctx.forward(**fwd_args), "sil_fwd")      # (no successor on the side stream: see side_own_vo)
            else:
                # the face setup (which also writes the camera-space vertices self.vo), the fork of the side stream, then the
                # rasteriser: the pair-wise losses do not wait for the raster and the raster has one successor on its chain
                ck(sctx.forward(phases=1, **fwd_args), "sil_fwd(setup)")
                self.ev_sil.record(main)
                ck(sctx.forward(phases=2, **fwd_args), "sil_fwd(raster)")
                if plan.use_aux:
                    self.ev_ras.record(main)     # the tile partials of the fused loss, for the reduction on the third stream
            if on["depth"] and not plan.merge_renders:
                # the OBJECT's depth render of the ordinal depth term rides this chain, right behind the silhouette raster (its
                # vertices are the face setup's): the hand's render runs on the side stream meanwhile - two renders after each
                # other there made the hand side twice as long as this chain
                self._depth_render(self.vo, self.dctx[0], self.d_sil_o, self.d_dep_o, sa)
                self.ev_dep.record(main)
            # (no vertex gather; the loss / IoU values come out of its first launch)
            bwd_args = dict(upstream=self.up_sil, keep_sum=m.keep_sum, clip_len=CL,
                            loss_out=self._slot("loss_sil_obj") if plan.sil_reduce_in_bwd else None, out_stride=NS, stream=sa)
            mode = 2 if self.lw["lw_sil_obj"] > 0 else 1
            if plan.pairs_after_lines:
                # a clip batch: the line expansion - latency-bound, and the kernel of this chain that suffers most from
                # neighbours holding its wave slots - runs ALONE; the pair-wise terms of the side stream wait for its end
                ck(sctx.backward(self.vo, self.sil_K, mode, phases=1, **bwd_args), "sil_bwd(lines)")
                self.ev_lines.record(main)
                ck(sctx.backward(self.vo, self.sil_K, mode, phases=2, **bwd_args), "sil_bwd(sweeps)")
            else:
                ck(sctx.backward(self.vo, self.sil_K, mode, **bwd_args), "sil_bwd")

    def _hand_term_args(self):
        """the hand-only reductions' share of the arguments of hm_hand_terms_fwd_clips / hm_pair_terms_fwd_clips"""
        m, P, on = self.model, _lib.ptr, self.on
        return (P(m.ref_verts2d_hand), float(m.image_size), P(self.U_v2d), self._slot("loss_v2d_hand"), P(self.U_smh),
                self._slot("loss_smooth_hand"), P(m.mano_pca_pose) if (on["pca"] or on["so"] or on["sh"]) else None,
                self.P * self.clip_len,                                         # PCA entries of one clip
                P(m.int_scales_object), P(m.int_scale_object_mean), P(m.int_scales_hand),
                P(m.int_scale_hand_mean), P(self.U_pca), P(self.U_so), P(self.U_sh), self._slot("loss_pca"))

    def _issue_hand_forward(self):
        """B: object / hand vertices, the hand-only terms, then the waits that place the pair-wise terms next to the silhouette chain"""
        m, L, P, ck, on, plan = self.model, self.L, _lib.ptr, _lib.check, self.on, self.plan
        B, Vo, Vh, CL, NS, side, sb = self.B, self.Vo, self.Vh, self.clip_len, self.NS, self.side, self.side.cuda_stream
        rws_b, pca = P(self.reduce_ws_b.buf), m.mano_pca_pose
        if not on["sil"]:    # (with the silhouette term the face setup of hm_sil_fwd has written self.vo already)
            ck(L.hm_rigid_fwd_clips(P(m.verts_object_og), P(m.rotations_object), P(m.translations_object),
                                    P(m.int_scales_object), 1, B, Vo, None, P(self.vo), CL, sb), "rigid_fwd(obj)")
        elif plan.side_own_vo:
            ck(L.hm_rigid_fwd_clips(P(m.verts_object_og), P(m.rotations_object), P(m.translations_object),
                                    P(m.int_scales_object), 1, B, Vo, None, P(self.vo_b), CL, sb), "rigid_fwd(obj, side copy)")
        if m.optimize_mano:
            ck(L.hm_mano_fwd_clips(self.mctx.ptrs, P(pca), self.P, P(m.mano_rot), P(m.mano_betas), P(m.mano_trans), B,
                                   P(self.vm), None, P(m.rotations_hand), P(m.translations_hand), P(m.int_scales_hand),
                                   P(self.vh), P(self.mano_state), CL, sb), "mano_fwd + rigid(hand)")
        else:           # the hand mesh is the constant `verts_hand_og` (reference homan.py:357-358): rigid transform only
            ck(L.hm_rigid_fwd_clips(P(m.verts_hand_og), P(m.rotations_hand), P(m.translations_hand),
                                    P(m.int_scales_hand), 0, B, Vh, None, P(self.vh), CL, sb), "rigid_fwd(hand)")
        if on["smooth"] and on["v2d"]:       # the three hand-only reductions in one launch
            if not plan.ht_fused:            # (else they ride the pair-terms launch)
                ht_args = self._hand_term_args()
                ck(L.hm_hand_terms_fwd_clips(P(self.vh), P(m.camintr), 1, ht_args[0], ht_args[1], B, Vh, *ht_args[2:], rws_b,
                                             CL, NS, sb), "hand terms")
        else:
            if on["pca"] or on["so"] or on["sh"]:
                ck(L.hm_priors_fwd_clips(P(pca), self.P * CL, P(m.int_scales_object), P(m.int_scale_object_mean),
                                         P(m.int_scales_hand), P(m.int_scale_hand_mean), P(self.U_pca), P(self.U_so),
                                         P(self.U_sh), self._slot("loss_pca"), self.C, NS, sb), "priors")
            if on["smooth"]:
                ck(L.hm_smooth_fwd_clips(P(self.vh), B, Vh, 1, P(self.U_smh), self._slot("loss_smooth_hand"), rws_b,
                                         CL, NS, sb), "smooth(hand)")
            if on["v2d"]:
                ck(L.hm_v2d_fwd_clips(P(self.vh), P(m.camintr), 1, P(m.ref_verts2d_hand), float(m.image_size), B, Vh,
                                      P(self.U_v2d), self._slot("loss_v2d_hand"), rws_b, CL, NS, sb), "v2d")
        if on["sil"]:
            if not plan.side_own_vo:
                side.wait_event(self.ev_sil)     # self.vo: camera-space object vertices from the calling stream
            if plan.pairs_after_lines:
                side.wait_event(self.ev_lines)   # (scheduling only, see the silhouette chain above)

    def _issue_pair_terms(self):
        """B: collision, nearest-vertex search, contact, interaction (centroid or min) - on the side stream"""
        m, L, P, ck, c, on, w, plan = self.model, self.L, _lib.ptr, _lib.check, self.c, self.on, self.w, self.plan
        B, Vo, Vh, CL, NS, side, sb = self.B, self.Vo, self.Vh, self.clip_len, self.NS, self.side, self.side.cuda_stream
        rws_b, cctx = P(self.reduce_ws_b.buf), m.collision_ctx
        fuse, nn_fused, nn_full_fused = plan.fuse, plan.nn_fused, plan.nn_full_fused
        if on["col"]:
            # (one clip, step-2 sets: the collision chain alone here and the rest of the hand side on the third stream, which
            #  then joins the calling stream - the HIP graph runtime crashes at replay when a forked stream rejoins the SIDE
            #  stream - measured +-0.4 % on cfg3: both chains already share a work-bound GPU)
            ck(L.hm_collision_fwd_clips(P(self.vh), P(cctx.f0), Vh, cctx.f0.shape[0], P(self.vo_b), P(cctx.f1), Vo,
                                        cctx.f1.shape[0], B, c.SDF_SCALE_FACTOR, P(self.U_colh), P(self.U_colo),
                                        self._slot("loss_collision"), P(cctx.ws), CL, NS, sb), "collision")
        if on["smooth"] and not fuse:
            ck(L.hm_smooth_fwd_clips(P(self.vo_b), B, Vo, 1, P(self.U_smo), self._slot("loss_smooth_obj"), rws_b, CL, NS,
                                     sb), "smooth(obj)")
        def search_and_contact():
            if plan.nn_separate:
                # (without the contact term only the logged distance is needed: metric-only search - its group table
                #  covers 4096 object vertices, larger meshes take the full search for the same number)
                full = on["con"] or Vo > 4096 or self.inter_min      # ('min' names the closest PAIR: indices needed)
                ck(L.hm_nn_fwd_rigid_clips(P(self.vh), P(self.vo_b), B, Vh, Vo, P(self.nn_idx) if full else None,
                                           P(self.nn_d2) if full else None, self._slot("handobj_maxdist"), rws_b, CL, NS,
                                           P(self.obj_order), P(self.obj_spheres), P(m.rotations_object),
                                           P(m.translations_object), P(m.int_scales_object), P(self.hand_order),
                                           None if full else P(self.nn_seed), sb), "nn")
            if on["con"]:
                ck(L.hm_contact_fwd_clips(P(self.vh), P(self.vo_b), P(self.nn_idx), B, Vh, Vo, c.COLLISION_THRESH,
                                          P(self.U_conh), P(self.U_cono), self._slot("loss_contact"), rws_b, CL, NS, sb),
                   "contact")
        # (the search on a third stream at one clip / step 1: +1 %; -9 % on an 8-clip batch.  Search + contact as a third
        #  branch next to the collision term: the HIP graph runtime crashes at replay when two side branches wait for
        #  each other's events.  Capturing the hand-side forward kernels BEFORE the silhouette chain: -38 %.)
        if not nn_full_fused:
            search_and_contact()
        if fuse:
            ck(L.hm_pair_terms_fwd_clips(P(self.vh), P(self.vo_b), P(m.camintr), B, Vh, Vo,
                                         self._slot("handobj_maxdist") if (nn_fused or nn_full_fused) else None,
                                         P(self.obj_order), rws_b,
                                         c.INTERACTION_BBOX_EXPANSION, float(c.INTERACTION_Z_THRESH), P(self.rec),
                                         self._slot("loss_inter"), P(self.reduce_ws_c.buf),
                                         P(self.U_smo) if on["smooth"] else None,
                                         self._slot("loss_smooth_obj") if on["smooth"] else None, P(self.reduce_ws_d.buf),
                                         *(self._hand_term_args() if plan.ht_fused else
                                           (None, 0.0, None, None, None, None, None, 0, None, None, None, None, None, None, None, None)),
                                         P(self.reduce_ws_e.buf), P(self.obj_spheres), P(m.rotations_object),
                                         P(m.translations_object), P(m.int_scales_object), P(self.hand_order),
                                         P(self.nn_idx) if nn_full_fused else None, P(self.nn_d2) if nn_full_fused else None,
                                         P(self.nn_seed), CL, NS, sb),
               "pair terms")
            if nn_full_fused:
                search_and_contact()          # (the contact launches only: the search ran above)
        elif on["inter"]:
            ck(L.hm_inter_fwd_clips(P(self.vh), P(self.vo_b), P(m.camintr), B, Vh, Vo, c.INTERACTION_BBOX_EXPANSION,
                                    float(c.INTERACTION_Z_THRESH), P(self.rec),
                                    P(self.tmp_inter) if self.inter_min else self._slot("loss_inter"), rws_b, CL,
                                    NS, sb), "inter")
        if on["inter"] and self.inter_min:
            with torch.cuda.stream(side):
                # inter_type "min" (losses.py:219-221): on the frames the gate lets through (rec[:, 0], same gate as the
                # centroid form) the smallest squared vertex distance; the search names the pair, the term and its
                # gradient live on the two vertices (hand: rigid pose only - the mesh-detached twin; object: only with a free
                # scale).  A handful of small device ops, same expressions as Losses.compute_interaction_loss.
                flags = (self.rec[:, 0] != 0).float()
                i_star = self.nn_d2.argmin(1)
                j_star = self.nn_idx.gather(1, i_star[:, None]).long()[:, 0]
                diff = self.vh[self.rows, i_star] - self.vo_b[self.rows, j_star]
                self.vals[0, self.SLOTS.index("loss_inter")] = ((diff * diff).sum(1) * flags).sum()
                pull = (2.0 * w["loss_inter"]) * diff * flags[:, None]
                self.G_min_h.zero_()
                self.G_min_h[self.rows, i_star] = pull
                if m.optimize_object_scale:
                    self.G_int_o.zero_()
                    self.G_int_o[self.rows, j_star] = -pull
        elif on["inter"] and m.optimize_object_scale:      # the object side of the term reaches the (free) scale: per-vertex form
            ck(L.hm_inter_bwd(P(self.rec), P(self.up_inter), B, Vh, Vo, None, P(self.G_int_o), sb), "inter_bwd")

    def _issue_depth_terms(self):
        """B: ordinal depth term - hand render, pair term per clip, the two depth-map backward passes"""
        m, L, P, ck, on = self.model, self.L, _lib.ptr, _lib.check, self.on
        B, Vo, Vh, CL, NS, side, sb = self.B, self.Vo, self.Vh, self.clip_len, self.NS, self.side, self.side.cuda_stream
        if on["depth"]:
            ctx_o, ctx_h, m_o, m_h = self.dctx
            Sd, K = ctx_o.S, P(m.camintr)
            self._depth_render(self.vh, ctx_h, self.d_sil_h, self.d_dep_h, sb)
            if on["sil"]:
                side.wait_event(self.ev_dep)        # the object's depth image, from the calling stream
            else:
                self._depth_render(self.vo, ctx_o, self.d_sil_o, self.d_dep_o, sb)
            rw_bytes = L.hm_reduce_workspace_bytes()
            for ci in range(self.C):      # per clip: the term normalises over the clip's own pairs and mask counts
                fr = slice(ci * CL, (ci + 1) * CL)
                args = (P(self.d_dep_o[fr]), P(self.d_dep_h[fr]), P(self.d_sil_o[fr]), P(self.d_sil_h[fr]), P(m_o[fr]),
                        P(m_h[fr]), CL, Sd)
                ck(L.hm_ordinal_depth_fwd(*args, P(self.d_part[8 * ci * CL:]), P(self.d_rec[ci]),
                                          self._slot("loss_depth") + 4 * NS * ci,
                                          self.rws_depth.buf.data_ptr() + rw_bytes * ci, sb), "ordinal depth")
                if self.d_flags is not None:
                    fo = ci * CL * Sd * (Sd // 64)
                    ck(L.hm_ordinal_depth_bwd_flags(*args, P(self.d_rec[ci]), P(self.up_depth), P(self.d_go[fr]), P(self.d_gh[fr]),
                                                    self.d_flags[0].data_ptr() + fo, self.d_flags[1].data_ptr() + fo, sb),
                       "ordinal depth bwd")
                else:
                    ck(L.hm_ordinal_depth_bwd(*args, P(self.d_rec[ci]), P(self.up_depth), P(self.d_go[fr]), P(self.d_gh[fr]),
                                              sb), "ordinal depth bwd")
            # the two depth images' backward passes are independent: the hand's stays here, the object's goes to the
            # calling stream (idle between its sweeps and the object's gradient launch) when that stream made the render
            self.ev_dgrad.record(side)
            for verts, ctx, V_, g, G, li in (((self.vh, ctx_h, Vh, self.d_gh, self.G_dep_h, 1),) if on["sil"] else
                                             ((self.vo, ctx_o, Vo, self.d_go, self.G_dep_o, 0),
                                              (self.vh, ctx_h, Vh, self.d_gh, self.G_dep_h, 1))):
                ck(L.hm_depth_bwd_sparse(P(verts), K, B, V_, ctx.F, Sd, 1.0, P(g), P(ctx.adj_off), P(ctx.adj_items), P(G),
                                         P(self.d_flags[li]) if self.d_flags is not None else None, P(ctx.workspace), sb),
                   "depth bwd")

    def _issue_hand_backward(self, log=False):
        """B: forward-done / pair-done events, the hand's rigid + MANO backward"""
        m, L, P, ck, on, w = self.model, self.L, _lib.ptr, _lib.check, self.on, self.w
        B, Vh, CL, side, sb = self.B, self.Vh, self.clip_len, self.side, self.side.cuda_stream
        pca, rot, betas, mtr = m.mano_pca_pose, m.mano_rot, m.mano_betas, m.mano_trans if m.optimize_mano else None
        self.ev_fwd.record(side)          # every forward loss value of this stream exists now
        self._aux_block(log)
        self.ev_pair.record(side)        # object-side terms of the pair-wise losses are ready
        # hand (full path: MANO + rigid): smooth + v2d + collision + contact, summed with their weights inside the rigid
        # backward; the interaction term reaches the rigid pose only, as one vector per frame (rec[:, 2:5] / Vh)
        tp, tw, tn = _lib.terms([(self.U_smh if on["smooth"] else None, w["loss_smooth_hand"]),
                                 (self.U_v2d if on["v2d"] else None, w["loss_v2d_hand"]),
                                 (self.U_colh if on["col"] else None, w["loss_collision"]),
                                 (self.U_conh if on["con"] else None, w["loss_contact"]),
                                 (self.G_dep_h if on["depth"] else None, 1.0)])       # (already times its weight)
        g_rig = P(self.G_min_h) if (on["inter"] and self.inter_min) else None
        g_frm = (self.rec.data_ptr() + 8) if (on["inter"] and not self.inter_min) else None
        if m.optimize_mano and self.plan.mano_bwd_rigid:
            # the hand's rigid backward inside the MANO backward's launch: one launch less on this chain
            ck(L.hm_mano_bwd_rigid_clips(self.mctx.ptrs, P(pca), self.P, P(rot), P(betas), B,
                                         P(self.U_pca) if on["pca"] else None, w["loss_pca"], P(pca.grad), P(rot.grad),
                                         P(betas.grad), P(mtr.grad), P(self.mano_state), P(self.mctx.workspace(B)),
                                         P(self.vm), P(m.rotations_hand), P(m.int_scales_hand), tp, tw, tn, g_rig, g_frm, 8,
                                         w["loss_inter"] / Vh, P(m.rotations_hand.grad), P(m.translations_hand.grad), CL,
                                         sb), "mano_bwd + rigid_bwd(hand)")
        else:
            ck(L.hm_rigid_bwd_clips(P(self.vm if m.optimize_mano else m.verts_hand_og), P(m.rotations_hand),
                                    P(m.int_scales_hand), 0, tp, tw, tn, g_rig, g_frm, 8, w["loss_inter"] / Vh, B, Vh,
                                    P(self.G_mesh) if m.optimize_mano else None, P(m.rotations_hand.grad),
                                    P(m.translations_hand.grad), None, P(self.rigid_ws_h), CL, sb), "rigid_bwd(hand)")
            if m.optimize_mano:
                ck(L.hm_mano_bwd(self.mctx.ptrs, P(pca), self.P, P(rot), P(betas), B, P(self.G_mesh),
                                 P(self.U_pca) if on["pca"] else None, w["loss_pca"], P(pca.grad), P(rot.grad),
                                 P(betas.grad), P(mtr.grad), P(self.mano_state), P(self.mctx.workspace(B)), sb),
                   "mano_bwd")

    def _issue_object_backward(self):
        """A, second half: [object depth backward], the object's rigid backward with the silhouette gather"""
        m, L, P, ck, on, w = self.model, self.L, _lib.ptr, _lib.check, self.on, self.w
        B, Vo, CL, sctx, main = self.B, self.Vo, self.clip_len, m.sil_ctx, torch.cuda.current_stream()
        sa, sm_in, sc_obj = main.cuda_stream, self.plan.sm_in, m.optimize_object_scale
        # ---------------- A: object backward: silhouette gradient + smooth + contact [+ interaction with a free scale],
        # summed with their weights inside the rigid backward
        if on["depth"] and on["sil"]:
            main.wait_event(self.ev_dgrad)       # d loss / d (object's depth image), from the side stream
            ctx_o = self.dctx[0]
            ck(L.hm_depth_bwd_sparse(P(self.vo), P(m.camintr), B, Vo, ctx_o.F, ctx_o.S, 1.0, P(self.d_go), P(ctx_o.adj_off),
                                     P(ctx_o.adj_items), P(self.G_dep_o),
                                     P(self.d_flags[0]) if self.d_flags is not None else None, P(ctx_o.workspace), sa),
               "depth bwd(obj)")
        if self.plan.side_terms:      # (else this chain needs nothing from the side stream before the join: see sm_in)
            main.wait_event(self.ev_pair)
        tp, tw, tn = _lib.terms([(self.U_smo if (on["smooth"] and not sm_in) else None, w["loss_smooth_obj"]),
                                 (self.U_cono if on["con"] else None, w["loss_contact"]),
                                 (self.G_int_o if (on["inter"] and sc_obj) else None, 1.0),
                                 (self.G_dep_o if on["depth"] else None, 1.0)])
        if on["sil"]:       # the silhouette term is gathered from the sweeps' per-corner gradients inside this launch
            ck(L.hm_rigid_bwd_sil_clips(P(m.verts_object_og), P(m.rotations_object), P(m.int_scales_object), 1, tp, tw, tn,
                                        sctx.parts_ptr(), P(sctx.adj_off),
                                        P(sctx.adj_items), P(self.vo), P(self.sil_K), 1.0, sctx.F, B, Vo,
                                        P(m.rotations_object.grad), P(m.translations_object.grad),
                                        P(self.g_so_part) if sc_obj else None, P(self.rigid_ws_o), CL, sctx.sum_log2q,
                                        P(self.vo) if sm_in else None, w["loss_smooth_obj"], sa),
               "rigid_bwd(obj) + silhouette gather")
        else:
            ck(L.hm_rigid_bwd_clips(P(m.verts_object_og), P(m.rotations_object), P(m.int_scales_object), 1, tp, tw, tn, None,
                                    None, 0, 0.0, B, Vo, None, P(m.rotations_object.grad), P(m.translations_object.grad),
                                    P(self.g_so_part) if sc_obj else None, P(self.rigid_ws_o), CL, sa), "rigid_bwd(obj)")

    def _issue_join(self, log):
        """tail: join, log row (two streams), scale gradients"""
        m, L, P, ck, C, main = self.model, self.L, _lib.ptr, _lib.check, self.C, torch.cuda.current_stream()
        sa = main.cuda_stream
        main.wait_stream(self.side)          # join
        if self.plan.use_aux:
            main.wait_stream(self.aux)
        elif log:
            ck(L.hm_log_total_clips(P(self.vals), P(self.weights), len(self.SLOTS), P(self.opt.step_t),
                                    self.max_steps, P(self.log_buf), C, sa), "log")
        if m.optimize_object_scale:          # per clip: sum of the frames' d loss / d scale + the scale prior's term
            ck(L.hm_sum_small_clips(P(self.g_so_part), self.clip_len, 1.0, P(self.U_so) if self.on["so"] else None,
                                    self.w["loss_scale_obj"], P(m.int_scales_object.grad), C, sa), "scale grad")
            if self.shared_scale:
                # ONE scalar tied across the clips: its gradient is the sum of the replicas' gradients - local clips
                # here, ranks in _reduce_shared_scale_grad
                ck(L.hm_sum_small_clips(P(m.int_scales_object.grad), C, 1.0, None, 0.0, P(self.g_shared), 1, sa),
                   "shared scale grad")

    def _forward_backward_hands(self, log=False):
        """two hands per frame: homan_amd/fused_hands.py"""
        from .fused_hands import forward_backward_hands
        return forward_backward_hands(self, log)

    def sil_chain_only(self):
        """Measurement helper (tools/bench_sil_kernels.py --chain): just the silhouette chain of an iteration - face setup,
        raster, lines, sweeps - on the current stream, with nothing on any other stream."""
        m, ck = self.model, _lib.check
        sctx, CL, NS = m.sil_ctx, self.clip_len, self.NS
        sa = torch.cuda.current_stream().cuda_stream
        ck(sctx.forward(verts=m.verts_object_og, K=self.sil_K, keep=self.sil_keep, ref=self.sil_ref, pooled=self.pooled,
                        rigid_rot6d=m.rotations_object, rigid_trans=m.translations_object, rigid_scale=m.int_scales_object,
                        rigid_abs=1, persistent_outputs=1, clip_len=CL, cam_verts_out=self.vo, out_stride=NS, stream=sa), "sil_fwd")
        ck(sctx.backward(self.vo, self.sil_K, 2, upstream=self.up_sil, keep_sum=m.keep_sum, clip_len=CL, out_stride=NS, stream=sa),
           "sil_bwd")

    def _depth_render(self, verts, ctx, sil, dep, stream_id):
        """depth + silhouette images of one mesh at the full-image camera (reference homan.py:391,406), all frames.  The
        renders write into buffers this stepper owns and keeps passing: a region that is empty again leaves the empty pattern it
        wrote last time alone (hm_sil_fwd's persistent_outputs, as the silhouette render does) - at the full-image camera nine
        regions in ten are background"""
        _lib.check(ctx.forward(verts=verts, K=self.model.camintr, pooled=sil, pooled_depth=dep, persistent_outputs=1,
                               stream=stream_id), "depth render")

    def _adam_log(self):
        if not self.plan.log_in_adam:
            return None
        return (self.vals, self.weights, len(self.SLOTS), self.max_steps, self.log_buf, self.C)

    def _iteration(self):
        if self.graph is not None:
            self.graph.replay()
            if self.shared_scale:
                self._reduce_shared_scale_grad()
                self.graph_b.replay()
        else:
            self.forward_backward(log=not self.plan.log_in_adam)
            if self.shared_scale:
                self._reduce_shared_scale_grad()
                self._spread_shared_scale_grad()
            self.opt.step(zero_grad=False, log=self._adam_log())

    def run(self, steps):
        if self.graph_k is not None:
            while steps >= self.plan.graph_iters:
                self.graph_k.replay()
                steps -= self.plan.graph_iters
        for _ in range(steps):
            self._iteration()

    def loss_evolution(self, steps, clip=None):
        """{name: [float] * steps} of one clip (reference jointopt.py:184-189); a batch of several clips returns the list
        of its clips' dictionaries unless `clip` picks one."""
        torch.cuda.synchronize()
        host = self.log_buf[:steps].cpu().numpy()           # (steps, C, NS)

        def one(ci):
            out = {k: host[:, ci, self.SLOTS.index(k)].astype(np.float64).tolist() for k in self.keys}
            out["loss"] = host[:, ci, len(self.SLOTS)].astype(np.float64).tolist()
            return out
        if clip is not None:
            return one(clip)
        return one(0) if self.C == 1 else [one(ci) for ci in range(self.C)]
