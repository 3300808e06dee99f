"""Hard silhouette rasteriser (csrc/raster_setup.hip, raster_fwd.hip, raster_lines.hip, raster_sweep.hip) on the edge scenes of
tests/raster_ref.py: exact ties, raster sizes that are no power of two, faces over many super-regions and sweep units, a bin
beyond CAND_CAP, units beyond one face pass, geometry over the border, through the near plane, behind the camera, non-finite.

The reference is the exact CPU oracle (oracle/csrc/nmr_raster.c, oracle/csrc/objchain.c), fed with the kernel's own packed faces
as tests/test_raster_gpu.py does; tests/test_raster_refs.py shows on the oracle alone that every scene has its property.  Nothing
here has a tolerance but the fused loss value and IoU (util.E32_FACTOR times the float32 floor raster_ref.E32_SIL_LOSS): index map,
pooled coverage, pooled depth, the per-(face, corner) sums `parts`, the per-vertex NDC gradient and the vertex gradient are
np.array_equal / torch.equal to the oracle, a frame equals itself run alone, and no scheduling knob changes a bit.
"""
import numpy as np
import pytest
import torch

from . import raster_ref as rr
from . import util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
f32 = np.float32

_ORACLE = {}            # scene name -> (faces9 of the kernel, both, idx, dep): computed once, shared, never modified
_PARTS = {}             # (scene name, pattern, log2q) -> parts of the oracle


def _oracle(sc, faces9):
    hit = _ORACLE.get(sc.name)
    if hit is None or not np.array_equal(hit[0], faces9, equal_nan=True):
        hit = (faces9,) + rr.oracle_maps(faces9, sc.S, sc.znear, sc.zfar)
        _ORACLE[sc.name] = hit
    return hit[1:]


def _oracle_parts(sc, faces9, pattern, gimg, log2q=0):
    both, idx, _ = _oracle(sc, faces9)
    key = (sc.name, pattern, log2q)
    if key not in _PARTS:
        _PARTS[key] = rr.oracle_parts(both, idx, rr.sample_gradient_generic(gimg.numpy()), rr.EPS, log2q)
    return _PARTS[key]


class _Run:
    """one forward (+ one generic backward, mode 0) of a scene through ops.SilhouetteContext; everything read back to the host"""

    def __init__(self, sc, gimg=None, log2q=0, sctx=None):
        from homan_amd import lib as hlib
        from homan_amd import ops
        B, V = sc.verts.shape[:2]
        self.sc, self.B, self.V = sc, B, V
        self.sctx = sctx or ops.SilhouetteContext(sc.faces[None].expand(B, -1, -1).to(DEV), V, B, sc.S, DEV)
        self.verts, self.K = sc.verts.to(DEV).contiguous(), sc.K.to(DEV).contiguous()
        pooled = torch.full((B, sc.S, sc.S), -7.0, device=DEV)
        depth = torch.full((B, sc.S, sc.S), -7.0, device=DEV)
        hlib.check(self.sctx.forward(verts=self.verts, K=self.K, pooled=pooled, pooled_depth=depth, znear=sc.znear, zfar=sc.zfar),
                   "forward")
        self.pooled, self.depth = pooled.cpu().numpy(), depth.cpu().numpy()
        self.faces9 = self.sctx.faces9().cpu().numpy()
        self.idx = self.sctx.idx_map().cpu().numpy()
        if gimg is not None:
            self.backward(gimg, log2q)

    def backward(self, gimg, log2q=0):
        from homan_amd import lib as hlib
        gv = torch.full((self.B, self.V, 3), -7.0, device=DEV)
        gn = torch.full((self.B, self.V, 3), -7.0, device=DEV)
        self.sctx.sum_log2q = log2q
        hlib.check(self.sctx.backward(self.verts, self.K, 0, grad_pooled=gimg.to(DEV).contiguous(), grad_verts=gv, grad_ndc=gn),
                   "backward")
        torch.cuda.synchronize()
        self.parts = self.sctx.parts().cpu().numpy()
        self.grad_verts, self.grad_ndc = gv.cpu().numpy(), gn.cpu().numpy()
        return self


def _assert_forward(run, depth=False):
    sc = run.sc
    both, idx, dep = _oracle(sc, run.faces9)
    assert np.array_equal(run.idx, idx), sc.name
    assert np.array_equal(run.pooled, rr.pool_alpha(idx)), sc.name
    if depth:
        assert np.array_equal(run.depth, rr.pool_depth(dep)), sc.name
    return both, idx


def _assert_backward(run, parts):
    sc = run.sc
    assert np.array_equal(run.parts, parts), sc.name
    ndc, gverts = rr.gather_ref(parts, sc.faces.numpy(), sc.verts.numpy(), sc.K.numpy())
    assert np.array_equal(run.grad_ndc[..., :2], ndc[..., :2]) and not run.grad_ndc[..., 2].any(), sc.name
    fin = np.isfinite(gverts).all(-1)
    assert fin.sum() > 0.9 * fin.size
    assert np.array_equal(run.grad_verts[fin], gverts[fin]), sc.name


# ---------------------------------------------------------------- A. projection
@pytest.mark.parametrize("name", ["border", "near-0.11", "near-0.06", "insane"])
def test_packed_faces_equal_the_oracle_projection(name):
    """same operations in the same order (oracle/nmr.py projection, csrc/raster_setup.hip project_vertex), also for vertices behind
    the camera, at z + 1e-9 == 0, non-finite or beyond the float range of the image plane"""
    sc = rr.scene(name)
    run = _Run(sc)
    want = rr.project(sc)
    if name == "insane":
        assert not np.isfinite(want).all()
    if name == "near-0.06":
        assert np.abs(want[..., [0, 1, 3, 4, 6, 7]]).max() > 100
    assert np.array_equal(run.faces9, want, equal_nan=(name == "insane"))


# ---------------------------------------------------------------- B. coverage, C. pseudo-gradient
_DEPTH_SCENES = ("slab", "near-0.11", "near-0.06") + tuple(f"nonpow2-{s}" for s in rr.NONPOW2_SIZES)
_CASES = [(n, p, 0) for n in rr.SCENES for p in rr.patterns_of(n)] + [(rr.COARSE_CASE[0], "coarse", rr.COARSE_CASE[1])]


@pytest.mark.parametrize("name,pattern,log2q", _CASES, ids=[f"{n}-{p}" for n, p, _ in _CASES])
def test_scene_equals_the_oracle_exactly(name, pattern, log2q):
    """index map, pooled coverage (and depth), `parts`, the per-vertex NDC gradient and the vertex gradient of one (scene, upstream
    pattern): all equal to the oracle's, bit for bit"""
    sc = rr.scene(name)
    gimg = rr.upstream_for(name, pattern)
    run = _Run(sc, gimg, log2q)
    both, idx = _assert_forward(run, depth=name in _DEPTH_SCENES)
    assert (idx >= 0).sum() > 50
    if name.startswith("lattice"):
        assert np.array_equal(run.idx, rr.lattice_integer_index_map(sc.faces.numpy()))
    parts = _oracle_parts(sc, run.faces9, pattern, gimg, log2q)
    assert rr.quanta_log2(parts, log2q) <= rr.MAX_QUANTA_LOG2
    _assert_backward(run, parts)
    if pattern == "zero":
        assert not run.parts.any() and not run.grad_ndc.any() and not run.grad_verts.any()
    else:
        assert np.count_nonzero(run.parts) > 40
    if name == "insane":
        assert np.isfinite(run.parts).all() and not run.parts[0][~rr.insane_kept_faces()].any()
    if name == "mixed":                                   # the off-screen frame: all background, exact zeros
        b = rr.MIXED_FRAMES.index("offscreen")
        assert (run.idx[b] == -1).all() and not run.pooled[b].any()
        assert not run.parts[b].any() and not run.grad_ndc[b].any() and not run.grad_verts[b].any()


# ---------------------------------------------------------------- D. frames do not see each other
def test_every_frame_of_a_batch_equals_the_frame_run_alone():
    sc = rr.scene("mixed")
    gimg = rr.upstream_for("mixed", "dense")
    batch = _Run(sc, gimg)
    for b in range(sc.verts.shape[0]):
        one = _Run(rr.frame_of(sc, b), gimg[b:b + 1])
        assert np.array_equal(one.idx[0], batch.idx[b]), b
        assert np.array_equal(one.pooled[0], batch.pooled[b]), b
        assert np.array_equal(one.depth[0], batch.depth[b]), b
        assert np.array_equal(one.parts[0], batch.parts[b]), b
        assert np.array_equal(one.grad_verts[0], batch.grad_verts[b], equal_nan=True), b


# ---------------------------------------------------------------- E. scheduling does not show
@pytest.mark.parametrize("name", ["quad_and_cube-256", "crowded-0.3", "border"])
def test_scheduling_knobs_change_no_bit(name):
    """Workgroup count of the persistent sweep, capacity tables shrunk to a handful of entries (units beyond the unit table find
    their first face by binary search), a calibrated launch order, either winding rasterised first: index map and `parts` stay
    what the oracle says."""
    from homan_amd import lib as hlib
    L = hlib.lib()
    sc = rr.scene(name)
    gimg = rr.upstream_for(name, "dense")
    base = _Run(sc, gimg)
    _assert_forward(base)
    assert np.array_equal(base.parts, _oracle_parts(sc, base.faces9, "dense", gimg)) and base.parts.any()

    def same(run, what):
        assert np.array_equal(run.idx, base.idx), (name, what)
        assert np.array_equal(run.pooled, base.pooled), (name, what)
        assert np.array_equal(run.parts, base.parts), (name, what)
        assert np.array_equal(run.grad_verts, base.grad_verts, equal_nan=True), (name, what)

    for blocks in (8, 768):
        prev = L.hm_tune_sweep_blocks(blocks)
        try:
            same(_Run(sc, gimg), f"blocks {blocks}")
        finally:
            L.hm_tune_sweep_blocks(prev)
    for cap in (1, 3):
        prev = L.hm_debug_sweep_caps(cap)
        try:
            same(_Run(sc, gimg), f"cap {cap}")
        finally:
            L.hm_debug_sweep_caps(prev)
    run = _Run(sc, gimg)
    run.sctx.calibrate()
    same(_Run(sc, gimg, sctx=run.sctx), "calibrated")
    for winding in (0, 1):
        hlib.check(L.hm_sil_hint_near_winding(hlib.ptr(run.sctx.workspace), winding, hlib.stream()), "hm_sil_hint_near_winding")
        same(_Run(sc, gimg, sctx=run.sctx), f"near winding {winding}")


# ---------------------------------------------------------------- F. fused loss
@pytest.mark.parametrize("weight", rr.FUSED_WEIGHTS)
@pytest.mark.parametrize("name", rr.FUSED_CASES)
def test_fused_loss_equals_the_oracle_chain(name, weight):
    """ops.silhouette_loss with a keep mask that has ignore bands and a reference from a shifted render: `parts` equal the oracle's
    on objchain.sample_gradient (a negative weight rebuilds the sweep planes in k_bwd_masks), the image equals the oracle's, the
    vertex gradient the restated gather; loss and IoU within E32_FACTOR x E32_SIL_LOSS of their float64 values:
    measured deviations are printed."""
    from homan_amd import ops
    from oracle import objchain
    sc = rr.scene(name)
    B, V = sc.verts.shape[:2]
    keep, ref = rr.fused_masks(sc)
    keep_sum = keep.sum().reshape(1)
    sctx = ops.SilhouetteContext(sc.faces[None].expand(B, -1, -1).to(DEV), V, B, sc.S, DEV)
    vh = sc.verts.to(DEV).requires_grad_(True)
    loss_h, iou_h, img_h = ops.silhouette_loss(vh, sc.K.to(DEV), keep.to(DEV), ref.to(DEV), keep_sum.to(DEV), sctx)
    (loss_h * weight).sum().backward()
    torch.cuda.synchronize()
    faces9 = sctx.faces9().cpu().numpy()
    both, idx, _ = _oracle(sc, faces9)
    assert np.array_equal(sctx.idx_map().cpu().numpy(), idx)
    ga, pool = objchain.sample_gradient(idx, keep.numpy(), ref.numpy(), weight, f32(keep_sum.item()), B)
    assert np.array_equal(img_h.cpu().numpy(), pool)
    parts = rr.oracle_parts(both, idx, ga)
    assert np.count_nonzero(parts) > 100 and rr.quanta_log2(parts, 0) <= rr.MAX_QUANTA_LOG2
    assert np.array_equal(sctx.parts().cpu().numpy(), parts)
    _, gverts = rr.gather_ref(parts, sc.faces.numpy(), sc.verts.numpy(), sc.K.numpy())
    assert np.array_equal(vh.grad.cpu().numpy(), gverts)
    want = rr.fused_loss_ref(pool, keep, ref, torch.float64)
    devs = [abs(float(g) - w) / abs(w) for g, w in zip((loss_h.item(), iou_h.item()), want)]
    bar = util.E32_FACTOR * rr.E32_SIL_LOSS
    print(f"fused {name} {weight:+.1f}: loss {loss_h.item():.9e} (ref {want[0]:.9e}, deviation {devs[0]:.3e}) "
          f"iou {iou_h.item():.9e} (ref {want[1]:.9e}, deviation {devs[1]:.3e}) bar {bar:.1e}")
    assert devs[0] <= bar and devs[1] <= bar, devs


# ---------------------------------------------------------------- G. 64-bit offsets
def test_64_bit_offset_instantiations_pass_the_edge_scenes():
    """HOMAN_FORCE_W64=1 (read when the library first launches the line expansion and the sweeps, hence a fresh process) takes their
    64-bit-index instantiations: the exact comparisons above must hold through them too."""
    import os
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    env = dict(os.environ, HOMAN_FORCE_W64="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_raster_edges_gpu.py"), "-x", "-q", "-m", "gpu",
                        "-k", "lattice or quad or crowded or nonpow2"], env=env, capture_output=True, text=True, cwd=root,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
