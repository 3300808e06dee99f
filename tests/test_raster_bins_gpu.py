"""Face bins of the hard silhouette rasteriser (csrc/raster_setup.hip fills them, csrc/raster_fwd.hip reads them): up to 512^2 samples
one bin per 32 x 32-sample region whose list IS the candidate set of the region's workgroup (entry = face | winding mask << 30, one
reader that empties the count itself), above that the 128 x 128-sample super-regions with box test and ticket.

What can go wrong there and nowhere else: a face left out of a bin its box touches (boxes that end exactly on a region border, a face
over every bin, grids of 1, 2 x 2 and 3 x 3 regions), a count that is not reset or a stale list entry read on the next forward of the
same workspace, an idle workgroup that leaves although its outputs are stale, a bin beyond one scan round, and both bin modes inside
one multi-render launch.  The reference is the exact CPU oracle of tests/raster_ref.py, fed with the kernel's own packed faces; every
comparison is np.array_equal / torch.equal.
"""
import numpy as np
import pytest
import torch

from . import raster_ref as rr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
f32 = np.float32
_EYE = torch.eye(3)


class _Raw:
    """One workspace of the C ABI at ANY raster size the forward takes (S % 16 == 0; ops.SilhouetteContext rounds up to 32), default
    launch order; forward only."""

    def __init__(self, faces, V, B, S):
        from homan_amd import lib as hlib
        self.L, self.P = hlib.lib(), hlib.ptr
        self.faces = torch.as_tensor(faces).to(device=DEV, dtype=torch.int32).contiguous()
        self.B, self.V, self.F, self.S = B, V, int(self.faces.shape[0]), S
        self.workspace = torch.zeros(self.L.hm_sil_workspace_bytes(B, V, self.F, S), dtype=torch.uint8, device=DEV)
        self.work_order = None

    def dims(self):
        return self.B, self.V, self.F, self.S

    def forward(self, verts, K, pooled, depth=None, persistent=0, znear=rr.NEAR, zfar=rr.FAR):
        from homan_amd import lib as hlib
        P = self.P
        hlib.check(self.L.hm_sil_fwd_phase_clips(P(verts), P(self.faces), 0, P(K), self.B, self.V, self.F, self.S, 1.0, znear, zfar, None,
                                                 None, None, P(pooled), None, None, P(depth), None, 0, None, None, None, 0, persistent,
                                                 P(self.workspace), 0, 0, None, 3, hlib.stream()), "hm_sil_fwd_phase_clips")

    def _read(self, fn, out):
        from homan_amd import lib as hlib
        hlib.check(getattr(self.L, fn)(self.P(self.workspace), *self.dims(), self.P(out), hlib.stream()), fn)
        return out.cpu().numpy()

    def idx_map(self):
        return self._read("hm_sil_read_idx_map", torch.empty(self.B, 2 * self.S, 2 * self.S, dtype=torch.int32, device=DEV))

    def faces9(self):
        return self._read("hm_sil_read_faces9", torch.empty(self.B, self.F, 9, device=DEV))

    def owned(self):
        return self._read("hm_sil_read_owned", torch.empty(self.B, 2 * self.F, dtype=torch.uint8, device=DEV))

    def boxes(self):
        """-> x0, y0, x1, y1, winding mask per (B,F)"""
        raw = self._read("hm_sil_read_boxes", torch.empty(self.B * self.F * 8, dtype=torch.uint8, device=DEV))
        bx = raw.view(np.uint16).reshape(self.B, self.F, 4).astype(np.int64)
        return bx[..., 0] & 0x3fff, bx[..., 1], bx[..., 2], bx[..., 3], bx[..., 0] >> 14


def _owned_ref(idx, F):
    """(B,2F) bytes: winding fn owns a sample of the oracle's index map"""
    own = np.zeros((idx.shape[0], 2 * F), np.uint8)
    for b in range(idx.shape[0]):
        u = np.unique(idx[b])
        own[b, u[u >= 0]] = 1
    return own


# ---------------------------------------------------------------- 1. smallest and odd grids, boxes on region borders
def _at(px, py, is_, z):
    """camera-space vertex (K = identity) that projects onto sample column px, sample row py (y up, as the face boxes count)"""
    return [z * (px + 0.5) / is_, z * (1.0 - (py + 0.5) / is_), z]


def border_scene(S, cover):
    """Triangles whose sample boxes end exactly on a region border, on either side of it and on both axes: around every inner
    border corner (k, k), k = 32, 64, .., boxes with x1 = k - 1 / x0 = k combined with y1 = k - 1 / y0 = k; at S = 16 (one region)
    the box with x1 = y1 = 31 on the raster's border.  `cover`: behind them one triangle that covers every region."""
    is_ = 2 * S
    v, f = [], []

    def tri(corners, z):
        n = len(v)
        v.extend(_at(x, y, is_, z) for x, y in corners)
        f.append([n, n + 1, n + 2])

    z = 1.0
    for k in range(32, is_ + 1, 32):
        lo, hi = k - 12, k + 12                                     # (the far side of each box stays off the next border)
        tri([(lo, lo + 2), (k - 1, lo), (lo + 4, k - 1)], z)        # x1 = k - 1, y1 = k - 1
        if k < is_:
            tri([(k, k), (hi, k + 2), (k + 4, hi)], z + 0.01)       # x0 = k, y0 = k
            tri([(lo, k), (k - 1, k + 3), (lo + 3, hi)], z + 0.02)  # x1 = k - 1, y0 = k
            tri([(k, lo), (hi, lo + 3), (k + 3, k - 1)], z + 0.03)  # x0 = k, y1 = k - 1
        z += 0.05
    if cover:
        tri([(-is_, -is_), (3 * is_, -is_), (-is_, 3 * is_)], 4.0)
    return rr._scene(f"bins-border-{S}-{int(cover)}", torch.tensor(v, dtype=torch.float32)[None], np.array(f, np.int64), _EYE, S)


@pytest.mark.parametrize("cover", [False, True])
@pytest.mark.parametrize("S", [16, 32, 48])
def test_smallest_and_odd_grids_with_boxes_on_region_borders(S, cover):
    """1 region, 2 x 2 and 3 x 3 (no power of two) regions: index map, pooled coverage and `owned` equal the oracle; the boxes are
    where the scene wants them (ending on x = 31 / starting on x = 32, and so on in y)."""
    sc = border_scene(S, cover)
    is_, F = 2 * S, sc.faces.shape[0]
    ws = _Raw(sc.faces, sc.verts.shape[1], 1, S)
    pooled = torch.full((1, S, S), -7.0, device=DEV)
    ws.forward(sc.verts.to(DEV), sc.K.to(DEV), pooled)
    x0, y0, x1, y1, m = ws.boxes()
    assert (m != 0).all()
    small = slice(0, F - 1 if cover else F)
    ends, starts = set(range(31, is_, 32)), set(range(32, is_, 32))
    assert ends <= set(x1[0, small]) and ends <= set(y1[0, small])
    assert starts <= set(x0[0, small]) and starts <= set(y0[0, small])
    if cover:
        assert (x0[0, -1], y0[0, -1], x1[0, -1], y1[0, -1]) == (0, 0, is_ - 1, is_ - 1)
    _, idx, _ = rr.oracle_maps(ws.faces9(), S)
    got = ws.idx_map()
    assert np.array_equal(got, idx)
    assert np.array_equal(pooled.cpu().numpy(), rr.pool_alpha(idx))
    own = _owned_ref(idx, F)
    assert np.array_equal(ws.owned(), own)
    assert own.reshape(2, F).any(0).all()                           # every triangle shows, through one of its windings
    assert ((idx >= 0).all()) == cover


# ---------------------------------------------------------------- 2. stale bins, 3. all faces off screen
def _cube(at, scale=0.15):
    from homan_amd import synth
    cv, cf = synth.box_mesh(1, 1, 1, scale=scale)
    R = torch.tensor(synth._rot_x(0.5) @ synth._rot_y(0.7), dtype=torch.float32)
    return (torch.from_numpy(cv).float() @ R + torch.tensor(at))[None].contiguous(), np.asarray(cf, np.int64)


class _Fused:
    """ops.SilhouetteContext + its fused-loss forward (keep / ref) and the backward of mode 1"""

    def __init__(self, faces, V, S):
        from homan_amd import ops
        self.sctx = ops.SilhouetteContext(torch.as_tensor(faces)[None].to(DEV), V, 1, S, DEV)
        self.V, self.S = V, S
        self.keep = torch.ones(1, S, S, device=DEV)
        self.ref = torch.zeros(1, S, S, device=DEV)
        self.ref[:, S // 4:3 * S // 4, S // 4:3 * S // 4] = 1.0
        self.keep_sum = self.keep.sum().reshape(1)
        self.pooled = torch.full((1, S, S), 7.0, device=DEV)
        self.out = torch.zeros(2, device=DEV)

    def step(self, verts, persistent, backward=True):
        from homan_amd import lib as hlib
        v, K = verts.to(DEV).contiguous(), _EYE[None].to(DEV).contiguous()
        hlib.check(self.sctx.forward(verts=v, K=K, keep=self.keep, ref=self.ref, keep_sum=self.keep_sum, pooled=self.pooled,
                                     loss_out=self.out, persistent_outputs=persistent), "forward")
        res = dict(pooled=self.pooled.clone(), out=self.out.clone(), idx=self.sctx.idx_map())
        if backward:
            gv = torch.full((1, self.V, 3), -7.0, device=DEV)
            hlib.check(self.sctx.backward(v, K, 1, upstream=torch.ones(1, device=DEV), keep_sum=self.keep_sum, grad_verts=gv),
                       "backward")
            res.update(parts=self.sctx.parts(), grad_verts=gv)
        return res


def _regions(idx):
    """set of the 32 x 32-sample regions (sample row // 32, sample column // 32) with a covered sample"""
    y, x = np.nonzero(idx[0] >= 0)
    return set(zip((y // 32).tolist(), (x // 32).tolist()))


@pytest.mark.parametrize("persistent", [0, 1])
def test_second_forward_on_one_workspace_sees_no_stale_bin(persistent):
    """Forward (+ backward) at pose A, then at pose B on the SAME workspace, the mesh moved so that the regions A filled are empty
    at B and the reverse; then back to A.  Every result equals a fresh workspace's: a count that was not reset, or an entry read
    from a stale list, would show."""
    S = 64
    va, faces = _cube([0.25, 0.25, 1.0])
    vb, _ = _cube([0.75, 0.75, 1.0])
    one = _Fused(faces, va.shape[1], S)
    seen = []
    for step, v in enumerate((va, vb, va, vb)):
        got = one.step(v, persistent)
        fresh = _Fused(faces, va.shape[1], S).step(v, 0)
        for k in fresh:
            assert torch.equal(got[k], fresh[k]), (step, k)
        assert fresh["parts"].any()
        seen.append(_regions(fresh["idx"].cpu().numpy()))
    assert seen[0] and seen[1] and not (seen[0] & seen[1]), seen[:2]


def test_all_faces_off_screen_twice_with_persistent_outputs():
    """No face in any bin: the first call writes the empty pattern, the second (idle workgroups: empty bin in front of outputs
    that hold the empty pattern) touches nothing and the outputs are still right."""
    S = 64
    v, faces = _cube([5.0, 0.3, 1.0])
    run = _Fused(faces, v.shape[1], S)
    first = run.step(v, 1, backward=False)
    assert not first["pooled"].any() and (first["idx"] == -1).all()
    # (exact: sum(ref^2) = S^2 / 4 over sum(keep) = S^2, one frame)
    assert float(first["out"][0]) == 0.25 and float(first["out"][1]) == 0.0
    run.pooled[0, 5, 9] = 3.0                                       # a mark in the caller's buffer: an untouched region keeps it
    second = run.step(v, 1)
    assert float(second["pooled"][0, 5, 9]) == 3.0
    second["pooled"][0, 5, 9] = 0.0
    assert not second["pooled"].any() and (second["idx"] == -1).all()
    assert torch.equal(second["out"], first["out"])
    assert not second["parts"].any() and not second["grad_verts"].any()


# ---------------------------------------------------------------- 4. a bin beyond CAND_CAP, faces in all 256 bins
@pytest.mark.parametrize("name", ["crowded-0.6", "quad_and_cube-256"])
def test_fill_pass_without_the_four_bin_cap(name):
    """crowded-0.6: one region's bin beyond CAND_CAP (several scan rounds over one list); quad_and_cube-256: two faces in all 256
    bins of a 512^2-sample render (every LDS counter of the fill pass).  Forward and `parts` against the oracle."""
    from homan_amd import lib as hlib
    from homan_amd import ops
    sc = rr.scene(name)
    B, V = sc.verts.shape[:2]
    sctx = ops.SilhouetteContext(sc.faces[None].expand(B, -1, -1).to(DEV), V, B, sc.S, DEV)
    verts, K = sc.verts.to(DEV).contiguous(), sc.K.to(DEV).contiguous()
    pooled = torch.full((B, sc.S, sc.S), -7.0, device=DEV)
    hlib.check(sctx.forward(verts=verts, K=K, pooled=pooled, znear=sc.znear, zfar=sc.zfar), "forward")
    faces9 = sctx.faces9().cpu().numpy()
    both, idx, _ = rr.oracle_maps(faces9, sc.S, sc.znear, sc.zfar)
    x0, y0, x1, y1, live = rr.sample_boxes(faces9, sc.S)
    per_bin = np.zeros((2 * sc.S // 32, 2 * sc.S // 32), np.int64)
    for a0, b0, a1, b1 in zip(x0[0][live[0]], y0[0][live[0]], x1[0][live[0]], y1[0][live[0]]):
        per_bin[b0 // 32:b1 // 32 + 1, a0 // 32:a1 // 32 + 1] += 1
    if name.startswith("crowded"):
        assert per_bin.max() > rr.CAND_CAP
    else:
        assert per_bin.size == 256 and (per_bin >= 2).all()
    assert np.array_equal(sctx.idx_map().cpu().numpy(), idx)
    assert np.array_equal(pooled.cpu().numpy(), rr.pool_alpha(idx))
    gimg = rr.upstream_for(name, "dense")
    gv = torch.full((B, V, 3), -7.0, device=DEV)
    hlib.check(sctx.backward(verts, K, 0, grad_pooled=gimg.to(DEV).contiguous(), grad_verts=gv), "backward")
    parts = rr.oracle_parts(both, idx, rr.sample_gradient_generic(gimg.numpy()))
    assert np.count_nonzero(parts) > 40
    assert np.array_equal(sctx.parts().cpu().numpy(), parts)


# ---------------------------------------------------------------- 5. both bin modes in one launch
def test_region_bins_and_super_regions_share_one_multi_launch():
    """hm_sil_fwd_multi with a 256^2 render (512^2 samples: region bins) and a 272^2 render (544^2 samples: super-regions) equals
    the two separate calls: pooled coverage, pooled depth, index map, `owned`."""
    from homan_amd import lib as hlib
    va, faces = _cube([0.4, 0.55, 1.0], scale=0.5)
    K = _EYE[None].to(DEV).contiguous()
    v = va.to(DEV)
    single, multi, rend = [], [], []
    for S in (256, 272):
        for store in (single, multi):
            store.append((_Raw(faces, v.shape[1], 1, S), torch.full((1, S, S), -3.0, device=DEV), torch.full((1, S, S), -3.0, device=DEV)))
        ws, p, d = single[-1]
        ws.forward(v, K, p, depth=d)
        ws, p, d = multi[-1]
        rend.append(dict(verts=v, faces=ws.faces, K=K, pooled=p, pooled_depth=d, workspace=ws.workspace, B=1, V=ws.V, F=ws.F, S=S,
                         orig_size=1.0, znear=rr.NEAR, zfar=rr.FAR, clip_len=1))
    hlib.check(hlib.lib().hm_sil_fwd_multi(hlib.sil_renders(rend), 2, 3, hlib.stream()), "hm_sil_fwd_multi")
    torch.cuda.synchronize()
    for (wa, pa, da), (wb, pb, db) in zip(single, multi):
        assert torch.equal(pa, pb) and torch.equal(da, db), wa.S
        assert np.array_equal(wa.idx_map(), wb.idx_map()) and np.array_equal(wa.owned(), wb.owned()), wa.S
        assert float(pa.sum()) > 100.0 and wa.owned().any()
    _, idx, _ = rr.oracle_maps(single[0][0].faces9(), 256)
    assert np.array_equal(single[0][0].idx_map(), idx)


# ---------------------------------------------------------------- 6. depth output
def test_pooled_depth_equals_the_pooled_oracle_depth():
    """the z-buffer a region workgroup builds from its own bin, as the depth output: pool_depth of the oracle's depth map, exactly
    (3 x 3 regions, triangles on the region borders in front of one that covers every region)"""
    sc = border_scene(48, True)
    ws = _Raw(sc.faces, sc.verts.shape[1], 1, sc.S)
    pooled = torch.full((1, sc.S, sc.S), -7.0, device=DEV)
    depth = torch.full((1, sc.S, sc.S), -7.0, device=DEV)
    ws.forward(sc.verts.to(DEV), sc.K.to(DEV), pooled, depth=depth)
    _, idx, dep = rr.oracle_maps(ws.faces9(), sc.S)
    assert np.array_equal(ws.idx_map(), idx)
    want = rr.pool_depth(dep)
    assert len(np.unique(want)) > 30 and float(want.max()) < rr.FAR
    assert np.array_equal(depth.cpu().numpy(), want)
