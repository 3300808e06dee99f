"""The edge scenes of tests/raster_ref.py on the CPU oracle alone: every scene has the property it is there for (exact ties, faces
over many sweep units, a bin beyond CAND_CAP, clipped geometry ...), so that no comparison of tests/test_raster_edges_gpu.py can
pass vacuously; every exact sum stays 2^8 inside its range; and the float32 noise floor of the fused loss is measured here."""
import functools

import numpy as np
import pytest
import torch

from . import raster_ref as rr

f32 = np.float32


@functools.lru_cache(maxsize=None)
def _maps(name):
    sc = rr.scene(name)
    return rr.oracle_maps(rr.project(sc), sc.S, sc.znear, sc.zfar)


@functools.lru_cache(maxsize=None)
def _parts(name, pattern, log2q=0):
    sc = rr.scene(name)
    both, idx, _ = _maps(name)
    ga = rr.sample_gradient_generic(rr.upstream_for(name, pattern).numpy())
    return rr.oracle_parts(both, idx, ga, rr.EPS, log2q)


def _covered(name):
    return int((_maps(name)[1] >= 0).sum())


# ---------------------------------------------------------------- 1. exact ties
def test_lattice_index_maps_equal_the_integer_reference_and_depend_on_the_face_order():
    idents = {}
    for order in rr.LATTICE_ORDERS:
        sc = rr.scene(f"lattice-{order}")
        both, idx, dep = _maps(sc.name)
        # the NDC coordinates are the exact sample positions the integer reference assumes
        n = rr.lattice_nodes()
        want = np.unique((2 * n + 1 - 64) / 64.0)
        assert np.array_equal(np.unique(both[..., 0::3]), want) and np.array_equal(np.unique(both[..., 1::3]), np.unique(-want))
        assert np.array_equal(idx, rr.lattice_integer_index_map(sc.faces.numpy())), order
        assert (idx >= 0).sum() == 57 * 57
        assert np.all(dep[idx >= 0] == 1.0)                                    # every covered sample of every face: the same depth
        idents[order] = rr.triangle_identity(idx[0], sc.faces.numpy())
    moved = int((idents["natural"] != idents["permuted"]).sum())
    print("lattice: samples whose owning triangle depends on the face order:", moved)
    assert moved > 500
    # doubled: both copies of a triangle cover the same samples at the same depth; the owner is the copy listed first
    sc = rr.scene("lattice-doubled")
    f = sc.faces.numpy()
    idx = _maps(sc.name)[1][0]
    F = len(f)
    key = {}
    for i, tri in enumerate(map(tuple, f)):
        key.setdefault(tri, i)
    owners = np.unique(idx[idx >= 0]) % F
    assert all(key[tuple(f[o])] == o for o in owners)
    # vertices on integer pixel coordinates: the backward meets use0 / use1 == false and integer crossings
    px = rr.topix(both[..., 0::3], 64)
    assert np.array_equal(px, np.round(px))


# ---------------------------------------------------------------- 2. large faces
@pytest.mark.parametrize("S", [256, 512])
def test_quad_and_cube_has_faces_over_many_units_and_all_super_regions(S):
    sc = rr.scene(f"quad_and_cube-{S}")
    both, idx, _ = _maps(sc.name)
    items, own = rr.face_items(both, idx, S)
    print(f"quad_and_cube({S}): items per face", items[0].tolist())
    assert (items >= 3 * rr.SWEEP_UNIT).sum() >= 2
    x0, y0, x1, y1, live = rr.sample_boxes(rr.project(sc), S)
    sh = rr.sr_shift(2 * S)
    assert sh == (6 if S == 256 else 7)
    nsr = ((x1 >> sh) - (x0 >> sh) + 1) * ((y1 >> sh) - (y0 >> sh) + 1)
    assert (nsr[live] == 64).any() and (nsr[live] > 4).sum() >= 2            # the `nloc >= 4` bins of the face setup
    assert own[0, :2].all() or own[0, 14:16].all()                            # the quad's triangles own samples around the box


# ---------------------------------------------------------------- 3. crowded region, tiny faces
@pytest.mark.parametrize("fx", [0.3, 0.6])
def test_crowded_fills_one_bin_beyond_cand_cap_and_units_beyond_a_face_pass(fx):
    sc = rr.scene(f"crowded-{fx}")
    both, idx, _ = _maps(sc.name)
    F = sc.faces.shape[0]
    x0, y0, x1, y1, live = rr.sample_boxes(rr.project(sc), sc.S)
    # the face setup bins a face only if its sample box is not empty: of the 3000 faces that is 413 (fx = 0.3: several record
    # passes of RB_PASS candidates) and 1312 (fx = 0.6: three binning rounds of CAND_CAP)
    assert live.sum() > (rr.CAND_CAP if fx == 0.6 else rr.RB_PASS)
    for lo, hi in ((x0, x1), (y0, y1)):
        assert len(np.unique(lo[live] // 32)) == 1 and np.array_equal(lo[live] // 32, hi[live] // 32)       # one 32 x 32 region
    items, own = rr.face_items(both, idx, sc.S)
    owners = int((own[:, :F] | own[:, F:]).sum())
    per_unit = rr.unit_face_counts(items)
    print(f"crowded({fx}): live boxes {int(live.sum())}, owning faces {owners}, faces per unit {per_unit.tolist()}")
    assert 0 < owners < F / 10
    # more faces in a unit than one pass stages (fx = 0.6: up to 60, four passes); fx = 0.3 tops out at exactly one full pass,
    # after which the sweep looks for a second pass and finds none
    assert per_unit.max() > rr.SWEEP_PASS_FACES if fx == 0.6 else per_unit.max() == rr.SWEEP_PASS_FACES


# ---------------------------------------------------------------- 4. / 5. clipped geometry
def test_border_scene_crosses_the_left_and_top_border():
    sc = rr.scene("border")
    both, idx, _ = _maps(sc.name)
    assert _covered("border") > 500
    assert (idx[0, :, 0] >= 0).any()                         # sample column 0
    assert (idx[0, 0] >= 0).any() and (idx[0, 1] >= 0).any()            # the first sample rows (the image's last: the grid is unflipped)
    owners = np.unique(idx[idx >= 0])
    assert (np.abs(both[0, owners].reshape(-1, 3, 3)[..., :2]) > 1).any()


def test_near_scenes_cross_the_near_plane_and_the_camera_plane():
    z = {tz: rr.scene(f"near-{tz}").verts[0, :, 2][rr.scene(f"near-{tz}").faces].numpy() for tz in rr.NEAR_TZ}
    zmin, zmax = z[0.11].min(1), z[0.11].max(1)
    print("near(0.11): faces with a vertex in front of znear", int((zmin < rr.NEAR).sum()), "straddling it", int(((zmin < rr.NEAR) & (zmax > rr.NEAR)).sum()))
    assert (zmin < rr.NEAR).sum() > 1000 and ((zmin < rr.NEAR) & (zmax > rr.NEAR)).sum() > 100 and (zmin > 0).all()
    zmin, zmax = z[0.06].min(1), z[0.06].max(1)
    assert (zmin <= 0).sum() > 200 and ((zmin <= 0) & (zmax > 0)).sum() > 50
    f9 = rr.project(rr.scene("near-0.06"))
    assert np.abs(f9[..., [0, 1, 3, 4, 6, 7]]).max() > 100
    for name in ("near-0.11", "near-0.06", "slab"):
        print(name, "covered samples", _covered(name))
        assert _covered(name) > 500
        assert np.count_nonzero(_parts(name, "dense")) > 100
    # the slab cuts on both sides: samples the default planes cover are empty here, and the survivors lie strictly inside
    sc = rr.scene("slab")
    _, idx_all, dep_all = rr.oracle_maps(rr.project(sc), sc.S)
    _, idx, dep = _maps("slab")
    lost = (idx_all >= 0) & (idx < 0)
    assert (lost & (dep_all <= sc.znear)).sum() > 10 or (idx_all != idx).sum() > 10
    assert np.all((dep[idx >= 0] > f32(sc.znear)) & (dep[idx >= 0] < f32(sc.zfar)))


# ---------------------------------------------------------------- 6. non-finite and overflowing vertices
def test_insane_vertices_remove_their_faces_and_nothing_else():
    sc = rr.scene("insane")
    both, idx, _ = _maps("insane")
    parts = _parts("insane", "dense")
    keep = rr.insane_kept_faces()
    F, Fk = len(keep), int(keep.sum())
    assert 10 < F - Fk < 100
    assert not np.isfinite(both).all()
    clean = rr.centred()
    reduced = clean._replace(name="insane-reduced", faces=clean.faces[torch.from_numpy(keep)])
    both_r, idx_r, _ = rr.oracle_maps(rr.project(reduced), reduced.S)
    ga = rr.sample_gradient_generic(rr.upstream("dense", 1, sc.S).numpy())
    parts_r = rr.oracle_parts(both_r, idx_r, ga)
    orig = np.flatnonzero(keep)
    m = idx_r.copy()
    w = m >= 0
    m[w] = np.where(m[w] < Fk, orig[m[w] % Fk], orig[m[w] % Fk] + F)
    assert np.array_equal(m, idx)
    assert np.array_equal(parts[0][keep], parts_r[0])
    assert np.all(parts[0][~keep] == 0) and np.isfinite(parts).all()
    assert np.count_nonzero(parts) > 100


# ---------------------------------------------------------------- 7. / 8.
@pytest.mark.parametrize("S", rr.NONPOW2_SIZES)
def test_nonpow2_sizes_are_covered_in_both_frames(S):
    assert (2 * S) & (2 * S - 1) and S % 32 == 0 and (2 * S // 64) in (3, 5, 11)
    _, idx, _ = _maps(f"nonpow2-{S}")
    assert all((idx[b] >= 0).sum() > 0.1 * idx[b].size for b in range(2))
    assert all(np.count_nonzero(_parts(f"nonpow2-{S}", "dense")[b]) > 1000 for b in range(2))


def test_mixed_frames_are_what_their_names_say():
    _, idx, _ = _maps("mixed")
    assert (idx[1] < 0).all()
    assert all((idx[b] >= 0).sum() > 500 for b in (0, 2, 3))
    for b, name in ((0, "border"), (2, "near-0.11")):
        assert np.array_equal(idx[b], _maps(name)[1][0])
    assert not _parts("mixed", "dense")[1].any()


# ---------------------------------------------------------------- range of the exact sums
def _cases():
    for name in rr.SCENES:
        for pattern in rr.patterns_of(name):
            yield name, pattern, 0
    yield rr.COARSE_CASE[0], "coarse", rr.COARSE_CASE[1]


def test_exact_sums_stay_far_inside_their_range():
    """include/homan_amd.h: a sum is exact while it stays below 2^53 quanta - and so must every partial sum of its mixed-sign
    addends, which may exceed the final value: every case of the GPU suite keeps max |parts| at or below 2^45 quanta."""
    worst = -np.inf
    for name, pattern, log2q in _cases():
        p = _parts(name, pattern, log2q)
        q = rr.quanta_log2(p, log2q)
        print(f"{name:18s} {pattern:9s} log2q {log2q:4d}: max |parts| = 2^{q:.1f} quanta, non-zero {np.count_nonzero(p)}")
        assert np.isfinite(p).all()
        assert (pattern == "zero") == (not p.any()), (name, pattern)
        worst = max(worst, q)
    for name in rr.FUSED_CASES:
        sc = rr.scene(name)
        both, idx, _ = _maps(name)
        keep, ref = rr.fused_masks(sc)
        from oracle import objchain
        for w in rr.FUSED_WEIGHTS:
            ga, _ = objchain.sample_gradient(idx, keep.numpy(), ref.numpy(), w, f32(keep.sum().item()), sc.verts.shape[0])
            p = rr.oracle_parts(both, idx, ga)
            q = rr.quanta_log2(p, 0)
            print(f"{name:18s} fused {w:+.1f}: max |parts| = 2^{q:.1f} quanta, non-zero {np.count_nonzero(p)}")
            assert np.count_nonzero(p) > 100
            worst = max(worst, q)
    assert worst <= rr.MAX_QUANTA_LOG2, worst


# ---------------------------------------------------------------- the one noise floor
def test_noise_floor_of_the_fused_loss():
    """E32_SIL_LOSS: float32 torch on the CPU against float64, same expression, on the oracle's pooled images of the fused cases."""
    worst = 0.0
    for name in rr.FUSED_CASES:
        sc = rr.scene(name)
        pooled = rr.pool_alpha(_maps(name)[1])
        keep, ref = rr.fused_masks(sc)
        assert 0 < (keep == 0).sum() < keep.numel() and 0 < ref.sum() < ref.numel() and not (ref * (1 - keep)).any()
        want = rr.fused_loss_ref(pooled, keep, ref, torch.float64)
        got = rr.fused_loss_ref(pooled, keep, ref, torch.float32)
        devs = [abs(g - w) / abs(w) for g, w in zip(got, want)]
        print(f"{name}: loss {want[0]:.9e} iou {want[1]:.9e}  float32 deviation loss {devs[0]:.3e} iou {devs[1]:.3e}")
        assert 0 < want[0] < 1 and 0 < want[1] < 1
        worst = max(worst, *devs)
    print(f"worst {worst:.3e} (E32_SIL_LOSS = {rr.E32_SIL_LOSS:.1e})")
    assert 0.5 * rr.E32_SIL_LOSS < worst <= rr.E32_SIL_LOSS, worst
