"""The kernels of csrc/solidvox.hip (hm_solid_voxels, hm_voxel_overlap, hm_mesh_volume), `pointmetrics.get_volume_metrics` and
`ho3deval.evaluate_sequence_plausibility` against the NumPy restatement of tests/volmetrics_ref.py.

Bars.  Occupancy words and overlap counts: equal, bit for bit - both sides perform the same fp32 operations and integers have
no rounding.  Mesh volume: |device - float64 restatement| <= 4 eps F sum_f |det_f| / 6, eps = 2^-52: each determinant is 14
double operations on differences of at most max|e| (under 4 eps |det|-scale each), and a sum of F terms in any order adds at
most (F - 1) eps sum|det|; both sides stay inside half the bar, so their difference is inside it.  The volumes are compared as
absolute m^3 (the bar carries the volume's unit).  Intersection volumes: count * (double)h^3 on both sides, equal.
Measured on the MI355X: every word and count equal; volume differences 0.0 against bars of 3e-17 to 3e-15 m^3."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import volmetrics_ref as ref
from tests.test_volmetrics import CUBES, H, own_box, rotated_bottle

pytestmark = pytest.mark.gpu

PITCHES = (0.01, 0.005, 0.002)
EPS = 2.0 ** -52


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    from homan_amd import synth
    from homan_amd.mano_assets import synthetic_mano
    if name == "hand":
        m = synthetic_mano(0)
        return m["v_template"].astype(np.float32), np.asarray(m["closed_faces"], np.int32)
    if name == "bottle":
        return rotated_bottle()
    if name == "box":
        v, f = synth.box_mesh()
        return (v + np.array([0.0137, -0.0291, 0.0453], np.float32)).astype(np.float32), f
    lo, hi, _ = CUBES[int(name[-1])]
    return ref.cube_mesh(lo, hi)


@functools.lru_cache(maxsize=None)
def restated(name, h):
    """(box, words (1, NZ, NY, NWX)) of the restatement on the mesh's own index box: computed once, shared, left unchanged"""
    v, f = mesh(name)
    box = own_box(v, h)
    words = ref.solid_voxels(v[None], f, h, box[None])
    words.setflags(write=False)
    return box, words


def device_words(verts, faces, h, boxes, dims=None):
    from homan_amd import ops
    words = ops.solid_voxels(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).cuda(), faces, h, np.asarray(boxes), dims)
    assert words.dtype == torch.int32 and words.is_contiguous()
    return words.cpu().numpy().view(np.uint32)


def unpack(words, nx):
    """uint32 (..., NWX) -> bool (..., nx)"""
    b = (words[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return b.reshape(words.shape[:-1] + (-1,))[..., :nx].astype(bool)


# =============================================================================================== occupancy
@pytest.mark.parametrize("h", PITCHES)
@pytest.mark.parametrize("name", ("box", "bottle", "hand", "cube0", "cube1", "cube2"))
def test_occupancy_equals_the_restatement(name, h):
    v, f = mesh(name)
    box, want = restated(name, h)
    assert {"box": 500, "bottle": 3000, "hand": 1552}.get(name, 12) == len(f)
    if name == "bottle" and h == 0.002:
        assert want.shape[3] == 3 and 64 < box[3] <= 96                      # rows of three words
    if name.startswith("cube") and h == H:
        assert ref.popcount(want) == CUBES[int(name[-1])][2]
    got = device_words(v[None], f, h, box[None])
    assert got.shape == want.shape and ref.popcount(want) > 30
    assert np.array_equal(got, want), (name, h, int((got != want).sum()))


@pytest.mark.parametrize("nx", (31, 32, 33, 64, 65))
def test_rows_that_end_at_the_word_seams(nx):
    """a bar whose index box is exactly nx voxels long: nx - 3 of them inside, the last one at bit (nx - 4) of the row"""
    v, f = ref.cube_mesh([0.0012, 0.0013, -0.0061], [(nx - 3 + 0.4) * H, 0.0113, 0.0041])
    box = own_box(v, H)
    assert box[3] == nx
    want = ref.solid_voxels(v[None], f, H, box[None])
    assert ref.popcount(want) == (nx - 3) * 2 * 2
    got = device_words(v[None], f, H, box[None])
    assert got.shape[3] == -(-nx // 32) and np.array_equal(got, want)
    row = unpack(got[0], nx)
    assert row.any((0, 1)).tolist() == [False] + [True] * (nx - 3) + [False, False]
    # the same bar seen through a box that starts 31 voxels earlier: every mark moves across a seam
    moved = box + np.array([-31, 0, 0, 31, 0, 0])
    assert np.array_equal(device_words(v[None], f, H, moved[None]), ref.solid_voxels(v[None], f, H, moved[None]))


def test_negative_and_far_indices():
    v, f = mesh("hand")
    for offset, h in (((-0.51, -0.33, -0.21), H), ((-3000.1, 1700.3, -900.7), 0.001)):
        moved = (v + np.asarray(offset, np.float32)).astype(np.float32)
        box = own_box(moved, h)
        assert (box[:3] < -32).sum() >= 2
        want = ref.solid_voxels(moved[None], f, h, box[None])
        assert np.array_equal(device_words(moved[None], f, h, box[None]), want) and ref.popcount(want) > 1000


def test_a_larger_box_a_crop_and_an_empty_box():
    v, f = mesh("hand")
    box, want = restated("hand", H)
    full = unpack(want[0], box[3])
    wider = box + np.array([-5, -7, -3, 40, 9, 8])
    got = device_words(v[None], f, H, wider[None])
    assert np.array_equal(got, ref.solid_voxels(v[None], f, H, wider[None]))
    assert np.array_equal(unpack(got[0], wider[3])[3:3 + box[5], 7:7 + box[4], 5:5 + box[3]], full)
    assert ref.popcount(got) == ref.popcount(want)
    sub = box + np.array([3, 2, 1, -9, -5, -3])
    crop = device_words(v[None], f, H, sub[None])
    assert np.array_equal(unpack(crop[0], sub[3]), full[1:1 + sub[5], 2:2 + sub[4], 3:3 + sub[3]]) and crop.any()
    # the crop inside launch dimensions larger than it: zero outside its own extents
    padded = device_words(v[None], f, H, sub[None], (2, 22, 12))
    assert np.array_equal(padded, ref.solid_voxels(v[None], f, H, sub[None], (2, 22, 12)))
    for empty in ((0, 0, 0, 0, 5, 5), (0, 0, 0, 5, 0, 5), (-3, 2, 1, 5, 5, 0)):
        assert not device_words(v[None], f, H, np.array([empty]), (1, 5, 5)).any()
    assert device_words(v[None], f, H, np.zeros((1, 6), np.int64)).shape == (1, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def hand_batch(B):
    """B hands of different sizes and places, their own index boxes (frame 3, if there, gets an empty one), and the restatement
    under the launch dimensions that hold them all"""
    v, f = mesh("hand")
    scale = (1.0, 0.6, 1.3, 0.8, 1.1)
    verts = np.stack([(v * np.float32(scale[b]) + np.float32(0.013 * b) * np.array([1, -2, 3], np.float32)).astype(np.float32)
                      for b in range(B)])
    boxes = np.stack([own_box(x, H) for x in verts])
    if B > 3:
        boxes[3, 3:] = 0
    want = ref.solid_voxels(verts, f, H, boxes)
    want.setflags(write=False)
    return verts, f, boxes, want


@pytest.mark.parametrize("B", (1, 3, 5))
def test_batches_with_per_frame_boxes(B):
    verts, f, boxes, want = hand_batch(B)
    dims = (want.shape[3], want.shape[2], want.shape[1])
    if B > 1:
        assert len({tuple(b[3:]) for b in boxes}) == B                            # every frame its own extents
    got = device_words(verts, f, H, boxes)
    assert np.array_equal(got, want)                                              # (zero outside each frame's own extents too)
    assert np.array_equal(device_words(verts, f, H, boxes), got)                  # two calls, the same bits
    for b in range(B):
        if boxes[b, 3] == 0:
            assert not got[b].any()
            continue
        inside = np.zeros(want.shape[1:3] + (32 * want.shape[3],), bool)
        inside[:boxes[b, 5], :boxes[b, 4], :boxes[b, 3]] = True
        assert not (unpack(got[b], 32 * want.shape[3]) & ~inside).any() and got[b].any()
        alone = device_words(verts[b:b + 1], f, H, boxes[b:b + 1], dims)          # a frame alone = the frame in the batch
        assert np.array_equal(alone[0], got[b]), b


def test_more_frames_than_one_launch_dimension():
    """65 537 frames of the 12-triangle cube on a 1-word x 4 x 4 region: the frame axis is split over launches of 65 535"""
    from homan_amd import ops
    B = 65537
    v, f = ref.cube_mesh([0.0, 0.0, 0.0], [0.01, 0.01, 0.01])
    kinds = 7
    offsets = np.stack([np.array([0.0047 * s, 0.0011 * s, 0.0006 * s], np.float32) for s in range(kinds)])
    verts = (v[None] + offsets[np.arange(B) % kinds][:, None]).astype(np.float32)
    box = np.array([-1, -1, -1, 32, 4, 4])
    patterns = ref.solid_voxels(verts[:kinds], f, H, np.tile(box, (kinds, 1)))
    assert patterns.shape == (kinds, 4, 4, 1) and len({p.tobytes() for p in patterns}) > 3
    dv = torch.from_numpy(verts).cuda()
    words = ops.solid_voxels(dv, f, H, np.tile(box, (B, 1)))
    counts = ops.voxel_overlap(words, words).cpu().numpy()
    got = words.cpu().numpy().view(np.uint32)
    for b in (0, B // 2, B - 1, 65534, 65535, 65536):
        assert np.array_equal(got[b], patterns[b % kinds]), b
    assert np.array_equal(got, patterns[np.arange(B) % kinds])
    per_kind = np.array([ref.popcount(p) for p in patterns])
    assert np.array_equal(counts, np.repeat(per_kind[np.arange(B) % kinds][:, None], 3, 1))
    vol = ops.mesh_volume(dv, f).cpu().numpy()
    assert vol.shape == (B,) and np.abs(vol - 1e-6).max() < 1e-12 and vol[0] == vol[kinds] == vol[B - 1 - (B - 1) % kinds]


# =============================================================================================== overlap
def test_overlap_counts_of_cubes():
    from homan_amd import ops
    a = ref.cube_mesh([0.0, 0.0, 0.0], [0.04, 0.04, 0.04])
    others = {"crossing": ([0.02, 0.01, -0.01], [0.06, 0.05, 0.03], 4 * 6 * 6), "touching": ([0.04, 0.0, 0.0], [0.08, 0.04, 0.04], 0),
              "disjoint": ([0.06, 0.05, 0.0], [0.09, 0.08, 0.04], 0), "inside": ([0.01, 0.01, 0.01], [0.03, 0.02, 0.03], 4 * 2 * 4)}
    box = np.array([-2, -3, -4, 40, 22, 18])
    verts_b = np.stack([ref.cube_mesh(lo, hi)[0] for lo, hi, _ in others.values()])
    verts_a = np.stack([a[0]] * len(others))
    boxes = np.tile(box, (len(others), 1))
    wa, wb = ref.solid_voxels(verts_a, a[1], H, boxes), ref.solid_voxels(verts_b, a[1], H, boxes)
    want = ref.overlap_counts(wa, wb)
    assert want[:, 0].tolist() == [n for _, _, n in others.values()] and want[:, 1].tolist() == [512] * 4
    assert want[:, 2].tolist() == [512, 512, 6 * 6 * 8, 4 * 2 * 4]
    da = ops.solid_voxels(torch.from_numpy(verts_a).cuda(), a[1], H, boxes)
    db = ops.solid_voxels(torch.from_numpy(verts_b).cuda(), a[1], H, boxes)
    got = ops.voxel_overlap(da, db)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy().astype(np.uint64), want)
    assert np.array_equal(ops.voxel_overlap(da[1:2], db[1:2]).cpu().numpy(), got[1:2].cpu().numpy())      # alone = in the batch
    # several voxelisations on the a side are OR-ed, not XOR-ed
    both = torch.stack([da, db])
    union = ref.overlap_counts(np.stack([wa, wb]), wa)
    assert np.array_equal(ops.voxel_overlap(both, da).cpu().numpy().astype(np.uint64), union)
    assert union[0].tolist() == [512, 512 + 512 - 144, 512]
    # long rows and a frame size that is no multiple of the workgroup: the bottle against itself, moved by 2 cm
    v, f = mesh("bottle")
    moved = (v + np.float32(0.02)).astype(np.float32)
    first, last = ref.index_box(np.concatenate([v, moved]), 0.002)
    region = ref.box_of(first, last)[None]
    want = ref.overlap_counts(ref.solid_voxels(v[None], f, 0.002, region), ref.solid_voxels(moved[None], f, 0.002, region))
    got = ops.voxel_overlap(ops.solid_voxels(torch.from_numpy(v[None]).cuda(), f, 0.002, region),
                            ops.solid_voxels(torch.from_numpy(moved[None]).cuda(), f, 0.002, region))
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), want) and 0 < want[0, 0] < want[0, 1]
    empty = torch.zeros(3, 0, 0, 0, dtype=torch.int32, device="cuda")
    assert not ops.voxel_overlap(empty, empty).any()


# =============================================================================================== volume
def test_mesh_volume():
    from homan_amd import ops
    v, f = ref.cube_mesh([-0.25, 0.0, 0.25], [0.5, 0.5, 1.0])
    for faces in (f, f[:, ::-1], np.roll(f, 1, axis=1)):
        assert ops.mesh_volume(torch.from_numpy(v[None]).cuda(), faces).cpu().numpy().tolist() == [0.28125]
    for name in ("bottle", "hand", "box"):
        v, f = mesh(name)
        want, sum_abs = ref.mesh_volume(v, f)
        bar = 4 * EPS * len(f) * sum_abs / 6
        batch = np.stack([v, (v * np.float32(1.5)).astype(np.float32), v, (v + np.float32(0.25)).astype(np.float32), v])
        got = ops.mesh_volume(torch.from_numpy(batch).cuda(), f)
        assert got.dtype == torch.float64
        got = got.cpu().numpy()
        print(f"{name}: volume {got[0]:.12e}, restatement {want:.12e}, difference {abs(got[0] - want):.3e}, bar {bar:.3e}")
        assert abs(got[0] - want) <= bar
        for b in (1, 3):
            want_b, sum_b = ref.mesh_volume(batch[b], f)
            assert abs(got[b] - want_b) <= 4 * EPS * len(f) * sum_b / 6
        assert got[0] == got[2] == got[4]                                                          # batch position
        again = ops.mesh_volume(torch.from_numpy(batch).cuda(), f).cpu().numpy()
        assert np.array_equal(bits(again), bits(got))                                              # repeat
        assert bits(ops.mesh_volume(torch.from_numpy(v[None]).cuda(), f).cpu().numpy())[0] == bits(got)[0]


# =============================================================================================== bad arguments
def test_bad_arguments_leave_the_outputs_untouched_and_the_buffers_usable():
    from homan_amd import lib
    h = lib.lib()
    ptr, stream = lib.ptr, lib.stream()
    v, f = mesh("cube0")
    box_np, want = restated("cube0", H)
    verts, faces = torch.from_numpy(v[None]).cuda(), torch.from_numpy(f).cuda()
    nwx, ny, nz = want.shape[3], want.shape[2], want.shape[1]
    words = torch.full((1, nz, ny, nwx), 7, dtype=torch.int32, device="cuda")
    boxes_dev = torch.full((6,), 7, dtype=torch.int32, device="cuda")
    arrays = {name: (ctypes.c_int * 6)(*vals) for name, vals in {
        "good": box_np.tolist(), "wide": box_np.tolist()[:3] + [32 * nwx + 1, ny, nz], "tall": box_np.tolist()[:3] + [11, ny + 1, nz],
        "deep": box_np.tolist()[:3] + [11, ny, nz + 1], "negative": box_np.tolist()[:3] + [11, -1, nz],
        "far": [(1 << 22) - 4, 0, 0, 11, ny, nz], "far_below": [0, 0, -(1 << 22) - 1, 11, ny, nz]}.items()}

    def voxels(vp=verts, fp=faces, B=1, V=8, F=12, pitch=H, box="good", dims=(nwx, ny, nz), bd=boxes_dev, w=words):
        return h.hm_solid_voxels(None if vp is None else ptr(vp), None if fp is None else ptr(fp), B, V, F, pitch,
                                 None if box is None else ctypes.addressof(arrays[box]), *dims, None if bd is None else ptr(bd),
                                 None if w is None else ptr(w), stream)
    for kw in (dict(B=0), dict(B=-1), dict(V=0), dict(F=0), dict(vp=None), dict(fp=None), dict(box=None), dict(bd=None), dict(w=None),
               dict(pitch=0.0), dict(pitch=-H), dict(pitch=float("nan")), dict(pitch=float("inf")), dict(dims=(-1, ny, nz)),
               dict(dims=(nwx, -1, nz)), dict(dims=(nwx, ny, -1)), dict(dims=(0, ny, nz)), dict(dims=(nwx, ny - 1, nz)),
               dict(dims=(nwx, ny, nz - 1)), dict(box="wide"), dict(box="tall"), dict(box="deep"), dict(box="negative"),
               dict(box="far"), dict(box="far_below")):
        assert voxels(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (words == 7).all() and (boxes_dev == 7).all()
    assert voxels() == 0
    torch.cuda.synchronize()
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want)

    counts = torch.full((1, 3), -7, dtype=torch.int64, device="cuda")
    per_frame = words.numel()

    def overlap(a=words, b=words, sets=1, B=1, n=per_frame, c=counts):
        return h.hm_voxel_overlap(None if a is None else ptr(a), sets, None if b is None else ptr(b), B, n,
                                  None if c is None else ptr(c), stream)
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(sets=0), dict(B=0), dict(B=-1), dict(n=-1)):
        assert overlap(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (counts == -7).all()
    assert overlap() == 0
    assert counts.cpu().numpy().tolist() == [[512, 512, 512]]

    vol = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")

    def volume(vp=verts, fp=faces, B=1, V=8, F=12, o=vol):
        return h.hm_mesh_volume(None if vp is None else ptr(vp), None if fp is None else ptr(fp), B, V, F,
                                None if o is None else ptr(o), stream)
    for kw in (dict(vp=None), dict(fp=None), dict(o=None), dict(B=0), dict(B=-3), dict(V=0), dict(F=0)):
        assert volume(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (vol == 7).all()
    assert volume() == 0
    want_vol, sum_abs = ref.mesh_volume(v, f)
    assert abs(vol.cpu().numpy()[0] - want_vol) <= 4 * EPS * 12 * sum_abs / 6 and abs(want_vol - 0.04 ** 3) < 1e-11
    # a face that names a vertex outside the mesh is skipped by the kernels (the wrappers refuse it earlier)
    broken = torch.from_numpy(np.concatenate([f, [[0, 1, 99], [-1, 2, 3]]]).astype(np.int32)).cuda()
    assert voxels(fp=broken, F=14) == 0
    torch.cuda.synchronize()
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want)


# =============================================================================================== the metric
def _pose(v, angle, shift):
    c, s = np.cos(angle), np.sin(angle)
    return (v.astype(np.float64) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).T + np.asarray(shift)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(hands):
    """5 frames: hand(s) at the bottle's side, in frame 3 far from it; (person (5*hands, 778, 3), object (5, Vo, 3), faces)"""
    hv, hf = mesh("hand")
    ov, of = mesh("bottle")
    centre = ov.mean(0)
    person, obj = [], []
    for b in range(5):
        obj.append((ov + np.float32(0.003 * b)).astype(np.float32))
        away = np.array([0.5, 0.0, 0.0]) if b == 3 else np.zeros(3)
        for k in range(hands):
            # the second hand overlaps the first one AND the object (the OR-not-XOR case)
            person.append(_pose(hv - hv.mean(0), 0.3 * b + 0.2 * k, centre + away + [0.012 * k + 0.004 * b, 0.03 - 0.01 * k, 0.002 * b]))
    return np.stack(person), np.stack(obj), hf, of


@functools.lru_cache(maxsize=None)
def scene_restated(hands):
    person, obj, hf, of = scene(hands)
    inter = [ref.inter_volume(list(person[b * hands:(b + 1) * hands]), hf, obj[b], of, H) for b in range(5)]
    hand_vol = [sum(ref.mesh_volume(person[b * hands + k], hf)[0] for k in range(hands)) for b in range(5)]
    return inter, hand_vol, [ref.mesh_volume(o, of)[0] for o in obj]


@pytest.mark.parametrize("hands", (1, 2))
def test_get_volume_metrics_against_the_restatement_loop(hands):
    from homan_amd import pointmetrics
    person, obj, hf, of = scene(hands)
    inter, hand_vol, obj_vol = scene_restated(hands)
    args = (torch.from_numpy(person), torch.from_numpy(obj), np.stack([hf] * hands), of[None])
    got = pointmetrics.get_volume_metrics(*args)
    assert sorted(got) == ["hand_volumes", "inter_volumes", "obj_volumes"] and all(len(v) == 5 for v in got.values())
    print(f"{hands} hand(s): intersection volumes (cm^3) {[round(x * 1e6, 3) for x in got['inter_volumes']]}")
    assert got["inter_volumes"] == inter
    assert inter[3] == 0.0 and min(inter[:3] + inter[4:]) > 50 * H ** 3
    np.testing.assert_allclose(got["hand_volumes"], hand_vol, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["obj_volumes"], obj_vol, rtol=1e-12, atol=0)
    if hands == 2:
        # the union of the two hands, not their parity and not their sum
        box_h = ref.index_box(person[:2], H)
        box_o = ref.index_box(obj[0], H)
        box = ref.box_of(np.maximum(box_h[0], box_o[0]), np.minimum(box_h[1], box_o[1]))
        h0, h1, o = (ref.occupancy(m, fc, H, box) for m, fc in ((person[0], hf), (person[1], hf), (obj[0], of)))
        cell = ref.cell_volume(H)
        assert (h0 & h1 & o).sum() > 10                                                     # the hands overlap inside the object
        assert abs(inter[0] - ((h0 | h1) & o).sum() * cell) < 1e-18 and inter[0] > ((h0 ^ h1) & o).sum() * cell + 9 * cell
        merged = ref.occupancy(np.concatenate([person[0], person[1]]), np.concatenate([hf, hf + 778]), H, box)
        assert ((merged & o).sum() < ((h0 | h1) & o).sum())                                 # what a merged mesh would have lost
    # any chunking, down to one frame per chunk, gives the same lists; a frame alone gives the frame's values
    firsts, lasts = zip(*[(np.maximum(a[0], b[0]), np.minimum(a[1], b[1])) for a, b in (
        (ref.index_box(person[b * hands:(b + 1) * hands], H), ref.index_box(obj[b], H)) for b in range(5))])
    extent = np.stack([ref.box_of(a, b)[3:] for a, b in zip(firsts, lasts)])
    frame_bytes = 4 * int(-(-extent[:, 0].max() // 32)) * int(extent[:, 1].max()) * int(extent[:, 2].max()) * (hands + 1)
    for frames_per_chunk in (5, 3, 2, 1):
        assert pointmetrics.get_volume_metrics(*args, max_bytes=frames_per_chunk * frame_bytes + 3) == got, frames_per_chunk
    with pytest.raises(ValueError):                      # a single frame no longer fits
        pointmetrics.get_volume_metrics(*args, max_bytes=frame_bytes - 1)
    alone = pointmetrics.get_volume_metrics(args[0][2 * hands:3 * hands], args[1][2:3], args[2], args[3])
    assert {k: v[0] for k, v in alone.items()} == {k: v[2] for k, v in got.items()}
    assert pointmetrics.get_volume_metrics(*args, voxel=0.002)["inter_volumes"][3] == 0.0


def test_a_known_overlap_and_the_limits():
    """a 2 x 8 x 3 cm slab as the hand, pushed 1.2 cm into a 6 cm cube: the overlap is the box 1.2 x 6 x 3 cm, whose voxel count
    at 5 mm is known (faces off the lattice planes by a tenth of a voxel: no centre on a face)"""
    from homan_amd import pointmetrics
    eps = 0.0005
    cube_v, f = ref.cube_mesh([eps, eps, eps], [0.06 + eps, 0.06 + eps, 0.06 + eps])
    slab_v, _ = ref.cube_mesh([0.048 + eps, -0.01 + eps, 0.015 + eps], [0.068 + eps, 0.07 + eps, 0.045 + eps])
    got = pointmetrics.get_volume_metrics(torch.from_numpy(slab_v[None]), torch.from_numpy(cube_v[None]), f[None], f[None])
    # centres (i + 0.5) * 5 mm inside (48.5, 60.5) x (0.5, 60.5) x (15.5, 45.5) mm: i = 10, 11; 12 rows; 6 slices
    assert got["inter_volumes"] == [2 * 12 * 6 * ref.cell_volume(H)]
    for key, v in (("hand_volumes", slab_v), ("obj_volumes", cube_v)):       # the product of the fp32 boxes' own edges
        np.testing.assert_allclose(got[key], [(v.max(0).astype(np.float64) - v.min(0)).prod()], rtol=1e-12)
    np.testing.assert_allclose(got["hand_volumes"], [0.02 * 0.08 * 0.03], rtol=1e-5)
    # 2 mm: centres at the odd millimetres, inside (48.5, 60.5) x (0.5, 60.5) x (15.5, 45.5) mm: 6 x 30 x 15
    fine = pointmetrics.get_volume_metrics(torch.from_numpy(slab_v[None]), torch.from_numpy(cube_v[None]), f[None], f[None], voxel=0.002)
    assert fine["inter_volumes"] == [6 * 30 * 15 * ref.cell_volume(0.002)]
    with pytest.raises(ValueError):                      # one frame does not fit
        pointmetrics.get_volume_metrics(torch.from_numpy(slab_v[None]), torch.from_numpy(cube_v[None]), f[None], f[None],
                                        voxel=0.001, max_bytes=1024)
    far = torch.from_numpy(cube_v[None]) + 3.0e4         # index 6e6 > 2^22
    with pytest.raises(ValueError):
        pointmetrics.get_volume_metrics(far, far, f[None], f[None])
    with pytest.raises(ValueError):
        pointmetrics.get_volume_metrics(far * float("nan"), far, f[None], f[None])


# =============================================================================================== sequences
def test_evaluate_sequence_plausibility_frame_by_frame(mano_model):
    from homan_amd import ho3deval, pointmetrics, synth
    from tests.test_ho3deval import _ground_truth, golden, golden_seq_res
    g = golden()
    closed = np.asarray(mano_model["closed_faces"])
    hand = np.asarray(mano_model["v_template"], np.float32) + np.array([0.0, 0.0, 0.5], np.float32)
    box, faces = synth.box_mesh(2, 2, 2, scale=0.08)
    box = np.asarray(box, np.float32) - np.asarray(box, np.float32).mean(0)
    joints = np.zeros((21, 3), np.float32) + hand.mean(0)
    seq = {f: {"hand_verts3d": hand + np.float32(0.001 * f), "hand_joints3d": joints,
               "obj_verts3d": (box + hand.mean(0) + np.float32(0.004 * f)).astype(np.float32), "img_path": "seq/rgb/0000.png"}
           for f in (0, 5)}
    runs = {chunk: ho3deval.evaluate_sequence_plausibility(seq, 6, faces, closed, chunk=chunk) for chunk in (1, 4, 512)}
    res = runs[4]
    assert list(res) == ["inter_volume", "pen_depth", "has_contact", "inter_volume_mean", "pen_depth_mean", "has_contact_mean"]
    for chunk in (1, 512):
        for key in res:
            assert np.array_equal(res[key], runs[chunk][key]), (key, chunk)
    pred_hand = ho3deval.interpolate_sequence(seq, 6, "hand_verts3d", ho3deval.CAMEXTR_SIGNS)
    pred_obj = ho3deval.interpolate_sequence(seq, 6, "obj_verts3d", ho3deval.CAMEXTR_SIGNS)
    for f in range(6):
        vol = pointmetrics.get_volume_metrics(pred_hand[f:f + 1], pred_obj[f:f + 1], closed[None], np.asarray(faces)[None])
        inter = pointmetrics.get_inter_metrics(pred_hand[f:f + 1], pred_obj[f:f + 1], torch.from_numpy(closed)[None],
                                               torch.from_numpy(np.asarray(faces))[None])
        assert res["inter_volume"][f] == vol["inter_volumes"][0] and res["pen_depth"][f] == inter["pen_depths"][0], f
        assert res["has_contact"][f] == float(inter["has_contact"][0]), f
    assert all(res[key].dtype == np.float64 and res[key].shape == (6,) for key in ("inter_volume", "pen_depth", "has_contact"))
    assert res["inter_volume"].min() > 20 * H ** 3 and res["has_contact"].max() == 1.0
    assert res["inter_volume_mean"] == float(res["inter_volume"].mean()) and res["pen_depth_mean"] == float(res["pen_depth"].mean())
    # against the restatement on the interpolated frames
    ph, po = pred_hand.cpu().numpy(), pred_obj.cpu().numpy()
    assert res["inter_volume"].tolist() == [ref.inter_volume([ph[f]], closed, po[f], np.asarray(faces), H) for f in range(6)]
    plain = ho3deval.evaluate_sequence(seq, 6, np.zeros((6, 26, 3)) + np.array([0.0, 0.0, -0.5]), np.zeros((6, 3)), faces, closed, chunk=4)
    assert np.array_equal(plain["pen_depths"], res["pen_depth"]) and np.array_equal(plain["has_contact"], res["has_contact"])
    # evaluate_sequence under the call of tests/test_ho3deval.py: the golden's export arrays bit for bit, the same arrays
    # before and after the new function ran, and its frame-by-frame scores
    gt_obj, gt_roots = _ground_truth()
    args = (golden_seq_res(), 10, gt_obj, gt_roots, g["obj_faces"], closed)
    before = ho3deval.evaluate_sequence(*args, chunk=4)
    ho3deval.evaluate_sequence_plausibility(golden_seq_res(), 10, g["obj_faces"], closed, chunk=4)
    after = ho3deval.evaluate_sequence(*args, chunk=4)
    assert list(before) == ["obj_dist", "obj_add-s", "hand_root", "pen_depths", "has_contact", "export_joints", "export_verts"]
    for key in before:
        assert before[key].dtype == after[key].dtype and np.array_equal(bits(before[key]), bits(after[key])), key
    assert np.array_equal(bits(after["export_joints"]), bits(g["seq_flip_hand_joints3d"]))
    assert np.array_equal(bits(after["export_verts"]), bits(g["seq_flip_hand_verts3d"]))
