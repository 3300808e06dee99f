"""CPU side of the volume metrics (csrc/solidvox.hip, homan_amd/pointmetrics.py get_volume_metrics): known answers of the fp32
NumPy restatement tests/volmetrics_ref.py, which the GPU tests hold the kernels to bit for bit, and the argument checks of the
wrappers and of the library that need no device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import volmetrics_ref as ref

H = 0.005
CUBES = (([0.0, 0.0, 0.0], [0.04, 0.04, 0.04], 512),              # face diagonals run through row centres: the tie rule
         ([-0.02, -0.02, -0.02], [0.02, 0.02, 0.02], 512),
         ([0.001, 0.002, -0.013], [0.031, 0.041, 0.018], 6 * 8 * 7))


def own_box(verts, h):
    return ref.box_of(*ref.index_box(verts, h))


def rotated_bottle():
    """the 3000-face bottle, long axis turned towards x, at z ~ 0.6"""
    from homan_amd import synth
    v, f = synth.bottle_mesh()
    a, b = 1.1, 0.4
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    return (v.astype(np.float64) @ (rz @ ry).T + np.array([0.031, -0.052, 0.6])).astype(np.float32), f


@pytest.mark.parametrize("lo,hi,want", CUBES)
def test_cubes_have_their_known_voxel_counts(lo, hi, want):
    v, f = ref.cube_mesh(lo, hi)
    box = own_box(v, H)
    first = ref.occupancy(v, f, H, box)
    assert first.sum() == want
    for faces in (f[:, ::-1], np.roll(f, 1, axis=1), np.roll(f, 2, axis=1), f[::-1]):      # winding, vertex order, face order
        assert np.array_equal(ref.occupancy(v, faces, H, box), first)
    # exactly the voxels whose centre lies strictly inside the cube
    cx, cy, cz = (ref.centres(box[a], box[3 + a], H) for a in range(3))
    inside = [(c > np.float32(l)) & (c < np.float32(u)) for c, l, u in zip((cx, cy, cz), lo, hi)]
    assert np.array_equal(first, inside[2][:, None, None] & inside[1][None, :, None] & inside[0][None, None, :])


def test_a_crop_equals_the_full_box(mano_model):
    v, f = mano_model["v_template"].astype(np.float32), mano_model["closed_faces"]
    box = own_box(v, H)
    full = ref.occupancy(v, f, H, box)
    assert full.sum() > 1000
    sub = box.copy()
    sub[:3] += (3, 2, 1)
    sub[3:] -= (9, 5, 3)
    crop = ref.occupancy(v, f, H, sub)
    assert np.array_equal(crop, full[1:1 + sub[5], 2:2 + sub[4], 3:3 + sub[3]]) and crop.any()
    wider = box.copy()
    wider[:3] -= 40
    wider[3:] += 77
    big = ref.occupancy(v, f, H, wider)
    assert big.sum() == full.sum() and np.array_equal(big[40:40 + box[5], 40:40 + box[4], 40:40 + box[3]], full)


def test_voxel_volume_within_the_surface_bound(mano_model):
    """A voxel can differ from the solid only where its cell meets the surface, i.e. within half a cell diagonal, sqrt(3) h / 2,
    of it on either side: |voxel volume - exact volume| <= area * sqrt(3) * h."""
    from homan_amd import synth
    meshes = {"hand": (mano_model["v_template"].astype(np.float32), mano_model["closed_faces"]), "bottle": rotated_bottle(),
              "box": synth.box_mesh()}
    for name, (v, f) in meshes.items():
        exact, _ = ref.mesh_volume(v, f)
        for h in (0.01, 0.005):
            vox = ref.occupancy(v, f, h, own_box(v, h)).sum() * float(np.float32(h)) ** 3
            print(f"{name} at {h}: voxel volume {vox:.6e}, exact {exact:.6e}, ratio {vox / exact:.4f}")
            assert abs(vox - exact) <= ref.surface_area(v, f) * np.sqrt(3.0) * h, (name, h)
    v, f = ref.cube_mesh([-0.25, 0.0, 0.25], [0.5, 0.5, 1.0])
    assert ref.mesh_volume(v, f)[0] == 0.28125


def test_packing_and_counts():
    rng = np.random.default_rng(0)
    occ = rng.random((3, 4, 70)) < 0.4
    words = ref.pack(occ, (3, 5, 4))
    assert words.shape == (4, 5, 3) and words.dtype == np.uint32 and ref.popcount(words) == occ.sum()
    assert all(((words[k, j, i >> 5] >> (i & 31)) & 1) == occ[k, j, i] for k in range(3) for j in range(4) for i in range(70))
    assert not words[3].any() and not words[:, 4].any() and not (words[:, :, 2] >> 6).any()
    other = ref.pack(rng.random((3, 4, 70)) < 0.4, (3, 5, 4))
    got = ref.overlap_counts(np.stack([words[None], other[None]]), words[None])
    assert got.tolist() == [[ref.popcount(words), ref.popcount(words | other), ref.popcount(words)]]


def test_wrappers_check_their_arguments_before_any_device_work():
    from homan_amd import ho3deval, ops, pointmetrics
    v, f = ref.cube_mesh([0, 0, 0], [0.04, 0.04, 0.04])
    verts = torch.from_numpy(v)[None]
    box = own_box(v, H)[None]
    for bad_verts in (verts[0], verts[:, :, :2], verts[:0], verts.int(), v):
        with pytest.raises(ValueError):
            ops.mesh_volume(bad_verts, f)
        with pytest.raises(ValueError):
            ops.solid_voxels(bad_verts, f, H, box)
    for bad_faces in (f[:, :2], f[:0], f.astype(np.float32), f + 1, f - 1):
        with pytest.raises(ValueError):
            ops.mesh_volume(verts, bad_faces)
        with pytest.raises(ValueError):
            ops.solid_voxels(verts, bad_faces, H, box)
    for bad_pitch in (0.0, -0.005, float("nan"), float("inf"), 1e39, 1e-50):
        with pytest.raises(ValueError):
            ops.solid_voxels(verts, f, bad_pitch, box)
        with pytest.raises(ValueError):
            pointmetrics.get_volume_metrics(verts, verts, f[None], f[None], voxel=bad_pitch)
    too_far = box.copy()
    too_far[0, 0] = (1 << 22) - 5
    for bad_box in (box[0], box[:, :5], box.astype(np.float64), box * [1, 1, 1, -1, 1, 1], too_far,
                    too_far * [-1, 1, 1, 1, 1, 1] - [10, 0, 0, 0, 0, 0]):
        with pytest.raises(ValueError):
            ops.solid_voxels(verts, f, H, bad_box)
    for bad_dims in ((0, 11, 11), (1, 10, 11), (1, 11, 10)):
        with pytest.raises(ValueError):
            ops.solid_voxels(verts, f, H, box, bad_dims)
    words = torch.zeros(2, 3, 3, 1, dtype=torch.int32)
    for a, b in ((words.long(), words), (words, words.float()), (words[:1], words), (words[None, :, :2], words),
                 (words[:0], words[:0]), (words.numpy(), words)):
        with pytest.raises(ValueError):
            ops.voxel_overlap(a, b)
    two = torch.cat([verts, verts])
    for kw in (dict(verts_person=torch.cat([two, verts])), dict(verts_person=verts[:, :, :2]), dict(max_bytes=0),
               dict(verts_object=two[:0])):
        args = dict(verts_person=two, verts_object=two, faces_person=f[None], faces_object=f[None])
        args.update(kw)
        with pytest.raises(ValueError):
            pointmetrics.get_volume_metrics(**args)
    with pytest.raises(ValueError):
        ho3deval.evaluate_sequence_plausibility({}, 4, f, f, chunk=0)
    with pytest.raises(ValueError):
        ho3deval.evaluate_sequence_plausibility({}, 4, f, f, voxel=0.0)
    params = lambda fn: list(inspect.signature(fn).parameters)  # noqa: E731
    assert params(pointmetrics.get_volume_metrics) == ["verts_person", "verts_object", "faces_person", "faces_object", "voxel",
                                                       "max_bytes"]
    assert inspect.signature(pointmetrics.get_volume_metrics).parameters["voxel"].default == 0.005
    assert inspect.signature(pointmetrics.get_volume_metrics).parameters["max_bytes"].default == 256 << 20
    assert params(ho3deval.evaluate_sequence_plausibility) == ["seq_res", "frame_nb", "obj_faces", "mano_faces_closed", "chunk",
                                                               "voxel"]
    assert params(ho3deval.evaluate_sequence) == ["seq_res", "frame_nb", "gt_obj_verts", "gt_hand_roots", "obj_faces",
                                                  "mano_faces_closed", "chunk"]
    assert params(pointmetrics.get_inter_metrics) == ["verts_person", "verts_object", "faces_person", "faces_object"]
    if not torch.cuda.is_available():            # no CPU path
        with pytest.raises(RuntimeError):
            pointmetrics.get_volume_metrics(verts, verts, f[None], f[None])


def test_index_boxes_carry_one_voxel_of_margin():
    from homan_amd import pointmetrics
    lo, hi = np.array([[0.0012, -0.0201, 0.6]], np.float32), np.array([[0.0399, 0.02, 0.64]], np.float32)
    first, last = pointmetrics.index_boxes(lo, hi, np.float32(H))
    assert first.tolist() == [[-1, -6, 119]] and last.tolist() == [[8, 5, 129]]
    v = np.stack([lo[0], hi[0]])
    assert np.array_equal(first[0], ref.index_box(v, H)[0]) and np.array_equal(last[0], ref.index_box(v, H)[1])
    with pytest.raises(ValueError):
        pointmetrics.index_boxes(lo, hi * 1e6, np.float32(H))
    with pytest.raises(ValueError):
        pointmetrics.index_boxes(lo, hi * np.float32("nan"), np.float32(H))


def test_library_refuses_bad_arguments_without_a_launch():
    """made-up device addresses: every call here must fail its host checks before anything is enqueued (HM_ERR_BAD_ARG = -1)"""
    from homan_amd import lib
    h, p = lib.lib(), 1 << 20
    box, wide, negative, low, high = ((ctypes.c_int * 6)(*vals) for vals in (
        (0, 0, 0, 32, 4, 4), (0, 0, 0, 33, 4, 4), (0, 0, 0, -1, 4, 4), (0, 0, -(1 << 22) - 1, 32, 4, 4), (0, (1 << 22) - 3, 0, 32, 4, 4)))
    at = ctypes.addressof

    def voxels(verts=p, faces=p, B=1, V=8, F=12, pitch=0.005, boxes=at(box), nwx=1, ny=4, nz=4, boxes_dev=p, words=p):
        return h.hm_solid_voxels(verts, faces, B, V, F, pitch, boxes, nwx, ny, nz, boxes_dev, words, None)
    for kw in (dict(verts=None), dict(faces=None), dict(boxes=None), dict(boxes_dev=None), dict(words=None), dict(B=0), dict(B=-2),
               dict(V=0), dict(F=0), dict(pitch=0.0), dict(pitch=-1.0), dict(pitch=float("nan")), dict(pitch=float("inf")),
               dict(nwx=-1), dict(ny=-1), dict(nz=-1), dict(nwx=0), dict(ny=3), dict(nz=3),
               dict(boxes=at(wide)), dict(boxes=at(negative)), dict(boxes=at(low)), dict(boxes=at(high))):
        assert voxels(**kw) == -1, kw
    for args in ((None, p, 1, 8, 12, p), (p, None, 1, 8, 12, p), (p, p, 0, 8, 12, p), (p, p, 1, 0, 12, p), (p, p, 1, 8, 0, p),
                 (p, p, 1, 8, 12, None)):
        assert h.hm_mesh_volume(*args, None) == -1, args
    for args in ((None, 1, p, 1, 16, p), (p, 0, p, 1, 16, p), (p, 1, None, 1, 16, p), (p, 1, p, 0, 16, p), (p, 1, p, 1, -1, p),
                 (p, 1, p, 1, 16, None)):
        assert h.hm_voxel_overlap(*args, None) == -1, args
