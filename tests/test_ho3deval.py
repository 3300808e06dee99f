"""Sequence evaluation and HO-3D export (homan_amd/postprocess.py, homan_amd/ho3deval.py, csrc/seqinterp.hip) against the
reference's own outputs (tests/golden/ho3deval_reference.npz, written by tools/refharness/gen_goldens_ho3deval.py from
homan/postprocess.py and homan/eval/ho3devalutils.py) and, at edge shapes, against the reference's formula in numpy."""
import ctypes
import importlib.util
import inspect
import json
import os
import subprocess
import sys
import zipfile

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ho3deval_reference.npz")
GENERATOR = os.path.join(ROOT, "tools", "refharness", "gen_goldens_ho3deval.py")
KEYS = ("hand_verts3d", "hand_joints3d", "obj_verts3d", "hand_roots")
SIGNS = (1.0, -1.0, -1.0)
UNORDER = [0, 5, 6, 7, 10, 11, 12, 17, 18, 19, 13, 14, 15, 1, 2, 3, 4, 8, 12, 16, 20]
STATE_KEYS = ("mano_pca_pose", "mano_rot", "mano_betas", "mano_trans", "rotations_hand", "translations_hand",
              "int_scales_hand", "int_scales_object", "translations_object", "rotations_object", "verts_object_og")
# Largest |difference| of post_process's 21 joints from the reference's golden measured on the MI355X, and the bar at twice
# that ("Sequence evaluation"): no bar existed for joints before.
JOINTS_MEASURED = 5.9604645e-08        # 2^-24: one fp32 ulp at the hand's depth of ~0.5 m
JOINTS_BAR = 2 * JOINTS_MEASURED

_CACHE = {}


def golden():
    if "g" not in _CACHE:
        z = np.load(GOLDEN)
        _CACHE["g"] = {k: z[k] for k in z.files}
    return _CACHE["g"]


def golden_seq_res():
    """the golden sequence as evalho3drecons.py:84-97 collects it: key frames 0, 3, 7 = the one-hand sample's first results"""
    g = golden()
    owner = int(g["pp1_out_hand_verts3d_hand"])
    return {int(f): {"hand_verts3d": g["pp1_out_all_hand_verts3d"][i, owner], "hand_joints3d": g["pp1_out_hand_joints3d"][i],
                     "obj_verts3d": g["seq_in_obj_verts3d"][i], "hand_roots": g["seq_in_hand_roots"][i],
                     "img_path": str(g["pp1_out_img_path"][i])}
            for i, f in enumerate(g["pp1_in_frame_idxs"][:3])}


def reference_formula(key_vals, key_frames, frame_nb):
    """ho3devalutils.py:53-96 in numpy: np.linspace weights, fp32 difference, fp64 blend; the last key held (K == 1 too)"""
    out = []
    for j in range(len(key_frames) - 1):
        n = key_frames[j + 1] - key_frames[j]
        weights = np.linspace(0, 1, n + 1)
        start, end = key_vals[j], key_vals[j + 1]
        vals = start + ((end - start) * weights[:, np.newaxis, np.newaxis])
        out.extend(vals[:n])
    out.extend([key_vals[-1].astype(np.float64)] * (frame_nb - key_frames[-1]))
    return np.stack(out)


def flipped(interp, signs, gather):
    """`.dot(diag(signs))[gather].astype(np.float32)` with the product by the diagonal taken as the sign flip it is"""
    vals = interp * np.asarray(signs, np.float64)
    return (vals if gather is None else vals[:, gather]).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# =============================================================================================== CPU
def test_dump_writes_the_reference_lists_and_a_zip_of_that_file(tmp_path, monkeypatch):
    from homan_amd import ho3deval
    g = golden()
    cwd = tmp_path / "cwd"
    cwd.mkdir()
    monkeypatch.chdir(cwd)
    path = tmp_path / "out" / "pred.json"
    path.parent.mkdir()
    zpath = ho3deval.dump(str(path), list(g["seq_flip_hand_joints3d"]), list(g["seq_flip_obj_verts3d"]))
    with open(path) as fh:
        assert json.load(fh) == [g["dump_out_xyz"].tolist(), g["dump_out_verts"].tolist()]
    assert zpath == str(tmp_path / "out" / "pred.zip")
    with zipfile.ZipFile(zpath) as zf:
        assert zf.namelist() == ["pred.json"]
        assert zf.read("pred.json") == path.read_bytes()
    assert os.listdir(cwd) == []                                    # (the reference drops ./pred.zip here)
    assert sorted(os.listdir(tmp_path)) == ["cwd", "out"] and sorted(os.listdir(path.parent)) == ["pred.json", "pred.zip"]
    copy = tmp_path / "out" / "copy.zip"
    ho3deval.dump(str(path), list(g["seq_flip_hand_joints3d"]), list(g["seq_flip_obj_verts3d"]), copy_to=str(copy))
    assert copy.read_bytes() == (tmp_path / "out" / "pred.zip").read_bytes()
    assert ho3deval.dump(str(path), [], [], codalab=False) is None
    assert sorted(os.listdir(path.parent)) == ["copy.zip", "pred.json", "pred.zip"] and os.listdir(cwd) == []


def _shims():
    spec = importlib.util.spec_from_file_location("_ho3d_shims", os.path.join(ROOT, "tools", "refharness", "shims.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_reproduces_committed_golden(tmp_path):
    if not os.path.isdir(os.path.join(_shims().REFERENCE_ROOT, "homan")):
        pytest.skip("the reference sources are not on this machine")
    out = str(tmp_path / "ho3deval.npz")
    subprocess.run([sys.executable, GENERATOR, out], check=True, cwd=ROOT, capture_output=True, timeout=600)
    a, b = np.load(GOLDEN), np.load(out)
    assert a.files == b.files
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_cfg1_cube_b10_s128.npz"))


def test_golden_holds_what_the_tests_rely_on():
    g = golden()
    assert g["pp1_in_frame_idxs"][:3].tolist() == [0, 3, 7] and g["seq_out_hand_verts3d"].shape == (10, 778, 3)
    assert [g[f"seq_out_{k}"].shape[1] for k in KEYS] == [778, 21, 26, 1]
    assert all(g[f"seq_out_{k}"].dtype == np.float64 and g[f"seq_flip_{k}"].dtype == np.float32 for k in KEYS)
    assert g["pp2_out_hand_sides"].tolist() == ["left", "right"] and g["pp2_in_labels"].tolist() == ["right_hand", "left_hand"]
    assert int(g["pp2_out_hand_verts3d_hand"]) == 1 and g["pp2_out_all_hand_verts3d"].shape == (4, 2, 778, 3)
    # the reference's formula restated above gives the reference's interpolation, bit for bit
    seq = golden_seq_res()
    for k in KEYS:
        want = reference_formula(np.stack([seq[f][k] for f in (0, 3, 7)]), [0, 3, 7], 10)
        np.testing.assert_array_equal(bits(want), bits(g[f"seq_out_{k}"]), err_msg=k)
        got = flipped(g[f"seq_out_{k}"], SIGNS, UNORDER if k == "hand_joints3d" else None)
        np.testing.assert_array_equal(got, g[f"seq_flip_{k}"], err_msg=k)


def _call_interp(h, key_frames, K, N, frame_nb, gather, M, signs=(1.0, 1.0, 1.0), out=1 << 20, key_vals=1 << 20):
    """hm_keyframe_interp with made-up device addresses: every call here must fail its host checks before anything is enqueued"""
    kf = (ctypes.c_int * max(len(key_frames), 1))(*key_frames)
    ga = None if gather is None else (ctypes.c_int * max(len(gather), 1))(*gather)
    sg = (ctypes.c_float * 3)(*signs)
    p = 1 << 20
    return h.hm_keyframe_interp(key_vals, ctypes.addressof(kf), K, N, frame_nb, None if ga is None else ctypes.addressof(ga), M,
                                ctypes.addressof(sg), 0, p, None if ga is None else p, out, None)


def test_host_validation_rejects_before_any_launch():
    from homan_amd import lib
    h = lib.lib()
    assert _call_interp(h, [0, 5, 3], 3, 4, 10, None, 4) == -1                  # unsorted
    assert _call_interp(h, [0, 3, 3], 3, 4, 10, None, 4) == -1                  # not strictly increasing
    assert _call_interp(h, [1, 3, 7], 3, 4, 10, None, 4) == -1                  # first key is not frame 0
    assert _call_interp(h, [0, 3, 11], 3, 4, 10, None, 4) == -1                 # last key above frame_nb
    assert _call_interp(h, [0, 3, 7], 3, 4, 10, [0, 4], 2) == -1                # gather index == N
    assert _call_interp(h, [0, 3, 7], 3, 4, 10, [0, -1], 2) == -1               # gather index below 0
    assert _call_interp(h, [0, 3, 7], 3, 4, 10, None, 3) == -1                  # no gather: M must be N
    assert _call_interp(h, [0, 3, 7], 3, 4, 10, None, 4, signs=(1.0, -1.0, 0.5)) == -1
    assert _call_interp(h, [0, 3, 7], 3, 4, 0, None, 4) == -1                   # no frames
    assert _call_interp(h, [0], 0, 4, 10, None, 4) == -1                        # no keys
    assert _call_interp(h, [0, 3, 7], 3, 4, 10, None, 4, out=None) == -1        # NULL buffers
    assert _call_interp(h, [0, 3, 7], 3, 4, 10, None, 4, key_vals=None) == -1


def test_signatures_and_host_side_helpers():
    from homan_amd import ho3deval, postprocess
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(postprocess.post_process) == ["sample_info", "state_dict", "frame_nb", "mano_model"]
    assert inspect.signature(postprocess.post_process).parameters["frame_nb"].default == 10
    assert params(postprocess.fit_geometry) == ["state_dict", "hand_sides", "mano_model"]
    assert params(ho3deval.interpolate_res) == ["seq_res", "frame_nb", "keys"]
    assert params(ho3deval.interpolate_sequence) == ["seq_res", "frame_nb", "key", "signs", "gather"]
    assert params(ho3deval.evaluate_sequence) == ["seq_res", "frame_nb", "gt_obj_verts", "gt_hand_roots", "obj_faces",
                                                  "mano_faces_closed", "chunk"]
    assert inspect.signature(ho3deval.evaluate_sequence).parameters["chunk"].default == 512
    assert params(ho3deval.dump) == ["pred_out_path", "xyz_pred_list", "verts_pred_list", "codalab", "copy_to"]
    assert list(ho3deval.UNORDER_IDXS) == UNORDER and ho3deval.UNORDER_IDXS.count(12) == 2
    # extend_res (ho3devalutils.py:36-50): regrouped per key; img_paths gains an entry per key AND frame
    seq = {f: {"a": np.full((2, 3), f, np.float32), "b": np.full((1, 3), -f, np.float32), "img_path": f"root/rgb/{f:04d}.png"}
           for f in range(3)}
    full = ho3deval.extend_res(seq, 3, keys=["a", "b"])
    assert [v[0, 0] for v in full["a"]] == [0, 1, 2] and [v[0, 0] for v in full["b"]] == [0, -1, -2]
    assert full["img_paths"] == [f"root/rgb/{f:04d}.png" for f in (0, 0, 1, 1, 2, 2)]
    # summarise (evalho3drecons.py:227-238, split of :140-146)
    per = {"obj_dist": [1.0, 2.0, 6.0], "obj_add-s": [0.5, 1.0, 3.0], "hand_root": [0.1, 0.2, 0.3], "has_contact": [1.0, 0.0, 0.0],
           "pen_depths": [0.01, 0.0, 0.0]}
    mean, median, largest = ho3deval.summarise([per, per], unseen_from=4)
    assert mean["obj_dist"] == 3.0 and median["obj_dist"] == 2.0 and largest["obj_dist"] == 6.0
    assert mean["obj_dist_seen"] == 2.5 and mean["obj_dist_unseen"] == 4.0 and largest["add-s_unseen"] == 3.0
    assert mean["has_contact"] == pytest.approx(1 / 3) and set(mean) == set(median) == set(largest)
    assert set(ho3deval.summarise(per)[0]) == set(per)
    assert "obj_dist_unseen" not in ho3deval.summarise(per, unseen_from=3)[0]
    if not torch.cuda.is_available():            # no CPU path: the GPU stages raise
        with pytest.raises(RuntimeError):
            ho3deval.interpolate_res(golden_seq_res(), 10)
        with pytest.raises(RuntimeError):
            postprocess.fit_geometry({}, ["right"], mano_model=object())


# =============================================================================================== GPU: kernel vs golden
@pytest.mark.gpu
def test_fp64_output_is_bit_equal_to_reference_interpolate_res():
    from homan_amd import ho3deval
    g = golden()
    res = ho3deval.interpolate_res(golden_seq_res(), 10)
    assert set(res) == set(KEYS) | {"img_paths"}
    assert res["img_paths"] == g["seq_out_img_paths"].tolist()
    for k in KEYS:
        got = np.stack(res[k])
        assert len(res[k]) == 10 and got.dtype == np.float64
        np.testing.assert_array_equal(bits(got), bits(g[f"seq_out_{k}"]), err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_fp32_output_with_signs_and_gather_is_bit_equal_to_reference(key):
    from homan_amd import ho3deval
    g = golden()
    gather = UNORDER if key == "hand_joints3d" else None
    got = ho3deval.interpolate_sequence(golden_seq_res(), 10, key, SIGNS, gather)
    assert got.is_cuda and got.dtype == torch.float32
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(g[f"seq_flip_{key}"]))


# =============================================================================================== GPU: edge shapes
def _check_edge(key_vals, key_frames, frame_nb, signs=(1.0, 1.0, 1.0), gather=None):
    from homan_amd import ops
    want = reference_formula(key_vals, list(key_frames), frame_nb)
    assert want.shape == (frame_nb,) + key_vals.shape[1:]
    dev_vals = torch.from_numpy(key_vals).cuda()
    got64 = ops.keyframe_interp(dev_vals, key_frames, frame_nb, out_dtype=torch.float64).cpu().numpy()
    np.testing.assert_array_equal(bits(got64), bits(want))
    got32 = ops.keyframe_interp(dev_vals, key_frames, frame_nb, gather=gather, signs=signs).cpu().numpy()
    np.testing.assert_array_equal(bits(got32), bits(flipped(want, signs, gather)))


def _vals(seed, K, N):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(K, N, 3)) * 0.1 + np.array([0.0, 0.0, 0.5])).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("key_frames,frame_nb", [((0, 1), 2), ((0, 4, 9), 9), ((0, 4, 8), 9), ((0,), 5), ((0,), 1),
                                                 ((0, 1, 2, 3), 3), ((0, 2, 5), 40)])
def test_edge_key_layouts(key_frames, frame_nb):
    _check_edge(_vals(frame_nb, len(key_frames), 21), key_frames, frame_nb, SIGNS)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 21, 65, 171, 778])         # 3 N = 3, 63, 195 (one workgroup), 513 (one lane of a third), 2334
def test_edge_row_counts(N):
    _check_edge(_vals(N, 3, N), (0, 2, 5), 7, SIGNS)


@pytest.mark.gpu
def test_edge_gather_with_a_repeated_row():
    assert UNORDER.count(12) == 2
    _check_edge(_vals(3, 3, 21), (0, 3, 7), 10, SIGNS, UNORDER)
    _check_edge(_vals(4, 2, 5), (0, 6), 8, (-1.0, 1.0, -1.0), [4, 4, 4, 0, 0, 1, 3, 2, 4])


@pytest.mark.gpu
def test_edge_one_segment_of_1000_frames():
    _check_edge(_vals(5, 2, 5), (0, 1000), 1000, SIGNS)
    _check_edge(_vals(6, 2, 5), (0, 1000), 1003, SIGNS)


@pytest.mark.gpu
def test_edge_frame_axis_beyond_one_launch():
    """65537 frames: the frame axis goes out in launches of at most 65535 frames"""
    key_frames = tuple(range(0, 65537, 2048))
    assert key_frames[-1] == 65536
    _check_edge(_vals(7, len(key_frames), 1), key_frames, 65537, SIGNS)


@pytest.mark.gpu
def test_edge_negative_zero_and_denormal_difference():
    tiny, least = np.float32(1.1754944e-38), np.float32(1e-45)          # smallest normal, smallest denormal
    start = np.array([[-0.0, 0.0, -0.0], [-0.0, tiny, least], [1.0, -tiny, 0.0], [-0.0, 0.25, -3.0]], np.float32)
    end = np.array([[-0.0, -0.0, -1.0], [1.0, tiny + 3 * least, 3 * least], [1.0, -tiny - least, -0.0], [0.0, 0.25, -3.0]], np.float32)
    diff = end - start
    assert np.signbit(start[0, 0]) and diff[1, 1] == 3 * least and 0 < abs(diff[2, 1]) < tiny       # denormal differences
    key_vals = np.stack([start, end, start])
    want = reference_formula(key_vals, [0, 4, 6], 8)
    assert np.signbit(want[0, 0, 2]) and np.signbit(want[7, 0, 0]) and not np.signbit(want[1, 0, 0])
    _check_edge(key_vals, (0, 4, 6), 8, SIGNS)
    _check_edge(key_vals, (0, 4, 6), 8, (1.0, 1.0, 1.0), [3, 0, 0])


@pytest.mark.gpu
def test_python_wrapper_refuses_bad_host_arrays():
    from homan_amd import ops
    vals = torch.from_numpy(_vals(0, 3, 4)).cuda()
    for key_frames, frame_nb, gather in (((0, 5, 3), 10, None), ((1, 3, 7), 10, None), ((0, 3, 11), 10, None),
                                         ((0, 3, 7), 10, [0, 4]), ((0, 3), 10, None)):
        with pytest.raises(ValueError):
            ops.keyframe_interp(vals, key_frames, frame_nb, gather=gather)
    with pytest.raises(ValueError):
        ops.keyframe_interp(vals, (0, 3, 7), 10, signs=(1.0, 2.0, 1.0))


# =============================================================================================== GPU: post_process
def _sample(tag):
    g = golden()
    sd = {k: torch.from_numpy(g[f"{tag}_sd_{k}"]) for k in STATE_KEYS}
    obj = {"path": g[f"{tag}_in_obj_path"].tolist()}
    if g[f"{tag}_in_scale"].size:
        obj["scale"] = [float(v) for v in g[f"{tag}_in_scale"]]
    info = {"hands": [{"label": label} for label in g[f"{tag}_in_labels"].tolist()],
            "camera": {"K": torch.from_numpy(g[f"{tag}_in_K"])}, "images": g[f"{tag}_in_images"].tolist(), "objects": [obj],
            "seq_idx": str(g[f"{tag}_in_seq_idx"]), "frame_idxs": g[f"{tag}_in_frame_idxs"].tolist()}
    return info, sd


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["pp1", "pp2"])
def test_post_process_against_reference_golden(tag, mano_model):
    from homan_amd import postprocess
    from homan_amd.manomodel import ManoModel
    g = golden()
    info, sd = _sample(tag)
    frames = len(info["frame_idxs"])
    infos, seq_idx, frame_idxs = postprocess.post_process(info, sd, frame_nb=frames, mano_model=ManoModel(mano_model=mano_model))
    assert seq_idx == info["seq_idx"] and frame_idxs == info["frame_idxs"] and len(infos) == frames
    owner = int(g[f"{tag}_out_hand_verts3d_hand"])
    joints_diff = 0.0
    for f, res in enumerate(infos):
        assert set(res) == {"all_hand_verts3d", "hand_verts3d", "hand_joints3d", "camintr", "img_path", "side", "obj_path",
                            "obj_rot", "obj_trans", "obj_scale", "hand_sides"}
        want_all = g[f"{tag}_out_all_hand_verts3d"][f]
        assert len(res["all_hand_verts3d"]) == want_all.shape[0]
        for got, want in zip(res["all_hand_verts3d"], want_all):
            assert got.dtype == np.float32
            np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)         # the bar get_verts_hand holds (test_model_gpu.py)
        np.testing.assert_array_equal(res["hand_verts3d"], res["all_hand_verts3d"][owner])      # the LAST hand's
        assert res["hand_joints3d"].shape == (21, 3)
        joints_diff = max(joints_diff, float(np.abs(res["hand_joints3d"].astype(np.float64) - g[f"{tag}_out_hand_joints3d"][f]).max()))
        # R = rot6d_to_matrix: entries of modulus <= 1 through two normalisations (3 products, 2 sums, a square root and a
        # division each), a projection and a cross product, every step rounded to fp32 on both sides: a dozen roundings of
        # 2^-24 relative on values <= 1 bound the difference by 1e-6
        np.testing.assert_allclose(res["obj_rot"], g[f"{tag}_out_obj_rot"][f], rtol=0, atol=1e-6)
        np.testing.assert_array_equal(res["obj_trans"], g[f"{tag}_out_obj_trans"][f])
        assert res["obj_trans"].shape == (1, 3) and res["obj_rot"].shape == (3, 3)
        assert res["obj_scale"] == float(g[f"{tag}_out_obj_scale"][f]) and isinstance(res["obj_scale"], float)
        np.testing.assert_array_equal(res["camintr"], g[f"{tag}_out_camintr"][f])
        assert res["img_path"] == str(g[f"{tag}_out_img_path"][f]) and res["obj_path"] == str(g[f"{tag}_out_obj_path"][f])
        assert res["side"] == str(g[f"{tag}_out_side"][f]) and res["hand_sides"] == g[f"{tag}_out_hand_sides"].tolist()
    print(f"post_process {tag}: largest joint difference from the reference {joints_diff:.3e} m (bar {JOINTS_BAR:.3e})")
    assert joints_diff <= JOINTS_BAR


@pytest.mark.gpu
def test_post_process_accepts_a_bare_float_scale(mano_model):
    """the documented divergence: the reference's isinstance test raises on a number (postprocess.py:105)"""
    from homan_amd import postprocess
    from homan_amd.manomodel import ManoModel
    info, sd = _sample("pp1")
    info["objects"][0]["scale"] = 1.25
    infos, _, _ = postprocess.post_process(info, sd, frame_nb=2, mano_model=ManoModel(mano_model=mano_model))
    assert len(infos) == 2 and infos[0]["obj_scale"] == float(golden()["pp1_out_obj_scale"][0])
    geo = postprocess.fit_geometry(sd, ["right"], ManoModel(mano_model=mano_model))
    assert all(geo[k].is_cuda for k in ("hand_verts", "hand_joints", "obj_rot", "obj_trans", "obj_verts"))
    assert geo["hand_verts"].shape == (1, 4, 778, 3) and geo["hand_joints"].shape == (1, 4, 21, 3)
    np.testing.assert_array_equal(geo["hand_verts"][0, 0].cpu().numpy(), infos[0]["hand_verts3d"])


# =============================================================================================== GPU: evaluate_sequence
def _ground_truth():
    g = golden()
    rng = np.random.default_rng(21)
    gt_obj = g["seq_flip_obj_verts3d"].astype(np.float64) + rng.normal(size=(10, 26, 3)) * 0.004 + np.array([0.01, 0.0, -0.005])
    gt_roots = g["seq_flip_hand_joints3d"][:, :1].astype(np.float64) + rng.normal(size=(10, 1, 3)) * 0.01
    return gt_obj, gt_roots


@pytest.mark.gpu
def test_evaluate_sequence_equals_frame_by_frame_pointmetrics(mano_model):
    from homan_amd import ho3deval, pointmetrics
    g = golden()
    gt_obj, gt_roots = _ground_truth()
    closed = np.asarray(mano_model["closed_faces"])
    runs = {chunk: ho3deval.evaluate_sequence(golden_seq_res(), 10, gt_obj, gt_roots, g["obj_faces"], closed, chunk=chunk)
            for chunk in (1, 4, 512)}
    res = runs[4]
    np.testing.assert_array_equal(bits(res["export_joints"]), bits(g["seq_flip_hand_joints3d"]))
    np.testing.assert_array_equal(bits(res["export_verts"]), bits(g["seq_flip_hand_verts3d"]))
    pred_obj, pred_hand = torch.from_numpy(g["seq_flip_obj_verts3d"]), torch.from_numpy(g["seq_flip_hand_verts3d"])
    hand_faces, obj_faces = torch.from_numpy(closed)[None].cuda(), torch.from_numpy(g["obj_faces"])[None].cuda()
    for f in range(10):
        point = pointmetrics.get_point_metrics(pred_obj[f:f + 1], torch.Tensor(gt_obj[f:f + 1]).float())      # prediction first
        inter = pointmetrics.get_inter_metrics(pred_hand[f:f + 1].cuda(), pred_obj[f:f + 1].cuda(), hand_faces, obj_faces)
        assert res["obj_dist"][f] == point["verts_dists"][0] and res["obj_add-s"][f] == point["add-s"][0], f
        assert res["pen_depths"][f] == inter["pen_depths"][0] and res["has_contact"][f] == float(inter["has_contact"][0]), f
        # (norm of three fp64 terms: the two summation orders differ by an ulp or two)
        np.testing.assert_allclose(res["hand_root"][f], np.linalg.norm(g["seq_flip_hand_joints3d"][f][0] - gt_roots[f][0]),
                                   rtol=1e-14, atol=0)
    assert res["obj_dist"].min() > 0 and not np.array_equal(res["obj_dist"], res["obj_add-s"])
    for key, vals in res.items():
        assert len(vals) == 10, key
        for chunk in (1, 512):
            assert np.array_equal(vals, runs[chunk][key]), (key, chunk)
    mean, median, largest = ho3deval.summarise(res, unseen_from=7)
    assert mean["obj_dist"] == float(np.mean(res["obj_dist"])) and largest["hand_root"] == float(res["hand_root"].max())
    assert mean["obj_dist_unseen"] == float(np.mean(res["obj_dist"][7:]))


@pytest.mark.gpu
def test_evaluate_sequence_contact(mano_model):
    """the hand pushed into the object: contact and a positive depth; 0.3 m apart: none"""
    from homan_amd import ho3deval, synth
    g = golden()
    hand = np.asarray(mano_model["v_template"], np.float32) + np.array([0.0, 0.0, 0.5], np.float32)
    box, faces = synth.box_mesh(2, 2, 2, scale=0.08)
    box = np.asarray(box, np.float32) - np.asarray(box, np.float32).mean(0)
    joints = np.zeros((21, 3), np.float32) + hand.mean(0)
    closed = np.asarray(mano_model["closed_faces"])

    def run(offset):
        seq = {f: {"hand_verts3d": hand + np.float32(0.001 * f), "hand_joints3d": joints,
                   "obj_verts3d": (box + hand.mean(0) + np.asarray(offset, np.float32) + np.float32(0.001 * f)).astype(np.float32),
                   "img_path": "seq/rgb/0000.png"} for f in (0, 5)}
        gt_obj = np.zeros((6, 26, 3)) + np.array([0.0, 0.0, -0.5])
        return ho3deval.evaluate_sequence(seq, 6, gt_obj, np.zeros((6, 3)), faces, closed, chunk=4)
    inside, apart = run([0.0, 0.0, 0.0]), run([0.3, 0.0, 0.0])
    assert inside["has_contact"].max() == 1.0 and inside["pen_depths"].max() > 0
    assert np.array_equal(inside["has_contact"], (inside["pen_depths"] > 0).astype(np.float64))
    assert apart["has_contact"].max() == 0.0 and apart["pen_depths"].max() == 0.0
    assert g["obj_faces"].shape == np.asarray(faces).shape
