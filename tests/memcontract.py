"""The memory contract of the C ABI as a table: for every pointer parameter of the audited entry points, the alignment in bytes
that include/homan_amd.h demands (Conventions, and the ALIGNMENT notes of the entry points; the audit is DESIGN.md section 9).

CONTRACT = {entry: {param: bytes}} drives tests/test_memcontract.py (completeness against the header, host-only rejection of
every requirement above the declared type's and of every workspace base) and tests/test_memcontract_gpu.py (every buffer of a
placed run sits at the LOWEST alignment its row accepts)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HM_ERR_BAD_ARG = -1

# alignment of the type a parameter is declared with; `void` declares nothing, so every void row is a stated requirement
NATURAL = {"float": 4, "int": 4, "double": 8, "unsigned char": 1, "void": 1}

# entry points whose every pointer parameter must have a row (the completeness test reads the header)
IN_SCOPE = (
    "hm_cloud_metrics", "hm_align_stats", "hm_procrustes_align", "hm_threshold_counts", "hm_fscore", "hm_keyframe_interp",
    "hm_solid_voxels", "hm_voxel_overlap", "hm_mesh_volume", "hm_point_mesh_distance", "hm_surface_contact_fwd",
    "hm_surface_contact_bwd", "hm_softsil_fwd", "hm_softsil_bwd", "hm_softsil_pose_terms", "hm_sigma_anneal", "hm_edge_edt",
    "hm_pose_edge_terms", "hm_pose_keep_best", "hm_pose_keep_best_log", "hm_offscreen_fwd", "hm_scale_by", "hm_mask_crop_resize",
    "hm_target_masks", "hm_instance_masks", "hm_sil_fwd", "hm_sil_reduce", "hm_sil_bwd", "hm_sil_read_idx_map",
    "hm_sil_read_parts",
)

_SIL_FWD = {"verts": 4, "faces": 4, "K": 4, "keep": 8, "ref": 8, "keep_sum": 4, "pooled": 4, "loss_out": 4, "work_order": 4,
            "pooled_depth": 4, "alpha_full": 8, "rigid_rot6d": 4, "rigid_trans": 4, "rigid_scale": 4, "workspace": 16}
_SIL_BWD = {"verts": 4, "K": 4, "upstream": 4, "grad_pooled": 8, "keep_sum": 4, "adj_off": 4, "adj_items": 4, "grad_verts": 4,
            "grad_ndc": 4, "workspace": 16}
_SIL_REDUCE = {"keep_sum": 4, "loss_out": 4, "frame_out": 4, "workspace": 16}

CONTRACT = {
    "hm_cloud_metrics": {"x": 4, "y": 4, "aff_x": 4, "aff_y": 4, "x_d2": 4, "x_idx": 4, "y_d2": 4, "y_idx": 4, "out4": 8,
                         "workspace": 8},
    "hm_align_stats": {"gt_hand": 4, "pred_hand": 4, "aff_gt": 4, "aff_pred": 4, "hand_mean": 8},
    "hm_procrustes_align": {"pred": 4, "gt": 4, "aligned": 4, "err": 8, "xform": 8},
    "hm_threshold_counts": {"dist": 8, "val_max": 8, "counts": 8},
    "hm_fscore": {"x_d2": 4, "y_d2": 4, "thresholds": 4, "out": 8},
    "hm_keyframe_interp": {"key_vals": 4, "key_frames": 4, "gather": 4, "signs": 4, "key_frames_dev": 4, "gather_dev": 4,
                           "out": 8},
    "hm_solid_voxels": {"verts": 4, "faces": 4, "boxes": 4, "boxes_dev": 4, "words": 4},
    "hm_voxel_overlap": {"a": 4, "b": 4, "counts": 8},
    "hm_mesh_volume": {"verts": 4, "faces": 4, "out": 8},
    "hm_point_mesh_distance": {"points": 4, "verts": 4, "faces": 4, "d2": 4, "face_idx": 4, "inside": 4, "closest": 4,
                               "workspace": 8},
    "hm_surface_contact_fwd": {"points": 4, "verts": 4, "faces": 4, "weights": 4, "out": 4, "grad_points": 4, "inside": 4,
                               "grad_verts_attr": 4, "grad_verts_rep": 4, "value": 4, "bary": 4, "d2": 4, "face_idx": 4,
                               "workspace": 8},
    "hm_surface_contact_bwd": {"unit_points": 4, "inside": 4, "unit_verts_attr": 4, "unit_verts_rep": 4, "upstream": 4,
                               "grad_points": 4, "grad_verts": 4},
    "hm_softsil_fwd": {"verts": 4, "faces": 4, "K": 4, "sigma": 4, "alpha": 4, "workspace": 4},
    "hm_softsil_bwd": {"verts": 4, "faces": 4, "K": 4, "sigma": 4, "alpha": 4, "grad_alpha": 4, "adj_off": 4, "adj_items": 4,
                       "grad_verts": 4, "workspace": 4},
    "hm_softsil_pose_terms": {"alpha": 4, "keep": 4, "ref": 4, "terms": 4, "grad": 4, "workspace": 4},
    "hm_sigma_anneal": {"sigma": 4},
    "hm_edge_edt": {"ref": 4, "edt": 4, "band_count": 4},
    "hm_pose_edge_terms": {"alpha": 4, "keep": 4, "ref": 4, "edt": 4, "terms": 4, "grad": 4, "workspace": 4},
    "hm_pose_keep_best": {"sums": 4, "extra": 4, "rot6d": 4, "trans": 4, "best_loss": 4, "best_rot6d": 4, "best_trans": 4,
                          "losses_out": 4},
    "hm_pose_keep_best_log": {"sums": 4, "extra": 4, "rot6d": 4, "trans": 4, "step": 4, "log": 4, "losses_out": 4},
    "hm_offscreen_fwd": {"verts": 4, "K": 4, "out": 4, "grad": 4},
    "hm_scale_by": {"in": 4, "s": 4, "out": 4},
    "hm_mask_crop_resize": {"masks": 4, "index": 4, "boxes": 4, "out": 1},
    "hm_target_masks": {"target": 4, "target_index": 4, "occluders": 4, "occluder_index": 4, "boxes": 4, "out": 4},
    "hm_instance_masks": {"idx_map": 4, "face_start": 4, "out": 1},
    "hm_sil_fwd": _SIL_FWD,
    "hm_sil_reduce": _SIL_REDUCE,
    "hm_sil_bwd": _SIL_BWD,
    "hm_sil_read_idx_map": {"workspace": 16, "out": 4},
    "hm_sil_read_parts": {"workspace": 16, "out": 8},
    "hm_sil_read_faces9": {"workspace": 16, "out": 4},
    # ---- outside the audited set: only the rows the audit found above the declared type's alignment
    "hm_sil_fwd_clips": {"keep": 8, "ref": 8, "alpha_full": 8, "workspace": 16},
    "hm_sil_fwd_phase_clips": {"keep": 8, "ref": 8, "alpha_full": 8, "workspace": 16},
    "hm_sil_reduce_clips": {"workspace": 16},
    "hm_sil_bwd_clips": {"grad_pooled": 8, "workspace": 16},
    "hm_sil_bwd_phase_clips": {"grad_pooled": 8, "workspace": 16},
    "hm_depth_bwd": {"workspace": 16},
    "hm_depth_bwd_sparse": {"gflags": 4, "workspace": 16},
    "hm_ordinal_depth_fwd": {"frame_part": 8, "workspace": 4},
    "hm_mano_fwd": {"model": 16}, "hm_mano_fwd_clips": {"model": 16}, "hm_mano_fwd_rows": {"model": 16},
    "hm_mano_bwd": {"model": 16, "workspace": 4}, "hm_mano_bwd_rows": {"model": 16, "workspace": 4},
    "hm_mano_bwd_rigid_clips": {"model": 16, "workspace": 4},
    "hm_rigid_bwd": {"workspace": 8}, "hm_rigid_bwd_clips": {"workspace": 8},
    "hm_rigid_bwd_sil": {"sil_parts": 16, "workspace": 8}, "hm_rigid_bwd_sil_clips": {"sil_parts": 16, "workspace": 8},
    "hm_collision_fwd": {"workspace": 16}, "hm_collision_fwd_clips": {"workspace": 16},
    "hm_collision_dist_values": {"workspace": 16}, "hm_collision_read_grid": {"workspace": 16},
    "hm_collision_read_needed": {"workspace": 16},
    # every other entry point that takes the silhouette workspace (hm_sil_fwd_multi and hm_sil_parts: tests of their own)
    "hm_sil_hint_near_winding": {"workspace": 16}, "hm_shade_rgb": {"workspace": 16}, "hm_sil_invalidate_outputs": {"workspace": 16},
    "hm_sil_read_boxes": {"workspace": 16}, "hm_sil_read_owned": {"workspace": 16}, "hm_bench_sil_kernels": {"workspace": 16},
    "hm_sil_timestamps": {"workspace": 16}, "hm_sil_timestamps_save": {"workspace": 16}, "hm_sil_timestamps_read": {"workspace": 16},
    # the reduce workspaces (hm_reduce_workspace_bytes): fp32 partials and a 32-bit ticket
    "hm_v2d_fwd": {"workspace": 4}, "hm_v2d_fwd_clips": {"workspace": 4}, "hm_smooth_fwd": {"workspace": 4},
    "hm_smooth_fwd_clips": {"workspace": 4}, "hm_inter_fwd": {"workspace": 4}, "hm_inter_fwd_clips": {"workspace": 4},
    "hm_hand_terms_fwd_clips": {"workspace": 4}, "hm_nn_fwd": {"workspace": 4}, "hm_nn_fwd_clips": {"workspace": 4},
    "hm_nn_fwd_rigid_clips": {"workspace": 4}, "hm_contact_fwd": {"workspace": 4}, "hm_contact_fwd_clips": {"workspace": 4},
    "hm_pair_terms_fwd_clips": {"ws_nn": 4, "ws_inter": 4, "ws_smooth": 4, "ws_hand": 4},
    # the optimiser's slot records (pointers and a long) behind a void pointer
    "hm_adam_step": {"slots": 8}, "hm_adam_step_log": {"slots": 8},
}

# a requirement that holds only under some arguments: the values that switch it on (the row's figure is the strictest case;
# otherwise the parameter needs the alignment in LOWEST)
WHEN = {
    ("hm_threshold_counts", "dist"): {"is_f64": 1},
    ("hm_keyframe_interp", "out"): {"out_f64": 1},
    ("hm_mask_crop_resize", "masks"): {"masks_f32": 1},
    ("hm_target_masks", "target"): {"target_f32": 1},
    ("hm_target_masks", "occluders"): {"occluders_f32": 1, "K": 1, "No": 1},
    ("hm_sil_bwd", "grad_pooled"): {"mode": 3}, ("hm_sil_bwd_clips", "grad_pooled"): {"mode": 3},
    ("hm_sil_bwd_phase_clips", "grad_pooled"): {"mode": 3},
    # keep / ref: in the per-sample mode, i.e. together with alpha_full (the fake addresses of the rejection test are all non-NULL)
}
LOWEST = {("hm_threshold_counts", "dist"): 4, ("hm_keyframe_interp", "out"): 4, ("hm_mask_crop_resize", "masks"): 1,
          ("hm_target_masks", "target"): 1, ("hm_target_masks", "occluders"): 1, ("hm_sil_bwd", "grad_pooled"): 4,
          ("hm_sil_fwd", "keep"): 4, ("hm_sil_fwd", "ref"): 4}

# parameters the entry point reads ON THE HOST during the call: the rejection test hands them real arrays.  `model` is the host
# array of 8 device pointers of the MANO entries; its row is the requirement on model[4] (lbs_weights)
HOST_PARAMS = {"hm_solid_voxels": {"boxes"}, "hm_instance_masks": {"face_start"},
               "hm_keyframe_interp": {"key_frames", "gather", "signs"}, "hm_fscore": {"thresholds"},
               "hm_threshold_counts": {"val_max"}, "hm_mano": {"model", "g_terms", "weights"}, "hm_rigid": {"g_terms", "weights"},
               "hm_shade_rgb": {"light_dir", "background"}, "hm_bench_sil_kernels": {"avg_ms"}, "hm_sil_timestamps_read": {"us3"}}

# optional pointers the rejection calls leave NULL, because giving them would be refused for a reason of its own
NULLS = {"hm_sil_bwd_clips": {"loss_out"}, "hm_sil_bwd_phase_clips": {"loss_out"}}

# by-value arguments of the rejection calls: small and valid, so that the alignment check is what refuses the call.  Integers
# that are not named get 2, floats 1.0.
SMALL = {
    "hm_cloud_metrics": dict(B=2, N=5, M=7),
    "hm_threshold_counts": dict(n=9, steps=3),
    "hm_keyframe_interp": dict(K=3, N=5, frame_nb=7, M=3),
    "hm_solid_voxels": dict(B=2, V=8, F=12, NWX=1, NY=4, NZ=4),
    "hm_voxel_overlap": dict(a_sets=1, B=2, words_per_frame=16),
    "hm_point_mesh_distance": dict(B=2, N=5, V=8, F=12),
    "hm_surface_contact_fwd": dict(B=2, N=5, V=8, F=12, log2q=-40),
    "hm_softsil_fwd": dict(B=2, V=8, F=12, S=8, znear=0.1, zfar=100.0),
    "hm_softsil_bwd": dict(B=2, V=8, F=12, S=8, znear=0.1, zfar=100.0),
    "hm_softsil_pose_terms": dict(N=2, S=8),
    "hm_pose_edge_terms": dict(N=2, size=16, stride=16, kernel_size=7),
    "hm_mask_crop_resize": dict(N=2, H=5, W=7, R=2, S=4),
    "hm_target_masks": dict(mode=0, Nt=2, H=5, W=7, R=2, S=4),
    "hm_sil": dict(B=2, V=8, F=12, S=32, faces_bstride=0, znear=0.1, zfar=100.0, mask_shared=1, rigid_abs=0, persistent_outputs=0,
                   clip_len=0, out_stride=0, phases=3, sum_log2q=0, mode=0, eps=1e-3),
    "hm_sil_hint_near_winding": dict(winding=1),
    "hm_depth": dict(B=2, V=8, F=12, S=64),
    "hm_ordinal_depth_fwd": dict(B=2, S=32),
    "hm_mano": dict(pca_dim=16, B=2, clip_len=0, row0=0, row_stride=1, n_terms=0, frame_stride=3),
    "hm_rigid": dict(abs_scale=0, n_terms=0, frame_stride=3, N=2, V=8, F=12, clip_len=0, sum_log2q=0),
    "hm_collision": dict(V0=8, F0=12, V1=8, F1=12, B=2, clip_len=0, out_stride=0, which=1, V=8, F=12),
}


def _by_prefix(table, entry, default):
    """the value under the longest key of `table` that `entry` starts with (hm_sil covers hm_sil_fwd_clips, ...)"""
    keys = [k for k in table if entry == k or entry.startswith(k + "_")]
    return table[max(keys, key=len)] if keys else default


def small_values(entry):
    return _by_prefix(SMALL, entry, {})


def host_params(entry):
    return _by_prefix(HOST_PARAMS, entry, set())


def header_params(entry=None):
    """{entry: [(base type, is_pointer, name), ...]} parsed off include/homan_amd.h with this module's own regex"""
    text = open(os.path.join(ROOT, "include", "homan_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(hm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.S):
        params = []
        for p in filter(None, (q.strip() for q in m.group(2).split(","))):
            if p == "void":
                continue
            words = p.replace("*", " * ").split()
            name = words.pop()
            base = " ".join(w for w in words if w not in ("*", "const"))
            params.append((base, "*" in words, name))
        out[m.group(1)] = params
    return out if entry is None else out[entry]


def is_workspace(name):
    return name == "workspace" or name.startswith("ws_")


def elevated_rows():
    """(entry, param, bytes, declared alignment) for every row the entry point must ENFORCE: above the declared type's alignment,
    or a workspace base"""
    decl = header_params()
    rows = []
    for entry, row in CONTRACT.items():
        types = {name: base for base, ptr, name in decl[entry] if ptr}
        for param, nbytes in row.items():
            nat = NATURAL[types[param]]
            if param == "model":
                nat = 4                                   # model[4] points to fp32
            if nbytes > nat or is_workspace(param):
                rows.append((entry, param, nbytes, nat))
    return rows


class FakeCall:
    """Arguments for one call that must be refused before anything is dereferenced on the device: integer addresses on a
    256-aligned grid for every device pointer, real host arrays where the entry point reads on the host, SMALL by-value arguments."""
    BASE = 0x7f0000000000                                 # (never dereferenced)

    def __init__(self, entry, overrides=None):
        self.entry = entry
        self.keep = []                                    # host arrays stay alive for the call
        vals = dict(small_values(entry))
        vals.update(overrides or {})
        self.params = header_params(entry)
        self.args = {}
        for i, (base, ptr, name) in enumerate(self.params):
            if ptr and name in NULLS.get(entry, ()):
                self.args[name] = None
            elif ptr:
                self.args[name] = self._host(name) if name in host_params(entry) else self.BASE + 0x100000 * (i + 1)
            elif base == "hipStream_t":
                self.args[name] = None
            elif base == "float":
                self.args[name] = float(vals.get(name, 1.0))
            else:
                self.args[name] = int(vals.get(name, 2))

    def _host(self, name):
        if name == "model":
            arr = self.model = (ctypes.c_void_p * 8)(*[self.BASE + 0x100000 * (40 + k) for k in range(8)])
        elif name == "g_terms":
            arr = (ctypes.c_void_p * 5)()
        else:
            data = {"key_frames": np.array([0, 3, 6], np.int32), "gather": np.array([4, 0, 2], np.int32),
                    "signs": np.array([1, -1, -1], np.float32), "thresholds": np.full(8, 0.5, np.float32),
                    "val_max": np.array([1.0], np.float64), "boxes": np.array([0, 0, 0, 4, 4, 4] * 2, np.int32),
                    "face_start": np.array([0, 1, 2, 2, 2, 2, 2, 2, 2], np.int32), "weights": np.ones(5, np.float32),
                    "light_dir": np.ones(3, np.float32), "background": np.zeros(3, np.float32),
                    "avg_ms": np.zeros(3, np.float32), "us3": np.zeros(3, np.float32)}[name]
            self.keep.append(data)
            return data.ctypes.data
        self.keep.append(arr)
        return ctypes.cast(arr, ctypes.c_void_p).value

    def misalign(self, param, by):
        if param == "model":
            self.model[4] = self.model[4] + by
        else:
            self.args[param] += by
        return self

    def __call__(self, handle):
        return getattr(handle, self.entry)(*[self.args[name] for _, _, name in self.params])
