"""Evaluation metrics of reference homan/eval/pointmetrics.py on the HIP kernels.

`get_point_metrics` (:17-44) and `get_align_metrics` (:61-99) - chamfer, ADD-S, vertex and hand-aligned errors, which the
reference computes with pytorch3d's `chamfer_distance` and scipy's `cKDTree` - run on an exact brute-force nearest-neighbour
search in both directions (`hm_cloud_metrics`, csrc/pointmetrics.hip) and the alignment statistics of `hm_align_stats`.
`get_inter_metrics` (:102-124, called by fit_vid_dataset.py:488-493) reads how deep the hand reaches into the object off
the object's signed-distance grid.  Inputs are torch tensors on any device and of any float dtype; they are moved to the GPU
as contiguous fp32, and each call syncs with the host once.  There is no CPU path: without a GPU these functions raise.
"""
import numpy as np
import torch

from . import constants, lib, ops


def _one_hand_mesh_per_scene(verts_person, faces_person, scenes):
    """(scenes * hands, Vh, 3) vertices ordered scene-major and (hands, Fh, 3) faces -> ONE mesh per scene: the hands'
    vertices laid end to end and their faces re-indexed into that concatenation.  (The reference offsets the second hand's
    faces by the length of the ALREADY merged vertex array, pointmetrics.py:104-110, i.e. past its end; the offset that
    indexes the second hand's block - one hand's vertex count - is used here.)"""
    hands, per_hand = verts_person.shape[0] // scenes, verts_person.shape[1]
    if hands > 3:
        raise ValueError(f"Invalid hand nb {hands}")
    faces_person = torch.as_tensor(faces_person)
    if hands == 1:
        return verts_person, faces_person[0]
    merged = verts_person.reshape(scenes, hands * per_hand, 3)
    faces = torch.cat([faces_person[h % faces_person.shape[0]] + h * per_hand for h in range(hands)], 0)
    return merged, faces


def get_inter_metrics(verts_person, verts_object, faces_person, faces_object):
    """verts_person (B*hand_nb, Vh, 3), verts_object (B, Vo, 3), faces_person (hand_nb, Fh, 3) closed hand faces,
    faces_object (>=1, Fo, 3)  ->  {"pen_depths": [B floats], "has_contact": [B bools]}.
    pen_depth = the largest value the object's clamped SDF takes at a hand vertex, in world units
    (`sdf_meta["dist_values"][(1, 0)]` of reference interactions/scenesdf.py:141-146); contact = any vertex inside."""
    scenes = verts_object.shape[0]
    hand_verts, hand_faces = _one_hand_mesh_per_scene(verts_person, faces_person, scenes)
    cctx = ops.CollisionContext(hand_faces.cpu().numpy(), torch.as_tensor(faces_object)[0], scenes, hand_verts.shape[1],
                                verts_object.shape[1], verts_object.device)
    depth_in_object = ops.collision_dist_values(hand_verts.contiguous(), verts_object, cctx, constants.SDF_SCALE_FACTOR)[(1, 0)]
    deepest = depth_in_object.amax(dim=1)
    return {"pen_depths": deepest.cpu().numpy().tolist(), "has_contact": (deepest > 0).cpu().numpy().tolist()}


def _on_gpu(*tensors):
    """The inputs as contiguous fp32 tensors on ONE GPU (the first CUDA input's device, else the current one)."""
    if not torch.cuda.is_available():
        raise lib.HomanAmdError("homan_amd.pointmetrics needs the GPU (there is no CPU fallback)")
    dev = next((t.device for t in tensors if t.is_cuda), torch.device("cuda"))
    return [t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in tensors]


def _check_clouds(**clouds):
    for name, t in clouds.items():
        if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] == 0 or t.shape[1] == 0:
            raise ValueError(f"{name}: expected a non-empty (B, N, 3) tensor, got {tuple(t.shape)}")
        if not t.is_floating_point():
            raise ValueError(f"{name}: expected a float tensor, got {t.dtype}")


def get_point_metrics(gt_points, pred_points):
    """gt_points (B,N,3), pred_points (B,M,3) -> {"chamfer_dists", "add-s", "verts_dists"}: lists of B floats.
    chamfer = mean_i min_j |g_i - p_j|^2 + mean_j min_i |p_j - g_i|^2 (pytorch3d chamfer_distance, batch_reduction=None);
    add-s = mean_i min_j |g_i - p_j| (cKDTree on pred queried with gt); verts_dists = mean_i |g_i - p_i| when N == M, else
    the add-s list (reference :37-43)."""
    _check_clouds(gt_points=gt_points, pred_points=pred_points)
    if gt_points.shape[0] != pred_points.shape[0]:
        raise ValueError(f"batch sizes differ: {gt_points.shape[0]} vs {pred_points.shape[0]}")
    gt, pred = _on_gpu(gt_points, pred_points)
    with torch.cuda.device(gt.device):          # (the launches go to the current stream of the inputs' device)
        tab = ops.cloud_metrics(gt, pred)
        chamfer, adds, verts = torch.stack([tab[:, 0] + tab[:, 1], tab[:, 2], tab[:, 3]]).cpu().tolist()
    return {"chamfer_dists": chamfer, "add-s": adds, "verts_dists": verts if gt.shape[1] == pred.shape[1] else list(adds)}


def repeat_hand_nb(tens, hand_nb):
    """Per-frame values repeated for each hand, frame-major, hand-minor (reference :47-58): (B,) -> (B*hand_nb, 1, 1),
    (B,C) -> (B*hand_nb, C, 1), (B,K,C) -> (B*hand_nb, K, C)."""
    if tens.dim() < 3:
        tens = tens.reshape(tens.shape[0], -1, 1)
    return tens.repeat_interleave(hand_nb, dim=0)


def get_align_metrics(gt_hand_verts, pred_hand_verts, gt_obj_verts, pred_obj_verts, pred_centroid_from_gt=True):
    """Hand-aligned errors: hands (B*h, Vh, 3) frame-major, objects (B, No, 3) and (B, Mo, 3) ->
    {"hand_mean_aligned": B*h floats, "obj_chamfer_aligned": B floats}.

    The first hand of each frame gives the centroids c and the scales s = sqrt(sum_i |v_i - c|^2 / Vh); the prediction
    (hands and object) is mapped to ((p - c_pred) / s_pred) * s_gt and the ground truth to g - c_gt.  hand_mean_aligned is
    the mean vertex distance of each aligned hand, obj_chamfer_aligned the chamfer distance of the aligned objects.

    pred_centroid_from_gt=True (default) reproduces the reference, which takes c_pred from the GROUND TRUTH hand
    (pointmetrics.py:68): the prediction is centred on the ground truth's centroid and s_pred is measured about that point
    - the computation behind the published numbers.  False uses the prediction's own first-hand centroid: the metrics are
    then invariant to a translation plus a positive scale of the prediction."""
    _check_clouds(gt_hand_verts=gt_hand_verts, pred_hand_verts=pred_hand_verts, gt_obj_verts=gt_obj_verts,
                  pred_obj_verts=pred_obj_verts)
    frames = gt_obj_verts.shape[0]
    hand_nb = gt_hand_verts.shape[0] // frames
    if hand_nb < 1 or gt_hand_verts.shape[0] != hand_nb * frames:
        raise ValueError(f"{gt_hand_verts.shape[0]} hands for {frames} frames")
    if pred_hand_verts.shape != gt_hand_verts.shape:
        raise ValueError(f"hand shapes differ: {tuple(gt_hand_verts.shape)} vs {tuple(pred_hand_verts.shape)}")
    if pred_obj_verts.shape[0] != frames:
        raise ValueError(f"batch sizes differ: {frames} vs {pred_obj_verts.shape[0]}")
    gt_h, pred_h, gt_o, pred_o = _on_gpu(gt_hand_verts, pred_hand_verts, gt_obj_verts, pred_obj_verts)
    with torch.cuda.device(gt_h.device):
        aff_gt, aff_pred, hand_mean = ops.align_stats(gt_h, pred_h, frames, pred_centroid_from_gt)
        tab = ops.cloud_metrics(pred_o, gt_o, aff_x=aff_pred, aff_y=aff_gt)
        values = torch.cat([hand_mean, tab[:, 0] + tab[:, 1]]).cpu().tolist()
    return {"hand_mean_aligned": values[:hand_nb * frames], "obj_chamfer_aligned": values[hand_nb * frames:]}


def index_boxes(lo, hi, h):
    """fp32 bounds (..., 3) of meshes -> inclusive voxel index boxes (first, last), int64: floor(min / h) - 1 .. floor(max / h)
    + 1 per axis, the division in double.  The one-voxel margin absorbs the rounding of the division and of the fp32 centres."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("vertices are not finite")
    first, last = np.floor(lo / float(h)) - 1, np.floor(hi / float(h)) + 1
    if max(np.abs(first).max(), np.abs(last).max()) > ops.VOXEL_MAX_INDEX:
        raise ValueError(f"voxel index beyond +-{ops.VOXEL_MAX_INDEX}: the mesh is too far from the origin for a pitch of {h}")
    return first.astype(np.int64), last.astype(np.int64)


def common_boxes(verts_hands, verts_object, h):
    """device (B, N, 3) vertices of all hands of each frame and (B, Vo, 3) of the object -> (boxes (B,6) int64 {i0, j0, k0, nx,
    ny, nz}, (NWX, NY, NZ)): per frame the intersection of the two meshes' index boxes, extents 0 where they do not meet, and
    the launch dimensions that hold every frame.  One read-back."""
    bounds = torch.stack([verts_hands.amin(1), verts_hands.amax(1), verts_object.amin(1), verts_object.amax(1)], 1).cpu().numpy()
    hand_first, hand_last = index_boxes(bounds[:, 0], bounds[:, 1], h)
    obj_first, obj_last = index_boxes(bounds[:, 2], bounds[:, 3], h)
    first = np.maximum(hand_first, obj_first)
    extent = np.minimum(hand_last, obj_last) - first + 1
    extent[(extent <= 0).any(1)] = 0                                        # the boxes do not meet: nothing to voxelise
    return (np.concatenate([first, extent], 1),
            (int(-(-extent[:, 0].max() // 32)), int(extent[:, 1].max()), int(extent[:, 2].max())))


def get_volume_metrics(verts_person, verts_object, faces_person, faces_object, voxel=0.005, max_bytes=256 << 20):
    """Intersection volume of hand(s) and object from solid voxelisations on one world-anchored lattice of pitch `voxel`
    (ObMan's physical-plausibility score), with the exact mesh volumes beside it.  Inputs as `get_inter_metrics`:
    verts_person (B*hand_nb, Vh, 3) frame-major, verts_object (B, Vo, 3), faces_person (hand_nb, Fh, 3) closed hand faces,
    faces_object (>=1, Fo, 3)  ->  {"inter_volumes", "hand_volumes", "obj_volumes"}: lists of B floats, m^3.

    inter_volume = popcount(hand & object) * h^3 (h = fp32(voxel), the cube in double) over the intersection of the two
    meshes' index boxes; each hand is voxelised separately and the hands are OR-ed.  Frames whose boxes do not meet score 0
    and are not voxelised.  hand_volumes: exact mesh volumes summed over the hands; obj_volumes: the object's.  The definitions
    are in include/homan_amd.h (csrc/solidvox.hip).  Frames are walked in chunks whose word arrays fit `max_bytes`; a
    frame's values do not depend on the chunking.  One read-back for the boxes, one for the results."""
    verts_person, verts_object = torch.as_tensor(verts_person), torch.as_tensor(verts_object)
    _check_clouds(verts_person=verts_person, verts_object=verts_object)
    h = ops.voxel_pitch(voxel)
    scenes = verts_object.shape[0]
    hands = verts_person.shape[0] // scenes
    if hands < 1 or hands > 3 or hands * scenes != verts_person.shape[0]:
        raise ValueError(f"{verts_person.shape[0]} hands for {scenes} frames")
    if int(max_bytes) < 1:
        raise ValueError(f"max_bytes must be positive, got {max_bytes}")
    faces_person = np.asarray(torch.as_tensor(faces_person).cpu())
    if faces_person.ndim == 2:
        faces_person = faces_person[None]
    hand_faces = [faces_person[k % faces_person.shape[0]] for k in range(hands)]
    obj_faces = np.asarray(torch.as_tensor(faces_object).cpu())
    obj_faces = obj_faces[0] if obj_faces.ndim == 3 else obj_faces
    person, obj = _on_gpu(verts_person, verts_object)
    with torch.cuda.device(obj.device):
        # hand k of every frame as its own contiguous batch (the voxeliser and the volume take one topology per call)
        per_hand = [person.reshape(scenes, hands, -1, 3)[:, k].contiguous() for k in range(hands)]
        boxes, dims = common_boxes(person.reshape(scenes, -1, 3), obj, h)
        extent = boxes[:, 3:]
        frame_bytes = 4 * dims[0] * dims[1] * dims[2] * (hands + 1)
        if frame_bytes > int(max_bytes):
            raise ValueError(f"one frame needs {frame_bytes} bytes of voxel words at a pitch of {h}; max_bytes is {max_bytes}")
        volumes = [ops.mesh_volume(v, f) for v, f in zip(per_hand, hand_faces)] + [ops.mesh_volume(obj, obj_faces)]
        counts = []
        if frame_bytes:
            chunk = max(int(max_bytes) // frame_bytes, 1)
            for f0 in range(0, scenes, chunk):
                sl = slice(f0, min(f0 + chunk, scenes))
                if not extent[sl].any():
                    counts.append(torch.zeros(sl.stop - sl.start, 3, dtype=torch.int64, device=obj.device))
                    continue
                hand_words = torch.empty(hands, sl.stop - sl.start, dims[2], dims[1], dims[0], dtype=torch.int32,
                                         device=obj.device)
                for k in range(hands):
                    ops.solid_voxels(per_hand[k][sl], hand_faces[k], h, boxes[sl], dims, out=hand_words[k])
                counts.append(ops.voxel_overlap(hand_words, ops.solid_voxels(obj[sl], obj_faces, h, boxes[sl], dims)))
            common = torch.cat(counts)[:, 0].cpu().numpy()
        else:
            common = np.zeros(scenes, np.int64)
        volumes = torch.stack(volumes).cpu().numpy()
    cell = (float(h) * float(h)) * float(h)
    hand_volumes = volumes[0].copy()
    for k in range(1, hands):
        hand_volumes = hand_volumes + volumes[k]
    return {"inter_volumes": (common.astype(np.float64) * cell).tolist(), "hand_volumes": hand_volumes.tolist(),
            "obj_volumes": volumes[hands].tolist()}
