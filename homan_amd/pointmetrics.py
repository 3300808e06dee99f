"""Evaluation metrics of reference homan/eval/pointmetrics.py on the HIP kernels.

`get_point_metrics` (:17-44) and `get_align_metrics` (:61-99) - chamfer, ADD-S, vertex and hand-aligned errors, which the
reference computes with pytorch3d's `chamfer_distance` and scipy's `cKDTree` - run on an exact brute-force nearest-neighbour
search in both directions (`hm_cloud_metrics`, csrc/pointmetrics.hip) and the alignment statistics of `hm_align_stats`.
`get_inter_metrics` (:102-124, called by fit_vid_dataset.py:488-493) reads how deep the hand reaches into the object off
the object's signed-distance grid.  Inputs are torch tensors on any device and of any float dtype; they are moved to the GPU
as contiguous fp32, and each call syncs with the host once.  There is no CPU path: without a GPU these functions raise.
"""
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
