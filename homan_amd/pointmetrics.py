"""Evaluation metrics of reference homan/eval/pointmetrics.py on the HIP kernels.

`get_point_metrics` (:17-44) and `get_align_metrics` (:61-99) - chamfer, ADD-S, vertex and hand-aligned errors, which the
reference computes with pytorch3d's `chamfer_distance` and scipy's `cKDTree` - run on an exact brute-force nearest-neighbour
search in both directions (`hm_cloud_metrics`, csrc/pointmetrics.hip) and the alignment statistics of `hm_align_stats`.
`get_inter_metrics` (:102-124, called by fit_vid_dataset.py:488-493) reads how deep the hand reaches into the object off
the object's signed-distance grid.  `get_volume_metrics` and `get_surface_metrics` are extras beyond the reference (DESIGN.md
section 7): the intersection volume on a solid voxeliser, and penetration depth / contact measured to the mesh surface on an
exact point-to-triangle distance.  Inputs are torch tensors on any device and of any float dtype; they are moved to the GPU
as contiguous fp32, and each call syncs with the host once.  There is no CPU path: without a GPU these functions raise.
"""
import numpy as np
import torch

from . import constants, lib, meshutils, ops


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


def surface_frame_bytes(hands, hand_verts, obj_verts, sign="parity"):
    """device bytes one frame of `get_surface_metrics` holds at a time: per hand and direction the three per-point outputs of
    `ops.point_mesh_distance` (d2, face, inside) and its merge words (8 + 4 bytes per point); with the winding-number sign
    (sign="winding", and "auto", which may choose it) the count and the flag of `ops.point_mesh_winding` on top (8 + 4)"""
    if sign not in meshutils.SIGN_MODES:
        raise ValueError(f"sign {sign!r} not in [parity|winding|auto]")
    return int(hands) * (int(hand_verts) + int(obj_verts)) * (24 if sign == "parity" else 36)


def _d2_at_most(dist):
    """the largest fp32 x with sqrt((double)x) <= dist (dist >= 0, finite): `d2 <= x` in fp32 is then exactly the comparison of
    the double distance with the threshold"""
    with np.errstate(over="ignore"):
        x = np.float32(float(dist) * float(dist))
    if not np.isfinite(x):
        x = np.float32(np.finfo(np.float32).max)
    while x > 0 and np.sqrt(np.float64(x)) > dist:
        x = np.nextafter(x, np.float32(-np.inf))
    while x < np.finfo(np.float32).max and np.sqrt(np.float64(np.nextafter(x, np.float32(np.inf)))) <= dist:
        x = np.nextafter(x, np.float32(np.inf))
    return float(x)


def get_surface_metrics(verts_person, verts_object, faces_person, faces_object, contact_thresh=0.005, per_vertex=False,
                        max_bytes=256 << 20):
    """Penetration depth and contact of hand(s) and object measured to the SURFACES (ObMan's definitions), from the exact
    point-to-triangle distances and the inside-outside sign of `ops.point_mesh_distance` (csrc/surfdist.hip; rules in
    include/homan_amd.h).  Inputs as `get_volume_metrics`: verts_person (B*hand_nb, Vh, 3) frame-major, verts_object (B, Vo, 3),
    faces_person (hand_nb, Fh, 3) closed hand faces, faces_object (>=1, Fo, 3).  Distances are sqrt((double)d2).  Lists of B:
      "pen_depth"      the largest distance to the object's surface over the hand vertices inside the object, 0.0 when none;
      "pen_depth_obj"  the same for the object's vertices inside a hand: each hand is queried as its own mesh (parity over
                       merged hands would cancel where they overlap) and the maximum over the hands is taken;
      "min_dist"       the smallest distance of a hand vertex to the object's surface;
      "contact_share"  the share of hand vertices with signed distance <= contact_thresh (inside counts), in double;
      "has_contact"    pen_depth > 0 or pen_depth_obj > 0 or min_dist <= contact_thresh.
    per_vertex adds "signed_dist" (B*hand_nb, Vh) float64, negative inside: the contact map.  Frames are walked in chunks whose
    outputs fit `max_bytes`; a frame's values do not depend on the chunking.  The sign is the ray parity, which needs closed
    meshes: `get_surface_metrics_signed` takes open ones.  No CPU path."""
    return get_surface_metrics_signed(verts_person, verts_object, faces_person, faces_object, contact_thresh, per_vertex,
                                      max_bytes, "parity")


def _inside(points, verts, faces, rule, searched):
    """the inside flags (bool) of one direction: the search's parity, or the winding number's |w| > 0.5"""
    if rule == "parity":
        return searched["inside"] == 1
    return ops._winding_run(points, verts, faces, None)[1] == 1


def get_surface_metrics_signed(verts_person, verts_object, faces_person, faces_object, contact_thresh=0.005, per_vertex=False,
                               max_bytes=256 << 20, sign="parity"):
    """`get_surface_metrics` with a choice of the inside-outside rule, in both directions; distances are the same search's.
    sign="parity": that function, its bits.  sign="winding": a point is inside a mesh iff its generalised winding number
    exceeds 0.5 in magnitude (`ops.point_mesh_winding`, csrc/winding.hip): meaningful for meshes with holes, missing caps or
    loose patches, and equal to parity on closed ones away from the surface.  sign="auto": per mesh, parity where
    `meshutils.mesh_topology` finds its faces closed, else winding.  Each hand stays its own query.  Any other string is a
    ValueError."""
    if sign not in meshutils.SIGN_MODES:
        raise ValueError(f"sign {sign!r} not in [parity|winding|auto]")
    verts_person, verts_object = torch.as_tensor(verts_person), torch.as_tensor(verts_object)
    _check_clouds(verts_person=verts_person, verts_object=verts_object)
    thresh = float(contact_thresh)
    if not (np.isfinite(thresh) and thresh >= 0):
        raise ValueError(f"contact_thresh must be finite and not negative, got {contact_thresh}")
    scenes = verts_object.shape[0]
    hands = verts_person.shape[0] // scenes
    if hands < 1 or hands > 3 or hands * scenes != verts_person.shape[0]:
        raise ValueError(f"{verts_person.shape[0]} hands for {scenes} frames")
    if int(max_bytes) < 1:
        raise ValueError(f"max_bytes must be positive, got {max_bytes}")
    faces_person = np.asarray(torch.as_tensor(faces_person).cpu())
    if faces_person.ndim == 2:
        faces_person = faces_person[None]
    obj_faces = np.asarray(torch.as_tensor(faces_object).cpu())
    obj_faces = obj_faces[0] if obj_faces.ndim == 3 else obj_faces
    Vh, Vo = verts_person.shape[1], verts_object.shape[1]
    frame_bytes = surface_frame_bytes(hands, Vh, Vo, sign)
    if frame_bytes > int(max_bytes):
        raise ValueError(f"one frame needs {frame_bytes} bytes of per-point outputs; max_bytes is {max_bytes}")
    person, obj = _on_gpu(verts_person, verts_object)
    dev = obj.device
    d2_contact = _d2_at_most(thresh)
    with torch.cuda.device(dev):
        hand_faces = [torch.from_numpy(np.ascontiguousarray(faces_person[k % faces_person.shape[0]], dtype=np.int32)).to(dev)
                      for k in range(hands)]
        object_faces = torch.from_numpy(np.ascontiguousarray(obj_faces, dtype=np.int32)).to(dev)
        object_rule = meshutils.resolve_sign(sign, obj_faces)
        hand_rules = [meshutils.resolve_sign(sign, faces_person[k % faces_person.shape[0]]) for k in range(hands)]
        per_hand = [person.reshape(scenes, hands, Vh, 3)[:, k].contiguous() for k in range(hands)]
        chunk = max(int(max_bytes) // frame_bytes, 1)
        rows, d2_maps, in_maps = [], [], []
        for f0 in range(0, scenes, chunk):
            sl = slice(f0, min(f0 + chunk, scenes))
            n = sl.stop - sl.start
            deep = torch.zeros(n, device=dev)                         # largest d2 of a hand vertex inside the object
            deep_obj = torch.zeros(n, device=dev)
            near = torch.full((n,), float("inf"), device=dev)         # smallest d2 of a hand vertex
            touching = torch.zeros(n, dtype=torch.int64, device=dev)
            chunk_d2, chunk_in = [], []
            for k in range(hands):
                to_obj = ops.point_mesh_distance(per_hand[k][sl], obj[sl], object_faces)
                inside = _inside(per_hand[k][sl], obj[sl], object_faces, object_rule, to_obj)
                deep = torch.maximum(deep, torch.where(inside, to_obj["d2"], torch.zeros_like(to_obj["d2"])).amax(1))
                near = torch.minimum(near, to_obj["d2"].amin(1))
                touching += (inside | (to_obj["d2"] <= d2_contact)).sum(1)
                chunk_d2.append(to_obj["d2"])
                chunk_in.append(inside)
                to_hand = ops.point_mesh_distance(obj[sl], per_hand[k][sl], hand_faces[k])
                in_hand = _inside(obj[sl], per_hand[k][sl], hand_faces[k], hand_rules[k], to_hand)
                deep_obj = torch.maximum(deep_obj, torch.where(in_hand, to_hand["d2"], torch.zeros_like(to_hand["d2"])).amax(1))
            rows.append(torch.stack([deep.double(), deep_obj.double(), near.double(), touching.double()]))
            if per_vertex:                                            # (frames, hands, Vh): frame-major, as verts_person
                d2_maps.append(torch.stack(chunk_d2, 1))
                in_maps.append(torch.stack(chunk_in, 1))
        table = torch.cat(rows, 1).cpu().numpy()                      # (exact: maxima and minima of fp32 values, counts)
        if per_vertex:
            d2_maps, in_maps = torch.cat(d2_maps).cpu().numpy(), torch.cat(in_maps).cpu().numpy()
    pen, pen_obj, min_dist = (np.sqrt(table[k]) for k in range(3))
    share = table[3] / np.float64(hands * Vh)
    res = {"pen_depth": pen.tolist(), "pen_depth_obj": pen_obj.tolist(), "min_dist": min_dist.tolist(),
           "contact_share": share.tolist(),
           "has_contact": ((pen > 0) | (pen_obj > 0) | (min_dist <= thresh)).tolist()}
    if per_vertex:
        dist = np.sqrt(d2_maps.astype(np.float64))
        res["signed_dist"] = np.where(in_maps, -dist, dist).reshape(scenes * hands, Vh)
    return res

