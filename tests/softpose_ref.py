"""Dense PyTorch restatement of the pose initialisation's soft mode (homan_amd/pose_optimization.py, sil_mode="soft"; the
semantics are spelt out in PoseOptimizer's docstring and include/homan_amd.h, hm_softsil_pose_terms), dtype-generic like
tests/softsil_ref.py, which supplies the image: rigid transform of the candidates, soft image at the mask's size, masked L2,
IoU, off-screen penalty, and the free-running fit with torch Adam.  Plus the one scene the GPU tests and the CPU check share."""
import functools
import math

import numpy as np
import torch

from tests import softsil_ref

FAR = softsil_ref.FAR
RULE_FACTOR, VALUE_ABS = softsil_ref.RULE_FACTOR, softsil_ref.IMAGE_ABS          # the same 4 x rule
IOU_REL = 3e-7                  # the IoU off exact sums: one add and one divide in float32


def rot6d_to_matrix(r6):
    """(n,3,2) -> (n,3,3), Gram-Schmidt, columns b1 b2 b3 (csrc/hm_common.h rot6d_to_mat)"""
    a1, a2 = r6[:, :, 0], r6[:, :, 1]
    b1 = a1 / a1.norm(dim=1, keepdim=True)
    u = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    b2 = u / u.norm(dim=1, keepdim=True)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=1)), dim=-1)


def offscreen(verts, K):
    """100000 x the hinge on the six clipping planes (PoseOptimizer.compute_offscreen_loss), K (3,3)"""
    x, y, z = verts[..., 0], verts[..., 1], verts[..., 2]
    xn, yn = x / (z + 1e-9), y / (z + 1e-9)
    u = K[0, 0] * xn + K[0, 1] * yn + K[0, 2]
    v = 1.0 - (K[1, 0] * xn + K[1, 1] * yn + K[1, 2])
    ndc = torch.stack([2 * (u - 0.5), 2 * (v - 0.5)], -1)
    relu = torch.relu
    return 100000 * (relu(ndc - 1).sum((1, 2)) + relu(-1 - ndc).sum((1, 2)) + relu(-z).sum(1) + relu(z - FAR).sum(1))


def masked_terms(alpha, mask):
    """alpha (n,S,S), mask (S,S) in {-1,0,1} -> (image, mask loss (n,), IoU (n,))"""
    keep, ref = (mask >= 0).to(alpha.dtype), (mask > 0).to(alpha.dtype)
    image = keep * alpha
    loss = ((image - ref) ** 2).sum((1, 2))
    iou = (image * ref).sum((1, 2)) / ((image + ref).clamp(0, 1).sum((1, 2)) + 1e-6)
    return image, loss, iou


def forward(rot6d, trans, mesh, faces, K, mask, sigma):
    """rot6d (n,3,2), trans (n,1,3), mesh (V,3), K (3,3), in ONE dtype; sigma a Python float -> dict of the module's outputs"""
    verts = mesh[None] @ rot6d_to_matrix(rot6d) + trans
    n, S = rot6d.shape[0], mask.shape[0]
    alpha = softsil_ref.soft_silhouette(verts, faces, K[None].expand(n, 3, 3), S, sigma)
    image, loss, iou = masked_terms(alpha, mask)
    off = offscreen(verts, K)
    return dict(image=image, mask=loss, iou=iou, offscreen=off, total=loss + off)


def forward_and_grads(rot6d, trans, mesh, faces, K, mask, sigma, dtype):
    """the same float32 inputs evaluated in `dtype` -> (outputs, d sum(total) / d rot6d, d sum(total) / d trans)"""
    r = rot6d.detach().to(dtype).clone().requires_grad_(True)
    t = trans.detach().to(dtype).clone().requires_grad_(True)
    out = forward(r, t, mesh.to(dtype), faces, K.to(dtype), mask, sigma)
    out["total"].sum().backward()
    return {k: v.detach() for k, v in out.items()}, r.grad, t.grad


def anneal_sequence(sigma, decay, floor, steps):
    """the float32 blur schedule: sigma <- max(sigma * decay, floor), one multiply and one max per step -> the `steps + 1` values"""
    s, d, f = np.float32(sigma), np.float32(decay), np.float32(floor or 0.0)
    seq = [s]
    for _ in range(steps):
        s = np.maximum(np.float32(s * d), f)
        seq.append(s)
    return seq


def fit(rot6d, trans, mesh, faces, K, mask, sigma, steps, lr, dtype, decay=1.0, floor=None):
    """`steps` free-running steps with torch Adam in `dtype` -> (final rot6d, final trans, per-step losses (steps, n))"""
    r = rot6d.detach().to(dtype).clone().requires_grad_(True)
    t = trans.detach().to(dtype).clone().requires_grad_(True)
    mesh, K = mesh.to(dtype), K.to(dtype)
    opt = torch.optim.Adam([r, t], lr=lr)
    sigmas = anneal_sequence(sigma, decay, floor, steps)
    losses = []
    for step in range(steps):
        opt.zero_grad()
        total = forward(r, t, mesh, faces, K, mask, float(sigmas[step]))["total"]
        total.sum().backward()
        opt.step()
        losses.append(total.detach().clone())
    return r.detach(), t.detach(), torch.stack(losses)


def axis_angle(axis, degrees):
    """float64 rotation matrix (Rodrigues)"""
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    th = math.radians(degrees)
    Kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


@functools.lru_cache(maxsize=None)
def scene(S):
    """The cube scene: mesh, K, the target's mask (the restatement's image of the target pose at sigma 1e-6, thresholded at 0.5,
    the left S // 8 columns occluded) and four candidates around the target; float32 tensors, as the module gets them."""
    from homan_amd import synth
    from homan_amd.homan import matrix_to_rot6d
    v, f = synth.box_mesh(1, 1, 1, scale=0.2)
    mesh, faces = torch.from_numpy(np.asarray(v)).float(), torch.from_numpy(np.asarray(f).astype(np.int64))
    K = torch.tensor([[1.2, 0.0, 0.5], [0.0, 1.2, 0.5], [0.0, 0.0, 1.0]])
    R_t = axis_angle((1.0, 2.0, 3.0), 35.0)
    t_t = torch.tensor([0.02, -0.01, 0.6], dtype=torch.float64)
    target = mesh.double()[None] @ R_t[None] + t_t
    alpha = softsil_ref.soft_silhouette(target, faces, K.double()[None], S, 1e-6)[0]
    mask = (alpha > 0.5).float()
    mask[:, : S // 8] = -1
    spins = [((1.0, 0.0, 0.0), 20.0), ((0.0, 1.0, 0.0), -25.0), ((0.0, 0.0, 1.0), 30.0), ((1.0, 1.0, 0.0), 15.0)]
    shifts = torch.tensor([[0.03, 0.02, 0.05], [-0.03, 0.0, -0.04], [0.0, 0.03, 0.02], [0.02, -0.02, 0.0]], dtype=torch.float64)
    rots = torch.stack([axis_angle(ax, deg) @ R_t for ax, deg in spins]).float()
    rot6d = matrix_to_rot6d(rots).contiguous()
    trans = (t_t[None] + shifts).float()[:, None, :].contiguous()
    return dict(mesh=mesh, faces=faces, K=K, mask=mask, rot6d=rot6d, trans=trans, rots=rots, S=S)
