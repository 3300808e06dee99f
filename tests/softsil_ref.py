"""Dense PyTorch restatement of the soft silhouette semantics (include/homan_amd.h, hm_softsil_fwd; Liu et al. 2019, silhouette
branch).  dtype-generic: every tensor takes the dtype of `verts`, the gradient comes from autograd.  Works on (B, F, S*S)
tensors, so it is for small shapes only."""
import torch

from oracle import nmr as o_nmr

NEAR, FAR, CUT, MIN_AREA2 = o_nmr.DEFAULT_NEAR, o_nmr.DEFAULT_FAR, 16.0, 1e-10


RULE_FACTOR, IMAGE_ABS = 4, 1e-6          # the kernel may be this many times as far from float64 as the float32 restatement (+ abs, images)


def pixel_centres(S, dtype):
    """(S*S, 2) NDC centres, row-major: pixel (r, c) at x = (2c + 1 - S) / S, y = (S - 1 - 2r) / S"""
    i = torch.arange(S, dtype=dtype)
    x, y = (2 * i + 1 - S) / S, (S - 1 - 2 * i) / S
    return torch.stack([x[None, :].expand(S, S), y[:, None].expand(S, S)], -1).reshape(S * S, 2)


def soft_silhouette(verts, faces, K, S, sigma, orig_size=1.0):
    """verts (B,V,3), faces (F,3) integer, K (B,3,3), sigma a Python float -> alpha (B,S,S) in the dtype of verts"""
    dt = verts.dtype
    K = K.to(dt)
    ndc = o_nmr.projection(verts, K, torch.eye(3, dtype=dt)[None], torch.zeros(1, 3, dtype=dt), torch.zeros(1, 5, dtype=dt),
                           orig_size)
    tri = ndc[:, faces.long()]                                  # (B,F,3,3)
    xy, z = tri[..., :2], tri[..., 2]
    area2 = ((xy[:, :, 1, 0] - xy[:, :, 0, 0]) * (xy[:, :, 2, 1] - xy[:, :, 0, 1])
             - (xy[:, :, 2, 0] - xy[:, :, 0, 0]) * (xy[:, :, 1, 1] - xy[:, :, 0, 1]))
    valid = ((z > NEAR) & (z < FAR)).all(-1) & (area2.abs() >= MIN_AREA2)
    # faces that take no part are computed on a stand-in triangle (no 0 / 0 reaches autograd) and masked out below
    xy = torch.where(valid[:, :, None, None], xy, torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], dtype=dt))
    P = pixel_centres(S, dt)[None, None]                         # (1,1,S*S,2)
    d2, pos, neg = None, True, True
    for e in range(3):
        a, b = xy[:, :, e, None, :], xy[:, :, (e + 1) % 3, None, :]
        ab, ap = b - a, P - a
        t = ((ap * ab).sum(-1) / (ab * ab).sum(-1)).clamp(0, 1)
        q = ap - t[..., None] * ab
        d2_e = (q * q).sum(-1)                                   # (B,F,S*S)
        d2 = d2_e if d2 is None else torch.minimum(d2, d2_e)
        cross = ab[..., 0] * ap[..., 1] - ab[..., 1] * ap[..., 0]
        pos, neg = pos & (cross >= 0), neg & (cross <= 0)
    inside = pos | neg                                           # the closed triangle, either winding
    x = torch.where(inside, d2, -d2) / sigma
    keep = valid[:, :, None] & (inside | (d2 < CUT * sigma))     # outside pairs at or beyond the cutoff are dropped exactly
    one_minus_d = torch.where(keep, torch.sigmoid(-x), torch.ones((), dtype=dt))
    return (1 - one_minus_d.prod(1)).reshape(verts.shape[0], S, S)


def alpha_and_grad(verts, faces, K, S, sigma, upstream, dtype, orig_size=1.0):
    """-> (alpha (B,S,S), d sum(upstream * alpha) / d verts (B,V,3)), both computed in `dtype` from the SAME input values"""
    v = verts.detach().to(dtype).clone().requires_grad_(True)
    alpha = soft_silhouette(v, faces, K.detach().to(dtype), S, sigma, orig_size)
    (alpha * upstream.to(dtype)).sum().backward()
    return alpha.detach(), v.grad.detach()
