"""Combined scene topology + per-face colours for the visualisation renders.

`get_faces_and_textures` has the call surface of reference homan/meshutils.py:7-51 (it is what `HOMan.__init__` calls to
build `model.faces` / `model.textures`, homan.py:199-219); the palette holds the colours of reference
homan/utils/nmr_renderer.py:7-23 (8-bit RGB triplets, "pink" excepted).

`mesh_topology` (a homan_amd extra, host-only NumPy: the topology is static) tells whether a face list is closed, which decides
the inside-outside rule of the surface metrics under sign="auto" (`resolve_sign`)."""
import numpy as np
import torch

_PALETTE_8BIT = {"blue": (166, 189, 219), "mint": (166, 229, 204), "mint2": (202, 229, 223), "green": (153, 216, 201),
                 "green2": (171, 221, 164), "red": (251, 128, 114), "orange": (253, 174, 97), "yellow": (210, 200, 124),
                 "white": (255, 255, 255), "gold": (240, 200, 0), "grey": (204, 204, 204)}
COLORS = {name: [c / 255.0 for c in rgb] for name, rgb in _PALETTE_8BIT.items()}
COLORS["pink"] = [0.9, 0.7, 0.7]


def _resolve_colours(n_meshes, color_names, colors_list):
    if colors_list is not None:
        return colors_list
    if len(color_names) != n_meshes:       # (color_names=None fails here with a TypeError, as in the reference)
        raise ValueError(f"Invalid number of colors {len(color_names)} for {n_meshes} verts")
    return [COLORS[name] for name in color_names]


def get_faces_and_textures(verts_list, faces_list, color_names=None, colors_list=None):
    """verts_list: [(B_k, V_k, 3)], faces_list: [(1 | B_k, f_k, 3)] -> (faces (1, F, 3) int64, textures (1, F, 1, 1, 1, 3)).
    Mesh k contributes B_k copies of its topology, copy i indexing vertices [offset_k + i * V_k, offset_k + (i + 1) * V_k)
    of the concatenated vertex array, in one flat colour."""
    colours = _resolve_colours(len(verts_list), color_names, colors_list)
    faces_out, tex_out, offset = [], [], 0
    for verts, faces, rgb in zip(verts_list, faces_list, colours):
        copies, nv = verts.shape[0], verts.shape[1]
        shift = offset + nv * torch.arange(copies, device=verts.device)
        topo = (faces.repeat(copies, 1, 1) + shift[:, None, None]).reshape(-1, 3).long()
        faces_out.append(topo)
        tex_out.append(torch.tensor(rgb, dtype=torch.float32, device=verts.device).expand(topo.shape[0], 1, 1, 1, 3))
        offset += nv * copies
    return torch.cat(faces_out)[None], torch.cat(tex_out)[None].contiguous()


def mesh_topology(faces):
    """faces (F,3) integers -> {"closed": every undirected edge is on exactly two faces, "oriented": every edge on two faces is
    run once in each direction, "boundary_edges": edges on one face, "nonmanifold_edges": edges on three or more faces}.  An
    edge whose two ends are one vertex (a face that repeats a vertex) is counted like any other."""
    faces = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.dtype.kind not in "iu":
        raise ValueError(f"faces: expected a non-empty integer (F, 3) array, got {faces.dtype} {faces.shape}")
    f = faces.astype(np.int64)
    tails, heads = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                 # the directed edges a->b, b->c, c->a of each face
    lo, hi = np.minimum(tails, heads), np.maximum(tails, heads)
    _, index, counts = np.unique(np.stack([lo, hi], 1), axis=0, return_inverse=True, return_counts=True)
    forward = np.bincount(index.reshape(-1), weights=(tails < heads), minlength=len(counts))
    paired = counts == 2
    return {"closed": bool((counts == 2).all()), "oriented": bool((forward[paired] == 1).all()),
            "boundary_edges": int((counts == 1).sum()), "nonmanifold_edges": int((counts > 2).sum())}


SIGN_MODES = ("parity", "winding", "auto")


def resolve_sign(sign, faces):
    """The inside-outside rule a `sign` argument asks for -> "parity" (the +x ray's crossings: closed meshes) or "winding" (the
    generalised winding number: open meshes too); "auto" is parity where `mesh_topology(faces)` is closed, else winding."""
    if sign not in SIGN_MODES:
        raise ValueError(f"sign {sign!r} not in [parity|winding|auto]")
    if sign != "auto":
        return sign
    return "parity" if mesh_topology(faces)["closed"] else "winding"
