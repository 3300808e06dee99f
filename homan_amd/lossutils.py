"""3-D space losses with the reference's function surface (reference homan/lossutils.py), on HIP kernels."""
import torch

from . import constants, ops


def compute_smooth_loss(verts_hand, verts_obj, rws):
    """reference lossutils.py:18-36."""
    hand_nb = verts_hand.shape[0] // verts_obj.shape[0]
    return {"loss_smooth_obj": ops.smooth_loss(verts_obj, 1, rws),
            "loss_smooth_hand": ops.smooth_loss(verts_hand, hand_nb, rws)}


def compute_collision_loss(verts_hand, verts_object, cctx):
    """reference lossutils.py:43-64 (collision_mode='sdf').  `cctx`: one CollisionContext (one hand), or the three of the
    two-hand scene [hand 0, hand 1, object] - (hand 0, hand 1), (hand 0, object), (hand 1, object) - whose two-mesh
    losses add up to the reference's sum over the six ordered pairs of meshes (scenesdf.py:131-146)."""
    if not isinstance(cctx, (tuple, list)):
        return {"loss_collision": ops.collision_loss(verts_hand, verts_object, cctx, constants.SDF_SCALE_FACTOR)}
    h0, h1 = verts_hand[0::2].contiguous(), verts_hand[1::2].contiguous()          # stride 2, lossutils.py:57-59
    loss = ops.collision_loss(h0, h1, cctx[0], constants.SDF_SCALE_FACTOR)
    loss = loss + ops.collision_loss(h0, verts_object, cctx[1], constants.SDF_SCALE_FACTOR)
    loss = loss + ops.collision_loss(h1, verts_object, cctx[2], constants.SDF_SCALE_FACTOR)
    return {"loss_collision": loss}


def compute_contact_loss(verts_hand_b, verts_object_b, rws, nn=None):
    """reference lossutils.py:112-130 -> interactions/contactloss.py:149-309 (as executed: SURVEY appendix B.1).  Several
    hands (:116-127): the per-hand terms (hand i = rows i::hand_nb) averaged.  -> ({loss}, nearest-vertex search of the
    hand(s): one tuple, or a list of one per hand)."""
    hand_nb = verts_hand_b.shape[0] // verts_object_b.shape[0]
    if hand_nb == 1:
        if nn is None:
            nn = ops.nearest_vertices(verts_hand_b, verts_object_b, rws)
        return {"loss_contact": ops.contact_loss(verts_hand_b, verts_object_b, nn[0], rws, constants.COLLISION_THRESH)}, nn
    nns, terms = [], []
    for i in range(hand_nb):
        vh = verts_hand_b[i::hand_nb].contiguous()
        nns.append(ops.nearest_vertices(vh, verts_object_b, rws) if nn is None else nn[i])
        terms.append(ops.contact_loss(vh, verts_object_b, nns[-1][0], rws, constants.COLLISION_THRESH))
    return {"loss_contact": torch.stack([t.reshape(()) for t in terms]).mean()}, nns      # 0-d, like the reference's (:126-127)


SURFACE_TIPS = (745, 317, 444, 556, 673)          # finger-tip vertices, reference interactions/contactloss.py:259


def surface_contact_contexts(batch, hand_nb, closed_faces_hand, faces_object, num_verts_object, device, two_way=False,
                             contact_zones="all"):
    """The state of `compute_surface_contact_loss` for a model: per hand one context hand -> object and, with two_way, one
    object -> hand (the hand's CLOSED mesh, so that inside means inside); the attraction weights of `contact_zones`."""
    if contact_zones not in ("all", "tips"):
        raise ValueError(f"contact_zones {contact_zones} not in [all|tips]")
    weights = None
    if contact_zones == "tips":
        weights = torch.zeros(778, device=device)
        weights[list(SURFACE_TIPS)] = 1.0
    return {"hand": [ops.SurfaceContactContext(batch, 778, num_verts_object, faces_object, device) for _ in range(hand_nb)],
            "object": [ops.SurfaceContactContext(batch, num_verts_object, 778, closed_faces_hand, device)
                       for _ in range(hand_nb)] if two_way else None,
            "weights": weights}


def compute_surface_contact_loss(verts_hand, verts_object, ctxs, contact_thresh=constants.CONTACT_THRESH,
                                 collision_thresh=constants.COLLISION_THRESH):
    """Surface contact loss (a homan_amd extra; ops.surface_contact_loss).  verts_hand (B * hand_nb, 778,
    3) frame-major, verts_object (B, Vo, 3), ctxs from `surface_contact_contexts` -> ({"loss_surf_attr", "loss_surf_rep"},
    {"surf_inside_share"}).  Each hand (rows i::hand_nb) is one call against the object: attraction of its vertices outside
    the object - all of them, or the five finger tips with contact_zones="tips" -, repulsion of those inside; the per-hand
    terms are averaged, as the contact term's are.  two_way: the object's vertices against each hand's closed mesh, of which
    only the repulsion is added.  surf_inside_share: the share of hand vertices inside the object (a 0-d device tensor)."""
    hand_nb = len(ctxs["hand"])
    attr, rep, inside = [], [], []
    for i in range(hand_nb):
        vh = verts_hand if hand_nb == 1 else verts_hand[i::hand_nb].contiguous()
        a, r = ops.surface_contact_loss(vh, verts_object, ctxs["hand"][i], weights=ctxs["weights"],
                                        contact_thresh=contact_thresh, collision_thresh=collision_thresh, weight_max=1.0)
        inside.append(ctxs["hand"][i].inside.float().mean())
        if ctxs["object"] is not None:
            _, back = ops.surface_contact_loss(verts_object, vh, ctxs["object"][i], contact_thresh=contact_thresh,
                                               collision_thresh=collision_thresh)
            r = r + back
        attr.append(a)
        rep.append(r)
    mean = lambda terms: terms[0] if hand_nb == 1 else torch.stack(terms).mean()  # noqa: E731
    return {"loss_surf_attr": mean(attr), "loss_surf_rep": mean(rep)}, {"surf_inside_share": mean(inside)}
