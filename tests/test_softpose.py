"""Host side of the pose initialisation's soft silhouette mode (no GPU): the C ABI of csrc/softpose.hip, the public keywords and
their validation, the resident-fitter key, and the float64 restatement (tests/softpose_ref.py) the GPU tests compare with,
pinned against central differences."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import softpose_ref as ref

SOFT_DEFAULTS = [("sil_mode", "nmr"), ("sil_sigma", 1e-4), ("sil_sigma_decay", 1.0), ("sil_sigma_min", None)]


def test_entry_points_are_declared_and_exported():
    from homan_amd import build, lib
    VP, I, F, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    with open(build.HEADER) as fh:
        header = fh.read()
    for name in ("hm_softsil_pose_workspace_bytes", "hm_softsil_pose_terms", "hm_sigma_anneal"):
        assert name + "(" in header and name in lib.exported_symbols()
    assert lib._SIGNATURES["hm_softsil_pose_workspace_bytes"] == (SZ, [I, I])
    assert lib._SIGNATURES["hm_softsil_pose_terms"] == (I, [VP, VP, VP, I, I, VP, VP, VP, VP])
    assert lib._SIGNATURES["hm_sigma_anneal"] == (I, [VP, F, F, VP])
    handle = lib.lib()                       # (raises if the built library lacks one of them)
    for good in ((1, 1), (70, 64), (3, 4096)):
        assert handle.hm_softsil_pose_workspace_bytes(*good) > 0, good
    for bad in ((0, 8), (2, 0), (2, 4097), (65536, 8)):
        assert handle.hm_softsil_pose_workspace_bytes(*bad) == 0, bad


def test_public_entry_points_take_the_soft_keywords():
    from homan_amd import pose_optimization as po
    for fn in (po.PoseOptimizer.__init__, po.PoseFitter.__init__, po._resident_fitter, po.find_optimal_pose, po.find_optimal_poses):
        params = inspect.signature(fn).parameters
        assert [(k, params[k].default) for k, _ in SOFT_DEFAULTS] == SOFT_DEFAULTS, fn.__qualname__


def _module(**kw):
    from homan_amd.pose_optimization import PoseOptimizer
    return PoseOptimizer(ref_image=np.zeros((4, 4)), vertices=torch.zeros(3, 3), faces=torch.tensor([[0, 1, 2]]),
                         rotation_init=torch.eye(3)[None, :, :2], translation_init=torch.zeros(1, 1, 3), **kw)


@pytest.mark.parametrize("kw", [dict(sil_mode="hard"), dict(sil_mode=None), dict(sil_mode="soft", sil_sigma=0.0),
                                dict(sil_mode="soft", sil_sigma=-1e-4), dict(sil_mode="soft", sil_sigma=float("inf")),
                                dict(sil_mode="soft", sil_sigma=float("nan")), dict(sil_mode="soft", sil_sigma="1e-4"),
                                dict(sil_mode="soft", sil_sigma_decay=0.0), dict(sil_mode="soft", sil_sigma_decay=1.01),
                                dict(sil_mode="soft", sil_sigma_decay=float("nan")),
                                dict(sil_mode="soft", sil_sigma=1e-3, sil_sigma_min=0.0),
                                dict(sil_mode="soft", sil_sigma=1e-3, sil_sigma_min=2e-3),
                                dict(sil_mode="soft", sil_sigma=1e-3, sil_sigma_min=float("nan")),
                                dict(sil_mode="nmr", sil_sigma_decay=2.0)], ids=str)
def test_bad_options_are_refused_before_any_device_work(kw):
    """ValueError on a machine without a GPU: the check precedes the "needs an MI355X" RuntimeError"""
    with pytest.raises(ValueError):
        _module(**kw)


def test_soft_mode_has_no_edge_chamfer_term():
    with pytest.raises(NotImplementedError):
        _module(sil_mode="soft", lw_chamfer=0.5)
    from homan_amd import pose_optimization as po
    with pytest.raises(NotImplementedError):
        po.find_optimal_pose(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]), np.zeros((4, 4)), [0, 0, 4, 4], [0, 0, 4, 4], (8, 8),
                             K=torch.eye(3), sil_mode="soft", lw_chamfer=0.5)
    with pytest.raises(ValueError):
        po.find_optimal_poses((8, 8), faces=torch.tensor([[0, 1, 2]]), vertices=torch.zeros(3, 3), annotations=[], Ks=[],
                              sil_mode="soft", sil_sigma_decay=0.0)


def test_resident_fitter_key_tells_the_modes_apart(monkeypatch):
    """a soft fit must not replay a graph captured for the hard rasteriser, nor one captured for another blur schedule"""
    from homan_amd import pose_optimization as po
    built = []

    class Recorder:
        def __init__(self, *args):
            built.append(args[2:])

    monkeypatch.setattr(po, "PoseFitter", Recorder)
    monkeypatch.setenv("HOMAN_POSE_FITTERS_MAX", "8")
    monkeypatch.setattr(po, "_FITTERS", type(po._FITTERS)())
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    hard = po._resident_fitter(v, f, 6, 64, 1e-2)
    assert po._resident_fitter(v, f, 6, 64, 1e-2, sil_mode="nmr", sil_sigma=5e-4) is hard        # (unused in mode "nmr")
    soft = po._resident_fitter(v, f, 6, 64, 1e-2, sil_mode="soft")
    others = [po._resident_fitter(v, f, 6, 64, 1e-2, sil_mode="soft", **kw)
              for kw in (dict(sil_sigma=1e-3), dict(sil_sigma_decay=0.9), dict(sil_sigma_decay=0.9, sil_sigma_min=5e-5))]
    assert len({id(x) for x in [hard, soft] + others}) == 5 and len(built) == 5
    assert built[0] == (6, 64, 1e-2, 0, 7, 0.25)
    assert built[1] == (6, 64, 1e-2, 0, 7, 0.25, "soft", 1e-4, 1.0, None)
    assert po._resident_fitter(v, f, 6, 64, 1e-2, sil_mode="soft") is soft
    assert po._resident_fitter(v, f, 6, 37, 1e-2, sil_mode="soft") is not soft


def test_restatement_against_central_differences():
    """The float64 restatement (soft image of tests/softsil_ref.py + masked L2 + off-screen penalty) at S = 8, one cube: autograd
    against central differences in all nine pose coordinates, the stated image gradient 2 keep (keep alpha - ref), the IoU
    formula, and the float32 blur schedule."""
    sc = ref.scene(8)
    sigma = float(np.float32(4e-3))
    r0, t0 = sc["rot6d"][:1], sc["trans"][:1]
    out, g_r, g_t = ref.forward_and_grads(r0, t0, sc["mesh"], sc["faces"], sc["K"], sc["mask"], sigma, torch.float64)
    assert float(out["mask"]) > 0 and float(out["offscreen"]) == 0 and float(g_t[..., 2].abs().max()) > 0
    x0 = torch.cat([r0.double().reshape(-1), t0.double().reshape(-1)])
    analytic = torch.cat([g_r.reshape(-1), g_t.reshape(-1)])

    def total(x):
        return float(ref.forward(x[:6].reshape(1, 3, 2), x[6:].reshape(1, 1, 3), sc["mesh"].double(), sc["faces"], sc["K"].double(),
                                 sc["mask"], sigma)["total"].sum())

    h = 1e-6
    numeric = torch.tensor([(total(x0 + h * e) - total(x0 - h * e)) / (2 * h) for e in torch.eye(9, dtype=torch.float64)])
    err = float((numeric - analytic).abs().max() / analytic.abs().max())
    print("central differences vs autograd, relative to the largest entry", err, analytic.tolist())
    assert err < 1e-6
    # d mask / d alpha and the IoU, on the image itself
    alpha = (out["image"] + 0.25 * (sc["mask"] < 0)).clone().requires_grad_(True)         # (something under the occluded band)
    image, loss, iou = ref.masked_terms(alpha, sc["mask"])
    loss.sum().backward()
    keep, tgt = (sc["mask"] >= 0).double(), (sc["mask"] > 0).double()
    assert torch.equal(alpha.grad, 2 * keep * (keep * alpha.detach() - tgt))
    assert float(alpha.grad[:, :, 0].abs().max()) == 0 and float(image.detach()[:, :, 0].abs().max()) == 0
    want = float((image.detach() * tgt).sum() / (torch.maximum(image.detach(), tgt).sum() + 1e-6))           # (clamp(a + b, 0, 1) = max for 0 / 1 ref)
    assert abs(float(iou.detach()) - want) < 1e-12 * max(want, 1)
    # off-screen: pushed half out of the image the hinge and its gradient join
    t_off = t0.clone()
    t_off[..., 0] += 0.25
    out_off, _, g_off = ref.forward_and_grads(r0, t_off, sc["mesh"], sc["faces"], sc["K"], sc["mask"], sigma, torch.float64)
    assert float(out_off["offscreen"]) > 0 and float(g_off[..., 0].abs().max()) > 1e4
    seq = ref.anneal_sequence(1e-3, 0.9, 3e-4, 20)
    assert seq[0] == np.float32(1e-3) and seq[1] == np.float32(np.float32(1e-3) * np.float32(0.9)) and seq[-1] == np.float32(3e-4)
    assert all(s.dtype == np.float32 for s in seq) and ref.anneal_sequence(1e-3, 1.0, None, 3)[-1] == np.float32(1e-3)
