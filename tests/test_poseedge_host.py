"""Host-side logic of the edge-chamfer term in the fused pose initialisation (no GPU): the public keywords, the resident-fitter
key, the grid of the order-independent sums, the new C-ABI prototypes."""
import ctypes
import inspect


def test_public_entry_points_take_the_edge_term_keywords():
    from homan_amd import pose_optimization as po
    for fn in (po.find_optimal_pose, po.find_optimal_poses, po._resident_fitter):
        params = inspect.signature(fn).parameters
        assert [params[k].default for k in ("lw_chamfer", "kernel_size", "power")] == [0, 7, 0.25], fn.__name__
    params = inspect.signature(po.PoseFitter.__init__).parameters
    assert [params[k].default for k in ("lw_chamfer", "kernel_size", "power")] == [0, 7, 0.25]


def test_resident_fitter_key_tells_the_edge_term_settings_apart(monkeypatch):
    """One resident fitter per (mesh, candidates, size, lr, lw_chamfer, kernel_size, power): a fit with another weight or window
    must not replay a graph captured for this one."""
    import torch
    from homan_amd import pose_optimization as po
    built = []

    class Recorder:
        def __init__(self, *args):
            built.append(args[2:])

    monkeypatch.setattr(po, "PoseFitter", Recorder)
    monkeypatch.setenv("HOMAN_POSE_FITTERS_MAX", "8")
    monkeypatch.setattr(po, "_FITTERS", type(po._FITTERS)())
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    a = po._resident_fitter(v, f, 6, 64, 1e-2)
    assert po._resident_fitter(v, f, 6, 64, 1e-2, None, 0, 7, 0.25) is a                   # the defaults ARE weight 0
    others = [po._resident_fitter(v, f, 6, 64, 1e-2, None, *kw) for kw in ((0.5, 7, 0.25), (0.5, 5, 0.25), (0.5, 7, 0.5))]
    assert len({id(x) for x in [a] + others}) == 4 and len(built) == 4
    assert built[1] == (6, 64, 1e-2, 0.5, 7, 0.25)
    assert po._resident_fitter(v, f, 6, 64, 1e-2, None, 0.5, 5, 0.25) is others[1]


def test_sum_grid_of_the_edge_term_keeps_the_headroom_of_the_plain_loop():
    """_edge_sum_log2q: the grid grows with the largest per-sample gradient, 2 -> 2 + lw k^2 (2 size^2)^power, by whole powers of
    two; it stays a valid argument (-60 .. -1; 0 would select the library's default 2^-44)."""
    import math
    from homan_amd.pose_optimization import _edge_sum_log2q
    assert _edge_sum_log2q(0.5, 256, 7, 0.25) == -16
    assert _edge_sum_log2q(0.0, 256, 7, 0.25) == -24
    for lw, size, k, power in ((0.5, 64, 3, 0.25), (2.0, 1024, 7, 0.25), (1e-3, 256, 7, 0.25), (0.5, 256, 7, 0.5), (1e9, 1024, 7, 1.0)):
        q = _edge_sum_log2q(lw, size, k, power)
        ratio = (2.0 + lw * k * k * (2.0 * size * size) ** power) / 2.0
        assert -60 <= q <= -1
        if q < -1:
            assert 2.0 ** (q + 24) >= ratio > 2.0 ** (q + 23) or ratio == 1.0          # the next power of two at or above the ratio
        assert math.isfinite(q)
    # the range check of the issue at the default setting: the largest single pseudo-gradient term, lw * 49 * max edt / eps
    largest_term = 0.5 * 49 * (2.0 * 256 * 256) ** 0.25 / 1e-3
    assert largest_term < 2.0 ** (53 - 24) and 2.0 ** (53 - 16) / largest_term > 1e5


def test_edge_term_prototypes():
    from homan_amd import lib
    VP, I, F, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert lib._SIGNATURES["hm_edge_edt"] == (I, [VP, I, I, I, F, VP, VP, VP])
    assert lib._SIGNATURES["hm_pose_edge_terms"] == (I, [VP, VP, VP, VP, I, I, I, I, F, VP, VP, VP, VP])
    assert lib._SIGNATURES["hm_pose_edge_workspace_bytes"] == (SZ, [I, I])
    handle = lib.lib()
    tiles = (256 // 64) * (256 // 32)
    assert handle.hm_pose_edge_workspace_bytes(500, 256) == 500 * 4 + 500 * tiles * 16
    assert handle.hm_pose_edge_workspace_bytes(0, 256) == 0
