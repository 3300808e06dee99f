"""Soft silhouette mode, CPU side: known answers and the finite-difference gradient of the float64 restatement
(tests/softsil_ref.py) the GPU tests compare the kernels with, the C ABI of the three hm_softsil_* entry points, and the
opt-in keywords of the Python layers."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import softsil_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
K_UNIT = torch.tensor([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]], dtype=torch.float64)


def from_ndc(uv, z=1.0):
    """camera-space vertices (1,V,3) that K_UNIT (orig_size 1) projects to the NDC points `uv`: u = 2 x / z, v = -2 y / z
    (exact wherever x = 0 or y = 0; elsewhere up to the projection's 1e-9 in the denominator).  z: one depth, or one per vertex"""
    uv = torch.as_tensor(uv, dtype=torch.float64)
    z = torch.as_tensor(z, dtype=torch.float64).expand(uv.shape[0])
    return torch.stack([uv[:, 0] * z / 2, -uv[:, 1] * z / 2, z], -1)[None]


def render(uv, faces, S, sigma, z=1.0):
    return ref.soft_silhouette(from_ndc(uv, z), torch.as_tensor(faces), K_UNIT, S, sigma)[0]


def test_full_screen_quad_is_opaque():
    # the shared diagonal (10,-2)-(-2,10) passes 4 NDC units from the image: every pixel is interior to one of the two faces
    uv = [[-2.0, -2.0], [10.0, -2.0], [10.0, 10.0], [-2.0, 10.0]]
    a = render(uv, [[0, 1, 3], [1, 2, 3]], 8, 1e-4)
    assert float((a - 1).abs().max()) <= 1e-12


# one face whose edge x = 0 runs through the centres of the middle column of a 5 x 5 image (centres at -0.8 ... 0.8)
EDGE_UV = [[0.0, -2.0], [0.0, 2.0], [3.0, 0.0]]


def test_edge_through_pixel_centres_gives_one_half():
    a = render(EDGE_UV, [[0, 1, 2]], 5, 1e-4)
    assert torch.equal(a[:, 2], torch.full((5,), 0.5, dtype=torch.float64))
    assert torch.equal(a[:, 3:], torch.ones(5, 2, dtype=torch.float64))          # 0.4 inside: sigmoid(-1600) underflows


def test_pixel_beyond_the_cutoff_is_exactly_zero():
    a = render(EDGE_UV, [[0, 1, 2]], 5, 1e-4)                  # column 1 lies 0.4 outside: d2 = 0.16 >= 16 sigma
    assert torch.equal(a[:, :2], torch.zeros(5, 2, dtype=torch.float64))
    b = render(EDGE_UV, [[0, 1, 2]], 5, 0.02)                  # 16 sigma = 0.32: column 1 counts, column 0 (d2 = 0.64) does not
    np.testing.assert_allclose(b[:, 1].numpy(), 1 / (1 + np.exp(0.4 ** 2 / 0.02)), rtol=1e-12)
    assert torch.equal(b[:, 0], torch.zeros(5, dtype=torch.float64))
    c = render(EDGE_UV, [[0, 1, 2]], 5, 0.01)                  # d2 == 16 sigma up to rounding: either side of the rule, at most 1.13e-7
    assert float(c[:, 1].max()) <= 1.13e-7


def test_degenerate_and_near_plane_faces_change_nothing():
    uv = EDGE_UV + [[-0.5, -0.5], [0.5, 0.5], [0.5, 0.5], [-0.9, 0.9]]
    base = render(uv, [[0, 1, 2]], 5, 0.02)
    assert torch.equal(render(uv, [[0, 1, 2], [3, 4, 5]], 5, 0.02), base)        # two corners on one point: zero area
    assert torch.equal(render(uv, [[0, 1, 2], [3, 3, 3]], 5, 0.02), base)
    z = torch.ones(7, dtype=torch.float64)
    z[6] = 0.05                                                                   # one vertex in front of the near plane
    assert torch.equal(render(uv, [[0, 1, 2], [3, 4, 6]], 5, 0.02, z=z), base)
    assert not torch.equal(render(uv, [[0, 1, 2], [3, 4, 6]], 5, 0.02), base)     # (the same face at z = 1 does count)
    # ... and such faces get a zero gradient, the others a finite one
    v = from_ndc(uv).requires_grad_(True)
    ref.soft_silhouette(v, torch.tensor([[0, 1, 2], [3, 4, 5]]), K_UNIT, 5, 0.02).sum().backward()
    assert torch.isfinite(v.grad).all() and float(v.grad[0, 3:6].abs().max()) == 0 and float(v.grad[0, :3].abs().max()) > 0


def test_autograd_matches_central_differences():
    gen = torch.Generator().manual_seed(3)
    V, S, sigma = 7, 6, 0.05
    verts = torch.cat([0.6 * (torch.rand(1, V, 2, generator=gen, dtype=torch.float64) - 0.5),
                       1.0 + 0.3 * torch.rand(1, V, 1, generator=gen, dtype=torch.float64)], -1)
    faces = torch.tensor([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 1, 3]])
    K = torch.tensor([[[1.1, 0.05, 0.48], [0.0, 0.9, 0.53], [0.0, 0.0, 1.0]]], dtype=torch.float64)
    up = torch.randn(1, S, S, generator=gen, dtype=torch.float64)
    _, grad = ref.alpha_and_grad(verts, faces, K, S, sigma, up, torch.float64)
    assert float(grad[..., 2].abs().max()) > 0                  # the depth coordinate takes part
    f = lambda v: float((ref.soft_silhouette(v, faces, K, S, sigma) * up).sum())
    h, fd = 1e-6, torch.zeros_like(verts)
    for i in range(V):
        for k in range(3):
            d = torch.zeros_like(verts)
            d[0, i, k] = h
            fd[0, i, k] = (f(verts + d) - f(verts - d)) / (2 * h)
    np.testing.assert_allclose(grad.numpy(), fd.numpy(), atol=1e-6 * float(fd.abs().max()))


# ---------------------------------------------------------------- the feature's surface (all of these fail without it)
def test_header_declares_and_library_exports_the_entry_points():
    from homan_amd import lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "homan_amd.h")).read(), flags=re.S)
    handle = lib.lib()
    for name in ("hm_softsil_workspace_bytes", "hm_softsil_fwd", "hm_softsil_bwd"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(handle, name), name
    # shapes are checked on the host: 48 bytes of record + 6 floats of per-corner gradients per (frame, face); 0 = unsupported
    assert handle.hm_softsil_workspace_bytes(2, 8, 12, 40) == 2 * 12 * (48 + 24)
    for bad in ((0, 8, 12, 40), (2, 8, 0, 40), (2, 8, 12, 0), (2, 8, 12, 4097)):
        assert handle.hm_softsil_workspace_bytes(*bad) == 0, bad
    assert handle.hm_softsil_workspace_bytes(1, 3, 1, 4096) > 0


def test_python_layers_accept_the_keywords():
    from homan_amd import HOMan
    from homan_amd.jointopt import ClipFitter, build_model, optimize_hand_object
    from homan_amd.losses import Losses
    for fn in (HOMan.__init__, build_model, optimize_hand_object, ClipFitter.__init__):
        par = inspect.signature(fn).parameters
        assert par["sil_mode"].default == "nmr" and par["sil_sigma"].default == 1e-4, fn
    par = inspect.signature(Losses.__init__).parameters
    assert par["sil_mode"].default == "nmr" and par["sil_sigma"].default is None


@pytest.mark.parametrize("kw", [dict(sil_mode="blur"), dict(sil_mode="soft", sil_sigma=0.0), dict(sil_mode="soft", sil_sigma=-1e-4),
                                dict(sil_mode="soft", sil_sigma=float("nan"))])
def test_bad_options_raise_before_any_device_work(kw):
    """ValueError comes first: with no inputs at all (and, on this machine, no GPU) the constructor gets no further"""
    from homan_amd import HOMan
    required = [n for n, p in inspect.signature(HOMan.__init__).parameters.items()
                if p.default is inspect.Parameter.empty and n != "self"]
    with pytest.raises(ValueError):
        HOMan(**{n: None for n in required}, **kw)
