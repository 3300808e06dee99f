"""SilhouetteContext's launch methods (forward / backward / reduce / parts_ptr) put every keyword at the position the header
gives its name.  No GPU and no library: `lib.lib()` is a recorder, tensors live on the CPU, and every keyword gets a sentinel
of its own, so an argument that lands one position off is seen."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("hm_sil_fwd_phase_clips", "hm_sil_bwd_phase_clips", "hm_sil_reduce_clips")
PRIMES = iter([101, 103, 107, 109, 113, 127, 131, 137, 139, 149, 151, 157, 163, 167, 173, 179, 181, 191, 193, 197])


def _header_params(name):
    """parameter names of prototype `name`, in order, read off include/homan_amd.h by this file's own regex"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "homan_amd.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return [re.search(r"(\w+)\s*$", p).group(1) for p in m.group(1).split(",")]


class _Recorder:
    """stands in for the loaded library: records the positional arguments of the rasteriser's entry points"""

    def __init__(self):
        self.calls = []

    def hm_sil_workspace_bytes(self, B, V, F, S):
        return 256

    def __getattr__(self, name):
        if name not in CALLS + ("hm_sil_parts",):
            raise AttributeError(name)

        def record(*args):
            self.calls.append((name, args))
            return 0
        return record


@pytest.fixture
def rec(monkeypatch):
    from homan_amd import lib
    r = _Recorder()
    monkeypatch.setattr(lib, "lib", lambda: r)
    monkeypatch.setattr(lib, "ptr", lambda t: None if t is None else t.data_ptr())
    return r


def _context(size, B=3):
    from homan_amd import ops, synth
    verts, faces = synth.box_mesh(1, 1, 1)          # the cube: 8 vertices, 12 faces
    assert verts.shape == (8, 3) and faces.shape == (12, 3)
    return ops.SilhouetteContext(torch.from_numpy(faces)[None].repeat(B, 1, 1), verts.shape[0], B, size, "cpu")


def _tensor():
    return torch.zeros(4)         # (a fresh allocation each: distinct addresses while all of them are alive)


def _own(ctx):
    """what the context supplies, by header name"""
    from homan_amd import ops
    return dict(faces=ctx.faces.data_ptr(), faces_bstride=0, B=ctx.B, V=ctx.V, F=ctx.F, S=ctx.S, znear=ops.NMR_NEAR,
                zfar=ops.NMR_FAR, work_order=ctx.work_order.data_ptr(), workspace=ctx.workspace.data_ptr(),
                adj_off=ctx.adj_off.data_ptr(), adj_items=ctx.adj_items.data_ptr())


def _check(rec, name, expect):
    from homan_amd import lib
    (got_name, args), = rec.calls
    rec.calls.clear()
    names = _header_params(name)
    assert got_name == name and len(args) == len(names) == len(lib._SIGNATURES[name][1])
    assert set(names) == set(expect), set(names) ^ set(expect)
    for pos, (n, a) in enumerate(zip(names, args)):
        assert a == expect[n] and type(a) is type(expect[n]), (name, pos, n, a, expect[n])


FWD_TENSORS = ("verts", "K", "keep", "ref", "keep_sum", "pooled", "loss_out", "pooled_depth", "alpha_full", "rigid_rot6d",
               "rigid_trans", "rigid_scale", "cam_verts_out")
FWD_INTS = ("mask_shared", "rigid_abs", "persistent_outputs", "clip_len", "out_stride", "phases", "stream")
BWD_TENSORS = ("verts", "K", "upstream", "grad_pooled", "keep_sum", "grad_verts", "grad_ndc", "loss_out")
BWD_INTS = ("mode", "clip_len", "out_stride", "phases", "sum_log2q", "stream")


def test_every_keyword_lands_on_its_header_position(rec):
    ctx = _context(32)
    assert (ctx.B, ctx.V, ctx.F, ctx.S, ctx.padded) == (3, 8, 12, 32, False)
    own = _own(ctx)
    assert len(set(map(str, own.values()))) == len(own)            # the context's own values tell positions apart too

    tens = {k: _tensor() for k in FWD_TENSORS}
    kw = dict(tens, orig_size=0.375, **{k: next(PRIMES) for k in FWD_INTS})
    assert ctx.forward(**kw) == 0
    expect = dict(own, **{k: t.data_ptr() for k, t in tens.items()}, **{k: kw[k] for k in FWD_INTS}, orig_size=0.375)
    del expect["adj_off"], expect["adj_items"]
    assert len(set(expect.values())) == len(expect)
    _check(rec, "hm_sil_fwd_phase_clips", expect)

    tens = {k: _tensor() for k in BWD_TENSORS}
    kw = dict(tens, orig_size=0.625, eps=0.21875, **{k: next(PRIMES) for k in BWD_INTS})
    assert ctx.backward(**kw) == 0
    expect = dict({k: own[k] for k in ("B", "V", "F", "S", "adj_off", "adj_items", "workspace")},
                  **{k: t.data_ptr() for k, t in tens.items()}, **{k: kw[k] for k in BWD_INTS}, orig_size=0.625, eps=0.21875)
    assert len(set(expect.values())) == len(expect)
    _check(rec, "hm_sil_bwd_phase_clips", expect)

    tens = {k: _tensor() for k in ("keep_sum", "loss_out", "frame_out")}
    ints = {k: next(PRIMES) for k in ("clip_len", "out_stride", "stream")}
    assert ctx.reduce(**tens, **ints) == 0
    _check(rec, "hm_sil_reduce_clips", dict({k: own[k] for k in ("B", "V", "F", "S", "workspace")},
                                            **{k: t.data_ptr() for k, t in tens.items()}, **ints))

    ctx.parts_ptr()
    assert rec.calls == [("hm_sil_parts", (ctx.workspace.data_ptr(), 3, 8, 12, 32))]


@pytest.mark.parametrize("size", [32, 40])
def test_omitted_keywords_and_defaults(rec, size):
    """size 40 is rendered padded, on S = 64: eps follows the grid, and K arrives as given (the caller rescales it)"""
    from homan_amd import ops
    ctx = _context(size)
    assert ctx.S == (32 if size == 32 else 64) and ctx.padded == (size == 40)
    own = _own(ctx)
    verts, K, pooled = _tensor(), torch.eye(3)[None].repeat(3, 1, 1).contiguous(), _tensor()
    K0 = K.clone()
    ctx.forward(verts=verts, K=K, pooled=pooled, stream=211)
    expect = dict.fromkeys(_header_params("hm_sil_fwd_phase_clips"))
    expect.update({k: v for k, v in own.items() if k in expect})
    expect.update(verts=verts.data_ptr(), K=K.data_ptr(), pooled=pooled.data_ptr(), orig_size=1.0, mask_shared=0, rigid_abs=0,
                  persistent_outputs=0, clip_len=0, out_stride=0, phases=3, stream=211)
    _check(rec, "hm_sil_fwd_phase_clips", expect)

    ctx.sum_log2q = -24
    ctx.backward(verts, K, 5, stream=223)
    expect = dict.fromkeys(_header_params("hm_sil_bwd_phase_clips"))
    expect.update({k: v for k, v in own.items() if k in expect})
    expect.update(verts=verts.data_ptr(), K=K.data_ptr(), mode=5, orig_size=1.0, eps=ctx.eps(), clip_len=0, out_stride=0, phases=3,
                  sum_log2q=-24, stream=223)
    _check(rec, "hm_sil_bwd_phase_clips", expect)
    assert ctx.eps() == (ops.NMR_EPS if size == 32 else ops.NMR_EPS * 40 / 64)
    assert torch.equal(K, K0)

    ctx.reduce(stream=227)
    expect = dict.fromkeys(_header_params("hm_sil_reduce_clips"))
    expect.update({k: v for k, v in own.items() if k in expect})
    expect.update(clip_len=0, out_stride=0, stream=227)
    _check(rec, "hm_sil_reduce_clips", expect)


def test_render_fields(rec):
    from homan_amd import lib, ops
    ctx = _context(32)
    verts, K, pooled = _tensor(), _tensor(), _tensor()
    d = ctx.render_fields(verts=verts, K=K, pooled=pooled, clip_len=2, orig_size=0.5)
    assert d == dict(faces=ctx.faces, faces_bstride=0, B=3, V=8, F=12, S=32, znear=ops.NMR_NEAR, zfar=ops.NMR_FAR, orig_size=0.5,
                     work_order=ctx.work_order, workspace=ctx.workspace, verts=verts, K=K, pooled=pooled, clip_len=2)
    assert set(d) <= {n for n, _ in lib.SilRender._fields_}
    with pytest.raises(TypeError):
        ctx.render_fields(verts=verts, K=K, pooled=pooled, bogus=1)
    with pytest.raises(TypeError):
        ctx.forward(verts=verts, K=K, pooled=pooled, bogus=1, stream=0)
    assert rec.calls == []
