"""Host-only half of the C ABI's memory contract (include/homan_amd.h, Conventions): the table of
tests/memcontract.py covers every pointer parameter of the audited entry points, every requirement above the declared type's
alignment and every workspace base is refused with HM_ERR_BAD_ARG before any HIP call, and the binding's helper hands an
aligned copy to such a parameter.  Nothing here touches a device: the addresses are integers that are never dereferenced."""
import pytest
import torch

from tests import memcontract as mc


def test_every_pointer_parameter_has_a_row():
    decl = mc.header_params()
    for entry in mc.IN_SCOPE:
        want = [name for _, ptr, name in decl[entry] if ptr]
        assert want, entry
        assert sorted(mc.CONTRACT[entry]) == sorted(want), (entry, set(mc.CONTRACT[entry]) ^ set(want))
    for entry, row in mc.CONTRACT.items():
        names = {name: base for base, ptr, name in decl[entry] if ptr}
        for param, nbytes in row.items():
            assert param in names, (entry, param)
            assert nbytes in (1, 4, 8, 16), (entry, param, nbytes)
            assert nbytes >= mc.NATURAL[names[param]], (entry, param)          # never below the declared type's alignment
            lowest = mc.LOWEST.get((entry, param), nbytes)
            assert mc.NATURAL[names[param]] <= lowest <= nbytes, (entry, param)


OWN_TESTS = {"hm_sil_parts"}        # returns a pointer, not a code (hm_sil_fwd_multi takes its workspaces inside HmSilRender)


def test_every_workspace_is_an_enforced_row():
    """of EVERY entry point the header declares, audited or not: a workspace parameter without a row fails here"""
    rows = {(e, p) for e, p, _, _ in mc.elevated_rows()}
    seen = 0
    for entry, params in mc.header_params().items():
        for _, ptr, name in params:
            if ptr and mc.is_workspace(name) and entry not in OWN_TESTS:
                assert (entry, name) in rows, (entry, name)
                seen += 1
    assert seen >= 55


def test_multi_render_and_parts_pointer_refuse_a_misaligned_workspace():
    """the two entries the table cannot drive: hm_sil_fwd_multi reads its workspaces out of the HOST array of HmSilRender, and
    hm_sil_parts returns a device pointer, NULL for a base that violates the contract"""
    import ctypes
    from homan_amd import lib
    handle = lib.lib()
    base = mc.FakeCall.BASE
    dims = dict(B=2, V=8, F=12, S=32)
    for by in (4, 8):
        arr = (lib.SilRender * 2)()
        for k, r in enumerate(arr):
            for j, name in enumerate(("verts", "faces", "K", "pooled", "workspace")):
                setattr(r, name, base + 0x100000 * (10 * k + j + 1))
            for name, v in dims.items():
                setattr(r, name, v)
            r.orig_size, r.znear, r.zfar = 1.0, 0.1, 100.0
        arr[1].workspace += by
        assert ctypes.sizeof(lib.SilRender) == handle.hm_sil_render_bytes()
        assert handle.hm_sil_fwd_multi(ctypes.cast(arr, ctypes.c_void_p), 2, 3, None) == mc.HM_ERR_BAD_ARG, by
        if not torch.cuda.is_available():                    # (the control of the rejection test below, for the same reason)
            arr[1].workspace -= by
            assert handle.hm_sil_fwd_multi(ctypes.cast(arr, ctypes.c_void_p), 2, 3, None) not in (0, mc.HM_ERR_BAD_ARG)
        assert handle.hm_sil_parts(base + by, 2, 8, 12, 32) is None
    got = handle.hm_sil_parts(base, 2, 8, 12, 32)            # (address arithmetic only)
    assert got is not None and got > base and got % 16 == 0


def test_header_states_every_elevated_requirement():
    """a row above the declared type's alignment is written into the header: an ALIGNMENT note or a typed void pointer"""
    text = open(mc.os.path.join(mc.ROOT, "include", "homan_amd.h")).read()
    assert "ALIGNMENT." in text                                               # the Conventions paragraph
    for needle in ("model[4] (lbs_weights) 16 bytes", "alpha_full 8 bytes", "keep and ref 8 bytes", "grad_pooled 8 bytes in mode 3",
                   "gflags 4 bytes", "frame_part: B*8 floats (8-byte aligned)", "sil_parts 16 bytes"):
        assert needle in text, needle


_ROWS = mc.elevated_rows()


@pytest.mark.parametrize("entry,param,nbytes,natural", _ROWS, ids=[f"{e}-{p}" for e, p, _, _ in _ROWS])
def test_misaligned_pointer_is_refused_before_any_hip_call(entry, param, nbytes, natural):
    from homan_amd import lib
    handle = lib.lib()
    # at the declared type's alignment and no better, and at half the requirement: both violate the row
    for by in sorted({natural, nbytes // 2} - {0, nbytes}):
        call = mc.FakeCall(entry, mc.WHEN.get((entry, param))).misalign(param, by)
        assert call(handle) == mc.HM_ERR_BAD_ARG, (entry, param, by)
    if not torch.cuda.is_available():
        # Without a device every HIP call fails at once and touches nothing: the same call with the pointer ALIGNED gets past every
        # argument check (so the alignment is what refused the calls above) and comes back with the launch error.  With a device
        # this control is left to tests/test_memcontract_gpu.py, on real buffers: fake addresses must never reach a kernel.
        assert mc.FakeCall(entry, mc.WHEN.get((entry, param)))(handle) not in (0, mc.HM_ERR_BAD_ARG), (entry, param)


def test_aligned_helper_copies_only_what_is_misaligned():
    from homan_amd import lib
    base = torch.arange(64, dtype=torch.float32)
    assert base.data_ptr() % 16 == 0
    assert lib.aligned(base, 16) is base and lib.aligned(None, 16) is None
    view = base.view(-1)[1:1 + 32].view(2, 4, 4)             # contiguous, element-aligned only
    assert view.is_contiguous() and view.data_ptr() % 8 == 4
    assert lib.aligned(view, 4) is view
    for nbytes in (8, 16):
        got = lib.aligned(view, nbytes)
        assert got is not view and got.data_ptr() % nbytes == 0 and got.data_ptr() != view.data_ptr()
        assert got.is_contiguous() and got.shape == view.shape and got.dtype == view.dtype and torch.equal(got, view)
    two = base.view(-1)[2:34]                                # 8-byte aligned: enough for 8, not for 16
    assert lib.aligned(two, 8) is two and lib.aligned(two, 16) is not two
