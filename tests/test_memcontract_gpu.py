"""Where the kernels read and write (include/homan_amd.h, Conventions), through the raw C ABI.

Every case runs twice.  BASELINE: each tensor an allocation of its own, outputs filled with a sentinel, the workspace exactly
*_workspace_bytes and prepared as the header demands; the outputs are checked against the family's own reference with the
family's own bar (imported, not restated).  PLACED: every input, output and workspace inside ONE byte arena, each at the lowest
alignment its row of tests/memcontract.py accepts and no better (a 4-byte parameter at an address = 4 mod 16), 256 bytes of
poison before and behind every input (NaN for floats, 0 for integers) and 256 bytes of 0xA5 before and behind every output and
workspace.  The placed run must return the baseline's bits in every output (and in what the read-back entry points return of a
workspace), leave every byte outside the outputs and workspaces as it was - guards, pads and inputs - and leave no sentinel in
an element the header says is written.  Then every requirement above the declared type's alignment, and every workspace base, is
violated once on real buffers: HM_ERR_BAD_ARG, every output still at its sentinel.

Every comparison between the two runs is an equality.  A misaligned wide access is never made: the placed run uses only
alignments the table accepts, and a violating pointer is refused on the host."""
import functools

import numpy as np
import pytest
import torch

from tests import memcontract as mc

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 0xC7                      # every byte of an output before the call: no legitimate fp32 / fp64 / index / count / mask value
PAT = 0xA5                       # guards of outputs and workspaces
JUNK = 0x3D                      # content of a workspace that needs no initialisation
BAD_ARG = mc.HM_ERR_BAD_ARG
F32, F64, I32, U8, U64, U32 = np.float32, np.float64, np.int32, np.uint8, np.uint64, np.uint32


class Buf:
    """one device buffer of a case: role "in" (data), "out" (shape, dtype; written = bool mask of the elements the header says are
    written, None = all), "io" (data, updated in place), "ws" (nbytes; zero = zero-filled, else junk)"""

    def __init__(self, name, role, data=None, shape=None, dtype=None, written=None, nbytes=None, zero=True, align=None):
        self.name, self.role, self.written, self.zero, self.align = name, role, written, zero, align
        self.place = None            # a placement better than the row demands, where a case is about what alignment selects
        if role in ("in", "io"):
            self.data = np.ascontiguousarray(data)
            self.shape, self.dtype = self.data.shape, self.data.dtype
        elif role == "out":
            self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        else:
            self.shape, self.dtype = (int(nbytes),), np.dtype(U8)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    def initial(self):
        """the bytes the buffer holds before the call"""
        if self.role in ("in", "io"):
            return self.data.reshape(-1).view(U8).copy()
        if self.role == "out":
            return np.full(self.nbytes, SENT, U8)
        return np.full(self.nbytes, 0 if self.zero else JUNK, U8)

    def poison(self, n, lead):
        """n guard bytes; `lead` = how many of them come before an element boundary of the buffer"""
        if self.role != "in":
            return np.full(n, PAT, U8)
        if self.dtype.kind != "f":
            return np.zeros(n, U8)
        word = np.array([np.nan], self.dtype).view(U8)
        out = np.tile(word, n // len(word) + 2)
        start = (len(word) - lead % len(word)) % len(word)
        return out[start:start + n].copy()


def In(name, data):
    return Buf(name, "in", data=data)


def Out(name, shape, dtype=F32, written=None):
    return Buf(name, "out", shape=shape, dtype=dtype, written=written)


def IO(name, data):
    return Buf(name, "io", data=data)


def Ws(name, nbytes, zero=True):
    return Buf(name, "ws", nbytes=nbytes, zero=zero) if nbytes else None


class Host:
    """a host array the entry point reads during the call"""

    def __init__(self, arr):
        self.arr = np.ascontiguousarray(arr)


def _params(entry):
    return [name for _, _, name in mc.header_params(entry)]


def _bufs(steps):
    seen = []
    for _, args in steps:
        for a in args:
            if isinstance(a, Buf) and all(a is not b for b in seen):
                seen.append(a)
    return seen


def _alignment(buf, steps):
    """the strictest row among the parameters the buffer is passed to (a case states a conditional row's lower figure itself)"""
    if buf.place is not None:
        return buf.place
    if buf.align is not None:
        return buf.align
    need = 1
    for entry, args in steps:
        for name, a in zip(_params(entry), args):
            if a is buf:
                need = max(need, mc.CONTRACT[entry][name])
    return need


def _call(entry, args, addr):
    handle = __import__("homan_amd.lib", fromlist=["lib"]).lib()
    real = []
    for a in args:
        if isinstance(a, Buf):
            real.append(addr[id(a)])
        elif isinstance(a, Host):
            real.append(a.arr.ctypes.data)
        else:
            real.append(a)
    return getattr(handle, entry)(*real)


def _view(raw, buf):
    return raw.view(buf.dtype).reshape(buf.shape)


def run_baseline(steps):
    bufs = _bufs(steps)
    dev = {id(b): torch.from_numpy(b.initial()).cuda() for b in bufs}
    for b in bufs:
        assert dev[id(b)].data_ptr() % 256 == 0
    addr = {k: t.data_ptr() for k, t in dev.items()}
    rcs = [_call(entry, args, addr) for entry, args in steps]
    torch.cuda.synchronize()
    return rcs, {b.name: dev[id(b)].cpu().numpy() for b in bufs}


def run_placed(steps):
    bufs = _bufs(steps)
    chunks, spans, cursor = [], {}, 0
    for b in bufs:
        a = _alignment(b, steps)
        mod, res = (16, a) if a < 16 else (32, 16)
        res = 1 if a == 1 else res
        start = cursor + GUARD
        start += (res - start) % mod
        chunks.append(b.poison(start - cursor, start - cursor))
        chunks.append(b.initial())
        chunks.append(b.poison(GUARD, b.nbytes))
        spans[id(b)] = (start, start + b.nbytes)
        cursor = start + b.nbytes + GUARD
    before = np.concatenate(chunks)
    assert before.shape[0] == cursor
    arena = torch.from_numpy(before).cuda()
    base = arena.data_ptr()
    assert base % 256 == 0
    addr = {k: base + s for k, (s, _) in spans.items()}
    for b in bufs:                                               # at the row's alignment and at no better
        a = _alignment(b, steps)
        assert addr[id(b)] % a == 0 and (a == 16 or addr[id(b)] % 16 == (1 if a == 1 else a)) and addr[id(b)] % 32 != 0
    rcs = [_call(entry, args, addr) for entry, args in steps]
    torch.cuda.synchronize()
    after = arena.cpu().numpy()
    free = np.ones(cursor, bool)                                 # bytes no call may change: guards, pads, inputs
    for b in bufs:
        if b.role != "in":
            s, e = spans[id(b)]
            free[s:e] = False
    changed = np.flatnonzero(free & (after != before))
    where = ""
    if changed.size:
        at = int(changed[0])
        owner = min(bufs, key=lambda b: min(abs(at - spans[id(b)][0]), abs(at - spans[id(b)][1])))
        where = f"{changed.size} bytes changed outside the outputs, first at {at - spans[id(owner)][0]:+d} from the start of " \
                f"`{owner.name}` ({owner.nbytes} bytes, {owner.role})"
    return rcs, {b.name: after[spans[id(b)][0]:spans[id(b)][1]] for b in bufs}, where


def _sentinel_left(raw, buf):
    """elements of an output the header says are written that still hold the sentinel"""
    per = raw.reshape(-1, buf.dtype.itemsize)
    still = (per == SENT).all(1).reshape(buf.shape)
    return int((still if buf.written is None else still & buf.written).sum())


def _bad_legs(steps):
    """(step index, parameter, offset) for every requirement of the case that the entry point must enforce"""
    decl = mc.header_params()
    legs = []
    for k, (entry, args) in enumerate(steps):
        types = {name: base for base, ptr, name in decl[entry] if ptr}
        for name, a in zip(_params(entry), args):
            if not isinstance(a, Buf):
                continue
            need, nat = (a.align or mc.CONTRACT[entry][name]), mc.NATURAL[types[name]]
            if need > nat or (mc.is_workspace(name) and need > 1):
                legs.append((k, name, max(nat, need // 2) if nat > 1 else need // 2))
    return legs


def run_bad_arguments(steps):
    """each enforced requirement violated once, on real device buffers 16 bytes larger than needed: refused, outputs untouched"""
    bufs = _bufs(steps)
    done = []
    for k, name, by in _bad_legs(steps):
        entry, args = steps[k]
        dev = {id(b): torch.from_numpy(np.concatenate([b.initial(), np.full(16, PAT, U8)])).cuda() for b in bufs}
        addr = {key: t.data_ptr() for key, t in dev.items()}
        target = args[_params(entry).index(name)]
        addr[id(target)] += by
        rc = _call(entry, args, addr)
        torch.cuda.synchronize()
        assert rc == BAD_ARG, (entry, name, by, rc)
        for b in bufs:
            if b.role != "in":
                assert np.array_equal(dev[id(b)].cpu().numpy()[:b.nbytes], b.initial()), (entry, name, "touched", b.name)
        done.append((entry, name))
    return done


def contract(steps, check, expect_bad=None):
    bufs = _bufs(steps)
    rcs, base = run_baseline(steps)
    assert rcs == [0] * len(steps), rcs
    for b in bufs:
        if b.role == "out":
            assert _sentinel_left(base[b.name], b) == 0, f"baseline: sentinel left in `{b.name}`"
    check({b.name: _view(base[b.name], b) for b in bufs if b.role != "ws"})
    rcs, placed, where = run_placed(steps)
    assert rcs == [0] * len(steps), rcs
    assert not where, where
    for b in bufs:
        if b.role in ("out", "io"):
            same = np.array_equal(placed[b.name], base[b.name])
            assert same, f"`{b.name}`: {int((placed[b.name] != base[b.name]).sum())} bytes differ from the baseline"
            if b.role == "out":
                assert _sentinel_left(placed[b.name], b) == 0, f"placed: sentinel left in `{b.name}`"
        elif b.role == "in":
            assert np.array_equal(placed[b.name], b.initial()), f"input `{b.name}` was written"
    done = run_bad_arguments(steps)
    if expect_bad is not None:
        assert sorted(set(done)) == sorted(set(expect_bad)), done


def bits(a):
    return np.ascontiguousarray(a).view({4: U32, 8: U64}[a.dtype.itemsize])


CASES = {}


def case(*ids):
    """register a case builder: () -> (steps, check, the enforced rows its bad-argument leg must cover); one case per id"""
    def deco(fn):
        for i in ids:
            CASES[f"{fn.__name__}-{i}"] = functools.partial(fn, i)
        if not ids:
            CASES[fn.__name__] = fn
        return fn
    return deco


# =============================================================================================== evaluation: point clouds
@case("plain", "affine")
def cloud_metrics(kind):
    from tests.test_pointmetrics_gpu import check_frame, cloud
    L = __import__("homan_amd.lib", fromlist=["lib"]).lib()
    B, N, M = 2, 65, 129
    rng = np.random.default_rng(5)
    x, y = cloud(rng, B, N), cloud(rng, B, M)
    aff = None
    if kind == "affine":
        aff = [np.concatenate([rng.normal(size=(B, 3)) * 0.05, rng.uniform(0.5, 2.0, size=(B, 2))], 1).astype(F32) for _ in range(2)]
    nbytes = L.hm_cloud_metrics_workspace_bytes(B, N, M)
    args = [In("x", x), In("y", y), B, N, M, In("aff_x", aff[0]) if aff else None, In("aff_y", aff[1]) if aff else None,
            Out("x_d2", (B, N)), Out("x_idx", (B, N), I32), Out("y_d2", (B, M)), Out("y_idx", (B, M), I32),
            Out("out4", (B, 4), F64), Ws("workspace", nbytes, zero=False), None]           # (out4[3]: NaN when N != M, but written)

    def check(o):
        for b in range(B):
            check_frame(x[b], y[b], o["out4"][b], o["x_d2"][b], o["x_idx"][b], o["y_d2"][b], o["y_idx"][b],
                        aff[0][b] if aff else None, aff[1][b] if aff else None)
    return [("hm_cloud_metrics", args)], check, [("hm_cloud_metrics", "workspace")]


@case()
def align_stats():
    from tests.test_pointmetrics import restate_align_metrics
    from tests.test_pointmetrics_gpu import ALIGN_ATOL, ALIGN_RTOL
    B, hands, V = 2, 2, 257
    rng = np.random.default_rng(11)
    gt = (rng.normal(size=(B * hands, V, 3)) * 0.05 + np.array([0.0, 0.1, 0.5])).astype(F32)
    pred = (gt * F32(1.3) + rng.normal(size=gt.shape).astype(F32) * F32(0.004) + F32(0.02)).astype(F32)
    args = [In("gt_hand", gt), In("pred_hand", pred), B, hands, V, 1, Out("aff_gt", (B, 5)), Out("aff_pred", (B, 5)),
            Out("hand_mean", (B * hands,), F64), None]

    def check(o):
        obj = np.zeros((B, 4, 3), F32)
        want = restate_align_metrics(gt, pred, obj, obj)["hand_mean_aligned"]
        np.testing.assert_allclose(o["hand_mean"], want, rtol=ALIGN_RTOL, atol=ALIGN_ATOL)
        assert np.array_equal(o["aff_gt"][:, 3:], np.ones((B, 2), F32))
        np.testing.assert_allclose(o["aff_gt"][:, :3], gt[::hands].astype(F64).mean(1), rtol=1e-6, atol=1e-7)
        assert np.array_equal(bits(o["aff_pred"][:, :3]), bits(o["aff_gt"][:, :3]))          # pred_centroid_from_gt
    return [("hm_align_stats", args)], check, []


@case("n21-m0", "n21-m1", "n21-m2", "n65-m0", "n65-m1", "n65-m2")
def procrustes_align(tag):
    from tests import handmetrics_ref as ref
    from tests.test_handmetrics_gpu import _anchors, apply_xform, err_bar, hand_sets
    N, mode = int(tag[1:3]), int(tag[-1])
    B = 2
    pred, gt, _ = hand_sets(B, N)
    a, b = _anchors(N)
    args = [In("pred", pred), In("gt", gt), B, N, mode, a, b, Out("aligned", (B, N, 3)), Out("err", (B, N), F64),
            Out("xform", (B, 13), F64), None]

    def check(o):
        rows = [ref.align(p, g, mode, (a, b)) for p, g in zip(pred, gt)]
        want_al, want_err = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        assert (np.abs(o["err"] - want_err) <= err_bar(pred, gt)).all()
        ulp = np.spacing(np.abs(want_al).astype(F32)).astype(F64)
        assert (np.abs(o["aligned"].astype(F64) - want_al) <= ulp).all()
        assert (np.abs(o["aligned"].astype(F64) - apply_xform(o["xform"], pred)) <= ulp).all()
    return [("hm_procrustes_align", args)], check, []


@case("f32-s3", "f32-s1024", "f64-s3", "f64-s1024")
def threshold_counts(tag):
    from tests import handmetrics_ref as ref
    from tests.test_handmetrics_gpu import _distances
    dtype, steps = (F32 if tag.startswith("f32") else F64), int(tag.split("-s")[1])
    n, val_max = 257, 0.05
    vals = _distances(n, val_max, steps, dtype, seed=n + steps)
    dist = In("dist", vals)
    dist.align = 8 if dtype == F64 else 4
    args = [dist, n, int(dtype == F64), Host(np.array([val_max], F64)), steps, Out("counts", (steps,), U64), None]

    def check(o):
        assert np.array_equal(o["counts"], ref.threshold_counts(vals, val_max, steps))
    return [("hm_threshold_counts", args)], check, [("hm_threshold_counts", "dist"), ("hm_threshold_counts", "counts")]


@case("t1", "t8")
def fscore(tag):
    from tests import handmetrics_ref as ref
    T = int(tag[1:])
    B, N, M = 2, 65, 257
    rng = np.random.default_rng(N + 7 * M)
    gt = (rng.normal(size=(B, M, 3)) * 0.04 + np.array([0.05, -0.1, 0.6])).astype(F32)
    pred = (rng.normal(size=(B, N, 3)) * 0.04 + np.array([0.05, -0.1, 0.6]) + 0.004).astype(F32)
    x_d2 = np.stack([ref.nn_d2(p, g) for p, g in zip(pred, gt)])
    y_d2 = np.stack([ref.nn_d2(g, p) for p, g in zip(pred, gt)])
    ths = np.array([0.005, 0.015, 0.002, 0.01, 0.02, 0.03, 0.001, 0.05][:T], F32)
    args = [In("x_d2", x_d2), In("y_d2", y_d2), B, N, M, Host(ths), T, Out("out", (B, T, 3), F64), None]

    def check(o):
        for f in range(B):
            assert np.abs(o["out"][f] - ref.fscore_from_d2(x_d2[f], y_d2[f], ths)).max() <= ref.FSCORE_BAR
    return [("hm_fscore", args)], check, []


@case("gather-f32", "gather-f64", "all-f32", "all-f64")
def keyframe_interp(tag):
    from tests.test_ho3deval import flipped, reference_formula
    K, N, frame_nb = 3, 5, 7
    gather = np.array([4, 0, 4], I32) if tag.startswith("gather") else None
    M = 3 if gather is not None else N
    f64 = tag.endswith("f64")
    rng = np.random.default_rng(3)
    key_vals = (rng.normal(size=(K, N, 3)) * 0.1).astype(F32)
    key_frames = np.array([0, 2, 5], I32)
    signs = np.array([1.0, -1.0, -1.0], F32)
    out = Out("out", (frame_nb, M, 3), F64 if f64 else F32)
    out.align = 8 if f64 else 4
    args = [In("key_vals", key_vals), Host(key_frames), K, N, frame_nb, Host(gather) if gather is not None else None, M, Host(signs),
            int(f64), Out("key_frames_dev", (K,), I32), Out("gather_dev", (M,), I32) if gather is not None else None, out, None]

    def check(o):
        interp = reference_formula(key_vals, key_frames, frame_nb)
        want = interp * signs.astype(F64)                                  # (the fp64 output: the sign on the double, no rounding)
        want = (want if gather is None else want[:, gather]) if f64 else flipped(interp, signs, gather)
        assert np.array_equal(bits(o["out"]), bits(np.ascontiguousarray(want)))
        assert np.array_equal(o["key_frames_dev"], key_frames)
    return [("hm_keyframe_interp", args)], check, [("hm_keyframe_interp", "out")]


# =============================================================================================== evaluation: volumes and surfaces
def _cube_batch():
    """the cube (12 faces) in two poses"""
    from tests import volmetrics_ref as ref
    v, f = ref.cube_mesh([0.001, 0.002, -0.013], [0.031, 0.041, 0.018])
    verts = np.stack([v, (v * F32(1.25) + np.array([0.004, -0.003, 0.002], F32)).astype(F32)])
    return verts, np.ascontiguousarray(f, I32)


@case()
def mesh_volume():
    from tests import volmetrics_ref as ref
    from tests.test_volmetrics_gpu import EPS
    verts, f = _cube_batch()
    args = [In("verts", verts), In("faces", f), 2, 8, 12, Out("out", (2,), F64), None]

    def check(o):
        for b in range(2):
            want, sum_abs = ref.mesh_volume(verts[b], f)
            assert abs(o["out"][b] - want) <= 4 * EPS * len(f) * sum_abs / 6
    return [("hm_mesh_volume", args)], check, []


@case()
def solid_voxels_and_overlap():
    from tests import volmetrics_ref as ref
    from tests.test_volmetrics import H, own_box
    verts, f = _cube_batch()
    B = 2
    boxes = np.stack([own_box(verts[b], H) for b in range(B)]).astype(I32)
    nwx, ny, nz = int(-(-boxes[:, 3].max() // 32)), int(boxes[:, 4].max()), int(boxes[:, 5].max())
    per = nwx * ny * nz
    other = (verts + np.array([0.006, 0.0, 0.004], F32)).astype(F32)
    words, words_b, faces = Out("words", (B, nz, ny, nwx), U32), Out("words_b", (B, nz, ny, nwx), U32), In("faces", f)
    steps = [("hm_solid_voxels", [In("verts", verts), faces, B, 8, 12, float(F32(H)), Host(boxes), nwx, ny, nz,
                                  Out("boxes_dev", (B, 6), I32), words, None]),
             ("hm_solid_voxels", [In("verts_b", other), faces, B, 8, 12, float(F32(H)), Host(boxes), nwx, ny, nz,
                                  Out("boxes_dev_b", (B, 6), I32), words_b, None]),
             ("hm_voxel_overlap", [words, 1, words_b, B, per, Out("counts", (B, 3), U64), None])]

    def check(o):
        wa, wb = ref.solid_voxels(verts, f, H, boxes, (nwx, ny, nz)), ref.solid_voxels(other, f, H, boxes, (nwx, ny, nz))
        assert np.array_equal(o["words"], wa) and np.array_equal(o["words_b"], wb) and ref.popcount(wa) > 30
        assert np.array_equal(o["counts"], ref.overlap_counts(wa, wb)) and o["counts"][:, 0].min() > 0
        assert np.array_equal(o["boxes_dev"], boxes)
    return steps, check, [("hm_solid_voxels", "words"), ("hm_voxel_overlap", "a"), ("hm_voxel_overlap", "b"),
                          ("hm_voxel_overlap", "counts")]


def _cube_points(N, seed=2, split=False):
    """cube in two poses (split: 257 faces of the 500-face box, one face into a second staging chunk, so that the faces of a frame
    are shared by two workgroups and the workspace is used) and N points about it: inside, outside, on a vertex"""
    verts, f = _cube_batch()
    if split:
        from homan_amd import ops, synth
        v, faces = synth.box_mesh()
        f = np.ascontiguousarray(faces[np.linspace(0, len(faces) - 1, ops.SURFDIST_CHUNK + 1).astype(int)], I32)
        verts = np.stack([v.astype(F32), (v * F32(1.25) + np.array([0.004, -0.003, 0.002], F32)).astype(F32)])
    rng = np.random.default_rng(seed)
    lo, hi = verts.min(1, keepdims=True), verts.max(1, keepdims=True)
    pts = (lo - 0.01 + rng.uniform(size=(2, N, 3)) * (hi - lo + 0.02)).astype(F32)
    pts[:, 0] = verts[:, 0]                                           # a point on a corner: D == 0
    return pts, verts, f


@case("cube", "split")
def point_mesh_distance(kind):
    from tests import surfmetrics_ref as ref
    L = __import__("homan_amd.lib", fromlist=["lib"]).lib()
    pts, verts, f = _cube_points(65, split=kind == "split")
    B, N, V, F = 2, 65, verts.shape[1], len(f)
    nbytes = L.hm_point_mesh_workspace_bytes(B, N, F)
    args = [In("points", pts), In("verts", verts), In("faces", f), B, N, V, F, Out("d2", (B, N)), Out("face_idx", (B, N), I32),
            Out("inside", (B, N), I32), Out("closest", (B, N, 3)), Ws("workspace", nbytes, zero=False), None]

    def check(o):
        for b in range(B):
            want = ref.point_mesh(pts[b], verts[b], f)
            for key, name in (("d2", "d2"), ("face", "face_idx"), ("inside", "inside"), ("closest", "closest")):
                assert np.array_equal(bits(o[name][b]), bits(want[key])), (b, key)
        assert 0 < o["inside"].sum() < B * N and (nbytes > 0) == (kind == "split")
    return [("hm_point_mesh_distance", args)], check, ([("hm_point_mesh_distance", "workspace")] if nbytes else [])


@case("detail", "tail", "tail-split")
def surface_contact(kind):
    """forward with every optional output (detail), and with face_idx == NULL so that the workspace's tail holds it (tail); then
    the backward on the forward's outputs"""
    from tests import surfcontact_ref as ref
    L = __import__("homan_amd.lib", fromlist=["lib"]).lib()
    pts, verts, f = _cube_points(65, seed=4, split=kind.endswith("split"))
    B, N, V, F = 2, 65, verts.shape[1], len(f)
    rng = np.random.default_rng(9)
    weights = rng.uniform(0.0, 2.0, size=N).astype(F32)
    c_a, c_r = 0.01, 0.02
    lq = ref.log2q(N, float(weights.max()), c_a, c_r)
    nbytes = L.hm_surface_contact_workspace_bytes(B, N, V, F)
    detail = kind == "detail"
    gp, ins = Out("grad_points", (B, N, 3)), Out("inside", (B, N), I32)
    ga, gr = Out("grad_verts_attr", (B, V, 3)), Out("grad_verts_rep", (B, V, 3))
    fwd = [In("points", pts), In("verts", verts), In("faces", f), In("weights", weights), B, N, V, F, c_a, c_r, lq, Out("out", (2,)),
           gp, ins, ga, gr, Out("value", (B, N)) if detail else None, Out("bary", (B, N, 3)) if detail else None,
           Out("d2", (B, N)) if detail else None, Out("face_idx", (B, N), I32) if detail else None,
           Ws("workspace", nbytes, zero=False), None]
    up = np.array([0.75, -1.5], F32)
    bwd = [gp, ins, ga, gr, In("upstream", up), B * N, B * V, Out("g_points", (B, N, 3)), Out("g_verts", (B, V, 3)), None]

    def check(o):
        want = ref.loss_and_gradients(pts, verts, f, weights, c_a, c_r, L=lq)
        names = ["out", "grad_points", "grad_verts_attr", "grad_verts_rep", "inside"] + (["value", "bary", "d2"] if detail else [])
        for k in names:
            assert np.array_equal(bits(o[k]), bits(want[k])), k
        if detail:
            assert np.array_equal(o["face_idx"], want["face"])
        assert 0 < want["inside"].sum() < B * N and (want["out"] > 0).all()
        assert (L.hm_point_mesh_workspace_bytes(B, N, F) > 0) == kind.endswith("split")
        scale = np.where(want["inside"][..., None] != 0, up[1], up[0]).astype(F32)
        assert np.array_equal(bits(o["g_points"]), bits((scale * want["grad_points"]).astype(F32)))
        assert np.array_equal(bits(o["g_verts"]), bits((up[0] * want["grad_verts_attr"] + up[1] * want["grad_verts_rep"]).astype(F32)))
    return [("hm_surface_contact_fwd", fwd), ("hm_surface_contact_bwd", bwd)], check, [("hm_surface_contact_fwd", "workspace")]


# =============================================================================================== soft silhouettes
def _lib():
    from homan_amd import lib
    return lib.lib()


@case()
def softsil():
    from homan_amd import ops
    from tests import softsil_ref as ref
    from tests.test_softsil_gpu import _mesh, _rot
    B, S, F = 2, 40, 65
    gen = torch.Generator().manual_seed(140)
    mesh, faces = _mesh(F)
    verts = torch.stack([(mesh.double() @ _rot(gen).T + torch.tensor([0.03 * b, -0.02 * b, 0.6 + 0.05 * b])).float() for b in range(B)])
    K = torch.tensor([[1.2, 0.02, 0.5], [0.0, 1.15, 0.52], [0.0, 0.0, 1.0]]).expand(B, 3, 3).contiguous()
    sigma = float(F32(4e-3))
    up = torch.randn(B, S, S, generator=gen)
    a64, g64 = ref.alpha_and_grad(verts, faces, K, S, sigma, up, torch.float64)
    a32, g32 = ref.alpha_and_grad(verts, faces, K, S, sigma, up, torch.float32)
    V = verts.shape[1]
    off, items = ops.build_adjacency(faces.numpy(), V)
    ws = Ws("workspace", _lib().hm_softsil_workspace_bytes(B, V, F, S), zero=False)
    v, f, k, sg = In("verts", verts.numpy()), In("faces", faces.numpy().astype(I32)), In("K", K.numpy()), In("sigma", np.array([sigma], F32))
    alpha = Out("alpha", (B, S, S))
    dims = [B, V, F, S, 1.0, ops.NMR_NEAR, ops.NMR_FAR]
    fwd = [v, f, k] + dims + [sg, alpha, ws, None]
    bwd = [v, f, k] + dims + [sg, alpha, In("grad_alpha", up.numpy()), In("adj_off", off.numpy()), In("adj_items", items.numpy()),
                              Out("grad_verts", (B, V, 3)), ws, None]

    def check(o):
        got_a, got_g = torch.from_numpy(o["alpha"]).double(), torch.from_numpy(o["grad_verts"]).double()
        assert float((got_a - a64).abs().max()) <= ref.RULE_FACTOR * float((a32.double() - a64).abs().max()) + ref.IMAGE_ABS
        gmax = float(g64.abs().max())
        assert gmax > 0 and float((got_g - g64).abs().max()) / gmax <= ref.RULE_FACTOR * float((g32.double() - g64).abs().max()) / gmax
    return [("hm_softsil_fwd", fwd), ("hm_softsil_bwd", bwd)], check, [("hm_softsil_fwd", "workspace"), ("hm_softsil_bwd", "workspace")]


@case("s15", "s16-scalar", "s16-vector")
def softsil_pose_terms(tag):
    """S = 15: npix odd, the scalar path.  S = 16: the baseline's own allocations take the 16-byte path; the placement at 4 mod 16
    must take the scalar path and the placement at 16 mod 32 the vector path - and all three give the same bits."""
    from tests import softpose_ref
    from tests.test_softpose_gpu import _grad32, _masks, _sums64
    N, S = 2, int(tag[1:3])
    gen = torch.Generator().manual_seed(1000 * N + S)
    alpha = torch.randint(0, 9, (N, S, S), generator=gen).float() / 8          # (exact inputs: any order of the sums is exact)
    mask = _masks(S, gen)["banded"]
    keep, tgt = (mask >= 0).float(), (mask > 0).float()
    imgs = [In("alpha", alpha.numpy()), In("keep", keep.numpy()), In("ref", tgt.numpy())]
    grad = Out("grad", (N, S, S))
    for b in imgs + [grad]:
        b.place = 16 if tag.endswith("vector") else None
    args = imgs + [N, S, Out("terms", (N, 2)), grad, Ws("workspace", _lib().hm_softsil_pose_workspace_bytes(N, S)), None]

    def check(o):
        sq, inter, union = _sums64(alpha, mask)
        iou = inter / (union + 1e-6)
        terms = torch.from_numpy(o["terms"])
        assert torch.equal(terms[:, 0].double(), sq) and ((terms[:, 1].double() - iou).abs() <= softpose_ref.IOU_REL * iou).all()
        assert torch.equal(torch.from_numpy(o["grad"]), _grad32(alpha, mask))
    return [("hm_softsil_pose_terms", args)], check, [("hm_softsil_pose_terms", "workspace")]


@case()
def sigma_anneal():
    from tests import softpose_ref as ref
    args = [IO("sigma", np.array([0.01], F32)), 0.5, 1e-3, None]

    def check(o):
        assert bits(o["sigma"])[0] == bits(np.array([ref.anneal_sequence(0.01, 0.5, 1e-3, 1)[1]], F32))[0]
    return [("hm_sigma_anneal", args)], check, []


# =============================================================================================== pose initialisation
@case()
def edge_edt_and_terms():
    """hm_edge_edt with power 1 (the output IS the exact squared distance), then hm_pose_edge_terms on two candidates"""
    from scipy.ndimage import distance_transform_edt
    from tests.test_poseedge_gpu import EDGE_REL, _band, _edge_case_images, _masks, _torch_edge_terms
    size, k, lw, n = 64, 7, 0.5, 2
    rng = np.random.default_rng(100 * size + k)
    target = (_masks(size, rng)["blobs"] > 0).astype(F32)
    band = _band(target, k)
    edt_step = ("hm_edge_edt", [In("target", target), size, size, k, 1.0, Out("d2", (size, size)), Out("band_count", (1,), I32), None])
    alpha7, keep, ref = _edge_case_images(size, rng)
    alpha = alpha7[[3, 4]]
    edt = (distance_transform_edt(~_band(ref, k)) ** 0.5).astype(F32)
    ws = Ws("workspace", _lib().hm_pose_edge_workspace_bytes(n, size))
    terms_step = ("hm_pose_edge_terms", [In("alpha", alpha.astype(F32)), In("keep", keep.astype(F32)), In("ref", ref.astype(F32)),
                                         In("edt", edt), n, size, size, k, lw, Out("terms", (n, 4)), Out("grad", (n, size, size)), ws, None])

    def check(o):
        want = np.rint(distance_transform_edt(~band) ** 2).astype(np.int64)
        assert int(o["band_count"][0]) == int(band.sum()) > 0 and np.array_equal(o["d2"], want.astype(F32))
        terms, grad = o["terms"], o["grad"]
        img = keep[None] * alpha
        inter, union = (img * ref).sum((1, 2)), np.clip(img + ref, 0, 1).sum((1, 2))
        mask, cham, g, mag, cham_mag = _torch_edge_terms(alpha, keep, ref, edt, k, lw, "cpu", torch.float64)
        assert np.array_equal(terms[:, 2], mask.astype(F32))
        assert np.array_equal(terms[:, 1], inter.astype(F32) / (union.astype(F32) + F32(1e-6)))
        assert (np.abs(terms[:, 3] - cham) <= EDGE_REL * cham_mag).all() and (np.abs(grad - g) <= EDGE_REL * mag).all()
        assert np.array_equal(terms[:, 0], terms[:, 2] + F32(lw) * terms[:, 3]) and float(terms[:, 3].max()) > 0
    return [edt_step, terms_step], check, [("hm_pose_edge_terms", "workspace")]


@case()
def pose_keep_best():
    n, T = 5, 3
    g = torch.Generator().manual_seed(3)
    rot, trans = torch.randn(n, 3, 2, generator=g).numpy(), torch.randn(n, 1, 3, generator=g).numpy()
    sums, extra = torch.rand(n, 2, generator=g).numpy(), (torch.rand(n, generator=g) * 0.1).numpy()
    sums[3, 0] = sums[1, 0] = -1.0                                   # a tie at the minimum: the first index wins
    extra[3] = extra[1]
    ins = [In("sums", sums), 2, In("extra", extra), n, In("rot6d", rot), In("trans", trans)]
    best = ins + [IO("best_loss", np.array([np.inf], F32)), IO("best_rot6d", np.zeros((3, 2), F32)), IO("best_trans", np.zeros((1, 3), F32)),
                  Out("losses_out", (n,)), None]
    rows = np.zeros((T, 16), bool)
    rows[1] = True                                                   # row step[0] - 1
    log = ins + [In("step", np.array([2, 0], I32)), T, Out("log", (T, 16), written=rows), Out("losses_log", (n,)), None]

    def check(o):
        losses = sums[:, 0] + extra
        assert np.array_equal(o["losses_out"], losses) and np.array_equal(o["losses_log"], losses) and int(np.argmin(losses)) == 1
        assert o["best_loss"][0] == losses[1] and np.array_equal(o["best_rot6d"], rot[1]) and np.array_equal(o["best_trans"], trans[1])
        rec = o["log"][1]
        assert rec[0] == losses[1] and int(rec[1:2].view(I32)[0]) == 1 and rec[2] == 0
        assert np.array_equal(rec[3:9], rot[1].reshape(-1)) and np.array_equal(rec[9:12], trans[1].reshape(-1)) and not rec[12:].any()
    return [("hm_pose_keep_best", best), ("hm_pose_keep_best_log", log)], check, []


@case()
def offscreen_and_scale_by():
    from homan_amd import ops
    from tests import softpose_ref as ref
    from tests.test_poseinit import OFFSCREEN_ATOL, OFFSCREEN_RTOL
    N, V = 2, 65
    rng = np.random.default_rng(8)
    verts = (rng.normal(size=(N, V, 3)) * 0.3 + np.array([0.1, -0.1, 0.0])).astype(F32)             # some outside the image ...
    verts[..., 2] = np.abs(verts[..., 2]) + F32(0.3)                                                 # (z well away from 0)
    verts[:, :5, 2] = F32(-0.4)                                                                      # ... some behind the camera
    verts[:, 5, 2] = F32(120.0)                                                                      # ... one beyond the far plane
    K = np.array([[1.2, 0.02, 0.5], [0.0, 1.15, 0.52], [0.0, 0.0, 1.0]], F32)
    grad = Out("grad", (N, V, 3))
    off = ("hm_offscreen_fwd", [In("verts", verts), In("K", K), N, V, ops.NMR_FAR, 100000.0, Out("out", (N,)), grad, None])
    s = np.array([-0.375], F32)
    scale = ("hm_scale_by", [grad, In("s", s), N * V * 3, Out("scaled", (N, V, 3)), None])

    def check(o):
        res = {}
        for dt in (torch.float64, torch.float32):
            v = torch.from_numpy(verts).to(dt).requires_grad_(True)
            val = ref.offscreen(v, torch.from_numpy(K).to(dt))
            val.sum().backward()
            res[dt] = (val.detach().double(), v.grad.double())
        (v64, g64), (v32, g32) = res[torch.float64], res[torch.float32]
        assert float(v64.min()) > 0
        np.testing.assert_allclose(o["out"], v64.numpy(), rtol=OFFSCREEN_RTOL, atol=OFFSCREEN_ATOL)
        top = float(g64.abs().max())
        got = torch.from_numpy(o["grad"]).double()
        assert float((got - g64).abs().max()) / top <= ref.RULE_FACTOR * float((g32 - g64).abs().max()) / top       # (the rule of _check_grads)
        assert np.array_equal(bits(o["scaled"]), bits(s[0] * o["grad"]))
    return [off, scale], check, []


# =============================================================================================== masks
def _mask_scene():
    rng = np.random.default_rng(37)
    H, W = 37, 53
    y, x = np.mgrid[:H, :W]
    masks = np.stack([((y - 18) / 11.0) ** 2 + ((x - 20) / 14.0) ** 2 <= 1, (rng.random((H, W)) < 0.5)])
    boxes = np.array([[3.3, 2.1, 40.7, 33.9], [-4.0, 6.5, 30.25, 41.0]], F32)
    return H, W, masks, boxes


@case("bytes", "f32")
def mask_crop_resize(tag):
    from tests import maskcrop_ref
    H, W, masks, boxes = _mask_scene()
    S, R = 16, 2
    index = np.array([1, 0], I32)
    f32 = tag == "f32"
    m = In("masks", (masks * F32(0.25)).astype(F32) if f32 else masks.astype(U8))
    m.align = 4 if f32 else 1
    args = [m, int(f32), 2, H, W, In("index", index), In("boxes", boxes), R, S, Out("out", (R, S, S), U8), None]

    def check(o):
        want = maskcrop_ref.crop_and_resize(masks, boxes, S, index)
        assert np.array_equal(o["out"], np.asarray(want).astype(U8)) and 0 < o["out"].sum() < o["out"].size
    return [("hm_mask_crop_resize", args)], check, [("hm_mask_crop_resize", "masks")] if f32 else []


@case("bytes", "f32")
def target_masks(tag):
    from tests import maskcrop_ref
    H, W, masks, boxes = _mask_scene()
    S, R, K = 16, 2, 2
    rng = np.random.default_rng(5)
    occ = np.stack([(rng.random((H, W)) < 0.15), np.zeros((H, W), bool)])
    occ[1, 10:20, 25:45] = True
    t_index, o_index = np.array([1, 0], I32), np.array([[0, -1], [1, 0]], I32)
    f32 = tag == "f32"
    tgt, oc = In("target", (masks * F32(0.5)).astype(F32) if f32 else masks.astype(U8)), In("occluders", (occ * F32(2.0)).astype(F32))
    tgt.align, oc.align = (4 if f32 else 1), 4
    args = [0, tgt, int(f32), 2, In("target_index", t_index), oc, 1, 2, In("occluder_index", o_index), K, H, W, In("boxes", boxes), R, S,
            Out("out", (R, S, S)), None]

    def check(o):
        t = np.asarray(maskcrop_ref.crop_and_resize(masks, boxes, S, t_index)).astype(F32)
        for r in range(R):
            for n in o_index[r]:
                if n >= 0:
                    t[r][np.asarray(maskcrop_ref.crop_and_resize(occ, boxes[r:r + 1], S, np.array([n])))[0]] = -1
        assert np.array_equal(o["out"], t) and set(np.unique(t)) == {-1.0, 0.0, 1.0}
    return [("hm_target_masks", args)], check, [("hm_target_masks", "occluders")] + ([("hm_target_masks", "target")] if f32 else [])


@case()
def instance_masks():
    B, S, F, I = 2, 16, 12, 2
    rng = np.random.default_rng(16)
    idx = rng.integers(-1, 2 * F, size=(B, 2 * S, 2 * S)).astype(I32)
    start = np.array([0, 5, 12], I32)
    args = [In("idx_map", idx), B, S, F, Host(start), I, Out("out", (B, I, S, S), U8), None]

    def check(o):
        f = np.where(idx >= F, idx - F, idx)[:, ::-1]                       # (sample rows are bottom-up)
        for i in range(I):
            own = (f >= start[i]) & (f < start[i + 1])
            assert np.array_equal(o["out"][:, i], own.reshape(B, S, 2, S, 2).sum((2, 4)).astype(U8)), i
    return [("hm_instance_masks", args)], check, []


# =============================================================================================== silhouette rasteriser
@functools.lru_cache(maxsize=None)
def _cube_scene():
    from homan_amd import synth
    from tests import raster_ref as rr
    cv, cf = synth.box_mesh(1, 1, 1, scale=0.2)
    frames = []
    for b, (ax, ay) in enumerate(((0.5, 0.7), (1.1, 0.4))):
        R = torch.tensor(synth._rot_x(ax) @ synth._rot_y(ay), dtype=torch.float32)
        frames.append(torch.from_numpy(cv).float() @ R + torch.tensor([0.02 * b, -0.015 * b, 0.6 + 0.05 * b]))
    return rr._scene("memcontract-cube", torch.stack(frames), np.asarray(cf, np.int64), rr._K_ROI, 32)


class _Sil:
    """the shared buffers and argument lists of the silhouette cases"""

    def __init__(self):
        from homan_amd import ops
        from tests import raster_ref as rr
        self.rr, self.sc = rr, _cube_scene()
        sc = self.sc
        self.B, self.V, self.F, self.S = sc.verts.shape[0], sc.verts.shape[1], sc.faces.shape[0], sc.S
        self.dims = [self.B, self.V, self.F, self.S]
        off, items = ops.build_adjacency(sc.faces.numpy(), self.V)
        self.verts, self.faces, self.K = In("verts", sc.verts.numpy()), In("faces", sc.faces.numpy().astype(I32)), In("K", sc.K.numpy())
        self.adj = [In("adj_off", off.numpy()), In("adj_items", items.numpy())]
        self.ws = Ws("workspace", _lib().hm_sil_workspace_bytes(*self.dims))
        self.idx, self.parts = Out("idx_map", (self.B, 64, 64), I32), Out("parts", (self.B, self.F, 3, 2), F64)
        self.faces9 = Out("faces9", (self.B, self.F, 9))

    def fwd(self, keep=None, ref=None, keep_sum=None, pooled=None, loss_out=None, depth=None, alpha_full=None, mask_shared=0):
        sc = self.sc
        return ("hm_sil_fwd", [self.verts, self.faces, 0, self.K] + self.dims + [1.0, sc.znear, sc.zfar, keep, ref, keep_sum, pooled,
                               loss_out, None, depth, alpha_full, mask_shared, None, None, None, 0, 0, self.ws, None])

    def bwd(self, mode, upstream=None, grad_pooled=None, keep_sum=None, grad_verts=None, grad_ndc=None):
        return ("hm_sil_bwd", [self.verts, self.K] + self.dims + [1.0, self.rr.EPS, mode, upstream, grad_pooled, keep_sum] + self.adj +
                [grad_verts, grad_ndc, self.ws, 0, None])

    def reduce(self, keep_sum=None, loss_out=None, frame_out=None):
        return ("hm_sil_reduce", self.dims + [keep_sum, loss_out, frame_out, self.ws, None])

    def read(self, what):
        buf = {"idx_map": self.idx, "parts": self.parts, "faces9": self.faces9}[what]
        return (f"hm_sil_read_{what}", [self.ws] + self.dims + [buf, None])

    def oracle(self, o):
        """(both, idx, dep) of the oracle on the kernel's own packed faces; the index map must be the oracle's"""
        both, idx, dep = self.rr.oracle_maps(o["faces9"], self.S, self.sc.znear, self.sc.zfar)
        assert np.array_equal(o["idx_map"], idx) and (idx >= 0).sum() > 50
        return both, idx, dep

    def check_gather(self, o, parts, name="grad_verts"):
        sc = self.sc
        ndc, gverts = self.rr.gather_ref(parts, sc.faces.numpy(), sc.verts.numpy(), sc.K.numpy())
        assert np.isfinite(gverts).all() and np.array_equal(o[name], gverts)
        return ndc


_SIL_WS = [(e, "workspace") for e in ("hm_sil_fwd", "hm_sil_reduce", "hm_sil_bwd", "hm_sil_read_idx_map", "hm_sil_read_parts",
                                      "hm_sil_read_faces9")]


@case()
def sil_plain():
    """the plain forward (pooled, pooled_depth) and the generic backward, mode 0, with grad_verts and grad_ndc"""
    s = _Sil()
    rr, B, S = s.rr, s.B, s.S
    gimg = rr.upstream("dense", B, S)
    pooled, depth = Out("pooled", (B, S, S)), Out("pooled_depth", (B, S, S))
    gv, gn = Out("grad_verts", (B, s.V, 3)), Out("grad_ndc", (B, s.V, 3))
    gin = In("grad_pooled", gimg.numpy())
    gin.align = 4                                                     # (mode 0 reads single floats; mode 3 is sil_noaa)
    steps = [s.fwd(pooled=pooled, depth=depth), s.read("faces9"), s.read("idx_map"),
             s.bwd(0, grad_pooled=gin, grad_verts=gv, grad_ndc=gn), s.read("parts")]

    def check(o):
        both, idx, dep = s.oracle(o)
        assert np.array_equal(o["pooled"], rr.pool_alpha(idx)) and np.array_equal(o["pooled_depth"], rr.pool_depth(dep))
        parts = rr.oracle_parts(both, idx, rr.sample_gradient_generic(gimg.numpy()), rr.EPS, 0)
        assert np.array_equal(o["parts"], parts) and np.count_nonzero(parts) > 40
        ndc = s.check_gather(o, parts)
        assert np.array_equal(o["grad_ndc"][..., :2], ndc[..., :2]) and not o["grad_ndc"][..., 2].any()
    return steps, check, [x for x in _SIL_WS if x[0] != "hm_sil_reduce"]


@case("batch", "shared")
def sil_fused(kind):
    """the fused pooled loss: forward with keep / ref / keep_sum / loss_out, hm_sil_reduce with frame_out, the backward in mode 1
    and again in mode 2 (positive upstream: the same bits); `shared`: mask_shared bit 0, one (S,S) mask for both frames"""
    from oracle import objchain
    from tests import util
    s = _Sil()
    rr, B, S = s.rr, s.B, s.S
    keep, ref = rr.fused_masks(s.sc)
    shared = kind == "shared"
    if shared:
        keep, ref = keep[0], ref[0]
    kb, rb = (keep.expand(B, S, S), ref.expand(B, S, S)) if shared else (keep, ref)
    keep_sum = kb.sum().reshape(1)
    weight = 3.0
    ksum, up = In("keep_sum", keep_sum.numpy()), In("upstream", np.array([weight], F32))
    pooled, loss = Out("pooled", (B, S, S)), Out("loss_out", (2,))
    gv1, gv2 = Out("grad_verts", (B, s.V, 3)), Out("grad_verts_mode2", (B, s.V, 3))
    kin, rin = In("keep", keep.numpy()), In("ref", ref.numpy())
    kin.align = rin.align = 4                                         # (the pooled mode reads single floats; float2 is sil_per_sample)
    steps = [s.fwd(keep=kin, ref=rin, keep_sum=ksum, pooled=pooled, loss_out=loss, mask_shared=int(shared)), s.read("faces9"),
             s.read("idx_map"),
             s.reduce(keep_sum=ksum, loss_out=Out("loss_again", (2,)), frame_out=Out("frame_out", (B, 2))),
             s.bwd(1, upstream=up, keep_sum=ksum, grad_verts=gv1), s.read("parts"),
             s.bwd(2, upstream=up, keep_sum=ksum, grad_verts=gv2)]

    def check(o):
        both, idx, _ = s.oracle(o)
        ga, pool = objchain.sample_gradient(idx, kb.numpy(), rb.numpy(), weight, F32(keep_sum.item()), B)
        assert np.array_equal(o["pooled"], pool)
        parts = rr.oracle_parts(both, idx, ga)
        assert np.count_nonzero(parts) > 40 and np.array_equal(o["parts"], parts)
        s.check_gather(o, parts)
        assert np.array_equal(bits(o["grad_verts_mode2"]), bits(o["grad_verts"]))
        want = rr.fused_loss_ref(pool, kb, rb, torch.float64)
        bar = util.E32_FACTOR * rr.E32_SIL_LOSS
        assert all(abs(float(g) - w) <= bar * abs(w) for g, w in zip(o["loss_out"], want))
        assert np.array_equal(bits(o["loss_again"]), bits(o["loss_out"]))
        img = kb.double() * torch.from_numpy(pool).double()
        sq = ((img - rb.double()) ** 2).sum((1, 2))
        iou = (img * rb.double()).sum((1, 2)) / ((img + rb.double()).clamp(0, 1).sum((1, 2)) + 1e-6)
        assert (np.abs(o["frame_out"][:, 0] - sq.numpy()) <= bar * sq.numpy()).all()
        assert (np.abs(o["frame_out"][:, 1] - iou.numpy()) <= bar * iou.numpy()).all()
    return steps, check, _SIL_WS


@case()
def sil_per_sample():
    """the per-sample loss: forward with alpha_full and one shared (2S,2S) keep / ref, per-frame sums from hm_sil_reduce, backward
    mode 4.  Binary masks and power-of-two upstreams: every product of the gradient is exact, whatever its order."""
    s = _Sil()
    rr, B, S = s.rr, s.B, s.S
    keep, ref = rr.fused_masks(s.sc)
    keep2, ref2 = (np.repeat(np.repeat(t[0].numpy(), 2, 0), 2, 1) for t in (keep, ref))
    up = np.array([2.0 ** -10, 2.0 ** -11], F32)
    alpha, pooled = Out("alpha_full", (B, 2 * S, 2 * S)), Out("pooled", (B, S, S))
    steps = [s.fwd(keep=In("keep", keep2), ref=In("ref", ref2), pooled=pooled, alpha_full=alpha, mask_shared=1), s.read("faces9"),
             s.read("idx_map"), s.reduce(frame_out=Out("frame_out", (B, 2))),
             s.bwd(4, upstream=In("upstream", up), grad_verts=Out("grad_verts", (B, s.V, 3))), s.read("parts")]

    def check(o):
        both, idx, _ = s.oracle(o)
        cover = (idx >= 0).astype(F32)[:, ::-1]
        assert np.array_equal(o["alpha_full"], cover) and np.array_equal(o["pooled"], rr.pool_alpha(idx))
        img = keep2[None] * cover
        sq, inter, union = ((img - ref2) ** 2).sum((1, 2)), (img * ref2).sum((1, 2)), np.clip(img + ref2, 0, 1).sum((1, 2))
        assert np.array_equal(o["frame_out"][:, 0], sq.astype(F32))                                  # counts: exact
        assert np.array_equal(o["frame_out"][:, 1], inter.astype(F32) / (union.astype(F32) + F32(1e-6)))
        g = (up[:, None, None] * F32(2.0)) * (keep2[None] * (img - ref2))                              # d sum_b / d alpha, output grid
        parts = rr.oracle_parts(both, idx, np.ascontiguousarray(g[:, ::-1], F32))
        assert np.count_nonzero(parts) > 40 and np.array_equal(o["parts"], parts)
        s.check_gather(o, parts)
    return steps, check, _SIL_WS + [("hm_sil_fwd", n) for n in ("keep", "ref", "alpha_full")]


@case()
def sil_noaa():
    """rendering without anti-aliasing: alpha_full alone, then the backward in mode 3 with a (B,2S,2S) upstream image"""
    s = _Sil()
    rr, B, S = s.rr, s.B, s.S
    gen = torch.Generator().manual_seed(9)
    gin = (torch.randn(B, 2 * S, 2 * S, generator=gen) * 2.0 ** -10).numpy()
    alpha, pooled = Out("alpha_full", (B, 2 * S, 2 * S)), Out("pooled", (B, S, S))
    steps = [s.fwd(pooled=pooled, alpha_full=alpha), s.read("faces9"), s.read("idx_map"),
             s.bwd(3, grad_pooled=In("grad_pooled", gin), grad_verts=Out("grad_verts", (B, s.V, 3))), s.read("parts")]

    def check(o):
        both, idx, _ = s.oracle(o)
        assert np.array_equal(o["alpha_full"], (idx >= 0).astype(F32)[:, ::-1])
        parts = rr.oracle_parts(both, idx, np.ascontiguousarray(gin[:, ::-1], F32))
        assert np.count_nonzero(parts) > 40 and np.array_equal(o["parts"], parts)
        s.check_gather(o, parts)
    return steps, check, [x for x in _SIL_WS if x[0] != "hm_sil_reduce"] + [("hm_sil_fwd", "alpha_full"), ("hm_sil_bwd", "grad_pooled")]


# =============================================================================================== the test
@pytest.mark.parametrize("name", sorted(CASES))
def test_contract(name):
    steps, check, expect_bad = CASES[name]()
    contract(steps, check, expect_bad)


def test_the_arena_sees_a_write_past_an_output_and_a_read_past_an_input():
    """the harness itself: hm_scale_by told that its arrays are one element longer than they are - inside the arena, so nothing
    faults - reads the NaN behind the input and puts it into the guard behind the output, and the placed run says where"""
    n = 65
    src = np.arange(n, dtype=F32)
    steps = [("hm_scale_by", [In("in", src), In("s", np.array([2.0], F32)), n + 1, Out("out", (n,)), None])]
    rcs, placed, where = run_placed(steps)
    assert rcs == [0] and np.array_equal(_view(placed["out"], steps[0][1][3]), 2 * src)
    assert where.startswith("4 bytes changed outside the outputs") and f"first at +{4 * n} from the start of `out`" in where, where
    steps[0][1][2] = n
    assert run_placed(steps)[2] == ""


def test_every_audited_entry_point_has_a_case():
    """every audited entry point is CALLED by some case (the cases are built here, not run), and every enforced row of an audited
    entry point is violated by some case's bad-argument leg"""
    called, legs = set(), set()
    for build in CASES.values():
        steps, _, expect_bad = build()
        called |= {entry for entry, _ in steps}
        legs |= set(expect_bad)
    assert set(mc.IN_SCOPE) <= called, set(mc.IN_SCOPE) - called
    want = {(e, p) for e, p, _, _ in mc.elevated_rows() if e in mc.IN_SCOPE}
    assert want <= legs, want - legs
