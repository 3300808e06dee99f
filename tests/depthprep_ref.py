"""NumPy restatement of the depth registration of csrc/depthprep.hip (not product code, no device): the rule of
include/homan_amd.h / DESIGN.md section 7.

register32 follows the kernels operation by operation in fp32 - validity, the edge filter on the source grid, the two corners and
the centre of every surviving pixel through Kd, T and Kc, the clipped footprint, the minimum over bit patterns - and is what the
GPU tests hold the kernels to bit for bit, statistics included.  project64 is the same geometry in float64 for arbitrary source
coordinates: the known answers of tests/test_depthprep.py and the analytic scenes of tests/test_depthprep_gpu.py rest on it."""
import numpy as np

F32, F64 = np.float32, np.float64
NEAR, FAR = 0.1, 100.0            # ops.NMR_NEAR / NMR_FAR
INF_BITS = np.uint32(0x7f800000)
PX_MAX = F32(16777216.0)


def _frame_matrix(M, b, shape):
    M = np.asarray(M, F32)
    return (M[b] if M.ndim == 3 else M).reshape(shape)


def register32(frames, scale, Kd, T, Kc, S, znear=NEAR, zfar=FAR, edge_radius=1, edge_jump_abs=0.02, edge_jump_rel=0.0,
               max_splat=8):
    """frames (B,Hd,Wd) uint16 / float32, Kd (3,3) | (B,3,3) pixels, T (3,4) | (B,3,4), Kc (3,3) | (B,3,3) normalised ->
    (maps (B,S,S) float32, stats (B,4) int32)"""
    frames = np.asarray(frames)
    assert frames.dtype in (np.uint16, np.float32) and frames.ndim == 3
    B, Hd, Wd = frames.shape
    near, far, r = F32(znear), F32(zfar), int(edge_radius)
    out = np.zeros((B, S, S), F32)
    stats = np.zeros((B, 4), np.int32)
    half, Sf = F32(0.5), F32(S)
    for b in range(B):
        kd, t, kc = _frame_matrix(Kd, b, (3, 3)), _frame_matrix(T, b, (3, 4)).reshape(-1), _frame_matrix(Kc, b, (3, 3))
        with np.errstate(all="ignore"):
            z = frames[b].astype(F32) * F32(scale)
            valid = (z >= near) & (z <= far)
            z = np.where(valid, z, F32(0.0)).astype(F32)
            thr = F32(edge_jump_rel) * z + F32(edge_jump_abs)
            pad = np.pad(z, r)
            edge = np.zeros_like(valid)
            for dy in range(2 * r + 1):
                for dx in range(2 * r + 1):
                    zn = pad[dy:dy + Hd, dx:dx + Wd]
                    edge |= (zn != 0) & (np.abs(zn - z) > thr)
            edge &= valid
            keep = valid & ~edge
            v, u = np.nonzero(keep)
            zk = z[keep]
            fxd, cxd, fyd, cyd = kd[0, 0], kd[0, 2], kd[1, 1], kd[1, 2]
            Fx, Cx, Fy, Cy = kc[0, 0] * Sf, kc[0, 2] * Sf, kc[1, 1] * Sf, kc[1, 2] * Sf

            def camera(p, q):
                X, Y = ((p - cxd) / fxd) * zk, ((q - cyd) / fyd) * zk
                return (((t[0] * X + t[1] * Y) + t[2] * zk) + t[3], ((t[4] * X + t[5] * Y) + t[6] * zk) + t[7],
                        ((t[8] * X + t[9] * Y) + t[10] * zk) + t[11])
            u0, v0 = u.astype(F32), v.astype(F32)
            Xc0, Yc0, Zc0 = camera(u0, v0)
            Xc1, Yc1, Zc1 = camera((u + 1).astype(F32), (v + 1).astype(F32))
            _, _, zc = camera(u0 + half, v0 + half)
            ok = (zc >= near) & (zc <= far) & (Zc0 >= near) & (Zc1 >= near)
            px0, py0 = (Xc0 / Zc0) * Fx + Cx, (Yc0 / Zc0) * Fy + Cy
            px1, py1 = (Xc1 / Zc1) * Fx + Cx, (Yc1 / Zc1) * Fy + Cy
            ok &= (np.abs(px0) <= PX_MAX) & (np.abs(px1) <= PX_MAX) & (np.abs(py0) <= PX_MAX) & (np.abs(py1) <= PX_MAX)
            dropped = int((~ok).sum())
            px0, px1, py0, py1, zc = px0[ok], px1[ok], py0[ok], py1[ok], zc[ok]
            xa, xb, ya, yb = np.minimum(px0, px1), np.maximum(px0, px1), np.minimum(py0, py1), np.maximum(py0, py1)
            c0 = np.maximum(np.ceil(xa - half), F32(0.0)).astype(np.int64)
            c1 = np.minimum(np.ceil(xb - half), Sf).astype(np.int64)
            r0 = np.maximum(np.ceil(ya - half), F32(0.0)).astype(np.int64)
            r1 = np.minimum(np.ceil(yb - half), Sf).astype(np.int64)
        empty = (c1 <= c0) | (r1 <= r0)
        big = ~empty & ((c1 - c0 > max_splat) | (r1 - r0 > max_splat))
        dropped += int(big.sum())
        w = ~empty & ~big
        c0, c1, r0, r1 = c0[w], c1[w], r0[w], r1[w]
        bits = np.ascontiguousarray(zc[w]).view(np.uint32)
        buf = np.full(S * S, INF_BITS, np.uint32)
        for dy in range(int((r1 - r0).max()) if len(bits) else 0):
            for dx in range(int((c1 - c0).max())):
                m = (r0 + dy < r1) & (c0 + dx < c1)
                np.minimum.at(buf, ((r0 + dy) * S + c0 + dx)[m], bits[m])
        buf[buf == INF_BITS] = 0
        out[b] = buf.view(F32).reshape(S, S)
        stats[b] = int(valid.sum()), int(edge.sum()), dropped, int((buf != 0).sum())
    return out, stats


def project64(u, v, z, Kd, T, Kc, S):
    """source coordinates (u, v) in the units of Kd, depth z along the depth camera's axis -> (px, py, zc): target pixel
    coordinates under the normalised Kc at size S and the depth in the colour camera, float64"""
    Kd, T, Kc = np.asarray(Kd, F64), np.asarray(T, F64).reshape(3, 4), np.asarray(Kc, F64)
    u, v, z = np.broadcast_arrays(np.asarray(u, F64), np.asarray(v, F64), np.asarray(z, F64))
    P = np.stack([(u - Kd[0, 2]) / Kd[0, 0] * z, (v - Kd[1, 2]) / Kd[1, 1] * z, z, np.ones_like(z)], -1) @ T.T
    return (P[..., 0] / P[..., 2] * Kc[0, 0] * S + Kc[0, 2] * S, P[..., 1] / P[..., 2] * Kc[1, 1] * S + Kc[1, 2] * S, P[..., 2])


def intrinsics(f, cx, cy, fy=None):
    return np.array([[f, 0, cx], [0, f if fy is None else fy, cy], [0, 0, 1]], F64)


IDENTITY = np.eye(3, 4)


def scaled_cameras(Hd, Wd, S, ratio, offset=(0.47, 0.53)):
    """(Kd pixels, Kc normalised) of one pinhole seen at two resolutions: one source pixel spans `ratio` target pixels, the
    source's principal point (its centre) lands at `offset` * S"""
    fd = 0.9 * max(Hd, Wd)
    return intrinsics(fd, Wd / 2.0, Hd / 2.0), intrinsics(ratio * fd / S, offset[0], offset[1])


def inside_source(Hd, Wd, S, Kd, Kc, margin=1e-3):
    """(S,S) bool: the target pixels whose centre falls inside the source frame [0, Wd) x [0, Hd) with T = identity (any depth),
    at least `margin` source pixels off its border (float64)"""
    c = np.arange(S) + 0.5
    u = (c / S - Kc[0, 2]) / Kc[0, 0] * Kd[0, 0] + Kd[0, 2]
    v = (c / S - Kc[1, 2]) / Kc[1, 1] * Kd[1, 1] + Kd[1, 2]
    return ((v >= margin) & (v <= Hd - margin))[:, None] & ((u >= margin) & (u <= Wd - margin))[None, :]


TILING_CASES = [  # (Hd, Wd, S, ratio): the source overhangs the target on some sides and ends inside it on others
    (30, 44, 16, 0.4), (20, 28, 24, 1.0), (9, 12, 32, 2.5), (5, 6, 48, 7.9)]
