"""NumPy restatement of the observed-depth term of csrc/depthobs.hip (not product code, no device): the rule of
include/homan_amd.h / DESIGN.md section 7.

forward32 / backward32 follow the kernels operation by operation - fp32 residuals, rho and clamp; every addend rounded to the
grid 2^-32 in double and summed as an integer count of quanta (exact, so the order of the sum is immaterial); the double
conversions of the finishing workgroup - and are what the GPU tests hold the kernels to bit for bit.  reference64 is the closed
form in float64, from the same fp32 inputs."""
import numpy as np

F32, F64 = np.float32, np.float64
NEAR, FAR = 0.1, 100.0            # ops.NMR_NEAR / NMR_FAR
FIX = 4294967296.0                # 2^32: quanta per unit
U32 = 2.0 ** -24                  # unit roundoff of fp32 (round to nearest)


def valid_masks(depths, sils, masks, D, near=NEAR, far=FAR):
    """([valid (B,S,S) bool per layer], [seen = mask set and sensor value usable]) - comparisons on the fp32 inputs, NaN fails"""
    near, far = F32(near), F32(far)
    with np.errstate(invalid="ignore"):
        usable = (D >= near) & (D <= far)
        seen = [usable & (m != 0) for m in masks]
        valid = [s & (a == F32(1.0)) & (d >= F32(0.0)) & (d <= far) for s, a, d in zip(seen, sils, depths)]
    return valid, seen


def _quanta(x):
    return np.rint(x.astype(F64) * FIX).astype(np.int64)


def forward32(depths, sils, masks, D, delta, near=NEAR, far=FAR):
    """depths / sils: L x (B,S,S) fp32, masks: L x (B,S,S) uint8, D (B,S,S) fp32 -> dict(loss, mae, share, N fp32 scalars;
    records (L,B,2) fp32; clamped: L x (B,S,S) fp32; n (L,B) int)"""
    delta, half = F32(delta), F32(0.5)
    depths = [np.asarray(d, F32) for d in depths]
    D = np.asarray(D, F32)
    L, B = len(depths), D.shape[0]
    valid, seen = valid_masks(depths, sils, masks, D, near, far)
    records, clamped = np.zeros((L, B, 2), F32), []
    n_all = np.zeros((L, B), np.int64)
    npos = sum_m = hi = lo = sum_n = sum_seen = 0
    for l in range(L):
        v = valid[l]
        with np.errstate(invalid="ignore", over="ignore"):
            r = np.where(v, depths[l] - D, F32(0.0)).astype(F32)
        ar = np.abs(r)
        rho = np.where(ar <= delta, (half * r) * r, delta * (ar - half * delta)).astype(F32)
        clamped.append(np.where(v, np.minimum(np.maximum(r, -delta), delta), F32(0.0)).astype(F32))
        q_rho, q_abs = np.where(v, _quanta(rho), 0), np.where(v, _quanta(ar), 0)
        for b in range(B):
            n, q1, q2 = int(v[b].sum()), int(q_rho[b].sum()), int(q_abs[b].sum())
            n_all[l, b] = n
            records[l, b] = F32(n), F32(float(q1) / FIX)
            if n:
                npos += 1
                sum_m += int(np.rint(float(q1) / float(n)))
            hi, lo = hi + (q2 >> 32), lo + (q2 & 0xffffffff)
            sum_n += n
            sum_seen += int(seen[l][b].sum())
    loss = F32((float(sum_m) / FIX) / float(npos)) if npos else F32(0.0)
    mae = F32(((float(hi) * FIX + float(lo)) / FIX) / float(sum_n)) if sum_n else F32(0.0)
    share = F32(float(sum_n) / float(sum_seen)) if sum_seen else F32(0.0)
    return dict(loss=loss, mae=mae, share=share, N=F32(npos), records=records, clamped=clamped, n=n_all)


def backward32(fwd, upstream=1.0):
    """-> (L x (B,S,S) fp32 gradient images, L x flags (B,S,S//64) uint8 or None when S % 64 != 0)"""
    grads, flags = [], []
    for l, c in enumerate(fwd["clamped"]):
        B, S = c.shape[:2]
        n = fwd["records"][l, :, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(n > 0, (F32(upstream) / fwd["N"]) / n, F32(0.0)).astype(F32)
        g = np.where(c != 0, c * w[:, None, None], F32(0.0)).astype(F32)
        grads.append(g)
        flags.append((g.reshape(B, S, S // 64, 64) != 0).any(-1).astype(np.uint8) if S % 64 == 0 else None)
    return grads, flags


def reference64(depths, sils, masks, D, delta, upstream=1.0, near=NEAR, far=FAR):
    """the closed form in float64 -> dict(loss, mae, share, grads: L x (B,S,S) float64)"""
    L, B = len(depths), D.shape[0]
    valid, seen = valid_masks([np.asarray(d, F32) for d in depths], sils, masks, np.asarray(D, F32), near, far)
    delta = float(F32(delta))
    means, grads, abs_sum, n_sum = [], [], 0.0, 0
    n_lb = np.zeros((L, B))
    res = []
    for l in range(L):
        r = np.where(valid[l], np.asarray(depths[l], F64) - np.asarray(D, F64), 0.0)
        res.append(r)
        rho = np.where(np.abs(r) <= delta, 0.5 * r * r, delta * (np.abs(r) - 0.5 * delta))
        for b in range(B):
            n = int(valid[l][b].sum())
            n_lb[l, b] = n
            if n:
                means.append(rho[b][valid[l][b]].sum() / n)
            abs_sum += np.abs(r[b][valid[l][b]]).sum()
            n_sum += n
    N = len(means)
    for l in range(L):
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(n_lb[l] > 0, float(upstream) / (n_lb[l] * max(N, 1)), 0.0)
        grads.append(np.where(valid[l], np.clip(res[l], -delta, delta) * w[:, None, None], 0.0))
    n_seen = sum(int(s.sum()) for s in seen)
    return dict(loss=sum(means) / N if N else 0.0, mae=abs_sum / n_sum if n_sum else 0.0,
                share=n_sum / n_seen if n_seen else 0.0, grads=grads, N=N)


def random_case(B, S, L, delta, seed=0, empty_layer_frame=True, empty_clip=False, rows=None):
    """Random layers holding every input class the rule names: sensor values NaN / +inf / negative / 0 / below near / above far;
    silhouette 1 with mask 0; mask set with silhouette < 1; residuals at exactly +-delta; with empty_layer_frame one (layer,
    frame) without a valid pixel; with empty_clip none anywhere; rows = (lo, hi): the random part of the masks covers those pixel
    rows only (a mask covers a small part of an image: most 64-pixel segments then hold no gradient).  -> (depths, sils, masks, D)"""
    rng = np.random.default_rng(seed)
    delta = F32(delta)
    D = rng.uniform(0.3, 1.5, (B, S, S)).astype(F32)
    flat = D.reshape(-1)
    bad = rng.choice(flat.size, 12, replace=False)
    flat[bad] = np.array([np.nan, np.inf, -0.5, 0.0, 0.05, 150.0] * 2, F32)
    depths, sils, masks = [], [], []
    for l in range(L):
        d = (D + rng.normal(0, 2.0 * float(delta), D.shape)).astype(F32)
        d[~np.isfinite(d)] = F32(1.0)
        d = np.clip(d, F32(0.11), F32(99.0)).astype(F32)
        a = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], F32), D.shape, p=[0.2, 0.05, 0.1, 0.05, 0.6]).astype(F32)
        m = (rng.uniform(size=D.shape) < 0.6).astype(np.uint8) * rng.integers(1, 256, D.shape).astype(np.uint8)
        if rows is not None:
            m[:, :rows[0]], m[:, rows[1]:] = 0, 0
        # residuals at exactly +-delta on pixels made valid: D + delta must be exact in fp32, so D is put on a coarse grid there
        for k, sign in enumerate((1.0, -1.0)):
            b, y, x = 0, (3 + 5 * l) % S, (1 + 2 * k) % S
            D[b, y, x] = F32(0.75)
            d[b, y, x] = F32(0.75) + F32(sign) * delta
            a[b, y, x], m[b, y, x] = F32(1.0), 7
        a[0, 0, :4], m[0, 0, :4] = F32(1.0), 0            # silhouette 1, mask 0
        a[0, 1, :4], m[0, 1, :4] = F32(0.75), 9           # mask set, silhouette < 1
        depths.append(d); sils.append(a); masks.append(m)
    if empty_layer_frame:
        masks[L - 1][B - 1] = 0
    if empty_clip:
        for a in sils:
            a[a == 1.0] = F32(0.75)
    return depths, sils, masks, D
