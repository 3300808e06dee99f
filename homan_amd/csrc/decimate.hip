// decimate.hip -- mesh preparation, second stage: a closed, oriented triangle mesh brought down to a vertex budget by quadric edge
// collapses in deterministic parallel rounds, behind ops.collapse_round / ops.decimate_mesh and meshprep.decimate /
// make_watertight_detail.  With csrc/remesh.hip at a fine lattice it stands in for the reference's external
// ManifoldPlus + ACVD stage (meshprocess/simplifymesh.py); the rules are in include/homan_amd.h and DESIGN.md section 7, pinned bit
// for bit by the NumPy restatement of tests/decimate_ref.py.  Floating point: doubles formed from the fp32 coordinates, one IEEE add
// or multiply at a time (no division, no sqrt, no contraction, no floating-point atomic).
//
// A round is six entry points with a sort or a scan of the caller's between them (plumbing: any stable sort, any inclusive scan):
//   k_dc_keys        a thread per corner: the half-edge key (u n + w) n + c and the corner key u 3m + corner.        [sort both]
//   k_dc_offsets     a thread per sorted half-edge: where a vertex's run starts, and whether u < w (an edge).         [scan the flags]
//   k_dc_quadric     a thread per vertex: its faces' quadrics, gathered in ascending face index.
//   k_dc_edges       a thread per sorted half-edge with u < w: the edge record, the three candidates' errors, the cost, the link
//                    condition by a merge of the two sorted neighbour runs, the flip test over both corner runs, the sort keys.
//                                                                                                     [stable sort by l2, then by cost]
//   k_dc_rank        rank[order[i]] = i for the valid edges; clears m1 and the selection flags.
//   k_dc_m1          a thread per edge: integer atomicMin of its rank into both endpoints (order-independent).
//   k_dc_m2          a thread per vertex: the minimum over its closed neighbourhood.
//   k_dc_select      a thread per edge: selected iff m2[a] == m2[b] == rank; the flag also lands at position rank.   [scan the flags]
//   k_dc_mark        a thread per edge: the budget (the `need` lowest ranks), then remap[b] = a, keep[b] = 0, moved[a] = e.
//   k_dc_face_keep   a thread per face: kept unless two corners now name one vertex.                                [scan both keeps]
//   k_dc_compact_v / k_dc_compact_f   a thread per vertex / face: the survivors at their scanned places, within the capacities.
// Every hand-off is a kernel boundary on the stream; nothing is allocated; nothing is read back.
#include "hm_common.h"

#define DC_THREADS 256
#define DC_MAX_VERTS (1 << 20)           // (u n + w) n + c < 2^60
#define DC_MAX_FACES (1 << 22)           // u 3m + corner < 2^44
#define DC_RANK_NONE 0x7fffffff

typedef long long dc_key;

struct DcVec { double x, y, z; };

__device__ __forceinline__ DcVec dc_load(const float* __restrict__ V, int v)
{
    DcVec p = {(double)V[3 * (long)v], (double)V[3 * (long)v + 1], (double)V[3 * (long)v + 2]};
    return p;
}
// rule 1: N = (b - a) x (c - a)
__device__ __forceinline__ DcVec dc_normal(const DcVec& a, const DcVec& b, const DcVec& c)
{
    const double e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z, e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
    DcVec n = {e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x};
    return n;
}
// rule 4: the quadric form in its one written-out order
__device__ __forceinline__ double dc_form(const double* q, const DcVec& p)
{
    double s = (q[0] * p.x) * p.x + (q[3] * p.y) * p.y;
    s = s + (q[5] * p.z) * p.z;
    s = s + 2.0 * ((q[1] * p.x) * p.y);
    s = s + 2.0 * ((q[2] * p.x) * p.z);
    s = s + 2.0 * ((q[4] * p.y) * p.z);
    s = s + 2.0 * (q[6] * p.x);
    s = s + 2.0 * (q[7] * p.y);
    s = s + 2.0 * (q[8] * p.z);
    return s + q[9];
}
// a double's bits as a signed integer of the same order (no -0.0 and no NaN reaches it)
__device__ __forceinline__ dc_key dc_ordered(double x)
{
    const dc_key b = __double_as_longlong(x);
    return b < 0 ? b ^ 0x7fffffffffffffffLL : b;
}
__device__ __forceinline__ void dc_candidate(const float* __restrict__ V, int a, int b, int choice, float* p)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float pa = V[3 * (long)a + k], pb = V[3 * (long)b + k];
        p[k] = choice == 0 ? pa : choice == 1 ? pb : (pa + pb) * 0.5f;
    }
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_keys(const int* __restrict__ F, int n, int m, dc_key* __restrict__ he,
                                                         dc_key* __restrict__ ck)
{
    const long t = (long)blockIdx.x * DC_THREADS + threadIdx.x, corners = 3L * m;
    if (t >= corners) return;
    const long f = t / 3;
    const int k = (int)(t % 3);
    const dc_key u = F[t], w = F[3 * f + (k + 1) % 3], c = F[3 * f + (k + 2) % 3];
    he[t] = (u * n + w) * n + c;
    ck[t] = u * corners + t;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_offsets(const dc_key* __restrict__ he, int n, int m, int* __restrict__ voff,
                                                            int* __restrict__ is_edge)
{
    const long t = (long)blockIdx.x * DC_THREADS + threadIdx.x, corners = 3L * m, nn = (long)n * n;
    if (t >= corners) return;
    const dc_key key = he[t];
    long u = key / nn;
    const long w = (key / n) % n;
    u = u < 0 ? 0 : u >= n ? n - 1 : u;                                    // (a mesh outside the contract cannot steer a store)
    long from = 0;
    if (t > 0) {
        long up = he[t - 1] / nn;
        up = up < 0 ? 0 : up >= n ? n - 1 : up;
        from = up + 1;
    }
    for (long v = from; v <= u; ++v) voff[v] = (int)t;                     // (one vertex, unless some are named by no face)
    if (t == corners - 1)
        for (long v = u + 1; v <= n; ++v) voff[v] = (int)corners;
    is_edge[t] = u < w ? 1 : 0;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_quadric(const float* __restrict__ V, const int* __restrict__ F,
                                                            const dc_key* __restrict__ ck, const int* __restrict__ voff, int n, int m,
                                                            double* __restrict__ Q)
{
    const int v = blockIdx.x * DC_THREADS + threadIdx.x;
    if (v >= n) return;
    const long corners = 3L * m;
    double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = voff[v]; i < voff[v + 1]; ++i) {                          // ascending corner = ascending face index
        const long f = (ck[i] % corners) / 3;
        const DcVec a = dc_load(V, F[3 * f]), b = dc_load(V, F[3 * f + 1]), c = dc_load(V, F[3 * f + 2]);
        const DcVec N = dc_normal(a, b, c);
        const double d = -((N.x * a.x + N.y * a.y) + N.z * a.z);
        q[0] = q[0] + N.x * N.x; q[1] = q[1] + N.x * N.y; q[2] = q[2] + N.x * N.z; q[3] = q[3] + N.y * N.y;
        q[4] = q[4] + N.y * N.z; q[5] = q[5] + N.z * N.z; q[6] = q[6] + N.x * d; q[7] = q[7] + N.y * d;
        q[8] = q[8] + N.z * d; q[9] = q[9] + d * d;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) Q[10 * (long)v + k] = q[k];
}

// rule 5, last item: every face at `end` that does not hold `other`, with its corner at `end` moved to p, keeps N_old . N_new > 0
__device__ __forceinline__ bool dc_no_flip(const float* __restrict__ V, const int* __restrict__ F, const dc_key* __restrict__ ck,
                                           const int* __restrict__ voff, long corners, int end, int other, const DcVec& p)
{
    for (int i = voff[end]; i < voff[end + 1]; ++i) {
        const long corner = ck[i] % corners, f = corner / 3;
        const int k = (int)(corner % 3);
        const int i0 = F[3 * f], i1 = F[3 * f + 1], i2 = F[3 * f + 2];
        if (i0 == other || i1 == other || i2 == other) continue;
        const DcVec a = dc_load(V, i0), b = dc_load(V, i1), c = dc_load(V, i2);
        const DcVec No = dc_normal(a, b, c);
        const DcVec Nn = dc_normal(k == 0 ? p : a, k == 1 ? p : b, k == 2 ? p : c);
        const double dot = (No.x * Nn.x + No.y * Nn.y) + No.z * Nn.z;
        if (!(dot > 0.0)) return false;
    }
    return true;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_edges(const float* __restrict__ V, const int* __restrict__ F,
                                                          const dc_key* __restrict__ he, const dc_key* __restrict__ ck,
                                                          const int* __restrict__ voff, const int* __restrict__ edge_scan, int n, int m,
                                                          float regularity, const double* __restrict__ Q, int* __restrict__ edges,
                                                          int* __restrict__ choice_out, double* __restrict__ cost_out,
                                                          double* __restrict__ l2_out, int* __restrict__ valid_out,
                                                          dc_key* __restrict__ cost_key, dc_key* __restrict__ l2_key)
{
    const long t = (long)blockIdx.x * DC_THREADS + threadIdx.x, corners = 3L * m;
    if (t >= corners) return;
    const dc_key key = he[t];
    const long pair = key / n;
    const int a = (int)(pair / n), b = (int)(pair % n), c = (int)(key % n);
    if (a >= b) return;
    const long e = (long)edge_scan[t] - 1, E = corners / 2;
    if (a < 0 || e < 0 || e >= E) return;                                  // (outside the contract: nothing is stored out of range)
    // the face across: the half-edge b -> a, by bisection in b's run
    int d = -1;
    {
        const dc_key want = (dc_key)b * n + a;
        int lo = voff[b], hi = voff[b + 1];
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (he[mid] / n < want) lo = mid + 1; else hi = mid;
        }
        if (lo < voff[b + 1] && he[lo] / n == want) d = (int)(he[lo] % n);
    }
    double q[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) q[k] = Q[10 * (long)a + k] + Q[10 * (long)b + k];
    float cand[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) dc_candidate(V, a, b, k, cand[k]);
    int choice = 0;
    double err = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const DcVec p = {(double)cand[k][0], (double)cand[k][1], (double)cand[k][2]};
        const double ek = dc_form(q, p);
        if (k == 0 || ek < err) { err = ek; choice = k; }
    }
    const DcVec pa = dc_load(V, a), pb = dc_load(V, b);
    const double dx = pb.x - pa.x, dy = pb.y - pa.y, dz = pb.z - pa.z;
    const double l2 = (dx * dx + dy * dy) + dz * dz;
    const double cost = err + (double)regularity * ((l2 * l2) * l2);
    bool valid = (cost - cost == 0.0) && m > 4 && d >= 0;
    if (valid) valid = voff[c + 1] - voff[c] > 3 && voff[d + 1] - voff[d] > 3;
    if (valid) {                                                           // the link condition: a merge of two ascending runs
        int i = voff[a], j = voff[b], common = 0;
        const int ie = voff[a + 1], je = voff[b + 1];
        while (i < ie && j < je) {
            const long x = (he[i] / n) % n, y = (he[j] / n) % n;
            common += x == y;
            i += x <= y;
            j += y <= x;
        }
        valid = common == 2;
    }
    if (valid) {
        const DcVec p = {(double)cand[choice][0], (double)cand[choice][1], (double)cand[choice][2]};
        valid = dc_no_flip(V, F, ck, voff, corners, a, b, p) && dc_no_flip(V, F, ck, voff, corners, b, a, p);
    }
    edges[4 * e] = a; edges[4 * e + 1] = b; edges[4 * e + 2] = c; edges[4 * e + 3] = d;
    choice_out[e] = choice;
    cost_out[e] = cost;
    l2_out[e] = l2;
    valid_out[e] = valid ? 1 : 0;
    cost_key[e] = valid ? dc_ordered(cost) : 0x7fffffffffffffffLL;
    l2_key[e] = valid ? __double_as_longlong(l2) : 0x7fffffffffffffffLL;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_rank(const dc_key* __restrict__ order, const int* __restrict__ valid, int n, long E,
                                                         int* __restrict__ rank, int* __restrict__ m1, int* __restrict__ sel_by_rank)
{
    const long t = (long)blockIdx.x * DC_THREADS + threadIdx.x;
    if (t < n) m1[t] = DC_RANK_NONE;
    if (t >= E) return;
    sel_by_rank[t] = 0;
    const dc_key e = order[t];
    if (e < 0 || e >= E) return;
    rank[e] = valid[e] ? (int)t : DC_RANK_NONE;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_m1(const int* __restrict__ edges, const int* __restrict__ rank, long E,
                                                       int* __restrict__ m1)
{
    const long e = (long)blockIdx.x * DC_THREADS + threadIdx.x;
    if (e >= E) return;
    const int r = rank[e];
    if (r == DC_RANK_NONE) return;
    atomicMin(&m1[edges[4 * e]], r);
    atomicMin(&m1[edges[4 * e + 1]], r);
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_m2(const dc_key* __restrict__ he, const int* __restrict__ voff,
                                                       const int* __restrict__ m1, int n, int* __restrict__ m2)
{
    const int v = blockIdx.x * DC_THREADS + threadIdx.x;
    if (v >= n) return;
    int least = m1[v];
    for (int i = voff[v]; i < voff[v + 1]; ++i) least = min(least, m1[(he[i] / n) % n]);
    m2[v] = least;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_select(const int* __restrict__ edges, const int* __restrict__ rank,
                                                           const int* __restrict__ m2, int n, long E, int* __restrict__ selected,
                                                           int* __restrict__ sel_by_rank, int* __restrict__ remap,
                                                           int* __restrict__ vkeep, int* __restrict__ moved)
{
    const long t = (long)blockIdx.x * DC_THREADS + threadIdx.x;
    if (t < n) { remap[t] = (int)t; vkeep[t] = 1; moved[t] = -1; }
    if (t >= E) return;
    const int r = rank[t];
    const bool sel = r != DC_RANK_NONE && m2[edges[4 * t]] == r && m2[edges[4 * t + 1]] == r;
    selected[t] = sel ? 1 : 0;
    if (sel && r < E) sel_by_rank[r] = 1;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_mark(const int* __restrict__ edges, const int* __restrict__ rank,
                                                         const int* __restrict__ sel_scan, int need, long E, int* __restrict__ selected,
                                                         int* __restrict__ remap, int* __restrict__ vkeep, int* __restrict__ moved)
{
    const long e = (long)blockIdx.x * DC_THREADS + threadIdx.x;
    if (e >= E || !selected[e]) return;
    const int r = rank[e];
    if (r < 0 || r >= E || sel_scan[r] > need) { selected[e] = 0; return; }    // rule 8: the `need` lowest ranks stay
    const int a = edges[4 * e], b = edges[4 * e + 1];
    remap[b] = a;
    vkeep[b] = 0;
    moved[a] = (int)e;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_face_keep(const int* __restrict__ F, const int* __restrict__ remap, int m,
                                                              int* __restrict__ fkeep)
{
    const int f = blockIdx.x * DC_THREADS + threadIdx.x;
    if (f >= m) return;
    const int a = remap[F[3 * (long)f]], b = remap[F[3 * (long)f + 1]], c = remap[F[3 * (long)f + 2]];
    fkeep[f] = (a != b && b != c && c != a) ? 1 : 0;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_compact_v(const float* __restrict__ V, const int* __restrict__ edges,
                                                              const int* __restrict__ choice, const int* __restrict__ moved,
                                                              const int* __restrict__ vkeep, const int* __restrict__ vscan, int n,
                                                              int max_vertices, float* __restrict__ out)
{
    const int v = blockIdx.x * DC_THREADS + threadIdx.x;
    if (v >= n || !vkeep[v]) return;
    const int at = vscan[v] - 1;
    if (at < 0 || at >= max_vertices) return;
    float p[3] = {V[3 * (long)v], V[3 * (long)v + 1], V[3 * (long)v + 2]};
    const int e = moved[v];
    if (e >= 0) dc_candidate(V, edges[4 * (long)e], edges[4 * (long)e + 1], choice[e], p);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * (long)at + k] = p[k];
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_compact_f(const int* __restrict__ F, const int* __restrict__ remap,
                                                              const int* __restrict__ vscan, const int* __restrict__ fkeep,
                                                              const int* __restrict__ fscan, int m, int max_faces, int* __restrict__ out)
{
    const int f = blockIdx.x * DC_THREADS + threadIdx.x;
    if (f >= m || !fkeep[f]) return;
    const int at = fscan[f] - 1;
    if (at < 0 || at >= max_faces) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * (long)at + k] = vscan[remap[F[3 * (long)f + k]]] - 1;
}

static inline bool dc_sizes_ok(int n, int m)
{
    return n >= 4 && n <= DC_MAX_VERTS && m >= 4 && m <= DC_MAX_FACES && m % 2 == 0;
}
#define DC_LAUNCH(kernel, items, ...) \
    hipLaunchKernelGGL(kernel, dim3(hm_cdiv((items), DC_THREADS)), dim3(DC_THREADS), 0, stream, __VA_ARGS__)

extern "C" {
int hm_decimate_keys(const int* faces, int n, int m, void* he_keys, void* corner_keys, hipStream_t stream)
{
    HM_CHECK_ARG(faces && he_keys && corner_keys && dc_sizes_ok(n, m));
    HM_CHECK_ARG(HM_ALIGNED(he_keys, 8) && HM_ALIGNED(corner_keys, 8));
    DC_LAUNCH(k_dc_keys, 3L * m, faces, n, m, (dc_key*)he_keys, (dc_key*)corner_keys);
    return hm_launch_status();
}

int hm_decimate_offsets(const void* he_sorted, int n, int m, int* vertex_offsets, int* is_edge, hipStream_t stream)
{
    HM_CHECK_ARG(he_sorted && vertex_offsets && is_edge && dc_sizes_ok(n, m) && HM_ALIGNED(he_sorted, 8));
    DC_LAUNCH(k_dc_offsets, 3L * m, (const dc_key*)he_sorted, n, m, vertex_offsets, is_edge);
    return hm_launch_status();
}

int hm_decimate_costs(const float* verts, const int* faces, const void* he_sorted, const void* corner_sorted,
                      const int* vertex_offsets, const int* edge_scan, int n, int m, float regularity, double* quadrics, int* edges,
                      int* choice, double* cost, double* l2, int* valid, void* cost_keys, void* l2_keys, hipStream_t stream)
{
    HM_CHECK_ARG(verts && faces && he_sorted && corner_sorted && vertex_offsets && edge_scan && dc_sizes_ok(n, m));
    HM_CHECK_ARG(quadrics && edges && choice && cost && l2 && valid && cost_keys && l2_keys);
    HM_CHECK_ARG(HM_ALIGNED(he_sorted, 8) && HM_ALIGNED(corner_sorted, 8) && HM_ALIGNED(cost_keys, 8) && HM_ALIGNED(l2_keys, 8));
    HM_CHECK_ARG(regularity - regularity == 0.f && regularity >= 0.f);
    DC_LAUNCH(k_dc_quadric, n, verts, faces, (const dc_key*)corner_sorted, vertex_offsets, n, m, quadrics);
    DC_LAUNCH(k_dc_edges, 3L * m, verts, faces, (const dc_key*)he_sorted, (const dc_key*)corner_sorted, vertex_offsets, edge_scan, n, m,
              regularity, (const double*)quadrics, edges, choice, cost, l2, valid, (dc_key*)cost_keys, (dc_key*)l2_keys);
    return hm_launch_status();
}

int hm_decimate_select(const int* edges, const int* valid, const void* order, const void* he_sorted, const int* vertex_offsets, int n,
                       int m, int* rank, int* m1, int* m2, int* selected, int* selected_by_rank, int* remap, int* vertex_keep,
                       int* moved, hipStream_t stream)
{
    HM_CHECK_ARG(edges && valid && order && he_sorted && vertex_offsets && dc_sizes_ok(n, m));
    HM_CHECK_ARG(rank && m1 && m2 && selected && selected_by_rank && remap && vertex_keep && moved);
    HM_CHECK_ARG(HM_ALIGNED(order, 8) && HM_ALIGNED(he_sorted, 8));
    const long E = 3L * m / 2, most = E > n ? E : n;
    DC_LAUNCH(k_dc_rank, most, (const dc_key*)order, valid, n, E, rank, m1, selected_by_rank);
    DC_LAUNCH(k_dc_m1, E, edges, (const int*)rank, E, m1);
    DC_LAUNCH(k_dc_m2, n, (const dc_key*)he_sorted, vertex_offsets, (const int*)m1, n, m2);
    DC_LAUNCH(k_dc_select, most, edges, (const int*)rank, (const int*)m2, n, E, selected, selected_by_rank, remap, vertex_keep, moved);
    return hm_launch_status();
}

int hm_decimate_mark(const int* faces, const int* edges, const int* rank, const int* selected_scan, int need, int n, int m,
                     int* selected, int* remap, int* vertex_keep, int* moved, int* face_keep, hipStream_t stream)
{
    HM_CHECK_ARG(faces && edges && rank && selected_scan && dc_sizes_ok(n, m) && need >= 0);
    HM_CHECK_ARG(selected && remap && vertex_keep && moved && face_keep);
    const long E = 3L * m / 2;
    DC_LAUNCH(k_dc_mark, E, edges, rank, selected_scan, need, E, selected, remap, vertex_keep, moved);
    DC_LAUNCH(k_dc_face_keep, m, faces, (const int*)remap, m, face_keep);
    return hm_launch_status();
}

int hm_decimate_compact(const float* verts, const int* faces, const int* edges, const int* choice, const int* remap, const int* moved,
                        const int* vertex_keep, const int* vertex_scan, const int* face_keep, const int* face_scan, int n, int m,
                        int max_vertices, int max_faces, float* out_verts, int* out_faces, hipStream_t stream)
{
    HM_CHECK_ARG(verts && faces && edges && choice && remap && moved && vertex_keep && vertex_scan && face_keep && face_scan);
    HM_CHECK_ARG(dc_sizes_ok(n, m) && max_vertices >= 0 && max_faces >= 0);
    HM_CHECK_ARG((out_verts || max_vertices == 0) && (out_faces || max_faces == 0));
    if (max_vertices > 0) DC_LAUNCH(k_dc_compact_v, n, verts, edges, choice, moved, vertex_keep, vertex_scan, n, max_vertices, out_verts);
    if (max_faces > 0) DC_LAUNCH(k_dc_compact_f, m, faces, remap, vertex_scan, face_keep, face_scan, m, max_faces, out_faces);
    return hm_launch_status();
}
}  // extern "C"
