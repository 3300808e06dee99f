// seqinterp.hip -- key-frame results interpolated over every frame of a sequence.
//
// Replaces the per-key Python walk of reference homan/eval/ho3devalutils.py:53-96 (interpolate_res) and the per-frame
// `.dot(camextr)[unorder_idxs].astype(np.float32)` of reference evalho3drecons.py:126-127,154-158 by one streaming launch:
// a workgroup owns 256 consecutive floats of one output frame, finds the frame's segment once (wave-uniform binary search
// over the key frames: scalar loads, no LDS) and blends the two keys with the reference's operations, one IEEE rounding
// each: d = e - s in fp32, w = i * (1 / n) in double (= np.linspace(0, 1, n + 1)[i]), v = s + d * w in double.
#include "hm_common.h"

#define KI_THREADS 256
#define KI_MAX_GRID_Y 65535

// grid (ceil(3 M / 256), frames of this launch); frame = f0 + blockIdx.y.  out (frame_nb, M, 3): element e of a frame is
// coordinate e % 3 of row e / 3, read from row gather[e / 3] (or e / 3) of the keys: the stores of a wave are contiguous.
template <typename T>
__global__ __launch_bounds__(KI_THREADS) void k_keyframe_interp(const float* __restrict__ key_vals,
                                                                const int* __restrict__ key_frames, int K, int N,
                                                                const int* __restrict__ gather, int M, float sx, float sy,
                                                                float sz, T* __restrict__ out, int f0)
{
    const int f = f0 + blockIdx.y;
    int lo = 0, hi = K - 1;                  // the last key at or before f (key_frames[0] == 0: there is one)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key_frames[mid] <= f) lo = mid; else hi = mid - 1;
    }
    const int j = lo;
    const bool held = j == K - 1;            // at or past the last key: its value, unblended
    double w = 0.0;
    if (!held) {
        const int kj = key_frames[j], n = key_frames[j + 1] - kj;
        w = __dmul_rn((double)(f - kj), __ddiv_rn(1.0, (double)n));
    }
    const int e = blockIdx.x * KI_THREADS + threadIdx.x;
    if (e >= 3 * M) return;
    const int r = e / 3, c = e - 3 * r;
    const long src = gather ? gather[r] : r;
    const float s = key_vals[((long)j * N + src) * 3 + c];
    double v = (double)s;
    if (!held) {
        const float d = __fsub_rn(key_vals[((long)(j + 1) * N + src) * 3 + c], s);
        v = __dadd_rn(v, __dmul_rn((double)d, w));
    }
    v *= (double)(c == 0 ? sx : c == 1 ? sy : sz);       // +-1: exact
    out[(long)f * (3 * M) + e] = (T)v;
}

extern "C" {
int hm_keyframe_interp(const float* key_vals, const int* key_frames, int K, int N, int frame_nb, const int* gather, int M,
                       const float* signs, int out_f64, int* key_frames_dev, int* gather_dev, void* out, hipStream_t stream)
{
    HM_CHECK_ARG(key_vals && key_frames && signs && key_frames_dev && out && K > 0 && N > 0 && frame_nb > 0);
    HM_CHECK_ARG(gather ? (gather_dev && M > 0) : M == N);
    HM_CHECK_ARG(M <= 0x7fffffff / 3 - KI_THREADS);
    HM_CHECK_ARG(HM_ALIGNED(out, out_f64 ? 8 : 4));  // the void pointer: fp32 or double elements
    HM_CHECK_ARG(key_frames[0] == 0 && key_frames[K - 1] <= frame_nb);
    for (int k = 1; k < K; ++k) HM_CHECK_ARG(key_frames[k] > key_frames[k - 1]);
    for (int i = 0; gather && i < M; ++i) HM_CHECK_ARG(gather[i] >= 0 && gather[i] < N);
    for (int c = 0; c < 3; ++c) HM_CHECK_ARG(signs[c] == 1.f || signs[c] == -1.f);
    // the kernel reads the arrays that were checked: this call's own copies, ordered on the stream before the launch
    if (hipMemcpyAsync(key_frames_dev, key_frames, (size_t)K * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess)
        return HM_ERR_LAUNCH;
    if (gather && hipMemcpyAsync(gather_dev, gather, (size_t)M * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess)
        return HM_ERR_LAUNCH;
    const int* gd = gather ? gather_dev : nullptr;
    for (int f0 = 0; f0 < frame_nb; f0 += KI_MAX_GRID_Y) {
        const dim3 grid(hm_cdiv(3L * M, KI_THREADS), min(frame_nb - f0, KI_MAX_GRID_Y));
        if (out_f64)
            hipLaunchKernelGGL(k_keyframe_interp<double>, grid, dim3(KI_THREADS), 0, stream, key_vals, key_frames_dev, K, N, gd,
                               M, signs[0], signs[1], signs[2], (double*)out, f0);
        else
            hipLaunchKernelGGL(k_keyframe_interp<float>, grid, dim3(KI_THREADS), 0, stream, key_vals, key_frames_dev, K, N, gd,
                               M, signs[0], signs[1], signs[2], (float*)out, f0);
    }
    return hm_launch_status();
}
}  // extern "C"
