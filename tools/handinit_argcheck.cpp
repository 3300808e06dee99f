// Stand-alone host program for a sanitizer run of the argument checks of csrc/handinit.hip (no GPU needed: every call below is
// refused with HM_ERR_BAD_ARG before anything is enqueued).  Build and run, from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -I homan_amd/csrc -I include \
//         homan_amd/csrc/handinit.hip tools/handinit_argcheck.cpp -o /tmp/handinit_argcheck && /tmp/handinit_argcheck
#include <cstdio>
#include <limits>
#include "homan_amd.h"

static int failures = 0;
#define EXPECT_BAD(call) do { const int rc = (call); if (rc != HM_ERR_BAD_ARG) { std::printf("line %d: rc %d\n", __LINE__, rc); ++failures; } } while (0)

int main()
{
    static float f[16];
    static int t[4];
    float* p = f;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // hm_keypoint_terms_clips: every required pointer in turn, the kp3d / c3 pair, N, clip_len, sigma
    EXPECT_BAD(hm_keypoint_terms_clips(nullptr, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, nullptr, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, nullptr, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, nullptr, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, nullptr, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, nullptr, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, nullptr, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, nullptr, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, nullptr, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, nullptr, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, nullptr, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, nullptr, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, nullptr, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 5, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 0, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, -4, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 0, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, -2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 0.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, -1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, nan, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, 2, nullptr));
    EXPECT_BAD(hm_keypoint_terms_clips(p, p, p, p, p, p, p, p, 1.f, .01f, 1.f, 1.f, 6, 2, p, p, p, t, p, -1, nullptr));
    // hm_handinit_finish_clips
    EXPECT_BAD(hm_handinit_finish_clips(nullptr, p, 6, 2, p, 8, 1.f, 1.f, 1.f, 1.f, 1.f, t, 4, p, nullptr));
    EXPECT_BAD(hm_handinit_finish_clips(p, p, 6, 2, nullptr, 8, 1.f, 1.f, 1.f, 1.f, 1.f, t, 4, p, nullptr));
    EXPECT_BAD(hm_handinit_finish_clips(p, p, 5, 2, p, 8, 1.f, 1.f, 1.f, 1.f, 1.f, t, 4, p, nullptr));
    EXPECT_BAD(hm_handinit_finish_clips(p, p, 0, 2, p, 8, 1.f, 1.f, 1.f, 1.f, 1.f, t, 4, p, nullptr));
    EXPECT_BAD(hm_handinit_finish_clips(p, p, 6, 0, p, 8, 1.f, 1.f, 1.f, 1.f, 1.f, t, 4, p, nullptr));
    EXPECT_BAD(hm_handinit_finish_clips(p, p, 6, 2, p, 7, 1.f, 1.f, 1.f, 1.f, 1.f, t, 4, p, nullptr));
    EXPECT_BAD(hm_handinit_finish_clips(p, p, 6, 2, p, 8, 1.f, 1.f, 1.f, 1.f, 1.f, nullptr, 4, p, nullptr));
    EXPECT_BAD(hm_handinit_finish_clips(p, p, 6, 2, p, 8, 1.f, 1.f, 1.f, 1.f, 1.f, t, 0, p, nullptr));
    for (int i = 0; i < 16; ++i) if (f[i] != 0.f) ++failures;            // nothing was written
    std::printf(failures ? "FAILED: %d\n" : "handinit argument checks: ok (%d failures)\n", failures);
    return failures != 0;
}
