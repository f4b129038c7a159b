// five_point_ref.cpp — the checker of limo_five_point: limo_amd/kba/five_point.hpp:estimateMotion (the host estimator, one sample
// after the other, early-abandoned counts) behind a C entry point, with the C-ABI's result struct.  Built by tests/five_point_common.py.
#include <cstring>
#include <vector>

#include "../../include/limo_hip.h"
#include "../../limo_amd/kba/five_point.hpp"

namespace kb = keyframe_bundle_adjustment;

extern "C" int five_point_ref_estimate(int32_t n, const double* pts_a, const double* pts_b, double focal, double cx, double cy, double probability,
                                       double threshold_px, uint64_t seed, int32_t max_samples, limo_five_point_motion* out, uint8_t* inlier) {
    if (n < 0 || !out || (n > 0 && (!pts_a || !pts_b))) return -1;
    std::vector<kb::Vector2d> a(n), b(n);
    for (int i = 0; i < n; ++i) {
        a[i] = kb::Vector2d(pts_a[2 * i], pts_a[2 * i + 1]);
        b[i] = kb::Vector2d(pts_b[2 * i], pts_b[2 * i + 1]);
    }
    const kb::five_point::Motion m = kb::five_point::estimateMotion(a, b, focal, kb::Vector2d(cx, cy), probability, threshold_px, seed, max_samples);
    std::memset(out, 0, sizeof(*out));
    out->ok = m.ok ? 1 : 0;
    out->inliers = m.inliers;
    out->in_front = m.in_front;
    out->samples = m.samples;
    for (int i = 0; i < 9; ++i) {
        out->E[i] = m.E[i];
        out->R[i] = m.R[i];
    }
    for (int i = 0; i < 3; ++i) out->t[i] = m.t[i];
    if (inlier) {  // estimateMotion keeps its mask to itself: the statement that fills it (five_point.hpp:614) on the E it returns
        const double thr2 = (threshold_px / focal) * (threshold_px / focal);
        for (int i = 0; i < n; ++i) {
            const double pa[2] = {(pts_a[2 * i] - cx) / focal, (pts_a[2 * i + 1] - cy) / focal}, pb[2] = {(pts_b[2 * i] - cx) / focal, (pts_b[2 * i + 1] - cy) / focal};
            inlier[i] = m.ok && kb::five_point::sampson2(m.E, pa, pb) < thr2 ? 1 : 0;
        }
    }
    return 0;
}
