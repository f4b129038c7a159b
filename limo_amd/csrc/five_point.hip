// five_point.hip — limo_five_point / limo_five_point_batch on gfx950: RANSAC over all minimal samples of a round at once
// (five_point_core.hpp; the host estimator it equals bit for bit is limo_amd/kba/five_point.hpp:estimateMotion).
//   k_fp_models  one lane per sample: null space, ten cubics, Gauss-Jordan, action matrix, eigenvalues, polish -> up to ten E.
//                The working set of a sample (fp5::kWs doubles + the sample itself, ~4 KB) lives in LDS, kSamplesPerBlock lanes a block.
//   k_fp_score   one block per (sample, frame): every model of the sample against every match, FULL integer counts.
//   k_fp_pose    one block per frame with a model: inlier mask of the winning E, its four (R, t), their in-front counts, the choice.
// The host draws the picks of all samples up front, normalises the matches, and after each round scans that round's counts with
// the stopping rule (fp5::scan_chunk; pow / log stay there).  Frames are a grid dimension; a frame whose scan has ended is left out
// of later rounds.  One stream (the context's), blocks from the context's pools.
// Compiled with floating-point contraction off (pragma + -ffp-contract=off in the build): see five_point_core.hpp.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "five_point_core.hpp"
#include "limo_ctx.hpp"

namespace {

namespace fp5 = kba::fp5;

constexpr int kSamplesPerBlock = 8;               // 8 x (498 + 20) doubles = 33 KB of LDS a block
constexpr int kLaneWs = fp5::kWs + 20;            // working set + the sample's five correspondences (a, b)
constexpr int kScoreThreads = 256, kPoseThreads = 256;
// Samples per round when the caller sets no chunk.  A round costs the time ONE lane needs for ONE sample (~2 ms), whatever its width,
// until the samples outnumber the lanes the device holds at once (4 blocks a CU by LDS and registers: 8192 samples on 256 CUs) - the
// 1000 samples of the default cap are 125 blocks, one round.  A narrow first round for clean frames would save nothing and cost
// frames with many outliers a second round (measured: DESIGN.md §2).
constexpr int kRound = 1024;

struct PoseOut {
    double R[9], t[3];
    int32_t in_front, inliers;
};

// pts: per match (a0, a1, b0, b1) in normalised coordinates, frame f at match offset f_off[f]
__global__ void __launch_bounds__(kSamplesPerBlock)
k_fp_models(const int32_t* __restrict__ active, const int32_t* __restrict__ f_off, const double* __restrict__ pts,
            const int32_t* __restrict__ picks, int max_samples, int s0, int len, double* __restrict__ models,
            int32_t* __restrict__ n_models) {
    __shared__ double lds[kSamplesPerBlock * kLaneWs];
    const int j = blockIdx.x * kSamplesPerBlock + threadIdx.x;
    if (j >= len) return;
    const int f = active[blockIdx.y];
    double* ws = lds + threadIdx.x * kLaneWs;
    double* sa = ws + fp5::kWs;
    double* sb = sa + 10;
    const int32_t* pick = picks + ((int64_t)f * max_samples + (s0 + j)) * 5;
    const double* p = pts + 4 * (int64_t)f_off[f];
    for (int q = 0; q < 5; ++q) {
        const double* m = p + 4 * (int64_t)pick[q];
        sa[2 * q] = m[0];
        sa[2 * q + 1] = m[1];
        sb[2 * q] = m[2];
        sb[2 * q + 1] = m[3];
    }
    const int64_t slot = (int64_t)blockIdx.y * len + j;
    n_models[slot] = fp5::essential_from_five(sa, sb, ws, models + slot * (9 * fp5::kMaxModels));
}

__global__ void __launch_bounds__(kScoreThreads)
k_fp_score(const int32_t* __restrict__ active, const int32_t* __restrict__ f_n, const int32_t* __restrict__ f_off,
           const double* __restrict__ pts, int len, double thr2, const double* __restrict__ models,
           const int32_t* __restrict__ n_models, int32_t* __restrict__ counts) {
    __shared__ double E[9 * fp5::kMaxModels];
    __shared__ int total[fp5::kMaxModels];
    const int f = active[blockIdx.y];
    const int64_t slot = (int64_t)blockIdx.y * len + blockIdx.x;
    const int cnt = n_models[slot];
    const int tid = threadIdx.x;
    if (tid < 9 * cnt) E[tid] = models[slot * (9 * fp5::kMaxModels) + tid];
    if (tid < fp5::kMaxModels) total[tid] = 0;
    __syncthreads();
    if (cnt > 0) {  // (uniform over the block)
        int c[fp5::kMaxModels];
#pragma unroll
        for (int k = 0; k < fp5::kMaxModels; ++k) c[k] = 0;
        const int n = f_n[f];
        const double* p = pts + 4 * (int64_t)f_off[f];
        for (int i = tid; i < n; i += kScoreThreads) {
            const double a0 = p[4 * (int64_t)i], a1 = p[4 * (int64_t)i + 1], b0 = p[4 * (int64_t)i + 2], b1 = p[4 * (int64_t)i + 3];
#pragma unroll
            for (int k = 0; k < fp5::kMaxModels; ++k)
                if (k < cnt) c[k] += fp5::sampson2(E + 9 * k, a0, a1, b0, b1) < thr2 ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < fp5::kMaxModels; ++k)
            if (k < cnt && c[k]) atomicAdd(&total[k], c[k]);
    }
    __syncthreads();
    if (tid < fp5::kMaxModels) counts[slot * fp5::kMaxModels + tid] = total[tid];
}

// posed[b]: the frame of block b
__global__ void __launch_bounds__(kPoseThreads)
k_fp_pose(const int32_t* __restrict__ posed, const int32_t* __restrict__ f_n, const int32_t* __restrict__ f_off,
          const double* __restrict__ pts, double thr2, const double* __restrict__ best_E, uint8_t* __restrict__ mask,
          PoseOut* __restrict__ out) {
    __shared__ double E[9];
    __shared__ double ws[24];
    __shared__ double cand[48];
    __shared__ int front[4];
    __shared__ int inl;
    const int f = posed[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid < 9) E[tid] = best_E[9 * (int64_t)f + tid];
    if (tid < 4) front[tid] = 0;
    if (tid == 0) inl = 0;
    __syncthreads();
    if (tid == 0) fp5::pose_candidates(E, ws, cand);
    __syncthreads();
    const int n = f_n[f];
    const double* p = pts + 4 * (int64_t)f_off[f];
    uint8_t* mk = mask + f_off[f];
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0, ci = 0;
    for (int i = tid; i < n; i += kPoseThreads) {
        const double a0 = p[4 * (int64_t)i], a1 = p[4 * (int64_t)i + 1], b0 = p[4 * (int64_t)i + 2], b1 = p[4 * (int64_t)i + 3];
        const bool in = fp5::sampson2(E, a0, a1, b0, b1) < thr2;
        mk[i] = in ? 1 : 0;
        if (in) {
            ++ci;
            c0 += fp5::in_front(cand, cand + 9, a0, a1, b0, b1) ? 1 : 0;
            c1 += fp5::in_front(cand + 12, cand + 21, a0, a1, b0, b1) ? 1 : 0;
            c2 += fp5::in_front(cand + 24, cand + 33, a0, a1, b0, b1) ? 1 : 0;
            c3 += fp5::in_front(cand + 36, cand + 45, a0, a1, b0, b1) ? 1 : 0;
        }
    }
    if (c0) atomicAdd(&front[0], c0);
    if (c1) atomicAdd(&front[1], c1);
    if (c2) atomicAdd(&front[2], c2);
    if (c3) atomicAdd(&front[3], c3);
    if (ci) atomicAdd(&inl, ci);
    __syncthreads();
    if (tid == 0) {  // the first candidate with the most inliers in front of both cameras (five_point.hpp:546-551)
        int best = -1, pickc = 0;
        for (int c4 = 0; c4 < 4; ++c4)
            if (front[c4] > best) {
                best = front[c4];
                pickc = c4;
            }
        PoseOut* o = out + f;
        for (int i = 0; i < 9; ++i) o->R[i] = cand[12 * pickc + i];
        for (int i = 0; i < 3; ++i) o->t[i] = cand[12 * pickc + 9 + i];
        o->in_front = best;
        o->inliers = inl;
    }
}

#define FP_TRY(expr)                                                             \
    do {                                                                         \
        hipError_t e__ = (expr);                                                 \
        if (e__ != hipSuccess) {                                                 \
            ctx->err = std::string(#expr) + ": " + hipGetErrorString(e__);       \
            rc = LIMO_ERR_RUNTIME;                                               \
            goto done;                                                           \
        }                                                                        \
    } while (0)

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

void motion_identity(limo_five_point_motion* m) {  // five_point::Motion's initial state
    std::memset(m, 0, sizeof(*m));
    m->R[0] = m->R[4] = m->R[8] = 1.;
    m->t[2] = 1.;
}

int round_len(const limo_five_point_params& prm, int start) {
    const int want = prm.chunk > 0 ? prm.chunk : kRound;
    return std::min(want, prm.max_samples - start);
}

int solve(limo_ctx* ctx, int32_t n_frames, const limo_five_point_frame* frames, double focal, double cx, double cy,
          const limo_five_point_params* params, limo_five_point_motion* out, uint8_t* inlier, const char* who) {
    if (!ctx) return LIMO_ERR_INVALID;  // device work: needs a context (no host fallback)
    if (n_frames < 0 || !params || (n_frames > 0 && (!frames || !out))) {
        ctx->err = std::string(who) + ": null pointer or negative frame count";
        return LIMO_ERR_INVALID;
    }
    const limo_five_point_params prm = *params;
    if (!(prm.probability > 0. && prm.probability <= 1.) || !(prm.threshold_px > 0.) || !std::isfinite(prm.threshold_px) ||
        prm.max_samples < 1 || prm.max_samples > 16384 || prm.chunk < 0) {
        ctx->err = std::string(who) + ": parameter out of range (probability in (0, 1], threshold_px > 0, max_samples 1 .. 16384, chunk >= 0)";
        return LIMO_ERR_INVALID;
    }
    if (!(focal > 0.) || !std::isfinite(focal) || !std::isfinite(cx) || !std::isfinite(cy)) {
        ctx->err = std::string(who) + ": focal length must be positive and finite, the principal point finite";
        return LIMO_ERR_INVALID;
    }
    int64_t total = 0;
    int32_t n_run = 0;  // frames with five correspondences or more
    for (int32_t f = 0; f < n_frames; ++f) {
        const limo_five_point_frame& fr = frames[f];
        if (fr.n < 0 || (fr.n > 0 && (!fr.pts_a || !fr.pts_b))) {
            ctx->err = std::string(who) + ": frame " + std::to_string(f) + ": negative match count or null point list";
            return LIMO_ERR_INVALID;
        }
        for (int64_t i = 0; i < 2 * (int64_t)fr.n; ++i)
            if (!std::isfinite(fr.pts_a[i]) || !std::isfinite(fr.pts_b[i])) {
                ctx->err = std::string(who) + ": frame " + std::to_string(f) + ": non-finite coordinate at match " + std::to_string(i / 2);
                return LIMO_ERR_INVALID;
            }
        total += fr.n;
        n_run += fr.n >= 5;
    }
    if (total > (int64_t(1) << 28)) {
        ctx->err = std::string(who) + ": more than 2^28 matches in one call";
        return LIMO_ERR_INVALID;
    }
    for (int32_t f = 0; f < n_frames; ++f) motion_identity(out + f);
    if (inlier && n_frames == 1 && frames[0].n > 0) std::memset(inlier, 0, (size_t)frames[0].n);
    if (n_run == 0) return LIMO_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) return LIMO_ERR_NO_DEVICE;

    const int F = n_frames, S = prm.max_samples;
    const int cap = prm.chunk > 0 ? std::min(prm.chunk, S) : std::min(kRound, S);  // widest round
    const double thr2 = (prm.threshold_px / focal) * (prm.threshold_px / focal);  // five_point.hpp:567
    // one device block and its pinned mirror: [pts | picks | f_n | f_off | list | n_models | counts | best_E | pose | mask | models]
    // (models stay on the device)
    const size_t o_pts = 0, o_picks = o_pts + align256(sizeof(double) * 4 * (size_t)total), o_fn = o_picks + align256(sizeof(int32_t) * 5 * (size_t)F * S),
                 o_foff = o_fn + align256(sizeof(int32_t) * F), o_list = o_foff + align256(sizeof(int32_t) * F),
                 o_nm = o_list + align256(sizeof(int32_t) * F), o_cnt = o_nm + align256(sizeof(int32_t) * (size_t)F * cap),
                 o_best = o_cnt + align256(sizeof(int32_t) * 10 * (size_t)F * cap), o_pose = o_best + align256(sizeof(double) * 9 * F),
                 o_mask = o_pose + align256(sizeof(PoseOut) * F), host_bytes = o_mask + align256((size_t)total),
                 o_models = host_bytes, dev_bytes = o_models + align256(sizeof(double) * 90 * (size_t)F * cap);
    int rc = LIMO_OK;
    char *h = nullptr, *d = nullptr;
    hipStream_t s = ctx->stream;
    std::vector<fp5::Scan> scan(F);
    std::vector<int32_t> active, posed;
    FP_TRY(ctx->host_alloc((void**)&h, host_bytes));
    FP_TRY(ctx->pool_alloc((void**)&d, dev_bytes));
    {
        double* pts = (double*)(h + o_pts);
        int32_t *picks = (int32_t*)(h + o_picks), *fn = (int32_t*)(h + o_fn), *foff = (int32_t*)(h + o_foff);
        int64_t off = 0;
        for (int f = 0; f < F; ++f) {
            const limo_five_point_frame& fr = frames[f];
            fn[f] = fr.n;
            foff[f] = (int32_t)off;
            for (int i = 0; i < fr.n; ++i) {
                double* m = pts + 4 * (off + i);
                m[0] = fp5::normalise(fr.pts_a[2 * i], cx, focal);
                m[1] = fp5::normalise(fr.pts_a[2 * i + 1], cy, focal);
                m[2] = fp5::normalise(fr.pts_b[2 * i], cx, focal);
                m[3] = fp5::normalise(fr.pts_b[2 * i + 1], cy, focal);
            }
            off += fr.n;
            if (fr.n >= 5) {
                fp5::draw_picks(fr.seed, fr.n, S, picks + 5 * (size_t)f * S);
                fp5::scan_begin(scan[f], S);
                active.push_back(f);
            } else {
                std::memset(picks + 5 * (size_t)f * S, 0, sizeof(int32_t) * 5 * (size_t)S);
            }
        }
        FP_TRY(hipMemcpyAsync(d, h, o_list, hipMemcpyHostToDevice, s));  // pts, picks, f_n, f_off
    }
    for (int start = 0; !active.empty();) {
        const int len = round_len(prm, start), na = (int)active.size();
        std::memcpy(h + o_list, active.data(), sizeof(int32_t) * na);
        FP_TRY(hipMemcpyAsync(d + o_list, h + o_list, sizeof(int32_t) * na, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fp_models, dim3((len + kSamplesPerBlock - 1) / kSamplesPerBlock, na), dim3(kSamplesPerBlock), 0, s,
                           (const int32_t*)(d + o_list), (const int32_t*)(d + o_foff), (const double*)(d + o_pts),
                           (const int32_t*)(d + o_picks), S, start, len, (double*)(d + o_models), (int32_t*)(d + o_nm));
        FP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_fp_score, dim3(len, na), dim3(kScoreThreads), 0, s, (const int32_t*)(d + o_list), (const int32_t*)(d + o_fn),
                           (const int32_t*)(d + o_foff), (const double*)(d + o_pts), len, thr2, (const double*)(d + o_models),
                           (const int32_t*)(d + o_nm), (int32_t*)(d + o_cnt));
        FP_TRY(hipGetLastError());
        FP_TRY(hipMemcpyAsync(h + o_nm, d + o_nm, sizeof(int32_t) * (size_t)na * len, hipMemcpyDeviceToHost, s));
        FP_TRY(hipMemcpyAsync(h + o_cnt, d + o_cnt, sizeof(int32_t) * 10 * (size_t)na * len, hipMemcpyDeviceToHost, s));
        FP_TRY(hipStreamSynchronize(s));
        std::vector<int32_t> next;
        for (int ai = 0; ai < na; ++ai) {
            const int f = active[ai];
            fp5::Scan& sc = scan[f];
            const int before_s = sc.best_sample, before_m = sc.best_model;
            fp5::scan_chunk(sc, frames[f].n, prm.probability, S, start, len, (const int32_t*)(h + o_nm) + (size_t)ai * len,
                            (const int32_t*)(h + o_cnt) + 10 * (size_t)ai * len);
            if (sc.best_sample != before_s || sc.best_model != before_m)  // the winner so far: kept before the next round overwrites it
                FP_TRY(hipMemcpyAsync(d + o_best + sizeof(double) * 9 * f,
                                      d + o_models + sizeof(double) * (90 * ((size_t)ai * len + (sc.best_sample - start)) + 9 * sc.best_model),
                                      sizeof(double) * 9, hipMemcpyDeviceToDevice, s));
            if (!sc.done) next.push_back(f);
        }
        active.swap(next);
        start += len;
    }
    for (int f = 0; f < F; ++f)
        if (scan[f].ok) posed.push_back(f);
    if (!posed.empty()) {
        std::memcpy(h + o_list, posed.data(), sizeof(int32_t) * posed.size());
        FP_TRY(hipMemcpyAsync(d + o_list, h + o_list, sizeof(int32_t) * posed.size(), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fp_pose, dim3((unsigned)posed.size()), dim3(kPoseThreads), 0, s, (const int32_t*)(d + o_list),
                           (const int32_t*)(d + o_fn), (const int32_t*)(d + o_foff), (const double*)(d + o_pts), thr2,
                           (const double*)(d + o_best), (uint8_t*)(d + o_mask), (PoseOut*)(d + o_pose));
        FP_TRY(hipGetLastError());
        FP_TRY(hipMemcpyAsync(h + o_best, d + o_best, (inlier ? host_bytes : o_mask) - o_best, hipMemcpyDeviceToHost, s));  // best_E, pose (, mask)
        FP_TRY(hipStreamSynchronize(s));
    }
    for (int f = 0; f < F; ++f) {
        limo_five_point_motion& m = out[f];
        const fp5::Scan& sc = scan[f];
        m.samples = sc.samples;
        if (!sc.ok) continue;
        const PoseOut& po = ((const PoseOut*)(h + o_pose))[f];
        m.ok = 1;
        m.inliers = sc.inliers;
        m.in_front = po.in_front;
        std::memcpy(m.E, h + o_best + sizeof(double) * 9 * f, sizeof(double) * 9);
        std::memcpy(m.R, po.R, sizeof(po.R));
        std::memcpy(m.t, po.t, sizeof(po.t));
        if (po.inliers != sc.inliers) {  // the score and the pose kernel count the same comparisons
            ctx->err = std::string(who) + ": frame " + std::to_string(f) + ": inlier counts of the two kernels differ";
            rc = LIMO_ERR_RUNTIME;
            goto done;
        }
    }
    if (inlier && F == 1 && scan[0].ok) std::memcpy(inlier, h + o_mask, (size_t)frames[0].n);
done:
    // an error after work was queued: drain the stream before the blocks go back to the pools
    if (rc != LIMO_OK) (void)hipStreamSynchronize(s);
    if (h) ctx->host_free(h, host_bytes);
    if (d) ctx->pool_free(d, dev_bytes);
    return rc;
}

}  // namespace

extern "C" void limo_five_point_default_params(limo_five_point_params* out) {
    if (!out) return;
    out->probability = 0.999;
    out->threshold_px = 2.0;
    out->max_samples = 1000;
    out->chunk = 0;
}

extern "C" int limo_five_point(limo_ctx* ctx, const limo_five_point_frame* frame, double focal, double cx, double cy,
                               const limo_five_point_params* params, limo_five_point_motion* out, uint8_t* inlier) {
    if (ctx && (!frame || !out)) ctx->err = "limo_five_point: null pointer";
    if (!ctx || !frame || !out) return LIMO_ERR_INVALID;
    return solve(ctx, 1, frame, focal, cx, cy, params, out, inlier, "limo_five_point");
}

extern "C" int limo_five_point_batch(limo_ctx* ctx, int32_t n_frames, const limo_five_point_frame* frames, double focal, double cx,
                                     double cy, const limo_five_point_params* params, limo_five_point_motion* out) {
    return solve(ctx, n_frames, frames, focal, cx, cy, params, out, nullptr, "limo_five_point_batch");
}
