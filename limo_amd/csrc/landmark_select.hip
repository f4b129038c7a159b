// landmark_select.hip — limo_landmark_select / limo_landmark_select_batch on gfx950 (landmark_select_core.hpp; the host classes it
// equals byte for byte are limo_amd/kba/landmark_selector.hpp and landmark_selection_voxel.hpp, wired as stream_driver.hpp:110-125).
//   k_ls_landmarks  one lane per landmark: cheirality over its observations, position in the newest keyframe's frame, plausibility cut,
//                   distance to the driven path, cell key; the far field's order key; the order key of every must-have entry.
//   k_ls_voxels     one workgroup per pool: bitonic sort of (cell key, landmark index) - in LDS when the pool fits kLdsSort entries,
//                   else the same network on a global-memory block - then one lane per voxel head: centroid and representative,
//                   sequentially in id order, its class (near / middle) and order key (image flow / hashed rank).
//   k_ls_rank       one lane per landmark and list (list 0: the three fields; list 1 + e: must-have entry e): the number of members of
//                   its class that come before it in the TOTAL order (key, landmark index); fewer than the budget = chosen.  The chosen
//                   sets do not depend on how they are found.  Bits are OR-ed into the output byte.
// The pool is a grid dimension of every kernel.  The host validates, forms the transforms of the (at most 64) keyframes and brings the
// observations into (landmark, time rank, camera) order; a pool whose cell indices leave (-2^20, 2^20) raises a flag and is finished
// with lsel::select_host.  No device-wide barrier, no cooperative launch; every loop bound comes from a validated size.
// Compiled with floating-point contraction off (pragma + -ffp-contract=off in the build): see landmark_select_core.hpp.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "landmark_select_core.hpp"
#include "limo_ctx.hpp"

namespace {

namespace ls = kba::lsel;

constexpr int kLmThreads = 256, kRankThreads = 256, kVoxelThreads = 1024;
constexpr int kLdsSort = 4096;  // entries of the LDS sort: 4096 x (8 + 4) bytes = 48 KB

struct PoolDesc {
    int32_t n_kf, n_cam, n_lm, n_obs, newest;
    int32_t kf_off, cam_off, lm_off, lmobs_off, obs_off, sort_off, sort_n, out_off, use_lds;
    uint64_t seed;
};
struct Dev {  // device block of one call, all pools one after the other
    const PoolDesc* desc;
    const ls::Add* add;
    const double *T_kf, *path, *T_cam, *lm_pos;
    const int32_t *kf_by_time, *lm_obs, *obs_rank, *obs_cam;
    const uint64_t* lm_id;
    const uint8_t* lm_flags;
    const float *obs_u, *obs_v, *obs_d;
    double *p3, *dist;
    uint8_t *status, *cls, *out;
    uint64_t *ord, *add_ord, *sort_key;
    uint32_t* sort_idx;
    int32_t* flag;
    int64_t total_lm;
};

__device__ __forceinline__ ls::Pool pool_view(const Dev& D, const PoolDesc& d) {
    ls::Pool P;
    P.n_kf = d.n_kf, P.n_cam = d.n_cam, P.n_lm = d.n_lm, P.n_obs = d.n_obs, P.newest = d.newest, P.seed = d.seed;
    P.T_kf = D.T_kf + 12 * (int64_t)d.kf_off;
    P.path = D.path + 3 * (int64_t)d.kf_off;
    P.kf_by_time = D.kf_by_time + d.kf_off;
    P.T_cam = D.T_cam + 12 * (int64_t)d.cam_off;
    P.lm_id = D.lm_id + d.lm_off;
    P.lm_pos = D.lm_pos + 3 * (int64_t)d.lm_off;
    P.lm_flags = D.lm_flags + d.lm_off;
    P.lm_obs = D.lm_obs + d.lmobs_off;
    P.obs_rank = D.obs_rank + d.obs_off;
    P.obs_cam = D.obs_cam + d.obs_off;
    P.obs_u = D.obs_u + d.obs_off;
    P.obs_v = D.obs_v + d.obs_off;
    P.obs_d = D.obs_d + d.obs_off;
    return P;
}

__global__ void __launch_bounds__(kLmThreads) k_ls_landmarks(Dev D, ls::Params prm) {
    const PoolDesc d = D.desc[blockIdx.y];
    const int i = blockIdx.x * kLmThreads + threadIdx.x;
    if (i >= d.sort_n) return;  // (sort_n >= n_lm: the padding of the sort network is written here too)
    if (i >= d.n_lm) {
        D.sort_key[d.sort_off + i] = ls::kNoKey;
        D.sort_idx[d.sort_off + i] = (uint32_t)i;
        return;
    }
    const ls::Pool P = pool_view(D, d);
    ls::Stage1 s;
    ls::stage1(P, prm, i, &s);
    const int64_t g = (int64_t)d.lm_off + i;
    D.p3[3 * g] = s.p[0];
    D.p3[3 * g + 1] = s.p[1];
    D.p3[3 * g + 2] = s.p[2];
    D.dist[g] = s.dist;
    D.status[g] = s.status;
    const bool pipe = s.status == ls::kPipe;
    if (pipe && !s.packed) D.flag[blockIdx.y] = 1;  // (every writer writes 1)
    D.sort_key[d.sort_off + i] = pipe && s.packed ? ls::cell_key(s.cell) : ls::kNoKey;
    D.sort_idx[d.sort_off + i] = (uint32_t)i;
    D.cls[g] = s.status == ls::kFar ? 3 : 0;
    D.ord[g] = s.status == ls::kFar ? ls::far_ord(d.n_kf, s.seen) : ls::kNoKey;
    D.out[d.out_off + i] = s.status == ls::kRejected ? 8 : 0;
    for (int e = 0; e < prm.n_add; ++e) {
        const ls::Add a = D.add[e];
        uint64_t o = ls::kNoKey;
        double k;
        if (a.frame_index >= 0 && a.frame_index <= d.n_kf - 1 && s.status != ls::kRejected && ls::predicate(P.lm_flags[i], a.predicate) &&
            ls::must_key(P, i, a.frame_index, a.key, &k))
            o = ls::ord_ascending(k);
        D.add_ord[(int64_t)e * D.total_lm + g] = o;
    }
}

__global__ void __launch_bounds__(kVoxelThreads) k_ls_voxels(Dev D, ls::Params prm) {
    __shared__ uint64_t s_key[kLdsSort];
    __shared__ uint32_t s_idx[kLdsSort];
    const PoolDesc d = D.desc[blockIdx.x];
    if (D.flag[blockIdx.x]) return;  // (uniform: written by the kernel before) - the host finishes this pool
    const int n = d.sort_n, tid = threadIdx.x;
    uint64_t* key = D.sort_key + d.sort_off;
    uint32_t* idx = D.sort_idx + d.sort_off;
    if (d.use_lds) {  // (use_lds implies n <= kLdsSort)
        for (int t = tid; t < n; t += kVoxelThreads) {
            s_key[t] = key[t];
            s_idx[t] = idx[t];
        }
        key = s_key;
        idx = s_idx;
    }
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < n; t += kVoxelThreads) {
                const int x = t ^ j;
                if (x <= t) continue;
                const uint64_t ka = key[t], kb = key[x];
                const uint32_t ia = idx[t], ib = idx[x];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                if (gt == ((t & k) == 0)) {
                    key[t] = kb, key[x] = ka;
                    idx[t] = ib, idx[x] = ia;
                }
            }
            __syncthreads();
        }
    const ls::Pool P = pool_view(D, d);
    const double* p3 = D.p3 + 3 * (int64_t)d.lm_off;
    for (int q = tid; q < n; q += kVoxelThreads) {
        const uint64_t kq = key[q];
        if (kq == ls::kNoKey || (q > 0 && key[q - 1] == kq)) continue;
        int q1 = q + 1;
        while (q1 < n && key[q1] == kq) ++q1;
        const int rep = (int)ls::voxel_representative(idx, q, q1, p3);
        uint8_t cls;
        uint64_t ord;
        ls::classify_representative(P, prm, rep, D.dist[d.lm_off + rep], &cls, &ord);
        D.cls[d.lm_off + rep] = cls;
        D.ord[d.lm_off + rep] = ord;
    }
}

__global__ void __launch_bounds__(kRankThreads) k_ls_rank(Dev D, ls::Params prm) {
    __shared__ uint64_t s_ord[kRankThreads];
    __shared__ uint8_t s_cls[kRankThreads];
    const PoolDesc d = D.desc[blockIdx.z];
    if (D.flag[blockIdx.z] || (int)(blockIdx.x * kRankThreads) >= d.n_lm) return;  // (uniform)
    const int list = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * kRankThreads + tid;
    const uint64_t* ord = list == 0 ? D.ord + d.lm_off : D.add_ord + (int64_t)(list - 1) * D.total_lm + d.lm_off;
    const uint8_t* cls = D.cls + d.lm_off;
    uint64_t mine = ls::kNoKey;
    int c = 0;
    int64_t budget = 0;
    if (i < d.n_lm) {
        mine = ord[i];
        if (list == 0) {
            c = cls[i];
            budget = (int64_t)ls::budget_of(prm, c);
        } else {
            c = mine != ls::kNoKey ? 1 : 0;
            budget = (int64_t)D.add[list - 1].count;
        }
    }
    int64_t before = 0;
    for (int tile = 0; tile < d.n_lm; tile += kRankThreads) {
        const int j = tile + tid;
        const uint64_t oj = j < d.n_lm ? ord[j] : ls::kNoKey;
        s_ord[tid] = oj;
        s_cls[tid] = j >= d.n_lm ? 0 : list == 0 ? cls[j] : (oj != ls::kNoKey ? 1 : 0);
        __syncthreads();
        if (c != 0) {
            const int m = min(kRankThreads, d.n_lm - tile);
            for (int jj = 0; jj < m; ++jj) {
                const uint64_t o = s_ord[jj];
                before += (s_cls[jj] == c && (o < mine || (o == mine && tile + jj < i))) ? 1 : 0;
            }
        }
        __syncthreads();
    }
    if (c != 0 && before < budget) {
        const uint32_t bits = list == 0 ? (uint32_t)c : 4u;
        const int64_t byte = (int64_t)d.out_off + i;  // (out_off is a multiple of 4)
        atomicOr(reinterpret_cast<unsigned int*>(D.out) + (byte >> 2), bits << (8 * (byte & 3)));
    }
}

#define LS_TRY(expr)                                                             \
    do {                                                                         \
        hipError_t e__ = (expr);                                                 \
        if (e__ != hipSuccess) {                                                 \
            ctx->err = std::string(#expr) + ": " + hipGetErrorString(e__);       \
            rc = LIMO_ERR_RUNTIME;                                               \
            goto done;                                                           \
        }                                                                        \
    } while (0)

struct Carver {  // offsets into one block, 256-byte aligned
    size_t top = 0;
    size_t take(size_t bytes) {
        const size_t at = top;
        top += (bytes + 255) / 256 * 256;
        return at;
    }
};

int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

std::string where(const char* who, int p) { return std::string(who) + ": pool " + std::to_string(p) + ": "; }

// every refusal of the header, before anything is allocated or launched
int validate(limo_ctx* ctx, int32_t n_pools, const limo_select_pool* pools, const limo_select_params* params, uint8_t* const* out, const char* who) {
    auto bad = [&](const std::string& msg) {
        ctx->err = msg;
        return LIMO_ERR_INVALID;
    };
    if (n_pools < 0 || !params || (n_pools > 0 && (!pools || !out))) return bad(std::string(who) + ": null pointer or negative pool count");
    const limo_select_params& q = *params;
    for (int a = 0; a < 3; ++a)
        if (!(q.voxel_size_xyz[a] > 0.)) return bad(std::string(who) + ": voxel_size_xyz must be positive");
    if (!(q.roi_far > 0.)) return bad(std::string(who) + ": roi_far must be positive");
    if (!(q.roi_middle > 0.)) return bad(std::string(who) + ": roi_middle must be positive");
    if (q.n_add < 0 || (q.n_add > 0 && !q.add)) return bad(std::string(who) + ": n_add negative, or add null");
    if (q.sort_capacity < 0) return bad(std::string(who) + ": sort_capacity negative");
    for (int e = 0; e < q.n_add; ++e)
        if (q.add[e].predicate < 0 || q.add[e].predicate > 1 || q.add[e].key < 0 || q.add[e].key > 1)
            return bad(std::string(who) + ": add[" + std::to_string(e) + "]: unknown predicate or key");
    int64_t total_lm = 0, total_obs = 0;
    for (int p = 0; p < n_pools; ++p) {
        const limo_select_pool& w = pools[p];
        if (w.n_kf < 0) return bad(where(who, p) + "n_kf negative");
        if (w.n_cam < 0) return bad(where(who, p) + "n_cam negative");
        if (w.n_lm < 0) return bad(where(who, p) + "n_lm negative");
        if (w.n_obs < 0) return bad(where(who, p) + "n_obs negative");
        if (w.n_kf > ls::kMaxKf) return bad(where(who, p) + "n_kf above 64");
        if (w.n_cam > ls::kMaxCam) return bad(where(who, p) + "n_cam above 8");
        if (w.n_kf > 0 && !w.kf_pose) return bad(where(who, p) + "kf_pose null");
        if (w.n_kf > 0 && !w.kf_stamp) return bad(where(who, p) + "kf_stamp null");
        if (w.n_cam > 0 && !w.cam) return bad(where(who, p) + "cam null");
        if (w.n_lm > 0 && !w.lm_id) return bad(where(who, p) + "lm_id null");
        if (w.n_lm > 0 && !w.lm_pos) return bad(where(who, p) + "lm_pos null");
        if (w.n_lm > 0 && !w.lm_has_depth) return bad(where(who, p) + "lm_has_depth null");
        if (w.n_lm > 0 && !w.lm_is_ground) return bad(where(who, p) + "lm_is_ground null");
        if (w.n_lm > 0 && !out[p]) return bad(where(who, p) + "out null");
        if (w.n_obs > 0 && (!w.obs_kf || !w.obs_lm || !w.obs_cam || !w.obs_u || !w.obs_v || !w.obs_d)) return bad(where(who, p) + "obs_* null");
        for (int i = 1; i < w.n_lm; ++i)
            if (!(w.lm_id[i - 1] < w.lm_id[i])) return bad(where(who, p) + "lm_id not strictly ascending at " + std::to_string(i));
        for (int o = 0; o < w.n_obs; ++o) {
            if (w.obs_kf[o] < 0 || w.obs_kf[o] >= w.n_kf) return bad(where(who, p) + "obs_kf out of range at observation " + std::to_string(o));
            if (w.obs_lm[o] < 0 || w.obs_lm[o] >= w.n_lm) return bad(where(who, p) + "obs_lm out of range at observation " + std::to_string(o));
            if (w.obs_cam[o] < 0 || w.obs_cam[o] >= w.n_cam) return bad(where(who, p) + "obs_cam out of range at observation " + std::to_string(o));
        }
        total_lm += w.n_lm;
        total_obs += w.n_obs;
    }
    if (total_lm > (int64_t(1) << 27) || total_obs > (int64_t(1) << 28)) return bad(std::string(who) + ": more than 2^27 landmarks or 2^28 observations in one call");
    return LIMO_OK;
}

int run(limo_ctx* ctx, int32_t n_pools, const limo_select_pool* pools, const limo_select_params* params, uint8_t* const* out, const char* who) {
    if (!ctx) return LIMO_ERR_INVALID;  // device work: needs a context
    {
        const int v = validate(ctx, n_pools, pools, params, out, who);
        if (v != LIMO_OK) return v;
    }
    ls::Params prm;
    for (int a = 0; a < 3; ++a) prm.voxel[a] = params->voxel_size_xyz[a];
    prm.roi_far = params->roi_far, prm.roi_middle = params->roi_middle;
    prm.max_near = params->max_near, prm.max_middle = params->max_middle, prm.max_far = params->max_far;
    prm.n_add = params->n_add;
    const int lds_cap = params->sort_capacity > 0 ? std::min(params->sort_capacity, kLdsSort) : kLdsSort;

    // the pools that run (a pool without landmarks or without keyframes selects nothing), their frames and observation order
    std::vector<int> runs;
    std::vector<ls::Frames> frames;
    std::vector<std::vector<int32_t>> orders;
    std::vector<std::vector<int32_t>> starts;
    std::vector<PoolDesc> desc;
    int64_t tot_kf = 0, tot_cam = 0, tot_lm = 0, tot_obs = 0, tot_sort = 0, tot_out = 0;
    int max_sort = 0, max_lm = 0;
    for (int p = 0; p < n_pools; ++p) {
        const limo_select_pool& w = pools[p];
        if (w.n_lm == 0) continue;
        if (w.n_kf == 0) {
            std::memset(out[p], 0, (size_t)w.n_lm);
            continue;
        }
        frames.emplace_back();
        ls::make_frames(w.n_kf, w.n_cam, w.kf_pose, w.kf_stamp, w.cam, &frames.back());
        starts.emplace_back((size_t)w.n_lm + 1);
        orders.emplace_back();
        int dup = 0;
        if (!ls::order_observations(w.n_lm, w.n_obs, w.obs_kf, w.obs_lm, w.obs_cam, frames.back().rank_of_kf.data(), starts.back().data(), orders.back(), &dup)) {
            ctx->err = where(who, p) + "duplicate (obs_kf, obs_lm, obs_cam) at observation " + std::to_string(dup);
            return LIMO_ERR_INVALID;
        }
        PoolDesc d;
        d.n_kf = w.n_kf, d.n_cam = w.n_cam, d.n_lm = w.n_lm, d.n_obs = w.n_obs, d.newest = frames.back().newest, d.seed = frames.back().seed;
        d.kf_off = (int32_t)tot_kf, d.cam_off = (int32_t)tot_cam, d.lm_off = (int32_t)tot_lm, d.lmobs_off = (int32_t)(tot_lm + (int64_t)runs.size());
        d.obs_off = (int32_t)tot_obs, d.sort_off = (int32_t)tot_sort, d.sort_n = pow2_at_least(w.n_lm), d.out_off = (int32_t)tot_out;
        d.use_lds = w.n_lm <= lds_cap ? 1 : 0;
        tot_kf += w.n_kf, tot_cam += w.n_cam, tot_lm += w.n_lm, tot_obs += w.n_obs, tot_sort += d.sort_n, tot_out += (w.n_lm + 3) / 4 * 4;
        max_sort = std::max(max_sort, d.sort_n), max_lm = std::max(max_lm, w.n_lm);
        desc.push_back(d);
        runs.push_back(p);
    }
    if (runs.empty()) return LIMO_OK;
    if (tot_sort > (int64_t(1) << 28)) {
        ctx->err = std::string(who) + ": pools too large for one call";
        return LIMO_ERR_INVALID;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return LIMO_ERR_NO_DEVICE;

    const int R = (int)runs.size(), n_add = prm.n_add;
    // one device block and the pinned mirror of its head: [uploaded | out, flag (come back) | scratch (stays on the device)]
    Carver c;
    const size_t o_desc = c.take(sizeof(PoolDesc) * R), o_add = c.take(sizeof(ls::Add) * std::max(1, n_add)), o_Tkf = c.take(sizeof(double) * 12 * tot_kf),
                 o_path = c.take(sizeof(double) * 3 * tot_kf), o_kbt = c.take(sizeof(int32_t) * tot_kf), o_Tcam = c.take(sizeof(double) * 12 * std::max<int64_t>(1, tot_cam)),
                 o_id = c.take(sizeof(uint64_t) * tot_lm), o_pos = c.take(sizeof(double) * 3 * tot_lm), o_flags = c.take((size_t)tot_lm),
                 o_lmobs = c.take(sizeof(int32_t) * (tot_lm + R)), o_rank = c.take(sizeof(int32_t) * std::max<int64_t>(1, tot_obs)),
                 o_cam = c.take(sizeof(int32_t) * std::max<int64_t>(1, tot_obs)), o_u = c.take(sizeof(float) * std::max<int64_t>(1, tot_obs)),
                 o_v = c.take(sizeof(float) * std::max<int64_t>(1, tot_obs)), o_d = c.take(sizeof(float) * std::max<int64_t>(1, tot_obs)), up_bytes = c.top,
                 o_out = c.take((size_t)tot_out), o_flag = c.take(sizeof(int32_t) * R), host_bytes = c.top, o_p3 = c.take(sizeof(double) * 3 * tot_lm),
                 o_dist = c.take(sizeof(double) * tot_lm), o_status = c.take((size_t)tot_lm), o_cls = c.take((size_t)tot_lm), o_ord = c.take(sizeof(uint64_t) * tot_lm),
                 o_aord = c.take(sizeof(uint64_t) * tot_lm * std::max(1, n_add)), o_skey = c.take(sizeof(uint64_t) * tot_sort),
                 o_sidx = c.take(sizeof(uint32_t) * tot_sort), dev_bytes = c.top;
    int rc = LIMO_OK;
    char *h = nullptr, *d = nullptr;
    hipStream_t s = ctx->stream;
    hipEvent_t ev[2] = {nullptr, nullptr};
    LS_TRY(ctx->host_alloc((void**)&h, host_bytes));
    LS_TRY(ctx->pool_alloc((void**)&d, dev_bytes));
    std::memcpy(h + o_desc, desc.data(), sizeof(PoolDesc) * R);
    for (int e = 0; e < n_add; ++e) {
        const limo_select_add& a = params->add[e];
        ((ls::Add*)(h + o_add))[e] = {a.frame_index, a.count, a.predicate, a.key};
    }
    for (int r = 0; r < R; ++r) {
        const limo_select_pool& w = pools[runs[r]];
        const PoolDesc& pd = desc[r];
        const ls::Frames& F = frames[r];
        std::memcpy((double*)(h + o_Tkf) + 12 * (size_t)pd.kf_off, F.T_kf.data(), sizeof(double) * 12 * w.n_kf);
        std::memcpy((double*)(h + o_path) + 3 * (size_t)pd.kf_off, F.path.data(), sizeof(double) * 3 * w.n_kf);
        std::memcpy((int32_t*)(h + o_kbt) + pd.kf_off, F.kf_by_time.data(), sizeof(int32_t) * w.n_kf);
        if (w.n_cam) std::memcpy((double*)(h + o_Tcam) + 12 * (size_t)pd.cam_off, F.T_cam.data(), sizeof(double) * 12 * w.n_cam);
        std::memcpy((uint64_t*)(h + o_id) + pd.lm_off, w.lm_id, sizeof(uint64_t) * w.n_lm);
        std::memcpy((double*)(h + o_pos) + 3 * (size_t)pd.lm_off, w.lm_pos, sizeof(double) * 3 * w.n_lm);
        uint8_t* fl = (uint8_t*)(h + o_flags) + pd.lm_off;
        for (int i = 0; i < w.n_lm; ++i) fl[i] = (w.lm_has_depth[i] ? 1 : 0) | (w.lm_is_ground[i] ? 2 : 0);
        std::memcpy((int32_t*)(h + o_lmobs) + pd.lmobs_off, starts[r].data(), sizeof(int32_t) * ((size_t)w.n_lm + 1));
        int32_t *rk = (int32_t*)(h + o_rank) + pd.obs_off, *cm = (int32_t*)(h + o_cam) + pd.obs_off;
        float *u = (float*)(h + o_u) + pd.obs_off, *v = (float*)(h + o_v) + pd.obs_off, *dd = (float*)(h + o_d) + pd.obs_off;
        for (int a = 0; a < w.n_obs; ++a) {
            const int32_t o = orders[r][a];
            rk[a] = F.rank_of_kf[w.obs_kf[o]];
            cm[a] = w.obs_cam[o];
            u[a] = w.obs_u[o];
            v[a] = w.obs_v[o];
            dd[a] = w.obs_d[o];
        }
    }
    {
        Dev D;
        D.desc = (const PoolDesc*)(d + o_desc), D.add = (const ls::Add*)(d + o_add);
        D.T_kf = (const double*)(d + o_Tkf), D.path = (const double*)(d + o_path), D.T_cam = (const double*)(d + o_Tcam), D.lm_pos = (const double*)(d + o_pos);
        D.kf_by_time = (const int32_t*)(d + o_kbt), D.lm_obs = (const int32_t*)(d + o_lmobs), D.obs_rank = (const int32_t*)(d + o_rank), D.obs_cam = (const int32_t*)(d + o_cam);
        D.lm_id = (const uint64_t*)(d + o_id), D.lm_flags = (const uint8_t*)(d + o_flags);
        D.obs_u = (const float*)(d + o_u), D.obs_v = (const float*)(d + o_v), D.obs_d = (const float*)(d + o_d);
        D.p3 = (double*)(d + o_p3), D.dist = (double*)(d + o_dist);
        D.status = (uint8_t*)(d + o_status), D.cls = (uint8_t*)(d + o_cls), D.out = (uint8_t*)(d + o_out);
        D.ord = (uint64_t*)(d + o_ord), D.add_ord = (uint64_t*)(d + o_aord), D.sort_key = (uint64_t*)(d + o_skey), D.sort_idx = (uint32_t*)(d + o_sidx);
        D.flag = (int32_t*)(d + o_flag), D.total_lm = tot_lm;
        LS_TRY(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, s));
        LS_TRY(hipMemsetAsync(d + o_out, 0, host_bytes - o_out, s));  // out (padding bytes too) and the flags
        if (ctx->select_timing) {
            for (hipEvent_t& e : ev) LS_TRY(hipEventCreate(&e));
            LS_TRY(hipEventRecord(ev[0], s));
        }
        hipLaunchKernelGGL(k_ls_landmarks, dim3((max_sort + kLmThreads - 1) / kLmThreads, R), dim3(kLmThreads), 0, s, D, prm);
        LS_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_ls_voxels, dim3(R), dim3(kVoxelThreads), 0, s, D, prm);
        LS_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_ls_rank, dim3((max_lm + kRankThreads - 1) / kRankThreads, 1 + n_add, R), dim3(kRankThreads), 0, s, D, prm);
        LS_TRY(hipGetLastError());
        if (ctx->select_timing) LS_TRY(hipEventRecord(ev[1], s));
        LS_TRY(hipMemcpyAsync(h + o_out, d + o_out, host_bytes - o_out, hipMemcpyDeviceToHost, s));
        LS_TRY(hipStreamSynchronize(s));
        if (ctx->select_timing) {
            float ms = 0.f;
            LS_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
            ctx->select_last_ms = ms;
        }
    }
    for (int r = 0; r < R; ++r) {
        const limo_select_pool& w = pools[runs[r]];
        const PoolDesc& pd = desc[r];
        if (((const int32_t*)(h + o_flag))[r] == 0) {
            std::memcpy(out[runs[r]], h + o_out + pd.out_off, (size_t)w.n_lm);
            continue;
        }
        // cell indices outside (-2^20, 2^20): the host statement of the same header, on the packed pool
        ls::Pool P;
        P.n_kf = pd.n_kf, P.n_cam = pd.n_cam, P.n_lm = pd.n_lm, P.n_obs = pd.n_obs, P.newest = pd.newest, P.seed = pd.seed;
        P.T_kf = (const double*)(h + o_Tkf) + 12 * (size_t)pd.kf_off, P.path = (const double*)(h + o_path) + 3 * (size_t)pd.kf_off;
        P.kf_by_time = (const int32_t*)(h + o_kbt) + pd.kf_off, P.T_cam = (const double*)(h + o_Tcam) + 12 * (size_t)pd.cam_off;
        P.lm_id = (const uint64_t*)(h + o_id) + pd.lm_off, P.lm_pos = (const double*)(h + o_pos) + 3 * (size_t)pd.lm_off;
        P.lm_flags = (const uint8_t*)(h + o_flags) + pd.lm_off, P.lm_obs = (const int32_t*)(h + o_lmobs) + pd.lmobs_off;
        P.obs_rank = (const int32_t*)(h + o_rank) + pd.obs_off, P.obs_cam = (const int32_t*)(h + o_cam) + pd.obs_off;
        P.obs_u = (const float*)(h + o_u) + pd.obs_off, P.obs_v = (const float*)(h + o_v) + pd.obs_off, P.obs_d = (const float*)(h + o_d) + pd.obs_off;
        ls::select_host(P, prm, (const ls::Add*)(h + o_add), out[runs[r]]);
    }
done:
    // an error after work was queued: drain the stream before the blocks go back to the pools
    if (rc != LIMO_OK) (void)hipStreamSynchronize(s);
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (h) ctx->host_free(h, host_bytes);
    if (d) ctx->pool_free(d, dev_bytes);
    return rc;
}

}  // namespace

extern "C" void limo_select_default_params(limo_select_params* out) {
    if (!out) return;
    out->voxel_size_xyz[0] = 0.5, out->voxel_size_xyz[1] = 0.5, out->voxel_size_xyz[2] = 0.3;
    out->roi_far = 40., out->roi_middle = 15.;
    out->max_near = 200, out->max_middle = 200, out->max_far = 100;
    out->n_add = 0;
    out->add = nullptr;
    out->sort_capacity = 0;
}

extern "C" int limo_landmark_select(limo_ctx* ctx, const limo_select_pool* pool, const limo_select_params* params, uint8_t* out) {
    if (ctx && !pool) ctx->err = "limo_landmark_select: null pointer";
    if (!ctx || !pool) return LIMO_ERR_INVALID;
    return run(ctx, 1, pool, params, &out, "limo_landmark_select");
}

extern "C" int limo_landmark_select_batch(limo_ctx* ctx, int32_t n_pools, const limo_select_pool* pools, const limo_select_params* params,
                                          uint8_t* const* out) {
    return run(ctx, n_pools, pools, params, out, "limo_landmark_select_batch");
}

extern "C" int limo_select_set_timing(limo_ctx* ctx, int32_t on) {
    if (!ctx) return LIMO_ERR_INVALID;
    ctx->select_timing = on != 0;
    return LIMO_OK;
}

extern "C" int limo_select_last_kernel_ms(limo_ctx* ctx, double* ms) {
    if (!ctx || !ms) return LIMO_ERR_INVALID;
    *ms = ctx->select_last_ms;
    return LIMO_OK;
}
