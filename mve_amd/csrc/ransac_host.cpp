/*
 * ransac_host.cpp -- mi_dmrecon_ransac_fundamental of include/mi_dmrecon.h: a list of RANSAC jobs through the kernels of
 * ransac_device.hip in one upload, three launches and one download.  Every index a kernel reads comes from a job that was
 * checked HERE: sample indices against n_matches, and the sizes against what a launch and an int32 hold.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/mi_dmrecon.h"
#include "ransac_device.h"

/* dmrecon_host.cpp (not exported, exports.map): the thread-local error message, and the context's device and RANSAC state */
struct RansacState;
int mi_host_fail(int code, const char* msg);
int mi_host_ctx_device(const mi_dmrecon_ctx* c);
RansacState** mi_host_ctx_ransac(mi_dmrecon_ctx* c);

/* The buffers of a context's calls; they grow only and go with the context (mi_ransac_release). */
struct RansacState {
    size_t in_cap = 0, out_cap = 0;
    uint8_t* d_in = nullptr;                 /* jobs | matches | samples */
    uint8_t* h_in = nullptr;                 /* pinned, the same layout */
    uint8_t* d_out = nullptr;                /* F_best | best | inliers | counts | F_all */
    uint8_t* h_out = nullptr;                /* pinned */
    unsigned long long* d_capped = nullptr;
    unsigned long long capped = 0;           /* as of the last call */
};

void mi_ransac_release(RansacState* s) {
    if (!s) return;
    if (s->d_in) (void)hipFree(s->d_in);
    if (s->h_in) (void)hipHostFree(s->h_in);
    if (s->d_out) (void)hipFree(s->d_out);
    if (s->h_out) (void)hipHostFree(s->h_out);
    if (s->d_capped) (void)hipFree(s->d_capped);
    delete s;
}

namespace {

#define RANSAC_MAX_HYP (1ll << 30)           /* hypotheses / matches of a call: indices stay far inside int32 / the buffers small */
#define RANSAC_MAX_BLOCKS ((1ll << 24) - 1)  /* workgroups of a launch */

int failf(int code, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), fmt, a, b, c);
    return mi_host_fail(code, buf);
}

#define RANSAC_HIP(expr)                                                                      \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            char _b[256];                                                                     \
            std::snprintf(_b, sizeof(_b), "%s failed: %s", #expr, hipGetErrorString(_e));     \
            return mi_host_fail(MI_DMRECON_EDEVICE, _b);                                      \
        }                                                                                     \
    } while (0)

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

int validate(int32_t n_jobs, const mi_dmrecon_ransac_job* jobs) {
    for (int32_t j = 0; j < n_jobs; ++j) {
        const mi_dmrecon_ransac_job& q = jobs[j];
        if (q.n_matches < 8) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has %lld matches, at least 8 matches required", j, q.n_matches);
        if (q.n_iterations < 1) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has %lld iterations, at least 1 required", j, q.n_iterations);
        if (!q.matches || !q.samples) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has null matches or samples", j);
        if (q.inliers_to_beat < 0) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has a negative inliers_to_beat", j);
        if (!(q.threshold == q.threshold)) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has a threshold that is not a number", j);
        for (int32_t it = 0; it < q.n_iterations; ++it) {
            const int32_t* r = q.samples + (size_t)it * 8;
            for (int a = 0; a < 8; ++a) {
                if (r[a] < 0 || r[a] >= q.n_matches)
                    return failf(MI_DMRECON_EINVAL, "ransac: job %lld, sample row %lld: index %lld outside the matches", j, it, r[a]);
                for (int b = 0; b < a; ++b)
                    if (r[a] == r[b])
                        return failf(MI_DMRECON_EINVAL, "ransac: job %lld, sample row %lld: index %lld is repeated", j, it, r[a]);
            }
        }
    }
    return 0;
}

int grow(RansacState& s, size_t in_bytes, size_t out_bytes) {
    if (!s.d_capped) {
        RANSAC_HIP(hipMalloc((void**)&s.d_capped, sizeof(unsigned long long)));
        RANSAC_HIP(hipMemset(s.d_capped, 0, sizeof(unsigned long long)));
    }
    if (in_bytes > s.in_cap) {
        if (s.d_in) (void)hipFree(s.d_in);
        if (s.h_in) (void)hipHostFree(s.h_in);
        s.d_in = nullptr; s.h_in = nullptr; s.in_cap = 0;
        RANSAC_HIP(hipMalloc((void**)&s.d_in, in_bytes));
        RANSAC_HIP(hipHostMalloc((void**)&s.h_in, in_bytes, hipHostMallocDefault));
        s.in_cap = in_bytes;
    }
    if (out_bytes > s.out_cap) {
        if (s.d_out) (void)hipFree(s.d_out);
        if (s.h_out) (void)hipHostFree(s.h_out);
        s.d_out = nullptr; s.h_out = nullptr; s.out_cap = 0;
        RANSAC_HIP(hipMalloc((void**)&s.d_out, out_bytes));
        RANSAC_HIP(hipHostMalloc((void**)&s.h_out, out_bytes, hipHostMallocDefault));
        s.out_cap = out_bytes;
    }
    return 0;
}

int ransac_impl(mi_dmrecon_ctx* ctx, int32_t n_jobs, const mi_dmrecon_ransac_job* jobs, int32_t* best_iteration, double* fundamental,
                int32_t* n_inliers, int32_t* const* inliers, int32_t* const* iteration_counts, double* const* iteration_F) {
    if (!ctx) return failf(MI_DMRECON_EINVAL, "ransac: null context");
    if (n_jobs < 0) return failf(MI_DMRECON_EINVAL, "ransac: negative number of jobs");
    if (n_jobs == 0) return 0;
    if (!jobs || !best_iteration || !fundamental || !n_inliers || !inliers) return failf(MI_DMRECON_EINVAL, "ransac: null argument");
    for (int32_t j = 0; j < n_jobs; ++j)
        if (!inliers[j]) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has no room for its inliers", j);
    if (int rc = validate(n_jobs, jobs)) return rc;

    /* the prefix table: where each job's workgroups, hypotheses and matches start */
    std::vector<RansacJobDev> dev(n_jobs);
    long long blocks = 0, hyps = 0, matches = 0;
    for (int32_t j = 0; j < n_jobs; ++j) {
        const mi_dmrecon_ransac_job& q = jobs[j];
        RansacJobDev& d = dev[j];
        d.n_matches = q.n_matches; d.n_iterations = q.n_iterations; d.inliers_to_beat = q.inliers_to_beat;
        d.chunks = (q.n_matches + RANSAC_CHUNK - 1) / RANSAC_CHUNK;
        d.block0 = (int32_t)blocks; d.hyp0 = (int32_t)hyps; d.match0 = matches;
        d.thr2 = q.threshold * q.threshold;
        blocks += (long long)((q.n_iterations + RANSAC_TILE - 1) / RANSAC_TILE) * d.chunks;
        hyps += q.n_iterations; matches += q.n_matches;
        if (blocks > RANSAC_MAX_BLOCKS || hyps > RANSAC_MAX_HYP || matches > RANSAC_MAX_HYP)
            return failf(MI_DMRECON_EINVAL, "ransac: with job %lld the call has more than 2^24 - 1 workgroups, or 2^30 iterations or matches", j);
    }
    bool per_iteration = false;
    for (int32_t j = 0; j < n_jobs; ++j)
        per_iteration = per_iteration || (iteration_counts && iteration_counts[j]) || (iteration_F && iteration_F[j]);

    const size_t in_matches = align256((size_t)n_jobs * sizeof(RansacJobDev));
    const size_t in_samples = in_matches + align256((size_t)matches * 4 * sizeof(double));
    const size_t in_bytes = in_samples + align256((size_t)hyps * 8 * sizeof(int32_t));
    const size_t out_best = align256((size_t)n_jobs * 9 * sizeof(double));
    const size_t out_inliers = out_best + align256((size_t)n_jobs * 2 * sizeof(int32_t));
    const size_t out_counts = out_inliers + align256((size_t)matches * sizeof(int32_t));
    const size_t out_F = out_counts + align256((size_t)hyps * sizeof(int32_t));
    const size_t out_bytes = out_F + align256((size_t)hyps * 9 * sizeof(double));

    RANSAC_HIP(hipSetDevice(mi_host_ctx_device(ctx)));
    RansacState*& state = *mi_host_ctx_ransac(ctx);
    if (!state) state = new RansacState();
    RansacState& s = *state;
    if (int rc = grow(s, in_bytes, out_bytes)) return rc;
    hipStream_t stream = (hipStream_t)mi_dmrecon_ctx_stream(ctx);

    std::memcpy(s.h_in, dev.data(), (size_t)n_jobs * sizeof(RansacJobDev));
    for (int32_t j = 0; j < n_jobs; ++j) {
        std::memcpy(s.h_in + in_matches + (size_t)dev[j].match0 * 4 * sizeof(double), jobs[j].matches,
                    (size_t)jobs[j].n_matches * 4 * sizeof(double));
        std::memcpy(s.h_in + in_samples + (size_t)dev[j].hyp0 * 8 * sizeof(int32_t), jobs[j].samples,
                    (size_t)jobs[j].n_iterations * 8 * sizeof(int32_t));
    }
    RANSAC_HIP(hipMemcpyAsync(s.d_in, s.h_in, in_bytes, hipMemcpyHostToDevice, stream));

    RansacBuffers b;
    b.jobs = (const RansacJobDev*)s.d_in;
    b.matches = (const double*)(s.d_in + in_matches);
    b.samples = (const int32_t*)(s.d_in + in_samples);
    b.F_best = (double*)s.d_out;
    b.best = (int32_t*)(s.d_out + out_best);
    b.inliers = (int32_t*)(s.d_out + out_inliers);
    b.counts = (int32_t*)(s.d_out + out_counts);
    b.F_all = (double*)(s.d_out + out_F);
    b.capped = s.d_capped;
    mi_ransac_launch(stream, b, n_jobs, (int32_t)hyps, (int32_t)blocks);
    RANSAC_HIP(hipGetLastError());
    RANSAC_HIP(hipMemcpyAsync(s.h_out, s.d_out, per_iteration ? out_bytes : out_counts, hipMemcpyDeviceToHost, stream));
    RANSAC_HIP(hipMemcpyAsync(&s.capped, s.d_capped, sizeof(s.capped), hipMemcpyDeviceToHost, stream));
    RANSAC_HIP(hipStreamSynchronize(stream));

    const double* h_Fbest = (const double*)s.h_out;
    const int32_t* h_best = (const int32_t*)(s.h_out + out_best);
    const int32_t* h_inliers = (const int32_t*)(s.h_out + out_inliers);
    const int32_t* h_counts = (const int32_t*)(s.h_out + out_counts);
    const double* h_F = (const double*)(s.h_out + out_F);
    for (int32_t j = 0; j < n_jobs; ++j) {
        if (iteration_counts && iteration_counts[j])
            std::memcpy(iteration_counts[j], h_counts + dev[j].hyp0, (size_t)dev[j].n_iterations * sizeof(int32_t));
        if (iteration_F && iteration_F[j])
            std::memcpy(iteration_F[j], h_F + (size_t)dev[j].hyp0 * 9, (size_t)dev[j].n_iterations * 9 * sizeof(double));
        best_iteration[j] = h_best[2 * j];
        if (h_best[2 * j] < 0) continue;                         /* nothing beat inliers_to_beat: the rest stays as it was */
        n_inliers[j] = h_best[2 * j + 1];
        std::memcpy(fundamental + (size_t)j * 9, h_Fbest + (size_t)j * 9, 9 * sizeof(double));
        std::memcpy(inliers[j], h_inliers + dev[j].match0, (size_t)h_best[2 * j + 1] * sizeof(int32_t));
    }
    return 0;
}

}  /* namespace */

extern "C" {

int mi_dmrecon_ransac_fundamental(mi_dmrecon_ctx* ctx, int32_t n_jobs, const mi_dmrecon_ransac_job* jobs, int32_t* best_iteration,
                                  double* fundamental, int32_t* n_inliers, int32_t* const* inliers, int32_t* const* iteration_counts,
                                  double* const* iteration_F) {
    try { return ransac_impl(ctx, n_jobs, jobs, best_iteration, fundamental, n_inliers, inliers, iteration_counts, iteration_F); }
    catch (const std::bad_alloc&) { return mi_host_fail(MI_DMRECON_EDEVICE, "out of host memory"); }
}

long long mi_dmrecon_ransac_sweep_capped(mi_dmrecon_ctx* ctx) {
    RansacState* s = ctx ? *mi_host_ctx_ransac(ctx) : nullptr;
    return s ? (long long)s->capped : 0;
}

}  /* extern "C" */
