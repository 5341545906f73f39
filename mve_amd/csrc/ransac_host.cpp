/*
 * ransac_host.cpp -- mi_dmrecon_ransac_fundamental, _homography and _pose_p3p of include/mi_dmrecon.h: a list of RANSAC jobs
 * of one model through the kernels of ransac_device.hip in one upload, three launches and one download.  Every index a
 * kernel reads comes from a job that was checked HERE: sample indices against the list's length, and the sizes against what
 * a launch and an int32 hold.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "host_common.h"
#include "ransac_device.h"

namespace {

/* The buffers of a context's calls; they grow only and go with the context. */
struct RansacState : HostModule {
    Buf d_in;                                /* jobs | list | samples */
    PinnedBuf h_in;                          /* the same layout */
    Buf d_out;                               /* best_model | best | inliers | counts | hyp_all */
    PinnedBuf h_out;
    Buf d_capped;                            /* one unsigned long long, zeroed when it is made */
    unsigned long long capped = 0;           /* as of the last call */
};

#define RANSAC_MAX_HYP (1ll << 30)           /* hypotheses / matches of a call: indices stay far inside int32 / the buffers small */
#define RANSAC_MAX_BLOCKS ((1ll << 24) - 1)  /* workgroups of a launch */

/* What the host has to know of a model (ransac_device.h has the kernels' side). */
struct Model {
    RansacModel id;
    const char* entries;          /* what the list holds, for the messages */
    int sample;                   /* indices per iteration, = the fewest entries a job may have */
    int entry_in, entry_dev;      /* doubles per list entry: as the caller has them, as the kernels read them */
    int per_iteration;            /* hypotheses per iteration */
    int hyp;                      /* doubles per hypothesis on the device ... */
    int all_off, all_n;           /* ... of which these leave through the optional per-hypothesis output */
    int best;                     /* doubles of the winner's output */
};
const Model MODEL_F = {RANSAC_F, "matches", 8, 4, 4, 1, RANSAC_F_HYP, 0, 9, 9};
const Model MODEL_H = {RANSAC_H, "matches", 4, 4, 4, 1, RANSAC_H_HYP, 0, 9, 9};
const Model MODEL_P3P = {RANSAC_P3P, "correspondences", 3, 5, RANSAC_P3P_ENTRY, 4, RANSAC_P3P_HYP, 12, 12, 12};

/* One job of any model */
struct Job {
    int32_t n, n_iterations, inliers_to_beat;
    const double* list;
    const int32_t* samples;
    double threshold;
    const double* k_matrix;       /* P3P only */
};

Job job_of(const mi_dmrecon_ransac_job& q) { return {q.n_matches, q.n_iterations, q.inliers_to_beat, q.matches, q.samples, q.threshold, nullptr}; }
Job job_of(const mi_dmrecon_ransac_p3p_job& q) { return {q.n_corr, q.n_iterations, q.inliers_to_beat, q.corr, q.samples, q.threshold, q.k_matrix}; }

/* K^-1 by adjugate over determinant; false for a K that has none */
bool invert3(const double* k, double* inv) {
    const double c0 = k[4] * k[8] - k[5] * k[7], c1 = k[5] * k[6] - k[3] * k[8], c2 = k[3] * k[7] - k[4] * k[6];
    const double det = k[0] * c0 + k[1] * c1 + k[2] * c2;
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
    inv[0] = c0 / det; inv[1] = (k[2] * k[7] - k[1] * k[8]) / det; inv[2] = (k[1] * k[5] - k[2] * k[4]) / det;
    inv[3] = c1 / det; inv[4] = (k[0] * k[8] - k[2] * k[6]) / det; inv[5] = (k[2] * k[3] - k[0] * k[5]) / det;
    inv[6] = c2 / det; inv[7] = (k[1] * k[6] - k[0] * k[7]) / det; inv[8] = (k[0] * k[4] - k[1] * k[3]) / det;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(inv[i])) return false;
    return true;
}

int validate(const Model& M, const std::vector<Job>& jobs) {
    char buf[256];
    for (int32_t j = 0; j < (int32_t)jobs.size(); ++j) {
        const Job& q = jobs[j];
        if (q.n < M.sample) {
            std::snprintf(buf, sizeof(buf), "ransac: job %d has %d %s, at least %d %s required", j, q.n, M.entries, M.sample, M.entries);
            return mi_host_fail(MI_DMRECON_EINVAL, buf);
        }
        if (q.n_iterations < 1) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has %lld iterations, at least 1 required", j, q.n_iterations);
        if (!q.list || !q.samples) {
            std::snprintf(buf, sizeof(buf), "ransac: job %d has null %s or samples", j, M.entries);
            return mi_host_fail(MI_DMRECON_EINVAL, buf);
        }
        if (q.inliers_to_beat < 0) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has a negative inliers_to_beat", j);
        if (!(q.threshold == q.threshold)) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has a threshold that is not a number", j);
        double inv[9];
        if (M.id == RANSAC_P3P && !invert3(q.k_matrix, inv)) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has a k_matrix without an inverse", j);
        for (int32_t it = 0; it < q.n_iterations; ++it) {
            const int32_t* r = q.samples + (size_t)it * M.sample;
            for (int a = 0; a < M.sample; ++a) {
                if (r[a] < 0 || r[a] >= q.n) {
                    std::snprintf(buf, sizeof(buf), "ransac: job %d, sample row %d: index %d outside the %s", j, it, r[a], M.entries);
                    return mi_host_fail(MI_DMRECON_EINVAL, buf);
                }
                for (int b = 0; b < a; ++b)
                    if (r[a] == r[b])
                        return failf(MI_DMRECON_EINVAL, "ransac: job %lld, sample row %lld: index %lld is repeated", j, it, r[a]);
            }
        }
    }
    return 0;
}

/* The prefix table: where each job's workgroups, hypotheses and list entries start, for a model whose iteration draws
 * `sample` indices (only its lower bound on the list is used here: validate has checked it), whose list entry is
 * `entry_dev` doubles on the device and which makes `per_iteration` hypotheses per iteration. */
struct Plan {
    std::vector<RansacJobDev> dev;
    long long blocks = 0, hyps = 0, entries = 0;
    size_t in_list = 0, in_samples = 0, in_bytes = 0;
};
int plan(const std::vector<Job>& jobs, int sample, int entry_dev, int per_iteration, Plan& p) {
    p.dev.assign(jobs.size(), RansacJobDev());
    for (int32_t j = 0; j < (int32_t)jobs.size(); ++j) {
        const Job& q = jobs[j];
        RansacJobDev& d = p.dev[j];
        const long long n_hyp = (long long)q.n_iterations * per_iteration;
        d.n_matches = q.n; d.n_hyp = (int32_t)n_hyp; d.inliers_to_beat = q.inliers_to_beat;
        d.chunks = (q.n + RANSAC_CHUNK - 1) / RANSAC_CHUNK;
        d.block0 = (int32_t)p.blocks; d.hyp0 = (int32_t)p.hyps; d.match0 = p.entries;
        d.thr2 = q.threshold * q.threshold;
        p.blocks += ((n_hyp + RANSAC_TILE - 1) / RANSAC_TILE) * d.chunks;
        p.hyps += n_hyp; p.entries += q.n;
        if (p.blocks > RANSAC_MAX_BLOCKS || p.hyps > RANSAC_MAX_HYP || p.entries > RANSAC_MAX_HYP)
            return failf(MI_DMRECON_EINVAL, "ransac: with job %lld the call has more than 2^24 - 1 workgroups, or 2^30 hypotheses or list entries", j);
    }
    p.in_list = align256(jobs.size() * sizeof(RansacJobDev));
    p.in_samples = p.in_list + align256((size_t)p.entries * entry_dev * sizeof(double));
    p.in_bytes = p.in_samples + align256((size_t)(p.hyps / per_iteration) * sample * sizeof(int32_t));
    return 0;
}

int grow(RansacState& s, size_t in_bytes, size_t out_bytes) {
    if (!s.d_capped.p) {
        MI_HIP(s.d_capped.need(sizeof(unsigned long long)));
        MI_HIP(hipMemset(s.d_capped.p, 0, sizeof(unsigned long long)));
    }
    /* (the device and the pinned half of a pair are asked for the same size every time, so they grow together) */
    MI_HIP(s.d_in.need(in_bytes));
    MI_HIP(s.h_in.need(in_bytes));
    MI_HIP(s.d_out.need(out_bytes));
    MI_HIP(s.h_out.need(out_bytes));
    return 0;
}

int ransac_impl(const Model& M, mi_dmrecon_ctx* ctx, const std::vector<Job>& jobs, int32_t* best_hypothesis, double* model,
                int32_t* n_inliers, int32_t* const* inliers, int32_t* const* hypothesis_counts, double* const* hypothesis_all) {
    const int32_t n_jobs = (int32_t)jobs.size();
    if (n_jobs == 0) return 0;
    if (!best_hypothesis || !model || !n_inliers || !inliers) return failf(MI_DMRECON_EINVAL, "ransac: null argument");
    for (int32_t j = 0; j < n_jobs; ++j)
        if (!inliers[j]) return failf(MI_DMRECON_EINVAL, "ransac: job %lld has no room for its inliers", j);
    if (int rc = validate(M, jobs)) return rc;

    Plan p;
    if (int rc = plan(jobs, M.sample, M.entry_dev, M.per_iteration, p)) return rc;
    const std::vector<RansacJobDev>& dev = p.dev;
    bool per_hypothesis = false;
    for (int32_t j = 0; j < n_jobs; ++j) {
        per_hypothesis = per_hypothesis || (hypothesis_counts && hypothesis_counts[j]) || (hypothesis_all && hypothesis_all[j]);
        if (M.id == RANSAC_P3P) {
            std::memcpy(p.dev[j].k, jobs[j].k_matrix, 9 * sizeof(double));
            invert3(jobs[j].k_matrix, p.dev[j].k_inv);
        }
    }

    const size_t out_best = align256((size_t)n_jobs * M.best * sizeof(double));
    const size_t out_inliers = out_best + align256((size_t)n_jobs * 2 * sizeof(int32_t));
    const size_t out_counts = out_inliers + align256((size_t)p.entries * sizeof(int32_t));
    const size_t out_hyp = out_counts + align256((size_t)p.hyps * sizeof(int32_t));
    const size_t out_bytes = out_hyp + align256((size_t)p.hyps * M.hyp * sizeof(double));

    MI_HIP(hipSetDevice(mi_host_ctx_device(ctx)));
    HostModule*& state = mi_host_ctx_module(ctx, MI_MODULE_RANSAC);
    if (!state) state = new RansacState();
    RansacState& s = *static_cast<RansacState*>(state);
    if (int rc = grow(s, p.in_bytes, out_bytes)) return rc;
    hipStream_t stream = (hipStream_t)mi_dmrecon_ctx_stream(ctx);
    uint8_t* const h_in = (uint8_t*)s.h_in.p;
    uint8_t* const d_in = (uint8_t*)s.d_in.p;
    uint8_t* const d_out = (uint8_t*)s.d_out.p;
    const uint8_t* const h_out = (const uint8_t*)s.h_out.p;

    std::memcpy(h_in, dev.data(), (size_t)n_jobs * sizeof(RansacJobDev));
    for (int32_t j = 0; j < n_jobs; ++j) {
        double* list = (double*)(h_in + p.in_list) + (size_t)dev[j].match0 * M.entry_dev;
        if (M.entry_in == M.entry_dev)
            std::memcpy(list, jobs[j].list, (size_t)jobs[j].n * M.entry_dev * sizeof(double));
        else
            for (int32_t i = 0; i < jobs[j].n; ++i) {             /* (the pad stays defined: nothing reads it) */
                std::memcpy(list + (size_t)i * M.entry_dev, jobs[j].list + (size_t)i * M.entry_in, M.entry_in * sizeof(double));
                for (int k = M.entry_in; k < M.entry_dev; ++k) list[(size_t)i * M.entry_dev + k] = 0.0;
            }
        std::memcpy(h_in + p.in_samples + (size_t)(dev[j].hyp0 / M.per_iteration) * M.sample * sizeof(int32_t), jobs[j].samples,
                    (size_t)jobs[j].n_iterations * M.sample * sizeof(int32_t));
    }
    MI_HIP(hipMemcpyAsync(d_in, h_in, p.in_bytes, hipMemcpyHostToDevice, stream));

    RansacBuffers b;
    b.jobs = (const RansacJobDev*)d_in;
    b.list = (const double*)(d_in + p.in_list);
    b.samples = (const int32_t*)(d_in + p.in_samples);
    b.best_model = (double*)d_out;
    b.best = (int32_t*)(d_out + out_best);
    b.inliers = (int32_t*)(d_out + out_inliers);
    b.counts = (int32_t*)(d_out + out_counts);
    b.hyp_all = (double*)(d_out + out_hyp);
    b.capped = (unsigned long long*)s.d_capped.p;
    mi_ransac_launch(stream, M.id, b, n_jobs, (int32_t)p.hyps, (int32_t)p.blocks);
    MI_HIP(hipGetLastError());
    MI_HIP(hipMemcpyAsync(s.h_out.p, d_out, per_hypothesis ? out_bytes : out_counts, hipMemcpyDeviceToHost, stream));
    MI_HIP(hipMemcpyAsync(&s.capped, s.d_capped.p, sizeof(s.capped), hipMemcpyDeviceToHost, stream));
    MI_HIP(hipStreamSynchronize(stream));

    const double* h_model = (const double*)h_out;
    const int32_t* h_best = (const int32_t*)(h_out + out_best);
    const int32_t* h_inliers = (const int32_t*)(h_out + out_inliers);
    const int32_t* h_counts = (const int32_t*)(h_out + out_counts);
    const double* h_hyp = (const double*)(h_out + out_hyp);
    for (int32_t j = 0; j < n_jobs; ++j) {
        if (hypothesis_counts && hypothesis_counts[j])
            std::memcpy(hypothesis_counts[j], h_counts + dev[j].hyp0, (size_t)dev[j].n_hyp * sizeof(int32_t));
        if (hypothesis_all && hypothesis_all[j])
            for (int32_t h = 0; h < dev[j].n_hyp; ++h)
                std::memcpy(hypothesis_all[j] + (size_t)h * M.all_n, h_hyp + (size_t)(dev[j].hyp0 + h) * M.hyp + M.all_off, M.all_n * sizeof(double));
        best_hypothesis[j] = h_best[2 * j];
        if (h_best[2 * j] < 0) continue;                         /* nothing beat inliers_to_beat: the rest stays as it was */
        n_inliers[j] = h_best[2 * j + 1];
        std::memcpy(model + (size_t)j * M.best, h_model + (size_t)j * M.best, M.best * sizeof(double));
        std::memcpy(inliers[j], h_inliers + dev[j].match0, (size_t)h_best[2 * j + 1] * sizeof(int32_t));
    }
    return 0;
}

template <class CJob>
int ransac_entry(const Model& M, mi_dmrecon_ctx* ctx, int32_t n_jobs, const CJob* jobs, int32_t* best, double* model, int32_t* n_inliers,
                 int32_t* const* inliers, int32_t* const* counts, double* const* all) {
    return guarded([&] {
        if (!ctx) return failf(MI_DMRECON_EINVAL, "ransac: null context");
        if (n_jobs < 0) return failf(MI_DMRECON_EINVAL, "ransac: negative number of jobs");
        if (n_jobs > 0 && !jobs) return failf(MI_DMRECON_EINVAL, "ransac: null argument");
        std::vector<Job> list;
        list.reserve(n_jobs);
        for (int32_t j = 0; j < n_jobs; ++j) list.push_back(job_of(jobs[j]));
        return ransac_impl(M, ctx, list, best, model, n_inliers, inliers, counts, all);
    });
}

}  /* namespace */

extern "C" {

int mi_dmrecon_ransac_fundamental(mi_dmrecon_ctx* ctx, int32_t n_jobs, const mi_dmrecon_ransac_job* jobs, int32_t* best_iteration,
                                  double* fundamental, int32_t* n_inliers, int32_t* const* inliers, int32_t* const* iteration_counts,
                                  double* const* iteration_F) {
    return ransac_entry(MODEL_F, ctx, n_jobs, jobs, best_iteration, fundamental, n_inliers, inliers, iteration_counts, iteration_F);
}

int mi_dmrecon_ransac_homography(mi_dmrecon_ctx* ctx, int32_t n_jobs, const mi_dmrecon_ransac_job* jobs, int32_t* best_iteration,
                                 double* homography, int32_t* n_inliers, int32_t* const* inliers, int32_t* const* iteration_counts,
                                 double* const* iteration_H) {
    return ransac_entry(MODEL_H, ctx, n_jobs, jobs, best_iteration, homography, n_inliers, inliers, iteration_counts, iteration_H);
}

int mi_dmrecon_ransac_pose_three_point(mi_dmrecon_ctx* ctx, int32_t n_jobs, const mi_dmrecon_ransac_p3p_job* jobs, int32_t* best_hypothesis,
                               double* pose, int32_t* n_inliers, int32_t* const* inliers, int32_t* const* hypothesis_counts,
                               double* const* hypothesis_pose) {
    return ransac_entry(MODEL_P3P, ctx, n_jobs, jobs, best_hypothesis, pose, n_inliers, inliers, hypothesis_counts, hypothesis_pose);
}

long long mi_dmrecon_ransac_sweep_capped(mi_dmrecon_ctx* ctx) {
    const RansacState* s = ctx ? static_cast<RansacState*>(mi_host_ctx_module(ctx, MI_MODULE_RANSAC)) : nullptr;
    return s ? (long long)s->capped : 0;
}

}  /* extern "C" */
