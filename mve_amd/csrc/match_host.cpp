/*
 * match_host.cpp -- the mi_dmrecon_match_* entry points of include/mi_dmrecon.h: descriptor sets resident on the device as
 * bytes, and batches of (set a, n_a, set b, n_b) jobs through the kernels of match_device.hip.  Every index a kernel reads
 * comes from a job that was checked HERE against the sizes of the sets.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/mi_dmrecon.h"
#include "../../include/mi_dmrecon_debug.h"
#include "match_device.h"

/* dmrecon_host.cpp: the thread-local error message and the context's device (not exported, exports.map) */
int mi_host_fail(int code, const char* msg);
int mi_host_ctx_device(const mi_dmrecon_ctx* c);

static_assert(MI_DMRECON_MATCH_SIFT == MATCH_SIFT && MI_DMRECON_MATCH_SURF == MATCH_SURF, "descriptor kinds");

namespace {

#define MATCH_SLOTS 4                        /* calls of mi_dmrecon_match_pairs in flight on one handle */
#define MATCH_BATCH_ENTRIES (1ll << 26)      /* rows + columns per pair of launches (16 bytes of keys each) */
#define MATCH_BATCH_BLOCKS ((1ll << 24) - 1)  /* workgroups per launch: HIP wants gridDim.x * blockDim.x < 2^32, the workgroups have 256 threads */

/* the limits in force: the two above unless mi_dmrecon_debug_match_limits replaced them */
std::atomic<long long> g_batch_entries(MATCH_BATCH_ENTRIES), g_batch_blocks(MATCH_BATCH_BLOCKS);

struct MatchSet {
    int32_t n = 0;
    int8_t* d_desc = nullptr;                /* n rows of 128 / 64 bytes */
    int32_t* d_off = nullptr;                /* MatchJobDev::off */
};

/* A stream and the buffers of one call; they grow only. */
struct MatchSlot {
    hipStream_t stream = nullptr;
    bool busy = false;
    size_t jobs_cap = 0, entries_cap = 0;
    MatchJobDev* d_jobs = nullptr;
    unsigned long long* d_best = nullptr;
    int32_t* d_matches = nullptr;
    int32_t* h_matches = nullptr;            /* pinned */
};

}  /* namespace */

struct mi_dmrecon_match {
    int device = -1;
    int32_t n_sets = 0;
    std::vector<MatchSet> sets[2];           /* by kind */
    std::mutex mu;
    std::condition_variable cv;
    MatchSlot slots[MATCH_SLOTS];
};

namespace {

int failf(int code, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), fmt, a, b, c);
    return mi_host_fail(code, buf);
}

#define MATCH_HIP(expr)                                                                       \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            char _b[256];                                                                     \
            std::snprintf(_b, sizeof(_b), "%s failed: %s", #expr, hipGetErrorString(_e));     \
            return mi_host_fail(MI_DMRECON_EDEVICE, _b);                                      \
        }                                                                                     \
    } while (0)

int dims_of(int kind) { return kind == MATCH_SIFT ? 128 : 64; }

void free_set(MatchSet& s) {
    if (s.d_desc) (void)hipFree(s.d_desc);
    if (s.d_off) (void)hipFree(s.d_off);
    s = MatchSet();
}

void release(mi_dmrecon_match* m) {
    if (!m) return;
    if (m->device >= 0) (void)hipSetDevice(m->device);
    for (int k = 0; k < 2; ++k)
        for (MatchSet& s : m->sets[k]) free_set(s);
    for (MatchSlot& s : m->slots) {
        if (s.stream) { (void)hipStreamSynchronize(s.stream); (void)hipStreamDestroy(s.stream); }
        if (s.d_jobs) (void)hipFree(s.d_jobs);
        if (s.d_best) (void)hipFree(s.d_best);
        if (s.d_matches) (void)hipFree(s.d_matches);
        if (s.h_matches) (void)hipHostFree(s.h_matches);
    }
    delete m;
}

/* A free slot for the length of a call. */
struct SlotLease {
    mi_dmrecon_match* m;
    MatchSlot* slot = nullptr;
    explicit SlotLease(mi_dmrecon_match* m_) : m(m_) {
        std::unique_lock<std::mutex> lock(m->mu);
        for (;;) {
            for (MatchSlot& s : m->slots)
                if (!s.busy) { s.busy = true; slot = &s; return; }
            m->cv.wait(lock);
        }
    }
    ~SlotLease() {
        { std::lock_guard<std::mutex> lock(m->mu); slot->busy = false; }
        m->cv.notify_one();
    }
};

int create_impl(mi_dmrecon_ctx* ctx, int32_t n_sets, mi_dmrecon_match** out) {
    if (!out) return failf(MI_DMRECON_EINVAL, "match: null argument");
    *out = nullptr;
    if (n_sets < 0) return failf(MI_DMRECON_EINVAL, "match: negative number of sets");
    if (!ctx) return failf(MI_DMRECON_EINVAL, "match: null context");
    const int device = mi_host_ctx_device(ctx);
    if (device < 0) return failf(MI_DMRECON_EINVAL, "match: the context has no device");
    MATCH_HIP(hipSetDevice(device));
    mi_dmrecon_match* m = new mi_dmrecon_match();
    m->device = device; m->n_sets = n_sets;
    m->sets[0].resize(n_sets); m->sets[1].resize(n_sets);
    *out = m;
    return 0;
}

int set_impl(mi_dmrecon_match* m, int32_t set, int32_t kind, int32_t dtype, int32_t n, const void* descriptors) {
    if (!m) return failf(MI_DMRECON_EINVAL, "match: null handle");
    if (kind != MATCH_SIFT && kind != MATCH_SURF) return failf(MI_DMRECON_EINVAL, "match: unknown descriptor kind %lld", kind);
    if (dtype != MI_DMRECON_MATCH_F32 && dtype != MI_DMRECON_MATCH_I16) return failf(MI_DMRECON_EINVAL, "match: unknown dtype %lld", dtype);
    if (set < 0 || set >= m->n_sets) return failf(MI_DMRECON_EINVAL, "match: set %lld outside [0, %lld)", set, m->n_sets);
    if (n < 0 || n > (1 << 24)) return failf(MI_DMRECON_EINVAL, "match: %lld descriptors (0 ... 2^24 allowed)", n);
    if (n > 0 && !descriptors) return failf(MI_DMRECON_EINVAL, "match: null descriptors");
    const int D = dims_of(kind);
    const size_t count = (size_t)n * D;

    /* the reference's in-memory form: 16-bit words that hold 8-bit values (exhaustive_matching.h:47-48) */
    std::vector<int8_t> bytes;
    std::vector<int32_t> off;
    if (dtype == MI_DMRECON_MATCH_I16 && n > 0) {
        bytes.resize(count); off.resize(n);
        for (int32_t i = 0; i < n; ++i) {
            int sum = 0;
            for (int j = 0; j < D; ++j) {
                int v;
                if (kind == MATCH_SIFT) {
                    v = ((const uint16_t*)descriptors)[(size_t)i * D + j];
                    if (v > 255) return failf(MI_DMRECON_EINVAL, "match: descriptor %lld component %lld is %lld, outside 0 ... 255", i, j, v);
                    v -= 128;
                } else {
                    v = ((const int16_t*)descriptors)[(size_t)i * D + j];
                    if (v < -128 || v > 127) return failf(MI_DMRECON_EINVAL, "match: descriptor %lld component %lld is %lld, outside -128 ... 127", i, j, v);
                }
                bytes[(size_t)i * D + j] = (int8_t)v;
                sum += v;
            }
            off[i] = kind == MATCH_SIFT ? 128 * sum + (1 << 20) : 0;
        }
    }

    std::lock_guard<std::mutex> lock(m->mu);
    MATCH_HIP(hipSetDevice(m->device));
    MatchSet& s = m->sets[kind][set];
    free_set(s);
    if (n == 0) return 0;
    MatchSet t;
    t.n = n;
    hipError_t e = hipMalloc((void**)&t.d_desc, count);
    if (e == hipSuccess) e = hipMalloc((void**)&t.d_off, (size_t)n * sizeof(int32_t));
    if (e == hipSuccess && dtype == MI_DMRECON_MATCH_I16) {
        e = hipMemcpy(t.d_desc, bytes.data(), count, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(t.d_off, off.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
    } else if (e == hipSuccess) {
        float* d_src = nullptr;
        e = hipMalloc((void**)&d_src, count * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(d_src, descriptors, count * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            mi_match_discretise(nullptr, kind, n, d_src, t.d_desc, t.d_off);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (d_src) (void)hipFree(d_src);
    }
    if (e != hipSuccess) {
        free_set(t);
        char b[200];
        std::snprintf(b, sizeof(b), "match: upload failed: %s", hipGetErrorString(e));
        return mi_host_fail(MI_DMRECON_EDEVICE, b);
    }
    s = t;
    return 0;
}

int count_consistent(const int32_t* ab, int32_t n_a, const int32_t* ba) {   /* Matching::count_consistent_matches, matching.cc:38-47 */
    int counter = 0;
    for (int32_t i = 0; i < n_a; ++i)
        if (ab[i] != -1 && ba[ab[i]] == i) ++counter;
    return counter;
}

int grow(MatchSlot& s, size_t n_jobs, size_t n_entries) {
    if (!s.stream) MATCH_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    if (n_jobs > s.jobs_cap) {
        if (s.d_jobs) (void)hipFree(s.d_jobs);
        s.d_jobs = nullptr; s.jobs_cap = 0;
        const size_t cap = std::max<size_t>(n_jobs, 256);
        MATCH_HIP(hipMalloc((void**)&s.d_jobs, cap * sizeof(MatchJobDev)));
        s.jobs_cap = cap;
    }
    if (n_entries > s.entries_cap) {
        if (s.d_best) (void)hipFree(s.d_best);
        if (s.d_matches) (void)hipFree(s.d_matches);
        if (s.h_matches) (void)hipHostFree(s.h_matches);
        s.d_best = nullptr; s.d_matches = nullptr; s.h_matches = nullptr; s.entries_cap = 0;
        MATCH_HIP(hipMalloc((void**)&s.d_best, n_entries * 2 * sizeof(unsigned long long)));
        MATCH_HIP(hipMalloc((void**)&s.d_matches, n_entries * sizeof(int32_t)));
        MATCH_HIP(hipHostMalloc((void**)&s.h_matches, n_entries * sizeof(int32_t), hipHostMallocDefault));
        s.entries_cap = n_entries;
    }
    return 0;
}

/* Where a job runs: its batch (-1: it has an empty side and runs nowhere) and its place in that batch's grid and buffers. */
struct MatchPlan {
    int32_t batch, block0, col_chunks;
    int64_t entry0;
};

long long job_chunks(int32_t n_b) { return ((long long)n_b + MATCH_CHUNK - 1) / MATCH_CHUNK; }
long long job_blocks(int32_t n_a, int32_t n_b) { return (((long long)n_a + MATCH_STRIP - 1) / MATCH_STRIP) * job_chunks(n_b); }

/* The batches of a job list: jobs in order, a new batch (one launch of each kernel, block0 and entry0 from 0 again) where
 * the next job would take the batch past lim_blocks workgroups or lim_entries rows + columns.  A single job above
 * lim_entries goes alone; one above lim_blocks fits no launch: MI_DMRECON_EINVAL.  Returns the number of batches. */
int plan_batches(int32_t n_jobs, const int32_t* n_a, const int32_t* n_b, long long lim_entries, long long lim_blocks, MatchPlan* out) {
    int32_t batch = -1;
    long long blocks = 0, entries = 0;
    for (int32_t j = 0; j < n_jobs; ++j) {
        MatchPlan& p = out[j];
        p.batch = -1; p.block0 = 0; p.col_chunks = 0; p.entry0 = 0;
        if (n_a[j] == 0 || n_b[j] == 0) continue;
        const long long nb = job_blocks(n_a[j], n_b[j]), ne = (long long)n_a[j] + n_b[j];
        if (nb > lim_blocks)
            return failf(MI_DMRECON_EINVAL, "match: job %lld needs %lld workgroups, a launch holds %lld", j, nb, lim_blocks);
        if (batch < 0 || blocks + nb > lim_blocks || entries + ne > lim_entries) { ++batch; blocks = 0; entries = 0; }
        p.batch = batch; p.block0 = (int32_t)blocks; p.col_chunks = (int32_t)job_chunks(n_b[j]); p.entry0 = entries;
        blocks += nb; entries += ne;
    }
    return batch + 1;
}

int pairs_impl(mi_dmrecon_match* m, int32_t kind, const mi_dmrecon_match_options* opt, int32_t n_jobs, const mi_dmrecon_match_job* jobs,
               int32_t* const* matches_ab, int32_t* const* matches_ba, int32_t* n_consistent) {
    if (!m) return failf(MI_DMRECON_EINVAL, "match: null handle");
    if (kind != MATCH_SIFT && kind != MATCH_SURF) return failf(MI_DMRECON_EINVAL, "match: unknown descriptor kind %lld", kind);
    if (!opt || opt->struct_size < (int32_t)sizeof(mi_dmrecon_match_options))
        return failf(MI_DMRECON_EINVAL, "match: options missing or their struct_size not set");
    if (n_jobs < 0) return failf(MI_DMRECON_EINVAL, "match: negative number of jobs");
    if (n_jobs == 0) return 0;
    if (!jobs) return failf(MI_DMRECON_EINVAL, "match: null jobs");

    std::vector<MatchSet> sets;
    {
        std::lock_guard<std::mutex> lock(m->mu);
        sets = m->sets[kind];
    }
    for (int32_t j = 0; j < n_jobs; ++j) {
        const mi_dmrecon_match_job& q = jobs[j];
        if (q.set_a < 0 || q.set_a >= m->n_sets || q.set_b < 0 || q.set_b >= m->n_sets)
            return failf(MI_DMRECON_EINVAL, "match: job %lld names a set outside [0, %lld)", j, m->n_sets);
        if (q.n_a < 0 || q.n_a > sets[q.set_a].n || q.n_b < 0 || q.n_b > sets[q.set_b].n)
            return failf(MI_DMRECON_EINVAL, "match: job %lld takes a prefix that is negative or longer than its set", j);
    }
    /* MATH_POW2 in float (matching.h:126-127) */
    const float square_lowe_thres = opt->lowe_ratio_threshold * opt->lowe_ratio_threshold;
    const float square_dist_thres = opt->distance_threshold * opt->distance_threshold;

    /* every batch is known, and a job no launch can hold refused, before anything is allocated or launched */
    std::vector<MatchPlan> plan(n_jobs);
    {
        std::vector<int32_t> na(n_jobs), nb(n_jobs);
        for (int32_t j = 0; j < n_jobs; ++j) { na[j] = jobs[j].n_a; nb[j] = jobs[j].n_b; }
        const int n_batches = plan_batches(n_jobs, na.data(), nb.data(), g_batch_entries.load(), g_batch_blocks.load(), plan.data());
        if (n_batches < 0) return n_batches;
    }

    /* a job with an empty side: all -1, nothing launched (matching.h:121-124) */
    for (int32_t j = 0; j < n_jobs; ++j) {
        const mi_dmrecon_match_job& q = jobs[j];
        if (q.n_a != 0 && q.n_b != 0) continue;
        if (matches_ab && matches_ab[j]) std::fill(matches_ab[j], matches_ab[j] + q.n_a, -1);
        if (matches_ba && matches_ba[j]) std::fill(matches_ba[j], matches_ba[j] + q.n_b, -1);
        if (n_consistent) n_consistent[j] = 0;
    }

    SlotLease lease(m);
    MatchSlot& s = *lease.slot;
    MATCH_HIP(hipSetDevice(m->device));
    std::vector<MatchJobDev> dev;
    std::vector<int32_t> which;
    int32_t j = 0;
    for (int32_t batch = 0;; ++batch) {
        dev.clear(); which.clear();
        long long blocks = 0, entries = 0;
        for (; j < n_jobs && plan[j].batch <= batch; ++j) {
            if (plan[j].batch < 0) continue;
            const mi_dmrecon_match_job& q = jobs[j];
            MatchJobDev d;
            d.a = sets[q.set_a].d_desc; d.off_a = sets[q.set_a].d_off;
            d.b = sets[q.set_b].d_desc; d.off_b = sets[q.set_b].d_off;
            d.n_a = q.n_a; d.n_b = q.n_b;
            d.block0 = plan[j].block0; d.col_chunks = plan[j].col_chunks; d.entry0 = plan[j].entry0;
            dev.push_back(d); which.push_back(j);
            blocks = plan[j].block0 + job_blocks(q.n_a, q.n_b); entries = plan[j].entry0 + q.n_a + q.n_b;
        }
        if (dev.empty()) break;
        if (int rc = grow(s, dev.size(), (size_t)entries)) return rc;
        MATCH_HIP(hipMemcpyAsync(s.d_jobs, dev.data(), dev.size() * sizeof(MatchJobDev), hipMemcpyHostToDevice, s.stream));
        MATCH_HIP(hipMemsetAsync(s.d_best, 0, (size_t)entries * 2 * sizeof(unsigned long long), s.stream));
        mi_match_launch(s.stream, kind, s.d_jobs, (int32_t)dev.size(), (int32_t)blocks, entries, s.d_best, s.d_matches,
                        square_lowe_thres, square_dist_thres);
        MATCH_HIP(hipGetLastError());
        MATCH_HIP(hipMemcpyAsync(s.h_matches, s.d_matches, (size_t)entries * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
        MATCH_HIP(hipStreamSynchronize(s.stream));       /* (before `dev` changes: the copy above may still read it) */
        for (size_t k = 0; k < dev.size(); ++k) {
            const int32_t jj = which[k];
            const int32_t* ab = s.h_matches + dev[k].entry0;
            const int32_t* ba = ab + dev[k].n_a;
            if (matches_ab && matches_ab[jj]) std::memcpy(matches_ab[jj], ab, (size_t)dev[k].n_a * sizeof(int32_t));
            if (matches_ba && matches_ba[jj]) std::memcpy(matches_ba[jj], ba, (size_t)dev[k].n_b * sizeof(int32_t));
            if (n_consistent) n_consistent[jj] = count_consistent(ab, dev[k].n_a, ba);
        }
    }
    return 0;
}

}  /* namespace */

extern "C" {

int mi_dmrecon_match_create(mi_dmrecon_ctx* ctx, int32_t n_sets, mi_dmrecon_match** out) {
    try { return create_impl(ctx, n_sets, out); }
    catch (const std::bad_alloc&) { return mi_host_fail(MI_DMRECON_EDEVICE, "out of host memory"); }
}

int mi_dmrecon_match_set(mi_dmrecon_match* m, int32_t set, int32_t kind, int32_t dtype, int32_t n, const void* descriptors) {
    try { return set_impl(m, set, kind, dtype, n, descriptors); }
    catch (const std::bad_alloc&) { return mi_host_fail(MI_DMRECON_EDEVICE, "out of host memory"); }
}

int mi_dmrecon_match_pairs(mi_dmrecon_match* m, int32_t kind, const mi_dmrecon_match_options* opt, int32_t n_jobs,
                           const mi_dmrecon_match_job* jobs, int32_t* const* matches_ab, int32_t* const* matches_ba,
                           int32_t* n_consistent) {
    try { return pairs_impl(m, kind, opt, n_jobs, jobs, matches_ab, matches_ba, n_consistent); }
    catch (const std::bad_alloc&) { return mi_host_fail(MI_DMRECON_EDEVICE, "out of host memory"); }
}

void mi_dmrecon_match_destroy(mi_dmrecon_match* m) { release(m); }

/* ---- mi_dmrecon_debug.h ------------------------------------------------------------------------------------------------ */

int mi_dmrecon_debug_match_get(mi_dmrecon_match* m, int32_t set, int32_t kind, int8_t* bytes_out, int32_t* off_out) {
    if (!m) return failf(MI_DMRECON_EINVAL, "match: null handle");
    if (kind != MATCH_SIFT && kind != MATCH_SURF) return failf(MI_DMRECON_EINVAL, "match: unknown descriptor kind %lld", kind);
    if (set < 0 || set >= m->n_sets) return failf(MI_DMRECON_EINVAL, "match: set %lld outside [0, %lld)", set, m->n_sets);
    std::lock_guard<std::mutex> lock(m->mu);
    const MatchSet& s = m->sets[kind][set];
    if (s.n == 0) return 0;
    MATCH_HIP(hipSetDevice(m->device));
    if (bytes_out) MATCH_HIP(hipMemcpy(bytes_out, s.d_desc, (size_t)s.n * dims_of(kind), hipMemcpyDeviceToHost));
    if (off_out) MATCH_HIP(hipMemcpy(off_out, s.d_off, (size_t)s.n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return s.n;
}

int mi_dmrecon_debug_match_limits(long long entries, long long blocks) {
    if (entries < 0 || blocks < 0 || blocks > MATCH_BATCH_BLOCKS)
        return failf(MI_DMRECON_EINVAL, "match: limits (%lld, %lld) negative, or more workgroups than a launch holds (%lld)", entries, blocks,
                     MATCH_BATCH_BLOCKS);
    g_batch_entries.store(entries ? entries : MATCH_BATCH_ENTRIES);
    g_batch_blocks.store(blocks ? blocks : MATCH_BATCH_BLOCKS);
    return 0;
}

int mi_dmrecon_debug_match_plan(int32_t n_jobs, const int32_t* n_a, const int32_t* n_b, long long entries, long long blocks,
                                int32_t* batch_out, int32_t* block0_out, int32_t* col_chunks_out, int64_t* entry0_out) {
    try {
        if (n_jobs < 0 || (n_jobs > 0 && (!n_a || !n_b))) return failf(MI_DMRECON_EINVAL, "match: a negative number of jobs or no sizes");
        if (entries < 0 || blocks < 0) return failf(MI_DMRECON_EINVAL, "match: negative limits");
        for (int32_t j = 0; j < n_jobs; ++j)
            if (n_a[j] < 0 || n_b[j] < 0) return failf(MI_DMRECON_EINVAL, "match: job %lld has a negative size", j);
        std::vector<MatchPlan> plan(n_jobs);
        const int n_batches = plan_batches(n_jobs, n_a, n_b, entries ? entries : g_batch_entries.load(), blocks ? blocks : g_batch_blocks.load(),
                                           plan.data());
        if (n_batches < 0) return n_batches;
        for (int32_t j = 0; j < n_jobs; ++j) {
            if (batch_out) batch_out[j] = plan[j].batch;
            if (block0_out) block0_out[j] = plan[j].block0;
            if (col_chunks_out) col_chunks_out[j] = plan[j].col_chunks;
            if (entry0_out) entry0_out[j] = plan[j].entry0;
        }
        return n_batches;
    }
    catch (const std::bad_alloc&) { return mi_host_fail(MI_DMRECON_EDEVICE, "out of host memory"); }
}

}  /* extern "C" */
