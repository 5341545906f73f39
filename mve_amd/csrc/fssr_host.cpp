/*
 * fssr_host.cpp -- the mi_dmrecon_fssr_* entry points of include/mi_dmrecon.h: upload of the flattened octree of
 * fssr::IsoOctree and its samples, and the chunked launches of fssr_device.hip.  The tree is checked HERE, before anything
 * is uploaded or launched: the kernel trusts every index it reads.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/mi_dmrecon.h"
#include "fssr_device.h"

/* dmrecon_host.cpp: the thread-local error message and the context's device (not exported, exports.map) */
int mi_host_fail(int code, const char* msg);
int mi_host_ctx_device(const mi_dmrecon_ctx* c);

static_assert(sizeof(mi_dmrecon_fssr_sample_t) == sizeof(FssrSample) && sizeof(FssrSample) == 44, "sample layout");
static_assert(sizeof(mi_dmrecon_fssr_node) == sizeof(FssrNode) && sizeof(FssrNode) == 16, "node layout");

struct mi_dmrecon_fssr {
    mi_dmrecon_ctx* ctx = nullptr;
    int device = -1;
    hipStream_t stream = nullptr;
    FssrTree tree{};
    FssrSample* d_samples = nullptr;
    FssrNode* d_nodes = nullptr;
    FssrLists lists{};             /* the part of the wavefronts' lists that does not fit their LDS */
    /* per-chunk buffers, grown on demand */
    int64_t chunk_cap = 0;
    double* d_pos = nullptr;
    float* d_f = nullptr;          /* value, conf, scale, max_scale: 4 x cap; color, deriv: 2 x 3 x cap */
    int32_t* d_n = nullptr;
};

namespace {

#define FSSR_CHUNK (1 << 18)       /* voxels per launch */
#define FSSR_MAX_COUNT (1 << 30)   /* samples / nodes: indices stay far inside int32 */

int failf(int code, const char* fmt, long long a = 0, long long b = 0) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), fmt, a, b);
    return mi_host_fail(code, buf);
}

#define FSSR_HIP(expr)                                                                        \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            char _b[256];                                                                     \
            std::snprintf(_b, sizeof(_b), "%s failed: %s", #expr, hipGetErrorString(_e));     \
            return mi_host_fail(MI_DMRECON_EDEVICE, _b);                                      \
        }                                                                                     \
    } while (0)

/* Everything the kernel relies on: children after parents (so the walk terminates), eight consecutive children inside the
 * array, sample ranges inside the samples, at most FSSR_MAX_LEVELS levels. */
int validate(int64_t n_samples, const mi_dmrecon_fssr_sample_t* samples, int64_t n_nodes, const mi_dmrecon_fssr_node* nodes,
             const double* root_center, double root_size) {
    if (n_samples < 0 || n_nodes < 0) return failf(MI_DMRECON_EINVAL, "fssr: negative count");
    if (n_samples > FSSR_MAX_COUNT || n_nodes > FSSR_MAX_COUNT) return failf(MI_DMRECON_EINVAL, "fssr: more than 2^30 samples or nodes");
    if (n_samples > 0 && !samples) return failf(MI_DMRECON_EINVAL, "fssr: null samples");
    for (int64_t i = 0; i < n_samples; ++i)
        /* the scale cut orders scales by their bit patterns (fssr::SampleIO drops samples with scale <= 0, sample_io.cc) */
        if (!(samples[i].scale > 0.0f) || !std::isfinite(samples[i].scale))
            return failf(MI_DMRECON_EINVAL, "fssr: sample %lld has a scale that is not positive and finite", i);
    if (n_nodes == 0) return 0;
    if (!nodes || !root_center) return failf(MI_DMRECON_EINVAL, "fssr: null nodes or root centre");
    if (!(root_size > 0.0) || !std::isfinite(root_size)) return failf(MI_DMRECON_EINVAL, "fssr: root_size must be positive and finite");
    for (int j = 0; j < 3; ++j)
        if (!std::isfinite(root_center[j])) return failf(MI_DMRECON_EINVAL, "fssr: root centre is not finite");
    std::vector<int8_t> level(n_nodes, 0);                   /* 0 = not reached from the root; else level + 1 */
    level[0] = 1;
    for (int64_t i = 0; i < n_nodes; ++i) {
        const mi_dmrecon_fssr_node& nd = nodes[i];
        if (nd.n_samples < 0 || nd.first_sample < 0 || (int64_t)nd.first_sample + nd.n_samples > n_samples)
            return failf(MI_DMRECON_EINVAL, "fssr: node %lld: sample range outside [0, %lld]", i, n_samples);
        if (nd.first_child == -1) continue;
        if (nd.first_child <= i || (int64_t)nd.first_child > n_nodes - 8)
            return failf(MI_DMRECON_EINVAL, "fssr: node %lld: first_child %lld is neither -1 nor in (own index, n_nodes - 8]", i, nd.first_child);
        if (level[i] == 0) continue;                         /* unreachable: never visited by the walk */
        if (level[i] + 1 > FSSR_MAX_LEVELS) return failf(MI_DMRECON_EINVAL, "fssr: node %lld: the tree is deeper than 21 levels", i);
        for (int k = 0; k < 8; ++k) {
            if (level[nd.first_child + k] != 0) return failf(MI_DMRECON_EINVAL, "fssr: node %lld has two parents", (long long)nd.first_child + k);
            level[nd.first_child + k] = (int8_t)(level[i] + 1);
        }
    }
    return 0;
}

void release(mi_dmrecon_fssr* f) {
    if (!f) return;
    if (f->device >= 0) (void)hipSetDevice(f->device);
    if (f->d_samples) (void)hipFree(f->d_samples);
    if (f->d_nodes) (void)hipFree(f->d_nodes);
    if (f->lists.entries) (void)hipFree(f->lists.entries);
    if (f->d_pos) (void)hipFree(f->d_pos);
    if (f->d_f) (void)hipFree(f->d_f);
    if (f->d_n) (void)hipFree(f->d_n);
    delete f;
}

int create_impl(mi_dmrecon_ctx* ctx, int64_t n_samples, const mi_dmrecon_fssr_sample_t* samples, int64_t n_nodes,
                const mi_dmrecon_fssr_node* nodes, const double* root_center, double root_size, mi_dmrecon_fssr** out) {
    if (!ctx || !out) return failf(MI_DMRECON_EINVAL, "fssr: null argument");
    *out = nullptr;
    if (int rc = validate(n_samples, samples, n_nodes, nodes, root_center, root_size)) return rc;
    const int device = mi_host_ctx_device(ctx);
    if (device < 0) return failf(MI_DMRECON_EINVAL, "fssr: the context has no device");
    FSSR_HIP(hipSetDevice(device));
    mi_dmrecon_fssr* f = new mi_dmrecon_fssr();
    f->ctx = ctx; f->device = device; f->stream = (hipStream_t)mi_dmrecon_ctx_stream(ctx);
    f->tree.n_samples = (int32_t)n_samples; f->tree.n_nodes = (int32_t)n_nodes;
    for (int j = 0; j < 3; ++j) f->tree.root_center[j] = n_nodes ? root_center[j] : 0.0;
    f->tree.root_size = n_nodes ? root_size : 1.0;
    hipError_t e = hipSuccess;
    if (n_samples) {
        e = hipMalloc((void**)&f->d_samples, (size_t)n_samples * sizeof(FssrSample));
        if (e == hipSuccess) e = hipMemcpy(f->d_samples, samples, (size_t)n_samples * sizeof(FssrSample), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && n_nodes) {
        e = hipMalloc((void**)&f->d_nodes, (size_t)n_nodes * sizeof(FssrNode));
        if (e == hipSuccess) e = hipMemcpy(f->d_nodes, nodes, (size_t)n_nodes * sizeof(FssrNode), hipMemcpyHostToDevice);
    }
    /* no list is longer than the number of samples */
    f->lists.max_blocks = mi_fssr_resident_blocks(device);
    f->lists.per_wave = (int32_t)std::min<int64_t>(FSSR_GLIST_MAX, std::max<int64_t>(0, n_samples - FSSR_LIST_MAX));
    if (e == hipSuccess && f->lists.per_wave > 0)
        e = hipMalloc((void**)&f->lists.entries, (size_t)f->lists.max_blocks * 4 * (size_t)f->lists.per_wave * sizeof(uint2));
    if (e != hipSuccess) {
        release(f);
        char b[160];
        std::snprintf(b, sizeof(b), "fssr: upload failed: %s", hipGetErrorString(e));
        return mi_host_fail(MI_DMRECON_EDEVICE, b);
    }
    f->tree.samples = f->d_samples; f->tree.nodes = f->d_nodes;
    *out = f;
    return 0;
}

int sample_impl(mi_dmrecon_fssr* f, const mi_dmrecon_fssr_options* opt, int64_t n_voxels, const double* positions, float* value,
                float* conf, float* scale, float* color, float* deriv, int32_t* n_influencing, float* max_scale) {
    if (!f) return failf(MI_DMRECON_EINVAL, "fssr: null handle");
    if (n_voxels < 0) return failf(MI_DMRECON_EINVAL, "fssr: negative voxel count");
    if (n_voxels == 0) return 0;
    if (!positions) return failf(MI_DMRECON_EINVAL, "fssr: null positions");
    int32_t cap = opt ? opt->list_capacity : 0;
    if (cap < 0) return failf(MI_DMRECON_EINVAL, "fssr: negative list_capacity");
    if (cap == 0) cap = FSSR_LIST_MAX + FSSR_GLIST_MAX;        /* (the launcher clamps it to what the lists hold) */
    FSSR_HIP(hipSetDevice(f->device));
    const int64_t chunk = n_voxels < FSSR_CHUNK ? n_voxels : FSSR_CHUNK;
    if (chunk > f->chunk_cap) {
        if (f->d_pos) (void)hipFree(f->d_pos);
        if (f->d_f) (void)hipFree(f->d_f);
        if (f->d_n) (void)hipFree(f->d_n);
        f->d_pos = nullptr; f->d_f = nullptr; f->d_n = nullptr; f->chunk_cap = 0;
        FSSR_HIP(hipMalloc((void**)&f->d_pos, (size_t)chunk * 3 * sizeof(double)));
        FSSR_HIP(hipMalloc((void**)&f->d_f, (size_t)chunk * 10 * sizeof(float)));
        FSSR_HIP(hipMalloc((void**)&f->d_n, (size_t)chunk * sizeof(int32_t)));
        f->chunk_cap = chunk;
    }
    const size_t C = (size_t)f->chunk_cap;
    FssrOut o;
    o.value = f->d_f; o.conf = f->d_f + C; o.scale = f->d_f + 2 * C; o.max_scale = f->d_f + 3 * C;
    o.color = f->d_f + 4 * C; o.deriv = f->d_f + 7 * C; o.n_influencing = f->d_n;
    for (int64_t v0 = 0; v0 < n_voxels; v0 += chunk) {
        const size_t m = (size_t)(n_voxels - v0 < chunk ? n_voxels - v0 : chunk);
        FSSR_HIP(hipMemcpyAsync(f->d_pos, positions + 3 * v0, m * 3 * sizeof(double), hipMemcpyHostToDevice, f->stream));
        mi_fssr_launch(f->stream, f->tree, cap, f->lists, (int32_t)m, f->d_pos, o);
        FSSR_HIP(hipGetLastError());
        if (value) FSSR_HIP(hipMemcpyAsync(value + v0, o.value, m * sizeof(float), hipMemcpyDeviceToHost, f->stream));
        if (conf) FSSR_HIP(hipMemcpyAsync(conf + v0, o.conf, m * sizeof(float), hipMemcpyDeviceToHost, f->stream));
        if (scale) FSSR_HIP(hipMemcpyAsync(scale + v0, o.scale, m * sizeof(float), hipMemcpyDeviceToHost, f->stream));
        if (max_scale) FSSR_HIP(hipMemcpyAsync(max_scale + v0, o.max_scale, m * sizeof(float), hipMemcpyDeviceToHost, f->stream));
        if (color) FSSR_HIP(hipMemcpyAsync(color + 3 * v0, o.color, m * 3 * sizeof(float), hipMemcpyDeviceToHost, f->stream));
        if (deriv) FSSR_HIP(hipMemcpyAsync(deriv + 3 * v0, o.deriv, m * 3 * sizeof(float), hipMemcpyDeviceToHost, f->stream));
        if (n_influencing) FSSR_HIP(hipMemcpyAsync(n_influencing + v0, o.n_influencing, m * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
        FSSR_HIP(hipStreamSynchronize(f->stream));
    }
    return 0;
}

}  /* namespace */

extern "C" {

void mi_dmrecon_fssr_options_default(mi_dmrecon_fssr_options* o) {
    if (o) o->list_capacity = 0;
}

int mi_dmrecon_fssr_create(mi_dmrecon_ctx* ctx, int64_t n_samples, const mi_dmrecon_fssr_sample_t* samples, int64_t n_nodes,
                           const mi_dmrecon_fssr_node* nodes, const double root_center[3], double root_size, mi_dmrecon_fssr** out) {
    try { return create_impl(ctx, n_samples, samples, n_nodes, nodes, root_center, root_size, out); }
    catch (const std::bad_alloc&) { return mi_host_fail(MI_DMRECON_EDEVICE, "out of host memory"); }
}

int mi_dmrecon_fssr_sample(mi_dmrecon_fssr* f, const mi_dmrecon_fssr_options* opt, int64_t n_voxels, const double* positions,
                           float* value, float* conf, float* scale, float* color, float* deriv, int32_t* n_influencing,
                           float* max_scale) {
    return sample_impl(f, opt, n_voxels, positions, value, conf, scale, color, deriv, n_influencing, max_scale);
}

void mi_dmrecon_fssr_destroy(mi_dmrecon_fssr* f) { release(f); }

}  /* extern "C" */
