/*
 * surf_host.cpp -- mi_dmrecon_surf_run / mi_dmrecon_surf_get of include/mi_dmrecon.h: sfm::Surf::set_image + process
 * (libs/sfm/surf.cc) for one image through the kernels of surf_device.hip.  One upload, every launch on the context's stream,
 * one small download of the counts.  Everything is checked HERE before anything is allocated or launched.  The tables of the
 * two per-keypoint kernels (sample offsets, weights, window bounds, scales) are made here once, so that every value in them is
 * the host's.  The keypoint list on the device has a capacity; a run whose count exceeds it is repeated with larger buffers.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "host_common.h"
#include "surf_device.h"

namespace {

struct SurfState : HostModule {
    PinnedBuf h_pix, h_tab, h_counts;
    Buf d_pix, d_sat, d_maps, d_words, d_kp, d_ori, d_stage, d_slot, d_tmp, d_xyso, d_desc, d_tab, d_counts;
    bool tables_up = false;
    int32_t kp_cap = 1 << 15;
    int32_t n_kp = -1, n_desc = -1;          /* of the last run; -1: there was none, or it failed */
};

#define SURF_MAX_SIDE 32767
#define SURF_MAX_PIXELS (1ll << 28)

void make_tables(SurfTables* t) {
    std::memset(t, 0, sizeof(*t));
    /* the 109 samples of the circle of radius 6 in the reference's order; its weights are exp(-(rx^2 + ry^2) / (2 * 2.5^2))
     * written with six significant digits, which is what is restated here digit for digit */
    int n = 0;
    for (int ry = -5; ry <= 5; ++ry)
        for (int rx = -5; rx <= 5; ++rx) {
            if (rx * rx + ry * ry >= 36) continue;
            char digits[32];
            std::snprintf(digits, sizeof(digits), "%.6g", std::exp(-(double)(rx * rx + ry * ry) / 12.5));
            t->gaussian[n] = (float)std::strtod(digits, nullptr);
            t->rx[n] = rx; t->ry[n] = ry;
            ++n;
        }
    /* the sliding windows: the reference's own accumulation of deg in double */
    const double pi = 3.14159265358979323846, increment = pi / 8.0, halfsize = pi / 6.0;
    for (double deg = -pi; deg < pi && t->n_win < SURF_MAX_WINDOWS; deg += increment) {
        t->win_start[t->n_win] = deg - halfsize;
        t->win_end[t->n_win] = deg + halfsize;
        ++t->n_win;
    }
    const int fs[4][4] = {{3, 5, 7, 9}, {5, 9, 13, 17}, {9, 17, 25, 33}, {17, 33, 49, 65}};
    for (int o = 0; o < 4; ++o)
        for (int k = 0; k < 4; ++k) t->scale[o][k] = (float)(3 * fs[o][k]) * 1.2f / 9.0f;
    const float sigma2 = (2.0f * 3.3f) * (2.0f * 3.3f);
    for (int r2 = 0; r2 <= 200; ++r2) t->weight[r2] = std::exp(-(float)r2 / sigma2);
}

int surf_run_impl(mi_dmrecon_ctx* ctx, const mi_dmrecon_surf_options* opt, const uint8_t* pixels, int32_t w, int32_t h, int32_t channels,
                  int32_t* n_keypoints, int32_t* n_descriptors) {
    if (!ctx) return failf(MI_DMRECON_EINVAL, "surf: null context");
    if (!opt || !pixels || !n_keypoints || !n_descriptors) return failf(MI_DMRECON_EINVAL, "surf: null argument");
    if (channels != 1 && channels != 3) return failf(MI_DMRECON_EINVAL, "surf: channels = %lld: Gray or color image expected", channels);
    if (w < 1 || h < 1 || w > SURF_MAX_SIDE || h > SURF_MAX_SIDE || (long long)w * h > SURF_MAX_PIXELS)
        return failf(MI_DMRECON_EINVAL, "surf: w, h: a %lld x %lld image; 1 ... %lld a side and 2^28 pixels expected", w, h, SURF_MAX_SIDE);
    if (!std::isfinite(opt->contrast_threshold)) return failf(MI_DMRECON_EINVAL, "surf: contrast_threshold is not finite");

    MI_HIP(hipSetDevice(mi_host_ctx_device(ctx)));
    HostModule*& state = mi_host_ctx_module(ctx, MI_MODULE_SURF);
    if (!state) state = new SurfState();
    SurfState& s = *static_cast<SurfState*>(state);
    s.n_kp = s.n_desc = -1;
    hipStream_t stream = (hipStream_t)mi_dmrecon_ctx_stream(ctx);

    SurfArgs a;
    std::memset(&a, 0, sizeof(a));
    a.channels = channels; a.w = w; a.h = h;
    a.contrast_threshold = opt->contrast_threshold; a.upright = opt->use_upright_descriptor ? 1 : 0;
    long long n_maps = 0, n_words = 0;
    for (int o = 0, ow = w, oh = h; o < 4; ++o, ow = (ow + 1) >> 1, oh = (oh + 1) >> 1) {
        a.ow[o] = ow; a.oh[o] = oh;
        a.map_off[o] = n_maps; a.word_off[o] = (int32_t)n_words;
        n_maps += 4ll * ow * oh;
        n_words += 2ll * oh * ((ow + 63) / 64);
    }
    a.n_words = (int32_t)n_words;
    const size_t in_bytes = (size_t)w * h * channels;
    MI_HIP(s.h_pix.need(in_bytes));
    MI_HIP(s.d_pix.need(in_bytes));
    MI_HIP(s.d_sat.need((size_t)w * h * sizeof(uint32_t)));
    MI_HIP(s.d_maps.need((size_t)n_maps * sizeof(float)));
    MI_HIP(s.d_words.need((size_t)n_words * sizeof(int32_t)));
    MI_HIP(s.h_tab.need(sizeof(SurfTables)));
    MI_HIP(s.d_tab.need(sizeof(SurfTables)));
    MI_HIP(s.d_counts.need(sizeof(SurfCounts)));
    MI_HIP(s.h_counts.need(sizeof(SurfCounts)));
    std::memcpy(s.h_pix.p, pixels, in_bytes);
    MI_HIP(hipMemcpyAsync(s.d_pix.p, s.h_pix.p, in_bytes, hipMemcpyHostToDevice, stream));
    if (!s.tables_up) {
        make_tables((SurfTables*)s.h_tab.p);
        MI_HIP(hipMemcpyAsync(s.d_tab.p, s.h_tab.p, sizeof(SurfTables), hipMemcpyHostToDevice, stream));
        s.tables_up = true;
    }
    a.pixels = (const unsigned char*)s.d_pix.p; a.sat = (uint32_t*)s.d_sat.p; a.maps = (float*)s.d_maps.p; a.words = (int32_t*)s.d_words.p;
    a.tab = (const SurfTables*)s.d_tab.p; a.counts = (SurfCounts*)s.d_counts.p;
    mi_surf_sat(stream, a);
    mi_surf_responses(stream, a);

    for (int attempt = 0; attempt < 4; ++attempt) {
        const size_t cap = (size_t)s.kp_cap;
        MI_HIP(s.d_kp.need(cap * sizeof(SurfKeypoint)));
        MI_HIP(s.d_ori.need(cap * sizeof(float)));
        MI_HIP(s.d_stage.need(cap * sizeof(int32_t)));
        MI_HIP(s.d_slot.need(cap * sizeof(int32_t)));
        MI_HIP(s.d_tmp.need(cap * 64 * sizeof(float)));
        MI_HIP(s.d_xyso.need(cap * 4 * sizeof(float)));
        MI_HIP(s.d_desc.need(cap * 64 * sizeof(float)));
        a.kp = (SurfKeypoint*)s.d_kp.p; a.kp_cap = s.kp_cap; a.ori = (float*)s.d_ori.p; a.stage = (int32_t*)s.d_stage.p;
        a.slot = (int32_t*)s.d_slot.p; a.tmp_desc = (float*)s.d_tmp.p; a.xyso = (float*)s.d_xyso.p; a.desc = (float*)s.d_desc.p;
        mi_surf_detect(stream, a);
        mi_surf_describe(stream, a);
        MI_HIP(hipGetLastError());
        MI_HIP(hipMemcpyAsync(s.h_counts.p, s.d_counts.p, sizeof(SurfCounts), hipMemcpyDeviceToHost, stream));
        MI_HIP(hipStreamSynchronize(stream));
        const SurfCounts c = *(const SurfCounts*)s.h_counts.p;
        if (c.n_kp <= s.kp_cap) {
            s.n_kp = c.n_kp; s.n_desc = c.n_desc;
            *n_keypoints = s.n_kp; *n_descriptors = s.n_desc;
            return 0;
        }
        /* the list was cut off; the count is not: the next run has room for all of it */
        if (c.n_kp > (1 << 26)) return failf(MI_DMRECON_EINVAL, "surf: pixels: %lld keypoints: more than the lists hold", c.n_kp);
        s.kp_cap = c.n_kp;
    }
    return failf(MI_DMRECON_EDEVICE, "surf: the keypoint list still overflows after four runs");
}

int surf_get_impl(mi_dmrecon_ctx* ctx, mi_dmrecon_surf_keypoint* kp, float* xyso, float* desc) {
    if (!ctx) return failf(MI_DMRECON_EINVAL, "surf: null context");
    const SurfState* s = static_cast<SurfState*>(mi_host_ctx_module(ctx, MI_MODULE_SURF));
    if (!s || s->n_kp < 0) return failf(MI_DMRECON_EINVAL, "surf: mi_dmrecon_surf_get without a successful mi_dmrecon_surf_run on this context");
    MI_HIP(hipSetDevice(mi_host_ctx_device(ctx)));
    hipStream_t stream = (hipStream_t)mi_dmrecon_ctx_stream(ctx);
    static_assert(sizeof(mi_dmrecon_surf_keypoint) == sizeof(SurfKeypoint), "the kernels write the public keypoint");
    if (kp && s->n_kp) MI_HIP(hipMemcpyAsync(kp, s->d_kp.p, (size_t)s->n_kp * sizeof(SurfKeypoint), hipMemcpyDeviceToHost, stream));
    if (xyso && s->n_desc) MI_HIP(hipMemcpyAsync(xyso, s->d_xyso.p, (size_t)s->n_desc * 4 * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (desc && s->n_desc) MI_HIP(hipMemcpyAsync(desc, s->d_desc.p, (size_t)s->n_desc * 64 * sizeof(float), hipMemcpyDeviceToHost, stream));
    MI_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  /* namespace */

extern "C" {

int mi_dmrecon_surf_run(mi_dmrecon_ctx* ctx, const mi_dmrecon_surf_options* opt, const uint8_t* pixels, int32_t w, int32_t h,
                        int32_t channels, int32_t* n_keypoints, int32_t* n_descriptors) {
    return guarded([&] { return surf_run_impl(ctx, opt, pixels, w, h, channels, n_keypoints, n_descriptors); });
}

int mi_dmrecon_surf_get(mi_dmrecon_ctx* ctx, mi_dmrecon_surf_keypoint* kp, float* xyso, float* desc) {
    return surf_get_impl(ctx, kp, xyso, desc);
}

}  /* extern "C" */
