/*
 * sift_host.cpp -- mi_dmrecon_sift_run / mi_dmrecon_sift_get of include/mi_dmrecon.h: sfm::Sift::process (libs/sfm/sift.cc)
 * for one image through the kernels of sift_device.hip.  One upload, every launch on the context's stream, one small
 * download of the counts.  The whole run is planned and checked HERE before anything is allocated or launched: the octave
 * sizes, the taps of every blur and the images that the reference would hand to rescale_half_size_gaussian.
 * The result lists on the device have capacities; a run whose counts exceed one is repeated with larger buffers.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/mi_dmrecon_debug.h"
#include "host_common.h"
#include "sift_device.h"

namespace {

/* the capacities a context's lists start with; a run that overflows one grows it for good */
enum { SIFT_CAND_CAP = 1 << 18, SIFT_KP_CAP = 1 << 16, SIFT_DESC_CAP = 1 << 16 };

struct SiftState : HostModule {
    PinnedBuf h_pix, h_counts;
    Buf d_pix, d_orig, d_pp[2], d_tmp, d_img, d_dog, d_masks, d_words, d_cand, d_loc, d_block, d_kp, d_ori, d_nori, d_xyso, d_desc, d_counts;
    int32_t cand_cap = SIFT_CAND_CAP, kp_cap = SIFT_KP_CAP, desc_cap = SIFT_DESC_CAP;
    int32_t n_kp = -1, n_desc = -1;          /* of the last run; -1: there was none, or it failed */
    int32_t attempts = 0;                    /* how often the last run went through its kernels */
};

#define SIFT_MAX_SIDE 32767                  /* a candidate is x | y << 16 */
#define SIFT_MAX_PIXELS (1ll << 28)          /* of the largest octave image */

/* One octave of the plan: its size, where its source comes from and the S + 3 blurs (the first one brings the source to
 * base_blur_sigma, sift.cc:221-226; ks = 0 stands for a copy). */
struct OctavePlan {
    int32_t octave, w, h;
    std::vector<SiftTaps> blurs;
};

/* blur_gaussian's kernel (image_tools.h:1032-1043); false: the radius is beyond SIFT_MAX_KS */
bool make_taps(float sigma, bool copy, SiftTaps* t, long long* ks_out) {
    std::memset(t, 0, sizeof(*t));
    if (copy || (-0.1f <= sigma && sigma <= 0.1f)) return true;
    const float r = std::ceil(sigma * 2.884f);
    *ks_out = r > 1e9f ? 1000000000ll : (long long)r;
    if (!(r <= (float)SIFT_MAX_KS)) return false;
    const int ks = (int)r;
    t->ks = ks;
    t->ntaps = (2 * ks + 1 + 3) & ~3;
    float wsum = 0.0f;
    for (int i = -ks; i <= ks; ++i) {
        const float x = (float)std::abs(i);
        const float wgt = std::exp(-((x * x) / (2.0f * sigma * sigma)));
        t->taps[i + ks] = wgt;
        wsum += wgt;
    }
    t->wsum = wsum;
    return true;
}

int plan_run(const mi_dmrecon_sift_options& o, int32_t w, int32_t h, std::vector<OctavePlan>* plan) {
    const int S = o.num_samples_per_octave;
    long long ks = 0;
    auto add = [&](int32_t octave, int32_t ow, int32_t oh, float has_sigma) -> int {
        OctavePlan p;
        p.octave = octave; p.w = ow; p.h = oh;
        p.blurs.resize(S + 3);
        const float target = o.base_blur_sigma;
        float sigma = std::sqrt(target * target - has_sigma * has_sigma);
        if (!make_taps(sigma, !(target > has_sigma), &p.blurs[0], &ks))
            return failf(MI_DMRECON_EINVAL, "sift: base_blur_sigma / inherent_blur_sigma: the first blur of octave %lld has ks = %lld, the kernels take %lld",
                         octave, ks, SIFT_MAX_KS);
        const float k = std::pow(2.0f, 1.0f / (float)S);
        sigma = target;
        for (int i = 1; i < S + 3; ++i) {
            const float sigmak = sigma * k;
            const float blur = std::sqrt(sigmak * sigmak - sigma * sigma);
            if (!make_taps(blur, false, &p.blurs[i], &ks))
                return failf(MI_DMRECON_EINVAL, "sift: num_samples_per_octave / base_blur_sigma: blur %lld of an octave has ks = %lld, the kernels take %lld",
                             i, ks, SIFT_MAX_KS);
            sigma = sigmak;
        }
        plan->push_back(std::move(p));
        return 0;
    };
    if (o.min_octave < 0) {
        if (2ll * w > SIFT_MAX_SIDE || 2ll * h > SIFT_MAX_SIDE || 4ll * w * h > SIFT_MAX_PIXELS)
            return failf(MI_DMRECON_EINVAL, "sift: w, h: octave -1 of a %lld x %lld image is beyond %lld pixels a side or 2^28 in all", w, h, SIFT_MAX_SIDE);
        if (int rc = add(-1, 2 * w, 2 * h, o.inherent_blur_sigma * 2.0f)) return rc;
    }
    int32_t cw = w, ch = h;
    auto halve = [&](int before_octave) -> int {                 /* rescale_half_size_gaussian's "Invalid input image" */
        if (cw < 2 || ch < 2)
            return failf(MI_DMRECON_EINVAL, "sift: w, h: the image is too small: the half-size step before octave %lld would get %lld x %lld pixels (Invalid input image)",
                         before_octave, cw, ch);
        cw = (cw + 1) >> 1; ch = (ch + 1) >> 1;
        return 0;
    };
    for (int i = 0; i < o.min_octave; ++i)
        if (int rc = halve(i + 1)) return rc;
    float img_sigma = o.inherent_blur_sigma;
    for (int i = std::max(0, o.min_octave); i <= o.max_octave; ++i) {
        if (int rc = add(i, cw, ch, img_sigma)) return rc;
        if (int rc = halve(i + 1)) return rc;                    /* also behind the last octave (sift.cc:205) */
        img_sigma = o.base_blur_sigma;
    }
    return 0;
}

/* A call that passed its checks: the options as they are used, the plan, the context's state with every buffer that does
 * not depend on a list capacity, and the pixels in pinned memory. */
struct SiftRun {
    mi_dmrecon_sift_options o;
    std::vector<OctavePlan> plan;
    SiftState* s = nullptr;
    hipStream_t stream = nullptr;
    const float* cur = nullptr;              /* the image chain: the source of the octave that comes next, or what it is halved from */
    int32_t is_float = 0, w = 0, h = 0, channels = 0, cw = 0, ch = 0, flip = 0;
    size_t in_bytes = 0;
};

int sift_prepare(mi_dmrecon_ctx* ctx, const mi_dmrecon_sift_options* opt, const void* pixels, int32_t is_float, int32_t w, int32_t h,
                 int32_t channels, SiftRun* r) {
    if (!ctx) return failf(MI_DMRECON_EINVAL, "sift: null context");
    if (!opt || !pixels) return failf(MI_DMRECON_EINVAL, "sift: null argument");
    mi_dmrecon_sift_options& o = r->o;
    o = *opt;
    if (o.min_octave < -1 || o.min_octave > o.max_octave)
        return failf(MI_DMRECON_EINVAL, "sift: min_octave %lld, max_octave %lld: Invalid octave range", o.min_octave, o.max_octave);
    if (o.max_octave - o.min_octave + 1 > SIFT_MAX_OCTAVES)
        return failf(MI_DMRECON_EINVAL, "sift: min_octave %lld to max_octave %lld are more than %lld octaves", o.min_octave, o.max_octave, SIFT_MAX_OCTAVES);
    if (channels != 1 && channels != 3) return failf(MI_DMRECON_EINVAL, "sift: channels = %lld: Gray or color image expected", channels);
    if (o.num_samples_per_octave < 1 || o.num_samples_per_octave > 32)
        return failf(MI_DMRECON_EINVAL, "sift: num_samples_per_octave = %lld, 1 ... 32 expected", o.num_samples_per_octave);
    if (w < 1 || h < 1 || w > SIFT_MAX_SIDE || h > SIFT_MAX_SIDE || (long long)w * h > SIFT_MAX_PIXELS)
        return failf(MI_DMRECON_EINVAL, "sift: w, h: a %lld x %lld image; 1 ... %lld a side and 2^28 pixels expected", w, h, SIFT_MAX_SIDE);
    if (!(o.base_blur_sigma > 0.0f) || !(o.base_blur_sigma <= 1e3f) || !(o.inherent_blur_sigma >= 0.0f) || !(o.inherent_blur_sigma <= 1e3f))
        return failf(MI_DMRECON_EINVAL, "sift: base_blur_sigma must lie in (0, 1000], inherent_blur_sigma in [0, 1000]");
    if (!(o.edge_ratio_threshold == o.edge_ratio_threshold) || !(o.contrast_threshold == o.contrast_threshold))
        return failf(MI_DMRECON_EINVAL, "sift: contrast_threshold or edge_ratio_threshold is not a number");
    if (o.contrast_threshold < 0.0f) o.contrast_threshold = 0.02f / (float)o.num_samples_per_octave;
    std::vector<OctavePlan>& plan = r->plan;
    if (int rc = plan_run(o, w, h, &plan)) return rc;
    const size_t n_values = (size_t)w * h * channels;
    if (is_float) {
        const float* f = (const float*)pixels;
        long long bad = -1;
#pragma omp parallel for schedule(static) reduction(max : bad)
        for (long long i = 0; i < (long long)n_values; ++i)
            if (!std::isfinite(f[i])) bad = std::max(bad, i);
        if (bad >= 0) return failf(MI_DMRECON_EINVAL, "sift: pixels: value %lld is not finite", bad);
    }

    MI_HIP(hipSetDevice(mi_host_ctx_device(ctx)));
    HostModule*& state = mi_host_ctx_module(ctx, MI_MODULE_SIFT);
    if (!state) state = new SiftState();
    SiftState& s = *static_cast<SiftState*>(state);
    s.n_kp = s.n_desc = -1;
    s.attempts = 0;
    r->s = &s;
    r->stream = (hipStream_t)mi_dmrecon_ctx_stream(ctx);
    r->is_float = is_float; r->w = w; r->h = h; r->channels = channels;
    const int S = o.num_samples_per_octave;
    size_t max_px = 0, max_words = 0;
    for (const OctavePlan& p : plan) {
        max_px = std::max(max_px, (size_t)p.w * p.h);
        max_words = std::max(max_words, (size_t)S * p.h * ((p.w + 63) / 64));
    }
    const size_t in_bytes = r->in_bytes = n_values * (is_float ? sizeof(float) : 1);
    MI_HIP(s.h_pix.need(in_bytes));
    MI_HIP(s.d_pix.need(in_bytes));
    MI_HIP(s.d_orig.need((size_t)w * h * sizeof(float)));
    MI_HIP(s.d_pp[0].need(max_px * sizeof(float)));
    MI_HIP(s.d_pp[1].need(max_px * sizeof(float)));
    MI_HIP(s.d_tmp.need(max_px * sizeof(float)));
    MI_HIP(s.d_img.need(max_px * (S + 3) * sizeof(float)));
    MI_HIP(s.d_dog.need(max_px * (S + 2) * sizeof(float)));
    MI_HIP(s.d_masks.need(max_words * sizeof(unsigned long long)));
    MI_HIP(s.d_words.need(max_words * sizeof(int32_t)));
    MI_HIP(s.d_counts.need(sizeof(SiftCounts)));
    MI_HIP(s.h_counts.need(sizeof(SiftCounts)));
    std::memcpy(s.h_pix.p, pixels, in_bytes);
    return 0;
}

/* the buffers whose size is a list capacity, as the capacities stand */
int sift_lists(SiftState& s) {
    MI_HIP(s.d_cand.need((size_t)s.cand_cap * sizeof(int2)));
    MI_HIP(s.d_loc.need((size_t)s.cand_cap * sizeof(float4)));
    MI_HIP(s.d_block.need((size_t)((s.cand_cap + 255) / 256) * sizeof(int32_t)));
    MI_HIP(s.d_kp.need((size_t)s.kp_cap * sizeof(SiftKeypoint)));
    MI_HIP(s.d_ori.need((size_t)s.kp_cap * SIFT_MAX_ORI * sizeof(float)));
    MI_HIP(s.d_nori.need((size_t)s.kp_cap * sizeof(int32_t)));
    MI_HIP(s.d_xyso.need((size_t)s.desc_cap * 4 * sizeof(float)));
    MI_HIP(s.d_desc.need((size_t)s.desc_cap * 128 * sizeof(float)));
    return 0;
}

int sift_upload(SiftRun& r) {
    SiftState& s = *r.s;
    MI_HIP(hipMemcpyAsync(s.d_pix.p, s.h_pix.p, r.in_bytes, hipMemcpyHostToDevice, r.stream));
    mi_sift_gray(r.stream, s.d_pix.p, r.is_float, r.channels, (float*)s.d_orig.p, (long long)r.w * r.h);
    return 0;
}

void sift_chain_start(SiftRun& r) {
    r.cur = (const float*)r.s->d_orig.p;
    r.cw = r.w; r.ch = r.h; r.flip = 0;
}

/* The octave in plan slot k, behind the slots before it: its source image (r.cur afterwards), its S + 3 Gaussian and S + 2
 * DoG images in d_img and d_dog, and everything of mi_sift_detect_describe.  What mi_dmrecon_sift_run and
 * mi_dmrecon_debug_sift_octave both run. */
void sift_octave(SiftRun& r, size_t k) {
    SiftState& s = *r.s;
    const mi_dmrecon_sift_options& o = r.o;
    const OctavePlan& p = r.plan[k];
    const int S = o.num_samples_per_octave;
    hipStream_t stream = r.stream;
    if (p.octave < 0) {
        mi_sift_double(stream, (const float*)s.d_orig.p, (float*)s.d_pp[0].p, r.w, r.h);
        r.cur = (const float*)s.d_pp[0].p;
    } else {
        if (k > 0 && r.plan[k - 1].octave < 0) { r.cur = (const float*)s.d_orig.p; r.cw = r.w; r.ch = r.h; }
        while (r.cw != p.w || r.ch != p.h) {                      /* the octave's SOURCE image halved (sift.cc:193, :205), never a blurred one */
            mi_sift_half(stream, r.cur, (float*)s.d_pp[r.flip].p, r.cw, r.ch);
            r.cur = (const float*)s.d_pp[r.flip].p; r.flip ^= 1;
            r.cw = (r.cw + 1) >> 1; r.ch = (r.ch + 1) >> 1;
        }
    }
    const size_t px = (size_t)p.w * p.h;
    float* img = (float*)s.d_img.p;
    float* dog = (float*)s.d_dog.p;
    mi_sift_blur(stream, r.cur, (float*)s.d_tmp.p, img, nullptr, p.w, p.h, p.blurs[0]);
    for (int i = 1; i < S + 3; ++i)
        mi_sift_blur(stream, img + (size_t)(i - 1) * px, (float*)s.d_tmp.p, img + (size_t)i * px, dog + (size_t)(i - 1) * px, p.w, p.h, p.blurs[i]);
    SiftOctaveArgs a;
    a.img = img; a.dog = dog; a.w = p.w; a.h = p.h; a.S = S; a.octave = p.octave; a.slot = (int32_t)k;
    a.contrast_threshold = o.contrast_threshold; a.edge_ratio_threshold = o.edge_ratio_threshold; a.base_blur_sigma = o.base_blur_sigma;
    a.masks = (unsigned long long*)s.d_masks.p; a.words = (int32_t*)s.d_words.p;
    a.cand = (int2*)s.d_cand.p; a.cand_cap = s.cand_cap; a.loc = (float4*)s.d_loc.p; a.block_off = (int32_t*)s.d_block.p;
    a.kp = (SiftKeypoint*)s.d_kp.p; a.kp_cap = s.kp_cap; a.ori = (float*)s.d_ori.p; a.n_ori = (int32_t*)s.d_nori.p;
    a.xyso = (float*)s.d_xyso.p; a.desc = (float*)s.d_desc.p; a.desc_cap = s.desc_cap; a.counts = (SiftCounts*)s.d_counts.p;
    mi_sift_detect_describe(stream, a);
}

int sift_run_impl(mi_dmrecon_ctx* ctx, const mi_dmrecon_sift_options* opt, const void* pixels, int32_t is_float, int32_t w, int32_t h,
                  int32_t channels, int32_t* n_keypoints, int32_t* n_descriptors) {
    if (ctx && (!n_keypoints || !n_descriptors)) return failf(MI_DMRECON_EINVAL, "sift: null argument");
    SiftRun r;
    if (int rc = sift_prepare(ctx, opt, pixels, is_float, w, h, channels, &r)) return rc;
    SiftState& s = *r.s;
    hipStream_t stream = r.stream;
    const std::vector<OctavePlan>& plan = r.plan;

    for (int attempt = 0; attempt < 8; ++attempt) {
        s.attempts = attempt + 1;
        if (int rc = sift_lists(s)) return rc;
        if (attempt == 0)
            if (int rc = sift_upload(r)) return rc;
        sift_chain_start(r);
        for (size_t k = 0; k < plan.size(); ++k) sift_octave(r, k);
        MI_HIP(hipGetLastError());
        MI_HIP(hipMemcpyAsync(s.h_counts.p, s.d_counts.p, sizeof(SiftCounts), hipMemcpyDeviceToHost, stream));
        MI_HIP(hipStreamSynchronize(stream));
        const SiftCounts& c = *(const SiftCounts*)s.h_counts.p;
        long long max_cand = 0, n_kp = 0, n_desc = 0;
        for (size_t k = 0; k < plan.size(); ++k) {
            max_cand = std::max<long long>(max_cand, c.n_cand[k]);
            n_kp += c.n_kp[k]; n_desc += c.n_desc[k];
        }
        if (max_cand <= s.cand_cap && n_kp <= s.kp_cap && n_desc <= s.desc_cap) {
            s.n_kp = (int32_t)n_kp; s.n_desc = (int32_t)n_desc;
            *n_keypoints = s.n_kp; *n_descriptors = s.n_desc;
            return 0;
        }
        /* a list was cut off: what lies behind it was counted short, so grow generously and run again */
        if (max_cand > (1ll << 28) || n_kp > (1ll << 26) || n_desc > (1ll << 24))
            return failf(MI_DMRECON_EINVAL, "sift: pixels: %lld extrema in an octave, %lld keypoints, %lld descriptors: more than the lists hold", max_cand, n_kp, n_desc);
        if (max_cand > s.cand_cap) s.cand_cap = (int32_t)(max_cand + max_cand / 4);
        if (n_kp > s.kp_cap) s.kp_cap = (int32_t)(n_kp * 2);
        if (n_desc > s.desc_cap) s.desc_cap = (int32_t)(n_desc * 2);
    }
    return failf(MI_DMRECON_EDEVICE, "sift: the result lists still overflow after eight runs");
}

/* mi_dmrecon_debug_sift_octave (include/mi_dmrecon_debug.h) */
int sift_debug_octave_impl(mi_dmrecon_ctx* ctx, const mi_dmrecon_sift_options* opt, const void* pixels, int32_t is_float, int32_t w, int32_t h,
                           int32_t channels, int32_t slot, int32_t* w_out, int32_t* h_out, float* gray_out, float* src_out, float* img_out,
                           float* dog_out, int32_t* ks_out, float* wsum_out, float* taps_out, int32_t cand_room, int32_t* n_cand_out,
                           int32_t* cand_out, float* loc_out, int32_t raw_room, int32_t* raw_cand_out, void* raw_kp_out,
                           float* raw_xyso_out) {
    SiftRun r;
    if (int rc = sift_prepare(ctx, opt, pixels, is_float, w, h, channels, &r)) return rc;
    if (slot < 0 || (size_t)slot >= r.plan.size())
        return failf(MI_DMRECON_EINVAL, "sift: slot %lld: the plan has %lld octaves", slot, (long long)r.plan.size());
    if (cand_room < 0 || raw_room < 0) return failf(MI_DMRECON_EINVAL, "sift: cand_room or raw_room is negative");
    SiftState& s = *r.s;
    hipStream_t stream = r.stream;
    const OctavePlan& p = r.plan[slot];
    const int S = r.o.num_samples_per_octave;
    if (int rc = sift_lists(s)) return rc;
    const size_t raw = (size_t)raw_room;
    if ((raw_cand_out && raw * sizeof(int2) > s.d_cand.cap) || (raw_kp_out && raw * sizeof(SiftKeypoint) > s.d_kp.cap)
        || (raw_xyso_out && raw * 4 * sizeof(float) > s.d_xyso.cap))
        return failf(MI_DMRECON_EINVAL, "sift: raw_room = %lld: the context's lists were never that long", raw_room);
    if (int rc = sift_upload(r)) return rc;
    sift_chain_start(r);
    for (int32_t k = 0; k <= slot; ++k) sift_octave(r, (size_t)k);
    MI_HIP(hipGetLastError());
    MI_HIP(hipMemcpyAsync(s.h_counts.p, s.d_counts.p, sizeof(SiftCounts), hipMemcpyDeviceToHost, stream));
    MI_HIP(hipStreamSynchronize(stream));
    const int32_t n_cand = ((const SiftCounts*)s.h_counts.p)->n_cand[slot];
    const size_t px = (size_t)p.w * p.h;
    const size_t n_list = (size_t)std::max(0, std::min(std::min(n_cand, s.cand_cap), cand_room));
    if (w_out) *w_out = p.w;
    if (h_out) *h_out = p.h;
    if (n_cand_out) *n_cand_out = n_cand;
    for (int i = 0; i < S + 3; ++i) {
        if (ks_out) ks_out[i] = p.blurs[i].ks;
        if (wsum_out) wsum_out[i] = p.blurs[i].wsum;
        if (taps_out) std::memcpy(taps_out + (size_t)i * SIFT_MAX_TAPS, p.blurs[i].taps, sizeof(p.blurs[i].taps));
    }
    if (gray_out) MI_HIP(hipMemcpyAsync(gray_out, s.d_orig.p, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (src_out) MI_HIP(hipMemcpyAsync(src_out, r.cur, px * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (img_out) MI_HIP(hipMemcpyAsync(img_out, s.d_img.p, px * (S + 3) * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (dog_out) MI_HIP(hipMemcpyAsync(dog_out, s.d_dog.p, px * (S + 2) * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (cand_out && n_list) MI_HIP(hipMemcpyAsync(cand_out, s.d_cand.p, n_list * sizeof(int2), hipMemcpyDeviceToHost, stream));
    if (loc_out && n_list) MI_HIP(hipMemcpyAsync(loc_out, s.d_loc.p, n_list * sizeof(float4), hipMemcpyDeviceToHost, stream));
    if (raw_cand_out && raw) MI_HIP(hipMemcpyAsync(raw_cand_out, s.d_cand.p, raw * sizeof(int2), hipMemcpyDeviceToHost, stream));
    if (raw_kp_out && raw) MI_HIP(hipMemcpyAsync(raw_kp_out, s.d_kp.p, raw * sizeof(SiftKeypoint), hipMemcpyDeviceToHost, stream));
    if (raw_xyso_out && raw) MI_HIP(hipMemcpyAsync(raw_xyso_out, s.d_xyso.p, raw * 4 * sizeof(float), hipMemcpyDeviceToHost, stream));
    MI_HIP(hipStreamSynchronize(stream));
    return 0;
}

/* mi_dmrecon_debug_sift_caps (include/mi_dmrecon_debug.h) */
int sift_debug_caps_impl(mi_dmrecon_ctx* ctx, int32_t cand, int32_t kp, int32_t desc) {
    if (!ctx) return failf(MI_DMRECON_EINVAL, "sift: null context");
    if (cand < 0 || kp < 0 || desc < 0) return failf(MI_DMRECON_EINVAL, "sift: a negative list capacity (%lld, %lld, %lld)", cand, kp, desc);
    HostModule*& state = mi_host_ctx_module(ctx, MI_MODULE_SIFT);
    if (!state) state = new SiftState();
    SiftState& s = *static_cast<SiftState*>(state);
    s.cand_cap = cand ? cand : SIFT_CAND_CAP;
    s.kp_cap = kp ? kp : SIFT_KP_CAP;
    s.desc_cap = desc ? desc : SIFT_DESC_CAP;
    return s.attempts;
}

int sift_get_impl(mi_dmrecon_ctx* ctx, mi_dmrecon_sift_keypoint* kp, float* xyso, float* desc) {
    if (!ctx) return failf(MI_DMRECON_EINVAL, "sift: null context");
    const SiftState* s = static_cast<SiftState*>(mi_host_ctx_module(ctx, MI_MODULE_SIFT));
    if (!s || s->n_kp < 0) return failf(MI_DMRECON_EINVAL, "sift: mi_dmrecon_sift_get without a successful mi_dmrecon_sift_run on this context");
    MI_HIP(hipSetDevice(mi_host_ctx_device(ctx)));
    hipStream_t stream = (hipStream_t)mi_dmrecon_ctx_stream(ctx);
    static_assert(sizeof(mi_dmrecon_sift_keypoint) == sizeof(SiftKeypoint), "the kernels write the public keypoint");
    if (kp && s->n_kp) MI_HIP(hipMemcpyAsync(kp, s->d_kp.p, (size_t)s->n_kp * sizeof(SiftKeypoint), hipMemcpyDeviceToHost, stream));
    if (xyso && s->n_desc) MI_HIP(hipMemcpyAsync(xyso, s->d_xyso.p, (size_t)s->n_desc * 4 * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (desc && s->n_desc) MI_HIP(hipMemcpyAsync(desc, s->d_desc.p, (size_t)s->n_desc * 128 * sizeof(float), hipMemcpyDeviceToHost, stream));
    MI_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  /* namespace */

extern "C" {

int mi_dmrecon_sift_run(mi_dmrecon_ctx* ctx, const mi_dmrecon_sift_options* opt, const void* pixels, int32_t is_float, int32_t w, int32_t h,
                        int32_t channels, int32_t* n_keypoints, int32_t* n_descriptors) {
    return guarded([&] { return sift_run_impl(ctx, opt, pixels, is_float, w, h, channels, n_keypoints, n_descriptors); });
}

int mi_dmrecon_sift_get(mi_dmrecon_ctx* ctx, mi_dmrecon_sift_keypoint* kp, float* xyso, float* desc) {
    return sift_get_impl(ctx, kp, xyso, desc);
}

int mi_dmrecon_debug_sift_octave(mi_dmrecon_ctx* ctx, const mi_dmrecon_sift_options* opt, const void* pixels, int32_t is_float, int32_t w,
                                 int32_t h, int32_t channels, int32_t slot, int32_t* w_out, int32_t* h_out, float* gray_out, float* src_out,
                                 float* img_out, float* dog_out, int32_t* ks_out, float* wsum_out, float* taps_out, int32_t cand_room,
                                 int32_t* n_cand_out, int32_t* cand_out, float* loc_out, int32_t raw_room, int32_t* raw_cand_out,
                                 void* raw_kp_out, float* raw_xyso_out) {
    return guarded([&] {
        return sift_debug_octave_impl(ctx, opt, pixels, is_float, w, h, channels, slot, w_out, h_out, gray_out, src_out, img_out, dog_out, ks_out,
                                      wsum_out, taps_out, cand_room, n_cand_out, cand_out, loc_out, raw_room, raw_cand_out,
                                      raw_kp_out, raw_xyso_out);
    });
}

int mi_dmrecon_debug_sift_caps(mi_dmrecon_ctx* ctx, int32_t cand, int32_t kp, int32_t desc) {
    return guarded([&] { return sift_debug_caps_impl(ctx, cand, kp, desc); });
}

}  /* extern "C" */
