/* Internal: layouts + launchers of sift_device.hip (sfm::Sift, libs/sfm/sift.cc, on the GPU). */
#ifndef MI_SIFT_DEVICE_H
#define MI_SIFT_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SIFT_MAX_KS 32            /* largest blur radius ceil(sigma * 2.884): num_samples_per_octave 1 ... 6 at the default sigmas
                                     need 32 (S = 1: the last blur of an octave has sigma 11.09), 14 (S = 2), 9 (S = 3) or less */
#define SIFT_MAX_TAPS 68          /* 2 * SIFT_MAX_KS + 1 taps, padded with zero weights to a multiple of four */
#define SIFT_MAX_OCTAVES 20
#define SIFT_MAX_ORI 18           /* strict local maxima of a circular histogram of 36 bins */
#define SIFT_BLUR_TW 256          /* k_sift_blur_rows: a workgroup makes 256 x 4 pixels, four neighbours per lane */
#define SIFT_BLUR_TH 32           /* k_sift_blur_cols: a workgroup makes 64 x 32 pixels, two groups of four rows per lane */
#define SIFT_EXT_TH 16            /* k_sift_extrema: a workgroup tests 64 x 16 centres */

/* the taps of one blur, i = -ks ... ks in taps[0 ... 2 ks], zeros behind them; wsum is their sum in that order */
struct SiftTaps {
    int32_t ks, ntaps;            /* ntaps: 2 ks + 1 rounded up to a multiple of four */
    float wsum;
    float taps[SIFT_MAX_TAPS];
};

/* the counters of a run, all on the device: what each octave found (uncapped), summed by the kernels that need a base */
struct SiftCounts {
    int32_t n_cand[SIFT_MAX_OCTAVES];
    int32_t n_kp[SIFT_MAX_OCTAVES];
    int32_t n_desc[SIFT_MAX_OCTAVES];
};

struct SiftKeypoint { int32_t octave; float sample, x, y; };        /* = mi_dmrecon_sift_keypoint = sfm::Sift::Keypoint */

/* One octave's detection and description: everything behind its Gaussian and DoG images. */
struct SiftOctaveArgs {
    const float* img;             /* S + 3 Gaussian images of w x h, one behind the other */
    const float* dog;             /* S + 2 DoG images likewise */
    int32_t w, h, S;
    int32_t octave;               /* the reference's octave number (-1 ...) */
    int32_t slot;                 /* index into SiftCounts */
    float contrast_threshold, edge_ratio_threshold, base_blur_sigma;
    unsigned long long* masks;    /* S x h x ceil(w / 64): which centres of a row piece are extrema */
    int32_t* words;               /* as many counts, then offsets */
    int2* cand;                   /* cand_cap: x | y << 16, sample */
    int32_t cand_cap;
    float4* loc;                  /* cand_cap: x, y, sample, kept */
    int32_t* block_off;           /* ceil(cand_cap / 256) */
    SiftKeypoint* kp;             /* kp_cap, all octaves */
    int32_t kp_cap;
    float* ori;                   /* kp_cap x SIFT_MAX_ORI */
    int32_t* n_ori;               /* kp_cap, then offsets within the octave */
    float* xyso;                  /* desc_cap x 4, all octaves */
    float* desc;                  /* desc_cap x 128 */
    int32_t desc_cap;
    SiftCounts* counts;
};

void mi_sift_gray(hipStream_t s, const void* pixels, int is_float, int channels, float* out, long long n);
/* out = blur(in); dog (may be null) = out - in.  tmp: w x h floats.  taps.ks == 0: a copy (dog: zeros). */
void mi_sift_blur(hipStream_t s, const float* in, float* tmp, float* out, float* dog, int w, int h, const SiftTaps& taps);
void mi_sift_half(hipStream_t s, const float* in, float* out, int w, int h);        /* out: (w + 1) / 2 x (h + 1) / 2 */
void mi_sift_double(hipStream_t s, const float* in, float* out, int w, int h);      /* out: 2 w x 2 h */
void mi_sift_detect_describe(hipStream_t s, const SiftOctaveArgs& a);
#endif
