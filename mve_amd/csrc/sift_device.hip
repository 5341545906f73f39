/*
 * sift_device.hip -- sfm::Sift::process (libs/sfm/sift.cc) on gfx950: scale space, extrema, localisation, orientations and
 * descriptors of one image.  All arithmetic is f32, as in the reference.  The stages and what they restate:
 *
 *   k_sift_gray        byte_to_float_image + desaturate<float>(DESATURATE_AVERAGE)      sift.cc:135-165
 *   k_sift_blur_rows   mve::image::blur_gaussian<float>, the x pass                      image_tools.h:1047-1061
 *   k_sift_blur_cols   ... the y pass, and the DoG image img - base in the same store    image_tools.h:1063-1077, sift.cc:252
 *   k_sift_copy        blur_gaussian with sigma < 0.1 (a copy; its DoG image is zero)    image_tools.h:1032
 *   k_sift_half        rescale_half_size_gaussian<float>                                 image_tools.h:619-693
 *   k_sift_double      rescale_double_size_supersample<float>                            image_tools.h:790-826
 *   k_sift_extrema     the 27-neighbour scan, one bit per centre                         sift.cc:287-335
 *   k_sift_scan        exclusive prefix sum of a count array (one workgroup)
 *   k_sift_emit        bits + offsets -> candidates in the order sample, y, x
 *   k_sift_localize    the Taylor steps and the five rejection tests, one lane per candidate   sift.cc:350-476
 *   k_sift_compact     survivors in list order -> keypoints
 *   k_sift_orient      36-bin histogram, smoothing, peaks: one wavefront per keypoint     sift.cc:579-589, :599-697
 *   k_sift_describe    4 x 4 x 8 histogram: one wavefront per (keypoint, orientation)    sift.cc:702-842
 *
 * Order and determinism.  Nothing is appended with atomics.  Lists are built from counts and a prefix sum (per row piece of
 * 64 centres for the extrema, per workgroup of 256 candidates for the survivors, per keypoint for the orientations), so
 * every list has the reference's order.  The two histogram kernels sum floats: every lane owns fixed window rows and a
 * histogram of its own in LDS (column `lane` of hist[bin][64]), walks its rows in the reference's order, and the 64 copies
 * are added in a fixed tree (lane l += lane l + 32, 16, ... 1).  The same input gives the same bits.
 *
 * The blur kernels stage a tile plus a halo of ks in LDS; a lane makes four neighbouring outputs and keeps a window of
 * eight inputs in registers, so four LDS values (one ds_read_b128 in the row pass) feed sixteen multiply-adds.  The taps run
 * i = -ks ... ks per output as in the reference; they are padded with zero weights to a multiple of four.
 *
 * No matrix instruction: the blurs are 1-D stencils with at most 65 taps on f32 data (an MFMA formulation as a banded
 * Toeplitz product would multiply mostly zeros), the rest is comparisons, a 3 x 3 solve per lane and scattered
 * histogram updates.
 *
 * Lists are capped by what the host allocated (cand_cap, kp_cap, desc_cap): writes beyond a cap are dropped, the counts
 * are not capped, and the host repeats the run with larger buffers when a count exceeds its cap.
 */
#include <hip/hip_runtime.h>

#include "sift_device.h"

typedef unsigned long long u64;

namespace {

#define SIFT_2PI 6.28318530717958647692f

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void k_sift_gray(const void* pixels, int is_float, int channels, float* out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v[3];
    for (int c = 0; c < channels; ++c) {
        if (is_float) v[c] = ((const float*)pixels)[i * channels + c];
        else v[c] = fminf(1.0f, fmaxf(0.0f, (float)((const unsigned char*)pixels)[i * channels + c] / 255.0f));
    }
    const float third = 1.0f / 3.0f;
    out[i] = channels == 3 ? v[0] * third + v[1] * third + v[2] * third : v[0];
}

/* four outputs of a lane against eight inputs: taps t0 ... t0 + 3 */
#define SIFT_TAPS4(v, wt, t0, acc)                                                  \
    _Pragma("unroll") for (int tt = 0; tt < 4; ++tt) {                              \
        const float wgt = wt[(t0) + tt];                                            \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) acc[j] += v[tt + j] * wgt;    \
    }

/* grid (ceil(w / 256), ceil(h / 4)), block (64, 4): a wavefront makes 256 pixels of one row.
 * LDS: 4 rows x (256 + 68) floats + 68 taps = 5.3 KiB. */
__global__ __launch_bounds__(256) void k_sift_blur_rows(const float* __restrict__ in, float* __restrict__ out, int w, int h, SiftTaps t) {
    __shared__ __attribute__((aligned(16))) float row[4][SIFT_BLUR_TW + SIFT_MAX_TAPS];
    __shared__ float wt[SIFT_MAX_TAPS];
    const int lane = threadIdx.x, r = threadIdx.y;
    const int y = blockIdx.y * 4 + r, x0 = blockIdx.x * SIFT_BLUR_TW;
    const float* src = in + (size_t)min(y, h - 1) * w;
    for (int p = lane; p < SIFT_BLUR_TW + t.ntaps; p += 64) row[r][p] = src[clampi(x0 - t.ks + p, 0, w - 1)];
    if (r == 0) for (int p = lane; p < SIFT_MAX_TAPS; p += 64) wt[p] = t.taps[p];
    __syncthreads();
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[8];
    const float4 a = *(const float4*)&row[r][lane * 4];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    for (int t0 = 0; t0 < t.ntaps; t0 += 4) {
        const float4 b = *(const float4*)&row[r][lane * 4 + t0 + 4];
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        SIFT_TAPS4(v, wt, t0, acc)
        v[0] = v[4]; v[1] = v[5]; v[2] = v[6]; v[3] = v[7];
    }
    if (y >= h) return;
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + lane * 4 + j;
        if (x < w) out[(size_t)y * w + x] = acc[j] / t.wsum;
    }
}

/* grid (ceil(w / 64), ceil(h / 32)), block (64, 4): a lane owns a column, a wavefront eight rows in two groups of four.
 * LDS: (32 + 68) rows x 64 floats + 68 taps = 25.3 KiB.  dog (may be null) = out - base. */
__global__ __launch_bounds__(256) void k_sift_blur_cols(const float* __restrict__ in, const float* __restrict__ base, float* __restrict__ out,
                                                        float* __restrict__ dog, int w, int h, SiftTaps t) {
    __shared__ float col[SIFT_BLUR_TH + SIFT_MAX_TAPS][64];
    __shared__ float wt[SIFT_MAX_TAPS];
    const int lane = threadIdx.x, wv = threadIdx.y;
    const int x = blockIdx.x * 64 + lane, y0 = blockIdx.y * SIFT_BLUR_TH;
    const int xc = min(x, w - 1);
    for (int r = wv; r < SIFT_BLUR_TH + t.ntaps; r += 4) col[r][lane] = in[(size_t)clampi(y0 - t.ks + r, 0, h - 1) * w + xc];
    if (wv == 0) for (int p = lane; p < SIFT_MAX_TAPS; p += 64) wt[p] = t.taps[p];
    __syncthreads();
    for (int g = 0; g < 2; ++g) {
        const int rb = wv * 8 + g * 4;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[8];
        for (int j = 0; j < 4; ++j) v[j] = col[rb + j][lane];
        for (int t0 = 0; t0 < t.ntaps; t0 += 4) {
            for (int j = 0; j < 4; ++j) v[4 + j] = col[rb + t0 + 4 + j][lane];
            SIFT_TAPS4(v, wt, t0, acc)
            v[0] = v[4]; v[1] = v[5]; v[2] = v[6]; v[3] = v[7];
        }
        for (int j = 0; j < 4; ++j) {
            const int y = y0 + rb + j;
            if (x >= w || y >= h) continue;
            const size_t o = (size_t)y * w + x;
            const float val = acc[j] / t.wsum;
            out[o] = val;
            if (dog) dog[o] = val - base[o];
        }
    }
}

__global__ __launch_bounds__(256) void k_sift_copy(const float* in, float* out, float* dog, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = in[i];
    if (dog) dog[i] = 0.0f;
}

/* one lane per output pixel, block (64, 4); 16 clamped taps with the weights w3 w2 w2 w3 / w2 w1 w1 w2 / ... */
__global__ __launch_bounds__(256) void k_sift_half(const float* __restrict__ in, float* __restrict__ out, int w, int h, float w1, float w2,
                                                   float w3, float wsum) {
    const int ow = (w + 1) >> 1, oh = (h + 1) >> 1;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ow || y >= oh) return;
    const int ys[4] = {max(0, 2 * y - 1), 2 * y, min(h - 1, 2 * y + 1), min(h - 1, 2 * y + 2)};
    const int xs[4] = {max(0, 2 * x - 1), 2 * x, min(w - 1, 2 * x + 1), min(w - 1, 2 * x + 2)};
    const float wr[4][4] = {{w3, w2, w2, w3}, {w2, w1, w1, w2}, {w2, w1, w1, w2}, {w3, w2, w2, w3}};
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc += in[(size_t)ys[r] * w + xs[c]] * wr[r][c];
    out[(size_t)y * ow + x] = acc / wsum;
}

__global__ __launch_bounds__(256) void k_sift_double(const float* __restrict__ in, float* __restrict__ out, int w, int h) {
    const int ow = w * 2, oh = h * 2;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ow || y >= oh) return;
    const int y0 = y >> 1, y1 = (y + (y + 1 < oh ? 1 : 0)) >> 1;
    const int x0 = x >> 1, x1 = (x + (x + 1 < ow ? 1 : 0)) >> 1;
    out[(size_t)y * ow + x] = in[(size_t)y0 * w + x0] * 0.25f + in[(size_t)y0 * w + x1] * 0.25f + in[(size_t)y1 * w + x0] * 0.25f
                              + in[(size_t)y1 * w + x1] * 0.25f;
}

/* grid (ceil(w / 64), ceil(h / 16), S), block (64, 4): the three DoG layers of 66 x 18 pixels in LDS (13.9 KiB); a wavefront
 * tests four rows of 64 centres and writes one word of bits and its count per row. */
__global__ __launch_bounds__(256) void k_sift_extrema(SiftOctaveArgs a) {
    __shared__ float t[3][SIFT_EXT_TH + 2][66];
    const int lane = threadIdx.x, wv = threadIdx.y, tid = wv * 64 + lane;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * SIFT_EXT_TH, s = blockIdx.z;
    const int w = a.w, h = a.h;
    const size_t wh = (size_t)w * h;
    for (int idx = tid; idx < 3 * (SIFT_EXT_TH + 2) * 66; idx += 256) {
        const int l = idx / ((SIFT_EXT_TH + 2) * 66), rem = idx % ((SIFT_EXT_TH + 2) * 66), ry = rem / 66, rx = rem % 66;
        t[l][ry][rx] = a.dog[(size_t)(s + l) * wh + (size_t)clampi(y0 - 1 + ry, 0, h - 1) * w + clampi(x0 - 1 + rx, 0, w - 1)];
    }
    __syncthreads();
    const int tiles_x = (w + 63) >> 6;
    for (int k = 0; k < 4; ++k) {
        const int ry = wv * 4 + k, y = y0 + ry, x = x0 + lane;
        const bool inside = y >= 1 && y < h - 1 && x >= 1 && x < w - 1;
        const float c = t[1][ry + 1][lane + 1];
        bool largest = inside, smallest = inside;
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                if (l == 1 && i == 4) continue;
                const float n = t[l][ry + i / 3][lane + i % 3];
                largest = largest && !(n >= c);
                smallest = smallest && !(n <= c);
            }
        const u64 mask = __ballot(largest || smallest);
        if (lane == 0 && y < h) {
            const size_t widx = ((size_t)s * h + y) * tiles_x + blockIdx.x;
            a.masks[widx] = mask;
            a.words[widx] = __popcll(mask);
        }
    }
}

/* data[0 ... n) becomes its exclusive prefix sum, *total the sum.  n = n_max, or min(n_max, *n_dev).  One workgroup of 1024. */
__global__ __launch_bounds__(1024) void k_sift_scan(int32_t* data, int n_max, const int32_t* n_dev, int32_t* total) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int n = n_dev ? min(n_max, *n_dev) : n_max;
    const int chunk = (n + 1023) / 1024;
    const int b = min(tid * chunk, n), e = min(b + chunk, n);
    int sum = 0;
    for (int i = b; i < e; ++i) sum += data[i];
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (int i = b; i < e; ++i) { const int v = data[i]; data[i] = run; run += v; }
    if (tid == 1023) *total = part[1023];
}

/* one wavefront per word of k_sift_extrema: candidates in the order sample, y, x */
__global__ __launch_bounds__(256) void k_sift_emit(SiftOctaveArgs a, int n_words) {
    const int lane = threadIdx.x & 63, widx = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (widx >= n_words) return;
    const u64 mask = a.masks[widx];
    if (!((mask >> lane) & 1ull)) return;
    const int tiles_x = (a.w + 63) >> 6;
    const int s = widx / (a.h * tiles_x), rem = widx % (a.h * tiles_x), y = rem / tiles_x, x = (rem % tiles_x) * 64 + lane;
    const long long i = (long long)a.words[widx] + __popcll(mask & ((1ull << lane) - 1ull));
    if (i < a.cand_cap) a.cand[i] = make_int2(x | (y << 16), s);
}

/* block 256, grid ceil(cand_cap / 256): loc[i] = x, y, sample, kept; block_off[b] = survivors of the workgroup */
__global__ __launch_bounds__(256) void k_sift_localize(SiftOctaveArgs a) {
    __shared__ int wave_total[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(a.counts->n_cand[a.slot], a.cand_cap);
    const int i = blockIdx.x * 256 + tid;
    bool keep = false;
    if (i < n) {
        const int2 c = a.cand[i];
        const int w = a.w, h = a.h, is = c.y;
        int ix = c.x & 0xffff, iy = c.x >> 16;
        const size_t wh = (size_t)w * h;
        const float* d0 = a.dog + (size_t)is * wh;
        const float* d1 = d0 + wh;
        const float* d2 = d1 + wh;
        float fx = 0.0f, fy = 0.0f, fs = 0.0f, Dx = 0.0f, Dy = 0.0f, Ds = 0.0f, Dxx = 0.0f, Dyy = 0.0f, Dxy = 0.0f;
        for (int j = 0; j < 5; ++j) {
            const size_t px = (size_t)iy * w + ix;
            const float c1 = d1[px];
            Dx = (d1[px + 1] - d1[px - 1]) * 0.5f;
            Dy = (d1[px + w] - d1[px - w]) * 0.5f;
            Ds = (d2[px] - d0[px]) * 0.5f;
            Dxx = d1[px + 1] + d1[px - 1] - 2.0f * c1;
            Dyy = d1[px + w] + d1[px - w] - 2.0f * c1;
            const float Dss = d2[px] + d0[px] - 2.0f * c1;
            Dxy = (d1[px + 1 + w] + d1[px - 1 - w] - d1[px - 1 + w] - d1[px + 1 - w]) * 0.25f;
            const float Dxs = (d2[px + 1] + d0[px - 1] - d2[px - 1] - d0[px + 1]) * 0.25f;
            const float Dys = (d2[px + w] + d0[px - w] - d2[px - w] - d0[px + w]) * 0.25f;
            /* A = [Dxx Dxy Dxs; Dxy Dyy Dys; Dxs Dys Dss]: determinant, then the adjugate over it */
            const float det = Dxx * Dyy * Dss + Dxy * Dys * Dxs + Dxs * Dxy * Dys - Dxs * Dyy * Dxs - Dxy * Dxy * Dss - Dxx * Dys * Dys;
            if (-1e-15f <= det && det <= 1e-15f) { fx = fy = fs = 0.0f; break; }
            const float r0 = (Dyy * Dss - Dys * Dys) / det, r1 = (Dxs * Dys - Dxy * Dss) / det, r2 = (Dxy * Dys - Dxs * Dyy) / det;
            const float r4 = (Dxx * Dss - Dxs * Dxs) / det, r5 = (Dxs * Dxy - Dxx * Dys) / det, r8 = (Dxx * Dyy - Dxy * Dxy) / det;
            fx = r0 * -Dx + r1 * -Dy + r2 * -Ds;
            fy = r1 * -Dx + r4 * -Dy + r5 * -Ds;
            fs = r2 * -Dx + r5 * -Dy + r8 * -Ds;
            const int dx = (fx > 0.6f && ix < w - 2 ? 1 : 0) - (fx < -0.6f && ix > 1 ? 1 : 0);
            const int dy = (fy > 0.6f && iy < h - 2 ? 1 : 0) - (fy < -0.6f && iy > 1 ? 1 : 0);
            if (dx == 0 && dy == 0) break;
            ix += dx; iy += dy;
        }
        const float val = d1[(size_t)iy * w + ix] + 0.5f * (Dx * fx + Dy * fy + Ds * fs);
        const float tr = Dxx + Dyy, hdet = Dxx * Dyy - Dxy * Dxy, score = tr * tr / hdet;
        const float thres = (a.edge_ratio_threshold + 1.0f) * (a.edge_ratio_threshold + 1.0f) / a.edge_ratio_threshold;
        const float kx = (float)ix + fx, ky = (float)iy + fy, ksm = (float)is + fs;
        const bool reject = fabsf(val) < a.contrast_threshold || score < 0.0f || score > thres || fabsf(fx) > 1.5f || fabsf(fy) > 1.5f
            || fabsf(fs) > 1.0f || ksm < -1.0f || ksm > (float)a.S || kx < 0.0f || kx > (float)(w - 1) || ky < 0.0f || ky > (float)(h - 1)
            || !(fx == fx) || !(fy == fy) || !(fs == fs);            /* (a solve that is not a number has no position) */
        keep = !reject;
        a.loc[i] = make_float4(kx, ky, ksm, keep ? 1.0f : 0.0f);
    }
    const u64 mask = __ballot(keep);
    if (lane == 0) wave_total[wave] = __popcll(mask);
    __syncthreads();
    if (tid == 0) a.block_off[blockIdx.x] = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
}

__device__ __forceinline__ int sift_base(const int32_t* per_octave, int slot) {
    long long b = 0;
    for (int o = 0; o < slot; ++o) b += per_octave[o];
    return (int)(b > 0x7fffffffll ? 0x7fffffffll : b);
}

__global__ __launch_bounds__(256) void k_sift_compact(SiftOctaveArgs a) {
    __shared__ int wave_total[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(a.counts->n_cand[a.slot], a.cand_cap);
    const int i = blockIdx.x * 256 + tid;
    float4 l = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < n) l = a.loc[i];
    const bool keep = l.w != 0.0f;
    const u64 mask = __ballot(keep);
    if (lane == 0) wave_total[wave] = __popcll(mask);
    __syncthreads();
    if (!keep) return;
    long long dst = (long long)sift_base(a.counts->n_kp, a.slot) + a.block_off[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int q = 0; q < wave; ++q) dst += wave_total[q];
    if (dst < a.kp_cap) { SiftKeypoint k; k.octave = a.octave; k.sample = l.z; k.x = l.x; k.y = l.y; a.kp[dst] = k; }
}

__device__ __forceinline__ float sift_round(float x) { return x > 0.0f ? floorf(x + 0.5f) : ceilf(x - 0.5f); }

/* generate_grad_ori_images (sift.cc:579-589) at one pixel; border pixels have magnitude 0 there and are skipped by the callers */
__device__ __forceinline__ void sift_grad(const float* img, int w, int x, int y, float* mag, float* ori) {
    const float* p = img + (size_t)y * w + x;
    const float dx = 0.5f * (p[1] - p[-1]), dy = 0.5f * (p[w] - p[-w]);
    const float at = atan2f(dy, dx);
    *mag = sqrtf(dx * dx + dy * dy);
    *ori = at < 0.0f ? at + SIFT_2PI : at;
}

/* the 64 per-lane copies of hist[nbins][64] added in a fixed tree; the sums end in column 0 */
__device__ __forceinline__ void sift_tree(float (*hist)[64], int nbins, int lane) {
    for (int stride = 32; stride >= 1; stride >>= 1) {
        __syncthreads();
        for (int idx = lane; idx < nbins * stride; idx += 64) {
            const int b = idx / stride, l = idx % stride;
            hist[b][l] += hist[b][l + stride];
        }
    }
    __syncthreads();
}

/* the window of descriptor_assignment (sift.cc:743-746); the product is double in the reference (MATH_SQRT2) */
__device__ __forceinline__ int sift_desc_win(float sigma) {
    return (int)(1.41421356237309504880 * (double)(3.0f * sigma) * 5.0 * 0.5);
}

/* block 64 (one wavefront), keypoints of the octave strided over the grid.  LDS: 36 x 64 floats + 36 = 9.1 KiB.
 * ori[i][0 ... n_ori[i]): the peaks in ascending bin order; i counts within the octave.  A keypoint whose descriptor window
 * leaves the image gets none: descriptor_assignment would refuse every one of them (its window is the larger one). */
__global__ __launch_bounds__(64) void k_sift_orient(SiftOctaveArgs a) {
    __shared__ float hist[36][64];
    __shared__ float hs[36];
    const int lane = threadIdx.x;
    const int base = sift_base(a.counts->n_kp, a.slot);
    const int n = min(a.counts->n_kp[a.slot], a.kp_cap);
    const int w = a.w, h = a.h;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        __syncthreads();
        if ((long long)base + i >= a.kp_cap) { if (lane == 0) a.n_ori[i] = 0; continue; }
        const SiftKeypoint kp = a.kp[base + i];
        const int ix = (int)(kp.x + 0.5f), iy = (int)(kp.y + 0.5f), is = clampi((int)sift_round(kp.sample), -1, a.S);
        const float sigma = a.base_blur_sigma * powf(2.0f, (kp.sample + 1.0f) / (float)a.S);
        const int win = (int)(sigma * 1.5f * 3.0f), dwin = sift_desc_win(sigma);
        if (ix < win || ix + win >= w || iy < win || iy + win >= h || ix < dwin || ix + dwin >= w || iy < dwin || iy + dwin >= h
            || win < 0 || dwin < 0) {
            if (lane == 0) a.n_ori[i] = 0;
            continue;
        }
        const float* img = a.img + (size_t)(is + 1) * w * h;
        const float dxf = kp.x - (float)ix, dyf = kp.y - (float)iy, maxdist = (float)(win * win) + 0.5f, sw = sigma * 1.5f;
        for (int b = 0; b < 36; ++b) hist[b][lane] = 0.0f;
        for (int dy = -win + lane; dy <= win; dy += 64) {
            const int y = iy + dy;
            if (y < 1 || y >= h - 1) continue;
            for (int dx = -win; dx <= win; ++dx) {
                const float dist = ((float)dx - dxf) * ((float)dx - dxf) + ((float)dy - dyf) * ((float)dy - dyf);
                const int x = ix + dx;
                if (dist > maxdist || x < 1 || x >= w - 1) continue;
                float gm, go;
                sift_grad(img, w, x, y, &gm, &go);
                const float weight = expf(-(dist / (2.0f * sw * sw)));
                const int bin = clampi((int)(36.0f * go / SIFT_2PI), 0, 35);
                hist[bin][lane] += gm * weight;
            }
        }
        sift_tree(hist, 36, lane);
        if (lane < 36) hs[lane] = hist[lane][0];
        __syncthreads();
        for (int pass = 0; pass < 6; ++pass) {                    /* every new value is made of old ones, also in the reference's loop */
            float v = 0.0f;
            if (lane < 36) v = (hs[(lane + 35) % 36] + hs[lane] + hs[(lane + 1) % 36]) / 3.0f;
            __syncthreads();
            if (lane < 36) hs[lane] = v;
            __syncthreads();
        }
        float maxh = hs[0];
        for (int b = 1; b < 36; ++b) maxh = fmaxf(maxh, hs[b]);
        bool peak = false;
        float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
        if (lane < 36) {
            h0 = hs[(lane + 35) % 36]; h1 = hs[lane]; h2 = hs[(lane + 1) % 36];
            peak = !(h1 <= 0.8f * maxh || h1 <= h0 || h1 <= h2);
        }
        const u64 mask = __ballot(peak);
        if (peak) {
            const float x = -0.5f * (h2 - h0) / (h0 - 2.0f * h1 + h2);
            a.ori[(size_t)i * SIFT_MAX_ORI + __popcll(mask & ((1ull << lane) - 1ull))] = SIFT_2PI * (x + (float)lane + 0.5f) / 36.0f;
        }
        if (lane == 0) a.n_ori[i] = __popcll(mask);
    }
}

__device__ __forceinline__ float sift_wave_sum(float v) {          /* the same tree in every lane: the same bits in every lane */
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

/* block 64 (one wavefront), the octave's (keypoint, orientation) pairs strided over the grid.  LDS: 128 x 64 floats = 32 KiB. */
__global__ __launch_bounds__(64) void k_sift_describe(SiftOctaveArgs a) {
    __shared__ float hist[128][64];
    const int lane = threadIdx.x;
    const int base_kp = sift_base(a.counts->n_kp, a.slot), base_desc = sift_base(a.counts->n_desc, a.slot);
    const int n_kp = min(a.counts->n_kp[a.slot], a.kp_cap), n_desc = a.counts->n_desc[a.slot];
    const int w = a.w, h = a.h;
    for (int d = blockIdx.x; d < n_desc; d += gridDim.x) {
        if ((long long)base_desc + d >= a.desc_cap) break;
        int lo = 0, hi = n_kp - 1;                                /* the last keypoint whose first pair is not behind d */
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.n_ori[mid] <= d) lo = mid; else hi = mid - 1;
        }
        const int j = d - a.n_ori[lo];
        if ((long long)base_kp + lo >= a.kp_cap || j < 0 || j >= SIFT_MAX_ORI) continue;
        const SiftKeypoint kp = a.kp[base_kp + lo];
        const float orientation = a.ori[(size_t)lo * SIFT_MAX_ORI + j];
        const int ix = (int)(kp.x + 0.5f), iy = (int)(kp.y + 0.5f), is = clampi((int)sift_round(kp.sample), -1, a.S);
        const float dxf = kp.x - (float)ix, dyf = kp.y - (float)iy;
        const float sigma = a.base_blur_sigma * powf(2.0f, (kp.sample + 1.0f) / (float)a.S);
        const float sino = sinf(orientation), coso = cosf(orientation), binsize = 3.0f * sigma;
        const int win = sift_desc_win(sigma);
        if (ix < win || ix + win >= w || iy < win || iy + win >= h || win < 0) continue;      /* (k_sift_orient gave these no pair) */
        const float* img = a.img + (size_t)(is + 1) * w * h;
        __syncthreads();
        for (int b = 0; b < 128; ++b) hist[b][lane] = 0.0f;
        for (int dy = -win + lane; dy <= win; dy += 64) {
            const int y = iy + dy;
            if (y < 1 || y >= h - 1) continue;
            for (int dx = -win; dx <= win; ++dx) {
                const int x = ix + dx;
                if (x < 1 || x >= w - 1) continue;
                float mod, angle;
                sift_grad(img, w, x, y, &mod, &angle);
                float theta = angle - orientation;
                if (theta < 0.0f) theta += SIFT_2PI;
                const float winx = (float)dx - dxf, winy = (float)dy - dyf;
                const float binx = (coso * winx + sino * winy) / binsize + 1.5f;
                const float biny = (-sino * winx + coso * winy) / binsize + 1.5f;
                const float bint = theta * 8.0f / SIFT_2PI - 0.5f;
                const float contrib = mod * expf(-(((binx - 1.5f) * (binx - 1.5f) + (biny - 1.5f) * (biny - 1.5f)) / 8.0f));
                const int bx0 = (int)floorf(binx), by0 = (int)floorf(biny), bt0 = (int)floorf(bint);
                const float wx[2] = {(float)(bx0 + 1) - binx, 1.0f - ((float)(bx0 + 1) - binx)};
                const float wy[2] = {(float)(by0 + 1) - biny, 1.0f - ((float)(by0 + 1) - biny)};
                const float wt[2] = {(float)(bt0 + 1) - bint, 1.0f - ((float)(bt0 + 1) - bint)};
                const int bt[2] = {bt0 < 0 ? bt0 + 8 : bt0, bt0 + 1 >= 8 ? bt0 + 1 - 8 : bt0 + 1};
                if (bt[0] < 0 || bt[0] > 7 || bt[1] < 0 || bt[1] > 7) continue;               /* (an angle that is not a number) */
#pragma unroll
                for (int yy = 0; yy < 2; ++yy)
#pragma unroll
                    for (int xx = 0; xx < 2; ++xx)
#pragma unroll
                        for (int tt = 0; tt < 2; ++tt) {
                            const int bx = bx0 + xx, by = by0 + yy;
                            if (bx < 0 || bx >= 4 || by < 0 || by >= 4) continue;
                            hist[bt[tt] + bx * 8 + by * 32][lane] += contrib * wx[xx] * wy[yy] * wt[tt];
                        }
            }
        }
        sift_tree(hist, 128, lane);
        float v0 = hist[lane][0], v1 = hist[lane + 64][0];
        float norm = sqrtf(sift_wave_sum(v0 * v0 + v1 * v1));
        v0 = fminf(v0 / norm, 0.2f); v1 = fminf(v1 / norm, 0.2f);
        norm = sqrtf(sift_wave_sum(v0 * v0 + v1 * v1));
        const size_t o = (size_t)base_desc + d;
        a.desc[o * 128 + lane] = v0 / norm;
        a.desc[o * 128 + lane + 64] = v1 / norm;
        if (lane == 0) {
            const float f = powf(2.0f, (float)kp.octave);
            a.xyso[o * 4 + 0] = f * (kp.x + 0.5f) - 0.5f;
            a.xyso[o * 4 + 1] = f * (kp.y + 0.5f) - 0.5f;
            a.xyso[o * 4 + 2] = a.base_blur_sigma * powf(2.0f, (float)kp.octave + (kp.sample + 1.0f) / (float)a.S);
            a.xyso[o * 4 + 3] = orientation;
        }
    }
}

}  /* namespace */

void mi_sift_gray(hipStream_t s, const void* pixels, int is_float, int channels, float* out, long long n) {
    hipLaunchKernelGGL(k_sift_gray, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pixels, is_float, channels, out, n);
}

void mi_sift_blur(hipStream_t s, const float* in, float* tmp, float* out, float* dog, int w, int h, const SiftTaps& taps) {
    if (taps.ks == 0) {
        const long long n = (long long)w * h;
        hipLaunchKernelGGL(k_sift_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, dog, n);
        return;
    }
    hipLaunchKernelGGL(k_sift_blur_rows, dim3((unsigned)((w + SIFT_BLUR_TW - 1) / SIFT_BLUR_TW), (unsigned)((h + 3) / 4)), dim3(64, 4), 0, s,
                       in, tmp, w, h, taps);
    hipLaunchKernelGGL(k_sift_blur_cols, dim3((unsigned)((w + 63) / 64), (unsigned)((h + SIFT_BLUR_TH - 1) / SIFT_BLUR_TH)), dim3(64, 4), 0, s,
                       (const float*)tmp, in, out, dog, w, h, taps);
}

void mi_sift_half(hipStream_t s, const float* in, float* out, int w, int h) {
    /* the three weights of sigma = 0.866025403784439 (image_tools.h:638-640), summed in the order of the 16 taps */
    const float sigma = 0.866025403784439f, s2 = 2.0f * (sigma * sigma);
    const float w1 = std::exp(-0.5f / s2), w2 = std::exp(-2.5f / s2), w3 = std::exp(-4.5f / s2);
    const float row[4][4] = {{w3, w2, w2, w3}, {w2, w1, w1, w2}, {w2, w1, w1, w2}, {w3, w2, w2, w3}};
    float wsum = 0.0f;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) wsum += row[r][c];
    const int ow = (w + 1) >> 1, oh = (h + 1) >> 1;
    hipLaunchKernelGGL(k_sift_half, dim3((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4)), dim3(64, 4), 0, s, in, out, w, h, w1, w2, w3, wsum);
}

void mi_sift_double(hipStream_t s, const float* in, float* out, int w, int h) {
    hipLaunchKernelGGL(k_sift_double, dim3((unsigned)((2 * w + 63) / 64), (unsigned)((2 * h + 3) / 4)), dim3(64, 4), 0, s, in, out, w, h);
}

void mi_sift_detect_describe(hipStream_t s, const SiftOctaveArgs& a) {
    SiftCounts* c = a.counts;
    if (a.w < 3 || a.h < 3) {                                     /* no interior pixel: the octave's three counts are zero */
        hipLaunchKernelGGL(k_sift_scan, dim3(1), dim3(1024), 0, s, a.words, 0, (const int32_t*)nullptr, &c->n_cand[a.slot]);
        hipLaunchKernelGGL(k_sift_scan, dim3(1), dim3(1024), 0, s, a.words, 0, (const int32_t*)nullptr, &c->n_kp[a.slot]);
        hipLaunchKernelGGL(k_sift_scan, dim3(1), dim3(1024), 0, s, a.words, 0, (const int32_t*)nullptr, &c->n_desc[a.slot]);
        return;
    }
    const int tiles_x = (a.w + 63) / 64, n_words = a.S * a.h * tiles_x, n_blocks = (a.cand_cap + 255) / 256;
    hipLaunchKernelGGL(k_sift_extrema, dim3((unsigned)tiles_x, (unsigned)((a.h + SIFT_EXT_TH - 1) / SIFT_EXT_TH), (unsigned)a.S), dim3(64, 4), 0, s, a);
    hipLaunchKernelGGL(k_sift_scan, dim3(1), dim3(1024), 0, s, a.words, n_words, (const int32_t*)nullptr, &c->n_cand[a.slot]);
    hipLaunchKernelGGL(k_sift_emit, dim3((unsigned)((n_words + 3) / 4)), dim3(256), 0, s, a, n_words);
    hipLaunchKernelGGL(k_sift_localize, dim3((unsigned)n_blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_sift_scan, dim3(1), dim3(1024), 0, s, a.block_off, n_blocks, (const int32_t*)nullptr, &c->n_kp[a.slot]);
    hipLaunchKernelGGL(k_sift_compact, dim3((unsigned)n_blocks), dim3(256), 0, s, a);
    const unsigned waves = (unsigned)(a.kp_cap < 8192 ? a.kp_cap : 8192);
    hipLaunchKernelGGL(k_sift_orient, dim3(waves), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_sift_scan, dim3(1), dim3(1024), 0, s, a.n_ori, a.kp_cap, (const int32_t*)&c->n_kp[a.slot], &c->n_desc[a.slot]);
    hipLaunchKernelGGL(k_sift_describe, dim3(waves), dim3(64), 0, s, a);
}
