/*
 * surf_device.hip -- sfm::Surf::set_image + process (libs/sfm/surf.cc) on gfx950: summed-area table, the 16 Hessian response
 * maps, extrema with sub-pixel localisation, orientations and the 64-value descriptors of one image.  The stages and what they
 * restate:
 *
 *   k_surf_rows        desaturate<uint8_t>(DESATURATE_LIGHTNESS) + the row sums of integral_image   surf.cc:124-138
 *   k_surf_cols        ... its column sums                                                          image_tools.h:1597-1635
 *   k_surf_response0   create_response_map, filter_dxx / dyy / dxy for octave 0 (fs 3 5 7 9)        surf.cc:158-306
 *   k_surf_response    ... for octaves 1 - 3
 *   k_surf_detect      extrema_detection, check_maximum, keypoint_localization (count / emit)      surf.cc:310-474
 *   k_surf_scan        exclusive prefix sum of a count array (one workgroup)
 *   k_surf_orient      descriptor_orientation, filter_dx_dy: one wavefront per keypoint             surf.cc:515-660
 *   k_surf_describe    descriptor_computation: one wavefront per keypoint                           surf.cc:664-732
 *   k_surf_compact     descriptor_assignment's push_back: descriptors in keypoint order            surf.cc:478-511
 *
 * The summed-area table holds the reference's int64 values modulo 2^32.  Every sum a filter takes is a combination of box
 * sums whose true value lies within +-2^24 (the largest box is 195 x 129 pixels of 255), so unsigned 32-bit arithmetic that
 * wraps gives it exactly whatever the image size.
 *
 * Rounding.  The filter sums are integers.  A response is float(sum) * inv_karea per filter, then dxx * dyy - 0.912f * dxy *
 * dxy as single f32 operations in that order; the file is compiled without contraction.  The localisation runs in f64 with
 * the reference's expressions.  dx and dy of a Haar sample are single f32 operations, atan2 runs in f64, and the window sums
 * and the descriptor bins are added by ONE lane each in the reference's own order (the samples wait in LDS), so they have
 * the reference's bits wherever sinf, cosf and atan2 agree.
 *
 * Order and determinism.  Nothing is appended with atomics.  k_surf_detect runs twice per octave: the first run counts the
 * survivors per row piece of 64 pixels, k_surf_scan turns the counts of all octaves into offsets, the second run repeats the
 * same arithmetic and writes each survivor to its place: the list has the reference's order (octave, sample, y, x).
 * Descriptors are written per keypoint and compacted by a scan of their flags.  The same input gives the same bytes.
 *
 * No matrix instruction: the maps are gathers of 32 table values per pixel and filter with integer adds, the per-keypoint
 * work is 109 + 400 Haar samples of 12 gathers each and a 3 x 3 solve; there is no product of matrices to feed an MFMA.
 *
 * The keypoint list is capped by what the host allocated (kp_cap): writes beyond it are dropped, the count is not capped,
 * and the host repeats the run with larger buffers when the count exceeds the cap.
 */
#include <hip/hip_runtime.h>

#include "surf_device.h"

typedef unsigned long long u64;

namespace {

__device__ const int c_surf_fs[4][4] = {{3, 5, 7, 9}, {5, 9, 13, 17}, {9, 17, 25, 33}, {17, 33, 49, 65}};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint32_t surf_grey(const unsigned char* row, int x, int channels) {
    if (channels == 1) return row[x];
    const uint32_t r = row[3 * x], g = row[3 * x + 1], b = row[3 * x + 2];
    return (max(r, max(g, b)) + min(r, min(g, b)) + 1u) >> 1;
}

/* inclusive sum over the lanes 0 ... lane of a wavefront */
__device__ __forceinline__ uint32_t surf_wave_scan(uint32_t s, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(s, d, 64);
        if (lane >= d) s += t;
    }
    return s;
}

/* grid h, block 256: a workgroup owns a row and walks it in pieces of 1024 pixels.  A lane sums its four pixels, the lane
 * totals are scanned across the wavefront, the four wavefront totals meet in LDS, the carry of the row stays in a register. */
__global__ __launch_bounds__(256) void k_surf_rows(SurfArgs a) {
    __shared__ uint32_t wave_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w = a.w;
    const unsigned char* src = a.pixels + (size_t)blockIdx.x * w * a.channels;
    uint32_t* dst = a.sat + (size_t)blockIdx.x * w;
    uint32_t carry = 0;
    for (int x0 = 0; x0 < w; x0 += SURF_ROW_CHUNK) {
        const int x = x0 + tid * 4;
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = x + j < w ? surf_grey(src, x + j, a.channels) : 0u;
        v[1] += v[0]; v[2] += v[1]; v[3] += v[2];
        const uint32_t s = surf_wave_scan(v[3], lane);
        if (lane == 63) wave_sum[wave] = s;
        __syncthreads();
        uint32_t base = carry + (s - v[3]);
        for (int q = 0; q < wave; ++q) base += wave_sum[q];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j < w) dst[x + j] = base + v[j];
        carry += wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        __syncthreads();
    }
}

/* grid ceil(w / 64), block (64, 4): a workgroup owns 64 columns and walks down in tiles of 64 rows.  A tile is read row by row
 * (a lane per column: coalesced), scanned TRANSPOSED (a lane per row, a wavefront per 16 columns; the row stride of 65 words
 * keeps the column reads free of bank conflicts), and written back row by row.  In place: a tile is read whole before it is
 * written.  LDS: 64 x 65 + 64 words = 16.5 KiB. */
__global__ __launch_bounds__(256) void k_surf_cols(SurfArgs a) {
    __shared__ uint32_t tile[SURF_COL_TILE][SURF_COL_TILE + 1];
    __shared__ uint32_t carry[SURF_COL_TILE];
    const int lane = threadIdx.x, wv = threadIdx.y, w = a.w, h = a.h;
    const int x = blockIdx.x * SURF_COL_TILE + lane;
    if (wv == 0) carry[lane] = 0u;
    for (int y0 = 0; y0 < h; y0 += SURF_COL_TILE) {
        __syncthreads();
        for (int r = wv; r < SURF_COL_TILE; r += 4) {
            const int y = y0 + r;
            tile[r][lane] = x < w && y < h ? a.sat[(size_t)y * w + x] : 0u;
        }
        __syncthreads();
        for (int c = wv * 16; c < wv * 16 + 16; ++c) {
            const uint32_t before = carry[c];
            const uint32_t s = surf_wave_scan(tile[lane][c], lane) + before;
            tile[lane][c] = s;
            if (lane == 63) carry[c] = s;
        }
        __syncthreads();
        for (int r = wv; r < SURF_COL_TILE; r += 4) {
            const int y = y0 + r;
            if (x < w && y < h) a.sat[(size_t)y * w + x] = tile[r][lane];
        }
    }
}

/* The Hessian response of filter size fs at a pixel; at(dx, dy) is the table value at that offset from it. */
template <class At>
__device__ __forceinline__ float surf_hessian(At at, int fs) {
    const int fs2 = fs / 2;
    uint32_t v0, v1, v2, v3, v4, v5, v6, v7;
    {   /* filter_dxx: three boxes of fs x (2 fs - 1) side by side, weights 1 -2 1 */
        const int ax = -fs - fs2 - 1, ay = -fs, by = ay + 2 * fs - 1;
        v0 = at(ax, ay); v1 = at(ax + fs, ay); v2 = at(ax + 2 * fs, ay); v3 = at(ax + 3 * fs, ay);
        v4 = at(ax, by); v5 = at(ax + fs, by); v6 = at(ax + 2 * fs, by); v7 = at(ax + 3 * fs, by);
    }
    const uint32_t dxx = (v5 + v0 - v4 - v1) - 2u * (v6 + v1 - v5 - v2) + (v7 + v2 - v6 - v3);
    {   /* filter_dyy: the same boxes one above the other */
        const int cx = -fs, ex = cx + 2 * fs - 1, cy = -fs - fs2 - 1;
        v0 = at(cx, cy); v1 = at(cx, cy + fs); v2 = at(cx, cy + 2 * fs); v3 = at(cx, cy + 3 * fs);
        v4 = at(ex, cy); v5 = at(ex, cy + fs); v6 = at(ex, cy + 2 * fs); v7 = at(ex, cy + 3 * fs);
    }
    const uint32_t dyy = (v5 + v0 - v1 - v4) - 2u * (v6 + v1 - v2 - v5) + (v7 + v2 - v3 - v6);
    /* filter_dxy: four boxes of fs x fs around the pixel, weights + - / - + */
    const int px = -fs - 1, qx = 0, r1 = -fs - 1, r2 = -1, r3 = 0, r4 = fs;
    uint32_t dxy = at(px + fs, r2) + at(px, r1) - at(px, r2) - at(px + fs, r1);
    dxy -= at(qx + fs, r2) + at(qx, r1) - at(qx, r2) - at(qx + fs, r1);
    dxy -= at(px + fs, r4) + at(px, r3) - at(px, r4) - at(px + fs, r3);
    dxy += at(qx + fs, r4) + at(qx, r3) - at(qx, r4) - at(qx + fs, r3);
    const float inv_karea = (float)(1.0 / (double)(fs * (2 * fs - 1)));
    const float dxx_t = __fmul_rn((float)(int32_t)dxx, inv_karea);
    const float dyy_t = __fmul_rn((float)(int32_t)dyy, inv_karea);
    const float dxy_t = __fmul_rn((float)(int32_t)dxy, inv_karea);
    return __fsub_rn(__fmul_rn(dxx_t, dyy_t), __fmul_rn(__fmul_rn(0.912f, dxy_t), dxy_t));
}

/* grid (ceil(w / 64), ceil(h / 16)), block (64, 4): the SAT tile of 64 x 16 pixels with its halo of 14 / 13 (91 x 43 values,
 * 15.3 KiB) is staged once; a wavefront makes four rows of all four maps of octave 0 from it: 128 LDS reads per pixel
 * instead of 128 gathers. */
__global__ __launch_bounds__(256) void k_surf_response0(SurfArgs a) {
    constexpr int TW = SURF_R0_TW + SURF_R0_LO + SURF_R0_HI, TH = SURF_R0_TH + SURF_R0_LO + SURF_R0_HI;
    __shared__ uint32_t t[TH][TW];
    const int lane = threadIdx.x, wv = threadIdx.y, tid = wv * 64 + lane;
    const int x0 = blockIdx.x * SURF_R0_TW, y0 = blockIdx.y * SURF_R0_TH, w = a.w, h = a.h;
    for (int idx = tid; idx < TH * TW; idx += 256) {
        const int ry = idx / TW, rx = idx % TW;
        t[ry][rx] = a.sat[(size_t)clampi(y0 - SURF_R0_LO + ry, 0, h - 1) * w + clampi(x0 - SURF_R0_LO + rx, 0, w - 1)];
    }
    __syncthreads();
    const size_t wh = (size_t)w * h;
    const int x = x0 + lane;
    if (x >= w) return;
    for (int k = 0; k < 4; ++k) {
        const int ry = wv * 4 + k, y = y0 + ry;
        if (y >= h) return;
        auto at = [&](int dx, int dy) { return t[ry + SURF_R0_LO + dy][lane + SURF_R0_LO + dx]; };
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int fs = 3 + 2 * m, border = fs + fs / 2 + 1;
            const bool out = x < border || x + border >= w || y < border || y + border >= h;
            a.maps[a.map_off[0] + (size_t)m * wh + (size_t)y * w + x] = out ? 0.0f : surf_hessian(at, fs);
        }
    }
}

/* grid (ceil(ow[1] / 64), ceil(oh[1] / 4), 3), block (64, 4): octaves 1 - 3 gather from the table directly.  Their halos
 * (26 ... 98 pixels) against a sample spacing of 2 ... 8 would make an LDS tile mostly halo; the 32 values of a filter lie on
 * eight rows and neighbouring lanes read neighbouring (strided) addresses of them, which the L2 serves. */
__global__ __launch_bounds__(256) void k_surf_response(SurfArgs a) {
    const int o = blockIdx.z + 1;
    const int xo = blockIdx.x * 64 + threadIdx.x, yo = blockIdx.y * 4 + threadIdx.y;
    const int ow = a.ow[o], oh = a.oh[o], w = a.w, h = a.h;
    if (xo >= ow || yo >= oh) return;
    const int x = xo << o, y = yo << o;
    const uint32_t* p = a.sat + (size_t)y * w + x;
    auto at = [&](int dx, int dy) { return p[(long long)dy * w + dx]; };
    for (int m = 0; m < 4; ++m) {
        const int fs = c_surf_fs[o][m], border = fs + fs / 2 + 1;
        const bool out = x < border || x + border >= w || y < border || y + border >= h;
        a.maps[a.map_off[o] + (size_t)m * ow * oh + (size_t)yo * ow + xo] = out ? 0.0f : surf_hessian(at, fs);
    }
}

/* keypoint_localization at the extremum (x, y) of sample s; s0 / s1 / s2 point at it in the three maps of width w */
__device__ bool surf_localize(const float* s0, const float* s1, const float* s2, int w, int o, int s, int x, int y, const SurfArgs& a,
                              SurfKeypoint* out) {
    const int off[9] = {-1 - w, -w, 1 - w, -1, 0, 1, w - 1, w, 1 + w};
    float n0[9], n1[9], n2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { n0[i] = s0[off[i]]; n1[i] = s1[off[i]]; n2[i] = s2[off[i]]; }
    /* differences of neighbours in f32, as the reference's expressions have them, everything behind in f64 */
    const double b0 = (double)(-(n1[5] - n1[3])) * 0.5, b1 = (double)(-(n1[7] - n1[1])) * 0.5, b2 = (double)(-(n2[4] - n0[4])) * 0.5;
    const double m0 = (double)n1[3] - 2.0 * (double)n1[4] + (double)n1[5];
    const double m1 = (double)(n1[8] - n1[6] - n1[2] + n1[0]) * 0.25;
    const double m2 = (double)(n2[5] - n2[3] - n0[5] + n0[3]) * 0.25;
    const double m4 = (double)n1[1] - 2.0 * (double)n1[4] + (double)n1[7];
    const double m5 = (double)(n2[7] - n2[1] - n0[7] + n0[1]) * 0.25;
    const double m8 = (double)n0[4] - 2.0 * (double)n1[4] + (double)n2[4];
    const double m3 = m1, m6 = m2, m7 = m5;
    const double det = m0 * m4 * m8 + m1 * m5 * m6 + m2 * m3 * m7 - m2 * m4 * m6 - m1 * m3 * m8 - m0 * m5 * m7;
    const double eps = (double)1.0e-5f;
    if (-eps <= det && det <= eps) return false;
    const double i0 = (m4 * m8 - m5 * m7) / det, i1 = (m2 * m7 - m1 * m8) / det, i2 = (m1 * m5 - m2 * m4) / det;
    const double i3 = (m5 * m6 - m3 * m8) / det, i4 = (m0 * m8 - m2 * m6) / det, i5 = (m2 * m3 - m0 * m5) / det;
    const double i6 = (m3 * m7 - m4 * m6) / det, i7 = (m1 * m6 - m0 * m7) / det, i8 = (m0 * m4 - m1 * m3) / det;
    const double vx = i0 * b0 + i1 * b1 + i2 * b2, vy = i3 * b0 + i4 * b1 + i5 * b2, vs = i6 * b0 + i7 * b1 + i8 * b2;
    const double hi = fmax(vx, fmax(vy, vs)), lo = fmin(vx, fmin(vy, vs));
    if (!(hi <= 0.5) || !(lo >= -0.5)) return false;               /* (a solve that is not a number has no position either) */
    const float value = (float)((double)n1[4] - 0.5 * (b0 * vx + b1 * vy + b2 * vs));
    if (value < a.contrast_threshold) return false;
    const float sampling = (float)(1 << o);
    const float kx = (float)(((double)(float)x + vx) * (double)sampling), ky = (float)(((double)(float)y + vy) * (double)sampling);
    if (kx < 0.0f || kx + 1.0f > (float)a.w || ky < 0.0f || ky + 1.0f > (float)a.h) return false;
    out->octave = o; out->sample = (float)((double)(float)s + vs); out->x = kx; out->y = ky;
    return true;
}

/* grid (ceil(ow / 64), ceil(oh / 4), 2), block (64, 4): a wavefront tests 64 pixels of a row of sample 1 or 2 of octave o.
 * EMIT false: words[piece] = survivors.  EMIT true (words hold offsets now): the same test again, survivors to their places.
 * Only interior pixels are tested: a pixel of the first or last row is in the zero border of every map, and 0 > 0 fails the
 * reference's first comparison, so it tests them in vain; every pixel it keeps has its 26 neighbours inside the maps. */
template <bool EMIT>
__global__ __launch_bounds__(256) void k_surf_detect(SurfArgs a, int o) {
    const int lane = threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, s = blockIdx.z + 1, x = blockIdx.x * 64 + lane;
    const int ow = a.ow[o], oh = a.oh[o];
    if (y >= oh) return;
    bool keep = false;
    SurfKeypoint kp;
    if (x >= 1 && x < ow - 1 && y >= 1 && y < oh - 1) {
        const size_t wh = (size_t)ow * oh;
        const float* s1 = a.maps + a.map_off[o] + (size_t)s * wh + (size_t)y * ow + x;
        const float* s0 = s1 - wh;
        const float* s2 = s1 + wh;
        const float v = s1[0];
        if (v > s1[-1] && v > s1[1]) {
            bool largest = true;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int q = dy * ow + dx;
                    if (q != 0 && s1[q] >= v) largest = false;
                    if (s0[q] >= v || s2[q] >= v) largest = false;
                }
            if (largest) keep = surf_localize(s0, s1, s2, ow, o, s, x, y, a, &kp);
        }
    }
    const u64 mask = __ballot(keep);
    const int tiles_x = (ow + 63) >> 6;
    const int widx = a.word_off[o] + ((s - 1) * oh + y) * tiles_x + (int)blockIdx.x;
    if (!EMIT) {
        if (lane == 0) a.words[widx] = __popcll(mask);
    } else if (keep) {
        const long long i = (long long)a.words[widx] + __popcll(mask & ((1ull << lane) - 1ull));
        if (i < a.kp_cap) a.kp[i] = kp;
    }
}

/* data[0 ... n) becomes its exclusive prefix sum, *total the sum.  n = n_max, or min(n_max, *n_dev).  One workgroup of 1024. */
__global__ __launch_bounds__(1024) void k_surf_scan(int32_t* data, int n_max, const int32_t* n_dev, int32_t* total) {
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

/* filter_dx_dy: the Haar responses of size fs at (x, y); the caller keeps x -+ (fs + 1) and y -+ (fs + 1) inside the image */
__device__ __forceinline__ void surf_haar(const uint32_t* sat, int w, int x, int y, int fs, float* dx, float* dy) {
    const uint32_t* top = sat + (size_t)(y - fs - 1) * w + (x - fs - 1);
    const uint32_t* bot = top + (size_t)(2 * fs + 1) * w;
    const uint32_t* mid = top + (size_t)fs * w;
    const uint32_t x1 = top[0], x2 = top[fs], x3 = top[fs + 1], x4 = top[2 * fs + 1];
    const uint32_t x5 = bot[0], x6 = bot[fs], x7 = bot[fs + 1], x8 = bot[2 * fs + 1];
    const uint32_t y1 = mid[0], y2 = mid[2 * fs + 1], y3 = mid[w], y4 = mid[w + 2 * fs + 1];
    const float norm = (float)((2 * fs + 1) * fs * (fs + 1));
    *dx = __fdiv_rn((float)(int32_t)((x8 + x2 - x4 - x6) - (x7 + x1 - x3 - x5)), norm);
    *dy = __fdiv_rn((float)(int32_t)((x8 + y1 - x5 - y2) - (y4 + x1 - y3 - x4)), norm);
}

/* Descriptor::scale of a keypoint and its integer part */
__device__ __forceinline__ float surf_scale(const SurfTables* tab, const SurfKeypoint& kp) {
    return tab->scale[clampi(kp.octave, 0, 3)][clampi((int)(kp.sample + 0.5f), 0, 3)];
}

/* block 64 (one wavefront), the keypoints strided over the grid.  The 109 samples go over the lanes (two rounds); dx, dy and
 * the f64 angle of each wait in LDS.  Then lane k < n_win adds window k's samples in the order 0 ... 108 in f64, exactly the
 * reference's loop, and lane 0 keeps the first longest window.  LDS: tables 1.3 KiB + samples 1.7 KiB. */
__global__ __launch_bounds__(64) void k_surf_orient(SurfArgs a) {
    __shared__ float g[SURF_SAMPLES], sdx[SURF_SAMPLES], sdy[SURF_SAMPLES];
    __shared__ int rx[SURF_SAMPLES], ry[SURF_SAMPLES];
    __shared__ double ang[SURF_SAMPLES], wsx[SURF_MAX_WINDOWS], wsy[SURF_MAX_WINDOWS];
    const int lane = threadIdx.x, w = a.w, h = a.h;
    const int n = min(a.counts->n_kp, a.kp_cap), n_win = min(a.tab->n_win, SURF_MAX_WINDOWS);
    for (int q = lane; q < SURF_SAMPLES; q += 64) { g[q] = a.tab->gaussian[q]; rx[q] = a.tab->rx[q]; ry[q] = a.tab->ry[q]; }
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const SurfKeypoint kp = a.kp[i];
        const int px = (int)(kp.x + 0.5f), py = (int)(kp.y + 0.5f), sc = (int)surf_scale(a.tab, kp);
        const int spacing = 8 * sc + 1;
        if (sc < 1 || px < spacing || py < spacing || px + spacing >= w || py + spacing >= h) {
            if (lane == 0) a.stage[i] = 0;
            continue;
        }
        __syncthreads();
        for (int q = lane; q < SURF_SAMPLES; q += 64) {
            float dx, dy;
            surf_haar(a.sat, w, px + rx[q] * sc, py + ry[q] * sc, 2 * sc, &dx, &dy);
            dx = __fmul_rn(dx, g[q]); dy = __fmul_rn(dy, g[q]);
            sdx[q] = dx; sdy[q] = dy;
            ang[q] = atan2((double)dy, (double)dx);
        }
        __syncthreads();
        if (lane < n_win) {
            const double ws = a.tab->win_start[lane], we = a.tab->win_end[lane];
            double sum_dx = 0.0, sum_dy = 0.0;
            for (int q = 0; q < SURF_SAMPLES; ++q) {
                const double d = ang[q], dp = d + two_pi, dm = d - two_pi;
                if ((d > ws && d < we) || (dp > ws && dp < we) || (dm > ws && dm < we)) { sum_dx += (double)sdx[q]; sum_dy += (double)sdy[q]; }
            }
            wsx[lane] = sum_dx; wsy[lane] = sum_dy;
        }
        __syncthreads();
        if (lane == 0) {
            double best_dx = 0.0, best_dy = 0.0, best_length = 0.0;
            for (int k = 0; k < n_win; ++k) {
                const double length = wsx[k] * wsx[k] + wsy[k] * wsy[k];
                if (length > best_length) { best_dx = wsx[k]; best_dy = wsy[k]; best_length = length; }
            }
            a.ori[i] = (float)atan2(best_dy, best_dx);
            a.stage[i] = 1;
        }
    }
}

__device__ __forceinline__ float surf_round(float x) { return x > 0.0f ? floorf(x + 0.5f) : ceilf(x - 0.5f); }

/* block 64 (one wavefront), the keypoints strided over the grid.  The 400 samples go over the lanes (seven rounds); their two
 * weighted responses wait in LDS.  Then lane 4 b + c adds value c of bin b over the bin's 25 samples in the reference's order
 * (y outer, x inner) in f32, and every lane adds the 64 squares in index order.  LDS: 3.4 KiB. */
__global__ __launch_bounds__(64) void k_surf_describe(SurfArgs a) {
    __shared__ float pdx[400], pdy[400], val[64];
    const int lane = threadIdx.x, w = a.w, h = a.h;
    const int n = min(a.counts->n_kp, a.kp_cap);
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const SurfKeypoint kp = a.kp[i];
        const int sc = (int)surf_scale(a.tab, kp);
        const float spacing = (float)(15 * sc + 1);
        const bool inside = !(kp.x < spacing || kp.y < spacing || kp.x + spacing >= (float)w || kp.y + spacing > (float)h);
        if (a.stage[i] != 1 || !inside) {
            if (lane == 0) { a.stage[i] = 0; a.slot[i] = 0; }
            continue;
        }
        const float orientation = a.ori[i];
        float sin_ori = 0.0f, cos_ori = 1.0f;
        /* sinf / cosf as the f64 value rounded once: the correctly rounded result, which is what the host's libm returns */
        if (!a.upright) { sin_ori = (float)sin((double)orientation); cos_ori = (float)cos((double)orientation); }
        __syncthreads();
        for (int q = lane; q < 400; q += 64) {
            const int iy = q / 20 - 10, ix = q % 20 - 10;
            const float xf = (float)ix + 0.5f, yf = (float)iy + 0.5f;
            int rot_x = (int)surf_round(kp.x + (cos_ori * xf - sin_ori * yf) * (float)sc);
            int rot_y = (int)surf_round(kp.y + (sin_ori * xf + cos_ori * yf) * (float)sc);
            /* inside by the window test above (15 sc + 1 against 9.5 sqrt(2) sc + 0.5 + sc + 1); the clamp changes no such value */
            rot_x = clampi(rot_x, sc + 1, w - 1 - sc); rot_y = clampi(rot_y, sc + 1, h - 1 - sc);
            float dx, dy;
            surf_haar(a.sat, w, rot_x, rot_y, sc, &dx, &dy);
            const float ori_dx = cos_ori * dx + sin_ori * dy, ori_dy = -sin_ori * dx + cos_ori * dy;
            const float weight = a.tab->weight[ix * ix + iy * iy];
            pdx[q] = weight * ori_dx; pdy[q] = weight * ori_dy;
        }
        __syncthreads();
        const int bin = lane >> 2, c = lane & 3, by = bin >> 2, bx = bin & 3;
        float sum = 0.0f;
        for (int yy = 0; yy < 5; ++yy)
            for (int xx = 0; xx < 5; ++xx) {
                const int q = (by * 5 + yy) * 20 + bx * 5 + xx;
                const float v = (c & 1) ? pdy[q] : pdx[q];
                sum += (c & 2) ? fabsf(v) : v;                       /* weight > 0: weight * |d| = |weight * d| */
            }
        val[lane] = sum;
        __syncthreads();
        float norm = 0.0f;
        for (int j = 0; j < 64; ++j) norm = norm + val[j] * val[j];
        const bool good = !((double)norm <= 1e-8);
        if (good) a.tmp_desc[(size_t)i * 64 + lane] = __fdiv_rn(sum, __fsqrt_rn(norm));
        if (lane == 0) { a.stage[i] = good ? 2 : 0; a.slot[i] = good ? 1 : 0; }
    }
}

/* block 64, the keypoints strided over the grid: slot[i] is the place of keypoint i's descriptor now */
__global__ __launch_bounds__(64) void k_surf_compact(SurfArgs a) {
    const int lane = threadIdx.x;
    const int n = min(a.counts->n_kp, a.kp_cap);
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        if (a.stage[i] != 2) continue;
        const size_t d = (size_t)a.slot[i];
        a.desc[d * 64 + lane] = a.tmp_desc[(size_t)i * 64 + lane];
        if (lane == 0) {
            const SurfKeypoint kp = a.kp[i];
            a.xyso[d * 4 + 0] = kp.x; a.xyso[d * 4 + 1] = kp.y; a.xyso[d * 4 + 2] = surf_scale(a.tab, kp); a.xyso[d * 4 + 3] = a.ori[i];
        }
    }
}

}  /* namespace */

void mi_surf_sat(hipStream_t s, const SurfArgs& a) {
    hipLaunchKernelGGL(k_surf_rows, dim3((unsigned)a.h), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_surf_cols, dim3((unsigned)((a.w + SURF_COL_TILE - 1) / SURF_COL_TILE)), dim3(64, 4), 0, s, a);
}

void mi_surf_responses(hipStream_t s, const SurfArgs& a) {
    hipLaunchKernelGGL(k_surf_response0, dim3((unsigned)((a.w + SURF_R0_TW - 1) / SURF_R0_TW), (unsigned)((a.h + SURF_R0_TH - 1) / SURF_R0_TH)),
                       dim3(64, 4), 0, s, a);
    hipLaunchKernelGGL(k_surf_response, dim3((unsigned)((a.ow[1] + 63) / 64), (unsigned)((a.oh[1] + 3) / 4), 3u), dim3(64, 4), 0, s, a);
}

void mi_surf_detect(hipStream_t s, const SurfArgs& a) {
    for (int pass = 0; pass < 2; ++pass) {
        for (int o = 0; o < 4; ++o) {
            const dim3 grid((unsigned)((a.ow[o] + 63) / 64), (unsigned)((a.oh[o] + 3) / 4), 2u);
            if (pass == 0) hipLaunchKernelGGL(k_surf_detect<false>, grid, dim3(64, 4), 0, s, a, o);
            else hipLaunchKernelGGL(k_surf_detect<true>, grid, dim3(64, 4), 0, s, a, o);
        }
        if (pass == 0) hipLaunchKernelGGL(k_surf_scan, dim3(1), dim3(1024), 0, s, a.words, a.n_words, (const int32_t*)nullptr, &a.counts->n_kp);
    }
}

void mi_surf_describe(hipStream_t s, const SurfArgs& a) {
    const unsigned waves = (unsigned)(a.kp_cap < 8192 ? a.kp_cap : 8192);
    hipLaunchKernelGGL(k_surf_orient, dim3(waves), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_surf_describe, dim3(waves), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_surf_scan, dim3(1), dim3(1024), 0, s, a.slot, a.kp_cap, (const int32_t*)&a.counts->n_kp, &a.counts->n_desc);
    hipLaunchKernelGGL(k_surf_compact, dim3(waves), dim3(64), 0, s, a);
}
