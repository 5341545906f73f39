/*
 * ransac_device.hip -- the three RANSAC loops of apps/sfmrecon on gfx950, for many jobs and all their iterations at once:
 *   F    sfm::RansacFundamental::estimate (libs/sfm/ransac_fundamental.cc:26-105) through fundamental_8_point,
 *        enforce_fundamental_constraints and sampson_distance (libs/sfm/fundamental.cc:77-126, :224-247),
 *   H    sfm::RansacHomography::estimate (libs/sfm/ransac_homography.cc:27-98) through homography_dlt and
 *        symmetric_transfer_error (libs/sfm/homography.cc:20-88),
 *   P3P  sfm::RansacPoseP3P::estimate (libs/sfm/ransac_pose_p3p.cc:26-122) through pose_p3p_kneip (libs/sfm/pose_p3p.cc).
 * All arithmetic is f64.
 *
 * Three kernels on one stream:
 *   k_ransac_f8     hypothesis -> F.  Sixteen lanes per hypothesis, four hypotheses per wavefront.  Lane c < 9 of a group
 *                   owns column c of the 8 x 9 system and column c of V; the SVD is a one-sided (Hestenes) Jacobi iteration
 *                   whose partner column comes across the lanes of the group.  Registers only.
 *   k_ransac_h4     hypothesis -> H, H^-1.  The same lanes and the same Jacobi on the 8 x 9 DLT system of four matches; the
 *                   inverse once per hypothesis (the reference inverts once per match).
 *   k_ransac_p3p    iteration -> four poses.  Four lanes per iteration: each computes Kneip's shared part, lane r the
 *                   back-substitution of root r.
 *   k_ransac_count  (hypothesis, entry) -> inlier counts, one instantiation per model.  One lane holds one hypothesis (F in
 *                   18 VGPRs, H and H^-1 in 36, P in 24), a workgroup walks a chunk of list entries staged once in LDS; every
 *                   lane reads the same address (a broadcast).  The count stays in a register and leaves with one integer
 *                   atomic per lane and chunk: sums of integers, any order.
 *   k_ransac_pick   job -> winner, one instantiation per model.  First strict maximum above inliers_to_beat, then the
 *                   winner's inliers once more over the list in index order, compacted ascending.
 *
 * Every product and sum of an inlier test is an explicit fma (sampson_inlier, transfer_inlier, reprojection_inlier), so
 * k_ransac_count and k_ransac_pick cannot be contracted differently: the winner's list has exactly as many entries as its
 * count said.
 *
 * No matrix instruction: the numerators of a (hypothesis x match) tile are a K = 9 product, but the f64 MFMA issues no
 * more multiply-adds per clock than the f64 vector unit, and its operand layout would cost shuffles.  The
 * tiles of H and P3P are K = 3 and K = 4 products per output, shorter still, so the same holds for them.
 */
#include <hip/hip_runtime.h>

#include "ransac_device.h"

typedef unsigned long long u64;

namespace {

__device__ __forceinline__ int find_by_block(const RansacJobDev* jobs, int n_jobs, int block) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block0 <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int find_by_hyp(const RansacJobDev* jobs, int n_jobs, int hyp) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].hyp0 <= hyp) lo = mid; else hi = mid - 1;
    }
    return lo;
}

/* sampson_distance(F, m) < threshold^2 (fundamental.cc:224-247) as  numerator < threshold^2 * denominator: no division,
 * and a zero denominator says "no" in both forms.  thr2 < 0 (a hypothesis that is not finite) says "no" to everything. */
__device__ __forceinline__ bool sampson_inlier(const double (&F)[9], double thr2, double x1, double y1, double x2, double y2) {
    const double l0 = fma(x1, F[0], fma(y1, F[1], F[2]));
    const double l1 = fma(x1, F[3], fma(y1, F[4], F[5]));
    const double l2 = fma(x1, F[6], fma(y1, F[7], F[8]));
    const double e = fma(x2, l0, fma(y2, l1, l2));
    const double r0 = fma(x2, F[0], fma(y2, F[3], F[6]));
    const double r1 = fma(x2, F[1], fma(y2, F[4], F[7]));
    const double sum = fma(l0, l0, fma(l1, l1, fma(r0, r0, r1 * r1)));
    return e * e < thr2 * sum;
}

/* symmetric_transfer_error(H, m) < threshold^2 (homography.cc:65-88) without a division: with a = H^-1 p2 and b = H p1,
 * 0.5 * (|a.xy / a.z - p1|^2 + |b.xy / b.z - p2|^2) < thr2  times  a.z^2 b.z^2.  A zero a.z or b.z says "no" in both forms.
 * G holds H, then H^-1. */
__device__ __forceinline__ bool transfer_inlier(const double (&G)[18], double thr2, double x1, double y1, double x2, double y2) {
    const double ax = fma(G[9], x2, fma(G[10], y2, G[11]));
    const double ay = fma(G[12], x2, fma(G[13], y2, G[14]));
    const double az = fma(G[15], x2, fma(G[16], y2, G[17]));
    const double bx = fma(G[0], x1, fma(G[1], y1, G[2]));
    const double by = fma(G[3], x1, fma(G[4], y1, G[5]));
    const double bz = fma(G[6], x1, fma(G[7], y1, G[8]));
    const double d1x = fma(-x1, az, ax), d1y = fma(-y1, az, ay);
    const double d2x = fma(-x2, bz, bx), d2y = fma(-y2, bz, by);
    const double n1 = fma(d1x, d1x, d1y * d1y), n2 = fma(d2x, d2x, d2y * d2y);
    const double az2 = az * az, bz2 = bz * bz;
    return 0.5 * fma(n1, bz2, n2 * az2) < thr2 * (az2 * bz2);
}

/* One 2D-3D correspondence on the device: 48 bytes, so that LDS and global reads are aligned 16-byte words. */
struct __align__(16) RansacCorr { double x, y, z, u, v, pad; };

/* find_inliers (ransac_pose_p3p.cc:106-122) without a division: with p = P (X, 1),
 * |p.xy / p.z - uv|^2 < thr2  times  p.z^2.  No test on the sign of p.z: the reference has none. */
__device__ __forceinline__ bool reprojection_inlier(const double (&P)[12], double thr2, const RansacCorr& e) {
    const double px = fma(P[0], e.x, fma(P[1], e.y, fma(P[2], e.z, P[3])));
    const double py = fma(P[4], e.x, fma(P[5], e.y, fma(P[6], e.z, P[7])));
    const double pz = fma(P[8], e.x, fma(P[9], e.y, fma(P[10], e.z, P[11])));
    const double dx = fma(-e.u, pz, px), dy = fma(-e.v, pz, py);
    return fma(dx, dx, dy * dy) < thr2 * (pz * pz);
}

/* thr2 for a finite hypothesis, -1 otherwise */
template <int N>
__device__ __forceinline__ double guard_threshold(const double (&F)[N], double thr2) {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < N; ++k) finite = finite && isfinite(F[k]);
    return finite ? thr2 : -1.0;
}

/* What k_ransac_count and k_ransac_pick need to know of a model: HYP doubles per hypothesis of which the first REG go into
 * registers and are guarded; the list entry as it lies in LDS; BEST doubles from offset BEST_OFF are the winner's output. */
struct ModelF {
    typedef double4 Entry;
    static constexpr int HYP = RANSAC_F_HYP, REG = 9, BEST = 9, BEST_OFF = 0;
    static __device__ __forceinline__ bool inlier(const double (&F)[9], double thr2, const double4& m) {
        return sampson_inlier(F, thr2, m.x, m.y, m.z, m.w);
    }
};
struct ModelH {
    typedef double4 Entry;
    static constexpr int HYP = RANSAC_H_HYP, REG = 18, BEST = 9, BEST_OFF = 0;
    static __device__ __forceinline__ bool inlier(const double (&G)[18], double thr2, const double4& m) {
        return transfer_inlier(G, thr2, m.x, m.y, m.z, m.w);
    }
};
struct ModelP3P {
    typedef RansacCorr Entry;
    static constexpr int HYP = RANSAC_P3P_HYP, REG = 12, BEST = 12, BEST_OFF = 12;
    static __device__ __forceinline__ bool inlier(const double (&P)[12], double thr2, const RansacCorr& e) {
        return reprojection_inlier(P, thr2, e);
    }
};

/* The index, among the first n lanes of a 16-lane group, of the lane with the smallest x (the lowest lane on a tie); the
 * same answer in every lane of the group. */
__device__ __forceinline__ int group_argmin(int c, int n, double x) {
    double best = c < n ? x : INFINITY;
    int bi = c;
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
        const double o = __shfl_xor(best, m, 16);
        const int oi = __shfl_xor(bi, m, 16);
        if (o < best || (o == best && oi < bi)) { best = o; bi = oi; }
    }
    return __shfl(bi, 0, 16);
}

/* One-sided Jacobi on the N columns (N odd, M rows) that lanes c < N of each 16-lane group hold: `a` becomes U * Sigma,
 * column by column, and `v` the matching column of V.  Round-robin pairing: in step s column c meets column (s - c) mod N
 * and the column with 2c = s (mod N) rests, so a step is (N - 1) / 2 disjoint pairs and N steps are a sweep.  Both lanes
 * of a pair compute the same rotation from the same numbers in the same order, and each applies it to its own column.
 * A pair rotates while its columns are not orthogonal to 1e-15 of their norms AND the rotation is larger than 1e-14: a
 * column that has become rounding noise (the system has rank 8) keeps a random angle to every other, and rotations of that
 * size no longer move V.  Returns false for a group that still rotated in sweep RANSAC_MAX_SWEEPS. */
template <int M, int N>
__device__ __forceinline__ bool jacobi(int c, int group, double (&a)[M], double (&v)[N]) {
    u64 rotated_mask = 0;
    for (int sweep = 0; sweep < RANSAC_MAX_SWEEPS; ++sweep) {
        bool rotated = false;
        for (int step = 0; step < N; ++step) {
            int partner = c;
            if (c < N) { partner = step - c; if (partner < 0) partner += N; }
            double b[M], w[N];
#pragma unroll
            for (int i = 0; i < M; ++i) b[i] = __shfl(a[i], partner, 16);
#pragma unroll
            for (int i = 0; i < N; ++i) w[i] = __shfl(v[i], partner, 16);
            double own = 0.0, other = 0.0, g = 0.0;
#pragma unroll
            for (int i = 0; i < M; ++i) {
                own = fma(a[i], a[i], own);
                other = fma(b[i], b[i], other);
                g = fma(a[i], b[i], g);
            }
            if (partner != c && g * g > 1e-30 * (own * other)) {
                const bool low = c < partner;                   /* this lane holds the pair's lower column */
                const double alpha = low ? own : other, beta = low ? other : own;
                const double zeta = (beta - alpha) / (2.0 * g);
                const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
                if (fabs(t) > 1e-14) {
                    const double cs = 1.0 / sqrt(fma(t, t, 1.0));
                    const double sn = low ? -(cs * t) : cs * t;
#pragma unroll
                    for (int i = 0; i < M; ++i) a[i] = fma(sn, b[i], cs * a[i]);
#pragma unroll
                    for (int i = 0; i < N; ++i) v[i] = fma(sn, w[i], cs * v[i]);
                    rotated = true;
                }
            }
        }
        rotated_mask = __ballot(rotated);
        if (rotated_mask == 0) break;                           /* (a group that is done earlier rotates no more) */
    }
    return ((rotated_mask >> (16 * group)) & 0xFFFFull) == 0;
}

/* 256 threads: 16 hypotheses */
__global__ __launch_bounds__(256) void k_ransac_f8(RansacBuffers B, int n_jobs, int n_hyp) {
    const int lane = threadIdx.x & 63;
    const int c = lane & 15, group = lane >> 4;
    const int h = (int)blockIdx.x * 16 + ((int)threadIdx.x >> 4);
    const int hc = min(h, n_hyp - 1);
    const RansacJobDev jb = B.jobs[find_by_hyp(B.jobs, n_jobs, hc)];

    /* column c of the system (fundamental.cc:84-98): row i is (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1) of sample i */
    double a[8], v[9];
    const int32_t* row = B.samples + (size_t)hc * 8;
    const int c3 = c / 3, cm = c - 3 * c3;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double* m = B.list + (size_t)(jb.match0 + row[i]) * 4;
        const double x1 = m[0], y1 = m[1], x2 = m[2], y2 = m[3];
        const double left = c3 == 0 ? x2 : c3 == 1 ? y2 : 1.0;
        const double right = cm == 0 ? x1 : cm == 1 ? y1 : 1.0;
        a[i] = c < 9 ? left * right : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) v[i] = i == c ? 1.0 : 0.0;
    bool converged = jacobi<8, 9>(c, group, a, v);

    /* the null vector: V's column of the smallest column */
    double norm = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) norm = fma(a[i], a[i], norm);
    const int null_lane = group_argmin(c, 9, norm);
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = __shfl(v[k], null_lane, 16);

    /* rank 2 (fundamental.cc:112-126): the same iteration on the three columns of F, then F = sum over the two larger
     * columns of (U Sigma)_c V_c^T */
    double a3[3], v3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a3[i] = c == 0 ? f[3 * i] : c == 1 ? f[3 * i + 1] : c == 2 ? f[3 * i + 2] : 0.0;
        v3[i] = i == c ? 1.0 : 0.0;
    }
    converged = jacobi<3, 3>(c, group, a3, v3) && converged;
    const double norm3 = fma(a3[0], a3[0], fma(a3[1], a3[1], a3[2] * a3[2]));
    const int drop = group_argmin(c, 3, norm3);
    const bool keep = c < 3 && c != drop;
    double F[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double p = keep ? a3[i] * v3[j] : 0.0;
            F[3 * i + j] = (__shfl(p, 0, 16) + __shfl(p, 1, 16)) + __shfl(p, 2, 16);
        }

    if (c == 0 && h < n_hyp) {
        double* out = B.hyp_all + (size_t)h * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = F[k];
        B.counts[h] = 0;
        if (!converged) atomicAdd(B.capped, 1ull);
    }
}

/* 256 threads: 16 hypotheses.  Column c of the DLT system (homography.cc:26-51): rows i and i + 4 belong to sample i,
 *   row i      0 0 0   x1 y1 1   -x1 y2  -y1 y2  -y2
 *   row i + 4  -x1 -y1 -1   0 0 0   x1 x2  y1 x2  x2 */
__global__ __launch_bounds__(256) void k_ransac_h4(RansacBuffers B, int n_jobs, int n_hyp) {
    const int lane = threadIdx.x & 63;
    const int c = lane & 15, group = lane >> 4;
    const int h = (int)blockIdx.x * 16 + ((int)threadIdx.x >> 4);
    const int hc = min(h, n_hyp - 1);
    const RansacJobDev* jb = B.jobs + find_by_hyp(B.jobs, n_jobs, hc);
    const int64_t match0 = jb->match0;

    double a[8], v[9];
    const int32_t* row = B.samples + (size_t)hc * 4;
    const int c3 = c / 3, cm = c - 3 * c3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double* m = B.list + (size_t)(match0 + row[i]) * 4;
        const double x1 = m[0], y1 = m[1], x2 = m[2], y2 = m[3];
        const double base = cm == 0 ? x1 : cm == 1 ? y1 : 1.0;
        a[i] = c3 == 1 ? base : c3 == 2 ? -base * y2 : 0.0;
        a[i + 4] = c3 == 0 ? -base : c3 == 2 ? base * x2 : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) v[i] = i == c ? 1.0 : 0.0;
    const bool converged = jacobi<8, 9>(c, group, a, v);

    double norm = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) norm = fma(a[i], a[i], norm);
    const int null_lane = group_argmin(c, 9, norm);
    double H[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = __shfl(v[k], null_lane, 16);
    const double last = H[8];                                   /* ransac_homography.cc:82 */
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] /= last;

    /* H^-1 = adjugate / determinant */
    double I[9];
    I[0] = H[4] * H[8] - H[5] * H[7]; I[1] = H[2] * H[7] - H[1] * H[8]; I[2] = H[1] * H[5] - H[2] * H[4];
    I[3] = H[5] * H[6] - H[3] * H[8]; I[4] = H[0] * H[8] - H[2] * H[6]; I[5] = H[2] * H[3] - H[0] * H[5];
    I[6] = H[3] * H[7] - H[4] * H[6]; I[7] = H[1] * H[6] - H[0] * H[7]; I[8] = H[0] * H[4] - H[1] * H[3];
    const double det = H[0] * I[0] + H[1] * I[3] + H[2] * I[6];

    if (c == 0 && h < n_hyp) {
        double* out = B.hyp_all + (size_t)h * RANSAC_H_HYP;
#pragma unroll
        for (int k = 0; k < 9; ++k) { out[k] = H[k]; out[9 + k] = I[k] / det; }
        B.counts[h] = 0;
        if (!converged) atomicAdd(B.capped, 1ull);
    }
}

struct V3 { double x, y, z; };
struct C2 { double re, im; };
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 normalized(V3 a) { const double n = sqrt(dot(a, a)); return {a.x / n, a.y / n, a.z / n}; }
__device__ __forceinline__ V3 mul(const double (&M)[9], V3 a) {
    return {M[0] * a.x + M[1] * a.y + M[2] * a.z, M[3] * a.x + M[4] * a.y + M[5] * a.z, M[6] * a.x + M[7] * a.y + M[8] * a.z};
}
/* the direction of an image point, to unit length unless it has it already (pose_p3p.cc:87-94) */
__device__ __forceinline__ V3 direction(const double (&k_inv)[9], double u, double v) {
    const V3 f = mul(k_inv, V3{u, v, 1.0});
    const double n = dot(f, f);
    return (1.0 - 1e-10 <= n && n <= 1.0 + 1e-10) ? f : normalized(f);
}
/* principal square root */
__device__ __forceinline__ C2 complex_sqrt(C2 z) {
    const double m = hypot(z.re, z.im);
    if (m == 0.0) return {0.0, 0.0};
    if (z.re >= 0.0) { const double re = sqrt(0.5 * (m + z.re)); return {re, z.im / (2.0 * re)}; }
    const double im = sqrt(0.5 * (m - z.re));
    return {fabs(z.im) / (2.0 * im), copysign(im, z.im)};
}
/* principal cube root: std::pow(z, 1.0 / 3.0) */
__device__ __forceinline__ C2 complex_cbrt(C2 z) {
    const double r = cbrt(hypot(z.re, z.im)), t = atan2(z.im, z.re) / 3.0;
    return {r * cos(t), r * sin(t)};
}

/* 256 threads: 64 iterations, four lanes each.  pose_p3p_kneip (pose_p3p.cc:74-236) with solve_quartic_roots (:21-70)
 * written out in real pairs; lane r keeps the real part of root r and substitutes it back. */
__global__ __launch_bounds__(256) void k_ransac_p3p(RansacBuffers B, int n_jobs, int n_it) {
    const int g = (int)blockIdx.x * 64 + ((int)threadIdx.x >> 2), r = (int)threadIdx.x & 3;
    const int gc = min(g, n_it - 1);
    const RansacJobDev* jb = B.jobs + find_by_hyp(B.jobs, n_jobs, 4 * gc);
    const int64_t match0 = jb->match0;
    double K[9], K_inv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { K[k] = jb->k[k]; K_inv[k] = jb->k_inv[k]; }

    const int32_t* row = B.samples + (size_t)gc * 3;
    const RansacCorr* list = (const RansacCorr*)B.list + match0;
    const RansacCorr c1 = list[row[0]], c2 = list[row[1]], c3 = list[row[2]];
    V3 p1 = {c1.x, c1.y, c1.z}, p2 = {c2.x, c2.y, c2.z}, p3 = {c3.x, c3.y, c3.z};
    V3 f1 = direction(K_inv, c1.u, c1.v), f2 = direction(K_inv, c2.u, c2.v), f3 = direction(K_inv, c3.u, c3.v);

    const V3 n12 = cross(sub(p2, p1), sub(p3, p1));
    const bool collinear = dot(n12, n12) < 1e-10;                /* :80-85: no solution */

    /* the camera frame, with the first two points swapped if the third then looks along +z (:96-120) */
    V3 e1 = f1, e3 = normalized(cross(f1, f2)), e2 = cross(e3, e1);
    if (dot(e3, f3) > 0.0) {
        const V3 tp = p1; p1 = p2; p2 = tp;
        const V3 tf = f1; f1 = f2; f2 = tf;
        e1 = f1; e3 = normalized(cross(f1, f2)); e2 = cross(e3, e1);
    }
    f3 = V3{dot(e1, f3), dot(e2, f3), dot(e3, f3)};

    /* the world frame (:122-132) */
    const V3 n1 = normalized(sub(p2, p1));
    const V3 n3 = normalized(cross(n1, sub(p3, p1)));
    const V3 n2 = cross(n3, n1);
    const V3 q3 = sub(p3, p1);
    p3 = V3{dot(n1, q3), dot(n2, q3), dot(n3, q3)};

    const V3 d = sub(p2, p1);
    const double d_12 = sqrt(dot(d, d));
    const double f_1 = f3.x / f3.z, f_2 = f3.y / f3.z, p_1 = p3.x, p_2 = p3.y;
    const double cos_beta = dot(f1, f2);
    double b = 1.0 / (1.0 - cos_beta * cos_beta) - 1.0;
    b = cos_beta < 0.0 ? -sqrt(b) : sqrt(b);

    const double f_1_pw2 = f_1 * f_1, f_2_pw2 = f_2 * f_2;
    const double p_1_pw2 = p_1 * p_1, p_1_pw3 = p_1_pw2 * p_1, p_1_pw4 = p_1_pw3 * p_1;
    const double p_2_pw2 = p_2 * p_2, p_2_pw3 = p_2_pw2 * p_2, p_2_pw4 = p_2_pw3 * p_2;
    const double d_12_pw2 = d_12 * d_12, b_pw2 = b * b;

    /* the five factors of the quartic (:161-194) */
    const double A = -f_2_pw2 * p_2_pw4 - p_2_pw4 * f_1_pw2 - p_2_pw4;
    const double Bq = 2.0 * p_2_pw3 * d_12 * b + 2.0 * f_2_pw2 * p_2_pw3 * d_12 * b - 2.0 * f_2 * p_2_pw3 * f_1 * d_12;
    const double Cq = -f_2_pw2 * p_2_pw2 * p_1_pw2 - f_2_pw2 * p_2_pw2 * d_12_pw2 * b_pw2 - f_2_pw2 * p_2_pw2 * d_12_pw2
        + f_2_pw2 * p_2_pw4 + p_2_pw4 * f_1_pw2 + 2.0 * p_1 * p_2_pw2 * d_12 + 2.0 * f_1 * f_2 * p_1 * p_2_pw2 * d_12 * b
        - p_2_pw2 * p_1_pw2 * f_1_pw2 + 2.0 * p_1 * p_2_pw2 * f_2_pw2 * d_12 - p_2_pw2 * d_12_pw2 * b_pw2
        - 2.0 * p_1_pw2 * p_2_pw2;
    const double Dq = 2.0 * p_1_pw2 * p_2 * d_12 * b + 2.0 * f_2 * p_2_pw3 * f_1 * d_12 - 2.0 * f_2_pw2 * p_2_pw3 * d_12 * b
        - 2.0 * p_1 * p_2 * d_12_pw2 * b;
    const double Eq = -2.0 * f_2 * p_2_pw2 * f_1 * p_1 * d_12 * b + f_2_pw2 * p_2_pw2 * d_12_pw2 + 2.0 * p_1_pw3 * d_12
        - p_1_pw2 * d_12_pw2 + f_2_pw2 * p_2_pw2 * p_1_pw2 - p_1_pw4 - 2.0 * f_2_pw2 * p_2_pw2 * p_1 * d_12
        + p_2_pw2 * f_1_pw2 * p_1_pw2 + f_2_pw2 * p_2_pw2 * d_12_pw2 * b_pw2;

    /* Ferrari (:24-60).  P and Q are real; R, U, y, w and part3 are not in general. */
    const double A2 = A * A, B2 = Bq * Bq, A3 = A2 * A, B3 = B2 * Bq, A4 = A3 * A, B4 = B3 * Bq;
    const double alpha = -3.0 * B2 / (8.0 * A2) + Cq / A;
    const double beta = B3 / (8.0 * A3) - Bq * Cq / (2.0 * A2) + Dq / A;
    const double gamma = -3.0 * B4 / (256.0 * A4) + B2 * Cq / (16.0 * A3) - Bq * Dq / (4.0 * A2) + Eq / A;
    const double alpha2 = alpha * alpha, alpha3 = alpha2 * alpha;
    const double P = -alpha2 / 12.0 - gamma;
    const double Q = -alpha3 / 108.0 + alpha * gamma / 3.0 - beta * beta / 8.0;
    const C2 root_d = complex_sqrt(C2{Q * Q / 4.0 + P * P * P / 27.0, 0.0});
    const C2 U = complex_cbrt(C2{-Q / 2.0 + root_d.re, root_d.im});
    C2 y;
    if (U.re == 0.0) {
        const C2 q = complex_cbrt(C2{Q, 0.0});
        y = C2{-5.0 * alpha / 6.0 - q.re, -q.im};
    } else {
        const double dr = 3.0 * U.re, di = 3.0 * U.im, den = dr * dr + di * di;   /* P / (3 U) */
        y = C2{-5.0 * alpha / 6.0 - P * dr / den + U.re, P * di / den + U.im};
    }
    const C2 w = complex_sqrt(C2{alpha + 2.0 * y.re, 2.0 * y.im});
    const double part1 = -Bq / (4.0 * A);
    const C2 part2 = {3.0 * alpha + 2.0 * y.re, 2.0 * y.im};
    const double wn = w.re * w.re + w.im * w.im;
    const C2 part3 = {2.0 * beta * w.re / wn, -2.0 * beta * w.im / wn};

    /* root r (:63-66): + + / + - / - + / - -, the real part */
    const double sw = r < 2 ? 1.0 : -1.0, ss = (r & 1) ? -1.0 : 1.0;
    const C2 s = complex_sqrt(C2{-(part2.re + sw * part3.re), -(part2.im + sw * part3.im)});
    const double root = part1 + 0.5 * (sw * w.re + ss * s.re);

    /* back-substitution (:203-235); a root outside [-1, 1] makes sin_theta, and with it the pose, NaN */
    const double cot_alpha = (-f_1 * p_1 / f_2 - root * p_2 + d_12 * b) / (-f_1 * root * p_2 / f_2 + p_1 - d_12);
    const double cos_theta = root, sin_theta = sqrt(1.0 - root * root);
    const double sin_alpha = sqrt(1.0 / (cot_alpha * cot_alpha + 1.0));
    double cos_alpha = sqrt(1.0 - sin_alpha * sin_alpha);
    if (cot_alpha < 0.0) cos_alpha = -cos_alpha;
    const double reach = sin_alpha * b + cos_alpha;
    const V3 Cn = {d_12 * cos_alpha * reach, cos_theta * d_12 * sin_alpha * reach, sin_theta * d_12 * sin_alpha * reach};
    const V3 Cw = {p1.x + (n1.x * Cn.x + n2.x * Cn.y + n3.x * Cn.z), p1.y + (n1.y * Cn.x + n2.y * Cn.y + n3.y * Cn.z),
                   p1.z + (n1.z * Cn.x + n2.z * Cn.y + n3.z * Cn.z)};
    const double Rm[9] = {-cos_alpha, -sin_alpha * cos_theta, -sin_alpha * sin_theta,
                          sin_alpha, -cos_alpha * cos_theta, -cos_alpha * sin_theta,
                          0.0, -sin_theta, cos_theta};
    /* the pose's rotation (N^T Rm^T T)^T = T^T (Rm N), and t = -R C */
    const double N[9] = {n1.x, n1.y, n1.z, n2.x, n2.y, n2.z, n3.x, n3.y, n3.z};
    const double T[9] = {e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, e3.x, e3.y, e3.z};
    double M[9], pose[12];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * i + j] = Rm[3 * i] * N[j] + Rm[3 * i + 1] * N[3 + j] + Rm[3 * i + 2] * N[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) pose[4 * i + j] = T[i] * M[j] + T[3 + i] * M[3 + j] + T[6 + i] * M[6 + j];
        pose[4 * i + 3] = -(pose[4 * i] * Cw.x + pose[4 * i + 1] * Cw.y + pose[4 * i + 2] * Cw.z);
    }

    if (g < n_it) {
        const int h = 4 * g + r;
        double* out = B.hyp_all + (size_t)h * RANSAC_P3P_HYP;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double p = K[3 * i] * pose[j] + K[3 * i + 1] * pose[4 + j] + K[3 * i + 2] * pose[8 + j];
                out[4 * i + j] = collinear ? NAN : p;
                out[12 + 4 * i + j] = collinear ? NAN : pose[4 * i + j];
            }
        B.counts[h] = 0;
    }
}

/* RANSAC_TILE hypotheses of one job against one chunk of its list */
template <class M>
__global__ __launch_bounds__(RANSAC_TILE) void k_ransac_count(RansacBuffers B, int n_jobs) {
    typedef typename M::Entry Entry;
    __shared__ Entry chunk_lds[RANSAC_CHUNK];
    const RansacJobDev* jp = B.jobs + find_by_block(B.jobs, n_jobs, (int)blockIdx.x);
    const int block0 = jp->block0, chunks = jp->chunks, n_matches = jp->n_matches, n_hyp = jp->n_hyp, hyp0 = jp->hyp0;
    const int local = (int)blockIdx.x - block0;
    const int tile = local / chunks, chunk = local - tile * chunks;
    const int m0 = chunk * RANSAC_CHUNK;
    const int nm = min(RANSAC_CHUNK, n_matches - m0);
    const Entry* src = (const Entry*)B.list + jp->match0 + m0;
    for (int i = threadIdx.x; i < nm; i += RANSAC_TILE) chunk_lds[i] = src[i];

    const int it = tile * RANSAC_TILE + (int)threadIdx.x;
    const double* Fp = B.hyp_all + (size_t)(hyp0 + min(it, n_hyp - 1)) * M::HYP;
    double F[M::REG];
#pragma unroll
    for (int k = 0; k < M::REG; ++k) F[k] = Fp[k];
    const double thr2 = guard_threshold(F, jp->thr2);
    __syncthreads();

    int count = 0;
#pragma unroll 4
    for (int i = 0; i < nm; ++i) {
        const Entry m = chunk_lds[i];
        count += M::inlier(F, thr2, m) ? 1 : 0;
    }
    if (it < n_hyp && count > 0) atomicAdd(&B.counts[hyp0 + it], count);
}

/* One workgroup of 256 per job. */
template <class M>
__global__ __launch_bounds__(256) void k_ransac_pick(RansacBuffers B) {
    typedef typename M::Entry Entry;
    __shared__ u64 keys[256];
    __shared__ int wave_total[4];
    const RansacJobDev* jp = B.jobs + blockIdx.x;
    const int n_matches = jp->n_matches, n_hyp = jp->n_hyp, hyp0 = jp->hyp0, inliers_to_beat = jp->inliers_to_beat;
    const int64_t match0 = jp->match0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    /* the first hypothesis with the largest count: the maximum of  count << 32 | ~hypothesis */
    u64 key = 0;
    for (int it = tid; it < n_hyp; it += 256) {
        const u64 k = ((u64)(unsigned)B.counts[hyp0 + it] << 32) | (u64)(0xFFFFFFFFu - (unsigned)it);
        key = k > key ? k : key;
    }
    keys[tid] = key;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) keys[tid] = keys[tid] > keys[tid + s] ? keys[tid] : keys[tid + s];
        __syncthreads();
    }
    key = keys[0];
    const int best_count = (int)(key >> 32);
    const int best_it = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    if (best_count <= inliers_to_beat) {                        /* (the reference's `>`, ransac_fundamental.cc:43) */
        if (tid == 0) { B.best[2 * blockIdx.x] = -1; B.best[2 * blockIdx.x + 1] = 0; }
        return;
    }

    const double* Fp = B.hyp_all + (size_t)(hyp0 + best_it) * M::HYP;
    double F[M::REG];
#pragma unroll
    for (int k = 0; k < M::REG; ++k) F[k] = Fp[k];
    const double thr2 = guard_threshold(F, jp->thr2);
    const Entry* src = (const Entry*)B.list + match0;
    int32_t* out = B.inliers + match0;
    int written = 0;
    for (int base = 0; base < n_matches; base += 256) {
        const int m = base + tid;
        bool in = false;
        if (m < n_matches) {
            const Entry p = src[m];
            in = M::inlier(F, thr2, p);
        }
        const u64 mask = __ballot(in);
        if (lane == 0) wave_total[wave] = __popcll(mask);
        __syncthreads();
        int before = written;
        for (int w = 0; w < wave; ++w) before += wave_total[w];
        if (in) out[before + __popcll(mask & ((1ull << lane) - 1ull))] = m;
        written += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        __syncthreads();
    }
    if (tid == 0) { B.best[2 * blockIdx.x] = best_it; B.best[2 * blockIdx.x + 1] = written; }
    if (tid < M::BEST) B.best_model[(size_t)blockIdx.x * M::BEST + tid] = Fp[M::BEST_OFF + tid];
}

template <class M>
void count_and_pick(hipStream_t s, const RansacBuffers& b, int32_t n_jobs, int32_t n_blocks) {
    hipLaunchKernelGGL(k_ransac_count<M>, dim3((unsigned)n_blocks), dim3(RANSAC_TILE), 0, s, b, (int)n_jobs);
    hipLaunchKernelGGL(k_ransac_pick<M>, dim3((unsigned)n_jobs), dim3(256), 0, s, b);
}

}  /* namespace */

void mi_ransac_launch(hipStream_t s, RansacModel model, const RansacBuffers& b, int32_t n_jobs, int32_t n_hyp, int32_t n_blocks) {
    if (model == RANSAC_F) {
        hipLaunchKernelGGL(k_ransac_f8, dim3((unsigned)((n_hyp + 15) / 16)), dim3(256), 0, s, b, (int)n_jobs, (int)n_hyp);
        count_and_pick<ModelF>(s, b, n_jobs, n_blocks);
    } else if (model == RANSAC_H) {
        hipLaunchKernelGGL(k_ransac_h4, dim3((unsigned)((n_hyp + 15) / 16)), dim3(256), 0, s, b, (int)n_jobs, (int)n_hyp);
        count_and_pick<ModelH>(s, b, n_jobs, n_blocks);
    } else {
        const int n_it = n_hyp / 4;
        hipLaunchKernelGGL(k_ransac_p3p, dim3((unsigned)((n_it + 63) / 64)), dim3(256), 0, s, b, (int)n_jobs, n_it);
        count_and_pick<ModelP3P>(s, b, n_jobs, n_blocks);
    }
}
