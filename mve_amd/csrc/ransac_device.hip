/*
 * ransac_device.hip -- RANSAC for the fundamental matrix on gfx950: what sfm::RansacFundamental::estimate computes
 * (libs/sfm/ransac_fundamental.cc:26-105) through fundamental_8_point, enforce_fundamental_constraints and sampson_distance
 * (libs/sfm/fundamental.cc:77-126, :224-247), for many view pairs and all their iterations at once.  All arithmetic is f64.
 *
 * Three kernels on one stream:
 *   k_ransac_f8     hypothesis -> F.  Sixteen lanes per hypothesis, four hypotheses per wavefront.  Lane c < 9 of a group
 *                   owns column c of the 8 x 9 system and column c of V; the SVD is a one-sided (Hestenes) Jacobi iteration
 *                   whose partner column comes across the lanes of the group.  Registers only.
 *   k_ransac_count  (hypothesis, match) -> inlier counts.  One lane holds one hypothesis (F in 18 VGPRs), a workgroup walks a
 *                   chunk of matches staged once in LDS; every lane reads the same address (a broadcast).  The count stays
 *                   in a register and leaves with one integer atomic per lane and chunk: sums of integers, any order.
 *   k_ransac_pick   job -> winner.  First strict maximum above inliers_to_beat, then the winner's inliers once more over the
 *                   matches in index order, compacted ascending.
 *
 * Every product and sum of the Sampson test is an explicit fma (sampson_inlier), so k_ransac_count and k_ransac_pick
 * cannot be contracted differently: the winner's list has exactly as many entries as its count said.
 *
 * No matrix instruction: the numerators of a (hypothesis x match) tile are a K = 9 product, but the f64 MFMA issues no
 * more multiply-adds per clock than the f64 vector unit, and its operand layout would cost shuffles.
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

/* thr2 for finite F, -1 otherwise */
__device__ __forceinline__ double guard_threshold(const double (&F)[9], double thr2) {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) finite = finite && isfinite(F[k]);
    return finite ? thr2 : -1.0;
}

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
        const double* m = B.matches + (size_t)(jb.match0 + row[i]) * 4;
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
        double* out = B.F_all + (size_t)h * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = F[k];
        B.counts[h] = 0;
        if (!converged) atomicAdd(B.capped, 1ull);
    }
}

/* RANSAC_TILE hypotheses of one job against one chunk of its matches */
__global__ __launch_bounds__(RANSAC_TILE) void k_ransac_count(RansacBuffers B, int n_jobs) {
    __shared__ double4 chunk_lds[RANSAC_CHUNK];
    const RansacJobDev jb = B.jobs[find_by_block(B.jobs, n_jobs, (int)blockIdx.x)];
    const int local = (int)blockIdx.x - jb.block0;
    const int tile = local / jb.chunks, chunk = local - tile * jb.chunks;
    const int m0 = chunk * RANSAC_CHUNK;
    const int nm = min(RANSAC_CHUNK, jb.n_matches - m0);
    const double4* src = (const double4*)B.matches + jb.match0 + m0;
    for (int i = threadIdx.x; i < nm; i += RANSAC_TILE) chunk_lds[i] = src[i];

    const int it = tile * RANSAC_TILE + (int)threadIdx.x;
    const double* Fp = B.F_all + (size_t)(jb.hyp0 + min(it, jb.n_iterations - 1)) * 9;
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = Fp[k];
    const double thr2 = guard_threshold(F, jb.thr2);
    __syncthreads();

    int count = 0;
#pragma unroll 4
    for (int i = 0; i < nm; ++i) {
        const double4 m = chunk_lds[i];
        count += sampson_inlier(F, thr2, m.x, m.y, m.z, m.w) ? 1 : 0;
    }
    if (it < jb.n_iterations && count > 0) atomicAdd(&B.counts[jb.hyp0 + it], count);
}

/* One workgroup of 256 per job. */
__global__ __launch_bounds__(256) void k_ransac_pick(RansacBuffers B) {
    __shared__ u64 keys[256];
    __shared__ int wave_total[4];
    const RansacJobDev jb = B.jobs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    /* the first iteration with the largest count: the maximum of  count << 32 | ~iteration */
    u64 key = 0;
    for (int it = tid; it < jb.n_iterations; it += 256) {
        const u64 k = ((u64)(unsigned)B.counts[jb.hyp0 + it] << 32) | (u64)(0xFFFFFFFFu - (unsigned)it);
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
    if (best_count <= jb.inliers_to_beat) {                     /* (the reference's `>`, ransac_fundamental.cc:43) */
        if (tid == 0) { B.best[2 * blockIdx.x] = -1; B.best[2 * blockIdx.x + 1] = 0; }
        return;
    }

    const double* Fp = B.F_all + (size_t)(jb.hyp0 + best_it) * 9;
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = Fp[k];
    const double thr2 = guard_threshold(F, jb.thr2);
    const double4* src = (const double4*)B.matches + jb.match0;
    int32_t* out = B.inliers + jb.match0;
    int written = 0;
    for (int base = 0; base < jb.n_matches; base += 256) {
        const int m = base + tid;
        bool in = false;
        if (m < jb.n_matches) {
            const double4 p = src[m];
            in = sampson_inlier(F, thr2, p.x, p.y, p.z, p.w);
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
    if (tid < 9) B.F_best[(size_t)blockIdx.x * 9 + tid] = Fp[tid];
}

}  /* namespace */

void mi_ransac_launch(hipStream_t s, const RansacBuffers& b, int32_t n_jobs, int32_t n_hyp, int32_t n_blocks) {
    hipLaunchKernelGGL(k_ransac_f8, dim3((unsigned)((n_hyp + 15) / 16)), dim3(256), 0, s, b, (int)n_jobs, (int)n_hyp);
    hipLaunchKernelGGL(k_ransac_count, dim3((unsigned)n_blocks), dim3(RANSAC_TILE), 0, s, b, (int)n_jobs);
    hipLaunchKernelGGL(k_ransac_pick, dim3((unsigned)n_jobs), dim3(256), 0, s, b);
}
