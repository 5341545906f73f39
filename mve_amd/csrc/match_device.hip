/*
 * match_device.hip -- exhaustive SIFT / SURF descriptor matching for gfx950: what sfm::Matching::twoway_match computes
 * through sfm::NearestNeighbor<T>::find (libs/sfm/nearest_neighbor.cc:64-133, :218-272; libs/sfm/matching.h:114-159).
 *
 * The |A| x |B| matrix of inner products of a pair is computed ONCE and serves both directions: its row-wise top two are
 * A -> B, its column-wise top two B -> A (the reference computes the matrix twice).  Inner products are exact int32 from
 * v_mfma_i32_16x16x64_i8 on bytes; SIFT's unsigned bytes are stored biased by -128 and the product is restored through the
 * accumulator's initial value (MatchJobDev::off).
 *
 * The reference's loop (`>=` twice, j ascending, start (0, index 0) twice) is, without the loop: the top two under the total
 * order (inner product, index) of the elements with inner product >= 0, padded with two dummies below every real element.
 * A candidate is the 64-bit key  inner product << 32 | index + 1;  0 is the dummy (and reports product 0, index 0).  Keys of
 * a row's real elements are distinct, the order is total, so the top two of a union is the top two of the parts' top twos
 * in any grouping: lanes are merged with shuffles, tiles with 64-bit atomic max (submit2), and nothing depends on which
 * workgroup arrives first.
 *
 * Operand layout of v_mfma_i32_16x16x64_i8: lane l gives row (l & 15) of A and column (l & 15) of B, 16 bytes of K each,
 * the same 16 for both operands; a dot product does not care which, so lane l simply takes bytes 16 * (l >> 4) ... + 15 of
 * each 64-byte half.  Result register r of lane l is row 4 * (l >> 4) + r, column (l & 15).
 */
#include <hip/hip_runtime.h>

#include "match_device.h"

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

namespace {

/* one step of the reference's loop (nearest_neighbor.cc:91-104): product v with index + 1 = i, visited in ascending index */
__device__ __forceinline__ void top2_step(int& d1, int& i1, int& d2, int& i2, int v, int i) {
    const bool first = v >= d1, second = v >= d2;
    i2 = first ? i1 : (second ? i : i2);
    d2 = first ? d1 : (second ? v : d2);
    i1 = first ? i : i1;
    d1 = first ? v : d1;
}

__device__ __forceinline__ u64 make_key(int d, int i) { return ((u64)(unsigned)d << 32) | (unsigned)i; }

__device__ __forceinline__ void top2_merge(u64& a1, u64& a2, u64 b1, u64 b2) {
    const u64 lo = a1 < b1 ? a1 : b1;
    const u64 hi = a2 > b2 ? a2 : b2;
    a1 = a1 < b1 ? b1 : a1;
    a2 = lo > hi ? lo : hi;
}

/* One key into the (first, second) pair at slot.  The first keeps the largest key ever offered; whatever loses there --
 * the key itself or the key it displaced -- is offered to the second.  The second largest key overall either loses on
 * arrival or is displaced by the largest, so it always reaches the second slot, and nothing larger than it can.
 * Keys not above `floor`, a value the second slot held at some time, cannot be among the top two (the slots only grow). */
__device__ __forceinline__ void submit(u64* slot, u64 k, u64 floor) {
    if (k <= floor) return;
    const u64 old = atomicMax(&slot[0], k);
    const u64 lose = old < k ? old : k;
    if (lose > floor) atomicMax(&slot[1], lose);
}

__device__ __forceinline__ void submit2(u64* slot, u64 k1, u64 k2) {
    const u64 floor = __atomic_load_n(&slot[1], __ATOMIC_RELAXED);
    submit(slot, k1, floor);
    submit(slot, k2, floor);
}

__device__ __forceinline__ int find_job(const MatchJobDev* jobs, int n_jobs, int block) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block0 <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

/* A workgroup: MATCH_STRIP rows of A against one chunk of MATCH_CHUNK columns of B.  Each of its four wavefronts holds all
 * 64 rows (the whole K fits the registers: 4 row blocks x HALVES x 16 bytes per lane) and takes every fourth block of 16
 * columns, whose bytes it reads straight from memory: a column block is used by one wavefront of the workgroup, once. */
template <int HALVES>
__global__ __launch_bounds__(256) void k_match_tiles(const MatchJobDev* __restrict__ jobs, int n_jobs, u64* __restrict__ best) {
    constexpr int D = 64 * HALVES;
    const MatchJobDev jb = jobs[find_job(jobs, n_jobs, (int)blockIdx.x)];
    const int local = (int)blockIdx.x - jb.block0;
    const int strip = local / jb.col_chunks, chunk = local - strip * jb.col_chunks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int row0 = strip * MATCH_STRIP;
    const int n_a = jb.n_a, n_b = jb.n_b;

    v4i a[4][HALVES];
    int roff[4][4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const int r = min(row0 + 16 * f + l15, n_a - 1);
        const v4i* p = (const v4i*)(jb.a + (size_t)r * D + lq * 16);
#pragma unroll
        for (int h = 0; h < HALVES; ++h) a[f][h] = p[h * 4];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) roff[f][r4] = jb.off_a[min(row0 + 16 * f + 4 * lq + r4, n_a - 1)];
    }

    /* Within a lane the columns of a row, and the rows of a column, come in ascending order, so the lane keeps its own
     * top two as the reference's loop does (nearest_neighbor.cc:91-104), in 32 bits: product and index + 1, from (0, index 0)
     * twice.  A dummy that survives becomes the key of a real (product 0, index 0): the lowest real key, and it reports the
     * same, so the merges below need not tell them apart. */
    int r1[4][4], r1i[4][4], r2[4][4], r2i[4][4];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) { r1[f][r4] = r2[f][r4] = 0; r1i[f][r4] = r2i[f][r4] = 1; }

    u64* const rowbest = best + 2 * jb.entry0;
    u64* const colbest = rowbest + 2 * (size_t)n_a;
    const int col_end = min(n_b, (chunk + 1) * MATCH_CHUNK);
    for (int c0 = chunk * MATCH_CHUNK + 16 * wave; c0 < col_end; c0 += 64) {      /* (uniform over the wavefront) */
        const int c = c0 + l15;
        const bool cv = c < col_end;
        const int cc = min(c, n_b - 1);
        const v4i* p = (const v4i*)(jb.b + (size_t)cc * D + lq * 16);
        v4i b[HALVES];
#pragma unroll
        for (int h = 0; h < HALVES; ++h) b[h] = p[h * 4];
        const int coff = jb.off_b[cc];
        int c1 = 0, c1i = 1, c2 = 0, c2i = 1;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            v4i acc = { roff[f][0] + coff, roff[f][1] + coff, roff[f][2] + coff, roff[f][3] + coff };
#pragma unroll
            for (int h = 0; h < HALVES; ++h) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[f][h], b[h], acc, 0, 0, 0);
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int row = row0 + 16 * f + 4 * lq + r4;
                const int v = (cv && row < n_a) ? acc[r4] : -1;    /* a negative product never enters (nearest_neighbor.cc:91) */
                top2_step(r1[f][r4], r1i[f][r4], r2[f][r4], r2i[f][r4], v, c + 1);
                top2_step(c1, c1i, c2, c2i, v, row + 1);
            }
        }
        /* the column's 64 rows lie in lanes l15, l15 + 16, + 32, + 48 */
        u64 cb1 = make_key(c1, c1i), cb2 = make_key(c2, c2i);
#pragma unroll
        for (int m = 16; m <= 32; m <<= 1) {
            const u64 o1 = __shfl_xor(cb1, m), o2 = __shfl_xor(cb2, m);
            top2_merge(cb1, cb2, o1, o2);
        }
        if (lq == 0 && cv) submit2(colbest + 2 * (size_t)c, cb1, cb2);
    }

    /* a row's columns of this wavefront lie in the 16 lanes that share lq */
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            u64 k1 = make_key(r1[f][r4], r1i[f][r4]), k2 = make_key(r2[f][r4], r2i[f][r4]);
#pragma unroll
            for (int m = 1; m <= 8; m <<= 1) {
                const u64 o1 = __shfl_xor(k1, m), o2 = __shfl_xor(k2, m);
                top2_merge(k1, k2, o1, o2);
            }
            const int row = row0 + 16 * f + 4 * lq + r4;
            if (l15 == 0 && row < n_a) submit2(rowbest + 2 * (size_t)row, k1, k2);
        }
}

/* The distances of NearestNeighbor<T>::find (nearest_neighbor.cc:238-241 short, :266-271 unsigned short) and the tests of
 * Matching::oneway_match (matching.h:138-144): both comparisons are `>` in float, the division is IEEE's (0/0 = NaN passes). */
__global__ __launch_bounds__(256) void k_match_final(long long n_entries, int kind, const u64* __restrict__ best, int32_t* __restrict__ matches,
                                                     float square_lowe_thres, float square_dist_thres) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    const u64 k1 = best[2 * e], k2 = best[2 * e + 1];
    const int ip1 = (int)(k1 >> 32), ip2 = (int)(k2 >> 32);
    const int idx1 = k1 ? (int)(unsigned)(k1 & 0xffffffffu) - 1 : 0;
    int d1, d2;
    if (kind == MATCH_SIFT) {
        d1 = 2 * min(32767, 65025 - min(65025, ip1));
        d2 = 2 * min(32767, 65025 - min(65025, ip2));
    } else {
        d1 = 32258 - 2 * min(16129, ip1);
        d2 = 32258 - 2 * min(16129, ip2);
    }
    const float f1 = (float)d1, f2 = (float)d2;
    int res = idx1;
    if (f1 > square_dist_thres) res = -1;
    else if (__fdiv_rn(f1, f2) > square_lowe_thres) res = -1;
    matches[e] = res;
}

/* math::round (libs/math/functions.h:70-73), with no contraction of the product into the sum */
__device__ __forceinline__ float ref_round(float x) {
    return x > 0.0f ? floorf(__fadd_rn(x, 0.5f)) : ceilf(__fadd_rn(x, -0.5f));
}

/* Four components per thread, D / 4 threads per descriptor (groups never straddle a wavefront). */
__global__ __launch_bounds__(256) void k_match_discretise(int kind, int n, const float4* __restrict__ src, int* __restrict__ dst,
                                                          int32_t* __restrict__ off) {
    const int per = kind == MATCH_SIFT ? 32 : 16;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long i = t / per;
    const bool valid = i < n;
    float v[4] = { 0.f, 0.f, 0.f, 0.f };
    if (valid) { const float4 q = src[t]; v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    int packed = 0, sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int byte;
        if (kind == MATCH_SIFT) {
            float x = v[j];
            x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);           /* math::clamp (functions.h:204-207) */
            x = ref_round(__fmul_rn(x, 255.0f));
            byte = (int)(unsigned char)x - 128;
        } else {
            float x = v[j];
            x = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
            x = ref_round(__fmul_rn(x, 127.0f));
            byte = (int)(signed char)x;
        }
        sum += byte;
        packed |= (byte & 0xff) << (8 * j);
    }
    for (int m = 1; m < per; m <<= 1) sum += __shfl_xor(sum, m);
    if (!valid) return;
    dst[t] = packed;
    if (t % per == 0) off[i] = kind == MATCH_SIFT ? 128 * sum + (1 << 20) : 0;
}

}  /* namespace */

void mi_match_discretise(hipStream_t s, int kind, int32_t n, const float* src, int8_t* dst, int32_t* off) {
    if (n <= 0) return;
    const long long threads = (long long)n * (kind == MATCH_SIFT ? 32 : 16);
    hipLaunchKernelGGL(k_match_discretise, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, kind, (int)n, (const float4*)src,
                       (int*)dst, off);
}

void mi_match_launch(hipStream_t s, int kind, const MatchJobDev* jobs, int32_t n_jobs, int32_t n_blocks, int64_t n_entries,
                     unsigned long long* best, int32_t* matches, float square_lowe_thres, float square_dist_thres) {
    if (n_jobs <= 0) return;
    if (kind == MATCH_SIFT)
        hipLaunchKernelGGL(k_match_tiles<2>, dim3((unsigned)n_blocks), dim3(256), 0, s, jobs, (int)n_jobs, best);
    else
        hipLaunchKernelGGL(k_match_tiles<1>, dim3((unsigned)n_blocks), dim3(256), 0, s, jobs, (int)n_jobs, best);
    hipLaunchKernelGGL(k_match_final, dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, s, (long long)n_entries,
                       kind, (const u64*)best, matches, square_lowe_thres, square_dist_thres);
}
