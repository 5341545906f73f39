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
 *
 * Second half of the file: cascade hashing (libs/sfm/cascade_hashing.h, cascade_hashing.cc) on the same resident bytes --
 * k_cashash_codes, k_cashash_buckets, k_cashash_match; each is described where it stands.
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
 * Matching::oneway_match (matching.h:138-144): both comparisons are `>` in float, the division is IEEE's (0/0 = NaN passes).
 * The index of the best of the two keys, or -1. */
__device__ __forceinline__ int match_decide(int kind, u64 k1, u64 k2, float square_lowe_thres, float square_dist_thres) {
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
    return res;
}

__global__ __launch_bounds__(256) void k_match_final(long long n_entries, int kind, const u64* __restrict__ best, int32_t* __restrict__ matches,
                                                     float square_lowe_thres, float square_dist_thres) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    matches[e] = match_decide(kind, best[2 * e], best[2 * e + 1], square_lowe_thres, square_dist_thres);
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

/* ---- cascade hashing ------------------------------------------------------------------------------------------------------
 *
 * k_cashash_codes.  The D + groups * bits projections of a descriptor are cut into blocks of 64 (blockIdx.y: the D / 64 code
 * words, then the secondary projections).  A lane IS one projection of its block: it keeps that projection's D coefficients
 * in registers for the whole kernel.  The workgroup stages CASHASH_TILE zero-mean descriptors in LDS, each wavefront takes
 * every fourth, reads it as broadcasts (every lane the same address) and the ballot of `sum > 0` is the whole code word:
 * lane k is projection k of the block, the reference puts the first projection into the most significant bit
 * (cascade_hashing.h:288-293), so the word is the ballot bit-reversed.  The bucket ids are fields of the reversed ballot of
 * the secondary block.  z = fl(fl(d / scale) - mean) as compute_zero_mean_descs (cascade_hashing.cc:187-195); the sum runs
 * in four strided partial sums of fused multiply-adds: the reference's own order is not defined (-funsafe-math-optimizations),
 * so a sum within rounding of zero may fall either way (include/mi_dmrecon.h). */
template <int D>
__global__ __launch_bounds__(256) void k_cashash_codes(int kind, int n, const int8_t* __restrict__ desc, const float* __restrict__ mean,
                                                       const float* __restrict__ proj, CashashParams p, CashashRecord* __restrict__ rec) {
    constexpr int WORDS = D / 64;
    __shared__ float z[CASHASH_TILE][D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int blk = blockIdx.y;
    const int base = blockIdx.x * CASHASH_TILE;
    const float scale = kind == MATCH_SIFT ? 255.0f : 127.0f;
    const int bias = kind == MATCH_SIFT ? 128 : 0;             /* (the stored bytes of SIFT are biased by -128) */
    for (int t = threadIdx.x; t < CASHASH_TILE * D / 4; t += 256) {
        const int j = t / (D / 4), c4 = t % (D / 4);
        const int packed = base + j < n ? ((const int*)desc)[(size_t)(base + j) * (D / 4) + c4] : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = (int)(signed char)(packed >> (8 * k)) + bias;
            z[j][4 * c4 + k] = __fsub_rn(__fdiv_rn((float)d, scale), mean[4 * c4 + k]);
        }
    }
    __syncthreads();

    float pr[D];
#pragma unroll
    for (int i = 0; i < D; ++i) pr[i] = proj[((size_t)blk * D + i) * 64 + lane];

    for (int j = wave; j < CASHASH_TILE && base + j < n; j += 4) {             /* (uniform over the wavefront) */
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
        for (int i = 0; i < D; i += 4) {
            const float4 v = *(const float4*)&z[j][i];
            s0 = fmaf(v.x, pr[i], s0); s1 = fmaf(v.y, pr[i + 1], s1); s2 = fmaf(v.z, pr[i + 2], s2); s3 = fmaf(v.w, pr[i + 3], s3);
        }
        const float sum = (s0 + s1) + (s2 + s3);
        const u64 bits = __brevll(__ballot(sum > 0.0f));
        if (lane != 0) continue;
        CashashRecord* r = rec + base + j;
        if (blk < WORDS) {
            r->code[blk] = bits;
            if (WORDS == 1) r->code[1] = 0;
        } else {
            u64 ids = 0;
            for (int g = 0; g < p.groups; ++g)
                ids |= ((bits >> (64 - (g + 1) * p.bits)) & ((1u << p.bits) - 1)) << (8 * g);
            *(u64*)r->bucket = ids;
            *(u64*)r->pad = 0;
        }
    }
}

/* k_cashash_buckets: one wavefront per group, a stable counting sort of the feature ids by bucket id.  Counts in LDS (integer
 * adds: the same whatever the order), an exclusive scan, then the features 64 at a time in feature order: the lanes that
 * share a bucket id find each other with one ballot per bit, a lane's rank among them is the number of lower lanes, and the
 * highest of them moves the bucket's cursor on.  No global atomics; ids ascend within a bucket. */
__global__ __launch_bounds__(64) void k_cashash_buckets(int n, const CashashRecord* __restrict__ rec, int32_t* __restrict__ bucket_off,
                                                        int32_t* __restrict__ bucket_ids) {
    __shared__ int cursor[CASHASH_BUCKETS];
    const int g = blockIdx.x, lane = threadIdx.x;
    for (int b = lane; b < CASHASH_BUCKETS; b += 64) cursor[b] = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) atomicAdd(&cursor[rec[i].bucket[g]], 1);
    __syncthreads();
    int c[4], total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { c[k] = cursor[4 * lane + k]; total += c[k]; }
    int incl = total;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_up(incl, m);
        if (lane >= m) incl += o;
    }
    __syncthreads();
    int at = incl - total;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cursor[4 * lane + k] = at;
        bucket_off[g * (CASHASH_BUCKETS + 1) + 4 * lane + k] = at;
        at += c[k];
    }
    if (lane == 63) bucket_off[g * (CASHASH_BUCKETS + 1) + CASHASH_BUCKETS] = at;
    __syncthreads();
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool valid = i < n;
        const int b = valid ? rec[i].bucket[g] : 0;
        u64 same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const u64 m = __ballot((b >> bit) & 1);
            same &= ((b >> bit) & 1) ? m : ~m;
        }
        const int start = cursor[b];
        if (valid) bucket_ids[(size_t)g * n + start + __popcll(same & ((1ull << lane) - 1))] = i;
        __syncthreads();
        if (valid && (same >> lane) == 1) cursor[b] = start + __popcll(same);
        __syncthreads();
    }
}

#define CASHASH_NONE 0xffffffffu  /* no candidate: above every key  level << 24 | seq  (level <= 128) */

/* one compare-exchange step of a bitonic network over the 16 lanes of a query */
__device__ __forceinline__ unsigned cashash_cmpx(unsigned key, int j, bool ascending, int lane) {
    const unsigned o = __shfl_xor(key, j);
    return (((lane & j) == 0) == ascending) ? min(key, o) : max(key, o);
}

/* Where position s of a query's walk lies: the walk is the query's bucket of group 0, then of group 1, ...; pre[k] is the
 * number of positions before group k.  Returns the index into bucket_ids and the group. */
__device__ __forceinline__ int cashash_locate(int s, const int (&pre)[CASHASH_MAX_GROUPS + 1], const int (&start)[CASHASH_MAX_GROUPS], int n_c,
                                              int& group) {
    int at = 0;
    group = 0;
#pragma unroll
    for (int k = 0; k < CASHASH_MAX_GROUPS; ++k)
        if (s >= pre[k] && s < pre[k + 1]) { group = k; at = k * n_c + start[k] + (s - pre[k]); }
    return at;
}

/* k_cashash_match: CascadeHashing::oneway_match for every entry of every job.  Sixteen lanes per query, four queries per
 * wavefront; the n_a queries of a job against b and its n_b queries against a are the same problem with the roles swapped.
 *
 * The reference groups the candidates by level (the Hamming distance of the codes), takes whole levels until it has `min`
 * and stops inside a level at `max` (collect_top_ranked_candidates, cascade_hashing.h:450-471).  Under the total order
 * (level, seq) -- seq: the position in the walk -- that is a PREFIX of the sorted candidates: the first min(max, number of
 * candidates of level <= h*), h* the level of the min-th.  max <= 16, so the prefix fits the query's 16 lanes, one key
 * level << 24 | seq  each: the lanes stride over the walk 16 positions at a time, sort the 16 new keys with a bitonic network
 * of shuffles and merge them into the 16 smallest so far (elementwise min against the reversed batch, four more steps).  A
 * batch none of whose keys is below the 16th so far is skipped.  No LDS, no atomics, and every candidate record is read once.
 *
 * A candidate met in group g was met before exactly when its bucket id equals the query's in some group below g
 * (collect_features_from_buckets marks it in data_index_used there, cascade_hashing.h:433-446): a test on the two records'
 * own bucket bytes -- "has the xor a zero byte below byte g" -- in place of the reference's bitmap.
 *
 * Then one selected candidate per lane: the inner product on the stored bytes (v_dot4c_i32_i8), the key of k_match_tiles with
 * the lane, i. e. the candidate's place in (level, seq) order, for the index, the top two merged by shuffles, and
 * match_decide.  A dummy that wins reports place 0 (nearest_neighbor.cc:218-272 starts from index 0). */
template <int HALVES>
__global__ __launch_bounds__(256) void k_cashash_match(const CashashJobDev* __restrict__ jobs, int n_jobs, long long n_entries, CashashParams p,
                                                       int kind, int32_t* __restrict__ matches, float square_lowe_thres,
                                                       float square_dist_thres) {
    constexpr int D = 64 * HALVES;
    const int lane = threadIdx.x & 63, l16 = lane & 15, first = lane & ~15;
    long long e = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = e < n_entries;
    if (!live) e = n_entries - 1;                              /* (its lanes stay for the shuffles and write nothing) */
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].entry0 <= e) lo = mid; else hi = mid - 1;
    }
    const long long local = e - jobs[lo].entry0;
    const bool forward = local < jobs[lo].a.n;
    const CashashSetDev Q = forward ? jobs[lo].a : jobs[lo].b, C = forward ? jobs[lo].b : jobs[lo].a;
    const int q = (int)(forward ? local : local - jobs[lo].a.n);

    const CashashRecord rq = Q.rec[q];
    const u64 qb = *(const u64*)rq.bucket;
    int pre[CASHASH_MAX_GROUPS + 1], start[CASHASH_MAX_GROUPS];
    pre[0] = 0;
#pragma unroll
    for (int g = 0; g < CASHASH_MAX_GROUPS; ++g) {
        int len = 0;
        start[g] = 0;
        if (g < p.groups) {
            const int32_t* o = C.bucket_off + g * (CASHASH_BUCKETS + 1) + (int)((qb >> (8 * g)) & 0xff);
            start[g] = o[0];
            len = o[1] - o[0];
        }
        pre[g + 1] = pre[g] + len;
    }
    const int L = live ? pre[CASHASH_MAX_GROUPS] : 0;
    int l_max = L;
    l_max = max(l_max, __shfl_xor(l_max, 16));
    l_max = max(l_max, __shfl_xor(l_max, 32));

    unsigned best = CASHASH_NONE;                              /* lane i: the i-th smallest key so far */
    for (int s0 = 0; s0 < l_max; s0 += 16) {                   /* (uniform over the wavefront) */
        const int s = s0 + l16;
        unsigned key = CASHASH_NONE;
        if (s < L) {
            int g;
            const int c = C.bucket_ids[cashash_locate(s, pre, start, C.n, g)];
            const CashashRecord* rc = C.rec + c;
            const u64 c0 = rc->code[0], c1 = rc->code[1];
            const u64 y = (*(const u64*)rc->bucket ^ qb) | (~0ull << (8 * g));
            const bool seen = ((y - 0x0101010101010101ull) & ~y & 0x8080808080808080ull) != 0;
            if (!seen) key = (unsigned)(__popcll(c0 ^ rq.code[0]) + __popcll(c1 ^ rq.code[1])) << 24 | (unsigned)s;
        }
        const unsigned worst = __shfl(best, first | 15);
        if (!__any(key < worst)) continue;
#pragma unroll
        for (int k = 2; k <= 16; k <<= 1)
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) key = cashash_cmpx(key, j, (l16 & k) == 0, lane);
        best = min(best, __shfl_xor(key, 15));
#pragma unroll
        for (int j = 8; j > 0; j >>= 1) best = cashash_cmpx(best, j, true, lane);
    }

    const unsigned h_star = __shfl(best, first | (p.min_candidates - 1)) >> 24;      /* 255: fewer than min, all are taken */
    const bool taken = l16 < p.max_candidates && best != CASHASH_NONE && (best >> 24) <= h_star;
    int c = 0;
    u64 k1 = 0, k2 = 0;
    if (taken) {
        int g;
        c = C.bucket_ids[cashash_locate((int)(best & 0xffffffu), pre, start, C.n, g)];
        const v4i* qd = (const v4i*)(Q.desc + (size_t)q * D);
        const v4i* cd = (const v4i*)(C.desc + (size_t)c * D);
        int ip = Q.off[q] + C.off[c];
#pragma unroll
        for (int w = 0; w < D / 16; ++w) {
            const v4i a = qd[w], b = cd[w];
#pragma unroll
            for (int k = 0; k < 4; ++k) ip = __builtin_amdgcn_sdot4(a[k], b[k], ip, false);
        }
        if (ip >= 0) k1 = make_key(ip, l16 + 1);               /* a negative product never enters (nearest_neighbor.cc:91) */
    }
#pragma unroll
    for (int m = 1; m <= 8; m <<= 1) {
        const u64 o1 = __shfl_xor(k1, m), o2 = __shfl_xor(k2, m);
        top2_merge(k1, k2, o1, o2);
    }
    const int place = match_decide(kind, k1, k2, square_lowe_thres, square_dist_thres);
    const int id = __shfl(c, first | max(place, 0));
    const bool any = __shfl(best, first) != CASHASH_NONE;      /* a query without any candidate: -1 (include/mi_dmrecon.h) */
    if (live && l16 == 0) matches[e] = (any && place >= 0) ? id : -1;
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

void mi_cashash_codes(hipStream_t s, int kind, int32_t n, const int8_t* desc, const float* mean, const float* proj,
                      CashashParams p, CashashRecord* rec) {
    if (n <= 0) return;
    const unsigned tiles = (unsigned)((n + CASHASH_TILE - 1) / CASHASH_TILE);
    if (kind == MATCH_SIFT)
        hipLaunchKernelGGL(k_cashash_codes<128>, dim3(tiles, 3), dim3(256), 0, s, kind, (int)n, desc, mean, proj, p, rec);
    else
        hipLaunchKernelGGL(k_cashash_codes<64>, dim3(tiles, 2), dim3(256), 0, s, kind, (int)n, desc, mean, proj, p, rec);
}

void mi_cashash_buckets(hipStream_t s, int32_t n, const CashashRecord* rec, CashashParams p, int32_t* bucket_off, int32_t* bucket_ids) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_cashash_buckets, dim3((unsigned)p.groups), dim3(64), 0, s, (int)n, rec, bucket_off, bucket_ids);
}

void mi_cashash_match(hipStream_t s, int kind, const CashashJobDev* jobs, int32_t n_jobs, int64_t n_entries, CashashParams p,
                      int32_t* matches, float square_lowe_thres, float square_dist_thres) {
    if (n_jobs <= 0 || n_entries <= 0) return;
    const dim3 grid((unsigned)((n_entries + 15) / 16));
    if (kind == MATCH_SIFT)
        hipLaunchKernelGGL(k_cashash_match<2>, grid, dim3(256), 0, s, jobs, (int)n_jobs, (long long)n_entries, p, kind, matches,
                           square_lowe_thres, square_dist_thres);
    else
        hipLaunchKernelGGL(k_cashash_match<1>, grid, dim3(256), 0, s, jobs, (int)n_jobs, (long long)n_entries, p, kind, matches,
                           square_lowe_thres, square_dist_thres);
}
