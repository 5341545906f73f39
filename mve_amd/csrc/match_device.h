/* Internal: layouts + launchers of match_device.hip. */
#ifndef MI_MATCH_DEVICE_H
#define MI_MATCH_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MATCH_SIFT 0              /* 128 dims, unsigned bytes stored biased by -128 (sfm/exhaustive_matching.cc:18-27) */
#define MATCH_SURF 1              /*  64 dims, signed bytes (exhaustive_matching.cc:29-39) */

#define MATCH_STRIP 64            /* rows of A a workgroup keeps in registers ... */
#define MATCH_CHUNK 2048          /* ... against this many columns of B, 16 at a time per wavefront */

/* One (set a, n_a, set b, n_b) job as the kernels see it.  `off` restores the unbiased inner product of SIFT:
 * <a, b> = <a', b'> + off_a + off_b with off = 128 * sum(a') + 2^20 (twice 2^20 = 128 * 128^2); all zeros for SURF. */
struct MatchJobDev {
    const int8_t* a;              /* n_a rows of 128 / 64 bytes */
    const int8_t* b;
    const int32_t* off_a;
    const int32_t* off_b;
    int32_t n_a, n_b;             /* both > 0 */
    int32_t block0;               /* the job's first workgroup in the tile kernel's grid */
    int32_t col_chunks;           /* workgroups per strip of rows */
    int64_t entry0;               /* the job's first entry in best[] / matches[]: its n_a rows, then its n_b columns */
};

/* n float descriptors -> packed bytes + off (the reference's convert_descriptor, exhaustive_matching.cc:18-39) */
void mi_match_discretise(hipStream_t s, int kind, int32_t n, const float* src, int8_t* dst, int32_t* off);

/* best: 2 keys per entry, zeroed by the caller.  One launch over every job's tiles, then one over every entry:
 * matches[e] = the one-way match of entry e (matching.h:114-146). */
void mi_match_launch(hipStream_t s, int kind, const MatchJobDev* jobs, int32_t n_jobs, int32_t n_blocks, int64_t n_entries,
                     unsigned long long* best, int32_t* matches, float square_lowe_thres, float square_dist_thres);

/* ---- cascade hashing (libs/sfm/cascade_hashing.h, cascade_hashing.cc) ---------------------------------------------------- */

#define CASHASH_MAX_GROUPS 8      /* bucket ids of a record */
#define CASHASH_MAX_CANDIDATES 16 /* one candidate per lane of a query's 16 */
#define CASHASH_BUCKETS 256       /* per group, whatever num_bucket_bits is: ids above 2^bits - 1 do not occur */
#define CASHASH_TILE 64           /* descriptors a workgroup of k_cashash_codes stages in LDS */

/* What the match kernel reads of a candidate, in one 32-byte load: the hash code in the reference's word layout (SURF: code[1]
 * is 0) and the bucket id of every group (groups past num_bucket_groups: 0). */
struct CashashRecord {
    unsigned long long code[2];
    uint8_t bucket[CASHASH_MAX_GROUPS];
    uint8_t pad[8];
};

/* The hashed state of one descriptor list: n records; per group CASHASH_BUCKETS + 1 offsets and the n feature ids, those of a
 * bucket contiguous and ascending (build_buckets, cascade_hashing.cc:200-223). */
struct CashashSetDev {
    const CashashRecord* rec;
    const int32_t* bucket_off;    /* groups x (CASHASH_BUCKETS + 1) */
    const int32_t* bucket_ids;    /* groups x n */
    const int8_t* desc;
    const int32_t* off;           /* MatchJobDev::off */
    int32_t n;
};

/* One two-way job: entries entry0 ... + a.n - 1 are the queries of a against b, the next b.n those of b against a. */
struct CashashJobDev {
    CashashSetDev a, b;           /* both n > 0 */
    int64_t entry0;
};

struct CashashParams {
    int32_t groups, bits, min_candidates, max_candidates;
};

/* compute_cascade_hashes (cascade_hashing.h:258-311) of n stored descriptors.  proj: ceil(D / 64) + 1 blocks of D x 64 floats,
 * block k < D / 64 holding the primary projections 64 k ... 64 k + 63 and the last the groups * bits secondary ones, padded
 * with zeros; within a block component-major (the 64 projections of a component are contiguous). */
void mi_cashash_codes(hipStream_t s, int kind, int32_t n, const int8_t* desc, const float* mean, const float* proj,
                      CashashParams p, CashashRecord* rec);

/* build_buckets from the records: no global atomics, the same bytes on every run. */
void mi_cashash_buckets(hipStream_t s, int32_t n, const CashashRecord* rec, CashashParams p, int32_t* bucket_off, int32_t* bucket_ids);

/* CascadeHashing::oneway_match (cascade_hashing.h:328-471) of every entry of every job, both directions, in one launch. */
void mi_cashash_match(hipStream_t s, int kind, const CashashJobDev* jobs, int32_t n_jobs, int64_t n_entries, CashashParams p,
                      int32_t* matches, float square_lowe_thres, float square_dist_thres);
#endif
