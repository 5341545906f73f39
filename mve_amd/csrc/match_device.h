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
#endif
