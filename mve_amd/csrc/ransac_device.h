/* Internal: layouts + launcher of ransac_device.hip. */
#ifndef MI_RANSAC_DEVICE_H
#define MI_RANSAC_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RANSAC_TILE 128           /* hypotheses of a k_ransac_count workgroup: one per lane, two wavefronts ... */
#define RANSAC_CHUNK 256          /* ... against this many matches, staged once in LDS (32 bytes each: 8 KiB) */
#define RANSAC_MAX_SWEEPS 30      /* Jacobi sweeps of one solve; a hypothesis that gets there is kept and counted */

/* One job as the kernels see it.  Matches, samples, counts, F and inlier lists of all jobs of a call lie behind one
 * another in one array each; a job knows where its part starts. */
struct RansacJobDev {
    int32_t n_matches, n_iterations;
    int32_t inliers_to_beat;
    int32_t block0;               /* the job's first workgroup in k_ransac_count's grid */
    int32_t chunks;               /* match chunks per hypothesis tile: the job has tiles x chunks workgroups */
    int32_t hyp0;                 /* first hypothesis: counts[hyp0 ...], F_all[9 * hyp0 ...], samples[8 * hyp0 ...] */
    int64_t match0;               /* first match: matches[4 * match0 ...], inliers[match0 ...] */
    double thr2;                  /* threshold squared */
};

struct RansacBuffers {
    const RansacJobDev* jobs;
    const double* matches;        /* 4 per match, 32-byte aligned */
    const int32_t* samples;       /* 8 per hypothesis, every index checked by the host */
    double* F_all;                /* 9 per hypothesis */
    int32_t* counts;              /* 1 per hypothesis */
    double* F_best;               /* 9 per job (written for a job that has a winner) */
    int32_t* best;                /* 2 per job: best_iteration (-1: none), n_inliers */
    int32_t* inliers;             /* 1 per match */
    unsigned long long* capped;   /* solves that ran into RANSAC_MAX_SWEEPS; only ever added to */
};

/* k_ransac_f8 over n_hyp hypotheses (it also zeroes their counts), k_ransac_count over n_blocks workgroups,
 * k_ransac_pick over n_jobs. */
void mi_ransac_launch(hipStream_t s, const RansacBuffers& b, int32_t n_jobs, int32_t n_hyp, int32_t n_blocks);
#endif
