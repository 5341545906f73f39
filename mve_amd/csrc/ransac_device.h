/* Internal: layouts + launcher of ransac_device.hip. */
#ifndef MI_RANSAC_DEVICE_H
#define MI_RANSAC_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RANSAC_TILE 128           /* hypotheses of a k_ransac_count workgroup: one per lane, two wavefronts ... */
#define RANSAC_CHUNK 256          /* ... against this many list entries, staged once in LDS (32 bytes each: 8 KiB; P3P 48: 12 KiB) */
#define RANSAC_MAX_SWEEPS 30      /* Jacobi sweeps of one solve; a hypothesis that gets there is kept and counted */

/* The three models.  A hypothesis is RANSAC_HYP doubles, of which the first RANSAC_GUARD are what the count reads (and must
 * be finite); a list entry (a match, a 2D-3D correspondence) is RANSAC_ENTRY doubles on the device. */
enum RansacModel { RANSAC_F = 0, RANSAC_H = 1, RANSAC_P3P = 2 };
#define RANSAC_F_HYP 9            /* F */
#define RANSAC_H_HYP 18           /* H, then H^-1 */
#define RANSAC_P3P_HYP 24         /* P = K [R|t], then the pose [R|t] itself */
#define RANSAC_P3P_ENTRY 6        /* x y z u v and one pad: 48 bytes, read as three aligned 16-byte words */

/* One job as the kernels see it.  List entries, samples, counts, hypotheses and inlier lists of all jobs of a call lie
 * behind one another in one array each; a job knows where its part starts. */
struct RansacJobDev {
    int32_t n_matches;            /* list entries */
    int32_t n_hyp;                /* hypotheses: the iterations (F, H), four per iteration (P3P) */
    int32_t inliers_to_beat;
    int32_t block0;               /* the job's first workgroup in k_ransac_count's grid */
    int32_t chunks;               /* list chunks per hypothesis tile: the job has tiles x chunks workgroups */
    int32_t hyp0;                 /* first hypothesis: counts[hyp0 ...], hyp_all[HYP * hyp0 ...]; its samples start at row
                                     hyp0 (F: 8 wide, H: 4 wide) or hyp0 / 4 (P3P: 3 wide) */
    int64_t match0;               /* first list entry: list[ENTRY * match0 ...], inliers[match0 ...] */
    double thr2;                  /* threshold squared */
    double k[9], k_inv[9];        /* P3P only: the calibration and its inverse (ransac_host.cpp), row-major */
};

struct RansacBuffers {
    const RansacJobDev* jobs;
    const double* list;           /* ENTRY per entry, 32-byte aligned */
    const int32_t* samples;       /* 8 / 4 / 3 per iteration, every index checked by the host */
    double* hyp_all;              /* HYP per hypothesis */
    int32_t* counts;              /* 1 per hypothesis */
    double* best_model;           /* 9 (F, H) or 12 (the pose) per job (written for a job that has a winner) */
    int32_t* best;                /* 2 per job: best hypothesis (-1: none), n_inliers */
    int32_t* inliers;             /* 1 per list entry */
    unsigned long long* capped;   /* solves that ran into RANSAC_MAX_SWEEPS; only ever added to */
};

/* The model's hypothesis kernel over n_hyp hypotheses (it also zeroes their counts), k_ransac_count over n_blocks
 * workgroups, k_ransac_pick over n_jobs. */
void mi_ransac_launch(hipStream_t s, RansacModel model, const RansacBuffers& b, int32_t n_jobs, int32_t n_hyp, int32_t n_blocks);
#endif
