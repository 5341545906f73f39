/* Internal: layouts + launchers of ba_device.hip. */
#ifndef MI_BA_DEVICE_H
#define MI_BA_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BA_CAM_BLOCK 256          /* threads of a camera's workgroup (k_ba_cam_build, k_ba_cam_pass) and of the one-workgroup kernels */
#define BA_POINT_LANES 4          /* lanes that share a point's observation list (k_ba_point_build, k_ba_point_pass) */
#define BA_CAM_DOUBLES 15         /* a camera on the device: f, k0, k1, t[3], R[9] */

#define BA_MODE_CAMERAS 1         /* MI_DMRECON_BA_CAMERAS / _POINTS of include/mi_dmrecon.h; 3 is both */
#define BA_MODE_POINTS 2

/* The observations of a call, grouped twice by the host.  A "slot" is an observation's place in point order (point, then
 * the caller's order), a "cpos" its place in camera order (camera, then slot).  Every index below was checked by the host. */
struct BaProblem {
    int32_t n_cam, n_pt, n_obs;
    const int32_t* pt_ptr;        /* [n_pt + 1] first slot of a point */
    const int32_t* cam_ptr;       /* [n_cam + 1] first cpos of a camera */
    const int32_t* s_cam;         /* [n_obs] camera of a slot */
    const int32_t* s_pt;          /* [n_obs] point of a slot */
    const int32_t* s_cpos;        /* [n_obs] cpos of a slot */
    const double* s_xy;           /* [2][n_obs] the observed position of a slot */
    const int32_t* pt_const;      /* [n_pt] Point3D::is_constant */
};

/* One parameter set: the current one or the candidate of an LM step. */
struct BaParams {
    double* cam;                  /* [n_cam][BA_CAM_DOUBLES] */
    double* pt;                   /* [3][n_pt] */
    double* F;                    /* [2][n_obs] residuals by slot */
};

/* alpha, beta and the other numbers of the CG recurrence, and what the host reads once per LM iteration */
struct BaScalars {
    double alpha, beta;
    double rz;                    /* z.r of the recurrence (ba_conjugate_gradient.h:162, :192) */
    double rr;                    /* r.r as last tested against 1e-20 */
    double mse;                   /* of the set k_ba_residual ran on last */
    double pred;                  /* predicted_error_decrease */
    int32_t iter;                 /* ConjugateGradient::Status::num_iterations */
    int32_t done;
};

/* Everything a linear step writes.  D is the camera block dimension (6 or 9); every [..][n] array is structure-of-arrays. */
struct BaWork {
    double* Jc_p;                 /* [2 D][n_obs] camera Jacobian by slot: row 2 j is d x / d param j, row 2 j + 1 d y */
    double* Jc_c;                 /* [2 D][n_obs] the same by cpos */
    double* Jp;                   /* [6][n_obs] point Jacobian by slot */
    double* F_c;                  /* [2][n_obs] residuals of the current set by cpos */
    double* q;                    /* [2][n_obs] Jp u of the point pass by cpos */
    double* Cinv;                 /* [6][n_pt] upper triangle of the inverted (or left) regularised block */
    double* Cdiag;                /* [3][n_pt] diagonal before regularisation */
    double* w;                    /* [3][n_pt] */
    double* dz;                   /* [3][n_pt] point step */
    double* B;                    /* [n_cam][D D] regularised */
    double* P;                    /* [n_cam][D D] preconditioner */
    double* Bdiag;                /* [n_cam][D] diagonal before regularisation */
    double* v;                    /* [n_cam][D] */
    double* x;                    /* [n_cam][D] camera step; r, d, z, Ad: the CG vectors */
    double* r;
    double* d;
    double* z;
    double* Ad;
    double* cam_part;             /* [n_cam] a camera's share of a dot product */
    double* blk_part;             /* [ceil(n_obs / BA_CAM_BLOCK)] a workgroup's share of the squared residuals */
    BaScalars* sc;
};

/* What an LM iteration asks of the launchers. */
struct BaStep {
    hipStream_t stream;
    int32_t dim;                  /* 6: fixed intrinsics, 9 */
    int32_t mode;                 /* BA_MODE_* */
    int32_t cg_max;
    double radius;                /* trust_region_radius */
};

/* k_ba_residual + k_ba_total: set.F and sc->mse */
void mi_ba_launch_residual(hipStream_t s, const BaProblem& p, const BaParams& set, const BaWork& w);
/* k_ba_jacobian (if `jacobian`: the set has changed since the last one), k_ba_point_build, k_ba_cam_build, k_ba_cg_init */
void mi_ba_launch_build(const BaStep& st, const BaProblem& p, const BaParams& cur, const BaWork& w, bool jacobian);
/* n CG iterations of three launches each (two in BA_MODE_CAMERAS); each returns at once when sc->done is set */
void mi_ba_launch_cg(const BaStep& st, const BaProblem& p, const BaWork& w, int32_t n);
/* back substitution, predicted decrease, k_ba_update into cand, and the residuals of cand */
void mi_ba_launch_finish(const BaStep& st, const BaProblem& p, const BaParams& cur, const BaParams& cand, const BaWork& w);
#endif
