/*
 * ba_device.hip -- bundle adjustment on gfx950: the Levenberg-Marquardt step of sfm::ba::BundleAdjustment
 * (libs/sfm/bundle_adjustment.cc:73-201) with the linear solvers of libs/sfm/ba_linear_solver.cc:141-313 and the
 * preconditioned CG of libs/sfm/ba_conjugate_gradient.h:132-210.  All arithmetic is f64.
 *
 * The reference builds J, B, C, E and the Schur complement S as sparse matrices.  Here neither E nor S exists: per
 * observation only the camera block Jc (2 x D, D = 6 or 9) and the point block Jp (2 x 3) are stored, and
 *     S d = B d - Jc^T Jp C^-1 Jp^T Jc d
 * is applied in two passes per CG iteration:
 *   k_ba_point_pass  BA_POINT_LANES lanes per point walk the point's observations (slot order), sum t = Jp^T (Jc d), apply
 *                    the 3 x 3 inverse the lanes hold, and leave q = Jp (C^-1 t) per observation in camera order;
 *   k_ba_cam_pass    one workgroup per camera walks the camera's observations (cpos order), sums Jc^T q, and forms
 *                    B d - sum and the camera's share of d . Ad;
 *   k_ba_cg_update   one workgroup: alpha, x, r, the convergence test, z = P r, beta, d, the iteration counter and `done`.
 * Jc is kept twice, by slot and by cpos, so that both walks read consecutive addresses.
 *
 * Every sum has a fixed order -- a serial walk with a fixed stride, then a butterfly over the lanes of a wavefront (both
 * partners add the same two numbers), then the wavefronts of the workgroup through LDS in index order -- and there is no
 * floating-point atomic: the same input gives the same bytes.  No kernel waits for another workgroup.
 *
 * No matrix instruction: the blocks are 9 x 3, 3 x 3 and 9 x 9 in f64 and every sum runs over a sparse list.
 */
#include <hip/hip_runtime.h>

#include "ba_device.h"

namespace {

constexpr int WAVES = BA_CAM_BLOCK / 64;

/* The sum of a[k] over the workgroup's BA_CAM_BLOCK threads, in every thread.  lds: WAVES * N doubles. */
template <int N>
__device__ __forceinline__ void block_sum(double (&a)[N], double* lds) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double x = a[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
        a[k] = x;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) lds[wave * N + k] = a[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double t = lds[k];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t += lds[w * N + k];
        a[k] = t;
    }
}

/* ... and over the BA_POINT_LANES lanes of a point */
template <int N>
__device__ __forceinline__ void point_sum(double (&a)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double x = a[k];
#pragma unroll
        for (int m = BA_POINT_LANES / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
        a[k] = x;
    }
}

/* What projecting a point into a camera gives (bundle_adjustment.cc:247-260, :425-435). */
struct Proj {
    double rx, ry, rz;            /* R X */
    double pz, ix, iy, r2, rd;    /* depth, image-plane position, its squared radius, the distortion factor */
};

__device__ __forceinline__ Proj project(const double* c, double X, double Y, double Z) {
    Proj p;
    p.rx = c[6] * X + c[7] * Y + c[8] * Z;
    p.ry = c[9] * X + c[10] * Y + c[11] * Z;
    p.rz = c[12] * X + c[13] * Y + c[14] * Z;
    p.pz = p.rz + c[5];
    p.ix = (p.rx + c[3]) / p.pz;
    p.iy = (p.ry + c[4]) / p.pz;
    p.r2 = p.ix * p.ix + p.iy * p.iy;
    p.rd = 1.0 + p.r2 * (c[1] + c[2] * p.r2);
    return p;
}

/* R = I + st K + ct K^2 with the reference's a == 0 case (bundle_adjustment.cc:287-304) */
__device__ __forceinline__ void rodrigues(const double* r, double (&m)[9]) {
    const double a = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    const double ct = a == 0.0 ? 0.5 : (1.0 - cos(a)) / (a * a);
    const double st = a == 0.0 ? 1.0 : sin(a) / a;
    m[0] = 1.0 - (r[1] * r[1] + r[2] * r[2]) * ct;
    m[1] = r[0] * r[1] * ct - r[2] * st;
    m[2] = r[2] * r[0] * ct + r[1] * st;
    m[3] = r[0] * r[1] * ct + r[2] * st;
    m[4] = 1.0 - (r[2] * r[2] + r[0] * r[0]) * ct;
    m[5] = r[1] * r[2] * ct - r[0] * st;
    m[6] = r[2] * r[0] * ct - r[1] * st;
    m[7] = r[1] * r[2] * ct + r[0] * st;
    m[8] = 1.0 - (r[0] * r[0] + r[1] * r[1]) * ct;
}

/* ---- residuals and their mean square (bundle_adjustment.cc:204-275) ---- */

__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_residual(BaProblem P, BaParams S, BaWork W) {
    __shared__ double lds[WAVES];
    const int s = (int)blockIdx.x * BA_CAM_BLOCK + (int)threadIdx.x;
    double sq[1] = {0.0};
    if (s < P.n_obs) {
        const int pt = P.s_pt[s];
        const Proj p = project(S.cam + (size_t)P.s_cam[s] * BA_CAM_DOUBLES, S.pt[pt], S.pt[P.n_pt + pt], S.pt[2 * (size_t)P.n_pt + pt]);
        const double f = S.cam[(size_t)P.s_cam[s] * BA_CAM_DOUBLES];
        const double fx = p.ix * p.rd * f - P.s_xy[s];
        const double fy = p.iy * p.rd * f - P.s_xy[(size_t)P.n_obs + s];
        S.F[s] = fx;
        S.F[(size_t)P.n_obs + s] = fy;
        sq[0] = fx * fx + fy * fy;
    }
    block_sum<1>(sq, lds);
    if (threadIdx.x == 0) W.blk_part[blockIdx.x] = sq[0];
}

/* one workgroup: out = (part[0] + ... + part[n - 1]) / divisor */
__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_total(const double* part, int n, double divisor, double* out) {
    __shared__ double lds[WAVES];
    double sum[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += BA_CAM_BLOCK) sum[0] += part[i];
    block_sum<1>(sum, lds);
    if (threadIdx.x == 0) *out = sum[0] / divisor;
}

/* ---- the Jacobian (bundle_adjustment.cc:381-635) ----
 * For a parameter that moves the image-plane position by (a, b):  d r2 = 2 (ix a + iy b),  d rd = rdp d r2  with
 * rdp = k0 + 2 k1 r2, and  d x = f (d rd ix + rd a),  d y = f (d rd iy + rd b): the reference's chain rule (:544-632).
 * With fixed intrinsics the reference treats rd as constant (:438-465): the same expressions with rdp = 0. */
template <int D>
__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_jacobian(BaProblem P, BaParams S, BaWork W, int mode) {
    const int s = (int)blockIdx.x * BA_CAM_BLOCK + (int)threadIdx.x;
    if (s >= P.n_obs) return;
    const size_t n = (size_t)P.n_obs;
    const int pt = P.s_pt[s], cpos = P.s_cpos[s];
    const double* c = S.cam + (size_t)P.s_cam[s] * BA_CAM_DOUBLES;
    const Proj p = project(c, S.pt[pt], S.pt[P.n_pt + pt], S.pt[2 * (size_t)P.n_pt + pt]);
    const double f = c[0];
    const double rdp = D == 9 ? c[1] + 2.0 * c[2] * p.r2 : 0.0;
    auto chain = [&](double a, double b, double& jx, double& jy) {
        const double drd = rdp * (2.0 * (p.ix * a + p.iy * b));
        jx = f * (drd * p.ix + p.rd * a);
        jy = f * (drd * p.iy + p.rd * b);
    };
    W.F_c[cpos] = S.F[s];
    W.F_c[n + cpos] = S.F[n + s];

    if (mode & BA_MODE_CAMERAS) {
        double jx[D], jy[D];
        constexpr int T = D - 6;                                /* translation starts here, rotation three further */
        if (D == 9) {
            jx[0] = p.ix * p.rd;             jy[0] = p.iy * p.rd;
            jx[1] = f * p.ix * p.r2;         jy[1] = f * p.iy * p.r2;
            jx[2] = f * p.ix * p.r2 * p.r2;  jy[2] = f * p.iy * p.r2 * p.r2;
        }
        chain(1.0 / p.pz, 0.0, jx[T], jy[T]);
        chain(0.0, 1.0 / p.pz, jx[T + 1], jy[T + 1]);
        chain(-p.ix / p.pz, -p.iy / p.pz, jx[T + 2], jy[T + 2]);
        chain(-p.ix * p.ry / p.pz, -(p.rz + p.ry * p.iy) / p.pz, jx[T + 3], jy[T + 3]);
        chain((p.rz + p.rx * p.ix) / p.pz, p.rx * p.iy / p.pz, jx[T + 4], jy[T + 4]);
        chain(-p.ry / p.pz, p.rx / p.pz, jx[T + 5], jy[T + 5]);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            W.Jc_p[(size_t)(2 * j) * n + s] = jx[j];
            W.Jc_p[(size_t)(2 * j + 1) * n + s] = jy[j];
            W.Jc_c[(size_t)(2 * j) * n + cpos] = jx[j];
            W.Jc_c[(size_t)(2 * j + 1) * n + cpos] = jy[j];
        }
    }
    if (mode & BA_MODE_POINTS) {
        const bool constant = P.pt_const[pt] != 0;              /* a zero block (:334-338) */
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double jx, jy;
            chain((c[6 + k] - c[12 + k] * p.ix) / p.pz, (c[9 + k] - c[12 + k] * p.iy) / p.pz, jx, jy);
            W.Jp[(size_t)(2 * k) * n + s] = constant ? 0.0 : jx;
            W.Jp[(size_t)(2 * k + 1) * n + s] = constant ? 0.0 : jy;
        }
    }
}

/* ---- the point blocks: C = Jp^T Jp, w = -Jp^T F, the inverse of the regularised block (ba_linear_solver.cc:60-84,
 * :161-179), C^-1 w, and q = Jp C^-1 w per observation for the right-hand side v - E C^-1 w ---- */
__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_point_build(BaProblem P, BaParams S, BaWork W, double reg, int schur) {
    const int gid = (int)blockIdx.x * BA_CAM_BLOCK + (int)threadIdx.x;
    const int pt = gid / BA_POINT_LANES, lane = gid % BA_POINT_LANES;
    const bool valid = pt < P.n_pt;
    const int begin = valid ? P.pt_ptr[pt] : 0, end = valid ? P.pt_ptr[pt + 1] : 0;
    const size_t n = (size_t)P.n_obs, np = (size_t)P.n_pt;

    double a[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};    /* C00 C01 C02 C11 C12 C22 w0 w1 w2 */
    for (int s = begin + lane; s < end; s += BA_POINT_LANES) {
        double jx[3], jy[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { jx[k] = W.Jp[(size_t)(2 * k) * n + s]; jy[k] = W.Jp[(size_t)(2 * k + 1) * n + s]; }
        const double fx = S.F[s], fy = S.F[n + s];
        a[0] += jx[0] * jx[0] + jy[0] * jy[0];
        a[1] += jx[0] * jx[1] + jy[0] * jy[1];
        a[2] += jx[0] * jx[2] + jy[0] * jy[2];
        a[3] += jx[1] * jx[1] + jy[1] * jy[1];
        a[4] += jx[1] * jx[2] + jy[1] * jy[2];
        a[5] += jx[2] * jx[2] + jy[2] * jy[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) a[6 + k] -= jx[k] * fx + jy[k] * fy;
    }
    point_sum<9>(a);

    const double d0 = a[0], d1 = a[3], d2 = a[5];
    const double c00 = a[0] * reg, c11 = a[3] * reg, c22 = a[5] * reg, c01 = a[1], c02 = a[2], c12 = a[4];
    /* determinant and adjugate; a block whose determinant is within +-MATH_DBL_EPS (DBL_MIN * 1e58) of zero stays as it is */
    const double m00 = c11 * c22 - c12 * c12, m01 = c02 * c12 - c01 * c22, m02 = c01 * c12 - c02 * c11;
    const double det = c00 * m00 + c01 * m01 + c02 * m02;
    double i00 = c00, i01 = c01, i02 = c02, i11 = c11, i12 = c12, i22 = c22;
    if (!(det >= -2.2250738585072014e-250 && det <= 2.2250738585072014e-250)) {
        i00 = m00 / det; i01 = m01 / det; i02 = m02 / det;
        i11 = (c00 * c22 - c02 * c02) / det;
        i12 = (c01 * c02 - c00 * c12) / det;
        i22 = (c00 * c11 - c01 * c01) / det;
    }
    const double u0 = i00 * a[6] + i01 * a[7] + i02 * a[8];
    const double u1 = i01 * a[6] + i11 * a[7] + i12 * a[8];
    const double u2 = i02 * a[6] + i12 * a[7] + i22 * a[8];
    if (valid && lane == 0) {
        W.Cinv[pt] = i00; W.Cinv[np + pt] = i01; W.Cinv[2 * np + pt] = i02;
        W.Cinv[3 * np + pt] = i11; W.Cinv[4 * np + pt] = i12; W.Cinv[5 * np + pt] = i22;
        W.Cdiag[pt] = d0; W.Cdiag[np + pt] = d1; W.Cdiag[2 * np + pt] = d2;
        W.w[pt] = a[6]; W.w[np + pt] = a[7]; W.w[2 * np + pt] = a[8];
        W.dz[pt] = u0; W.dz[np + pt] = u1; W.dz[2 * np + pt] = u2;           /* the whole step of BA_MODE_POINTS (:295-302) */
    }
    if (!schur) return;
    for (int s = begin + lane; s < end; s += BA_POINT_LANES) {
        const int cpos = P.s_cpos[s];
        W.q[cpos] = W.Jp[s] * u0 + W.Jp[2 * n + s] * u1 + W.Jp[4 * n + s] * u2;
        W.q[n + cpos] = W.Jp[n + s] * u0 + W.Jp[3 * n + s] * u1 + W.Jp[5 * n + s] * u2;
    }
}

/* ---- the camera blocks: B = Jc^T Jc, v = -Jc^T F, the right-hand side, the preconditioner (ba_linear_solver.cc:29-54,
 * :159-190, :253-268) and the first search direction (ba_conjugate_gradient.h:143-164).  One workgroup per camera. ---- */
template <int D>
__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_cam_build(BaProblem P, BaWork W, double reg, int schur) {
    constexpr int NB = D * (D + 1) / 2, N = NB + 2 * D;
    __shared__ double lds[WAVES * N];
    __shared__ double A[D * D], L[D * D], Li[D * D];
    const int cam = blockIdx.x, tid = threadIdx.x;
    const int begin = P.cam_ptr[cam], end = P.cam_ptr[cam + 1];
    const size_t n = (size_t)P.n_obs;

    double a[N];
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = 0.0;
    for (int i = begin + tid; i < end; i += BA_CAM_BLOCK) {
        double jx[D], jy[D];
#pragma unroll
        for (int j = 0; j < D; ++j) { jx[j] = W.Jc_c[(size_t)(2 * j) * n + i]; jy[j] = W.Jc_c[(size_t)(2 * j + 1) * n + i]; }
        const double fx = W.F_c[i], fy = W.F_c[n + i];
        const double qx = schur ? W.q[i] : 0.0, qy = schur ? W.q[n + i] : 0.0;
        int k = 0;
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int l = j; l < D; ++l) a[k++] += jx[j] * jx[l] + jy[j] * jy[l];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            a[NB + j] -= jx[j] * fx + jy[j] * fy;
            a[NB + D + j] += jx[j] * qx + jy[j] * qy;
        }
    }
    block_sum<N>(a, lds);
    if (tid != 0) return;

    double* B = W.B + (size_t)cam * D * D;
    double* Pc = W.P + (size_t)cam * D * D;
    {
        int k = 0;
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int l = j; l < D; ++l) { A[j * D + l] = a[k]; A[l * D + j] = a[k]; ++k; }
    }
    for (int j = 0; j < D; ++j) {
        W.Bdiag[(size_t)cam * D + j] = A[j * D + j];
        A[j * D + j] *= reg;
    }
    for (int k = 0; k < D * D; ++k) B[k] = A[k];

    if (schur) {
        /* the Cholesky inverse L^-T L^-1 of the block, entries that are not finite set to 0 (ba_cholesky.h:59-131) */
        for (int r = 0; r < D; ++r) {
            for (int c = 0; c < r; ++c) {
                double sum = 0.0;
                for (int ci = 0; ci < c; ++ci) sum += L[r * D + ci] * L[c * D + ci];
                L[r * D + c] = (A[r * D + c] - sum) / L[c * D + c];
            }
            double sum = 0.0;
            for (int c = 0; c < r; ++c) sum += L[r * D + c] * L[r * D + c];
            L[r * D + r] = sqrt(fmax(0.0, A[r * D + r] - sum));
            for (int c = r + 1; c < D; ++c) L[r * D + c] = 0.0;
        }
        for (int r = 0; r < D; ++r) {
            for (int c = 0; c < r; ++c) {
                double sum = 0.0;
                for (int ci = 0; ci < r; ++ci) sum -= L[r * D + ci] * Li[ci * D + c];
                Li[r * D + c] = sum / L[r * D + r];
            }
            Li[r * D + r] = 1.0 / L[r * D + r];
            for (int c = r + 1; c < D; ++c) Li[r * D + c] = 0.0;
        }
        for (int r = 0; r < D; ++r)
            for (int c = 0; c < D; ++c) {
                double sum = 0.0;
                for (int k = 0; k < D; ++k) sum += Li[k * D + r] * Li[k * D + c];
                Pc[r * D + c] = isfinite(sum) ? sum : 0.0;
            }
    } else {
        /* BA_MODE_CAMERAS: the reciprocal diagonal */
        for (int r = 0; r < D; ++r)
            for (int c = 0; c < D; ++c) Pc[r * D + c] = r == c ? 1.0 / A[r * D + r] : 0.0;
    }

    /* x = 0, r = rhs, z = P r, d = z, and this camera's share of z . r */
    double r0[D], part = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        W.v[(size_t)cam * D + j] = a[NB + j];
        r0[j] = a[NB + j] - a[NB + D + j];
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double z = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) z += Pc[j * D + k] * r0[k];
        W.x[(size_t)cam * D + j] = 0.0;
        W.r[(size_t)cam * D + j] = r0[j];
        W.d[(size_t)cam * D + j] = z;
        part += z * r0[j];
    }
    W.cam_part[cam] = part;
}

__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_cg_init(BaProblem P, BaWork W) {
    __shared__ double lds[WAVES];
    double sum[1] = {0.0};
    for (int i = threadIdx.x; i < P.n_cam; i += BA_CAM_BLOCK) sum[0] += W.cam_part[i];
    block_sum<1>(sum, lds);
    if (threadIdx.x == 0) {
        W.sc->rz = sum[0];
        W.sc->rr = 0.0; W.sc->alpha = 0.0; W.sc->beta = 0.0;
        W.sc->iter = 0; W.sc->done = 0;
    }
}

/* ---- S d, first half: per point  t = sum Jp^T (Jc vec[camera]).  As a CG pass: q = Jp (C^-1 t) per observation, by cpos.
 * As the back substitution (BACK, vec = the camera step): dz = C^-1 (w - t) (ba_linear_solver.cc:221). ---- */
template <int D, bool BACK>
__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_point_pass(BaProblem P, BaWork W, const double* vec) {
    if (!BACK && W.sc->done) return;
    const int gid = (int)blockIdx.x * BA_CAM_BLOCK + (int)threadIdx.x;
    const int pt = gid / BA_POINT_LANES, lane = gid % BA_POINT_LANES;
    const bool valid = pt < P.n_pt;
    const int begin = valid ? P.pt_ptr[pt] : 0, end = valid ? P.pt_ptr[pt + 1] : 0;
    const size_t n = (size_t)P.n_obs, np = (size_t)P.n_pt;

    double t[3] = {0.0, 0.0, 0.0};
    for (int s = begin + lane; s < end; s += BA_POINT_LANES) {
        const double* dv = vec + (size_t)P.s_cam[s] * D;
        double ex = 0.0, ey = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            ex += W.Jc_p[(size_t)(2 * j) * n + s] * dv[j];
            ey += W.Jc_p[(size_t)(2 * j + 1) * n + s] * dv[j];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] += W.Jp[(size_t)(2 * k) * n + s] * ex + W.Jp[(size_t)(2 * k + 1) * n + s] * ey;
    }
    point_sum<3>(t);
    if (!valid) return;
    if (BACK) {
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = W.w[k * np + pt] - t[k];
    }
    const double i00 = W.Cinv[pt], i01 = W.Cinv[np + pt], i02 = W.Cinv[2 * np + pt];
    const double i11 = W.Cinv[3 * np + pt], i12 = W.Cinv[4 * np + pt], i22 = W.Cinv[5 * np + pt];
    const double u0 = i00 * t[0] + i01 * t[1] + i02 * t[2];
    const double u1 = i01 * t[0] + i11 * t[1] + i12 * t[2];
    const double u2 = i02 * t[0] + i12 * t[1] + i22 * t[2];
    if (BACK) {
        if (lane == 0) { W.dz[pt] = u0; W.dz[np + pt] = u1; W.dz[2 * np + pt] = u2; }
        return;
    }
    for (int s = begin + lane; s < end; s += BA_POINT_LANES) {
        const int cpos = P.s_cpos[s];
        W.q[cpos] = W.Jp[s] * u0 + W.Jp[2 * n + s] * u1 + W.Jp[4 * n + s] * u2;
        W.q[n + cpos] = W.Jp[n + s] * u0 + W.Jp[3 * n + s] * u1 + W.Jp[5 * n + s] * u2;
    }
}

/* ---- S d, second half: per camera  Ad = B d - sum Jc^T q  and the camera's share of d . Ad ---- */
template <int D>
__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_cam_pass(BaProblem P, BaWork W, int schur) {
    __shared__ double lds[WAVES * D];
    __shared__ double prod[D];
    if (W.sc->done) return;
    const int cam = blockIdx.x, tid = threadIdx.x;
    const size_t n = (size_t)P.n_obs;
    double e[D];
#pragma unroll
    for (int j = 0; j < D; ++j) e[j] = 0.0;
    if (schur) {
        const int begin = P.cam_ptr[cam], end = P.cam_ptr[cam + 1];
        for (int i = begin + tid; i < end; i += BA_CAM_BLOCK) {
            const double qx = W.q[i], qy = W.q[n + i];
#pragma unroll
            for (int j = 0; j < D; ++j) e[j] += W.Jc_c[(size_t)(2 * j) * n + i] * qx + W.Jc_c[(size_t)(2 * j + 1) * n + i] * qy;
        }
        block_sum<D>(e, lds);
    }
    if (tid < D) {
        const double* B = W.B + (size_t)cam * D * D + (size_t)tid * D;
        const double* d = W.d + (size_t)cam * D;
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) sum += B[k] * d[k];
        double mine = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) mine = tid == j ? e[j] : mine;
        sum -= mine;
        W.Ad[(size_t)cam * D + tid] = sum;
        prod[tid] = d[tid] * sum;
    }
    __syncthreads();
    if (tid == 0) {
        double part = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) part += prod[j];
        W.cam_part[cam] = part;
    }
}

/* ---- the rest of a CG iteration (ba_conjugate_gradient.h:170-206), one workgroup over the n_cam * D entries ---- */
template <int D>
__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_cg_update(BaProblem P, BaWork W, int cg_max) {
    __shared__ double lds[WAVES];
    if (W.sc->done) return;
    const int tid = threadIdx.x, ne = P.n_cam * D;
    const double rz = W.sc->rz;
    const int iter = W.sc->iter;

    double sum[1] = {0.0};
    for (int i = tid; i < P.n_cam; i += BA_CAM_BLOCK) sum[0] += W.cam_part[i];
    block_sum<1>(sum, lds);
    const double alpha = rz / sum[0];

    sum[0] = 0.0;
    for (int e = tid; e < ne; e += BA_CAM_BLOCK) {
        W.x[e] += W.d[e] * alpha;
        const double r = W.r[e] - W.Ad[e] * alpha;
        W.r[e] = r;
        sum[0] += r * r;
    }
    block_sum<1>(sum, lds);                                     /* (its barriers also publish r to the workgroup) */
    const double rr = sum[0];
    if (rr < 1e-20) {                                           /* CG_CONVERGENCE: the iteration is not counted (:182-186) */
        if (tid == 0) { W.sc->alpha = alpha; W.sc->rr = rr; W.sc->done = 1; }
        return;
    }

    sum[0] = 0.0;
    for (int e = tid; e < ne; e += BA_CAM_BLOCK) {
        const int cam = e / D, j = e - cam * D;
        const double* Pc = W.P + (size_t)cam * D * D + (size_t)j * D;
        const double* r = W.r + (size_t)cam * D;
        double z = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) z += Pc[k] * r[k];
        W.z[e] = z;
        sum[0] += z * r[j];
    }
    block_sum<1>(sum, lds);
    const double beta = sum[0] / rz;
    for (int e = tid; e < ne; e += BA_CAM_BLOCK) W.d[e] = W.z[e] + W.d[e] * beta;
    if (tid == 0) {
        W.sc->alpha = alpha; W.sc->beta = beta; W.sc->rr = rr; W.sc->rz = sum[0];
        W.sc->iter = iter + 1;
        if (iter + 1 >= cg_max) W.sc->done = 1;                 /* CG_MAX_ITERATIONS */
    }
}

/* ---- predicted_error_decrease (ba_linear_solver.cc:236-240, :309-310): the camera part, then the point part ---- */
template <int D>
__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_pred(BaProblem P, BaWork W, double inv_radius, int mode) {
    __shared__ double lds[WAVES * 2];
    double sum[2] = {0.0, 0.0};
    if (mode & BA_MODE_CAMERAS)
        for (int e = threadIdx.x; e < P.n_cam * D; e += BA_CAM_BLOCK)
            sum[0] += W.x[e] * (W.Bdiag[e] * W.x[e] * inv_radius + W.v[e]);
    if (mode & BA_MODE_POINTS)
        for (int e = threadIdx.x; e < 3 * P.n_pt; e += BA_CAM_BLOCK)
            sum[1] += W.dz[e] * (W.Cdiag[e] * W.dz[e] * inv_radius + W.w[e]);
    block_sum<2>(sum, lds);
    if (threadIdx.x == 0) W.sc->pred = sum[0] + sum[1];
}

/* ---- the candidate set: update_camera / update_point (bundle_adjustment.cc:662-697); what the mode does not move is copied ---- */
template <int D>
__global__ __launch_bounds__(BA_CAM_BLOCK) void k_ba_update(BaProblem P, BaParams cur, BaParams cand, BaWork W, int mode) {
    const int i = (int)blockIdx.x * BA_CAM_BLOCK + (int)threadIdx.x;
    if (i < P.n_cam) {
        const double* c = cur.cam + (size_t)i * BA_CAM_DOUBLES;
        double* o = cand.cam + (size_t)i * BA_CAM_DOUBLES;
        if (mode & BA_MODE_CAMERAS) {
            const double* u = W.x + (size_t)i * D;
            constexpr int T = D - 6;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = D == 9 ? c[k] + u[k] : c[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) o[3 + k] = c[3 + k] + u[T + k];
            double m[9];
            rodrigues(u + T + 3, m);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    o[6 + 3 * r + k] = m[3 * r] * c[6 + k] + m[3 * r + 1] * c[9 + k] + m[3 * r + 2] * c[12 + k];
        } else {
#pragma unroll
            for (int k = 0; k < BA_CAM_DOUBLES; ++k) o[k] = c[k];
        }
    }
    if (i < P.n_pt) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t e = (size_t)k * P.n_pt + i;
            cand.pt[e] = (mode & BA_MODE_POINTS) ? cur.pt[e] + W.dz[e] : cur.pt[e];
        }
    }
}

unsigned blocks_for(int n) { return (unsigned)((n + BA_CAM_BLOCK - 1) / BA_CAM_BLOCK); }

template <int D>
void build(const BaStep& st, const BaProblem& p, const BaParams& cur, const BaWork& w, bool jacobian) {
    const double reg = 1.0 + 1.0 / st.radius;
    const int schur = st.mode == (BA_MODE_CAMERAS | BA_MODE_POINTS);
    if (jacobian) hipLaunchKernelGGL(k_ba_jacobian<D>, dim3(blocks_for(p.n_obs)), dim3(BA_CAM_BLOCK), 0, st.stream, p, cur, w, (int)st.mode);
    if (st.mode & BA_MODE_POINTS)
        hipLaunchKernelGGL(k_ba_point_build, dim3(blocks_for(p.n_pt * BA_POINT_LANES)), dim3(BA_CAM_BLOCK), 0, st.stream, p, cur, w, reg, schur);
    if (st.mode & BA_MODE_CAMERAS) {
        hipLaunchKernelGGL(k_ba_cam_build<D>, dim3((unsigned)p.n_cam), dim3(BA_CAM_BLOCK), 0, st.stream, p, w, reg, schur);
        hipLaunchKernelGGL(k_ba_cg_init, dim3(1), dim3(BA_CAM_BLOCK), 0, st.stream, p, w);
    }
}

template <int D>
void cg(const BaStep& st, const BaProblem& p, const BaWork& w, int32_t n) {
    const int schur = st.mode == (BA_MODE_CAMERAS | BA_MODE_POINTS);
    for (int32_t i = 0; i < n; ++i) {
        if (schur)
            hipLaunchKernelGGL((k_ba_point_pass<D, false>), dim3(blocks_for(p.n_pt * BA_POINT_LANES)), dim3(BA_CAM_BLOCK), 0, st.stream, p, w,
                               (const double*)w.d);
        hipLaunchKernelGGL(k_ba_cam_pass<D>, dim3((unsigned)p.n_cam), dim3(BA_CAM_BLOCK), 0, st.stream, p, w, schur);
        hipLaunchKernelGGL(k_ba_cg_update<D>, dim3(1), dim3(BA_CAM_BLOCK), 0, st.stream, p, w, (int)st.cg_max);
    }
}

template <int D>
void finish(const BaStep& st, const BaProblem& p, const BaParams& cur, const BaParams& cand, const BaWork& w) {
    if (st.mode == (BA_MODE_CAMERAS | BA_MODE_POINTS))
        hipLaunchKernelGGL((k_ba_point_pass<D, true>), dim3(blocks_for(p.n_pt * BA_POINT_LANES)), dim3(BA_CAM_BLOCK), 0, st.stream, p, w,
                           (const double*)w.x);
    hipLaunchKernelGGL(k_ba_pred<D>, dim3(1), dim3(BA_CAM_BLOCK), 0, st.stream, p, w, 1.0 / st.radius, (int)st.mode);
    hipLaunchKernelGGL(k_ba_update<D>, dim3(blocks_for(p.n_cam > p.n_pt ? p.n_cam : p.n_pt)), dim3(BA_CAM_BLOCK), 0, st.stream, p, cur, cand, w,
                       (int)st.mode);
    mi_ba_launch_residual(st.stream, p, cand, w);
}

}  /* namespace */

void mi_ba_launch_residual(hipStream_t s, const BaProblem& p, const BaParams& set, const BaWork& w) {
    hipLaunchKernelGGL(k_ba_residual, dim3(blocks_for(p.n_obs)), dim3(BA_CAM_BLOCK), 0, s, p, set, w);
    hipLaunchKernelGGL(k_ba_total, dim3(1), dim3(BA_CAM_BLOCK), 0, s, (const double*)w.blk_part, (int)blocks_for(p.n_obs), (double)p.n_obs,
                       &w.sc->mse);
}

void mi_ba_launch_build(const BaStep& st, const BaProblem& p, const BaParams& cur, const BaWork& w, bool jacobian) {
    if (st.dim == 9) build<9>(st, p, cur, w, jacobian); else build<6>(st, p, cur, w, jacobian);
}

void mi_ba_launch_cg(const BaStep& st, const BaProblem& p, const BaWork& w, int32_t n) {
    if (st.dim == 9) cg<9>(st, p, w, n); else cg<6>(st, p, w, n);
}

void mi_ba_launch_finish(const BaStep& st, const BaProblem& p, const BaParams& cur, const BaParams& cand, const BaWork& w) {
    if (st.dim == 9) finish<9>(st, p, cur, cand, w); else finish<6>(st, p, cur, cand, w);
}
