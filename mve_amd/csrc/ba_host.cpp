/*
 * ba_host.cpp -- mi_dmrecon_ba_optimize of include/mi_dmrecon.h: the Levenberg-Marquardt loop of
 * sfm::ba::BundleAdjustment::lm_optimize (libs/sfm/bundle_adjustment.cc:73-201) on the host, every sum of it in the kernels
 * of ba_device.hip.  Every index a kernel reads comes from the two lists built HERE out of ids that were checked here.
 * One upload, one small readback per batch of CG iterations and per LM iteration, one download at the end.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "host_common.h"
#include "ba_device.h"

/* CG iterations enqueued between two reads of the `done` flag (profiles/ba.md; a build with -DBA_CG_BATCH=n measures another) */
#ifndef BA_CG_BATCH
#define BA_CG_BATCH 16
#endif

namespace {

/* The buffers of a context's calls; they grow only and go with the context. */
struct BaState : HostModule {
    Buf d_mem;                               /* lists | two parameter sets | the work arrays of BaWork */
    PinnedBuf h_mem;                         /* the lists and the parameters as uploaded and downloaded */
    Buf d_sc;                                /* one BaScalars */
    PinnedBuf h_sc;
};

#define BA_MAX_ITEMS (1ll << 27)             /* observations / points / cameras of a call: BA_POINT_LANES * n_points and every slot stay inside int32 */

/* hands out 256-byte aligned pieces of one allocation */
struct Arena {
    size_t used = 0;
    size_t take(size_t bytes) { const size_t at = used; used += align256(bytes); return at; }
};

int validate(const mi_dmrecon_ba_options* o, int32_t nc, const mi_dmrecon_ba_camera* cams, int32_t np, const mi_dmrecon_ba_point* pts,
             int32_t no, const mi_dmrecon_ba_observation* obs, const mi_dmrecon_ba_status* status, const mi_dmrecon_ba_trace* trace,
             int32_t trace_capacity) {
    if (!o) return failf(MI_DMRECON_EINVAL, "ba: null options");
    if (!cams) return failf(MI_DMRECON_EINVAL, "ba: null cameras (No cameras given)");
    if (!pts) return failf(MI_DMRECON_EINVAL, "ba: null points (No tracks given)");
    if (!obs) return failf(MI_DMRECON_EINVAL, "ba: null observations (No observations given)");
    if (!status) return failf(MI_DMRECON_EINVAL, "ba: null status");
    if (trace_capacity < 0 || (trace_capacity > 0 && !trace)) return failf(MI_DMRECON_EINVAL, "ba: trace_capacity %lld without room for it", trace_capacity);
    if (o->bundle_mode < 1 || o->bundle_mode > 3) return failf(MI_DMRECON_EINVAL, "ba: bundle_mode %lld is not 1, 2 or 3 (Invalid bundle mode)", o->bundle_mode);
    if (o->lm_max_iterations < 1) return failf(MI_DMRECON_EINVAL, "ba: lm_max_iterations %lld, at least 1 required", o->lm_max_iterations);
    if (o->lm_min_iterations < 0) return failf(MI_DMRECON_EINVAL, "ba: lm_min_iterations %lld is negative", o->lm_min_iterations);
    if (o->cg_max_iterations < 1) return failf(MI_DMRECON_EINVAL, "ba: cg_max_iterations %lld, at least 1 required", o->cg_max_iterations);
    if (nc < 1 || np < 1 || no < 1 || nc > BA_MAX_ITEMS || np > BA_MAX_ITEMS || no > BA_MAX_ITEMS)
        return failf(MI_DMRECON_EINVAL, "ba: n_cameras, n_points and n_observations must each lie in 1 ... 2^27");
    for (int32_t i = 0; i < nc; ++i)
        if (!(cams[i].focal_length > 0.0)) return failf(MI_DMRECON_EINVAL, "ba: camera %lld has no positive focal length (Camera with invalid focal length)", i);
    for (int32_t i = 0; i < no; ++i) {
        if (obs[i].camera_id < 0 || obs[i].camera_id >= nc)
            return failf(MI_DMRECON_EINVAL, "ba: observation %lld has camera_id %lld (Observation with invalid camera ID)", i, obs[i].camera_id);
        if (obs[i].point_id < 0 || obs[i].point_id >= np)
            return failf(MI_DMRECON_EINVAL, "ba: observation %lld has point_id %lld (Observation with invalid track ID)", i, obs[i].point_id);
    }
    return 0;
}

int ba_impl(mi_dmrecon_ctx* ctx, const mi_dmrecon_ba_options* o, int32_t nc, mi_dmrecon_ba_camera* cams, int32_t np, mi_dmrecon_ba_point* pts,
            int32_t no, const mi_dmrecon_ba_observation* obs, mi_dmrecon_ba_status* status, mi_dmrecon_ba_trace* trace, int32_t trace_capacity) {
    if (!ctx) return failf(MI_DMRECON_EINVAL, "ba: null context");
    if (int rc = validate(o, nc, cams, np, pts, no, obs, status, trace, trace_capacity)) return rc;
    const int D = o->fixed_intrinsics ? 6 : 9;
    const size_t n = (size_t)no, ncam = (size_t)nc, npt = (size_t)np;

    /* the layout: what is uploaded first, in the order of the pinned mirror */
    Arena A;
    const size_t o_pt_ptr = A.take((npt + 1) * 4), o_cam_ptr = A.take((ncam + 1) * 4), o_s_cam = A.take(n * 4), o_s_pt = A.take(n * 4);
    const size_t o_s_cpos = A.take(n * 4), o_s_xy = A.take(2 * n * 8), o_const = A.take(npt * 4);
    const size_t o_cam0 = A.take(ncam * BA_CAM_DOUBLES * 8), o_pt0 = A.take(3 * npt * 8);
    const size_t upload = A.used;
    const size_t o_cam1 = A.take(ncam * BA_CAM_DOUBLES * 8), o_pt1 = A.take(3 * npt * 8);
    const size_t o_F0 = A.take(2 * n * 8), o_F1 = A.take(2 * n * 8);
    const size_t o_Jc_p = A.take(2 * D * n * 8), o_Jc_c = A.take(2 * D * n * 8), o_Jp = A.take(6 * n * 8);
    const size_t o_F_c = A.take(2 * n * 8), o_q = A.take(2 * n * 8);
    const size_t o_Cinv = A.take(6 * npt * 8), o_Cdiag = A.take(3 * npt * 8), o_w = A.take(3 * npt * 8), o_dz = A.take(3 * npt * 8);
    const size_t o_B = A.take(ncam * D * D * 8), o_P = A.take(ncam * D * D * 8);
    size_t o_vec[7];                                             /* Bdiag v x r d z Ad */
    for (size_t& at : o_vec) at = A.take(ncam * D * 8);
    const size_t o_cam_part = A.take(ncam * 8), o_blk = A.take(((n + BA_CAM_BLOCK - 1) / BA_CAM_BLOCK) * 8);

    MI_HIP(hipSetDevice(mi_host_ctx_device(ctx)));
    HostModule*& state = mi_host_ctx_module(ctx, MI_MODULE_BA);
    if (!state) state = new BaState();
    BaState& s = *static_cast<BaState*>(state);
    MI_HIP(s.d_sc.need(sizeof(BaScalars)));
    MI_HIP(s.h_sc.need(sizeof(BaScalars)));
    MI_HIP(s.d_mem.need(A.used));
    MI_HIP(s.h_mem.need(upload));
    hipStream_t stream = (hipStream_t)mi_dmrecon_ctx_stream(ctx);
    uint8_t* const h_mem = (uint8_t*)s.h_mem.p;
    BaScalars* const d_sc = (BaScalars*)s.d_sc.p;
    const BaScalars* const h_sc = (const BaScalars*)s.h_sc.p;

    /* two stable counting sorts: observations by point (slots), slots by camera (cpos) */
    int32_t* pt_ptr = (int32_t*)(h_mem + o_pt_ptr);
    int32_t* cam_ptr = (int32_t*)(h_mem + o_cam_ptr);
    int32_t* s_cam = (int32_t*)(h_mem + o_s_cam);
    int32_t* s_pt = (int32_t*)(h_mem + o_s_pt);
    int32_t* s_cpos = (int32_t*)(h_mem + o_s_cpos);
    double* s_xy = (double*)(h_mem + o_s_xy);
    std::fill(pt_ptr, pt_ptr + npt + 1, 0);
    std::fill(cam_ptr, cam_ptr + ncam + 1, 0);
    for (size_t i = 0; i < n; ++i) { ++pt_ptr[obs[i].point_id + 1]; ++cam_ptr[obs[i].camera_id + 1]; }
    for (size_t p = 0; p < npt; ++p) pt_ptr[p + 1] += pt_ptr[p];
    for (size_t c = 0; c < ncam; ++c) cam_ptr[c + 1] += cam_ptr[c];
    {
        std::vector<int32_t> next(pt_ptr, pt_ptr + npt);
        for (size_t i = 0; i < n; ++i) {
            const int32_t slot = next[obs[i].point_id]++;
            s_cam[slot] = obs[i].camera_id; s_pt[slot] = obs[i].point_id;
            s_xy[slot] = obs[i].pos[0]; s_xy[n + slot] = obs[i].pos[1];
        }
        next.assign(cam_ptr, cam_ptr + ncam);
        for (size_t slot = 0; slot < n; ++slot) s_cpos[slot] = next[s_cam[slot]]++;
    }
    int32_t* h_const = (int32_t*)(h_mem + o_const);
    double* h_cam = (double*)(h_mem + o_cam0);
    double* h_pt = (double*)(h_mem + o_pt0);
    for (size_t p = 0; p < npt; ++p) {
        h_const[p] = pts[p].is_constant != 0;
        for (int k = 0; k < 3; ++k) h_pt[k * npt + p] = pts[p].pos[k];
    }
    for (size_t c = 0; c < ncam; ++c) {
        double* q = h_cam + c * BA_CAM_DOUBLES;
        q[0] = cams[c].focal_length; q[1] = cams[c].distortion[0]; q[2] = cams[c].distortion[1];
        for (int k = 0; k < 3; ++k) q[3 + k] = cams[c].translation[k];
        for (int k = 0; k < 9; ++k) q[6 + k] = cams[c].rotation[k];
    }
    MI_HIP(hipMemcpyAsync(s.d_mem.p, h_mem, upload, hipMemcpyHostToDevice, stream));

    uint8_t* m = (uint8_t*)s.d_mem.p;
    BaProblem P;
    P.n_cam = nc; P.n_pt = np; P.n_obs = no;
    P.pt_ptr = (const int32_t*)(m + o_pt_ptr); P.cam_ptr = (const int32_t*)(m + o_cam_ptr);
    P.s_cam = (const int32_t*)(m + o_s_cam); P.s_pt = (const int32_t*)(m + o_s_pt); P.s_cpos = (const int32_t*)(m + o_s_cpos);
    P.s_xy = (const double*)(m + o_s_xy); P.pt_const = (const int32_t*)(m + o_const);
    BaParams cur{(double*)(m + o_cam0), (double*)(m + o_pt0), (double*)(m + o_F0)};
    BaParams cand{(double*)(m + o_cam1), (double*)(m + o_pt1), (double*)(m + o_F1)};
    BaWork W;
    W.Jc_p = (double*)(m + o_Jc_p); W.Jc_c = (double*)(m + o_Jc_c); W.Jp = (double*)(m + o_Jp); W.F_c = (double*)(m + o_F_c);
    W.q = (double*)(m + o_q); W.Cinv = (double*)(m + o_Cinv); W.Cdiag = (double*)(m + o_Cdiag); W.w = (double*)(m + o_w);
    W.dz = (double*)(m + o_dz); W.B = (double*)(m + o_B); W.P = (double*)(m + o_P);
    W.Bdiag = (double*)(m + o_vec[0]); W.v = (double*)(m + o_vec[1]); W.x = (double*)(m + o_vec[2]); W.r = (double*)(m + o_vec[3]);
    W.d = (double*)(m + o_vec[4]); W.z = (double*)(m + o_vec[5]); W.Ad = (double*)(m + o_vec[6]);
    W.cam_part = (double*)(m + o_cam_part); W.blk_part = (double*)(m + o_blk); W.sc = d_sc;

    auto read_scalars = [&]() -> hipError_t {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(s.h_sc.p, d_sc, sizeof(BaScalars), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        return e;
    };

    BaStep st;
    st.stream = stream; st.dim = D; st.mode = o->bundle_mode; st.cg_max = o->cg_max_iterations;
    st.radius = 1000.0;                                          /* TRUST_REGION_RADIUS_INIT */

    mi_ba_launch_residual(stream, P, cur, W);
    MI_HIP(read_scalars());
    double current_mse = h_sc->mse;
    mi_dmrecon_ba_status out;
    std::memset(&out, 0, sizeof(out));
    out.initial_mse = current_mse;
    out.final_mse = current_mse;

    bool jacobian = true;                                        /* the current set has no Jacobian yet */
    for (int lm_iter = 0;; ++lm_iter) {
        if (lm_iter + 1 > o->lm_min_iterations && current_mse < o->lm_mse_threshold) break;

        mi_ba_launch_build(st, P, cur, W, jacobian);
        jacobian = false;
        int32_t cg_iterations = 0;
        if (st.mode & BA_MODE_CAMERAS) {
            /* every batch is bounded, and so is the number of batches */
            for (int32_t enqueued = 0; enqueued < st.cg_max;) {
                const int32_t batch = std::min<int32_t>(BA_CG_BATCH, st.cg_max - enqueued);
                mi_ba_launch_cg(st, P, W, batch);
                enqueued += batch;
                MI_HIP(read_scalars());
                if (h_sc->done) break;
            }
            cg_iterations = h_sc->iter;
        }
        mi_ba_launch_finish(st, P, cur, cand, W);
        MI_HIP(read_scalars());

        /* (the reference's CG cannot fail on these inputs: its sizes always agree, ba_conjugate_gradient.h:126-130) */
        const double new_mse = h_sc->mse;
        const double delta_mse = current_mse - new_mse;
        const double delta_mse_ratio = 1.0 - new_mse / current_mse;
        out.num_cg_iterations += cg_iterations;
        const bool successful = delta_mse > 0.0;
        if (lm_iter < trace_capacity) {
            mi_dmrecon_ba_trace& t = trace[lm_iter];
            t.mse_before = current_mse; t.mse_after = new_mse; t.radius = st.radius;
            t.cg_iterations = cg_iterations; t.accepted = successful ? 1 : 0;
        }
        out.num_lm_iterations += 1;
        if (successful) {
            out.num_lm_successful_iterations += 1;
            std::swap(cur, cand);
            jacobian = true;
            current_mse = new_mse;
            const double gain_ratio = delta_mse * (double)no / h_sc->pred;
            const double c3 = 2.0 * gain_ratio - 1.0;
            st.radius *= 1.0 / std::max(1.0 / 3.0, 1.0 - c3 * c3 * c3);
        } else {
            out.num_lm_unsuccessful_iterations += 1;
            st.radius *= 0.5;                                    /* TRUST_REGION_RADIUS_DECREMENT */
        }

        if (lm_iter + 1 < o->lm_min_iterations) continue;
        if (lm_iter + 1 >= o->lm_max_iterations) break;
        if (successful && delta_mse_ratio < o->lm_delta_threshold) break;
    }
    out.final_mse = current_mse;

    /* the current set comes back through the pinned mirror */
    MI_HIP(hipMemcpyAsync(h_cam, cur.cam, ncam * BA_CAM_DOUBLES * 8, hipMemcpyDeviceToHost, stream));
    MI_HIP(hipMemcpyAsync(h_pt, cur.pt, 3 * npt * 8, hipMemcpyDeviceToHost, stream));
    MI_HIP(hipStreamSynchronize(stream));
    for (size_t c = 0; c < ncam; ++c) {
        const double* q = h_cam + c * BA_CAM_DOUBLES;
        cams[c].focal_length = q[0]; cams[c].distortion[0] = q[1]; cams[c].distortion[1] = q[2];
        for (int k = 0; k < 3; ++k) cams[c].translation[k] = q[3 + k];
        for (int k = 0; k < 9; ++k) cams[c].rotation[k] = q[6 + k];
    }
    for (size_t p = 0; p < npt; ++p)
        for (int k = 0; k < 3; ++k) pts[p].pos[k] = h_pt[k * npt + p];
    *status = out;
    return 0;
}

}  /* namespace */

extern "C" {

void mi_dmrecon_ba_options_default(mi_dmrecon_ba_options* o) {
    if (!o) return;
    o->bundle_mode = MI_DMRECON_BA_CAMERAS_AND_POINTS;
    o->fixed_intrinsics = 0;
    o->lm_max_iterations = 50;
    o->lm_min_iterations = 0;
    o->lm_delta_threshold = 1e-4;
    o->lm_mse_threshold = 1e-8;
    o->cg_max_iterations = 1000;
    o->reserved = 0;
}

int mi_dmrecon_ba_optimize(mi_dmrecon_ctx* ctx, const mi_dmrecon_ba_options* options, int32_t n_cameras, mi_dmrecon_ba_camera* cameras,
                           int32_t n_points, mi_dmrecon_ba_point* points, int32_t n_observations,
                           const mi_dmrecon_ba_observation* observations, mi_dmrecon_ba_status* status, mi_dmrecon_ba_trace* trace,
                           int32_t trace_capacity) {
    return guarded([&] { return ba_impl(ctx, options, n_cameras, cameras, n_points, points, n_observations, observations, status, trace, trace_capacity); });
}

}  /* extern "C" */
