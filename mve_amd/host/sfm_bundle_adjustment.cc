/*
 * sfm_bundle_adjustment.cc -- every member of sfm::ba::BundleAdjustment that the reference defines in
 * libs/sfm/bundle_adjustment.cc, on top of libmi_dmrecon.so: linked INSTEAD of that one file, with the rest of libs/sfm and
 * apps/sfmrecon unmodified (mve_amd/host/Makefile, build/sfmrecon_mi).  Compiled against the reference's own
 * sfm/bundle_adjustment.h (the class is the reference's; only these definitions are ours).
 *
 * Behaviour kept from the reference (libs/sfm/bundle_adjustment.cc):
 *   :44-70    the sanity checks with their exception texts,
 *   :93, :142-148, :165-171, :183-194  the verbose lines (here: after the call, from the trace of LM iterations),
 *   :37-40    status is reset, filled and returned, runtime_ms included,
 *   :700-725  print_status.
 * What differs: the whole optimisation runs on the GPU in one mi_dmrecon_ba_optimize call; the results agree with the
 * reference's to rounding and to where its CG stops, not bit for bit (include/mi_dmrecon.h).  The private helpers have no
 * other caller in the reference and throw std::logic_error.
 *
 * One context for the process, shared with every other drop-in of this directory that the binary links (shim_common.h): made
 * by the first call of any of them on the first entry of MI_DMRECON_DEVICES (default 0); every calling thread works on its
 * own fork (its own stream and buffers); all are released at exit.
 */
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <iomanip>
#include <iostream>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "util/timer.h"
#include "sfm/bundle_adjustment.h"

#include "shim_common.h"

#define LOG_V this->log.verbose()

SFM_NAMESPACE_BEGIN
SFM_BA_NAMESPACE_BEGIN

BundleAdjustment::Status
BundleAdjustment::optimize (void)
{
    util::WallTimer timer;
    this->sanity_checks();
    this->status = Status();
    this->lm_optimize();
    this->status.runtime_ms = timer.get_elapsed();
    return this->status;
}

void
BundleAdjustment::sanity_checks (void)
{
    if (this->cameras == nullptr)
        throw std::invalid_argument("No cameras given");
    if (this->points == nullptr)
        throw std::invalid_argument("No tracks given");
    if (this->observations == nullptr)
        throw std::invalid_argument("No observations given");
    for (std::size_t i = 0; i < this->cameras->size(); ++i)
        if (this->cameras->at(i).focal_length <= 0.0)
            throw std::invalid_argument("Camera with invalid focal length");
    for (std::size_t i = 0; i < this->observations->size(); ++i)
    {
        Observation const& obs = this->observations->at(i);
        if (obs.camera_id < 0 || obs.camera_id >= static_cast<int>(this->cameras->size()))
            throw std::invalid_argument("Observation with invalid camera ID");
        if (obs.point_id < 0 || obs.point_id >= static_cast<int>(this->points->size()))
            throw std::invalid_argument("Observation with invalid track ID");
    }
}

void
BundleAdjustment::lm_optimize (void)
{
    if (this->opts.bundle_mode < BA_CAMERAS || this->opts.bundle_mode > BA_CAMERAS_AND_POINTS)
        throw std::runtime_error("Invalid bundle mode");

    mi_dmrecon_ba_options o;
    mi_dmrecon_ba_options_default(&o);
    o.bundle_mode = this->opts.bundle_mode;
    o.fixed_intrinsics = this->opts.fixed_intrinsics ? 1 : 0;
    o.lm_max_iterations = std::max(1, this->opts.lm_max_iterations);   /* the reference runs one iteration whatever the limit */
    o.lm_min_iterations = std::max(0, this->opts.lm_min_iterations);
    o.lm_delta_threshold = this->opts.lm_delta_threshold;
    o.lm_mse_threshold = this->opts.lm_mse_threshold;
    o.cg_max_iterations = this->opts.linear_opts.cg_max_iterations;

    static_assert(sizeof(Observation) == sizeof(mi_dmrecon_ba_observation), "an observation is pos[2], camera_id, point_id");
    std::vector<mi_dmrecon_ba_camera> cams(this->cameras->size());
    std::vector<mi_dmrecon_ba_point> pts(this->points->size());
    for (std::size_t i = 0; i < cams.size(); ++i)
    {
        Camera const& c = this->cameras->at(i);
        cams[i].focal_length = c.focal_length;
        std::copy(c.distortion, c.distortion + 2, cams[i].distortion);
        std::copy(c.translation, c.translation + 3, cams[i].translation);
        std::copy(c.rotation, c.rotation + 9, cams[i].rotation);
    }
    for (std::size_t i = 0; i < pts.size(); ++i)
    {
        Point3D const& p = this->points->at(i);
        std::copy(p.pos, p.pos + 3, pts[i].pos);
        pts[i].is_constant = p.is_constant ? 1 : 0;
        pts[i].reserved = 0;
    }

    int const capacity = std::max(o.lm_max_iterations, o.lm_min_iterations);
    std::vector<mi_dmrecon_ba_trace> trace(capacity);
    mi_dmrecon_ba_status st;
    mi_shim::check(mi_dmrecon_ba_optimize(mi_shim::context_of_this_thread("sfm::ba::BundleAdjustment"), &o, static_cast<int32_t>(cams.size()), cams.data(),
        static_cast<int32_t>(pts.size()), pts.data(), static_cast<int32_t>(this->observations->size()),
        reinterpret_cast<mi_dmrecon_ba_observation const*>(this->observations->data()), &st, trace.data(), capacity),
        "mi_dmrecon_ba_optimize");

    for (std::size_t i = 0; i < cams.size(); ++i)
    {
        Camera& c = this->cameras->at(i);
        c.focal_length = cams[i].focal_length;
        std::copy(cams[i].distortion, cams[i].distortion + 2, c.distortion);
        std::copy(cams[i].translation, cams[i].translation + 3, c.translation);
        std::copy(cams[i].rotation, cams[i].rotation + 9, c.rotation);
    }
    for (std::size_t i = 0; i < pts.size(); ++i)
        std::copy(pts[i].pos, pts[i].pos + 3, this->points->at(i).pos);

    this->status.initial_mse = st.initial_mse;
    this->status.final_mse = st.final_mse;
    this->status.num_lm_iterations = st.num_lm_iterations;
    this->status.num_lm_successful_iterations = st.num_lm_successful_iterations;
    this->status.num_lm_unsuccessful_iterations = st.num_lm_unsuccessful_iterations;
    this->status.num_cg_iterations = st.num_cg_iterations;

    /* the verbose lines, in the reference's words and order */
    bool ended = false;
    for (int i = 0; i < st.num_lm_iterations; ++i)
    {
        mi_dmrecon_ba_trace const& t = trace[i];
        if (t.accepted)
            LOG_V << "BA: #" << std::setw(2) << std::left << i << " success" << std::right
                << ", MSE " << std::setw(11) << t.mse_before << " -> " << std::setw(11) << t.mse_after
                << ", CG " << std::setw(3) << t.cg_iterations << ", TRR " << t.radius << std::endl;
        else
            LOG_V << "BA: #" << std::setw(2) << std::left << i << " failure" << std::right
                << ", MSE " << std::setw(11) << t.mse_before << ",    " << std::setw(11) << " "
                << " CG " << std::setw(3) << t.cg_iterations << ", TRR " << t.radius << std::endl;
        if (i + 1 < st.num_lm_iterations || i + 1 < o.lm_min_iterations)
            continue;
        if (i + 1 >= o.lm_max_iterations)
        {
            LOG_V << "BA: Reached maximum LM iterations of " << this->opts.lm_max_iterations << std::endl;
            ended = true;
        }
        else if (t.accepted && 1.0 - t.mse_after / t.mse_before < o.lm_delta_threshold)
        {
            LOG_V << "BA: Satisfied delta mse ratio threshold of " << this->opts.lm_delta_threshold << std::endl;
            ended = true;
        }
    }
    if (!ended)                                                 /* the only other way out of the loop (:90-95) */
        LOG_V << "BA: Satisfied MSE threshold." << std::endl;
}

void
BundleAdjustment::print_status (bool detailed) const
{
    if (!detailed)
    {
        std::cout << "BA: MSE " << this->status.initial_mse
            << " -> " << this->status.final_mse << ", "
            << this->status.num_lm_iterations << " LM iters, "
            << this->status.num_cg_iterations << " CG iters, "
            << this->status.runtime_ms << "ms."
            << std::endl;
        return;
    }

    std::cout << "Bundle Adjustment Status:" << std::endl;
    std::cout << "  Initial MSE: " << this->status.initial_mse << std::endl;
    std::cout << "  Final MSE: " << this->status.final_mse << std::endl;
    std::cout << "  LM iterations: " << this->status.num_lm_iterations << " ("
        << this->status.num_lm_successful_iterations << " successful, "
        << this->status.num_lm_unsuccessful_iterations << " unsuccessful)" << std::endl;
    std::cout << "  CG iterations: " << this->status.num_cg_iterations << std::endl;
}

/* ---- the private helpers of the reference's CPU path: the kernels of mve_amd/csrc/ba_device.hip do their work ---- */

#define BA_NO_CPU_PATH(what) throw std::logic_error("sfm::ba::BundleAdjustment::" what " (MI355X build): computed on the GPU by optimize")

void
BundleAdjustment::compute_reprojection_errors (DenseVectorType* /*vector_f*/, DenseVectorType const* /*delta_x*/)
{
    BA_NO_CPU_PATH("compute_reprojection_errors");
}

double
BundleAdjustment::compute_mse (DenseVectorType const& /*vector_f*/)
{
    BA_NO_CPU_PATH("compute_mse");
}

void
BundleAdjustment::radial_distort (double* /*x*/, double* /*y*/, double const* /*dist*/)
{
    BA_NO_CPU_PATH("radial_distort");
}

void
BundleAdjustment::rodrigues_to_matrix (double const* /*r*/, double* /*rot*/)
{
    BA_NO_CPU_PATH("rodrigues_to_matrix");
}

void
BundleAdjustment::analytic_jacobian (SparseMatrixType* /*jac_cam*/, SparseMatrixType* /*jac_points*/)
{
    BA_NO_CPU_PATH("analytic_jacobian");
}

void
BundleAdjustment::analytic_jacobian_entries (Camera const& /*cam*/, Point3D const& /*point*/,
    double* /*cam_x_ptr*/, double* /*cam_y_ptr*/, double* /*point_x_ptr*/, double* /*point_y_ptr*/)
{
    BA_NO_CPU_PATH("analytic_jacobian_entries");
}

void
BundleAdjustment::update_parameters (DenseVectorType const& /*delta_x*/)
{
    BA_NO_CPU_PATH("update_parameters");
}

void
BundleAdjustment::update_camera (Camera const& /*cam*/, double const* /*update*/, Camera* /*out*/)
{
    BA_NO_CPU_PATH("update_camera");
}

void
BundleAdjustment::update_point (Point3D const& /*pt*/, double const* /*update*/, Point3D* /*out*/)
{
    BA_NO_CPU_PATH("update_point");
}

SFM_BA_NAMESPACE_END
SFM_NAMESPACE_END
