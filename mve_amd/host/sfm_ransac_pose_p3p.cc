/*
 * sfm_ransac_pose_p3p.cc -- the four members of sfm::RansacPoseP3P that the reference defines in
 * libs/sfm/ransac_pose_p3p.cc (the constructor, estimate, compute_p3p, find_inliers), on top of libmi_dmrecon.so: linked
 * INSTEAD of that one file, with the rest of libs/sfm (pose_p3p.cc included) and apps/sfmrecon unmodified
 * (mve_amd/host/Makefile, build/sfmrecon_mi).  Compiled against the reference's own sfm/ransac_pose_p3p.h.
 *
 * Behaviour kept from the reference (libs/sfm/ransac_pose_p3p.cc):
 *   :30-35    the verbose header line; :67-73 one verbose line per improving hypothesis (here: after the call, from the
 *             per-hypothesis counts; the iteration printed is hypothesis / 4),
 *   :85-86    fewer than 3 correspondences: std::invalid_argument("At least 3 correspondences required"),
 *   :89-91    the draws: util::system::rand_int() % corresp.size() into a std::set until it holds 3 -- made for all
 *             max_iterations iterations up front (ransac_shim.h),
 *   :61-65    result is written only by a pose with MORE inliers than result->inliers holds on entry.
 * What differs: Kneip's solves and the reprojection tests of all iterations run on the GPU (mi_dmrecon_ransac_pose_three_point);
 * the pose and the inlier set agree with the reference's to rounding, not bit for bit (include/mi_dmrecon.h).
 * The reference's loop is an OpenMP loop (:41-46): which thread draws which sample, and which of two poses with equally
 * many inliers reaches the critical section first, depend on the thread schedule.  This shim reproduces the SINGLE-THREAD
 * order: iteration i uses the i-th draws, and the winner is the first hypothesis 4 * iteration + root with the most inliers.
 * The context and its forks: shim_common.h.
 */
#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "sfm/ransac_pose_p3p.h"

#include "ransac_shim.h"

SFM_NAMESPACE_BEGIN

RansacPoseP3P::RansacPoseP3P (Options const& options)
    : opts(options)
{
}

void
RansacPoseP3P::estimate (Correspondences2D3D const& corresp,
    math::Matrix<double, 3, 3> const& k_matrix, Result* result) const
{
    if (this->opts.verbose_output)
    {
        std::cout << "RANSAC-3: Running for " << this->opts.max_iterations
            << " iterations, threshold " << this->opts.threshold
            << "..." << std::endl;
    }
    if (this->opts.max_iterations < 1)
        return;
    if (corresp.size() < 3)
        throw std::invalid_argument("At least 3 correspondences required");

    static_assert(sizeof(Correspondence2D3D) == 5 * sizeof(double), "a correspondence is p3d.x p3d.y p3d.z p2d.x p2d.y");
    static_assert(sizeof(int) == sizeof(int32_t), "Result::inliers holds int");
    std::vector<int32_t> const samples = mi_ransac_shim::draw_samples(this->opts.max_iterations, 3, corresp.size());

    mi_dmrecon_ransac_p3p_job job;
    job.n_corr = static_cast<int32_t>(corresp.size());
    job.n_iterations = this->opts.max_iterations;
    job.corr = corresp[0].p3d;
    for (int i = 0; i < 9; ++i)
        job.k_matrix[i] = k_matrix[i];
    job.samples = samples.data();
    job.threshold = this->opts.threshold;
    job.inliers_to_beat = static_cast<int32_t>(result->inliers.size());

    int32_t best_hypothesis = -1, n_inliers = 0;
    double pose[12];
    std::vector<int32_t> inliers(corresp.size());
    std::vector<int32_t> counts(this->opts.verbose_output ? 4 * static_cast<std::size_t>(this->opts.max_iterations) : 0);
    int32_t* inliers_ptr = inliers.data();
    int32_t* counts_ptr = counts.data();
    mi_shim::check(mi_dmrecon_ransac_pose_three_point(mi_shim::context_of_this_thread("sfm::RansacPoseP3P"), 1, &job,
        &best_hypothesis, pose, &n_inliers, &inliers_ptr, this->opts.verbose_output ? &counts_ptr : nullptr, nullptr),
        "mi_dmrecon_ransac_pose_three_point");

    if (this->opts.verbose_output)
    {
        std::size_t most = result->inliers.size();
        for (std::size_t hypothesis = 0; hypothesis < counts.size(); ++hypothesis)
        {
            if (static_cast<std::size_t>(counts[hypothesis]) <= most)
                continue;
            most = counts[hypothesis];
            std::cout << "RANSAC-3: Iteration " << hypothesis / 4
                << ", inliers " << most << " ("
                << (100.0 * most / corresp.size())
                << "%)" << std::endl;
        }
    }

    if (best_hypothesis < 0)
        return;
    for (int i = 0; i < 12; ++i)
        result->pose[i] = pose[i];
    result->inliers.assign(inliers.begin(), inliers.begin() + n_inliers);
}

void
RansacPoseP3P::compute_p3p (Correspondences2D3D const& /*corresp*/, math::Matrix<double, 3, 3> const& /*inv_k_matrix*/,
    PutativePoses* /*poses*/) const
{
    throw std::logic_error("sfm::RansacPoseP3P::compute_p3p (MI355X build): hypotheses are solved by estimate");
}

void
RansacPoseP3P::find_inliers (Correspondences2D3D const& /*corresp*/, math::Matrix<double, 3, 3> const& /*k_matrix*/,
    Pose const& /*pose*/, std::vector<int>* /*inliers*/) const
{
    throw std::logic_error("sfm::RansacPoseP3P::find_inliers (MI355X build): inliers are counted by estimate");
}

SFM_NAMESPACE_END
