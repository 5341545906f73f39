/*
 * sfm_ransac_homography.cc -- the four members of sfm::RansacHomography that the reference defines in
 * libs/sfm/ransac_homography.cc (the constructor, estimate, compute_homography, evaluate_homography), on top of
 * libmi_dmrecon.so: linked INSTEAD of that one file, with the rest of libs/sfm and apps/sfmrecon unmodified
 * (mve_amd/host/Makefile, build/sfmrecon_mi).  Compiled against the reference's own sfm/ransac_homography.h.
 *
 * Behaviour kept from the reference (libs/sfm/ransac_homography.cc):
 *   :30-35    the verbose header line; :46-52 one verbose line per improving iteration (here: after the call, from the
 *             per-iteration counts),
 *   :65-66    fewer than 4 matches: std::invalid_argument("At least 4 matches required"),
 *   :72-74    the draws: util::system::rand_int() % matches.size() into a std::set until it holds 4 -- made for all
 *             max_iterations iterations up front, in the reference's order (ransac_shim.h),
 *   :44, :54-55  result is written only by an iteration with MORE inliers than result->inliers holds on entry.
 * What differs: the DLT solves and the symmetric transfer errors of all iterations run on the GPU
 * (mi_dmrecon_ransac_homography); H and the inlier set agree with the reference's to rounding, not bit for bit
 * (include/mi_dmrecon.h).  The context and its forks: shim_common.h.
 */
#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "sfm/ransac_homography.h"

#include "ransac_shim.h"

SFM_NAMESPACE_BEGIN

RansacHomography::RansacHomography (Options const& options)
    : opts(options)
{
}

void
RansacHomography::estimate (Correspondences2D2D const& matches, Result* result)
{
    if (this->opts.verbose_output)
    {
        std::cout << "RANSAC-H: Running for " << this->opts.max_iterations
            << " iterations, threshold " << this->opts.threshold
            << "..." << std::endl;
    }
    if (this->opts.max_iterations < 1)
        return;
    if (matches.size() < 4)
        throw std::invalid_argument("At least 4 matches required");

    static_assert(sizeof(Correspondence2D2D) == 4 * sizeof(double), "a match is p1.x p1.y p2.x p2.y");
    static_assert(sizeof(int) == sizeof(int32_t), "Result::inliers holds int");
    std::vector<int32_t> const samples = mi_ransac_shim::draw_samples(this->opts.max_iterations, 4, matches.size());

    mi_dmrecon_ransac_job job;
    job.n_matches = static_cast<int32_t>(matches.size());
    job.n_iterations = this->opts.max_iterations;
    job.matches = matches[0].p1;
    job.samples = samples.data();
    job.threshold = this->opts.threshold;
    job.inliers_to_beat = static_cast<int32_t>(result->inliers.size());

    int32_t best_iteration = -1, n_inliers = 0;
    double homography[9];
    std::vector<int32_t> inliers(matches.size());
    std::vector<int32_t> counts(this->opts.verbose_output ? this->opts.max_iterations : 0);
    int32_t* inliers_ptr = inliers.data();
    int32_t* counts_ptr = counts.data();
    mi_shim::check(mi_dmrecon_ransac_homography(mi_shim::context_of_this_thread("sfm::RansacHomography"), 1,
        &job, &best_iteration, homography, &n_inliers, &inliers_ptr, this->opts.verbose_output ? &counts_ptr : nullptr,
        nullptr), "mi_dmrecon_ransac_homography");

    if (this->opts.verbose_output)
    {
        std::size_t most = result->inliers.size();
        for (int iteration = 0; iteration < this->opts.max_iterations; ++iteration)
        {
            if (static_cast<std::size_t>(counts[iteration]) <= most)
                continue;
            most = counts[iteration];
            std::cout << "RANSAC-H: Iteration " << iteration
                << ", inliers " << most << " ("
                << (100.0 * most / matches.size())
                << "%)" << std::endl;
        }
    }

    if (best_iteration < 0)
        return;
    for (int i = 0; i < 9; ++i)
        result->homography[i] = homography[i];
    result->inliers.assign(inliers.begin(), inliers.begin() + n_inliers);
}

void
RansacHomography::compute_homography (Correspondences2D2D const& /*matches*/, HomographyMatrix* /*homography*/)
{
    throw std::logic_error("sfm::RansacHomography::compute_homography (MI355X build): hypotheses are solved by estimate");
}

void
RansacHomography::evaluate_homography (Correspondences2D2D const& /*matches*/, HomographyMatrix const& /*homography*/,
    std::vector<int>* /*inliers*/)
{
    throw std::logic_error("sfm::RansacHomography::evaluate_homography (MI355X build): inliers are counted by estimate");
}

SFM_NAMESPACE_END
