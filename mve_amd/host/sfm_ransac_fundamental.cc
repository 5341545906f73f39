/*
 * sfm_ransac_fundamental.cc -- the four members of sfm::RansacFundamental that the reference defines in
 * libs/sfm/ransac_fundamental.cc (the constructor, estimate, estimate_8_point, find_inliers), on top of libmi_dmrecon.so:
 * linked INSTEAD of that one file, with the rest of libs/sfm and apps/sfmrecon unmodified (mve_amd/host/Makefile, build/sfmrecon_mi).
 * Compiled against the reference's own sfm/ransac_fundamental.h (the class is the reference's; only these definitions are ours).
 *
 * Behaviour kept from the reference (libs/sfm/ransac_fundamental.cc):
 *   :29-34    the verbose header line; :45-51 one verbose line per improving iteration (here: after the call, from the
 *             per-iteration counts),
 *   :64-65    fewer than 8 matches: std::invalid_argument("At least 8 matches required"),
 *   :71-73    the draws: util::system::rand_int() % matches.size() into a std::set until it holds 8 -- made for all
 *             max_iterations iterations up front, in the reference's order, so a single-threaded run with a given srand seed
 *             consumes the generator as the reference does and tests the same samples (a std::set iterates ascending: so do
 *             the rows handed to the library),
 *   :43, :53-54  result is written only by an iteration with MORE inliers than result->inliers holds on entry.
 * What differs: the 8-point solves and the Sampson tests of all iterations run on the GPU (mi_dmrecon_ransac_fundamental);
 * F and the inlier set agree with the reference's to rounding, not bit for bit (include/mi_dmrecon.h).
 *
 * One context for the process, shared with every other drop-in of this directory that the binary links (shim_common.h): made
 * by the first call of any of them on the first entry of MI_DMRECON_DEVICES (default 0); every calling thread works on its
 * own fork (its own stream and buffers); all are released at exit.
 */
#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "sfm/ransac_fundamental.h"

#include "ransac_shim.h"

SFM_NAMESPACE_BEGIN

RansacFundamental::RansacFundamental (Options const& options)
    : opts(options)
{
}

void
RansacFundamental::estimate (Correspondences2D2D const& matches, Result* result)
{
    if (this->opts.verbose_output)
    {
        std::cout << "RANSAC-F: Running for " << this->opts.max_iterations
            << " iterations, threshold " << this->opts.threshold
            << "..." << std::endl;
    }
    if (this->opts.max_iterations < 1)
        return;
    if (matches.size() < 8)
        throw std::invalid_argument("At least 8 matches required");

    static_assert(sizeof(Correspondence2D2D) == 4 * sizeof(double), "a match is p1.x p1.y p2.x p2.y");
    static_assert(sizeof(int) == sizeof(int32_t), "Result::inliers holds int");
    std::vector<int32_t> const samples = mi_ransac_shim::draw_samples(this->opts.max_iterations, 8, matches.size());

    mi_dmrecon_ransac_job job;
    job.n_matches = static_cast<int32_t>(matches.size());
    job.n_iterations = this->opts.max_iterations;
    job.matches = matches[0].p1;
    job.samples = samples.data();
    job.threshold = this->opts.threshold;
    job.inliers_to_beat = static_cast<int32_t>(result->inliers.size());

    int32_t best_iteration = -1, n_inliers = 0;
    double fundamental[9];
    std::vector<int32_t> inliers(matches.size());
    std::vector<int32_t> counts(this->opts.verbose_output ? this->opts.max_iterations : 0);
    int32_t* inliers_ptr = inliers.data();
    int32_t* counts_ptr = counts.data();
    mi_shim::check(mi_dmrecon_ransac_fundamental(mi_shim::context_of_this_thread("sfm::RansacFundamental"), 1, &job, &best_iteration, fundamental, &n_inliers,
        &inliers_ptr, this->opts.verbose_output ? &counts_ptr : nullptr, nullptr), "mi_dmrecon_ransac_fundamental");

    if (this->opts.verbose_output)
    {
        std::size_t most = result->inliers.size();
        for (int iteration = 0; iteration < this->opts.max_iterations; ++iteration)
        {
            if (static_cast<std::size_t>(counts[iteration]) <= most)
                continue;
            most = counts[iteration];
            std::cout << "RANSAC-F: Iteration " << iteration
                << ", inliers " << most << " ("
                << (100.0 * most / matches.size())
                << "%)" << std::endl;
        }
    }

    if (best_iteration < 0)
        return;
    for (int i = 0; i < 9; ++i)
        result->fundamental[i] = fundamental[i];
    result->inliers.assign(inliers.begin(), inliers.begin() + n_inliers);
}

void
RansacFundamental::estimate_8_point (Correspondences2D2D const& /*matches*/, FundamentalMatrix* /*fundamental*/)
{
    throw std::logic_error("sfm::RansacFundamental::estimate_8_point (MI355X build): hypotheses are solved by estimate");
}

void
RansacFundamental::find_inliers (Correspondences2D2D const& /*matches*/, FundamentalMatrix const& /*fundamental*/,
    std::vector<int>* /*result*/)
{
    throw std::logic_error("sfm::RansacFundamental::find_inliers (MI355X build): inliers are counted by estimate");
}

SFM_NAMESPACE_END
