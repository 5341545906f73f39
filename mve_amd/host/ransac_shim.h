/*
 * ransac_shim.h -- what the three RANSAC drop-ins (sfm_ransac_fundamental.cc, sfm_ransac_homography.cc,
 * sfm_ransac_pose_p3p.cc) share beyond shim_common.h (the device, the process-wide context with one fork per calling thread):
 * the draws.  Inline, so each drop-in stands alone in whatever binary links it.
 */
#ifndef MI_RANSAC_SHIM_H
#define MI_RANSAC_SHIM_H
#include <cstdint>
#include <set>
#include <vector>

#include "util/system.h"

#include "shim_common.h"

namespace mi_ransac_shim {

/* The reference's draws: util::system::rand_int() % size into a std::set until it holds `width`, for all iterations up
 * front and in the reference's order, so a single-threaded run with a given srand seed consumes the generator as the
 * reference does and tests the same samples (a std::set iterates ascending: so do the rows). */
inline std::vector<int32_t> draw_samples(int iterations, std::size_t width, std::size_t size)
{
    std::vector<int32_t> samples;
    samples.reserve(static_cast<std::size_t>(iterations) * width);
    for (int iteration = 0; iteration < iterations; ++iteration)
    {
        std::set<int> drawn;
        while (drawn.size() < width)
            drawn.insert(util::system::rand_int() % size);
        samples.insert(samples.end(), drawn.begin(), drawn.end());
    }
    return samples;
}

}  /* namespace mi_ransac_shim */
#endif
