/*
 * ransac_shim.h -- what the three RANSAC drop-ins (sfm_ransac_fundamental.cc, sfm_ransac_homography.cc,
 * sfm_ransac_pose_p3p.cc) share: the device of MI_DMRECON_DEVICES, the process-wide context with one fork per calling thread,
 * and the draws.  Everything is inline or static: each drop-in stands alone in whatever binary links it, and all that are
 * linked into one binary share one context (the inline function's static is one object).
 */
#ifndef MI_RANSAC_SHIM_H
#define MI_RANSAC_SHIM_H
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "util/system.h"

#include "mi_dmrecon.h"

namespace mi_ransac_shim {

/* the first usable entry of MI_DMRECON_DEVICES (default 0), as the other shims read it */
inline int first_device(char const* who)
{
    int const n = mi_dmrecon_device_count();
    if (n <= 0)
        throw std::runtime_error(std::string(who) + " (MI355X build): no HIP device available; there is no CPU path");
    char const* env = std::getenv("MI_DMRECON_DEVICES");
    if (env && *env)
    {
        std::stringstream ss(env);
        std::string tok;
        while (std::getline(ss, tok, ','))
        {
            int const d = std::atoi(tok.c_str());
            if (d >= 0 && d < n)
                return d;
        }
    }
    return 0;
}

inline void check(int rc, char const* what)
{
    if (rc != 0)
        throw std::runtime_error(std::string(what) + ": " + mi_dmrecon_last_error());
}

/* the process-wide context and its forks, released at exit */
struct Contexts
{
    std::mutex mutex;
    mi_dmrecon_ctx* parent = nullptr;
    std::vector<mi_dmrecon_ctx*> forks;
    ~Contexts (void)
    {
        for (std::size_t i = 0; i < this->forks.size(); ++i)
            mi_dmrecon_ctx_destroy(this->forks[i]);
        if (this->parent != nullptr)
            mi_dmrecon_ctx_destroy(this->parent);
    }
};

/* every calling thread works on its own fork: its own stream and buffers */
inline mi_dmrecon_ctx* context_of_this_thread(char const* who)
{
    static Contexts contexts;
    static thread_local mi_dmrecon_ctx* mine = nullptr;
    if (mine != nullptr)
        return mine;
    std::lock_guard<std::mutex> lock(contexts.mutex);
    if (contexts.parent == nullptr)
        check(mi_dmrecon_ctx_create(first_device(who), &contexts.parent), "mi_dmrecon_ctx_create");
    check(mi_dmrecon_ctx_fork(contexts.parent, &mine), "mi_dmrecon_ctx_fork");
    contexts.forks.push_back(mine);
    return mine;
}

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
