/*
 * shim_common.h -- what the drop-ins of this directory share: the device of MI_DMRECON_DEVICES, the two ways a return code
 * of the library becomes an exception, and the process-wide context with one fork per calling thread.  Everything is inline:
 * each drop-in stands alone in whatever binary links it, and all that are linked into one binary share one parent context and
 * one fork per thread (an inline function's static is one object).  That is safe because a context keeps the state of each
 * module (RANSAC, SIFT, SURF, BA) apart, every entry point synchronises before it returns, and a thread calls one at a time.
 */
#ifndef MI_SHIM_COMMON_H
#define MI_SHIM_COMMON_H
#include <cstddef>
#include <cstdlib>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "mi_dmrecon.h"

namespace mi_shim {

/* the first usable entry of MI_DMRECON_DEVICES (default 0); `who` is the class the message names */
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

/* ... for a call whose arguments come from the caller of the class: MI_DMRECON_EINVAL is the reference's
 * std::invalid_argument, with the library's message alone */
inline void check_args(int rc, char const* what)
{
    if (rc == MI_DMRECON_EINVAL)
        throw std::invalid_argument(mi_dmrecon_last_error());
    check(rc, what);
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

/* every calling thread works on its own fork: its own stream and buffers.  The parent is made by the first call, on
 * first_device(who) */
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

}  /* namespace mi_shim */
#endif
