/*
 * sfm_matcher_registry.h -- the matcher handle of an sfm::ExhaustiveMatching object, for the drop-ins that work on it:
 * sfm_exhaustive_matching.cc makes it in init and defines matcher_of; sfm_cascade_hashing.cc, whose class derives from
 * ExhaustiveMatching and calls its init first, hashes and matches on the same handle.
 */
#ifndef MI_SFM_MATCHER_REGISTRY_H
#define MI_SFM_MATCHER_REGISTRY_H
#include <memory>

#include "mi_dmrecon.h"

namespace mi_shim {

/* the context and the matcher of one ExhaustiveMatching object */
struct MatcherDevice
{
    mi_dmrecon_ctx* ctx = nullptr;
    mi_dmrecon_match* match = nullptr;
    ~MatcherDevice (void)
    {
        mi_dmrecon_match_destroy(this->match);
        if (this->ctx != nullptr)
            mi_dmrecon_ctx_destroy(this->ctx);
    }
};

/* throws std::runtime_error before the object's init */
std::shared_ptr<MatcherDevice> matcher_of(void const* self);

}  /* namespace mi_shim */
#endif
