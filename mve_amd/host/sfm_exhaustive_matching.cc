/*
 * sfm_exhaustive_matching.cc -- the five members of sfm::ExhaustiveMatching that the reference defines in
 * libs/sfm/exhaustive_matching.cc (init, init_sift, init_surf, pairwise_match, pairwise_match_lowres), on top of
 * libmi_dmrecon.so: linked INSTEAD of that one file, with the rest of libs/sfm and apps/sfmrecon unmodified, this makes
 * build/sfmrecon_mi (mve_amd/host/Makefile).  Compiled against the reference's own sfm/exhaustive_matching.h (the class is
 * the reference's; only these definitions are ours).
 *
 * Behaviour kept from the reference (libs/sfm/exhaustive_matching.cc):
 *   :55-108   init fills processed_feature_sets with the discretised descriptors (:18-39: clamp, scale, math::round),
 *   :110-140  pairwise_match: SIFT and SURF two-way matches, each only if view 1 has descriptors of that type,
 *             Matching::remove_inconsistent_matches on each, Matching::combine_results -- the reference's functions, linked in,
 *   :142-176  pairwise_match_lowres: the first min(N, size) descriptors, SIFT if view 1 has any, else SURF; the count of
 *             consistent matches.
 * What differs: Matching::twoway_match (libs/sfm/matching.h:148-159) runs on the GPU (mi_dmrecon_match_pairs).
 *
 * The class has no spare member and a defaulted destructor, so the matcher handle of an object lives in a registry keyed
 * by `this`: replaced by the next init of the same object, released at process exit.
 * Device choice: the first entry of MI_DMRECON_DEVICES (default 0), as the dmrecon shim reads it.
 */
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "sfm/exhaustive_matching.h"

#include "mi_dmrecon.h"

SFM_NAMESPACE_BEGIN

namespace {

int first_device(void)
{
    int const n = mi_dmrecon_device_count();
    if (n <= 0)
        throw std::runtime_error("sfm::ExhaustiveMatching (MI355X build): no HIP device available; there is no CPU path");
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

void check(int rc, char const* what)
{
    if (rc != 0)
        throw std::runtime_error(std::string(what) + ": " + mi_dmrecon_last_error());
}

/* the context and the matcher of one ExhaustiveMatching object */
struct Device
{
    mi_dmrecon_ctx* ctx = nullptr;
    mi_dmrecon_match* match = nullptr;
    ~Device (void)
    {
        mi_dmrecon_match_destroy(this->match);
        if (this->ctx != nullptr)
            mi_dmrecon_ctx_destroy(this->ctx);
    }
};

std::mutex registry_mutex;
std::map<void const*, std::shared_ptr<Device> > registry;      /* destroyed at process exit, and its handles with it */

std::shared_ptr<Device> device_of(void const* self)
{
    std::lock_guard<std::mutex> lock(registry_mutex);
    std::map<void const*, std::shared_ptr<Device> >::const_iterator it = registry.find(self);
    if (it == registry.end())
        throw std::runtime_error("sfm::ExhaustiveMatching (MI355X build): pairwise_match before init");
    return it->second;
}

/* Matching::twoway_match of the first n_1 / n_2 descriptors of two views; raw, as the reference's */
void twoway(Device const& dev, int kind, Matching::Options const& options, int view_1, std::size_t n_1, int view_2,
    std::size_t n_2, Matching::Result* result)
{
    mi_dmrecon_match_options opt;
    opt.struct_size = static_cast<int32_t>(sizeof(opt));
    opt.lowe_ratio_threshold = options.lowe_ratio_threshold;
    opt.distance_threshold = options.distance_threshold;
    mi_dmrecon_match_job job;
    job.set_a = view_1;
    job.n_a = static_cast<int32_t>(n_1);
    job.set_b = view_2;
    job.n_b = static_cast<int32_t>(n_2);
    static_assert(sizeof(int) == sizeof(int32_t), "Matching::Result holds int");
    result->matches_1_2.assign(n_1, -1);
    result->matches_2_1.assign(n_2, -1);
    int32_t* ab = result->matches_1_2.data();
    int32_t* ba = result->matches_2_1.data();
    check(mi_dmrecon_match_pairs(dev.match, kind, &opt, 1, &job, &ab, &ba, nullptr), "mi_dmrecon_match_pairs");
}

}  /* namespace */

void
ExhaustiveMatching::init (bundler::ViewportList* viewports)
{
    std::size_t const num_views = viewports->size();
    this->processed_feature_sets.clear();
    this->processed_feature_sets.resize(num_views);
    for (std::size_t i = 0; i < num_views; ++i)
    {
        this->init_sift(&this->processed_feature_sets[i].sift_descr, viewports->at(i).features.sift_descriptors);
        this->init_surf(&this->processed_feature_sets[i].surf_descr, viewports->at(i).features.surf_descriptors);
    }

    /* the discretised sets, as the class holds them, onto the device */
    std::shared_ptr<Device> dev(new Device());
    check(mi_dmrecon_ctx_create(first_device(), &dev->ctx), "mi_dmrecon_ctx_create");
    check(mi_dmrecon_match_create(dev->ctx, static_cast<int32_t>(viewports->size()), &dev->match), "mi_dmrecon_match_create");
    for (std::size_t i = 0; i < viewports->size(); ++i)
    {
        ProcessedFeatureSet const& pfs = this->processed_feature_sets[i];
        check(mi_dmrecon_match_set(dev->match, static_cast<int32_t>(i), MI_DMRECON_MATCH_SIFT, MI_DMRECON_MATCH_I16,
            static_cast<int32_t>(pfs.sift_descr.size()), pfs.sift_descr.size() ? pfs.sift_descr.data()->begin() : nullptr),
            "mi_dmrecon_match_set");
        check(mi_dmrecon_match_set(dev->match, static_cast<int32_t>(i), MI_DMRECON_MATCH_SURF, MI_DMRECON_MATCH_I16,
            static_cast<int32_t>(pfs.surf_descr.size()), pfs.surf_descr.size() ? pfs.surf_descr.data()->begin() : nullptr),
            "mi_dmrecon_match_set");
    }
    std::lock_guard<std::mutex> lock(registry_mutex);
    registry[this] = dev;
}

void
ExhaustiveMatching::init_sift (SiftDescriptors* dst, Sift::Descriptors const& src)
{
    dst->resize(src.size());
    uint16_t* ptr = dst->data()->begin();
    for (std::size_t i = 0; i < src.size(); ++i, ptr += 128)
        for (int k = 0; k < 128; ++k)
        {
            float value = math::clamp(src[i].data[k], 0.0f, 1.0f);
            value = math::round(value * 255.0f);
            ptr[k] = static_cast<unsigned char>(value);
        }
}

void
ExhaustiveMatching::init_surf (SurfDescriptors* dst, Surf::Descriptors const& src)
{
    dst->resize(src.size());
    int16_t* ptr = dst->data()->begin();
    for (std::size_t i = 0; i < src.size(); ++i, ptr += 64)
        for (int k = 0; k < 64; ++k)
        {
            float value = math::clamp(src[i].data[k], -1.0f, 1.0f);
            value = math::round(value * 127.0f);
            ptr[k] = static_cast<signed char>(value);
        }
}

void
ExhaustiveMatching::pairwise_match (int view_1_id, int view_2_id, Matching::Result* result) const
{
    ProcessedFeatureSet const& pfs_1 = this->processed_feature_sets[view_1_id];
    ProcessedFeatureSet const& pfs_2 = this->processed_feature_sets[view_2_id];
    std::shared_ptr<Device> dev = device_of(this);

    Matching::Result sift_result;
    if (pfs_1.sift_descr.size() > 0)
    {
        twoway(*dev, MI_DMRECON_MATCH_SIFT, this->opts.sift_matching_opts, view_1_id, pfs_1.sift_descr.size(),
            view_2_id, pfs_2.sift_descr.size(), &sift_result);
        Matching::remove_inconsistent_matches(&sift_result);
    }

    Matching::Result surf_result;
    if (pfs_1.surf_descr.size() > 0)
    {
        twoway(*dev, MI_DMRECON_MATCH_SURF, this->opts.surf_matching_opts, view_1_id, pfs_1.surf_descr.size(),
            view_2_id, pfs_2.surf_descr.size(), &surf_result);
        Matching::remove_inconsistent_matches(&surf_result);
    }

    Matching::combine_results(sift_result, surf_result, result);
}

int
ExhaustiveMatching::pairwise_match_lowres (int view_1_id, int view_2_id, std::size_t num_features) const
{
    ProcessedFeatureSet const& pfs_1 = this->processed_feature_sets[view_1_id];
    ProcessedFeatureSet const& pfs_2 = this->processed_feature_sets[view_2_id];
    std::shared_ptr<Device> dev = device_of(this);

    if (pfs_1.sift_descr.size() > 0)
    {
        Matching::Result sift_result;
        twoway(*dev, MI_DMRECON_MATCH_SIFT, this->opts.sift_matching_opts,
            view_1_id, std::min(num_features, pfs_1.sift_descr.size()),
            view_2_id, std::min(num_features, pfs_2.sift_descr.size()), &sift_result);
        return Matching::count_consistent_matches(sift_result);
    }

    if (pfs_1.surf_descr.size() > 0)
    {
        Matching::Result surf_result;
        twoway(*dev, MI_DMRECON_MATCH_SURF, this->opts.surf_matching_opts,
            view_1_id, std::min(num_features, pfs_1.surf_descr.size()),
            view_2_id, std::min(num_features, pfs_2.surf_descr.size()), &surf_result);
        return Matching::count_consistent_matches(surf_result);
    }

    return 0;
}

SFM_NAMESPACE_END
