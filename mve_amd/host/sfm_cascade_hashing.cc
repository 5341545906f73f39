/*
 * sfm_cascade_hashing.cc -- the members of sfm::CascadeHashing that the reference defines in libs/sfm/cascade_hashing.cc, on
 * top of libmi_dmrecon.so: linked INSTEAD of that one file (mve_amd/host/Makefile), so that build/sfmrecon_mi
 * --cascade-hashing hashes and matches on the GPU.  Compiled against the reference's own sfm/cascade_hashing.h: the class,
 * its options and the generator of the projection matrices (a template of that header: std::mt19937(0) with
 * std::normal_distribution, cascade_hashing.h:225-254) are the reference's.
 *
 * Behaviour kept from the reference (libs/sfm/cascade_hashing.cc):
 *   :33-69    init: ExhaustiveMatching::init (ours: it uploads the discretised sets), the matrices, the mean descriptors,
 *             the hashes of every view, and the timing line,
 *   :145-177  compute_avg_descriptors: one float sum of d / 255 (SIFT) or d / 127 (SURF) over all views in view order, then
 *             one division by the count,
 *   :71-104   pairwise_match: SIFT and SURF two-way matches, each only if view 1 has descriptors of that type,
 *             Matching::remove_inconsistent_matches on each, Matching::combine_results -- the reference's functions, linked in.
 * What differs: compute_cascade_hashes, build_buckets and twoway_match run on the GPU (mi_dmrecon_match_hash,
 * mi_dmrecon_match_pairs_hashed) on the handle ExhaustiveMatching::init made (sfm_matcher_registry.h); the hash bits carry no
 * bit-parity with a CPU build (include/mi_dmrecon.h).  local_data_sift / local_data_surf stay empty, and the three private
 * members that filled them (compute, compute_zero_mean_descs, build_buckets) have no caller left: they throw.
 */
#include <cstdint>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <vector>

#include "sfm/cascade_hashing.h"

#include "shim_common.h"
#include "sfm_matcher_registry.h"

SFM_NAMESPACE_BEGIN

namespace {

using mi_shim::check;

/* mi_dmrecon_match_hash for one descriptor type: the matrices row by row, as the header's ProjMats hold them */
template <typename T>
void hash_kind(mi_shim::MatcherDevice const& dev, int kind, T const& mean, std::size_t num_descs,
    std::vector<T> const& primary, std::vector<std::vector<T> > const& secondary, uint8_t groups, uint8_t bits,
    uint16_t min_candidates, uint16_t max_candidates)
{
    mi_dmrecon_match_hash_options opt;
    opt.struct_size = static_cast<int32_t>(sizeof(opt));
    opt.num_bucket_groups = groups;
    opt.num_bucket_bits = bits;
    opt.min_num_candidates = min_candidates;
    opt.max_num_candidates = max_candidates;
    std::vector<float> m(T::dim, 0.0f), p, s;
    if (num_descs > 0)              /* (without descriptors the mean is 0 / 0, and nothing reads it) */
        m.assign(mean.begin(), mean.end());
    for (std::size_t k = 0; k < primary.size(); ++k)
        p.insert(p.end(), primary[k].begin(), primary[k].end());
    for (std::size_t g = 0; g < secondary.size(); ++g)
        for (std::size_t k = 0; k < secondary[g].size(); ++k)
            s.insert(s.end(), secondary[g][k].begin(), secondary[g][k].end());
    check(mi_dmrecon_match_hash(dev.match, kind, &opt, m.data(), p.data(), s.data()), "mi_dmrecon_match_hash");
}

/* CascadeHashing::twoway_match of two views' whole lists; raw, as the reference's */
void twoway(mi_shim::MatcherDevice const& dev, int kind, Matching::Options const& options, int view_1, std::size_t n_1,
    int view_2, std::size_t n_2, Matching::Result* result)
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
    check(mi_dmrecon_match_pairs_hashed(dev.match, kind, &opt, 1, &job, &ab, &ba, nullptr), "mi_dmrecon_match_pairs_hashed");
}

}  /* namespace */

void
CascadeHashing::GlobalData::generate_proj_matrices (Options const& opts)
{
    /* SIFT and SURF each from a generator seeded with 0 (the header's template) */
    this->generate_proj_matrices(&this->sift.prim_proj_mat, &this->sift.sec_proj_mats, opts);
    this->generate_proj_matrices(&this->surf.prim_proj_mat, &this->surf.sec_proj_mats, opts);
}

void
CascadeHashing::init (bundler::ViewportList* viewports)
{
    ExhaustiveMatching::init(viewports);

    util::WallTimer timer;
    this->local_data_sift.clear();
    this->local_data_surf.clear();
    this->global_data.generate_proj_matrices(this->cashash_opts);

    math::Vec128f sift_avg;
    math::Vec64f surf_avg;
    this->compute_avg_descriptors(this->processed_feature_sets, &sift_avg, &surf_avg);
    std::size_t num_sift = 0, num_surf = 0;
    for (std::size_t i = 0; i < this->processed_feature_sets.size(); ++i)
    {
        num_sift += this->processed_feature_sets[i].sift_descr.size();
        num_surf += this->processed_feature_sets[i].surf_descr.size();
    }

    std::shared_ptr<mi_shim::MatcherDevice> dev = mi_shim::matcher_of(this);
    Options const& o = this->cashash_opts;
    hash_kind(*dev, MI_DMRECON_MATCH_SIFT, sift_avg, num_sift, this->global_data.sift.prim_proj_mat,
        this->global_data.sift.sec_proj_mats, o.num_bucket_groups, o.num_bucket_bits, o.min_num_candidates, o.max_num_candidates);
    hash_kind(*dev, MI_DMRECON_MATCH_SURF, surf_avg, num_surf, this->global_data.surf.prim_proj_mat,
        this->global_data.surf.sec_proj_mats, o.num_bucket_groups, o.num_bucket_bits, o.min_num_candidates, o.max_num_candidates);
    std::cout << "Computing cascade hashes took " << timer.get_elapsed() << " ms" << std::endl;
}

void
CascadeHashing::pairwise_match (int view_1_id, int view_2_id, Matching::Result* result) const
{
    ProcessedFeatureSet const& pfs_1 = this->processed_feature_sets[view_1_id];
    ProcessedFeatureSet const& pfs_2 = this->processed_feature_sets[view_2_id];
    std::shared_ptr<mi_shim::MatcherDevice> dev = mi_shim::matcher_of(this);

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

void
CascadeHashing::compute_avg_descriptors (ProcessedFeatureSets const& pfs, math::Vec128f* sift_avg, math::Vec64f* surf_avg)
{
    /* float sums in view order, descriptor order, of value / 255.0f and value / 127.0f; one division by the count */
    math::Vec128f sift_sum(0.0f);
    math::Vec64f surf_sum(0.0f);
    std::size_t num_sift = 0, num_surf = 0;
    for (std::size_t i = 0; i < pfs.size(); ++i)
    {
        SiftDescriptors const& sift = pfs[i].sift_descr;
        for (std::size_t j = 0; j < sift.size(); ++j)
            for (int k = 0; k < 128; ++k)
                sift_sum[k] += sift[j][k] / 255.0f;
        num_sift += sift.size();

        SurfDescriptors const& surf = pfs[i].surf_descr;
        for (std::size_t j = 0; j < surf.size(); ++j)
            for (int k = 0; k < 64; ++k)
                surf_sum[k] += surf[j][k] / 127.0f;
        num_surf += surf.size();
    }
    *sift_avg = sift_sum / num_sift;
    *surf_avg = surf_sum / num_surf;
}

/* ---- the members the GPU path leaves without a caller ---- */

void
CascadeHashing::compute (LocalData*, LocalData*, std::vector<math::Vec128f> const&, std::vector<math::Vec64f> const&,
    GlobalData const&, Options const&)
{
    throw std::logic_error("sfm::CascadeHashing::compute (MI355X build): the hashes are computed by mi_dmrecon_match_hash");
}

void
CascadeHashing::compute_zero_mean_descs (std::vector<math::Vec128f>*, std::vector<math::Vec64f>*, SiftDescriptors const&,
    SurfDescriptors const&, math::Vec128f const&, math::Vec64f const&)
{
    throw std::logic_error("sfm::CascadeHashing::compute_zero_mean_descs (MI355X build): the hashes are computed by mi_dmrecon_match_hash");
}

void
CascadeHashing::build_buckets (BucketGroupsFeatures*, BucketGroupsBuckets const&, size_t, Options const&)
{
    throw std::logic_error("sfm::CascadeHashing::build_buckets (MI355X build): the buckets are built by mi_dmrecon_match_hash");
}

SFM_NAMESPACE_END
