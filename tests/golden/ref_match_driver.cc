/*
 * ref_match_driver.cc -- runs sfm::ExhaustiveMatching on descriptor sets read from a file and writes what it returns.
 * Linked with the reference's own libs/sfm/exhaustive_matching.cc it produces the fixture tests/golden/match_m1.npz
 * (make_golden_match.py); linked with mve_amd/host/sfm_exhaustive_matching.cc instead it is build/match_class_check, the
 * same calls on the drop-in class (mve_amd/host/Makefile).  Includes the reference's headers at build time only.
 *
 *   ref_match_driver IN OUT [bench REPEATS]
 *
 * IN (little endian): int32 n_views; per view: int32 n_sift, float[n_sift * 128], int32 n_surf, float[n_surf * 64];
 *   float sift_lowe, sift_dist, surf_lowe, surf_dist; int32 n_lowres, int32 N[n_lowres].
 * OUT, per pair i < j in ascending order, lists as int32 count + int32 values:
 *   pairwise_match matches_1_2, matches_2_1; raw twoway_match of the SIFT sets 1_2, 2_1; of the SURF sets 1_2, 2_1;
 *   pairwise_match_lowres for every N.
 * The pairs run in an OpenMP loop of four threads, as apps/sfmrecon runs them (bundler_matching.cc).
 * `bench`: instead, time Matching::twoway_match on the SIFT sets of all pairs (OMP_NUM_THREADS threads) REPEATS times and
 * print the seconds of each repeat.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <omp.h>

#include "util/timer.h"
#include "sfm/bundler_common.h"
#include "sfm/exhaustive_matching.h"
#include "sfm/matching.h"

namespace {

template <typename T>
T get(std::ifstream& in)
{
    T v;
    in.read(reinterpret_cast<char*>(&v), sizeof(T));
    if (!in)
        throw std::runtime_error("input file too short");
    return v;
}

void put_list(std::vector<int32_t>* out, std::vector<int> const& v)
{
    out->push_back(static_cast<int32_t>(v.size()));
    out->insert(out->end(), v.begin(), v.end());
}

/* the discretised sets are protected members of the class */
class Matcher : public sfm::ExhaustiveMatching
{
public:
    void raw_sift (int a, int b, sfm::Matching::Result* r) const
    {
        ProcessedFeatureSet const& p = this->processed_feature_sets[a];
        ProcessedFeatureSet const& q = this->processed_feature_sets[b];
        sfm::Matching::twoway_match(this->opts.sift_matching_opts, p.sift_descr.data()->begin(), p.sift_descr.size(),
            q.sift_descr.data()->begin(), q.sift_descr.size(), r);
    }
    void raw_surf (int a, int b, sfm::Matching::Result* r) const
    {
        ProcessedFeatureSet const& p = this->processed_feature_sets[a];
        ProcessedFeatureSet const& q = this->processed_feature_sets[b];
        sfm::Matching::twoway_match(this->opts.surf_matching_opts, p.surf_descr.data()->begin(), p.surf_descr.size(),
            q.surf_descr.data()->begin(), q.surf_descr.size(), r);
    }
};

}  /* namespace */

int main (int argc, char** argv)
{
    if (argc != 3 && !(argc == 5 && std::string(argv[3]) == "bench"))
    {
        std::cerr << "usage: " << argv[0] << " IN OUT [bench REPEATS]" << std::endl;
        return 2;
    }
    try
    {
        std::ifstream in(argv[1], std::ios::binary);
        if (!in)
            throw std::runtime_error(std::string("cannot read ") + argv[1]);
        int const n_views = get<int32_t>(in);
        sfm::bundler::ViewportList viewports(n_views);
        for (int v = 0; v < n_views; ++v)
        {
            sfm::FeatureSet& fs = viewports[v].features;
            fs.sift_descriptors.resize(get<int32_t>(in));
            for (std::size_t i = 0; i < fs.sift_descriptors.size(); ++i)
                for (int k = 0; k < 128; ++k)
                    fs.sift_descriptors[i].data[k] = get<float>(in);
            fs.surf_descriptors.resize(get<int32_t>(in));
            for (std::size_t i = 0; i < fs.surf_descriptors.size(); ++i)
                for (int k = 0; k < 64; ++k)
                    fs.surf_descriptors[i].data[k] = get<float>(in);
        }
        Matcher matcher;
        matcher.opts.sift_matching_opts.lowe_ratio_threshold = get<float>(in);
        matcher.opts.sift_matching_opts.distance_threshold = get<float>(in);
        matcher.opts.surf_matching_opts.lowe_ratio_threshold = get<float>(in);
        matcher.opts.surf_matching_opts.distance_threshold = get<float>(in);
        std::vector<int32_t> lowres(get<int32_t>(in));
        for (std::size_t i = 0; i < lowres.size(); ++i)
            lowres[i] = get<int32_t>(in);

        matcher.init(&viewports);

        std::vector<std::pair<int, int> > pairs;
        for (int i = 0; i < n_views; ++i)
            for (int j = i + 1; j < n_views; ++j)
                pairs.push_back(std::make_pair(i, j));

        if (argc == 5)
        {
            int const repeats = std::atoi(argv[4]);
            std::printf("threads %d pairs %d\n", omp_get_max_threads(), static_cast<int>(pairs.size()));
            for (int r = 0; r < repeats; ++r)
            {
                util::WallTimer timer;
                long total = 0;
#pragma omp parallel for schedule(dynamic) reduction(+:total)
                for (std::size_t p = 0; p < pairs.size(); ++p)
                {
                    sfm::Matching::Result res;
                    matcher.raw_sift(pairs[p].first, pairs[p].second, &res);
                    total += sfm::Matching::count_consistent_matches(res);
                }
                std::printf("repeat %d seconds %.4f consistent %ld\n", r, timer.get_elapsed() / 1000.0, total);
                std::fflush(stdout);
            }
            return 0;
        }

        std::vector<std::vector<int32_t> > out(pairs.size());
#pragma omp parallel for schedule(dynamic) num_threads(4)
        for (std::size_t p = 0; p < pairs.size(); ++p)
        {
            int const a = pairs[p].first, b = pairs[p].second;
            sfm::Matching::Result res, sift, surf;
            matcher.pairwise_match(a, b, &res);
            matcher.raw_sift(a, b, &sift);
            matcher.raw_surf(a, b, &surf);
            put_list(&out[p], res.matches_1_2);
            put_list(&out[p], res.matches_2_1);
            put_list(&out[p], sift.matches_1_2);
            put_list(&out[p], sift.matches_2_1);
            put_list(&out[p], surf.matches_1_2);
            put_list(&out[p], surf.matches_2_1);
            for (std::size_t i = 0; i < lowres.size(); ++i)
                out[p].push_back(matcher.pairwise_match_lowres(a, b, lowres[i]));
        }
        std::ofstream os(argv[2], std::ios::binary);
        for (std::size_t p = 0; p < out.size(); ++p)
            os.write(reinterpret_cast<char const*>(out[p].data()), out[p].size() * sizeof(int32_t));
        if (!os)
            throw std::runtime_error(std::string("cannot write ") + argv[2]);
    }
    catch (std::exception const& e)
    {
        std::cerr << "ref_match_driver: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
