/*
 * ref_sift_driver.cc -- runs sfm::Sift on images read from a file and writes its keypoints and descriptors.  Linked with
 * the reference's own libs/sfm/sift.cc it produces the fixture tests/golden/sift_s1.npz (make_golden_sift.py).  Includes the
 * reference's headers at build time only.
 *
 *   ref_sift_driver IN OUT [bench REPEATS]
 *
 * IN (little endian): int32 n_cases; per case: int32 w, h, channels, is_float; int32 num_samples_per_octave, min_octave,
 *   max_octave; float contrast_threshold, edge_ratio_threshold, base_blur_sigma, inherent_blur_sigma; the pixels.
 * OUT, per case: int32 n_keypoints, then octave (as float), sample, x, y of each; int32 n_descriptors, then x, y, scale,
 *   orientation and the 128 values of each.
 * `bench`: instead, OMP_NUM_THREADS threads each process the first case REPEATS times (apps/sfmrecon computes the features
 *   of its views in such a loop); prints the seconds of each repeat and the counts.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include <omp.h>

#include "util/timer.h"
#include "mve/image.h"
#include "sfm/sift.h"

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

struct Case
{
    sfm::Sift::Options options;
    mve::ByteImage::Ptr bytes;
    mve::FloatImage::Ptr floats;
};

void run(Case const& c, sfm::Sift::Keypoints* kp, sfm::Sift::Descriptors* desc)
{
    sfm::Sift sift(c.options);
    if (c.floats != nullptr)
        sift.set_float_image(c.floats);
    else
        sift.set_image(c.bytes);
    sift.process();
    *kp = sift.get_keypoints();
    *desc = sift.get_descriptors();
}

}  /* namespace */

int main(int argc, char** argv)
{
    if (argc != 3 && !(argc == 5 && std::string(argv[3]) == "bench"))
    {
        std::cerr << "usage: " << argv[0] << " IN OUT [bench REPEATS]" << std::endl;
        return 2;
    }
    std::ifstream in(argv[1], std::ios::binary);
    int32_t const n_cases = get<int32_t>(in);
    std::vector<Case> cases(n_cases);
    for (int32_t i = 0; i < n_cases; ++i)
    {
        Case& c = cases[i];
        int32_t const w = get<int32_t>(in), h = get<int32_t>(in), ch = get<int32_t>(in), is_float = get<int32_t>(in);
        c.options.num_samples_per_octave = get<int32_t>(in);
        c.options.min_octave = get<int32_t>(in);
        c.options.max_octave = get<int32_t>(in);
        c.options.contrast_threshold = get<float>(in);
        c.options.edge_ratio_threshold = get<float>(in);
        c.options.base_blur_sigma = get<float>(in);
        c.options.inherent_blur_sigma = get<float>(in);
        if (is_float)
        {
            c.floats = mve::FloatImage::create(w, h, ch);
            in.read(reinterpret_cast<char*>(c.floats->begin()), sizeof(float) * w * h * ch);
        }
        else
        {
            c.bytes = mve::ByteImage::create(w, h, ch);
            in.read(reinterpret_cast<char*>(c.bytes->begin()), static_cast<std::streamsize>(w) * h * ch);
        }
        if (!in)
            throw std::runtime_error("input file too short");
    }

    if (argc == 5)
    {
        int const repeats = std::atoi(argv[4]);
        for (int r = 0; r < repeats; ++r)
        {
            util::WallTimer timer;
            std::size_t n_kp = 0, n_desc = 0;
#pragma omp parallel
            {
                sfm::Sift::Keypoints kp;
                sfm::Sift::Descriptors desc;
                run(cases[0], &kp, &desc);
#pragma omp master
                { n_kp = kp.size(); n_desc = desc.size(); }
            }
            std::printf("repeat %d: %d images on %d threads in %.4f s; %zu keypoints, %zu descriptors each\n", r,
                omp_get_max_threads(), omp_get_max_threads(), timer.get_elapsed() / 1000.0, n_kp, n_desc);
        }
        return 0;
    }

    std::ofstream out(argv[2], std::ios::binary);
    for (int32_t i = 0; i < n_cases; ++i)
    {
        sfm::Sift::Keypoints kp;
        sfm::Sift::Descriptors desc;
        run(cases[i], &kp, &desc);
        std::vector<float> rec;
        for (std::size_t k = 0; k < kp.size(); ++k)
        {
            float const v[4] = { static_cast<float>(kp[k].octave), kp[k].sample, kp[k].x, kp[k].y };
            rec.insert(rec.end(), v, v + 4);
        }
        int32_t n = static_cast<int32_t>(kp.size());
        out.write(reinterpret_cast<char const*>(&n), 4);
        out.write(reinterpret_cast<char const*>(rec.data()), rec.size() * sizeof(float));
        n = static_cast<int32_t>(desc.size());
        out.write(reinterpret_cast<char const*>(&n), 4);
        for (std::size_t k = 0; k < desc.size(); ++k)
        {
            float const v[4] = { desc[k].x, desc[k].y, desc[k].scale, desc[k].orientation };
            out.write(reinterpret_cast<char const*>(v), sizeof(v));
            out.write(reinterpret_cast<char const*>(desc[k].data.begin()), 128 * sizeof(float));
        }
    }
    return out.good() ? 0 : 1;
}
