/*
 * sfm_sift.cc -- the members of sfm::Sift that the reference defines in libs/sfm/sift.cc, on top of libmi_dmrecon.so: linked
 * INSTEAD of that one file, with the rest of libs/sfm and apps/sfmrecon unmodified (mve_amd/host/Makefile, build/sfmrecon_mi).
 * Compiled against the reference's own sfm/sift.h (the class, its Options, Keypoint and Descriptor are the reference's; only
 * these definitions are ours).
 *
 * Behaviour kept from the reference (libs/sfm/sift.cc):
 *   :24-37    the constructor: std::invalid_argument("Invalid octave range"), the contrast threshold 0.02 / samples for a
 *             negative one, debug_output switches verbose_output on,
 *   :135-165  set_image / set_float_image keep the grey float image `orig` on the host and throw
 *             std::invalid_argument("Gray or color image expected"),
 *   :51-57, :109-126  the verbose lines of process with their counts (the debug lines of the stages too, without times of
 *             their own: the stages run in one call),
 *   :871-906  load_lowe_descriptors.
 * What differs: process is one mi_dmrecon_sift_run + mi_dmrecon_sift_get on the GPU; keypoints and descriptors agree with the
 * reference's to rounding, not bit for bit (include/mi_dmrecon.h).  The protected stage members have no other caller and
 * throw std::logic_error.
 *
 * One context for the process, shared with every other drop-in of this directory that the binary links (shim_common.h): made
 * by the first call of any of them on the first entry of MI_DMRECON_DEVICES (default 0); every calling thread works on its
 * own fork (its own stream and buffers); all are released at exit.
 */
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "util/timer.h"
#include "mve/image.h"
#include "sfm/sift.h"

#include "shim_common.h"

SFM_NAMESPACE_BEGIN

namespace {

/* one grey float channel: a byte is value / 255 clamped to [0, 1], a colour is the mean of its three channels */
template <typename T>
mve::FloatImage::Ptr grey_image(typename mve::Image<T>::ConstPtr img)
{
    int const channels = img->channels();
    if (channels != 1 && channels != 3)
        throw std::invalid_argument("Gray or color image expected");
    mve::FloatImage::Ptr out = mve::FloatImage::create(img->width(), img->height(), 1);
    float const third = 1.0f / 3.0f;
    std::size_t const n = static_cast<std::size_t>(img->width()) * img->height();
    for (std::size_t i = 0; i < n; ++i)
    {
        float v[3];
        for (int c = 0; c < channels; ++c)
        {
            v[c] = static_cast<float>(img->at(i * channels + c));
            if (sizeof(T) == 1)
                v[c] = std::min(1.0f, std::max(0.0f, v[c] / 255.0f));
        }
        out->at(i) = channels == 3 ? v[0] * third + v[1] * third + v[2] * third : v[0];
    }
    return out;
}

}  /* namespace */

Sift::Sift (Options const& options)
    : options(options)
{
    if (this->options.min_octave < -1 || this->options.min_octave > this->options.max_octave)
        throw std::invalid_argument("Invalid octave range");
    if (this->options.contrast_threshold < 0.0f)
        this->options.contrast_threshold = 0.02f / static_cast<float>(this->options.num_samples_per_octave);
    if (this->options.debug_output)
        this->options.verbose_output = true;
}

void
Sift::set_image (mve::ByteImage::ConstPtr img)
{
    this->orig = grey_image<uint8_t>(img);
}

void
Sift::set_float_image (mve::FloatImage::ConstPtr img)
{
    this->orig = grey_image<float>(img);
}

void
Sift::process (void)
{
    util::ClockTimer total_timer;
    if (this->options.verbose_output)
    {
        std::cout << "SIFT: Creating " << (this->options.max_octave - this->options.min_octave) << " octaves ("
            << this->options.min_octave << " to " << this->options.max_octave << ")..." << std::endl;
    }
    if (this->orig == nullptr)
        throw std::invalid_argument("Gray or color image expected");

    static_assert(sizeof(Keypoint) == sizeof(mi_dmrecon_sift_keypoint), "a keypoint is octave, sample, x, y");
    mi_dmrecon_sift_options opt;
    opt.num_samples_per_octave = this->options.num_samples_per_octave;
    opt.min_octave = this->options.min_octave;
    opt.max_octave = this->options.max_octave;
    opt.contrast_threshold = this->options.contrast_threshold;
    opt.edge_ratio_threshold = this->options.edge_ratio_threshold;
    opt.base_blur_sigma = this->options.base_blur_sigma;
    opt.inherent_blur_sigma = this->options.inherent_blur_sigma;

    mi_dmrecon_ctx* ctx = mi_shim::context_of_this_thread("sfm::Sift");
    int32_t n_keypoints = 0, n_descriptors = 0;
    mi_shim::check_args(mi_dmrecon_sift_run(ctx, &opt, this->orig->begin(), 1, this->orig->width(), this->orig->height(), 1,
        &n_keypoints, &n_descriptors), "mi_dmrecon_sift_run");
    std::vector<mi_dmrecon_sift_keypoint> kp(n_keypoints);
    std::vector<float> xyso(static_cast<std::size_t>(n_descriptors) * 4), data(static_cast<std::size_t>(n_descriptors) * 128);
    mi_shim::check_args(mi_dmrecon_sift_get(ctx, kp.data(), xyso.data(), data.data()), "mi_dmrecon_sift_get");

    this->keypoints.resize(n_keypoints);
    for (int32_t i = 0; i < n_keypoints; ++i)
    {
        this->keypoints[i].octave = kp[i].octave;
        this->keypoints[i].sample = kp[i].sample;
        this->keypoints[i].x = kp[i].x;
        this->keypoints[i].y = kp[i].y;
    }
    this->descriptors.clear();
    this->descriptors.resize(n_descriptors);
    for (int32_t i = 0; i < n_descriptors; ++i)
    {
        Descriptor& d = this->descriptors[i];
        d.x = xyso[4 * i + 0];
        d.y = xyso[4 * i + 1];
        d.scale = xyso[4 * i + 2];
        d.orientation = xyso[4 * i + 3];
        std::memcpy(d.data.begin(), &data[static_cast<std::size_t>(i) * 128], 128 * sizeof(float));
    }

    if (this->options.debug_output)
        std::cout << "SIFT: Retained " << this->keypoints.size() << " stable keypoints." << std::endl;
    if (this->options.verbose_output)
    {
        std::cout << "SIFT: Generating keypoint descriptors..." << std::endl;
        std::cout << "SIFT: Generated " << this->descriptors.size() << " descriptors from " << this->keypoints.size()
            << " keypoints," << " took " << total_timer.get_elapsed() << "ms." << std::endl;
    }
    this->octaves.clear();
}

void
Sift::load_lowe_descriptors (std::string const& filename, Descriptors* result)
{
    /* Lowe's text format: the number of descriptors and 128, then per descriptor y x scale orientation and 128 values */
    std::ifstream in(filename.c_str());
    if (!in.good())
        throw std::runtime_error("Cannot open descriptor file");
    int count = 0, dimensions = 0;
    in >> count >> dimensions;
    if (count > 100000 || dimensions != 128)
        throw std::runtime_error("Invalid number of descriptors/dimensions");
    result->clear();
    result->reserve(count);
    for (int i = 0; i < count; ++i)
    {
        Descriptor d;
        in >> d.y >> d.x >> d.scale >> d.orientation;
        for (int j = 0; j < 128; ++j)
            in >> d.data[j];
        d.data.normalize();
        result->push_back(d);
    }
    if (!in.good())
    {
        result->clear();
        throw std::runtime_error("Error while reading descriptors");
    }
}

/* ---- the stages run inside mi_dmrecon_sift_run; nothing else calls these ---- */

#define MI_SIFT_STAGE(what) throw std::logic_error("sfm::Sift::" what " (MI355X build): the stages run inside process")

void Sift::create_octaves (void) { MI_SIFT_STAGE("create_octaves"); }
void Sift::add_octave (mve::FloatImage::ConstPtr, float, float) { MI_SIFT_STAGE("add_octave"); }
void Sift::extrema_detection (void) { MI_SIFT_STAGE("extrema_detection"); }
std::size_t Sift::extrema_detection (mve::FloatImage::ConstPtr*, int, int) { MI_SIFT_STAGE("extrema_detection"); }
void Sift::keypoint_localization (void) { MI_SIFT_STAGE("keypoint_localization"); }
void Sift::descriptor_generation (void) { MI_SIFT_STAGE("descriptor_generation"); }
void Sift::generate_grad_ori_images (Octave*) { MI_SIFT_STAGE("generate_grad_ori_images"); }
void Sift::orientation_assignment (Keypoint const&, Octave const*, std::vector<float>&) { MI_SIFT_STAGE("orientation_assignment"); }
bool Sift::descriptor_assignment (Keypoint const&, Descriptor&, Octave const*) { MI_SIFT_STAGE("descriptor_assignment"); }
float Sift::keypoint_relative_scale (Keypoint const&) { MI_SIFT_STAGE("keypoint_relative_scale"); }
float Sift::keypoint_absolute_scale (Keypoint const&) { MI_SIFT_STAGE("keypoint_absolute_scale"); }

SFM_NAMESPACE_END
