/*
 * sfm_surf.cc -- the members of sfm::Surf that the reference defines in libs/sfm/surf.cc, on top of libmi_dmrecon.so: linked
 * INSTEAD of that one file, with the rest of libs/sfm and apps/sfmrecon unmodified (mve_amd/host/Makefile, build/sfmrecon_mi).
 * Compiled against the reference's own sfm/surf.h (the class, its Options, Keypoint and Descriptor are the reference's; only
 * these definitions are ours).
 *
 * Behaviour kept from the reference (libs/sfm/surf.cc):
 *   :39-44    the constructor: debug_output switches verbose_output on,
 *   :123-138  set_image throws std::invalid_argument("Gray or color image expected"),
 *   :58-61, :98-115  the verbose lines of process with their counts (the debug lines of the stages too, without times of
 *             their own: the stages run in one call).
 * What differs: set_image keeps the byte image instead of a summed-area table (the table is built on the device), in the
 * class's own `sat` member: a one-channel int64 image of ceil(bytes / 8) + 3 values that holds width, height, channels and
 * then the bytes.  process is one mi_dmrecon_surf_run + mi_dmrecon_surf_get on the GPU and, like the reference, releases
 * `sat`.  The protected stage members have no other caller and throw std::logic_error.
 *
 * One context for the process, shared with every other drop-in of this directory that the binary links (shim_common.h): made
 * by the first call of any of them on the first entry of MI_DMRECON_DEVICES (default 0); every calling thread works on its
 * own fork (its own stream and buffers); all are released at exit.
 */
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "util/timer.h"
#include "mve/image.h"
#include "sfm/surf.h"

#include "shim_common.h"

SFM_NAMESPACE_BEGIN

Surf::Surf (Options const& options)
    : options(options)
{
    if (this->options.debug_output)
        this->options.verbose_output = true;
}

void
Surf::set_image (mve::ByteImage::ConstPtr image)
{
    if (image->channels() != 1 && image->channels() != 3)
        throw std::invalid_argument("Gray or color image expected");
    std::size_t const bytes = image->get_byte_size();
    this->sat = SatImage::create(static_cast<int>((bytes + 7) / 8 + 3), 1, 1);
    this->sat->at(0) = image->width();
    this->sat->at(1) = image->height();
    this->sat->at(2) = image->channels();
    std::memcpy(&this->sat->at(3), image->get_byte_pointer(), bytes);
}

void
Surf::process (void)
{
    this->keypoints.clear();
    this->descriptors.clear();
    this->octaves.clear();

    util::WallTimer total_timer;
    if (this->options.verbose_output)
        std::cout << "SURF: Creating 4 octaves (0 to 4)..." << std::endl;
    if (this->sat == nullptr)
        throw std::invalid_argument("Gray or color image expected");

    static_assert(sizeof(Keypoint) == sizeof(mi_dmrecon_surf_keypoint), "a keypoint is octave, sample, x, y");
    mi_dmrecon_surf_options opt;
    opt.contrast_threshold = this->options.contrast_threshold;
    opt.use_upright_descriptor = this->options.use_upright_descriptor ? 1 : 0;

    mi_dmrecon_ctx* ctx = mi_shim::context_of_this_thread("sfm::Surf");
    int32_t n_keypoints = 0, n_descriptors = 0;
    mi_shim::check_args(mi_dmrecon_surf_run(ctx, &opt, reinterpret_cast<uint8_t const*>(&this->sat->at(3)), static_cast<int32_t>(this->sat->at(0)),
        static_cast<int32_t>(this->sat->at(1)), static_cast<int32_t>(this->sat->at(2)), &n_keypoints, &n_descriptors),
        "mi_dmrecon_surf_run");
    this->keypoints.resize(n_keypoints);
    std::vector<float> xyso(static_cast<std::size_t>(n_descriptors) * 4), data(static_cast<std::size_t>(n_descriptors) * 64);
    mi_shim::check_args(mi_dmrecon_surf_get(ctx, reinterpret_cast<mi_dmrecon_surf_keypoint*>(this->keypoints.data()), xyso.data(), data.data()),
        "mi_dmrecon_surf_get");

    if (this->options.debug_output)
    {
        std::cout << "SURF: Detecting local extrema..." << std::endl;
        std::cout << "SURF: Localizing and filtering keypoints..." << std::endl;
    }
    if (this->options.verbose_output)
        std::cout << "SURF: Generating keypoint descriptors..." << std::endl;

    this->descriptors.resize(n_descriptors);
    for (int32_t i = 0; i < n_descriptors; ++i)
    {
        Descriptor& d = this->descriptors[i];
        d.x = xyso[4 * i + 0];
        d.y = xyso[4 * i + 1];
        d.scale = xyso[4 * i + 2];
        d.orientation = xyso[4 * i + 3];
        std::memcpy(d.data.begin(), &data[static_cast<std::size_t>(i) * 64], 64 * sizeof(float));
    }

    if (this->options.debug_output)
    {
        std::cout << "SURF: Generated " << this->descriptors.size() << " descriptors, took " << total_timer.get_elapsed()
            << "ms." << std::endl;
    }
    if (this->options.verbose_output)
    {
        std::cout << "SURF: Generated " << this->descriptors.size() << " descriptors from " << this->keypoints.size()
            << " keypoints," << " took " << total_timer.get_elapsed() << "ms." << std::endl;
    }
    this->sat.reset();
}

/* ---- the stages run inside mi_dmrecon_surf_run; nothing else calls these ---- */

#define MI_SURF_STAGE(what) throw std::logic_error("sfm::Surf::" what " (MI355X build): the stages run inside process")

void Surf::create_octaves (void) { MI_SURF_STAGE("create_octaves"); }
void Surf::create_response_map (int, int) { MI_SURF_STAGE("create_response_map"); }
Surf::SatType Surf::filter_dxx (int, int, int) { MI_SURF_STAGE("filter_dxx"); }
Surf::SatType Surf::filter_dyy (int, int, int) { MI_SURF_STAGE("filter_dyy"); }
Surf::SatType Surf::filter_dxy (int, int, int) { MI_SURF_STAGE("filter_dxy"); }
void Surf::extrema_detection (void) { MI_SURF_STAGE("extrema_detection"); }
void Surf::check_maximum (int, int, int, int) { MI_SURF_STAGE("check_maximum"); }
void Surf::keypoint_localization_and_filtering (void) { MI_SURF_STAGE("keypoint_localization_and_filtering"); }
bool Surf::keypoint_localization (Surf::Keypoint*) { MI_SURF_STAGE("keypoint_localization"); }
void Surf::descriptor_assignment (void) { MI_SURF_STAGE("descriptor_assignment"); }
bool Surf::descriptor_orientation (Descriptor*) { MI_SURF_STAGE("descriptor_orientation"); }
bool Surf::descriptor_computation (Descriptor*, bool) { MI_SURF_STAGE("descriptor_computation"); }
void Surf::filter_dx_dy (int, int, int, float*, float*) { MI_SURF_STAGE("filter_dx_dy"); }

SFM_NAMESPACE_END
