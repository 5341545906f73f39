/*
 * fssr_iso_octree.cc -- the four members of fssr::IsoOctree that the reference defines in libs/fssr/iso_octree.cc
 * (compute_voxels, compute_all_voxels, sample_ifn, print_progress), on top of libmi_dmrecon.so: linked INSTEAD of that one
 * file, with the rest of libs/fssr and apps/fssrecon unmodified, this makes build/fssrecon_mi (mve_amd/host/Makefile).
 * Compiled against the reference's own fssr/iso_octree.h (the class is the reference's; only these definitions are ours).
 *
 * Behaviour kept from the reference (libs/fssr/iso_octree.cc):
 *   :34-35  "Generated N voxels, took X ms."
 *   :42     "Computing sampling of the implicit function..."
 *   :43-66  the voxels are the unique VoxelIndex set of all leaf corners, in ascending index order,
 *   :68-69  "Sampling the implicit function at N positions, fetch a beer...",
 *   :215-250 the progress line (between the chunks the GPU works through, and once at 100 %).
 * Device choice: the first entry of MI_DMRECON_DEVICES (default 0), as the dmrecon shim reads it.
 */
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "util/string_utils.h"
#include "util/timer.h"
#include "fssr/iso_octree.h"

#include "mi_dmrecon.h"

FSSR_NAMESPACE_BEGIN

namespace {

int first_device(void)
{
    int const n = mi_dmrecon_device_count();
    if (n <= 0)
        throw std::runtime_error("fssr::IsoOctree (MI355X build): no HIP device available; there is no CPU path");
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

/* The tree as include/mi_dmrecon.h wants it: nodes breadth first (the eight children of a node consecutive and after it),
 * samples in the order Octree::influence_query visits them (a node's own, then its subtrees 0..7). */
struct FlatTree
{
    std::vector<mi_dmrecon_fssr_node> nodes;
    std::vector<mi_dmrecon_fssr_sample_t> samples;
};

void number_samples(Octree::Node const* node, std::size_t index, FlatTree* flat)
{
    flat->nodes[index].first_sample = static_cast<int32_t>(flat->samples.size());
    flat->nodes[index].n_samples = static_cast<int32_t>(node->samples.size());
    for (std::size_t i = 0; i < node->samples.size(); ++i)
    {
        Sample const& s = node->samples[i];
        mi_dmrecon_fssr_sample_t o;
        for (int j = 0; j < 3; ++j)
        {
            o.pos[j] = s.pos[j];
            o.normal[j] = s.normal[j];
            o.color[j] = s.color[j];
        }
        o.scale = s.scale;
        o.confidence = s.confidence;
        flat->samples.push_back(o);
    }
    if (node->children == nullptr)
        return;
    for (int k = 0; k < 8; ++k)
        number_samples(node->children + k, flat->nodes[index].first_child + k, flat);
}

void flatten(Octree const& octree, FlatTree* flat)
{
    if (octree.get_num_samples() >= (std::size_t(1) << 30) || octree.get_num_nodes() >= (std::size_t(1) << 30))
        throw std::runtime_error("fssr::IsoOctree (MI355X build): more than 2^30 samples or nodes");
    std::vector<Octree::Node const*> order(1, octree.get_root_node());
    for (std::size_t i = 0; i < order.size(); ++i)
    {
        mi_dmrecon_fssr_node n;
        n.first_child = order[i]->children ? static_cast<int32_t>(order.size()) : -1;
        n.first_sample = n.n_samples = n.reserved = 0;
        flat->nodes.push_back(n);
        if (order[i]->children)
            for (int k = 0; k < 8; ++k)
                order.push_back(order[i]->children + k);
    }
    flat->samples.reserve(octree.get_num_samples());
    number_samples(octree.get_root_node(), 0, flat);
}

}  /* namespace */

void
IsoOctree::compute_voxels (void)
{
    util::WallTimer timer;
    this->voxels.clear();
    this->compute_all_voxels();
    std::cout << "Generated " << this->voxels.size()
        << " voxels, took " << timer.get_elapsed() << "ms." << std::endl;
}

void
IsoOctree::compute_all_voxels (void)
{
    std::cout << "Computing sampling of the implicit function..." << std::endl;
    {
        std::set<VoxelIndex> voxel_set;
        Octree::Iterator iter = this->get_iterator_for_root();
        for (iter.first_leaf(); iter.current != nullptr; iter.next_leaf())
            for (int i = 0; i < 8; ++i)
            {
                VoxelIndex index;
                index.from_path_and_corner(iter.level, iter.path, i);
                voxel_set.insert(index);
            }
        this->voxels.clear();
        this->voxels.reserve(voxel_set.size());
        for (std::set<VoxelIndex>::const_iterator i = voxel_set.begin(); i != voxel_set.end(); ++i)
            this->voxels.push_back(std::make_pair(*i, VoxelData()));
    }

    std::cout << "Sampling the implicit function at " << this->voxels.size()
        << " positions, fetch a beer..." << std::endl;

    std::size_t const num = this->voxels.size();
    std::vector<double> pos(3 * num);
    for (std::size_t i = 0; i < num; ++i)
    {
        math::Vec3d const p = this->voxels[i].first.compute_position(
            this->get_root_node_center(), this->get_root_node_size());
        for (int j = 0; j < 3; ++j)
            pos[3 * i + j] = p[j];
    }

    FlatTree flat;
    flatten(*this, &flat);

    mi_dmrecon_ctx* ctx = nullptr;
    check(mi_dmrecon_ctx_create(first_device(), &ctx), "mi_dmrecon_ctx_create");
    mi_dmrecon_fssr* handle = nullptr;
    math::Vec3d const center = this->get_root_node_center();
    double const root_center[3] = { center[0], center[1], center[2] };
    int rc = mi_dmrecon_fssr_create(ctx, static_cast<int64_t>(flat.samples.size()), flat.samples.data(),
        static_cast<int64_t>(flat.nodes.size()), flat.nodes.data(), root_center, this->get_root_node_size(), &handle);
    std::string error;
    if (rc != 0)
        error = std::string("mi_dmrecon_fssr_create: ") + mi_dmrecon_last_error();

    std::vector<float> value(num), conf(num), scale(num), color(3 * num), deriv(3 * num);
    std::size_t const chunk = 1 << 16;
    for (std::size_t v0 = 0; rc == 0 && v0 < num; v0 += chunk)
    {
        std::size_t const m = std::min(chunk, num - v0);
        rc = mi_dmrecon_fssr_sample(handle, nullptr, static_cast<int64_t>(m), &pos[3 * v0], &value[v0], &conf[v0],
            &scale[v0], &color[3 * v0], &deriv[3 * v0], nullptr, nullptr);
        if (rc != 0)
            error = std::string("mi_dmrecon_fssr_sample: ") + mi_dmrecon_last_error();
        else
            this->print_progress(v0 + m, num);
    }
    mi_dmrecon_fssr_destroy(handle);
    mi_dmrecon_ctx_destroy(ctx);
    if (rc != 0)
        throw std::runtime_error(error);

    for (std::size_t i = 0; i < num; ++i)
    {
        VoxelData& d = this->voxels[i].second;
        d.value = value[i];
        d.conf = conf[i];
        d.scale = scale[i];
        for (int j = 0; j < 3; ++j)
        {
            d.color[j] = color[3 * i + j];
            d.deriv[j] = deriv[3 * i + j];
        }
    }

    /* Print progress one last time to get the 100% progress output. */
    this->print_progress(num, num);
    std::cout << std::endl;
}

VoxelData
IsoOctree::sample_ifn (math::Vec3d const& /*voxel_pos*/)
{
    /* private, and compute_all_voxels above is its only caller in the reference: the voxels are sampled there, all at once */
    throw std::logic_error("fssr::IsoOctree::sample_ifn (MI355X build): voxels are sampled by compute_all_voxels");
}

void
IsoOctree::print_progress (std::size_t voxels_done, std::size_t voxels_total)
{
    static util::WallTimer timer;
    static std::size_t last_elapsed = 0;

    /* not more often than every 100 ms, except for the last line */
    std::size_t const elapsed = timer.get_elapsed();
    if (voxels_done != voxels_total && elapsed - last_elapsed < 100)
        return;
    last_elapsed = elapsed;

    float const percentage = static_cast<float>(voxels_done) / static_cast<float>(voxels_total);
    std::size_t const total = static_cast<std::size_t>(elapsed / percentage);
    std::size_t const remaining = total - elapsed;
    std::cout << "\rProcessing voxel " << voxels_done
        << " (" << util::string::get_fixed(percentage * 100.0f, 2) << "%, "
        << elapsed / (1000 * 60) << ":" << util::string::get_filled((elapsed / 1000) % 60, 2, '0') << ", ETA "
        << remaining / (1000 * 60) << ":" << util::string::get_filled((remaining / 1000) % 60, 2, '0') << ")..."
        << std::flush;
}

FSSR_NAMESPACE_END
