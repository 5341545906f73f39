/*
 * ref_fssr_driver.cc -- TEST INFRASTRUCTURE: our own driver against the reference's fssr classes (libs/fssr), compiled
 * and run by tests/golden/make_golden_fssr.py only (by hand, where the reference tree exists; never by build()).
 *
 *   ref_fssr_driver voxels IN.ply OUTDIR   the octree of apps/fssrecon for IN.ply, flattened as include/mi_dmrecon.h
 *                                          describes it, and IsoOctree::compute_voxels' result per voxel, as raw arrays
 *   ref_fssr_driver mesh IN.ply OUTDIR     the mesh apps/fssrecon writes (fssrecon.cc:40-132), as raw arrays
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "fssr/iso_octree.h"
#include "fssr/iso_surface.h"
#include "fssr/sample_io.h"
#include "mve/mesh.h"

namespace {

template <typename T>
void dump(std::string const& dir, char const* name, std::vector<T> const& v) {
    std::string const path = dir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::perror(path.c_str()); std::exit(1); }
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    std::fclose(f);
}

void load(fssr::IsoOctree& octree, std::string const& ply) {
    fssr::SampleIO::Options opts;
    fssr::SampleIO loader(opts);
    loader.open_file(ply);
    fssr::Sample sample;
    while (loader.next_sample(&sample)) octree.insert_sample(sample);
    octree.limit_octree_level();
}

struct Flat {
    std::vector<int32_t> nodes;      /* first_child, first_sample, n_samples, 0 */
    std::vector<float> samples;      /* 11 floats each, in the order influence_query visits them */
};

/* samples: a node's own, then its subtrees 0..7 */
void number_samples(fssr::Octree::Node const* node, int32_t index, Flat& flat, std::vector<int32_t> const& first_child) {
    flat.nodes[4 * index + 1] = (int32_t)(flat.samples.size() / 11);
    flat.nodes[4 * index + 2] = (int32_t)node->samples.size();
    for (fssr::Sample const& s : node->samples) {
        for (int j = 0; j < 3; ++j) flat.samples.push_back(s.pos[j]);
        for (int j = 0; j < 3; ++j) flat.samples.push_back(s.normal[j]);
        for (int j = 0; j < 3; ++j) flat.samples.push_back(s.color[j]);
        flat.samples.push_back(s.scale);
        flat.samples.push_back(s.confidence);
    }
    if (node->children == nullptr) return;
    for (int k = 0; k < 8; ++k) number_samples(node->children + k, first_child[index] + k, flat, first_child);
}

Flat flatten(fssr::Octree const& octree) {
    /* nodes breadth first: the eight children of a node are consecutive and lie after it */
    std::vector<fssr::Octree::Node const*> order(1, octree.get_root_node());
    std::vector<int32_t> first_child;
    for (std::size_t i = 0; i < order.size(); ++i) {
        fssr::Octree::Node const* n = order[i];
        first_child.push_back(n->children ? (int32_t)order.size() : -1);
        if (n->children) for (int k = 0; k < 8; ++k) order.push_back(n->children + k);
    }
    Flat flat;
    flat.nodes.assign(4 * order.size(), 0);
    for (std::size_t i = 0; i < order.size(); ++i) flat.nodes[4 * i] = first_child[i];
    number_samples(octree.get_root_node(), 0, flat, first_child);
    return flat;
}

int voxels(std::string const& ply, std::string const& dir) {
    fssr::IsoOctree octree;
    load(octree, ply);
    Flat const flat = flatten(octree);
    dump(dir, "nodes.i32", flat.nodes);
    dump(dir, "samples.f32", flat.samples);
    math::Vec3d const c = octree.get_root_node_center();
    dump(dir, "root.f64", std::vector<double>{c[0], c[1], c[2], octree.get_root_node_size()});

    octree.compute_voxels();
    fssr::IsoOctree::VoxelVector const& vox = octree.get_voxels();
    std::vector<uint64_t> index;
    std::vector<double> pos;
    std::vector<float> data, max_scale;
    std::vector<int32_t> n_infl;
    std::vector<fssr::Sample const*> found;
    for (std::size_t i = 0; i < vox.size(); ++i) {
        index.push_back(vox[i].first.index);
        math::Vec3d const p = vox[i].first.compute_position(octree.get_root_node_center(), octree.get_root_node_size());
        for (int j = 0; j < 3; ++j) pos.push_back(p[j]);
        fssr::VoxelData const& d = vox[i].second;
        data.push_back(d.value); data.push_back(d.conf); data.push_back(d.scale);
        for (int j = 0; j < 3; ++j) data.push_back(d.color[j]);
        for (int j = 0; j < 3; ++j) data.push_back(d.deriv[j]);
        /* what sample_ifn derives from the query (iso_octree.cc:97-112) */
        octree.influence_query(p, 3.0, &found);
        n_infl.push_back((int32_t)found.size());
        float ms = 0.0f;
        if (!found.empty()) {
            std::size_t const k = found.size() / 10;
            std::nth_element(found.begin(), found.begin() + k, found.end(), fssr::sample_scale_compare);
            ms = found[k]->scale * 2.0f;
        }
        max_scale.push_back(ms);
    }
    dump(dir, "vox_index.u64", index);
    dump(dir, "vox_pos.f64", pos);
    dump(dir, "vox_data.f32", data);
    dump(dir, "vox_n.i32", n_infl);
    dump(dir, "vox_max_scale.f32", max_scale);
    return 0;
}

int mesh(std::string const& ply, std::string const& dir) {
    fssr::IsoOctree octree;
    load(octree, ply);
    octree.compute_voxels();
    octree.clear_samples();
    fssr::IsoSurface iso_surface(&octree, fssr::INTERPOLATION_CUBIC);
    mve::TriangleMesh::Ptr m = iso_surface.extract_mesh();
    octree.clear();
    mve::TriangleMesh::DeleteList del(m->get_vertices().size(), false);
    for (std::size_t i = 0; i < del.size(); ++i)
        if (m->get_vertex_confidences()[i] == 0.0f) del[i] = true;
    m->delete_vertices_fix_faces(del);
    std::vector<float> verts;
    for (math::Vec3f const& v : m->get_vertices()) for (int j = 0; j < 3; ++j) verts.push_back(v[j]);
    dump(dir, "mesh_verts.f32", verts);
    dump(dir, "mesh_faces.u32", std::vector<uint32_t>(m->get_faces().begin(), m->get_faces().end()));
    dump(dir, "mesh_conf.f32", std::vector<float>(m->get_vertex_confidences().begin(), m->get_vertex_confidences().end()));
    dump(dir, "mesh_values.f32", std::vector<float>(m->get_vertex_values().begin(), m->get_vertex_values().end()));
    return 0;
}

}  /* namespace */

int main(int argc, char** argv) {
    if (argc != 4) { std::cerr << "usage: ref_fssr_driver voxels|mesh IN.ply OUTDIR" << std::endl; return 2; }
    std::string const mode = argv[1];
    try {
        if (mode == "voxels") return voxels(argv[2], argv[3]);
        if (mode == "mesh") return mesh(argv[2], argv[3]);
    } catch (std::exception& e) { std::cerr << "Error: " << e.what() << std::endl; return 1; }
    return 2;
}
