/*
 * ref_ba_driver.cc -- runs sfm::ba::BundleAdjustment on the problems of a file and writes what it leaves behind.  Linked
 * against the reference's libs/sfm/bundle_adjustment.cc and ba_linear_solver.cc by tests/golden/make_golden_ba.py (the
 * fixture), and against mve_amd/host/sfm_bundle_adjustment.cc by mve_amd/host/Makefile (build/ba_class_check).
 *
 *   ref_ba_driver IN OUT
 * IN:  int32 n_cases, then per case  int32 mode, fixed_intrinsics, lm_max_iterations, n_cameras, n_points, n_observations;
 *      double cameras[n][15] (f k0 k1 t R); double points[m][3]; int32 is_constant[m]; double xy[o][2]; int32 camera_id[o];
 *      int32 point_id[o].
 * OUT: per case  double cameras[n][15]; double points[m][3]; double initial_mse, final_mse; int32 LM iterations, successful,
 *      unsuccessful, CG iterations.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sfm/bundle_adjustment.h"

namespace {

template <typename T>
std::vector<T> read(std::FILE* f, std::size_t n)
{
    std::vector<T> v(n);
    if (n > 0 && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    return v;
}

}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t const n_cases = read<int32_t>(in, 1)[0];
    for (int32_t c = 0; c < n_cases; ++c)
    {
        std::vector<int32_t> const h = read<int32_t>(in, 6);
        std::vector<double> const cam = read<double>(in, (std::size_t)h[3] * 15);
        std::vector<double> const pt = read<double>(in, (std::size_t)h[4] * 3);
        std::vector<int32_t> const constant = read<int32_t>(in, h[4]);
        std::vector<double> const xy = read<double>(in, (std::size_t)h[5] * 2);
        std::vector<int32_t> const cid = read<int32_t>(in, h[5]);
        std::vector<int32_t> const pid = read<int32_t>(in, h[5]);

        std::vector<sfm::ba::Camera> cameras(h[3]);
        std::vector<sfm::ba::Point3D> points(h[4]);
        std::vector<sfm::ba::Observation> observations(h[5]);
        for (int i = 0; i < h[3]; ++i)
        {
            double const* q = &cam[(std::size_t)i * 15];
            cameras[i].focal_length = q[0];
            for (int k = 0; k < 2; ++k) cameras[i].distortion[k] = q[1 + k];
            for (int k = 0; k < 3; ++k) cameras[i].translation[k] = q[3 + k];
            for (int k = 0; k < 9; ++k) cameras[i].rotation[k] = q[6 + k];
        }
        for (int i = 0; i < h[4]; ++i)
        {
            for (int k = 0; k < 3; ++k) points[i].pos[k] = pt[(std::size_t)i * 3 + k];
            points[i].is_constant = constant[i] != 0;
        }
        for (int i = 0; i < h[5]; ++i)
        {
            observations[i].pos[0] = xy[(std::size_t)i * 2];
            observations[i].pos[1] = xy[(std::size_t)i * 2 + 1];
            observations[i].camera_id = cid[i];
            observations[i].point_id = pid[i];
        }

        sfm::ba::BundleAdjustment::Options opts;
        opts.bundle_mode = static_cast<sfm::ba::BundleAdjustment::BAMode>(h[0]);
        opts.fixed_intrinsics = h[1] != 0;
        opts.lm_max_iterations = h[2];
        sfm::ba::BundleAdjustment ba(opts);
        ba.set_cameras(&cameras);
        ba.set_points(&points);
        ba.set_observations(&observations);
        sfm::ba::BundleAdjustment::Status const st = ba.optimize();

        for (int i = 0; i < h[3]; ++i)
        {
            double q[15];
            q[0] = cameras[i].focal_length;
            for (int k = 0; k < 2; ++k) q[1 + k] = cameras[i].distortion[k];
            for (int k = 0; k < 3; ++k) q[3 + k] = cameras[i].translation[k];
            for (int k = 0; k < 9; ++k) q[6 + k] = cameras[i].rotation[k];
            std::fwrite(q, sizeof(double), 15, out);
        }
        for (int i = 0; i < h[4]; ++i) std::fwrite(points[i].pos, sizeof(double), 3, out);
        double const m[2] = { st.initial_mse, st.final_mse };
        int32_t const n[4] = { st.num_lm_iterations, st.num_lm_successful_iterations, st.num_lm_unsuccessful_iterations, st.num_cg_iterations };
        std::fwrite(m, sizeof(double), 2, out);
        std::fwrite(n, sizeof(int32_t), 4, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
