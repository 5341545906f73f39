/*
 * fssr_device.hip -- the implicit function of Floating Scale Surface Reconstruction sampled at the octree corners
 * ("voxels") on the GPU: fssr::IsoOctree::sample_ifn (libs/fssr/iso_octree.cc:93-169, the FSSR_USE_DERIVATIVES branch that
 * defines.h:17-20 select) per voxel position.
 *
 * One wavefront per voxel, four voxels per 256-thread block; the wavefronts of a block never synchronise with each other.
 *
 *   1. influence query (octree.cc:346-400, factor 3.0): the flattened octree is walked from the root with an explicit
 *      per-level stack (no recursion).  The walk is the same in all 64 lanes; the lanes split a node's samples, and the
 *      accepted ones are appended in walk order (ballot + prefix popcount) to the wavefront's list in LDS.
 *   2. scale cut (iso_octree.cc:109-112): the floor(n/10)-th smallest scale of the accepted samples, found by a bitwise
 *      search over the scales' bit patterns (positive floats order like their bits): exact, ties included.
 *   3. accumulation (iso_octree.cc:127-169, basis_function.cc:20-74, basis_function.h:93-164) in double: the term of the
 *      i-th accepted sample goes into the partial sums of lane i mod 64, in ascending i; the 64 partials are combined in one
 *      fixed butterfly.
 *
 * The first FSSR_LIST_MAX entries of a list are in LDS, the rest in the wavefront's slice of a global buffer (the host sizes it
 * by the number of samples, so that it covers every voxel of all but very dense point sets).
 * A voxel with more accepted samples than the list holds walks the tree again: for every step of the selection and once for
 * the sums, where the j-th accepted sample of a 64-sample chunk is handed to the lane its index selects.  Both forms add the
 * same terms to the same lanes in the same order, so they agree bit for bit -- as does the walk without a tree (n_nodes = 0:
 * every sample tested in index order; the samples are stored in walk order).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fssr_device.h"

/* every product and sum below is the reference's own operation: nothing is fused */
#pragma clang fp contract(off)

#define FSSR_PI       3.14159265358979323846264338327950288      /* MATH_PI       (math/defines.h:42) */
#define FSSR_SQRT_2PI 2.506628274631000502415765284811045253     /* MATH_SQRT_2PI (math/defines.h:54) */
#define FSSR_SQRT3    1.7320508075688772935274463415058723669    /* MATH_SQRT3    (math/defines.h:50) */

struct FssrStack {                /* per wavefront, in LDS: the state of the walk per level */
    double ctr[FSSR_MAX_LEVELS][3];   /* centre of the node being visited at that level */
    int32_t first[FSSR_MAX_LEVELS];   /* index of child 0 of the node's parent */
    int32_t oct[FSSR_MAX_LEVELS];     /* octant of the node being visited */
};

struct FssrAcc {                  /* the partial sums of one lane (iso_octree.cc:127-133) */
    double tv, tw, ts, tcw, tvd[3], twd[3], tc[3];
};

/* a list entry written by one lane is read by another lane of the same wavefront: from LDS ... */
__device__ __forceinline__ void fssr_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
/* ... or from the wavefront's slice of global memory */
__device__ __forceinline__ void fssr_list_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
    __builtin_amdgcn_wave_barrier();
}

/* Vector::square_norm / dot: std::accumulate from T(0) (math/vector.h:441-444, :542-545) */
__device__ __forceinline__ double fssr_sqn(double a, double b, double c) { return ((0.0 + a * a) + b * b) + c * c; }

/* octree.cc:389: a sample is dropped when (pos - s.pos).square_norm() > MATH_POW2(factor * s.scale) */
__device__ __forceinline__ bool fssr_accept(const double* p, const FssrSample& s) {
    const double d0 = p[0] - (double)s.pos[0], d1 = p[1] - (double)s.pos[1], d2 = p[2] - (double)s.pos[2];
    const double r = 3.0 * (double)s.scale;
    return !(fssr_sqn(d0, d1, d2) > r * r);
}

/* Walks the tree as Octree::influence_query does (a node's own samples, then children 0..7) and calls
 * f(first_sample, n_samples) for every node that is not ruled out.  Uniform across the wavefront. */
template <typename F>
__device__ __forceinline__ void fssr_walk(const FssrTree& T, const double* p, FssrStack& st, F f) {
    if (T.n_nodes == 0) { f(0, T.n_samples); return; }
    int level = 0, node = 0, oct = 0;
    for (;;) {
        /* octree.cc:368-376: the centre from the parent's */
        const double node_size = T.root_size / (double)(1 << level);
        const double offset = (double)(level > 0) * node_size / 2.0;
        double c[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double parent = level > 0 ? st.ctr[level - 1][j] : T.root_center[j];
            c[j] = parent - offset + (double)((oct >> j) & 1) * node_size;
        }
        /* octree.cc:379-383 */
        const double min_distance = sqrt(fssr_sqn(p[0] - c[0], p[1] - c[1], p[2] - c[2])) - FSSR_SQRT3 * node_size / 2.0;
        const double max_scale = node_size * 2.0;
        bool descend = false;
        if (!(min_distance > max_scale * 3.0)) {
            const FssrNode nd = T.nodes[node];
            const int first_sample = __builtin_amdgcn_readfirstlane(nd.first_sample);
            const int n_samples = __builtin_amdgcn_readfirstlane(nd.n_samples);
            const int first_child = __builtin_amdgcn_readfirstlane(nd.first_child);
            if (n_samples > 0) f(first_sample, n_samples);
            if (first_child >= 0 && level + 1 < FSSR_MAX_LEVELS) {
                st.ctr[level][0] = c[0]; st.ctr[level][1] = c[1]; st.ctr[level][2] = c[2];
                ++level;
                st.first[level] = first_child; st.oct[level] = 0;
                node = first_child; oct = 0;
                descend = true;
            }
        }
        if (descend) continue;
        /* next sibling, or the next sibling of the closest ancestor that has one */
        while (level > 0 && st.oct[level] == 7) --level;
        if (level == 0) return;
        oct = st.oct[level] + 1;
        st.oct[level] = oct;
        node = st.first[level] + oct;
    }
}

/* position of the j-th set bit of m (j < popcount(m)) */
__device__ __forceinline__ int fssr_nth_bit(unsigned long long m, int j) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const unsigned long long low = m & ((1ull << w) - 1ull);
        const int c = __popcll(low);
        if (j >= c) { j -= c; m >>= w; pos += w; } else m = low;
    }
    return pos;
}

/* predicate_epsilon_equal (math/algo.h:135-141) as Vector::is_similar applies it: v1 = own component, v2 = other's */
__device__ __forceinline__ bool fssr_eps_eq(float v1, float v2, float eps) { return v1 - eps <= v2 && v2 <= v1 + eps; }

/* rotation_from_normal (basis_function.cc:49-74), row-major */
__device__ __forceinline__ void fssr_rotation(const float* n, float* R) {
    if (fssr_eps_eq(n[0], 1.0f, 0.001f) && fssr_eps_eq(n[1], 0.0f, 0.001f) && fssr_eps_eq(n[2], 0.0f, 0.001f)) {
        R[0] = 1.f; R[1] = 0.f; R[2] = 0.f; R[3] = 0.f; R[4] = 1.f; R[5] = 0.f; R[6] = 0.f; R[7] = 0.f; R[8] = 1.f;
        return;
    }
    if (fssr_eps_eq(n[0], -1.0f, 0.001f) && fssr_eps_eq(n[1], 0.0f, 0.001f) && fssr_eps_eq(n[2], 0.0f, 0.001f)) {
        R[0] = -1.f; R[1] = 0.f; R[2] = 0.f; R[3] = 0.f; R[4] = -1.f; R[5] = 0.f; R[6] = 0.f; R[7] = 0.f; R[8] = 1.f;
        return;
    }
    /* axis1 = normal.cross(ref).normalized(), ref = (1, 0, 0): cross_product (math/vector.h:370-375) term by term */
    float a[3];
    a[0] = n[1] * 0.0f - n[2] * 0.0f;
    a[1] = n[2] * 1.0f - n[0] * 0.0f;
    a[2] = n[0] * 0.0f - n[1] * 1.0f;
    const float len = sqrtf(((0.0f + a[0] * a[0]) + a[1] * a[1]) + a[2] * a[2]);
    a[0] /= len; a[1] /= len; a[2] /= len;
    R[0] = n[0]; R[1] = n[1]; R[2] = n[2];
    R[3] = a[0]; R[4] = a[1]; R[5] = a[2];
    R[6] = n[1] * a[2] - n[2] * a[1];
    R[7] = n[2] * a[0] - n[0] * a[2];
    R[8] = n[0] * a[1] - n[1] * a[0];
}

/* one sample's term of the sums (iso_octree.cc:135-160 with evaluate(), basis_function.cc:20-44) */
__device__ __forceinline__ void fssr_term(const double* p, const float* pf, const FssrSample& s, FssrAcc& A) {
    /* rotate the voxel position into the sample's frame, in float (Matrix3f * Vec3f: std::inner_product from 0) */
    float R[9];
    fssr_rotation(s.normal, R);
    const float d0 = pf[0] - s.pos[0], d1 = pf[1] - s.pos[1], d2 = pf[2] - s.pos[2];
    double x[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = (double)(((0.0f + R[3 * i] * d0) + R[3 * i + 1] * d1) + R[3 * i + 2] * d2);
    const double sc = (double)s.scale;
    const double sc2 = sc * sc;
    const double sqn = fssr_sqn(x[0], x[1], x[2]);

    /* fssr_basis<double> (basis_function.h:109-127) */
    const double g = exp(-sqn / (2.0 * sc2));
    const double value_norm = 2.0 * FSSR_PI * (sc2 * sc2);
    const double deriv_norm = value_norm * 2.0 * sc2;
    double vd[3];
    vd[0] = 2.0 * (sc2 - x[0] * x[0]) * g / deriv_norm;
    vd[1] = (-2.0 * x[0] * x[1]) * g / deriv_norm;
    vd[2] = (-2.0 * x[0] * x[2]) * g / deriv_norm;
    const double value = x[0] * g / value_norm;

    /* fssr_weight<double>, the new weight function (basis_function.h:133-164) */
    const double sr = sqn / sc2;
    double weight = 0.0, wd[3] = {0.0, 0.0, 0.0};
    if (!(sr >= 9.0)) {
        const double df = -4.0 / 3.0 + 48.0 / 54.0 * sqrt(sr) - 4.0 / 27.0 * sr;
        wd[0] = df * x[0] / sc;
        wd[1] = df * x[1] / sc;
        wd[2] = df * x[2] / sc;
        weight = 1.0 - 2.0 / 3.0 * sr + 8.0 / 27.0 * pow(sr, 1.5) - 1.0 / 27.0 * (sr * sr);
    }

    /* the derivatives back in world coordinates: Matrix3f::mult takes a Vec3f, so they are narrowed to float, multiplied
     * in float with the transposed rotation and widened again (basis_function.cc:39-43) */
    const float vf[3] = {(float)vd[0], (float)vd[1], (float)vd[2]};
    const float wf[3] = {(float)wd[0], (float)wd[1], (float)wd[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        vd[i] = (double)(((0.0f + R[i] * vf[0]) + R[3 + i] * vf[1]) + R[6 + i] * vf[2]);
        wd[i] = (double)(((0.0f + R[i] * wf[0]) + R[3 + i] * wf[1]) + R[6 + i] * wf[2]);
    }

    const double conf = (double)s.confidence;
    A.tv += value * weight * conf;
    A.tw += weight * conf;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        A.tvd[i] += (vd[i] * weight + wd[i] * value) * conf;
        A.twd[i] += wd[i] * conf;
    }

    /* colour and scale: gaussian_normalized<double>(s.scale / 5.0f, voxel_pos - s.pos) * confidence */
    const double sigma = (double)(s.scale / 5.0f);
    const double e0 = p[0] - (double)s.pos[0], e1 = p[1] - (double)s.pos[1], e2 = p[2] - (double)s.pos[2];
    const double cw = exp(-fssr_sqn(e0, e1, e2) / (2.0 * (sigma * sigma))) / (sigma * FSSR_SQRT_2PI) * conf;
    A.ts += sc * cw;
    const float cwf = (float)cw;                      /* Vec3f * double: the weight is narrowed (Vector<float,3>::operator*) */
#pragma unroll
    for (int i = 0; i < 3; ++i) A.tc[i] += (double)(s.color[i] * cwf);
    A.tcw += cw;
}

__device__ __forceinline__ double fssr_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

/* one voxel by one wavefront; idx / key: the wavefront's list in LDS, g: its continuation in global memory */
__device__ __forceinline__ void fssr_voxel(const FssrTree& T, int cap, int32_t* idx, uint32_t* key, uint2* g, FssrStack& st, int lane,
                                           long long v, const double* __restrict__ positions, const FssrOut& out) {
    const unsigned long long lt = (1ull << lane) - 1ull;
    const double p[3] = {positions[3 * v], positions[3 * v + 1], positions[3 * v + 2]};
    const float pf[3] = {(float)p[0], (float)p[1], (float)p[2]};

    /* 1. influence query */
    int n = 0;
    fssr_walk(T, p, st, [&](int first, int cnt) {
        for (int base = 0; base < cnt; base += 64) {
            const int i = first + base + lane;
            bool ok = false;
            uint32_t k = 0;
            if (base + lane < cnt) {
                const FssrSample& s = T.samples[i];
                ok = fssr_accept(p, s);
                k = __float_as_uint(s.scale);
            }
            const unsigned long long mask = __ballot(ok);
            if (ok) {
                const int slot = n + __popcll(mask & lt);
                if (slot < cap) {
                    if (slot < FSSR_LIST_MAX) { idx[slot] = i; key[slot] = k; }
                    else g[slot - FSSR_LIST_MAX] = make_uint2((unsigned)i, k);
                }
            }
            n += __popcll(mask);
        }
    });
    fssr_list_fence();

    FssrAcc A;
    A.tv = A.tw = A.ts = A.tcw = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) A.tvd[i] = A.twd[i] = A.tc[i] = 0.0;
    float max_scale = 0.0f;

    if (n > 0) {
        /* 2. the floor(n/10)-th smallest scale: the largest x with #{key < x} <= k, bit by bit (bit 31 is the sign) */
        const int k = n / 10;
        const bool listed = n <= cap;
        uint32_t sel = 0;
        for (int bit = 30; bit >= 0; --bit) {
            const uint32_t cand = sel | (1u << bit);
            int below = 0;
            if (listed) {
                for (int j0 = 0; j0 < n; j0 += 64) {
                    const int j = j0 + lane;
                    bool hit = false;
                    if (j < n) hit = (j < FSSR_LIST_MAX ? key[j] : g[j - FSSR_LIST_MAX].y) < cand;
                    below += __popcll(__ballot(hit));
                }
            } else {
                fssr_walk(T, p, st, [&](int first, int cnt) {
                    for (int base = 0; base < cnt; base += 64) {
                        bool hit = false;
                        if (base + lane < cnt) {
                            const FssrSample& s = T.samples[first + base + lane];
                            hit = fssr_accept(p, s) && __float_as_uint(s.scale) < cand;
                        }
                        below += __popcll(__ballot(hit));
                    }
                });
            }
            if (below <= k) sel = cand;
        }
        max_scale = __uint_as_float(sel) * 2.0f;

        /* 3. the sums: accepted sample i on lane i mod 64, ascending i */
        if (listed) {
            for (int j = lane; j < n; j += 64) {
                const FssrSample s = T.samples[j < FSSR_LIST_MAX ? idx[j] : (int)g[j - FSSR_LIST_MAX].x];
                if (!(s.scale > max_scale)) fssr_term(p, pf, s, A);
            }
        } else {
            int m = 0;
            fssr_walk(T, p, st, [&](int first, int cnt) {
                for (int base = 0; base < cnt; base += 64) {
                    bool ok = false;
                    if (base + lane < cnt) ok = fssr_accept(p, T.samples[first + base + lane]);
                    const unsigned long long mask = __ballot(ok);
                    const int c = __popcll(mask);
                    const int j = (lane - m) & 63;                /* accepted sample m + j belongs to this lane */
                    if (j < c) {
                        const FssrSample s = T.samples[first + base + fssr_nth_bit(mask, j)];
                        if (!(s.scale > max_scale)) fssr_term(p, pf, s, A);
                    }
                    m += c;
                }
            });
        }
    }

    /* the 64 partials in one fixed butterfly: every lane ends with the same totals */
    const double tv = fssr_wave_sum(A.tv), tw = fssr_wave_sum(A.tw), ts = fssr_wave_sum(A.ts), tcw = fssr_wave_sum(A.tcw);
    double tvd[3], twd[3], tc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { tvd[i] = fssr_wave_sum(A.tvd[i]); twd[i] = fssr_wave_sum(A.twd[i]); tc[i] = fssr_wave_sum(A.tc[i]); }

    if (lane != 0) return;
    if (out.n_influencing) out.n_influencing[v] = n;
    if (out.max_scale) out.max_scale[v] = max_scale;
    /* iso_octree.cc:162-169; a voxel without samples is VoxelData() (iso_octree.cc:101-102, voxel.h:98-105) */
    const bool empty = n == 0;
    if (out.value) out.value[v] = empty ? 0.0f : (float)(tv / tw);
    if (out.conf) out.conf[v] = empty ? 0.0f : (float)tw;
    if (out.scale) out.scale[v] = empty ? 0.0f : (float)(ts / tcw);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (out.deriv) out.deriv[3 * v + i] = empty ? 0.0f : (float)((tvd[i] * tw - twd[i] * tv) / (tw * tw));
        if (out.color) out.color[3 * v + i] = empty ? 0.0f : (float)(tc[i] / tcw);
    }
}

__global__ __launch_bounds__(256) void k_fssr_sample(FssrTree T, int cap, int gcap, uint2* glist, int n_voxels,
                                                    const double* __restrict__ positions, FssrOut out) {
    __shared__ int32_t s_idx[4][FSSR_LIST_MAX];
    __shared__ uint32_t s_key[4][FSSR_LIST_MAX];
    __shared__ FssrStack s_stack[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    /* list entries FSSR_LIST_MAX .. cap - 1 live in this wavefront's slice of global memory: (sample index, scale bits) */
    uint2* const g = glist + (size_t)(blockIdx.x * 4 + wv) * (size_t)gcap;
    /* a wavefront works through every (4 x gridDim.x)-th voxel; the wavefronts of a block never wait for each other */
    for (long long v = (long long)blockIdx.x * 4 + wv; v < n_voxels; v += (long long)gridDim.x * 4) {
        fssr_voxel(T, cap, s_idx[wv], s_key[wv], g, s_stack[wv], lane, v, positions, out);
        fssr_lds_fence();                             /* the next voxel reuses the list */
    }
}

int mi_fssr_resident_blocks(int device) {
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_fssr_sample, 256, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 1;
    return per_cu * cus;
}

void mi_fssr_launch(hipStream_t s, const FssrTree& tree, int32_t list_capacity, const FssrLists& lists, int32_t n_voxels,
                    const double* positions, const FssrOut& out) {
    if (n_voxels <= 0 || lists.max_blocks < 1) return;
    const int gcap = lists.entries && lists.per_wave > 0 ? lists.per_wave : 0;
    const int most = FSSR_LIST_MAX + gcap;
    const int cap = list_capacity < 1 ? 1 : (list_capacity > most ? most : list_capacity);
    const int blocks = (n_voxels + 3) / 4 < lists.max_blocks ? (n_voxels + 3) / 4 : lists.max_blocks;
    hipLaunchKernelGGL(k_fssr_sample, dim3((unsigned)blocks), dim3(256), 0, s, tree, cap, gcap, lists.entries, n_voxels, positions, out);
}
