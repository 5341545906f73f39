/* Internal: layouts + launcher of fssr_device.hip. */
#ifndef MI_FSSR_DEVICE_H
#define MI_FSSR_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FSSR_MAX_LEVELS 21        /* levels 0..20: fssr::Octree::max_level <= 20 (octree.h:201, voxel.h:31-35) */
#define FSSR_LIST_MAX   1024      /* entries of a wavefront's accepted-sample list in LDS ... */

struct FssrSample {               /* = fssr::Sample (sample.h:21-28) = mi_dmrecon_fssr_sample_t */
    float pos[3], normal[3], color[3], scale, confidence;
};

struct FssrNode {                 /* = mi_dmrecon_fssr_node */
    int32_t first_child, first_sample, n_samples, reserved;
};

struct FssrTree {
    const FssrSample* samples;
    const FssrNode* nodes;        /* n_nodes == 0: no tree, every sample is tested in index order */
    int32_t n_samples, n_nodes;
    double root_center[3], root_size;
};

struct FssrOut {                  /* device pointers, each may be NULL */
    float *value, *conf, *scale, *color, *deriv;
    int32_t* n_influencing;
    float* max_scale;
};

#define FSSR_GLIST_MAX  15360     /* ... and of its continuation in global memory */

struct FssrLists {                /* the global continuation of the lists: max_blocks x 4 slices of per_wave entries */
    uint2* entries;               /* (sample index, scale bits); may be NULL with per_wave == 0 */
    int32_t per_wave, max_blocks;
};

/* blocks of the kernel the device holds at a time (the grid never exceeds lists.max_blocks) */
int mi_fssr_resident_blocks(int device);

/* n_voxels positions (3 doubles each); list_capacity is clamped to 1..FSSR_LIST_MAX + lists.per_wave */
void mi_fssr_launch(hipStream_t s, const FssrTree& tree, int32_t list_capacity, const FssrLists& lists, int32_t n_voxels,
                    const double* positions, const FssrOut& out);
#endif
