/* Internal: layouts + launchers of surf_device.hip (sfm::Surf, libs/sfm/surf.cc, on the GPU). */
#ifndef MI_SURF_DEVICE_H
#define MI_SURF_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SURF_ROW_CHUNK 1024       /* k_surf_rows: a workgroup of 256 lanes scans a row in pieces of 1024 pixels, four per lane */
#define SURF_COL_TILE 64          /* k_surf_cols: tiles of 64 x 64 SAT values, transposed through LDS */
#define SURF_R0_TW 64             /* k_surf_response0: a workgroup makes 64 x 16 pixels of the four maps of octave 0 ... */
#define SURF_R0_TH 16
#define SURF_R0_LO 14             /* ... from a SAT tile with this halo to the left / above (fs = 9: fs + fs / 2 + 1) ... */
#define SURF_R0_HI 13             /* ... and this one to the right / below */
#define SURF_SAMPLES 109          /* the orientation samples: the grid points of -5 ... 5 with rx^2 + ry^2 < 36 */
#define SURF_MAX_WINDOWS 17       /* deg = -pi; deg < pi; deg += pi / 8 in double: 16 windows, 17 if the sum came out short */

struct SurfKeypoint { int32_t octave; float sample, x, y; };         /* = mi_dmrecon_surf_keypoint = sfm::Surf::Keypoint */

struct SurfCounts { int32_t n_kp, n_desc; };                           /* of a run, uncapped */

/* What the two per-keypoint kernels look up; made once on the host (surf_host.cpp) so that every value is the host's. */
struct SurfTables {
    float gaussian[SURF_SAMPLES];                 /* the weights of descriptor_orientation */
    int32_t rx[SURF_SAMPLES], ry[SURF_SAMPLES];   /* the sample offsets in the reference's order (ry outer, rx inner) */
    double win_start[SURF_MAX_WINDOWS], win_end[SURF_MAX_WINDOWS];
    int32_t n_win;
    float scale[4][4];                            /* Descriptor::scale of (octave, rounded sample) */
    float weight[201];                            /* descriptor_computation's exp(-(x^2 + y^2) / 6.6^2) by x^2 + y^2 */
};

struct SurfArgs {
    const unsigned char* pixels;  /* w x h x channels */
    int32_t channels, w, h;
    uint32_t* sat;                /* w x h: the inclusive summed-area table modulo 2^32 */
    float* maps;                  /* octave o: four maps of ow[o] x oh[o] one behind the other, from map_off[o] */
    int32_t ow[4], oh[4];
    long long map_off[4];
    int32_t word_off[4];          /* octave o's counts in `words`: (sample - 1, y, piece of 64 x) from here */
    int32_t n_words;
    int32_t* words;               /* survivors per row piece, then their offsets */
    float contrast_threshold;
    int32_t upright;
    SurfKeypoint* kp;             /* kp_cap */
    int32_t kp_cap;
    float* ori;                   /* kp_cap: the orientation */
    int32_t* stage;               /* kp_cap: 0 dropped, 1 has an orientation, 2 has a descriptor */
    int32_t* slot;                /* kp_cap: 1 for a descriptor, then its place in the output */
    float* tmp_desc;              /* kp_cap x 64, by keypoint */
    float* xyso;                  /* kp_cap x 4, compacted */
    float* desc;                  /* kp_cap x 64, compacted */
    const SurfTables* tab;
    SurfCounts* counts;
};

void mi_surf_sat(hipStream_t s, const SurfArgs& a);          /* grey + summed-area table */
void mi_surf_responses(hipStream_t s, const SurfArgs& a);    /* the 16 response maps */
void mi_surf_detect(hipStream_t s, const SurfArgs& a);       /* extrema, localisation, filtering -> kp, counts->n_kp */
void mi_surf_describe(hipStream_t s, const SurfArgs& a);     /* orientation, descriptor, compaction -> xyso, desc, counts->n_desc */
#endif
