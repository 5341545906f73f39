/*
 * mi_dmrecon_debug.h -- test and development hooks of libmi_dmrecon.so.
 *
 * NOT part of the drop-in boundary (include/mi_dmrecon.h is; nothing here replaces anything of the reference): these eleven
 * entry points exist for tests/ and tools/ -- fault injection, the host-only halves of the planning (so that they can be
 * checked against the oracle without a GPU), pool introspection, the probe buffer of -DMI_PROBE builds, the stored
 * bytes and the batching of the descriptor matching, and the stages and the list capacities of SIFT.  They are
 * declared here so that the library exports nothing that no header declares (the link uses a version script: only
 * mi_dmrecon_* symbols leave the library, tests/test_abi_and_host.py checks that every one of them is declared in one of
 * the two headers).  A production caller never needs them; they may change without notice.
 */
#ifndef MI_DMRECON_DEBUG_H
#define MI_DMRECON_DEBUG_H

#include "mi_dmrecon.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference view with this id gets a non-positive pixel footprint in the reconstruct calls that follow (-1: none): the
 * path of patch_sampler.cc:78-82 (std::out_of_range -> that view's MI_DMRECON_EFOOTPRINT), which no valid camera reaches. */
void mi_dmrecon_debug_inject_footprint(int view_id);

/* The block map of a front launch with teams for n_views views on a device of n_cus compute units (`want`: the largest
 * team allowed; empty: per view the pixels not filled at the hand-over, or NULL): map_out gets min(grid, cap) words
 * view | member << 16 | team size << 24 (0xFFFFFFFF: a block without work).  A pure function: needs no GPU. */
int mi_dmrecon_debug_front_teams(int32_t n_views, int32_t n_cus, int32_t want, const int64_t* empty, uint32_t* map_out, int32_t cap,
                                 int32_t* grid_out, int32_t* team_min_out, int32_t* team_max_out);

/* The HOST half of a reconstruct call's planning on cameras and features alone -- global view selection of reference view
 * `ref` (DMRecon::globalViewSelection, global_view_selection.cc:33-101; tables = 1: from the dense scene tables, 0: directly)
 * and, if n_seeds_out is given, the view's seeds (the host half of DMRecon::processFeatures, dmrecon.cc:243-296): exactly the
 * code a call runs, checked against the oracle without a GPU.  ms_out (optional): the time of `repeats` selections. */
int mi_dmrecon_debug_plan_views_host(int32_t n_views, const mi_dmrecon_camera* cams, const int32_t* widths, const int32_t* heights,
                                     int32_t n_feat, const float* pos, const int32_t* off, const int32_t* ids,
                                     const mi_dmrecon_settings* st, int32_t ref, int32_t tables, int32_t repeats,
                                     int32_t* ids_out, int32_t* n_out, double* ms_out,
                                     int32_t seed_cap, int32_t* seed_xy_out, float* seed_depth_out, int32_t* n_seeds_out);

/* The scratch sets of the context's scene that no call holds at the moment (return value) and the pixel capacity of the
 * largest of them. */
int mi_dmrecon_debug_scratch_sets(mi_dmrecon_ctx* ctx, long long* pixels_max);

/* Launches an empty one-lane kernel (`k_region_mark`) on the context's stream and waits for it: bench.py brackets every timed
 * region with one, so that a rocprofv3 kernel trace can be cut to the timed regions (tools/trace_regions.py). */
int mi_dmrecon_debug_region_mark(mi_dmrecon_ctx* ctx, int tag);

/* The debug buffer of -DMI_PROBE builds (tools/patch_probe.py): the first call allocates n 8-byte words on the device; later
 * calls copy up to n words out and clear the buffer. */
int mi_dmrecon_debug_buffer(unsigned long long* out, int n);

/* Set `set`'s list of `kind` as the device holds it: n x 128 / n x 64 packed bytes (SIFT biased by -128) to bytes_out and the n
 * `off` words (128 * the sum of a row's stored bytes + 2^20; 0 for SURF) to off_out; either may be NULL.  Returns n. */
int mi_dmrecon_debug_match_get(mi_dmrecon_match* m, int32_t set, int32_t kind, int8_t* bytes_out, int32_t* off_out);

/* Replaces the two limits of a batch of mi_dmrecon_match_pairs (rows + columns, workgroups) for the calls that follow, in the
 * whole process; 0 restores a default.  MI_DMRECON_EINVAL for more workgroups than a launch holds.  Not to be called while
 * mi_dmrecon_match_pairs runs. */
int mi_dmrecon_debug_match_limits(long long entries, long long blocks);

/* The batches mi_dmrecon_match_pairs makes of n_jobs jobs of n_a[j] x n_b[j] descriptors under the two limits (0: the one in
 * force): per job its batch (-1: an empty side, it runs nowhere), its first workgroup and its workgroups per strip of rows
 * in that batch's grid, and its first entry in that batch's buffers; each array may be NULL.  Returns the number of batches,
 * or MI_DMRECON_EINVAL for a job that needs more workgroups than the limit.  The function the call itself runs on; needs no GPU. */
int mi_dmrecon_debug_match_plan(int32_t n_jobs, const int32_t* n_a, const int32_t* n_b, long long entries, long long blocks,
                                int32_t* batch_out, int32_t* block0_out, int32_t* col_chunks_out, int64_t* entry0_out);

/* mi_dmrecon_sift_run's plan and image chain up to and including the octave in plan slot `slot` (0: the first octave, which is
 * octave min_octave), through the code that call runs, and what the device holds of that octave afterwards.  Every output
 * pointer may be NULL.  w_out, h_out: the octave's size; gray_out: the w x h gray image; src_out: the octave's source image,
 * the input of blur 0; img_out, dog_out: the S + 3 Gaussian and the S + 2 DoG images, one behind the other; ks_out, wsum_out
 * (S + 3 each) and taps_out ((S + 3) x 68, i = -ks ... ks first, zeros behind): the taps of each blur as the host made them
 * (ks = 0: a copy); n_cand_out: the octave's extrema, not capped; cand_out (x | y << 16 and the sample, two words per entry)
 * and loc_out (x, y, sample, kept per entry): the first min(*n_cand_out, the list's capacity, cand_room) entries.  raw_cand_out, raw_kp_out
 * (mi_dmrecon_sift_keypoint) and raw_xyso_out (four floats): the first raw_room entries of the three lists' memory as it
 * lies there, behind the capacities too (what a dropped write must have left alone); MI_DMRECON_EINVAL where the context
 * never allocated that many.  Runs the kernels once, whatever overflows.  Leaves the context without a result for
 * mi_dmrecon_sift_get. */
int mi_dmrecon_debug_sift_octave(mi_dmrecon_ctx* ctx, const mi_dmrecon_sift_options* opt, const void* pixels, int32_t is_float, int32_t w,
                                 int32_t h, int32_t channels, int32_t slot, int32_t* w_out, int32_t* h_out, float* gray_out, float* src_out,
                                 float* img_out, float* dog_out, int32_t* ks_out, float* wsum_out, float* taps_out, int32_t cand_room,
                                 int32_t* n_cand_out, int32_t* cand_out, float* loc_out, int32_t raw_room, int32_t* raw_cand_out,
                                 void* raw_kp_out, float* raw_xyso_out);

/* The capacities of the context's three SIFT lists (extrema of an octave, keypoints, descriptors) for the runs that follow: what
 * the next mi_dmrecon_sift_run starts with; a run that overflows one grows it and runs again, and the context keeps what it
 * grew.  0 restores a default; MI_DMRECON_EINVAL for a negative value.  Returns how often the context's last
 * mi_dmrecon_sift_run went through its kernels (1: no list overflowed; 0: there was no run). */
int mi_dmrecon_debug_sift_caps(mi_dmrecon_ctx* ctx, int32_t cand, int32_t kp, int32_t desc);

#ifdef __cplusplus
}
#endif
#endif
