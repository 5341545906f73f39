/* Host-callable launchers of the kernels in dmrecon_device.hip (internal). */
#ifndef MI_DMRECON_DEVICE_H
#define MI_DMRECON_DEVICE_H

#include <hip/hip_runtime.h>
#include "dmrecon_types.h"

/*
 * The kernels that depend on the filter width (mvs::Settings::filterWidth: 3, 5 or 7 -> 9 / 25 / 49 samples per
 * patch) are compiled once per width (dmrecon_device.hip with -DMI_FW=...); mi_device_api() returns the launchers
 * of a width, or null.  A launcher takes the stream, what every launch of a batch shares (MiLaunchBase) and a
 * descriptor of the launch: plain structs whose defaults mean "not used", so that a call names what it uses and
 * nothing else.  The launchers translate a descriptor into the kernel's own argument struct (OptArgs, ... in the .hip).
 *
 * optimize -- the caller NAMES the kernel (MiOptForm); the launcher picks the view slots (4 / 8 / 16) from st.K:
 *   MI_OPT_LOOP     k_optimize<L, false>: all the attempts an entry has left, in a row.  Continues follow.in if given.
 *   MI_OPT_FAST     k_optimize<L, true>: one attempt, no view selection (a patch that needs one goes on to the next list): the first
 *                   launch of a large round, follow-up launches if asked for.  Needs follow.out or .mask; no hyp; 4 / 8 slots.
 *   MI_OPT_SINGLE   k_optimize<L, false, true>: one attempt, general kernel.  Needs hyp (the parity hook), or follow.in and .out.
 *   MI_OPT_SEED     k_optimize<L, false, true, true>: the seeds, each re-optimised once from its own result.  Needs hyp.
 *   MI_OPT_LATENCY  k_optimize<Lay<16, 4>> / <Lay<8, 8>>: one patch per wavefront.  Four or eight slots only.
 *   A combination without a kernel launches nothing and returns non-zero.
 *   follow.out / follow.mask given: ONE attempt per entry; entries with further candidate hypotheses are appended to follow.out
 *   (or leave a mask per wavefront unit in follow.mask: mi_launch_follow_compact makes the list).  follow.in: continue the entries
 *   work[follow.in[..]].  A follow-up list is MI_FOLLOW_SEGS segments of follow.seg entries, one per XCD (workgroups b with
 *   equal b % 8), each with its own counter follow.*_n[segment] (OptArgs::follow_seg); follow.seg_in: the same of follow.in.
 * generate -- k_generate scans MI_GEN_TILE_W x MI_GEN_TILE_H pixel tiles; max_tiles = max over the jobs of their tile count.
 *   A view's entries go to `work` (count round_work[round]) while the view is in the throughput layout, to `work_lat`
 *   (round_work_lat[round]) once it has handed over: for good, from the round after the first one in which the VIEW's
 *   own list had fewer than `handover` entries -- decided on the device from view_count ([3][n_jobs], rotating per round;
 *   the caller presets slot 0 = what "the round before round 1" counts as, slot 1 = 0) and recorded in view_mode
 *   ([n_jobs], preset 0; the round of the hand-over).
 * tail -- one fused tail round: candidates from (prev_work, prev_results, round_work[round - 1]) -> this round's list,
 *   results and pixel-state writes (second state slot, see DevJob).  speculative: workgroups of four wavefronts, a
 *   pixel's candidate hypotheses tried at the same time; else one wavefront per pixel tries them in turn.
 * front -- the end of the tail, one persistent workgroup per reference view (k_front): the accepted entries of
 *   (list, list_results, *list_n) = round first_round - 1 are dealt out to per-view lists (view j's at job_off[j] of
 *   work[0] / results[0], its size in job_count[j], zeroed by the caller), then every view runs its own rounds
 *   first_round, first_round + 1, ... until its front is empty (lists alternate between the two buffer pairs).
 *   job_stats[4 j ..]: rounds run, attempts run, sum of list sizes, 100 MHz ticks (zeroed by the caller).
 *   Same maps as one `tail` launch per round.
 *   team.size > 1: that many workgroups per view (k_front<TEAM>): the attempts of a round are dealt out over them, every
 *   member runs the whole round otherwise (same numbering, same state writes) and fetches the others' results from the
 *   view's mailbox: mail = MI_FRONT_MAIL_WORDS 8-byte words per view, flags = MI_FRONT_FLAG_STRIDE words per view,
 *   zeroed by the caller; team_filled = one word per view, zeroed.  The members wait for each other at every pass, at
 *   most spin_ticks (100 MHz ticks): if one does not show up (all n_jobs * team workgroups must be resident at once; the
 *   caller keeps it <= the CUs, but cannot know what else holds them) the team GIVES UP -- error_flags bit 5 (32) is set
 *   and job_resume[j] (zeroed by the caller of a first launch) says from where view j goes on: round << 32 | entries << 1
 *   | list buffer, or >= MI_FRONT_DONE_HOST for a view that ran to its end.  A second launch with job_start = that array
 *   (no dealing out, the views start where it says) and no team finishes them; same maps either way.
 */
#define MI_FOLLOW_SEGS 8            /* segments of a follow-up list = XCDs (MI_XCDS of dmrecon_device.hip) */
#define MI_FRONT_DONE_HOST 0xFFFFFFFF00000000ull
#define MI_FRONT_TEAM_MAX 32
#define MI_FRONT_FLAG_STRIDE 40     /* team.flags words per view: MI_FRONT_TEAM_MAX pass flags, the XCC registration word, "several XCDs" */
#define MI_FRONT_MAIL_WORDS (2 * 1024 * 12)

/* what every launch of a batch shares (a round that needs other settings -- self_round, seed_reopt -- launches with a copy) */
struct MiLaunchBase { const DevJob* jobs = nullptr; const DevView* views = nullptr; const float* lut = nullptr; DevSettings st = {}; DevCounters* counters = nullptr; };
/* the list a launch works on: it only acts if min_work <= n < max_work, n = *n_work_ptr (if given) or n_work */
struct MiWorkList { const unsigned* n_work_ptr = nullptr; unsigned n_work = 0, min_work = 0, max_work = 0xFFFFFFFFu; int round = 0; };
enum MiOptForm { MI_OPT_LOOP, MI_OPT_FAST, MI_OPT_SINGLE, MI_OPT_SEED, MI_OPT_LATENCY };
struct MiFollow {                   /* the follow-up lists of an `optimize` launch; the defaults: none */
    const unsigned* in = nullptr; const unsigned* in_n = nullptr; unsigned* out = nullptr; unsigned* out_n = nullptr;
    unsigned seg = 0, seg_in = 0;   /* entries per segment of out / of in (0: one list with one counter) */
    unsigned long long* mask = nullptr;   /* first launch of a large round: a mask per wavefront unit instead of appending to out */
};
struct MiOptLaunch : MiWorkList {
    MiOptForm form = MI_OPT_LOOP; unsigned grid_blocks = 0;
    const DevEntry* work = nullptr; const DevHyp* hyp = nullptr; DevResult* results = nullptr;
    MiFollow follow;
};
/* optimize_spec / mi_launch_apply_spec -- a round of the throughput layout with every (entry, candidate rank) pair on a quad of
 * its own: `items` (entry << 2 | rank, *n_items of them: written by `generate` when given an item list) are the attempts, spec
 * holds one record per item; mi_launch_apply_spec applies the reference's sequential rule to the records and writes the pixels
 * back.  Same maps and counters as `optimize` + mi_launch_apply. */
struct MiSpecLaunch : MiWorkList {
    unsigned grid_blocks = 0; const DevEntry* work = nullptr; DevSpec* spec = nullptr; const unsigned* items = nullptr; const unsigned* n_items = nullptr;
};
struct MiGenLaunch {
    int n_jobs = 0, max_tiles = 0, round = 0; unsigned handover = 0;
    DevEntry* work = nullptr; DevEntry* work_lat = nullptr; unsigned* round_work = nullptr; unsigned* round_work_lat = nullptr;
    unsigned* view_count = nullptr; unsigned* view_mode = nullptr; unsigned* items = nullptr; unsigned* round_items = nullptr;
    int self_round = 0;             /* 1: the entries are the pixels written in round - 1 themselves (the seed re-optimisation
                                     * round, DevSettings::self_round), not their neighbours */
};
struct MiTailLaunch {
    unsigned grid_blocks = 0; int round = 0; bool speculative = false;
    const DevEntry* prev_work = nullptr; const DevResult* prev_results = nullptr; DevEntry* work = nullptr; DevResult* results = nullptr; unsigned* round_work = nullptr;
};
struct MiFrontTeam {                /* the teams of a first `front` launch; the defaults: one workgroup per view */
    int size = 1; unsigned grid_blocks = 0; unsigned long long* mail = nullptr; unsigned* flags = nullptr;
    const unsigned* block_map = nullptr;   /* per block of the grid job | member << 16 | team size << 24, 0xFFFFFFFF = none; the
                                            * blocks of a team share b % n_xcd */
};
struct MiFrontDebug {               /* test hooks (MI_DMRECON_DEBUG_FRONT_FAULT, MI_DMRECON_DEBUG_TEAM_WT) */
    int vanish_member = -1, vanish_round = 0;   /* that member of every team vanishes at that round of its view; -1: nobody */
    bool write_through = false;                  /* the teams write through their L2s as if found on several XCDs */
    bool exchange_through_memory = false;        /* ... and exchange through memory even within one XCD (A/B) */
};
struct MiFrontLaunch {
    int n_jobs = 0, first_round = 0, max_rounds = 0;
    const DevEntry* list = nullptr; const DevResult* list_results = nullptr; const unsigned* list_n = nullptr;
    DevEntry* work[2] = {nullptr, nullptr}; DevResult* results[2] = {nullptr, nullptr};
    const unsigned* job_off = nullptr; unsigned* job_count = nullptr; unsigned* job_stats = nullptr;
    const unsigned long long* job_start = nullptr; unsigned long long* job_resume = nullptr; unsigned* team_filled = nullptr; unsigned spin_ticks = 0;
    int n_xcd = 1;                  /* teams: XCDs of the device; a view's team is confined to the blocks of one (b % n_xcd) */
    unsigned* host_done = nullptr;  /* page-locked host memory, n_jobs zeroed words, or null: set to 1 per view that has run to its
                                     * end, after its state has been written back to memory */
    const unsigned* job_order = nullptr;   /* one workgroup per view: the view every block runs (a permutation of 0 .. n_jobs - 1: the
                                            * views the host expects to run longest first), or null: block b runs view b */
    MiFrontTeam team; MiFrontDebug debug;
};
struct MiEvalLaunch {               /* patch_eval: one patch of base.jobs[0] sampled at a given hypothesis (the parity hook) */
    int x = 0, y = 0; float depth = 0.f, dzI = 0.f, dzJ = 0.f;
    float* master = nullptr; float* ncc = nullptr; int32_t* ok = nullptr; float* col = nullptr; float* deriv = nullptr; int32_t* level = nullptr;
};
struct MiDeviceApi {
    int filter_width;
    int (*optimize)(hipStream_t s, const MiLaunchBase& b, const MiOptLaunch& l);      /* non-zero: the form has no such kernel */
    void (*patch_eval)(hipStream_t s, const MiLaunchBase& b, const MiEvalLaunch& l);
    void (*generate)(hipStream_t s, const MiLaunchBase& b, const MiGenLaunch& l);
    void (*tail)(hipStream_t s, const MiLaunchBase& b, const MiTailLaunch& l);
    void (*front)(hipStream_t s, const MiLaunchBase& b, const MiFrontLaunch& l);
    void (*optimize_spec)(hipStream_t s, const MiLaunchBase& b, const MiSpecLaunch& l);
};
const MiDeviceApi* mi_device_api(int filter_width);
extern unsigned long long* mi_debug_tbuf;

/* ---- kernels that do not depend on the filter width (defined once, in the width-5 object) ---- */
#define MI_GEN_TILE_W 64
#define MI_GEN_TILE_H 32
/* writes back the results of the `optimize` launches over l's list (its work, results, sizes and round; a grid of its own) */
void mi_launch_apply(hipStream_t s, const MiLaunchBase& b, const MiOptLaunch& l, unsigned grid_blocks);
void mi_launch_apply_spec(hipStream_t s, const MiLaunchBase& b, const MiSpecLaunch& l);
/* maps: [slot 0: depth | conf | dz x2 | normal x3][slot 1: same], imaps: [views | upd][views1 | upd1], per batch */
/* eight_views: imaps also holds [views_hi | views1_hi] behind them (nrReconNeighbors > 4) */
/* ... for the pixels [first, first + count) of the batch */
void mi_launch_flatten(hipStream_t s, float* maps, uint32_t* imaps, size_t total_px, bool eight_views, size_t first, size_t count);
/* the pixels [first, first + count) of the batch that were written from round r0 on, appended as records of `stride` words
 * ({view, pixel - first, depth, conf, dzI, dzJ [, nx, ny, nz]}) to `out` (page-locked host memory, `cap` records; *d_count counts
 * them all, also those that did not fit) */
struct MiEmitLaunch { int r0 = 0; unsigned view = 0, stride = 0; unsigned* d_count = nullptr; unsigned cap = 0; uint32_t* out = nullptr; };
void mi_launch_emit_changed(hipStream_t s, const float* maps, const uint32_t* imaps, size_t total_px, size_t first, size_t count,
                            const MiEmitLaunch& l);
/* seed_reopt: the records come from the re-optimising seed launch (DevSettings::seed_reopt: first confidence in `accepted`,
 * "propagates" in `tried`) -- the pixels are stamped round 1 / round 0 accordingly, and seed_count[job] (zeroed by the caller)
 * counts the pixels written: the propagation then starts with round 2 */
void mi_launch_apply_seeds(hipStream_t s, const MiLaunchBase& b, const MiOptLaunch& l, unsigned long long* seed_keys,
                           const unsigned* key_off, int seed_reopt = 0, unsigned* seed_count = nullptr);
/* one dispatch instead of four small copies: a[0..n_a) | b[0..n_b) -> out_rw, *counters -> *out_hc, per job (flags, n_filled,
 * view_count[job] or 0) -> out_dyn (12 bytes per job); the out pointers are page-locked host memory */
void mi_launch_round_report(hipStream_t s, const unsigned* a, int n_a, const unsigned* b, int n_b, const DevCounters* counters,
                            const DevJob* jobs, int n_jobs, unsigned* out_rw, DevCounters* out_hc, void* out_dyn, const unsigned* view_count);
/* the job records of a batch from their packed upload (words_per_job 32-bit words each: the part of DevJob in use, the
 * same for every job of the batch) to their places in jobs[] */
void mi_launch_unpack_jobs(hipStream_t s, const uint32_t* packed, unsigned words_per_job, DevJob* jobs, int n_jobs);
/* an empty one-lane kernel: where profiles are cut (mi_dmrecon_debug_region_mark) */
void mi_launch_region_mark(hipStream_t s, unsigned tag);
/* the first follow-up list of a round from the masks of its first launch, in list order (k_follow_count + k_follow_scatter);
 * blk_sum: 1024 words of scratch; acts like the launches of the round only if l.min_work <= *l.n_work_ptr < l.max_work */
void mi_launch_follow_compact(hipStream_t s, const MiWorkList& l, const unsigned long long* mask, unsigned ppw, unsigned lpp,
                              unsigned* blk_sum, unsigned* out, unsigned* out_n);
/* dst: w*h footprint elements of MI_QUAD_WORDS words (texels (x,y) (x,y+1), edge-clamped: DevView::quad) */
void mi_launch_quadify(hipStream_t s, const uint32_t* src, uint32_t* dst, int w, int h);
void mi_launch_pack_rgba(hipStream_t s, const uint8_t* src, uint32_t* dst, int n, int channels);
void mi_launch_unpack_rgb(hipStream_t s, const uint32_t* src, uint8_t* dst, int n);
void mi_launch_pyramid(hipStream_t s, const uint32_t* src, uint32_t* dst, int iw, int ih, int ow, int oh, const float w[3]);
#endif
