#!/usr/bin/env python
"""bench.py -- depth-maps/sec of the dmrecon hot path on MI355X (BASELINE.json metric).

A "step" = one pass of the hot path over one batch: DMRecon::start() for every reference view
of the 20-view 1920x1080 synthetic scene at scale 2 (BASELINE config 3), i.e. 20 depth maps of
480x270.  The scene (all pyramid levels of all views, RGBA8) is resident in HBM before the timed
region; the timed region contains everything DMRecon::start() does (host-side global view
selection and seed extraction, all kernels, and the copy of the maps back to host memory).

N > 1 (launched by torch.distributed.run, one rank per GPU): weak scaling -- every rank
reconstructs the 20 depth maps of its own scene replica per step; no data-path collective,
torch.distributed (RCCL) only provides the barrier and the max-over-ranks of the elapsed time.

A plain run (`--gpus 1 --steps K --warmup W`) sets the scene up, warms up, times ONE region of exactly K steps and prints the
JSON line (`value`, `ms_per_step`, the roofline of the timed region from its own device counts).  `--full` adds what takes runs
of its own: five timed regions with `value` their median, the all-seeds variant, `one_call`, the distinct-scenes variant, the
CPU baseline with `parity`, the strong-scaling mode at N > 1.  `--dump-outputs DIR` writes the maps of the last timed step.
"""
import argparse
import json
import os

# one hardware queue per host thread / HIP stream (the ROCm default of 4 makes streams share queues, and a tail
# launch then waits behind another stream's bulk kernel); must be set before the HIP runtime initialises
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from mve_amd import api  # noqa: E402
from mve_amd.dist import Collective, rank_views, rank_world, shard_views  # noqa: E402
from mve_amd.synth import CONFIGS, make_scene  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec (guide: 8.0 TB/s; 6.29 TB/s measured copy)
N_SIMDS = 256 * 4          # 256 CUs x 4 SIMDs
SHADER_CLOCK_HZ = 2.4e9    # guide: 2400 MHz
CYCLES_PER_VALU_INST = 4.0 # one f32 VALU wave-instruction occupies its SIMD's issue port for four cycles (measured:
                           # tools/ubench/valu_rate2.hip, profiles/r4_valu_rate.txt; SQ counters of the kernel itself: 4.1)
ALGORITHMIC_VALU_PER_SAMPLE = 57.0   # f32 operations per sample the reference's arithmetic needs (VERDICT r3 / DESIGN section 5)


def algorithmic_bytes(stats, n_maps, scene, cfg):
    """B_alg = 300 B * N_eval + 75 B * N_patch + 28 B * N_filled + B_compulsory,
    N_* counted on the device.  B_compulsory per depth map = reference level (3 B/texel) + for each
    of the <= 20 global neighbour views the two pyramid levels the sampler can select
    (scale-1 and scale), 3 B/texel as in the reference's RGB8 layout."""
    p, s = cfg["params"], cfg["scale"]
    def lvl(l):
        w, h = p.width, p.height
        for _ in range(l):
            w, h = (w + 1) // 2, (h + 1) // 2
        return w * h * 3
    n_glob = min(20, p.n_views - 1)
    comp = lvl(s) + n_glob * (lvl(max(s - 1, 0)) + lvl(s))
    return 300.0 * stats["n_eval"] + 75.0 * stats["n_patch"] + 28.0 * stats["n_filled"] + comp * n_maps


def plan_calls(steps, streams, steps_per_call=0):
    """How the K timed steps are issued: `spc` steps (spc x 20 reference views) per library call, the calls dealt
    over the host threads.  Larger batches amortise the ~600-round latency tail of a call (measured, 60 steps on 6
    threads: 852 depth-maps/s with 1 step per call, 948 with 5; 10 steps: 588 vs 827; 5 steps: 490 vs 612)."""
    steps = max(1, int(steps))
    if steps_per_call and steps_per_call > 0:
        spc = min(int(steps_per_call), steps)
        if steps % spc:
            raise SystemExit("--steps must be a multiple of --steps-per-call")
    else:
        spc = max(d for d in range(1, 6) if steps % d == 0)
    n_calls = steps // spc
    return spc, n_calls, max(1, min(int(streams), n_calls))


TRAFFIC_PROFILES = ("r6_traffic.json",)     # this round's PMC passes only: without them `traffic` is null (no silent fall-back to older trees)
# executed VALU wave-instructions per wavefront pass (16 patches x 4 views x 25 samples) of the bulk kernel: SQ_INSTS_VALU of a
# PMC pass / (device-counted passes / 64); a STORED profile value like `traffic` (profiles/r<N>_traffic.json:
# "valu_wave_insts_per_wave_pass"), r3's figure when the newest profile does not carry one
VALU_PER_WAVE_PASS_R3 = 3460.0


def stored_valu_per_wave_pass(lone=False):
    """(count, source) at the call plan closest to this run: a lone 20-view call runs all its rounds speculatively (more
    instructions executed per COUNTED pass: the attempts the reference's rule discards are executed too), the merged batches
    of the multi-threaded plans run the plain kernels."""
    for name in TRAFFIC_PROFILES:
        f = os.path.join(ROOT, "profiles", name)
        if os.path.exists(f):
            j = json.load(open(f))
            by = j.get("valu_wave_insts_per_wave_pass_by_plan", {})
            for plan, v in by.items():
                if plan.startswith("1 host thread") == bool(lone) and v:
                    return float(v), "profiles/%s (profiled plan: %s)" % (name, plan)
            v = j.get("valu_wave_insts_per_wave_pass")
            if v:
                return float(v), "profiles/" + name
    return None, None


def measured_traffic(n_streams, spc, config_is_c3=True):
    """HBM-side bytes per STEP of the optimise kernel families from the committed PMC passes
    (tools/collect_profiles.sh -> tools/summarize_profiles.py -> profiles/r<N>_traffic.json), at the call plan closest
    to this run: "1 host thread" profiles for a lone 20-view call, "default" (several host threads, five steps per
    call) otherwise; ({}, None) when no profile is present.  PMC counters cannot be read from inside the timed run: this
    is a STORED value of an earlier run of the same workload, labelled as such (`stored_profile`, `profiled_plan`);
    FETCH_SIZE is already corrected (x2, calibrated)."""
    for name in TRAFFIC_PROFILES:
        f = os.path.join(ROOT, "profiles", name)
        if not os.path.exists(f) or not config_is_c3:
            continue
        j = json.load(open(f))
        this = "%d host thread(s), %d step(s) per call" % (n_streams, spc)
        plans = j.get("plans", {})
        # the profile taken at exactly this run's plan, else the nearest kind (a lone call / a merged multi-thread batch)
        pick = this if this in plans else next((pl for pl in plans if pl.startswith("1 host thread") == (n_streams == 1 and spc == 1)), None)
        if pick is not None:
            return plans[pick], {"file": "profiles/" + name, "profiled_plan": pick, "stored_profile": True,
                                 "this_run_plan": this, "profiled_plan_is_this_runs": pick == this,
                                 "correction": j.get("correction", "")}
    return {}, None


def cpu_quota():
    """CPUs' worth of time the container may use (cgroup quota / period), or None: a box can show 256 cores to
    os.cpu_count() and give the process tree the time of 16 -- then 20 reference threads share 16 cores' worth."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]                      # cgroup v2
        return None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())                   # cgroup v1
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except (OSError, ValueError):
        return None


def cpu_baseline(scene, cfg, gpu_maps=None, gpu_maps_last=None, global_views=None):
    """The reference CPU path timed on this box's host cores on a bounded sample of the same workload.
    With gpu_maps (the HIP path's depth / conf maps of the same views) the reference's own output -- which this
    leg produces anyway -- is read back and diffed: the `parity` object of the JSON line."""
    cores = os.cpu_count() or 1
    ref_exe = os.path.join(ROOT, "oracle", "_ref", "dmrecon_ref_fast")
    p, s, k = cfg["params"], cfg["scale"], cfg["local_neighbors"]
    # (a scene of gigabytes -- C5: 100 x 36.6 MB -- is not written to disk as PNGs for the reference binary inside a
    # bench run: the restatement on one view stands in, `kind` says so)
    big = sum(im.nbytes for im in scene.images) >= (1 << 30)
    ref_failure = None
    if os.path.exists(ref_exe) and (not big or global_views is not None):
        from mve_amd.scene_io import SceneData, read_mvei, view_dir, write_scene
        work = tempfile.mkdtemp(prefix="bench_ref_")
        try:
            sdir = os.path.join(work, "scene")
            if not big:
                n_sample = max(1, min(cores, p.n_views))
                sample = list(range(n_sample))
                write_scene(sdir, scene)
                which = "views 0-%d" % (n_sample - 1)
            else:
                # a scene of gigabytes (C5: 100 x 36.6 MB): a bounded sample -- the first, the middle and the last reference
                # view -- and on disk only the images the reference will read for them: the sample's global view sets (the
                # library's selection, which is the reference's: tests; a view without its image is no candidate for the
                # reference, dmrecon.cc:62-79, and a greedy selection does not change when never-selected candidates are
                # missing), stored uncompressed (.mvei) so that neither side spends its time in a PNG codec
                sample = sorted(set([0, p.n_views // 2, p.n_views - 1]))
                need = set(sample)
                for v in sample:
                    need.update(int(g) for g in global_views(v))
                sub = SceneData(scene.cameras, [im if i in need else None for i, im in enumerate(scene.images)], scene.features)
                write_scene(sdir, sub, raw=True)
                n_sample = len(sample)
                which = "views %s (on disk: the %d images of their global view sets, uncompressed)" % (sample, len(need))
            env = dict(os.environ, OMP_NUM_THREADS=str(cores))
            cmd = [ref_exe, "-s%d" % s, "--local-neighbors=%d" % k, "--force", "--progress=silent", "--keep-conf",
                   "--list-view=%s" % ",".join(str(v) for v in sample), sdir]
            t0 = time.time()
            run = subprocess.run(cmd, check=True, env=env, capture_output=True, text=True)
            out = run.stdout
            wall = time.time() - t0
            # The reference ends a view that throws and goes on with the others (apps/dmrecon/dmrecon.cc:314-317): exit code 0 and
            # one view of the 20 without a depth map has been seen once on a GPU box (round 6; the cause is not established -- its
            # threads share mve::View objects without locks).  Such a view is run again by itself (the same maps as in the
            # all-views run, SURVEY App. B run 3; the time of the retry is added and the line says so); what is still missing
            # afterwards fails this leg, not the bench line.
            missing = [v for v in sample if not os.path.exists(os.path.join(view_dir(sdir, v), "depth-L%d.mvei" % s))]
            retried = list(missing)
            for v in missing:
                sys.stderr.write("cpu_baseline: the reference wrote no depth map for view %d (its messages: %s); running it again by itself\n"
                                 % (v, run.stderr.strip()[-300:]))
                t1 = time.time()
                subprocess.run(cmd[:-2] + ["--list-view=%d" % v, sdir], check=True, env=env, capture_output=True, text=True)
                wall += time.time() - t1
            missing = [v for v in sample if not os.path.exists(os.path.join(view_dir(sdir, v), "depth-L%d.mvei" % s))]
            if missing:
                raise RuntimeError("the reference binary wrote no depth map for views %s: %s" % (missing, run.stderr.strip()[-500:]))
            app_ms = None
            for ln in out.splitlines():
                if ln.startswith("Reconstruction took"):
                    app_ms = float(ln.split()[2].rstrip("ms.").rstrip("ms"))
            t = (app_ms / 1000.0) if (app_ms and not retried) else wall
            quota = cpu_quota()
            base = {"value": n_sample / t, "unit": "depth-maps/s", "cores": min(cores, n_sample), "kind": "reference",
                    "cpu_quota": quota,
                    "sample": "unmodified apps/dmrecon (oracle/_ref/dmrecon_ref_fast: -O3 -march=x86-64-v3 "
                              "-funsafe-math-optimizations, OpenMP over views) on %s of the same scene at scale %d; "
                              "time = the app's own 'Reconstruction took' (%.1f s, includes its image decode + pyramid); "
                              "%d host cores visible%s, one thread per view" % (
                                  which, s, t, cores,
                                  "" if quota is None else " (the container's CPU quota: the time of %.0f)" % quota)}
            if retried:
                base["views_run_again_alone"] = retried
            parity = None
            if gpu_maps is not None:
                ref_maps = [(read_mvei(os.path.join(view_dir(sdir, v), "depth-L%d.mvei" % s)),
                             read_mvei(os.path.join(view_dir(sdir, v), "conf-L%d.mvei" % s))) for v in sample]
                against = "the reference's own depth-L%d / conf-L%d of %s (the cpu_baseline run), this run" % (s, s, which.split(" (")[0])
                bounds = parity_bounds(cfg.get("name", ""))
                parity = map_parity_all([gpu_maps[v] for v in sample], ref_maps, against, bounds, sample)
                parity["which"] = "maps of the first timed call"
                if gpu_maps_last is not None:
                    pl = map_parity_all([gpu_maps_last[v] for v in sample], ref_maps, against, bounds, sample)
                    parity["last_timed_call"] = {k: pl[k] for k in ("min_fill_iou", "max_rel_depth_median", "max_rel_depth_p99", "max_conf_abs_p99", "within_bounds")}
                    parity["last_timed_call"]["bit_identical_to_first"] = bool(all(
                        np.array_equal(gpu_maps[v][0], gpu_maps_last[v][0]) and np.array_equal(gpu_maps[v][1], gpu_maps_last[v][1]) for v in sample))
                    parity["within_bounds"] = bool(parity["within_bounds"] and pl["within_bounds"])
            # The same scene directory once through the DROP-IN binary (MVE's unmodified apps/dmrecon linked against the shim,
            # build/dmrecon_mi; a cold process: HIP start-up, PNG decode, staging, one batch, image hand-back) -- the reference-compatible
            # entry point.  `value` above is measured through the C ABI WITHOUT a progress array (mve_amd/api.py): calls that meet are
            # merged and large batches send their maps back as snapshot + changed pixels; the shim passes progress arrays (it batches
            # its instances itself) and takes neither path.  Run after the reference's maps have been read (it overwrites them).
            app = os.path.join(ROOT, "build", "dmrecon_mi")
            if os.path.exists(app) and not big:
                try:
                    ra = subprocess.run([app] + cmd[1:-2] + [sdir], check=True, env=env, capture_output=True, text=True, timeout=300)
                    ms = [float(ln.split()[2].rstrip("ms.").rstrip("ms")) for ln in ra.stdout.splitlines() if ln.startswith("Reconstruction took")]
                    if ms:
                        base["drop_in_app_same_scene"] = {
                            "reconstruction_took_ms": ms[-1], "depth_maps_per_s": 1000.0 * n_sample / ms[-1],
                            "what": "build/dmrecon_mi (apps/dmrecon unmodified + the mvs::DMRecon shim) on the same scene directory, one cold "
                                    "process, its own 'Reconstruction took': HIP start-up, PNG decode, staging, the batch, image hand-back"}
                except (OSError, subprocess.SubprocessError, ValueError) as e:
                    base["drop_in_app_same_scene"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
            return base, parity
        except (OSError, RuntimeError, subprocess.SubprocessError, ValueError) as e:
            # (the restatement below stands in: a bench line with a "port" baseline instead of no line)
            ref_failure = "%s: %s" % (type(e).__name__, str(e)[:400])
            sys.stderr.write("cpu_baseline: the reference leg failed (%s); falling back to the restatement\n" % ref_failure)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    from oracle import oracle as orc
    S = orc.OracleScene(scene)
    # a bounded sample: the first, the middle and the last reference view (one view where there are only two)
    sample = sorted(set([0, p.n_views // 2, p.n_views - 1])) if p.n_views >= 8 else [0]
    t0 = time.time()
    outs = [S.reconstruct(orc.make_settings(ref_view=v, scale=s, local_neighbors=k)) for v in sample]
    t = time.time() - t0
    parity = None
    if gpu_maps is not None:
        against = "oracle restatement (bit-identical to the reference build on every fixture), views %s, this run" % sample
        ref_maps = [(o["depth"], o["conf"]) for o in outs]
        cb = parity_bounds(cfg.get("name", ""))
        parity = map_parity_all([gpu_maps[v] for v in sample], ref_maps, against, cb, sample)
        parity["which"] = "maps of the first timed call"
        if gpu_maps_last is not None:
            pl = map_parity_all([gpu_maps_last[v] for v in sample], ref_maps, against, cb, sample)
            parity["last_timed_call"] = {kk: pl[kk] for kk in ("min_fill_iou", "max_rel_depth_median", "max_rel_depth_p99", "max_conf_abs_p99", "within_bounds")}
            parity["last_timed_call"]["bit_identical_to_first"] = bool(all(
                np.array_equal(gpu_maps[v][0], gpu_maps_last[v][0]) and np.array_equal(gpu_maps[v][1], gpu_maps_last[v][1]) for v in sample))
            parity["within_bounds"] = bool(parity["within_bounds"] and pl["within_bounds"])
    base = {"value": len(sample) / t, "unit": "depth-maps/s", "cores": 1, "kind": "port",
            "sample": "oracle/dmrecon_oracle.cc restatement, views %s one after the other, single thread (%.1f s; "
                      "the reference binary needs the scene on disk as PNGs: not written for a scene of gigabytes)" % (sample, t)}
    if ref_failure:
        base["reference_leg_failed"] = ref_failure
    return base, parity


def parity_bounds(config_name):
    """The map-level bounds of a configuration and where each comes from.  Relative depth median <= 1e-3 / p99 <= 5e-3 and
    confidence p99 <= 5e-3 are the tolerances of tests/test_gpu_parity.py; fill IoU >= 0.98 is SURVEY 8c's.  Where the
    reference ALGORITHM does not reach such a figure against itself -- the restatement with its queue popped in another
    order: reversed, random, the reference's order with other tie-breaks -- the bound is that measured floor with a margin
    (tests/golden/order_floor_<config>.json, written by tools/order_floor.py from the CPU restatement; C5:
    profiles/r4_c5_order_floor.json): a parallel sweep is one more re-ordering of the same algorithm and cannot be asked to be
    closer to the reference than the reference's own orders are to each other."""
    b = {"fill_iou": 0.98, "rel_depth_median": 1e-3, "rel_depth_p99": 5e-3, "conf_abs_p99": 5e-3, "sources": {}}
    f = os.path.join(ROOT, "tests", "golden", "order_floor_%s.json" % config_name.lower())
    if os.path.exists(f):
        j = json.load(open(f))
        # per view: SURVEY's 0.98, or -- where the reference algorithm's own orders fall below it -- their minimum - 0.002
        per_view = {int(v): min(0.98, float(x) - 0.002) for v, x in j["worst"]["iou"].items()}
        b["fill_iou_per_view"] = per_view
        b["fill_iou"] = round(min(per_view.values()), 4)
        low = sorted(v for v, x in per_view.items() if x < 0.98)
        b["sources"]["fill_iou"] = ("per view min(0.98, floor - 0.002), floor = the reference algorithm (CPU restatement) against itself: the "
                                    "minimum over %d alternative queue orders (%s), tests/golden/%s; below 0.98 on views %s"
                                    % (len(j["orders"]), ", ".join(j["orders"]), os.path.basename(f), low))
        for key, src in (("conf_abs_p99", "max_conf_abs_p99"), ("rel_depth_p99", "max_rel_depth_p99")):
            if 1.5 * float(j[src]) > b[key]:
                b[key] = round(1.5 * float(j[src]), 5)
                b["sources"][key] = "1.5 x the reference algorithm's own order sensitivity (%.2e over those orders, worst view)" % float(j[src])
    elif config_name == "C5":
        # the restatement against itself with its queue reversed on views 0 / 50 of the C5 scene: confidence p99 7.8e-3 /
        # 6.0e-3 (tools/c5_order_floor.py -> profiles/r4_c5_order_floor.json)
        b["conf_abs_p99"] = 1e-2
        b["sources"]["conf_abs_p99"] = "the reference algorithm against itself in reversed queue order on this scene: conf p99 7.8e-3 (view 0), 6.0e-3 (view 50): profiles/r4_c5_order_floor.json"
    return b


def map_parity_all(gpu, ref, against, bounds, view_ids=None):
    """Worst case over the views of the map-level parity metrics against `bounds` (parity_bounds: every bound with its source;
    the fill mask per view where the bounds are per view)."""
    iou, med, p99, cp99, n = [], [], [], [], 0
    for (gd, gc), (rd, rc) in zip(gpu, ref):
        rd = np.asarray(rd, np.float32).reshape(gd.shape)
        rc = np.asarray(rc, np.float32).reshape(gc.shape)
        ma, mb = gd > 0, rd > 0
        both = ma & mb
        iou.append(float(both.sum()) / max(int((ma | mb).sum()), 1))
        rel = np.abs(gd[both] - rd[both]) / rd[both]
        med.append(float(np.median(rel))); p99.append(float(np.percentile(rel, 99)))
        cp99.append(float(np.percentile(np.abs(gc[both] - rc[both]), 99)))
        n += 1
    pv = bounds.get("fill_iou_per_view")
    ids = list(view_ids) if view_ids is not None else list(range(n))
    iou_ok = all(v >= (pv.get(i, bounds["fill_iou"]) if pv else bounds["fill_iou"]) for i, v in zip(ids, iou))
    ok = (iou_ok and max(med) <= bounds["rel_depth_median"] and max(p99) <= bounds["rel_depth_p99"]
          and max(cp99) <= bounds["conf_abs_p99"])
    return {"against": against, "views": n, "min_fill_iou": min(iou), "fill_iou_per_view": [round(v, 4) for v in iou],
            "max_rel_depth_median": max(med),
            "max_rel_depth_p99": max(p99), "max_conf_abs_p99": max(cp99),
            "bounds": {k: ([round(v[i], 4) for i in sorted(v)] if k == "fill_iou_per_view" else v) for k, v in bounds.items() if k != "sources"},
            "bound_sources": bounds.get("sources", {}),
            "within_bounds": bool(ok)}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, maps, view_ids):
    """--dump-outputs: the maps a caller of the timed path received for the LAST timed step (one dict of float32 arrays per
    reference view: depth, dz, conf) as DIR/<name>.npy, the views stacked along the first axis, and the reference view of
    every row as DIR/view_ids.npy (float64).  Where all views together exceed 64 MB (config C5) a fixed, seeded choice of
    the views is written: the same rows in every run of the same command."""
    names = [k for k in ("depth", "dz", "conf") if k in maps[0]]
    per_view = sum(maps[0][k].size * 4 for k in names) + 8
    keep = list(range(len(maps)))
    if per_view * len(maps) > DUMP_LIMIT_BYTES:
        keep = sorted(np.random.RandomState(0).permutation(len(maps))[:max(1, DUMP_LIMIT_BYTES // per_view)].tolist())
    os.makedirs(dirname, exist_ok=True)
    for k in names:
        np.save(os.path.join(dirname, k + ".npy"), np.stack([np.asarray(maps[i][k], np.float32) for i in keep]))
    np.save(os.path.join(dirname, "view_ids.npy"), np.asarray([view_ids[i] for i in keep], np.float64))


def timed_region(coll, ctxs, st, refs, n_calls, warmup, repeats=1, n_keep=None, keep_last_step=False, keep_first=True):
    """W untimed warm-up calls per host thread, then `repeats` timed regions of exactly n_calls library calls of `refs`
    each, dealt over the host threads (one forked context / HIP stream each), every region bracketed by barrier +
    synchronise on both sides (a library call returns with its maps on the host: the stream is idle when it does);
    returns (per-region max-over-ranks elapsed seconds, stats summed over all regions, the maps of the first and of the
    last timed call).  keep_first=False: the maps of the first timed call are not copied (the copy, a few milliseconds, lies
    inside the first region: a run with one region only would carry it in `value`); the last call's maps stand in for them.
    keep_last_step: after the regions, all maps of the last step of the last call are kept too (--dump-outputs).
    The host threads live across warm-up and timed regions, as the threads of a long-running process do: thread
    creation -- and with it the creation of each thread's OpenMP team inside the library (~10 ms) -- is not part of
    a step."""
    import threading
    n_streams = len(ctxs)
    # refs: the reference views of every call, or a function (host thread, call number of that thread) -> views (all calls
    # the same number of views of the same size: the distinct-scenes variant walks through its scenes)
    refs_of = refs if callable(refs) else (lambda i, k: refs)
    outs = [c.alloc_outputs(st, refs_of(i, 0), want_normal=False, pinned=True) for i, c in enumerate(ctxs)]   # reused, page-locked
    share = [n_calls // n_streams + (1 if i < n_calls % n_streams else 0) for i in range(n_streams)]
    acc, last, t_calls, done_at = {}, {}, [0.0] * n_streams, [0.0] * n_streams
    t_go = [0.0]
    lock = threading.Lock()
    warmed = threading.Barrier(n_streams + 1)
    go, fin = threading.Barrier(n_streams + 1), threading.Barrier(n_streams + 1)

    def worker(i, c, o, n):
        for w in range(max(warmup, 1)):
            tw = time.perf_counter()
            c.reconstruct(st, refs_of(i, w), want_normal=False, out=o)
            t_calls[i] = time.perf_counter() - tw
        warmed.wait()
        for rep in range(repeats):
            go.wait()
            # (no phase offsets: every host thread starts at once; calls that meet inside the library are merged)
            for k in range(n):
                r = c.reconstruct(st, refs_of(i, k), want_normal=False, out=o)   # synchronous: returns with the maps on the host
                with lock:
                    if keep_first and "res" not in last:
                        # (the first n_keep maps of the first timed call: a few milliseconds inside the FIRST region only)
                        last["res"] = [(m["depth"].copy(), m["conf"].copy()) for m in r[:n_keep]]
                        last["shape"] = r[0]["depth"].shape
                    done_at[i] = time.perf_counter()
                    for k, v in c.last_stats.items():
                        acc[k] = acc.get(k, 0) + v
                    if c.last_stats.get("clk_real_ticks", 0):
                        acc["_calls"] = acc.get("_calls", 0) + 1          # (calls that carry clk_real_mhz: a constant, averaged back)
                    # how the library batched the timed calls: (calls merged into the batch this call ran, its host clock)
                    if rep == 0:
                        acc.setdefault("_batches", []).append((int(c.last_stats.get("n_merged_calls", 0)), round(c.last_stats.get("ms_total", 0.0), 1),
                                                               round(1000.0 * (time.perf_counter() - t_go[0]), 1)))
                    # every region: the calls per library batch (the batch's leader reports them)
                    if int(c.last_stats.get("n_merged_calls", 0)) > 0:
                        acc.setdefault("_shape", {}).setdefault(rep, []).append(int(c.last_stats.get("n_merged_calls", 0)))
                        if os.environ.get("MI_BENCH_REGION_LOG"):
                            ls = c.last_stats
                            sys.stderr.write("region %d batch of %d calls: total %.1f ms = plan %.1f + %.1f, setup %.1f, rounds %.1f, front %.1f, download %.1f | kernels bulk %.1f front %.1f sweeps %.1f | returned at %.1f ms\n" % (
                                rep, ls["n_merged_calls"], ls["ms_total"], ls["ms_plan_gvs"], ls["ms_plan_seeds"], ls["ms_wall_setup"], ls["ms_wall_rounds"],
                                ls["ms_wall_front"], ls["ms_wall_download"], ls["ms_bulk_kernel"], ls["ms_front_kernel"],
                                ls["ms_sweep_kernels"], 1000.0 * (time.perf_counter() - t_go[0])))
            fin.wait()

    threads = [threading.Thread(target=worker, args=(i, c, o, n)) for i, (c, o, n) in enumerate(zip(ctxs, outs, share))]
    for t in threads:
        t.start()
    warmed.wait()
    elapsed = []
    for rep in range(repeats):
        # (a mark kernel on either side of the region, outside its clock: where a rocprofv3 kernel trace of this command is cut
        # to the timed regions -- tools/trace_regions.py; the warm-up calls and everything after the regions stay out)
        ctxs[0].debug_region_mark(2 * rep)
        coll.barrier()
        t0 = time.perf_counter()
        t_go[0] = t0
        go.wait()
        fin.wait()
        coll.barrier()
        elapsed.append(coll.max(time.perf_counter() - t0))
        ctxs[0].debug_region_mark(2 * rep + 1)
    for t in threads:
        t.join()
    # the maps of the LAST timed call: still in the output buffers of the host thread that finished last
    i_last = int(np.argmax(done_at))
    last["res_last"] = [(m["depth"].copy(), m["conf"].copy()) for m in outs[i_last][:n_keep]]
    if "res" not in last:
        # keep_first=False (a plain run): nothing is copied inside the region; the maps are the same in every call (the
        # `parity` object of a --full run: last_timed_call.bit_identical_to_first)
        last["res"], last["shape"] = last["res_last"], last["res_last"][0][0].shape
    if keep_last_step:
        # everything the caller received for the last step of that call (a call's views are its steps one after the other)
        last["last_step"] = [{k: m[k].copy() for k in ("depth", "dz", "conf")} for m in outs[i_last][-(n_keep or len(outs[i_last])):]]
    last["batch_shapes"] = [sorted(v) for _, v in sorted(acc.pop("_shape", {}).items())]
    batches = acc.pop("_batches", [])
    last["batches"] = sorted(b for b in batches if b[0] > 0)      # first region: (calls in the batch, ms of the batch, ms since the start when it returned)
    return elapsed, acc, last


def roofline(acc, n_maps, scene, cfg, n_streams, spc, elapsed):
    """The `roofline` object of a run from its summed call statistics: HBM bound, ALGORITHMIC bytes (SURVEY 8d:
    300 B per patch-view evaluation + 75 B per patch + 28 B per filled pixel + the compulsory image bytes, counted on
    the device) over the HIP-event durations of the optimise launches of the timed region."""
    p = cfg["params"]
    b_alg = algorithmic_bytes(acc, n_maps, scene, cfg)
    opt_s = acc["ms_opt_kernel"] / 1000.0
    n_launch = max(int(acc["n_launches"]), 1)
    achieved = b_alg / opt_s / 1e9 if opt_s > 0 else 0.0
    fams, traffic_src = measured_traffic(n_streams, spc, p.n_views == 20 and p.width == 1920)    # (the stored PMC passes are of C3)
    steps_rank = max(n_maps // p.n_views, 1)

    def fam_bytes(name):                                  # stored HBM-side bytes of a family, scaled to this run's steps
        v = fams.get(name)
        return None if v is None else (v["read_bytes_per_step"] + v["written_bytes_per_step"]) * steps_rank
    t_bulk = fam_bytes("k_optimize<1> (host-visible rounds)")
    t_tail = fam_bytes("k_tail + k_front (tail rounds)") or fam_bytes("k_tail (blind tail rounds)")
    traffic = None if t_bulk is None or t_tail is None else (t_bulk + t_tail) / n_launch
    # the kernels behind `achieved`, each with its own share of the algorithmic bytes
    bulk_stats = {"n_eval": acc.get("n_eval_bulk", 0), "n_patch": acc.get("n_patch_bulk", 0), "n_filled": acc.get("n_filled_bulk", 0)}
    b_bulk = algorithmic_bytes(bulk_stats, n_maps, scene, cfg)        # the compulsory bytes go with the bulk rounds
    b_tail = b_alg - b_bulk                                            # tail rounds: k_tail launches + the front kernel
    ms_bulk, ms_tail, ms_front = acc.get("ms_bulk_kernel", 0.0), acc.get("ms_tail_kernel", 0.0), acc.get("ms_front_kernel", 0.0)
    nb, nt = max(int(acc.get("n_bulk_launches", 0)), 1), max(int(acc.get("n_tail_launches", 0)), 1)
    n_pass = acc.get("n_pass", 0)
    # the same fraction on the sampling passes actually executed: one fused pass gathers a patch-view's 100 texels
    # once where the reference evaluates -- and n_eval counts -- it up to twice
    b_pass = b_alg - 300.0 * acc["n_eval"] + 300.0 * n_pass
    ms_tail_all = ms_tail + ms_front

    def fam(launches, ms, b, t):
        return {"launches": launches, "avg_launch_ms": ms / max(launches, 1), "algorithmic_bytes_per_launch": b / max(launches, 1),
                "traffic": None if t is None else t / max(launches, 1),
                "traffic_over_algorithmic": None if (t is None or b <= 0) else t / b,
                "achieved": (b / (ms / 1e3) / 1e9) if ms > 0 else None,
                "frac": (b / (ms / 1e3) / 1e9 / HBM_PEAK_GBS) if ms > 0 else None}
    per_kernel = {"k_optimize<1> (host-visible rounds)": fam(nb, ms_bulk, b_bulk, t_bulk),
                  "k_tail + k_front (tail rounds)": dict(
                      fam(nt + int(acc.get("n_front_launches", 0)), ms_tail_all, b_tail, t_tail),
                      k_tail_launches=nt, k_tail_ms=ms_tail, k_front_launches=int(acc.get("n_front_launches", 0)),
                      k_front_ms=ms_front, k_front_rounds_slowest_view=int(acc.get("n_front_rounds_max", 0)),
                      k_front_attempts=int(acc.get("n_front_attempts", 0)))}
    bulk_pass_frac = None
    if ms_bulk > 0 and acc["n_eval"] > 0:
        # the bulk kernel's share of the executed passes follows its share of the evaluations
        bulk_pass_frac = (b_bulk - 300.0 * bulk_stats["n_eval"] * (1.0 - n_pass / acc["n_eval"])) / (ms_bulk / 1e3) / 1e9 / HBM_PEAK_GBS
    # the same counts per kernel TEMPLATE (mi_dmrecon_stats::*_by_kernel), per step: what the per-kernel times of a rocprofv3
    # trace of this command are divided by (tools/roofline_check.py -> profiles/r6_roofline_check.md)
    from mve_amd.api import KERNEL_KINDS
    by_template = {}
    for kind in KERNEL_KINDS:
        ne, npass, npatch, nex = (acc.get("%s.%s" % (f, kind), 0) for f in ("n_eval_by_kernel", "n_pass_by_kernel", "n_patch_by_kernel", "n_pass_executed_by_kernel"))
        if ne or npass or npatch or nex:
            by_template[kind] = {"n_eval_per_step": ne / steps_rank, "n_pass_per_step": npass / steps_rank, "n_patch_per_step": npatch / steps_rank,
                                 "n_pass_executed_per_step": nex / steps_rank,
                                 "algorithmic_bytes_per_step": (300.0 * ne + 75.0 * npatch) / steps_rank}
    return {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "per_kernel_template": by_template,
            # the shader clock the k_optimize launches of this run ran at (mi_dmrecon_stats::clk_*: shader cycles over constant-rate
            # ticks of every 1024th wavefront's life, summed over the timed calls) -- the data sheet says 2400 MHz
            "shader_clock_mhz_measured": measured_shader_clock(acc),
            # host-visible rounds in the latency layout (views that have handed over while others of their batch have not): part of
            # the bulk kernels' time
            "latency_layout_rounds": {"ms_per_step": acc.get("ms_latency_rounds", 0.0) / steps_rank, "entries_per_step": acc.get("n_latency_entries", 0) / steps_rank,
                                      "share_of_bulk_kernel_time": (acc.get("ms_latency_rounds", 0.0) / ms_bulk) if ms_bulk > 0 else None},
            "frac_on_passes": (b_pass / opt_s / 1e9 / HBM_PEAK_GBS) if opt_s > 0 else None,
            "bulk_kernel_frac": per_kernel["k_optimize<1> (host-visible rounds)"]["frac"],
            "bulk_kernel_frac_on_passes": bulk_pass_frac,
            "traffic": traffic, "traffic_source": traffic_src,
            "kernel": "k_optimize<1> + k_tail + k_front (patch optimisation, both lane layouts)", "launches": n_launch,
            "avg_launch_ms": acc["ms_opt_kernel"] / n_launch,
            "algorithmic_bytes_per_launch": b_alg / n_launch,
            "traffic_over_algorithmic": None if traffic is None else traffic * n_launch / b_alg,
            "n_eval": int(acc["n_eval"]), "n_patch": int(acc["n_patch"]), "n_filled": int(acc["n_filled"]),
            "n_pass": int(n_pass),
            # bytes the sampling passes actually requested (RGBA8 footprints: 400 B per pass)
            "gathered_bytes_per_launch": 400.0 * n_pass / n_launch,
            "per_kernel": per_kernel,
            # the secondary roofs SURVEY 8d names (the real limiters are on-chip):
            # fp32 VALU with SURVEY's algorithmic flop counts (3.6 kflop per derivative evaluation, 1.6 kflop
            # per colour evaluation, mix 19.9 : 11.9), and the L2 with the bytes the passes request from it
            "secondary_roofs": {
                "valu_issue": valu_issue_roof(acc, bulk_stats, n_pass, ms_bulk, steps_rank, lone=(n_streams == 1 and spc == 1)),
                "l1_gather": l1_gather_roof(acc, bulk_stats, n_pass, ms_bulk, steps_rank, lone=(n_streams == 1 and spc == 1)),
                "valu_fp32": {"algorithmic_flop": 2.85e3 * acc["n_eval"], "achieved": 2.85e3 * acc["n_eval"] / opt_s / 1e12 if opt_s > 0 else None,
                              "peak": 157.3, "unit": "TFLOP/s", "frac": 2.85e3 * acc["n_eval"] / opt_s / 1e12 / 157.3 if opt_s > 0 else None},
                "l2": {"requested_bytes": 400.0 * n_pass, "achieved": 400.0 * n_pass / opt_s / 1e9 if opt_s > 0 else None,
                       "peak": 34500.0, "unit": "GB/s", "frac": 400.0 * n_pass / opt_s / 1e9 / 34500.0 if opt_s > 0 else None}},
            "kernel_time_share": opt_s / elapsed if elapsed > 0 else None,
            # the launches of the host threads' streams overlap on the GPU, so each launch's own duration
            # (above, as the contract asks) stretches; the same bytes over the wall time of the region:
            "aggregate_achieved": b_alg / elapsed / 1e9 if elapsed > 0 else None,
            "aggregate_frac": b_alg / elapsed / 1e9 / HBM_PEAK_GBS if elapsed > 0 else None}


def predicted_strong_scaling(n_views):
    """BASELINE config 4 on 1 / 2 / 4 / 8 GPUs as the measurements of ONE GPU predict it -- no 8-GPU node has run it (the
    driver's SCALE record would be the measurement): a rank that has its GPU to itself reconstructs its share of the
    scene's reference views per step, one library call; lone calls of exactly those sizes were timed on one MI355X
    (tools/lone_calls.py -> profiles/r<N>_lone_calls.json, a STORED profile).  The floor: one view's dependent propagation
    rounds do not shrink with the share."""
    for tag in ("r6",):                                  # this round's collection only (no silent fall-back to older trees)
        f = os.path.join(ROOT, "profiles", "%s_lone_calls.json" % tag)
        if not os.path.exists(f):
            continue
        j = json.load(open(f))
        sizes = {int(k): v for k, v in j.get("sizes", {}).items()}
        curve = {}
        for world in (1, 2, 4, 8):
            share = (n_views + world - 1) // world              # the slowest rank's share (round-robin: ranks differ by <= 1 view)
            if share in sizes:
                ms = sizes[share]["ms_median"]
                curve[str(world)] = {"views_on_slowest_rank": share, "ms_per_step": ms, "depth_maps_per_s": 1000.0 * n_views / ms}
        if curve:
            one = sizes.get(1, {}).get("ms_median")
            return {"predicted": True, "measured_on": "one MI355X: lone calls of a rank's share (%s)" % ("profiles/%s_lone_calls.json" % tag),
                    "stored_profile": True, "gpus": curve,
                    "floor_ms_per_step": one, "floor_note": "a single reference view: its ~580 dependent propagation rounds",
                    "speedup_8_over_1": (curve["8"]["depth_maps_per_s"] / curve["1"]["depth_maps_per_s"]) if ("8" in curve and "1" in curve) else None}
    return None


def measured_shader_clock(acc):
    """MHz, or None: the summed shader cycles over the summed constant-rate ticks x the rate of the constant clock (a per-call
    constant that the sums carry once per call that sampled it: _calls)."""
    if not acc.get("clk_real_ticks"):
        return None
    return acc["clk_shader_cycles"] / acc["clk_real_ticks"] * (acc.get("clk_real_mhz", 0.0) / max(acc.get("_calls", 1), 1))


# what a compute unit's vector L1 serves of the bulk kernels' access pattern -- 64-lane 16-byte gathers from 8-byte aligned
# addresses, five in flight per wavefront, 12 wavefronts per CU -- while the L1 / L2 hold the lines: measured by
# tools/ubench/gather_rate.hip on the MI355X (profiles/r6_gather_rate.txt: 37.1 gathers per microsecond and CU = 62 shader
# cycles per gather = 1.03 lane accesses per cycle), a STORED figure like the PMC ones
L1_LANE_ACCESSES_PER_US_PER_CU = 37.1 * 64.0
N_CUS = 256


def stored_l1_per_wave_pass(lone=False):
    for name in TRAFFIC_PROFILES:
        f = os.path.join(ROOT, "profiles", name)
        if os.path.exists(f):
            by = json.load(open(f)).get("l1_accesses_per_wave_pass_by_plan", {})
            for plan, v in by.items():
                if plan.startswith("1 host thread") == bool(lone) and v:
                    return float(v), "profiles/%s (profiled plan: %s)" % (name, plan)
    return None, None


def l1_gather_roof(acc, bulk_stats, n_pass, ms_bulk, steps, lone=False):
    """The vector L1's rate on the bulk kernels' gathers as a third ceiling: the L1 accesses the kernels make (one per lane of a
    gather; a stored TCP_TOTAL_CACHE_ACCESSES figure per wavefront pass x the passes this run counted) over what the L1s of
    all CUs serve of this access pattern by the micro-benchmark's measure.  `frac` well below 1 says the kernels are not
    bound by the L1's rate either (no single ceiling is saturated; the time follows the lines touched)."""
    if not acc.get("n_eval") or ms_bulk <= 0:
        return None
    per_wave_pass, src = stored_l1_per_wave_pass(lone)
    if per_wave_pass is None:
        return None
    passes_bulk = n_pass * (bulk_stats["n_eval"] / acc["n_eval"])
    accesses = per_wave_pass * passes_bulk / 64.0
    peak = L1_LANE_ACCESSES_PER_US_PER_CU * N_CUS * 1e6                     # lane accesses per second, whole chip
    floor_ms = 1000.0 * accesses / peak
    return {"bound": "l1_gather", "kernel": "k_optimize<1> (host-visible rounds)", "l1_accesses_per_step": accesses / max(steps, 1),
            "l1_accesses_per_wave_pass": per_wave_pass, "l1_accesses_per_sample_and_lane": per_wave_pass / 25.0 / 64.0,
            "source": {"file": src, "stored_profile": True, "peak_from": "profiles/r6_gather_rate.txt (tools/ubench/gather_rate.hip)"},
            "peak": peak / 1e9, "unit": "G lane accesses/s", "achieved": accesses / (ms_bulk / 1e3) / 1e9,
            "floor_ms_per_step": floor_ms / max(steps, 1), "measured_ms_per_step": ms_bulk / max(steps, 1), "frac": floor_ms / ms_bulk}


def valu_issue_roof(acc, bulk_stats, n_pass, ms_bulk, steps, lone=False):
    """A second ceiling next to the HBM one (round 5 took it for the binding one; round 6's experiments say it is not: DESIGN.md
    section 5): how fast the SIMDs could issue the VALU wave-instructions the bulk kernel EXECUTES -- a stored SQ_INSTS_VALU
    figure per wavefront pass x the passes this run counted on the device -- over the chip's issue rate, SIMDs x shader
    clock / 4 cycles per instruction.  `frac` = that floor / the kernel's measured time: 1.0 = every SIMD issues a VALU
    instruction whenever it can.  `executed_per_algorithmic`: the instructions executed per f32 operation the reference's
    arithmetic needs (57 per sample): what the formulation adds on top (addressing, table look-ups, control)."""
    if not acc.get("n_eval") or ms_bulk <= 0:
        return None
    per_wave_pass, src = stored_valu_per_wave_pass(lone)
    if per_wave_pass is None:
        return None
    passes_bulk = n_pass * (bulk_stats["n_eval"] / acc["n_eval"])           # the bulk kernel's share of the executed passes
    insts = per_wave_pass * passes_bulk / 64.0                              # a wavefront pass = 64 patch-view passes
    rate = N_SIMDS * SHADER_CLOCK_HZ / CYCLES_PER_VALU_INST                 # wave-instructions per second, whole chip
    floor_ms = 1000.0 * insts / rate
    alg = ALGORITHMIC_VALU_PER_SAMPLE * 25.0 * passes_bulk / 64.0
    # the shader clock the kernels actually ran at (mi_dmrecon_stats::clk_*: shader cycles over constant-rate ticks, sampled
    # inside the k_optimize launches of THIS run): the roof above is priced at the data sheet's 2.4 GHz
    clk = measured_shader_clock(acc)
    measured = None
    if clk:
        rate_m = N_SIMDS * clk * 1e6 / CYCLES_PER_VALU_INST
        measured = {"shader_clock_mhz": clk, "peak": rate_m / 1e9, "floor_ms_per_step": 1000.0 * insts / rate_m / max(steps, 1),
                    "frac": 1000.0 * insts / rate_m / ms_bulk,
                    "what": "the same roof priced at the shader clock sampled inside this run's k_optimize launches "
                            "(shader cycles / constant-rate ticks of every 1024th wavefront)"}
    return {"bound": "valu_issue", "kernel": "k_optimize<1> (host-visible rounds)", "at_measured_clock": measured,
            "executed_valu_wave_insts_per_step": insts / max(steps, 1), "valu_wave_insts_per_wave_pass": per_wave_pass,
            "source": {"file": src, "stored_profile": True},
            "peak": rate / 1e9, "unit": "G wave-instructions/s", "cycles_per_valu_wave_inst": CYCLES_PER_VALU_INST,
            "achieved": insts / (ms_bulk / 1e3) / 1e9,
            "floor_ms_per_step": floor_ms / max(steps, 1), "measured_ms_per_step": ms_bulk / max(steps, 1),
            "frac": floor_ms / ms_bulk,
            "executed_per_algorithmic": insts / alg if alg > 0 else None,
            "valu_insts_per_sample": per_wave_pass / 25.0}


def run_one_call(ctx, st, views, scene, cfg, n_timed=50):
    """What a user of apps/dmrecon gets: ONE library call for the scene's reference views (20 on C3) on one host
    thread, nothing else on the GPU.  Measured after the timed region, same resident scene: 2 warm-up calls, then
    n_timed calls; ms per call (median / mean), depth-maps/s, where the time goes, and the roofline of that call."""
    out = ctx.alloc_outputs(st, views, want_normal=False, pinned=True)
    for _ in range(2):
        ctx.reconstruct(st, views, want_normal=False, out=out)
    ts, acc = [], {}
    for _ in range(n_timed):
        t0 = time.perf_counter()
        ctx.reconstruct(st, views, want_normal=False, out=out)
        ts.append(time.perf_counter() - t0)
        for k, v in ctx.last_stats.items():
            acc[k] = acc.get(k, 0) + v
        if ctx.last_stats.get("clk_real_ticks", 0):
            acc["_calls"] = acc.get("_calls", 0) + 1
    med = float(np.median(ts))
    roof = roofline(acc, len(views) * n_timed, scene, cfg, 1, 1, float(np.sum(ts)))
    pk = roof["per_kernel"]
    return {"what": "one library call = the %d reference views of the scene once, 1 host thread, GPU otherwise idle; "
                    "median of %d calls after the timed region" % (len(views), n_timed),
            "ms_per_call": 1000.0 * med, "ms_per_call_mean": 1000.0 * float(np.mean(ts)),
            "ms_per_call_min_max": [1000.0 * float(np.min(ts)), 1000.0 * float(np.max(ts))],
            "ms_front_view_max": acc.get("ms_front_view_max", 0.0) / n_timed, "front_fallbacks": int(acc.get("front_fallbacks", 0)),
            "valu_issue_frac": (roof["secondary_roofs"]["valu_issue"] or {}).get("frac"),
            "depth_maps_per_s": len(views) / med,
            "ms_host_planning": (acc.get("ms_plan_gvs", 0.0) + acc.get("ms_plan_seeds", 0.0)) / n_timed,
            "ms_bulk_kernel": acc.get("ms_bulk_kernel", 0.0) / n_timed,
            "ms_tail_kernel": acc.get("ms_tail_kernel", 0.0) / n_timed,
            "ms_front_kernel": acc.get("ms_front_kernel", 0.0) / n_timed,
            "rounds": int(acc.get("n_rounds", 0) / n_timed), "front_first_round": int(acc.get("front_first_round", 0) / n_timed),
            "bulk_launches": int(acc.get("n_bulk_launches", 0) / n_timed),
            "bulk_kernel_avg_launch_ms": pk["k_optimize<1> (host-visible rounds)"]["avg_launch_ms"],
            "bulk_kernel_frac": roof["bulk_kernel_frac"], "bulk_kernel_frac_on_passes": roof["bulk_kernel_frac_on_passes"],
            "tail_frac": pk["k_tail + k_front (tail rounds)"]["frac"],
            "frac": roof["frac"], "frac_on_passes": roof["frac_on_passes"]}


def run_distinct_scenes(coll, device, cfg, st, n_scenes, spc, n_calls, n_streams, warmup, repeats):
    """The headline's plan on DISTINCT data: the timed steps walk through `n_scenes` differently seeded scenes (cameras,
    texture and features of their own, same size and settings), all resident in one context -- a region of 20 steps = 400
    depth maps of 20 scenes, where the headline reconstructs the same 20 views twenty times (its images: a 200 MB hot set
    that every one of the 400 concurrent jobs shares).  Step s of a region is scene s mod n_scenes.  The scenes are rendered
    on the GPU (mve_amd/csrc/synth_render_gpu.hip: harness code) -- 20 scenes on the box's CPU quota would take 100 s."""
    import dataclasses
    from mve_amd.synth import merge_scenes
    p = cfg["params"]
    t0 = time.perf_counter()
    scenes = [make_scene(dataclasses.replace(p, texture_seed=p.texture_seed + 31 * k, camera_seed=p.camera_seed + 17 * k,
                                             feature_seed=p.feature_seed + 13 * k), gpu=True) for k in range(n_scenes)]
    big = merge_scenes(scenes)
    t_render = time.perf_counter() - t0
    ctx = api.Context(device)
    t0 = time.perf_counter()
    ctx.load_scene(big, pinned_staging=True)
    t_stage = time.perf_counter() - t0
    ctxs = [ctx] + [ctx.fork() for _ in range(n_streams - 1)]
    share = [n_calls // n_streams + (1 if i < n_calls % n_streams else 0) for i in range(n_streams)]
    first = [sum(share[:i]) for i in range(n_streams)]            # the region's steps in thread order: thread i holds calls first[i] ...

    def refs_of(i, k):
        out = []
        for s_ in range(spc):
            sc = ((first[i] + k) * spc + s_) % n_scenes
            out += list(range(sc * p.n_views, (sc + 1) * p.n_views))
        return out
    el, acc, last = timed_region(coll, ctxs, st, refs_of, n_calls, warmup, repeats=repeats, n_keep=p.n_views)
    n_maps = p.n_views * spc * n_calls
    fill = float(np.mean([(c > 0).mean() for _, c in last["res"]]))
    ms_bulk = acc.get("ms_bulk_kernel", 0.0)
    bulk_stats = {"n_eval": acc.get("n_eval_bulk", 0), "n_patch": acc.get("n_patch_bulk", 0), "n_filled": acc.get("n_filled_bulk", 0)}
    b_bulk = algorithmic_bytes(bulk_stats, n_maps * len(el), big, cfg)
    for c in ctxs[1:]:
        c.close()
    ctx.close()
    return {"scenes": n_scenes, "value": n_maps / float(np.median(el)), "unit": "depth-maps/s", "repeats": [n_maps / e for e in el],
            "what": "the same call plan, every step a different one of %d differently seeded scenes (step s = scene s mod %d), "
                    "all %d views resident in one context" % (n_scenes, n_scenes, big.n_views),
            "resident_host_image_GB": sum(im.nbytes for im in big.images) / 1e9,
            "render_seconds_gpu": t_render, "staging_seconds": t_stage, "mean_fill_first_call": round(fill, 4),
            "bulk_kernel_frac": (b_bulk / (ms_bulk / 1e3) / 1e9 / HBM_PEAK_GBS) if ms_bulk > 0 else None,
            "ms_bulk_kernel_per_step": ms_bulk / max(1, n_maps * len(el) // p.n_views),
            "ms_front_kernel_per_step": acc.get("ms_front_kernel", 0.0) / max(1, n_maps * len(el) // p.n_views),
            "calls_per_library_batch_by_region": last.get("batch_shapes", [])}


def self_launch(n_ranks):
    """Re-executes this command line under torch.distributed.run with n_ranks processes on this node (MASTER_ADDR 127.0.0.1, a
    port nobody holds) and returns its exit code."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # (RCCL across processes: the host driver supports dmabuf IPC only)
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=240,
                    help="timed steps (one step = all reference views of the scene once); the default keeps the GPU busy "
                         "for several seconds so that an outside utilisation sampler sees the run")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="C3", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=None,
                    help="the timed region (exactly --steps steps, barrier + synchronise on both sides) is run this many "
                         "times in the same process; `value` is the median region, `repeats` lists them all.  Default: 1 "
                         "(--steps is the number of timed steps of the run), 5 with --full")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure, each a run of its own after the timed region: five timed regions "
                         "instead of one, the all-seeds variant, the `one_call` object, the distinct-scenes variant, the CPU baseline "
                         "with the `parity` object, and at N > 1 the strong-scaling mode next to the weak line.  Without it the "
                         "run sets up, warms up, times --steps steps and prints the line; the --no-* switches and "
                         "--distinct-scenes / --one-call-n select among the parts of a --full run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the maps the timed path returned for its last step (depth, dz, conf of "
                         "every reference view of the step, float32) to DIR/<name>.npy; the scene is the same in every run "
                         "of the same command, so two builds can be compared map for map")
    ap.add_argument("--one-call-n", type=int, default=50, help="library calls behind the `one_call` object")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--distinct-scenes", type=int, default=-1,
                    help="after the timed regions, the same plan once more on this many differently seeded scenes "
                         "(config.distinct_scenes_variant); -1 = 20 for config C3 on one GPU, else none; 0 = none")
    ap.add_argument("--no-seed-variant", action="store_true", help="skip the two extra regions with MI_DMRECON_SEED_REOPT=0 (config.all_seeds_propagate_variant)")
    ap.add_argument("--no-one-call", action="store_true",
                    help="skip the `one_call` object (one 20-view library call on one host thread, measured after the timed region)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="N > 1 only.  weak (default): every rank reconstructs all views of its own scene replica per "
                         "step.  strong (BASELINE config 4): ONE scene, its reference views dealt round-robin over the "
                         "ranks (mve_amd.dist.shard_views), value = views x steps / slowest rank.  The weak line also "
                         "carries the strong-mode figure of the same run as `strong_scaling`.")
    ap.add_argument("--streams", type=int, default=6,
                    help="host threads per GPU, each driving its own forked context / HIP stream; steps are "
                         "dealt round-robin (the reference runs its views under an OpenMP loop the same way).  Calls "
                         "that meet inside the library are merged into one batch (config.views_per_library_batch)")
    ap.add_argument("--steps-per-call", type=int, default=0,
                    help="steps (passes over the rank's reference views) handed to ONE mi_dmrecon_reconstruct batch. "
                         "0 = the largest divisor of --steps that is <= 5")
    args = ap.parse_args()
    full = args.full
    n_regions = max(1, args.repeats if args.repeats is not None else (5 if full else 1))
    rank, world, local_rank = rank_world()
    if world == 1 and args.gpus > 1:
        # `python bench.py --gpus N` by itself: start the N ranks (one process per GPU, rank r on device r) the way the driver's
        # N > 1 command does -- torch.distributed.run on this node, rendezvous on 127.0.0.1 at a free port -- and hand its exit
        # code on; the ranks find WORLD_SIZE = N and take the branch below.  rank 0 prints the JSON line.
        raise SystemExit(self_launch(args.gpus))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d was started with WORLD_SIZE=%d: launch it as `python bench.py --gpus N` or as "
                         "`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`" % (args.gpus, world))
    cfg = dict(CONFIGS[args.config], name=args.config)
    p = cfg["params"]
    # MI_BENCH_SHARE_GPU=1 (development only, never the driver's command): all ranks of an N > 1 launch use GPU 0 and
    # the gloo backend -- the strong-scaling plumbing and the per-rank time of a 1/N share of the scene on a one-GPU box
    # (profiles/r3_strong_2ranks_one_gpu.json); the line is labelled with it
    share_gpu = world > 1 and os.environ.get("MI_BENCH_SHARE_GPU") == "1"
    if share_gpu:
        local_rank = 0
        # (default environment: one call per GPU runs front teams at a time -- the library's team token --, a team that is not
        # given its compute units in time gives up and the views finish with one workgroup each)
    coll = Collective("gloo" if share_gpu else "nccl", local_rank)

    t0 = time.perf_counter()
    # synthetic, deterministic, identical on every rank; the large configuration (C5: 100 x 12 MP) is rendered on the GPU
    # (harness code, mve_amd/csrc/synth_render_gpu.hip: 87 s on the box's CPU quota otherwise)
    scene = make_scene(p, gpu=(p.n_views * p.width * p.height > 400e6))
    t_render = time.perf_counter() - t0
    ctx = api.Context(local_rank)
    # upload + device pyramid: inputs resident in HBM before any timed region starts.  Timed by itself (`staging`): images
    # over PCIe from page-locked staging buffers, asynchronously (mi_dmrecon_set_view_async), RGBA pack + pyramid +
    # footprint records on the device -- the PCIe-inclusive rate of a scene that is reconstructed once
    t0 = time.perf_counter()
    ctx.load_scene(scene, pinned_staging=True)
    t_stage = time.perf_counter() - t0
    host_bytes = int(sum(im.nbytes for im in scene.images))
    st = api.Settings(scale=cfg["scale"], nrReconNeighbors=cfg["local_neighbors"])
    all_views = list(range(p.n_views))

    # one forked context (own HIP stream + scratch, shared resident scene) per host thread; the
    # latency-bound tail of one call's propagation overlaps the throughput-bound start of another's
    spc, n_calls, n_streams = plan_calls(args.steps, args.streams, args.steps_per_call)
    ctxs = [ctx] + [ctx.fork() for _ in range(n_streams - 1)]

    def run_mode(mode):
        mine = rank_views(all_views, rank, world, mode)
        if not mine:                                        # more ranks than views: this rank only keeps the barriers
            els = []
            for _ in range(n_regions):
                coll.barrier(); coll.barrier()
                els.append(coll.max(0.0))
            return els, {}, {}, 0
        el, acc, last = timed_region(coll, ctxs, st, mine * spc, n_calls, args.warmup, repeats=n_regions, n_keep=len(mine),
                                     keep_last_step=bool(args.dump_outputs), keep_first=full)
        last["views"] = mine
        return el, acc, last, len(mine) * spc * n_calls

    elapsed_all, acc, last, n_maps_rank = run_mode(args.scaling if world > 1 else "weak")
    if args.dump_outputs and rank == 0 and last.get("last_step"):
        dump_outputs(args.dump_outputs, last["last_step"], last["views"])
    n_rep = len(elapsed_all)
    elapsed = float(np.median(elapsed_all))                 # the headline: the median region
    elapsed_sum = float(np.sum(elapsed_all))                # the statistics are summed over all regions
    n_maps = int(round(coll.sum(n_maps_rank)))              # depth maps of ONE region, all ranks
    strong = None
    if full and world > 1 and args.scaling == "weak":
        s_all, _, _, s_rank = run_mode("strong")
        s_el = float(np.median(s_all))
        s_maps = int(round(coll.sum(s_rank)))
        strong = {"value": s_maps / s_el, "unit": "depth-maps/s", "ms_per_step": 1000.0 * s_el / args.steps,
                  "repeats": [s_maps / e for e in s_all],
                  "views_per_rank": [len(shard_views(all_views, r, world)) for r in range(world)],
                  "note": "BASELINE config 4: the %d reference views of ONE scene dealt round-robin over the %d ranks, "
                          "same steps / warm-up / call plan; depth maps of all ranks / slowest rank" % (p.n_views, world)}

    # The same plan with the sweep's former seed rule (MI_DMRECON_SEED_REOPT=0: every seed propagates at once -- faster, but it
    # can fill pixels the reference's queue never reaches; the default since round 5 is the reference's rule): reported next to
    # `value`, never as `value`.  Only where the default is in force and the run is the plain one-GPU line.
    seed_env = os.environ.get("MI_DMRECON_SEED_REOPT")
    seed_variant = None
    if full and world == 1 and seed_env is None and not args.no_seed_variant:
        os.environ["MI_DMRECON_SEED_REOPT"] = "0"
        try:
            mine = rank_views(all_views, rank, world, "weak")
            v_el, _, _ = timed_region(coll, ctxs, st, mine * spc, n_calls, min(args.warmup, 1), repeats=2, n_keep=len(mine))
            seed_variant = {"value": len(mine) * spc * n_calls / float(np.median(v_el)), "unit": "depth-maps/s",
                            "repeats": [len(mine) * spc * n_calls / e for e in v_el],
                            "what": "MI_DMRECON_SEED_REOPT=0: every seed propagates at once (the sweep's rule until round 5; not the "
                                    "reference's: on some scenes it fills pixels the reference does not, DESIGN section 2)"}
        finally:
            del os.environ["MI_DMRECON_SEED_REOPT"]

    one_call = None
    if full and rank == 0 and world == 1 and not args.no_one_call:
        one_call = run_one_call(ctx, st, all_views, scene, cfg, n_timed=max(1, args.one_call_n))

    distinct = None
    n_distinct = args.distinct_scenes if args.distinct_scenes >= 0 else (20 if (args.config == "C3" and world == 1) else 0)
    if full and rank == 0 and world == 1 and n_distinct > 0:
        distinct = run_distinct_scenes(coll, local_rank, cfg, st, n_distinct, spc, n_calls, n_streams, min(args.warmup, 2), min(n_regions, 3))

    if rank == 0:
        res = last["res"]
        shape = last["shape"]
        fill = float(np.mean([(c > 0).mean() for _, c in res]))
        sharding = ("reference views are independent; each rank reconstructs all views of its scene replica per step, no collective"
                    if (world == 1 or args.scaling == "weak") else
                    "ONE scene: its reference views are dealt round-robin over the ranks (shard_views), every rank holds the "
                    "whole scene resident, no collective")
        roof = roofline(acc, n_maps_rank * n_rep, scene, cfg, n_streams, spc, elapsed_sum)
        out = {
            "metric": "depth-maps/sec (1920x1080, 20 views, scale=2)" if args.config == "C3" else "depth-maps/sec (%s)" % args.config,
            "value": n_maps / elapsed, "unit": "depth-maps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1000.0 * elapsed / args.steps, "higher_is_better": True,
            # every timed region of this process (each exactly `steps` steps between barriers); `value` is their median
            "repeats": [n_maps / e for e in elapsed_all],
            "scaling": args.scaling if world > 1 else "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s: %d-view %dx%d synthetic height-field scene, scale=%d (%dx%d depth maps), "
                                   "%d local neighbours, 2000 features; one step = all %d reference views"
                                   % (args.config, p.n_views, p.width, p.height, cfg["scale"], shape[1],
                                      shape[0], cfg["local_neighbors"], p.n_views),
                       "sharding": sharding,
                       "host_threads_per_gpu": n_streams, "steps_per_call": spc,
                       # concurrent calls with equal settings are merged into one batch by the library
                       # (mi_dmrecon_reconstruct; MI_DMRECON_MERGE_CALLS=0 switches it off): how large the batches were
                       "library_batches": int(n_calls * n_rep - acc.get("merged_into_other_call", 0)),   # all regions
                       "views_per_library_batch": round(n_maps_rank * n_rep / max(1, n_calls * n_rep - acc.get("merged_into_other_call", 0)), 1),
                       # (calls merged, batch ms, ms after the start of the timed region at which it returned), per batch
                       "library_batch_log": last.get("batches", [])[:16],
                       # calls per library batch in every timed region (same order as `repeats`)
                       "calls_per_library_batch_by_region": last.get("batch_shapes", []),
                       "mean_fill": round(fill, 4),
                       # how the maps of a timed batch reached the host (mi_dmrecon_stats::n_sparse_records): batches of 48+ views get a
                       # snapshot of the state at the hand-over to the front kernel, copied while that kernel runs, plus the pixels
                       # the front changed afterwards (this many per depth map; 0: the maps of a view are copied when the view has
                       # ended; MI_DMRECON_SPARSE_MAPS) -- the maps are on the host when a call returns either way
                       "maps_changed_pixels_per_depth_map": round(max(0, acc.get("n_sparse_records", 0)) / max(1, n_maps_rank * n_rep), 1),
                       # what `value` batches: every timed step reconstructs the SAME scene's reference views (one resident
                       # scene: a saturated-throughput figure whose concurrent jobs share one image set) ...
                       "distinct_scenes": 1,
                       # which entry point `value` is measured through (the drop-in binary's own figure: cpu_baseline.drop_in_app_same_scene)
                       "entry_point": "mi_dmrecon_reconstruct through mve_amd/api.py, no progress array: concurrent calls are merged into one "
                                      "batch, batches of 48+ views return their maps as snapshot + changed pixels; the mvs::DMRecon shim passes "
                                      "progress arrays and batches its instances itself (neither path)",
                       # which seeds propagate (MI_DMRECON_SEED_REOPT): the reference's rule unless the environment says otherwise
                       "seed_semantics": {None: "reference (a seed propagates only if re-optimising it raised its confidence; in the seed launch)",
                                          "2": "reference (a seed propagates only if re-optimising it raised its confidence; in the seed launch)",
                                          "1": "reference (as a round of its own)", "0": "every seed propagates at once (not the reference's rule)"}.get(seed_env, "reference")},
            "roofline": roof,
            # the scene's way into HBM, timed by itself before the timed regions (never part of `value`): host images ->
            # page-locked staging -> PCIe -> RGBA pack, pyramid and footprint records on the device
            "staging": {"seconds": t_stage, "host_image_bytes": host_bytes, "GB_per_s": host_bytes / t_stage / 1e9,
                        "synthetic_render_seconds": t_render,
                        # reconstructing the scene ONCE, staging included: n views / (staging + one pass over them)
                        "pcie_inclusive_depth_maps_per_s": p.n_views / (t_stage + elapsed * p.n_views / max(n_maps, 1))},
        }
        if share_gpu:
            out["config"]["ranks_share_one_gpu"] = True
            out["per_rank_ms_per_step"] = 1000.0 * elapsed / args.steps
        if one_call is not None:
            out["one_call"] = one_call
            # ... what ONE scene reconstructed once gets (a user of apps/dmrecon): the `one_call` object's rate
            out["config"]["single_scene_value"] = one_call["depth_maps_per_s"]
        if distinct is not None:
            # ... and the same plan on distinct data: every step another scene
            out["config"]["distinct_scenes_variant"] = distinct
        if seed_variant is not None:
            out["config"]["all_seeds_propagate_variant"] = seed_variant
        if strong is not None:
            out["strong_scaling"] = strong
        if args.config == "C3":
            pred = predicted_strong_scaling(p.n_views)
            if pred is not None:
                # (next to the measured sub-object when N > 1; at N = 1 the only thing there is to say about config 4)
                out.setdefault("strong_scaling", {})["predicted_from_one_gpu"] = pred
        if full and world == 1 and not args.no_cpu_baseline:
            # the maps of the FIRST timed call (first region) and of the LAST one (last region) against the reference's
            last_maps = last.get("res_last", res)
            out["cpu_baseline"], parity = cpu_baseline(scene, cfg, gpu_maps=res[:p.n_views], gpu_maps_last=last_maps[:p.n_views],
                                                       global_views=lambda v: ctx.global_view_selection(st, v))
            if parity is not None:
                out["parity"] = parity
    coll.barrier()
    for c in ctxs[1:]:
        c.close()
    ctx.close()
    coll.close()
    if rank == 0:
        # the one JSON line, last on stdout: RCCL writes its version banner through C stdio, which would otherwise
        # be flushed only at exit, i.e. after this line
        import ctypes
        sys.stdout.flush()
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
