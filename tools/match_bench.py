"""Measures the exhaustive matching of mi_dmrecon_match_pairs against the reference's Matching::twoway_match on the same box.

    python tools/match_bench.py --build-ref [--ref /path/to/mve]     # where the reference tree exists: build/ref_match_bench
    python tools/match_bench.py [--sets 20] [--n 10000] [--repeats 5] [--cpu-repeats 2] [--threads 16] [--out FILE.json]

Workload: `--sets` SIFT sets of `--n` unit-norm descriptors (a fifth of each planted as near-duplicates of a shared pool),
all sets * (sets - 1) / 2 pairs in ONE pairs call.  GPU: one warm-up call, then the median wall time of `--repeats` calls,
each ending with its results in host memory (the call synchronises).  CPU: tests/golden/ref_match_driver.cc in its `bench`
mode, linked with the reference's own libs/sfm built with the reference's flags (Makefile.inc: -O3 -funsafe-math-optimizations,
-march=x86-64-v3 in place of -march=native), OMP_NUM_THREADS = `--threads`: twoway_match over the same pairs, best of
`--cpu-repeats`.  Prints one JSON line; profiles/sfm_match.md quotes it.

A pair of |A| x |B| descriptors of D dims is |A| * |B| * D 8-bit multiply-adds for the library, which computes the matrix
once; the reference computes it twice (once per direction).  Rates below count the matrix ONCE for both, so they compare
the same useful work."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import match_restatement as R  # noqa: E402

REF_EXE = os.path.join(ROOT, "build", "ref_match_bench")
REF_FLAGS = ("-O3 -march=x86-64-v3 -funsafe-math-optimizations -fno-math-errno -fopenmp -DMVE_NO_JPEG_SUPPORT "
             "-DMVE_NO_TIFF_SUPPORT -std=c++17 -pthread -w")
PNGLIB = "/usr/lib/x86_64-linux-gnu/libpng16.so.16"
PNGINC = "/opt/conda/include"
FLT_MAX = float(np.finfo(np.float32).max)


def build_ref(ref: str) -> None:
    work = tempfile.mkdtemp(prefix="match_bench_")
    inc = os.path.join(work, "pnginc")
    os.makedirs(inc)
    for h in ("png.h", "pngconf.h", "pnglibconf.h"):
        shutil.copy(os.path.join(PNGINC, h), inc)
    srcs = [s for lib in ("util", "mve", "sfm") for s in sorted(glob.glob(os.path.join(ref, "libs", lib, "[!_]*.cc")))]
    srcs.append(os.path.join(ROOT, "tests", "golden", "ref_match_driver.cc"))
    flags = REF_FLAGS.split() + ["-I" + inc, "-I" + os.path.join(ref, "libs")]

    def compile_one(src):
        obj = os.path.join(work, os.path.relpath(src, "/").replace("/", "_") + ".o")
        subprocess.check_call(["g++"] + flags + ["-c", src, "-o", obj])
        return obj

    with ThreadPoolExecutor(max(1, min(os.cpu_count() or 1, 8))) as pool:
        objs = list(pool.map(compile_one, srcs))
    os.makedirs(os.path.dirname(REF_EXE), exist_ok=True)
    subprocess.check_call(["g++", "-fopenmp", "-pthread"] + objs + [PNGLIB, "-o", REF_EXE])
    shutil.rmtree(work, ignore_errors=True)
    print("built", REF_EXE)


def make_sets(n_sets: int, n: int, seed: int = 7):
    rng = np.random.default_rng(seed)
    pool = R.unit_descriptors(rng, n, R.SIFT)
    sets = []
    for _ in range(n_sets):
        s = R.unit_descriptors(rng, n, R.SIFT)
        k = n // 5
        v = np.abs(pool[rng.permutation(n)[:k]] + rng.normal(scale=0.02, size=(k, 128)))
        s[rng.permutation(n)[:k]] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        sets.append(s)
    return sets


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-ref", action="store_true")
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--sets", type=int, default=20)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.build_ref:
        build_ref(a.ref)
        return

    from mve_amd import api
    assert api.device_count() > 0, "match_bench needs a HIP device"
    sets = make_sets(a.sets, a.n)
    jobs = [(i, a.n, j, a.n) for i in range(a.sets) for j in range(i + 1, a.sets)]
    macs = len(jobs) * a.n * a.n * 128
    ctx = api.Context(0)
    m = ctx.match_open(a.sets)
    t0 = time.perf_counter()
    for v, s in enumerate(sets):
        m.set(v, api.MATCH_SIFT, s)
    t_upload = time.perf_counter() - t0
    res = m.pairs(api.MATCH_SIFT, jobs, 0.8, FLT_MAX)               # warm-up (buffers, code objects)
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        res = m.pairs(api.MATCH_SIFT, jobs, 0.8, FLT_MAX)
        times.append(time.perf_counter() - t0)
    gpu_s = float(np.median(times))
    consistent = int(sum(r[2] for r in res))
    m.close()
    ctx.close()
    out = dict(workload="%d SIFT sets x %d descriptors, %d pairs in one call" % (a.sets, a.n, len(jobs)),
               mult_adds_matrix_once=macs, gpu_upload_s=round(t_upload, 4), gpu_call_s=[round(t, 5) for t in times],
               gpu_median_s=round(gpu_s, 5), gpu_pairs_per_s=round(len(jobs) / gpu_s, 1), gpu_mult_adds_per_s=macs / gpu_s,
               gpu_consistent=consistent)

    if os.path.exists(REF_EXE) and a.cpu_repeats > 0:
        work = tempfile.mkdtemp(prefix="match_bench_")
        fin = os.path.join(work, "bench.in")
        empty = [np.zeros((0, 64), np.float32)] * a.sets
        R.write_driver_input(fin, sets, empty, (0.8, FLT_MAX), (0.7, FLT_MAX), [])
        env = dict(os.environ, OMP_NUM_THREADS=str(a.threads))
        txt = subprocess.check_output([REF_EXE, fin, os.path.join(work, "unused"), "bench", str(a.cpu_repeats)], env=env, text=True)
        shutil.rmtree(work, ignore_errors=True)
        secs = [float(l.split()[3]) for l in txt.splitlines() if l.startswith("repeat")]
        cons = [int(l.split()[5]) for l in txt.splitlines() if l.startswith("repeat")]
        threads = int(txt.splitlines()[0].split()[1])
        cpu_s = min(secs)
        out.update(cpu_threads=threads, cpu_call_s=secs, cpu_best_s=cpu_s, cpu_pairs_per_s=round(len(jobs) / cpu_s, 2),
                   cpu_mult_adds_per_s=macs / cpu_s, cpu_consistent=cons[0], speedup=round(cpu_s / gpu_s, 1),
                   same_consistent_count=bool(cons[0] == consistent))
    else:
        out.update(cpu="not measured (build/ref_match_bench missing: --build-ref where the reference tree exists)")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
