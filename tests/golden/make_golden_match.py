"""Regenerates tests/golden/match_m1.npz.  Run by hand where the reference tree exists:

    python tests/golden/make_golden_match.py [--ref /path/to/mve] [--out DIR] [--keep DIR]

Compiles the reference's libs/util, libs/mve, libs/sfm (its own exhaustive_matching.cc included) and
tests/golden/ref_match_driver.cc into a temporary directory outside the repository, with -O2 -ffp-contract=off (the
discretisation rounds value * 255 + 0.5: unfused, as the sources say), runs the driver on fixture M1 and writes the .npz.
Never run by build() or by a test.

M1: four views.  SIFT sets of 300, 257, 1 and 0 descriptors, SURF sets of 200, 64, 0 and 5: unit-norm random vectors with
near-duplicates planted across the views (so that a healthy share of the matches passes Lowe 0.8 / 0.7), exact duplicates
WITHIN a set (ties: the larger index wins), and one pair of identical descriptors across two sets (d1 = 0)."""
import argparse
import glob
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import match_restatement as R  # noqa: E402

FLAGS = "-O2 -ffp-contract=off -fopenmp -DMVE_NO_JPEG_SUPPORT -DMVE_NO_TIFF_SUPPORT -std=c++17 -pthread -w"
PNGLIB = "/usr/lib/x86_64-linux-gnu/libpng16.so.16"
PNGINC = "/opt/conda/include"
FLT_MAX = float(np.finfo(np.float32).max)
SIFT_OPTS, SURF_OPTS = (0.8, FLT_MAX), (0.7, FLT_MAX)          # MatchingBase::Options (libs/sfm/matching_base.h:25-31)
LOWRES = [50, 300]


def noisy(rng, base, kind, sigma=0.02):
    v = base + rng.normal(scale=sigma, size=base.shape)
    if kind == R.SIFT:
        v = np.abs(v)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def make_m1(seed: int = 20151104):
    rng = np.random.default_rng(seed)
    sets = {}
    for kind, sizes, n_pool in ((R.SIFT, (300, 257, 1, 0), 200), (R.SURF, (200, 64, 0, 5), 120)):
        pool = R.unit_descriptors(rng, n_pool, kind)
        v = []
        # view 0: the whole pool, noisy, then random ones; view 1: a shuffled part of the pool, noisy, then random ones
        v.append(np.concatenate([noisy(rng, pool, kind), R.unit_descriptors(rng, sizes[0] - n_pool, kind)]))
        part = rng.permutation(n_pool)[:sizes[1] * 3 // 5]
        v.append(np.concatenate([noisy(rng, pool[part], kind), R.unit_descriptors(rng, sizes[1] - len(part), kind)]))
        v[1] = v[1][rng.permutation(sizes[1])]
        for n in sizes[2:]:
            v.append(noisy(rng, pool[rng.permutation(n_pool)[:n]], kind) if n else np.zeros((0, R.DIMS[kind]), np.float32))
        # exact duplicates within a set: ties, which go to the larger index
        for s in (0, 1):
            for _ in range(6):
                a, b = rng.integers(0, sizes[s], 2)
                v[s][a] = v[s][b]
        # one descriptor shared exactly by views 0 and 1, a little longer than 1 so that its product with itself reaches
        # 255^2 (127^2): d1 = 0
        shared = (R.unit_descriptors(rng, 1, kind)[0] * np.float32(1.003)).astype(np.float32)
        v[0][7], v[1][5] = shared, shared
        sets[kind] = v
    return sets[R.SIFT], sets[R.SURF]


def check_domain(sets, kind):
    """The contract's domain: every inner product between two descriptors that meet in a call fits the reference's 16 bits."""
    d = [R.discretise(s, kind) for s in sets]
    for i in range(len(d)):
        for j in range(len(d)):
            if i != j and len(d[i]) and len(d[j]):
                assert R.in_domain(R.inner_products(d[i], d[j]), kind), (kind, i, j)


def build_driver(ref: str, work: str) -> str:
    inc = os.path.join(work, "pnginc")
    os.makedirs(inc, exist_ok=True)
    for h in ("png.h", "pngconf.h", "pnglibconf.h"):
        shutil.copy(os.path.join(PNGINC, h), inc)
    out = os.path.join(work, "obj")
    os.makedirs(out, exist_ok=True)
    srcs = [s for lib in ("util", "mve", "sfm") for s in sorted(glob.glob(os.path.join(ref, "libs", lib, "[!_]*.cc")))]
    srcs.append(os.path.join(HERE, "ref_match_driver.cc"))
    flags = FLAGS.split() + ["-I" + inc, "-I" + os.path.join(ref, "libs")]

    def compile_one(src):
        obj = os.path.join(out, os.path.relpath(src, "/").replace("/", "_") + ".o")
        subprocess.check_call(["g++"] + flags + ["-c", src, "-o", obj])
        return obj

    with ThreadPoolExecutor(max(1, min(os.cpu_count() or 1, 8))) as pool:
        objs = list(pool.map(compile_one, srcs))
    exe = os.path.join(work, "ref_match_driver")
    subprocess.check_call(["g++", "-fopenmp", "-pthread"] + objs + [PNGLIB, "-o", exe])
    return exe


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE, help="where match_m1.npz goes")
    ap.add_argument("--keep", default=None, help="keep the build directory here (e.g. to reuse the driver)")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="match_golden_")
    os.makedirs(work, exist_ok=True)
    sift, surf = make_m1()
    check_domain(sift, R.SIFT)
    check_domain(surf, R.SURF)
    d0, d1 = R.discretise(sift[0][7:8], R.SIFT), R.discretise(surf[0][7:8], R.SURF)
    assert 65025 <= int(R.inner_products(d0, d0)[0, 0]) <= 65535 and 16129 <= int(R.inner_products(d1, d1)[0, 0]) <= 32767
    exe = os.path.join(work, "ref_match_driver")
    if not os.path.exists(exe):
        exe = build_driver(a.ref, work)
    fin, fout = os.path.join(work, "m1.in"), os.path.join(work, "m1.out")
    R.write_driver_input(fin, sift, surf, SIFT_OPTS, SURF_OPTS, LOWRES)
    subprocess.check_call([exe, fin, fout])
    res = R.read_driver_output(fout, 4, len(LOWRES))

    out = dict(sift_opts=np.asarray(SIFT_OPTS, np.float32), surf_opts=np.asarray(SURF_OPTS, np.float32),
               lowres=np.asarray(LOWRES, np.int32))
    for v in range(4):
        out["sift_%d" % v], out["surf_%d" % v] = sift[v], surf[v]
    passed = {"sift": 0, "surf": 0}
    for (i, j), rec in res.items():
        for k, arr in rec.items():
            out["%s_%d_%d" % (k, i, j)] = arr
        passed["sift"] += int((rec["sift12"] >= 0).sum())
        passed["surf"] += int((rec["surf12"] >= 0).sum())
    assert passed["sift"] >= 100 and passed["surf"] >= 30, passed
    path = os.path.join(a.out, "match_m1.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); raw 1->2 matches that pass: %s" % (path, os.path.getsize(path), passed))
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
