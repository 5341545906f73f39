"""Measures mi_dmrecon_ransac_fundamental (or, with --model, _homography or _pose_p3p) on the workload sfmrecon gives it:
one RANSAC per view pair (f, h), one per view that is tried (p3p).

    python tools/ransac_bench.py [--model f|h|p3p] [--jobs 190] [--iterations 1000] [--matches 3000] [--repeats 5] [--out FILE.json]

Workload: `--jobs` match sets of `--matches` synthetic two-view correspondences (points at depth 3-6 in front of two
cameras a baseline apart, noise 4e-4 on the normalised coordinates, the first 30 % of the second view's points replaced by
uniform outliers; one seed per job), `--iterations` samples of 8 distinct matches each, threshold 0.0015 -- all jobs in ONE
call.  One warm-up call, then the median wall time of `--repeats` calls, each ending with its results in host memory (the
call synchronises).  Prints one JSON line; profiles/ransac_f.md quotes it.

--model h: the same, over a near-plane (z = 4 + 0.15 x), samples of 4, threshold 0.005.  --model p3p: `--matches` 2D-3D
correspondences per job (default 5000; `--jobs` defaults to 1) of a camera turned 0.2 rad at (-0.4, 0.1, 0.3), K = diag(0.9,
0.9, 1), the first 30 % of the 2D points uniform, samples of 3, threshold 0.005; four hypotheses per iteration, so `tests`
counts 4 x iterations x correspondences.  profiles/ransac_hp.md quotes these two.

Counted work: jobs x iterations 8-point solves and jobs x iterations x matches Sampson tests.  The reference's own
RansacFundamental::estimate over the same match sets is NOT run by this tool: the comparison needs a driver built against
the reference tree, out of tree, and does not exist yet (profiles/ransac_f.md says so)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def two_view(n, seed, planar=False):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 6.0, n)], 1)
    if planar:
        X[:, 2] = 4.0 + 0.15 * X[:, 0]
    a = 0.12
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Y = X @ R.T + np.array([-1.0, 0.05, 0.1])
    m = np.hstack([X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]]) + rng.normal(0, 4e-4, (n, 4))
    k = int(0.3 * n)
    m[:k, 2:] = rng.uniform(-0.5, 0.5, (k, 2))
    return m


K = np.diag([0.9, 0.9, 1.0])


def view_of_points(n, seed):
    """n rows X Y Z u v"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 6.0, n)], 1)
    a = 0.2
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Y = (X @ R.T + np.array([-0.4, 0.1, 0.3])) @ K.T
    u = Y[:, :2] / Y[:, 2:] + rng.normal(0, 4e-4, (n, 2))
    k = int(0.3 * n)
    u[:k] = rng.uniform(-0.4, 0.4, (k, 2))
    return np.hstack([X, u])


def draw(n, iterations, seed, width=8):
    """`iterations` rows of `width` distinct indices below n, ascending (a std::set iterates ascending)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, n, (iterations, width))
    for r in np.flatnonzero((np.diff(np.sort(s, 1), axis=1) == 0).any(1)):
        s[r] = rng.choice(n, width, replace=False)
    return np.sort(s, 1).astype(np.int32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["f", "h", "p3p"], default="f")
    ap.add_argument("--jobs", type=int, default=None)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.jobs = a.jobs if a.jobs is not None else 1 if a.model == "p3p" else 190
    a.matches = a.matches if a.matches is not None else 5000 if a.model == "p3p" else 3000

    from mve_amd import api
    assert api.device_count() > 0, "ransac_bench needs a HIP device"
    ctx = api.Context(0)
    if a.model == "f":
        jobs = [(two_view(a.matches, 100 + j), draw(a.matches, a.iterations, 500 + j), 0.0015) for j in range(a.jobs)]
        call, best = ctx.ransac_fundamental, "best_iteration"
    elif a.model == "h":
        jobs = [(two_view(a.matches, 100 + j, planar=True), draw(a.matches, a.iterations, 500 + j, 4), 0.005) for j in range(a.jobs)]
        call, best = ctx.ransac_homography, "best_iteration"
    else:
        jobs = [(view_of_points(a.matches, 100 + j), K, draw(a.matches, a.iterations, 500 + j, 3), 0.005) for j in range(a.jobs)]
        call, best = ctx.ransac_pose_p3p, "best_hypothesis"
    res = call(jobs)                                                  # warm-up (buffers, code objects)
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        res = call(jobs)
        times.append(time.perf_counter() - t0)
    gpu_s = float(np.median(times))
    solves = a.jobs * a.iterations
    tests = solves * a.matches * (4 if a.model == "p3p" else 1)
    out = dict(model=a.model, workload="%d jobs x %d iterations x %d matches in one call" % (a.jobs, a.iterations, a.matches),
               solves=solves, sampson_tests=tests, gpu_call_s=[round(t, 6) for t in times], gpu_median_s=round(gpu_s, 6),
               gpu_jobs_per_s=round(a.jobs / gpu_s, 1), gpu_sampson_tests_per_s=tests / gpu_s,
               inliers_mean=float(np.mean([len(r["inliers"]) for r in res])), jobs_with_a_winner=int(sum(r[best] >= 0 for r in res)),
               sweep_capped=ctx.ransac_sweep_capped, cpu="not measured")
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
