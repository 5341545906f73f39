"""Measures mi_dmrecon_ransac_fundamental on the workload sfmrecon gives it: one RANSAC per view pair.

    python tools/ransac_bench.py [--jobs 190] [--iterations 1000] [--matches 3000] [--repeats 5] [--out FILE.json]

Workload: `--jobs` match sets of `--matches` synthetic two-view correspondences (points at depth 3-6 in front of two
cameras a baseline apart, noise 4e-4 on the normalised coordinates, the first 30 % of the second view's points replaced by
uniform outliers; one seed per job), `--iterations` samples of 8 distinct matches each, threshold 0.0015 -- all jobs in ONE
call.  One warm-up call, then the median wall time of `--repeats` calls, each ending with its results in host memory (the
call synchronises).  Prints one JSON line; profiles/ransac_f.md quotes it.

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


def two_view(n, seed):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 6.0, n)], 1)
    a = 0.12
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Y = X @ R.T + np.array([-1.0, 0.05, 0.1])
    m = np.hstack([X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]]) + rng.normal(0, 4e-4, (n, 4))
    k = int(0.3 * n)
    m[:k, 2:] = rng.uniform(-0.5, 0.5, (k, 2))
    return m


def draw(n, iterations, seed):
    """`iterations` rows of 8 distinct indices below n, ascending (a std::set iterates ascending)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, n, (iterations, 8))
    for r in np.flatnonzero((np.diff(np.sort(s, 1), axis=1) == 0).any(1)):
        s[r] = rng.choice(n, 8, replace=False)
    return np.sort(s, 1).astype(np.int32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=190)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from mve_amd import api
    assert api.device_count() > 0, "ransac_bench needs a HIP device"
    jobs = [(two_view(a.matches, 100 + j), draw(a.matches, a.iterations, 500 + j), 0.0015) for j in range(a.jobs)]
    ctx = api.Context(0)
    res = ctx.ransac_fundamental(jobs)                                # warm-up (buffers, code objects)
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        res = ctx.ransac_fundamental(jobs)
        times.append(time.perf_counter() - t0)
    gpu_s = float(np.median(times))
    solves, tests = a.jobs * a.iterations, a.jobs * a.iterations * a.matches
    out = dict(workload="%d jobs x %d iterations x %d matches in one call" % (a.jobs, a.iterations, a.matches),
               solves=solves, sampson_tests=tests, gpu_call_s=[round(t, 5) for t in times], gpu_median_s=round(gpu_s, 5),
               gpu_jobs_per_s=round(a.jobs / gpu_s, 1), gpu_sampson_tests_per_s=tests / gpu_s,
               inliers_mean=float(np.mean([len(r["inliers"]) for r in res])), jobs_with_a_winner=int(sum(r["best_iteration"] >= 0 for r in res)),
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
