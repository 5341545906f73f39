"""Measures mi_dmrecon_ba_optimize on the workload the incremental bundler gives it.

    python tools/ba_bench.py [--cameras 20] [--points 50000] [--track 4] [--repeats 5] [--out FILE.json]

Workload: `--cameras` cameras on an arc around a cloud of `--points` points, each point seen by `--track` cameras (about
cameras x points x track / cameras observations: 200 000 by default), pixel noise 5e-4, initial parameters perturbed by
1e-2 (tests/ba_restatement.py make_scene).  Timed, each after one warm-up call, as the median wall time of `--repeats`
calls that end with the results in host memory (the call synchronises):
  full      one BA_CAMERAS_AND_POINTS run with the default options, as after every added view and at the end;
  cameras   BA_CAMERAS, and
  points    BA_POINTS, the two calls the bundler makes for one added view (here over the whole scene).
Prints one JSON line; profiles/ba.md quotes it.  MI_DMRECON_LIB chooses the library (a build with another BA_CG_BATCH).

The reference's own BundleAdjustment::optimize over the same scene is NOT run by this tool: that needs
tests/golden/ref_ba_driver.cc built against the reference tree (tests/golden/make_golden_ba.py shows how)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=20)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--track", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mve_amd import api
    import ba_restatement as R
    assert api.device_count() > 0, "ba_bench needs a HIP device"

    tracks = [[(p + k * (a.cameras // a.track)) % a.cameras for k in range(a.track)] for p in range(a.points)]
    P = R.make_scene(a.cameras, tracks, 7)
    cams, pts, obs = np.zeros(a.cameras, api.BA_CAMERA), np.zeros(a.points, api.BA_POINT), np.zeros(len(P["cam"]), api.BA_OBSERVATION)
    cams["focal_length"], cams["distortion"], cams["translation"], cams["rotation"] = P["cams"][:, 0], P["cams"][:, 1:3], P["cams"][:, 3:6], P["cams"][:, 6:]
    pts["pos"] = P["pts"]
    obs["pos"], obs["camera_id"], obs["point_id"] = P["xy"], P["cam"], P["pt"]

    ctx = api.Context(0)
    res = dict(cameras=a.cameras, points=a.points, observations=int(len(obs)), repeats=a.repeats, library=api.LIB_PATH)
    for name, mode in (("full", api.BA_CAMERAS_AND_POINTS), ("cameras", api.BA_CAMERAS), ("points", api.BA_POINTS)):
        _, _, st, _ = ctx.bundle_adjust(cams, pts, obs, bundle_mode=mode)
        times = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            ctx.bundle_adjust(cams, pts, obs, bundle_mode=mode)
            times.append((time.perf_counter() - t0) * 1e3)
        res[name] = dict(ms_median=float(np.median(times)), ms_min=float(min(times)), ms_max=float(max(times)),
                         lm_iterations=st["num_lm_iterations"], cg_iterations=st["num_cg_iterations"],
                         initial_mse=st["initial_mse"], final_mse=st["final_mse"])
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
