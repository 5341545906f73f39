"""Regenerates tests/golden/ba_b1.npz.  Run by hand where the reference tree exists:

    python tests/golden/make_golden_ba.py [--ref /path/to/mve] [--out DIR] [--keep DIR]

Compiles the reference's libs/sfm/bundle_adjustment.cc and ba_linear_solver.cc with tests/golden/ref_ba_driver.cc twice, into
a temporary directory outside the repository:
  route A  -O3 -march=x86-64-v3 -funsafe-math-optimizations -fno-math-errno   (the reference's own flags, Makefile.inc)
  route B  -O2 -ffp-contract=off
and records what both leave behind on the cases below, run to convergence with default options.  Never run by build() or
by a test.

The fixture also holds, per quantity (final MSE relative, camera parameters, point coordinates), the largest difference
over the four CPU routes -- the two builds and the two solves of tests/ba_restatement.py (Schur + CG, dense) -- which
tests/test_ba.py multiplies by 8: `spread` for the runs to convergence, and `spread_step` for the same four routes stopped
after one LM iteration on STEP_CASES (nothing else of those is stored).  The two differ: at convergence the MSE is
stationary and the routes agree on it to 1e-11, after a single step a CG that stops at r.r < 1e-20 and a dense solve are
1e-8 apart.  A case on which the four routes disagree about an LM count is refused: change the seed, not the band."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ba_restatement as R  # noqa: E402

ROUTES = {"a": "-O3 -march=x86-64-v3 -funsafe-math-optimizations -fno-math-errno", "b": "-O2 -ffp-contract=off"}
COMMON = "-fopenmp -std=c++17 -pthread -w"
CASES = [("c3", R.BOTH, 0), ("c3", R.BOTH, 1), ("c2", R.CAMERAS, 0), ("c2", R.POINTS, 0), ("reject", R.BOTH, 0)]
STEP_CASES = [("c2", R.BOTH, 0), ("c2", R.BOTH, 1), ("c3", R.BOTH, 0), ("c3", R.BOTH, 1), ("c2", R.CAMERAS, 0), ("c2", R.POINTS, 0)]
COUNTS = ("num_lm_iterations", "num_lm_successful_iterations", "num_lm_unsuccessful_iterations")


def build_driver(ref, work, route):
    exe = os.path.join(work, "ref_ba_driver_" + route)
    srcs = [os.path.join(ref, "libs", "sfm", "bundle_adjustment.cc"), os.path.join(ref, "libs", "sfm", "ba_linear_solver.cc"),
            os.path.join(HERE, "ref_ba_driver.cc")]
    subprocess.check_call(["g++"] + ROUTES[route].split() + COMMON.split() + ["-I" + os.path.join(ref, "libs")] + srcs + ["-o", exe])
    return exe


def write_input(path, cases):
    """The format of ref_ba_driver.cc; also used by tests/test_ba.py for build/ba_class_check."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for P, mode, fixed, lm_max in cases:
            f.write(struct.pack("<6i", mode, fixed, lm_max, len(P["cams"]), len(P["pts"]), len(P["cam"])))
            for a, t in ((P["cams"], np.float64), (P["pts"], np.float64), (P["const"], np.int32), (P["xy"], np.float64),
                         (P["cam"], np.int32), (P["pt"], np.int32)):
                f.write(np.ascontiguousarray(a, t).tobytes())


def read_output(path, cases):
    buf, res, off = open(path, "rb").read(), [], 0
    for P, _, _, _ in cases:
        n, m = len(P["cams"]), len(P["pts"])
        cams = np.frombuffer(buf, np.float64, n * 15, off).reshape(n, 15).copy()
        off += n * 120
        pts = np.frombuffer(buf, np.float64, m * 3, off).reshape(m, 3).copy()
        off += m * 24
        mse = np.frombuffer(buf, np.float64, 2, off).copy()
        counts = np.frombuffer(buf, np.int32, 4, off + 16).copy()
        off += 32
        res.append((cams, pts, mse, counts))
    return res


def four_routes(a, work, tag, cases):
    """Per case the results of the two builds and the two restated solves as (cameras, points, final MSE, LM counts), and
    what the drivers wrote."""
    fin = os.path.join(work, tag + ".in")
    write_input(fin, cases)
    res = {}
    for route in ROUTES:
        exe = os.path.join(work, "ref_ba_driver_" + route)
        if not os.path.exists(exe):
            exe = build_driver(a.ref, work, route)
        subprocess.check_call([exe, fin, os.path.join(work, tag + ".out_" + route)])
        res[route] = read_output(os.path.join(work, tag + ".out_" + route), cases)
    every = []
    for c, (P, mode, fixed, lm_max) in enumerate(cases):
        routes = [(r[0], r[1], r[2][1], r[3][:3]) for r in (res["a"][c], res["b"][c])]
        for step in (R.step_schur, R.step_dense):
            cams, pts, st, _ = R.optimize(P, step, bundle_mode=mode, fixed_intrinsics=fixed, lm_max_iterations=lm_max)
            routes.append((cams, pts, st["final_mse"], np.array([st[k] for k in COUNTS], np.int32)))
        for r in routes[1:]:
            assert np.array_equal(r[3], routes[0][3]), "%s case %d: the CPU routes disagree about an LM count: change the seed" % (tag, c)
        every.append(routes)
    return every, res


def worst_pair(routes):
    worst = np.zeros(3)
    for i in range(4):
        for j in range(i):
            x, y = routes[i], routes[j]
            worst = np.maximum(worst, [abs(x[2] - y[2]) / y[2], np.abs(x[0] - y[0]).max(), np.abs(x[1] - y[1]).max()])
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE, help="where ba_b1.npz goes")
    ap.add_argument("--keep", default=None, help="keep the build directory here (e.g. to reuse the drivers)")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="ba_golden_")
    os.makedirs(work, exist_ok=True)
    cases = [(R.scene(name), mode, fixed, 50) for name, mode, fixed in CASES]
    every, res = four_routes(a, work, "b1", cases)

    out = dict(n_cases=np.int32(len(cases)), scenes=np.array([c[0] for c in CASES]))
    spread = np.zeros(3)                                                  # final MSE (relative), cameras, points
    for c, (P, mode, fixed, _) in enumerate(cases):
        routes = every[c]
        worst = worst_pair(routes)
        print("case %d: %s mode %d fixed %d: LM %s, CG %d / %d, final MSE %.6e; spread mse %.2e cameras %.2e points %.2e"
              % (c, CASES[c][0], mode, fixed, routes[0][3], res["a"][c][3][3], res["b"][c][3][3], routes[0][2], *worst))
        spread = np.maximum(spread, worst)
        out["options_%d" % c] = np.array([mode, fixed], np.int32)
        for k in ("cams", "pts", "const", "xy", "cam", "pt"):
            out["%s_%d" % (k, c)] = P[k]
        for r in ("a", "b"):
            out["cams_%s_%d" % (r, c)], out["pts_%s_%d" % (r, c)], out["mse_%s_%d" % (r, c)], out["counts_%s_%d" % (r, c)] = res[r][c]
    out["spread"] = spread
    steps, _ = four_routes(a, work, "b1_step", [(R.scene(name), mode, fixed, 1) for name, mode, fixed in STEP_CASES])
    out["spread_step"] = np.max([worst_pair(r) for r in steps], axis=0)
    print("spread_step (MSE after one step relative, cameras, points):", out["spread_step"])
    print("spread (final MSE relative, cameras, points):", spread)
    path = os.path.join(a.out, "ba_b1.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
