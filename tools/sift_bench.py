"""Measures Context.sift (mi_dmrecon_sift_run + mi_dmrecon_sift_get) on one image of sfmrecon's default max_image_size.

    python tools/sift_bench.py [--width 3000] [--height 2000] [--repeats 5] [--ref-driver EXE [--threads 16]] [--out FILE.json]

Workload: one synthetic grey float image (band-passed noise of four scales, seeded: extrema at every octave), default
Sift::Options.  One warm-up call, then the median wall time of `--repeats` calls, each ending with keypoints and descriptors
in host memory (the calls synchronise).  Prints one JSON line; profiles/sift.md quotes it.

`--ref-driver`: a build of tests/golden/ref_sift_driver.cc against the reference tree (tests/golden/make_golden_sift.py
--keep DIR leaves two).  Its `bench` mode processes the same image once per thread on `--threads` threads, as apps/sfmrecon
runs its views; the tool prints its lines.  Without it the reference's time is "not measured"."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(w, h, seed=20151104):
    rng = np.random.default_rng(seed)
    f = np.fft.rfft2(rng.normal(size=(h, w)))
    r = np.hypot(*np.meshgrid(np.fft.rfftfreq(w), np.fft.fftfreq(h)))
    img = np.zeros((h, w))
    for s in (0.15, 0.05, 0.015, 0.005):                          # cycles per pixel
        band = np.fft.irfft2(f * np.exp(-0.5 * (r / s) ** 2), s=(h, w))
        img += band / band.std()
    return np.clip(0.5 + 0.08 * img, 0.0, 1.0).astype(np.float32)


def reference(exe, img, threads, repeats):
    from mve_amd import api
    with tempfile.TemporaryDirectory() as d:
        fin = os.path.join(d, "bench.in")
        with open(fin, "wb") as f:
            o = api.SIFT_DEFAULTS
            f.write(struct.pack("<i4i3i4f", 1, img.shape[1], img.shape[0], 1, 1, *[o[k] for k in o]))
            f.write(img.tobytes())
        env = dict(os.environ, OMP_NUM_THREADS=str(threads))
        return subprocess.check_output([exe, fin, os.path.join(d, "unused"), "bench", str(repeats)], env=env, text=True).splitlines()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3000)
    ap.add_argument("--height", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-driver", default=None)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-gpu", action="store_true", help="only the reference driver")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from mve_amd import api
    img = synthetic(a.width, a.height)
    out = dict(workload="%d x %d float grey, default options" % (a.width, a.height), reference="not measured")
    if a.ref_driver:
        out["reference"] = reference(a.ref_driver, img, a.threads, a.repeats)
    if not a.no_gpu:
        assert api.device_count() > 0, "sift_bench needs a HIP device"
        ctx = api.Context(0)
        kp, xyso, desc = ctx.sift(img)                                # warm-up (buffers, code objects)
        times = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            kp, xyso, desc = ctx.sift(img)
            times.append(time.perf_counter() - t0)
        ctx.close()
        out.update(gpu_call_s=[round(t, 5) for t in times], gpu_median_s=round(float(np.median(times)), 5),
                   keypoints=len(kp), descriptors=len(desc), keypoints_per_octave=np.bincount(kp["octave"]).tolist())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
