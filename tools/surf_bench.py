"""Measures Context.surf (mi_dmrecon_surf_run + mi_dmrecon_surf_get) on one image of sfmrecon's default max_image_size.

    python tools/surf_bench.py [--width 3000] [--height 2000] [--repeats 20] [--ref-driver EXE] [--out FILE.json]

Workload: one synthetic grey uint8 image (band-passed noise of four scales, seeded: extrema at every octave), default
Surf::Options.  Two warm-up calls (buffers, code objects), then `--repeats` calls, each ending with keypoints and descriptors
in host memory (the calls synchronise); the median and the spread are reported.  Prints one JSON line; profiles/surf.md
quotes it.  Without a HIP device the tool fails; it has no CPU path.

`--ref-driver`: a program built against the reference tree that takes `IN OUT` (IN: int32 count, then per image int32 w, h,
channels, upright, float32 threshold and the bytes), runs sfm::Surf::process on one thread and prints the seconds it took per
image.  It is not part of this repository; without it the reference's time is "not measured"."""
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
    return np.clip((0.5 + 0.08 * img) * 255.0 + 0.5, 0, 255).astype(np.uint8)


def reference(exe, img):
    with tempfile.TemporaryDirectory() as d:
        fin = os.path.join(d, "bench.in")
        with open(fin, "wb") as f:
            f.write(struct.pack("<iiiiif", 1, img.shape[1], img.shape[0], 1, 0, 500.0))
            f.write(img.tobytes())
        env = dict(os.environ, OMP_NUM_THREADS="1")
        return subprocess.check_output([exe, fin, os.path.join(d, "unused")], env=env, text=True).splitlines()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3000)
    ap.add_argument("--height", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--ref-driver", default=None)
    ap.add_argument("--no-gpu", action="store_true", help="only the reference driver")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from mve_amd import api
    img = synthetic(a.width, a.height)
    out = dict(workload="%d x %d uint8 grey, default options" % (a.width, a.height), reference="not measured")
    if a.ref_driver:
        out["reference"] = reference(a.ref_driver, img)
    if not a.no_gpu:
        assert api.device_count() > 0, "surf_bench needs a HIP device"
        ctx = api.Context(0)
        for _ in range(2):
            kp, xyso, desc = ctx.surf(img)
        times = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            kp, xyso, desc = ctx.surf(img)
            times.append(time.perf_counter() - t0)
        ctx.close()
        out.update(gpu_call_s=[round(t, 5) for t in times], gpu_median_s=round(float(np.median(times)), 5),
                   gpu_min_s=round(min(times), 5), gpu_max_s=round(max(times), 5),
                   keypoints=len(kp), descriptors=len(desc), keypoints_per_octave=np.bincount(kp["octave"], minlength=4).tolist())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
