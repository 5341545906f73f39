"""Regenerates tests/golden/sift_s1.npz or, with --set s2, tests/golden/sift_s2.npz.  Run by hand where the reference tree exists:

    python tests/golden/make_golden_sift.py [--set s1|s2] [--ref /path/to/mve] [--out DIR] [--keep DIR]

Compiles the reference's libs/sfm/sift.cc and libs/mve/image_tools.cc with tests/golden/ref_sift_driver.cc twice, into a
temporary directory outside the repository:
  route A  -O3 -march=x86-64-v3 -funsafe-math-optimizations -fno-math-errno   (the reference's own flags, Makefile.inc)
  route B  -O2 -ffp-contract=off
and records keypoints and descriptors of both for the cases of the set (s1: the six of make_cases; s2: the three of
make_cases_s2, at the shapes of tests/test_sift_stages.py).  Never run by build() or by a test.

The images are synthetic: Gaussian blobs of mixed sigma and sign on low-pass noise, seeded.  A descriptor of route A is
STABLE if route B has it too (sift_pairing.STABLE_GATE); the script asserts that at least 95 % are on every case, and
writes the largest A-versus-B difference per quantity over all stable pairs of all cases into the fixture (tol_desc: position
/ scale, log2 scale, orientation, descriptor L2; tol_kp: position, sample), which tests/test_sift.py multiplies by 8.
Set s2 also stores loc_bound = 8 x its tol_kp: what tests/test_sift_stages.py allows between the device's localisation and
the float64 restatement of it, a bound that comes from the reference's two builds and not from the device."""
import argparse
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sift_pairing as P  # noqa: E402
import sift_restatement as R  # noqa: E402

ROUTES = {"a": "-O3 -march=x86-64-v3 -funsafe-math-optimizations -fno-math-errno", "b": "-O2 -ffp-contract=off"}
COMMON = "-fopenmp -DMVE_NO_JPEG_SUPPORT -DMVE_NO_TIFF_SUPPORT -DMVE_NO_PNG_SUPPORT -std=c++17 -pthread -w"
DEFAULTS = dict(num_samples_per_octave=3, min_octave=0, max_octave=4, contrast_threshold=-1.0, edge_ratio_threshold=10.0,
                base_blur_sigma=1.6, inherent_blur_sigma=0.5)
FIELDS = list(DEFAULTS)


def blobs(w, h, n, n_central, seed):
    """Gaussian blobs of mixed sigma and sign on low-pass noise, float32 in [0, 1].  The first n_central are small and keep
    19 pixels from the border where the image has the room: only there does a descriptor window (17 pixels and more to
    each side) stay inside an image of these sizes."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 0.5)
    for k in range(n):
        m = min(19.0, 0.4 * w, 0.4 * h) if k < n_central else 0.12 * min(w, h)
        cx, cy = rng.uniform(m, w - 1 - m), rng.uniform(m, h - 1 - m)
        s = rng.choice([1.1, 1.3, 1.5] if k < n_central else [1.2, 1.7, 2.4, 3.4, 4.8]) * rng.uniform(0.9, 1.1)
        ax = rng.uniform(1.0, 1.6)                                # a little elongated: a clear gradient orientation
        th = rng.uniform(0, np.pi)
        u, v = (x - cx) * np.cos(th) + (y - cy) * np.sin(th), -(x - cx) * np.sin(th) + (y - cy) * np.cos(th)
        img += rng.choice([-1.0, 1.0]) * rng.uniform(0.15, 0.35) * np.exp(-0.5 * ((u / (s * ax)) ** 2 + (v / s) ** 2))
    noise = rng.normal(size=(h, w))
    f = np.fft.rfft2(noise) * np.exp(-0.5 * (np.hypot(*np.meshgrid(np.fft.rfftfreq(w), np.fft.fftfreq(h))) / 0.06) ** 2)
    noise = np.fft.irfft2(f, s=(h, w))
    img += 0.03 * noise / noise.std()
    return np.clip(img, 0.0, 1.0).astype(np.float32)


def make_cases():
    g97 = blobs(97, 71, 40, 24, 20151104)
    g64 = blobs(64, 48, 18, 10, 20151105)
    rgb = np.clip(np.stack([g64 * 1.05, g64, g64 * 0.92], axis=2) * 255.0 + 0.5, 0, 255).astype(np.uint8)
    g33 = blobs(33, 20, 5, 0, 20151106)
    return [(g97, {}), (rgb, {}), (g97, dict(min_octave=-1, max_octave=2)), (g97, dict(min_octave=1)),
            (g64, dict(num_samples_per_octave=2)), (g33, dict(max_octave=3))]


def make_cases_s2():
    """The shapes no case of s1 reaches: two column tiles of the row blur (261 > 256), S = 1 with its 65 taps and descriptor
    windows of more than 64 rows, and octave -1 of an image that doubles past 256.  Windows of more than 128 rows stay
    unreached: they need a keypoint of octave 0 with a sample above 0.915, and the one extremum layer of S = 1 gives samples
    within +-0.5 unless the x / y steps of the localisation carry the fit away from it."""
    return [(blobs(261, 141, 60, 20, 20151117), dict(num_samples_per_octave=1, max_octave=1)),
            (blobs(261, 67, 60, 40, 20151108), {}),
            (blobs(131, 35, 24, 16, 20151109), dict(min_octave=-1, max_octave=1))]


SETS = {"s1": make_cases, "s2": make_cases_s2}


def unconditioned(img, o, kp, xyso, bound):
    """The descriptors of a route whose orientation a THIRD computation, sift_restatement.orientations on a float64 scale
    space, does not reproduce within `bound`: [(record, difference)].  Routes A and B round the Gaussian images the same way
    nearly everywhere, so they agree even where a pixel's gradient angle lies on the edge between two of the 36 histogram
    bins (36 * angle / 2 pi within rounding of an integer); any other rounding of the images, float64 here or the
    device's, moves that pixel's whole weight into the neighbouring bin and the peak with it, by up to 7e-3 rad for one
    pixel near the centre.  Such a record is stable between A and B but not a property of the image."""
    S, far = int(o["num_samples_per_octave"]), []
    space = {octave: imgs for octave, imgs, _ in R.scale_space(img, o)}
    for r, (x, y, s, ori) in enumerate(xyso.astype(np.float64)):
        f = 2.0 ** kp[:, 0].astype(np.float64)
        k = kp[np.argmin(np.abs(f * (kp[:, 2] + 0.5) - 0.5 - x) + np.abs(f * (kp[:, 3] + 0.5) - 0.5 - y)
                         + np.abs(np.log2(o["base_blur_sigma"] * f * 2.0 ** ((kp[:, 1] + 1.0) / S) / s)))]
        d = [abs((q - ori + np.pi) % (2 * np.pi) - np.pi) for q in R.orientations(space[int(k[0])], k[2], k[3], k[1], S, o["base_blur_sigma"])]
        if not d or min(d) > bound:
            far.append((r, float("%.3g" % min(d)) if d else None))
    return far


def build_driver(ref, work, route):
    exe = os.path.join(work, "ref_sift_driver_" + route)
    srcs = [os.path.join(ref, "libs", "sfm", "sift.cc"), os.path.join(ref, "libs", "mve", "image_tools.cc"),
            os.path.join(HERE, "ref_sift_driver.cc")]
    subprocess.check_call(["g++"] + ROUTES[route].split() + COMMON.split() + ["-I" + os.path.join(ref, "libs")] + srcs + ["-o", exe])
    return exe


def write_input(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for img, opts in cases:
            o = dict(DEFAULTS, **opts)
            h, w = img.shape[:2]
            f.write(struct.pack("<4i3i4f", w, h, img.shape[2] if img.ndim == 3 else 1, int(img.dtype == np.float32), *[o[k] for k in FIELDS]))
            f.write(np.ascontiguousarray(img).tobytes())


def read_output(path, n_cases):
    buf, res, off = open(path, "rb").read(), [], 0
    for _ in range(n_cases):
        n = struct.unpack_from("<i", buf, off)[0]
        kp = np.frombuffer(buf, np.float32, n * 4, off + 4).reshape(n, 4)
        off += 4 + n * 16
        n = struct.unpack_from("<i", buf, off)[0]
        rec = np.frombuffer(buf, np.float32, n * 132, off + 4).reshape(n, 132)
        off += 4 + n * 528
        res.append((kp.copy(), rec[:, :4].copy(), rec[:, 4:].copy()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--set", default="s1", choices=sorted(SETS), dest="name")
    ap.add_argument("--out", default=HERE, help="where sift_<set>.npz goes")
    ap.add_argument("--keep", default=None, help="keep the build directory here (e.g. to reuse the drivers)")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="sift_golden_")
    os.makedirs(work, exist_ok=True)
    cases = SETS[a.name]()
    fin = os.path.join(work, a.name + ".in")
    write_input(fin, cases)
    res = {}
    for route in ROUTES:
        exe = os.path.join(work, "ref_sift_driver_" + route)
        if not os.path.exists(exe):
            exe = build_driver(a.ref, work, route)
        subprocess.check_call([exe, fin, os.path.join(work, a.name + ".out_" + route)])
        res[route] = read_output(os.path.join(work, a.name + ".out_" + route), len(cases))

    out = dict(n_cases=np.int32(len(cases)))
    gate_d = [P.STABLE_GATE[k] for k in ("pos", "scale", "ori", "desc")]
    gate_k = [P.STABLE_GATE[k] for k in ("pos", "sample")]
    tol_d, tol_k, n_desc_all = np.zeros(4), np.zeros(2), 0
    for c, (img, opts) in enumerate(cases):
        o = dict(DEFAULTS, **opts)
        out["image_%d" % c] = img
        out["options_%d" % c] = np.asarray([o[k] for k in FIELDS], np.float64)
        (kpa, xa, da), (kpb, xb, db) = res["a"][c], res["b"][c]
        for r, (kp, x, d) in (("a", res["a"][c]), ("b", res["b"][c])):
            out["kp_%s_%d" % (r, c)], out["xyso_%s_%d" % (r, c)], out["desc_%s_%d" % (r, c)] = kp, x, d
        _, ed = P.descriptor_errors(xa, da, xb, db)
        _, ek = P.keypoint_errors(kpa, kpb)
        sd, sk = P.within(ed, gate_d), P.within(ek, gate_k)
        print("case %d: %s %s: route A %d keypoints %d descriptors, route B %d / %d; stable %d (%.1f %%) / %d (%.1f %%)"
              % (c + 1, img.shape, opts, len(kpa), len(xa), len(kpb), len(xb), sk.sum(), 100.0 * sk.mean(), sd.sum(), 100.0 * sd.mean() if len(sd) else 100.0))
        assert len(kpa) >= 4 and sk.mean() >= 0.95 and (len(xa) == 0 or sd.mean() >= 0.95), "change the image, not the cap"
        n_desc_all += len(xa)
        tol_d = np.maximum(tol_d, ed[sd].max(axis=0)) if sd.any() else tol_d
        tol_k = np.maximum(tol_k, ek[sk].max(axis=0))
    assert n_desc_all >= 40, n_desc_all
    out["tol_desc"], out["tol_kp"] = tol_d, tol_k
    if a.name == "s2":
        out["loc_bound"] = 8.0 * tol_k
        for c, (img, opts) in enumerate(cases):
            far = unconditioned(img, dict(DEFAULTS, **opts), res["a"][c][0], res["a"][c][1], 8.0 * tol_d[2])
            print("case %d: orientations of route A the float64 restatement does not reproduce within 8 x %.3g: %s" % (c + 1, tol_d[2], far))
            assert not far, "change the image, not the cap"
    print("largest A-versus-B difference: descriptors position/scale %.3g, log2 scale %.3g, orientation %.3g, L2 %.3g; "
          "keypoints position %.3g, sample %.3g" % (*tol_d, *tol_k))
    path = os.path.join(a.out, "sift_%s.npz" % a.name)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
