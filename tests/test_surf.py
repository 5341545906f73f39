"""SURF detection and description on the GPU (mve_amd/csrc/surf_device.hip behind Context.surf) against the numpy restatement
of sfm::Surf in surf_restatement.py, which agrees with the reference's own build without contraction byte for byte on cases
(a) - (e) (profiles/surf.md).  Keypoints and descriptor records must be the same lists, sub-pixel values to 1e-5, orientations
to 1e-5 rad; descriptor values within MARGIN x the largest L2 distance between the restatement's float32 and float64
descriptor routes (what rounding alone does to the reference's formula).  MARGIN = 8 as in test_sift.py: the device's sin,
cos and atan2 are a third route.  The distance is taken over the cases whose descriptors are compared, (a) - (e): 2.32e-7
when this was written, so the bound is 1.85e-6; with (f), where one rounded sample coordinate differs between the two
routes, it would be 1.67e-3.  Measured on an MI355X: the largest descriptor distance is 1.6e-7, every orientation is equal.

Equality of lists is asked only of inputs on which the restatement is not on an edge itself; the margins it returns are
asserted per case (EDGE)."""
import numpy as np
import pytest

import surf_restatement as R
from mve_amd import api

pytestmark = pytest.mark.gpu

MARGIN = 8.0
EDGE = dict(det=1e-6, half=1e-6, contrast=1e-6, bounds=1e-6, window=1e-9, length=1e-9)


def blobs(w, h, seed, sigmas, n, rgb=False):
    """Gaussian blobs of mixed sigma and sign on low-pass noise, uint8."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 0.5)
    for _ in range(n):
        s, cx, cy = rng.choice(sigmas) * rng.uniform(0.9, 1.1), rng.uniform(0, w), rng.uniform(0, h)
        img += rng.choice([-1.0, 1.0]) * rng.uniform(0.2, 0.45) * np.exp(-0.5 * (((x - cx) / (s * rng.uniform(1.0, 1.5))) ** 2 + ((y - cy) / s) ** 2))
    f = np.fft.rfft2(rng.normal(size=(h, w))) * np.exp(-0.5 * (np.hypot(*np.meshgrid(np.fft.rfftfreq(w), np.fft.fftfreq(h))) / 0.06) ** 2)
    noise = np.fft.irfft2(f, s=(h, w))
    g = np.clip((img + 0.03 * noise / noise.std()) * 255.0 + 0.5, 0, 255).astype(np.uint8)
    return np.stack([g, (g * 0.8 + 20).astype(np.uint8), (g * 0.6 + 60).astype(np.uint8)], axis=2) if rgb else g


# (f): the issue's 4104 x 4104 of 255 sums to 4104^2 x 255 = 2^32 - 49 216, which does not wrap; 4168 does, inside the patch
# (3848^2 x 255 < 2^32 < 4168^2 x 255 less what the patch is darker by), and 4168 - 640 is a multiple of 8 as well.
BIG, CROP, PATCH = 4168, 640, 320
CASES = "abcdef"


def images():
    big = blobs(641, 479, 2, [2, 3, 5, 8, 13, 20, 30, 40], 160, rgb=True)
    wrap = np.full((BIG, BIG), 255, np.uint8)
    wrap[-PATCH:, -PATCH:] = blobs(PATCH, PATCH, 6, [2, 3, 5, 8], 60)
    return dict(a=(blobs(131, 97, 1, [2, 3, 4, 6], 40), {}), b=(big, {}), c=(big, dict(use_upright_descriptor=True)),
                d=(blobs(67, 300, 3, [2, 3, 4], 50), {}), e=(blobs(20, 20, 4, [2], 3), {}), f=(wrap, {}))


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def runs(ctx):
    """Per case: the image and options, the GPU's results, the restatement's two routes and its margins; made once."""
    out = {}
    for name, (img, opts) in images().items():
        ref_img = img[-CROP:, -CROP:] if name == "f" else img
        kps, rec32, margins = R.surf(ref_img, **opts)
        _, rec64, _ = R.surf(ref_img, dtype=np.float64, keypoints=kps, **opts)
        out[name] = dict(img=img, opts=opts, gpu=ctx.surf(img, **opts), kps=kps, rec32=rec32, rec64=rec64, margins=margins)
    return out


def in_patch(x, y, side):
    return x >= side - PATCH and y >= side - PATCH


@pytest.mark.parametrize("name", CASES)
def test_against_the_restatement(runs, name):
    r = runs[name]
    kp, xyso, desc = r["gpu"]
    kps, rec32 = r["kps"], r["rec32"]
    shift = 0.0
    if name == "f":                                               # the keypoints inside the patch
        shift = float(BIG - CROP)
        kps = [k for k in kps if in_patch(k[5], k[6], CROP)]
        kp = kp[[in_patch(x, y, BIG) for x, y in zip(kp["x"], kp["y"])]]
    for k, v in r["margins"].items():
        assert v > EDGE[k], "the restatement is on an edge itself (%s: %g): change the seed" % (k, v)
    compared = [runs[c] for c in "abcde"]
    distance = max(np.linalg.norm(np.float64(a[5]) - b[5]) for q in compared for a, b in zip(q["rec32"], q["rec64"]))
    assert all([a[0] for a in q["rec32"]] == [b[0] for b in q["rec64"]] for q in compared)
    print("%s: %d keypoints, %d descriptors; float32-versus-float64 distance over (a) - (e) %.3e" % (name, len(kps), len(rec32), distance))
    # keypoints: the same extrema in the same order, sub-pixel values to 1e-5.  (f): a float32 position beyond 4096 is half an
    # ulp (2^-12) from its value, the crop's (near 600) another 2^-15, and only the keypoints are compared: a descriptor
    # samples at round(x + ...), which those 2^-12 move to the next pixel now and then.
    pos_tol = 1e-5 + (2.0 ** -12 + 2.0 ** -15 if name == "f" else 0.0)
    step = np.array([2.0 ** k[0] for k in kps])
    cells = np.stack([kp["octave"], np.rint(kp["sample"]), np.rint((kp["x"] - shift) / step), np.rint((kp["y"] - shift) / step)], axis=1)
    assert len(kp) == len(kps) and (cells == np.array([k[:4] for k in kps], np.float64).reshape(-1, 4)).all()
    for got, k in zip(kp, kps):
        assert abs(float(got["sample"]) - k[4]) <= 1e-5 and abs(float(got["x"]) - shift - k[5]) <= pos_tol and abs(float(got["y"]) - shift - k[6]) <= pos_tol
    if name == "f":
        assert len(kps) >= 20 and len(desc) > 0
        return
    # descriptor records: the same keypoints, x y scale equal, orientation to 1e-5 rad, values to MARGIN x distance
    assert len(xyso) == len(rec32)
    print("%s: largest descriptor L2 to the float32 restatement %.3e, bound %.3e; largest orientation difference %.3e"
          % (name, max([np.linalg.norm(d.astype(np.float64) - q[5]) for d, q in zip(desc, rec32)], default=0.0), MARGIN * distance,
             max([abs(float(g[3]) - float(q[4])) for g, q in zip(xyso, rec32)], default=0.0)))
    for g, d, q in zip(xyso, desc, rec32):
        assert g[0] == q[1] and g[1] == q[2] and g[2] == q[3]
        assert abs((float(g[3]) - float(q[4]) + np.pi) % (2 * np.pi) - np.pi) <= 1e-5
        l2 = np.linalg.norm(d.astype(np.float64) - q[5])
        assert l2 <= MARGIN * distance, (l2, MARGIN * distance)
    if name == "b":
        assert set(kp["octave"]) == {0, 1, 2, 3}
        assert sum(len(runs[c]["rec32"]) for c in "abcd") >= 40
    if name == "e":
        assert len(kp) == 0 and len(desc) == 0


def test_same_bytes_again_and_on_a_fork(ctx, runs):
    img, first = runs["b"]["img"], runs["b"]["gpu"]
    fork = ctx.fork()
    for other in (ctx, fork):
        other.sift(np.ascontiguousarray(img[:97, :131, 0]))       # a SIFT run in between leaves the SURF results alone
        again = other.surf(img)
        assert len(again[2]) > 30 and all(a.tobytes() == b.tobytes() for a, b in zip(again, first))
    fork.close()


@pytest.mark.parametrize("image, options, field", [
    (lambda: np.zeros((20, 33, 2), np.uint8), {}, "channels"),
    (lambda: np.zeros((20, 33), np.float32), {}, "image must be uint8"),
    (lambda: np.zeros((2, 40000), np.uint8), {}, "w, h"),
    (lambda: np.zeros((20, 33), np.uint8), dict(contrast_threshold=float("nan")), "contrast_threshold"),
], ids=["channels", "float32", "w", "nan"])
def test_refusals(ctx, runs, image, options, field):
    with pytest.raises(ValueError, match=field):
        ctx.surf(image(), **options)
    again = ctx.surf(runs["a"]["img"])                            # ... and the context still works
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, runs["a"]["gpu"]))
