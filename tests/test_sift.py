"""SIFT detection and description on the GPU (mve_amd/csrc/sift_device.hip behind Context.sift) against the reference's own
sfm::Sift, recorded in tests/golden/sift_s1.npz and sift_s2.npz (the shapes of test_sift_stages.py: two column tiles of the
row blur, S = 1 with 65 taps and descriptor windows of 79 rows, octave -1 past 256 columns) from two builds of it
(tests/golden/make_golden_sift.py): route A with the reference's flags, route B with -O2 -ffp-contract=off.  A record of route A is STABLE if route B has it too
(sift_pairing.STABLE_GATE).  Every stable record needs a GPU partner within 8 x the largest A-versus-B difference of each
quantity (measured over all cases when the fixture was made and stored in it); at most 1 % of the GPU's records (one at
least) may be without a partner in A or B.  8 x: the GPU's sums run in a lane tree, an order neither CPU route uses, while
A and B differ only by reassociation inside one loop."""
import os

import numpy as np
import pytest

import sift_pairing as P
from mve_amd import api

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_s1.npz"))
G2 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_s2.npz"))
FIELDS = list(api.SIFT_DEFAULTS)
MARGIN = 8.0


def options_of(c, G=G):
    o = dict(zip(FIELDS, G["options_%d" % c]))
    return {k: (int(v) if k in ("num_samples_per_octave", "min_octave", "max_octave") else float(v)) for k, v in o.items()}


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpu(ctx):
    """Every case once: (keypoints as (n, 4) octave sample x y, xyso, descriptors)."""
    out = []
    for c in range(int(G["n_cases"])):
        kp, xyso, desc = ctx.sift(G["image_%d" % c], **options_of(c))
        out.append((np.stack([kp["octave"].astype(np.float32), kp["sample"], kp["x"], kp["y"]], axis=1), xyso, desc))
    return out


def check(name, errors_of, a, b, g, gate, bound):
    """errors_of(x, y): per record of x the differences to its nearest record of y."""
    stable = P.within(errors_of(a, b), gate)
    e = errors_of(a, g)
    print("%s: %d of route A, %d stable, %d of the GPU; largest GPU-versus-A difference of the stable ones / bound: %s"
          % (name, len(stable), stable.sum(), len(g[0]), np.array2string(e[stable].max(axis=0) / bound, precision=3) if stable.any() else "-"))
    assert P.within(e[stable], bound).all(), "stable records of route A without a GPU partner: %s" % np.flatnonzero(stable)[~P.within(e[stable], bound)]
    lonely = ~(P.within(errors_of(g, a), bound) | P.within(errors_of(g, b), bound))
    assert lonely.sum() <= max(1, len(lonely) // 100), "GPU records without a partner in A or B: %s" % np.flatnonzero(lonely)


def as_rows(kp):
    return np.stack([kp["octave"].astype(np.float32), kp["sample"], kp["x"], kp["y"]], axis=1)


@pytest.mark.parametrize("c", range(3))
def test_against_the_reference_s2(ctx, c):
    """The three cases of sift_s2.npz under the same check.  make_golden_sift.py keeps out of them (`unconditioned`) any record
    whose orientation a float64 restatement does not reproduce: one where a pixel's gradient angle lies on the edge between
    two histogram bins, so that the last bit of a Gaussian image decides the bin and moves the peak by up to 7e-3 rad."""
    kp, xyso, desc = ctx.sift(G2["image_%d" % c], **options_of(c, G2))
    against(G2, c, as_rows(kp), xyso, desc)


@pytest.mark.parametrize("c", range(6))
def test_against_the_reference(gpu, c):
    against(G, c, *gpu[c])


def against(G, c, kp_g, xyso_g, desc_g):
    (kp_a, xyso_a, desc_a), (kp_b, xyso_b, desc_b) = [(G["kp_%s_%d" % (r, c)], G["xyso_%s_%d" % (r, c)], G["desc_%s_%d" % (r, c)]) for r in "ab"]
    gate_d = [P.STABLE_GATE[k] for k in ("pos", "scale", "ori", "desc")]
    gate_k = [P.STABLE_GATE[k] for k in ("pos", "sample")]
    check("keypoints", lambda x, y: P.keypoint_errors(x[0], y[0])[1], (kp_a,), (kp_b,), (kp_g,), gate_k, MARGIN * G["tol_kp"])
    check("descriptors", lambda x, y: P.descriptor_errors(*x, *y)[1], (xyso_a, desc_a), (xyso_b, desc_b), (xyso_g, desc_g), gate_d,
          MARGIN * G["tol_desc"])


def test_same_bytes_again_and_on_a_fork(ctx, gpu):
    c = 2                                                         # octave -1: the most keypoints, orientations and descriptors
    fork = ctx.fork()
    for other in (ctx, fork):
        kp, xyso, desc = other.sift(G["image_%d" % c], **options_of(c))
        assert len(desc) > 30 and xyso.tobytes() == gpu[c][1].tobytes() and desc.tobytes() == gpu[c][2].tobytes()
        assert np.stack([kp["octave"].astype(np.float32), kp["sample"], kp["x"], kp["y"]], axis=1).tobytes() == gpu[c][0].tobytes()
    fork.close()


def nan_pixel():
    img = G["image_0"].copy()
    img[5, 7] = np.nan
    return img


@pytest.mark.parametrize("image, options, field", [
    (lambda: G["image_0"], dict(min_octave=3, max_octave=2), "min_octave"),
    (lambda: G["image_0"], dict(min_octave=-2), "min_octave"),
    (lambda: np.zeros((20, 33, 2), np.float32), {}, "channels"),
    (nan_pixel, {}, "pixels"),
    (lambda: G["image_5"], dict(max_octave=5), "too small"),      # octave 5 of 33 x 20 has 2 x 1 pixels: "Invalid input image"
    (lambda: G["image_0"], dict(num_samples_per_octave=1, base_blur_sigma=3.2), "ks"),
], ids=["range", "below", "channels", "nan", "small", "ks"])
def test_refusals(ctx, gpu, image, options, field):
    with pytest.raises(ValueError, match=field):
        ctx.sift(image(), **options)
    kp, xyso, desc = ctx.sift(G["image_5"], **options_of(5))      # ... and the context still works
    assert xyso.tobytes() == gpu[5][1].tobytes() and len(kp) == len(gpu[5][0])
