"""SIFT stage by stage: every kernel in front of the orientations against the float64 restatement (tests/sift_restatement.py)
of the DEVICE'S OWN input to that stage (Context.debug_sift_octave), so that errors do not chain and a wrong tap, clamp or
weight shows in the stage that has it -- and the regrow loop of mi_dmrecon_sift_run against the same call at default capacities
(Context.debug_sift_caps).

Exact bytes: dog[i] = img[i + 1] - img[i] in float32; a blur that is a copy (sigma below 0.1, or an octave whose source already
has base_blur_sigma: every octave behind the first, and the first where inherent_blur_sigma >= base_blur_sigma); the gray
image of a one-channel float image; the candidate list = the restatement's extrema of the device's DoG bytes, in order.

Bounded: gray, the double step, the half step, every blur.  The bound is arithmetic, not a measurement.  With u = 2^-24, a
float32 sum of n products v_i w_i (each product rounded once, or fused into the addition and not rounded at all), added in
any order (each partial sum rounded once: a term passes through at most n - 1 additions), then divided once by wsum, differs
from the exact quotient by at most ((1 + u)^(n + 1) - 1) sum |v_i| w_i / wsum, which is below (n + 2) u sum |v_i| w_i / wsum for
every n here (n <= 65; the second-order terms are below n^2 u^2 < u).  The restatement divides by the same float32 wsum and
uses the same float32 weights, so nothing else differs.  The zero weights behind the 2 ks + 1 taps add exact zeros.
  gray    n = 3 products by float32(1/3) (a u8 value is divided by 255 first: one more rounding, inside the "+ 2"); n = 1 for u8 gray
  double  n = 4, no division       half  n = 16
  blur    two passes of n = 2 ks + 1.  The row pass leaves e1 <= (n + 2) u R|v| (R, C: the exact row and column operators, both
          positive); the column pass adds (n + 2) u C|R v + e1| <= (n + 2) u C(R|v| + e1) to C e1.  Together at most
          (n + 2) u (2 + (n + 2) u) C R |v|, the restated blur of |v|.
A tap shifted by one pixel, or a clamp to the wrong column, changes a pixel by a fraction of the local gradient, 1e-3 ... 1e-1
on these images: four to five orders of magnitude above the bound (6e-8 ... 8e-6 of a pixel value).

Localization: loc against the restatement run on the device's DoG bytes.  A candidate is DECISIVE if in float64 no compared
quantity lies within 1e-3 of its threshold (sift_restatement.localize).  Decisive candidates agree in `kept`, and kept ones
in x, y and sample within loc_bound of tests/golden/sift_s2.npz: 8 x the largest difference between the reference's two
builds (make_golden_sift.py; the 8 of test_sift.py), a bound from the reference, not from the device.  At least 90 % of the
candidates of every case are decisive; test_decisive_share_on_the_cpu checks that without a GPU on a float64 scale space.

The shapes are the smallest that reach the paths: widths around the row blur's tile of 256 (255, 256, 257, 261, 513: a seam,
a tile of one pixel, two seams), heights around the column tile of 32 and the extrema tile of 16 (31, 32, 33, 65), widths
around the extrema tile of 64 (63, 64, 65, 129), an octave smaller than its blurs (5 x 3 under ks = 4 ... 9), S = 1 (ks = 32, 65
taps; its descriptor windows reach 79 rows, two strides of 64 lanes -- a third stride needs a sample above 0.915, which a
parabola through an extremum of three DoG images does not give), S = 6 (the shortest kernels), octave -1 of 131 x 35, u8 RGB, and word counts on both sides of
k_sift_scan's 1024 lanes (S h ceil(w / 64): 1050 for 262 x 70, 1170 for 129 x 65 at S = 6; below it elsewhere)."""
import os
import sys

import numpy as np
import pytest

import sift_restatement as R
from mve_amd import api

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_sift import blobs  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G1, G2 = np.load(os.path.join(GOLDEN, "sift_s1.npz")), np.load(os.path.join(GOLDEN, "sift_s2.npz"))
U = 2.0 ** -24


def rgb_u8(g):
    return np.clip(np.stack([g * 1.05, g, g * 0.92], axis=2) * 255.0 + 0.5, 0, 255).astype(np.uint8)


def rgb_f32(g):
    return np.stack([g * 0.9, g, g * 0.8], axis=2).astype(np.float32)


# name: (image, options).  blobs(w, h, blobs, small central ones, seed)
CASES = {
    "255x31": (lambda: blobs(255, 31, 40, 0, 701), dict(max_octave=1)),
    "256x32": (lambda: blobs(256, 32, 40, 0, 702), dict(max_octave=1)),
    "257x33_u8_rgb": (lambda: rgb_u8(blobs(257, 33, 40, 0, 703)), dict(max_octave=1)),
    "261x65": (lambda: blobs(261, 65, 60, 30, 704), dict(max_octave=2)),
    "513x33": (lambda: blobs(513, 33, 80, 0, 705), dict(max_octave=1)),
    "63x33": (lambda: blobs(63, 33, 12, 0, 706), dict(max_octave=0)),
    "64x31_u8": (lambda: (blobs(64, 31, 12, 0, 707) * 255.0 + 0.5).astype(np.uint8), dict(max_octave=0)),
    "65x32_f32_rgb": (lambda: rgb_f32(blobs(65, 32, 12, 0, 708)), dict(max_octave=0)),
    "129x65_min1": (lambda: blobs(129, 65, 30, 10, 709), dict(min_octave=1, max_octave=2)),
    "129x65_S6": (lambda: blobs(129, 65, 30, 10, 710), dict(num_samples_per_octave=6, max_octave=0)),
    "33x20_to_5x3": (lambda: G1["image_5"], dict(max_octave=3)),
    "261x141_S1": (lambda: G2["image_0"], dict(num_samples_per_octave=1, max_octave=1)),
    "131x35_octave-1": (lambda: G2["image_2"], dict(min_octave=-1, max_octave=1)),
    "64x32_copy": (lambda: blobs(64, 32, 12, 0, 711), dict(max_octave=0, inherent_blur_sigma=2.0)),
}
NAMES = list(CASES)
gpu = pytest.mark.gpu


def options_of(name):
    return dict(api.SIFT_DEFAULTS, **CASES[name][1])


def contrast_of(o):
    c = np.float32(o["contrast_threshold"])
    return float(c) if c >= 0 else float(np.float32(0.02) / np.float32(o["num_samples_per_octave"]))


@pytest.mark.parametrize("name", NAMES)
def test_decisive_share_on_the_cpu(name):
    """The condition under which the localization test says anything: on a float64 scale space of the case, at least 90 %
    of the extrema are decisive.  (Change the image, not the share, if a case falls short.)"""
    o = options_of(name)
    n = n_dec = 0
    for _, _, dog in R.scale_space(CASES[name][0](), o):
        cand = R.extrema(dog)
        _, dec = R.localize(dog, cand, o["num_samples_per_octave"], contrast_of(o), o["edge_ratio_threshold"])
        n, n_dec = n + len(dec), n_dec + int(dec.sum())
    print("%s: %d of %d extrema decisive (%.1f %%)" % (name, n_dec, n, 100.0 * n_dec / max(n, 1)))
    assert n >= 1 and n_dec >= 0.9 * n


@pytest.mark.parametrize("c", range(3))
def test_restatement_against_the_reference(c):
    """The restatement's own check, without a GPU: its extrema and localization on a float64 scale space of the cases of
    sift_s2 give the keypoints the reference's route B recorded, within the largest A-versus-B difference (tol_kp); both ways,
    but for the restatement's indecisive candidates, which either side may keep or drop."""
    import sift_pairing as P
    o = {k: (int(v) if k in ("num_samples_per_octave", "min_octave", "max_octave") else float(v))
         for k, v in zip(api.SIFT_DEFAULTS, G2["options_%d" % c])}
    rows, sure = [], []
    for octave, _, dog in R.scale_space(G2["image_%d" % c], o):
        loc, dec = R.localize(dog, R.extrema(dog), o["num_samples_per_octave"], contrast_of(o), o["edge_ratio_threshold"])
        kept = loc[:, 3] != 0
        rows.append(np.column_stack([np.full(kept.sum(), octave), loc[kept, 2], loc[kept, 0], loc[kept, 1]]))
        sure.append(dec[kept])
    mine, sure, ref = np.concatenate(rows), np.concatenate(sure), G2["kp_b_%d" % c].astype(np.float64)
    e_mine, e_ref = P.keypoint_errors(mine, ref)[1], P.keypoint_errors(ref, mine)[1]
    print("case %d: %d restated keypoints (%d decisive), %d of route B; largest difference / tol_kp %s"
          % (c, len(mine), sure.sum(), len(ref), np.array2string(e_ref[P.within(e_ref, [1, 1])].max(axis=0) / G2["tol_kp"], precision=3)))
    assert len(ref) >= 30 and P.within(e_mine[sure], G2["tol_kp"]).all()
    assert (~P.within(e_ref, G2["tol_kp"])).sum() <= (~sure).sum()


@pytest.mark.parametrize("c", range(3))
def test_restated_orientations_against_the_reference(c):
    """sift_restatement.orientations, which make_golden_sift.py filters its images with, without a GPU: on a float64 scale space
    it gives every orientation route B recorded for sift_s2, within the 8 x tol_desc that test_sift.py allows the device."""
    from make_golden_sift import unconditioned
    o = {k: (int(v) if k in ("num_samples_per_octave", "min_octave", "max_octave") else float(v))
         for k, v in zip(api.SIFT_DEFAULTS, G2["options_%d" % c])}
    xyso = G2["xyso_b_%d" % c]
    assert len(xyso) >= 10 and unconditioned(G2["image_%d" % c], o, G2["kp_b_%d" % c], xyso, 8.0 * G2["tol_desc"][2]) == []


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


_octaves = {}


@pytest.fixture
def octaves(ctx):
    """name -> (image, options, [the hook's record of every plan slot]); every case runs once."""
    def get(name):
        if name not in _octaves:
            image, o = CASES[name][0](), options_of(name)
            n_slots = len(R.octave_plan(image.shape[1], image.shape[0], o))
            _octaves[name] = (image, o, [ctx.debug_sift_octave(image, k, **CASES[name][1]) for k in range(n_slots)])
        return _octaves[name]
    return get


def ratio(got, want, bound):
    """largest |got - want| / bound; a bound of zero (a pixel sum of zeros) wants the exact value"""
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_plan_and_taps(octaves, name):
    """The host's plan: octave sizes, radii and taps are the restatement's, bit for bit where float32 says so (the weights may
    differ in their last bit: exp is the C library's in the one and float64's, rounded, in the other)."""
    image, o, recs = octaves(name)
    plan = R.octave_plan(image.shape[1], image.shape[0], o)
    assert len(plan) == len(recs)
    for (_, w, h, sig), r in zip(plan, recs):
        assert (r["w"], r["h"]) == (w, h) and r["img"].shape == (o["num_samples_per_octave"] + 3, h, w)
        for i, s in enumerate(sig):
            ks, wsum, taps = (0, 0.0, np.zeros(0)) if s is None else R.make_taps(s)
            assert r["ks"][i] == ks and ks <= 32
            got = r["taps"][i]
            assert np.all(got[2 * ks + 1 if ks else 0:] == 0) and np.array_equal(got[:2 * ks + 1], got[:2 * ks + 1][::-1])
            if ks:
                assert np.allclose(got[:2 * ks + 1], taps, rtol=2.0 ** -22, atol=0) and abs(r["wsum"][i] - wsum) <= (2 * ks + 3) * 2.0 ** -23 * wsum
                tot = np.float32(0)
                for t in got[:2 * ks + 1]:
                    tot = np.float32(tot + t)
                assert tot == r["wsum"][i]
    if name == "261x141_S1":
        assert recs[0]["ks"].max() == 32
    if name == "33x20_to_5x3":
        assert (recs[3]["w"], recs[3]["h"]) == (5, 3) and recs[3]["ks"][1:].min() > 3 and recs[3]["ks"].max() > 5      # radii beyond the image


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_gray_double_half(octaves, name):
    image, o, recs = octaves(name)
    plan = R.octave_plan(image.shape[1], image.shape[0], o)
    g = recs[0]["gray"]
    out = []
    if image.dtype == np.float32 and image.ndim == 2:
        assert g.tobytes() == image.tobytes()
    else:
        n = 3 if image.ndim == 3 else 1
        v = image.astype(np.float64) / (255.0 if image.dtype == np.uint8 else 1.0)
        bound = (n + 2) * U * (np.abs(v).sum(axis=2) * float(np.float32(1) / np.float32(3)) if n == 3 else np.abs(v))
        out.append(("gray", ratio(g, R.gray(image), bound)))
    src, at = g, 0                                                 # the image the next octave's source is halved from, and its slot
    for k, ((octave, w, h, _), r) in enumerate(zip(plan, recs)):
        if octave < 0:
            out.append(("double", ratio(r["src"], R.double_size(g), 6 * U * R.double_size(np.abs(g)))))
            continue
        want, bound_of, steps = src.astype(np.float64), np.abs(src.astype(np.float64)), 0
        while want.shape != (h, w):                                # (more than one step only in front of the first octave: min_octave > 0)
            want, bound_of, steps = R.half_size(want), R.half_size(bound_of), steps + 1
        if steps == 0:
            assert r["src"].tobytes() == src.tobytes()
        elif steps == 1:
            out.append(("half %d" % k, ratio(r["src"], want, 18 * U * bound_of)))
        else:                                                      # the steps in between are not downloaded: every one within its bound of the one before
            out.append(("half x%d %d" % (steps, k), ratio(r["src"], want, steps * 18 * U * (1 + 18 * U) ** steps * bound_of)))
        src = r["src"]
    print("%s: largest error / bound: %s" % (name, ", ".join("%s %.3f" % p for p in out)))
    assert all(p[1] <= 1.0 for p in out), out


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_blurs_and_dog(octaves, name):
    image, o, recs = octaves(name)
    out, copies = [], 0
    for k, r in enumerate(recs):
        for i in range(len(r["ks"])):
            inp = r["src"] if i == 0 else r["img"][i - 1]
            ks, wsum, taps = int(r["ks"][i]), float(r["wsum"][i]), r["taps"][i].astype(np.float64)
            if ks == 0:
                assert r["img"][i].tobytes() == inp.tobytes()
                copies += 1
            else:
                n = 2 * ks + 1
                bound = (n + 2) * U * (2 + (n + 2) * U) * R.blur(np.abs(inp), ks, wsum, taps)
                out.append(("%d.%d" % (k, i), ratio(r["img"][i], R.blur(inp, ks, wsum, taps), bound)))
        assert r["dog"].tobytes() == (r["img"][1:] - r["img"][:-1]).astype(np.float32).tobytes()
    print("%s: %d copies; blur slot.index largest error / bound: %s" % (name, copies, ", ".join("%s %.3f" % p for p in out)))
    assert all(p[1] <= 1.0 for p in out), out
    if name == "64x32_copy" or len(recs) > 1:
        assert copies >= 1


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_candidates_are_the_extrema_of_the_dog_bytes(octaves, name):
    image, o, recs = octaves(name)
    total = 0
    for r in recs:
        want = R.extrema(r["dog"])
        assert r["n_cand"] == len(want) and np.array_equal(r["cand"], want)
        total += len(want)
    assert total >= 1
    S = o["num_samples_per_octave"]
    words = [S * r["h"] * ((r["w"] + 63) // 64) for r in recs]
    if name in ("131x35_octave-1", "129x65_S6"):
        assert max(words) > 1024
    if name == "513x33":
        assert max(words) < 1024


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_localization(octaves, name):
    image, o, recs = octaves(name)
    n = n_dec = n_kept = 0
    worst = np.zeros(2)
    for r in recs:
        want, dec = R.localize(r["dog"], r["cand"], o["num_samples_per_octave"], contrast_of(o), o["edge_ratio_threshold"])
        got = r["loc"].astype(np.float64)
        assert np.array_equal(got[dec, 3], want[dec, 3]), "kept differs at candidates %s" % np.flatnonzero(dec & (got[:, 3] != want[:, 3]))
        both = dec & (want[:, 3] != 0)
        if both.any():
            d = np.abs(got[both, :3] - want[both, :3])
            worst = np.maximum(worst, [d[:, :2].max(), d[:, 2].max()])
        n, n_dec, n_kept = n + len(dec), n_dec + int(dec.sum()), n_kept + int(both.sum())
    print("%s: %d candidates, %d decisive (%.1f %%), %d of them kept; largest position, sample difference / bound: %s"
          % (name, n, n_dec, 100.0 * n_dec / max(n, 1), n_kept, np.array2string(worst / G2["loc_bound"], precision=4)))
    assert n_dec >= 0.9 * n and np.all(worst <= G2["loc_bound"])


# ---- the regrow loop

REGROW_IMAGE, REGROW_OPTIONS = G1["image_2"], dict(min_octave=-1, max_octave=2)       # octave -1 to 2 of 97 x 71: the most of everything


def as_bytes(result):
    kp, xyso, desc = result
    return kp.tobytes(), xyso.tobytes(), desc.tobytes()


@pytest.fixture(scope="module")
def regrow_default(ctx):
    """(the bytes at default capacities, the exact counts: extrema of the fullest octave, keypoints, descriptors)"""
    kp, xyso, desc = ctx.sift(REGROW_IMAGE, **REGROW_OPTIONS)
    assert ctx.debug_sift_caps() == 1                              # nothing overflowed
    n_cand = max(ctx.debug_sift_octave(REGROW_IMAGE, k, **REGROW_OPTIONS)["n_cand"] for k in range(4))
    assert len(desc) > 30 and len(set(kp["octave"])) > 1
    return as_bytes((kp, xyso, desc)), (n_cand, len(kp), len(desc))


@gpu
@pytest.mark.parametrize("setting", ["ones", "exact", "minus_one", "desc_short", "cand_short"])
def test_regrown_lists_give_the_same_bytes(regrow_default, setting):
    want, (n_cand, n_kp, n_desc) = regrow_default
    caps = dict(ones=(1, 1, 1), exact=(n_cand, n_kp, n_desc), minus_one=(n_cand - 1, n_kp - 1, n_desc - 1), desc_short=(0, 0, n_desc // 2),
                cand_short=(n_cand // 2, 0, 0))[setting]
    c = api.Context(0)
    try:
        assert c.debug_sift_caps(*caps) == 0                       # no run on this context yet
        got = as_bytes(c.sift(REGROW_IMAGE, **REGROW_OPTIONS))
        attempts = c.debug_sift_caps(*caps)                        # ... and short again for the second image
        print("%s: capacities %s, %d runs through the kernels" % (setting, caps, attempts))
        assert got == want
        assert attempts == 1 if setting == "exact" else 2 <= attempts <= 8
        # a context whose lists were regrown, and are short once more, on another image: the bytes of a context that never regrew
        other = G1["image_0"]
        fresh = api.Context(0)
        try:
            assert as_bytes(c.sift(other)) == as_bytes(fresh.sift(other)) and fresh.debug_sift_caps() == 1
        finally:
            fresh.close()
        # ... and with the lists it grew then, the first image again
        assert as_bytes(c.sift(REGROW_IMAGE, **REGROW_OPTIONS)) == want
    finally:
        c.close()


@gpu
@pytest.mark.parametrize("short", ["cand", "kp", "desc"])
def test_a_short_list_leaves_the_memory_behind_it_alone(ctx, regrow_default, short):
    """The writes that k_sift_emit (cand_cap), k_sift_compact (kp_cap) and k_sift_describe (desc_cap) drop.  The final bytes of a
    regrown run cannot show a missing guard: the last attempt overwrites everything.  So ONE pass through the kernels
    (the octave hook runs one) on a context whose lists are allocated at their default length, hold another image's
    entries, and have one capacity set one below what the image needs: in front of the capacity the list holds the image's
    entries, and from the capacity on, every byte is still the other image's -- also the entry the dropped write would have
    gone to, which the same pass at the default capacity does change."""
    _, (_, n_kp, n_desc) = regrow_default
    slot = 0 if short == "cand" else 3                             # the fullest octave for its extrema; all four for the other two
    key = dict(cand="raw_cand", kp="raw_kp", desc="raw_xyso")[short]
    room = 2 * max(n_kp, n_desc, 2 ** 10)
    full = ctx.debug_sift_octave(REGROW_IMAGE, slot, raw_room=room, **REGROW_OPTIONS)
    n = dict(cand=full["n_cand"], kp=n_kp, desc=n_desc)[short]
    assert 8 < n < room
    other = blobs(97, 71, 80, 40, 712)
    c = api.Context(0)
    try:
        kp, xyso, _ = c.sift(other, **REGROW_OPTIONS)              # allocates the lists at their default length
        before = c.debug_sift_octave(other, slot, raw_room=room, **REGROW_OPTIONS)
        assert dict(cand=before["n_cand"], kp=len(kp), desc=len(xyso))[short] >= n
        c.debug_sift_caps(**{short: n - 1})
        after = c.debug_sift_octave(REGROW_IMAGE, slot, raw_room=room, **REGROW_OPTIONS)
    finally:
        c.close()
    assert after["n_cand"] == full["n_cand"]                       # counted in full, whatever was dropped
    assert after[key][:n - 1].tobytes() == full[key][:n - 1].tobytes()
    assert after[key][n - 1:].tobytes() == before[key][n - 1:].tobytes()
    assert full[key][n - 1].tobytes() != before[key][n - 1].tobytes()


@gpu
def test_caps_hook_refuses_negative_values(ctx):
    for caps in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        with pytest.raises(ValueError, match="negative"):
            ctx.debug_sift_caps(*caps)
