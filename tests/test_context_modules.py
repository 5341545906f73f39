"""What the modules behind a context keep between calls: the buffers of the RANSAC, SIFT, SURF and BA entry points (one state
per module and context, deleted with the context), and those of a Matcher and an FssrSampler.  A buffer that was regrown, reused
or handed back wrongly shows as a result that differs from the same call on a context of its own, so every comparison here
is bit for bit and within one build: no tolerance."""
import numpy as np
import pytest

import test_ba as TB
import test_fssr as TF
import test_match as TM
import test_ransac as TR
import test_ransac_hp as TH
import test_sift as TSI
import test_surf as TSU
from mve_amd import api

pytestmark = pytest.mark.gpu


def same(a, b):
    """a and b, nested lists / tuples / dicts of arrays and numbers, are equal to the bit (NaN included)"""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def on_a_fresh_context(call):
    c = api.Context(0)
    try:
        return call(c)
    finally:
        c.close()


# ---- the calls: each takes a context and returns everything the call hands back ----------------------------------------

def ransac_calls(model):
    """small: one job of exactly the shortest list the model takes and one iteration; large: three jobs of about 300 entries
    and 64 iterations with the per-iteration outputs (the download then takes the hypotheses too)."""
    def jobs(sizes, iterations):
        if model == "f":
            return [(TR.two_view(n, seed), TR.draw(n, iterations, seed + 1), TR.threshold_of(n)) for seed, n in enumerate(sizes)]
        if model == "h":
            return [(TH.planar(n, seed), TH.draw(n, iterations, 4, seed + 1), TH.THRESHOLD) for seed, n in enumerate(sizes)]
        return [(TH.scene(n, seed), TH.K, TH.draw(n, iterations, 3, seed + 1), TH.THRESHOLD) for seed, n in enumerate(sizes)]
    method = dict(f="ransac_fundamental", h="ransac_homography", p3p="ransac_pose_p3p")[model]
    shortest = dict(f=8, h=4, p3p=3)[model]

    def call(js, per_iteration):
        return lambda c: (getattr(c, method)(js, per_iteration=per_iteration), c.ransac_sweep_capped)
    return call(jobs([shortest], 1), False), call(jobs([299, 300, 301], 64), True)


def structured(w, h, seed):
    return TSU.blobs(w, h, seed, [2, 3, 5, 8], 60)


def sift_calls():
    """small: the 33 x 20 image of the fixture (four keypoints); large: 160 x 120 from octave -1.  The result lists start at
    2^16 keypoints and descriptors and 2^18 candidates per octave, more than an image of this size has pixels, so they cannot
    be made to grow here: what regrows between the calls are the image, pyramid and mask buffers."""
    large = structured(160, 120, 21)
    return (lambda c: c.sift(TSI.G["image_5"], **TSI.options_of(5))), (lambda c: c.sift(large, min_octave=-1))


def surf_calls():
    """small: 131 x 97, the smallest image of test_surf.py that has keypoints; large: 160 x 120.  The keypoint list starts at
    2^15 entries, more than the large image has pixels: as for SIFT, the image, table and map buffers are what regrows."""
    small, large = TSU.blobs(131, 97, 1, [2, 3, 4, 6], 40), structured(160, 120, 22)
    return (lambda c: c.surf(small)), (lambda c: c.surf(large))


def ba_calls(golden):
    """small: 2 cameras, 4 points, 8 observations; large: the case of tests/golden/ba_b1.npz with the most observations"""
    small = TB.R.make_scene(2, [[0, 1]] * 4, 31)
    _, large, mode, fixed = max(TB.fixture_cases(golden), key=lambda case: len(case[1]["cam"]))
    return (lambda c: c.bundle_adjust(*TB.records(small), lm_max_iterations=5)), \
           (lambda c: c.bundle_adjust(*TB.records(large), bundle_mode=mode, fixed_intrinsics=fixed))


def matcher_calls():
    """One matcher per context; a job of 1 x 1 descriptors, then one of 300 x 400"""
    a, b = TM.planted(np.random.default_rng(41), 300, 400, TM.R.SIFT)

    def opened(c):
        m = c.match_open(2)
        m.set(0, TM.R.SIFT, a)
        m.set(1, TM.R.SIFT, b)
        return m
    return opened, (lambda m: m.pairs(TM.R.SIFT, [(0, 1, 1, 1)], *TM.DEFAULT[TM.R.SIFT])), \
        (lambda m: m.pairs(TM.R.SIFT, [(0, 300, 1, 400)], *TM.DEFAULT[TM.R.SIFT]))


def sampler_calls(f1):
    """One sampler of fixture F1 per context; 1 voxel, then 5000"""
    return (lambda c: TF.open_tree(c, f1)), (lambda s: s.sample(f1["positions"][:1])), (lambda s: s.sample(f1["positions"][:5000]))


@pytest.fixture(scope="module")
def golden_ba():
    return np.load(TB.os.path.join(TB.HERE, "golden", "ba_b1.npz"))


@pytest.fixture(scope="module")
def f1():
    return dict(np.load(TF.os.path.join(TF.GOLDEN, "fssr_f1.npz")))


# ---- 1 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("module", ["ransac_f", "ransac_h", "ransac_p3p", "sift", "surf", "ba", "matcher", "sampler"])
def test_small_large_small_on_one_context(module, golden_ba, f1):
    """A small call, a large one and the small one again on ONE context (for the Matcher, whose sequential calls take the same
    slot, and the FssrSampler: on one handle): the buffers grow once and are then larger than the call needs.  Each result is
    the one of the same call on a context of its own (for RANSAC with the count of capped Jacobi sweeps, which the context
    carries from call to call)."""
    opened = None
    if module.startswith("ransac"):
        small, large = ransac_calls(module[7:])
    elif module in ("matcher", "sampler"):
        opened, small, large = matcher_calls() if module == "matcher" else sampler_calls(f1)
    else:
        small, large = dict(sift=sift_calls, surf=surf_calls, ba=lambda: ba_calls(golden_ba))[module]()

    def run(calls):
        """the calls in turn on one new context (and one new handle on it)"""
        c = api.Context(0)
        h = opened(c) if opened else c
        try:
            return [call(h) for call in calls]
        finally:
            if opened:
                h.close()
            c.close()
    alone = run([small]) + run([large])
    assert not same(alone[0], alone[1]), "the two calls must differ for this test to see anything"
    for k, (got, want) in enumerate(zip(run([small, large, small]), [alone[0], alone[1], alone[0]])):
        assert same(got, want), "%s: call %d on the shared context differs from the same call alone" % (module, k)


# ---- 2 -----------------------------------------------------------------------------------------------------------------

def test_every_module_on_one_context_and_an_orderly_teardown(golden_ba, f1):
    """A context and a fork of it run all four per-context modules; a Matcher and an FssrSampler live on the parent.  Sampler,
    matcher, fork and parent are closed in that order (each module's state goes with its context), and a new context then
    gives the parent's four results again."""
    calls = [ransac_calls("f")[1], sift_calls()[1], surf_calls()[0], ba_calls(golden_ba)[1]]
    open_matcher, _, match = matcher_calls()
    open_sampler, _, sample = sampler_calls(f1)
    parent = api.Context(0)
    fork = parent.fork()
    matcher, sampler = open_matcher(parent), open_sampler(parent)
    try:
        first = [call(parent) for call in calls]
        forked = [call(fork) for call in calls]
        matched, sampled = match(matcher), sample(sampler)
        assert len(matched[0][0]) == 300 and len(sampled["value"]) == 5000
    finally:
        sampler.close()
        matcher.close()
        fork.close()
        parent.close()
    assert same(first, forked)
    assert same(on_a_fresh_context(lambda c: [call(c) for call in calls]), first)


# ---- 3 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per_iteration", [False, True])
@pytest.mark.parametrize("with_out", [False, True])
def test_ransac_fundamental_keeps_its_contract(gpu_ctx, per_iteration, with_out):
    """Context.ransac_fundamental through the call it shares with its two siblings: the keys, dtypes and shapes of what it
    returns, the caller's ``out`` written into, and a job without a winner that leaves ``out`` alone (NaN and an empty array
    without ``out``).  The job is the smallest case of test_ransac.py."""
    n, it = TR.CASES[0]
    m, s, thr = TR.two_view(n), TR.draw(n, it), TR.threshold_of(n)

    def outs():
        return [(np.full((3, 3), -7.0), np.full(n, -7, np.int32))] if with_out else None
    out = outs()
    r = gpu_ctx.ransac_fundamental([(m, s, thr)], per_iteration=per_iteration, out=out)
    assert len(r) == 1
    r = r[0]
    assert sorted(r) == sorted(["best_iteration", "F", "inliers"] + (["counts", "F_all"] if per_iteration else []))
    assert isinstance(r["best_iteration"], int) and -1 <= r["best_iteration"] < it
    assert r["F"].dtype == np.float64 and r["F"].shape == (3, 3)
    assert r["inliers"].dtype == np.int32 and r["inliers"].ndim == 1 and len(r["inliers"]) <= n
    if per_iteration:
        assert r["counts"].dtype == np.int32 and r["counts"].shape == (it,)
        assert r["F_all"].dtype == np.float64 and r["F_all"].shape == (it, 3, 3)
        if r["best_iteration"] >= 0:
            assert np.array_equal(r["F"], r["F_all"][r["best_iteration"]]) and len(r["inliers"]) == r["counts"][r["best_iteration"]]
    if with_out:
        assert r["F"] is out[0][0] and (len(r["inliers"]) == 0 or np.shares_memory(r["inliers"], out[0][1]))
    plain = gpu_ctx.ransac_fundamental([(m, s, thr)])[0]          # the same job, no `out`, no per-iteration outputs
    assert plain["best_iteration"] == r["best_iteration"] and same(plain["inliers"], r["inliers"])
    assert r["best_iteration"] < 0 or same(plain["F"], r["F"])
    # nobody has more than n inliers out of n matches: no winner
    out = outs()
    r = gpu_ctx.ransac_fundamental([(m, s, thr, n)], per_iteration=per_iteration, out=out)[0]
    assert r["best_iteration"] == -1 and len(r["inliers"]) == 0 and r["inliers"].dtype == np.int32
    if with_out:
        assert (out[0][0] == -7.0).all() and (out[0][1] == -7).all() and r["F"] is out[0][0]
    else:
        assert np.isnan(r["F"]).all() and r["F"].shape == (3, 3)
    if per_iteration:                                            # ... and the per-iteration outputs are filled all the same
        assert r["counts"].shape == (it,) and r["F_all"].shape == (it, 3, 3) and np.isfinite(r["F_all"]).all()
