"""RANSAC for the fundamental matrix on the GPU (mve_amd/csrc/ransac_device.hip behind mi_dmrecon_ransac_fundamental) against
a plain NumPy restatement of sfm::RansacFundamental::estimate (libs/sfm/ransac_fundamental.cc:26-105, fundamental.cc:77-126,
:224-247): np.linalg.svd for both solves, the Sampson distance in long double, the first strict maximum.  Inlier counts,
the winner and its inlier list must be EQUAL; only (hypothesis, match) pairs whose restated distance lies within a relative
1e-6 of threshold^2 are left out, and there may be at most 0.1 % of them (there are none for the seeds below)."""
import numpy as np
import pytest

from mve_amd import api

pytestmark = pytest.mark.gpu

THRESHOLD = 0.0015                                   # RansacFundamental::Options::threshold
SMALL_THRESHOLD = 0.03                               # for 8 or 9 matches (two of them outliers): nothing is an inlier at 0.0015
C, T = api.RANSAC_CHUNK, api.RANSAC_TILE


def threshold_of(n):
    return SMALL_THRESHOLD if n < 16 else THRESHOLD


# (matches, iterations): every edge of the match chunk and of the hypothesis tile, a ladder instead of the product
CASES = [(8, 1), (9, 3), (8, 4), (9, 5), (C - 1, T - 1), (C, T), (C + 1, T + 1), (2 * C + 1, 4 * T + 1), (C - 1, 4 * T + 1),
         (2 * C + 1, T - 1)]
# 1 - |cos| between the 9-vectors of two F, in long double.  Between the two float64 routes on the CPU (SVD of A; eigh of
# A^T A) its maximum over all hypotheses of CASES is 2.74e-15 (profiles/ransac_f.md); a Jacobi solve on A lies between
# the two in conditioning, and ten times that leaves room for another rotation order.
F_ANGLE_MEASURED, F_ANGLE_BOUND = 2.74e-15, 2.74e-14


def two_view(n, seed=7):
    """n matches of two cameras a baseline apart: points at depth 3-6, noise 4e-4 on the normalised coordinates, the first
    30 % of the second view's points replaced by uniform outliers."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 6.0, n)], 1)
    a = 0.12
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Y = X @ R.T + np.array([-1.0, 0.05, 0.1])
    m = np.hstack([X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]]) + rng.normal(0, 4e-4, (n, 4))
    k = int(0.3 * n)
    m[:k, 2:] = rng.uniform(-0.5, 0.5, (k, 2))
    return m


def draw(n, iterations, seed=11):
    rng = np.random.default_rng(seed)
    return np.stack([np.sort(rng.choice(n, 8, replace=False)) for _ in range(iterations)]).astype(np.int32)


def restate(m, samples, threshold=THRESHOLD, to_beat=0):
    """F (it, 3, 3), Sampson distances (it, n) in long double, counts, the winner (-1: none)."""
    x1, y1, x2, y2 = (m[samples][..., k] for k in range(4))
    A = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], -1)      # fundamental.cc:84-98
    f = np.linalg.svd(A)[2][:, 8].reshape(-1, 3, 3)
    u, s, vt = np.linalg.svd(f)
    s[:, 2] = 0.0
    F = (u * s[:, None, :]) @ vt
    L = np.longdouble
    G = F.astype(L)[:, None]                                                                       # (it, 1, 3, 3)
    p1 = np.concatenate([m[:, :2], np.ones((len(m), 1))], 1).astype(L)
    p2 = np.concatenate([m[:, 2:], np.ones((len(m), 1))], 1).astype(L)
    Fx = (G * p1[None, :, None, :]).sum(-1)                                                        # F p1: (it, n, 3)
    Ftx = (G * p2[None, :, :, None]).sum(-2)                                                       # p2^T F
    num = ((Fx * p2[None]).sum(-1)) ** 2
    d = num / (Fx[..., 0] ** 2 + Fx[..., 1] ** 2 + Ftx[..., 0] ** 2 + Ftx[..., 1] ** 2)
    counts = (d < L(threshold) ** 2).sum(1)
    best, most = -1, to_beat
    for it, c in enumerate(counts):
        if c > most:
            best, most = it, c
    return F, d, counts, best


@pytest.fixture(scope="module")
def solved(gpu_ctx):
    """case -> (matches, samples, restatement, GPU result with the per-iteration arrays), each computed once"""
    cache = {}

    def get(case):
        if case not in cache:
            m, s, thr = two_view(case[0]), draw(*case), threshold_of(case[0])
            ref = restate(m, s, thr)
            near = np.abs(ref[1] - np.longdouble(thr) ** 2) <= 1e-6 * np.longdouble(thr) ** 2
            assert near.mean() <= 1e-3, "too many distances at the threshold: change the seed, not the band"
            cache[case] = (m, s, ref, near, gpu_ctx.ransac_fundamental([(m, s, thr)], per_iteration=True)[0])
        return cache[case]
    return get


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d" % c)
def test_counts_winner_and_inliers_equal_the_restatement(solved, case, gpu_ctx):
    m, s, (F, d, counts, best), near, g = solved(case)
    clean = ~near.any(1)
    assert np.array_equal(g["counts"][clean], counts[clean])
    if clean.all():
        assert g["best_iteration"] == best >= 0
        assert np.array_equal(g["inliers"], np.flatnonzero(d[best] < np.longdouble(threshold_of(case[0])) ** 2))
    assert len(g["inliers"]) == g["counts"][g["best_iteration"]]
    assert np.array_equal(g["F"], g["F_all"][g["best_iteration"]]) and g["inliers"].dtype == np.int32
    assert gpu_ctx.ransac_sweep_capped == 0


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d" % c)
def test_F_has_rank_two_and_the_restatement_s_direction(solved, case):
    F, g = solved(case)[2][0], solved(case)[4]["F_all"]
    sv = np.linalg.svd(g, compute_uv=False)
    assert (sv[:, 2] <= 1e-12 * sv[:, 0]).all()
    a, b = F.reshape(-1, 9).astype(np.longdouble), g.reshape(-1, 9).astype(np.longdouble)
    angle = 1 - np.abs((a * b).sum(1)) / np.sqrt((a * a).sum(1) * (b * b).sum(1))
    print("max 1 - |cos|: %.3g" % angle.max())
    assert angle.max() <= F_ANGLE_BOUND


@pytest.mark.parametrize("rule", ["duplicate", "equal", "one_below"])
def test_winner_rules(solved, gpu_ctx, rule):
    m, s, (F, d, counts, best), near, g = solved((C + 1, T + 1))
    most = int(counts[best])
    if rule == "duplicate":                          # every row once more, later: the first copy of the best one keeps winning
        r = gpu_ctx.ransac_fundamental([(m, np.concatenate([s, s]), THRESHOLD)], per_iteration=True)[0]
        assert r["best_iteration"] == g["best_iteration"] and np.array_equal(r["counts"], np.tile(g["counts"], 2))
        return
    F0, inl0 = np.full((3, 3), -7.0), np.full(len(m), -7, np.int32)
    r = gpu_ctx.ransac_fundamental([(m, s, THRESHOLD, most if rule == "equal" else most - 1)], out=[(F0, inl0)])[0]
    if rule == "equal":                              # `>`, not `>=` (ransac_fundamental.cc:43): nobody wins, nothing is written
        assert r["best_iteration"] == -1 and (F0 == -7.0).all() and (inl0 == -7).all()
    else:
        assert r["best_iteration"] == g["best_iteration"] and np.array_equal(F0, g["F"])
        assert np.array_equal(inl0[:most], g["inliers"]) and (inl0[most:] == -7).all()


def test_a_batch_equals_its_single_calls_and_itself(gpu_ctx):
    jobs = [(two_view(n, seed), draw(n, it, seed + 1), threshold_of(n))
            for seed, (n, it) in enumerate([(8, 4), (2 * C + 1, 2 * T + 3), (100, 7), (C, 1), (3 * C - 5, T)])]
    batch = gpu_ctx.ransac_fundamental(jobs, per_iteration=True)
    again = gpu_ctx.ransac_fundamental(jobs, per_iteration=True)
    for job, b, a in zip(jobs, batch, again):
        single = gpu_ctx.ransac_fundamental([job], per_iteration=True)[0]
        assert b["best_iteration"] == single["best_iteration"] == a["best_iteration"]
        for k in ("F", "inliers", "counts", "F_all"):
            assert b[k].tobytes() == single[k].tobytes() == a[k].tobytes(), k


@pytest.mark.parametrize("fault", ["seven_matches", "index_out_of_range", "repeated_index"])
def test_a_bad_job_is_refused_by_name_and_nothing_runs(gpu_ctx, fault):
    m, s = two_view(40), draw(40, 6)
    bad_m, bad_s = m, s.copy()
    if fault == "seven_matches":
        bad_m, bad_s = m[:7], np.tile(np.arange(8, dtype=np.int32) % 7, (2, 1))
    elif fault == "index_out_of_range":
        bad_s[3, 7] = len(m)
    else:
        bad_s[5, 2] = bad_s[5, 6]
    F0, inl0 = np.full((3, 3), -7.0), np.full(len(m), -7, np.int32)
    out = [(F0, inl0), (np.full((3, 3), -7.0), np.full(len(m), -7, np.int32))]
    with pytest.raises(ValueError, match="job 1"):
        gpu_ctx.ransac_fundamental([(m, s, THRESHOLD), (bad_m, bad_s, THRESHOLD)], out=out)
    assert (F0 == -7.0).all() and (inl0 == -7).all()
