"""RANSAC for the homography and for the P3P pose on the GPU (mve_amd/csrc/ransac_device.hip behind
mi_dmrecon_ransac_homography and mi_dmrecon_ransac_pose_three_point) against a plain NumPy restatement of
sfm::RansacHomography::estimate (libs/sfm/ransac_homography.cc, homography.cc: np.linalg.svd, np.linalg.inv) and of
sfm::RansacPoseP3P::estimate (ransac_pose_p3p.cc, pose_p3p.cc: Kneip's formulas in complex128), both inlier tests in long
double, the first strict maximum.  Counts, the winner and its inlier list must be EQUAL; only (hypothesis, entry) pairs whose
restated error lies within a relative 1e-6 of threshold^2 are left out, and there may be at most 0.1 % of them."""
import numpy as np
import pytest

from mve_amd import api

pytestmark = pytest.mark.gpu

L = np.longdouble
THRESHOLD = 0.005                                    # Options::threshold of both classes
C, T = api.RANSAC_CHUNK, api.RANSAC_TILE
# (entries, iterations): every edge of the list chunk and of the hypothesis tile (four hypotheses per P3P iteration)
CASES = {"h": [(4, 1), (5, 3), (C - 1, T - 1), (C, T), (C + 1, T + 1), (2 * C + 1, 4 * T + 1)],
         "p3p": [(3, 1), (4, 3), (C - 1, T // 4 - 1), (C, T // 4), (C + 1, T // 4 + 1), (2 * C + 1, T + 1)]}
ALL = [(m, c) for m in CASES for c in CASES[m]]
IDS = ["%s-%dx%d" % (m, *c) for m, c in ALL]
# What two CPU routes differ by over all hypotheses of CASES (profiles/ransac_hp.md), times ten for another rotation order
# and the device's cbrt / atan2, as test_ransac.py argues.  H: 1 - |cos| of the 9-vectors, SVD of A against eigh of A^T A.
# Pose: the largest absolute difference of an element, the complex128 restatement against the same in clongdouble.
H_ANGLE_MEASURED, H_ANGLE_BOUND = 1.18e-15, 1.18e-14
POSE_MEASURED, POSE_BOUND = 6.39e-06, 6.39e-05


def planar(n, seed=7):
    """two_view's cameras over the near-plane z = 4 + 0.15 x: noise 4e-4, the first 30 % of the second view's points uniform"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), np.full(n, 4.0)], 1)
    X[:, 2] += 0.15 * X[:, 0]
    a = 0.12
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Y = X @ R.T + np.array([-1.0, 0.05, 0.1])
    m = np.hstack([X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]]) + rng.normal(0, 4e-4, (n, 4))
    k = int(0.3 * n)
    m[:k, 2:] = rng.uniform(-0.5, 0.5, (k, 2))
    return m


K = np.diag([0.9, 0.9, 1.0])


def scene(n, seed=7):
    """n rows X Y Z u v: points at depth 3-6 seen by a camera turned 0.2 rad about y at t = (-0.4, 0.1, 0.3) with K; noise
    4e-4, the first 30 % of the 2D points uniform in +-0.4"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 6.0, n)], 1)
    a = 0.2
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Y = (X @ R.T + np.array([-0.4, 0.1, 0.3])) @ K.T
    u = Y[:, :2] / Y[:, 2:] + rng.normal(0, 4e-4, (n, 2))
    k = int(0.3 * n)
    u[:k] = rng.uniform(-0.4, 0.4, (k, 2))
    return np.hstack([X, u])


def draw(n, iterations, width, seed=11):
    rng = np.random.default_rng(seed)
    return np.stack([np.sort(rng.choice(n, width, replace=False)) for _ in range(iterations)]).astype(np.int32)


def dlt(m, samples):
    """the 8 x 9 systems of homography_dlt (homography.cc:26-51): (it, 8, 9)"""
    x1, y1, x2, y2 = (m[samples][..., k] for k in range(4))
    z, o = np.zeros_like(x1), np.ones_like(x1)
    return np.concatenate([np.stack([z, z, z, x1, y1, o, -x1 * y2, -y1 * y2, -y2], -1),
                           np.stack([-x1, -y1, -o, z, z, z, x1 * x2, y1 * x2, x2], -1)], 1)


def homographies(m, samples):
    h = np.linalg.svd(dlt(m, samples))[2][:, 8]
    return (h / h[:, 8:]).reshape(-1, 3, 3)                                          # ransac_homography.cc:82


def transfer_errors(H, m):
    """symmetric_transfer_error (homography.cc:65-88) of every (hypothesis, match) in long double"""
    p1 = np.concatenate([m[:, :2], np.ones((len(m), 1))], 1).astype(L)
    p2 = np.concatenate([m[:, 2:], np.ones((len(m), 1))], 1).astype(L)
    a = np.einsum("hij,nj->hni", np.linalg.inv(H).astype(L), p2)
    b = np.einsum("hij,nj->hni", H.astype(L), p1)
    return 0.5 * (((p1[None, :, :2] - a[..., :2] / a[..., 2:]) ** 2).sum(-1) + ((b[..., :2] / b[..., 2:] - p2[None, :, :2]) ** 2).sum(-1))


def unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def kneip(corr, samples, real=np.float64):
    """pose_p3p_kneip (pose_p3p.cc:74-236) of every row of samples: (it, 4, 3, 4), NaN where there is no pose.  ``real``:
    the precision of every step (np.longdouble measures what complex128 loses, profiles/ransac_hp.md)."""
    cplx = np.complex128 if real is np.float64 else np.clongdouble
    c, third = corr.astype(real), real(1) / real(3)
    p1, p2, p3 = (c[samples[:, j], :3] for j in range(3))
    Ki = (1 / np.diag(K)).astype(real)
    f1, f2, f3 = (np.concatenate([c[samples[:, j], 3:], np.ones((len(samples), 1), real)], 1) * Ki for j in range(3))
    collinear = (np.cross(p2 - p1, p3 - p1) ** 2).sum(1) < 1e-10                      # :80-85
    f1, f2, f3 = (np.where(np.abs((f * f).sum(1, keepdims=True) - 1) <= 1e-10, f, unit(f)) for f in (f1, f2, f3))

    def frame(a, b):
        e3 = unit(np.cross(a, b))
        return np.stack([a, np.cross(e3, a), e3], 1)
    swap = ((frame(f1, f2)[:, 2] * f3).sum(1) > 0)[:, None]                           # :107-119
    p1, p2, f1, f2 = np.where(swap, p2, p1), np.where(swap, p1, p2), np.where(swap, f2, f1), np.where(swap, f1, f2)
    Tm = frame(f1, f2)
    f3 = np.einsum("hij,hj->hi", Tm, f3)
    n1 = unit(p2 - p1)
    n3 = unit(np.cross(n1, p3 - p1))
    N = np.stack([n1, np.cross(n3, n1), n3], 1)
    q3 = np.einsum("hij,hj->hi", N, p3 - p1)
    d12, F1, F2, P1, P2 = np.sqrt(((p2 - p1) ** 2).sum(1)), f3[:, 0] / f3[:, 2], f3[:, 1] / f3[:, 2], q3[:, 0], q3[:, 1]
    cb = (f1 * f2).sum(1)
    b = np.sqrt(1 / (1 - cb ** 2) - 1) * np.where(cb < 0, -1, 1)
    f12, f22, p12, p22, d2, b2 = F1 ** 2, F2 ** 2, P1 ** 2, P2 ** 2, d12 ** 2, b ** 2
    p13, p14, p23, p24 = p12 * P1, p12 * p12, p22 * P2, p22 * p22
    A = -f22 * p24 - p24 * f12 - p24                                                  # :161-194
    B = 2 * p23 * d12 * b + 2 * f22 * p23 * d12 * b - 2 * F2 * p23 * F1 * d12
    Cc = (-f22 * p22 * p12 - f22 * p22 * d2 * b2 - f22 * p22 * d2 + f22 * p24 + p24 * f12 + 2 * P1 * p22 * d12
          + 2 * F1 * F2 * P1 * p22 * d12 * b - p22 * p12 * f12 + 2 * P1 * p22 * f22 * d12 - p22 * d2 * b2 - 2 * p12 * p22)
    D = 2 * p12 * P2 * d12 * b + 2 * F2 * p23 * F1 * d12 - 2 * f22 * p23 * d12 * b - 2 * P1 * P2 * d2 * b
    E = (-2 * F2 * p22 * F1 * P1 * d12 * b + f22 * p22 * d2 + 2 * p13 * d12 - p12 * d2 + f22 * p22 * p12 - p14
         - 2 * f22 * p22 * P1 * d12 + p22 * f12 * p12 + f22 * p22 * d2 * b2)
    al = -3 * B ** 2 / (8 * A ** 2) + Cc / A                                          # solve_quartic_roots, :24-66
    be = B ** 3 / (8 * A ** 3) - B * Cc / (2 * A ** 2) + D / A
    ga = -3 * B ** 4 / (256 * A ** 4) + B ** 2 * Cc / (16 * A ** 3) - B * D / (4 * A ** 2) + E / A
    P, Q = (-al ** 2 / 12 - ga).astype(cplx), (-al ** 3 / 108 + al * ga / 3 - be ** 2 / 8).astype(cplx)
    U = (-Q / 2 + np.sqrt(Q * Q / 4 + P * P * P / 27)) ** third
    y = np.where(U.real == 0, -5 * al / 6 - Q ** third, -5 * al / 6 - P / (3 * U) + U)
    w, pt1, pt2 = np.sqrt(al + 2 * y), -B / (4 * A), 3 * al + 2 * y
    pt3 = 2 * be / w
    sp, sm = np.sqrt(-(pt2 + pt3)), np.sqrt(-(pt2 - pt3))
    roots = np.stack([pt1 + (w + sp) / 2, pt1 + (w - sp) / 2, pt1 + (-w + sm) / 2, pt1 + (-w - sm) / 2], 1).real
    poses = []
    for r in roots.T:                                                                 # :203-235
        cot = (-F1 * P1 / F2 - r * P2 + d12 * b) / (-F1 * r * P2 / F2 + P1 - d12)
        st, sa = np.sqrt(1 - r * r), np.sqrt(1 / (cot ** 2 + 1))
        ca = np.sqrt(1 - sa ** 2) * np.where(cot < 0, -1, 1)
        k, z = d12 * (sa * b + ca), np.zeros_like(r)
        Cw = p1 + np.einsum("hji,hj->hi", N, np.stack([k * ca, r * k * sa, st * k * sa], 1))
        Rm = np.stack([np.stack([-ca, -sa * r, -sa * st], 1), np.stack([sa, -ca * r, -ca * st], 1), np.stack([z, -st, r], 1)], 1)
        R = np.einsum("hji,hjk,hkl->hil", Tm, Rm, N)                                  # (N^T Rm^T T)^T
        poses.append(np.concatenate([R, -np.einsum("hij,hj->hi", R, Cw)[:, :, None]], 2))
    poses = np.stack(poses, 1)
    poses[collinear[:, None] | ~np.isfinite(poses).all((2, 3))] = np.nan
    return poses


def reprojection_errors(poses, corr):
    """find_inliers (ransac_pose_p3p.cc:106-122) of every (hypothesis, correspondence) in long double: (4 it, n)"""
    X = np.concatenate([corr[:, :3], np.ones((len(corr), 1))], 1).astype(L)
    p = np.einsum("ij,hjk,nk->hni", K.astype(L), poses.reshape(-1, 3, 4).astype(L), X)
    return ((p[..., :2] / p[..., 2:] - corr[None, :, 3:].astype(L)) ** 2).sum(-1)


def restate(model, data, samples, to_beat=0):
    """hypotheses, errors (hypotheses, n) in long double, counts, the first strict maximum above to_beat (-1: none)"""
    with np.errstate(all="ignore"):
        hyp = homographies(data, samples) if model == "h" else kneip(data, samples)
        d = transfer_errors(hyp, data) if model == "h" else reprojection_errors(hyp, data)
        counts = (d < L(THRESHOLD) ** 2).sum(1)
    best, most = -1, to_beat
    for h, c in enumerate(counts):
        if c > most:
            best, most = h, c
    return hyp, d, counts, best


def gpu(ctx, model, data, samples, to_beat=0, **kw):
    """one job; the result's keys made the same for both models: hyp, hyp_all, counts (flat), inliers, best"""
    if model == "h":
        r = ctx.ransac_homography([(data, samples, THRESHOLD, to_beat)], **kw)[0]
        names = dict(hyp="H", hyp_all="H_all", best="best_iteration")
    else:
        r = ctx.ransac_pose_p3p([(data, K, samples, THRESHOLD, to_beat)], **kw)[0]
        names = dict(hyp="pose", hyp_all="pose_all", best="best_hypothesis")
    g = dict(inliers=r["inliers"], **{k: r[v] for k, v in names.items() if v in r})
    if "counts" in r:
        g["counts"] = r["counts"].ravel()
    return g


def inputs(model, case, seed=7):
    return (planar(case[0], seed), draw(*case, 4, seed + 4)) if model == "h" else (scene(case[0], seed), draw(*case, 3, seed + 4))


@pytest.fixture(scope="module")
def solved(gpu_ctx):
    """(model, case) -> (data, samples, restatement, pairs at the threshold, GPU result), each computed once"""
    cache = {}

    def get(model, case):
        if (model, case) not in cache:
            data, s = inputs(model, case)
            ref = restate(model, data, s)
            with np.errstate(invalid="ignore"):
                near = np.abs(ref[1] - L(THRESHOLD) ** 2) <= 1e-6 * L(THRESHOLD) ** 2
            assert near.mean() <= 1e-3, "too many errors at the threshold: change the seed, not the band"
            cache[model, case] = (data, s, ref, near, gpu(gpu_ctx, model, data, s, per_iteration=True))
        return cache[model, case]
    return get


@pytest.mark.parametrize("model,case", ALL, ids=IDS)
def test_counts_winner_and_inliers_equal_the_restatement(solved, model, case, gpu_ctx):
    data, s, (hyp, d, counts, best), near, g = solved(model, case)
    clean = ~near.any(1)
    assert np.array_equal(g["counts"][clean], counts[clean])
    if clean.all():
        assert g["best"] == best >= 0
        assert np.array_equal(g["inliers"], np.flatnonzero(d[best] < L(THRESHOLD) ** 2))
    assert len(g["inliers"]) == g["counts"][g["best"]] and g["inliers"].dtype == np.int32
    assert np.array_equal(g["hyp"], g["hyp_all"].reshape((-1,) + g["hyp"].shape)[g["best"]])
    assert gpu_ctx.ransac_sweep_capped == 0
    if model == "p3p":                               # no pose: the same hypotheses as in the restatement, and no inliers
        missing = ~np.isfinite(g["hyp_all"]).all((2, 3)).ravel()
        assert np.array_equal(missing, np.isnan(hyp).any((2, 3)).ravel()) and (g["counts"][missing] == 0).all()


@pytest.mark.parametrize("model,case", ALL, ids=IDS)
def test_hypotheses_agree_with_the_restatement(solved, model, case):
    hyp, g = solved(model, case)[2][0], solved(model, case)[4]["hyp_all"]
    if model == "h":
        a, b = hyp.reshape(-1, 9).astype(L), g.reshape(-1, 9).astype(L)
        worst = (1 - np.abs((a * b).sum(1)) / np.sqrt((a * a).sum(1) * (b * b).sum(1))).max()
        print("max 1 - |cos|: %.3g" % worst)
        assert worst <= H_ANGLE_BOUND
    else:
        worst = np.abs(hyp - g)[np.isfinite(hyp)].max(initial=0.0)
        print("max |pose - restated pose|: %.3g" % worst)
        assert worst <= POSE_BOUND


@pytest.mark.parametrize("model", ["h", "p3p"])
@pytest.mark.parametrize("rule", ["duplicate", "equal", "one_below"])
def test_winner_rules(solved, gpu_ctx, model, rule):
    data, s, (hyp, d, counts, best), near, g = solved(model, CASES[model][4])
    most = int(counts[best])
    if rule == "duplicate":                          # every row once more, later: the first copy of the best one keeps winning
        r = gpu(gpu_ctx, model, data, np.concatenate([s, s]), per_iteration=True)
        assert r["best"] == g["best"] and np.array_equal(r["counts"], np.tile(g["counts"], 2))
        return
    m0, inl0 = np.full(g["hyp"].shape, -7.0), np.full(len(data), -7, np.int32)
    r = gpu(gpu_ctx, model, data, s, most if rule == "equal" else most - 1, out=[(m0, inl0)])
    if rule == "equal":                              # `>`, not `>=`: nobody wins, nothing is written
        assert r["best"] == -1 and (m0 == -7.0).all() and (inl0 == -7).all()
    else:
        assert r["best"] == g["best"] and np.array_equal(m0, g["hyp"])
        assert np.array_equal(inl0[:most], g["inliers"]) and (inl0[most:] == -7).all()


def test_a_collinear_sample_has_no_pose_and_no_inliers(solved, gpu_ctx):
    data, s, _, _, g = solved("p3p", CASES["p3p"][4])
    data, s = data.copy(), np.concatenate([[[0, 1, 2]], s]).astype(np.int32)
    data[1, :3], data[2, :3] = data[0, :3] + [0.5, 0.25, 0.125], data[0, :3] + [1.0, 0.5, 0.25]
    r = gpu(gpu_ctx, "p3p", data, s, per_iteration=True)
    assert np.isnan(r["hyp_all"][0]).all() and (r["counts"][:4] == 0).all()
    assert r["best"] >= 4 and r["counts"][r["best"]] == r["counts"].max() > 0 and np.isfinite(r["hyp"]).all()


def test_a_batch_equals_its_single_calls_and_itself(gpu_ctx):
    sizes = [(8, 4), (2 * C + 1, 2 * T + 3), (100, 7), (C, 1), (3 * C - 5, T)]
    for call, keys, make in [
            (gpu_ctx.ransac_homography, ("H", "inliers", "counts", "H_all"), lambda n, it, sd: (planar(n, sd), draw(n, it, 4, sd + 1), THRESHOLD)),
            (gpu_ctx.ransac_pose_p3p, ("pose", "inliers", "counts", "pose_all"), lambda n, it, sd: (scene(n, sd), K, draw(n, it, 3, sd + 1), THRESHOLD))]:
        jobs = [make(n, it, seed) for seed, (n, it) in enumerate(sizes)]
        batch, again = call(jobs, per_iteration=True), call(jobs, per_iteration=True)
        for job, b, a in zip(jobs, batch, again):
            single = call([job], per_iteration=True)[0]
            for k in keys:
                assert b[k].tobytes() == single[k].tobytes() == a[k].tobytes(), k


def test_the_three_models_on_one_context_leave_each_other_s_results_alone(gpu_ctx):
    jobs = {"h": (planar(C + 1), draw(C + 1, 9, 4), THRESHOLD), "p3p": (scene(2 * C + 1), K, draw(2 * C + 1, 5, 3), THRESHOLD),
            "f": (np.hstack([scene(300)[:, :2] / scene(300)[:, 2:3], scene(300)[:, 3:] / 0.9]), draw(300, 11, 8), 0.0015)}
    calls = {"h": gpu_ctx.ransac_homography, "p3p": gpu_ctx.ransac_pose_p3p, "f": gpu_ctx.ransac_fundamental}
    alone = {m: calls[m]([jobs[m]], per_iteration=True)[0] for m in ("f", "p3p", "h")}
    for m in ("h", "p3p", "f"):
        r = calls[m]([jobs[m]], per_iteration=True)[0]
        assert all(np.asarray(r[k]).tobytes() == np.asarray(alone[m][k]).tobytes() for k in r), m


@pytest.mark.parametrize("model,fault", [("h", "too_few"), ("h", "index_out_of_range"), ("h", "repeated_index"), ("p3p", "too_few"),
                                         ("p3p", "index_out_of_range"), ("p3p", "repeated_index"), ("p3p", "singular_k")])
def test_a_bad_job_is_refused_by_name_and_nothing_runs(gpu_ctx, model, fault):
    width = 4 if model == "h" else 3
    data, s = inputs(model, (40, 6))
    bad_data, bad_s, bad_k = data, s.copy(), K
    if fault == "too_few":
        bad_data, bad_s = data[:width - 1], np.tile(np.arange(width, dtype=np.int32) % (width - 1), (2, 1))
    elif fault == "index_out_of_range":
        bad_s[3, width - 1] = len(data)
    elif fault == "repeated_index":
        bad_s[5, 0] = bad_s[5, 2]
    else:
        bad_k = np.array([[0.9, 0, 0.1], [0, 0.9, 0.2], [0, 0, 0]])
    shape = (3, 3) if model == "h" else (3, 4)
    out = [(np.full(shape, -7.0), np.full(len(data), -7, np.int32)) for _ in range(2)]
    with pytest.raises(ValueError, match="job 1"):
        if model == "h":
            gpu_ctx.ransac_homography([(data, s, THRESHOLD), (bad_data, bad_s, THRESHOLD)], out=out)
        else:
            gpu_ctx.ransac_pose_p3p([(data, K, s, THRESHOLD), (bad_data, bad_k, bad_s, THRESHOLD)], out=out)
    assert (out[0][0] == -7.0).all() and (out[0][1] == -7).all()
