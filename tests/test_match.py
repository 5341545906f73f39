"""Exhaustive SIFT / SURF matching: sfm::Matching::twoway_match on the GPU (mve_amd/csrc/match_device.hip behind
mi_dmrecon_match_*) and the drop-in build/sfmrecon_mi, against fixture M1 (tests/golden/make_golden_match.py: written by the
reference itself) and the NumPy restatement (match_restatement.py, itself pinned to the reference on M1).  The arithmetic
is integer and the two float tests are single IEEE operations, so every comparison is exact."""
import ctypes
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import match_restatement as R
from mve_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
APP = os.path.join(ROOT, "build", "sfmrecon_mi")
CHECK = os.path.join(ROOT, "build", "match_class_check")
NAMES = ["mi_dmrecon_match_create", "mi_dmrecon_match_set", "mi_dmrecon_match_pairs", "mi_dmrecon_match_destroy"]
FLT_MAX = float(np.finfo(np.float32).max)
KINDS = (R.SIFT, R.SURF)
KIND_NAME = {R.SIFT: "sift", R.SURF: "surf"}
DEFAULT = {R.SIFT: (0.8, FLT_MAX), R.SURF: (0.7, FLT_MAX)}     # MatchingBase::Options (libs/sfm/matching_base.h:25-31)
PAIRS4 = [(i, j) for i in range(4) for j in range(i + 1, 4)]


@pytest.fixture(scope="module")
def m1():
    return dict(np.load(os.path.join(GOLDEN, "match_m1.npz")))


def m1_sets(m1, kind):
    return [m1["%s_%d" % (KIND_NAME[kind], v)] for v in range(4)]


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_reference_on_m1(m1):
    """Discretisation, the sequential top two, the distances and the two float tests, against what the reference wrote:
    the raw two-way results of every pair, what pairwise_match makes of them, and the lowres counts."""
    for kind in KINDS:
        name = KIND_NAME[kind]
        lowe, dist = (float(v) for v in m1[name + "_opts"])
        d = [R.discretise(s, kind) for s in m1_sets(m1, kind)]
        for i, j in PAIRS4:
            assert R.in_domain(R.inner_products(d[i], d[j]), kind)
            ab, ba = R.twoway(d[i], d[j], kind, lowe, dist)
            assert np.array_equal(ab, m1["%s12_%d_%d" % (name, i, j)]), (name, i, j)
            assert np.array_equal(ba, m1["%s21_%d_%d" % (name, i, j)]), (name, i, j)
    sift = [R.discretise(s, R.SIFT) for s in m1_sets(m1, R.SIFT)]
    surf = [R.discretise(s, R.SURF) for s in m1_sets(m1, R.SURF)]
    for i, j in PAIRS4:
        ab, ba = expected_pairwise(sift, surf, i, j, lambda kind, a, b: R.twoway(a, b, kind, *DEFAULT[kind]))
        assert np.array_equal(ab, m1["pm12_%d_%d" % (i, j)]) and np.array_equal(ba, m1["pm21_%d_%d" % (i, j)]), (i, j)
        for k, n in enumerate(m1["lowres"]):
            kind, sets = (R.SIFT, sift) if len(sift[i]) else (R.SURF, surf)
            cnt = R.count_consistent(*R.twoway(sets[i][:n], sets[j][:n], kind, *DEFAULT[kind])) if len(sets[i]) else 0
            assert cnt == m1["lowres_%d_%d" % (i, j)][k], (i, j, n)
    assert sum(int((m1["sift12_%d_%d" % p] >= 0).sum()) for p in PAIRS4) >= 100       # (the fixture is not all -1)


def expected_pairwise(sift, surf, i, j, twoway):
    """ExhaustiveMatching::pairwise_match (libs/sfm/exhaustive_matching.cc:110-140) with Matching::combine_results
    (libs/sfm/matching.cc:49-88) from a two-way matcher: a type is matched only if view 1 has descriptors of it."""
    e = np.zeros(0, np.int32)
    s12, s21 = R.remove_inconsistent(*twoway(R.SIFT, sift[i], sift[j])) if len(sift[i]) else (e, e)
    u12, u21 = R.remove_inconsistent(*twoway(R.SURF, surf[i], surf[j])) if len(surf[i]) else (e, e)
    ab = np.concatenate([s12, np.where(u12 >= 0, u12 + len(s21), u12)]).astype(np.int32)
    ba = np.concatenate([s21, np.where(u21 >= 0, u21 + len(s12), u21)]).astype(np.int32)
    return ab, ba


def test_sequential_top_two_is_the_total_order():
    """The reference's loop equals "the top two under (inner product, index) of the non-negative elements, padded with two
    dummies": the property that lets the kernel merge tiles in any order.  Many ties, zeros and negatives."""
    rng = np.random.default_rng(5)
    for trial in range(40):
        n, m = int(rng.integers(1, 40)), int(rng.integers(1, 70))
        ip = rng.integers(-3, 4, size=(n, m)).astype(np.int64) * int(rng.integers(1, 1000))
        if trial % 4 == 0:
            ip = -np.abs(ip)                                   # nothing positive: zeros against the dummies
        seq, tot = R.top2_sequential(ip), R.top2_total_order(ip)
        for a, b in zip(seq, tot):
            assert np.array_equal(a, b), trial
    # and it is associative: the top two of the parts' top twos, whatever the split and the order of the merge
    ip = rng.integers(-2, 3, size=(50, 64)).astype(np.int64)
    whole = R.top2_keys(ip)
    for cuts in ((23,), (1, 63), (16, 32, 48)):
        edges = [0] + list(cuts) + [64]
        parts = [R.top2_keys(ip[:, lo:hi], lo) for lo, hi in zip(edges[:-1], edges[1:])]
        for order in (parts, parts[::-1]):
            acc = order[0]
            for p in order[1:]:
                acc = R.merge_keys(acc, p)
            assert np.array_equal(acc, whole), cuts


def test_match_symbols_are_exported():
    L = api.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines()}
    header = open(os.path.join(ROOT, "include", "mi_dmrecon.h")).read()
    for n in NAMES:
        assert hasattr(L, n) and n in exported and n in api.EXPORTS and re.search(r"\b%s\s*\(" % n, header), n


def test_argument_checks_without_a_device():
    L = api.load_library()
    h = ctypes.c_void_p()
    opt = api.CMatchOptions(ctypes.sizeof(api.CMatchOptions), 0.8, 1.0)
    job = api.CMatchJob(0, 0, 0, 0)
    assert L.mi_dmrecon_match_create(None, 4, ctypes.byref(h)) == api.E_INVAL and b"context" in L.mi_dmrecon_last_error()
    assert L.mi_dmrecon_match_create(None, -1, ctypes.byref(h)) == api.E_INVAL and b"negative" in L.mi_dmrecon_last_error()
    assert L.mi_dmrecon_match_create(None, 4, None) == api.E_INVAL
    assert L.mi_dmrecon_match_set(None, 0, api.MATCH_SIFT, api.MATCH_F32, 0, None) == api.E_INVAL
    assert L.mi_dmrecon_match_pairs(None, api.MATCH_SIFT, ctypes.byref(opt), 1, ctypes.byref(job), None, None, None) == api.E_INVAL
    assert b"null handle" in L.mi_dmrecon_last_error()
    L.mi_dmrecon_match_destroy(None)                           # a no-op


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def planted(rng, n_a, n_b, kind, share=0.4):
    """Two float sets: random unit vectors, a share of B being noisy copies of elements of A."""
    a, b = R.unit_descriptors(rng, n_a, kind), R.unit_descriptors(rng, n_b, kind)
    k = int(min(n_a, n_b) * share)
    if k:
        src, dst = rng.permutation(n_a)[:k], rng.permutation(n_b)[:k]
        v = a[src] + rng.normal(scale=0.02, size=(k, R.DIMS[kind]))
        if kind == R.SIFT:
            v = np.abs(v)
        b[dst] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    return a, b


def expect(a16, b16, kind, lowe, dist, top2=R.top2_sequential):
    ab, ba = R.twoway(a16, b16, kind, lowe, dist, top2)
    return ab, ba, R.count_consistent(ab, ba)


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "a->b", np.nonzero(got[0] != want[0])[0][:8])
    assert np.array_equal(got[1], want[1]), (what, "b->a", np.nonzero(got[1] != want[1])[0][:8])
    assert got[2] == want[2], (what, "consistent", got[2], want[2])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["f32", "i16"])
def test_gpu_m1_through_the_python_binding(gpu_ctx, m1, form):
    """1. Fixture M1 in both input forms: raw two-way results, consistent counts and lowres prefix jobs, SIFT and SURF."""
    m = gpu_ctx.match_open(4)
    try:
        for kind in KINDS:
            name = KIND_NAME[kind]
            sets = m1_sets(m1, kind)
            for v, s in enumerate(sets):
                m.set(v, kind, s if form == "f32" else R.discretise(s, kind))
            lowe, dist = (float(x) for x in m1[name + "_opts"])
            res = m.pairs(kind, [(i, len(sets[i]), j, len(sets[j])) for i, j in PAIRS4], lowe, dist)
            for (i, j), (ab, ba, cnt) in zip(PAIRS4, res):
                w12, w21 = m1["%s12_%d_%d" % (name, i, j)], m1["%s21_%d_%d" % (name, i, j)]
                assert_same((ab, ba, cnt), (w12, w21, R.count_consistent(w12, w21)), (name, i, j))
        # pairwise_match_lowres: SIFT if view 1 has any, else SURF (exhaustive_matching.cc:142-176)
        for k, n in enumerate(int(x) for x in m1["lowres"]):
            for i, j in PAIRS4:
                kind = R.SIFT if len(m1["sift_%d" % i]) else R.SURF
                sets = m1_sets(m1, kind)
                job = (i, min(n, len(sets[i])), j, min(n, len(sets[j])))
                cnt = m.pairs(kind, [job], *DEFAULT[kind])[0][2] if len(sets[i]) else 0
                assert cnt == m1["lowres_%d_%d" % (i, j)][k], (i, j, n)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (17, 255), (255, 17), (257, 256), (1000, 1500)])
def test_gpu_shapes_off_the_tile_grid(gpu_ctx, shape):
    """2. Against the restatement; |B| = 1 has the dummy as its second best (d2 = 65534, or 32258 for SURF)."""
    rng = np.random.default_rng(shape[0] * 7919 + shape[1])
    m = gpu_ctx.match_open(2)
    try:
        for kind in KINDS:
            a, b = planted(rng, shape[0], shape[1], kind)
            m.set(0, kind, a)
            m.set(1, kind, b)
            a16, b16 = R.discretise(a, kind), R.discretise(b, kind)
            assert R.in_domain(R.inner_products(a16, b16), kind)
            for lowe, dist in (DEFAULT[kind], (1.0, FLT_MAX), (0.95, 150.0), (0.5, 60.0)):
                got = m.pairs(kind, [(0, shape[0], 1, shape[1])], lowe, dist)[0]
                assert_same(got, expect(a16, b16, kind, lowe, dist), (KIND_NAME[kind], shape, lowe, dist))
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_ties_go_to_the_larger_index(gpu_ctx):
    """3. 64 copies of one descriptor spread over a 600-element set: the winner is the largest index, the runner-up another
    copy (ratio exactly 1: accepted at Lowe 1.0 because the test is `>`, rejected just below), in both directions."""
    rng = np.random.default_rng(33)
    m = gpu_ctx.match_open(2)
    try:
        for kind in KINDS:
            b = R.unit_descriptors(rng, 600, kind)
            x, y = R.unit_descriptors(rng, 2, kind) * np.float32(0.97)     # (shorter than 1: the copies are at a distance > 0, not 0 / 0)
            where = np.sort(rng.permutation(600)[:64])
            b[where] = x
            free = int(np.setdiff1d(np.arange(600), where)[17])
            b[free] = y
            a = R.unit_descriptors(rng, 40, kind)
            a[11] = x
            a[[5, 20, 33]] = y
            m.set(0, kind, a)
            m.set(1, kind, b)
            a16, b16 = R.discretise(a, kind), R.discretise(b, kind)
            assert R.distances(R.inner_products(a16[11:12], a16[11:12]), kind)[0, 0] > 0
            ab, ba, _ = m.pairs(kind, [(0, 40, 1, 600)], 1.0, FLT_MAX)[0]
            assert ab[11] == where[-1] and ba[free] == 33, (KIND_NAME[kind], ab[11], where[-1], ba[free])
            ab, ba, _ = m.pairs(kind, [(0, 40, 1, 600)], 0.999, FLT_MAX)[0]
            assert ab[11] == -1 and ba[free] == -1, (KIND_NAME[kind], ab[11], ba[free])
            ab, ba, _ = m.pairs(kind, [(1, 600, 0, 40)], 1.0, FLT_MAX)[0]          # the same with rows and columns swapped
            assert ba[11] == where[-1] and ab[free] == 33, (KIND_NAME[kind], ba[11], where[-1], ab[free])
            for lowe in (1.0, 0.999, DEFAULT[kind][0]):
                assert_same(m.pairs(kind, [(0, 40, 1, 600)], lowe, FLT_MAX)[0], expect(a16, b16, kind, lowe, FLT_MAX), (KIND_NAME[kind], lowe))
                assert_same(m.pairs(kind, [(1, 600, 0, 40)], lowe, FLT_MAX)[0], expect(b16, a16, kind, lowe, FLT_MAX), (KIND_NAME[kind], lowe))
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_surf_all_inner_products_negative(gpu_ctx):
    """4. B = -A, permuted, all components of A positive: nothing enters the top two, the result is index 0 at distance
    32258 twice -- rejected at ratio 0.7 (1 > 0.49), accepted as index 0 at ratio 1.0."""
    rng = np.random.default_rng(4)
    a = np.abs(R.unit_descriptors(rng, 70, R.SURF)) + np.float32(0.01)
    b = -a[rng.permutation(70)]
    assert R.inner_products(R.discretise(a, R.SURF), R.discretise(b, R.SURF)).max() < 0
    m = gpu_ctx.match_open(2)
    try:
        m.set(0, R.SURF, a)
        m.set(1, R.SURF, b)
        ab, ba, cnt = m.pairs(R.SURF, [(0, 70, 1, 70)], 0.7, FLT_MAX)[0]
        assert (ab == -1).all() and (ba == -1).all() and cnt == 0
        ab, ba, cnt = m.pairs(R.SURF, [(0, 70, 1, 70)], 1.0, FLT_MAX)[0]
        assert (ab == 0).all() and (ba == 0).all() and cnt == 1
        ab, ba, cnt = m.pairs(R.SURF, [(0, 70, 1, 70)], 1.0, 179.0)[0]       # 179^2 < 32258 < 180^2
        assert (ab == -1).all() and (ba == -1).all()
        ab, ba, cnt = m.pairs(R.SURF, [(0, 70, 1, 70)], 1.0, 180.0)[0]
        assert (ab == 0).all() and (ba == 0).all()
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_zero_distances_and_the_threshold_itself(gpu_ctx):
    """5. d1 = d2 = 0 (the same descriptor twice in B): 0 / 0 is NaN and NaN > t is false, so the match is accepted, to the
    larger index.  And d1 == distance_threshold^2 exactly is not rejected: the comparison is `>`."""
    m = gpu_ctx.match_open(2)
    try:
        # SIFT: <q, e> = 255 * 255 = 65025 -> d = 0;  <q2, e2> = 245 * 245 = 60025 -> d = 2 * 5000 = 10000 = 100^2
        q = np.zeros((2, 128), np.uint16)
        q[0, 0], q[1, 1] = 255, 245
        e = np.zeros((5, 128), np.uint16)
        e[1, 0] = e[3, 0] = 255
        e[2, 1] = 245
        e[0, 2] = e[4, 3] = 9
        m.set(0, R.SIFT, q)
        m.set(1, R.SIFT, e)
        ab, ba, _ = m.pairs(R.SIFT, [(0, 2, 1, 5)], 0.8, FLT_MAX)[0]
        assert ab[0] == 3 and ab[1] == 2, ab
        assert_same(m.pairs(R.SIFT, [(0, 2, 1, 5)], 0.8, FLT_MAX)[0], expect(q, e, R.SIFT, 0.8, FLT_MAX), "sift nan")
        below = float(np.nextafter(np.float32(100.0), np.float32(0.0)))
        assert m.pairs(R.SIFT, [(0, 2, 1, 5)], 1.0, 100.0)[0][0][1] == 2
        assert m.pairs(R.SIFT, [(0, 2, 1, 5)], 1.0, below)[0][0][1] == -1
        for dist in (100.0, below):
            assert_same(m.pairs(R.SIFT, [(0, 2, 1, 5)], 1.0, dist)[0], expect(q, e, R.SIFT, 1.0, dist), ("sift", dist))
        # SURF: 127 * 127 = 16129 -> d = 0;  127 * 87 + 8 * 10 = 11129 -> d = 32258 - 22258 = 10000
        q = np.zeros((2, 64), np.int16)
        q[0, 0] = 127
        q[1, 1], q[1, 2] = 127, 8
        e = np.zeros((5, 64), np.int16)
        e[1, 0] = e[3, 0] = 127
        e[2, 1], e[2, 2] = 87, 10
        e[0, 5] = e[4, 6] = -9
        m.set(0, R.SURF, q)
        m.set(1, R.SURF, e)
        ab, ba, _ = m.pairs(R.SURF, [(0, 2, 1, 5)], 0.7, FLT_MAX)[0]
        assert ab[0] == 3, ab
        assert m.pairs(R.SURF, [(0, 2, 1, 5)], 1.0, 100.0)[0][0][1] == 2
        assert m.pairs(R.SURF, [(0, 2, 1, 5)], 1.0, below)[0][0][1] == -1
        for lowe, dist in ((0.7, FLT_MAX), (1.0, 100.0), (1.0, below)):
            assert_same(m.pairs(R.SURF, [(0, 2, 1, 5)], lowe, dist)[0], expect(q, e, R.SURF, lowe, dist), ("surf", lowe, dist))
    finally:
        m.close()


@pytest.fixture(scope="module")
def twenty_sets():
    """20 SIFT sets of unequal sizes between 0 and 400 (two of them empty) that share a pool of descriptors; the 190 jobs
    and what the restatement says of them."""
    rng = np.random.default_rng(190)
    sizes = [int(v) for v in rng.integers(1, 401, 20)]
    sizes[3], sizes[12], sizes[7], sizes[15] = 0, 0, 400, 1
    pool = R.unit_descriptors(rng, 300, R.SIFT)
    sets = []
    for n in sizes:
        s = R.unit_descriptors(rng, n, R.SIFT)
        k = n // 2
        v = np.abs(pool[rng.permutation(300)[:k]] + rng.normal(scale=0.02, size=(k, 128)))
        s[:k] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        sets.append(s[rng.permutation(n)] if n else s)
    d = [R.discretise(s, R.SIFT) for s in sets]
    jobs = [(i, sizes[i], j, sizes[j]) for i in range(20) for j in range(i + 1, 20)]
    # (the sorted form: quicker than the loop on many small jobs, and the same by test_sequential_top_two_is_the_total_order)
    want = [expect(d[i], d[j], R.SIFT, *DEFAULT[R.SIFT], top2=R.top2_total_order) for i, _, j, _ in jobs]
    return sets, jobs, want


@pytest.mark.gpu
def test_gpu_190_jobs_in_one_call(gpu_ctx, twenty_sets):
    """6a. One call with 190 jobs equals the same jobs one by one and the restatement."""
    sets, jobs, want = twenty_sets
    m = gpu_ctx.match_open(20)
    try:
        for v, s in enumerate(sets):
            m.set(v, R.SIFT, s)
        batch = m.pairs(R.SIFT, jobs, *DEFAULT[R.SIFT])
        assert len(batch) == 190 and sum(w[2] for w in want) > 500
        for k, job in enumerate(jobs):
            assert_same(batch[k], want[k], ("batch", job))
            assert_same(m.pairs(R.SIFT, [job], *DEFAULT[R.SIFT])[0], want[k], ("single", job))
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_merge_across_many_tiles(gpu_ctx):
    """6b. 4096 x 4096: 64 strips of rows and two chunks of columns meet in every column's and every row's top two."""
    rng = np.random.default_rng(4096)
    m = gpu_ctx.match_open(2)
    try:
        for kind in KINDS:
            a, b = planted(rng, 4096, 4096, kind)
            b[rng.permutation(4096)[:300]] = b[rng.permutation(4096)[:300]]          # ties far apart
            m.set(0, kind, a)
            m.set(1, kind, b)
            got = m.pairs(kind, [(0, 4096, 1, 4096)], *DEFAULT[kind])[0]
            want = expect(R.discretise(a, kind), R.discretise(b, kind), kind, *DEFAULT[kind])
            assert want[2] > 1000
            assert_same(got, want, KIND_NAME[kind])
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_four_threads_on_one_handle(gpu_ctx, twenty_sets):
    """7. Four Python threads call pairs on one handle at the same time; the results are the serial ones."""
    sets, jobs, want = twenty_sets
    m = gpu_ctx.match_open(20)
    try:
        for v, s in enumerate(sets):
            m.set(v, R.SIFT, s)
        got, errors = [None] * len(jobs), []

        def work(t):
            try:
                for rnd in range(3):
                    mine = list(range(t, len(jobs), 4))
                    for k0 in range(0, len(mine), 7):
                        part = mine[k0:k0 + 7]
                        for k, r in zip(part, m.pairs(R.SIFT, [jobs[k] for k in part], *DEFAULT[R.SIFT])):
                            got[k] = r
            except Exception as e:              # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for k, job in enumerate(jobs):
            assert_same(got[k], want[k], job)
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_argument_checks_on_a_handle(gpu_ctx):
    m = gpu_ctx.match_open(2)
    try:
        m.set(0, R.SIFT, np.zeros((3, 128), np.float32))
        with pytest.raises(ValueError):
            m.set(2, R.SIFT, np.zeros((3, 128), np.float32))                       # set out of range
        bad = np.zeros((2, 128), np.uint16)
        bad[1, 5] = 256
        with pytest.raises(ValueError):
            m.set(1, R.SIFT, bad)
        bad = np.zeros((2, 64), np.int16)
        bad[0, 63] = -129
        with pytest.raises(ValueError):
            m.set(1, R.SURF, bad)
        for job in ((0, 4, 1, 0), (0, -1, 1, 0), (0, 3, 2, 0), (-1, 0, 0, 0)):
            with pytest.raises(ValueError):
                m.pairs(R.SIFT, [job], 0.8, 1.0)
        with pytest.raises(ValueError):
            m.pairs(2, [(0, 3, 1, 0)], 0.8, 1.0)                                    # unknown kind
        ab, ba, cnt = m.pairs(R.SIFT, [(0, 3, 1, 0)], 0.8, 1.0)[0]                   # an empty side: all -1
        assert (ab == -1).all() and len(ab) == 3 and len(ba) == 0 and cnt == 0
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(CHECK), reason="build/match_class_check not built (needs the reference tree at build time)")
def test_gpu_drop_in_class_on_m1(tmp_path, m1):
    """8. The fixture's own driver linked with mve_amd/host/sfm_exhaustive_matching.cc instead of the reference's
    exhaustive_matching.cc: init, pairwise_match on every pair from an OpenMP loop of four threads, pairwise_match_lowres."""
    fin, fout = str(tmp_path / "m1.in"), str(tmp_path / "m1.out")
    R.write_driver_input(fin, m1_sets(m1, R.SIFT), m1_sets(m1, R.SURF), m1["sift_opts"], m1["surf_opts"], m1["lowres"])
    out = subprocess.run([CHECK, fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = R.read_driver_output(fout, 4, len(m1["lowres"]))
    for (i, j), rec in res.items():
        for name in ("pm12", "pm21", "lowres"):
            assert np.array_equal(rec[name], m1["%s_%d_%d" % (name, i, j)]), (name, i, j)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(APP), reason="build/sfmrecon_mi not built (needs the reference tree at build time)")
def test_gpu_unmodified_apps_sfmrecon_on_the_gpu_library(tmp_path):
    """9. MVE's own apps/sfmrecon and libs/sfm minus exhaustive_matching.cc, linked against the shim and libmi_dmrecon.so,
    computes the prebundle of a five-view synthetic scene.  A smoke check of the app: SIFT is float host code and the order
    of RANSAC's pairs depends on the thread schedule, so nothing is compared byte for byte."""
    from mve_amd import scene_io
    from mve_amd.synth import SynthParams, make_scene
    sc = make_scene(SynthParams(n_views=5, width=160, height=120, n_features=300))
    sdir = str(tmp_path / "scene")
    scene_io.write_scene(sdir, sc, embedding="original")
    out = subprocess.run([APP, "--skip-sfm", sdir], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert os.path.getsize(os.path.join(sdir, "prebundle.sfm")) > 0
    found = re.search(r"Found a total of (\d+) matching image pairs", out.stdout)
    assert found and int(found.group(1)) >= 1, out.stdout[-3000:]
