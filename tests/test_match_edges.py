"""Exhaustive SIFT / SURF matching past its author's fixtures: the rounding of the device's discretisation read back byte
for byte, inputs on which the runner-up decides, shapes on the edges of the 64 x 2048 tiles, prefixes with better matches
beyond them, inner products outside the reference's 16-bit domain, several batches in one call, and the small paths of the
API.  Every comparison is exact, against match_restatement.py.

Each family of inputs comes with a CPU test which asserts, from the restatement and its mutants alone, that the family
tells the restatement from the wrong implementation it is aimed at; the GPU never enters those conditions."""
import threading

import numpy as np
import pytest

import match_restatement as R
from mve_amd import api
from test_match import DEFAULT, FLT_MAX, KIND_NAME, KINDS, assert_same, expect, planted, twenty_sets   # noqa: F401  (a fixture)

TOP = {R.SIFT: 255, R.SURF: 127}
I16 = {R.SIFT: np.uint16, R.SURF: np.int16}
SWEEP = (0.3, 0.45, 0.6, 0.7, 0.8, 0.9, 0.95, 1.0)
EDGE_SHAPES = [(64, 2048), (63, 2047), (65, 2049), (2049, 65), (1, 4097), (4097, 1), (16, 16), (49, 48), (129, 2064), (129, 2065)]
CHUNK, STRIP = 2048, 64                                       # MATCH_CHUNK, MATCH_STRIP (mve_amd/csrc/match_device.h)
DEFAULT_ENTRIES, DEFAULT_BLOCKS = 1 << 26, (1 << 24) - 1     # MATCH_BATCH_ENTRIES, MATCH_BATCH_BLOCKS (mve_amd/csrc/match_host.cpp)


# ---- the families of inputs ---------------------------------------------------------------------------------------------

def rounding_candidates(kind):
    """For every k the nine floats around (k + 0.5) / scale, where the product with the scale lands on or next to a tie."""
    scale, ks = (255.0, range(0, 255)) if kind == R.SIFT else (127.0, range(-127, 127))
    out = []
    for k in ks:
        c = np.float32((k + 0.5) / scale)
        lo, hi = [c], [c]
        for _ in range(4):
            lo.append(np.nextafter(lo[-1], np.float32(-np.inf)))
            hi.append(np.nextafter(hi[-1], np.float32(np.inf)))
        out += lo[:0:-1] + hi
    return np.asarray(out, np.float32)


def special_values(kind):
    """The clamp's edges and what lies beyond them (no NaN: the reference's cast of NaN is undefined)."""
    f = np.float32
    tiny, lowest = f(1e-45), f(-1.0) if kind == R.SURF else f(0.0)
    v = [f(-0.0), f(0.0), tiny, -tiny, f(1e-39), f(-1e-39), f(np.inf), f(-np.inf), f(1.0), f(-1.0), f(2.0), f(-2.0)]
    for bound in (lowest, f(1.0)):
        v += [np.nextafter(bound, f(-np.inf)), np.nextafter(bound, f(np.inf))]
    return np.asarray(v, np.float32)


def rounding_set(kind):
    """The candidates and the specials packed into descriptors (the last one padded with zeros), then 300 unit-norm ones."""
    D = R.DIMS[kind]
    v = np.concatenate([rounding_candidates(kind), special_values(kind)])
    v = np.concatenate([v, np.zeros(-len(v) % D, np.float32)]).reshape(-1, D)
    return np.concatenate([v, R.unit_descriptors(np.random.default_rng(11 + kind), 300, kind)]).astype(np.float32)


def ladder(kind, n_a=None, n_b=4500, ties=False, seed=7):
    """A: one-hot rows, `top` at dimension i % D.  B: zeros, but per dimension five rows at random places that carry the
    distinct bytes top - g at that dimension, g without repetition from 1 ... 40 (in a B too short for 5 * D such rows the
    places run out rank by rank).  The products of a row of A are top * one byte column of B, its distances 2 * top * g:
    inside the reference's domain, and whether Lowe's test passes depends on exactly which g is the runner-up.
    ties: on every third dimension the best byte stands a second time, in another chunk of 2048 columns.
    Returns (A, B, the rows of A whose best is tied) in the reference's 16-bit form."""
    rng = np.random.default_rng(seed + 1000 * kind + (1 if ties else 0))
    D, top = R.DIMS[kind], TOP[kind]
    n_a = D + 2 if n_a is None else n_a
    a = np.zeros((n_a, D), I16[kind])
    a[np.arange(n_a), np.arange(n_a) % D] = top
    b = np.zeros((n_b, D), I16[kind])
    g = np.stack([rng.permutation(40)[:5] + 1 for _ in range(D)])              # [dimension, rank]
    place = rng.permutation(n_b)
    m = min(n_b, 5 * D)
    for s in range(m):
        b[place[s], s % D] = top - g[s % D, s // D]
    tied = []
    if ties:
        assert m == 5 * D and n_b > 2 * CHUNK
        spare = list(place[m:])
        for d in range(0, D, 3):
            best = int(np.argmin(g[d]))
            at = int(place[best * D + d])
            other = next(p for p in spare if p // CHUNK != at // CHUNK)
            spare.remove(other)
            b[other, d] = top - g[d, best]
            tied += [i for i in range(n_a) if i % D == d]
    return a, b, np.asarray(sorted(tied), np.int64)


def prefix_sets(kind):
    """Sets of 300 and 2600 for the job (200, 2049) and its swap.  Beyond the prefixes lie exact copies of the other side's
    rows: a[200:] are 100 vectors that every second row of b[:2049] repeats, b[2049:] repeats a[:200]."""
    rng = np.random.default_rng(41 + kind)
    a, b = R.unit_descriptors(rng, 300, kind), R.unit_descriptors(rng, 2600, kind)
    odd = np.arange(1, 2049, 2)
    b[odd] = a[200 + rng.integers(0, 100, len(odd))]
    b[2049:] = a[np.arange(2600 - 2049) % 200]
    return a, b


def full_range_sets(kind):
    """(70, 2100) bytes over the whole range of the type, with the constant rows of its extremes on both sides."""
    rng = np.random.default_rng(55 + kind)
    lo, hi = (0, 255) if kind == R.SIFT else (-128, 127)
    a = rng.integers(lo, hi + 1, (70, R.DIMS[kind])).astype(I16[kind])
    b = rng.integers(lo, hi + 1, (2100, R.DIMS[kind])).astype(I16[kind])
    a[3], a[40], a[69] = lo, hi, hi
    b[0], b[1000], b[2047], b[2048], b[2099] = hi, lo, hi, lo, hi
    return a, b


def changed_at_some_ratio(a, b, kind, mutant):
    """Per row of a: does the one-way result a -> b under `mutant` differ from the restatement's at some ratio of SWEEP?"""
    out = np.zeros(len(a), bool)
    for lowe in SWEEP:
        out |= R.oneway(a, b, kind, lowe, FLT_MAX) != R.oneway(a, b, kind, lowe, FLT_MAX, mutant)
    return out


# ---- CPU: the plan of the batches ---------------------------------------------------------------------------------------

def check_plan(sizes, entries, blocks):
    """The invariants of api.match_plan on one job list under one pair of limits."""
    n_batches, batch, block0, chunks, entry0 = api.match_plan(sizes, entries, blocks)
    lim_e, lim_b = entries or DEFAULT_ENTRIES, blocks or DEFAULT_BLOCKS
    cur, nb, ne, jobs_in = -1, 0, 0, 0
    for j, (n_a, n_b) in enumerate(sizes):
        if n_a == 0 or n_b == 0:
            assert batch[j] == -1, (j, "an empty side is in no batch")
            continue
        need_b, need_e = -(-n_a // STRIP) * -(-n_b // CHUNK), n_a + n_b
        assert need_b <= lim_b
        assert chunks[j] == -(-n_b // CHUNK), j
        assert batch[j] in (cur, cur + 1), (j, "every job once, in order, batches without a gap")
        if batch[j] != cur:                                    # a new batch: only where the old one could not take the job
            assert cur < 0 or nb + need_b > lim_b or ne + need_e > lim_e, (j, "a batch closed early")
            cur, nb, ne, jobs_in = cur + 1, 0, 0, 0
        assert block0[j] == nb and entry0[j] == ne, (j, "running sums that restart at 0")
        nb, ne, jobs_in = nb + need_b, ne + need_e, jobs_in + 1
        assert nb <= lim_b, (j, "workgroups of a batch")
        assert ne <= lim_e or jobs_in == 1, (j, "only a job alone may pass the entries limit")
    assert n_batches == cur + 1, "no batch without a job"
    return n_batches, batch


def test_plan_invariants_on_random_job_lists():
    """C1.  Random job lists with empty sides mixed in, several pairs of limits, one of them tiny."""
    rng = np.random.default_rng(2048)
    seen_many, seen_alone = False, False
    for trial in range(60):
        n = int(rng.integers(1, 40))
        sizes = [(int(rng.integers(0, 700)) * int(rng.integers(0, 4) > 0), int(rng.integers(0, 9000)) * int(rng.integers(0, 4) > 0))
                 for _ in range(n)]
        if trial % 5 == 0:
            sizes += [(0, 5), (7, 0), (0, 0)]                  # trailing jobs with an empty side
        if trial % 7 == 0:
            sizes = [(0, 3)] + sizes
        need = max([-(-a // STRIP) * -(-b // CHUNK) for a, b in sizes] + [1])
        for entries, blocks in ((0, 0), (500, need), (20000, need + 3), (10 ** 9, need), (3000, 0), (1, need)):
            n_batches, batch = check_plan(sizes, entries, blocks)
            seen_many |= n_batches > 3
            seen_alone |= any(a and b and a + b > (entries or DEFAULT_ENTRIES) for a, b in sizes)
    assert seen_many and seen_alone                             # (the lists did exercise several batches and jobs over the entries limit)


def test_plan_fixed_cases():
    """C1.  A job over the block limit is the error and names itself; trailing empty jobs make no batch; nothing but
    empty jobs is no batch at all; 190 jobs of 10 000 x 10 000 are one batch under the default limits."""
    with pytest.raises(ValueError, match=r"job 2 needs 10 workgroups"):
        api.match_plan([(64, 2048), (0, 9), (128, 2049 + 3 * 2048), (5, 5)], 10 ** 9, 9)
    assert api.match_plan([(64, 2048), (0, 9), (128, 2049 + 3 * 2048), (5, 5)], 10 ** 9, 10)[0] == 3
    n_batches, batch, block0, chunks, entry0 = api.match_plan([(100, 100), (50, 3000), (0, 4), (4, 0)], 0, 0)
    assert n_batches == 1 and list(batch) == [0, 0, -1, -1] and list(block0[:2]) == [0, 2] and list(entry0[:2]) == [0, 200]
    assert list(chunks[:2]) == [1, 2]
    assert api.match_plan([(0, 4), (4, 0), (0, 0)], 500, 8)[0] == 0
    assert api.match_plan([], 0, 0)[0] == 0
    n_batches, batch, block0, _, entry0 = api.match_plan([(10000, 10000)] * 190, 0, 0)
    assert n_batches == 1 and (batch == 0).all()
    assert block0[189] == 189 * 157 * 5 and entry0[189] == 189 * 20000
    # the entries limit is soft: a job over it goes alone, and is not refused
    n_batches, batch, block0, _, entry0 = api.match_plan([(5, 5), (300, 300), (5, 5), (6, 6)], 500, 0)
    assert n_batches == 3 and list(batch) == [0, 1, 2, 2] and list(block0) == [0, 0, 0, 1] and list(entry0) == [0, 0, 0, 10]


def test_plan_default_block_limit_is_what_a_launch_holds():
    """C1 / B.  2^24 workgroups of 256 threads are 2^32 threads, one more than HIP launches: the job is refused, and the
    largest grid below it is taken."""
    with pytest.raises(ValueError, match=r"job 1 needs 16777216 workgroups"):
        api.match_plan([(9, 9), (1 << 24, 1 << 17)], 0, 0)                          # 2^18 strips x 2^6 chunks
    assert api.match_plan([(9, 9), ((1 << 24) - 64, 1 << 17)], 0, 0)[0] == 1       # 1 + 2^24 - 64 workgroups
    assert api.match_plan([(4096, 9), ((1 << 24) - 64, 1 << 17)], 0, 0)[0] == 2    # 64 + 2^24 - 64: one too many for a launch
    check_plan([((1 << 24) - 64, 1 << 17), (64, 63 * 2048), (64, 2049)], 0, 0)     # 2^24 - 1 exactly, then the next batch
    with pytest.raises(ValueError):
        api.match_limits(0, 1 << 24)                                                # the hook does not lift the limit either


def test_debug_hooks_are_listed():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mi_dmrecon_debug.h")).read(), flags=re.S)
    assert sorted(api.DEBUG_EXPORTS) == sorted(set(re.findall(r"\b(mi_dmrecon_debug_[a-z_]+)\s*\(", src)))
    L = api.load_library()
    assert all(hasattr(L, n) for n in api.DEBUG_EXPORTS)


# ---- CPU: the families separate the restatement from its mutants ---------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_rounding_candidates_separate_the_rounding_mutants(kind):
    """C2 / D1.  Each rounding mutant gives another byte on at least 100 of the candidate values; floor(x + 0.5) differs
    from math::round on negative values alone, so on SURF only."""
    c = rounding_candidates(kind)
    assert len(c) == (2295 if kind == R.SIFT else 2286)
    D = R.DIMS[kind]
    v = np.concatenate([c, np.zeros(-len(c) % D, np.float32)]).reshape(-1, D)
    truth = R.discretise(v, kind).ravel()[:len(c)]
    for mutant in (R.quantise_rint, R.quantise_in_double) + ((R.quantise_floor_half,) if kind == R.SURF else ()):
        differ = int((R.discretise(v, kind, mutant).ravel()[:len(c)] != truth).sum())
        assert differ >= 100, (KIND_NAME[kind], mutant.__name__, differ)
    # every byte of the type is among the truths, and the specials reach both ends of the clamp
    assert len(np.unique(truth)) == (256 if kind == R.SIFT else 255)
    s = special_values(kind)
    sp = R.discretise(np.concatenate([s, np.zeros(-len(s) % D, np.float32)]).reshape(-1, D), kind).ravel()[:len(s)]
    assert sp.min() == (0 if kind == R.SIFT else -127) and sp.max() == TOP[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_ladder_separates_the_runner_up_mutants(kind):
    """C2 / D2.  On the one-hot side, at some ratio of the sweep: the third best for the second changes at least half of
    the entries, the best for the second at least 80 %.  With tied tops, ties to the smaller index change at least 20 %
    of the tied entries at Lowe 1.0, and the tied entries are at least a quarter."""
    a, b, _ = ladder(kind)
    assert R.in_domain(R.inner_products(a, b), kind) and len(a) == R.DIMS[kind] + 2 and len(b) == 4500
    third = changed_at_some_ratio(a, b, kind, R.top2_second_is_third).mean()
    first = changed_at_some_ratio(a, b, kind, R.top2_second_is_first).mean()
    assert third >= 0.5 and first >= 0.8, (KIND_NAME[kind], third, first)
    a, b, tied = ladder(kind, ties=True)
    assert R.in_domain(R.inner_products(a, b), kind) and len(tied) >= len(a) / 4
    truth, small = R.oneway(a, b, kind, 1.0, FLT_MAX), R.oneway(a, b, kind, 1.0, FLT_MAX, R.top2_ties_to_smaller)
    assert (truth[tied] != small[tied]).mean() >= 0.2, KIND_NAME[kind]
    assert (truth[tied] // CHUNK != small[tied] // CHUNK).all()          # (the two copies lie in different chunks)


@pytest.mark.parametrize("kind", KINDS)
def test_prefix_sets_separate_the_prefix_mutant(kind):
    """C2 / D4.  Searching the whole sets changes more than half of the entries of the job (200, 2049)."""
    a, b = (R.discretise(s, kind) for s in prefix_sets(kind))
    truth = R.twoway_prefix(a, 200, b, 2049, kind, 1.0, FLT_MAX)
    wrong = R.twoway_prefix_ignored(a, 200, b, 2049, kind, 1.0, FLT_MAX)
    changed = int((truth[0] != wrong[0]).sum() + (truth[1] != wrong[1]).sum())
    assert changed > (200 + 2049) / 2, (KIND_NAME[kind], changed)
    assert (wrong[0] >= 2049).mean() > 0.9 and (wrong[1] >= 200).mean() > 0.4


@pytest.mark.parametrize("kind", KINDS)
def test_full_range_sets_leave_the_domain(kind):
    """C2 / D5.  The products leave the reference's 16 bits on both ends that the type has, and -128 x -128 occurs."""
    a, b = full_range_sets(kind)
    ip = R.inner_products(a, b)
    assert not R.in_domain(ip, kind)
    if kind == R.SIFT:
        assert ip.max() == 128 * 255 * 255 and ip.min() == 0
    else:
        assert ip.max() == 64 * 128 * 128 and ip.min() == -64 * 128 * 127


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def stored(d16, kind):
    """The bytes and the `off` words the device holds for a discretised set (match_device.h: SIFT biased by -128)."""
    s = (d16.astype(np.int32) - (128 if kind == R.SIFT else 0))
    off = 128 * s.sum(axis=1) + (1 << 20) if kind == R.SIFT else np.zeros(len(s), np.int64)
    return s.astype(np.int8), off.astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_discretisation_read_back(gpu_ctx, kind):
    """D1.  The device's bytes on the rounding candidates, the clamp's edges and 300 unit-norm descriptors are the
    restatement's, `off` is 128 * sum + 2^20 (0 for SURF), and the 16-bit upload of the same bytes stores the same."""
    x = rounding_set(kind)
    d16 = R.discretise(x, kind)
    want_bytes, want_off = stored(d16, kind)
    m = gpu_ctx.match_open(2)
    try:
        m.set(0, kind, x)
        m.set(1, kind, d16)
        for s in (0, 1):
            got_bytes, got_off = m.debug_get(s, kind)
            bad = np.nonzero((got_bytes != want_bytes).ravel())[0]
            assert bad.size == 0, (KIND_NAME[kind], s, len(bad), [(float(x.ravel()[i]), int(got_bytes.ravel()[i]), int(want_bytes.ravel()[i])) for i in bad[:6]])
            assert np.array_equal(got_off, want_off), (KIND_NAME[kind], s, np.nonzero(got_off != want_off)[0][:8])
        assert m.debug_get(0, 1 - kind)[0].shape == (0, R.DIMS[1 - kind])           # (the other kind's list: never set)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_second_best_ladder(gpu_ctx, kind, ties):
    """D2.  The ladder and its swap over the sweep of ratios: every decision hangs on the exact runner-up."""
    a, b, _ = ladder(kind, ties=ties)
    m = gpu_ctx.match_open(2)
    try:
        m.set(0, kind, a)
        m.set(1, kind, b)
        for lowe in SWEEP:
            assert_same(m.pairs(kind, [(0, len(a), 1, len(b))], lowe, FLT_MAX)[0], expect(a, b, kind, lowe, FLT_MAX), (KIND_NAME[kind], lowe))
            assert_same(m.pairs(kind, [(1, len(b), 0, len(a))], lowe, FLT_MAX)[0], expect(b, a, kind, lowe, FLT_MAX), (KIND_NAME[kind], lowe, "swap"))
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_gpu_tile_edges(gpu_ctx, shape):
    """D3.  Strips of 63 / 64 / 65 rows, chunks of 2047 / 2048 / 2049 columns (a last chunk of one column: three of the
    four wavefronts have nothing to do), a block of 16 columns that just passes a chunk (2064 / 2065): the ladder resized
    and planted unit vectors, at the thresholds of test_gpu_shapes_off_the_tile_grid."""
    rng = np.random.default_rng(shape[0] * 7919 + shape[1] + 1)
    m = gpu_ctx.match_open(2)
    try:
        for kind in KINDS:
            la, lb, _ = ladder(kind, shape[0], shape[1])
            pa, pb = (R.discretise(s, kind) for s in planted(rng, shape[0], shape[1], kind))
            for what, a, b in (("ladder", la, lb), ("planted", pa, pb)):
                assert R.in_domain(R.inner_products(a, b), kind)
                m.set(0, kind, a)
                m.set(1, kind, b)
                for lowe, dist in (DEFAULT[kind], (1.0, FLT_MAX), (0.95, 150.0), (0.5, 60.0)):
                    got = m.pairs(kind, [(0, shape[0], 1, shape[1])], lowe, dist)[0]
                    assert_same(got, expect(a, b, kind, lowe, dist), (KIND_NAME[kind], what, shape, lowe, dist))
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_prefix_with_better_matches_beyond_it(gpu_ctx, kind):
    """D4.  The job (0, 200, 1, 2049) on sets of 300 and 2600 whose tails hold exact copies of the other side's rows, and
    its swap: nothing beyond a prefix may be seen."""
    a, b = prefix_sets(kind)
    a16, b16 = R.discretise(a, kind), R.discretise(b, kind)
    m = gpu_ctx.match_open(2)
    try:
        m.set(0, kind, a)
        m.set(1, kind, b)
        for lowe in (1.0, DEFAULT[kind][0]):
            want = expect(a16[:200], b16[:2049], kind, lowe, FLT_MAX)
            assert_same(m.pairs(kind, [(0, 200, 1, 2049)], lowe, FLT_MAX)[0], want, (KIND_NAME[kind], lowe))
            want = expect(b16[:2049], a16[:200], kind, lowe, FLT_MAX)
            assert_same(m.pairs(kind, [(1, 2049, 0, 200)], lowe, FLT_MAX)[0], want, (KIND_NAME[kind], lowe, "swap"))
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_full_range_bytes(gpu_ctx, kind):
    """D5.  Bytes over the whole range of the type: true 32-bit products, far outside the reference's 16 bits (SIFT: the
    bias of -128 and the two `off` words at their extremes).  The distances of the random rows saturate at 0 and 0 / 0 is
    accepted, so their entries show the argmax and its tie rule; the constant rows show the saturation at the other end."""
    a, b = full_range_sets(kind)
    m = gpu_ctx.match_open(2)
    try:
        m.set(0, kind, a)
        m.set(1, kind, b)
        assert np.array_equal(m.debug_get(0, kind)[1], stored(a, kind)[1])
        for lowe in (1.0, 0.8):
            got = m.pairs(kind, [(0, 70, 1, 2100)], lowe, FLT_MAX)[0]
            assert_same(got, expect(a, b, kind, lowe, FLT_MAX), (KIND_NAME[kind], lowe))
            assert (got[0] >= 0).sum() >= 60 and (got[1] >= 0).sum() >= 2000
            got = m.pairs(kind, [(1, 2100, 0, 70)], lowe, FLT_MAX)[0]
            assert_same(got, expect(b, a, kind, lowe, FLT_MAX), (KIND_NAME[kind], lowe, "swap"))
    finally:
        m.close()


def blocks_of(job):
    return -(-job[1] // STRIP) * -(-job[3] // CHUNK) if job[1] and job[3] else 0


@pytest.mark.gpu
def test_gpu_several_batches_in_one_call(gpu_ctx, twenty_sets):
    """D6.  The 190 jobs under limits that cut the call into many batches -- (500 entries, 8 workgroups), then (10^9, 3)
    -- and under the defaults again: the results are the restatement's every time.  Jobs with an empty side stand first,
    last and where a batch ends.  A job that needs more workgroups than the limit is refused (ValueError) and the handle
    works on: under (10^9, 3) that is every job of more than 192 rows, so there the call takes the jobs that fit and each
    of the others is shown to be refused; under (500, 8) every job fits, which is asserted."""
    sets, jobs, want = twenty_sets
    empty = (0, len(sets[0]), 3, 0)
    want_empty = (np.full(len(sets[0]), -1, np.int32), np.zeros(0, np.int32), 0)
    m = gpu_ctx.match_open(20)
    try:
        for v, s in enumerate(sets):
            m.set(v, R.SIFT, s)
        assert max(blocks_of(j) for j in jobs) <= 8 and max(blocks_of(j) for j in jobs) > 3
        for entries, blocks in ((500, 8), (10 ** 9, 3), (0, 0)):
            api.match_limits(entries, blocks)
            fit = [k for k, j in enumerate(jobs) if blocks_of(j) <= (blocks or DEFAULT_BLOCKS)]
            batch = api.match_plan([(jobs[k][1], jobs[k][3]) for k in fit])[1]
            if blocks:
                assert batch.max() >= 20, (entries, blocks, batch.max())
                cut = next(i for i in range(1, len(fit)) if batch[i] > batch[i - 1] >= 0)      # fit[cut] opens a batch
            else:
                assert batch.max() == 0
                cut = len(fit) // 2
            call = [empty] + [jobs[k] for k in fit[:cut]] + [empty, (3, 0, 12, 0)] + [jobs[k] for k in fit[cut:]] + [empty]
            wanted = [want_empty] + [want[k] for k in fit[:cut]] + [want_empty, (np.zeros(0, np.int32),) * 2 + (0,)] + [want[k] for k in fit[cut:]] + [want_empty]
            got = m.pairs(R.SIFT, call, *DEFAULT[R.SIFT])
            assert len(got) == len(wanted)
            for k, (g, w) in enumerate(zip(got, wanted)):
                assert_same(g, w, ((entries, blocks), k, call[k]))
            refused = [k for k in range(len(jobs)) if k not in set(fit)]
            assert (len(refused) > 0) == (blocks == 3)
            for k in refused[:3] + refused[-1:]:
                with pytest.raises(ValueError, match="workgroups"):
                    m.pairs(R.SIFT, [jobs[fit[0]], jobs[k]], *DEFAULT[R.SIFT])
                assert_same(m.pairs(R.SIFT, [jobs[fit[0]]], *DEFAULT[R.SIFT])[0], want[fit[0]], "the call after a refusal")
    finally:
        api.match_limits(0, 0)
        m.close()


@pytest.mark.gpu
def test_gpu_a_list_is_replaced(gpu_ctx):
    """D7.  A second set() of a list: the old length is refused, the results follow the new data, and the other kind's
    list of the same set is what it was."""
    rng = np.random.default_rng(77)
    old, new, other = R.unit_descriptors(rng, 500, R.SIFT), R.unit_descriptors(rng, 130, R.SIFT), R.unit_descriptors(rng, 300, R.SIFT)
    surf, surf_other = R.unit_descriptors(rng, 90, R.SURF), R.unit_descriptors(rng, 200, R.SURF)
    m = gpu_ctx.match_open(2)
    try:
        m.set(0, R.SIFT, old)
        m.set(0, R.SURF, surf)
        m.set(1, R.SIFT, other)
        m.set(1, R.SURF, surf_other)
        d = {k: R.discretise(v, R.SIFT) for k, v in (("old", old), ("new", new), ("other", other))}
        assert_same(m.pairs(R.SIFT, [(0, 500, 1, 300)], 1.0, FLT_MAX)[0], expect(d["old"], d["other"], R.SIFT, 1.0, FLT_MAX), "old")
        surf_before = m.pairs(R.SURF, [(0, 90, 1, 200)], 1.0, FLT_MAX)[0]
        m.set(0, R.SIFT, new)
        with pytest.raises(ValueError, match="prefix"):
            m.pairs(R.SIFT, [(0, 500, 1, 300)], 1.0, FLT_MAX)
        with pytest.raises(ValueError, match="prefix"):
            m.pairs(R.SIFT, [(0, 131, 1, 300)], 1.0, FLT_MAX)
        for lowe in (1.0, 0.8):
            assert_same(m.pairs(R.SIFT, [(0, 130, 1, 300)], lowe, FLT_MAX)[0], expect(d["new"], d["other"], R.SIFT, lowe, FLT_MAX), "new")
        assert np.array_equal(m.debug_get(0, R.SIFT)[0], stored(d["new"], R.SIFT)[0])
        assert np.array_equal(m.debug_get(0, R.SURF)[0], stored(R.discretise(surf, R.SURF), R.SURF)[0])
        assert_same(m.pairs(R.SURF, [(0, 90, 1, 200)], 1.0, FLT_MAX)[0], surf_before, "surf untouched")
        assert_same(surf_before, expect(R.discretise(surf, R.SURF), R.discretise(surf_other, R.SURF), R.SURF, 1.0, FLT_MAX), "surf")
        m.set(0, R.SIFT, np.zeros((0, 128), np.float32))                           # ... and by an empty one
        with pytest.raises(ValueError, match="prefix"):
            m.pairs(R.SIFT, [(0, 1, 1, 300)], 1.0, FLT_MAX)
        assert m.debug_get(0, R.SIFT)[0].shape == (0, 128)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_a_set_against_itself_and_a_job_repeated(gpu_ctx, kind):
    """D7.  The job (i, n, i, n) at Lowe 1.0: every descriptor finds itself, or the largest index among its exact
    duplicates, in both directions.  And the same job three times in one call gives the same three times."""
    rng = np.random.default_rng(99 + kind)
    n = 333
    x = R.unit_descriptors(rng, n, kind)
    x[[10, 200, 332]] = x[4]
    x[[150, 64]] = x[63]
    d = R.discretise(x, kind)
    last = np.asarray([max(j for j in range(n) if np.array_equal(d[j], d[i])) for i in range(n)])
    assert last[4] == 332 and last[63] == 150 and (last == np.arange(n)).sum() == n - 5
    assert np.array_equal(R.oneway(d, d, kind, 1.0, FLT_MAX), last)                # (a condition on the data)
    m = gpu_ctx.match_open(1)
    try:
        m.set(0, kind, x)
        ab, ba, cnt = m.pairs(kind, [(0, n, 0, n)], 1.0, FLT_MAX)[0]
        assert np.array_equal(ab, last) and np.array_equal(ba, last) and cnt == n - 5, KIND_NAME[kind]
        want = expect(d, d, kind, *DEFAULT[kind])
        got = m.pairs(kind, [(0, n, 0, n), (0, 100, 0, n), (0, n, 0, n), (0, n, 0, n)], *DEFAULT[kind])
        for k in (0, 2, 3):
            assert_same(got[k], want, (KIND_NAME[kind], k))
        assert_same(got[1], expect(d[:100], d, kind, *DEFAULT[kind]), (KIND_NAME[kind], "prefix of itself"))
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_sift_and_surf_calls_at_the_same_time(gpu_ctx):
    """D7.  Two threads issue SIFT jobs and two SURF jobs on one handle at once, as the sfmrecon shim does from its OpenMP
    loop; the results are the serial ones, and the restatement's."""
    rng = np.random.default_rng(123)
    sizes = [400, 1, 257, 64, 0, 399]
    sets = {kind: [R.unit_descriptors(rng, n, kind) for n in sizes] for kind in KINDS}
    for kind in KINDS:
        sets[kind][5][:150] = sets[kind][0][50:200]
    jobs = [(i, sizes[i], j, sizes[j]) for i in range(6) for j in range(6) if i != j]
    m = gpu_ctx.match_open(6)
    try:
        for kind in KINDS:
            for v, s in enumerate(sets[kind]):
                m.set(v, kind, s)
        serial = {kind: m.pairs(kind, jobs, *DEFAULT[kind]) for kind in KINDS}
        for kind in KINDS:
            d = [R.discretise(s, kind) for s in sets[kind]]
            for job, got in zip(jobs, serial[kind]):
                assert_same(got, expect(d[job[0]], d[job[2]], kind, *DEFAULT[kind], top2=R.top2_total_order), (KIND_NAME[kind], job))
        got, errors = {}, []

        def work(t):
            kind, half = KINDS[t % 2], t // 2
            try:
                for rnd in range(4):
                    mine = list(range(half, len(jobs), 2))
                    for k0 in range(0, len(mine), 4):
                        part = mine[k0:k0 + 4]
                        for k, r in zip(part, m.pairs(kind, [jobs[k] for k in part], *DEFAULT[kind])):
                            got[(kind, k, rnd)] = r
            except Exception as e:              # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert len(got) == 2 * len(jobs) * 4
        for (kind, k, rnd), r in got.items():
            assert_same(r, serial[kind][k], (KIND_NAME[kind], jobs[k], rnd))
    finally:
        m.close()
