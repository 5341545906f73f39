"""NumPy restatement of the reference's exhaustive descriptor matching, for the tests of the mi_dmrecon_match_* entry points.

What it restates (paths in the reference tree):
  libs/sfm/exhaustive_matching.cc:18-39   convert_descriptor: float -> 8-bit values held in 16-bit words
  libs/sfm/nearest_neighbor.cc:64-133     the loop over the inner products (`>=` twice, j ascending)
  libs/sfm/nearest_neighbor.cc:218-272    the start values and the distances of the two 16-bit types
  libs/sfm/matching.h:114-159             oneway_match / twoway_match: the two tests, in float
  libs/sfm/matching.cc:18-47              remove_inconsistent_matches, count_consistent_matches

Inner products are true integers here, as in the library; the reference holds them in 16 bits and agrees inside the domain
`in_domain` checks.  Pinned to tests/golden/match_m1.npz, which the reference itself wrote, by tests/test_match.py.
"""
import numpy as np

SIFT, SURF = 0, 1
DIMS = {SIFT: 128, SURF: 64}
F32 = np.float32


def ref_round(x):
    """math::round (libs/math/functions.h:70-73) on float32."""
    x = np.asarray(x, F32)
    return np.where(x > 0, np.floor(x + F32(0.5)), np.ceil(x - F32(0.5))).astype(F32)


def quantise(v, scale):
    """math::round of the float product (exhaustive_matching.cc:24, :36)."""
    return ref_round(v * F32(scale))


def discretise(desc, kind, quantise=quantise):
    """(n, 128) / (n, 64) float32 -> uint16 / int16, the reference's ProcessedFeatureSet storage."""
    v = np.asarray(desc, F32).reshape(-1, DIMS[kind])
    if kind == SIFT:
        v = np.where(v < 0, F32(0), np.where(v > 1, F32(1), v)).astype(F32)
        return quantise(v, 255.0).astype(np.uint8).astype(np.uint16)
    v = np.where(v < -1, F32(-1), np.where(v > 1, F32(1), v)).astype(F32)
    return quantise(v, 127.0).astype(np.int8).astype(np.int16)


def inner_products(a, b):
    """(|a|, |b|) int64; exact: every partial sum is an integer below 2^53."""
    return np.rint(np.asarray(a, np.float64) @ np.asarray(b, np.float64).T).astype(np.int64)


def in_domain(ip, kind):
    lo, hi = (0, 65535) if kind == SIFT else (-32768, 32767)
    return ip.size == 0 or (int(ip.min()) >= lo and int(ip.max()) <= hi)


def top2_sequential(ip):
    """The reference's loop, column by column, for all rows at once: (ip1, idx1, ip2, idx2)."""
    n = ip.shape[0]
    d1, d2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    i1, i2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for j in range(ip.shape[1]):
        v = ip[:, j]
        first = v >= d1
        second = (v >= d2) & ~first
        d2 = np.where(first, d1, np.where(second, v, d2))
        i2 = np.where(first, i1, np.where(second, j, i2))
        d1 = np.where(first, v, d1)
        i1 = np.where(first, j, i1)
    return d1, i1, d2, i2


def top2_keys(ip, first_index=0):
    """(n, 2) int64: per row the two largest keys  inner product << 32 | index + 1  of the elements with inner product >= 0
    (columns count from first_index), 0 where there is none: the dummy, below every real element."""
    n, m = ip.shape
    key = np.where(ip >= 0, (ip << 32) | (np.arange(m, dtype=np.int64)[None, :] + first_index + 1), 0)
    key = np.concatenate([key, np.zeros((n, 2), np.int64)], axis=1)
    return -np.sort(-key, axis=1)[:, :2]


def merge_keys(a, b):
    """The top two of the union of two top twos (keys of real elements are distinct)."""
    return -np.sort(-np.concatenate([a, b], axis=1), axis=1)[:, :2]


def decode_keys(key):
    """(ip1, idx1, ip2, idx2); a dummy reports product 0 and index 0."""
    ipk, idx = key >> 32, np.where(key != 0, (key & 0xffffffff) - 1, 0)
    return ipk[:, 0], idx[:, 0], ipk[:, 1], idx[:, 1]


def top2_total_order(ip):
    """The same without the loop: the top two under (inner product, index) of the elements with inner product >= 0, padded
    with two dummies that rank below every real element and report product 0, index 0."""
    return decode_keys(top2_keys(ip))


def distances(ip, kind):
    if kind == SIFT:
        return 2 * np.minimum(32767, 65025 - np.minimum(65025, ip))
    return 32258 - 2 * np.minimum(16129, np.maximum(0, ip))


def oneway(a, b, kind, lowe_ratio, distance, top2=top2_sequential):
    """Matching::oneway_match on discretised sets: int32 [|a|], -1 = no match."""
    a, b = np.asarray(a), np.asarray(b)
    res = np.full(len(a), -1, np.int32)
    if len(a) == 0 or len(b) == 0:
        return res
    ip1, i1, ip2, _ = top2(inner_products(a, b))
    d1, d2 = distances(ip1, kind).astype(F32), distances(ip2, kind).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lowe2, dist2 = F32(lowe_ratio) * F32(lowe_ratio), F32(distance) * F32(distance)          # MATH_POW2 in float
        reject = (d1 > dist2) | ((d1 / d2) > lowe2)
    return np.where(reject, -1, i1).astype(np.int32)


def twoway(a, b, kind, lowe_ratio, distance, top2=top2_sequential):
    return oneway(a, b, kind, lowe_ratio, distance, top2), oneway(b, a, kind, lowe_ratio, distance, top2)


def remove_inconsistent(ab, ba):
    ab, ba = ab.copy(), ba.copy()
    for i in range(len(ab)):
        if ab[i] >= 0 and ba[ab[i]] != i:
            ab[i] = -1
    for i in range(len(ba)):
        if ba[i] >= 0 and ab[ba[i]] != i:
            ba[i] = -1
    return ab, ba


def count_consistent(ab, ba):
    return int(sum(1 for i in range(len(ab)) if ab[i] != -1 and ba[ab[i]] == i))


def unit_descriptors(rng, n, kind):
    """n random unit-norm descriptors, non-negative for SIFT."""
    v = rng.standard_normal((n, DIMS[kind]))
    if kind == SIFT:
        v = np.abs(v)
    return (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)).astype(F32)


# ---- mutants: what a subtly wrong implementation would compute ------------------------------------------------------------
# None of these is the reference.  tests/test_match_edges.py asserts, on the CPU and from this file alone, that each family of
# inputs it sends to the GPU tells the restatement above from the mutant the family is aimed at: a condition on the inputs.

def quantise_rint(v, scale):
    """Mutant of quantise: round half to even (rintf)."""
    return np.rint(v * F32(scale)).astype(F32)


def quantise_in_double(v, scale):
    """Mutant of quantise: product and sum in double, where neither is rounded."""
    x = v.astype(np.float64) * scale
    return np.where(x > 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(F32)


def quantise_floor_half(v, scale):
    """Mutant of quantise: floor(x + 0.5) in float for either sign."""
    return np.floor(v * F32(scale) + F32(0.5)).astype(F32)


def top3_keys(ip):
    """top2_keys with a third: (n, 3), padded with three dummies."""
    n, m = ip.shape
    key = np.where(ip >= 0, (ip << 32) | (np.arange(m, dtype=np.int64)[None, :] + 1), 0)
    key = np.concatenate([key, np.zeros((n, 3), np.int64)], axis=1)
    return -np.sort(-key, axis=1)[:, :3]


def top2_second_is_third(ip):
    """Mutant: the runner-up is lost and the third best reported in its place."""
    return decode_keys(top3_keys(ip)[:, [0, 2]])


def top2_second_is_first(ip):
    """Mutant: the best reported twice."""
    return decode_keys(top3_keys(ip)[:, [0, 0]])


def top2_ties_to_smaller(ip):
    """Mutant: the reference's loop with `>` for `>=`: among equal products the smaller index wins."""
    n = ip.shape[0]
    d1, d2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    i1, i2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for j in range(ip.shape[1]):
        v = ip[:, j]
        first = v > d1
        second = (v > d2) & ~first
        d2 = np.where(first, d1, np.where(second, v, d2))
        i2 = np.where(first, i1, np.where(second, j, i2))
        d1 = np.where(first, v, d1)
        i1 = np.where(first, j, i1)
    return d1, i1, d2, i2


def twoway_prefix(a, n_a, b, n_b, kind, lowe_ratio, distance, top2=top2_sequential):
    """The job (a, n_a, b, n_b): the first n_a of a against the first n_b of b."""
    return twoway(a[:n_a], b[:n_b], kind, lowe_ratio, distance, top2)


def twoway_prefix_ignored(a, n_a, b, n_b, kind, lowe_ratio, distance, top2=top2_sequential):
    """Mutant of twoway_prefix: the whole sets are searched, the prefixes only cut the lists of results."""
    ab, ba = twoway(a, b, kind, lowe_ratio, distance, top2)
    return ab[:n_a], ba[:n_b]


# ---- the file format of tests/golden/ref_match_driver.cc ------------------------------------------------------------------

def write_driver_input(path, sift_sets, surf_sets, sift_opts, surf_opts, lowres):
    """sift_sets / surf_sets: per view a float32 (n, 128) / (n, 64); *_opts: (lowe_ratio, distance); lowres: list of N."""
    with open(path, "wb") as f:
        np.int32(len(sift_sets)).tofile(f)
        for s, u in zip(sift_sets, surf_sets):
            np.int32(len(s)).tofile(f)
            np.ascontiguousarray(s, F32).tofile(f)
            np.int32(len(u)).tofile(f)
            np.ascontiguousarray(u, F32).tofile(f)
        np.asarray(list(sift_opts) + list(surf_opts), F32).tofile(f)
        np.int32(len(lowres)).tofile(f)
        np.asarray(lowres, np.int32).tofile(f)


DRIVER_LISTS = ("pm12", "pm21", "sift12", "sift21", "surf12", "surf21")


def read_driver_output(path, n_views, n_lowres):
    """{(i, j): {pm12, pm21, sift12, sift21, surf12, surf21: int32 arrays, lowres: int32 [n_lowres]}} for i < j."""
    raw = np.fromfile(path, np.int32)
    at, out = 0, {}
    for i in range(n_views):
        for j in range(i + 1, n_views):
            rec = {}
            for name in DRIVER_LISTS:
                n = int(raw[at])
                rec[name] = raw[at + 1:at + 1 + n].copy()
                at += 1 + n
            rec["lowres"] = raw[at:at + n_lowres].copy()
            at += n_lowres
            out[(i, j)] = rec
    assert at == len(raw), "trailing data in the driver's output"
    return out
