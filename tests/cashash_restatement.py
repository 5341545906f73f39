"""NumPy restatement of the reference's cascade hashing, for tests/test_cashash.py.

What it restates (paths in the reference tree):
  libs/sfm/cascade_hashing.cc:187-195    compute_zero_mean_descs: d / scale - mean in float
  libs/sfm/cascade_hashing.h:258-311     compute_cascade_hashes: the signs of the projections, first bit most significant
  libs/sfm/cascade_hashing.cc:200-223    build_buckets: per group and bucket the features in ascending id
  libs/sfm/cascade_hashing.h:417-448     collect_features_from_buckets: the walk, with its bitmap of used candidates
  libs/sfm/cascade_hashing.h:450-471     collect_top_ranked_candidates: whole levels up to min, a cut at max
  libs/sfm/cascade_hashing.h:328-415     oneway_match: NearestNeighbor<T>::find over the selected candidates, the two tests

The duplicate test here IS the reference's bitmap, not the identity on bucket ids the kernel uses: the two must agree.
"""
import numpy as np

import match_restatement as R

F32 = np.float32
SCALE = {R.SIFT: 255.0, R.SURF: 127.0}


def hash_sums(d, kind, mean, primary, secondary):
    """The D primary and groups * bits secondary projections of the discretised descriptors d in float64, and next to each
    sum its sum of magnitudes  sum |z_i| |p_i|  (the scale of any float32 evaluation's error).  z is the reference's float32."""
    D = R.DIMS[kind]
    z = (np.asarray(d).astype(F32) / F32(SCALE[kind]) - np.asarray(mean, F32)).astype(F32).astype(np.float64)
    P = np.concatenate([np.asarray(primary, F32).reshape(-1, D), np.asarray(secondary, F32).reshape(-1, D)]).astype(np.float64)
    return z @ P.T, np.abs(z) @ np.abs(P).T


def pack(bits, groups, n_bits):
    """(n, D + groups * bits) booleans -> (codes uint64 (n, D / 64), bucket ids uint16 (n, groups)), first bit most significant."""
    n, D = len(bits), bits.shape[1] - groups * n_bits
    w64 = np.uint64(1) << np.arange(63, -1, -1, dtype=np.uint64)
    codes = (bits[:, :D].reshape(n, D // 64, 64).astype(np.uint64) * w64).sum(axis=2, dtype=np.uint64)
    wb = 1 << np.arange(n_bits - 1, -1, -1)
    ids = (bits[:, D:].reshape(n, groups, n_bits) * wb).sum(axis=2).astype(np.uint16)
    return codes, ids


def popcount(x):
    """Per row of a (m, words) uint64 array."""
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=1).sum(axis=1).astype(np.int64)


def oneway(codes_q, buckets_q, desc_q, codes_c, buckets_c, desc_c, kind, options, lowe_ratio, distance):
    """CascadeHashing::oneway_match of the queries q against the set c: int32 [|q|], -1 = no match (also for a query without
    any candidate, where the reference is undefined).  options: num_bucket_groups, min_num_candidates, max_num_candidates."""
    groups, lo, hi = options["num_bucket_groups"], options["min_num_candidates"], options["max_num_candidates"]
    n_q, n_c = len(desc_q), len(desc_c)
    res = np.full(n_q, -1, np.int32)
    if n_q == 0 or n_c == 0:
        return res
    lists = []                                                 # build_buckets: a stable sort is "ascending id within a bucket"
    for g in range(groups):
        order = np.argsort(buckets_c[:, g], kind="stable")
        lists.append((order, np.searchsorted(buckets_c[order, g], np.arange(257))))
    top = np.full((n_q, hi), -1, np.int64)
    used = np.zeros(n_c, bool)
    for i in range(n_q):
        used[:] = False
        walk = []
        for g in range(groups):
            order, off = lists[g]
            b = int(buckets_q[i, g]) & 0xff                    # (read back through a uint8_t, cascade_hashing.h:430)
            ids = order[off[b]:off[b + 1]]
            ids = ids[~used[ids]]
            used[ids] = True
            walk.append(ids)
        walk = np.concatenate(walk)
        level = popcount(codes_q[i][None, :] ^ codes_c[walk])
        ranked = np.argsort(level, kind="stable")              # (level, seq)
        take = len(walk)
        if take >= lo:
            take = min(hi, int((level <= level[ranked[lo - 1]]).sum()))
        top[i, :take] = walk[ranked[:take]]
    # NearestNeighbor<T>::find over the selected descriptors in that order; the padding can never enter (product -1)
    a = np.asarray(desc_q, np.int64)
    c = np.asarray(desc_c, np.int64)[np.maximum(top, 0)]
    ip = np.where(top >= 0, np.einsum("qd,qkd->qk", a, c), -1)
    ip1, i1, ip2, _ = R.top2_sequential(ip)
    d1, d2 = R.distances(ip1, kind).astype(F32), R.distances(ip2, kind).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lowe2, dist2 = F32(lowe_ratio) * F32(lowe_ratio), F32(distance) * F32(distance)
        reject = (d1 > dist2) | ((d1 / d2) > lowe2) | (top[:, 0] < 0)
    return np.where(reject, -1, top[np.arange(n_q), i1]).astype(np.int32)
