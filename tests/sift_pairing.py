"""Pairing of two SIFT outputs of the same image, shared by tests/test_sift.py and tests/golden/make_golden_sift.py.

A descriptor record is x, y, scale, orientation (xyso) + 128 values; a keypoint record is octave, sample, x, y.  Two records
are partners if they differ by no more than a bound per quantity:
  descriptors  position max(|dx|, |dy|) / scale, scale |log2 ratio|, orientation (circular, radians), values (L2)
  keypoints    same octave; position max(|dx|, |dy|) in the octave's pixels; sample
The partner of a record is the candidate nearest in position + orientation (position + sample)."""
import numpy as np

# "Both routes have it": far above rounding, far below what separates two features (a pixel, a histogram bin of 0.17 rad).
STABLE_GATE = dict(pos=0.1, scale=0.1, ori=0.1, desc=np.inf, sample=0.1)


def descriptor_errors(a_xyso, a_desc, b_xyso, b_desc):
    """Per record of a: index of its nearest record of b (-1: b is empty) and the four differences to it."""
    n = len(a_xyso)
    idx, err = np.full(n, -1), np.full((n, 4), np.inf)
    if n == 0 or len(b_xyso) == 0:
        return idx, err
    a, b = a_xyso.astype(np.float64), b_xyso.astype(np.float64)
    pos = np.maximum(np.abs(a[:, None, 0] - b[None, :, 0]), np.abs(a[:, None, 1] - b[None, :, 1])) / a[:, None, 2]
    d = np.abs(a[:, None, 3] - b[None, :, 3]) % (2 * np.pi)
    ori = np.minimum(d, 2 * np.pi - d)
    idx = np.argmin(pos + ori, axis=1)
    r = np.arange(n)
    err = np.stack([pos[r, idx], np.abs(np.log2(a[:, 2] / b[idx, 2])), ori[r, idx],
                    np.linalg.norm(a_desc.astype(np.float64) - b_desc[idx].astype(np.float64), axis=1)], axis=1)
    return idx, err


def keypoint_errors(a, b):
    """Keypoints as (n, 4) arrays octave, sample, x, y: nearest partner in the same octave, differences in position and sample."""
    n = len(a)
    idx, err = np.full(n, -1), np.full((n, 2), np.inf)
    if n == 0 or len(b) == 0:
        return idx, err
    a, b = a.astype(np.float64), b.astype(np.float64)
    pos = np.maximum(np.abs(a[:, None, 2] - b[None, :, 2]), np.abs(a[:, None, 3] - b[None, :, 3]))
    smp = np.abs(a[:, None, 1] - b[None, :, 1])
    cost = np.where(a[:, None, 0] == b[None, :, 0], pos + smp, np.inf)
    idx = np.argmin(cost, axis=1)
    r = np.arange(n)
    same = np.isfinite(cost[r, idx])
    err = np.where(same[:, None], np.stack([pos[r, idx], smp[r, idx]], axis=1), np.inf)
    return idx, err


def within(err, bounds):
    return np.all(err <= np.asarray(bounds, np.float64)[None, :], axis=1)
