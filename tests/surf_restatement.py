"""A plain numpy restatement of sfm::Surf (libs/sfm/surf.cc): set_image + process for one uint8 image.

Arithmetic as in the reference built without contraction: the summed-area table and the filter sums are int64; a response is
float32(sum) * inv_karea per filter, then dxx * dyy - 0.912f * dxy * dxy in single float32 operations; the Haar responses dx,
dy are single float32 operations; the localisation and the orientation windows run in float64 with the reference's
expressions and its order of additions.  ``dtype`` applies to the descriptor stage only (rotation, rounding, bin sums,
normalisation): float32 is the reference, float64 shows what rounding alone does to the same formula.

One thing is not restated: extrema_detection also tests the first and the last row of a map (and check_maximum would read a
row outside the map for them).  Those rows lie in the zero border of every map and 0 > 0 fails its first comparison, so only
interior pixels are tested here.

surf(image, ...) returns (keypoints, records, margins): keypoints as rows (octave, integer sample, integer x, integer y,
sample, x, y) in the reference's order; records as rows (keypoint index, x, y, scale, orientation, 64 values); margins: how
close the input came to one of the reference's decisions (see test_surf.py)."""
import numpy as np

FS = [[3, 5, 7, 9], [5, 9, 13, 17], [9, 17, 25, 33], [17, 33, 49, 65]]
F = np.float32
PI = 3.14159265358979323846
SAMPLES = [(rx, ry) for ry in range(-5, 6) for rx in range(-5, 6) if rx * rx + ry * ry < 36]
GAUSSIAN = np.array([float("%.6g" % np.exp(-(rx * rx + ry * ry) / 12.5)) for rx, ry in SAMPLES]).astype(F)   # the table's digits
WINDOWS = []
_deg = -PI
while _deg < PI:
    WINDOWS.append((_deg - PI / 6.0, _deg + PI / 6.0))
    _deg += PI / 8.0


def grey(image):
    if image.ndim == 2:
        return image
    v = image.astype(np.int64)
    return ((v.max(axis=2) + v.min(axis=2) + 1) >> 1).astype(np.uint8)


def response_map(sat, fs, step):
    h, w = sat.shape
    out = np.zeros((len(range(0, h, step)), len(range(0, w, step))), F)
    border = fs + fs // 2 + 1
    xs, ys = np.arange(0, w, step), np.arange(0, h, step)
    ix, iy = np.flatnonzero((xs >= border) & (xs + border < w)), np.flatnonzero((ys >= border) & (ys + border < h))
    if len(ix) == 0 or len(iy) == 0:
        return out
    X, Y = xs[ix], ys[iy]
    at = lambda dx, dy: sat[np.ix_(Y + dy, X + dx)]
    box = lambda x0, y0, x1, y1: at(x1, y1) + at(x0, y0) - at(x0, y1) - at(x1, y0)      # the pixels x0 < x <= x1, y0 < y <= y1
    f2 = fs // 2
    ax, ay, by = -fs - f2 - 1, -fs, fs - 1
    dxx = box(ax, ay, ax + fs, by) - 2 * box(ax + fs, ay, ax + 2 * fs, by) + box(ax + 2 * fs, ay, ax + 3 * fs, by)
    dyy = box(ay, ax, by, ax + fs) - 2 * box(ay, ax + fs, by, ax + 2 * fs) + box(ay, ax + 2 * fs, by, ax + 3 * fs)
    dxy = box(-fs - 1, -fs - 1, -1, -1) - box(0, -fs - 1, fs, -1) - box(-fs - 1, 0, -1, fs) + box(0, 0, fs, fs)
    inv = F(1.0 / (fs * (2 * fs - 1)))
    dxx_t, dyy_t, dxy_t = dxx.astype(F) * inv, dyy.astype(F) * inv, dxy.astype(F) * inv
    out[np.ix_(iy, ix)] = dxx_t * dyy_t - F(0.912) * dxy_t * dxy_t
    return out


def localize(maps, o, s, x, y, threshold, w, h, margins):
    """keypoint_localization: (sample, x, y) or None."""
    n0, n1, n2 = [m[y - 1:y + 2, x - 1:x + 2].reshape(9) for m in maps[s - 1:s + 2]]
    d = np.float64
    b = [d(-(n1[5] - n1[3])) * 0.5, d(-(n1[7] - n1[1])) * 0.5, d(-(n2[4] - n0[4])) * 0.5]
    m = [0.0] * 9
    m[0] = d(n1[3]) - 2.0 * d(n1[4]) + d(n1[5])
    m[1] = d(n1[8] - n1[6] - n1[2] + n1[0]) * 0.25
    m[2] = d(n2[5] - n2[3] - n0[5] + n0[3]) * 0.25
    m[3] = m[1]
    m[4] = d(n1[1]) - 2.0 * d(n1[4]) + d(n1[7])
    m[5] = d(n2[7] - n2[1] - n0[7] + n0[1]) * 0.25
    m[6], m[7] = m[2], m[5]
    m[8] = d(n0[4]) - 2.0 * d(n1[4]) + d(n2[4])
    det = m[0] * m[4] * m[8] + m[1] * m[5] * m[6] + m[2] * m[3] * m[7] - m[2] * m[4] * m[6] - m[1] * m[3] * m[8] - m[0] * m[5] * m[7]
    eps = d(F(1.0e-5))
    margins["det"] = min(margins["det"], abs(abs(det) - eps) / eps)
    if -eps <= det <= eps:
        return None
    inv = [(m[4] * m[8] - m[5] * m[7]) / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
           (m[5] * m[6] - m[3] * m[8]) / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
           (m[3] * m[7] - m[4] * m[6]) / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det]
    v = [inv[3 * r] * b[0] + inv[3 * r + 1] * b[1] + inv[3 * r + 2] * b[2] for r in range(3)]
    margins["half"] = min(margins["half"], abs(max(v) - 0.5) / 0.5, abs(min(v) + 0.5) / 0.5)
    if max(v) > 0.5 or min(v) < -0.5:
        return None
    value = F(d(n1[4]) - 0.5 * (b[0] * v[0] + b[1] * v[1] + b[2] * v[2]))
    margins["contrast"] = min(margins["contrast"], abs(d(value) - d(threshold)) / abs(d(threshold)))
    if value < threshold:
        return None
    sampling = d(F(2 ** o))
    kx, ky = F((d(F(x)) + v[0]) * sampling), F((d(F(y)) + v[1]) * sampling)
    margins["bounds"] = min(margins["bounds"], abs(d(kx)), abs(d(ky)), abs(d(kx) + 1.0 - w) / w, abs(d(ky) + 1.0 - h) / h)
    if kx < F(0) or kx + F(1) > F(w) or ky < F(0) or ky + F(1) > F(h):
        return None
    return F(d(F(s)) + v[2]), kx, ky


def haar(sat, x, y, fs):
    """filter_dx_dy at the pixels (x, y) (arrays): float32 dx, dy."""
    at = lambda dx, dy: sat[y + dy, x + dx]
    x1, x2, x3, x4 = at(-fs - 1, -fs - 1), at(-1, -fs - 1), at(0, -fs - 1), at(fs, -fs - 1)
    x5, x6, x7, x8 = at(-fs - 1, fs), at(-1, fs), at(0, fs), at(fs, fs)
    y1, y2, y3, y4 = at(-fs - 1, -1), at(fs, -1), at(-fs - 1, 0), at(fs, 0)
    norm = F((2 * fs + 1) * fs * (fs + 1))
    return ((x8 + x2 - x4 - x6) - (x7 + x1 - x3 - x5)).astype(F) / norm, ((x8 + y1 - x5 - y2) - (y4 + x1 - y3 - x4)).astype(F) / norm


def orientation(sat, x, y, scale, margins):
    """descriptor_orientation: float32 orientation or None."""
    h, w = sat.shape
    px, py, sc = int(x + F(0.5)), int(y + F(0.5)), int(scale)
    spacing = 8 * sc + 1
    if px < spacing or py < spacing or px + spacing >= w or py + spacing >= h:
        return None
    rx, ry = np.array(SAMPLES).T
    dx, dy = haar(sat, px + rx * sc, py + ry * sc, 2 * sc)
    dx, dy = dx * GAUSSIAN, dy * GAUSSIAN
    ang = np.arctan2(dy.astype(np.float64), dx.astype(np.float64))
    best, sums = (0.0, 0.0, 0.0), []
    for ws, we in WINDOWS:
        near = np.abs(np.stack([ang, ang + 2.0 * PI, ang - 2.0 * PI])[:, :, None] - np.array([ws, we])).min()
        margins["window"] = min(margins["window"], near)
        inside = ((ang > ws) & (ang < we)) | ((ang + 2.0 * PI > ws) & (ang + 2.0 * PI < we)) | ((ang - 2.0 * PI > ws) & (ang - 2.0 * PI < we))
        # cumsum adds one after the other, as the reference's loop does
        sx = np.cumsum(dx[inside].astype(np.float64))[-1] if inside.any() else 0.0
        sy = np.cumsum(dy[inside].astype(np.float64))[-1] if inside.any() else 0.0
        length = sx * sx + sy * sy
        sums.append((length, (sx, sy)))
        if length > best[2]:
            best = (sx, sy, length)
    for i, (la, sa) in enumerate(sums):
        for lb, sb in sums[i + 1:]:
            if sa != sb:                                          # (windows with the same two sums are the same window to the test)
                margins["length"] = min(margins["length"], abs(la - lb) / max(la, lb))
    return F(np.arctan2(best[1], best[0]))


def descriptor(sat, x, y, scale, ori, upright, dtype):
    """descriptor_computation in ``dtype``: 64 values or None."""
    h, w = sat.shape
    sc = int(scale)
    spacing = F(15 * sc + 1)
    if x < spacing or y < spacing or x + spacing >= F(w) or y + spacing > F(h):
        return None
    T = dtype
    # sinf, cosf and expf as the correctly rounded values (numpy's own float32 routines are allowed more than an ulp)
    sin_ori, cos_ori = (T(0), T(1)) if upright else (T(np.sin(np.float64(ori))), T(np.cos(np.float64(ori))))
    gy, gx = np.mgrid[-10:10, -10:10]
    xf, yf = gx.astype(T) + T(0.5), gy.astype(T) + T(0.5)
    rnd = lambda v: np.where(v > 0, np.floor(v + T(0.5)), np.ceil(v - T(0.5))).astype(np.int64)
    rot_x = rnd(T(x) + (cos_ori * xf - sin_ori * yf) * T(sc))
    rot_y = rnd(T(y) + (sin_ori * xf + cos_ori * yf) * T(sc))
    dx, dy = [v.astype(T) for v in haar(sat, rot_x, rot_y, sc)]
    ori_dx, ori_dy = cos_ori * dx + sin_ori * dy, -sin_ori * dx + cos_ori * dy
    weight = np.exp((-(gx * gx + gy * gy).astype(T) / ((T(2.0) * T(3.3)) * (T(2.0) * T(3.3)))).astype(np.float64)).astype(T)
    vals = np.stack([weight * ori_dx, weight * ori_dy, weight * np.abs(ori_dx), weight * np.abs(ori_dy)], axis=2)     # y, x, value
    # a bin's 25 samples one after the other, y outer and x inner: (by, yy, bx, xx, c) -> (by, bx, c, yy, xx)
    bins = vals.reshape(4, 5, 4, 5, 4).transpose(0, 2, 4, 1, 3).reshape(64, 25)
    data = np.cumsum(bins, axis=1, dtype=T)[:, -1]
    norm = np.cumsum(data * data, dtype=T)[-1]
    if np.float64(norm) <= 1e-8:
        return None
    return data / np.sqrt(norm)


def surf(image, contrast_threshold=500.0, use_upright_descriptor=False, dtype=np.float32, keypoints=None):
    """``keypoints``: the first result of an earlier call on the same image (the descriptor stage alone is run again)."""
    g = grey(np.asarray(image))
    h, w = g.shape
    sat = np.cumsum(np.cumsum(g.astype(np.int64), axis=0), axis=1)
    margins = dict(det=np.inf, half=np.inf, contrast=np.inf, bounds=np.inf, window=np.inf, length=np.inf)
    if keypoints is None:
        keypoints = []
        for o in range(4):
            maps = [response_map(sat, fs, 2 ** o) for fs in FS[o]]
            for s in (1, 2):
                c = maps[s][1:-1, 1:-1]
                largest = np.ones(c.shape, bool)
                for l in (s - 1, s, s + 1):
                    for dy in range(3):
                        for dx in range(3):
                            if l != s or dx != 1 or dy != 1:
                                largest &= c > maps[l][dy:dy + c.shape[0], dx:dx + c.shape[1]]
                for y, x in np.argwhere(largest) + 1:
                    kp = localize(maps, o, s, x, y, F(contrast_threshold), w, h, margins)
                    if kp is not None:
                        keypoints.append((o, s, x, y) + kp)
    records = []
    for i, (o, _, _, _, sample, x, y) in enumerate(keypoints):
        scale = F(3 * FS[o][int(sample + F(0.5))]) * F(1.2) / F(9.0)
        ori = orientation(sat, x, y, scale, margins)
        if ori is None:
            continue
        data = descriptor(sat, x, y, scale, ori, use_upright_descriptor, dtype)
        if data is not None:
            records.append((i, x, y, scale, ori, data))
    return keypoints, records, margins
