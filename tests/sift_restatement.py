"""A plain numpy restatement, in float64, of the stages of sfm::Sift (libs/sfm/sift.cc) in front of the orientations, and of
the image operations of libs/mve/image_tools.h they use.  Each function restates ONE stage on whatever input it is given,
so that tests/test_sift_stages.py can hand it the device's own input to that stage and errors do not chain:

  gray               byte_to_float_image + desaturate<float>(DESATURATE_AVERAGE)   image_tools.cc:23-36, image_tools.h:1339-1343
  double_size        rescale_double_size_supersample<float>                         image_tools.h:790-826
  half_size          rescale_half_size_gaussian<float>                              image_tools.h:619-693
  blur               blur_gaussian<float>, clamped, taps i = -ks ... ks             image_tools.h:1047-1077
  make_taps          blur_gaussian's kernel and its sum                             image_tools.h:1032-1043, accum.h
  octave_plan        the sizes, sources and blurs of create_octaves / add_octave    sift.cc:170-259
  extrema            the 27-neighbour test, in the order sample, y, x               sift.cc:287-335
  localize           keypoint_localization: five steps, every rejection test        sift.cc:350-476
  orientations       the 36-bin histogram and its peaks (for make_golden_sift.py)   sift.cc:579-589, :599-697

The weights are the reference's float32 numbers (the device receives the same ones); every sum, product and quotient of
them is float64.  The same operation on |v| is what a rounding bound is made of (tests/test_sift_stages.py)."""
import numpy as np

F = np.float32


def gray(image):
    """u8 or f32, H x W or H x W x 3 -> float64 H x W (sift.cc:135-165)."""
    v = image.astype(np.float64)
    if image.dtype == np.uint8:
        v = np.clip(v / 255.0, 0.0, 1.0)
    if image.ndim == 2:
        return v
    third = float(F(1.0) / F(3.0))                                # image_tools.h:1341
    return v[:, :, 0] * third + v[:, :, 1] * third + v[:, :, 2] * third


def double_size(img):
    """image_tools.h:790-826: four input pixels, a quarter each."""
    v = img.astype(np.float64)
    h, w = v.shape
    y, x = np.arange(2 * h), np.arange(2 * w)
    y0, y1 = y >> 1, (y + (y + 1 < 2 * h)) >> 1
    x0, x1 = x >> 1, (x + (x + 1 < 2 * w)) >> 1
    return v[np.ix_(y0, x0)] * 0.25 + v[np.ix_(y0, x1)] * 0.25 + v[np.ix_(y1, x0)] * 0.25 + v[np.ix_(y1, x1)] * 0.25


def half_weights():
    """w1, w2, w3 of sigma = sqrt(3) / 2 and their sum over the sixteen taps in the reference's order, all float32
    (image_tools.h:638-640, :667-688)."""
    sigma = F(0.866025403784439)
    s2 = F(2.0) * (sigma * sigma)
    w1, w2, w3 = [F(np.exp(np.float64(F(a) / s2))) for a in (-0.5, -2.5, -4.5)]
    rows = [[w3, w2, w2, w3], [w2, w1, w1, w2], [w2, w1, w1, w2], [w3, w2, w2, w3]]
    wsum = F(0.0)
    for r in rows:
        for wgt in r:
            wsum = F(wsum + wgt)
    return np.array(rows, np.float64), float(wsum)


def half_size(img):
    """image_tools.h:619-693: sixteen clamped taps around the pixel pair (2x, 2y)."""
    v = img.astype(np.float64)
    h, w = v.shape
    wr, wsum = half_weights()
    y, x = np.arange((h + 1) >> 1), np.arange((w + 1) >> 1)
    ys = [np.maximum(0, 2 * y - 1), 2 * y, np.minimum(h - 1, 2 * y + 1), np.minimum(h - 1, 2 * y + 2)]
    xs = [np.maximum(0, 2 * x - 1), 2 * x, np.minimum(w - 1, 2 * x + 1), np.minimum(w - 1, 2 * x + 2)]
    acc = np.zeros((len(y), len(x)))
    for r in range(4):
        for c in range(4):
            acc += v[np.ix_(ys[r], xs[c])] * wr[r, c]
    return acc / wsum


def make_taps(sigma):
    """blur_gaussian's kernel for a float32 sigma: (ks, wsum, taps[2 ks + 1]) with float32 weights and their float32 sum in
    the order i = -ks ... ks, or (0, 0, []) where the reference returns a copy (image_tools.h:1032-1043)."""
    sigma = F(sigma)
    if -0.1 <= float(sigma) <= 0.1:
        return 0, 0.0, np.zeros(0)
    ks = int(np.ceil(F(sigma * F(2.884))))
    i = np.abs(np.arange(-ks, ks + 1)).astype(F)
    taps = np.exp(-((i * i) / (F(2.0) * sigma * sigma)).astype(np.float64)).astype(F)
    wsum = F(0.0)
    for t in taps:
        wsum = F(wsum + t)
    return ks, float(wsum), taps.astype(np.float64)


def blur_pass(v, ks, wsum, taps, axis):
    n = v.shape[axis]
    acc = np.zeros_like(v)
    for i in range(-ks, ks + 1):
        idx = np.clip(np.arange(n) + i, 0, n - 1)                 # image_tools.h:1057, :1073
        acc += np.take(v, idx, axis=axis) * float(taps[i + ks])
    return acc / float(wsum)


def blur(img, ks, wsum, taps):
    """image_tools.h:1047-1077 with the given taps (taps[i + ks], i = -ks ... ks): the x pass, then the y pass."""
    v = img.astype(np.float64)
    return blur_pass(blur_pass(v, ks, wsum, taps, 1), ks, wsum, taps, 0)


def octave_plan(w, h, o):
    """create_octaves / add_octave (sift.cc:170-259): per octave (octave, w, h, [sigma of each of the S + 3 blurs, None: a copy])."""
    S, base, inh = int(o["num_samples_per_octave"]), F(o["base_blur_sigma"]), F(o["inherent_blur_sigma"])

    def sigmas(has):
        first = F(np.sqrt(F(base * base - has * has))) if base > has else None
        k = F(np.power(np.float64(2.0), np.float64(F(1.0) / F(S))))
        out, sigma = [first], base
        for _ in range(1, S + 3):
            sk = F(sigma * k)
            out.append(F(np.sqrt(F(sk * sk - sigma * sigma))))
            sigma = sk
        return out

    plan = []
    if o["min_octave"] < 0:
        plan.append((-1, 2 * w, 2 * h, sigmas(F(inh * F(2.0)))))
    for _ in range(max(0, o["min_octave"])):
        w, h = (w + 1) >> 1, (h + 1) >> 1
    has = inh
    for i in range(max(0, o["min_octave"]), o["max_octave"] + 1):
        plan.append((i, w, h, sigmas(has)))
        w, h = (w + 1) >> 1, (h + 1) >> 1
        has = base
    return plan


def scale_space(image, o):
    """The whole chain in float64: per octave of octave_plan (octave, img (S + 3, h, w), dog (S + 2, h, w))."""
    orig = gray(image)
    h, w = orig.shape
    out, cur = [], orig
    for octave, ow, oh, sig in octave_plan(w, h, o):
        if octave < 0:
            src = double_size(orig)
        else:
            if out and out[-1][0] < 0:
                cur = orig
            while cur.shape != (oh, ow):
                cur = half_size(cur)
            src = cur
        imgs = [src if sig[0] is None or make_taps(sig[0])[0] == 0 else blur(src, *make_taps(sig[0]))]
        for s in sig[1:]:
            imgs.append(blur(imgs[-1], *make_taps(s)))
        imgs = np.stack(imgs)
        out.append((octave, imgs, imgs[1:] - imgs[:-1]))
    return out


def extrema(dog):
    """sift.cc:287-335 on the S + 2 DoG images of an octave: (n, 3) int x, y, sample, in the order sample, y, x.  Comparisons
    only: a centre is kept if every one of its 26 neighbours is smaller, or every one larger."""
    n, h, w = dog.shape
    if n < 3 or h < 3 or w < 3:
        return np.zeros((0, 3), np.int64)
    c = dog[1:-1, 1:-1, 1:-1]
    largest, smallest = np.ones(c.shape, bool), np.ones(c.shape, bool)
    for l in range(3):
        for dy in range(3):
            for dx in range(3):
                if (l, dy, dx) == (1, 1, 1):
                    continue
                nb = dog[l:n - 2 + l, dy:h - 2 + dy, dx:w - 2 + dx]
                largest &= ~(nb >= c)
                smallest &= ~(nb <= c)
    s, y, x = np.nonzero(largest | smallest)
    return np.stack([x + 1, y + 1, s], axis=1)


def orientations(img, x, y, sample, S, base_blur_sigma):
    """generate_grad_ori_images at the window's pixels (sift.cc:579-589) and orientation_assignment (sift.cc:599-697) for one
    keypoint (x, y, sample as the reference prints them) on the S + 3 Gaussian images of its octave, in float64: the peaks
    in ascending bin order, [] where the window leaves the image.  The window's size and centre are the reference's float32
    numbers; every sum is float64."""
    ix, iy = int(F(x) + F(0.5)), int(F(y) + F(0.5))
    s = int(np.floor(sample + 0.5) if sample > 0 else np.ceil(sample - 0.5))          # math::round
    sigma = F(base_blur_sigma) * F(np.power(2.0, float((F(sample) + F(1.0)) / F(S))))  # keypoint_relative_scale
    win = int(F(sigma * F(1.5)) * F(3.0))
    v = img[s + 1].astype(np.float64)
    h, w = v.shape
    if ix < win or ix + win >= w or iy < win or iy + win >= h:
        return []
    gdx, gdy = np.zeros((h, w)), np.zeros((h, w))                  # (the border pixels keep magnitude 0)
    gdx[1:-1, 1:-1] = 0.5 * (v[1:-1, 2:] - v[1:-1, :-2])
    gdy[1:-1, 1:-1] = 0.5 * (v[2:, 1:-1] - v[:-2, 1:-1])
    box = (slice(iy - win, iy + win + 1), slice(ix - win, ix + win + 1))
    gm, go = np.hypot(gdx, gdy)[box], np.arctan2(gdy, gdx)[box]
    go = np.where(go < 0.0, go + 2.0 * np.pi, go)
    d = np.arange(-win, win + 1, dtype=np.float64)
    dist = (d[None, :] - float(F(x) - F(ix))) ** 2 + (d[:, None] - float(F(y) - F(iy))) ** 2
    weight = np.exp(-dist / (2.0 * float(sigma * F(1.5)) ** 2)) * (dist <= win * win + 0.5)
    hist = np.bincount(np.clip((36.0 * go / (2.0 * np.pi)).astype(int), 0, 35).ravel(), (gm * weight).ravel(), 36)
    for _ in range(6):
        hist = (np.roll(hist, 1) + hist + np.roll(hist, -1)) / 3.0
    out = []
    for i in range(36):
        h0, h1, h2 = hist[i - 1], hist[i], hist[(i + 1) % 36]
        if h1 <= 0.8 * hist.max() or h1 <= h0 or h1 <= h2:
            continue
        out.append(2.0 * np.pi * (-0.5 * (h2 - h0) / (h0 - 2.0 * h1 + h2) + i + 0.5) / 36.0)
    return out


def localize(dog, cand, S, contrast_threshold, edge_ratio_threshold, dtype=np.float64, margin=1e-3):
    """keypoint_localization (sift.cc:350-476) for the candidates (x, y, sample) on an octave's DoG images.  Returns
    (loc (n, 4): x, y, sample, kept; decisive (n,) bool).  A candidate is DECISIVE if no quantity the reference compares lies
    within `margin` of its threshold: relative for |det| against 1e-15, the contrast and the edge score; absolute for the
    offsets (+-0.6 per step, 1.5 / 1.0 at the end) and, relative to max(1, |limit|), for the scale-space borders (-1, S, 0,
    w - 1, h - 1) and the edge score against 0.  ``dtype``: float64, or float32 for the reference's own arithmetic."""
    T = dtype
    d = dog.astype(T)
    _, h, w = d.shape
    half, quarter, two = T(0.5), T(0.25), T(2.0)
    thres = (T(edge_ratio_threshold) + T(1.0)) * (T(edge_ratio_threshold) + T(1.0)) / T(edge_ratio_threshold)
    contrast = T(contrast_threshold)
    loc, decisive = np.zeros((len(cand), 4), np.float64), np.ones(len(cand), bool)
    with np.errstate(all="ignore"):
        for n, (ix, iy, s) in enumerate(np.asarray(cand).tolist()):
            d0, d1, d2 = d[s], d[s + 1], d[s + 2]
            ok = True
            fx = fy = fs = T(0.0)
            for _ in range(5):
                c1 = d1[iy, ix]
                Dx = (d1[iy, ix + 1] - d1[iy, ix - 1]) * half
                Dy = (d1[iy + 1, ix] - d1[iy - 1, ix]) * half
                Ds = (d2[iy, ix] - d0[iy, ix]) * half
                Dxx = d1[iy, ix + 1] + d1[iy, ix - 1] - two * c1
                Dyy = d1[iy + 1, ix] + d1[iy - 1, ix] - two * c1
                Dss = d2[iy, ix] + d0[iy, ix] - two * c1
                Dxy = (d1[iy + 1, ix + 1] + d1[iy - 1, ix - 1] - d1[iy + 1, ix - 1] - d1[iy - 1, ix + 1]) * quarter
                Dxs = (d2[iy, ix + 1] + d0[iy, ix - 1] - d2[iy, ix - 1] - d0[iy, ix + 1]) * quarter
                Dys = (d2[iy + 1, ix] + d0[iy - 1, ix] - d2[iy - 1, ix] - d0[iy + 1, ix]) * quarter
                # math::matrix_determinant and matrix_inverse of the symmetric 3 x 3 (matrix_tools.h:394, :462)
                det = Dxx * Dyy * Dss + Dxy * Dys * Dxs + Dxs * Dxy * Dys - Dxs * Dyy * Dxs - Dxy * Dxy * Dss - Dxx * Dys * Dys
                ok &= not abs(abs(float(det)) - 1e-15) <= margin * 1e-15
                if -1e-15 <= det <= 1e-15:
                    fx = fy = fs = T(0.0)
                    break
                r0, r1, r2 = (Dyy * Dss - Dys * Dys) / det, (Dxs * Dys - Dxy * Dss) / det, (Dxy * Dys - Dxs * Dyy) / det
                r4, r5, r8 = (Dxx * Dss - Dxs * Dxs) / det, (Dxs * Dxy - Dxx * Dys) / det, (Dxx * Dyy - Dxy * Dxy) / det
                fx = r0 * -Dx + r1 * -Dy + r2 * -Ds
                fy = r1 * -Dx + r4 * -Dy + r5 * -Ds
                fs = r2 * -Dx + r5 * -Dy + r8 * -Ds
                ok &= not (abs(abs(float(fx)) - 0.6) <= margin or abs(abs(float(fy)) - 0.6) <= margin)
                dx = int(fx > T(0.6) and ix < w - 2) - int(fx < T(-0.6) and ix > 1)
                dy = int(fy > T(0.6) and iy < h - 2) - int(fy < T(-0.6) and iy > 1)
                if dx == 0 and dy == 0:
                    break
                ix += dx
                iy += dy
            val = d1[iy, ix] + half * (Dx * fx + Dy * fy + Ds * fs)
            tr, hdet = Dxx + Dyy, Dxx * Dyy - Dxy * Dxy
            score = tr * tr / hdet
            kx, ky, ksm = T(ix) + fx, T(iy) + fy, T(s) + fs
            reject = (abs(val) < contrast or score < 0 or score > thres or abs(fx) > 1.5 or abs(fy) > 1.5 or abs(fs) > 1.0
                      or ksm < -1.0 or ksm > S or kx < 0 or kx > w - 1 or ky < 0 or ky > h - 1
                      or not (fx == fx and fy == fy and fs == fs))
            v = [float(q) for q in (val, score, fx, fy, fs, kx, ky, ksm)]
            if not all(np.isfinite(v)):
                ok &= bool(reject) and np.isfinite(v[2:5]).all()      # a score of +-inf or nan (hdet = 0) rejects either way
            else:
                ok &= not (abs(abs(v[0]) - float(contrast)) <= margin * float(contrast)
                           or abs(v[1]) <= margin or abs(v[1] - float(thres)) <= margin * float(thres)
                           or abs(abs(v[2]) - 1.5) <= margin or abs(abs(v[3]) - 1.5) <= margin or abs(abs(v[4]) - 1.0) <= margin
                           or abs(v[7] + 1.0) <= margin or abs(v[7] - S) <= margin * max(1.0, S)
                           or abs(v[5]) <= margin or abs(v[5] - (w - 1)) <= margin * max(1.0, w - 1)
                           or abs(v[6]) <= margin or abs(v[6] - (h - 1)) <= margin * max(1.0, h - 1))
            loc[n] = (v[5], v[6], v[7], 0.0 if reject else 1.0)
            decisive[n] = ok
    return loc, decisive
