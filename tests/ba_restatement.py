"""A plain NumPy float64 restatement of sfm::ba::BundleAdjustment (libs/sfm/bundle_adjustment.cc, ba_linear_solver.cc,
ba_conjugate_gradient.h): residuals, both Jacobian forms, the parameter update, the LM loop, and the linear step two ways --
a dense solve of the damped normal equations, and the Schur complement with preconditioned CG as the reference runs it.
Also the synthetic scenes of tests/test_ba.py and tests/golden/make_golden_ba.py.

A problem is a dict: cams (n, 15) rows f k0 k1 t[3] R[9]; pts (m, 3); const (m,) bool; xy (o, 2); cam, pt (o,) int."""
import numpy as np

CAMERAS, POINTS, BOTH = 1, 2, 3
DBL_EPS = 2.2250738585072014e-308 * 1e58                                  # MATH_DBL_EPS (libs/math/defines.h:90)


def project(cams, pts, oc, op):
    c, X = cams[oc], pts[op]
    r = np.einsum("nij,nj->ni", c[:, 6:].reshape(-1, 3, 3), X)
    p = r + c[:, 3:6]
    ix, iy = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    r2 = ix * ix + iy * iy
    rd = 1.0 + r2 * (c[:, 1] + c[:, 2] * r2)
    return c, r, p[:, 2], ix, iy, r2, rd


def residuals(P, cams, pts):
    c, _, _, ix, iy, _, rd = project(cams, pts, P["cam"], P["pt"])
    return np.stack([ix * rd * c[:, 0] - P["xy"][:, 0], iy * rd * c[:, 0] - P["xy"][:, 1]], 1)


def mse(F):
    return float((F * F).sum() / len(F))


def jacobian(P, cams, pts, fixed):
    """Jc (o, 2, D) and Jp (o, 2, 3): analytic_jacobian_entries (bundle_adjustment.cc:381-635)."""
    c, r, pz, ix, iy, r2, rd = project(cams, pts, P["cam"], P["pt"])
    f, R = c[:, 0], c[:, 6:]
    rx, ry, rz = r.T
    o = len(f)
    if fixed:                                                             # :438-465
        g = f / pz * rd
        z = np.zeros(o)
        jx = [g, z, -g * ix, -g * ry * ix, g * (rz + rx * ix), -g * ry]
        jy = [z, g, -g * iy, -g * (rz + ry * iy), g * rx * iy, g * rx]
        px = [g * (R[:, k] - R[:, 6 + k] * ix) for k in range(3)]
        py = [g * (R[:, 3 + k] - R[:, 6 + k] * iy) for k in range(3)]
    else:                                                                 # :467-474, :544-632
        rdp = c[:, 1] + 2.0 * c[:, 2] * r2

        def chain(a, b):
            drd = rdp * (2.0 * ix * a + 2.0 * iy * b)
            return f * (drd * ix + rd * a), f * (drd * iy + rd * b)
        z = np.zeros(o)
        ext = [chain(1 / pz, z), chain(z, 1 / pz), chain(-ix / pz, -iy / pz),
               chain(-ix * ry / pz, -(rz + ry * iy) / pz), chain((rz + rx * ix) / pz, rx * iy / pz), chain(-ry / pz, rx / pz)]
        jx = [ix * rd, f * ix * r2, f * ix * r2 * r2] + [e[0] for e in ext]
        jy = [iy * rd, f * iy * r2, f * iy * r2 * r2] + [e[1] for e in ext]
        pp = [chain((R[:, k] - R[:, 6 + k] * ix) / pz, (R[:, 3 + k] - R[:, 6 + k] * iy) / pz) for k in range(3)]
        px, py = [e[0] for e in pp], [e[1] for e in pp]
    Jc = np.stack([np.stack(jx, 1), np.stack(jy, 1)], 1)
    Jp = np.stack([np.stack(px, 1), np.stack(py, 1)], 1)
    Jp[P["const"][P["pt"]]] = 0.0                                         # :334-338
    return Jc, Jp


def rodrigues(r):
    a = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    ct = 0.5 if a == 0.0 else (1.0 - np.cos(a)) / (a * a)
    st = 1.0 if a == 0.0 else np.sin(a) / a
    return np.array([[1.0 - (r[1] * r[1] + r[2] * r[2]) * ct, r[0] * r[1] * ct - r[2] * st, r[2] * r[0] * ct + r[1] * st],
                     [r[0] * r[1] * ct + r[2] * st, 1.0 - (r[2] * r[2] + r[0] * r[0]) * ct, r[1] * r[2] * ct - r[0] * st],
                     [r[2] * r[0] * ct - r[1] * st, r[1] * r[2] * ct + r[0] * st, 1.0 - (r[0] * r[0] + r[1] * r[1]) * ct]])


def update(cams, pts, dy, dz, fixed):
    """update_camera / update_point (:662-697); dy (n, D) or None, dz (m, 3) or None."""
    cams, pts = cams.copy(), pts.copy()
    if dy is not None:
        off = 0 if fixed else 3
        if not fixed:
            cams[:, :3] += dy[:, :3]
        cams[:, 3:6] += dy[:, off:off + 3]
        for i in range(len(cams)):
            cams[i, 6:] = (rodrigues(dy[i, off + 3:off + 6]) @ cams[i, 6:].reshape(3, 3)).ravel()
    if dz is not None:
        pts += dz
    return cams, pts


def blocks(P, Jc, Jp, F, n, m):
    """B (n, D, D), C (m, 3, 3), v (n, D), w (m, 3), summed in observation order."""
    D = Jc.shape[2]
    B, C, v, w = np.zeros((n, D, D)), np.zeros((m, 3, 3)), np.zeros((n, D)), np.zeros((m, 3))
    np.add.at(B, P["cam"], np.einsum("oij,oik->ojk", Jc, Jc))
    np.add.at(C, P["pt"], np.einsum("oij,oik->ojk", Jp, Jp))
    np.add.at(v, P["cam"], -np.einsum("oij,oi->oj", Jc, F))
    np.add.at(w, P["pt"], -np.einsum("oij,oi->oj", Jp, F))
    return B, C, v, w


def invert_3x3(C):
    """invert_block_matrix_3x3_inplace (ba_linear_solver.cc:60-84): a block with |det| <= MATH_DBL_EPS stays as it is."""
    out = C.copy()
    for i, c in enumerate(C):
        det = np.linalg.det(c)
        if not (-DBL_EPS <= det <= DBL_EPS):
            out[i] = np.linalg.inv(c)
    return out


def cg(A, b, precond, max_iterations):
    """ConjugateGradient::solve (ba_conjugate_gradient.h:132-210); A and precond are functions."""
    x, r = np.zeros_like(b), b.copy()
    z = precond(r)
    rz, d = z @ r, z.copy()
    for it in range(max_iterations):
        Ad = A(d)
        alpha = rz / (d @ Ad)
        x = x + alpha * d
        r = r - alpha * Ad
        if r @ r < 1e-20:
            return x, it
        z = precond(r)
        new = z @ r
        d = z + (new / rz) * d
        rz = new
    return x, max_iterations


def scale_diag(M, s):
    M = M.copy()
    i = np.arange(M.shape[1])
    M[:, i, i] *= s
    return M


def step_schur(P, Jc, Jp, F, n, m, mode, radius, cg_max):
    """LinearSolver::solve_schur / solve (ba_linear_solver.cc:141-313).  Returns dy, dz, predicted decrease, CG iterations."""
    B, C, v, w = blocks(P, Jc, Jp, F, n, m)
    D = Jc.shape[2]
    reg = 1.0 + 1.0 / radius
    Bd, Cd = np.einsum("nii->ni", B).copy(), np.einsum("nii->ni", C).copy()
    if mode == POINTS:
        dz = np.einsum("mij,mj->mi", invert_3x3(scale_diag(C, reg)), w)
        return None, dz, float((dz * (Cd * dz * (1.0 / radius) + w)).sum()), 0
    Br = scale_diag(B, reg)
    if mode == CAMERAS:
        pre = 1.0 / np.einsum("nii->ni", Br)
        dy, it = cg(lambda d: np.einsum("nij,nj->ni", Br, d.reshape(n, D)).ravel(), v.ravel(), lambda r: pre.ravel() * r, cg_max)
        dy = dy.reshape(n, D)
        return dy, None, float((dy * (Bd * dy * (1.0 / radius) + v)).sum()), it
    Ci = invert_3x3(scale_diag(C, reg))
    E = np.zeros((n * D, m * 3))
    for o in range(len(F)):
        c, p = P["cam"][o], P["pt"][o]
        E[c * D:(c + 1) * D, p * 3:(p + 1) * 3] += Jc[o].T @ Jp[o]
    Cfull = np.zeros((m * 3, m * 3))
    Bfull = np.zeros((n * D, n * D))
    Pfull = np.zeros((n * D, n * D))
    for p in range(m):
        Cfull[p * 3:(p + 1) * 3, p * 3:(p + 1) * 3] = Ci[p]
    for c in range(n):
        Bfull[c * D:(c + 1) * D, c * D:(c + 1) * D] = Br[c]
        Li = np.linalg.inv(np.linalg.cholesky(Br[c]))                     # cholesky_invert_inplace (ba_cholesky.h:59-68)
        inv = Li.T @ Li
        Pfull[c * D:(c + 1) * D, c * D:(c + 1) * D] = np.where(np.isfinite(inv), inv, 0.0)
    S = Bfull - E @ Cfull @ E.T
    rhs = v.ravel() - E @ (Cfull @ w.ravel())
    dy, it = cg(lambda d: S @ d, rhs, lambda r: Pfull @ r, cg_max)
    dz = (Cfull @ (w.ravel() - E.T @ dy)).reshape(m, 3)
    dy = dy.reshape(n, D)
    pred = float((dy * (Bd * dy * (1.0 / radius) + v)).sum()) + float((dz * (Cd * dz * (1.0 / radius) + w)).sum())
    return dy, dz, pred, it


def step_dense(P, Jc, Jp, F, n, m, mode, radius, cg_max):
    """(H + diag(H) / radius) delta = -J^T F by a dense solve; columns whose diagonal is zero (constant points, points
    without observations) are removed and get a zero step."""
    D, o = Jc.shape[2], len(F)
    nc = n * D if mode & CAMERAS else 0
    J = np.zeros((2 * o, nc + (m * 3 if mode & POINTS else 0)))
    for i in range(o):
        c, p = P["cam"][i], P["pt"][i]
        if mode & CAMERAS:
            J[2 * i:2 * i + 2, c * D:(c + 1) * D] = Jc[i]
        if mode & POINTS:
            J[2 * i:2 * i + 2, nc + p * 3:nc + (p + 1) * 3] = Jp[i]
    H, g = J.T @ J, -J.T @ F.ravel()
    diag = np.diag(H).copy()
    keep = diag > 0.0
    delta = np.zeros(len(g))
    delta[keep] = np.linalg.solve((H + np.diag(diag / radius))[np.ix_(keep, keep)], g[keep])
    pred = float(delta @ (diag * delta * (1.0 / radius) + g))
    dy = delta[:nc].reshape(n, D) if mode & CAMERAS else None
    dz = delta[nc:].reshape(m, 3) if mode & POINTS else None
    return dy, dz, pred, 0


DEFAULTS = dict(bundle_mode=BOTH, fixed_intrinsics=False, lm_max_iterations=50, lm_min_iterations=0, lm_delta_threshold=1e-4,
                lm_mse_threshold=1e-8, cg_max_iterations=1000)


def optimize(P, step=step_schur, **options):
    """lm_optimize (bundle_adjustment.cc:73-201).  Returns cams, pts, status dict, trace list of (mse before, mse after, CG
    iterations, radius, accepted)."""
    o = dict(DEFAULTS, **options)
    mode, fixed = o["bundle_mode"], bool(o["fixed_intrinsics"])
    cams, pts = P["cams"].copy(), P["pts"].copy()
    n, m = len(cams), len(pts)
    radius = 1000.0
    F = residuals(P, cams, pts)
    cur = mse(F)
    st = dict(initial_mse=cur, final_mse=cur, num_lm_iterations=0, num_lm_successful_iterations=0, num_lm_unsuccessful_iterations=0,
              num_cg_iterations=0)
    trace = []
    it = 0
    while True:
        if it + 1 > o["lm_min_iterations"] and cur < o["lm_mse_threshold"]:
            break
        Jc, Jp = jacobian(P, cams, pts, fixed)
        dy, dz, pred, cgi = step(P, Jc, Jp, F, n, m, mode, radius, o["cg_max_iterations"])
        ncams, npts = update(cams, pts, dy, dz, fixed)
        Fn = residuals(P, ncams, npts)
        new = mse(Fn)
        delta, ratio = cur - new, 1.0 - new / cur
        st["num_cg_iterations"] += cgi
        ok = delta > 0.0
        trace.append((cur, new, cgi, radius, ok))
        st["num_lm_iterations"] += 1
        if ok:
            st["num_lm_successful_iterations"] += 1
            cams, pts, F, cur = ncams, npts, Fn, new
            gain = delta * len(F) / pred
            radius *= 1.0 / max(1.0 / 3.0, 1.0 - (2.0 * gain - 1.0) ** 3)
        else:
            st["num_lm_unsuccessful_iterations"] += 1
            radius *= 0.5
        it += 1
        if it < o["lm_min_iterations"]:
            continue
        if it >= o["lm_max_iterations"]:
            break
        if ok and ratio < o["lm_delta_threshold"]:
            break
    st["final_mse"] = cur
    return cams, pts, st, trace


def make_scene(n_cams, tracks, seed, noise=5e-4, perturb=1e-2, distortion=(0.0, 0.0), const=(), big_start=False):
    """Cameras on an arc of radius 4 looking at the origin, points in a cloud of size 1 around it.  ``tracks``: per point the
    list of cameras that see it (an empty list: a point without observations).  Observations are the exact projections plus
    pixel noise; the initial parameters are the true ones perturbed by ``perturb`` (relative to the scene size).  ``big_start``
    moves the points a hundred times further, so that the first full step overshoots and is rejected."""
    rng = np.random.default_rng(seed)
    m = len(tracks)
    pts = rng.uniform(-0.5, 0.5, (m, 3))
    cams = np.zeros((n_cams, 15))
    for i in range(n_cams):
        a = (i - (n_cams - 1) / 2.0) * (1.6 / max(n_cams, 2)) + 0.05
        centre = np.array([4.0 * np.sin(a), 0.3 * np.cos(3.0 * i), -4.0 * np.cos(a)])
        zax = -centre / np.linalg.norm(centre)
        xax = np.cross([0.0, 1.0, 0.0], zax)
        xax /= np.linalg.norm(xax)
        R = np.stack([xax, np.cross(zax, xax), zax])
        cams[i] = np.concatenate([[1.1 + 0.01 * i, distortion[0], distortion[1]], -R @ centre, R.ravel()])
    oc = np.array([c for t in tracks for c in t], np.int32)
    op = np.array([p for p, t in enumerate(tracks) for _ in t], np.int32)
    P = dict(cam=oc, pt=op, const=np.zeros(m, bool), xy=np.zeros((len(oc), 2)))
    P["const"][list(const)] = True
    P["xy"] = residuals(P, cams, pts) + rng.normal(0.0, noise, (len(oc), 2))
    scale = 100.0 if big_start else 1.0
    P["pts"] = pts + perturb * scale * rng.normal(0.0, 1.0, (m, 3)) * ~P["const"][:, None]
    d = perturb * rng.normal(0.0, 1.0, (n_cams, 9))
    cams0 = cams.copy()
    cams0[:, 0] *= 1.0 + d[:, 0]
    cams0[:, 3:6] += d[:, 3:6]
    for i in range(n_cams):
        cams0[i, 6:] = (rodrigues(d[i, 6:9]) @ cams[i, 6:].reshape(3, 3)).ravel()
    P["cams"] = cams0
    return P


def shuffled(P, seed):
    """The same problem with its observations in another order."""
    order = np.random.default_rng(seed).permutation(len(P["cam"]))
    return dict(P, cam=P["cam"][order], pt=P["pt"][order], xy=P["xy"][order])


def scene(name):
    """The scenes of the tests, smallest first: what each is for stands beside it."""
    if name == "c1":                                                      # the bundler's single new camera
        return make_scene(1, [[0]] * 40, 11)
    if name == "c2":                                                      # 63 points, every track sees all cameras
        return make_scene(2, [[0, 1]] * 63, 12)
    if name == "c3":                                  # 64 points; tracks of 1, 2 and 3; a constant point, an unseen one; distortion
        tracks = [[0, 1, 2] if i % 3 == 0 else [i % 3, (i + 1) % 3] if i % 3 == 1 else [2] for i in range(64)]
        tracks[5] = []
        return make_scene(3, tracks, 13, distortion=(0.05, -0.02), const=(7,))
    if name == "c33":                                                     # 65 points, more cameras than a wavefront half
        return make_scene(33, [list(range(33))] * 65, 14)
    if name == "edge":                                # cameras with 255, 256 and 257 observations: around the workgroup size
        return make_scene(3, [[0, 1, 2] if i < 255 else [1, 2] if i < 256 else [2] for i in range(257)], 15)
    if name == "wide":                                                    # 513 observations per camera: three strides
        return make_scene(2, [[0, 1]] * 513, 16)
    if name == "reject":                                                  # a start so far off that a step is rejected
        return make_scene(3, [[0, 1, 2]] * 64, 19, big_start=True)
    raise KeyError(name)
