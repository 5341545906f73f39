"""Generates tests/golden/m1_mixed_8views*.npz from the REAL reference (oracle/_ref, built by oracle/Makefile
from /root/reference).  Run in the authoring container only:

    python tests/golden/make_golden_mixed.py

Scene M1 (mve_amd.synth.make_mixed_scene): the smooth height field under eight UNLIKE cameras -- a portrait view,
pixel aspect 1.25, an off-centre principal point on odd sizes, a view of twice the sampling density whose mip level
flips between 0 and 1 across ONE reference image, rolls of 90 and 180 degrees, a close view that is sampled at level
2, and a view with two pyramid levels only that the rule wants at level 2 (the clamp of single_view.h:112-123).

Three files, each below one MiB (tests/test_mixed_cameras.py loads them as one dictionary):
  m1_mixed_8views.npz          the scene (images as img_0 ... img_7: their sizes differ) and the reference's global view
                               selection of every view (`gvs` mode of oracle/ref_patch_driver.cc) with globalVSMax 20 and 3
  m1_mixed_8views_maps.npz     the reference's depth / conf / dz maps of views 0, 1, 4 at scale 0 and of view 2 at scale 1
  m1_mixed_8views_patches.npz  `eval` and `opt` dumps of the reference's own PatchSampler / PatchOptimization for
                               reference views 0 and 1; half of the `opt` hypotheses carry a propagated local view set

A scene that is degenerate for the reference proves nothing: the coverage conditions are asserted before anything is
written, and printed.
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import run_maps  # noqa: E402
from mve_amd.scene_io import write_scene  # noqa: E402
from mve_amd.synth import MIXED_SURFACE, _calib, make_mixed_scene, pixel_rays, project, true_depth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
NAME = "m1_mixed_8views"
MAPS = ((0, 0), (1, 0), (4, 0), (2, 1))          # (reference view, scale)
N_HYP = {0: 120, 1: 84}                          # hypotheses per reference view (each dumped in `eval` and in `opt` mode)


def save_npz(path, arrays):
    """np.savez_compressed with fixed entry times: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in arrays.items():
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            with z.open(zi, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def mixed_scene_arrays(sc):
    g = dict(cams=np.stack([c.as_f32() for c in sc.cameras]))
    for i, im in enumerate(sc.images):
        g["img_%d" % i] = im
    g["fpos"] = np.asarray([f.pos for f in sc.features], np.float32)
    foff = np.zeros(len(sc.features) + 1, np.int32)
    foff[1:] = np.cumsum([len(f.view_ids) for f in sc.features])
    g["foff"] = foff
    g["fref"] = np.asarray([v for f in sc.features for v in f.view_ids], np.int32)
    return g


def surface_points(sc, ref):
    """World points of the true surface behind every pixel of view `ref`, and its true radial depth."""
    h, w = sc.images[ref].shape[:2]
    td = true_depth(MIXED_SURFACE, sc.cameras[ref], w, h).astype(np.float64)
    rays = pixel_rays(sc.cameras[ref], w, h)
    rays /= np.linalg.norm(rays, axis=-1, keepdims=True)
    return sc.cameras[ref].position() + rays * td[..., None], td


def border_distance(sc, v, pts):
    """Distance [px, level 0] of the projections of `pts` into view v from its image border (negative: outside)."""
    h, w = sc.images[v].shape[:2]
    u, vv, z = project(sc.cameras[v], w, h, pts.reshape(-1, 3))
    d = np.minimum(np.minimum(u, w - 1 - u), np.minimum(vv, h - 1 - vv))
    return np.where(z > 0, d, -1e9).reshape(pts.shape[:-1])


def unclamped_level(sc, ref, v, p0):
    """patch_sampler.cc:76-90 without the clamp of :91, from footprints in float64."""
    def fp(view):
        cam = sc.cameras[view]
        h, w = sc.images[view].shape[:2]
        z = (np.asarray(cam.rot, np.float64).reshape(3, 3) @ p0 + np.asarray(cam.trans, np.float64))[2]
        return z / _calib(cam, w, h)[0]
    ratio, mm = fp(v) / fp(ref), 0
    if not ratio > 0:
        return -1
    while ratio < 0.5:
        mm += 1
        ratio *= 2.0
    return mm


def make_hypotheses(sc, ref, gvs, n, rng):
    """Pixels and (depth, dzI, dzJ) near the true surface (+-1 % / +-0.01 as scene H1's): a third of them where the patch
    meets a neighbour's image border, a sixth each inside the two close views' small footprints, the rest anywhere."""
    h, w = sc.images[ref].shape[:2]
    P, td = surface_points(sc, ref)
    inner = np.zeros((h, w), bool); inner[2:h - 2, 2:w - 2] = True
    bd = {v: border_distance(sc, v, P) for v in gvs}
    near = np.zeros((h, w), bool)
    for v in gvs:
        near |= (bd[v] > -1.0) & (bd[v] < 3.0)
    pools = [np.argwhere(near & inner)]
    for v in (2, 7):
        pools.append(np.argwhere((bd[v] > (18.0 if v == 7 else 16.0)) & inner) if v in gvs else np.zeros((0, 2), int))
    xs, ys = rng.randint(2, w - 2, n), rng.randint(2, h - 2, n)
    takes = (n // 3, n // 6, n // 6)
    at = 0
    for half in (0, n // 2):                                  # both halves (with / without a propagated set) get every kind
        at = half
        for pool, k in zip(pools, takes):
            k = k // 2
            if len(pool):
                pick = pool[rng.randint(len(pool), size=k)]
                ys[at:at + k], xs[at:at + k] = pick[:, 0], pick[:, 1]
            at += k
    depth = td[ys, xs] * (1.0 + rng.uniform(-0.01, 0.01, n))
    dzi, dzj = rng.uniform(-0.01, 0.01, n), rng.uniform(-0.01, 0.01, n)
    local = np.full((n, 4), -1, np.int32)
    for i in range(n // 2, n):
        seen = [v for v in gvs if bd[v][ys[i], xs[i]] > 4.0]
        hid = [v for v in gvs if bd[v][ys[i], xs[i]] <= 4.0]
        if len(seen) >= 4 and len(hid) >= 1 and i % 3 == 0:       # one view that cannot see the point: it must be replaced
            pick = list(rng.choice(hid, 1)) + list(rng.choice(seen, 3, replace=False))
        elif len(seen) >= 4 and i % 4 == 1:                       # three views only: the fourth is selected beside them
            pick = list(rng.choice(seen, 3, replace=False))       # (local_view_selection.cc:37-38,59-62 with selected views)
        elif len(seen) >= 4:
            pick = list(rng.choice(seen, 4, replace=False))
        else:
            pick = list(rng.choice(gvs, 4, replace=False))
        local[i, :len(pick)] = sorted(int(v) for v in pick)
    n_near = int(near[ys, xs].sum())
    return (np.stack([xs, ys], 1).astype(np.int32), np.stack([depth, dzi, dzj], 1).astype(np.float32), local, n_near, P)


def dump_patches(sdir, ref, gvs, xy, hyp, local):
    n, G = len(xy), len(gvs)
    seeds = [[int(xy[i, 0]), int(xy[i, 1]), float(hyp[i, 0]), float(hyp[i, 1]), float(hyp[i, 2])] + [int(v) for v in local[i] if v >= 0]
             for i in range(n)]
    lines = orc.run_reference_patch_driver(sdir, ref, 0, 4, "opt", seeds)
    assert [int(v) for v in lines[0][1:]] == list(gvs)
    opt = np.zeros((n, 8), np.float32)
    opt_local = np.full((n, 4), -1, np.int32)
    for ln in lines[1:]:
        assert ln[0] == "P"
        i = int(ln[1])
        opt[i, :7] = [np.float32(v) for v in ln[2:9]]
        nl = int(ln[9])
        opt_local[i, :nl] = [int(v) for v in ln[10:10 + nl]]
    lines = orc.run_reference_patch_driver(sdir, ref, 0, 4, "eval", [s[:5] for s in seeds])
    ev = dict(master=np.zeros((n, 5), np.float32), ncc=np.zeros((n, G), np.float32), ok=np.zeros((n, G), np.int32),
              col=np.zeros((n, G, 25, 3), np.float32), der=np.zeros((n, G, 25, 3), np.float32))
    cur = -1
    for ln in lines[1:]:
        if ln[0] == "S":
            cur = int(ln[1])
            ev["master"][cur, 0] = int(ln[2])
            if int(ln[2]):
                ev["master"][cur, 1:5] = [np.float32(v) for v in ln[3:7]]
        else:
            gi = list(gvs).index(int(ln[1]))
            ev["ncc"][cur, gi] = np.float32(ln[2])
            ev["ok"][cur, gi] = int(ln[3])
            if int(ln[3]):
                vals = np.asarray([np.float32(v) for v in ln[4:]], np.float32)
                ev["col"][cur, gi] = vals[:75].reshape(25, 3)
                ev["der"][cur, gi] = vals[75:].reshape(25, 3)
    return opt, opt_local, ev


def main():
    sc = make_mixed_scene()
    nv = sc.n_views
    work = tempfile.mkdtemp(prefix="golden_mixed_")
    sdir = os.path.join(work, "m1")
    write_scene(sdir, sc)
    S = orc.OracleScene(sc)

    # --- the scene and the reference's global view selections
    g = mixed_scene_arrays(sc)
    for v in range(nv):
        for gmax in (20, 3):
            ids = [int(x) for x in orc.run_reference_patch_driver(sdir, v, 0, 4, "gvs", [], global_max=gmax)[0][1:]]
            g["gvs%d_v%d" % (gmax, v)] = np.asarray(ids, np.int32)
        unlike = [x for x in g["gvs20_v%d" % v]
                  if sc.images[x].shape != sc.images[v].shape or tuple(sc.cameras[x].as_f32()[:4]) != tuple(sc.cameras[v].as_f32()[:4])]
        print("view %d: global views %s (%d unlike it), with globalVSMax 3: %s"
              % (v, list(g["gvs20_v%d" % v]), len(unlike), list(g["gvs3_v%d" % v])))
        assert len(unlike) >= 2, v
    assert S.pyramid_levels(7) == 2

    # --- the reference's maps
    gm = {}
    for v, s in MAPS:
        m = run_maps(sdir, s, v, 4)
        fill = float((m["depth"] > 0).mean())
        print("map of view %d at scale %d: %d x %d, filled %.3f" % (v, s, m["depth"].shape[1], m["depth"].shape[0], fill))
        assert fill >= 0.5, (v, s, fill)
        for k, val in m.items():
            gm["s%dv%d_%s" % (s, v, k)] = val

    # --- patch-level dumps of reference views 0 and 1
    gp = {}
    rng = np.random.RandomState(41)
    for ref in (0, 1):
        gvs = [int(x) for x in g["gvs20_v%d" % ref]]
        xy, hyp, local, n_near, P = make_hypotheses(sc, ref, gvs, N_HYP[ref], rng)
        opt, opt_local, ev = dump_patches(sdir, ref, gvs, xy, hyp, local)
        n = len(xy)
        okp = opt[:, 0] > 0
        changed = okp[n // 2:] & (opt_local[n // 2:] != local[n // 2:]).any(1)
        print("view %d: %d hypotheses, %d within 3 px of a neighbour's border; opt: %d succeed, %d of %d propagated sets re-selected"
              % (ref, n, n_near, okp.sum(), changed.sum(), n - n // 2))
        print("view %d: eval (hypothesis, view) pairs: %d succeed, %d fail (patch_sampler.cc:116-119 / behind the view)"
              % (ref, int(ev["ok"].sum()), int(((ev["ok"] == 0) & (ev["master"][:, :1] > 0)).sum())))
        # the oracle's level per (hypothesis, view), and the rule without its clamp from float64 footprints
        st = orc.make_settings(ref_view=ref)
        lvl = np.full((n, len(gvs)), -1, np.int32)
        raw = np.full((n, len(gvs)), -1, np.int32)
        for i in range(n):
            e = S.patch_eval(st, int(xy[i, 0]), int(xy[i, 1]), float(hyp[i, 0]), float(hyp[i, 1]), float(hyp[i, 2]))
            if len(e["level"]):
                lvl[i] = e["level"]
            h, w = sc.images[ref].shape[:2]
            ray = pixel_rays(sc.cameras[ref], w, h, np.asarray(xy[i, 0]), np.asarray(xy[i, 1]))
            p0 = sc.cameras[ref].position() + ray / np.linalg.norm(ray) * float(hyp[i, 0])
            raw[i] = [unclamped_level(sc, ref, v, p0) for v in gvs]
        seen = {v: sorted(set(int(x) for x in lvl[:, gi] if x >= 0)) for gi, v in enumerate(gvs)}
        n_clamp = int(((lvl[:, gvs.index(7)] == 1) & (raw[:, gvs.index(7)] >= 2)).sum()) if 7 in gvs else 0
        print("view %d: levels sampled per neighbour %s; view 7 clamped from level >= 2 to its last level 1 on %d hypotheses" % (ref, seen, n_clamp))
        assert n_near >= 20 * (2 if ref == 0 else 1)
        if ref == 0:
            assert set(x for s in seen.values() for x in s) >= {0, 1, 2} and seen[3] == [0, 1], seen
            assert n_clamp >= 10, n_clamp
            assert int(((ev["ok"] == 0) & (ev["master"][:, :1] > 0)).sum()) >= 20 and int(ev["ok"].sum()) >= 100
        for k, val in dict(seeds_xy=xy, seeds_hyp=hyp, seeds_local=local, opt=opt, opt_local=opt_local, ev_master=ev["master"],
                           ev_ncc=ev["ncc"], ev_ok=ev["ok"], ev_col=ev["col"], ev_der=ev["der"], ev_rawlvl=raw).items():
            gp["v%d_%s" % (ref, k)] = val

    total = 0
    for suffix, d in (("", g), ("_maps", gm), ("_patches", gp)):
        path = os.path.join(OUT, NAME + suffix + ".npz")
        save_npz(path, d)
        print(os.path.basename(path), os.path.getsize(path) // 1024, "KiB")
        assert os.path.getsize(path) < 1 << 20
        total += os.path.getsize(path)
    assert total <= os.path.getsize(os.path.join(OUT, "w2_wider_100views_96x72.npz"))
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
