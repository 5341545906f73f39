"""Scene M1: eight UNLIKE cameras on one scene (tests/golden/make_golden_mixed.py, mve_amd.synth.make_mixed_scene).

Every other fixture uses one camera model: pixel aspect 1, a centred principal point, focal length 1, landscape images
of one size per scene, no roll, all views at one distance.  M1 has a portrait view (the image_aspect < 1 branch of
libs/mve/camera.cc:124-144), pixel aspect 1.25, an off-centre principal point on odd sizes (image_pyramid.cc:39-44),
a 320 x 240 view among 160 x 120 ones whose mip level flips between 0 and 1 across one reference image
(patch_sampler.cc:85-91), rolls of 90 and 180 degrees, a close view sampled at level 2 and a close view with two
pyramid levels that the rule wants at level 2 (SingleView::clampLevel, single_view.h:112-123).

The fixture comes from the compiled reference.  CPU tests: the restatement (oracle/dmrecon_oracle.cc) reproduces it bit
for bit.  GPU tests (marked gpu): the HIP path against the fixture and the restatement at the project's stated
tolerances (tests/test_gpu_parity.py docstring).

A view smaller than 30 pixels is not in the fixture: the reference never gives such a view an image (the loop of
image_pyramid.cc:78 does not run once) and crashes when it samples it.  The library and the restatement do serve one
(a single level, every level request clamped to 0); that case is checked between the two of them only.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, map_parity
from oracle import oracle as orc

MAPS = ((0, 0), (1, 0), (4, 0), (2, 1))          # (reference view, scale) of the fixture's maps
MAP_TOL = dict(iou=0.98, rel_med=1e-3, rel_p99=5e-3, conf_med=1e-3, conf_p99=5e-3)      # tests/test_gpu_parity.py


def load_m1():
    g = {}
    for part in ("", "_maps", "_patches"):
        g.update(np.load(os.path.join(GOLDEN, "m1_mixed_8views%s.npz" % part)))
    return g


def scene_of(g):
    """conftest.scene_from_golden for images of unlike sizes (keys img_0 ... img_7)."""
    from mve_amd.scene_io import Camera, Feature, SceneData
    cams = [Camera(flen=float(c[0]), paspect=float(c[1]), ppoint=[float(c[2]), float(c[3])], rot=[float(v) for v in c[4:13]],
                   trans=[float(v) for v in c[13:16]]) for c in g["cams"]]
    imgs = [np.ascontiguousarray(g["img_%d" % i]) for i in range(len(cams))]
    off, ref = g["foff"], g["fref"]
    feats = [Feature([float(v) for v in g["fpos"][i]], [int(v) for v in ref[off[i]:off[i + 1]]]) for i in range(len(g["fpos"]))]
    return SceneData(cams, imgs, feats)


@pytest.fixture(scope="module")
def m1():
    return load_m1()


@pytest.fixture(scope="module")
def m1_scene(m1):
    return scene_of(m1)


@pytest.fixture(scope="module")
def m1_oracle(m1_scene):
    return orc.OracleScene(m1_scene)


@pytest.fixture(scope="module")
def m1_oracle_eval(m1, m1_oracle):
    """The restatement's PatchSampler values (with its mip level per view) for the fixture's hypotheses, computed once."""
    out = {}
    for ref in (0, 1):
        st = orc.make_settings(ref_view=ref)
        out[ref] = [m1_oracle.patch_eval(st, int(x), int(y), float(h[0]), float(h[1]), float(h[2]))
                    for (x, y), h in zip(m1["v%d_seeds_xy" % ref], m1["v%d_seeds_hyp" % ref])]
    return out


# ---- CPU: the fixture itself, and the restatement against it ------------------------------------------------------

def test_fixture_covers_what_it_is_for(m1, m1_scene):
    sizes = [im.shape[1::-1] for im in m1_scene.images]
    assert sizes == [(160, 120), (120, 160), (161, 121), (320, 240), (160, 120), (96, 72), (160, 120), (100, 56)]
    c = m1_scene.cameras
    assert c[1].flen == pytest.approx(1.1) and c[4].paspect == 1.25 and c[6].flen == pytest.approx(0.85)
    assert tuple(np.float32(c[2].ppoint)) == (np.float32(0.46), np.float32(0.55))
    for v, s in MAPS:
        assert (m1["s%dv%d_depth" % (s, v)] > 0).mean() >= 0.5, (v, s)
    for v in range(8):
        unlike = [x for x in m1["gvs20_v%d" % v] if sizes[x] != sizes[v] or tuple(m1["cams"][x][:4]) != tuple(m1["cams"][v][:4])]
        assert len(unlike) >= 2 and len(m1["gvs3_v%d" % v]) == 3


def test_mixed_scene_maps_bit_exact(m1, m1_oracle):
    for v, s in MAPS:
        r = m1_oracle.reconstruct(orc.make_settings(ref_view=v, scale=s))
        for k in ("depth", "conf", "dz"):
            assert np.array_equal(r[k], m1["s%dv%d_%s" % (s, v, k)]), (v, s, k)
    assert np.array_equal(m1_oracle.pyramid_level(2, 1)[0], m1["s1v2_undist"])      # the reference's own "undist-L1"


def test_mixed_scene_view_selection_exact(m1, m1_oracle):
    for v in range(8):
        for gmax in (20, 3):
            assert m1_oracle.global_vs(orc.make_settings(ref_view=v, global_max=gmax)) == list(m1["gvs%d_v%d" % (gmax, v)]), (v, gmax)


def test_mixed_scene_patch_sampler_exact(m1, m1_oracle_eval):
    """`eval` dumps of the reference's PatchSampler for reference views 0 (plain) and 1 (portrait): success per view, master
    mean colour and patch normal, NCC, colours and derivatives, all bit for bit; and the mip levels behind them: 0, 1 and 2 from
    view 0, both 0 and 1 for the 320 x 240 view alone, and the clamp to the last level of view 7."""
    for ref in (0, 1):
        gvs = list(m1["gvs20_v%d" % ref])
        n_ok = n_fail = 0
        lvl = np.full((len(m1_oracle_eval[ref]), len(gvs)), -1)
        for i, e in enumerate(m1_oracle_eval[ref]):
            assert e["master"][0] == m1["v%d_ev_master" % ref][i, 0], (ref, i)
            if not e["master"][0]:
                continue
            assert np.array_equal(e["master"][1:], m1["v%d_ev_master" % ref][i, 1:]), (ref, i)
            assert np.array_equal(e["ok"], m1["v%d_ev_ok" % ref][i]), (ref, i)
            assert np.array_equal(e["ncc"], m1["v%d_ev_ncc" % ref][i]), (ref, i)
            okv = e["ok"] > 0
            assert np.array_equal(e["col"][okv], m1["v%d_ev_col" % ref][i][okv]), (ref, i)
            assert np.array_equal(e["deriv"][okv], m1["v%d_ev_der" % ref][i][okv]), (ref, i)
            lvl[i] = np.where(okv, e["level"], -1)
            n_ok += int(okv.sum()); n_fail += int((~okv).sum())
        assert n_ok >= 100 and n_fail >= 20, (ref, n_ok, n_fail)
        check_level_coverage(lvl, m1["v%d_ev_rawlvl" % ref], gvs, ref)


def check_level_coverage(lvl, raw, gvs, ref):
    """lvl: the level each successfully sampled (hypothesis, view) was drawn from (-1 elsewhere); raw: the rule without its clamp
    from float64 footprints (the generator's).  The conditions the generator asserted on the restatement's levels."""
    seen = {v: set(int(x) for x in lvl[:, gi] if x >= 0) for gi, v in enumerate(gvs)}
    if ref == 0:
        assert set().union(*seen.values()) >= {0, 1, 2}, seen
        assert seen[3] == {0, 1}, seen                       # the rule flips across the image of ONE reference view
    g7 = gvs.index(7)
    assert seen[7] == {1} and ((lvl[:, g7] == 1) & (raw[:, g7] >= 2)).sum() >= 10       # the clamp fired
    on = lvl >= 0
    assert (np.minimum(raw, 1)[:, g7][on[:, g7]] == lvl[:, g7][on[:, g7]]).all()
    for gi, v in enumerate(gvs):
        if v != 7:                                           # every other view has the level the rule asks for
            assert (raw[:, gi][on[:, gi]] == lvl[:, gi][on[:, gi]]).all(), v


def test_mixed_scene_patch_optimization_exact(m1, m1_oracle):
    for ref in (0, 1):
        xy, hyp, local = m1["v%d_seeds_xy" % ref], m1["v%d_seeds_hyp" % ref], m1["v%d_seeds_local" % ref]
        out, loc = m1_oracle.patch_optimize(orc.make_settings(ref_view=ref), xy, hyp, local)
        want, want_loc = m1["v%d_opt" % ref], m1["v%d_opt_local" % ref]
        ok = want[:, 0] > 0
        assert np.array_equal(out[:, 0] > 0, ok) and ok.sum() >= 40 and (~ok).sum() >= 20, ref
        assert np.array_equal(out[ok, :7], want[ok, :7]) and np.array_equal(loc[ok], want_loc[ok]), ref
        n = len(want)
        changed = ok[n // 2:] & (want_loc[n // 2:] != local[n // 2:]).any(1)
        assert changed.sum() >= 3, ref                       # propagated sets the reference completed / re-selected


# the worst of four other queue orders per map (test_order_sensitivity_floors_on_mixed_scene measures them again)
ORDER_FLOOR = {
    (0, 0): dict(iou=0.9996, rel_med=1.88e-4, rel_p99=4.78e-3, conf_med=7.40e-5, conf_p99=0.0638),
    (1, 0): dict(iou=0.9990, rel_med=2.00e-4, rel_p99=3.91e-3, conf_med=1.04e-4, conf_p99=0.0789),
    (4, 0): dict(iou=0.9998, rel_med=1.65e-4, rel_p99=2.94e-3, conf_med=2.27e-4, conf_p99=0.0460),
    (2, 1): dict(iou=0.9998, rel_med=9.45e-4, rel_p99=8.82e-3, conf_med=2.34e-3, conf_p99=0.144),
}


def map_bound(v, s, k):
    """The general map-level bound where the algorithm's own order floor leaves room for it, twice the floor where it does not."""
    floor, general = ORDER_FLOOR[(v, s)][k], MAP_TOL[k]
    if k == "iou":
        return general if floor >= general else 1.0 - 2.0 * (1.0 - floor)
    return general if floor <= general else 2.0 * floor


def test_order_sensitivity_floors_on_mixed_scene(m1):
    """The reference ALGORITHM against itself on M1's four maps: the restatement with its queue popped in another valid order
    (ORC_QUEUE_ORDER = reverse, random:1, random:2, jitter:1; a subprocess, as the floor tests of tests/test_oracle_golden.py)
    against the reference binary's maps.  The floor the map-level bounds of test_mixed_scene_maps are set against.  Measured
    (worst of the four orders; fill IoU, relative depth p99, confidence p99; the medians behind):

      view 0, scale 0 (160 x 120):  0.9996   4.78e-3   0.0638      (relative depth median 1.9e-4, confidence median 7.4e-5)
      view 1, scale 0 (120 x 160):  0.9990   3.91e-3   0.0789      (2.0e-4, 1.0e-4)
      view 4, scale 0 (160 x 120):  0.9998   2.94e-3   0.046       (1.7e-4, 2.3e-4)
      view 2, scale 1 (81 x 61):    0.9998   8.82e-3   0.144       (9.5e-4, 2.3e-3)
    """
    import tempfile
    code = ("import os, sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_mixed_cameras import load_m1, scene_of, MAPS\nfrom oracle import oracle as orc\n"
            "S = orc.OracleScene(scene_of(load_m1()))\nout = {}\n"
            "for o in ('reverse', 'random:1', 'random:2', 'jitter:1'):\n"
            "    os.environ['ORC_QUEUE_ORDER'] = o\n"
            "    for v, s in MAPS:\n"
            "        r = S.reconstruct(orc.make_settings(ref_view=v, scale=s))\n"
            "        out['%%s_%%d_d' %% (o, v)] = r['depth']; out['%%s_%%d_c' %% (o, v)] = r['conf']\n"
            "np.savez(sys.argv[1], **out)\n" % (ROOT, os.path.join(ROOT, "tests")))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "orders.npz")
        subprocess.run([sys.executable, "-c", code, path], check=True)
        got = dict(np.load(path))
    for v, s in MAPS:
        ref_d, ref_c = m1["s%dv%d_depth" % (s, v)], m1["s%dv%d_conf" % (s, v)]
        ms = [map_parity(got["%s_%d_d" % (o, v)], got["%s_%d_c" % (o, v)], ref_d, ref_c) for o in ("reverse", "random:1", "random:2", "jitter:1")]
        assert all(not np.array_equal(got["%s_%d_d" % (o, v)], ref_d) for o in ("reverse", "random:1", "random:2", "jitter:1"))
        worst = {k: (min if k == "iou" else max)(m[k] for m in ms) for k in MAP_TOL}
        print("M1 view %d scale %d: order floor" % (v, s), {k: float("%.3g" % x) for k, x in worst.items()})
        # the restatement is deterministic: the recorded floor is reproduced (to the digits written down)
        for k, x in worst.items():
            want = ORDER_FLOOR[(v, s)][k]
            assert abs(x - want) <= 5e-4 if k == "iou" else abs(x / want - 1) <= 0.02, (v, s, k, x)


# ---- GPU: the HIP path on the same scene ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx_m1(gpu_ctx, m1_scene):
    gpu_ctx.load_scene(m1_scene)
    return gpu_ctx


@pytest.mark.gpu
def test_gpu_pyramid_and_calibration(ctx_m1, m1, m1_oracle):
    """calibration() on the portrait branch, with pixel aspect 1.25 and with the odd-size principal-point rule at 0.46 / 0.55:
    every level of every view has the restatement's bytes, projection and inverse projection."""
    for v in range(8):
        assert ctx_m1.num_levels(v) == m1_oracle.pyramid_levels(v), v
        for lvl in range(ctx_m1.num_levels(v)):
            img, proj, inv = ctx_m1.get_level(v, lvl)
            oimg, oproj, oinv = m1_oracle.pyramid_level(v, lvl)
            assert np.array_equal(img, oimg), (v, lvl)
            assert np.array_equal(proj, oproj) and np.array_equal(inv, oinv), (v, lvl)
    assert ctx_m1.num_levels(7) == 2 and ctx_m1.num_levels(3) == 5
    assert np.array_equal(ctx_m1.get_level(2, 1)[0], m1["s1v2_undist"])             # the reference's own "undist-L1"
    p1, p4 = ctx_m1.get_level(1, 0)[1], ctx_m1.get_level(4, 0)[1]
    assert p1[0] == p1[4] == np.float32(1.1) * 160 and p4[0] == 160 and p4[4] == 200      # camera.cc:133-142


@pytest.mark.gpu
def test_gpu_view_selection(ctx_m1, m1, monkeypatch):
    from mve_amd import api
    for gmax in (20, 3):
        for ref in range(8):
            st = api.Settings(refViewNr=ref, globalVSMax=gmax)
            monkeypatch.setenv("MI_DMRECON_GVS_DEVICE", "0")
            host = ctx_m1.global_view_selection(st)
            monkeypatch.setenv("MI_DMRECON_GVS_DEVICE", "1")
            dev = ctx_m1.global_view_selection(st)
            assert host == dev == list(m1["gvs%d_v%d" % (gmax, ref)]), (gmax, ref)


def check_patch_eval(e, o, want, level_width):
    """One hypothesis: the library's patch_eval `e` against the restatement's `o` (levels) and the reference's dump `want`
    (master, ncc, ok, col, der).  Returns the levels of the successfully sampled views (-1 elsewhere)."""
    assert e["master"][0] == want["master"][0]
    if not e["master"][0]:
        return np.full(len(want["ok"]), -1)
    assert abs(e["master"][1] - want["master"][1]) <= 1e-6                   # masterMeanCol
    assert np.abs(e["master"][2:] - want["master"][2:]).max() <= 1e-4        # patch normal
    assert np.array_equal(e["ok"], want["ok"])
    okv = e["ok"] > 0
    assert np.array_equal(e["level"][okv], o["level"][okv])
    for gi in np.nonzero(okv)[0]:
        assert abs(e["ncc"][gi] - want["ncc"][gi]) <= 1e-4
        # 3e-5 = 2 ulp of a sample position of ~150 px times a gradient < 1; positions on a wider level carry larger ulps
        tol = 3e-5 * max(1.0, level_width(gi, int(e["level"][gi])) / 160.0)
        assert np.abs(e["col"][gi] - want["col"][gi]).max() <= tol, (gi, np.abs(e["col"][gi] - want["col"][gi]).max(), tol)
        assert np.abs(e["deriv"][gi] - want["der"][gi]).max() <= 1e-4 * max(np.abs(want["der"][gi]).max(), 1.0)
    return np.where(okv, e["level"], -1)


@pytest.mark.gpu
def test_gpu_patch_sampler(ctx_m1, m1, m1_oracle_eval):
    """patch_eval for reference views 0 and 1 against the reference's `eval` dumps: per-neighbour homographies, footprints,
    mip levels (each of 0, 1, 2 and the clamp reached by the GPU's own level output) and samples drawn from images of other
    sizes and pitches than the reference view's."""
    from mve_amd import api
    for ref in (0, 1):
        gvs = list(m1["gvs20_v%d" % ref])
        widths = {}

        def level_width(gi, lvl):
            if (gi, lvl) not in widths:
                widths[(gi, lvl)] = max(ctx_m1.level_size(gvs[gi], lvl))
            return widths[(gi, lvl)]
        st = api.Settings(refViewNr=ref)
        n = len(m1["v%d_seeds_xy" % ref])
        lvl = np.full((n, len(gvs)), -1)
        for i in range(n):
            x, y = [int(v) for v in m1["v%d_seeds_xy" % ref][i]]
            d, dzi, dzj = [float(v) for v in m1["v%d_seeds_hyp" % ref][i]]
            e = ctx_m1.patch_eval(st, ref, x, y, d, dzi, dzj)
            want = {k: m1["v%d_ev_%s" % (ref, k)][i] for k in ("master", "ncc", "ok", "col", "der")}
            assert len(e["ok"]) == len(gvs)
            lvl[i] = check_patch_eval(e, m1_oracle_eval[ref][i], want, level_width)
        assert (lvl >= 0).sum() >= 100 and ((lvl < 0) & (m1["v%d_ev_master" % ref][:, :1] > 0)).sum() >= 20
        check_level_coverage(lvl, m1["v%d_ev_rawlvl" % ref], gvs, ref)


@pytest.mark.gpu
def test_gpu_patch_optimization(ctx_m1, m1):
    """patch_optimize in both lane layouts against the reference's `opt` dumps (the shares of scene H1's test), the two
    layouts against each other (the bounds of test_lane_layouts_agree), and the propagated sets the reference completed or
    re-selected."""
    from mve_amd import api
    for ref in (0, 1):
        xy, hyp, local = m1["v%d_seeds_xy" % ref], m1["v%d_seeds_hyp" % ref], m1["v%d_seeds_local" % ref]
        want, want_loc = m1["v%d_opt" % ref], m1["v%d_opt_local" % ref]
        got = {}
        for lpv in (1, 16):
            out, loc = ctx_m1.patch_optimize(api.Settings(refViewNr=ref), ref, xy, hyp, local, lanes_per_view=lpv)
            got[lpv] = (out, loc)
            agree = (out[:, 0] > 0) == (want[:, 0] > 0)
            ok = (out[:, 0] > 0) & (want[:, 0] > 0)
            rel = np.abs(out[ok, 1] - want[ok, 1]) / want[ok, 1]
            dconf = np.abs(out[ok, 0] - want[ok, 0])
            same_views = (loc[ok] == want_loc[ok]).all(1)
            print("M1 view %d patches lpv=%s: outcome agreement %.4f, ok %d, rel depth <= 1e-3: %.4f, |dconf| <= 5e-3: %.4f, same views %.4f"
                  % (ref, lpv, agree.mean(), ok.sum(), (rel <= 1e-3).mean(), (dconf <= 5e-3).mean(), same_views.mean()))
            assert agree.mean() >= 0.97 and ok.sum() >= 40
            assert (rel <= 1e-3).mean() >= 0.97 and (dconf <= 5e-3).mean() >= 0.97 and same_views.mean() >= 0.97
            n = len(want)
            changed = (want[n // 2:, 0] > 0) & (want_loc[n // 2:] != local[n // 2:]).any(1)
            both = changed & (out[n // 2:, 0] > 0)
            assert both.sum() >= 3 and (loc[n // 2:][both] == want_loc[n // 2:][both]).all()
        (a, al), (b, bl) = got[1], got[16]
        assert np.array_equal(a[:, 0] > 0, b[:, 0] > 0)
        ok = a[:, 0] > 0
        assert np.abs(a[ok, 1] - b[ok, 1]).max() / 10.0 <= 1e-5      # only the summation order differs
        assert np.abs(a[ok, 0] - b[ok, 0]).max() <= 1e-4
        assert np.array_equal(al[ok], bl[ok]) and np.array_equal(a[ok, 7], b[ok, 7])


# what this build measures on the MI355X per map (fill IoU, relative depth median / p99, confidence median / p99); the
# regression guards of test_gpu_maps are 1.25 x these
GPU_MEASURED = {     # (IoU rounded down: the guard is on 1 - IoU)
    (0, 0): dict(iou=0.9997, rel_med=4.94e-5, rel_p99=3.91e-3, conf_med=2.21e-5, conf_p99=0.0533),
    (1, 0): dict(iou=0.9991, rel_med=6.75e-5, rel_p99=3.53e-3, conf_med=3.61e-5, conf_p99=0.0659),
    (4, 0): dict(iou=0.9998, rel_med=5.43e-5, rel_p99=2.63e-3, conf_med=7.78e-5, conf_p99=0.0382),
    (2, 1): dict(iou=0.9997, rel_med=2.98e-4, rel_p99=7.03e-3, conf_med=1.97e-4, conf_p99=0.0978),
}


@pytest.mark.gpu
def test_gpu_maps(ctx_m1, m1, monkeypatch):
    """reconstruct for views 0, 1 and 4 in ONE call -- map sizes 160 x 120, 120 x 160 and 160 x 120 with pixel aspect 1.25 in one
    batch -- and for view 2 at scale 1: every view alone gives the bits it gives in the batch, a second call and a call without
    the front kernel give them again, and the maps are the reference's within the general map-level bounds, or twice the
    algorithm's own order floor where that is worse (ORDER_FLOOR, measured on the CPU)."""
    from mve_amd import api
    keys = ("depth", "conf", "dz", "normal", "views")
    res = {}
    for s, refs in ((0, [0, 1, 4]), (1, [2])):
        st = api.Settings(scale=s)
        batch = ctx_m1.reconstruct(st, refs, want_views=True)
        again = ctx_m1.reconstruct(st, refs, want_views=True)
        monkeypatch.setenv("MI_DMRECON_FRONT", "0")
        tail = ctx_m1.reconstruct(st, refs, want_views=True)
        assert ctx_m1.last_stats["n_front_launches"] == 0
        monkeypatch.delenv("MI_DMRECON_FRONT")
        for i, v in enumerate(refs):
            single = ctx_m1.reconstruct(st, [v], want_views=True)[0] if len(refs) > 1 else batch[i]
            for k in keys:
                assert np.array_equal(again[i][k], batch[i][k]), ("run to run", v, k)
                assert np.array_equal(tail[i][k], batch[i][k]), ("front kernel", v, k)
                assert np.array_equal(single[k], batch[i][k]), ("batch", v, k)
            res[(v, s)] = batch[i]
    for (v, s), r in res.items():
        want_d, want_c = m1["s%dv%d_depth" % (s, v)], m1["s%dv%d_conf" % (s, v)]
        assert r["depth"].shape == want_d.shape
        m = map_parity(r["depth"], r["conf"], want_d, want_c)
        print("M1 view %d scale %d:" % (v, s), {k: float("%.4g" % x) for k, x in m.items()})
        assert m["iou"] >= map_bound(v, s, "iou"), (v, s, m)
        for k in ("rel_med", "rel_p99", "conf_med", "conf_p99"):
            assert m[k] <= map_bound(v, s, k), (v, s, k, m[k], map_bound(v, s, k), ORDER_FLOOR[(v, s)][k])
        g = GPU_MEASURED[(v, s)]                             # regression guard: 1.25 x what this build measures
        assert 1.0 - m["iou"] <= 1.25 * (1.0 - g["iou"]) + 1e-12, (v, s, m)
        for k in ("rel_med", "rel_p99", "conf_med", "conf_p99"):
            assert m[k] <= 1.25 * g[k], (v, s, k, m[k], g[k])
        # unfilled pixels are exactly zero in every map; the 2-pixel border is never filled
        un = r["conf"] == 0
        assert (r["depth"][un] == 0).all() and (r["dz"][un] == 0).all() and (r["normal"][un] == 0).all()
        assert (r["depth"][:2] == 0).all() and (r["depth"][-2:] == 0).all()
        assert (r["depth"][:, :2] == 0).all() and (r["depth"][:, -2:] == 0).all()
        assert r["conf"].max() <= 1.0 and (r["conf"][~un] > 0).all() and (r["depth"][~un] > 0).all()
        assert np.abs(np.linalg.norm(r["normal"][~un], axis=1) - 1).max() < 1e-4
        assert (r["views"][un] == -1).all() and (r["views"][~un] >= 0).all() and (np.diff(r["views"][~un], axis=1) > 0).all()


@pytest.mark.gpu
def test_gpu_view_below_30_pixels_has_one_level(gpu_ctx, m1, m1_scene, m1_oracle_eval):
    """A neighbour of 56 x 28 pixels has level 0 only (image_pyramid.cc:37): every level the rule asks for is clamped to 0
    (DevJobView::maxl = 0).  The reference cannot sample such a view (module docstring), so this is the library against the
    restatement: M1 with view 7 cut down to 56 x 28 (the same field of view at lower resolution; what the pixels show does not
    matter for this), the fixture's hypotheses of reference view 0."""
    from mve_amd import api
    from mve_amd.scene_io import SceneData
    imgs = list(m1_scene.images)
    imgs[7] = np.ascontiguousarray(imgs[7][14:42, 22:78])
    small = SceneData(m1_scene.cameras, imgs, m1_scene.features)
    S = orc.OracleScene(small)
    assert S.pyramid_levels(7) == 1
    try:
        gpu_ctx.load_scene(small)
        assert gpu_ctx.num_levels(7) == 1
        img, proj, inv = gpu_ctx.get_level(7, 0)
        oimg, oproj, oinv = S.pyramid_level(7, 0)
        assert np.array_equal(img, oimg) and np.array_equal(proj, oproj) and np.array_equal(inv, oinv)
        gvs = S.global_vs(orc.make_settings(ref_view=0))
        assert gpu_ctx.global_view_selection(api.Settings(refViewNr=0)) == gvs and 7 in gvs
        g7, n_clamped = gvs.index(7), 0
        for i in range(len(m1["v0_seeds_xy"])):
            if m1_oracle_eval[0][i]["ok"][list(m1["gvs20_v0"]).index(7)] == 0:
                continue                                      # (only the hypotheses that view 7 can see)
            x, y = [int(v) for v in m1["v0_seeds_xy"][i]]
            d, dzi, dzj = [float(v) for v in m1["v0_seeds_hyp"][i]]
            o = S.patch_eval(orc.make_settings(ref_view=0), x, y, d, dzi, dzj)
            e = gpu_ctx.patch_eval(api.Settings(refViewNr=0), 0, x, y, d, dzi, dzj)
            want = dict(master=o["master"], ncc=o["ncc"], ok=o["ok"], col=o["col"], der=o["deriv"])
            lvl = check_patch_eval(e, o, want, lambda gi, l: max(gpu_ctx.level_size(gvs[gi], l)))
            assert lvl[g7] <= 0
            n_clamped += int(lvl[g7] == 0 and m1["v0_ev_rawlvl"][i][list(m1["gvs20_v0"]).index(7)] >= 1)
        assert n_clamped >= 10
    finally:
        gpu_ctx.load_scene(m1_scene)                          # what the module's other tests expect (ctx_m1)
