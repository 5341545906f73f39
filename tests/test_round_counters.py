"""The work counters of mi_dmrecon_stats after the counters were striped on the device (DevCounterStripe: the kernels add the
per-kind words to one of MI_COUNTER_STRIPES copies, k_round_report sums the copies and forms the totals): the totals are the sums
of the per-kernel arrays, and every count is what the build before the change reported -- tests/golden/round_counters.json,
written by tests/golden/make_golden_round_counters.py with that build, for scenes G1, H1 and M1 by default and under the switches
that force the other round plans (among them the forms of the follow-up launches that nothing else selects, and the eight-slot
layout through them: a launch that reaches another kernel template moves counts between the kinds).  Integer for integer; the
two diagnostics that build did not report the same from call to call
(n_view_replaced, n_iter14 under the front kernel's teams: "unstable" in the file) are not compared in those cases."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_golden_round_counters", os.path.join(GOLDEN, "make_golden_round_counters.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

OPTIMIZE_KINDS = ("fast", "follow", "seed", "loop", "latency")      # templates of k_optimize: every pass they run is one they count


@pytest.fixture(scope="module")
def golden_counters():
    with open(os.path.join(GOLDEN, "round_counters.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def counters_ctx():
    from mve_amd import api
    assert api.device_count() > 0, "no HIP device visible: -m gpu tests need an MI355X"
    ctx = api.Context(0)
    yield ctx
    ctx.close()


def test_golden_file_covers_the_cases(golden_counters):
    assert sorted(golden_counters) == sorted("%s/%s" % c for c in gen.CASES)
    for name, g in golden_counters.items():
        assert set(g["unstable"]) <= set(gen.MAY_VARY), name
        assert set(g) | set(g["unstable"]) == set(gen.SCALARS) | set(gen.ARRAYS) | {"unstable"}, name
        # the build that wrote the file already satisfied the identities
        for tot, arr in (("n_eval", "n_eval_by_kernel"), ("n_pass", "n_pass_by_kernel"), ("n_patch", "n_patch_by_kernel")):
            assert g[tot] == sum(g[arr]), (name, tot)
    # the cases are not all the same plan: every kernel template but the fused tail rounds counts somewhere
    for scene in ("g1", "h1", "m1"):
        for case, kinds in (("handover", ("seed", "spec", "latency", "front")), ("two_launches", ("fast", "follow", "latency", "front")),
                            ("two_launches_loop", ("fast", "loop")), ("all_speculative", ("spec",)), ("default", ("latency", "front"))):
            for kind in kinds:
                assert golden_counters["%s/%s" % (scene, case)]["n_patch_by_kernel"][gen.KINDS.index(kind)] > 0, (scene, case, kind)
    # the follow-up forms no other case selects, and the eight-slot layout, do reach both the FAST and the single-attempt kernel
    for name in ["%s/%s" % (scene, case) for scene in ("g1", "h1", "m1") for case in gen.SAME_MAPS_AS_TWO_LAUNCHES] + ["h1_k8/two_launches"]:
        for kind in ("fast", "follow"):
            assert golden_counters[name]["n_patch_by_kernel"][gen.KINDS.index(kind)] > 0, (name, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", sorted(gen.SCENES))
def test_counter_identities_and_parent_counts(counters_ctx, golden_counters, scene_name):
    counters_ctx.load_scene(gen.load_scene_data(scene_name.split("_")[0]))
    maps_of = {}
    for switch_name in gen.ONLY.get(scene_name, gen.SWITCHES):
        got, maps_of[switch_name], _ = gen.measure(counters_ctx, scene_name, switch_name, want_maps=True)
        want = golden_counters["%s/%s" % (scene_name, switch_name)]
        print(scene_name, switch_name, {k: got[k] for k in gen.SCALARS})
        for tot, arr in (("n_eval", "n_eval_by_kernel"), ("n_pass", "n_pass_by_kernel"), ("n_patch", "n_patch_by_kernel")):
            assert got[tot] == sum(got[arr]), (scene_name, switch_name, tot, got[tot], got[arr])
        for kind in OPTIMIZE_KINDS:
            i = gen.KINDS.index(kind)
            assert got["n_pass_executed_by_kernel"][i] == got["n_pass_by_kernel"][i], (scene_name, switch_name, kind)
        for k in want:
            if k != "unstable":
                assert got[k] == want[k], (scene_name, switch_name, k, got[k], want[k])
    # the forms of the follow-up launches change which kernel runs an attempt, never what it computes
    for switch_name in gen.SAME_MAPS_AS_TWO_LAUNCHES:
        if switch_name in maps_of:
            for a, b in zip(maps_of[switch_name], maps_of["two_launches"]):
                for k in ("depth", "conf", "dz", "normal", "views"):
                    assert np.array_equal(a[k], b[k]), (scene_name, switch_name, k)
