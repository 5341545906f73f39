"""Generates tests/golden/round_counters.json: the work counters of mi_dmrecon_stats -- totals and the per-kernel arrays -- that
the library reports for scenes G1 (views 0-4), H1 (views 0-8) and the mixed-size scene M1, by default and under the switches
that force the other round plans.  Run on an MI355X with the build whose counts are to be pinned (the commit before the work
counters were striped and k_generate claimed its list slots per strip of tiles; the forms of the follow-up launches and the
eight-slot case: the commit before the launchers took descriptors, which reproduced every older entry):

    python tests/golden/make_golden_round_counters.py [output file, default tests/golden/round_counters.json]

The work counts are deterministic (tests/test_gpu_parity.py::test_batch_equals_single_and_is_deterministic): every case is run
three times here and must give the same integers before anything is written.  The two diagnostics n_view_replaced and n_iter14
are the exception where the front kernel's teams run (H1 by default: 41 063 / 41 064 and 2 950 / 2 943 in two calls of the build
this file was made with): a case whose three runs disagree on one of them records it under "unstable" instead of a value.
tests/test_round_counters.py runs the same cases (CASES, measure) and demands equality, integer for integer, of what is recorded.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))

SCALARS = ("n_patch", "n_eval", "n_pass", "n_filled", "n_rounds", "n_view_replaced", "n_iter14", "n_seeds_ok")
ARRAYS = ("n_eval_by_kernel", "n_pass_by_kernel", "n_patch_by_kernel", "n_pass_executed_by_kernel")
MAY_VARY = ("n_view_replaced", "n_iter14")     # diagnostics of rare events, counted per event: not the same from call to call under the front's teams
KINDS = ("fast", "follow", "seed", "loop", "spec", "latency", "tail", "front")

# "handover": a hand-over threshold (the scene's own value below) low enough that the views of these small scenes stay in the
# throughput layout for rounds -- by default they leave it at once and the front kernel does nearly everything -- and hand over at
# different rounds; with it the forced plans of tests/test_gpu_parity.py::test_maps_do_not_depend_on_the_batch, as there
SWITCHES = {
    "default": {},
    "handover": {"MI_DMRECON_VIEW_HANDOVER": None},
    "two_launches": {"MI_DMRECON_VIEW_HANDOVER": None, "MI_DMRECON_ONE_LAUNCH": "0", "MI_DMRECON_SPEC_ROUNDS": "0"},
    "two_launches_loop": {"MI_DMRECON_VIEW_HANDOVER": None, "MI_DMRECON_ONE_LAUNCH": "0", "MI_DMRECON_SPEC_ROUNDS": "0", "MI_DMRECON_SINGLE_FOLLOW": "0"},
    "all_speculative": {"MI_DMRECON_VIEW_HANDOVER": None, "MI_DMRECON_SPEC_ROUNDS": "1000000"},
}
# the forms of the two-launch plan's follow-up launches that no other case selects: the first two follow-ups in the FAST kernel, the
# first follow-up list appended by atomics instead of compacted in list order, one list for all XCDs instead of a segment each
TWO_LAUNCHES = SWITCHES["two_launches"]
SWITCHES["fast_follow"] = dict(TWO_LAUNCHES, MI_DMRECON_FAST_FOLLOW="2")
SWITCHES["unordered"] = dict(TWO_LAUNCHES, MI_DMRECON_FOLLOW_ORDERED="0")
SWITCHES["one_list"] = dict(TWO_LAUNCHES, MI_DMRECON_FOLLOW_SEGMENTS="0")
SAME_MAPS_AS_TWO_LAUNCHES = ("fast_follow", "unordered", "one_list")
# scene -> (scale, reference views, MI_DMRECON_VIEW_HANDOVER of the "handover" case, settings other than the defaults)
SCENES = {"g1": (0, [0, 1, 2, 3, 4], "150", {}), "h1": (0, list(range(9)), "60", {}), "m1": (0, [0, 1, 4], "150", {}),
          "m1_scale1": (1, [2], "150", {}),
          # the eight-slot layout (nrReconNeighbors > 4) through the follow-up launches: the two-launch plan only.  (With eight
          # neighbours H1's lists are short: at 40 entries every view hands over at once and neither kernel of the plan runs, at 20
          # most rounds run it and the views still end in the eight-slot latency layout and the front kernel.)
          "h1_k8": (0, list(range(9)), "20", {"nrReconNeighbors": 8})}
ONLY = {"h1_k8": ("two_launches",)}
CASES = [(s, w) for s in SCENES for w in ONLY.get(s, SWITCHES)]


def load_scene_data(name):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import scene_from_golden
    if name == "g1":
        return scene_from_golden(dict(np.load(os.path.join(OUT, "g1_5views_160x120.npz"))))
    if name == "h1":
        return scene_from_golden(dict(np.load(os.path.join(OUT, "h1_hard_9views_208x156.npz"))))
    from test_mixed_cameras import load_m1, scene_of
    return scene_of(load_m1())


def counters_of(stats):
    out = {k: int(stats[k]) for k in SCALARS}
    for a in ARRAYS:
        out[a] = [int(stats["%s.%s" % (a, kind)]) for kind in KINDS]
    return out


def measure(ctx, scene_name, switch_name, want_maps=False):
    """The counters of one case on a context that holds the scene; the environment is put back afterwards."""
    from mve_amd import api
    scale, refs, handover, settings = SCENES[scene_name]
    env = {k: (handover if v is None else v) for k, v in SWITCHES[switch_name].items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        maps = ctx.reconstruct(api.Settings(scale=scale, **settings), refs, want_views=True)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    c = counters_of(ctx.last_stats)
    return (c, maps, dict(ctx.last_stats)) if want_maps else c


def main():
    sys.path.insert(0, ROOT)
    from mve_amd import api
    ctx = api.Context(0)
    out, loaded = {}, None
    for scene_name, switch_name in CASES:
        data_name = scene_name.split("_")[0]
        if data_name != loaded:
            ctx.load_scene(load_scene_data(data_name))
            loaded = data_name
        a, b, c3 = measure(ctx, scene_name, switch_name), measure(ctx, scene_name, switch_name), measure(ctx, scene_name, switch_name)
        unstable = sorted(k for k in a if not (a[k] == b[k] == c3[k]))
        assert set(unstable) <= set(MAY_VARY), ("not deterministic", scene_name, switch_name, a, b, c3)
        assert a["n_patch"] > 1000 and a["n_filled"] > 1000, (scene_name, switch_name, a)
        for k in unstable:
            del a[k]
        a["unstable"] = unstable
        out["%s/%s" % (scene_name, switch_name)] = a
        print(scene_name, switch_name, {k: a.get(k) for k in SCALARS}, "unstable:", unstable, flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(OUT, "round_counters.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
