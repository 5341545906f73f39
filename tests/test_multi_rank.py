"""CPU test of the N > 1 path: two gloo processes run the bench's barrier / shard / max-over-ranks logic."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shard_views_partition():
    from mve_amd.dist import shard_views
    views = list(range(20))
    for world in (1, 2, 4, 8):
        parts = [shard_views(views, r, world) for r in range(world)]
        assert sorted(v for p in parts for v in p) == views
        assert max(map(len, parts)) - min(map(len, parts)) <= 1


def test_two_rank_gloo_barrier_and_max(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(textwrap.dedent("""
        import sys, time
        sys.path.insert(0, %r)
        from mve_amd.dist import Collective, shard_views
        c = Collective("gloo")
        assert c.world == 2
        mine = shard_views(list(range(5)), c.rank, c.world)
        c.barrier()
        t0 = time.perf_counter()
        time.sleep(0.05 * (c.rank + 1))                 # rank 1 is the slow one
        c.barrier()
        el = c.max(0.05 * (c.rank + 1))
        total = c.sum(len(mine))
        assert abs(el - 0.10) < 1e-9, el
        assert int(total) == 5
        if c.rank == 0:
            print("OK", el, int(total))
        c.close()
    """ % ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29617", str(script)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "OK 0.1" in out.stdout


def test_two_rank_gloo_strong_and_weak_modes(tmp_path):
    """bench.py's two multi-GPU modes on two gloo ranks with a stand-in for the library call (time ~ views):
    weak = every rank all 5 views, strong = the 5 views of one scene dealt 3 + 2; value = maps of all ranks /
    slowest rank, exactly as bench.py computes it."""
    script = tmp_path / "worker2.py"
    script.write_text(textwrap.dedent("""
        import sys, time
        sys.path.insert(0, %r)
        from mve_amd.dist import Collective, rank_views
        c = Collective("gloo")
        views, steps, per_view = list(range(5)), 4, 0.01
        out = {}
        for mode in ("weak", "strong"):
            mine = rank_views(views, c.rank, c.world, mode)
            c.barrier()
            t0 = time.perf_counter()
            time.sleep(per_view * len(mine) * steps)       # the reconstruct calls
            c.barrier()
            el = c.max(time.perf_counter() - t0)
            n = int(round(c.sum(len(mine) * steps)))
            out[mode] = (n, n / el, mine)
        assert out["weak"][0] == 2 * 5 * steps and out["strong"][0] == 5 * steps
        assert out["strong"][2] == ([0, 2, 4] if c.rank == 0 else [1, 3])
        # weak: 40 maps in ~0.2 s; strong: 20 maps in ~0.12 s (the rank with 3 views is the slow one)
        assert 150 < out["weak"][1] < 210 and 120 < out["strong"][1] < 175, out
        if c.rank == 0:
            print("MODES_OK")
        c.close()
    """ % ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29618", str(script)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "MODES_OK" in out.stdout


def test_bench_gpus_2_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` as the driver types it (no torchrun around it) must start its two ranks itself, bind rank r to
    device r and print ONE JSON line with n_gpus = 2, the weak value and (--full) the strong-scaling sub-object with the ranks' shares.
    No GPU here: the ranks load tests/stub/mi_dmrecon_stub.c (a stand-in that computes nothing -- test infrastructure, built
    into a temporary directory; MI_DMRECON_LIB) and share "device 0" over gloo (MI_BENCH_SHARE_GPU=1)."""
    import json
    lib = tmp_path / "libmi_dmrecon_stub.so"
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "stub", "mi_dmrecon_stub.c"), "-o", str(lib)])
    env = dict(os.environ, MI_DMRECON_LIB=str(lib), MI_BENCH_SHARE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "C1", "--steps", "4", "--warmup", "1",
                          "--repeats", "2", "--no-cpu-baseline", "--full"], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["steps"] == 4 and d["warmup"] == 1
    assert d["value"] > 0 and len(d["repeats"]) == 2
    assert d["config"]["ranks_share_one_gpu"] is True
    ss = d["strong_scaling"]
    assert ss["value"] > 0 and ss["views_per_rank"] == [1, 1]            # C1: two reference views, one per rank
    # weak: both ranks reconstruct both views per step; strong: one view each -- twice the weak maps per rank-second at best
    assert d["value"] > ss["value"] * 0.5


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times ONE region of K steps and prints the line without the parts that
    take runs of their own (--full); --dump-outputs writes the maps of the last timed step as float32 .npy files, the same
    in two runs of the same command.  On the stand-in library, as above."""
    import json
    import numpy as np
    lib = tmp_path / "libmi_dmrecon_stub.so"
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "stub", "mi_dmrecon_stub.c"), "-o", str(lib)])
    env = dict(os.environ, MI_DMRECON_LIB=str(lib))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MI_FORCE_DIST"):
        env.pop(k, None)
    dumps = []
    for name in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", "--steps", "4", "--warmup", "1",
                              "--dump-outputs", str(tmp_path / name)], capture_output=True, text=True, env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 4 and d["warmup"] == 1 and len(d["repeats"]) == 1 and d["higher_is_better"] is True
        assert d["value"] > 0 and d["unit"] == "depth-maps/s" and d["dtype"] == "f32"
        assert d["ms_per_step"] == pytest.approx(1000.0 * 2 / d["value"])          # C1: two depth maps per step
        for key in ("one_call", "cpu_baseline", "parity"):
            assert key not in d, key
        assert "all_seeds_propagate_variant" not in d["config"] and "distinct_scenes_variant" not in d["config"]
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["conf.npy", "depth.npy", "dz.npy", "view_ids.npy"]
        dumps.append({f: np.load(tmp_path / name / f) for f in files})
    a, b = dumps
    assert a["depth.npy"].shape == (2, 480, 640) and a["dz.npy"].shape == (2, 480, 640, 2) and list(a["view_ids.npy"]) == [0.0, 1.0]
    for f in a:
        assert a[f].dtype in (np.float32, np.float64) and np.array_equal(a[f], b[f]), f
    assert sum(v.nbytes for v in a.values()) <= 64 << 20


import pytest  # noqa: E402


@pytest.mark.gpu
def test_collective_on_rccl_one_rank(tmp_path):
    """The backend the N > 1 bench runs on -- "nccl" = RCCL -- on the one GPU a test box has: a one-rank process group
    (MI_FORCE_DIST=1), barrier + max + sum through Collective exactly as bench.py's timed region uses them."""
    script = tmp_path / "rccl1.py"
    script.write_text(textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        from mve_amd.dist import Collective
        c = Collective("nccl", 0)
        assert c.dist is not None and c.device.type == "cuda"
        c.barrier()
        assert c.max(1.25) == 1.25 and c.sum(3.0) == 3.0
        c.barrier()
        c.close()
        print("RCCL_OK")
    """ % ROOT))
    env = dict(os.environ, MI_FORCE_DIST="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29631",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "RCCL_OK" in out.stdout
