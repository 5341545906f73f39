"""Regenerates tests/golden/fssr_f1.npz and fssr_f1_mesh.npz, or (--fixture f2) tests/golden/fssr_f2.npz.  Run by hand where
the reference tree exists:

    python tests/golden/make_golden_fssr.py [--fixture f1|f2] [--ref /path/to/mve] [--samples N] [--out DIR]

Compiles the reference's libs/util, libs/mve, libs/fssr and tests/golden/ref_fssr_driver.cc into a temporary directory
outside the repository, in the two flavours of oracle/Makefile (STRICT: what the fixture stores; FAST: the reference's own
flags, from which the anchors -- the error between two builds of the SAME code -- are taken), runs both on the fixture
and writes the .npz files.  Never run by build() or by a test."""
import argparse
import glob
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fssr_restatement import QUANTITIES, influence_pairs, rel_error, sample_levels  # noqa: E402
from mve_amd.scene2pset import write_ply  # noqa: E402

# quoted from oracle/Makefile
REF_DEFS = "-DMVE_NO_JPEG_SUPPORT -DMVE_NO_TIFF_SUPPORT -std=c++17 -pthread -w"
FLAVOURS = {
    "fast": "-O3 -march=x86-64-v3 -funsafe-math-optimizations -fno-math-errno -fopenmp",
    "strict": "-O2 -ffp-contract=off -fopenmp",
}
PNGLIB = "/usr/lib/x86_64-linux-gnu/libpng16.so.16"
PNGINC = "/opt/conda/include"


def make_f1(n_sphere: int = 800, n_cluster: int = 300, seed: int = 20150715) -> dict:
    """Fixture F1: a noisy unit sphere with two scale populations, three samples with the special normals of
    rotation_from_normal, and a dense patch whose scales take three values only (ties at the scale cut, voxels with more
    than 128 influencing samples)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_sphere, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = d * (1.0 + rng.normal(scale=0.004, size=(n_sphere, 1)))
    nrm = d + rng.normal(scale=0.03, size=(n_sphere, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    scale = rng.uniform(0.03, 0.06, n_sphere)
    big = np.arange(n_sphere) % 7 == 0
    scale[big] = rng.uniform(0.12, 0.22, big.sum())
    # the branches of rotation_from_normal: exactly (1,0,0), exactly (-1,0,0), within 0.001 of (1,0,0) but not equal
    sp_pos = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.99875, 0.05, 0.0]])
    sp_nrm = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.9999998, 0.0005, 0.0]])
    sp_scale = np.array([0.05, 0.05, 0.05])
    # the dense patch around (0, 0, 1)
    u = rng.uniform(-0.07, 0.07, size=(n_cluster, 2))
    cd = np.concatenate([u, np.ones((n_cluster, 1))], 1)
    cd /= np.linalg.norm(cd, axis=1, keepdims=True)
    c_pos = cd * (1.0 + rng.normal(scale=0.002, size=(n_cluster, 1)))
    c_scale = np.array([0.04, 0.05, 0.0625])[rng.integers(0, 3, n_cluster)]
    pos = np.concatenate([pos, sp_pos, c_pos])
    nrm = np.concatenate([nrm, sp_nrm, cd])
    scale = np.concatenate([scale, sp_scale, c_scale])
    n = len(pos)
    return {
        "pos": pos.astype(np.float32), "normal": nrm.astype(np.float32), "scale": scale.astype(np.float32),
        "conf": rng.uniform(0.2, 1.0, n).astype(np.float32), "color": rng.integers(0, 256, size=(n, 3)).astype(np.uint8),
    }


def make_f2(n_sphere: int = 600, n_ball: int = 1300, n_ladder: int = 60, seed: int = 20150716) -> dict:
    """Fixture F2: a tree of 21 levels and lists longer than a wavefront's on-chip part.  A noisy unit sphere with scales
    over almost two decades (the first sample, scale 0.05, sets the first root), a ball of samples around (0, 0, 1) whose
    supports all overlap (more than 1024 samples influence the voxels there, and they crowd into few nodes; scales as in
    the dense GPU test: ties at the scale cut), and a "ladder" around (1, 0, 0) whose scales fall geometrically to far below
    the node size of level 20, each sample scattered by its own scale (samples on every level down to the max_level
    clamp)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_sphere, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = d * (1.0 + rng.normal(scale=0.004, size=(n_sphere, 1)))
    nrm = d + rng.normal(scale=0.03, size=(n_sphere, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    scale = np.exp(rng.uniform(np.log(0.004), np.log(0.25), n_sphere))
    scale[0] = 0.05
    # the ball
    b_pos = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.012, 0.012, size=(n_ball, 3))
    bd = rng.normal(size=(n_ball, 3))
    b_nrm = bd / np.linalg.norm(bd, axis=1, keepdims=True)
    b_scale = np.where(np.arange(n_ball) % 3 == 0, rng.uniform(0.05, 0.1, n_ball), np.array([0.05, 0.0625, 0.08])[rng.integers(0, 3, n_ball)])
    # the ladder
    l_scale = 2e-3 * (2e-7 / 2e-3) ** (np.arange(n_ladder) / (n_ladder - 1.0))
    l_pos = np.array([1.0, 0.0, 0.0]) + rng.normal(size=(n_ladder, 3)) * l_scale[:, None]
    l_nrm = np.array([1.0, 0.0, 0.0]) + rng.normal(scale=0.2, size=(n_ladder, 3))
    l_nrm /= np.linalg.norm(l_nrm, axis=1, keepdims=True)
    pos = np.concatenate([pos, b_pos, l_pos])
    nrm = np.concatenate([nrm, b_nrm, l_nrm])
    scale = np.concatenate([scale, b_scale, l_scale])
    n = len(pos)
    return {
        "pos": pos.astype(np.float32), "normal": nrm.astype(np.float32), "scale": scale.astype(np.float32),
        "conf": rng.uniform(0.2, 1.0, n).astype(np.float32), "color": rng.integers(0, 256, size=(n, 3)).astype(np.uint8),
    }


def f2_subset(nodes: np.ndarray, samples: np.ndarray, positions: np.ndarray, n: np.ndarray, every: int) -> np.ndarray:
    """The voxels of F2 the fixture stores (a committed file stays under 1 MiB): every voxel with more than 1024 influencing
    samples, every voxel that a sample on levels 12-20 influences, every empty voxel, and every `every`-th of the rest."""
    lvl = sample_levels(nodes, len(samples))
    vi, si = influence_pairs(samples, positions)
    deep = np.zeros(len(positions), bool)
    deep[vi[lvl[si] >= 12]] = True
    must = (n > 1024) | deep | (n == 0)
    rest = np.nonzero(~must)[0][::every]
    keep = must.copy()
    keep[rest] = True
    return np.nonzero(keep)[0].astype(np.int32)


def build_driver(ref: str, work: str, flavour: str) -> str:
    inc = os.path.join(work, "pnginc")
    os.makedirs(inc, exist_ok=True)
    for h in ("png.h", "pngconf.h", "pnglibconf.h"):
        shutil.copy(os.path.join(PNGINC, h), inc)
    out = os.path.join(work, flavour)
    srcs = [s for lib in ("util", "mve", "fssr") for s in sorted(glob.glob(os.path.join(ref, "libs", lib, "[!_]*.cc")))]
    srcs.append(os.path.join(HERE, "ref_fssr_driver.cc"))
    flags = FLAVOURS[flavour].split() + REF_DEFS.split() + ["-I" + inc, "-I" + os.path.join(ref, "libs")]
    objs = []

    def compile_one(src):
        obj = os.path.join(out, os.path.relpath(src, "/").replace("/", "_") + ".o")
        subprocess.check_call(["g++"] + flags + ["-c", src, "-o", obj])
        return obj

    os.makedirs(out, exist_ok=True)
    with ThreadPoolExecutor(max(1, min(os.cpu_count() or 1, 8))) as pool:
        objs = list(pool.map(compile_one, srcs))
    exe = os.path.join(out, "ref_fssr_driver")
    subprocess.check_call(["g++", "-fopenmp", "-pthread"] + objs + [PNGLIB, "-o", exe])
    return exe


def run(exe: str, mode: str, ply: str, out: str) -> dict:
    os.makedirs(out, exist_ok=True)
    subprocess.check_call([exe, mode, ply, out], stdout=subprocess.DEVNULL)
    types = {"i32": np.int32, "u32": np.uint32, "u64": np.uint64, "f32": np.float32, "f64": np.float64}
    return {f.split(".")[0]: np.fromfile(os.path.join(out, f), types[f.split(".")[1]]) for f in sorted(os.listdir(out))}


def voxel_fields(r: dict) -> dict:
    d = r["vox_data"].reshape(-1, 9)
    return {"value": d[:, 0], "conf": d[:, 1], "scale": d[:, 2], "color": d[:, 3:6], "deriv": d[:, 6:9]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--fixture", choices=("f1", "f2"), default="f1")
    ap.add_argument("--samples", type=int, default=800, help="F1: samples on the sphere")
    ap.add_argument("--every", type=int, default=3, help="F2: every k-th of the voxels the subset need not hold is stored")
    ap.add_argument("--out", default=HERE, help="where the .npz files go")
    ap.add_argument("--keep", default=None, help="keep the build directory here (e.g. to reuse the drivers)")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="fssr_golden_")
    os.makedirs(work, exist_ok=True)
    f2 = a.fixture == "f2"
    ps = make_f2() if f2 else make_f1(a.samples)
    ply = os.path.join(work, a.fixture + ".ply")
    write_ply(ply, ps, with_normals=True, with_scale=True, with_conf=True)
    res = {}
    for fl in FLAVOURS:
        exe = os.path.join(work, fl, "ref_fssr_driver")
        if not os.path.exists(exe):
            exe = build_driver(a.ref, work, fl)
        res[fl] = (run(exe, "voxels", ply, os.path.join(work, fl, a.fixture + "_vox")),
                   None if f2 else run(exe, "mesh", ply, os.path.join(work, fl, "mesh")))
    (sv, sm), (fv, fm) = res["strict"], res["fast"]

    for k in ("nodes", "root", "vox_pos", "vox_n", "vox_max_scale"):
        assert np.array_equal(sv[k], fv[k]), "the two flavours disagree on " + k
    # (the colours may differ in the last bit: the fast flavour's loader multiplies by 1/255 where the strict one divides)
    cols = [0, 1, 2, 3, 4, 5, 9, 10]
    assert np.array_equal(sv["samples"].reshape(-1, 11)[:, cols], fv["samples"].reshape(-1, 11)[:, cols])
    out = {"ply_" + k: v for k, v in ps.items()}
    out.update(nodes=sv["nodes"].reshape(-1, 4), samples=sv["samples"].reshape(-1, 11), root=sv["root"],
               positions=sv["vox_pos"].reshape(-1, 3), n_influencing=sv["vox_n"], max_scale=sv["vox_max_scale"])
    s, f = voxel_fields(sv), voxel_fields(fv)
    nonempty = sv["vox_n"] > 0
    # VoxelData() leaves `deriv` uninitialised (voxel.h:98-105): for an empty voxel the reference holds whatever the memory
    # held, which nothing reads (such a voxel has conf 0).  The fixture stores zeros there.
    s["deriv"][~nonempty] = 0.0
    if f2:
        # a fixed subset of the voxels, and the anchors over the rows that are stored: the rows the tests measure on
        keep = f2_subset(out["nodes"], out["samples"], out["positions"], sv["vox_n"], a.every)
        out.update(voxel_index=keep, n_voxels_full=np.int64(len(sv["vox_n"])))
        for k in ("positions", "n_influencing", "max_scale"):
            out[k] = out[k][keep]
        for q in QUANTITIES:
            out[q] = s[q][keep]
            out["anchor_" + q] = np.float64(rel_error(f[q][keep], s[q][keep], nonempty[keep]))
        fn = os.path.join(a.out, "fssr_f2.npz")
        np.savez_compressed(fn, **out)
        lvl = sample_levels(out["nodes"], len(out["samples"]))
        print("F2: %d samples on levels %s, %d nodes (largest %d samples), %d of %d voxels stored (%d empty, %d with n > 1024, max n %d)"
              % (len(lvl), sorted(set(lvl.tolist())), len(out["nodes"]), out["nodes"][:, 2].max(), len(keep), len(sv["vox_n"]),
                 (out["n_influencing"] == 0).sum(), (out["n_influencing"] > 1024).sum(), sv["vox_n"].max()))
        print("anchors:", {q: float(out["anchor_" + q]) for q in QUANTITIES})
        print(fn, os.path.getsize(fn), "bytes")
        if not a.keep:
            shutil.rmtree(work)
        return
    for q in QUANTITIES:
        out[q] = s[q]
        out["anchor_" + q] = np.float64(rel_error(f[q], s[q], nonempty))
    np.savez_compressed(os.path.join(a.out, "fssr_f1.npz"), **out)

    # (the fast flavour may split some polygons along the other diagonal: IsoSurface's triangulation compares float
    # geometry that its own flags round differently; vertices and their order are the same)
    assert len(sm["mesh_verts"]) == len(fm["mesh_verts"]) and len(sm["mesh_faces"]) == len(fm["mesh_faces"])
    print("faces that differ between the flavours: %d" % (sm["mesh_faces"].reshape(-1, 3) != fm["mesh_faces"].reshape(-1, 3)).any(1).sum())
    mesh = {"verts": sm["mesh_verts"].reshape(-1, 3), "faces": sm["mesh_faces"].reshape(-1, 3), "conf": sm["mesh_conf"],
            "values": sm["mesh_values"]}
    mesh["anchor_pos"] = np.float64(np.max(np.abs(sm["mesh_verts"].astype(np.float64) - fm["mesh_verts"])))
    mesh["anchor_attr"] = np.float64(max(rel_error(fm["mesh_conf"], sm["mesh_conf"]), rel_error(fm["mesh_values"], sm["mesh_values"])))
    np.savez_compressed(os.path.join(a.out, "fssr_f1_mesh.npz"), **mesh)

    print("F1: %d samples, %d nodes, %d voxels (%d empty, max n %d); mesh %d vertices, %d faces"
          % (len(out["samples"]), len(out["nodes"]), len(out["positions"]), (~nonempty).sum(), sv["vox_n"].max(),
             len(mesh["verts"]), len(mesh["faces"])))
    print("anchors:", {q: float(out["anchor_" + q]) for q in QUANTITIES}, "mesh pos %.3g attr %.3g" % (mesh["anchor_pos"], mesh["anchor_attr"]))
    for fn in ("fssr_f1.npz", "fssr_f1_mesh.npz"):
        print(fn, os.path.getsize(os.path.join(a.out, fn)), "bytes")
    if not a.keep:
        shutil.rmtree(work)


if __name__ == "__main__":
    main()
