"""Regenerates tests/golden/fssr_f1.npz and fssr_f1_mesh.npz.  Run by hand where the reference tree exists:

    python tests/golden/make_golden_fssr.py [--ref /path/to/mve] [--samples N]

Compiles the reference's libs/util, libs/mve, libs/fssr and tests/golden/ref_fssr_driver.cc into a temporary directory
outside the repository, in the two flavours of oracle/Makefile (STRICT: what the fixture stores; FAST: the reference's own
flags, from which the anchors -- the error between two builds of the SAME code -- are taken), runs both on fixture F1
and writes the two .npz files.  Never run by build() or by a test."""
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

from fssr_restatement import QUANTITIES, rel_error  # noqa: E402
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
    ap.add_argument("--samples", type=int, default=800)
    ap.add_argument("--keep", default=None, help="keep the build directory here (e.g. to reuse the drivers)")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="fssr_golden_")
    os.makedirs(work, exist_ok=True)
    ps = make_f1(a.samples)
    ply = os.path.join(work, "f1.ply")
    write_ply(ply, ps, with_normals=True, with_scale=True, with_conf=True)
    res = {}
    for fl in FLAVOURS:
        exe = os.path.join(work, fl, "ref_fssr_driver")
        if not os.path.exists(exe):
            exe = build_driver(a.ref, work, fl)
        res[fl] = (run(exe, "voxels", ply, os.path.join(work, fl, "vox")), run(exe, "mesh", ply, os.path.join(work, fl, "mesh")))
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
    for q in QUANTITIES:
        out[q] = s[q]
        out["anchor_" + q] = np.float64(rel_error(f[q], s[q], nonempty))
    np.savez_compressed(os.path.join(HERE, "fssr_f1.npz"), **out)

    # (the fast flavour may split some polygons along the other diagonal: IsoSurface's triangulation compares float
    # geometry that its own flags round differently; vertices and their order are the same)
    assert len(sm["mesh_verts"]) == len(fm["mesh_verts"]) and len(sm["mesh_faces"]) == len(fm["mesh_faces"])
    print("faces that differ between the flavours: %d" % (sm["mesh_faces"].reshape(-1, 3) != fm["mesh_faces"].reshape(-1, 3)).any(1).sum())
    mesh = {"verts": sm["mesh_verts"].reshape(-1, 3), "faces": sm["mesh_faces"].reshape(-1, 3), "conf": sm["mesh_conf"],
            "values": sm["mesh_values"]}
    mesh["anchor_pos"] = np.float64(np.max(np.abs(sm["mesh_verts"].astype(np.float64) - fm["mesh_verts"])))
    mesh["anchor_attr"] = np.float64(max(rel_error(fm["mesh_conf"], sm["mesh_conf"]), rel_error(fm["mesh_values"], sm["mesh_values"])))
    np.savez_compressed(os.path.join(HERE, "fssr_f1_mesh.npz"), **mesh)

    print("F1: %d samples, %d nodes, %d voxels (%d empty, max n %d); mesh %d vertices, %d faces"
          % (len(out["samples"]), len(out["nodes"]), len(out["positions"]), (~nonempty).sum(), sv["vox_n"].max(),
             len(mesh["verts"]), len(mesh["faces"])))
    print("anchors:", {q: float(out["anchor_" + q]) for q in QUANTITIES}, "mesh pos %.3g attr %.3g" % (mesh["anchor_pos"], mesh["anchor_attr"]))
    for fn in ("fssr_f1.npz", "fssr_f1_mesh.npz"):
        print(fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")
    if not a.keep:
        shutil.rmtree(work)


if __name__ == "__main__":
    main()
