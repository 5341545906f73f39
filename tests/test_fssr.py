"""The FSSR stage: fssr::IsoOctree::sample_ifn on the GPU (mve_amd/csrc/fssr_device.hip behind mi_dmrecon_fssr_*) and the
drop-in build/fssrecon_mi, against fixture F1 (tests/golden/make_golden_fssr.py: the strict build of the reference, with
the error between the reference's strict and fast builds as the yardstick of every tolerance).

Error measure (fssr_restatement.rel_error): for a quantity q, max over the non-empty voxels of
|q - q_strict| / (|q_strict| + median |q_strict|); asserted <= 8 * max(anchor_q, 2^-23), anchor_q being the same
expression between the reference's two builds.  The mesh: max |position difference| <= min(8 * max(anchor_pos, one float
ulp of the largest coordinate), 1e-3 * the smallest sample scale); confidences and values as the voxel quantities.

The measured errors stand in the docstrings of the GPU tests and in DESIGN.md, section 11."""
import os
import re
import subprocess

import numpy as np
import pytest

import fssr_restatement as R
from mve_amd import api
from mve_amd.scene2pset import write_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
APP = os.path.join(ROOT, "build", "fssrecon_mi")
NAMES = ["mi_dmrecon_fssr_options_default", "mi_dmrecon_fssr_create", "mi_dmrecon_fssr_sample", "mi_dmrecon_fssr_destroy"]
OUTPUTS = R.QUANTITIES + ("n_influencing", "max_scale")


@pytest.fixture(scope="module")
def f1():
    return dict(np.load(os.path.join(GOLDEN, "fssr_f1.npz")))


@pytest.fixture(scope="module")
def f1_mesh():
    return dict(np.load(os.path.join(GOLDEN, "fssr_f1_mesh.npz")))


@pytest.fixture(scope="module")
def pairs(f1):
    """(voxel, sample) pairs of the influence query, brute force in double."""
    return R.influence_pairs(f1["samples"], f1["positions"])


def bound(f1, q):
    return 8.0 * max(float(f1["anchor_" + q]), 2.0 ** -23)


# ---------------------------------------------------------------------------------------------------------- CPU

def test_header_library_and_api_agree_on_the_entry_points():
    src = open(os.path.join(ROOT, "include", "mi_dmrecon.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = api.load_library()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), "include/mi_dmrecon.h does not declare %s" % n
        assert hasattr(L, n), "libmi_dmrecon.so does not export %s" % n
        assert n in api.EXPORTS
    assert ctypes_sizes() == (44, 16, 4)


def ctypes_sizes():
    import ctypes
    return ctypes.sizeof(api.CFssrSample), ctypes.sizeof(api.CFssrNode), ctypes.sizeof(api.CFssrOptions)


def test_restatement_reproduces_f1(f1):
    """Pins the fixture and the semantics without a GPU: the NumPy restatement of the kernel's arithmetic against the
    strict build of the reference -- n and sample_max_scale exactly, the outputs inside the tolerance of the GPU test."""
    o = R.sample(f1["samples"], f1["positions"])
    assert np.array_equal(o["n_influencing"], f1["n_influencing"])
    assert np.array_equal(o["max_scale"], f1["max_scale"])
    nonempty = f1["n_influencing"] > 0
    for q in R.QUANTITIES:
        err = R.rel_error(o[q], f1[q], nonempty)
        print("restatement err_%s = %.3g (bound %.3g)" % (q, err, bound(f1, q)))
        assert err <= bound(f1, q), (q, err)
        assert not np.any(o[q][~nonempty]) and not np.any(f1[q][~nonempty])


def test_f1_tree_is_well_formed(f1):
    """What mi_dmrecon_fssr_create demands of a tree holds for the fixture's, and its samples are in walk order."""
    nodes, S = f1["nodes"], len(f1["samples"])
    fc = nodes[:, 0]
    idx = np.arange(len(nodes))
    inner = fc >= 0
    assert np.all((fc == -1) | ((fc > idx) & (fc <= len(nodes) - 8)))
    assert np.all(nodes[:, 1] >= 0) and np.all(nodes[:, 2] >= 0) and np.all(nodes[:, 1] + nodes[:, 2] <= S)
    assert nodes[:, 2].sum() == S and len(np.unique(fc[inner])) == inner.sum()
    # depth first from the root: every node's own samples directly follow those visited before it
    nxt, stack = 0, [0]
    while stack:
        i = stack.pop()
        assert nodes[i, 1] == nxt
        nxt += nodes[i, 2]
        if fc[i] >= 0:
            stack.extend(range(fc[i] + 7, fc[i] - 1, -1))
    assert nxt == S


def test_f1_coverage(f1, pairs):
    """A regenerated fixture cannot silently lose the cases it exists for."""
    n = f1["n_influencing"]
    assert np.any(n == 0) and np.any((n >= 1) & (n < 10)) and np.any(n > 128)
    assert n.max() > 16                                    # the forced small list_capacity of the GPU test is exceeded
    vi, si = pairs
    assert np.array_equal(np.bincount(vi, minlength=len(n)), n)
    # a tie at position floor(n/10): the scale there occurs more than once among the voxel's samples
    scale = f1["samples"][si, 9]
    order = np.lexsort((scale, vi))
    ss, start = scale[order], np.concatenate([[0], np.cumsum(n)])[:-1]
    k = (start + n // 10)[n > 1]
    lo, hi = start[n > 1], (start + n)[n > 1]
    tie = ((k + 1 < hi) & (ss[np.minimum(k + 1, len(ss) - 1)] == ss[k])) | ((k > lo) & (ss[k - 1] == ss[k]))
    assert tie.sum() > 10
    # every branch of rotation_from_normal is taken by a sample that influences some voxel
    nrm = f1["samples"][:, 3:6]
    ident = np.all(nrm == np.float32([1, 0, 0]), 1)
    mirror = np.all(nrm == np.float32([-1, 0, 0]), 1)
    near = np.all(np.abs(nrm - np.float32([1, 0, 0])) <= np.float32(0.001), 1) & ~ident
    for name, sel in (("(1,0,0)", ident), ("(-1,0,0)", mirror), ("near (1,0,0)", near)):
        assert sel.sum() >= 1, name
        assert np.isin(si, np.nonzero(sel)[0]).any(), "no voxel is influenced by the sample with normal " + name
    assert np.all(f1["samples"][:, 10] > 0)


# ---------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpu_default(ctx, f1):
    """F1 through the tree walk with the default list capacity: computed once, shared, never modified."""
    s = ctx.fssr_open(f1["samples"], f1["nodes"], f1["root"][:3], float(f1["root"][3]))
    out = s.sample(f1["positions"])
    s.close()
    return out


@pytest.mark.gpu
def test_gpu_against_the_reference(f1, gpu_default):
    """n_influencing and sample_max_scale exactly; value, conf, scale, color, deriv inside 8 x the error between the
    reference's own two builds; empty voxels exactly zero.

    Measured on the MI355X (F1, 22004 voxels; anchor / bound in brackets): err_value 0 (7.28e-07 / 5.82e-06), err_conf
    3.53e-15 (2.02e-07 / 1.61e-06), err_scale 0 (1.12e-06 / 8.95e-06), err_color 0 (2.56e-04 / 2.05e-03), err_deriv 0
    (3.79e-06 / 3.03e-05): every float but one near-zero confidence is the strict reference's."""
    o = gpu_default
    assert np.array_equal(o["n_influencing"], f1["n_influencing"])
    assert np.array_equal(o["max_scale"], f1["max_scale"])
    nonempty = f1["n_influencing"] > 0
    errs = {q: R.rel_error(o[q], f1[q], nonempty) for q in R.QUANTITIES}
    for q in R.QUANTITIES:
        print("gpu err_%s = %.3g (anchor %.3g, bound %.3g)" % (q, errs[q], float(f1["anchor_" + q]), bound(f1, q)))
    for q in R.QUANTITIES:
        assert errs[q] <= bound(f1, q), (q, errs[q], bound(f1, q))
        assert not np.any(o[q][~nonempty])


@pytest.mark.gpu
def test_gpu_paths_agree_bit_for_bit(ctx, f1, gpu_default):
    """The listed path (default), the re-walk path (list_capacity 16: most voxels exceed it) and the walk without a tree
    (n_nodes = 0, every sample tested in index order) add the same terms to the same lanes in the same order."""
    tree = ctx.fssr_open(f1["samples"], f1["nodes"], f1["root"][:3], float(f1["root"][3]))
    rewalk = tree.sample(f1["positions"], list_capacity=16)
    tree.close()
    flat = ctx.fssr_open(f1["samples"])
    brute = flat.sample(f1["positions"])
    brute16 = flat.sample(f1["positions"], list_capacity=16)
    flat.close()
    for k in OUTPUTS:
        for name, other in (("list_capacity=16", rewalk), ("n_nodes=0", brute), ("n_nodes=0, list_capacity=16", brute16)):
            assert np.array_equal(gpu_default[k], other[k], equal_nan=True), (k, name)


@pytest.mark.gpu
def test_gpu_lists_longer_than_the_on_chip_part(ctx):
    """1500 samples in a small ball, no tree: most voxels are influenced by more samples than the 1024 a wavefront lists in
    LDS, so their lists continue in global memory.  The re-walk path (list_capacity 16 and 1100) gives the same bits; n and
    sample_max_scale equal the NumPy restatement's exactly, the outputs to rounding: the restatement (pinned to the
    reference on F1) differs by the order of <= 1500 double additions and by exp / pow / sqrt, ~1e-13 relative before the
    narrowing to float, so the floor of the tolerance, 8 * 2^-23 in the error measure of this file, is the bound."""
    rng = np.random.default_rng(7)
    S = 1500
    d = rng.normal(size=(S, 3))
    nrm = d / np.linalg.norm(d, axis=1, keepdims=True)
    samples = np.zeros((S, 11), np.float32)
    samples[:, 0:3] = rng.uniform(-0.02, 0.02, size=(S, 3))
    samples[:, 3:6] = nrm
    samples[:, 6:9] = rng.integers(0, 256, size=(S, 3)) / 255.0
    samples[:, 9] = np.where(np.arange(S) % 3 == 0, rng.uniform(0.05, 0.1, S), np.float32([0.05, 0.0625, 0.08])[rng.integers(0, 3, S)])
    samples[:, 10] = rng.uniform(0.2, 1.0, S)
    v = rng.normal(size=(96, 3))
    positions = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.0, 0.3, size=(96, 1))
    expect = R.sample(samples, positions)
    n = expect["n_influencing"]
    assert (n > 1024).sum() >= 16 and (n <= 1024).sum() >= 16 and n.max() == S
    s = ctx.fssr_open(samples)
    out = s.sample(positions)
    rewalk = [s.sample(positions, list_capacity=c) for c in (16, 1100)]
    s.close()
    assert np.array_equal(out["n_influencing"], n) and np.array_equal(out["max_scale"], expect["max_scale"])
    for k in OUTPUTS:
        for other in rewalk:
            assert np.array_equal(out[k], other[k], equal_nan=True), k
    for q in R.QUANTITIES:
        err = R.rel_error(out[q], expect[q], n > 0)
        print("dense err_%s = %.3g" % (q, err))
        assert err <= 8.0 * 2.0 ** -23, (q, err)


@pytest.mark.gpu
def test_gpu_is_deterministic(ctx, f1, gpu_default):
    s = ctx.fssr_open(f1["samples"], f1["nodes"], f1["root"][:3], float(f1["root"][3]))
    a = s.sample(f1["positions"])
    b = s.sample(f1["positions"][:1001])                   # another chunk size, the same voxels
    s.close()
    for k in OUTPUTS:
        assert np.array_equal(a[k], gpu_default[k], equal_nan=True), k
        assert np.array_equal(b[k], gpu_default[k][:1001], equal_nan=True), k


@pytest.mark.gpu
def test_gpu_malformed_trees_are_refused_on_the_host(ctx, f1):
    """EINVAL (ValueError) before anything is uploaded or launched."""
    root = (f1["root"][:3], float(f1["root"][3]))
    good = f1["nodes"]
    parent = int(np.nonzero(good[:, 0] > 0)[0][1])          # an inner node other than the root

    def broken(row, col, val):
        n = good.copy()
        n[row, col] = val
        return n

    cases = {
        "child before its parent": broken(parent, 0, parent - 1),
        "child is the node itself": broken(parent, 0, parent),
        "sample range out of bounds": broken(len(good) - 1, 2, len(f1["samples"]) + 1),
        "negative sample count": broken(3, 2, -1),
        "first_child = n_nodes - 7": broken(parent, 0, len(good) - 7),
    }
    for name, nodes in cases.items():
        with pytest.raises(ValueError):
            ctx.fssr_open(f1["samples"], nodes, *root)
    with pytest.raises(ValueError):
        ctx.fssr_open(f1["samples"], good, root[0], 0.0)
    with pytest.raises(ValueError):
        ctx.fssr_open(f1["samples"], good, root[0], float("inf"))
    bad = f1["samples"].copy()
    bad[5, 9] = 0.0
    with pytest.raises(ValueError):
        ctx.fssr_open(bad, good, *root)
    # a chain deeper than 21 levels: node i's child 0 is node 1 + 8 i
    deep = np.zeros((1 + 8 * 22, 4), np.int32)
    deep[:, 0] = -1
    deep[0, 0] = 1
    for lvl in range(1, 22):
        deep[1 + 8 * (lvl - 1), 0] = 1 + 8 * lvl
    with pytest.raises(ValueError):
        ctx.fssr_open(f1["samples"][:0], deep, *root)
    ok = deep.copy()
    ok[1 + 8 * 19, 0] = -1                                  # 21 levels are allowed
    ctx.fssr_open(f1["samples"][:0], ok, *root).close()
    # the context still works
    s = ctx.fssr_open(f1["samples"], good, *root)
    o = s.sample(f1["positions"][:64])
    s.close()
    assert np.array_equal(o["n_influencing"], f1["n_influencing"][:64])


def read_ply_mesh(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    tmap = {"float": "<f4", "uchar": "u1", "int": "<i4", "uint": "<u4"}
    fields, nv, nf, elem = [], 0, 0, None
    for line in raw[:end].decode("ascii").splitlines():
        t = line.split()
        if t[:1] == ["element"]:
            elem = t[1]
            if elem == "vertex":
                nv = int(t[2])
            elif elem == "face":
                nf = int(t[2])
        elif t[:1] == ["property"] and elem == "vertex":
            fields.append((t[2], tmap[t[1]]))
    assert b"format binary_little_endian" in raw[:end] and b"property list uchar int vertex_indices" in raw[:end]
    v = np.frombuffer(raw, np.dtype(fields), nv, end)
    f = np.frombuffer(raw, np.dtype([("n", "u1"), ("v", "<i4", 3)]), nf, end + v.nbytes)
    assert np.all(f["n"] == 3)
    return dict(verts=np.stack([v["x"], v["y"], v["z"]], 1), faces=f["v"].astype(np.uint32), conf=v["confidence"], values=v["value"])


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(APP), reason="build/fssrecon_mi not built (needs the reference tree at build time)")
def test_gpu_unmodified_apps_fssrecon_on_the_gpu_library(tmp_path, f1, f1_mesh):
    """MVE's own apps/fssrecon and libs/fssr minus iso_octree.cc, linked against mve_amd/host/fssr_iso_octree.cc and
    libmi_dmrecon.so, on F1's PLY: the mesh of the reference's strict build -- the same vertices and faces (the host code
    that orders them is the reference's own), positions / confidences / values to rounding.

    Measured on the MI355X: 8056 vertices and 16108 faces as the fixture, no face differs; position error 0 (anchor
    3.58e-07, bound 2.86e-06), confidence 9.27e-16, value 0 (anchor 5.98e-07, bound 4.79e-06)."""
    ply = str(tmp_path / "f1.ply")
    ps = {k[4:]: f1[k] for k in f1 if k.startswith("ply_")}
    write_ply(ply, ps, with_normals=True, with_scale=True, with_conf=True)
    out_ply = str(tmp_path / "f1_surface.ply")
    out = subprocess.run([APP, ply, out_ply], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Computing sampling of the implicit function..." in out.stdout
    assert "Sampling the implicit function at %d positions, fetch a beer..." % len(f1["positions"]) in out.stdout
    m = re.search(r"Generated (\d+) voxels, took (\d+)ms\.", out.stdout)
    assert m and int(m.group(1)) == len(f1["positions"])
    print(m.group(0))
    mesh = read_ply_mesh(out_ply)
    assert len(mesh["verts"]) == len(f1_mesh["verts"]) and len(mesh["faces"]) == len(f1_mesh["faces"])
    pos_err = float(np.max(np.abs(mesh["verts"].astype(np.float64) - f1_mesh["verts"])))
    ulp = float(np.spacing(np.float32(np.abs(f1_mesh["verts"]).max())))
    pos_bound = min(8.0 * max(float(f1_mesh["anchor_pos"]), ulp), 1e-3 * float(f1["samples"][:, 9].min()))
    attr_bound = 8.0 * max(float(f1_mesh["anchor_attr"]), 2.0 ** -23)
    conf_err, val_err = R.rel_error(mesh["conf"], f1_mesh["conf"]), R.rel_error(mesh["values"], f1_mesh["values"])
    print("mesh: position error %.3g (bound %.3g), confidence %.3g, value %.3g (bound %.3g), faces that differ: %d"
          % (pos_err, pos_bound, conf_err, val_err, attr_bound, (mesh["faces"] != f1_mesh["faces"]).any(1).sum()))
    assert np.array_equal(mesh["faces"], f1_mesh["faces"])
    assert pos_err <= pos_bound
    assert conf_err <= attr_bound and val_err <= attr_bound
