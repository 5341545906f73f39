"""The FSSR stage: fssr::IsoOctree::sample_ifn on the GPU (mve_amd/csrc/fssr_device.hip behind mi_dmrecon_fssr_*) and the
drop-in build/fssrecon_mi, against fixtures F1 and F2 (tests/golden/make_golden_fssr.py: the strict build of the reference,
with the error between the reference's strict and fast builds as the yardstick of every tolerance) and, where no tree is
involved, against the NumPy restatement (fssr_restatement.py, itself pinned to the reference on F1 and F2).

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


@pytest.fixture(scope="module")
def f2():
    """Fixture F2 (make_golden_fssr.py --fixture f2): a tree of 21 levels, lists of more than 1024 samples.  The node and
    sample arrays are whole; of the voxels a fixed subset is stored (voxel_index into the reference's n_voxels_full)."""
    return dict(np.load(os.path.join(GOLDEN, "fssr_f2.npz")))


@pytest.fixture(scope="module")
def pairs2(f2):
    return R.influence_pairs(f2["samples"], f2["positions"])


def bound(f1, q):
    return 8.0 * max(float(f1["anchor_" + q]), 2.0 ** -23)


FLOOR = 8.0 * 2.0 ** -23                                   # bound(., q) where the anchor is below one float ulp


def dense_samples(rng, S, half=0.02):
    """S samples in a cube of +-half whose supports (scales 0.05 .. 0.1) all overlap; two thirds of the scales take three
    values only: ties at the scale cut."""
    d = rng.normal(size=(S, 3))
    nrm = d / np.linalg.norm(d, axis=1, keepdims=True)
    samples = np.zeros((S, 11), np.float32)
    samples[:, 0:3] = rng.uniform(-half, half, size=(S, 3))
    samples[:, 3:6] = nrm
    samples[:, 6:9] = rng.integers(0, 256, size=(S, 3)) / 255.0
    samples[:, 9] = np.where(np.arange(S) % 3 == 0, rng.uniform(0.05, 0.1, S), np.float32([0.05, 0.0625, 0.08])[rng.integers(0, 3, S)])
    samples[:, 10] = rng.uniform(0.2, 1.0, S)
    return samples


def dense_positions(rng, V):
    v = rng.normal(size=(V, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.0, 0.3, size=(V, 1))


@pytest.fixture(scope="module")
def dense1500():
    """The input of test_gpu_lists_longer_than_the_on_chip_part and the restatement's result on it."""
    rng = np.random.default_rng(7)
    samples = dense_samples(rng, 1500)
    positions = dense_positions(rng, 96)
    return samples, positions, R.sample(samples, positions)


@pytest.fixture(scope="module")
def dense17000():
    """17000 samples, 64 positions: more accepted samples than the default list capacity (1024 in LDS + 15360 in global
    memory) holds."""
    rng = np.random.default_rng(17)
    samples = dense_samples(rng, 17000)
    positions = dense_positions(rng, 64)
    return samples, positions, R.sample(samples, positions)


def ties_at_the_cut(samples, n, vi, si):
    """Voxels whose floor(n/10)-th smallest scale occurs more than once among the voxel's samples."""
    scale = samples[si, 9]
    order = np.lexsort((scale, vi))
    ss, start = scale[order], np.concatenate([[0], np.cumsum(n)])[:-1]
    k = (start + n // 10)[n > 1]
    lo, hi = start[n > 1], (start + n)[n > 1]
    tie = ((k + 1 < hi) & (ss[np.minimum(k + 1, len(ss) - 1)] == ss[k])) | ((k > lo) & (ss[k - 1] == ss[k]))
    return int(tie.sum())


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
    restatement_reproduces(f1)


def test_restatement_reproduces_f2(f2):
    """The same on F2: 21 levels do not matter to the brute-force restatement, lists of up to 1316 samples do."""
    restatement_reproduces(f2)


def restatement_reproduces(f1):
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
    tree_is_well_formed(f1)


def test_f2_tree_is_well_formed(f2):
    tree_is_well_formed(f2)


def tree_is_well_formed(f1):
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
    assert ties_at_the_cut(f1["samples"], n, vi, si) > 10
    # every branch of rotation_from_normal is taken by a sample that influences some voxel
    nrm = f1["samples"][:, 3:6]
    ident = np.all(nrm == np.float32([1, 0, 0]), 1)
    mirror = np.all(nrm == np.float32([-1, 0, 0]), 1)
    near = np.all(np.abs(nrm - np.float32([1, 0, 0])) <= np.float32(0.001), 1) & ~ident
    for name, sel in (("(1,0,0)", ident), ("(-1,0,0)", mirror), ("near (1,0,0)", near)):
        assert sel.sum() >= 1, name
        assert np.isin(si, np.nonzero(sel)[0]).any(), "no voxel is influenced by the sample with normal " + name
    assert np.all(f1["samples"][:, 10] > 0)


def test_f2_coverage(f2, pairs2):
    """What F2 exists for, asserted on the stored file: a walk over all 21 levels with samples on each of 5 .. 20 (and
    below the max_level clamp, octree.cc:257), nodes with more samples than one pass of the wavefront takes, inner nodes with
    samples of their own, lists that continue in global memory, and stored voxels that the deepest samples influence."""
    nodes, samples, n = f2["nodes"], f2["samples"], f2["n_influencing"]
    nlvl, slvl = R.node_levels(nodes), R.sample_levels(nodes, len(samples))
    assert nlvl.min() >= 0 and nlvl.max() == 20            # 21 levels: FSSR_MAX_LEVELS
    assert set(range(5, 21)) <= set(slvl.tolist())
    assert np.any(samples[slvl == 20, 9].astype(np.float64) < float(f2["root"][3]) / 2.0 ** 20)
    cnt = nodes[:, 2]
    assert np.any((cnt > 64) & (cnt % 64 != 0))
    assert ((nodes[:, 0] >= 0) & (cnt > 0)).sum() >= 20
    assert (n > 1024).sum() >= 50 and np.any(n == 0)
    vi, si = pairs2
    assert np.array_equal(np.bincount(vi, minlength=len(n)), n)
    assert np.any(slvl[si] == 20)                          # a stored voxel within 3 x scale of a level-20 sample
    assert ties_at_the_cut(samples, n, vi, si) > 10
    # the stored subset: a strictly ascending index into the reference's voxels
    idx = f2["voxel_index"]
    assert len(idx) == len(n) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < int(f2["n_voxels_full"])


def test_dense_inputs_reach_every_list_regime(dense1500, dense17000):
    """The inputs of the GPU tests without a tree, on the restatement: lists inside LDS, continued in global memory, and
    past the default capacity of 16384; and the order of the double sums is invisible after the narrowing to float -- the
    restatement against itself with the samples shuffled stays within a quarter of the floor bound, so the margin of the
    GPU tests belongs to the kernel."""
    n = dense1500[2]["n_influencing"]
    assert (n > 1024).sum() >= 16 and (n <= 1024).sum() >= 16 and n.max() == 1500
    samples, positions, expect = dense17000
    n = expect["n_influencing"]
    assert (n > 16384).sum() >= 4 and ((n > 1024) & (n <= 16384)).sum() >= 4 and (n <= 1024).sum() >= 4
    shuffled = R.sample(samples[np.random.default_rng(3).permutation(len(samples))], positions)
    assert np.array_equal(shuffled["n_influencing"], n) and np.array_equal(shuffled["max_scale"], expect["max_scale"])
    for q in R.QUANTITIES:
        err = R.rel_error(shuffled[q], expect[q], n > 0)
        print("shuffled err_%s = %.3g" % (q, err))
        assert err <= FLOOR / 4.0, (q, err)


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
def test_gpu_lists_longer_than_the_on_chip_part(ctx, dense1500):
    """1500 samples in a small ball, no tree: most voxels are influenced by more samples than the 1024 a wavefront lists in
    LDS, so their lists continue in global memory.  The re-walk path (list_capacity 16 and 1100) gives the same bits; n and
    sample_max_scale equal the NumPy restatement's exactly, the outputs to rounding: the restatement (pinned to the
    reference on F1) differs by the order of <= 1500 double additions and by exp / pow / sqrt, ~1e-13 relative before the
    narrowing to float, so the floor of the tolerance, 8 * 2^-23 in the error measure of this file, is the bound."""
    samples, positions, expect = dense1500
    S = len(samples)
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


# ---------------------------------------------------------------------------------------------------------- GPU: fixture F2

def open_tree(ctx, fx):
    return ctx.fssr_open(fx["samples"], fx["nodes"], fx["root"][:3], float(fx["root"][3]))


def assert_same_bits(a, b, what, rows=None):
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k] if rows is None else b[k][rows], equal_nan=True), (k, what)


def assert_floor(out, expect, tag):
    """n and sample_max_scale exactly, the quantities at the floor of the tolerance, empty voxels exactly zero."""
    n = expect["n_influencing"]
    assert np.array_equal(out["n_influencing"], n) and np.array_equal(out["max_scale"], expect["max_scale"])
    errs = {q: R.rel_error(out[q], expect[q], n > 0) for q in R.QUANTITIES}
    print(tag, " ".join("err_%s = %.3g" % (q, errs[q]) for q in R.QUANTITIES))
    for q in R.QUANTITIES:
        assert errs[q] <= FLOOR, (q, errs[q])
        assert not np.any(out[q][n == 0])


@pytest.fixture(scope="module")
def gpu_f2_default(ctx, f2):
    """F2 through the tree walk with the default list capacity: computed once, shared, never modified."""
    s = open_tree(ctx, f2)
    out = s.sample(f2["positions"])
    s.close()
    return out


@pytest.mark.gpu
def test_gpu_f2_against_the_reference(f2, gpu_f2_default):
    """The assertions of test_gpu_against_the_reference on F2 with F2's own anchors: a walk over 21 levels, nodes of up to
    1300 samples, 115 lists that continue in global memory.

    Measured on the MI355X (F2, 10107 stored voxels; anchor / bound in brackets): err_value 0 (1.14e-04 / 9.08e-04), err_conf
    2.98e-14 (1.86e-07 / 1.49e-06), err_scale 0 (2.07e-06 / 1.66e-05), err_color 0 (4.99e-04 / 3.99e-03), err_deriv 0
    (2.35e-04 / 1.88e-03)."""
    o = gpu_f2_default
    assert np.array_equal(o["n_influencing"], f2["n_influencing"])
    assert np.array_equal(o["max_scale"], f2["max_scale"])
    nonempty = f2["n_influencing"] > 0
    errs = {q: R.rel_error(o[q], f2[q], nonempty) for q in R.QUANTITIES}
    for q in R.QUANTITIES:
        print("gpu f2 err_%s = %.3g (anchor %.3g, bound %.3g)" % (q, errs[q], float(f2["anchor_" + q]), bound(f2, q)))
    for q in R.QUANTITIES:
        assert errs[q] <= bound(f2, q), (q, errs[q], bound(f2, q))
        assert not np.any(o[q][~nonempty])


@pytest.mark.gpu
def test_gpu_f2_paths_agree_bit_for_bit(ctx, f2, gpu_f2_default):
    """Default, list_capacity 16 and the walk without a tree on F2.  The last is the statement that pruning over 21 levels
    never drops an influencing sample (and that the explicit stack returns to the right sibling from any depth)."""
    tree = open_tree(ctx, f2)
    rewalk = tree.sample(f2["positions"], list_capacity=16)
    tree.close()
    flat = ctx.fssr_open(f2["samples"])
    brute = flat.sample(f2["positions"])
    flat.close()
    assert_same_bits(gpu_f2_default, rewalk, "list_capacity=16")
    assert_same_bits(gpu_f2_default, brute, "n_nodes=0")


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(APP), reason="build/fssrecon_mi not built (needs the reference tree at build time)")
def test_gpu_apps_fssrecon_on_f2(tmp_path, f2):
    """The shim's own flattening of a 21-level octree (mve_amd/host/fssr_iso_octree.cc, other code than the fixture's
    driver) passes mi_dmrecon_fssr_create, and the app samples every voxel of F2, not only the stored ones."""
    ply = str(tmp_path / "f2.ply")
    write_ply(ply, {k[4:]: f2[k] for k in f2 if k.startswith("ply_")}, with_normals=True, with_scale=True, with_conf=True)
    out = subprocess.run([APP, ply, str(tmp_path / "f2_surface.ply")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"Generated (\d+) voxels, took (\d+)ms\.", out.stdout)
    assert m and int(m.group(1)) == int(f2["n_voxels_full"])
    print(m.group(0))


# ------------------------------------------------------------------------------- GPU: lists in global memory, no tree

CUS = 256   # the MI355X's compute units.  A CU holds at most 32 wavefronts, so the grid is at most 8 blocks per CU


@pytest.mark.gpu
def test_gpu_global_lists_are_reused(ctx, dense1500):
    """The 96 positions of test_gpu_lists_longer_than_the_on_chip_part and 32 far outside (n = 0), tiled at random to
    96 x CUS voxels: every wavefront of the grid works through at least three voxels, so a list in its slice of the global
    buffer is followed by a shorter, a longer or an empty one on the same slice.  A voxel's result does not depend on its
    neighbours: all copies of a position are bit-identical, and equal the restatement's row -- n and sample_max_scale
    exactly, the quantities at the floor of the tolerance (the argument of that test's docstring); the re-walk path
    (list_capacity 16 and 1100) gives the same bits.

    Measured on the MI355X (24576 voxels): every error 0 (bound 9.54e-07): each float is the restatement's."""
    samples, positions, _ = dense1500
    rng = np.random.default_rng(23)
    base = np.concatenate([positions, 10.0 + rng.uniform(-1.0, 1.0, size=(32, 3))])
    expect = R.sample(samples, base)
    assert np.all(expect["n_influencing"][96:] == 0)
    tile = rng.integers(0, len(base), 96 * CUS)
    uniq, first = np.unique(tile, return_index=True)
    assert len(uniq) == len(base)
    s = ctx.fssr_open(samples)
    out = s.sample(base[tile])
    rewalk = [s.sample(base[tile], list_capacity=c) for c in (16, 1100)]
    s.close()
    for other in rewalk:
        assert_same_bits(out, other, "re-walk")
    rows = {k: out[k][first] for k in OUTPUTS}             # one copy of each position, in the order of `base` ...
    assert_same_bits(out, rows, "copies of one position differ", tile)     # ... and every copy has its bits
    assert_floor(rows, expect, "reuse")


@pytest.mark.gpu
def test_gpu_more_samples_than_the_default_capacity(ctx, dense17000):
    """17000 samples without a tree: voxels with more accepted samples than the 16384 the default capacity lists fall back
    to walking again, next to voxels whose lists fit (in global memory, and in LDS alone).  The forced re-walk
    (list_capacity 16) gives the same bits; against the restatement n and sample_max_scale are exact and the quantities at
    the floor of the tolerance (test_dense_inputs_reach_every_list_regime: the order of the sums takes none of it).

    Measured on the MI355X: 27 / 29 / 8 of the 64 voxels above 16384 / in global memory / in LDS; every error 0 (bound 9.54e-07)."""
    samples, positions, expect = dense17000
    n = expect["n_influencing"]
    assert (n > 16384).sum() >= 4 and ((n > 1024) & (n <= 16384)).sum() >= 4 and (n <= 1024).sum() >= 4
    s = ctx.fssr_open(samples)
    out = s.sample(positions)
    rewalk = s.sample(positions, list_capacity=16)
    s.close()
    assert_same_bits(out, rewalk, "list_capacity=16")
    assert_floor(out, expect, "over capacity")


# ------------------------------------------------------------------------------- GPU: the host side of mi_dmrecon_fssr_sample

@pytest.mark.gpu
def test_gpu_two_chunks(ctx, f1, gpu_default):
    """2^18 + 1907 voxels are two launches, the second of a size that is no multiple of the four voxels of a block: every
    output of every voxel is the one of gpu_default for the position it repeats."""
    N, V = len(f1["positions"]), (1 << 18) + 1907
    rng = np.random.default_rng(29)
    idx = np.concatenate([rng.permutation(N) for _ in range(-(-V // N))])[:V]
    s = open_tree(ctx, f1)
    out = s.sample(f1["positions"][idx])
    s.close()
    assert_same_bits(out, gpu_default, "two chunks", idx)
    assert np.array_equal(out["n_influencing"], f1["n_influencing"][idx]) and np.array_equal(out["max_scale"], f1["max_scale"][idx])


@pytest.mark.gpu
def test_gpu_chunk_buffers_grow(ctx, f1, gpu_default):
    """1001 voxels, then all, then 64 on one handle: the per-chunk buffers are replaced by larger ones, then reused."""
    s = open_tree(ctx, f1)
    for m in (1001, len(f1["positions"]), 64):
        assert_same_bits(s.sample(f1["positions"][:m]), gpu_default, "%d voxels" % m, slice(0, m))
    s.close()


@pytest.mark.gpu
def test_gpu_null_outputs(ctx, f1, gpu_default):
    """mi_dmrecon_fssr_sample itself: only the outputs asked for are written (all of their rows), NULL options are the
    defaults, and a call that asks for everything afterwards is not disturbed."""
    L = api.load_library()
    V = 3001
    pos = np.ascontiguousarray(f1["positions"][:V])
    order = ("value", "conf", "scale", "color", "deriv", "n_influencing", "max_scale")
    s = open_tree(ctx, f1)
    for want in (("value", "n_influencing"), ("deriv",), order):
        bufs = {k: np.full_like(gpu_default[k][:V], -7) for k in order}
        rc = L.mi_dmrecon_fssr_sample(s._h, None, V, api._ptr(pos), *[api._ptr(bufs[k]) if k in want else None for k in order])
        assert rc == 0, want
        for k in order:
            if k in want:
                assert np.array_equal(bufs[k], gpu_default[k][:V], equal_nan=True), (k, want)
            else:
                assert np.all(bufs[k] == -7), (k, want)
    s.close()


@pytest.mark.gpu
def test_gpu_two_handles_on_one_context(ctx, f1, gpu_default, dense1500):
    """A tree and a flat sample set open on the same context (the same stream), called in turn: each keeps its own tree,
    lists and chunk buffers."""
    samples, positions, expect = dense1500
    P = f1["positions"]
    tree, flat = open_tree(ctx, f1), ctx.fssr_open(samples)
    a1 = tree.sample(P[:4000])
    b1 = flat.sample(positions)
    a2 = tree.sample(P[4000:9001])
    b2 = flat.sample(positions[::-1], list_capacity=16)
    a3 = tree.sample(P[:4000], list_capacity=16)
    b3 = flat.sample(positions)
    tree.close()
    b4 = flat.sample(positions)                             # closing one leaves the other whole
    flat.close()
    assert_same_bits(a1, gpu_default, "tree, first call", slice(0, 4000))
    assert_same_bits(a2, gpu_default, "tree, second call", slice(4000, 9001))
    assert_same_bits(a3, gpu_default, "tree, third call", slice(0, 4000))
    assert np.array_equal(b1["n_influencing"], expect["n_influencing"]) and np.array_equal(b1["max_scale"], expect["max_scale"])
    assert_same_bits(b2, b1, "flat, second call", slice(None, None, -1))
    assert_same_bits(b3, b1, "flat, third call")
    assert_same_bits(b4, b1, "flat, after the tree is closed")


# ------------------------------------------------------------------------------- GPU: boundary cases against the restatement

def flat_and_tree(ctx, samples, positions, root_size):
    """Without a tree and under a tree of one node (centre 0, size root_size): the same bits; returns them."""
    samples = np.ascontiguousarray(samples, np.float32)
    nodes = np.int32([[-1, 0, len(samples), 0]])
    outs = []
    for args in ((samples,), (samples, nodes, np.zeros(3), root_size)):
        s = ctx.fssr_open(*args)
        outs.append(s.sample(positions))
        s.close()
    assert_same_bits(outs[0], outs[1], "one-node tree against no tree")
    return outs[0]


def sample_row(pos, normal, scale, conf=1.0, color=(0.25, 0.5, 0.75)):
    return np.float32(list(pos) + list(normal) + list(color) + [scale, conf])


@pytest.mark.gpu
@pytest.mark.parametrize("normal", [(0, 0, 1), (1, 0, 0), (-1, 0, 0)], ids=["general", "identity", "mirror"])
def test_gpu_sample_on_the_acceptance_boundary(ctx, normal):
    """One sample of scale 0.25 at the origin; voxels at distance exactly 3 x scale on each axis, and one float64 step
    further.  The first are accepted (octree.cc:389 drops on >) but get weight 0 (basis_function.h: sr >= 9): n = 1, conf 0,
    value and deriv 0 / 0 = NaN, scale and color the sample's.  The second are empty: all zero.  The three normals take
    the three branches of rotation_from_normal."""
    samples = sample_row((0, 0, 0), normal, 0.25)[None]
    on = 0.75 * np.eye(3)
    positions = np.concatenate([on, np.nextafter(0.75, 1.0) * np.eye(3)])
    with np.errstate(all="ignore"):
        expect = R.sample(samples, positions)
    assert expect["n_influencing"].tolist() == [1, 1, 1, 0, 0, 0]
    assert np.all(expect["conf"] == 0) and np.all(np.isnan(expect["value"][:3])) and np.all(np.isnan(expect["deriv"][:3]))
    assert np.all(expect["scale"][:3] == np.float32(0.25)) and np.all(expect["max_scale"][:3] == np.float32(0.5))
    out = flat_and_tree(ctx, samples, positions, 1.0)
    for k in ("n_influencing", "max_scale", "conf"):
        assert np.array_equal(out[k], expect[k]), k
    for k in ("value", "deriv"):
        assert np.array_equal(np.isnan(out[k]), np.isnan(expect[k])), k
        assert np.array_equal(np.isfinite(out[k]), np.isfinite(expect[k])), k
    for k in R.QUANTITIES:
        assert not np.any(out[k][3:]), k
    # one term: scale = (0.25 * cw) / cw, exact whatever exp returns; the colour weight exp(-112.5) / ... is 0 as a float
    assert np.array_equal(out["scale"], expect["scale"]) and np.array_equal(out["color"], expect["color"])


@pytest.mark.gpu
def test_gpu_zero_weight_sample_in_a_finite_voxel(ctx):
    """The boundary sample next to one whose support holds the voxel: the zero weight adds nothing, the voxel is finite."""
    samples = np.stack([sample_row((0, 0, 0), (0, 0, 1), 0.25), sample_row((0.6, 0.1, 0), (0.6, 0.0, 0.8), 0.2, 0.5, (1, 0, 0.5))])
    positions = np.float64([[0.75, 0, 0], [0.5, 0.1, 0.05]])
    expect = R.sample(samples, positions)
    assert expect["n_influencing"].tolist() == [2, 2] and np.all(expect["max_scale"] == np.float32(0.4))
    assert all(np.all(np.isfinite(expect[q])) for q in R.QUANTITIES) and np.all(expect["conf"] > 0)
    out = flat_and_tree(ctx, samples, positions, 4.0)
    assert all(np.all(np.isfinite(out[q])) for q in R.QUANTITIES)
    assert_floor(out, expect, "zero weight")


@pytest.mark.gpu
def test_gpu_scales_from_1e_minus_30_to_1e30(ctx):
    """Three groups of four samples around one centre, scales about 1e-30, 1 and 1e30, each with six voxels at multiples of
    its scale: the bit patterns of the scales span the whole range the selection searches, the squares and fourth powers
    the range of double.  n and sample_max_scale exactly; per group, the quantities at the floor of the tolerance where
    the restatement is finite, and non-finite in the same places (the narrowing of 1 / scale^3 to float overflows for the
    smallest group).

    Measured on the MI355X: every error 0 (bound 9.54e-07); value and deriv of the smallest group are +-inf and NaN as the
    restatement's, those of the largest group 0: no voxel at which the device's exp / pow / sqrt show."""
    rng = np.random.default_rng(31)
    rows, vox = [], []
    for sc in (1e-30, 1.0, 1e30):
        for off in rng.uniform(-1.0, 1.0, size=(4, 3)):
            nrm = rng.normal(size=3)
            rows.append(sample_row(off * sc, nrm / np.linalg.norm(nrm), sc * rng.uniform(0.8, 1.25), rng.uniform(0.2, 1.0), rng.uniform(0, 1, 3)))
        vox.append(rng.uniform(-1.5, 1.5, size=(6, 3)) * sc)
    samples, positions = np.stack(rows), np.concatenate(vox)
    assert np.all(np.isfinite(samples))
    with np.errstate(all="ignore"):
        expect = R.sample(samples, positions)
    n = expect["n_influencing"]
    assert all(n[6 * g:6 * g + 6].max() > 0 for g in range(3)) and n.max() == 12
    out = flat_and_tree(ctx, samples, positions, 1e32)
    assert np.array_equal(out["n_influencing"], n) and np.array_equal(out["max_scale"], expect["max_scale"])
    for g in range(3):
        rows_g = np.arange(6 * g, 6 * g + 6)[n[6 * g:6 * g + 6] > 0]
        for q in R.QUANTITIES:
            if not np.any(expect[q][rows_g]):               # (value and deriv of the largest group: 1 / scale^3 underflows)
                assert not np.any(out[q][rows_g]), (g, q)
                continue
            err = R.rel_error(out[q], expect[q], rows_g)
            print("scale group %d err_%s = %.3g" % (g, q, err))
            assert err <= FLOOR, (g, q, err)


@pytest.mark.gpu
@pytest.mark.parametrize("distinct", [True, False], ids=["distinct", "equal"])
def test_gpu_lists_of_9_10_19_20(ctx, distinct):
    """floor(n / 10) steps from 0 to 1 between 9 and 10 accepted samples and from 1 to 2 between 19 and 20: four clusters
    far from each other, a voxel in each; scales all distinct (in no order), or all equal."""
    rng = np.random.default_rng(37)
    counts = (9, 10, 19, 20)
    rows, cut = [], []
    for c, cnt in enumerate(counts):
        sc = np.float32(0.1) * (1 + np.float32(0.01) * rng.permutation(cnt).astype(np.float32)) if distinct else np.full(cnt, 0.1, np.float32)
        cut.append(np.sort(sc)[cnt // 10] * np.float32(2.0))
        for j in range(cnt):
            nrm = rng.normal(size=3)
            rows.append(sample_row(np.float64([10.0 * c, 0, 0]) + rng.uniform(-0.02, 0.02, 3), nrm / np.linalg.norm(nrm), sc[j], rng.uniform(0.2, 1.0)))
    samples = np.stack(rows)
    positions = np.float64([[10.0 * c, 0.01, -0.01] for c in range(len(counts))])
    expect = R.sample(samples, positions)
    assert expect["n_influencing"].tolist() == list(counts)
    assert np.array_equal(expect["max_scale"], np.float32(cut))
    assert not distinct or all(len(set(samples[si:si + c, 9].tolist())) == c for si, c in zip(np.cumsum((0,) + counts), counts))
    out = flat_and_tree(ctx, samples, positions, 100.0)
    assert_floor(out, expect, "n / 10")
