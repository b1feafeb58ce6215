"""k-medoids on the GPU (po_kmedoids*): every case the reference's KMedoids recorded (tests/golden/kmedoids.npz), the two
kernels the loop is made of at awkward shapes, end-to-end runs against the numpy restatement, refusals, the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmedoids_ref  # noqa: E402

import phyloligo_amd as pa  # noqa: E402
from phyloligo_amd import _lib, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kmedoids.npz")
CASES = kmedoids_ref.cases()
# order-of-summation noise of float64 sums of n <= 1100 non-negative terms is about n 2^-53 ~ 1e-13
COST_RTOL = 1e-12


@pytest.fixture(scope="module")
def ctx():
    with pa.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _rand_matrix(n, dtype, seed=0):
    rng = np.random.RandomState(seed)
    m = rng.rand(n, n)
    m = (m + m.T) * 0.5
    np.fill_diagonal(m, 0.0)
    return m.astype(dtype)


# ---- 1. the recorded cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [c[0] for c in CASES])
def test_golden_cases(ctx, torch, key):
    g = np.load(GOLDEN)
    _, make, k, init, max_iter = next(c for c in CASES if c[0] == key)
    d = np.array(make())                                              # (a writable copy: torch wraps it)
    want_labels, want_medoids, want_iter = g[key + "_labels"].astype(np.int32), g[key + "_medoids"], int(g[key + "_n_iter"])
    start = "heuristic" if init is None else init
    labels, medoids, st = ctx.kmedoids(d, k, max_iter=max_iter, init=start, want_stats=True)
    assert labels.dtype == np.int32 and medoids.dtype == np.int32
    assert np.array_equal(labels, want_labels) and np.array_equal(medoids, want_medoids) and st["iterations"] == want_iter
    assert st["empty_clusters"] == int((np.bincount(want_labels, minlength=k) == 0).sum())
    if st["converged"]:
        np.testing.assert_allclose(st["inertia"], kmedoids_ref.inertia(d, want_labels, want_medoids), rtol=COST_RTOL)
    t_labels, t_medoids, t_st = ctx.kmedoids(torch.from_numpy(d).cuda(), k, max_iter=max_iter, init=start, want_stats=True)
    assert t_labels.is_cuda and t_labels.dtype == torch.int32 and t_medoids.dtype == torch.int32
    assert np.array_equal(t_labels.cpu().numpy(), want_labels) and np.array_equal(t_medoids.cpu().numpy(), want_medoids)
    assert t_st["iterations"] == want_iter and t_st["inertia"] == st["inertia"]


def test_empty_cluster_and_iteration_cap_details(ctx):
    g = np.load(GOLDEN)
    d = kmedoids_ref.empty_cluster_matrix()
    labels, medoids, st = ctx.kmedoids(d, 4, init=np.array(kmedoids_ref.EMPTY_START), want_stats=True)
    assert list(np.bincount(labels)) == [150, 2, 273, 175] and list(medoids) == [103, 9, 336, 329]
    assert st["iterations"] == 4 and st["converged"] and st["empty_clusters"] == 0
    # one pass only: cluster 1 is still empty, its medoid stays, the labels are those of the first assignment
    labels, medoids, st = ctx.kmedoids(d, 4, init=np.array(kmedoids_ref.EMPTY_START), max_iter=1, want_stats=True)
    assert st["iterations"] == 1 and not st["converged"] and st["empty_clusters"] == 1 and medoids[1] == 9
    assert np.array_equal(labels, kmedoids_ref.assign(d, kmedoids_ref.EMPTY_START))
    d = kmedoids_ref.matrix(600)
    labels, _, st = ctx.kmedoids(d, 7, init=kmedoids_ref.random_start(600, 7, 0), max_iter=2, want_stats=True)
    assert st["iterations"] == 2 and np.array_equal(labels, g["cap_labels"])


# ---- 2. masked row sums -----------------------------------------------------------------------------------------------------------
def _check_costs(ctx, d, labels, **kw):
    got = ctx.kmedoids_costs(d, labels, **kw)
    want = kmedoids_ref.masked_costs(d, labels, kw.get("rows"))
    assert got.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=COST_RTOL, atol=0.0)
    again = ctx.kmedoids_costs(d, labels, **kw)
    assert got.tobytes() == again.tobytes()
    return got


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1100])
def test_costs_shapes(ctx, n, dtype):
    d = _rand_matrix(n, dtype, seed=n)
    rng = np.random.RandomState(n + 1)
    for labels in (rng.randint(0, 5, n), np.zeros(n), np.arange(n), (np.arange(n) == n - 1) * 7):
        labels = labels.astype(np.int32)
        got = _check_costs(ctx, d, labels)
        if np.array_equal(labels, np.arange(n)):
            assert not got.any()                                     # n clusters of one member: the diagonal, exactly 0
    if n > 1:                                                        # one cluster holding only the last column
        labels = ((np.arange(n) == n - 1) * 7).astype(np.int32)
        assert ctx.kmedoids_costs(d, labels)[n - 1] == 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_costs_do_not_depend_on_layout_or_on_the_other_rows(ctx, torch, dtype):
    """rows that do not start on 16-byte boundaries (n = 257 with ld = n; a view with ld = n + 3; a view that starts one
    element into an aligned buffer) take the element-wise path: the same bytes as the 16-byte path, and the same bytes
    whichever other rows are in the launch"""
    n = 257
    d = _rand_matrix(n, dtype, seed=3)
    labels = np.random.RandomState(4).randint(0, 6, n).astype(np.int32)
    base = _check_costs(ctx, d, labels)                                # ld = n = 257: unaligned rows
    wide = np.zeros((n, n + 3), dtype=dtype)
    wide[:, :n] = d
    assert _check_costs(ctx, wide[:, :n], labels).tobytes() == base.tobytes()
    t_wide = torch.zeros((n, 264), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    t_wide[:, :n] = torch.from_numpy(d).cuda()                         # ld = 264: every row on a 16-byte boundary
    t_labels = torch.from_numpy(labels).cuda()
    got = ctx.kmedoids_costs(t_wide[:, :n], t_labels)
    assert got.is_cuda and got.cpu().numpy().tobytes() == base.tobytes()
    t_off = torch.zeros((n, 265), dtype=t_wide.dtype, device="cuda")
    t_off[:, 1:n + 1] = torch.from_numpy(d).cuda()                     # one element into the buffer, odd ld
    assert ctx.kmedoids_costs(t_off[:, 1:n + 1], t_labels).cpu().numpy().tobytes() == base.tobytes()
    for rows in ([5], [256], [0, 1, 2], [200, 3, 3, 77, 256, 0, 9]):
        rows = np.array(rows, dtype=np.int32)
        one = _check_costs(ctx, d, labels, rows=rows)
        assert one.tobytes() == base[rows].tobytes()
        assert ctx.kmedoids_costs(t_wide[:, :n], t_labels, rows=torch.from_numpy(rows).cuda()).cpu().numpy().tobytes() == base[rows].tobytes()


def test_loop_sums_are_the_costs_kernels_sums(ctx):
    """after a converged run the medoid of every cluster is its cheapest member, and the inertia is the sum of the medoids'
    costs: both through the bytes kmedoids_costs gives for those rows"""
    d = kmedoids_ref.matrix(600)
    labels, medoids, st = ctx.kmedoids(d, 7, want_stats=True)
    assert st["converged"]
    costs = ctx.kmedoids_costs(d, labels)
    for c in range(7):
        members = np.flatnonzero(labels == c)
        assert labels[medoids[c]] == c and costs[medoids[c]] == costs[members].min()
    np.testing.assert_allclose(st["inertia"], costs[medoids].sum(), rtol=COST_RTOL)


def test_a_nan_outside_the_cluster_stays_outside(ctx):
    n = 130
    d = _rand_matrix(n, np.float64, seed=9)
    labels = (np.arange(n) % 3).astype(np.int32)
    d[4, 5] = np.nan                                                  # row 4 is in cluster 1, column 5 in cluster 2
    d[7, 9] = np.inf
    got = ctx.kmedoids_costs(d, labels)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, kmedoids_ref.masked_costs(d, labels), rtol=COST_RTOL)


# ---- 3. assignment -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n, k", [(1, 1), (65, 1), (65, 65), (257, 6), (600, 300), (1027, 13)])
def test_assign(ctx, torch, n, k, dtype):
    d = _rand_matrix(n, dtype, seed=n + k)
    med = np.random.RandomState(k).permutation(n)[:k].astype(np.int32)
    want = np.argmin(d[med], axis=0)
    got = ctx.kmedoids_assign(d, med)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    wide = torch.zeros((n, n + 3), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    wide[:, :n] = torch.from_numpy(d).cuda()
    assert np.array_equal(ctx.kmedoids_assign(wide[:, :n], torch.from_numpy(med).cuda()).cpu().numpy(), want)


def test_assign_ties_go_to_the_smaller_cluster(ctx):
    n = 200
    d = _rand_matrix(n, np.float64, seed=1)
    d[17] = d[3]                                                      # two identical medoid rows
    med = np.array([50, 17, 3, 120], dtype=np.int32)
    got = ctx.kmedoids_assign(d, med)
    assert np.array_equal(got, np.argmin(d[med], axis=0)) and (got == 1).any() and not (got == 2).any()


# ---- 4. end to end against the restatement --------------------------------------------------------------------------------------------
_PROFILES = {}


def _profiles(ctx, n):
    if n not in _PROFILES:
        seq, offsets = synthetic.ragged_assembly(n, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
        _PROFILES[n] = ctx.count_profiles(seq, offsets, "1111", "both")
    return _PROFILES[n]


def _same_as_restatement(ctx, d, k, **kw):
    labels, medoids, st = ctx.kmedoids(d, k, want_stats=True, **kw)
    init = kw.get("init")
    w_labels, w_medoids, w_iter, w_conv = kmedoids_ref.kmedoids(d, k, kw.get("max_iter", 300), None if init is None else init)
    assert np.array_equal(labels, w_labels) and np.array_equal(medoids, w_medoids)
    assert st["iterations"] == w_iter and st["converged"] == w_conv
    return labels, medoids, st


@pytest.mark.parametrize("metric", ["JSD", "BC"])
def test_end_to_end_on_pairwise_matrices(ctx, metric):
    counts, totals = _profiles(ctx, 300)
    d = ctx.pairwise(counts, totals, metric)
    for k in (3, 8):
        _same_as_restatement(ctx, d, k)
    _same_as_restatement(ctx, d, 8, max_iter=1)
    _same_as_restatement(ctx, d, 5, init=kmedoids_ref.random_start(300, 5, 11))


def test_end_to_end_many_clusters(ctx):
    d = kmedoids_ref.matrix(600)
    labels, medoids, st = _same_as_restatement(ctx, d, 300)
    assert len(set(medoids.tolist())) == 300
    d = kmedoids_ref.matrix(257)
    labels, medoids, st = _same_as_restatement(ctx, d, 257)            # K = n: every row its own medoid
    assert sorted(medoids.tolist()) == list(range(257)) and st["inertia"] == 0.0 and st["iterations"] == 1
    assert np.array_equal(medoids[labels], np.arange(257))
    _same_as_restatement(ctx, kmedoids_ref.matrix(600, np.float32), 7, max_iter=1)
    wide = np.zeros((600, 603))                                        # a view into a wider array: ld = n + 3 through the host form
    wide[:, :600] = kmedoids_ref.matrix(600)
    _same_as_restatement(ctx, wide[:, :600], 7)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def _refused(call, *words):
    with pytest.raises(pa.PhyloligoError) as e:
        call()
    assert e.value.status == _lib.PO_EINVAL, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals_leave_the_context_usable(ctx, torch):
    n = 100
    d = _rand_matrix(n, np.float64, seed=2)
    t = torch.from_numpy(d).cuda()
    _refused(lambda: ctx.kmedoids(d, 0), "n_clusters")
    _refused(lambda: ctx.kmedoids(d, n + 1), "n_clusters")
    _refused(lambda: ctx.kmedoids(d, 3, max_iter=0), "max_iter")
    _refused(lambda: ctx.kmedoids(d, 3, init=np.array([4, 9, 4])), "twice", "row 4")
    _refused(lambda: ctx.kmedoids(d, 3, init=np.array([4, 9, n])), "init")
    _refused(lambda: ctx.kmedoids(torch.from_numpy(d), 3), "cuda:0")                    # a tensor on the wrong device
    _refused(lambda: ctx.kmedoids(torch.as_strided(t, (n, n), (n - 1, 1)), 3), "ld = 99", "n = 100")
    bad = d.copy()
    bad[41, 7] = np.nan
    _refused(lambda: ctx.kmedoids(bad, 3), "row 41 ", "NaN")
    _refused(lambda: ctx.kmedoids(torch.from_numpy(bad).cuda(), 3), "row 41 ", "NaN")
    _refused(lambda: ctx.kmedoids_costs(d, np.zeros(n, np.int32), rows=np.array([1, n], np.int32)), "rows[1]")
    _refused(lambda: ctx.kmedoids_assign(d, np.array([0, -1], np.int32)), "medoids[1]")
    # the library's own argument checks, past the Python layer
    lib = _lib.load()
    labels, medoids = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    start = np.array([1, 2, 2], dtype=np.int32)
    for k, init, it, ld, word in ((0, None, 300, n, "n_clusters = 0"), (n + 1, None, 300, n, "n_clusters = 101"), (3, None, 0, n, "max_iter"),
                                  (3, None, 300, n - 1, "ld = 99"), (3, start.ctypes.data, 300, n, "twice")):
        rc = lib.po_kmedoids_dev(ctx._h, t.data_ptr(), _lib.PO_F64, n, ld, k, init, it, labels.data_ptr(), medoids.data_ptr(), None)
        assert rc == _lib.PO_EINVAL and word in lib.po_last_error().decode(), lib.po_last_error().decode()
    # BC of two empty records is 0 / 0: refused with the heuristic start, and the context still works
    m = 24
    seq, offsets = synthetic.ragged_assembly(m, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
    parts = [seq[int(offsets[i]):int(offsets[i + 1])] for i in range(m)]
    parts[7] = parts[12] = seq[:0]
    off2 = np.zeros(m + 1, dtype=np.uint64)
    off2[1:] = np.cumsum([len(q) for q in parts])
    counts, totals = ctx.count_profiles(np.concatenate(parts), off2, "1111", "both")
    bc = ctx.pairwise(counts, totals, "BC")
    if np.isnan(bc).any():
        _refused(lambda: ctx.kmedoids(bc, 2), "row %d " % int(np.flatnonzero(np.isnan(bc.sum(axis=1)))[0]), "NaN")
    labels, medoids = ctx.kmedoids(d, 3)
    assert labels.shape == (n,) and np.array_equal(labels, kmedoids_ref.kmedoids(d, 3)[0])


# ---- 6. CLI ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_cli_kmedoids(ctx, tmp_path, dtype):
    n, k = 600, 4
    seq, offsets = synthetic.ragged_assembly(n, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
    fa = tmp_path / "asm.fa"
    fa.write_bytes(synthetic.fasta_bytes(seq, offsets))
    out, js = tmp_path / "clusters.txt", tmp_path / "stats.json"
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", str(fa), "-d", "Eucl", "--method", "joblib", "--kmedoids", str(k),
                        "--kmedoids-dtype", dtype, "-o", str(out), "--json-stats", str(js)], capture_output=True, text=True, timeout=600,
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    counts, totals = _profiles(ctx, n)
    want_labels, want_medoids, st = ctx.kmedoids(ctx.pairwise(counts, totals, "Eucl", dtype=dtype), k, want_stats=True)
    assert out.read_bytes() == b"".join(b"%d\n" % x for x in want_labels)
    labels = np.loadtxt(str(out), dtype=np.int64)
    species = np.arange(n) % 4                                          # record i of the assembly is of species i mod 4 (tsne_ref.make_input)
    for s in range(4):
        assert len(set(labels[species == s].tolist())) == 1                  # each species sits in one cluster
    assert sorted(np.bincount(labels).tolist()) == [150] * 4
    stats = json.load(open(js))
    assert stats["kmedoids"] == k and stats["kmedoids_medoids"] == want_medoids.tolist()
    assert stats["kmedoids_iterations"] == st["iterations"] and stats["kmedoids_converged"] is True
    assert stats["kmedoids_sizes"] == [150] * 4 and stats["kmedoids_ms"] > 0


def test_cli_kmedoids_refuses_more_clusters_than_contigs(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGCAA\n>c\nACGGGTGCAA\n")
    out = tmp_path / "c.txt"
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", str(fa), "--method", "joblib", "--kmedoids", "4", "-o", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 1 and "--kmedoids K needs 1 <= K" in r.stderr and "3 contigs" in r.stderr and not out.exists()
