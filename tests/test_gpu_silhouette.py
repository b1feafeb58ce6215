"""Silhouettes on the GPU (po_cluster_sums_dev, po_silhouette*): every case scikit-learn recorded (tests/golden/silhouette.npz),
the per-cluster row sums at awkward shapes and cluster counts, layouts, the rules of the header block, refusals, the CLI
(--silhouette, --kmedoids-sweep)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmedoids_ref  # noqa: E402
import silhouette_ref  # noqa: E402

import phyloligo_amd as pa  # noqa: E402
from phyloligo_amd import _lib, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "silhouette.npz")
C = _lib.PO_SILHOUETTE_CHUNK
# order-of-summation noise of float64 sums of n <= 1100 non-negative terms is about n 2^-53 ~ 1e-13 (tests/test_gpu_kmedoids.py)
COST_RTOL = 1e-12
# a and b each carry at most COST_RTOL; (b - a) / max(a, b) turns relative errors e of a and b into an absolute error of at most
# 4 e; the rest of the margin covers the last division
VALUE_ATOL = 1e-11


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


def _bytes(t):
    return (t.cpu().numpy() if hasattr(t, "cpu") else t).tobytes()


# ---- 1. the recorded cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", silhouette_ref.GOLDEN_N)
@pytest.mark.parametrize("name", ["f64", "f32"])
def test_golden_cases(ctx, torch, n, name):
    g = np.load(GOLDEN)
    d = np.array(kmedoids_ref.matrix(n, np.float64 if name == "f64" else np.float32))       # (a writable copy: torch wraps it)
    t = torch.from_numpy(d).cuda()
    for k in silhouette_ref.GOLDEN_K:
        key = "n%d_%s_k%d" % (n, name, k)
        labels, want = g[key + "_labels"].astype(np.int32), g[key + "_values"]
        values, st = ctx.silhouette(d, labels, k, want_stats=True)
        assert values.dtype == np.float64 and values.shape == (n,)
        err, mean_err = np.abs(values - want).max(), abs(st["mean"] - want.mean())
        print("%s: max |s - sklearn| %.3e, |mean - sklearn| %.3e" % (key, err, mean_err))
        assert err <= VALUE_ATOL and mean_err <= VALUE_ATOL
        assert st["nonempty_clusters"] == k and st["passes"] == 1
        t_values, t_st = ctx.silhouette(t, torch.from_numpy(labels).cuda(), want_stats=True)       # n_clusters = max + 1
        assert t_values.is_cuda and t_values.dtype == torch.float64
        assert _bytes(t_values) == values.tobytes() and t_st["mean"] == st["mean"]
        assert _bytes(ctx.silhouette(t, labels, k)) == values.tobytes()


# ---- 2. per-cluster row sums and the values at awkward shapes ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 257, 1100])
def test_shapes(ctx, torch, n, dtype):
    d = _rand_matrix(n, dtype, seed=n)
    t = torch.from_numpy(d).cuda()
    rng = np.random.RandomState(n + 1)
    big = 2 * C + 1
    for k in sorted(set(q for q in (2, 3, C, C + 1, big, n) if q <= n)):
        last_only = np.zeros(n, dtype=np.int32)
        last_only[n - 1] = k - 1                                          # one cluster holding only the last column
        for labels in (rng.randint(0, k, n).astype(np.int32), last_only):
            t_labels = torch.from_numpy(labels).cuda()
            sums = ctx.cluster_sums(t, t_labels, k)
            assert sums.is_cuda and sums.dtype == torch.float64 and tuple(sums.shape) == (n, k)
            got = sums.cpu().numpy()
            np.testing.assert_allclose(got, silhouette_ref.cluster_sums(d, labels, k), rtol=COST_RTOL, atol=0.0)
            assert got[np.arange(n), labels].tobytes() == ctx.kmedoids_costs(d, labels).tobytes()
            assert _bytes(ctx.cluster_sums(t, t_labels, k)) == got.tobytes()
            if k < big <= n:                                              # the same columns from another variant of the kernel / a full chunk
                wide = ctx.cluster_sums(t, t_labels, big).cpu().numpy()
                assert np.ascontiguousarray(wide[:, :k]).tobytes() == got.tobytes() and not wide[:, k:].any()
            sizes = np.bincount(labels, minlength=k)
            if (sizes > 0).sum() < 2:
                continue
            values, st = ctx.silhouette(d, labels, k, want_stats=True)
            want, want_mean, live = silhouette_ref.silhouette(d, labels, k)
            assert st["passes"] == (k + C - 1) // C and st["nonempty_clusters"] == live
            assert np.abs(values - want).max() <= VALUE_ATOL and abs(st["mean"] - want_mean) <= VALUE_ATOL
            assert not values[sizes[labels] == 1].any()                   # a cluster of one: exactly 0
            again, st2 = ctx.silhouette(t, t_labels, k, want_stats=True)
            assert _bytes(again) == values.tobytes() and st2["mean"] == st["mean"]
    if n == 2:
        assert ctx.silhouette(d, np.array([0, 1], dtype=np.int32), 2).tolist() == [0.0, 0.0]


def test_a_column_does_not_depend_on_the_cluster_count(ctx, torch):
    """column c from n_clusters = c + 1 (the last, short chunk: the smallest kernel variant that holds it) and from
    n_clusters = 2 C + 1 (a full chunk, or the single cluster of the third pass): the same bytes"""
    n, big = 257, 2 * C + 1
    for dtype in (np.float64, np.float32):
        t = torch.from_numpy(_rand_matrix(n, dtype, seed=5)).cuda()
        labels = torch.from_numpy(np.random.RandomState(6).randint(0, big, n).astype(np.int32)).cuda()
        for c in (0, 1, 3, 4, 7, 8, C - 1, C, C + 3, C + 4, 2 * C - 1):
            some = torch.clamp(labels, max=c)                             # labels 0 .. c
            part = ctx.cluster_sums(t, some, c + 1).cpu().numpy()
            full = ctx.cluster_sums(t, some, big).cpu().numpy()           # the same labels, more (empty) clusters
            assert np.ascontiguousarray(full[:, :c + 1]).tobytes() == part.tobytes() and not full[:, c + 1:].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [5, 257, 1027])
def test_three_kernels_share_one_summation_order(ctx, torch, n, dtype):
    """one cluster that holds every column: the silhouette sums kernel, the masked k-medoids row sums and the unmasked row sums
    of the heuristic start add the same values, and csrc/po_rows.h gives all three their order - the same bytes.  The unmasked
    sums are seen through the start they decide: with n_clusters = n every row is a medoid of a cluster of one (zero diagonal,
    positive elsewhere), no update moves it, and the medoids are the rows in ascending order of their sums, ties to the
    smaller row.  ld = n (element loads) and rows padded to 16 bytes (one load per group)."""
    d = _rand_matrix(n, dtype, seed=n + 7)
    zeros = torch.zeros(n, dtype=torch.int32, device="cuda")
    padded = torch.zeros((n, (n + 3) // 4 * 4), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    padded[:, :n] = torch.from_numpy(d).cuda()
    want = None
    for t in (torch.from_numpy(d).cuda(), padded[:, :n]):
        column = ctx.cluster_sums(t, zeros, 1).cpu().numpy()[:, 0]
        np.testing.assert_allclose(column, d.astype(np.float64).sum(axis=1), rtol=COST_RTOL, atol=0.0)
        assert _bytes(ctx.kmedoids_costs(t, zeros)) == column.tobytes()
        labels, medoids = ctx.kmedoids(t, n_clusters=n, init="heuristic")
        assert medoids.cpu().numpy().tolist() == np.argsort(column, kind="stable").tolist()
        assert labels.cpu().numpy()[medoids.cpu().numpy()].tolist() == list(range(n))
        want = column.tobytes() if want is None else want
        assert column.tobytes() == want


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_results_do_not_depend_on_layout(ctx, torch, dtype):
    """n = 257 with ld = n; a view with ld = n + 3; a view one element into an aligned buffer; ld = 264 (every row on a 16-byte
    boundary): identical bytes of the sums and of the values"""
    n, k = 257, C + 1
    d = _rand_matrix(n, dtype, seed=3)
    labels = np.random.RandomState(4).randint(0, k, n).astype(np.int32)
    t_labels = torch.from_numpy(labels).cuda()
    tt = torch.float32 if dtype == np.float32 else torch.float64
    base_sums = ctx.cluster_sums(torch.from_numpy(d).cuda(), t_labels, k).cpu().numpy()      # ld = n = 257: unaligned rows
    base_values, st = ctx.silhouette(torch.from_numpy(d).cuda(), t_labels, k, want_stats=True)
    base_values = base_values.cpu().numpy()
    assert np.abs(base_values - silhouette_ref.silhouette(d, labels, k)[0]).max() <= VALUE_ATOL
    views = []
    wide = torch.zeros((n, n + 3), dtype=tt, device="cuda")
    wide[:, :n] = torch.from_numpy(d).cuda()
    views.append(wide[:, :n])
    off = torch.zeros((n, 265), dtype=tt, device="cuda")
    off[:, 1:n + 1] = torch.from_numpy(d).cuda()                           # one element into the buffer, odd ld
    views.append(off[:, 1:n + 1])
    aligned = torch.zeros((n, 264), dtype=tt, device="cuda")
    aligned[:, :n] = torch.from_numpy(d).cuda()
    views.append(aligned[:, :n])
    for v in views:
        assert _bytes(ctx.cluster_sums(v, t_labels, k)) == base_sums.tobytes()
        values, st2 = ctx.silhouette(v, t_labels, k, want_stats=True)
        assert _bytes(values) == base_values.tobytes() and st2["mean"] == st["mean"]
    host_wide = np.zeros((n, n + 3), dtype=dtype)                          # the host form copies a strided view
    host_wide[:, :n] = d
    assert ctx.silhouette(host_wide[:, :n], labels, k).tobytes() == base_values.tobytes()


# ---- 3. the rules ------------------------------------------------------------------------------------------------------------------
def test_duplicates_give_zero_not_nan(ctx):
    n = 96
    d = _rand_matrix(n, np.float64, seed=8)
    d[:40, :40] = 0.0                                                     # forty copies of one record, split over two clusters
    labels = (np.arange(n) % 2).astype(np.int32)
    labels[40:] += 2
    d[:40, 40:] = d[0, 40:]
    d[40:, :40] = d[40:, :1]
    values = ctx.silhouette(d, labels, 4)
    want = silhouette_ref.silhouette(d, labels, 4)[0]
    assert np.isfinite(values).all() and np.abs(values - want).max() <= VALUE_ATOL
    zero = np.zeros((8, 8))
    assert ctx.silhouette(zero, (np.arange(8) % 2).astype(np.int32)).tolist() == [0.0] * 8      # m == 0 everywhere


def test_empty_cluster_is_skipped(ctx):
    d = kmedoids_ref.empty_cluster_matrix()
    labels = kmedoids_ref.assign(d, kmedoids_ref.EMPTY_START)
    assert np.bincount(labels, minlength=4).tolist() == [13, 0, 164, 423]
    values, st = ctx.silhouette(d, labels, 4, want_stats=True)
    want, want_mean, _ = silhouette_ref.silhouette(d, labels, 4)
    assert st["nonempty_clusters"] == 3 and st["passes"] == 1
    assert np.abs(values - want).max() <= VALUE_ATOL and abs(st["mean"] - want_mean) <= VALUE_ATOL


def test_nan_marks_exactly_the_rows_the_definition_names(ctx):
    n, k = 130, 3
    d = _rand_matrix(n, np.float64, seed=9)
    labels = (np.arange(n) % k).astype(np.int32)
    clean, st = ctx.silhouette(d, labels, k, want_stats=True)
    assert np.isfinite(clean).all() and np.isfinite(st["mean"])
    d[4, 5] = np.nan                                                      # S[4][labels[5]] is NaN: row 4, nothing else (d[5, 4] is a number)
    values, st = ctx.silhouette(d, labels, k, want_stats=True)
    want = silhouette_ref.silhouette(d, labels, k)[0]
    assert np.isnan(values[4]) and np.isnan(st["mean"]) and np.array_equal(np.isnan(values), np.isnan(want))
    assert np.delete(values, 4).tobytes() == np.delete(clean, 4).tobytes()
    single = labels.copy()
    single[4] = 3                                                         # row 4 alone in its cluster: a NaN sum still gives NaN, not 0
    assert np.isnan(ctx.silhouette(d, single, 4)[4]) and np.isnan(silhouette_ref.silhouette(d, single, 4)[0][4])
    d[4, 5] = 0.25
    d[4, 4] = np.nan                                                      # the diagonal is part of the row as stored
    assert np.flatnonzero(np.isnan(ctx.silhouette(d, labels, k))).tolist() == [4]


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
    good = (np.arange(n) % 3).astype(np.int32)
    want = ctx.silhouette(d, good, 3)
    _refused(lambda: ctx.silhouette(d, np.zeros(n, np.int32), 1), "1 non-empty cluster", "at least 2")
    _refused(lambda: ctx.silhouette(d, np.full(n, 2, np.int32), 4), "1 non-empty cluster")
    assert ctx.silhouette(d, good, 3).tobytes() == want.tobytes()
    bad = good.copy()
    bad[37] = 3
    _refused(lambda: ctx.silhouette(d, bad, 3), "labels[37]")
    _refused(lambda: ctx.cluster_sums(t, torch.from_numpy(bad).cuda(), 3), "labels[37]")
    bad[12] = -1
    _refused(lambda: ctx.silhouette(t, torch.from_numpy(bad).cuda(), 3), "labels[12]")
    _refused(lambda: ctx.silhouette(d, good, 0), "n_clusters")
    _refused(lambda: ctx.silhouette(d, good, n + 1), "n_clusters")
    _refused(lambda: ctx.silhouette(d, good[:-1], 3), "labels")
    _refused(lambda: ctx.silhouette(torch.as_strided(t, (n, n), (n - 1, 1)), good, 3), "ld = 99", "n = 100")
    lib = _lib.load()                                                    # the library's own argument checks, past the Python layer
    values = torch.zeros(n, dtype=torch.float64, device="cuda")
    t_good = torch.from_numpy(good).cuda()
    for k, ld, word in ((0, n, "n_clusters = 0"), (n + 1, n, "n_clusters = 101"), (3, n - 1, "ld = 99")):
        rc = lib.po_silhouette_dev(ctx._h, t.data_ptr(), _lib.PO_F64, n, ld, t_good.data_ptr(), k, values.data_ptr(), None)
        assert rc == _lib.PO_EINVAL and word in lib.po_last_error().decode(), lib.po_last_error().decode()
    assert ctx.silhouette(d, good, 3).tobytes() == want.tobytes()
    assert _bytes(ctx.silhouette(t, t_good)) == want.tobytes()


# ---- 4. CLI ------------------------------------------------------------------------------------------------------------------------
N_CLI = 300
_RUNS = {}


def _fasta(tmp_path_factory):
    if "fa" not in _RUNS:
        seq, offsets = synthetic.ragged_assembly(N_CLI, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
        fa = tmp_path_factory.mktemp("sil") / "asm.fa"
        fa.write_bytes(synthetic.fasta_bytes(seq, offsets))
        _RUNS["fa"] = (fa, seq, offsets)
    return _RUNS["fa"]


def _cli(tmp_path_factory, mode, clip, *extra):
    """one CLI run, cached: (labels bytes, stats, directory)"""
    key = (tuple(mode), clip) + extra
    if key not in _RUNS:
        fa = _fasta(tmp_path_factory)[0]
        work = tmp_path_factory.mktemp("run")
        args = [sys.executable, "-m", "phyloligo_amd", "-i", str(fa), "-d", "Eucl", "--method", "joblib", "-o", str(work / "labels.txt"),
                "--json-stats", str(work / "stats.json")] + list(mode) + (["--clip-percentile", "0.97"] if clip else [])
        for name, flag in (("s.txt", "--silhouette"), ("t.tsv", "--sweep-out")):
            if flag in extra:
                args += [flag, str(work / name)]
        r = subprocess.run(args, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stdout + r.stderr
        _RUNS[key] = ((work / "labels.txt").read_bytes(), json.load(open(work / "stats.json")), work)
    return _RUNS[key]


def _matrix(ctx, tmp_path_factory, clip):
    """the matrix the CLI clusters: Euclidean distances of the records --clip-percentile 0.97 keeps (or of all)"""
    if ("matrix", clip) not in _RUNS:
        _, seq, offsets = _fasta(tmp_path_factory)
        counts, totals = ctx.count_profiles(seq, offsets, "1111", "both")
        d = ctx.pairwise(counts, totals, "Eucl")
        if clip:
            keep = pa.api.clip_keep(ctx.row_medians(d), 0.97)
            d = ctx.pairwise(counts[keep], totals[keep], "Eucl")
        _RUNS["matrix", clip] = d
    return _RUNS["matrix", clip]


@pytest.mark.parametrize("clip", [False, True])
def test_cli_silhouette_file(ctx, tmp_path_factory, clip):
    labels_bytes, stats, work = _cli(tmp_path_factory, ["--kmedoids", "4"], clip, "--silhouette")
    d = _matrix(ctx, tmp_path_factory, clip)
    n = d.shape[0]
    assert (n == N_CLI) != clip
    labels = np.array(labels_bytes.split(), dtype=np.int32)
    assert labels.shape == (n,) and np.array_equal(labels, ctx.kmedoids(d, 4)[0])
    values, st = ctx.silhouette(d, labels, 4, want_stats=True)
    lines = (work / "s.txt").read_text().split("\n")
    assert lines[-1] == "" and len(lines) == n + 1 and lines[:-1] == [repr(float(v)) for v in values]
    assert stats["silhouette_mean"] == st["mean"] and stats["silhouette_passes"] == 1 and stats["silhouette_ms"] > 0
    means = stats["silhouette_cluster_means"]
    assert len(means) == 4 and means == [float(values[labels == c].mean()) for c in range(4)]
    plain_bytes, plain_stats, _ = _cli(tmp_path_factory, ["--kmedoids", "4"], clip)
    assert plain_bytes == labels_bytes                                    # --silhouette changes nothing about the labels
    assert plain_stats["silhouette_mean"] == st["mean"]                    # the mean is reported without --silhouette too


LO, HI = 2, 6


def _sweep(ctx, tmp_path_factory, clip):
    """the cached sweep run and what the restatement says about the same matrix: (labels bytes, stats, directory, table lines,
    reference means, winner)"""
    if ("sweep", clip) not in _RUNS:
        d = _matrix(ctx, tmp_path_factory, clip)
        ref_means = [silhouette_ref.silhouette(d, kmedoids_ref.kmedoids(d, k)[0], k)[1] for k in range(LO, HI + 1)]
        order = np.sort(ref_means)
        assert order[-1] - order[-2] > 1e-6                               # (0.030 without the clip, 0.128 with it)
        run = _cli(tmp_path_factory, ["--kmedoids-sweep", "%d:%d" % (LO, HI)], clip, "--sweep-out", "--silhouette")
        table = (run[2] / "t.tsv").read_text().split("\n")
        _RUNS["sweep", clip] = run + (table, ref_means, LO + silhouette_ref.winner(ref_means))
    return _RUNS["sweep", clip]


@pytest.mark.parametrize("clip", [False, True])
def test_cli_sweep_table_and_stats(ctx, tmp_path_factory, clip):
    _, stats, _, table, _, k_best = _sweep(ctx, tmp_path_factory, clip)
    assert table[0] == "#K\titerations\tconverged\tempty_clusters\tinertia\tsilhouette_mean\tsizes" and table[-1] == ""
    assert len(table) == 1 + (HI - LO + 1) + 1 and [int(q.split("\t")[0]) for q in table[1:-1]] == list(range(LO, HI + 1))
    assert stats["kmedoids_sweep_best"] == k_best and stats["kmedoids"] == k_best and len(stats["kmedoids_sweep"]) == HI - LO + 1
    assert stats["silhouette_passes"] == 1 and len(stats["silhouette_cluster_means"]) == k_best


@pytest.mark.parametrize("k", range(LO, HI + 1))
@pytest.mark.parametrize("clip", [False, True])
def test_cli_sweep_row_equals_the_single_run(ctx, tmp_path_factory, clip, k):
    """row K of the table is what `--kmedoids K --json-stats` reports; -o and --silhouette hold the winner's single run"""
    sweep_bytes, stats, work, table, ref_means, k_best = _sweep(ctx, tmp_path_factory, clip)
    t = k - LO
    single_bytes, single, _ = _cli(tmp_path_factory, ["--kmedoids", str(k)], clip, *(("--silhouette",) if k == 4 else ()))
    sizes = single["kmedoids_sizes"]
    want = "%d\t%d\t%d\t%d\t%r\t%r\t%s" % (k, single["kmedoids_iterations"], single["kmedoids_converged"], sizes.count(0),
                                         single["kmedoids_inertia"], single["silhouette_mean"], ",".join(str(x) for x in sizes))
    assert table[1 + t] == want
    row = stats["kmedoids_sweep"][t]
    assert (row["K"], row["iterations"], row["converged"], row["inertia"], row["silhouette_mean"], row["sizes"]) == \
           (k, single["kmedoids_iterations"], single["kmedoids_converged"], single["kmedoids_inertia"], single["silhouette_mean"], sizes)
    assert abs(single["silhouette_mean"] - ref_means[t]) <= VALUE_ATOL
    if k == k_best:
        assert sweep_bytes == single_bytes                                # -o holds the labels of the --kmedoids Kbest run
        assert stats["kmedoids_medoids"] == single["kmedoids_medoids"] and stats["silhouette_mean"] == single["silhouette_mean"]
        labels = np.array(single_bytes.split(), dtype=np.int32)
        d = _matrix(ctx, tmp_path_factory, clip)
        assert (work / "s.txt").read_text() == "".join("%r\n" % float(v) for v in ctx.silhouette(d, labels, k))
