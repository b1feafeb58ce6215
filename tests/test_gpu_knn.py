"""K nearest neighbours on the GPU (po_knn*, Context.knn / knn_blocks / knn_merge, `--knn`): every list is the stable-argsort
rule applied to the dense matrix of the same library, bit for bit, whatever the panels, blocks or ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ["Eucl", "JSD", "KT", "BC", "SC"]


def rule(dense, k, desc, rows=None):
    """np.argsort(key, kind="stable")[:k] over every row without its diagonal; key = v (-v for KT), NaN last"""
    n = dense.shape[1]
    rows = np.arange(dense.shape[0]) if rows is None else np.asarray(rows)
    k = min(k, n - 1)
    idx = np.empty((len(rows), k), dtype=np.int32)
    for a, i in enumerate(rows):
        d = dense[a]
        cols = np.concatenate([np.arange(i), np.arange(i + 1, n)])
        key = d[cols]
        key = -key if desc else key
        idx[a] = cols[np.argsort(key, kind="stable")[:k]]
    return idx


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def ctx():
    import phyloligo_amd as pa
    with pa.Context(0) as c:
        yield c


def profiles(ctx, kind, n, seed=7):
    from phyloligo_amd import synthetic
    if kind == "equal":
        seq, off = synthetic.contig_bytes(n, 2000, seed=seed)
    else:
        seq, off = synthetic.ragged_assembly(n, seed=seed, median=3000, lo=300, hi=20000, dirt=True)
    return ctx.count_profiles(seq, off.astype(np.uint64), "1111", "both")


@pytest.fixture(scope="module", params=["equal", "ragged"])
def inputs(request, ctx):
    return profiles(ctx, request.param, 1999)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("metric", METRICS)
def test_knn_equals_rule_on_dense_matrix(ctx, inputs, metric, dtype):
    counts, totals = inputs
    dense = ctx.pairwise(counts, totals, metric, dtype=dtype)
    want_all = rule(dense, 301, metric == "KT")
    for k in (1, 7, 64, 301):
        idx, val = ctx.knn(counts, totals, k, metric, dtype=dtype)
        assert idx.shape == (1999, k) and val.dtype == dense.dtype
        assert np.array_equal(idx, want_all[:, :k]), (metric, dtype, k)
        assert np.array_equal(bits(val), bits(np.take_along_axis(dense, idx.astype(np.int64), axis=1))), (metric, dtype, k)


@pytest.mark.parametrize("metric", METRICS)
def test_knn_against_oracle(ctx, metric):
    from oracle import phyloligo_oracle as po
    from phyloligo_amd import synthetic
    n = 200
    seq, off = synthetic.contig_bytes(n, 2000, seed=31)
    contigs = [seq[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    oc, ot = po.compute_counts(contigs, "1111", "both")
    want = po.pairwise_distances(po.counts_to_frequencies(oc, ot), metric)
    for k in (7, 64):
        idx, val = ctx.knn(oc.astype(np.uint32), ot.astype(np.uint64), k, metric)
        ref = np.take_along_axis(want, idx.astype(np.int64), axis=1)
        np.testing.assert_allclose(val, ref, rtol=1e-6, atol=1e-12)
        for i in range(n):
            cols = np.concatenate([np.arange(i), np.arange(i + 1, n)])
            key = want[i, cols] * (-1 if metric == "KT" else 1)
            s = np.sort(key)
            if abs(s[k] - s[k - 1]) > 1e-9 * max(abs(s[k - 1]), 1e-300):     # a clear boundary after the k-th neighbour
                assert set(idx[i]) == set(cols[np.argsort(key, kind="stable")[:k]]), (metric, k, i)


def check_against_dense(ctx, counts, totals, metric, k, dtype="float64"):
    dense = ctx.pairwise(counts, totals, metric, dtype=dtype)
    idx, val = ctx.knn(counts, totals, k, metric, dtype=dtype)
    assert np.array_equal(idx, rule(dense, k, metric == "KT"))
    assert np.array_equal(bits(val), bits(np.take_along_axis(dense, idx.astype(np.int64), axis=1)))
    return idx, val, dense


@pytest.mark.parametrize("metric", METRICS)
def test_groups_of_identical_records(ctx, metric):
    rng = np.random.default_rng(5)
    base = rng.integers(0, 40, size=(30, 256)).astype(np.uint32)
    counts = np.ascontiguousarray(base[np.repeat(np.arange(30), 5)])          # five copies of every record
    totals = counts.sum(axis=1).astype(np.uint64)
    idx, val, _ = check_against_dense(ctx, counts, totals, metric, 9)
    if metric != "KT":
        for i in range(counts.shape[0]):
            g = i // 5 * 5
            assert list(idx[i, :4]) == [j for j in range(g, g + 5) if j != i]      # the exact ties, by index
            assert np.all(val[i, :4] == 0)


def test_bray_curtis_empty_records_go_last(ctx):
    rng = np.random.default_rng(6)
    counts = rng.integers(0, 30, size=(300, 256)).astype(np.uint32)
    counts[[3, 77, 150, 151, 299]] = 0
    totals = counts.sum(axis=1).astype(np.uint64)
    idx, val, dense = check_against_dense(ctx, counts, totals, "BC", 299)
    assert np.isnan(dense[3]).sum() == 4 and dense[3, 3] == 0               # 0 / 0 between two empty records; the diagonal is 0
    row = val[3]
    assert np.isnan(row[-4:]).all() and not np.isnan(row[:-4]).any()      # NaN after every number
    assert list(idx[3, -4:]) == [77, 150, 151, 299]                        # and by index among themselves
    assert not np.isnan(val[0]).any()


def test_kendall_descending_with_constant_row(ctx):
    rng = np.random.default_rng(8)
    counts = rng.integers(0, 50, size=(260, 256)).astype(np.uint32)
    counts[10] = 7                                                           # a constant record: diagonal 0, not 1
    totals = counts.sum(axis=1).astype(np.uint64)
    idx, val, dense = check_against_dense(ctx, counts, totals, "KT", 40)
    assert dense[10, 10] == 0 and dense[0, 0] == 1
    assert np.all(np.diff(val[0]) <= 0)                                        # a similarity: best first


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_every_candidate_beats_the_threshold(ctx, dtype):
    """record j comes closer to record 0 as j grows: row 0's threshold tightens at every candidate"""
    n = 3000
    counts = np.zeros((n, 256), dtype=np.uint32)
    counts[:, :] = 1000
    counts[1:, 0] = 1000 + (n - np.arange(1, n)).astype(np.uint32)
    totals = counts.sum(axis=1).astype(np.uint64)
    for k in (1, 64, 1024):
        idx, _, _ = check_against_dense(ctx, counts, totals, "Eucl", k, dtype)
        assert idx[0, 0] == n - 1


def test_small_and_degenerate_sizes(ctx):
    from phyloligo_amd import _lib
    rng = np.random.default_rng(9)
    counts = rng.integers(0, 30, size=(10, 256)).astype(np.uint32)
    totals = counts.sum(axis=1).astype(np.uint64)
    for metric in METRICS:
        idx, val, _ = check_against_dense(ctx, counts, totals, metric, 20)          # K >= n - 1
        assert idx.shape == (10, 9)
        idx, val, _ = check_against_dense(ctx, counts[:2], totals[:2], metric, 5)   # n = 2
        assert list(idx[:, 0]) == [1, 0]
        idx, val = ctx.knn(counts[:1], totals[:1], 5, metric)                    # n = 1: no neighbour
        assert idx.shape == (1, 0) and val.shape == (1, 0)
    for k in (0, 1025):
        with pytest.raises(_lib.PhyloligoError) as e:
            ctx.knn(counts, totals, k, "JSD")
        assert e.value.status == _lib.PO_EINVAL
        lib = _lib.load()
        out_i, out_v = np.zeros(10 * 1024, np.int32), np.zeros(10 * 1024)
        st = lib.po_knn(ctx._h, counts.ctypes.data, totals.ctypes.data, 10, 256, 1, k, 0, 0, out_i.ctypes.data, out_v.ctypes.data,
                        0, None)
        assert st == _lib.PO_EINVAL


@pytest.mark.parametrize("metric,dtype", [("JSD", "float64"), ("Eucl", "float32"), ("KT", "float64"), ("BC", "float32"),
                                          ("SC", "float64")])
def test_decomposition_independence(ctx, inputs, metric, dtype):
    import torch
    from phyloligo_amd.dist import RowBlockPlan
    counts, totals = inputs
    d_counts, d_totals = torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(totals.view(np.int64)).cuda()
    k = 64
    ref_i, ref_v = ctx.knn(d_counts, d_totals, k, metric, dtype=dtype)
    for panel in (128, 256):
        i2, v2 = ctx.knn(d_counts, d_totals, k, metric, dtype=dtype, panel_rows=panel)
        assert np.array_equal(i2.cpu().numpy(), ref_i.cpu().numpy()), (metric, panel)
        assert np.array_equal(bits(v2.cpu().numpy()), bits(ref_v.cpu().numpy())), (metric, panel)
    n = counts.shape[0]
    for w in (2, 3, 4):
        plan = RowBlockPlan(n, w)
        parts = [ctx.knn_blocks(d_counts, d_totals, k, plan.work(r), metric, dtype=dtype, panel_rows=256 if r % 2 else 0)
                 for r in range(w)]
        mi, mv = ctx.knn_merge([p[0] for p in parts], [p[1] for p in parts], metric)
        assert np.array_equal(mi.cpu().numpy(), ref_i.cpu().numpy()), (metric, w)
        assert np.array_equal(bits(mv.cpu().numpy()), bits(ref_v.cpu().numpy())), (metric, w)


def test_full_size_rows(ctx):
    import torch
    from phyloligo_amd import synthetic
    n = 50000
    seq, off = synthetic.contig_bytes(n, 2000, seed=1001)
    counts, totals = ctx.count_profiles(torch.from_numpy(seq).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), "1111", "both")
    idx, val = ctx.knn(counts, totals, 32, "JSD")
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    rows = np.linspace(0, n - 1, 64).astype(np.int64)
    for r in rows:
        dense = ctx.pairwise(counts, totals, "JSD", row_begin=int(r), row_end=int(r) + 1).cpu().numpy()
        want = rule(dense, 32, False, rows=[r])[0]
        assert np.array_equal(idx[r], want), r
        assert np.array_equal(bits(val[r]), bits(dense[0, want])), r


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    from phyloligo_amd import synthetic
    n = 300
    seq, off = synthetic.contig_bytes(n, 1500, seed=77)
    path = tmp_path_factory.mktemp("knncli") / "asm.fasta"
    path.write_bytes(synthetic.fasta_bytes(seq, off))
    return str(path), seq, off


def run_cli(args, env_extra=None):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, "-m", "phyloligo_amd"] + args, capture_output=True, text=True, timeout=600, cwd=ROOT,
                          env=env)


def test_cli_knn_graph(ctx, fasta, tmp_path):
    import json
    path, seq, off = fasta
    out, st = tmp_path / "g.npz", tmp_path / "st.json"
    r = run_cli(["-i", path, "-d", "JSD", "--method", "joblib", "--knn", "16", "-o", str(out), "--json-stats", str(st)])
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["Using pattern 1111", "Computing frequencies", "Computing Pairwise distances",
                                     "Writing distance matrix"]
    z = np.load(str(out))
    n = 300
    assert z["format"].item() == "csr" and list(z["shape"]) == [n, n]
    assert np.array_equal(z["indptr"], np.arange(0, n * 17 + 1, 17))
    ind, data = z["indices"].reshape(n, 17), z["data"].reshape(n, 17)
    assert np.array_equal(ind[:, 0], np.arange(n)) and np.all(data[:, 0] == 0) and data.dtype == np.float64
    counts, totals = ctx.count_profiles(seq, off.astype(np.uint64), "1111", "both")
    idx, val = ctx.knn(counts, totals, 16, "JSD")
    assert np.array_equal(ind[:, 1:], idx) and np.array_equal(bits(data[:, 1:]), bits(val))
    s = json.load(open(st))
    assert s["knn"] == 16 and s["knn_select_ms"] is not None and s["contigs"] == n
    # the same job on two ranks (one GPU, gloo collectives) writes the same bytes
    two = tmp_path / "g2.npz"
    r = run_cli(["--gpus", "2", "-i", path, "-d", "JSD", "--method", "joblib", "--knn", "16", "-o", str(two)],
                {"PO_CLI_REHEARSAL": "1", "MASTER_ADDR": "127.0.0.1"})
    assert r.returncode == 0, r.stderr
    assert two.read_bytes() == out.read_bytes()


def test_cli_knn_kendall_and_refusal(fasta, tmp_path):
    path, _, _ = fasta
    out = tmp_path / "kt.npz"
    r = run_cli(["-i", path, "-d", "KT", "--method", "hip", "--knn", "5", "-o", str(out)])
    assert r.returncode == 0, r.stderr
    z = np.load(str(out))
    d = z["data"].reshape(300, 6)
    assert np.all(d[:, 0] == 1) and np.all(np.diff(d[:, 1:], axis=1) <= 0)
    r = run_cli(["-i", path, "--method", "joblib", "--knn", "5", "--large", "memmap", "-o", str(tmp_path / "x")])
    assert r.returncode == 1 and "--large" in r.stderr


def test_cli_graph_feeds_tsne(fasta, tmp_path):
    sparse = pytest.importorskip("scipy.sparse")
    manifold = pytest.importorskip("sklearn.manifold")
    path, _, _ = fasta
    out = tmp_path / "g.npz"
    r = run_cli(["-i", path, "-d", "JSD", "--method", "joblib", "--knn", "16", "-o", str(out)])
    assert r.returncode == 0, r.stderr
    g = sparse.load_npz(str(out))
    emb = manifold.TSNE(metric="precomputed", init="random", perplexity=5, random_state=0).fit_transform(g)
    assert emb.shape == (300, 2) and np.isfinite(emb).all()
