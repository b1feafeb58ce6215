"""--silhouette / --kmedoids-sweep on the host side (no GPU): the numpy restatement against what scikit-learn recorded
(tests/golden/silhouette.npz), the lead the sweep tests rest on, option parsing, refusals, the two file formats."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmedoids_ref  # noqa: E402
import silhouette_ref  # noqa: E402

from phyloligo_amd import phyloligo as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "silhouette.npz")
CASES = silhouette_ref.cases()
FOUR = b">a\nACGTACGTAC\n>b\nACGTTTGCAA\n>c\nACGGGTGCAA\n>d\nTTGGGTGCAA\n"


def test_record_holds_every_case():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1000000
    assert len(CASES) == 3 * 2 * 9 and str(g["sklearn_version"])
    for key, n, _, _, k in CASES:
        labels, values = g[key + "_labels"], g[key + "_values"]
        assert labels.shape == (n,) and values.shape == (n,) and values.dtype == np.float64
        assert labels.min() == 0 and labels.max() == k - 1 and np.isfinite(values).all()
    # the labels are those of the numpy k-medoids restatement (one small and one larger case regenerated here)
    for n, name, k in ((257, "f64", 7), (600, "f32", 4)):
        assert np.array_equal(g["n%d_%s_k%d_labels" % (n, name, k)], silhouette_ref.golden_labels(n, name, k))


@pytest.mark.parametrize("n", silhouette_ref.GOLDEN_N)
def test_restatement_reproduces_scikit_learn_and_k2_leads(n):
    """numpy against numpy, absolute 1e-12; and over K = 2 .. 10 the winner is K = 2 with a lead over the runner-up far above the
    1e-6 the sweep tests ask for (0.092 .. 0.112)"""
    g = np.load(GOLDEN)
    for dt, name in silhouette_ref.GOLDEN_DTYPES:
        d = kmedoids_ref.matrix(n, dt)
        means = []
        for k in silhouette_ref.GOLDEN_K:
            key = "n%d_%s_k%d" % (n, name, k)
            values, mean, live = silhouette_ref.silhouette(d, g[key + "_labels"].astype(np.int32), k)
            assert np.abs(values - g[key + "_values"]).max() <= 1e-12 and abs(mean - g[key + "_values"].mean()) <= 1e-12
            assert live == k
            means.append(mean)
        order = np.sort(means)
        assert silhouette_ref.winner(means) == 0 and order[-1] - order[-2] > 1e-6
        assert 0.09 < order[-1] - order[-2] < 0.115


def test_restatement_rules_scikit_learn_does_not_have():
    d = np.array(kmedoids_ref.empty_cluster_matrix())
    labels = kmedoids_ref.assign(d, kmedoids_ref.EMPTY_START)
    assert np.bincount(labels, minlength=4).tolist() == [13, 0, 164, 423]
    values, mean, live = silhouette_ref.silhouette(d, labels, 4)
    assert live == 3 and np.isfinite(values).all()
    # the same clustering with the empty cluster renumbered away is an input scikit-learn accepts: the same values
    dense = np.searchsorted([0, 2, 3], labels)
    assert np.array_equal(silhouette_ref.silhouette(d, dense, 3)[0], values)
    # a NaN at (i, j) makes S[i][labels[j]] NaN: row i alone becomes NaN, and the mean
    i, j = 20, 300
    d[i, j] = np.nan
    v2, m2, _ = silhouette_ref.silhouette(d, labels, 4)
    assert np.isnan(v2[i]) and np.isnan(m2) and np.array_equal(np.delete(v2, i), np.delete(values, i))
    with pytest.raises(ValueError):
        silhouette_ref.silhouette(d, np.full(600, 2), 4)
    assert silhouette_ref.winner([float("nan"), 0.25, 0.25, 0.1]) == 1 and silhouette_ref.winner([float("nan")] * 2) is None


def test_options_parse():
    p = P.get_cmd(["-i", "x.fa", "--method", "joblib", "--kmedoids", "4", "--silhouette", "s.txt", "-o", "c.txt"])
    assert (p.kmedoids, p.silhouette, p.kmedoids_sweep, p.sweep_out) == (4, "s.txt", None, None) and P._kmedoids_refused(p) is None
    p = P.get_cmd(["-i", "x.fa", "--method", "hip", "--kmedoids-sweep", "2:10", "--sweep-out", "t.tsv", "--silhouette", "s.txt",
                   "--kmedoids-iter", "7", "--kmedoids-dtype", "float32", "--clip-percentile", "0.97"])
    assert (p.kmedoids, p.kmedoids_sweep, p.sweep_out, p.kmedoids_iter, p.kmedoids_dtype) == (None, "2:10", "t.tsv", 7, "float32")
    assert P._kmedoids_refused(p) is None and P._sweep_range(p) == (2, 10)
    assert P.parse_sweep("3:3") == (3, 3) and P.parse_sweep(" 2 : 6 ") == (2, 6)
    for bad in ("1:4", "5:3", "2:x", "4", "2:3:4", "", "0:0", "-2:5"):
        with pytest.raises(ValueError) as e:
            P.parse_sweep(bad)
        assert "--kmedoids-sweep" in str(e.value)
    p = P.get_cmd(["-i", "x.fa", "--method", "joblib"])                               # a run without the new options sees none of them
    assert (p.silhouette, p.kmedoids_sweep, p.sweep_out) == (None, None, None) and P._kmedoids_refused(p) is None


def test_help_shows_the_options():
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0
    for w in ("--silhouette FILE", "--kmedoids-sweep LO:HI", "--sweep-out FILE", "--kmedoids K"):
        assert w in r.stdout, r.stdout


@pytest.mark.parametrize("args, words", [
    (["--silhouette", "S"], ["--silhouette", "--kmedoids K"]),
    (["--sweep-out", "T", "--kmedoids", "2"], ["--sweep-out", "--kmedoids-sweep"]),
    (["--kmedoids-sweep", "2:3", "--kmedoids", "2"], ["--kmedoids-sweep", "--kmedoids 2"]),
    (["--kmedoids-sweep", "1:4"], ["--kmedoids-sweep", "2 <= LO <= HI", "1:4"]),
    (["--kmedoids-sweep", "5:3"], ["--kmedoids-sweep", "2 <= LO <= HI", "5:3"]),
    (["--kmedoids-sweep", "2:x"], ["--kmedoids-sweep", "two integers", "2:x"]),
    (["--kmedoids-sweep", "2:3", "--knn", "2"], ["--kmedoids-sweep", "--knn"]),
    (["--kmedoids-sweep", "2:3", "--tsne", "30"], ["--kmedoids-sweep", "--tsne"]),
    (["--kmedoids-sweep", "2:3", "--large", "memmap"], ["--kmedoids-sweep", "--large memmap"]),
    (["--kmedoids-sweep", "2:3", "-d", "KT"], ["--kmedoids-sweep", "KT", "correlation"]),
    (["--kmedoids-sweep", "2:3", "--gpus", "2"], ["--kmedoids-sweep", "one GPU", "out of scope"]),
    (["--kmedoids-sweep=2:3", "--gpus=2"], ["--kmedoids-sweep", "one GPU", "out of scope"]),
    (["--kmedoids-sweep", "2:3", "--method", "scoop"], ["--kmedoids-sweep supports --method joblib|hip"]),
    (["--kmedoids-sweep", "2:3", "--kmedoids-iter", "0"], ["--kmedoids-iter", "at least 1"]),
])
def test_refused_by_the_cli(tmp_path, args, words):
    """every refusal ends with status 1, names the option and leaves no output file behind"""
    fa = tmp_path / "a.fa"
    fa.write_bytes(FOUR)
    out, sil, tab = tmp_path / "c.txt", tmp_path / "s.txt", tmp_path / "t.tsv"
    args = [str(sil) if a == "S" else str(tab) if a == "T" else a for a in args]
    base = [] if "--method" in args else ["--method", "joblib"]
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", str(fa), "-o", str(out)] + base + args,
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 1, r.stdout + r.stderr
    for w in words:
        assert w in r.stderr, r.stderr
    assert not out.exists() and not sil.exists() and not tab.exists()


def test_silhouette_file_format(tmp_path):
    path = tmp_path / "s.txt"
    values = np.array([0.5, -0.125, 0.0, 1.0 / 3.0, float("nan"), 1e-300])
    P.write_silhouette(str(path), values)
    lines = path.read_text().split("\n")
    assert lines == ["0.5", "-0.125", "0.0", "0.3333333333333333", "nan", "1e-300", ""]
    back = np.array([float(q) for q in lines[:-1]])                   # repr round-trips every float64
    assert back.tobytes() == values.tobytes()


def test_sweep_table_format_and_winner(tmp_path):
    rows = [{"K": 2, "iterations": 3, "converged": True, "empty_clusters": 0, "inertia": 12.5, "silhouette_mean": 0.25, "sizes": [3, 4]},
            {"K": 3, "iterations": 300, "converged": False, "empty_clusters": 1, "inertia": 0.1, "silhouette_mean": float("nan"), "sizes": [6, 0, 1]},
            {"K": 4, "iterations": 2, "converged": True, "empty_clusters": 0, "inertia": 1.0 / 3.0, "silhouette_mean": 0.25, "sizes": [1, 2, 2, 2]}]
    path = tmp_path / "t.tsv"
    P.write_sweep_table(str(path), rows)
    assert path.read_text() == ("#K\titerations\tconverged\tempty_clusters\tinertia\tsilhouette_mean\tsizes\n"
                                "2\t3\t1\t0\t12.5\t0.25\t3,4\n"
                                "3\t300\t0\t1\t0.1\tnan\t6,0,1\n"
                                "4\t2\t1\t0\t0.3333333333333333\t0.25\t1,2,2,2\n")
    assert P.sweep_best(rows)["K"] == 2                               # a tie goes to the smaller K, a NaN never wins
    assert P.sweep_best(rows[::-1])["K"] == 2
    assert P.sweep_best([dict(rows[1]), dict(rows[1], K=5)]) is None
    assert P.sweep_best([rows[1], dict(rows[0], silhouette_mean=-0.5, K=9)])["K"] == 9
    assert P.silhouette_cluster_means([0.5, 0.25, -1.0, 0.75], [0, 2, 2, 0], 3) == [0.625, None, -0.375]
