"""--kmedoids on the host side (no GPU): the numpy restatement against what the reference's KMedoids recorded, option parsing,
refusals, the label file."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmedoids_ref  # noqa: E402

from phyloligo_amd import phyloligo as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kmedoids.npz")
CASES = kmedoids_ref.cases()


def test_record_holds_every_case():
    g = np.load(GOLDEN)
    assert len(CASES) == 30 + 12 + 2 and str(g["sklearn_version"])
    for key, _, k, _, _ in CASES:
        assert g[key + "_medoids"].shape == (k,) and g[key + "_labels"].max() < k
    assert os.path.getsize(GOLDEN) < 1 << 20
    # what the issue quotes of the reference's runs
    assert int(g["empty_n_iter"]) == 4 and int(g["empty_warned"]) == 1
    assert list(g["empty_medoids"]) == [103, 9, 336, 329] and list(np.bincount(g["empty_labels"])) == [150, 2, 273, 175]
    assert list(np.bincount(g["heur_n600_k4_f64_labels"])) == [150] * 4
    assert int(g["cap_n_iter"]) == 2
    iters = [int(g[key + "_n_iter"]) for key, *_ in CASES]
    assert min(iters) == 1 and max(iters) == 4


@pytest.mark.parametrize("key", [c[0] for c in CASES])
def test_restatement_reproduces_the_reference(key):
    g = np.load(GOLDEN)
    _, make, k, init, max_iter = next(c for c in CASES if c[0] == key)
    labels, medoids, iterations, _ = kmedoids_ref.kmedoids(make(), k, max_iter, init)
    assert np.array_equal(labels, g[key + "_labels"].astype(np.int32))
    assert np.array_equal(medoids, g[key + "_medoids"])
    assert iterations == int(g[key + "_n_iter"])


def test_exact_ties_exist_in_the_record():
    """n = 257, K = 13 ends with clusters of two whose candidate costs tie exactly (d[i, j] == d[j, i]): the smaller row is the
    candidate, and it replaces the medoid only if the medoid is not the other member (a tie is not "strictly below")"""
    g = np.load(GOLDEN)
    labels, medoids = g["heur_n257_k13_f64_labels"], g["heur_n257_k13_f64_medoids"]
    d = kmedoids_ref.matrix(257)
    pairs = [c for c in range(13) if (labels == c).sum() == 2]
    assert pairs
    for c in pairs:
        i, j = np.flatnonzero(labels == c)
        assert d[i, j] == d[j, i] and i < j and medoids[c] in (i, j)
        costs = kmedoids_ref.masked_costs(d, labels, [i, j])
        assert costs[0] == costs[1] == d[i, j]


def test_empty_cluster_is_empty_in_the_first_pass():
    d = kmedoids_ref.empty_cluster_matrix()
    labels = kmedoids_ref.assign(d, kmedoids_ref.EMPTY_START)
    assert (labels == 1).sum() == 0 and np.array_equal(d[5], d[9])


def test_kmedoids_options_parse():
    p = P.get_cmd(["-i", "x.fa", "--method", "joblib", "-d", "JSD", "--kmedoids", "8", "-o", "c.txt"])
    assert (p.kmedoids, p.kmedoids_iter, p.kmedoids_dtype) == (8, 300, "float64") and P._kmedoids_refused(p) is None
    p = P.get_cmd(["-i", "x.fa", "--method", "hip", "--kmedoids", "3", "--kmedoids-iter", "5", "--kmedoids-dtype", "float32"])
    assert (p.kmedoids, p.kmedoids_iter, p.kmedoids_dtype) == (3, 5, "float32") and P._kmedoids_refused(p) is None
    assert P.get_cmd(["-i", "x.fa", "--method", "joblib"]).kmedoids is None
    with pytest.raises(SystemExit):
        P.get_cmd(["-i", "x.fa", "--method", "joblib", "--kmedoids", "3", "--kmedoids-dtype", "float16"])


def test_help_shows_kmedoids():
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and "--kmedoids K" in r.stdout and "--kmedoids-iter" in r.stdout and "--kmedoids-dtype" in r.stdout


@pytest.mark.parametrize("extra, words", [
    (["--knn", "16"], ["--kmedoids", "--knn"]),
    (["--tsne", "30"], ["--kmedoids", "--tsne"]),
    (["--large", "memmap"], ["--kmedoids", "--large memmap"]),
    (["--large", "h5py"], ["--kmedoids", "--large h5py"]),
    (["-d", "KT"], ["--kmedoids", "KT", "correlation"]),
    (["--gpus", "2"], ["--kmedoids", "one GPU", "out of scope"]),
    (["--kmedoids-iter", "0"], ["--kmedoids-iter", "at least 1"]),
])
def test_kmedoids_refused_by_the_cli(tmp_path, extra, words):
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGCAA\n>c\nACGGGTGCAA\n>d\nTTGGGTGCAA\n")
    out = tmp_path / "c.txt"
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", str(fa), "--method", "joblib", "--kmedoids", "2", "-o", str(out)] + extra,
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 1, r.stdout + r.stderr
    for w in words:
        assert w in r.stderr, r.stderr
    assert not out.exists()


@pytest.mark.parametrize("k", ["0", "-3"])
def test_kmedoids_k_below_one_is_refused_by_the_cli(tmp_path, k):
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGCAA\n")
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", str(fa), "--method", "joblib", "--kmedoids", k],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 1 and "--kmedoids K needs 1 <= K" in r.stderr and "(got %s)" % k in r.stderr


def test_kmedoids_with_the_scoop_method_is_refused():
    p = P.get_cmd(["-i", "x.fa", "--method", "scoop", "--kmedoids", "3"])
    assert "--kmedoids supports --method joblib|hip" in P._kmedoids_refused(p)


def test_label_file_format(tmp_path):
    path = tmp_path / "c.txt"
    P.write_labels(str(path), np.array([3, 0, 12, 0, 1], dtype=np.int32))
    assert path.read_bytes() == b"3\n0\n12\n0\n1\n"
    assert np.array_equal(np.loadtxt(str(path), dtype=np.int64), [3, 0, 12, 0, 1])
    P.write_labels(str(path), np.zeros(0, dtype=np.int32))
    assert path.read_bytes() == b""
