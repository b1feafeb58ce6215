"""--tsne on the host side (no GPU): the numpy restatement against what scikit-learn recorded, option parsing, refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_ref  # noqa: E402

from phyloligo_amd import _lib, api  # noqa: E402
from phyloligo_amd import phyloligo as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tsne_sklearn.npz")
F32_EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def recorded():
    g = np.load(GOLDEN)
    n, perplexity = int(g["n"]), float(g["perplexity"])
    counts, totals, _ = tsne_ref.make_input(n)
    idx, val = tsne_ref.knn_lists(tsne_ref.eucl_matrix(counts, totals), tsne_ref.n_neighbours(n, perplexity))
    return g, n, perplexity, idx, val


def test_ref_conditional_probabilities_are_sklearns(recorded):
    g, n, perplexity, idx, val = recorded
    cond, beta = tsne_ref.binary_search_perplexity(val, perplexity)
    assert g["cond"].shape == cond.shape == (1000, 91) and g["cond"].dtype == np.float32
    # the record is float32: half an ulp of rounding on top of the same float64 search
    np.testing.assert_allclose(cond, g["cond"].astype(np.float64), rtol=F32_EPS, atol=float(np.finfo(np.float32).tiny))
    assert np.abs(cond.sum(axis=1) - 1).max() < 1e-12


def test_ref_joint_probabilities_are_sklearns(recorded):
    g, n, perplexity, idx, val = recorded
    cond, _ = tsne_ref.binary_search_perplexity(val, perplexity)
    rowptr, col, values = tsne_ref.csr_of(tsne_ref.joint_dense(idx, cond))
    assert np.array_equal(rowptr, g["indptr"].astype(np.int64))
    assert np.array_equal(col, g["indices"].astype(np.int32))
    np.testing.assert_allclose(values, g["data"].astype(np.float64), rtol=F32_EPS)
    assert abs(values.sum() - 1) < 1e-12


def test_record_holds_sklearns_runs():
    g = np.load(GOLDEN)
    assert list(g["seeds"]) == [0, 1, 2] and g["kl"].shape == (3,) and str(g["sklearn_version"])
    assert (g["purity"] == 1.0).all() and (g["trust"] > 0.8).all() and (g["kl"] > 0).all()
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_ref_gradient_is_the_derivative_of_its_kl():
    """the restatement's own consistency: grad = d KL / d y by central differences (exaggeration 1)"""
    rng = np.random.RandomState(1)
    n = 40
    c = rng.rand(n, n) * (rng.rand(n, n) < 0.3)
    np.fill_diagonal(c, 0)
    p = (c + c.T) / (c + c.T).sum()
    y = rng.standard_normal((n, 2))
    grad = tsne_ref.gradient(p, y)[0]
    for i, a in ((0, 0), (7, 1), (39, 0)):
        h = 1e-6
        yp, ym = y.copy(), y.copy()
        yp[i, a] += h
        ym[i, a] -= h
        num = (tsne_ref.kl_divergence(p, yp) - tsne_ref.kl_divergence(p, ym)) / (2 * h)
        assert abs(num - grad[i, a]) < 1e-7


def test_tsne_options_parse():
    p = P.get_cmd(["-i", "x.fa", "--method", "joblib", "-d", "JSD", "--tsne", "30", "-o", "y.txt"])
    assert p.tsne == 30.0 and p.tsne_seed == 0 and p.tsne_iter == 1000 and P._tsne_refused(p) is None
    p = P.get_cmd(["-i", "x.fa", "--method", "joblib", "--tsne", "12.5", "--tsne-seed", "3", "--tsne-iter", "500"])
    assert (p.tsne, p.tsne_seed, p.tsne_iter) == (12.5, 3, 500)
    assert P.get_cmd(["-i", "x.fa", "--method", "joblib"]).tsne is None


def test_help_shows_tsne():
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and "--tsne PERPLEXITY" in r.stdout and "--tsne-seed" in r.stdout and "--tsne-iter" in r.stdout


@pytest.mark.parametrize("extra, words", [
    (["--knn", "16"], ["--tsne", "--knn"]),
    (["--large", "memmap"], ["--tsne", "--large"]),
    (["--large", "h5py"], ["--tsne", "--large"]),
    (["-d", "KT"], ["--tsne", "KT"]),
    (["--gpus", "2"], ["--tsne", "one GPU", "out of scope"]),
    (["--tsne-iter", "0"], ["--tsne-iter", "at least 1"]),
])
def test_tsne_refused_by_the_cli(tmp_path, extra, words):
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGCAA\n>c\nACGGGTGCAA\n>d\nTTGGGTGCAA\n")
    out = tmp_path / "y.txt"
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", str(fa), "--method", "joblib", "--tsne", "30", "-o", str(out)] + extra,
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 1, r.stdout + r.stderr
    for w in words:
        assert w in r.stderr, r.stderr
    assert not out.exists()


def test_tsne_with_the_scoop_method_is_refused():
    p = P.get_cmd(["-i", "x.fa", "--method", "scoop", "--tsne", "30"])
    assert "--tsne supports --method joblib|hip" in P._tsne_refused(p)


@pytest.mark.parametrize("perplexity", ["0.5", "342", "1000", "nan"])
def test_tsne_perplexity_out_of_range_is_refused_by_the_cli(tmp_path, perplexity):
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGCAA\n")
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", str(fa), "--method", "joblib", "--tsne", perplexity],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 1 and "--tsne PERPLEXITY" in r.stderr and "341" in r.stderr


@pytest.mark.parametrize("perplexity", [0.99, 341.4, float("nan"), "x", None])
def test_perplexity_validation(perplexity):
    with pytest.raises(_lib.PhyloligoError) as e:
        api.check_tsne_perplexity(perplexity)
    assert e.value.status == _lib.PO_EINVAL


def test_perplexity_accepted_range_and_neighbours():
    assert api.check_tsne_perplexity(1) == 1.0 and api.check_tsne_perplexity(341) == 341.0
    assert api.tsne_neighbours(50000, 30) == 91 and api.tsne_neighbours(50000, 100) == 301 and api.tsne_neighbours(20, 30) == 19
    assert api.tsne_neighbours(50000, 341) == 1024


def test_start_is_sklearns_random_init():
    y0 = api.tsne_start(5, 0)
    want = (1e-4 * np.random.RandomState(0).standard_normal(size=(5, 2))).astype(np.float32)
    assert y0.dtype == np.float32 and np.array_equal(y0, want)
