"""--knn on the host side (no GPU): option parsing, the refusal next to --large, the CSR file layout, k validation."""
import os
import subprocess
import sys

import numpy as np
import pytest

from phyloligo_amd import _lib, api
from phyloligo_amd import phyloligo as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_option_parses():
    p = P.get_cmd(["-i", "x.fa", "--method", "joblib", "-d", "JSD", "--knn", "32", "-o", "g.npz"])
    assert p.knn == 32 and p.dist == "JSD" and p.out_file == "g.npz"
    assert P.get_cmd(["-i", "x.fa", "--method", "joblib"]).knn is None


@pytest.mark.parametrize("large", ["memmap", "h5py"])
def test_knn_with_large_container_is_refused(tmp_path, large):
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGCAA\n")
    out = tmp_path / "g.npz"
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", str(fa), "--method", "joblib", "--knn", "4",
                        "--large", large, "-o", str(out)], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 1
    assert "--knn" in r.stderr and "--large" in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("k", [0, 1025])
def test_knn_k_out_of_range_is_refused_by_the_cli(k):
    p = P.get_cmd(["-i", "x.fa", "--method", "joblib", "--knn", str(k)])
    assert "--knn" in P._knn_refused(p)


def test_write_knn_npz_layout(tmp_path):
    idx = np.array([[2, 1], [0, 2], [1, 0]], dtype=np.int32)
    val = np.array([[0.5, 0.75], [0.75, 1.0], [0.5, 1.0]])
    path = tmp_path / "graph"                                   # no suffix: the file is written to exactly this name
    api.write_knn_npz(str(path), idx, val, 0.0)
    assert path.exists() and not os.path.exists(str(path) + ".npz")
    z = np.load(str(path))
    assert set(z.files) == {"data", "indices", "indptr", "format", "shape"}
    assert z["format"].item() == "csr" and list(z["shape"]) == [3, 3]
    assert list(z["indptr"]) == [0, 3, 6, 9]
    assert list(z["indices"]) == [0, 2, 1, 1, 0, 2, 2, 1, 0]
    assert np.array_equal(z["data"], [0.0, 0.5, 0.75, 0.0, 0.75, 1.0, 0.0, 0.5, 1.0])
    assert z["data"].dtype == np.float64


def test_write_knn_npz_per_row_self_values(tmp_path):
    counts = np.array([[1, 2, 3, 4], [2, 2, 2, 2]], dtype=np.uint32)       # record 1 is constant: its Kendall diagonal is 0
    idx = np.array([[1], [0]], dtype=np.int32)
    val = np.array([[0.2], [0.2]])
    self_kt = api.knn_self_values("KT", val, counts=counts)
    assert list(self_kt) == [1.0, 0.0]
    assert list(api.knn_self_values("JSD", val)) == [0.0, 0.0]
    buf = tmp_path / "kt.npz"
    api.write_knn_npz(str(buf), idx, val, self_kt)
    z = np.load(str(buf))
    assert list(z["data"]) == [1.0, 0.2, 0.0, 0.2]


def test_write_knn_npz_empty_rows(tmp_path):
    path = tmp_path / "one.npz"
    api.write_knn_npz(str(path), np.zeros((1, 0), np.int32), np.zeros((1, 0)), 0.0)
    z = np.load(str(path))
    assert list(z["indptr"]) == [0, 1] and list(z["indices"]) == [0] and list(z["data"]) == [0.0]


@pytest.mark.parametrize("k", [0, 1025, -3, 2.0, True, "8"])
def test_knn_k_validation(k):
    with pytest.raises(_lib.PhyloligoError) as e:
        api.check_knn_k(k)
    assert e.value.status == _lib.PO_EINVAL


def test_knn_k_accepted_range():
    assert api.check_knn_k(1) == 1 and api.check_knn_k(np.int64(301)) == 301 and api.check_knn_k(1024) == 1024


def test_write_knn_npz_is_deterministic(tmp_path):
    idx = np.arange(12, dtype=np.int32).reshape(4, 3) % 4
    val = np.linspace(0, 1, 12).reshape(4, 3)
    a, b = tmp_path / "a.npz", tmp_path / "b.npz"
    api.write_knn_npz(str(a), idx, val, 0.0)
    api.write_knn_npz(str(b), idx, val, 0.0)
    assert a.read_bytes() == b.read_bytes()


def test_write_knn_npz_reads_back_with_scipy(tmp_path):
    sparse = pytest.importorskip("scipy.sparse")
    idx = np.array([[1, 2], [2, 0], [0, 1]], dtype=np.int32)
    val = np.array([[0.1, 0.3], [0.2, 0.1], [0.3, 0.2]])
    path = tmp_path / "g.npz"
    api.write_knn_npz(str(path), idx, val, 0.0)
    g = sparse.load_npz(str(path))
    assert g.format == "csr" and g.shape == (3, 3)
    assert np.array_equal(g.indptr, [0, 3, 6, 9])
    assert g[0, 2] == 0.3 and g[2, 1] == 0.2
