"""t-SNE of the k-NN graph on the GPU (po_tsne*): affinities, gradient, the first steps of the optimiser, whole runs
against what scikit-learn recorded (tests/golden/tsne_sklearn.npz), determinism, refusals, the CLI and one run at 50 000."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_ref  # noqa: E402

import phyloligo_amd as pa  # noqa: E402
from phyloligo_amd import _lib, api, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tsne_sklearn.npz")
F32_EPS = float(np.finfo(np.float32).eps)


def _assembly(n):
    return synthetic.ragged_assembly(n, seed=7, median=3000, lo=1000, hi=20000, dirt=False)


@pytest.fixture(scope="module")
def ctx():
    with pa.Context(0) as c:
        yield c


def _child(tmp_path, job, *args, timeout):
    """one long GPU step in a process of its own, ended after `timeout` seconds: its results as a dict of arrays"""
    out = tmp_path / (job + ".npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tsne_child.py"), job, str(out)] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(str(out)))


_PROFILES = {}


def _profiles(ctx, n):
    if n not in _PROFILES:
        seq, offsets = _assembly(n)
        _PROFILES[n] = ctx.count_profiles(seq, offsets, "1111", "both")
    return _PROFILES[n]


_LISTS = {}


def _lists(ctx, n, metric, perplexity):
    key = (n, metric, perplexity)
    if key not in _LISTS:
        counts, totals = _profiles(ctx, n)
        _LISTS[key] = ctx.knn(counts, totals, api.tsne_neighbours(n, perplexity), metric)
    return _LISTS[key]


# ---- 1. affinities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["Eucl", "JSD"])
@pytest.mark.parametrize("perplexity", [5, 30, 100])
def test_affinities(ctx, metric, perplexity):
    from scipy import sparse
    n = 1999
    idx, val = _lists(ctx, n, metric, perplexity)
    a = ctx.tsne_affinities(idx, val, perplexity, metric)
    cond, beta = a["cond"], a["beta"]
    assert cond.shape == idx.shape and cond.dtype == np.float64
    # properties of the search itself: rows sum to 1, entropy within the stopping rule of log(perplexity)
    assert np.abs(cond.sum(axis=1) - 1.0).max() < 1e-12
    h = -(cond * np.log(np.maximum(cond, 1e-300))).sum(axis=1)
    print("entropy error", np.abs(h - np.log(perplexity)).max())
    assert np.abs(h - np.log(perplexity)).max() <= 1e-5 + 1e-12
    # the same search in numpy: float64 rounding only (sums in another order)
    rc, rb = tsne_ref.binary_search_perplexity(val, perplexity)
    print("beta rel", np.abs(beta / rb - 1).max(), "cond abs", np.abs(cond - rc).max())
    np.testing.assert_allclose(beta, rb, rtol=1e-12)
    np.testing.assert_allclose(cond, rc, rtol=1e-9, atol=1e-15)
    # the CSR against scipy's (C + C^T) / sum of the same C
    k = idx.shape[1]
    c = sparse.csr_matrix((cond.ravel(), idx.ravel().astype(np.int64), np.arange(0, n * k + 1, k)), shape=(n, n))
    p = c + c.T
    p = p / p.sum()
    p.sort_indices()
    assert np.array_equal(a["rowptr"], p.indptr.astype(np.int64))
    assert np.array_equal(a["col"], p.indices.astype(np.int32))
    assert a["p"].dtype == np.float32
    np.testing.assert_allclose(a["p"], p.data, rtol=4 * F32_EPS)                       # a few ulp of float32, the storage type
    assert all(np.all(np.diff(a["col"][a["rowptr"][i]:a["rowptr"][i + 1]]) > 0) for i in range(n))
    assert abs(float(a["p"].astype(np.float64).sum()) - 1.0) < 1e-5


# ---- 2. gradient --------------------------------------------------------------------------------------------------------------
def _clouds(n):
    rng = np.random.RandomState(11)
    start = api.tsne_start(n, 0)
    spread = (30.0 * rng.standard_normal((n, 2))).astype(np.float32)
    coincident = spread.copy()
    coincident[rng.choice(n, 200, replace=False)] = coincident[0]
    return {"start": start, "spread": spread, "coincident": coincident}


@pytest.mark.parametrize("cloud", ["start", "spread", "coincident"])
@pytest.mark.parametrize("exaggeration", [12.0, 1.0])
def test_gradient(ctx, cloud, exaggeration):
    n, perplexity = 1999, 30
    idx, val = _lists(ctx, n, "Eucl", perplexity)
    a = ctx.tsne_affinities(idx, val, perplexity, "Eucl")
    p = tsne_ref.dense_of(a["rowptr"], a["col"], a["p"].astype(np.float64), n)
    y = _clouds(n)[cloud]
    grad, z, kl = ctx.tsne_gradient(a["rowptr"], a["col"], a["p"], y, exaggeration)
    g64, z64, kl64 = tsne_ref.gradient(p, y, exaggeration, np.float64)
    g32, z32, kl32 = tsne_ref.gradient(p, y, exaggeration, np.float32)
    scale = np.abs(g64).max()
    err_np32 = np.abs(g32.astype(np.float64) - g64).max() / scale
    err_gpu = np.abs(grad.astype(np.float64) - g64).max() / scale
    zerr_np32, zerr_gpu = abs(z32 / z64 - 1), abs(z / z64 - 1)
    kl_limit = exaggeration * (zerr_gpu + 4 * F32_EPS)
    print("%s e=%g: grad err / max|grad|: numpy float32 %.3e, GPU %.3e, limit %.3e; Z rel: numpy float32 %.3e, GPU %.3e, limit %.3e; "
          "KL abs: numpy float32 q %.3e, GPU %.3e, limit %.3e"
          % (cloud, exaggeration, err_np32, err_gpu, 4 * err_np32, zerr_np32, zerr_gpu, 4 * zerr_np32, abs(kl32 - kl64), abs(kl - kl64),
             kl_limit))
    # Gradient, max-norm relative to max|grad|.  Limit = 4 x the error of the same sums in numpy float32 (per-pair terms and pairwise
    # accumulation in float32) of the same case: same per-term rounding, another blocked summation order.  Measured on the MI355X,
    # numpy float32 / GPU / limit, for start, spread, coincident:
    #   e = 12:  7.1e-8 / 3.2e-8 / 2.8e-7    8.9e-8 / 6.8e-8 / 3.6e-7    3.4e-7 / 1.4e-7 / 1.4e-6
    #   e = 1:   7.1e-8 / 5.0e-8 / 2.8e-7    2.6e-7 / 4.3e-7 / 1.0e-6    5.4e-7 / 2.5e-7 / 2.2e-6
    assert err_gpu <= 4 * err_np32
    # Z, relative; the same rule.  Measured numpy float32 / GPU / limit: start 3.9e-8 / 3.8e-8 / 1.5e-7, spread 1.1e-7 / 1.1e-8 /
    # 4.4e-7, coincident 7.4e-7 / 6.8e-8 / 3.0e-6 (the kernel adds its 256-point tiles in float64)
    assert zerr_gpu <= 4 * zerr_np32
    # KL = sum of e p log(e p Z / q) in float64 with the kernel's float32 q and its Z: an error dZ / Z moves it by e sum(p) dZ / Z =
    # e dZ / Z, and q carries at most 4 float32 ulp (three roundings in 1 + d^2, one ulp of v_rcp_f32), so |dKL| <= e (dZ / Z +
    # 4 ulp) if every error had the same sign.  Measured GPU / limit: e = 12: 2e-7 / 6.2e-6, 1e-7 / 5.9e-6, 1e-6 / 6.5e-6;
    # e = 1: 2e-8 / 5.2e-7, < 1e-8 / 4.9e-7, 6e-8 / 5.5e-7
    assert abs(kl - kl64) <= kl_limit


def test_gradient_at_50000(tmp_path):
    """the j-split and the large-n summation: repulsion of 256 sampled rows and Z against float64 over all pairs"""
    import torch
    import tsne_child
    n = 50000
    y = tsne_child.cloud50000()
    got = _child(tmp_path, "grad50000", timeout=300)            # an empty P: the gradient is -4 repulsion / Z
    grad, z = got["grad"], float(got["z"])
    yt = torch.from_numpy(y.astype(np.float64))
    z64 = 0.0
    for lo in range(0, n, 1000):
        d = ((yt[lo:lo + 1000, None, :] - yt[None, :, :]) ** 2).sum(dim=2)
        z64 += float((1.0 / (1.0 + d)).sum())
    z64 -= n
    rows = np.random.RandomState(6).choice(n, 256, replace=False)

    def repulsion(dtype):
        yy = y.astype(dtype)
        dx = yy[rows, None, 0] - yy[None, :, 0]
        dy = yy[rows, None, 1] - yy[None, :, 1]
        q = dtype(1) / (dtype(1) + dx * dx + dy * dy)
        q2 = q * q
        return np.stack([(q2 * dx).sum(axis=1, dtype=dtype), (q2 * dy).sum(axis=1, dtype=dtype)], axis=1).astype(np.float64)

    want = -4.0 * repulsion(np.float64) / z64
    np32 = -4.0 * repulsion(np.float32) / z64
    err = np.abs(grad[rows].astype(np.float64) - want).max() / np.abs(want).max()
    err_np32 = np.abs(np32 - want).max() / np.abs(want).max()
    print("n=50000: Z GPU %.12g float64 %.12g rel %.3e, limit %.3e; repulsion of 256 rows, err / max: numpy float32 %.3e, GPU %.3e, "
          "limit %.3e" % (z, z64, abs(z / z64 - 1), 4 * F32_EPS, err_np32, err, 4 * err_np32))
    # Z is a sum of positive terms, so its relative error is at most that of a term - 4 float32 ulp (three roundings in 1 + d^2,
    # one ulp of v_rcp_f32) - plus the accumulation, which averages out over 10^7 tiles added in float64.  Measured: 6.5e-9, limit 4.8e-7.
    assert abs(z / z64 - 1) <= 4 * F32_EPS
    # the 256 rows: the gradient's rule, 4 x the same sums in numpy float32.  Measured: numpy float32 1.5e-7, GPU 2.8e-7 of the largest force, limit 6.1e-7.
    assert err <= 4 * err_np32


# ---- 3. trajectory --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exploration_iter", [None, 2])
def test_first_steps_follow_the_float64_optimiser(ctx, exploration_iter):
    import torch
    n, perplexity = 1000, 30
    idx, val = _lists(ctx, n, "Eucl", perplexity)
    a = ctx.tsne_affinities(idx, val, perplexity, "Eucl")
    p = tsne_ref.dense_of(a["rowptr"], a["col"], a["p"].astype(np.float64), n)
    y0 = api.tsne_start(n, 0)
    explore = 250 if exploration_iter is None else exploration_iter
    _, y64, b64 = tsne_ref.optimise(p, y0, 5, explore, dtype=np.float64, keep=(1, 3, 5))
    _, y32, b32 = tsne_ref.optimise(p, y0, 5, explore, dtype=np.float32, keep=(1, 3, 5))
    dev = {key: torch.from_numpy(v).cuda() for key, v in a.items()}
    for it in (1, 3, 5):
        y = ctx.tsne_optimise(dev["rowptr"], dev["col"], dev["p"], torch.from_numpy(y0).cuda(), max_iter=it,
                              exploration_iter=exploration_iter).cpu().numpy()
        scale = np.abs(y64[it]).max()
        err_np32 = np.abs(y32[it].astype(np.float64) - y64[it]).max() / scale
        err_gpu = np.abs(y.astype(np.float64) - y64[it]).max() / scale
        print("exploration %s, %d steps: deviation / max|y|: numpy float32 %.3e, GPU %.3e, limit %.3e; gain branches differing "
              "(numpy float32) %d" % (exploration_iter, it, err_np32, err_gpu, 4 * err_np32, int((b32[it] != b64[it]).sum())))
        # Limit = 4 x the float32 numpy run of the same optimiser (another summation order, the same per-term rounding); every point
        # counts.  Measured on the MI355X after 1 / 3 / 5 steps, numpy float32 / GPU / limit:
        #   default schedule:   8.5e-8 / 8.0e-8 / 3.4e-7    3.7e-7 / 2.6e-7 / 1.5e-6    2.4e-7 / 2.6e-7 / 9.6e-7
        #   phase switch at 2:  8.5e-8 / 8.0e-8 / 3.4e-7    1.3e-7 / 9.8e-8 / 5.4e-7    2.8e-7 / 3.9e-7 / 1.1e-6
        assert err_gpu <= 4 * err_np32


# ---- 4. whole runs against scikit-learn's record -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_whole_run_against_sklearn_record(tmp_path, seed):
    g = np.load(GOLDEN)
    n = int(g["n"])
    counts, totals, labels = tsne_ref.make_input(n)
    d = tsne_ref.eucl_matrix(counts, totals)
    got = _child(tmp_path, "whole", seed, timeout=300)
    y, kl = got["y"], float(got["kl"])
    p = tsne_ref.dense_of(got["rowptr"], got["col"], got["p"].astype(np.float64), n)
    kl64 = tsne_ref.kl_divergence(p, y)
    spread_kl = float(g["kl"].max() - g["kl"].min())
    spread_tr = float(g["trust"].max() - g["trust"].min())
    pur, tru = tsne_ref.purity(y, labels, 10), tsne_ref.trustworthiness(d, y, 10)
    print("seed %d: KL %.9f (float64 from y: %.9f), sklearn %s; purity %.4f; trustworthiness %.4f (sklearn %s); iterations %d"
          % (seed, kl, kl64, g["kl"], pur, tru, g["trust"], int(got["iterations"])))
    assert np.isfinite(y).all() and y.shape == (n, 2) and y.dtype == np.float32
    # the same sum with float32 q and Z: |dKL| <= dZ / Z + 4 float32 ulp (see test_gradient), dZ / Z itself at most 4 ulp
    assert abs(kl - kl64) <= 8 * F32_EPS
    assert kl <= float(g["kl"].max()) + 3 * spread_kl
    assert pur == 1.0
    assert tru >= float(g["trust"].min()) - spread_tr


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------
def test_same_bytes_twice_and_through_torch(ctx):
    import torch
    n, perplexity = 1999, 30
    idx, val = _lists(ctx, n, "JSD", perplexity)
    y1, s1 = ctx.tsne(idx, val, perplexity, max_iter=300, want_stats=True, metric="JSD")
    y2, s2 = ctx.tsne(idx, val, perplexity, max_iter=300, want_stats=True, metric="JSD")
    assert y1.tobytes() == y2.tobytes() and s1["kl"] == s2["kl"] and s1["iterations"] == s2["iterations"]
    assert s1["history"] == s2["history"]
    yt, st = ctx.tsne(torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda(), perplexity, max_iter=300, want_stats=True,
                      metric="JSD")
    assert yt.is_cuda and yt.cpu().numpy().tobytes() == y1.tobytes() and st["kl"] == s1["kl"] and st["iterations"] == s1["iterations"]
    a1, a2 = ctx.tsne_affinities(idx, val, perplexity, "JSD"), ctx.tsne_affinities(idx, val, perplexity, "JSD")
    assert all(a1[key].tobytes() == a2[key].tobytes() for key in a1)


# ---- 6. refusals on the device ------------------------------------------------------------------------------------------------------
def _refused(ctx, idx, val, perplexity, metric, *words):
    with pytest.raises(_lib.PhyloligoError) as e:
        ctx.tsne(idx, val, perplexity, max_iter=50, metric=metric)
    assert e.value.status == _lib.PO_EINVAL
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals_leave_the_context_usable(ctx):
    n, perplexity = 600, 10
    idx, val = _lists(ctx, n, "Eucl", perplexity)
    # a BC input with two empty records: 0 / 0 between them is NaN, and with K = n - 1 every list holds every other record
    m = 24
    seq, offsets = _assembly(m)
    parts = [seq[int(offsets[i]):int(offsets[i + 1])] for i in range(m)]
    parts[7] = parts[12] = seq[:0]
    off2 = np.zeros(m + 1, dtype=np.uint64)
    off2[1:] = np.cumsum([len(q) for q in parts])
    counts, totals = ctx.count_profiles(np.concatenate(parts), off2, "1111", "both")
    assert totals[7] == 0 and totals[12] == 0
    bi, bv = ctx.knn(counts, totals, api.tsne_neighbours(m, perplexity), "BC")
    assert np.isnan(bv).any()
    first_nan = int(np.flatnonzero(np.isnan(bv).any(axis=1))[0])
    _refused(ctx, bi, bv, perplexity, "BC", "NaN", "row %d " % first_nan)
    neg = val.copy()
    neg[41, 3] = -1.0
    _refused(ctx, idx, neg, perplexity, "Eucl", "negative", "row 41 ")
    ki, kv = ctx.knn(*_profiles(ctx, n), api.tsne_neighbours(n, perplexity), "KT")
    _refused(ctx, ki, kv, perplexity, "KT", "KT")
    _refused(ctx, idx, val, 342, "Eucl", "perplexity", "1024")
    _refused(ctx, idx[:3, :2], val[:3, :2], 1, "Eucl", "at least 4")
    dup = idx.copy()
    dup[17, 5] = dup[17, 2]
    _refused(ctx, dup, val, perplexity, "Eucl", "twice", "row 17 ")
    # the library's own argument checks, past the Python layer: perplexity too large for PO_KNN_MAX_K, and a k that is not
    # min(n - 1, int(3 perplexity + 1))
    import ctypes
    lib = _lib.load()
    y0, y = api.tsne_start(n, 0), np.zeros((n, 2), np.float32)
    idx32, val64 = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(val, np.float64)
    for perp, k, words in ((342.0, idx.shape[1], ("perplexity 342", "PO_KNN_MAX_K")), (float(perplexity), idx.shape[1] - 1, ("k = 30", "31"))):
        rc = lib.po_tsne(ctx._h, n, k, _lib.METRICS["Eucl"], _lib.PO_F64, idx32.ctypes.data, val64.ctypes.data, perp, y0.ctypes.data,
                         None, y.ctypes.data, None)
        msg = lib.po_last_error().decode()
        assert rc == _lib.PO_EINVAL and all(w in msg for w in words), msg
    rc = lib.po_tsne_affinities_dev(ctx._h, n, idx.shape[1], _lib.METRICS["Eucl"], _lib.PO_F64, None, None, 342.0, None, None, None, None,
                                    None, 0, ctypes.byref(ctypes.c_uint64()))
    assert rc == _lib.PO_EINVAL and "perplexity 342" in lib.po_last_error().decode()
    y = ctx.tsne(idx, val, perplexity, max_iter=50)
    assert y.shape == (n, 2) and np.isfinite(y).all()


# ---- 7. CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_tsne(ctx, tmp_path):
    n, perplexity = 1000, 30
    seq, offsets = _assembly(n)
    fa = tmp_path / "asm.fa"
    fa.write_bytes(synthetic.fasta_bytes(seq, offsets))
    out, js = tmp_path / "y.txt", tmp_path / "stats.json"
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", str(fa), "-d", "JSD", "--method", "joblib", "--tsne", str(perplexity),
                        "-o", str(out), "--json-stats", str(js)], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    y = np.loadtxt(str(out))
    assert y.shape == (n, 2) and np.isfinite(y).all()
    idx, val = _lists(ctx, n, "JSD", perplexity)
    want, st = ctx.tsne(idx, val, perplexity, metric="JSD", want_stats=True)
    ref = tmp_path / "ref.txt"
    np.savetxt(str(ref), want)
    assert out.read_bytes() == ref.read_bytes()
    assert tsne_ref.purity(y, np.arange(n) % 4, 10) == 1.0
    stats = json.load(open(js))
    assert stats["tsne_iterations"] == st["iterations"] and stats["tsne_kl"] == st["kl"] and stats["tsne_ms"] > 0


# ---- 8. size ------------------------------------------------------------------------------------------------------------------------------
def test_50000_contigs(tmp_path):
    n = 50000
    got = _child(tmp_path, "run50000", timeout=600)
    y, kl, history = got["y"], float(got["kl"]), got["history"]
    assert y.shape == (n, 2) and np.isfinite(y).all()
    kl300 = [k for it, k, _ in history if it == 300]
    sample = np.random.RandomState(3).choice(n, 2000, replace=False)
    pur = tsne_ref.purity(y, np.arange(n) % 4, 10, sample=sample)
    print("n=50000: KL at 300 %.5f, final %.5f, iterations %d, purity %.4f, affinities %.1f ms, optimiser %.1f ms"
          % (kl300[0], kl, int(got["iterations"]), pur, got["ms"][0], got["ms"][1]))
    assert kl < kl300[0]
    assert pur > 0.9
