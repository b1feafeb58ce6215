"""numpy restatement of the silhouette of po_cluster_sums_dev / po_silhouette* (include/phyloligo_amd.h): what the tests compare
the library with.  sklearn.metrics.silhouette_samples(D, labels, metric="precomputed") on the inputs scikit-learn accepts, plus the
two rules it does not have: clusters without a member are skipped, and a NaN sum over a non-empty cluster makes the value NaN
(scikit-learn prints 0).  Also the inputs the recorded cases (tests/golden/silhouette.npz) were made from."""
import numpy as np

import kmedoids_ref

# the recorded cases: what make_golden_silhouette.py runs and the tests regenerate
GOLDEN_N = (257, 600, 1000)
GOLDEN_K = tuple(range(2, 11))
GOLDEN_DTYPES = ((np.float64, "f64"), (np.float32, "f32"))


def cluster_sums(d, labels, k=None):
    """float64 [n, k]: S[i, c] = sum of d[i, j] over the columns j with labels[j] == c; an entry of another cluster is left out,
    never multiplied by 0, so a NaN outside a cluster stays outside it"""
    d64 = np.asarray(d).astype(np.float64)
    labels = np.asarray(labels)
    k = int(labels.max()) + 1 if k is None else int(k)
    out = np.zeros((d64.shape[0], k))
    for c in range(k):
        out[:, c] = d64[:, labels == c].sum(axis=1)
    return out


def silhouette(d, labels, k=None):
    """(values float64 [n], mean, non-empty clusters); ValueError for fewer than two non-empty clusters"""
    labels = np.asarray(labels)
    k = int(labels.max()) + 1 if k is None else int(k)
    n = labels.shape[0]
    sizes = np.bincount(labels, minlength=k)
    live = np.flatnonzero(sizes > 0)
    if live.size < 2:
        raise ValueError("fewer than two non-empty clusters")
    sums = cluster_sums(d, labels, k)
    values = np.zeros(n)
    for i in range(n):
        own = labels[i]
        if np.isnan(sums[i, live]).any():
            values[i] = np.nan
            continue
        if sizes[own] == 1:
            continue
        a = sums[i, own] / (sizes[own] - 1)
        b = min(sums[i, c] / sizes[c] for c in live if c != own)
        m = max(a, b)
        values[i] = 0.0 if m == 0 else (b - a) / m
    return values, float(values.sum() / n), int(live.size)


def winner(means):
    """index of the largest mean, the first one on a tie, a NaN never wins; None if all are NaN"""
    best = None
    for t, m in enumerate(means):
        if m == m and (best is None or m > means[best]):
            best = t
    return best


_LABELS = {}


def golden_labels(n, name, k):
    """labels of the numpy k-medoids restatement for the recorded matrix (n, dtype name) and k clusters; cached"""
    dt = np.float64 if name == "f64" else np.float32
    if (n, name, k) not in _LABELS:
        _LABELS[n, name, k] = kmedoids_ref.kmedoids(kmedoids_ref.matrix(n, dt), k)[0]
    return _LABELS[n, name, k]


def cases():
    """every recorded case: (key, n, dtype, dtype name, k)"""
    return [("n%d_%s_k%d" % (n, name, k), n, dt, name, k) for n in GOLDEN_N for dt, name in GOLDEN_DTYPES for k in GOLDEN_K]
