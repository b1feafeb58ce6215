"""Dense numpy restatement of the t-SNE steps of po_tsne* (scikit-learn 1.7 manifold/_t_sne.py, _utils.pyx with the exact
repulsive sum of method="barnes_hut", angle=0.0): what the tests compare the library with.  float64 unless a dtype is given;
for n up to a few thousand (everything is n x n).  No scikit-learn at run time."""
import numpy as np

PERPLEXITY_TOLERANCE = 1e-5
EPSILON_DBL = 1e-8
FLOAT32_TINY = float(np.finfo(np.float32).tiny)


def n_neighbours(n, perplexity):
    return min(n - 1, int(3.0 * perplexity + 1))


def make_input(n, k=4):
    """(counts uint32 [n, 4^k], totals uint64 [n], labels [n]) of synthetic.ragged_assembly(n, seed=7, median=3000, lo=1000,
    hi=20000, dirt=False), both strands, counted by the numpy oracle"""
    from oracle import phyloligo_oracle as po
    from phyloligo_amd import synthetic
    seq, offsets = synthetic.ragged_assembly(n, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
    contigs = [seq[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(n)]
    counts, totals = po.compute_counts(contigs, "1" * k, "both")
    return counts.astype(np.uint32), totals.astype(np.uint64), np.arange(n) % 4


def eucl_matrix(counts, totals):
    f = counts.astype(np.float64) / totals.astype(np.float64)[:, None]
    d = np.empty((f.shape[0], f.shape[0]))
    for lo in range(0, f.shape[0], 64):                       # phylodist.Eucl: sqrt(sum((a - b)^2)), no Gram cancellation
        d[lo:lo + 64] = np.sqrt(((f[lo:lo + 64, None, :] - f[None, :, :]) ** 2).sum(axis=2))
    return d


def knn_lists(d, k):
    """idx int32 [n, k], val [n, k]: the k nearest j != i of every row, ascending, ties by the smaller index"""
    n = d.shape[0]
    key = d.copy()
    np.fill_diagonal(key, np.inf)
    idx = np.argsort(key, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int32), np.take_along_axis(d, idx, axis=1)


def squared_f32(val):
    """the neighbour values as scikit-learn's search sees them: squared, then float32"""
    return (np.asarray(val, dtype=np.float64) ** 2).astype(np.float32).astype(np.float64)


def binary_search_perplexity(val, perplexity):
    """_utils._binary_search_perplexity on the squared float32 neighbour values, all rows at once: (cond [n, k], beta [n])"""
    d2 = squared_f32(val)
    n = d2.shape[0]
    beta = np.ones(n)
    lo = np.full(n, -np.inf)
    hi = np.full(n, np.inf)
    p = np.zeros_like(d2)
    active = np.ones(n, dtype=bool)
    want = np.log(perplexity)
    for _ in range(100):
        a = np.flatnonzero(active)
        if a.size == 0:
            break
        e = np.exp(-d2[a] * beta[a, None])
        s = e.sum(axis=1)
        s[s == 0.0] = EPSILON_DBL
        q = e / s[:, None]
        p[a] = q
        diff = np.log(s) + beta[a] * (d2[a] * q).sum(axis=1) - want
        done = np.abs(diff) <= PERPLEXITY_TOLERANCE
        active[a[done]] = False
        up = a[~done & (diff > 0)]
        dn = a[~done & ~(diff > 0)]
        lo[up] = beta[up]
        beta[up] = np.where(np.isinf(hi[up]), beta[up] * 2.0, (beta[up] + hi[up]) / 2.0)
        hi[dn] = beta[dn]
        beta[dn] = np.where(np.isinf(lo[dn]), beta[dn] / 2.0, (beta[dn] + lo[dn]) / 2.0)
    return p, beta


def joint_dense(idx, cond):
    """P = (C + C^T) / sum(C + C^T), dense float64 [n, n]"""
    n, k = idx.shape
    c = np.zeros((n, n))
    c[np.repeat(np.arange(n), k), idx.reshape(-1)] = cond.reshape(-1)
    p = c + c.T
    return p / max(p.sum(), np.finfo(np.float64).eps)


def csr_of(p):
    """(rowptr int64, col int32, values) of a dense matrix's non-zeros, columns ascending"""
    rows, cols = np.nonzero(p)
    rowptr = np.zeros(p.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=p.shape[0]), out=rowptr[1:])
    return rowptr, cols.astype(np.int32), p[rows, cols]


def dense_of(rowptr, col, values, n):
    p = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    p[rows, col] = values
    return p


def gradient(p, y, exaggeration=1.0, dtype=np.float64):
    """(grad [n, 2], Z, KL) of KL(exaggeration * P || Q): per-pair terms and sums in `dtype` (numpy's pairwise summation)"""
    y = np.asarray(y).astype(dtype)
    pe = (np.asarray(p) * exaggeration).astype(dtype)
    one = dtype(1.0)
    dx = y[:, None, 0] - y[None, :, 0]
    dy = y[:, None, 1] - y[None, :, 1]
    q = one / (one + dx * dx + dy * dy)
    np.fill_diagonal(q, 0)
    z = max(float(q.sum(dtype=dtype)), float(np.finfo(np.float64).eps))
    q2 = q * q
    rep = np.stack([(q2 * dx).sum(axis=1, dtype=dtype), (q2 * dy).sum(axis=1, dtype=dtype)], axis=1)
    pq = pe * q
    att = np.stack([(pq * dx).sum(axis=1, dtype=dtype), (pq * dy).sum(axis=1, dtype=dtype)], axis=1)
    grad = (dtype(4.0) * (att - rep / dtype(z))).astype(dtype)
    nz = pe > 0
    pv = pe[nz].astype(np.float64)
    qn = q[nz].astype(np.float64) / z
    kl = float(np.sum(pv * np.log(np.maximum(pv, FLOAT32_TINY) / np.maximum(qn, FLOAT32_TINY))))
    return grad, z, kl


def kl_divergence(p, y):
    return gradient(p, y, 1.0)[2]


def optimise(p, y0, n_iter, exploration_iter=250, early_exaggeration=12.0, learning_rate=None, dtype=np.float64, keep=()):
    """scikit-learn's _gradient_descent for n_iter update steps (no stopping rules: the tests compare the first few steps).
    Returns (y, {it: y after it steps for it in keep}, branches) - branches[it]: the gain branch (True = +0.2) of every
    coordinate at step it, for it in keep."""
    n = y0.shape[0]
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate is None else learning_rate
    y = np.asarray(y0).astype(dtype)
    update = np.zeros_like(y)
    gains = np.ones_like(y)
    kept, branches = {}, {}
    for it in range(n_iter):
        early = it < exploration_iter
        grad = gradient(p, y, early_exaggeration if early else 1.0, dtype)[0]
        inc = update * grad < 0
        gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8)).astype(dtype)
        gains = np.maximum(gains, dtype(0.01))
        grad = grad * gains
        update = (dtype(0.5 if early else 0.8) * update - dtype(lr) * grad).astype(dtype)
        y = y + update
        if it + 1 in keep:
            kept[it + 1] = y.copy()
            branches[it + 1] = inc.copy()
    return y, kept, branches


def purity(y, labels, k=10, sample=None):
    """fraction of the k nearest embedded neighbours (of every point, or of the sampled ones) that carry the point's label"""
    y = np.asarray(y, dtype=np.float64)
    rows = np.arange(y.shape[0]) if sample is None else np.asarray(sample)
    hits = 0
    for lo in range(0, rows.size, 512):
        r = rows[lo:lo + 512]
        d = ((y[r, None, :] - y[None, :, :]) ** 2).sum(axis=2)
        d[np.arange(r.size), r] = np.inf
        nb = np.argpartition(d, k, axis=1)[:, :k]
        hits += int((labels[nb] == labels[r, None]).sum())
    return hits / (rows.size * k)


def trustworthiness(d, y, k=10):
    """sklearn.manifold.trustworthiness(d, y, n_neighbors=k, metric="precomputed") in numpy"""
    n = d.shape[0]
    dx = np.asarray(d, dtype=np.float64).copy()
    np.fill_diagonal(dx, np.inf)
    order = np.argsort(dx, axis=1)
    rank = np.empty((n, n), dtype=np.int64)
    rank[np.arange(n)[:, None], order] = np.arange(1, n + 1)[None, :]
    y = np.asarray(y, dtype=np.float64)
    dy = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(dy, np.inf)
    nb = np.argsort(dy, axis=1)[:, :k]
    r = np.take_along_axis(rank, nb, axis=1) - k
    t = float(r[r > 0].sum())
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))
