"""numpy restatement of the k-medoids of po_kmedoids* (the reference's KMedoids with distance_metric="precomputed",
bin/phyloselect.py:37-309): what the tests compare the library with.  Sums in float64 whatever the matrix holds, ties to the
smaller index everywhere.  Also the inputs the recorded cases (tests/golden/kmedoids.npz) were made from."""
import numpy as np

# the recorded cases: what make_golden_kmedoids.py runs and the tests regenerate
HEURISTIC_N = (257, 600, 1000)
HEURISTIC_K = (1, 2, 4, 7, 13)
RANDOM_SEEDS = (0, 1, 2, 3, 4, 5)
RANDOM_K = (4, 7)
EMPTY_START = (5, 9, 100, 201)


def assign(d, medoids):
    """label[j] = argmin_c d[medoids[c], j]; numpy.argmin keeps the first minimum, i.e. the smaller c"""
    return np.argmin(np.asarray(d)[np.asarray(medoids, dtype=np.int64), :], axis=0).astype(np.int32)


def masked_costs(d, labels, rows=None):
    """float64: for every row i (of `rows`, or all) the sum of d[i, j] over the columns j with labels[j] == labels[i]"""
    d64 = np.asarray(d).astype(np.float64)
    labels = np.asarray(labels)
    rows = np.arange(d64.shape[0]) if rows is None else np.asarray(rows)
    out = np.zeros(rows.size)
    for t, i in enumerate(rows):
        out[t] = d64[i, labels == labels[i]].sum()
    return out


def heuristic_start(d, k):
    sums = np.asarray(d).astype(np.float64).sum(axis=1)
    return np.argsort(sums, kind="stable")[:k].astype(np.int32)


def random_start(n, k, seed):
    """the reference's init="random" with random_state=seed"""
    return np.random.RandomState(seed).permutation(n)[:k].astype(np.int32)


def kmedoids(d, k, max_iter=300, init=None):
    """(labels int32 [n], medoids int32 [k], iterations, converged)"""
    d64 = np.asarray(d).astype(np.float64)
    med = heuristic_start(d64, k) if init is None else np.array(init, dtype=np.int32)
    iterations = 0
    while True:
        iterations += 1
        labels = assign(d, med)
        changed = False
        for c in range(k):
            members = np.flatnonzero(labels == c)
            if members.size == 0:
                continue
            rows = np.concatenate([members, [med[c]]])
            costs = d64[np.ix_(rows, members)].sum(axis=1)           # the medoid's own sum by the same summation
            best = int(np.argmin(costs[:-1]))                         # first minimum: the smaller row
            if costs[best] < costs[-1] and members[best] != med[c]:
                med[c] = members[best]
                changed = True
        if not changed:
            return labels, med, iterations, True
        if iterations >= max_iter:
            return labels, med, iterations, False


def inertia(d, labels, medoids):
    d64 = np.asarray(d).astype(np.float64)
    return float(d64[np.asarray(medoids)[np.asarray(labels)], np.arange(d64.shape[0])].sum())


_INPUTS = {}


def matrix(n, dtype=np.float64):
    """Euclidean distances of tests/tsne_ref.make_input(n) in float64 numpy, rounded once for float32; cached"""
    import tsne_ref
    if n not in _INPUTS:
        counts, totals, _ = tsne_ref.make_input(n)
        m = tsne_ref.eucl_matrix(counts, totals)
        m.setflags(write=False)
        _INPUTS[n] = m
    m = _INPUTS[n]
    return m if dtype == np.float64 else m.astype(dtype)


def empty_cluster_matrix():
    """n = 600 with record 9 made a copy of record 5 (counts and totals): the start EMPTY_START leaves cluster 1 empty at first"""
    import tsne_ref
    if "empty" not in _INPUTS:
        counts, totals, _ = tsne_ref.make_input(600)
        counts, totals = counts.copy(), totals.copy()
        counts[9] = counts[5]
        totals[9] = totals[5]
        m = tsne_ref.eucl_matrix(counts, totals)
        m.setflags(write=False)
        _INPUTS["empty"] = m
    return _INPUTS["empty"]


def cases():
    """every recorded case: (key, matrix maker, k, init or None, max_iter)"""
    out = []
    for n in HEURISTIC_N:
        for k in HEURISTIC_K:
            for dt, name in ((np.float64, "f64"), (np.float32, "f32")):
                out.append(("heur_n%d_k%d_%s" % (n, k, name), (lambda n=n, dt=dt: matrix(n, dt)), k, None, 300))
    for seed in RANDOM_SEEDS:
        for k in RANDOM_K:
            out.append(("rand_s%d_k%d" % (seed, k), (lambda: matrix(600)), k, random_start(600, k, seed), 300))
    out.append(("empty", empty_cluster_matrix, 4, np.array(EMPTY_START, dtype=np.int32), 300))
    out.append(("cap", (lambda: matrix(600)), 7, random_start(600, 7, 0), 2))
    return out
