"""numpy restatement of the DBSCAN of po_dbscan* (include/phyloligo_amd.h): what the tests compare the library with, and the
inputs the recorded cases (tests/golden/dbscan.npz) were made from.  Every entry is widened to float64 before it is compared; a
NaN is nobody's neighbour."""
import numpy as np

# the recorded cases: what make_golden_dbscan.py runs through scikit-learn and the tests regenerate.  Every eps is a value
# float32 holds exactly: scikit-learn compares a float32 matrix with float32(eps), the library with the float64 eps.
EUCL_N = (257, 600)
EUCL_QUANTILES = (0.01, 0.03, 0.1)          # eps = that quantile of the matrix, rounded to float32
EUCL_MIN_SAMPLES = (3, 5, 10)
GRID_SEEDS = (0, 1, 2, 3, 4, 5)
GRID_N = (1, 2, 7, 40, 79, 130)
GRID_EPS = (1.0, 1.5, 2.0, 2.5)
GRID_MIN_SAMPLES = (1, 2, 4, 6)


def neighbours(d, eps):
    """bool [n, n]: d[i, j] <= eps in float64 (False for NaN)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(d).astype(np.float64) <= float(eps)


def degrees(d, eps):
    return neighbours(d, eps).sum(axis=1).astype(np.int32)


def dbscan(d, eps, min_samples):
    """(labels int32 [n], core bool [n]) by rules 1 - 6 of the header"""
    nb = neighbours(d, eps)
    n = nb.shape[0]
    core = nb.sum(axis=1) >= min_samples
    root = np.full(n, -1, dtype=np.int64)
    for i in np.flatnonzero(core):                      # ascending: the first record of a component is its smallest core index
        if root[i] >= 0:
            continue
        root[i] = i
        stack = [i]
        while stack:
            a = stack.pop()
            for b in np.flatnonzero(nb[a] & core & (root < 0)):
                root[b] = i
                stack.append(b)
    roots = np.flatnonzero(core & (root == np.arange(n)))
    ident = {int(r): c for c, r in enumerate(roots)}    # ids ascend with the roots
    labels = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        if core[i]:
            labels[i] = ident[int(root[i])]
        else:
            near = np.flatnonzero(nb[i] & core)
            if near.size:
                labels[i] = min(ident[int(root[j])] for j in near)
    return labels, core


def rounds(d, eps, min_samples):
    """the propagation rounds the library's loop makes (the one that changes nothing included): minimum label within eps,
    hooking of every tree's root, pointer jumping - po_dbscan_result.passes"""
    nb = neighbours(d, eps)
    n = nb.shape[0]
    core = nb.sum(axis=1) >= min_samples
    idx = np.flatnonzero(core)
    if idx.size == 0:
        return 0
    none = np.iinfo(np.int32).max
    lab = np.where(core, np.arange(n), none).astype(np.int64)
    passes = 0
    while True:
        passes += 1
        m = np.array([lab[nb[i]].min() if nb[i].any() else none for i in idx])
        new = lab.copy()
        new[idx] = np.minimum(lab[idx], m)
        np.minimum.at(new, lab[idx], new[idx])           # hook
        while True:                                      # jump
            nxt = new.copy()
            nxt[idx] = new[new[idx]]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            return passes
        lab = new


def grid_matrix(n, seed, dtype=np.float64):
    """Euclidean distances of n random points of an integer grid with about four cells per point (duplicates, entries equal to
    eps and border records within eps of two clusters are the rule)"""
    rng = np.random.RandomState(1000 + seed)
    p = rng.randint(0, max(3, int(2.0 * np.sqrt(n))), size=(n, 2)).astype(np.float64)
    diff = p[:, None, :] - p[None, :, :]
    return np.sqrt((diff * diff).sum(axis=2)).astype(dtype)


def line_matrix(n, seed=0, dtype=np.float64):
    """|x_i - x_j| for a random permutation x of 0 .. n-1: with eps = 1 one chain of n records"""
    x = np.random.RandomState(seed).permutation(n).astype(dtype)
    return np.abs(x[:, None] - x[None, :])


# positions on a line, eps = 1, min_samples = 4: A = {0, 0.5, 0.75, 1}, B = {3, 3.25, 3.5, 4}, all core; 2 is within eps of A's 1
# and of B's 3 and has 3 neighbours; 5 is within eps of B's 4 only; 9 of nobody
LINE = [5.0, 0.0, 3.0, 2.0, 1.0, 0.5, 0.75, 3.25, 3.5, 4.0, 9.0]
LINE_LABELS = [1, 0, 1, 0, 0, 0, 0, 1, 1, 1, -1]
LINE_CORE = [0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0]


def hand_built(dtype=np.float64):
    x = np.array(LINE, dtype=np.float64)
    return np.abs(x[:, None] - x[None, :]).astype(dtype)


def eucl_eps(n, q):
    """the q quantile of kmedoids_ref.matrix(n), rounded to float32"""
    import kmedoids_ref
    return float(np.float32(np.quantile(kmedoids_ref.matrix(n), q)))


def cases():
    """every recorded case: (key, matrix maker (dtype) -> matrix, eps, min_samples); recorded for float64 and float32 (<key>_f64 ...)"""
    import kmedoids_ref
    out = []
    for n in EUCL_N:
        for q in EUCL_QUANTILES:
            for ms in EUCL_MIN_SAMPLES:
                out.append(("eucl_n%d_q%g_m%d" % (n, q, ms), (lambda dt, n=n: kmedoids_ref.matrix(n, dt)), eucl_eps(n, q), ms))
    for seed, n in zip(GRID_SEEDS, GRID_N):
        for eps in GRID_EPS:
            for ms in GRID_MIN_SAMPLES:
                out.append(("grid_s%d_n%d_e%g_m%d" % (seed, n, eps, ms), (lambda dt, n=n, seed=seed: grid_matrix(n, seed, dt)), eps, ms))
    return out
