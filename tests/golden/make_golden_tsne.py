#!/usr/bin/env python3
"""Generate tests/golden/tsne_sklearn.npz by RUNNING scikit-learn on the CPU (build container only; the tests never import it):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tsne.py

Input: tests/tsne_ref.make_input(1000) - synthetic.ragged_assembly(1000, seed=7, median=3000, lo=1000, hi=20000, dirt=False),
4-mers, both strands - and the Euclidean distances of its frequencies in float64 numpy.  The tests regenerate it from the
seed, so the file holds only what scikit-learn answered:
    cond                 sklearn.manifold._utils._binary_search_perplexity on the 91 squared neighbour distances, as float32
    indptr/indices/data  the CSR of sklearn.manifold._t_sne._joint_probabilities_nn (indices int16, data float32)
    seeds, kl, purity, trust, n_iter
                         per seed: TSNE(n_components=2, perplexity=30, metric="precomputed", init="random", random_state=seed,
                         method="barnes_hut", angle=0.0, max_iter=1000).fit(D): kl_divergence_, purity and trustworthiness
                         (10 neighbours, tests/tsne_ref.py's definitions) of the embedding, n_iter_
    sklearn_version, perplexity, n
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import sklearn
    from scipy.sparse import csr_matrix
    from sklearn.manifold import TSNE, _utils
    from sklearn.manifold._t_sne import _joint_probabilities_nn
    import tsne_ref

    n, perplexity = 1000, 30.0
    counts, totals, labels = tsne_ref.make_input(n)
    d = tsne_ref.eucl_matrix(counts, totals)
    k = tsne_ref.n_neighbours(n, perplexity)
    idx, val = tsne_ref.knn_lists(d, k)
    d2 = (val ** 2).astype(np.float32)
    cond = _utils._binary_search_perplexity(d2, perplexity, 0)
    # the graph TSNE builds for itself: sorted indices per row, squared distances
    order = np.argsort(idx, axis=1)
    graph = csr_matrix((np.take_along_axis(val ** 2, order, axis=1).ravel(), np.take_along_axis(idx, order, axis=1).ravel(),
                        np.arange(0, n * k + 1, k)), shape=(n, n))
    p = _joint_probabilities_nn(graph, perplexity, 0)
    p.sort_indices()
    seeds = [0, 1, 2]
    kl, pur, tru, iters = [], [], [], []
    for seed in seeds:
        t = TSNE(n_components=2, perplexity=perplexity, metric="precomputed", init="random", random_state=seed, method="barnes_hut",
                 angle=0.0, max_iter=1000)
        y = t.fit_transform(d)
        kl.append(t.kl_divergence_)
        pur.append(tsne_ref.purity(y, labels, 10))
        tru.append(tsne_ref.trustworthiness(d, y, 10))
        iters.append(t.n_iter_)
        print("seed", seed, "kl", kl[-1], "purity", pur[-1], "trust", tru[-1], "n_iter", iters[-1], flush=True)
    out = os.path.join(HERE, "tsne_sklearn.npz")
    np.savez_compressed(out, cond=cond.astype(np.float32), indptr=p.indptr.astype(np.int32), indices=p.indices.astype(np.int16),
                        data=p.data.astype(np.float32), seeds=np.array(seeds), kl=np.array(kl), purity=np.array(pur),
                        trust=np.array(tru), n_iter=np.array(iters), sklearn_version=np.array(sklearn.__version__),
                        perplexity=np.array(perplexity), n=np.array(n))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
