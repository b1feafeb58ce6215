#!/usr/bin/env python3
"""Generate tests/golden/silhouette.npz by RUNNING scikit-learn's silhouette_samples on the CPU (build container only; the tests
do not import scikit-learn):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_silhouette.py

The matrices are tests/kmedoids_ref.matrix(n) for n = 257, 600, 1000 in float64 and float32 (the float32 matrix is cast to
float64 for scikit-learn: exactly the values the library widens), the labels those of the numpy k-medoids restatement
(tests/kmedoids_ref.kmedoids(D, K)) for K = 2 .. 10: no GPU result goes into the file.  Per case <key> of
tests/silhouette_ref.cases():
    <key>_labels   the labels (int8)
    <key>_values   sklearn.metrics.silhouette_samples(D, labels, metric="precomputed") (float64)
plus sklearn_version.
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
    from sklearn.metrics import silhouette_samples
    import kmedoids_ref
    import silhouette_ref

    out = {"sklearn_version": np.array(sklearn.__version__)}
    for key, n, dt, name, k in silhouette_ref.cases():
        d = np.array(kmedoids_ref.matrix(n, dt)).astype(np.float64)
        labels = silhouette_ref.golden_labels(n, name, k)
        values = silhouette_samples(d, labels, metric="precomputed")
        mine, mean, live = silhouette_ref.silhouette(d, labels, k)
        out[key + "_labels"] = labels.astype(np.int8)
        out[key + "_values"] = np.asarray(values, dtype=np.float64)
        print("%-16s sizes %s mean %.6f restatement max |diff| %.2e" % (key, np.bincount(labels, minlength=k).tolist(), values.mean(),
                                                                      np.abs(mine - values).max()), flush=True)
    path = os.path.join(HERE, "silhouette.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
