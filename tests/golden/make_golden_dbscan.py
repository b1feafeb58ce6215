#!/usr/bin/env python3
"""Generate tests/golden/dbscan.npz by RUNNING scikit-learn's DBSCAN on the CPU (build container only; the tests do not import
scikit-learn):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dbscan.py

The matrices are tests/kmedoids_ref.matrix(n) for n = 257 and 600 at three quantiles of the matrix as eps, and distances of
random points of an integer grid (tests/dbscan_ref.grid_matrix: duplicates, entries equal to eps, border records between two
clusters), each in float64 and float32.  Every eps is a value float32 holds exactly, because scikit-learn compares a float32
matrix with float32(eps) and the library compares the widened entry with the float64 eps.  No GPU result goes into the file.
Per case <key> of tests/dbscan_ref.cases() and <t> in f64, f32:
    <key>_<t>_labels   sklearn.cluster.DBSCAN(eps=eps, min_samples=m, metric="precomputed").fit(D).labels_ (int16)
    <key>_<t>_core     the mask of core_sample_indices_ (bool)
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
    from sklearn.cluster import DBSCAN
    import dbscan_ref

    out = {"sklearn_version": np.array(sklearn.__version__)}
    borders = 0
    for key, make, eps, ms in dbscan_ref.cases():
        assert float(np.float32(eps)) == eps, key
        for dt, name in ((np.float64, "f64"), (np.float32, "f32")):
            d = np.array(make(dt))
            fit = DBSCAN(eps=eps, min_samples=ms, metric="precomputed").fit(d)
            labels = fit.labels_.astype(np.int32)
            core = np.zeros(d.shape[0], dtype=bool)
            core[fit.core_sample_indices_] = True
            mine, mine_core = dbscan_ref.dbscan(d, eps, ms)
            same = np.array_equal(mine, labels) and np.array_equal(mine_core, core)
            out["%s_%s_labels" % (key, name)] = labels.astype(np.int16)
            out["%s_%s_core" % (key, name)] = core
            borders += int(((labels >= 0) & ~core).sum())
            print("%-26s %s eps %-12.9g clusters %3d core %4d border %3d noise %4d restatement %s"
                  % (key, name, eps, labels.max() + 1, core.sum(), ((labels >= 0) & ~core).sum(), (labels < 0).sum(),
                     "equal" if same else "DIFFERS"), flush=True)
            assert same
    path = os.path.join(HERE, "dbscan.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", borders, "border records in all")


if __name__ == "__main__":
    main()
