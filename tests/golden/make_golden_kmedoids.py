#!/usr/bin/env python3
"""Generate tests/golden/kmedoids.npz by RUNNING THE REFERENCE'S OWN KMedoids class on the CPU (build container only; needs the
reference tree, scikit-learn and matplotlib, none of which the tests import):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kmedoids.py

bin/phyloselect.py is loaded with importlib, unmodified, after empty stand-in modules for Bio, Bio.SeqIO, hdbscan and h5py have
been placed in sys.modules (none of them is touched by the class).  Its KMedoids(distance_metric="precomputed") is run on the
cases of tests/kmedoids_ref.cases(); the inputs are regenerated from seeds by the tests (tests/tsne_ref.make_input and
eucl_matrix), so the file holds only what the reference answered, per case <key>:
    <key>_labels   labels_ (int16)
    <key>_n_iter   n_iter_
    <key>_medoids  the medoid indices after the last update, recorded by a subclass hook around _update_medoid_ics_in_place
    <key>_warned   number of "Cluster c is empty!" warnings
plus sklearn_version.  A float32 matrix is handed over as float32: the reference then sums in float32.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REF_ROOT = os.environ.get("PHYLOLIGO_REFERENCE", "/root/reference")


def load_reference():
    import matplotlib
    matplotlib.use("Agg")
    for name in ("Bio", "Bio.SeqIO", "hdbscan", "h5py"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
    spec = importlib.util.spec_from_file_location("phyloselect_ref", os.path.join(REF_ROOT, "phylopackage/bin/phyloselect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import sklearn
    import kmedoids_ref
    ref = load_reference()

    class Recording(ref.KMedoids):
        start = None                                     # explicit start rows (the empty-cluster case), else the reference's own

        def _get_initial_medoid_indices(self, D, n_clusters):
            if self.start is not None:
                return list(self.start)
            return super()._get_initial_medoid_indices(D, n_clusters)

        def _update_medoid_ics_in_place(self, D, cluster_ics, medoid_ics):
            super()._update_medoid_ics_in_place(D, cluster_ics, medoid_ics)
            self.medoids_seen_ = np.array(medoid_ics, dtype=np.int64)

    out = {"sklearn_version": np.array(sklearn.__version__)}
    for key, make, k, init, max_iter in kmedoids_ref.cases():
        d = make()
        if key.startswith("rand_") or key == "cap":
            seed = int(key.split("_")[1][1:]) if key.startswith("rand_") else 0
            km = Recording(n_clusters=k, distance_metric="precomputed", init="random", random_state=seed, max_iter=max_iter)
        else:
            km = Recording(n_clusters=k, distance_metric="precomputed", init="heuristic", max_iter=max_iter)
            if key == "empty":
                km.start = [int(x) for x in init]
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            km.fit(np.array(d))
        warned = sum("is empty" in str(w.message) for w in caught)
        labels = np.asarray(km.labels_)
        out[key + "_labels"] = labels.astype(np.int16)
        out[key + "_n_iter"] = np.array(km.n_iter_)
        out[key + "_medoids"] = km.medoids_seen_.astype(np.int32)
        out[key + "_warned"] = np.array(warned)
        mine = kmedoids_ref.kmedoids(d, k, max_iter, init)
        same = np.array_equal(mine[0], labels) and np.array_equal(mine[1], km.medoids_seen_) and mine[2] == km.n_iter_
        print("%-22s n_iter %d sizes %s medoids %s warned %d restatement %s" % (key, km.n_iter_, np.bincount(labels, minlength=k).tolist()
                                                                               if k <= 13 else "-", km.medoids_seen_.tolist(), warned,
                                                                               "same" if same else "DIFFERS"), flush=True)
    path = os.path.join(HERE, "kmedoids.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
