"""DBSCAN without a GPU: the numpy restatement (tests/dbscan_ref.py) against what scikit-learn recorded (tests/golden/dbscan.npz),
the numbering and border rules on a hand-built case, the rounds of the hook-and-jump loop, the command line's rules."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbscan_ref  # noqa: E402

from phyloligo_amd import phyloligo as P  # noqa: E402

BASE = ["-i", "x.fa", "--method", "joblib"]


def test_restatement_reproduces_every_recorded_case(golden_dir):
    g = np.load(os.path.join(golden_dir, "dbscan.npz"))
    assert str(g["sklearn_version"])
    cases = dbscan_ref.cases()
    assert len(cases) == (len(g.files) - 1) // 4 >= 100
    borders = two_clusters = 0
    for key, make, eps, ms in cases:
        assert float(np.float32(eps)) == eps, key                         # float32 holds it: no tie can depend on the rounding of eps
        for dt, name in ((np.float64, "f64"), (np.float32, "f32")):
            labels, core = dbscan_ref.dbscan(make(dt), eps, ms)
            want, want_core = g["%s_%s_labels" % (key, name)], g["%s_%s_core" % (key, name)]
            assert np.array_equal(labels, want) and np.array_equal(core, want_core), (key, name)
            borders += int(((want >= 0) & ~want_core).sum())
            two_clusters += int(want.max() >= 1)
    assert borders >= 1000 and two_clusters >= 100                        # the cases do reach the rules they are there for


LINE_LABELS, LINE_CORE, hand_built = dbscan_ref.LINE_LABELS, dbscan_ref.LINE_CORE, dbscan_ref.hand_built


def test_numbering_and_border_rules():
    """record 0 is a border record of B, so ids follow the smallest CORE index (A's 1 before B's 2), not the smallest member;
    record 3 is within eps of both clusters and its core neighbour with the lower index (2) lies in the later cluster B: it takes
    the smaller id, A's"""
    d = hand_built()
    assert dbscan_ref.degrees(d, 1.0).tolist() == [2, 4, 5, 3, 5, 4, 4, 4, 4, 5, 1]
    labels, core = dbscan_ref.dbscan(d, 1.0, 4)
    assert labels.tolist() == LINE_LABELS and core.astype(int).tolist() == LINE_CORE
    near = np.flatnonzero(dbscan_ref.neighbours(d, 1.0)[3] & core)
    assert near.tolist() == [2, 4] and labels[2] == 1 and labels[4] == 0
    labels3, core3 = dbscan_ref.dbscan(d, 1.0, 3)                          # min_samples = 3 makes record 3 core: it joins A and B
    assert core3[3] and labels3.tolist() == [0] * 10 + [-1]


def test_nan_is_nobodys_neighbour():
    d = hand_built()
    d[4, 3] = d[3, 4] = np.nan                                            # the border record's link to A
    labels, _ = dbscan_ref.dbscan(d, 1.0, 4)
    assert labels[3] == 1 and dbscan_ref.degrees(d, 1.0)[3] == 2
    d[5, :] = d[:, 5] = np.nan                                            # a record without any defined distance, its own included
    labels, core = dbscan_ref.dbscan(d, 1.0, 4)
    assert labels[5] == -1 and not core[5] and dbscan_ref.degrees(d, 1.0)[5] == 0


def test_hooking_and_jumping_bound_the_rounds():
    """one chain of n records in random order: propagation alone needs about n / 2 rounds"""
    assert dbscan_ref.rounds(dbscan_ref.line_matrix(256), 1.0, 2) <= 8
    assert dbscan_ref.rounds(hand_built(), 1.0, 4) == 2 and dbscan_ref.rounds(hand_built(), 1.0, 40) == 0


# ---- the command line ------------------------------------------------------------------------------------------------------------------
ONE_OF = ("Error, --dbscan, --kmedoids and --kmedoids-sweep write cluster labels to -o, --knn a neighbour graph and --tsne an embedding: "
          "give one of them")


@pytest.mark.parametrize("extra,want", [
    (["--dbscan", "0.1", "--kmedoids", "3"], ONE_OF),
    (["--dbscan", "0.1", "--kmedoids-sweep", "2:4"], ONE_OF),
    (["--dbscan", "0.1", "--knn", "8"], ONE_OF),
    (["--dbscan", "0.1", "--tsne", "30"], ONE_OF),
    (["--dbscan", "0.1", "--large", "memmap"],
     "Error, --dbscan writes one label per contig as text, not a matrix container: it cannot be combined with --large memmap"),
    (["--dbscan", "0.1", "--large", "h5py"],
     "Error, --dbscan writes one label per contig as text, not a matrix container: it cannot be combined with --large h5py"),
    (["--dbscan", "0.1", "-d", "KT"], "Error, --dbscan needs a distance: -d KT is a correlation (larger means closer)"),
    (["--dbscan", "-0.5"], "Error, --dbscan EPS needs a distance EPS >= 0 (got -0.5)"),
    (["--dbscan", "nan"], "Error, --dbscan EPS needs a distance EPS >= 0 (got nan)"),
    (["--dbscan", "0.1", "--dbscan-min-samples", "0"], "Error, --dbscan-min-samples M needs M >= 1 contigs (got 0)"),
    (["--dbscan-core", "core.txt"], "Error, --dbscan-core marks the core contigs of a density clustering: give --dbscan EPS with it"),
    (["--dbscan", "0.1", "--gpus", "2"], "Error, --dbscan runs on one GPU: clustering over several ranks (--gpus N > 1) is out of scope"),
    (["--dbscan", "0.1", "--method", "scoop"], "Error, --dbscan supports --method joblib|hip"),
    (["--dbscan", "0.1", "--silhouette", "s.txt"],
     "Error, --silhouette scores a clustering: give --kmedoids K or --kmedoids-sweep LO:HI with it"),
    (["--dbscan", "0.1", "--clip-percentile", "0.9", "-d", "KT"],
     "Error, --clip-percentile / --min-size need a distance: -d KT is a correlation (a large median does not mean distant)"),
])
def test_cli_refusals(monkeypatch, extra, want):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    argv = ["-i", "x.fa"] + (extra if "--method" in extra else ["--method", "joblib"] + extra)
    params = P.get_cmd(argv)
    assert P.refusal(params) == want
    assert P.launch_plan(params, {})[0] == want
    with pytest.raises(SystemExit) as e:
        P.refuse(P.refusal(params), speak=False)
    assert e.value.code == 1


def test_cli_accepts_and_plans(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    p = P.get_cmd(BASE + ["--dbscan", "0.02"])
    assert (p.dbscan, p.dbscan_min_samples, p.dbscan_dtype, p.dbscan_core) == (0.02, 5, "float64", None)
    assert P.launch_plan(p, {}) == (None, 1, True)                        # the matrix stays in a torch tensor: torch is loaded first
    for extra in (["--dbscan", "0"], ["--dbscan", "inf"], ["--dbscan", "0.02", "--dbscan-min-samples", "10", "--dbscan-dtype", "float32"],
                  ["--dbscan", "0.02", "--dbscan-core", "core.txt", "--clip-percentile", "0.9", "--min-size", "500"],
                  ["--dbscan", "0.02", "--method", "hip", "-d", "JSD", "--json-stats", "s.json"]):
        assert P.launch_plan(P.get_cmd(["-i", "x.fa"] + (extra if "--method" in extra else ["--method", "joblib"] + extra)), {}) == (None, 1, True)
    assert "--dbscan runs on one GPU" in P.launch_plan(p, {"WORLD_SIZE": "2"})[0]
    assert P.launch_plan(P.get_cmd(BASE), {}) == (None, 1, False)         # and nothing changes for a run without it


def test_abbreviations_the_other_tests_rely_on_still_parse():
    p = P.get_cmd(BASE + ["--min-s", "5"])
    assert p.min_size == 5 and p.dbscan_min_samples == 5 and p.dbscan is None
    assert P.get_cmd(BASE + ["--min-s", "7"]).dbscan_min_samples == 5
    assert P.get_cmd(BASE + ["--clip-p", "0.9"]).clip_percentile == 0.9
    assert P.get_cmd(BASE + ["--kmedoids-s", "2:3"]).kmedoids_sweep == "2:3"
    assert P.get_cmd(BASE + ["--tsne-s", "3"]).tsne_seed == 3
    assert P.get_cmd(BASE + ["--gp", "2"]).gpus == 2


def test_label_and_core_files(tmp_path):
    P.write_labels(tmp_path / "l.txt", np.array([1, -1, 0], dtype=np.int32))
    P.write_core(tmp_path / "c.txt", np.array([True, False, True]))
    assert (tmp_path / "l.txt").read_bytes() == b"1\n-1\n0\n" and (tmp_path / "c.txt").read_bytes() == b"1\n0\n1\n"
