"""The host side of the outlier clip (--clip-percentile / --min-size): R's type-7 quantile, the order of the two filters of
bin/phyloselect.R:339-357, the refusals and the options.  No GPU."""
import argparse

import numpy as np
import pytest

from phyloligo_amd import _lib, api, phyloligo


def _refused(call, *words):
    with pytest.raises(_lib.PhyloligoError) as e:
        call()
    assert e.value.status == _lib.PO_EINVAL
    for w in words:
        assert w in str(e.value), str(e.value)


# ---- clip_threshold ------------------------------------------------------------------------------------------------------------------
def test_threshold_hand_worked():
    one = [0.25]
    for p in (0, 0.5, 0.97, 1):
        assert api.clip_threshold(one, p) == 0.25
    two = [3.0, 1.0]                                                 # sorted 1, 3: idx = p
    assert api.clip_threshold(two, 0) == 1.0 and api.clip_threshold(two, 1) == 3.0
    assert api.clip_threshold(two, 0.5) == 2.0
    assert api.clip_threshold(two, 0.97) == (1.0 - 0.97) * 1.0 + 0.97 * 3.0
    five = [0.5, 0.1, 0.4, 0.2, 0.3]                                 # sorted .1 .2 .3 .4 .5: idx = 4 p
    assert api.clip_threshold(five, 0) == 0.1 and api.clip_threshold(five, 1) == 0.5
    assert api.clip_threshold(five, 0.5) == 0.3                      # h == 0: an element, bit for bit
    assert api.clip_threshold(five, 0.25) == 0.2 and api.clip_threshold(five, 0.75) == 0.4
    h = 4 * 0.97 - 3
    assert api.clip_threshold(five, 0.97) == (1.0 - h) * 0.4 + h * 0.5
    # h == 0: the threshold element itself is kept
    assert api.clip_keep(five, 0.5).tolist() == [1, 3, 4]
    assert api.clip_keep(five, 0.75).tolist() == [1, 2, 3, 4]
    assert isinstance(api.clip_threshold(five, 0.5), float)


def test_threshold_against_numpy_quantile_kept_sets():
    rng = np.random.RandomState(42)
    for trial in range(2000):
        n = int(rng.randint(1, 60))
        x = rng.rand(n) if trial % 3 else np.round(rng.rand(n), 1)   # every third vector is full of ties
        p = float(rng.choice([0.0, 0.5, 0.9, 0.97, 1.0, rng.rand()]))
        ours = x <= api.clip_threshold(x, p)
        theirs = x <= np.quantile(x, p, method="linear")
        assert np.array_equal(ours, theirs), (trial, n, p)


def test_threshold_refusals():
    _refused(lambda: api.clip_threshold([0.1, 0.2], 1.5), "[0, 1]")
    _refused(lambda: api.clip_threshold([0.1, 0.2], -0.01), "[0, 1]")
    _refused(lambda: api.clip_threshold([0.1, 0.2], float("nan")), "[0, 1]")
    _refused(lambda: api.clip_threshold([], 0.5), "no medians")
    _refused(lambda: api.clip_threshold([0.1, 0.2, np.nan, 0.3, np.nan], 0.5), "row 2 ", "NaN")


# ---- clip_keep -----------------------------------------------------------------------------------------------------------------------
def test_keep_order_of_the_filters():
    # the short contig 4 holds the largest median: it takes part in the quantile (so 3 survives the median cut), then leaves by size
    med = np.array([0.10, 0.20, 0.30, 0.40, 0.90])
    lengths = np.array([5000, 5000, 5000, 5000, 300])
    thr = api.clip_threshold(med, 0.75)
    assert thr == 0.40
    keep = api.clip_keep(med, 0.75, lengths, 1000)
    assert keep.dtype == np.int64 and keep.tolist() == [0, 1, 2, 3]
    # had the size cut come first the quantile of the four others would have removed 3 as well
    assert (med[:4] <= api.clip_threshold(med[:4], 0.75)).tolist() == [True, True, True, False]
    # a short contig under the threshold goes by size only
    assert api.clip_keep(med, 0.75, np.array([5000, 300, 5000, 5000, 5000]), 1000).tolist() == [0, 2, 3]
    assert api.clip_keep(med, 0.75, lengths, 300).tolist() == [0, 1, 2, 3]          # lengths >= min_size: 300 stays ... by size


def test_keep_ties_skips_and_nan():
    med = np.array([0.3, 0.1, 0.3, 0.3, 0.2, 0.9])
    assert api.clip_threshold(med, 0.6) == 0.3
    assert api.clip_keep(med, 0.6).tolist() == [0, 1, 2, 3, 4]                       # every tie at the threshold is kept
    lengths = np.array([10, 20, 30, 40, 50, 60])
    assert api.clip_keep(med, 1, lengths, 0).tolist() == [0, 1, 2, 3, 4, 5]          # both off
    assert api.clip_keep(med, 1, lengths, 35).tolist() == [3, 4, 5]                  # the median cut skipped
    assert api.clip_keep(med, 0.6, lengths, 0).tolist() == [0, 1, 2, 3, 4]           # the size cut skipped
    assert api.clip_keep(med, 0.6).tolist() == api.clip_keep(med, 0.6, None, 0).tolist()
    assert api.clip_keep(med, 0).tolist() == [1]
    nan = np.array([0.3, np.nan, 0.2])
    _refused(lambda: api.clip_keep(nan, 0.97), "row 1 ", "NaN")
    assert api.clip_keep(nan, 1, np.array([1, 2, 3]), 2).tolist() == [1, 2]          # percentile == 1 never looks at the medians
    _refused(lambda: api.clip_keep(med, 0.5, None, 10), "length")
    _refused(lambda: api.clip_keep(med, 0.5, lengths[:3], 10), "length")
    _refused(lambda: api.clip_keep(med, 2.0), "[0, 1]")
    _refused(lambda: api.clip_keep(med, 0.5, lengths, -1), "negative")
    assert api.clip_keep(np.zeros(0), 0.5).tolist() == []


# ---- the CLI's options and refusals --------------------------------------------------------------------------------------------------
def _params(*extra):
    return phyloligo.get_cmd(["-i", "x.fa", "--method", "joblib"] + list(extra))


def test_options_parse():
    p = _params()
    assert p.clip_percentile == 1.0 and p.min_size == 0 and p.clip_out is None
    assert not phyloligo._clip_active(p) and phyloligo._clip_refused(p) is None
    p = _params("--clip-percentile", "0.97", "--min-size", "1000", "--clip-out", "kept.tsv")
    assert p.clip_percentile == 0.97 and p.min_size == 1000 and p.clip_out == "kept.tsv"
    assert phyloligo._clip_active(p) and phyloligo._clip_refused(p) is None
    assert phyloligo._clip_active(_params("--min-size", "500")) and phyloligo._clip_active(_params("--clip-percentile=0.5"))
    assert not phyloligo._clip_active(_params("--clip-percentile", "1", "--min-size", "0"))
    with pytest.raises(SystemExit):
        _params("--min-size", "1.5")
    with pytest.raises(SystemExit):
        _params("--clip-percentile", "most")


def test_clip_refused(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    r = phyloligo._clip_refused
    assert "0 <= P <= 1" in r(_params("--clip-percentile", "1.5")) and "1.5" in r(_params("--clip-percentile", "1.5"))
    assert "0 <= P <= 1" in r(_params("--clip-percentile", "-0.1"))
    assert "0 <= P <= 1" in r(_params("--clip-percentile", "nan"))
    assert "L >= 0" in r(_params("--min-size", "-5")) and "-5" in r(_params("--min-size", "-5"))
    assert "--clip-out" in r(_params("--clip-out", "k.tsv")) and "filter" in r(_params("--clip-out", "k.tsv"))
    assert "--clip-out" in r(_params("--clip-out", "k.tsv", "--clip-percentile", "1", "--min-size", "0"))
    assert "KT" in r(_params("--clip-percentile", "0.9", "-d", "KT")) and "correlation" in r(_params("--min-size", "10", "-d", "KT"))
    assert "one GPU" in r(_params("--clip-percentile", "0.9", "--gpus", "2"))
    assert "joblib|hip" in r(phyloligo.get_cmd(["-i", "x.fa", "--method", "scoop", "--min-size", "10"]))
    # options that are off refuse nothing, whatever else is asked for
    assert r(_params("-d", "KT", "--gpus", "4")) is None
    assert r(phyloligo.get_cmd(["-i", "x.fa", "--method", "scoop"])) is None
    assert r(argparse.Namespace(dist="JSD", gpus=1, mthdrun="hip")) is None          # a caller's own namespace without the options
    for mode in (["--kmedoids", "4"], ["--knn", "8"], ["--tsne", "10"], ["--large", "memmap"], ["--large", "h5py"], ["-q", "f.txt"]):
        assert r(_params("--clip-percentile", "0.97", "--min-size", "1000", *mode)) is None
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "one GPU" in r(_params("--min-size", "10"))
    assert r(_params()) is None
