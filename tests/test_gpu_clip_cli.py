"""--clip-percentile / --min-size / --clip-out through the command line: a clipped run equals, byte for byte, the same run on a
FASTA file that holds only the kept records; the kept set is the reference's (bin/phyloselect.R:339-357) on the oracle medians.

Input: the 600-contig ragged four-species assembly of test_cli_kmedoids plus 20 records spread through it: 12 low-complexity
outliers (homopolymer / dinucleotide repeats of 3 - 6 kb) and 8 ordinary records of 300 - 900 bases.  With the CPU oracle
(oracle/phyloligo_oracle.py, Eucl and JSD) the 0.97 quantile of the 620 medians removes 19 records: the 12 outliers and 7 ordinary
ones; the 8 short records rank 247 .. 599 of 620 by median, pass that cut and leave by --min-size 1000: 593 are kept."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import phyloligo_amd as pa
from phyloligo_amd import api, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ALL, N_KEPT, BY_MEDIAN, BY_SIZE = 620, 593, 19, 8
CLIP = ["--clip-percentile", "0.97", "--min-size", "1000"]


def _records(seed=7):
    n = 600
    seq, offsets = synthetic.ragged_assembly(n, seed=seed, median=3000, lo=1000, hi=20000, dirt=False)
    recs = [("c%07d" % i, seq[int(offsets[i]):int(offsets[i + 1])].tobytes()) for i in range(n)]
    rng = np.random.default_rng(seed + 100)
    extra = []
    for j, u in enumerate([b"A", b"C", b"AT", b"CG", b"AC", b"GT", b"AG", b"T", b"G", b"CT", b"TA", b"GC"]):
        length = int(rng.integers(3000, 6001))
        extra.append(("lowcomplexity%02d repeat=%s" % (j, u.decode()), (u * (length // len(u) + 1))[:length]))
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for j in range(8):
        extra.append(("short%02d" % j, acgt[rng.integers(0, 4, size=int(rng.integers(300, 901)))].tobytes()))
    out, kind, e = [], [], 0
    for i, r in enumerate(recs):                                      # one extra record after every 30th of the assembly
        out.append(r)
        kind.append("ordinary")
        if i % 30 == 29 and e < len(extra):
            out.append(extra[e])
            kind.append("low" if e < 12 else "short")
            e += 1
    assert e == len(extra) and len(out) == N_ALL
    return out, np.array(kind)


def _write_fasta(path, recs, width=80):
    parts = []
    for title, s in recs:
        parts.append(b">" + title.encode() + b"\n")
        parts.extend(s[p:p + width] + b"\n" for p in range(0, len(s), width))
    path.write_bytes(b"".join(parts))


def _run(*args, timeout=600):
    return subprocess.run([sys.executable, "-m", "phyloligo_amd", "--method", "joblib"] + [str(a) for a in args], capture_output=True,
                          text=True, timeout=timeout, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))


def _read_kept(path):
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    assert all(len(r) == 4 for r in rows)
    return (np.array([int(r[0]) for r in rows], dtype=np.int64), [r[1] for r in rows], np.array([int(r[2]) for r in rows], dtype=np.int64),
            np.array([float(r[3]) for r in rows]))


@pytest.fixture(scope="module")
def ctx():
    with pa.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def asm(tmp_path_factory, ctx):
    recs, kind = _records()
    fa = tmp_path_factory.mktemp("clip") / "asm.fa"
    _write_fasta(fa, recs)
    lengths = np.array([len(s) for _, s in recs], dtype=np.int64)
    offsets = np.zeros(N_ALL + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)
    counts, totals = ctx.count_profiles(np.frombuffer(b"".join(s for _, s in recs), dtype=np.uint8), offsets, "1111", "both")
    return {"fa": fa, "recs": recs, "kind": kind, "lengths": lengths, "counts": counts, "totals": totals}


def _oracle_keep(ctx, asm, metric, dtype):
    """the kept set and the medians from ctx.pairwise + numpy (not through row_medians)"""
    d = ctx.pairwise(asm["counts"], asm["totals"], metric, dtype=dtype)
    med = np.median(d.astype(np.float64), axis=1)
    return med, api.clip_keep(med, 0.97), api.clip_keep(med, 0.97, asm["lengths"], 1000)


# ---- 1. equivalence: a clipped run == the same run on the kept records -----------------------------------------------------------
MODES = {"kmedoids": (["--kmedoids", "4"], "Eucl", "float64"), "knn": (["--knn", "8"], "JSD", "float64"),
         "tsne": (["--tsne", "10", "--tsne-iter", "50"], "Eucl", "float64"), "mat": ([], "JSD", "float64"),
         "memmap": (["--large", "memmap"], "Eucl", "float32")}


@pytest.mark.parametrize("mode", list(MODES))
def test_clipped_run_equals_run_on_kept_records(ctx, asm, tmp_path, mode):
    opts, metric, clip_dtype = MODES[mode]
    suffix = ".npz" if mode == "knn" else ".out"
    out1, out2, kept_tsv = tmp_path / ("clipped" + suffix), tmp_path / ("plain" + suffix), tmp_path / "kept.tsv"
    q1, q2 = tmp_path / "freq1.txt", tmp_path / "freq2.txt"
    freq = mode == "mat"                                               # -q composes too: the frequencies of the kept records
    r = _run("-i", asm["fa"], "-d", metric, "-o", out1, *opts, *CLIP, "--clip-out", kept_tsv, *(["-q", q1] if freq else []))
    assert r.returncode == 0, r.stdout + r.stderr
    idx, words, lengths, medians = _read_kept(kept_tsv)
    # the kept set is the reference's on the oracle medians
    med, by_median, keep = _oracle_keep(ctx, asm, metric, clip_dtype)
    assert np.array_equal(idx, keep) and idx.size == N_KEPT
    dropped_m = np.setdiff1d(np.arange(N_ALL), by_median)
    dropped_s = np.setdiff1d(by_median, keep)
    assert dropped_m.size == BY_MEDIAN and set(np.flatnonzero(asm["kind"] == "low")) <= set(dropped_m)      # 12 outliers + 7 others
    assert np.array_equal(dropped_s, np.flatnonzero(asm["kind"] == "short")) and dropped_s.size == BY_SIZE
    assert np.array_equal(medians, med[idx])
    # the same mode on a FASTA file of the kept records
    fa2 = tmp_path / "kept.fa"
    _write_fasta(fa2, [asm["recs"][int(i)] for i in idx])
    r = _run("-i", fa2, "-d", metric, "-o", out2, *opts, *(["-q", q2] if freq else []))
    assert r.returncode == 0, r.stdout + r.stderr
    if mode == "knn":
        a, b = np.load(str(out1)), np.load(str(out2))
        assert sorted(a.files) == sorted(b.files)
        for key in a.files:
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
    else:
        assert out1.stat().st_size > 0 and out1.read_bytes() == out2.read_bytes()
    if mode == "memmap":
        assert out1.stat().st_size == N_KEPT * N_KEPT * 4
    if freq:
        assert q1.read_bytes() == q2.read_bytes()


# ---- 2. the list of kept records and the statistics ---------------------------------------------------------------------------------
def test_clip_out_and_json_stats(ctx, asm, tmp_path):
    out, kept_tsv, js = tmp_path / "labels.txt", tmp_path / "kept.tsv", tmp_path / "stats.json"
    r = _run("-i", asm["fa"], "-d", "Eucl", "-o", out, "--kmedoids", "4", "--kmedoids-dtype", "float32", *CLIP, "--clip-out", kept_tsv,
             "--json-stats", js)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(kept_tsv).read()
    assert text.endswith("\n") and text.count("\n") == N_KEPT
    idx, words, lengths, medians = _read_kept(kept_tsv)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < N_ALL
    assert words == [asm["recs"][int(i)][0].split()[0] for i in idx]
    assert np.array_equal(lengths, asm["lengths"][idx]) and lengths.min() >= 1000
    d = ctx.pairwise(asm["counts"], asm["totals"], "Eucl", dtype="float32")                   # --kmedoids-dtype float32: a float32 matrix
    assert np.array_equal(medians, ctx.row_medians(d)[idx])
    for i, m in zip(idx[:5], medians[:5]):                                                    # %.17g reads back exactly and is what is written
        assert ("%d\t" % i) in text and ("\t%.17g\n" % m) in text
    assert len(out.read_text().splitlines()) == N_KEPT
    st = json.load(open(js))
    assert st["clip_percentile"] == 0.97 and st["clip_min_size"] == 1000 and st["clip_dtype"] == "float32"
    assert st["clip_kept"] == N_KEPT and st["clip_dropped_by_median"] == BY_MEDIAN and st["clip_dropped_by_size"] == BY_SIZE
    assert st["clip_kept"] + st["clip_dropped_by_median"] + st["clip_dropped_by_size"] == N_ALL
    assert st["clip_threshold"] == api.clip_threshold(ctx.row_medians(d), 0.97)
    assert st["clip_medians_ms"] > 0 and st["clip_matrix_ms"] > 0 and st["contigs"] == N_KEPT


# ---- 3. the defaults change nothing ----------------------------------------------------------------------------------------------------
def test_defaults_are_off(asm, tmp_path):
    fa = tmp_path / "few.fa"
    _write_fasta(fa, asm["recs"][:64])
    a, b = tmp_path / "a.mat", tmp_path / "b.mat"
    r = _run("-i", fa, "-d", "JSD", "-o", a)
    assert r.returncode == 0, r.stdout + r.stderr
    r2 = _run("-i", fa, "-d", "JSD", "-o", b, "--clip-percentile", "1", "--min-size", "0")
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert a.read_bytes() == b.read_bytes() and r.stdout == r2.stdout


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,words", [
    (["-d", "KT", "--clip-percentile", "0.97"], ["KT", "correlation"]),
    (["--gpus", "2", "--clip-percentile", "0.97"], ["one GPU"]),
    (["--clip-percentile", "1.5"], ["0 <= P <= 1", "1.5"]),
    (["--clip-out", "KEPT"], ["--clip-out", "filter"]),
    (["--kmedoids", "700", *CLIP, "--clip-out", "KEPT"], ["--kmedoids K needs 1 <= K", "%d contigs" % N_KEPT]),
], ids=["kt", "gpus", "percentile", "clip-out-alone", "kmedoids-above-kept"])
def test_cli_refusals(asm, tmp_path, args, words):
    out, kept = tmp_path / "out.txt", tmp_path / "kept.tsv"
    r = _run("-i", asm["fa"], "-o", out, *[str(kept) if a == "KEPT" else a for a in args])
    assert r.returncode == 1, r.stdout + r.stderr
    for w in words:
        assert w in r.stderr, r.stderr
    assert not out.exists() and not kept.exists()
