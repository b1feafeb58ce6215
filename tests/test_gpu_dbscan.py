"""DBSCAN on the GPU (po_eps_degrees_dev, po_dbscan*): every case scikit-learn recorded (tests/golden/dbscan.npz), the numpy
restatement (tests/dbscan_ref.py) at the shapes and layouts where the row reader can go wrong, the rules of the header block, the
bound on the rounds of the component loop, refusals, the CLI (--dbscan)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbscan_ref  # noqa: E402
from dbscan_ref import LINE_CORE, LINE_LABELS, hand_built  # noqa: E402

import phyloligo_amd as pa  # noqa: E402
from phyloligo_amd import _lib, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dbscan.npz")
DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def ctx():
    with pa.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def _check(got, want_labels, want_core):
    labels, core = _np(got[0]), _np(got[1])
    assert labels.dtype == np.int32 and core.dtype == np.bool_
    assert np.array_equal(labels, want_labels) and np.array_equal(core, want_core)
    if len(got) == 3:
        st = got[2]
        assert st["core"] == int(np.sum(want_core)) and st["noise"] == int(np.sum(want_labels < 0))
        assert st["border"] == labels.size - st["core"] - st["noise"] and st["clusters"] == int(want_labels.max(initial=-1)) + 1


# ---- 1. the recorded cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f64", "f32"])
@pytest.mark.parametrize("family", ["eucl_n257", "eucl_n600", "grid"])
def test_golden_cases(ctx, torch, family, name):
    g = np.load(GOLDEN)
    dt = np.float64 if name == "f64" else np.float32
    seen = 0
    device = {}
    for key, make, eps, ms in dbscan_ref.cases():
        if not key.startswith(family):
            continue
        seen += 1
        d = np.array(make(dt))                                            # (a writable copy: torch wraps it)
        want, want_core = g["%s_%s_labels" % (key, name)].astype(np.int32), g["%s_%s_core" % (key, name)]
        _check(ctx.dbscan(d, eps, ms, want_stats=True), want, want_core)  # host pointers
        shape = key.rsplit("_", 2)[0] if family == "grid" else family
        if shape not in device:
            device[shape] = torch.from_numpy(d).cuda()
        _check(ctx.dbscan(device[shape], eps, ms, want_stats=True), want, want_core)
    assert seen >= 9


# ---- 2. against the restatement, at the shapes and layouts where the row reader can go wrong ---------------------------------------
EPS, MS = 1.5, 4
_REF = {}


def _reference(n, dtype):
    """(matrix, labels, core, degrees) of grid_matrix(n, seed n): computed once, never written"""
    if (n, dtype) not in _REF:
        d = dbscan_ref.grid_matrix(n, n, dtype)
        labels, core = dbscan_ref.dbscan(d, EPS, MS)
        for a in (d, labels, core):
            a.setflags(write=False)
        _REF[n, dtype] = (d, labels, core, dbscan_ref.degrees(d, EPS))
    return _REF[n, dtype]


def _layouts(torch, d):
    """the same matrix as: ld = n; a view one element into an (n + 3)-wide buffer (element loads); rows padded to 128-byte lines
    (one 16-byte load per group); ld = n + 5 from the start of the buffer"""
    n = d.shape[0]
    t = torch.from_numpy(np.array(d)).cuda()
    esz = d.dtype.itemsize
    out = [("ld=n", t)]
    off = torch.zeros((n, n + 3), dtype=t.dtype, device="cuda")
    off[:, 1:n + 1] = t
    out.append(("offset", off[:, 1:n + 1]))
    line = (n * esz + 127) // 128 * 128 // esz
    padded = torch.full((n, line), -1.0, dtype=t.dtype, device="cuda")     # (padding that would count as a neighbour if it were read)
    padded[:, :n] = t
    out.append(("lines", padded[:, :n]))
    wide = torch.full((n, n + 5), -1.0, dtype=t.dtype, device="cuda")
    wide[:, :n] = t
    out.append(("ld>n", wide[:, :n]))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_shapes_and_layouts(ctx, torch, n, dtype):
    d, labels, core, degree = _reference(n, dtype)
    if n >= 255:
        assert labels.max() >= 1 and (labels < 0).any() and ((labels >= 0) & ~core).any()
    host = ctx.dbscan(np.array(d), EPS, MS, want_stats=True)              # host pointers
    _check(host, labels, core)
    assert host[2]["passes"] == dbscan_ref.rounds(d, EPS, MS)
    host_degree = ctx.eps_degrees(np.array(d), EPS)
    assert host_degree.dtype == np.int32 and np.array_equal(host_degree, degree)
    for what, view in _layouts(torch, d):
        got = ctx.dbscan(view, EPS, MS, want_stats=True)
        _check(got, labels, core)
        assert got[0].is_cuda and got[2]["passes"] == host[2]["passes"], what
        deg = ctx.eps_degrees(view, EPS)
        assert deg.is_cuda and np.array_equal(_np(deg), degree), what
        again = ctx.dbscan(view, EPS, MS)
        assert _np(again[0]).tobytes() == _np(got[0]).tobytes() and _np(again[1]).tobytes() == _np(got[1]).tobytes(), what
        assert _np(ctx.eps_degrees(view, EPS)).tobytes() == _np(deg).tobytes(), what


# ---- 3. the rules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_numbering_and_border_rules(ctx, dtype):
    got = ctx.dbscan(hand_built(dtype), 1.0, 4, want_stats=True)
    _check(got, np.array(LINE_LABELS, dtype=np.int32), np.array(LINE_CORE, dtype=bool))
    assert got[2]["passes"] == 2 and (got[2]["clusters"], got[2]["core"], got[2]["border"], got[2]["noise"]) == (2, 8, 2, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_min_samples_one_and_above_n(ctx, dtype):
    d = np.array(_reference(257, dtype)[0])
    labels, core, st = ctx.dbscan(d, EPS, 1, want_stats=True)
    want, want_core = dbscan_ref.dbscan(d, EPS, 1)
    assert core.all() and want_core.all() and np.array_equal(labels, want) and st["noise"] == 0 and st["border"] == 0
    for ms in (258, 2 ** 40):
        labels, core, st = ctx.dbscan(d, EPS, ms, want_stats=True)
        assert (labels == -1).all() and not core.any()
        assert (st["clusters"], st["core"], st["border"], st["noise"], st["passes"]) == (0, 0, 0, 257, 0)
    labels, core, st = ctx.dbscan(d, np.inf, 257, want_stats=True)          # min_samples == n is reachable
    assert (labels == 0).all() and core.all() and st["clusters"] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_eps_zero_clusters_the_duplicates(ctx, dtype):
    d = np.array(_reference(255, dtype)[0])
    want, want_core = dbscan_ref.dbscan(d, 0.0, 2)
    assert want.max() >= 3 and (want < 0).any()                            # the grid has duplicate points and single ones
    _check(ctx.dbscan(d, 0.0, 2, want_stats=True), want, want_core)
    assert np.array_equal(ctx.eps_degrees(d, 0.0), (d == 0).sum(axis=1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_eps_inf_gives_one_cluster(ctx, dtype):
    d = np.array(_reference(257, dtype)[0])
    d[3, 9] = d[9, 3] = np.finfo(dtype).max
    d[4, 8] = d[8, 4] = np.inf
    labels, core, st = ctx.dbscan(d, np.inf, 5, want_stats=True)
    assert (labels == 0).all() and core.all() and (st["clusters"], st["passes"]) == (1, 2)
    assert (ctx.eps_degrees(d, np.inf) == 257).all()
    assert ctx.eps_degrees(d, 1e300).tolist() == dbscan_ref.degrees(d, 1e300).tolist()      # above every float32: all but the inf


def test_an_entry_equal_to_eps_is_a_neighbour(ctx):
    for dtype in DTYPES:
        e = dtype(0.1)
        d = np.array([[0, e], [e, 0]], dtype=dtype)
        at, below = float(e), float(np.nextafter(np.float64(e), 0.0))      # the entry as float64; the float64 just under it
        assert ctx.dbscan(d, at, 2)[0].tolist() == [0, 0] and ctx.eps_degrees(d, at).tolist() == [2, 2]
        assert ctx.dbscan(d, below, 2)[0].tolist() == [-1, -1] and ctx.eps_degrees(d, below).tolist() == [1, 1]
        assert ctx.dbscan(d, float(np.nextafter(np.float64(e), 1.0)), 2)[0].tolist() == [0, 0]
    # float32(0.1) is above the float64 0.1: the entry is widened, eps is not rounded
    d = np.array([[0, 0.1], [0.1, 0]], dtype=np.float32)
    assert float(d[0, 1]) > 0.1 and ctx.dbscan(d, 0.1, 2)[0].tolist() == [-1, -1]
    d = np.array([[0, 0.7], [0.7, 0]], dtype=np.float32)                   # float32(0.7) is below the float64 0.7
    assert float(d[0, 1]) < 0.7 and ctx.dbscan(d, 0.7, 2)[0].tolist() == [0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_entries(ctx, torch, dtype):
    d = hand_built(dtype)
    d[5, :] = d[:, 5] = np.nan                                            # a record without a defined distance: noise, degree 0
    labels, core = ctx.dbscan(d, 1.0, 4)
    want, want_core = dbscan_ref.dbscan(d, 1.0, 4)
    assert labels[5] == -1 and not core[5] and np.array_equal(labels, want) and np.array_equal(core, want_core)
    assert ctx.eps_degrees(d, 1.0)[5] == 0 and ctx.eps_degrees(d, np.inf)[5] == 0
    # two chains of core records whose only link is undefined stay two clusters
    x = np.arange(12, dtype=np.float64)
    d = np.abs(x[:, None] - x[None, :]).astype(dtype)
    joined = ctx.dbscan(d, 1.0, 2)[0]
    d[5, 6] = d[6, 5] = np.nan
    labels, core, st = ctx.dbscan(torch.from_numpy(d).cuda(), 1.0, 2, want_stats=True)
    assert (joined == 0).all() and _np(labels).tolist() == [0] * 6 + [1] * 6 and _np(core).all() and st["clusters"] == 2
    assert np.array_equal(_np(labels), dbscan_ref.dbscan(d, 1.0, 2)[0])


def _refused(call, *words):
    with pytest.raises(pa.PhyloligoError) as e:
        call()
    assert e.value.status == _lib.PO_EINVAL, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals_leave_the_context_usable(ctx, torch):
    n = 100
    d = np.array(dbscan_ref.grid_matrix(n, 3))
    t = torch.from_numpy(d).cuda()
    want = ctx.dbscan(d, EPS, MS)
    for who, call in (("po_dbscan:", lambda e, m: ctx.dbscan(d, e, m)), ("po_dbscan_dev:", lambda e, m: ctx.dbscan(t, e, m))):
        _refused(lambda: call(-1.0, 5), who, "eps = -1 is not a distance", "+inf is allowed")
        _refused(lambda: call(float("nan"), 5), who, "eps = nan is not a distance")
        _refused(lambda: call(1.0, 0), who, "min_samples = 0 must be at least 1")
        _refused(lambda: call(1.0, -3), who, "min_samples = -3 must be at least 1")
    _refused(lambda: ctx.dbscan(d, 1.0, 2.5), "min_samples must be an integer")
    _refused(lambda: ctx.eps_degrees(t, -0.5), "po_eps_degrees_dev:", "eps = -0.5 is not a distance")
    _refused(lambda: ctx.eps_degrees(t, float("nan")), "po_eps_degrees_dev:", "eps = nan")
    _refused(lambda: ctx.dbscan(torch.as_strided(t, (n, n), (n - 1, 1)), 1.0, 5), "po_dbscan_dev:", "ld = 99 is smaller than n = 100")
    _refused(lambda: ctx.eps_degrees(torch.as_strided(t, (n, n), (n - 1, 1)), 1.0), "po_eps_degrees_dev:", "ld = 99 is smaller than n = 100")
    _refused(lambda: ctx.dbscan(d[:, :-1], 1.0, 5), "square")
    lib = _lib.load()                                                    # the library's own argument checks, past the Python layer
    labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    host_labels = np.zeros(n, dtype=np.int32)
    big = 2 ** 31
    for kw, word in ((dict(dtype=7), "dtype must be PO_F64 or PO_F32 (got 7)"), (dict(n=big, ld=big), "n = 2147483648 outside 0 .. 2^31 - 1"),
                     (dict(ld=n - 1), "ld = 99 is smaller than n = 100"), (dict(eps=-2.0), "eps = -2 is not a distance"),
                     (dict(ms=0), "min_samples = 0 must be at least 1")):
        a = dict(dtype=_lib.PO_F64, n=n, ld=n, eps=1.0, ms=5)
        a.update(kw)
        rc = lib.po_dbscan_dev(ctx._h, t.data_ptr(), a["dtype"], a["n"], a["ld"], a["eps"], a["ms"], labels.data_ptr(), None, None)
        assert rc == _lib.PO_EINVAL and ("po_dbscan_dev: " + word) in lib.po_last_error().decode(), lib.po_last_error().decode()
        rc = lib.po_dbscan(ctx._h, d.ctypes.data, a["dtype"], a["n"], a["ld"], a["eps"], a["ms"], host_labels.ctypes.data, None, None)
        assert rc == _lib.PO_EINVAL and ("po_dbscan: " + word) in lib.po_last_error().decode(), lib.po_last_error().decode()
        if "ms" not in kw:
            rc = lib.po_eps_degrees_dev(ctx._h, t.data_ptr(), a["dtype"], a["n"], a["ld"], a["eps"], labels.data_ptr())
            assert rc == _lib.PO_EINVAL and ("po_eps_degrees_dev: " + word) in lib.po_last_error().decode(), lib.po_last_error().decode()
    # n == 0 does nothing, whatever the pointers
    assert lib.po_dbscan_dev(ctx._h, None, _lib.PO_F32, 0, 0, 1.0, 5, None, None, None) == 0
    assert lib.po_dbscan(ctx._h, None, _lib.PO_F64, 0, 0, 1.0, 5, None, None, None) == 0
    assert lib.po_eps_degrees_dev(ctx._h, None, _lib.PO_F64, 0, 0, 1.0, None) == 0
    empty = ctx.dbscan(np.zeros((0, 0)), 1.0, 5, want_stats=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0,) and empty[2]["clusters"] == 0 and ctx.eps_degrees(np.zeros((0, 0)), 1.0).shape == (0,)
    got = ctx.dbscan(d, EPS, MS)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    core_less = torch.zeros(n, dtype=torch.int32, device="cuda")            # d_core may be NULL
    assert lib.po_dbscan_dev(ctx._h, t.data_ptr(), _lib.PO_F64, n, n, EPS, MS, core_less.data_ptr(), None, None) == 0
    assert np.array_equal(_np(core_less), want[0])


# ---- 4. the rounds of the component loop: a condition, not a measurement ------------------------------------------------------------
def test_a_chain_of_4096_records_takes_few_rounds(ctx, torch):
    """4 096 records at a random permutation of 0 .. 4095 on a line, eps = 1, min_samples = 2: one cluster, no noise.  Propagation
    alone needs about 2 000 rounds; with hooking and jumping the restatement of the loop needs 9 (6 at n = 256).  The bound of 32
    is a condition on the algorithm, not a measurement."""
    n = 4096
    d = dbscan_ref.line_matrix(n)
    want, want_core = dbscan_ref.dbscan(d, 1.0, 2)
    assert (want == 0).all() and want_core.all()
    t = torch.from_numpy(d).cuda()
    got = ctx.dbscan(t, 1.0, 2, want_stats=True)
    _check(got, want, want_core)
    print("passes at n = 4096: %d (restatement %d)" % (got[2]["passes"], dbscan_ref.rounds(d, 1.0, 2)))
    assert got[2]["passes"] <= 32
    assert got[2]["passes"] == dbscan_ref.rounds(d, 1.0, 2)
    small = ctx.dbscan(dbscan_ref.line_matrix(256).astype(np.float32), 1.0, 2, want_stats=True)
    assert small[2]["passes"] == dbscan_ref.rounds(dbscan_ref.line_matrix(256), 1.0, 2) <= 8 and (small[0] == 0).all()


# ---- 5. CLI ------------------------------------------------------------------------------------------------------------------------
N_SPECIES, N_SHORT = 240, 10
Q, M = 0.1, 5
_RUNS = {}


def _records():
    """240 ragged records of four species and, after every 24th, one random record of 300 - 900 bases"""
    seq, offsets = synthetic.ragged_assembly(N_SPECIES, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
    rng = np.random.default_rng(107)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for i in range(N_SPECIES):
        out.append(("c%07d" % i, seq[int(offsets[i]):int(offsets[i + 1])].tobytes()))
        if i % 24 == 23:
            out.append(("short%02d" % (i // 24), acgt[rng.integers(0, 4, size=int(rng.integers(300, 901)))].tobytes()))
    assert len(out) == N_SPECIES + N_SHORT
    return out


def _write_fasta(path, recs, width=80):
    parts = []
    for title, s in recs:
        parts.append(b">" + title.encode() + b"\n")
        parts.extend(s[p:p + width] + b"\n" for p in range(0, len(s), width))
    path.write_bytes(b"".join(parts))


def _run(*args):
    r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "--method", "joblib", "-d", "JSD"] + [str(a) for a in args], capture_output=True,
                       text=True, timeout=600, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    return r


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """the assembly, the matrix the command line writes for it as text, and eps = the Q quantile of that matrix"""
    work = tmp_path_factory.mktemp("dbscan")
    recs = _records()
    _write_fasta(work / "asm.fa", recs)
    _run("-i", work / "asm.fa", "-o", work / "matrix.txt")
    d = np.loadtxt(work / "matrix.txt")
    assert d.shape == (len(recs), len(recs))
    return {"work": work, "fa": work / "asm.fa", "recs": recs, "matrix": d, "eps": float(np.quantile(d, Q))}


def test_cli_labels_core_and_stats(asm):
    work, d, eps = asm["work"], asm["matrix"], asm["eps"]
    r = _run("-i", asm["fa"], "-o", work / "labels.txt", "--dbscan", repr(eps), "--dbscan-min-samples", M, "--dbscan-core", work / "core.txt",
             "--json-stats", work / "stats.json")
    assert r.stdout.splitlines()[-1] == "Writing cluster labels"
    want, want_core = dbscan_ref.dbscan(d, eps, M)
    text = (work / "labels.txt").read_text()
    assert text == "".join("%d\n" % x for x in want)
    assert want.max() >= 1 and (want < 0).any() and "-1\n" in text        # at least two clusters, at least one contig in none
    assert (work / "core.txt").read_text() == "".join("1\n" if x else "0\n" for x in want_core)
    short = np.array([title.startswith("short") for title, _ in asm["recs"]])
    assert (want[short] == -1).all()                                      # the random short records belong nowhere
    st = json.load(open(work / "stats.json"))
    degree = dbscan_ref.degrees(d, eps)
    assert (st["dbscan_eps"], st["dbscan_min_samples"], st["dbscan_dtype"]) == (eps, M, "float64")
    assert (st["dbscan_clusters"], st["dbscan_core"], st["dbscan_noise"]) == (int(want.max()) + 1, int(want_core.sum()), int((want < 0).sum()))
    assert st["dbscan_border"] == int(((want >= 0) & ~want_core).sum()) and st["dbscan_sizes"] == np.bincount(want[want >= 0]).tolist()
    assert st["dbscan_passes"] == dbscan_ref.rounds(d, eps, M) and st["contigs"] == d.shape[0]
    assert (st["dbscan_degree_min"], st["dbscan_degree_median"], st["dbscan_degree_max"]) == (int(degree.min()), float(np.median(degree)), int(degree.max()))
    assert st["dbscan_ms"] > 0 and sorted(st["dbscan_phases_ms"]) == ["degree", "finish", "label"] and st["dbscan_phases_ms"]["degree"] > 0


def test_cli_clipped_run_equals_run_on_kept_records(asm, tmp_path):
    eps, L = asm["eps"], 1000
    opts = ["--dbscan", repr(eps), "--dbscan-min-samples", M, "--dbscan-dtype", "float32"]
    _run("-i", asm["fa"], "-o", tmp_path / "l1.txt", *opts, "--dbscan-core", tmp_path / "c1.txt", "--clip-percentile", "0.9", "--min-size", L,
         "--clip-out", tmp_path / "kept.tsv", "--json-stats", tmp_path / "s1.json")
    idx = [int(line.split("\t")[0]) for line in open(tmp_path / "kept.tsv").read().splitlines()]
    lengths = np.array([len(s) for _, s in asm["recs"]])
    st = json.load(open(tmp_path / "s1.json"))
    assert st["clip_dtype"] == "float32" and st["dbscan_dtype"] == "float32" and st["clip_kept"] == len(idx) == st["contigs"]
    assert 0 < len(idx) < len(asm["recs"]) and lengths[idx].min() >= L and st["clip_dropped_by_median"] > 0
    _write_fasta(tmp_path / "kept.fa", [asm["recs"][i] for i in idx])
    _run("-i", tmp_path / "kept.fa", "-o", tmp_path / "l2.txt", *opts, "--dbscan-core", tmp_path / "c2.txt")
    l1 = (tmp_path / "l1.txt").read_bytes()
    assert l1.count(b"\n") == len(idx) and l1 == (tmp_path / "l2.txt").read_bytes()
    assert (tmp_path / "c1.txt").read_bytes() == (tmp_path / "c2.txt").read_bytes()
