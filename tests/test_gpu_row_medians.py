"""Row medians on the GPU (po_row_medians_dev, Context.row_medians): exact against numpy.median(m.astype(float64), axis=1) -
a median is an element of the row or the mean of two, so every comparison is for equality, NaN rows by position."""
import os
import warnings

import numpy as np
import pytest

import phyloligo_amd as pa
from phyloligo_amd import _lib, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def ctx():
    with pa.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _oracle(m):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (inf - inf and NaN rows warn)
        with np.errstate(all="ignore"):
            return np.median(np.asarray(m).astype(np.float64), axis=1)


def _same(got, want):
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (np.flatnonzero(np.isnan(got)), np.flatnonzero(np.isnan(want)))
    bad = np.flatnonzero(~((got == want) | np.isnan(want)))
    assert bad.size == 0, "rows %r: got %r, want %r" % (bad[:8], got[bad[:8]], want[bad[:8]])


def _check_both(ctx, torch, m):
    """numpy in and torch in, both against the oracle"""
    want = _oracle(m)
    _same(ctx.row_medians(m), want)
    t = ctx.row_medians(torch.from_numpy(np.ascontiguousarray(m)).cuda())
    assert t.is_cuda and t.dtype == torch.float64
    _same(t.cpu().numpy(), want)
    return want


def _rand_matrix(n, dtype, seed=0):
    rng = np.random.RandomState(seed)
    m = rng.rand(n, n)
    m = (m + m.T) * 0.5
    np.fill_diagonal(m, 0.0)
    return m.astype(dtype)


# ---- 1. sizes: odd / even, below / at / above the wave and the workgroup, the partial last vector group ---------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_sizes(ctx, torch, n, dtype):
    _check_both(ctx, torch, _rand_matrix(n, dtype, seed=n))


# ---- 2. layouts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts_give_the_same_bytes(ctx, torch, dtype):
    n = 257
    m = _rand_matrix(n, dtype, seed=5)
    want = _oracle(m)
    flat = ctx.row_medians(torch.from_numpy(m).cuda()).cpu().numpy()
    _same(flat, want)
    # misaligned base, ld > n
    big = torch.zeros((n + 3, n + 3), dtype=torch.from_numpy(m).dtype, device="cuda")
    big[1:n + 1, 1:n + 1] = torch.from_numpy(m).cuda()
    view = big[1:n + 1, 1:n + 1]
    assert view.data_ptr() % 16 != 0 and view.stride(0) == n + 3
    assert ctx.row_medians(view).cpu().numpy().tobytes() == flat.tobytes()
    nbig = np.zeros((n + 3, n + 3), dtype=dtype)
    nbig[1:n + 1, 1:n + 1] = m
    assert ctx.row_medians(nbig[1:n + 1, 1:n + 1]).tobytes() == flat.tobytes()
    # rows on whole 128-byte lines
    per = 128 // m.itemsize
    ld = (n + per - 1) // per * per
    pad = torch.full((n, ld), 7.0, dtype=big.dtype, device="cuda")
    pad[:, :n] = torch.from_numpy(m).cuda()
    assert pad[:, :n].data_ptr() % 16 == 0 and pad[:, :n].stride(0) == ld
    assert ctx.row_medians(pad[:, :n]).cpu().numpy().tobytes() == flat.tobytes()
    # a non-square panel, alone and as rows of a wider buffer
    rng = np.random.RandomState(11)
    panel = rng.rand(5, 1000).astype(dtype)
    got = _check_both(ctx, torch, panel)
    wide = torch.zeros((5, 1003), dtype=big.dtype, device="cuda")
    wide[:, 2:1002] = torch.from_numpy(panel).cuda()
    assert ctx.row_medians(wide[:, 2:1002]).cpu().numpy().tobytes() == got.tobytes()
    one = ctx.row_medians(torch.from_numpy(panel[3:4]).cuda())
    assert one.shape == (1,) and one.cpu().numpy()[0] == got[3]


# ---- 3. adversarial rows ------------------------------------------------------------------------------------------------------------
def _adversarial(n, dtype, seed=3):
    rng = np.random.RandomState(seed)
    T = dtype
    rows = []

    def put(values):
        v = np.asarray(values, dtype=T)
        assert v.shape == (n,)
        rows.append(v[rng.permutation(n)])

    put(np.full(n, 0.25))                                                           # all equal
    put([0.25] * (n // 2) + [0.75] * (n - n // 2))                                   # two values split at the middle
    put([0.25] * (n // 2 + 1) + [0.75] * (n - n // 2 - 1))                           # ... and one off it
    put([0.25] * (n // 2 - 1) + [0.75] * (n - n // 2 + 1))
    below = np.nextafter(T(0.5), T(0))                                              # the middle pair straddles an exponent boundary
    lows = (n - 1) // 2
    put(np.concatenate([rng.rand(lows) * 0.49, [below, T(0.5)], 0.51 + rng.rand(n - lows - 2) * 0.49]))
    lows = (n - 100) // 2                                                           # the middle inside 100 duplicates
    put(np.concatenate([rng.rand(lows) * 0.49, [0.5] * 100, 0.51 + rng.rand(n - lows - 100) * 0.49]))
    ulp = 2.0 ** -52 if T is np.float64 else 2.0 ** -24                             # decided in the lowest bits
    put(0.5 + np.arange(n) * ulp)
    if T is np.float64:                                                             # 600 binary orders of magnitude, subnormals included
        wide = np.ldexp(0.5 + rng.rand(n) * 0.5, rng.randint(-1074, -474, size=n)) * rng.choice([-1.0, 1.0], size=n)
    else:                                                                           # every finite float32
        wide = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
        wide[~np.isfinite(wide)] = 0.0
    put(wide)
    lows = n // 2 - 2                                                               # zeros of both signs at the median rank
    put(np.concatenate([-1.0 - rng.rand(lows), [-0.0, -0.0, 0.0, -0.0], 1.0 + rng.rand(n - lows - 4)]))
    put(np.concatenate([rng.rand(n - n // 2), [np.inf] * (n // 2)]))                 # half +inf
    put(np.concatenate([rng.rand(n // 2), [np.inf] * (n - n // 2)]))
    put(np.concatenate([[-np.inf] * 3, rng.rand(n - 6), [np.inf] * 3]))
    put(np.concatenate([rng.rand(n - 1), [np.nan]]))                                 # one NaN, all NaN
    put(np.full(n, np.nan))
    put(rng.rand(n))
    put(-rng.rand(n) * 1e-30)
    return np.stack(rows)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1024, 1025])
def test_adversarial_rows(ctx, torch, n, dtype):
    m = _adversarial(n, dtype)
    want = _check_both(ctx, torch, m)
    assert np.isnan(want[-4]) and np.isnan(want[-3]) and int(np.isnan(want).sum()) == 2
    assert want[0] == 0.25 and want[8] == 0.0


# ---- 4. a real matrix ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def profiles(ctx, torch):
    seq, offsets = synthetic.ragged_assembly(600, seed=7, median=3000, lo=1000, hi=20000)
    counts, totals = ctx.count_profiles(seq, offsets, "1111", "both")
    return (torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(totals.view(np.int64)).cuda())


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("metric", ["JSD", "Eucl"])
def test_real_matrix(ctx, profiles, metric, dtype):
    d = ctx.pairwise(profiles[0], profiles[1], metric, dtype=dtype)
    got = ctx.row_medians(d)
    host = d.cpu().numpy()
    want = _oracle(host)
    _same(got.cpu().numpy(), want)
    _same(ctx.row_medians(host), want)


# ---- 5. rows longer than one LDS-full: several passes over memory ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_rows(ctx, torch, dtype):
    n, rows = 20001, 64
    rng = np.random.RandomState(21)
    m = rng.rand(rows, n).astype(dtype)
    ulp = 2.0 ** -52 if dtype is np.float64 else 2.0 ** -24
    m[5] = (0.5 + np.arange(n) * ulp)[rng.permutation(n)].astype(dtype)
    m[6, ::2] = 0.125                                                              # duplicates across the middle
    m[7] = np.where(np.arange(n) < n // 2, m[7] * 0.25, np.inf)
    t = torch.from_numpy(m).cuda()
    want = _oracle(m)
    got = ctx.row_medians(t).cpu().numpy()
    _same(got, want)
    passes = ctx.row_medians_passes()
    assert rows * 2 <= passes <= rows * 7, passes                                  # at least a histogram and a collect, at most 7 reads
    # even n, the same rows: the two middle elements
    _same(ctx.row_medians(t[:, :n - 1]).cpu().numpy(), _oracle(m[:, :n - 1]))


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes(ctx, torch):
    t = torch.from_numpy(_rand_matrix(1025, np.float64, seed=9)).cuda()
    a = ctx.row_medians(t).cpu().numpy()
    b = ctx.row_medians(t).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    assert ctx.row_medians_passes() == 1025                                         # 1 025 columns fit LDS: every row is read once


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def _refused(call, *words):
    with pytest.raises(_lib.PhyloligoError) as e:
        call()
    assert e.value.status == _lib.PO_EINVAL
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(ctx, torch):
    t = torch.from_numpy(_rand_matrix(64, np.float64)).cuda()
    _refused(lambda: ctx.row_medians(t.as_strided((4, 64), (32, 1))), "ld = 32", "n = 64")
    _refused(lambda: ctx.row_medians(t.half()), "float32 / float64")
    _refused(lambda: ctx.row_medians(t.to(torch.int32)), "float32 / float64")
    _refused(lambda: ctx.row_medians(t[0]), "2-D")
    _refused(lambda: ctx.row_medians(t.reshape(4, 16, 64)), "2-D")
    _refused(lambda: ctx.row_medians(np.zeros((2, 3, 4))), "2-D")
    _refused(lambda: ctx.row_medians(t.cpu()), "cuda:0")
    _refused(lambda: ctx.row_medians(t.t()), "unit inner stride")
    lib = _lib.load()
    out = torch.zeros(64, dtype=torch.float64, device="cuda")
    for dtype, rows, n, ld, word in ((7, 64, 64, 64, "dtype"), (_lib.PO_F64, 64, 64, 63, "ld = 63"), (_lib.PO_F64, 1, 2 ** 31, 2 ** 31, "2^31")):
        rc = lib.po_row_medians_dev(ctx._h, t.data_ptr(), dtype, rows, n, ld, out.data_ptr())
        assert rc == _lib.PO_EINVAL and word in lib.po_last_error().decode(), lib.po_last_error().decode()
    # nothing to do is not an error, and the context still works
    assert lib.po_row_medians_dev(ctx._h, t.data_ptr(), _lib.PO_F64, 0, 64, 64, out.data_ptr()) == 0
    assert lib.po_row_medians_dev(ctx._h, t.data_ptr(), _lib.PO_F64, 64, 0, 64, out.data_ptr()) == 0
    assert ctx.row_medians(np.zeros((0, 5))).shape == (0,)
    _same(ctx.row_medians(t).cpu().numpy(), _oracle(t.cpu().numpy()))
