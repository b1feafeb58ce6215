"""The word loop of jsd_lut_rows_kernel (csrc/po_jsd_lut.hip) feeds its lookups from a ring of column terms that is refilled
behind the words that consumed it, takes the table at LDS address 0 and loads the column terms from a uniform base plus a lane
offset.  The shapes here are the smallest at which that can go wrong: every peeled / clamped round and the doubling point on
its own, edge-only and interior-only grids, a misaligned row range, both table layouts, both output types, counts that make a
stale ring slot visible, and a block of another class among equal ones.  Every case is checked against the general kernel
(table_path=False) and the oracle with the tolerances of test_gpu_edge_cases.py::test_jsd_table_kernel_widths_not_multiple_of_four."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import phyloligo_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def rc_index(dim):
    k = int(round(np.log(dim) / np.log(4)))
    x = np.arange(dim)
    r = np.zeros(dim, dtype=np.int64)
    for _ in range(k):
        r = (r << 2) | ((x & 3) ^ 1)
        x = x >> 2
    return r


def plain_records(n, dim, total, seed):
    """n records of `dim` words that all sum to `total` (no count above it)"""
    rng = np.random.default_rng(seed)
    return rng.multinomial(total, rng.dirichlet(np.ones(dim) * 0.7), size=n).astype(np.uint32)


def strand_symmetric_records(n, dim, total, seed):
    """count[w] == count[rc(w)] for every record, every record sums to `total` (even): what reverse-complement folding needs"""
    rng = np.random.default_rng(seed)
    rc = rc_index(dim)
    rep = np.flatnonzero(np.arange(dim) <= rc)                   # one word per orbit, self-paired words included
    units = rng.multinomial(total // 2, rng.dirichlet(np.ones(len(rep)) * 0.7), size=n)
    counts = np.zeros((n, dim), dtype=np.int64)
    counts[:, rep] += units                                      # a unit is one count on w and one on rc(w):
    np.add.at(counts, (slice(None), rc[rep]), units)             # two on a word that is its own reverse complement
    assert np.array_equal(counts, counts[:, rc])
    return counts.astype(np.uint32)


def ring_records(n):
    """word w of record j holds (7 w + 3 j) mod 97 for the first 16 words: consecutive words of one column differ strongly, and
    so do the columns of one word; eight more words bring every record to the same total"""
    w, j = np.arange(16)[None, :], np.arange(n)[:, None]
    head = (7 * w + 3 * j) % 97
    rest = head.sum(axis=1).max() - head.sum(axis=1)
    tail = rest[:, None] // 8 + (np.arange(8)[None, :] < (rest % 8)[:, None])
    return np.concatenate([head, tail], axis=1).astype(np.uint32)


def check(ctx, counts, want_folded=None, **kw):
    """table kernel against the general kernel and the oracle; float32 output against the rounded float64 one"""
    from oracle import phyloligo_oracle as po
    n = counts.shape[0]
    totals = counts.sum(axis=1).astype(np.uint64)
    got, st = ctx.pairwise(counts, totals, "JSD", want_stats=True, **kw)
    assert st["kernel_id"] == 6                                  # the table kernel took part
    if want_folded is not None:
        assert bool(st["rc_folded"]) == want_folded
    gen, st2 = ctx.pairwise(counts, totals, "JSD", table_path=False, want_stats=True, **kw)
    assert st2["kernel_id"] == 1
    np.testing.assert_allclose(got, gen, rtol=1e-9, atol=1e-13)
    want = po.pairwise_block(po.counts_to_frequencies(counts.astype(np.int64), totals), "JSD")
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-12)
    assert got.shape == (n, n) and np.array_equal(got, got.T) and np.all(np.diag(got) == 0.0)
    got32 = ctx.pairwise(counts, totals, "JSD", dtype="float32", **kw)
    np.testing.assert_array_equal(got32, got.astype(np.float32))
    return got, want


# rounds of four words over the width padded to 8; the last two rounds clamp their operand pointers.  1, 4, 5, 8: clamped rounds
# only; 9, 12, 16: the first widths with unclamped rounds in front (two); 20, 24: four.  (rc_fold=False: 4 and 16 would fold.)
@pytest.mark.parametrize("dim", [1, 4, 5, 8, 9, 12, 16, 20, 24])
def test_widths_around_the_peeled_rounds(ctx, dim):
    counts = plain_records(257, dim, 96, 2000 + dim)
    counts[7] = counts[3]                                        # a duplicate pair
    assert counts.max() <= 127
    got, _ = check(ctx, counts, rc_fold=False)
    assert got[3, 7] < 1e-13


# (dim, folded width, word at which the sums double): 16 -> 8 + 8, doubling inside the clamped rounds; 64 -> 32 + 0, doubling
# behind the last word (dbl_at == dim8); 256 -> 120 + 16, the benchmark's shape
@pytest.mark.parametrize("dim", [16, 64, 256])
def test_folded_widths_and_doubling_points(ctx, dim):
    counts = strand_symmetric_records(257, dim, 96, 3000 + dim)
    assert counts.max() <= 127
    check(ctx, counts, want_folded=True)


def test_full_width_without_folding(ctx):
    counts = strand_symmetric_records(257, 256, 96, 3300)
    check(ctx, counts, want_folded=False, rc_fold=False)         # 256 words, no doubling


# 129: no tile is interior (the second block holds one record); 257: interior and edge tiles; 384: every tile interior, with
# diagonal and mirrored ones
@pytest.mark.parametrize("n", [129, 257, 384])
def test_record_counts_edge_and_interior_tiles(ctx, n):
    check(ctx, strand_symmetric_records(n, 256, 96, 4000 + n), want_folded=True)


def test_misaligned_row_range_takes_the_bounds_tested_path(ctx):
    from oracle import phyloligo_oracle as po
    counts = strand_symmetric_records(384, 256, 96, 4500)
    totals = counts.sum(axis=1).astype(np.uint64)
    want = po.pairwise_block(po.counts_to_frequencies(counts.astype(np.int64), totals), "JSD")
    for dtype in ("float64", "float32"):
        part, st = ctx.pairwise(counts, totals, "JSD", row_begin=1, row_end=383, dtype=dtype, want_stats=True)
        assert st["kernel_id"] == 6 and part.shape == (382, 384)
        gen = ctx.pairwise(counts, totals, "JSD", row_begin=1, row_end=383, dtype=dtype, table_path=False)
        if dtype == "float64":
            np.testing.assert_allclose(part, gen, rtol=1e-9, atol=1e-13)
            np.testing.assert_allclose(part, want[1:383], rtol=1e-6, atol=1e-12)
            part64 = part
        else:
            np.testing.assert_array_equal(part, part64.astype(np.float32))


@pytest.mark.parametrize("dim,fold", [(20, False), (256, True)])
def test_counts_above_127_take_the_wide_layout(ctx, dim, fold):
    counts = (strand_symmetric_records if fold else plain_records)(257, dim, 250, 5000 + dim)
    counts[0] = 0
    counts[0, np.flatnonzero(rc_index(256) == np.arange(256))[0] if fold else 0] = 250   # (a word that is its own reverse complement)
    assert 127 < counts.max() <= 255
    check(ctx, counts, want_folded=fold)


def test_ring_slots_are_consumed_in_order(ctx):
    """a ring slot that is read before its refill has landed, or after the next one, shows up as another word's counts: with
    these counts that moves many entries by far more than the tolerance"""
    counts = ring_records(257)
    assert counts.max() <= 127 and len(set(counts.sum(axis=1).tolist())) == 1
    assert np.abs(np.diff(counts[:, :16].astype(np.int64), axis=1)).min() >= 7
    check(ctx, counts)


def test_one_block_of_another_total_among_equal_ones(ctx):
    counts = strand_symmetric_records(384, 256, 96, 6000)
    counts[128:256] = strand_symmetric_records(128, 256, 80, 6001)
    check(ctx, counts, want_folded=True)                         # tiles (0,1) and (1,2) belong to the general kernel
