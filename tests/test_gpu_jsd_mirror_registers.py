"""JSD table kernel, mirrored tile of a float64 matrix transposed in registers (csrc/po_jsd_lut.hip): interior tiles store their
transpose straight from registers, edge tiles, float32 matrices and misaligned targets keep the LDS path.  Equal-total count
matrices, so that the table kernel owns every tile; sizes chosen so that interior mirrored tiles lie next to edge tiles
(n = 256, 384, 300) or do not occur at all (n = 130).  Needs an MI355X."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-6      # the general-kernel tolerance of tests/test_gpu_parity.py
ATOL = 1e-12
SIZES = [256, 384, 300, 130]
WIDTHS = [8, 136, 256]
PO_KERNEL_VALU_JSD = 1


@pytest.fixture(scope="module")
def ctx():
    import phyloligo_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def equal_total_counts(n, width, wide):
    """n records of `width` words with one common total; the largest count is exactly 127 (narrow table layout) or 255 (wide)"""
    rng = np.random.default_rng(1000 * n + 10 * width + int(wide))
    counts = rng.multinomial(30 * width, np.full(width, 1.0 / width), size=n).astype(np.int64)
    top = 255 if wide else 127
    assert counts.max() < top
    counts[:, 0] += top - counts[:, 0].max()          # the same shift for every record: totals stay equal
    assert counts.max() == top and counts.min() >= 0 and len(set(counts.sum(1).tolist())) == 1
    return counts.astype(np.uint32), counts.sum(1).astype(np.uint64)


def device_counts(n, width, wide):
    import torch
    counts, totals = equal_total_counts(n, width, wide)
    return torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(totals.view(np.int64)).cuda()


_full = {}


def full_matrix(ctx, n, width, wide, dtype="float64"):
    """the whole matrix through the table kernel, computed once per case and shared (never modified)"""
    key = (n, width, wide, dtype)
    if key not in _full:
        dc, dt = device_counts(n, width, wide)
        m, st = ctx.pairwise(dc, dt, "JSD", dtype=dtype, want_stats=True)
        assert st["kernel_id"] != PO_KERNEL_VALU_JSD
        _full[key] = m.cpu().numpy()
    return _full[key]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("wide", [False, True], ids=["max127", "max255"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_symmetric_and_equal_to_general_kernel(ctx, n, width, wide, dtype):
    got = full_matrix(ctx, n, width, wide, dtype)
    assert got.shape == (n, n) and got.dtype == np.dtype(dtype)
    assert np.array_equal(got, got.T)                                 # one value, stored twice
    assert np.array_equal(np.diag(got), np.zeros(n, dtype=got.dtype))
    dc, dt = device_counts(n, width, wide)
    gen, st = ctx.pairwise(dc, dt, "JSD", dtype=dtype, table_path=False, want_stats=True)
    assert st["kernel_id"] == PO_KERNEL_VALU_JSD
    np.testing.assert_allclose(got, gen.cpu().numpy(), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_row_range(ctx, dtype):
    """rows 128 .. 256 of n = 384: one tile row of the block, its tiles left and right of the diagonal"""
    n, width = 384, 136
    dc, dt = device_counts(n, width, False)
    got = ctx.pairwise(dc, dt, "JSD", row_begin=128, row_end=256, dtype=dtype).cpu().numpy()
    assert np.array_equal(got, full_matrix(ctx, n, width, False, dtype)[128:256])


@pytest.mark.parametrize("wide", [False, True], ids=["max127", "max255"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_rectangular_blocks_with_mirror_buffers(ctx, dtype, wide):
    """The work lists of 2 virtual ranks: rectangular blocks whose transpose goes to a buffer of its own.  Every mirror buffer
    equals its transposed block bit for bit, and the assembled matrix is the single-call matrix."""
    import torch
    from phyloligo_amd.dist import RowBlockPlan, assemble_virtual
    n, width = 512, 136
    dc, dt = device_counts(n, width, wide)
    tdtype = torch.float64 if dtype == "float64" else torch.float32
    plan = RowBlockPlan(n, 2)
    slabs, mirrors, rect = [], [], 0
    for g in range(2):
        slab, mir = plan.allocate(g, dc.device, tdtype)
        slab.fill_(float("nan"))
        for m in mir:
            if m is not None:
                m.fill_(float("nan"))
        plan.compute(ctx, dc, dt, "JSD", g, slab, mir)
        lo, _ = plan.rows(g)
        for ((r0, r1), (c0, c1), kind, peer), m in zip(plan.work(g), mir):
            if kind != "diag":
                assert torch.equal(m, slab[r0 - lo:r1 - lo, c0:c1].T)
                rect += 1
        slabs.append(slab)
        mirrors.append(mir)
    assert rect == 2
    got = assemble_virtual(plan, slabs, mirrors).cpu().numpy()
    assert np.array_equal(got, full_matrix(ctx, n, width, wide, dtype))


@pytest.mark.parametrize("how", ["odd_leading_dimension", "pointer_off_by_one_element"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_misaligned_targets_take_the_old_path(ctx, dtype, how):
    """a target whose rows are not 16-byte (float64) / 8-byte (float32) aligned fails the interior test: the same values"""
    import torch
    n, width = 384, 136
    dc, dt = device_counts(n, width, False)
    tdtype = torch.float64 if dtype == "float64" else torch.float32
    if how == "odd_leading_dimension":
        out = torch.full((n, n + 1), -7.0, dtype=tdtype, device=dc.device)[:, :n]
    else:
        out = torch.full((n * n + 2,), -7.0, dtype=tdtype, device=dc.device)[1:1 + n * n].view(n, n)
        assert out.data_ptr() % (2 * out.element_size()) != 0
    ctx.pairwise(dc, dt, "JSD", dtype=dtype, out=out)
    assert np.array_equal(out.cpu().numpy(), full_matrix(ctx, n, width, False, dtype))
