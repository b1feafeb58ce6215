#!/usr/bin/env python3
"""Record what the C entry points of the host layer refuse, and with which words: tests/golden/api_refusals.json.

Run from the repository root on a GPU (python tests/golden/make_golden_api_refusals.py), against the library built from the
commit whose behaviour is to be kept.  Every case calls one raw ctypes entry point (_lib.load()) with one argument set and
records (status, po_last_error() text when the status is not PO_OK, whether the call's out-struct - po_stats, po_tsne_result or
*nnz, filled with a pattern before the call - came back all zero, null when the call has none).  The file holds the table of
distinct outcomes and one index into it per case.  tests/test_gpu_api_refusals.py replays it.

An entry point is described once by a call that succeeds (SPECS: n <= 8, dim = 4; n = 130 where a rule about multiples of 128
needs it) and by named changes to that call: `faults` are refused, `empty` are accepted and do nothing.  Recorded are the good
call, every change alone, and every two faults that change different arguments together - the second pins which message comes
first.  Every pointer that is not NULL is a real allocation that fits the good call, so a check that went missing shows as
another status, never as a stray access.  (n >= 2^31 cannot be had that way: those rules are checked by reading.)
"""
import ctypes
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "api_refusals.json")

N, DIM, K = 8, 4, 3
N128 = 130            # two blocks of 128 records
TSNE_K, PERPLEXITY = 7, 2.0          # min(n - 1, int(3 * 2 + 1)) = 7 neighbours on 8 points
PATTERN = 0xAB


class Misaligned:
    """the address of a device buffer plus one byte"""
    def __init__(self, buf):
        self.buf = buf


def _block(r0, r1, c0, c1, out=None, ld_out=0, mirror=None, ld_mirror=0, triangular=0):
    return dict(row_begin=r0, row_end=r1, col_begin=c0, col_end=c1, out=out, ld_out=ld_out, mirror=mirror, ld_mirror=ld_mirror,
                triangular=triangular)


def build_specs(torch, ctx):
    """[(entry point, out-struct kind or None, [(argument, value)], faults, empty)]"""
    rng = np.random.default_rng(20261019)
    keep = []

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        keep.append(t)
        return t

    def room(nbytes):
        t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        keep.append(t)
        return t

    def host(a):
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a

    counts = rng.integers(1, 20, size=(N, DIM)).astype(np.uint32)
    totals = counts.sum(axis=1).astype(np.uint64)
    freq = counts / totals[:, None].astype(np.float64)
    proto = np.full(DIM, 1.0 / DIM)
    counts128 = rng.integers(1, 20, size=(N128, DIM)).astype(np.uint32)
    totals128 = counts128.sum(axis=1).astype(np.uint64)
    seq = np.frombuffer(b"ACGT" * 16 + b"\0" * 256, dtype=np.uint8).copy()      # 64 bases and the slack a reader may take
    offsets = np.array([0, 32, 64], dtype=np.uint64)
    begins, ends = offsets[:2].copy(), offsets[1:].copy()
    u64 = lambda *v: np.array(v, dtype=np.uint64)                                   # noqa: E731
    specs = []

    # ---- context and pattern -------------------------------------------------------------------------------------------
    name_buf = ctypes.create_string_buffer(64)
    keep.append(name_buf)
    specs.append(("po_ctx_create", None, [("out", None), ("device", 0)], {"out_null": {}}, {}))      # (no good call: it would leak a context)
    for fn in ("po_ctx_trim", "po_ctx_synchronize"):
        specs.append((fn, None, [("ctx", ctx)], {"ctx_null": {"ctx": None}}, {}))
    specs.append(("po_ctx_set_stream", None, [("ctx", ctx), ("stream", None)], {"ctx_null": {"ctx": None}}, {}))
    specs.append(("po_ctx_device_name", None, [("ctx", ctx), ("buf", name_buf), ("len", 64)],
                  {"ctx_null": {"ctx": None}, "buf_null": {"buf": None}, "len_0": {"len": 0}}, {}))
    window, kk, dim64 = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    bad_patterns = {"pattern_null": {"pattern": None}, "pattern_empty": {"pattern": b""}, "pattern_letters": {"pattern": b"1x1"},
                    "pattern_long": {"pattern": b"1" + b"0" * 64}, "pattern_no_ones": {"pattern": b"0000"},
                    "pattern_nine_ones": {"pattern": b"1" * 9}}
    specs.append(("po_pattern_info", None,
                  [("pattern", b"1101"), ("window", ctypes.pointer(window)), ("k", ctypes.pointer(kk)), ("dim", ctypes.pointer(dim64))],
                  bad_patterns, {"outs_null": {"window": None, "k": None, "dim": None}}))

    # ---- stage 1 and windows -------------------------------------------------------------------------------------------
    d_seq, d_off, d_beg, d_end = dev(seq), dev(offsets), dev(begins), dev(ends)
    stage1 = dict(bad_patterns, ctx_null={"ctx": None}, strand_3={"strand": 3}, strand_negative={"strand": -1})
    specs.append(("po_count_profiles_dev", None,
                  [("ctx", ctx), ("d_seq", d_seq), ("d_offsets", d_off), ("n_seqs", 2), ("total_bytes", 64), ("pattern", b"11"),
                   ("strand", 0), ("d_counts", room(2 * 16 * 4)), ("d_totals", room(2 * 8))],
                  dict(stage1, seq_null={"d_seq": None}, seq_misaligned={"d_seq": Misaligned(d_seq)}, offsets_null={"d_offsets": None},
                       counts_null={"d_counts": None}, totals_null={"d_totals": None}),
                  {"n_0": {"n_seqs": 0}, "n_0_all_null": {"n_seqs": 0, "d_seq": None, "d_offsets": None, "d_counts": None, "d_totals": None}}))
    specs.append(("po_count_profiles", None,
                  [("ctx", ctx), ("seq", host(seq)), ("offsets", host(offsets)), ("n_seqs", 2), ("pattern", b"11"), ("strand", 0),
                   ("counts", host(np.zeros((2, 16), np.uint32))), ("totals", host(np.zeros(2, np.uint64)))],
                  dict(stage1, seq_null={"seq": None}, offsets_null={"offsets": None}, counts_null={"counts": None},
                       totals_null={"totals": None}, offsets_start_at_1={"offsets": host(u64(1, 32, 64))},
                       offsets_decrease={"offsets": host(u64(0, 40, 32))}),
                  {"n_0": {"n_seqs": 0}}))
    specs.append(("po_count_profiles_ranges_dev", None,
                  [("ctx", ctx), ("d_seq", d_seq), ("total_bytes", 64), ("d_begins", d_beg), ("d_ends", d_end), ("n_ranges", 2),
                   ("sum_lengths", 64), ("pattern", b"11"), ("strand", 0), ("d_counts", room(2 * 16 * 4)), ("d_totals", room(2 * 8))],
                  dict(stage1, seq_null={"d_seq": None}, seq_misaligned={"d_seq": Misaligned(d_seq)}, begins_null={"d_begins": None},
                       ends_null={"d_ends": None}, counts_null={"d_counts": None}, totals_null={"d_totals": None}),
                  {"n_0": {"n_ranges": 0}}))
    specs.append(("po_count_profiles_ranges", None,
                  [("ctx", ctx), ("seq", host(seq)), ("total_bytes", 64), ("begins", host(begins)), ("ends", host(ends)), ("n_ranges", 2),
                   ("pattern", b"11"), ("strand", 0), ("counts", host(np.zeros((2, 16), np.uint32))), ("totals", host(np.zeros(2, np.uint64)))],
                  dict(stage1, seq_null={"seq": None}, begins_null={"begins": None}, ends_null={"ends": None}, counts_null={"counts": None},
                       totals_null={"totals": None}, range_past_the_end={"ends": host(u64(32, 65))},
                       range_reversed={"begins": host(u64(0, 65))}),
                  {"n_0": {"n_ranges": 0}}))
    specs.append(("po_count_byte_ranges_dev", None,
                  [("ctx", ctx), ("d_seq", d_seq), ("total_bytes", 64), ("d_begins", d_beg), ("d_ends", d_end), ("n_ranges", 2),
                   ("byte", 67), ("d_out", room(2 * 8))],
                  {"ctx_null": {"ctx": None}, "seq_null": {"d_seq": None}, "seq_misaligned": {"d_seq": Misaligned(d_seq)},
                   "begins_null": {"d_begins": None}, "ends_null": {"d_ends": None}, "out_null": {"d_out": None}, "byte_256": {"byte": 256},
                   "byte_negative": {"byte": -1}},
                  {"n_0": {"n_ranges": 0}}))

    def profile_faults(c, t, f=None):
        out = {"ctx_null": {"ctx": None}, "counts_null": {c: None}, "totals_null": {t: None}, "dim_0": {"dim": 0}}
        if f:
            out["out_null"] = {f: None}
        return out

    for fn, mk, pre in (("po_frequencies_dev", dev, "d_"), ("po_frequencies", host, "")):
        out = room(N * DIM * 8) if mk is dev else host(np.zeros((N, DIM)))
        specs.append((fn, None, [("ctx", ctx), (pre + "counts", mk(counts)), (pre + "totals", mk(totals)), ("n", N), ("dim", DIM), (pre + "freq", out)],
                      profile_faults(pre + "counts", pre + "totals", pre + "freq"), {"n_0": {"n": 0}}))
    for fn, mk, pre in (("po_profile_distances_dev", dev, "d_"), ("po_profile_distances", host, "")):
        out = room(N * 8) if mk is dev else host(np.zeros(N))
        specs.append((fn, None,
                      [("ctx", ctx), (pre + "counts", mk(counts)), (pre + "totals", mk(totals)), ("n", N), ("dim", DIM), (pre + "proto", mk(proto)),
                       ("metric", 1), (pre + "out", out)],
                      dict(profile_faults(pre + "counts", pre + "totals", pre + "out"), proto_null={pre + "proto": None}, metric_negative={"metric": -1},
                           metric_kt={"metric": 2}, metric_6={"metric": 6}),
                      {"n_0": {"n": 0}, "metric_kl": {"metric": 5}}))

    # ---- stage 2 -------------------------------------------------------------------------------------------------------
    stats = ("stats", "stats")
    common = {"ctx_null": {"ctx": None}, "metric_negative": {"metric": -1}, "metric_5": {"metric": 5}, "dim_0": {"dim": 0}}
    specs.append(("po_pairwise_reserve", None, [("ctx", ctx), ("n", N), ("dim", DIM), ("metric", 1)],
                  {"ctx_null": {"ctx": None}, "metric_negative": {"metric": -1}, "metric_5": {"metric": 5}}, {"n_0": {"n": 0}}))
    rows = dict(common, dtype_2={"out_dtype": 2}, rows_past_n={"row_end": N + 1}, rows_reversed={"row_begin": 5, "row_end": 4},
                ld_out_short={"ld_out": N - 1})
    rows_empty = {"n_0": {"n": 0, "row_end": 0}, "rows_empty": {"row_begin": 3, "row_end": 3}, "stats_null": {"stats": None},
                  "rows_empty_all_null": {"row_begin": 3, "row_end": 3, "out": None}}
    for fn, mk in (("po_pairwise_dev", dev), ("po_pairwise", host)):
        out = room(N * 32 * 8) if mk is dev else host(np.zeros((N, N)))
        specs.append((fn, "stats",
                      [("ctx", ctx), ("counts", mk(counts)), ("totals", mk(totals)), ("n", N), ("dim", DIM), ("metric", 1), ("row_begin", 0),
                       ("row_end", N), ("out_dtype", 0), ("out", out), ("ld_out", N), ("flags", 0), stats],
                      dict(rows, counts_null={"counts": None}, totals_null={"totals": None}, out_null={"out": None}), rows_empty))
    for fn, mk in (("po_pairwise_freq_dev", dev), ("po_pairwise_freq", host)):
        out = room(N * 32 * 8) if mk is dev else host(np.zeros((N, N)))
        specs.append((fn, "stats",
                      [("ctx", ctx), ("freq", mk(freq)), ("n", N), ("dim", DIM), ("metric", 1), ("row_begin", 0), ("row_end", N), ("out_dtype", 0),
                       ("out", out), ("ld_out", N), ("flags", 0), stats],
                      dict(rows, freq_null={"freq": None}, out_null={"out": None}), rows_empty))
    b_out, b_mirror = room(N * N * 8), room(N * N * 8)
    good = _block(0, 4, 4, N, b_out, 4, b_mirror, 4)
    specs.append(("po_pairwise_blocks_dev", "stats",
                  [("ctx", ctx), ("counts", dev(counts)), ("totals", dev(totals)), ("n", N), ("dim", DIM), ("metric", 1), ("out_dtype", 0),
                   ("blocks", [_block(0, N, 0, N, b_out, N, triangular=1), good]), ("n_blocks", 2), ("flags", 0), stats],
                  dict(common, dtype_2={"out_dtype": 2}, counts_null={"counts": None}, totals_null={"totals": None}, blocks_null={"blocks": None},
                       block_past_n={"blocks": [good, _block(0, 4, 4, N + 1, b_out, 5)]},
                       block_reversed={"blocks": [_block(4, 3, 0, N, b_out, N), good]},
                       block_triangular_uneven={"blocks": [good, _block(0, 4, 0, N, b_out, N, triangular=1)]},
                       block_ld_out_short={"blocks": [good, _block(0, 4, 4, N, b_out, 3)]},
                       block_ld_mirror_short={"blocks": [good, _block(0, 4, 4, N, b_out, 4, b_mirror, 3)]},
                       block_no_output={"blocks": [good, _block(0, 4, 4, N)]}),
                  {"n_blocks_0": {"n_blocks": 0}, "n_blocks_0_list_null": {"n_blocks": 0, "blocks": None},
                   "blocks_empty": {"blocks": [_block(2, 2, 0, N), _block(0, N, 5, 5)]}, "n_0": {"n": 0, "blocks": [_block(0, 0, 0, 0)] * 2},
                   "stats_null": {"stats": None}}))

    # ---- k nearest neighbours ------------------------------------------------------------------------------------------
    knn = dict(common, k_0={"k": 0}, k_1025={"k": 1025}, dtype_2={"val_dtype": 2}, panel_rows_100={"panel_rows": 100},
               counts_null={"counts": None}, totals_null={"totals": None}, idx_null={"idx": None}, val_null={"val": None})
    for fn, mk in (("po_knn_dev", dev), ("po_knn", host)):
        idx, val = (room(N * K * 4), room(N * K * 8)) if mk is dev else (host(np.zeros((N, K), np.int32)), host(np.zeros((N, K))))
        specs.append((fn, "stats",
                      [("ctx", ctx), ("counts", mk(counts)), ("totals", mk(totals)), ("n", N), ("dim", DIM), ("metric", 1), ("k", K), ("val_dtype", 0),
                       ("panel_rows", 0), ("idx", idx), ("val", val), ("flags", 0), stats],
                      knn, {"n_1": {"n": 1}, "n_0": {"n": 0}, "n_1_all_null": {"n": 1, "counts": None, "totals": None, "idx": None, "val": None},
                            "stats_null": {"stats": None}, "panel_rows_128": {"panel_rows": 128}}))
    rect = _block(0, 128, 128, N128)
    specs.append(("po_knn_blocks_dev", "stats",
                  [("ctx", ctx), ("counts", dev(counts128)), ("totals", dev(totals128)), ("n", N128), ("dim", DIM), ("metric", 1), ("k", K),
                   ("val_dtype", 0), ("panel_rows", 128), ("blocks", [_block(0, 128, 0, 128, triangular=1), rect]), ("n_blocks", 2),
                   ("idx", room(N128 * K * 4)), ("val", room(N128 * K * 8)), ("flags", 0), stats],
                  dict(knn, blocks_null={"blocks": None}, block_past_n={"blocks": [rect, _block(0, 128, 128, N128 + 1)]},
                       block_reversed={"blocks": [_block(128, 0, 128, N128), rect]},
                       block_rows_off_128={"blocks": [rect, _block(1, 128, 128, N128)]},
                       block_cols_off_128={"blocks": [rect, _block(128, N128, 64, 128)]},
                       block_triangular_uneven={"blocks": [rect, _block(0, 128, 0, N128, triangular=1)]},
                       block_across_diagonal={"blocks": [rect, _block(0, N128, 128, N128)]},
                       block_square_not_triangular={"blocks": [_block(0, N128, 0, N128), rect]}),
                  {"n_blocks_0": {"n_blocks": 0}, "n_blocks_0_list_null": {"n_blocks": 0, "blocks": None},
                   "blocks_empty": {"blocks": [_block(128, 128, 0, 128), _block(0, 128, 128, 128)]}, "n_1": {"n": 1, "blocks": [_block(0, 1, 0, 1, triangular=1)] * 2}}))
    lists_idx = np.stack([np.stack([rng.permutation(N)[:K] for _ in range(N)]) for _ in range(2)]).astype(np.int32)
    lists_val = np.sort(rng.random((2, N, K)), axis=2)
    specs.append(("po_knn_merge_dev", None,
                  [("ctx", ctx), ("n", N), ("k", K), ("metric", 1), ("val_dtype", 0), ("idx_in", dev(lists_idx)), ("val_in", dev(lists_val)), ("m", 2),
                   ("idx", room(N * K * 4)), ("val", room(N * K * 8))],
                  {"ctx_null": {"ctx": None}, "metric_negative": {"metric": -1}, "metric_5": {"metric": 5}, "k_0": {"k": 0}, "k_1025": {"k": 1025},
                   "dtype_2": {"val_dtype": 2}, "idx_in_null": {"idx_in": None}, "val_in_null": {"val_in": None}, "idx_null": {"idx": None},
                   "val_null": {"val": None}},
                  {"n_0": {"n": 0}, "m_0_inputs_null": {"m": 0, "idx_in": None, "val_in": None}}))

    # ---- t-SNE ---------------------------------------------------------------------------------------------------------
    others = np.array([[j for j in range(N) if j != i] for i in range(N)], dtype=np.int32)
    dist = np.abs(others - np.arange(N)[:, None]).astype(np.float64)
    order = np.argsort(dist, axis=1, kind="stable")
    t_idx, t_val = np.take_along_axis(others, order, 1), np.take_along_axis(dist, order, 1)

    def changed(a, value, at=(2, 1)):
        b = a.copy()
        b[at] = value
        return b

    list_rules = {"ctx_null": {"ctx": None}, "metric_negative": {"metric": -1}, "metric_5": {"metric": 5}, "metric_kt": {"metric": 2},
                  "dtype_2": {"val_dtype": 2}, "perplexity_half": {"perplexity": 0.5}, "perplexity_nan": {"perplexity": float("nan")},
                  "perplexity_400": {"perplexity": 400.0}, "n_3": {"n": 3, "k": 2}, "k_6": {"k": 6}, "idx_null": {"idx": None}, "val_null": {"val": None}}

    def list_data(mk):
        return {"list_self": {"idx": mk(changed(t_idx, 2))}, "list_index_8": {"idx": mk(changed(t_idx, N))},
                "list_index_negative": {"idx": mk(changed(t_idx, -1))}, "list_duplicate": {"idx": mk(changed(t_idx, t_idx[2, 0]))},
                "list_nan": {"val": mk(changed(t_val, np.nan))}, "list_negative": {"val": mk(changed(t_val, -1.0))}}

    cap = 2 * N * TSNE_K
    specs.append(("po_tsne_affinities_dev", "nnz",
                  [("ctx", ctx), ("n", N), ("k", TSNE_K), ("metric", 1), ("val_dtype", 0), ("idx", dev(t_idx)), ("val", dev(t_val)),
                   ("perplexity", PERPLEXITY), ("beta", room(N * 8)), ("cond", room(N * TSNE_K * 8)), ("rowptr", room((N + 1) * 8)),
                   ("col", room(cap * 4)), ("p", room(cap * 4)), ("cap", cap), ("nnz", "nnz")],
                  dict(list_rules, **list_data(dev), rowptr_null={"rowptr": None}, col_null={"col": None}, p_null={"p": None}, nnz_null={"nnz": None},
                       cap_1={"cap": 1}),
                  {"beta_cond_null": {"beta": None, "cond": None}}))
    rowptr = (np.arange(N + 1) * (N - 1)).astype(np.int64)
    col = others.reshape(-1).copy()
    p = np.full(col.size, 1.0 / col.size, dtype=np.float32)
    y0 = (rng.standard_normal((N, 2)) * 1e-4).astype(np.float32)
    nnz = int(col.size)
    csr = {"csr_column_8": {"col": dev(changed(col, N, 9))}, "csr_column_negative": {"col": dev(changed(col, -1, 9))},
           "csr_rowptr_past_nnz": {"rowptr": dev(changed(rowptr, nnz + 1, 3))}, "rowptr_null": {"rowptr": None}, "col_null": {"col": None},
           "p_null": {"p": None}, "ctx_null": {"ctx": None}}
    z, kl = ctypes.c_double(), ctypes.c_double()
    specs.append(("po_tsne_gradient_dev", None,
                  [("ctx", ctx), ("n", N), ("rowptr", dev(rowptr)), ("col", dev(col)), ("p", dev(p)), ("nnz", nnz), ("y", dev(y0)), ("exaggeration", 1.0),
                   ("grad", room(N * 2 * 4)), ("z", ctypes.pointer(z)), ("kl", ctypes.pointer(kl))],
                  dict(csr, n_0={"n": 0}, y_null={"y": None}, grad_null={"grad": None}, exaggeration_0={"exaggeration": 0.0},
                       exaggeration_nan={"exaggeration": float("nan")}),
                  {"z_kl_null": {"z": None, "kl": None}, "nnz_0_col_p_null": {"nnz": 0, "col": None, "p": None, "rowptr": dev(np.zeros(N + 1, np.int64))}}))
    quick = dict(max_iter=10, n_iter_check=5)
    params = {"early_exaggeration_half": {"params": dict(quick, early_exaggeration=0.5)}, "learning_rate_negative": {"params": dict(quick, learning_rate=-1.0)},
              "min_grad_norm_negative": {"params": dict(quick, min_grad_norm=-1.0)}}
    specs.append(("po_tsne_dev", "result",
                  [("ctx", ctx), ("n", N), ("rowptr", dev(rowptr)), ("col", dev(col)), ("p", dev(p)), ("nnz", nnz), ("y0", dev(y0)), ("params", quick),
                   ("y", room(N * 2 * 4)), ("result", "result")],
                  dict(csr, **params, n_3={"n": 3}, y0_null={"y0": None}, y_null={"y": None}), {"result_null": {"result": None}}))
    specs.append(("po_tsne", "result",
                  [("ctx", ctx), ("n", N), ("k", TSNE_K), ("metric", 1), ("val_dtype", 0), ("idx", host(t_idx)), ("val", host(t_val)),
                   ("perplexity", PERPLEXITY), ("y0", host(y0)), ("params", quick), ("y", host(np.zeros((N, 2), np.float32))), ("result", "result")],
                  dict(list_rules, **list_data(host), **params, y0_null={"y0": None}, y_null={"y": None}), {"result_null": {"result": None}}))
    return specs, keep


def _convert(value, structs, torch):
    from phyloligo_amd import _lib
    if isinstance(value, Misaligned):
        return value.buf.data_ptr() + 1
    if isinstance(value, torch.Tensor):
        return value.data_ptr()
    if isinstance(value, np.ndarray):
        return value.ctypes.data
    if isinstance(value, list):                      # a block list
        arr = (_lib.PoBlock * len(value))()
        for dst, src in zip(arr, value):
            for key, v in src.items():
                setattr(dst, key, _convert(v, structs, torch) if key in ("out", "mirror") else v)
        structs.append(arr)
        return arr
    if isinstance(value, dict):                      # po_tsne_params
        par = _lib.PoTsneParams(**value)
        structs.append(par)
        return ctypes.pointer(par)
    return value


def run_cases(lib, torch):
    """{"entry point::case": [status, message or None, out-struct zeroed or None]} of the loaded library"""
    from phyloligo_amd import _lib
    handle = ctypes.c_void_p()
    assert lib.po_ctx_create(ctypes.byref(handle), 0) == 0, lib.po_last_error()
    specs, keep = build_specs(torch, handle)
    outs = {"stats": _lib.PoStats(), "result": _lib.PoTsneResult(), "nnz": ctypes.c_uint64()}
    results = {}
    for fn, out_kind, args, faults, empty in specs:
        call = getattr(lib, fn)
        cases = [("good", {})] + sorted(faults.items()) + sorted(empty.items())
        for (a, fa), (b, fb) in itertools.combinations(sorted(faults.items()), 2):
            if not set(fa) & set(fb):
                cases.append((a + "+" + b, dict(fa, **fb)))
        for case, change in cases:
            unknown = set(change) - {key for key, _ in args}
            assert not unknown, (fn, case, unknown)
            structs, argv = [], []
            for key, value in args:
                value = change.get(key, value)
                if isinstance(value, str):           # this call's out-struct
                    ctypes.memset(ctypes.byref(outs[value]), PATTERN, ctypes.sizeof(outs[value]))
                    value = ctypes.pointer(outs[value])
                argv.append(_convert(value, structs, torch))
            status = call(*argv)
            message = lib.po_last_error().decode("utf-8", "replace") if status else None
            zeroed = None
            if out_kind and change.get(out_kind, out_kind) is not None:
                zeroed = not any(ctypes.string_at(ctypes.byref(outs[out_kind]), ctypes.sizeof(outs[out_kind])))
            results["%s::%s" % (fn, case)] = [status, message, zeroed]
    assert lib.po_ctx_synchronize(handle) == 0, lib.po_last_error()
    lib.po_ctx_destroy(handle)
    del keep
    return results


def main():
    import torch
    from phyloligo_amd import _lib
    lib = _lib.load()
    results = run_cases(lib, torch)
    outcomes, index = [], {}
    for name, outcome in results.items():
        if outcome not in outcomes:
            outcomes.append(outcome)
        index[name] = outcomes.index(outcome)
    with open(PATH, "w") as fh:
        json.dump({"library": lib.po_version().decode(), "outcomes": outcomes, "cases": index}, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    refused = sum(1 for o in results.values() if o[0])
    print("%s: %d cases (%d refused, %d accepted), %d distinct outcomes" % (PATH, len(results), refused, len(results) - refused, len(outcomes)))


if __name__ == "__main__":
    main()
