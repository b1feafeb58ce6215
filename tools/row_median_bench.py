#!/usr/bin/env python3
"""Row medians of a matrix in HBM (po_pairwise_dev + po_row_medians_dev) on the GPU.
    python tools/row_median_bench.py            BASELINE config 2 (50 000 contigs x 2 kb, JSD), float64 and float32 matrix; 50 000
                                                contigs of the four-species ragged assembly (JSD, float64: the value distribution
                                                real rows have); then 200 000 contigs, Eucl, float32; one JSON line per case
    python tools/row_median_bench.py --quick    the 50 000 cases only (for a rocprofv3 --kernel-trace --stats pass)
Times are device-event times, the best of --reps calls after one warm-up call.
  median_ms          po_row_medians_dev over the whole matrix
  reads_per_row      how often the selection read a row from memory, averaged over the rows (po_row_medians_passes): the bytes
                     read per matrix byte; read_tb_s = reads_per_row x matrix bytes / median_ms
  rowsum_ms          the read-once floor of this access pattern: the k-medoids row-sum kernel over the same matrix, one workgroup
                     per few rows, every byte read once (po_kmedoids_costs_dev with one label for all: every column counts; it
                     also reads 4 bytes of label per column from L2); start_ms: the unmasked pass of the heuristic start, which
                     includes copying the n sums to the host and selecting there
  sort_ms            what a user would otherwise call: torch.sort(dim=1) of a row panel that fits beside the matrix, scaled to
                     all rows (the median is then two gathers)
  median_over_rowsum, sort_over_median       the two ratios"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import phyloligo_amd as pa  # noqa: E402
from phyloligo_amd import synthetic  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def matrix(ctx, n, metric, dtype, ragged=False):
    if ragged:
        seq, off = synthetic.ragged_assembly(n, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
    else:
        seq, off = synthetic.contig_bytes(n, 2000, seed=synthetic.SEEDS["C2" if n <= 50000 else "C4"])
    c, t = ctx.count_profiles(torch.from_numpy(seq).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), "1111", "both")
    del seq
    esz = 4 if dtype == "float32" else 8
    ld = (n + 128 // esz - 1) // (128 // esz) * (128 // esz)
    buf = torch.empty((n, ld), dtype=torch.float32 if dtype == "float32" else torch.float64, device="cuda")
    _, ms = timed(lambda: ctx.pairwise(c, t, metric, dtype=dtype, out=buf))
    return buf, ld, ms


def sort_ms(d, reps):
    """torch.sort(dim=1) of as many rows as fit (values + int64 indices + scratch), scaled to all rows"""
    n = d.shape[0]
    free = torch.cuda.mem_get_info()[0]
    rows = int(max(1, min(n, 4096, (free * 0.2) // (d.shape[1] * (d.element_size() + 8)))))
    panel = d[:rows].contiguous()
    torch.sort(panel, dim=1)
    best = min(timed(lambda: torch.sort(panel, dim=1))[1] for _ in range(reps))
    return best * n / rows, rows


def case(ctx, name, n, metric, dtype, reps, ragged=False):
    buf, ld, pair_ms = matrix(ctx, n, metric, dtype, ragged)
    d = buf[:, :n]
    nbytes = n * n * buf.element_size()
    med = ctx.row_medians(d)
    med_ms = min(timed(lambda: ctx.row_medians(d))[1] for _ in range(reps))
    reads = ctx.row_medians_passes() / n
    labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx.kmedoids_costs(d, labels)
    rowsum = min(timed(lambda: ctx.kmedoids_costs(d, labels))[1] for _ in range(reps))
    _, _, st = ctx.kmedoids(d, 8, max_iter=1, want_stats=True)
    srt, srt_rows = sort_ms(d, reps)
    # the sorted panel gives the same medians (a spot check of the measured call, not the test)
    rows = min(n, 256)
    s = torch.sort(d[:rows].double(), dim=1)[0]
    want = (s[:, (n - 1) // 2] + s[:, n // 2]) * 0.5
    res = {"case": name, "n": n, "metric": metric, "matrix": dtype, "ld": ld, "pairwise_ms": pair_ms, "median_ms": med_ms,
           "reads_per_row": reads, "read_tb_s": reads * nbytes / (med_ms * 1e-3) / 1e12, "rowsum_ms": rowsum,
           "rowsum_read_tb_s": nbytes / (rowsum * 1e-3) / 1e12, "start_ms": st["start_ms"], "sort_ms": srt, "sort_rows": srt_rows,
           "median_over_rowsum": med_ms / rowsum, "sort_over_median": srt / med_ms,
           "spot_check_equal": bool(torch.equal(med[:rows], want)),
           "median_of_medians": float(torch.sort(med)[0][n // 2]), "q97": float(pa.api.clip_threshold(med.cpu().numpy(), 0.97))}
    print(json.dumps(res), flush=True)
    del buf, d, s
    ctx.trim()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = pa.Context(0)
    print("library", pa._lib.load().po_version().decode(), "--", ctx.device_name, flush=True)
    results = [case(ctx, "n50k", 50000, "JSD", dtype, a.reps) for dtype in ("float64", "float32")]
    results.append(case(ctx, "n50k_ragged_assembly", 50000, "JSD", "float64", a.reps, ragged=True))
    if not a.quick:
        results.append(case(ctx, "n200k", 200000, "Eucl", "float32", a.reps))
    print(json.dumps({"row_median_bench": results}))


if __name__ == "__main__":
    main()
