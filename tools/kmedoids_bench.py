#!/usr/bin/env python3
"""k-medoids on a matrix in HBM (po_pairwise_dev + po_kmedoids_dev) on the GPU.
    python tools/kmedoids_bench.py            BASELINE config 2 (50 000 contigs x 2 kb, JSD), float64 and float32 matrix, K = 8 and
                                              K = 64 (random contigs: the loop ends after one pass); 50 000 contigs of a four-species
                                              ragged assembly, K = 8 (several passes); then 200 000 contigs, Eucl, float32, K = 8;
                                              one JSON line per case
    python tools/kmedoids_bench.py --quick    the 50 000 cases only (for a rocprofv3 --kernel-trace --stats pass)
    python tools/kmedoids_bench.py --cli      also the whole command line at 50 000 contigs (python -m phyloligo_amd --kmedoids 8)
Times are device-event times after one warm-up call that grows the workspaces.  start_ms: the heuristic start (one unmasked
row-sum pass, n doubles to the host, selection there).  rowsum_ms / assign_ms / update_ms: per iteration, from the library's
own events (po_kmedoids_result), of a run of at most --iters iterations.  copy_ms: a plain device-to-device copy of the same
matrix bytes in the same process (of the first rows that fit beside the matrix, scaled to the whole) - the yardstick of the
row-sum kernel: the copy moves twice the bytes, so a read-only streaming kernel should not take longer.  rowsum_over_copy is
that ratio, read_tb_s the matrix bytes (plus the K medoid rows) over rowsum_ms."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

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
    if ragged:                     # four species, contig lengths of a real assembly: clusters exist, the loop takes several passes
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


def copy_ms(buf, reps=3):
    """device-to-device copy of the matrix bytes: of as many whole rows as fit into the free memory, scaled to all rows"""
    n, ld = buf.shape
    free = torch.cuda.mem_get_info()[0]
    rows = int(min(n, (free * 0.9) // (ld * buf.element_size())))
    dst = torch.empty((rows, ld), dtype=buf.dtype, device="cuda")
    dst.copy_(buf[:rows])
    best = min(timed(lambda: dst.copy_(buf[:rows]))[1] for _ in range(reps))
    del dst
    return best * n / rows, rows


def cases(ctx, name, n, metric, dtype, ks, iters, ragged=False):
    buf, ld, pair_ms = matrix(ctx, n, metric, dtype, ragged)
    d = buf[:, :n]
    cp, cp_rows = copy_ms(buf)
    nbytes = n * ld * buf.element_size()
    out = []
    for k in ks:
        ctx.kmedoids(d, k, max_iter=1)
        (_, _, st), whole = timed(lambda: ctx.kmedoids(d, k, max_iter=iters, want_stats=True))
        it = st["iterations"]
        rowsum = st["rowsum_ms"] / it
        out.append({"case": name, "n": n, "metric": metric, "matrix": dtype, "ld": ld, "k": k, "pairwise_ms": pair_ms,
                    "start_ms": st["start_ms"], "iterations": it, "converged": st["converged"], "rowsum_ms": rowsum,
                    "assign_ms": st["assign_ms"] / it, "update_ms": st["update_ms"] / it, "call_ms": whole,
                    "copy_ms": cp, "copy_rows": cp_rows, "copy_tb_s_read_plus_write": 2 * nbytes / (cp * 1e-3) / 1e12,
                    "rowsum_over_copy": rowsum / cp, "read_tb_s": (n + k) * n * buf.element_size() / (rowsum * 1e-3) / 1e12,
                    "empty_clusters": st["empty_clusters"], "inertia": st["inertia"]})
        print(json.dumps(out[-1]), flush=True)
    del buf, d
    ctx.trim()
    torch.cuda.empty_cache()
    return out


def cli(n, k):
    seq, off = synthetic.contig_bytes(n, 2000, seed=synthetic.SEEDS["C2"])
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "asm.fa")
        with open(fa, "wb") as fh:
            fh.write(synthetic.fasta_bytes(seq, off))
        res = {"case": "cli_n%d" % n, "k": k}
        for dtype in ("float64", "float32"):
            js = os.path.join(tmp, "stats.json")
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", fa, "-d", "JSD", "--method", "joblib", "--kmedoids", str(k),
                                "--kmedoids-dtype", dtype, "--kmedoids-iter", "20", "-o", os.path.join(tmp, "c.txt"), "--json-stats", js],
                               cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
            res[dtype + "_wall_s"] = time.perf_counter() - t0
            if r.returncode != 0:
                res[dtype + "_error"] = r.stderr[-400:]
                continue
            s = json.load(open(js))
            res[dtype] = {"seconds": s["seconds"], "kmedoids_ms": s["kmedoids_ms"], "kmedoids_iterations": s["kmedoids_iterations"],
                          "kmedoids_phases_ms": s["kmedoids_phases_ms"]}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    ctx = pa.Context(0)
    print("library", pa._lib.load().po_version().decode(), "--", ctx.device_name, flush=True)
    results = []
    for dtype in ("float64", "float32"):
        results += cases(ctx, "n50k", 50000, "JSD", dtype, (8, 64), a.iters)
    results += cases(ctx, "n50k_ragged_assembly", 50000, "JSD", "float64", (8,), a.iters, ragged=True)
    if not a.quick:
        results += cases(ctx, "n200k", 200000, "Eucl", "float32", (8,), a.iters)
    if a.cli:
        results.append(cli(50000, 8))
    print(json.dumps({"kmedoids_bench": results}))


if __name__ == "__main__":
    main()
