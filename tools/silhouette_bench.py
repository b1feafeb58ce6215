#!/usr/bin/env python3
"""Silhouettes of a clustering of a matrix in HBM (po_silhouette_dev) on the GPU.
    python tools/silhouette_bench.py            BASELINE config 2 (50 000 contigs x 2 kb, JSD), float64 and float32 matrix; 50 000
                                                contigs of a four-species ragged assembly, JSD float64; 200 000 contigs, Eucl,
                                                float32; each with K = 8, C and C + 1 clusters (C = PO_SILHOUETTE_CHUNK: the last
                                                one reads the matrix twice); one JSON line per case
    python tools/silhouette_bench.py --quick    the 50 000 cases only (for a rocprofv3 --kernel-trace --stats pass)
    python tools/silhouette_bench.py --cli      also the command line at 50 000 contigs of the ragged assembly: one
                                                --kmedoids-sweep 2:10 run end to end, and the nine --kmedoids K runs it replaces
Times are device-event times after one warm-up call that grows the workspaces.  sums_ms / finish_ms: the library's own events
(po_silhouette_result): the passes over the matrix, and everything else.  call_ms: the whole Context.silhouette call.  The labels
are uniformly random (what the pass costs does not depend on them).  rowsum_ms: the read-once floor of the same run - the row-sum
kernel of the k-medoids update (po_kmedoids_costs_dev) with every column in one cluster, which reads the matrix once and keeps
one sum per row.  copy_ms: a plain device-to-device copy of the same matrix bytes (of the first rows that fit beside the matrix,
scaled to the whole).  sums_over_rowsum is the ratio the design section quotes; read_tb_s the matrix bytes times the passes over
sums_ms."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import phyloligo_amd as pa  # noqa: E402
from phyloligo_amd import _lib, synthetic  # noqa: E402
from kmedoids_bench import copy_ms, matrix, timed  # noqa: E402

C = _lib.PO_SILHOUETTE_CHUNK


def cases(ctx, name, n, metric, dtype, ks, ragged=False, reps=3):
    buf, ld, pair_ms = matrix(ctx, n, metric, dtype, ragged)
    d = buf[:, :n]
    cp, cp_rows = copy_ms(buf)
    nbytes = n * n * buf.element_size()
    one = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx.kmedoids_costs(d, one)
    rowsum = min(timed(lambda: ctx.kmedoids_costs(d, one))[1] for _ in range(reps))
    out = []
    for k in ks:
        labels = torch.from_numpy(np.random.RandomState(k).randint(0, k, n).astype(np.int32)).cuda()
        ctx.silhouette(d, labels, k)
        best = None
        for _ in range(reps):
            (_, st), whole = timed(lambda: ctx.silhouette(d, labels, k, want_stats=True))
            if best is None or st["sums_ms"] < best[0]["sums_ms"]:
                best = (st, whole)
        st, whole = best
        out.append({"case": name, "n": n, "metric": metric, "matrix": dtype, "ld": ld, "k": k, "passes": st["passes"],
                    "pairwise_ms": pair_ms, "sums_ms": st["sums_ms"], "finish_ms": st["finish_ms"], "call_ms": whole,
                    "rowsum_ms": rowsum, "copy_ms": cp, "copy_rows": cp_rows, "sums_over_rowsum": st["sums_ms"] / rowsum,
                    "sums_per_pass_over_rowsum": st["sums_ms"] / st["passes"] / rowsum, "rowsum_over_copy": rowsum / cp,
                    "read_tb_s": st["passes"] * nbytes / (st["sums_ms"] * 1e-3) / 1e12, "mean": st["mean"]})
        print(json.dumps(out[-1]), flush=True)
    del buf, d
    ctx.trim()
    torch.cuda.empty_cache()
    return out


def cli(n, lo, hi):
    seq, off = synthetic.ragged_assembly(n, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
    res = {"case": "cli_ragged_n%d" % n, "sweep": "%d:%d" % (lo, hi)}
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "asm.fa")
        with open(fa, "wb") as fh:
            fh.write(synthetic.fasta_bytes(seq, off))
        js = os.path.join(tmp, "stats.json")

        def run(*mode):
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", fa, "-d", "JSD", "--method", "joblib", "--kmedoids-iter", "20",
                                "-o", os.path.join(tmp, "c.txt"), "--json-stats", js] + list(mode),
                               cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-400:])
            return wall, json.load(open(js))

        wall, s = run("--kmedoids-sweep", "%d:%d" % (lo, hi))
        res.update(sweep_wall_s=wall, sweep_seconds=s["seconds"], sweep_best=s["kmedoids_sweep_best"],
                   sweep_means=[r["silhouette_mean"] for r in s["kmedoids_sweep"]])
        singles = [run("--kmedoids", str(k)) for k in range(lo, hi + 1)]
        res.update(singles_wall_s=[w for w, _ in singles], singles_wall_sum_s=sum(w for w, _ in singles),
                   singles_means=[q["silhouette_mean"] for _, q in singles],
                   single_silhouette_ms=[q["silhouette_ms"] for _, q in singles], single_kmedoids_ms=[q["kmedoids_ms"] for _, q in singles])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--cli", action="store_true")
    a = ap.parse_args()
    ctx = pa.Context(0)
    print("library", pa._lib.load().po_version().decode(), "--", ctx.device_name, flush=True)
    ks = (8, C, C + 1)
    results = []
    for dtype in ("float64", "float32"):
        results += cases(ctx, "n50k", 50000, "JSD", dtype, ks)
    results += cases(ctx, "n50k_ragged_assembly", 50000, "JSD", "float64", ks, ragged=True)
    if not a.quick:
        results += cases(ctx, "n200k", 200000, "Eucl", "float32", ks)
    if a.cli:
        del ctx
        torch.cuda.empty_cache()
        results.append(cli(50000, 2, 10))
    print(json.dumps({"silhouette_bench": results}))


if __name__ == "__main__":
    main()
