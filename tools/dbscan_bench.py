#!/usr/bin/env python3
"""DBSCAN of a matrix in HBM (po_eps_degrees_dev, po_dbscan_dev) on the GPU.
    python tools/dbscan_bench.py            BASELINE config 2 (50 000 contigs x 2 kb, JSD), float64 and float32 matrix; 50 000
                                            contigs of a four-species ragged assembly, JSD float64 and float32; 200 000 contigs,
                                            Eucl, float32; one JSON line per case
    python tools/dbscan_bench.py --quick    the 50 000 cases only
    python tools/dbscan_bench.py --cli      also the command line at 50 000 contigs of the ragged assembly: --dbscan EPS
                                            --dbscan-min-samples 10 end to end against --kmedoids 8 of the same input
Times are device-event times, the best of three after one warm-up call that grows the workspace.
  eps            the median, over 2 048 evenly spaced rows, of the distance to the M-th nearest record (M = min_samples = 10, the
                 record itself counted): a point of the k-distance curve that `--knn M` writes
  degree_ms      Context.eps_degrees: one read of every row
  pass_ms        one propagation round over ALL rows: label_ms / passes of a call with min_samples = 1 (every record core, no
                 border pass); the hook and jump kernels of the round are in it
  border_ms      the minimum-label pass over all rows as the border pass runs it: label_ms of a call with min_samples = n + 1 (no
                 record core, no round)
  call_ms        the whole Context.dbscan call at (eps, M) with its phases and counts (passes: rounds the input needed)
against two yardsticks of the same run: rowsum_ms, the row-sum kernel of the k-medoids update over the same matrix with every
column in one cluster (the read-once floor), and copy_ms, a device-to-device copy of the same bytes (of the first rows that fit
beside the matrix, scaled to the whole), which moves twice the bytes."""
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
from phyloligo_amd import synthetic  # noqa: E402
from kmedoids_bench import copy_ms, matrix, timed  # noqa: E402

M = 10


def k_distance(d, m, rows=2048):
    """the distance of `rows` evenly spaced records to their m-th nearest record, themselves counted: ascending float64 numpy"""
    n = d.shape[0]
    pick = torch.linspace(0, n - 1, min(rows, n), device=d.device).long()
    kth = torch.kthvalue(d[pick].double(), m, dim=1).values
    return np.sort(kth.cpu().numpy())


def case(ctx, name, n, metric, dtype, ragged=False, reps=3):
    buf, ld, pair_ms = matrix(ctx, n, metric, dtype, ragged)
    d = buf[:, :n]
    cp, cp_rows = copy_ms(buf)
    nbytes = n * n * buf.element_size()
    one = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx.kmedoids_costs(d, one)
    rowsum = min(timed(lambda: ctx.kmedoids_costs(d, one))[1] for _ in range(reps))
    eps = float(np.median(k_distance(d, M)))
    ctx.dbscan(d, eps, M)                                                 # grows the workspace
    degree = min(timed(lambda: ctx.eps_degrees(d, eps))[1] for _ in range(reps))

    def best(min_samples, key):
        runs = [timed(lambda: ctx.dbscan(d, eps, min_samples, want_stats=True)) for _ in range(reps)]
        return min(runs, key=lambda r: key(r[0][2]))

    (_, _, st1), _ = best(1, lambda st: st["label_ms"] / st["passes"])
    (_, _, st0), _ = best(n + 1, lambda st: st["label_ms"])
    (_, _, st), whole = best(M, lambda st: st["degree_ms"] + st["label_ms"] + st["finish_ms"])
    one_pass = st1["label_ms"] / st1["passes"]
    out = {"case": name, "n": n, "metric": metric, "matrix": dtype, "ld": ld, "eps": eps, "min_samples": M, "pairwise_ms": pair_ms,
           "degree_ms": degree, "pass_ms": one_pass, "passes_all_core": st1["passes"], "border_ms": st0["label_ms"],
           "rowsum_ms": rowsum, "copy_ms": cp, "copy_rows": cp_rows, "degree_over_rowsum": degree / rowsum,
           "pass_over_rowsum": one_pass / rowsum, "border_over_rowsum": st0["label_ms"] / rowsum, "degree_over_copy": degree / cp,
           "pass_over_copy": one_pass / cp, "border_over_copy": st0["label_ms"] / cp, "rowsum_over_copy": rowsum / cp,
           "degree_read_tb_s": nbytes / (degree * 1e-3) / 1e12, "pass_read_tb_s": nbytes / (one_pass * 1e-3) / 1e12,
           "call_ms": whole, "call_degree_ms": st["degree_ms"], "call_label_ms": st["label_ms"], "call_finish_ms": st["finish_ms"],
           "passes": st["passes"], "clusters": st["clusters"], "core": st["core"], "border": st["border"], "noise": st["noise"]}
    print(json.dumps(out), flush=True)
    del buf, d
    ctx.trim()
    torch.cuda.empty_cache()
    return out


def cli(n, eps):
    seq, off = synthetic.ragged_assembly(n, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
    res = {"case": "cli_ragged_n%d" % n, "eps": eps, "min_samples": M}
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "asm.fa")
        with open(fa, "wb") as fh:
            fh.write(synthetic.fasta_bytes(seq, off))
        js = os.path.join(tmp, "stats.json")

        def run(*mode):
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", fa, "-d", "JSD", "--method", "joblib",
                                "-o", os.path.join(tmp, "c.txt"), "--json-stats", js] + list(mode),
                               cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-400:])
            return wall, json.load(open(js))

        run("--dbscan", repr(eps), "--dbscan-min-samples", str(M))            # (the first run of a process tree pays for the page cache)
        wall, s = run("--dbscan", repr(eps), "--dbscan-min-samples", str(M))
        res.update(dbscan_wall_s=wall, dbscan_seconds=s["seconds"], dbscan_ms=s["dbscan_ms"], dbscan_phases_ms=s["dbscan_phases_ms"],
                   dbscan_passes=s["dbscan_passes"], dbscan_clusters=s["dbscan_clusters"], dbscan_noise=s["dbscan_noise"],
                   dbscan_sizes=s["dbscan_sizes"][:16])
        wall, s = run("--kmedoids", "8")
        res.update(kmedoids_wall_s=wall, kmedoids_seconds=s["seconds"], kmedoids_ms=s["kmedoids_ms"], kmedoids_iterations=s["kmedoids_iterations"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--cli", action="store_true")
    a = ap.parse_args()
    ctx = pa.Context(0)
    print("library", pa._lib.load().po_version().decode(), "--", ctx.device_name, flush=True)
    results = []
    for dtype in ("float64", "float32"):
        results.append(case(ctx, "n50k", 50000, "JSD", dtype))
    ragged = [case(ctx, "n50k_ragged_assembly", 50000, "JSD", dtype, ragged=True) for dtype in ("float64", "float32")]
    results += ragged
    if not a.quick:
        results.append(case(ctx, "n200k", 200000, "Eucl", "float32"))
    if a.cli:
        del ctx
        torch.cuda.empty_cache()
        results.append(cli(50000, ragged[0]["eps"]))
    print(json.dumps({"dbscan_bench": results}))


if __name__ == "__main__":
    main()
