#!/usr/bin/env python3
"""k-NN graph (po_knn_dev) against the dense matrix (po_pairwise_dev) on the same GPU, inputs and dtype, and the CLI end to end.
    python tools/knn_bench.py            C2 size (50 000 x 2 kb, JSD, float64, K = 32), 200 000 contigs (Eucl, float32, K = 32),
                                         the CLI with --knn 32 at C2 size; one line per measurement and a JSON summary
    python tools/knn_bench.py --quick    C2 size only (for a rocprofv3 --kernel-trace --stats pass)
Times are HIP-event times of the call on the device (total_ms of po_stats; best of --reps after one warm-up call that grows the
workspaces); for the k-NN call also the split into preparation, tile kernels and selection."""
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


def profiles(ctx, n, length, seed):
    seq, off = synthetic.contig_bytes(n, length, seed=seed)
    c, t = ctx.count_profiles(torch.from_numpy(seq).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), "1111", "both")
    return c, t, seq, off


def case(ctx, name, n, metric, dtype, k, reps, seed=50001):
    c, t, _, _ = profiles(ctx, n, 2000, seed)
    res = {"case": name, "n": n, "metric": metric, "dtype": dtype, "k": k}
    tdt = torch.float32 if dtype == "float32" else torch.float64
    try:
        out = torch.empty((n, n), dtype=tdt, device="cuda")
        dense = []
        for _ in range(reps + 1):
            _, st = ctx.pairwise(c, t, metric, out=out, dtype=dtype, want_stats=True)
            dense.append(st["total_ms"])
        res["dense_ms"] = min(dense[1:])
        del out
    except (RuntimeError, pa.PhyloligoError) as exc:           # a matrix that does not fit next to its workspaces
        res["dense_ms"] = None
        res["dense_error"] = str(exc)[:200]
    torch.cuda.empty_cache()
    ctx.trim()
    knn = []
    for _ in range(reps + 1):
        _, _, st = ctx.knn(c, t, k, metric, dtype=dtype, want_stats=True)
        knn.append(st)
    best = min(knn[1:], key=lambda s: s["total_ms"])
    res.update(knn_ms=best["total_ms"], knn_prep_ms=best["prep_ms"], knn_tiles_ms=best["kernel_ms"], knn_select_ms=best["select_ms"])
    if res["dense_ms"]:
        res["ratio"] = res["knn_ms"] / res["dense_ms"]
    ctx.trim()
    return res


def cli(ctx, n, k, reps):
    _, _, seq, off = profiles(ctx, n, 2000, 50001)
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "asm.fasta")
        with open(fa, "wb") as fh:
            fh.write(synthetic.fasta_bytes(seq, off))
        out = os.path.join(tmp, "g.npz")
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "phyloligo_amd", "-i", fa, "-d", "JSD", "--method", "joblib", "--knn", str(k),
                                "-o", out], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
            walls.append(time.perf_counter() - t0)
            if r.returncode:
                return {"case": "cli", "error": r.stderr[-400:]}
        return {"case": "cli", "n": n, "k": k, "metric": "JSD", "wall_s": min(walls), "walls_s": walls,
                "file_bytes": os.path.getsize(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = pa.Context(0)
    print("library", pa._lib.load().po_version().decode(), "--", ctx.device_name, flush=True)
    results = [case(ctx, "C2", 50000, "JSD", "float64", 32, a.reps)]
    print(json.dumps(results[-1]), flush=True)
    if not a.quick:
        results.append(case(ctx, "n200k", 200000, "Eucl", "float32", 32, a.reps, seed=200001))
        print(json.dumps(results[-1]), flush=True)
        results.append(cli(ctx, 50000, 32, a.reps))
        print(json.dumps(results[-1]), flush=True)
    print(json.dumps({"knn_bench": results}))


if __name__ == "__main__":
    main()
