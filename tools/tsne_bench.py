#!/usr/bin/env python3
"""t-SNE of the k-NN graph (po_tsne_affinities_dev + po_tsne_dev) on the GPU.
    python tools/tsne_bench.py            50 000 contigs (JSD, float64 lists) and 200 000 (Eucl, float32 lists), perplexity 30:
                                          graph, affinities, the optimiser per iteration and its split into the repulsion
                                          kernel, the attraction + update kernel and the rest; one JSON line per case
    python tools/tsne_bench.py --quick    50 000 only (for a rocprofv3 --kernel-trace --stats pass)
Times are device-event times after one warm-up call that grows the workspaces.  iteration_ms: the median over --reps runs of
--iters iterations divided by --iters (the checks every 50 iterations included).  repulsion_ms / attraction_ms / rest_ms: one more
run with po_tsne_params.time_kernels, events around the kernels of every iteration, median over the iterations (rest: start of
an iteration to the start of the next, less the two kernels - the Z reduction and the gaps between launches)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import phyloligo_amd as pa  # noqa: E402
from phyloligo_amd import api, synthetic  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def case(ctx, name, n, metric, dtype, perplexity, iters, reps):
    seq, off = synthetic.ragged_assembly(n, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
    c, t = ctx.count_profiles(torch.from_numpy(seq).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), "1111", "both")
    del seq
    k = api.tsne_neighbours(n, perplexity)
    res = {"case": name, "n": n, "metric": metric, "lists": dtype, "perplexity": perplexity, "k": k}
    ctx.knn(c, t, k, metric, dtype=dtype)
    (idx, val), res["graph_ms"] = timed(lambda: ctx.knn(c, t, k, metric, dtype=dtype))
    ctx.tsne_affinities(idx, val, perplexity, metric)
    a, res["affinities_ms"] = timed(lambda: ctx.tsne_affinities(idx, val, perplexity, metric))
    res["nnz"] = int(a["col"].numel())
    y0 = torch.from_numpy(api.tsne_start(n, 0)).cuda()
    ctx.tsne_optimise(a["rowptr"], a["col"], a["p"], y0, max_iter=50)
    per = []
    for _ in range(reps):
        (_, st), ms = timed(lambda: ctx.tsne_optimise(a["rowptr"], a["col"], a["p"], y0, max_iter=iters, want_stats=True))
        per.append(ms / st["iterations"])
    _, st = ctx.tsne_optimise(a["rowptr"], a["col"], a["p"], y0, max_iter=iters, want_stats=True, time_kernels=True)
    res.update(repulsion_ms=st["repulsion_ms"], attraction_ms=st["attraction_ms"], rest_ms=st["rest_ms"])
    res.update(iterations=iters, iteration_ms=float(np.median(per)), pairs_per_s=n * float(n) / (float(np.median(per)) * 1e-3))
    ctx.trim()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    ctx = pa.Context(0)
    print("library", pa._lib.load().po_version().decode(), "--", ctx.device_name, flush=True)
    results = [case(ctx, "n50k", 50000, "JSD", "float64", 30, a.iters, a.reps)]
    print(json.dumps(results[-1]), flush=True)
    if not a.quick:
        results.append(case(ctx, "n200k", 200000, "Eucl", "float32", 30, a.iters, a.reps))
        print(json.dumps(results[-1]), flush=True)
    print(json.dumps({"tsne_bench": results}))


if __name__ == "__main__":
    main()
