"""The long GPU steps of tests/test_gpu_tsne.py, run as a child process so that each has a time limit of its own:
    python tests/tsne_child.py JOB OUT.npz [ARG]
JOB: whole (ARG = seed: the 1 000-contig Eucl input, perplexity 30, 1 000 iterations), grad50000 (gradient of a seeded cloud of
50 000 points under an empty P), run50000 (50 000 contigs, JSD, perplexity 30, 1 000 iterations).  Results go to OUT.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import tsne_ref  # noqa: E402

import phyloligo_amd as pa  # noqa: E402
from phyloligo_amd import api, synthetic  # noqa: E402


def cloud50000():
    return (30.0 * np.random.RandomState(5).standard_normal((50000, 2))).astype(np.float32)


def main():
    job, out = sys.argv[1], sys.argv[2]
    with pa.Context(0) as ctx:
        if job == "whole":
            g = np.load(os.path.join(HERE, "golden", "tsne_sklearn.npz"))
            n, perplexity = int(g["n"]), float(g["perplexity"])
            counts, totals, _ = tsne_ref.make_input(n)
            idx, val = ctx.knn(counts, totals, api.tsne_neighbours(n, perplexity), "Eucl")
            y, st = ctx.tsne(idx, val, perplexity, seed=int(sys.argv[3]), max_iter=1000, want_stats=True)
            a = ctx.tsne_affinities(idx, val, perplexity, "Eucl")
            np.savez(out, y=y, kl=st["kl"], iterations=st["iterations"], rowptr=a["rowptr"], col=a["col"], p=a["p"])
        elif job == "grad50000":
            y = cloud50000()
            grad, z, _ = ctx.tsne_gradient(np.zeros(50001, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), y, 1.0)
            np.savez(out, grad=grad, z=z)
        elif job == "run50000":
            n, perplexity = 50000, 30
            seq, offsets = synthetic.ragged_assembly(n, seed=7, median=3000, lo=1000, hi=20000, dirt=False)
            counts, totals = ctx.count_profiles(seq, offsets, "1111", "both")
            idx, val = ctx.knn(counts, totals, api.tsne_neighbours(n, perplexity), "JSD")
            y, st = ctx.tsne(idx, val, perplexity, max_iter=1000, want_stats=True, metric="JSD")
            np.savez(out, y=y, kl=st["kl"], iterations=st["iterations"], history=np.array(st["history"]),
                     ms=np.array([st["affinities_ms"], st["optimise_ms"]]))
        else:
            raise SystemExit("unknown job %r" % job)


if __name__ == "__main__":
    main()
