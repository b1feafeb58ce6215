#!/usr/bin/env python3
"""Record which command lines the CLI refuses, and with which words: tests/golden/cli_refusals.json.

Run from the repository root (python tests/golden/make_golden_cli_refusals.py), on the commit whose behaviour is to be kept;
needs no GPU.  Every element of the product of the factor lists below goes through get_cmd() and then through the four refusal
functions in the order main() asks them (clip, k-medoids, t-SNE, k-NN); the first reason found, or null, is the outcome.  The file
holds the factor lists, the table of distinct outcomes and one index into that table per element, in itertools.product order.
tests/test_cli_refusals.py replays it.

Every `return "Error ..."` site of the four functions occurs at least once, with each `who` it can take (SITES below is checked
against the recorded outcomes before the file is written):

  _clip_refused      P outside [0, 1]; --min-size < 0; --clip-out alone; -d KT; several ranks; --method
  _kmedoids_refused  --sweep-out alone; --silhouette alone; sweep with --kmedoids; sweep not LO:HI; sweep range (3:2 and 1:3);
                     with --knn / --tsne (both whos); --large (both); -d KT (both); K < 1; --kmedoids-iter < 1;
                     several ranks (both); --method (both)
  _tsne_refused      with --knn; --large; -d KT; perplexity (below 1, above the most); --tsne-iter < 1; several ranks; --method
  _knn_refused       K out of range (0 and above the most); --large; --method
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FACTORS = {
    "mode": [[], ["--knn", "8"], ["--knn", "0"], ["--knn", "2000"], ["--tsne", "30"], ["--tsne", "0.5"], ["--tsne", "400"],
             ["--tsne", "30", "--tsne-iter", "0"], ["--kmedoids", "3"], ["--kmedoids", "0"], ["--kmedoids", "3", "--kmedoids-iter", "0"],
             ["--kmedoids-sweep", "2:4"], ["--kmedoids-sweep", "3:2"], ["--kmedoids-sweep", "x"], ["--kmedoids-sweep", "1:3"],
             ["--kmedoids-sweep", "2:4", "--kmedoids-iter", "0"], ["--kmedoids-sweep", "2:4", "--kmedoids", "3"],
             ["--sweep-out", "s.tsv"], ["--silhouette", "s.txt"], ["--knn", "8", "--tsne", "30"], ["--kmedoids", "3", "--knn", "8"],
             ["--kmedoids", "3", "--tsne", "30"], ["--kmedoids-sweep", "2:4", "--knn", "8"], ["--kmedoids-sweep", "2:4", "--tsne", "30"]],
    "large": [[], ["--large", "memmap"], ["--large", "h5py"]],
    "distance": [["-d", "Eucl"], ["-d", "KT"]],
    "gpus": [[], ["--gpus", "2"]],
    "method": [["--method", "joblib"], ["--method", "hip"], ["--method", "scoop"]],
    "clip": [[], ["--clip-percentile", "0.97"], ["--clip-percentile", "1.5"], ["--min-size", "-1"], ["--min-size", "500"],
             ["--clip-out", "kept.tsv"], ["--clip-percentile", "0.9", "--clip-out", "kept.tsv"]],
}

SITES = [
    "--clip-percentile P needs 0 <= P <= 1 (got 1.5)", "--min-size L needs L >= 0 bases (got -1)", "--clip-out lists the contigs a filter keeps",
    "--clip-percentile / --min-size need a distance", "--clip-percentile / --min-size run on one GPU",
    "--clip-percentile / --min-size support --method",
    "--sweep-out lists the runs of a sweep", "--silhouette scores a clustering", "it cannot be combined with --kmedoids 3",
    "needs two integers separated by a colon (got 'x')", "<= number of contigs (got 3:2)", "<= number of contigs (got 1:3)",
    "--kmedoids writes cluster labels to -o", "--kmedoids-sweep writes cluster labels to -o",
    "--kmedoids writes one label per contig as text", "--kmedoids-sweep writes one label per contig as text",
    "--kmedoids needs a distance", "--kmedoids-sweep needs a distance", "--kmedoids K needs 1 <= K <= number of contigs (got 0)",
    "--kmedoids-iter needs at least 1 iteration (got 0)", "--kmedoids runs on one GPU", "--kmedoids-sweep runs on one GPU",
    "--kmedoids supports --method", "--kmedoids-sweep supports --method",
    "--tsne writes an embedding and --knn a neighbour graph", "--tsne writes n x 2 coordinates as text", "--tsne needs a distance",
    "at most 341 (got 0.5)", "at most 341 (got 400)", "--tsne-iter needs at least 1 iteration (got 0)", "--tsne runs on one GPU",
    "--tsne supports --method",
    "--knn K needs 1 <= K <= 1024 (got 0)", "--knn K needs 1 <= K <= 1024 (got 2000)", "--knn writes a neighbour graph, not a matrix container",
    "--knn supports --method",
]


def command_lines(factors):
    """every element of the product as an argument list, in itertools.product order of the factor lists as the file names them"""
    for parts in itertools.product(*factors.values()):
        yield ["-i", "x.fa"] + [word for part in parts for word in part]


def main():
    from phyloligo_amd import phyloligo as P
    os.environ.pop("WORLD_SIZE", None)
    messages, index = [], []
    for argv in command_lines(FACTORS):
        params = P.get_cmd(argv)
        outcome = next((r for r in (P._clip_refused(params), P._kmedoids_refused(params), P._tsne_refused(params), P._knn_refused(params)) if r),
                       None)
        if outcome not in messages:
            messages.append(outcome)
        index.append(messages.index(outcome))
    missing = [s for s in SITES if not any(m is not None and s in m for m in messages)]
    assert not missing, "refusal sites that no command line reaches: %r" % missing
    path = os.path.join(ROOT, "tests", "golden", "cli_refusals.json")
    with open(path, "w") as fh:
        json.dump({"factors": FACTORS, "messages": messages, "index": index}, fh, separators=(",", ":"))
        fh.write("\n")
    print("%s: %d command lines, %d distinct outcomes" % (path, len(index), len(messages)))


if __name__ == "__main__":
    main()
