#!/usr/bin/env python3
"""Host-side mirror of the reference's dispatcher interface for the all-by-all distance path.

Same names, argument order and error behaviour as /root/reference/phylopackage/bin/phyloligo.py:
    compute_frequencies(...)  :980-997      compute_distances(...)  :536-553
    get_cmd()                 :1000-1034    main()                  :1036-1068
so a script written against the reference runs unchanged; every `--method` value executes the
HIP kernels of libphyloligo_amd.so (there is no joblib/scoop task farm and no CPU fallback).
"""
import argparse
import os
import sys
import time

import numpy as np

from . import api
from ._lib import METRICS, PO_KNN_MAX_K, STRANDS

_ctx = None
LAST_INGEST = None       # phase -> ms of the last compute_frequencies() when INGEST_PHASES is set (--json-stats, bench.py)
INGEST_PHASES = False    # time every step of compute_frequencies() (synchronises the device between steps)


def _timing(text):
    """PO_CLI_TIMING=1: phase times on stderr (tools/container_writer_bench.py compares the multi-rank writer with the
    single-process one); silent otherwise - the reference prints nothing of the kind."""
    if os.environ.get("PO_CLI_TIMING") == "1":
        sys.stderr.write("phyloligo_amd timing: %s\n" % text)


def _context(device=None):
    """the process's one context; the first call chooses its device (LOCAL_RANK unless a rank names its own)"""
    global _ctx
    if _ctx is None:
        _ctx = api.Context(int(os.environ.get("LOCAL_RANK", "0")) if device is None else device)
    return _ctx


class ProfileMatrix(np.ndarray):
    """float64[N, 4^k] frequencies exactly as compute_frequencies_joblib returns them
    (phyloligo.py:847-877), carrying the exact integer profile they were derived from."""

    def __new__(cls, freq, counts=None, totals=None, titles=None, lengths=None):
        obj = np.asarray(freq, dtype=np.float64).view(cls)
        obj.counts, obj.totals, obj.titles = counts, totals, titles
        obj.lengths = lengths                            # int64[N]: bases of every record as ingested (--min-size)
        return obj

    def __array_finalize__(self, obj):
        if obj is None:
            return
        self.counts = self.totals = self.titles = self.lengths = None   # slices/copies are plain frequencies


def read_fasta(genome):
    """(seq uint8, offsets uint64[n+1], titles) of a multi-FASTA file, record order preserved."""
    size = os.path.getsize(genome)
    if size == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64), []
    data = np.memmap(genome, dtype=np.uint8, mode="r")
    try:
        return api.fasta_index(data)
    finally:
        del data


def read_fasta_device(genome, phases=None):
    """The same records through the on-device parser: (seq CUDA uint8, offsets CUDA int64[n+1], titles), or None when
    the file has the one construct that parser leaves to the host (tabs on sequence lines) or is empty."""
    from ._lib import PhyloligoError, PO_EUNSUPPORTED
    if os.path.getsize(genome) == 0 or "torch" not in sys.modules:      # the device buffers of this path are torch tensors
        return None
    try:
        return api.fasta_index_dev(_context(), genome, phases)
    except PhyloligoError as exc:
        if exc.status == PO_EUNSUPPORTED:
            return None
        raise


def compute_frequencies(mthdrun, large, genome, pattern, strand, distchunksize=250, threads_max=4, workdir="."):
    """phyloligo.py:980-997.  Returns (frequencies, freq_name); freq_name is always None here
    (no on-disk frequency container: the count matrix lives in HBM / host memory)."""
    global LAST_INGEST
    if mthdrun not in ("joblib", "scoop", "hip"):
        print("Method {} is unknown".format(mthdrun), file=sys.stderr)      # :995, no exit
        return None, None
    if strand not in STRANDS:                                                # select_strand :146-148
        print("Error, strand parameter of selectd_strand() should be choose from {'both', 'minus', 'plus'}",
              file=sys.stderr)
        sys.exit(1)
    phases = {} if INGEST_PHASES else None
    t_last = [time.perf_counter()]

    def mark(name, sync=None):
        if phases is not None:
            if sync is not None:
                sync()
            now = time.perf_counter()
            phases[name] = phases.get(name, 0.0) + (now - t_last[0]) * 1e3
            t_last[0] = now

    ctx = _context()
    mark("context_ms")
    ingest = read_fasta_device(genome, phases)
    mark("fasta_index_other_ms")
    if phases is not None:                 # (the steps inside were timed there: only what is left of the call counts here)
        phases["fasta_index_other_ms"] -= sum(phases.get(k, 0.0) for k in ("file_read_ms", "file_h2d_ms", "fasta_scan_ms", "device_alloc_ms",
                                                                             "fasta_extract_ms", "title_spans_d2h_ms"))
    if ingest is not None:
        # file bytes -> HBM -> records -> profiles -> frequencies without the sequence ever being walked on the host
        import torch
        d_seq, d_off, titles = ingest
        d_counts, d_totals = ctx.count_profiles(d_seq, d_off, pattern, strand)
        mark("stage1_ms", torch.cuda.synchronize)
        d_freq = ctx.frequencies(d_counts, d_totals)
        mark("count2freq_ms", torch.cuda.synchronize)
        freq = d_freq.cpu().numpy()
        mark("frequencies_d2h_ms")
        counts = d_counts.cpu().numpy().view(np.uint32)
        totals = d_totals.cpu().numpy().view(np.uint64)
        lengths = np.diff(d_off.cpu().numpy().astype(np.int64))
        mark("counts_d2h_ms")
    else:
        seq, offsets, titles = read_fasta(genome)
        mark("host_parse_ms")
        counts, totals = ctx.count_profiles(seq, offsets, pattern, strand)
        mark("stage1_host_pointers_ms")
        freq = ctx.frequencies(counts, totals)
        lengths = np.diff(np.asarray(offsets).astype(np.int64))
        mark("count2freq_host_pointers_ms")
    result = ProfileMatrix(freq, counts, totals, titles, lengths)
    mark("wrap_ms")
    LAST_INGEST = phases
    return result, None


def _reserve_file(fd, size):
    """Size the container and, where the filesystem can, allocate its blocks up front: parallel pwrite into a preallocated
    file measured 12.2-12.6 GB/s against 10.5-10.9 GB/s into a merely truncated one (gpurun box, overlay on ext4, 4 GB,
    tools/exp/pwrite_rate.py).  fallocate(2) itself, not posix_fallocate: glibc's emulation for filesystems without
    it writes into every block."""
    if size > 0:
        try:
            import ctypes
            libc = ctypes.CDLL(None, use_errno=True)
            libc.fallocate.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
            libc.fallocate.restype = ctypes.c_int
            if libc.fallocate(fd, 0, 0, size) == 0:
                return
        except (OSError, AttributeError):
            pass
    if os.fstat(fd).st_size < size:          # never shorten: an HDF5 file keeps whatever the library has put behind the data
        os.ftruncate(fd, size)


def _open_raw_container(out_file, size):
    """A raw container of exactly `size` bytes, every one of which the caller is going to write.  An existing file is reused, not
    truncated to nothing first: O_TRUNC on a 10 GB file whose pages sit in the page cache took 0.72 - 0.78 s on the gpurun box
    (as long as removing it), overwriting it in place nothing beyond the write (tools/exp/overwrite_cost.py) - a second run of the
    same command went from 2.1 s to 1.4 s.  Only a longer file is cut back, to the new size."""
    fd = os.open(out_file, os.O_RDWR | os.O_CREAT, 0o666)
    try:
        if os.fstat(fd).st_size > size:
            os.ftruncate(fd, size)
        _reserve_file(fd, size)
    except BaseException:
        os.close(fd)
        raise
    return fd


def _pwrite_rows(fd, host, row0, col0, n, threads=8, base=0):
    """host[R, C] float32 (unit inner stride) -> rows row0.., columns col0.. of the n x n float32 matrix that starts at byte
    `base` of the file behind fd (0: the raw container; the data offset of the "distances" dataset: the HDF5 container)
    (po_pwrite_rows: parallel pwrite in C, no Python per row)."""
    import ctypes
    from . import _lib
    rows, cols = host.shape
    if rows == 0 or cols == 0:
        return
    assert host.dtype == np.float32 and host.strides[1] == 4 and host.strides[0] >= cols * 4
    _lib.check(_lib.load().po_pwrite_rows(fd, ctypes.c_void_p(host.ctypes.data), rows, cols * 4, host.strides[0],
                                          base + (row0 * n + col0) * 4, n * 4, threads))


def _bc_memmap_diagonal(buf, lo, hi, empty):
    """The reference's memmap variant evaluates Bray-Curtis through BC_loc -> phylodist.BC -> pairwise_distances(X, X[s],
    metric="braycurtis") (bin/phyloligo.py:214-217, core/phylodist.py:76-79), i.e. SciPy cdist: an EMPTY profile against
    itself is 0/0 = nan there, where the joblib variant (pdist + squareform, :381) has an exact 0 on the diagonal
    (tests/golden/memmap.npz vs distances.npz).  The container follows the variant it stands for."""
    for i in empty:
        if lo <= i < hi:
            buf[i - lo, i] = np.nan


def _write_raw_f32(out_file, n, rows, writers=8, fix=None, base=None):
    """The container of compute_distances_memmap (phyloligo.py:394-427): headerless row-major float32[n, n] (:413), the
    file phyloligo_comparemat.py:16-24 and phyloselect.py:606-614 read back.  Row blocks come off the device into
    one of two reusable host buffers and go to the file through po_pwrite_rows (parallel pwrite) on a background thread
    while the next block is computed and copied: no second ndarray, no page faults on a file mapping (numpy.memmap
    assignment measured ~3 GB/s).  fix(buf, lo, hi): host-side touch-up of a finished row block before it is written."""
    import concurrent.futures as cf
    # base is None: a new raw container.  base = byte offset: the matrix goes into an EXISTING file from there on (the HDF5
    # container: created and sized by libhdf5, phyloligo_amd/hdf5.py)
    fd = os.open(out_file, os.O_RDWR) if base is not None else _open_raw_container(out_file, n * n * 4)
    try:
        # blocks allocated up front either way (fallocate keeps what libhdf5 has already written at the head of its file)
        if base is not None:
            _reserve_file(fd, base + n * n * 4)
        if n == 0:
            return
        step = min(n, _row_chunk(n, 4, budget=512 << 20))
        bufs = [np.empty((step, n), dtype=np.float32) for _ in range(2 if step < n else 1)]
        pending = [None for _ in bufs]
        with cf.ThreadPoolExecutor(max_workers=1) as pool:       # one submitter; the parallelism is inside po_pwrite_rows
            for k, lo in enumerate(range(0, n, step)):
                hi = min(n, lo + step)
                which = k % len(bufs)
                if pending[which] is not None:                   # the block written from this buffer two rounds ago
                    pending[which].result()
                buf = bufs[which][:hi - lo]
                rows(lo, hi, "float32", lo == 0 and hi == n, out=buf)
                if fix is not None:
                    fix(buf, lo, hi)
                pending[which] = pool.submit(_pwrite_rows, fd, buf, lo, 0, n, writers, base or 0)
            for f in pending:
                if f is not None:
                    f.result()
    finally:
        os.close(fd)


_SINGLE_CALL_BYTES = 4 << 30      # larger float64 matrices are computed and copied in row blocks


def _row_chunk(n, itemsize, budget=1 << 30):
    return max(128, (budget // max(1, n * itemsize)) // 128 * 128)


def _hdf5_or_refuse(speak=True):
    """the HDF5 writer, or exit 1 where this system has no libhdf5 for --large h5py"""
    from . import hdf5
    if not hdf5.available():
        refuse("Error, --large h5py needs libhdf5 (>= 1.10), which was not found on this system", speak)
    return hdf5


def compute_distances(mthdrun, large, frequencies, freq_name, out_file, dist, threads_max=4, freqchunksize=250,
                      workdir="."):
    """phyloligo.py:536-553.  `--large None`: returns the float64[N,N] matrix (main writes it).
    `--large memmap`: writes the headerless float32 row-major matrix to out_file as
    compute_distances_memmap does (:394-427, container dtype :413) and returns None.
    `--large h5py`: writes the HDF5 file of compute_distances_h5py / join_distance_results (:456-534): one float32 dataset
    "distances" of shape (N, N), and returns None."""
    return _distances(mthdrun, large, frequencies, out_file, dist)[0]


def _distances(mthdrun, large, frequencies, out_file, dist):
    """compute_distances() and, for --json-stats, the PoStats of its first stage-2 call: (result, stats or None)"""
    if mthdrun not in ("joblib", "scoop", "hip"):
        print("Error, method {} is not implemented for pairwise distances computation".format(mthdrun), file=sys.stderr)
        return None, None
    if dist not in METRICS:                                                  # :383-385
        print("Error, unknown metric methodfor joblib: {}".format(dist), file=sys.stderr)
        sys.exit(1)
    if large == "h5py" and mthdrun != "scoop":
        hdf5 = _hdf5_or_refuse()
    ctx = _context()
    counts = getattr(frequencies, "counts", None)
    totals = getattr(frequencies, "totals", None)
    n = frequencies.shape[0]
    if mthdrun == "scoop":                   # compute_distances_scoop (:313-362) has no --large variants
        large = "None"
    # The reference computes from the array it is handed.  The integer profiles riding on a ProfileMatrix are only
    # a shortcut while they still ARE that array: in-place edits (frequencies *= w, frequencies[mask] = 0, ...)
    # keep the attributes, so check count/total == array bit for bit and otherwise go by the array's values.
    if counts is not None and (counts.shape != frequencies.shape or
                               not np.array_equal(ctx.frequencies(counts, totals), np.asarray(frequencies))):
        counts = totals = None

    first = []                               # the stats of the first stage-2 call

    def rows(lo, hi, dtype, symmetric, out=None):
        if counts is not None:
            res, st = ctx.pairwise(counts, totals, dist, lo, hi, dtype=dtype, symmetric=symmetric, out=out, want_stats=True)
        else:
            res, st = ctx.pairwise_freq(np.asarray(frequencies, dtype=np.float64), dist, lo, hi, dtype=dtype,
                                        symmetric=symmetric, out=out, want_stats=True)
        if not first:
            first.append(dict(st, rows=[int(lo), int(hi)]))
        return res

    if large in ("memmap", "h5py"):
        fix = None
        if dist == "BC":                     # BC_loc and BC_h5py both go through phylodist.BC (SciPy cdist): see _bc_memmap_diagonal
            empty = np.flatnonzero(~np.asarray(frequencies).any(axis=1))
            if empty.size:
                fix = lambda buf, lo, hi: _bc_memmap_diagonal(buf, lo, hi, empty)      # noqa: E731
        base = None
        if large == "h5py":
            # join_distance_results (:456-478): ONE dataset "distances", (N, N), float32.  libhdf5 creates and sizes the file; the
            # matrix then goes into the dataset's contiguous data range exactly as it goes into the raw container
            base = hdf5.create_f32_dataset(out_file, "distances", n, n)
        _write_raw_f32(out_file, n, rows, fix=fix, base=base)
        return None, (first[0] if first else None)
    if n * n * 8 <= _SINGLE_CALL_BYTES:
        return rows(0, n, "float64", True), first[0]
    res = np.empty((n, n), dtype=np.float64)
    step = _row_chunk(n, 8)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        rows(lo, hi, "float64", False, out=res[lo:hi])          # straight into the result: no per-block ndarray
    return res, (first[0] if first else None)


def get_cmd(argv=None):
    """phyloligo.py:1000-1034, option for option.  -k and -p share dest="pattern": whichever comes
    last on the command line wins; with neither the int default 4 is used (-> "1111")."""
    parser = argparse.ArgumentParser(prog="phyloligo.py")
    parser.add_argument("-i", "--assembly", action="store", required=True, dest="genome",
                        help="multifasta of the genome assembly")
    parser.add_argument("-k", "--lgMot", action="store", dest="pattern", default=4, type=int,
                        help="word lenght / kmer length / k [default:%(default)d]")
    parser.add_argument("-s", "--strand", action="store", dest="strand", default="both",
                        choices=["both", "plus", "minus"],
                        help="strand used to compute microcomposition. [default:%(default)s]")
    parser.add_argument("-d", "--distance", action="store", dest="dist", default="Eucl",
                        choices=["Eucl", "JSD", "KT", "BC", "SC"],
                        help="how to compute distance between two signatures : Eucl : Euclidean[default:%(default)s], "
                             "JSD : Jensen-Shannon divergence, KT: Kendall's tau, BC: Bray-Curtis, SC:Spearman Correlation")
    parser.add_argument("--freq-chunk-size", action="store", dest="freqchunksize", type=int, default=250,
                        help="accepted for compatibility (scoop chunking; unused on the GPU)")
    parser.add_argument("--dist-chunk-size", action="store", dest="distchunksize", type=int, default=250,
                        help="accepted for compatibility (scoop chunking; unused on the GPU)")
    parser.add_argument("--method", action="store", choices=["scoop", "joblib", "hip"], default="joblib",
                        dest="mthdrun", required=True,
                        help="kept from the reference; every value runs the MI355X HIP path")
    parser.add_argument("--large", action="store", dest="large", choices=["None", "memmap", "h5py"], default="None",
                        help="memmap: write the matrix as raw float32 instead of text")
    parser.add_argument("-c", "--cpu", action="store", dest="threads_max", type=int, default=4,
                        help="accepted for compatibility (host threads are not the compute resource)")
    parser.add_argument("-o", "--out", action="store", dest="out_file", default="phyloligo.out",
                        help="output file[default:%(default)s]")
    parser.add_argument("-q", "--outfreq", action="store", dest="out_freq_file",
                        help="kmer frequencies output file")
    parser.add_argument("-w", "--workdir", action="store", dest="workdir", default=".", help="working directory")
    parser.add_argument("-p", "--pattern", action="store", dest="pattern", default="1111",
                        help="spaced-word pattern string, only containing 1s and 0s, i.e. '100101001', default='1111'")
    parser.add_argument("--json-stats", action="store", dest="json_stats", default=None,
                        help="not in the reference (SURVEY section 5): write sizes, phase times and the stage-2 kernel of this run "
                             "to this file as JSON; the five progress lines on stdout stay as they are")
    parser.add_argument("--gpus", action="store", dest="gpus", type=int, default=1,
                        help="not in the reference: GPUs of this node to use, one process each (python -m phyloligo_amd starts "
                             "the ranks itself; the analogue of the reference fanning out to -c joblib workers) [default:%(default)d]")
    parser.add_argument("--knn", action="store", dest="knn", type=int, default=None, metavar="K",
                        help="not in the reference: write the K nearest neighbours of every contig (1 <= K <= 1024) to -o as a "
                             "sparse CSR graph (scipy.sparse.load_npz reads it; row i: i itself, then its neighbours by distance) "
                             "instead of the N x N matrix; float64 values")
    parser.add_argument("--tsne", action="store", dest="tsne", type=float, default=None, metavar="PERPLEXITY",
                        help="not in the reference's phyloligo.py: embed the contigs in 2-D with t-SNE at this perplexity, from the "
                             "int(3 * PERPLEXITY + 1) nearest neighbours of every contig, and write the n x 2 coordinates to -o as "
                             "text (what phyloselect.py -t -p PERPLEXITY computes from the whole matrix); 1 <= PERPLEXITY <= 341")
    parser.add_argument("--tsne-seed", action="store", dest="tsne_seed", type=int, default=0,
                        help="with --tsne: seed of the random start, phyloselect.py's random_state [default:%(default)d]")
    parser.add_argument("--tsne-iter", action="store", dest="tsne_iter", type=int, default=1000,
                        help="with --tsne: most iterations of the optimiser, scikit-learn's max_iter [default:%(default)d]")
    parser.add_argument("--kmedoids", action="store", dest="kmedoids", type=int, default=None, metavar="K",
                        help="not in the reference's phyloligo.py: cluster the contigs into K groups with k-medoids on the N x N "
                             "matrix, which stays in GPU memory, and write one cluster label per contig to -o, in input order "
                             "(what phyloselect.py -m kmedoids computes from the matrix file); 1 <= K <= N")
    parser.add_argument("--kmedoids-iter", action="store", dest="kmedoids_iter", type=int, default=300,
                        help="with --kmedoids: most iterations, the reference's max_iter [default:%(default)d]")
    parser.add_argument("--kmedoids-dtype", action="store", dest="kmedoids_dtype", choices=["float64", "float32"], default="float64",
                        help="with --kmedoids: element type of the matrix in GPU memory; float32 takes half the memory, sums are "
                             "float64 either way [default:%(default)s]")
    parser.add_argument("--kmedoids-sweep", action="store", dest="kmedoids_sweep", default=None, metavar="LO:HI",
                        help="not in the reference's phyloligo.py: compute the matrix once, cluster it with k-medoids for every K in "
                             "LO..HI, score every clustering by its mean silhouette and write the labels of the best K to -o (the "
                             "largest mean wins, a tie goes to the smaller K): phyloselect.py --interactive's \"change nbk\" loop "
                             "without the person; 2 <= LO <= HI <= N; honours --kmedoids-iter and --kmedoids-dtype")
    parser.add_argument("--sweep-out", action="store", dest="sweep_out", default=None, metavar="FILE",
                        help="with --kmedoids-sweep: write one tab-separated line per K to FILE: K, iterations, converged, empty "
                             "clusters, inertia, mean silhouette and the cluster sizes")
    parser.add_argument("--silhouette", action="store", dest="silhouette", default=None, metavar="FILE",
                        help="with --kmedoids or --kmedoids-sweep: write the silhouette value of every contig for the labels written to "
                             "-o to FILE, one per line in input order (sklearn.metrics.silhouette_samples on the matrix in GPU memory; "
                             "a value near 0 or below marks a contig between two clusters)")
    parser.add_argument("--dbscan", action="store", dest="dbscan", type=float, default=None, metavar="EPS",
                        help="not in the reference's phyloligo.py: cluster the contigs by density with DBSCAN on the N x N matrix, "
                             "which stays in GPU memory, and write one cluster label per contig to -o, in input order; two contigs "
                             "are neighbours when their distance is at most EPS, and a contig that belongs to no cluster gets -1 "
                             "(what phyloselect.py -m hdbscan sends to data_fasta_unclust.fa); the labels are those of "
                             "sklearn.cluster.DBSCAN(eps=EPS, metric=\"precomputed\"); EPS >= 0")
    parser.add_argument("--dbscan-min-samples", action="store", dest="dbscan_min_samples", type=int, default=5, metavar="M",
                        help="with --dbscan: a contig with at least M contigs within EPS, itself included, is a core contig, "
                             "scikit-learn's min_samples [default:%(default)d]")
    parser.add_argument("--dbscan-dtype", action="store", dest="dbscan_dtype", choices=["float64", "float32"], default="float64",
                        help="with --dbscan: element type of the matrix in GPU memory; float32 takes half the memory "
                             "[default:%(default)s]")
    parser.add_argument("--dbscan-core", action="store", dest="dbscan_core", default=None, metavar="FILE",
                        help="with --dbscan: write one line per contig to FILE, 1 for a core contig and 0 for any other")
    parser.add_argument("--clip-percentile", action="store", dest="clip_percentile", type=float, default=1.0, metavar="P",
                        help="not in the reference's phyloligo.py: before anything is computed from the matrix, drop the contigs whose "
                             "median distance to all contigs lies above the P quantile of those medians (what phyloselect.R -c P "
                             "does to the matrix file; its help suggests 0.97); the medians are taken in GPU memory and the run "
                             "continues as if the input held only the kept contigs; 0 <= P <= 1 [default:%(default)g = off]")
    parser.add_argument("--min-size", action="store", dest="min_size", type=int, default=0, metavar="L",
                        help="after --clip-percentile: drop the contigs shorter than L bases (phyloselect.R -s L) "
                             "[default:%(default)d = off]")
    parser.add_argument("--clip-out", action="store", dest="clip_out", default=None, metavar="FILE",
                        help="with --clip-percentile / --min-size: write one line per kept contig to FILE: its 0-based index in the "
                             "input, the first word of its title, its length and its median distance, tab separated")
    params = parser.parse_args(argv)
    params.workdir = os.path.abspath(params.workdir)
    return params


# ---- refusals: the rules every mode shares, stated once --------------------------------------------------------------------------------
# A mode is refused, in this order, by: its own checks of what it was combined with (`first`); --large, when it writes `writes` to
# -o and no matrix container; -d KT, which is a correlation, `kt` saying why that matters to the mode; the checks of its own values
# (`values`); more than one rank, `ranks` naming what would have to be spread over them; --method scoop.  A rule whose wording
# the mode does not give does not apply to it.  `first` and `values` are iterables of reasons: the first one counts.
def _first_reason(params, environ, who, first=(), writes=None, kt=None, values=(), ranks=None):
    s = "" if " / " in who else "s"                      # "--clip-percentile / --min-size need", "--tsne needs"
    for reason in first:
        return reason
    if writes is not None and params.large != "None":
        return "Error, %s writes %s, not a matrix container: it cannot be combined with --large %s" % (who, writes, params.large)
    if kt is not None and params.dist == "KT":
        return "Error, %s need%s a distance: -d KT is a correlation (%s)" % (who, s, kt)
    for reason in values:
        return reason
    if ranks is not None and (params.gpus > 1 or int(environ.get("WORLD_SIZE", "1")) > 1):
        return "Error, %s run%s on one GPU: %s over several ranks (--gpus N > 1) is out of scope" % (who, s, ranks)
    if params.mthdrun not in ("joblib", "hip"):
        return "Error, %s support%s --method joblib|hip" % (who, s)
    return None


def _clip_active(params):
    return getattr(params, "clip_percentile", 1.0) != 1 or getattr(params, "min_size", 0) != 0


def _clip_refused(params, environ=os.environ):
    """the reason --clip-percentile / --min-size cannot run with these options, or None"""
    p, size = getattr(params, "clip_percentile", 1.0), getattr(params, "min_size", 0)
    if not 0.0 <= p <= 1.0:
        return "Error, --clip-percentile P needs 0 <= P <= 1 (got %g)" % p
    if size < 0:
        return "Error, --min-size L needs L >= 0 bases (got %d)" % size
    if not _clip_active(params):
        if getattr(params, "clip_out", None) is not None:
            return "Error, --clip-out lists the contigs a filter keeps: give --clip-percentile P < 1 or --min-size L > 0 with it"
        return None
    return _first_reason(params, environ, "--clip-percentile / --min-size", kt="a large median does not mean distant", ranks="a clip")


def _knn_refused(params, environ=os.environ):
    """the reason --knn cannot run with these options, or None"""
    if params.knn is None:
        return None

    def first():
        if not 1 <= params.knn <= PO_KNN_MAX_K:
            yield "Error, --knn K needs 1 <= K <= %d (got %d)" % (PO_KNN_MAX_K, params.knn)

    return _first_reason(params, environ, "--knn", first(), writes="a neighbour graph")


def _tsne_refused(params, environ=os.environ):
    """the reason --tsne cannot run with these options, or None"""
    if getattr(params, "tsne", None) is None:
        return None

    def first():
        if params.knn is not None:
            yield "Error, --tsne writes an embedding and --knn a neighbour graph to -o: give one of them"

    def values():
        if not params.tsne >= 1.0 or int(3.0 * params.tsne + 1) > PO_KNN_MAX_K:
            yield ("Error, --tsne PERPLEXITY needs 1 <= PERPLEXITY and int(3 * PERPLEXITY + 1) <= %d neighbours, i.e. at most %d (got %g)"
                   % (PO_KNN_MAX_K, (PO_KNN_MAX_K - 1) // 3, params.tsne))
        if params.tsne_iter < 1:
            yield "Error, --tsne-iter needs at least 1 iteration (got %d)" % params.tsne_iter

    return _first_reason(params, environ, "--tsne", first(), writes="n x 2 coordinates as text",
                         kt="its neighbour lists are ordered descending", values=values(), ranks="an embedding")


def parse_sweep(text):
    """(LO, HI) of --kmedoids-sweep LO:HI, 2 <= LO <= HI; ValueError says what is wrong"""
    parts = str(text).split(":")
    try:
        if len(parts) != 2:
            raise ValueError
        lo, hi = (int(q) for q in parts)
    except ValueError:
        raise ValueError("--kmedoids-sweep LO:HI needs two integers separated by a colon (got %r)" % (text,)) from None
    if not 2 <= lo <= hi:
        raise ValueError("--kmedoids-sweep LO:HI needs 2 <= LO <= HI <= number of contigs (got %d:%d)" % (lo, hi))
    return lo, hi


def _sweep_range(params):
    """(LO, HI) of a --kmedoids-sweep run that passed _kmedoids_refused, else None"""
    text = getattr(params, "kmedoids_sweep", None)
    return None if text is None else parse_sweep(text)


def _kmedoids_refused(params, environ=os.environ):
    """the reason --kmedoids / --kmedoids-sweep (and --silhouette, --sweep-out with them) cannot run with these options, or None"""
    sweep = getattr(params, "kmedoids_sweep", None)
    if getattr(params, "sweep_out", None) is not None and sweep is None:
        return "Error, --sweep-out lists the runs of a sweep: give --kmedoids-sweep LO:HI with it"
    if getattr(params, "kmedoids", None) is None and sweep is None:
        if getattr(params, "silhouette", None) is not None:
            return "Error, --silhouette scores a clustering: give --kmedoids K or --kmedoids-sweep LO:HI with it"
        return None
    who = "--kmedoids" if sweep is None else "--kmedoids-sweep"

    def first():
        if sweep is not None:
            if params.kmedoids is not None:
                yield "Error, --kmedoids-sweep tries every K of its range: it cannot be combined with --kmedoids %d" % params.kmedoids
            try:
                parse_sweep(sweep)
            except ValueError as e:
                yield "Error, %s" % e
        if params.knn is not None or getattr(params, "tsne", None) is not None:
            yield "Error, %s writes cluster labels to -o, --knn a neighbour graph and --tsne an embedding: give one of them" % who

    def values():
        if sweep is None and params.kmedoids < 1:
            yield "Error, --kmedoids K needs 1 <= K <= number of contigs (got %d)" % params.kmedoids
        if params.kmedoids_iter < 1:
            yield "Error, --kmedoids-iter needs at least 1 iteration (got %d)" % params.kmedoids_iter

    return _first_reason(params, environ, who, first(), writes="one label per contig as text", kt="larger means closer",
                         values=values(), ranks="clustering")


def _dbscan_refused(params, environ=os.environ):
    """the reason --dbscan (and --dbscan-core with it) cannot run with these options, or None"""
    eps = getattr(params, "dbscan", None)
    if eps is None:
        if getattr(params, "dbscan_core", None) is not None:
            return "Error, --dbscan-core marks the core contigs of a density clustering: give --dbscan EPS with it"
        return None

    def first():
        if (params.kmedoids is not None or getattr(params, "kmedoids_sweep", None) is not None or params.knn is not None or
                getattr(params, "tsne", None) is not None):
            yield ("Error, --dbscan, --kmedoids and --kmedoids-sweep write cluster labels to -o, --knn a neighbour graph and --tsne an "
                   "embedding: give one of them")

    def values():
        if not eps >= 0.0:
            yield "Error, --dbscan EPS needs a distance EPS >= 0 (got %g)" % eps
        if params.dbscan_min_samples < 1:
            yield "Error, --dbscan-min-samples M needs M >= 1 contigs (got %d)" % params.dbscan_min_samples

    return _first_reason(params, environ, "--dbscan", first(), writes="one label per contig as text", kt="larger means closer",
                         values=values(), ranks="clustering")


def refusal(params, environ=os.environ):
    """the first reason this command line cannot run, or None; a new mode adds its function here, where main() is to ask it"""
    for refused in (_clip_refused, _kmedoids_refused, _dbscan_refused, _tsne_refused, _knn_refused):
        reason = refused(params, environ)
        if reason:
            return reason
    return None


def refuse(reason, speak=True):
    """exit 1 when there is a reason; one process says it on stderr (of several ranks: rank 0)"""
    if reason:
        if speak:
            print(reason, file=sys.stderr)
        sys.exit(1)


def launch_plan(params, environ):
    """What `python -m phyloligo_amd` decides before anything touches torch or the library: (the reason to refuse or None,
    the GPUs asked for, whether torch has to be loaded before the library).  torch comes first exactly where the run keeps the
    matrix in a torch tensor (k-medoids, the sweep, DBSCAN, an active clip) or is one of several ranks: it bundles its own HIP
    runtime, and a process must hold exactly one (_lib.PREFER_NO_TORCH)."""
    needs_torch = (int(environ.get("WORLD_SIZE", "1")) > 1 or params.kmedoids is not None or params.kmedoids_sweep is not None or
                   getattr(params, "dbscan", None) is not None or _clip_active(params))
    return refusal(params, environ), params.gpus, needs_torch


# ---- the modes: what a run computes from the profiles and writes to -o -----------------------------------------------------------------
# A mode is a function (params, frequencies) -> (PO_CLI_TIMING label, the line printed before writing or None, the function that
# writes its output, the stats of its first stage-2 call, its own --json-stats keys).  main() owns everything around it.
def _write_freq(params, frequencies, speak=True):
    """-q: the frequency matrix as text, before the run's own output (frequencies: a function, called only when it is wanted)"""
    if params.out_freq_file and speak:
        print("Writing frequency matrix")
        api.write_mat_text(params.out_freq_file, frequencies())


def _matrix_mode(params, frequencies):
    """the N x N matrix: returned and written as text, or written into its container by compute_distances itself"""
    res, stage2 = _distances(params.mthdrun, params.large, frequencies, params.out_file, params.dist)
    text = not (params.mthdrun in ("joblib", "hip") and params.large != "None")          # :1064
    return ("distances%s" % (" + container" if params.large in ("memmap", "h5py") else ""), "Writing distance matrix" if text else None,
            lambda: api.write_mat_text(params.out_file, res), stage2, {})


def _knn_mode(params, frequencies):
    """--knn in one process: the graph from the integer profiles (po_knn, float64), written to -o"""
    counts, n = frequencies.counts, frequencies.shape[0]
    idx, val, st = _context().knn(counts, frequencies.totals, params.knn, params.dist, "float64", want_stats=True)
    return ("k-NN graph", "Writing distance matrix", lambda: _write_knn(params, counts, idx, val), dict(st, rows=[0, n]),
            {"knn": params.knn, "knn_select_ms": st.get("select_ms")})


def _write_knn(params, counts, idx, val):
    api.write_knn_npz(params.out_file, idx, val, api.knn_self_values(params.dist, val, counts=counts))


def _tsne_mode(params, frequencies):
    """--tsne: the graph as --knn int(3 p + 1) selects it (po_knn, float64), embedded by po_tsne, written to -o as text"""
    n = frequencies.shape[0]
    if n < 4:
        refuse("Error, --tsne needs at least 4 contigs (got %d)" % n)
    ctx = _context()
    idx, val, st = ctx.knn(frequencies.counts, frequencies.totals, api.tsne_neighbours(n, params.tsne), params.dist, "float64", want_stats=True)
    t0 = time.perf_counter()
    try:
        y, ts = ctx.tsne(idx, val, params.tsne, seed=params.tsne_seed, max_iter=params.tsne_iter, want_stats=True, metric=params.dist)
    except api._lib.PhyloligoError as e:
        refuse("Error, --tsne: %s" % e)
    return ("k-NN graph + t-SNE", "Writing t-SNE embedding", lambda: np.savetxt(params.out_file, y), dict(st, rows=[0, n]),
            {"tsne_ms": (time.perf_counter() - t0) * 1e3, "tsne_iterations": ts["iterations"], "tsne_kl": ts["kl"], "tsne_perplexity": params.tsne})


def _device_matrix(params, ctx, frequencies, f32, who, half):
    """the dense n x n matrix of the run's metric in device memory (po_pairwise_dev), rows on whole 128-byte lines: (buffer, ld,
    stage-2 stats); exits with the sizes, and `half` as what would take half of them, when it does not fit"""
    import torch
    n = frequencies.shape[0]
    dev = torch.device("cuda", ctx.device)
    esz = 4 if f32 else 8
    name = "float32" if f32 else "float64"
    ld = (n + 128 // esz - 1) // (128 // esz) * (128 // esz)
    try:
        buf = torch.empty((n, ld), dtype=torch.float32 if f32 else torch.float64, device=dev)
    except torch.cuda.OutOfMemoryError:
        refuse("Error, %s: the %d x %d %s matrix (%.1f GB) does not fit the memory of the GPU%s"
               % (who, n, n, name, n * ld * esz / 1e9, "" if f32 else "; %s takes half (%.1f GB)" % (half, n * ld * 4 / 1e9)))
    d_counts = torch.from_numpy(np.ascontiguousarray(frequencies.counts).view(np.int32)).to(dev)
    d_totals = torch.from_numpy(np.ascontiguousarray(frequencies.totals).view(np.int64)).to(dev)
    _, st = ctx.pairwise(d_counts, d_totals, params.dist, dtype=name, out=buf, want_stats=True)
    torch.cuda.synchronize(dev)
    return buf, ld, st


def _clip(params, frequencies):
    """--clip-percentile / --min-size (bin/phyloselect.R:339-357): the dense matrix computed into device memory, its row medians
    taken there (po_row_medians_dev), the two filters applied to those n doubles on the host; returns the profiles of the kept
    records, in input order - everything after this runs as it would on an input that held only them - and the clip_* keys of
    --json-stats."""
    import torch
    print("Clipping outlier contigs")
    n = frequencies.shape[0]
    ctx = _context()
    f32 = (params.large in ("memmap", "h5py") or params.kmedoids_dtype == "float32" or      # the run's output is float32 data anyway
           getattr(params, "dbscan_dtype", "float64") == "float32")
    t0 = time.perf_counter()
    medians = np.zeros(0)
    t1 = t2 = t0
    if n:
        buf, _, _ = _device_matrix(params, ctx, frequencies, f32, "--clip-percentile", "a float32 matrix")
        t1 = time.perf_counter()
        d_med = ctx.row_medians(buf[:, :n])
        torch.cuda.synchronize(d_med.device)
        t2 = time.perf_counter()
        medians = d_med.cpu().numpy()
        del buf, d_med
        torch.cuda.empty_cache()                         # the matrix of the kept records is computed afresh: give the room back
    lengths = np.asarray(frequencies.lengths, dtype=np.int64)
    p, size = params.clip_percentile, params.min_size
    try:
        by_median = api.clip_keep(medians, p)
        keep = api.clip_keep(medians, p, lengths, size)
        threshold = api.clip_threshold(medians, p) if p != 1 and n else None
    except api._lib.PhyloligoError as e:
        refuse("Error, --clip-percentile: %s" % e)
    stats = {"clip_percentile": p, "clip_min_size": size, "clip_threshold": threshold, "clip_kept": int(keep.size),
             "clip_dropped_by_median": int(n - by_median.size), "clip_dropped_by_size": int(by_median.size - keep.size),
             "clip_medians_ms": (t2 - t1) * 1e3, "clip_matrix_ms": (t1 - t0) * 1e3, "clip_dtype": "float32" if f32 else "float64",
             "clip_input_contigs": int(n)}
    if keep.size < 1:
        refuse("Error, --clip-percentile %g --min-size %d keep none of the %d contigs" % (p, size, n))
    titles = frequencies.titles
    sweep = _sweep_range(params)
    downstream_runs = ((params.kmedoids is None or params.kmedoids <= keep.size) and (sweep is None or sweep[1] <= keep.size) and
                       (params.tsne is None or keep.size >= 4) and (params.knn is None or params.knn < keep.size))
    if params.clip_out and downstream_runs:              # (a run its mode refuses for the kept count leaves no file behind)
        with open(params.clip_out, "w") as fh:
            for i in keep:
                words = titles[int(i)].split()
                fh.write("%d\t%s\t%d\t%.17g\n" % (i, words[0] if words else "", lengths[i], medians[i]))
    return ProfileMatrix(np.asarray(frequencies)[keep], frequencies.counts[keep], frequencies.totals[keep],
                         [titles[int(i)] for i in keep], lengths[keep]), stats


def write_labels(path, labels):
    """one integer cluster label per contig, in input order: n lines, each an integer and a line feed"""
    with open(path, "w") as fh:
        fh.write("".join("%d\n" % int(x) for x in labels))


def write_silhouette(path, values):
    """one silhouette value per contig, in input order: n lines, each repr(float(value)) and a line feed"""
    with open(path, "w") as fh:
        fh.write("".join("%r\n" % float(x) for x in values))


SWEEP_COLUMNS = ("K", "iterations", "converged", "empty_clusters", "inertia", "silhouette_mean", "sizes")


def write_sweep_table(path, rows):
    """the runs of a --kmedoids-sweep, one tab-separated line per K behind one '#' header line: K, iterations, converged (1 / 0),
    empty_clusters, repr of the inertia, repr of the mean silhouette, the cluster sizes joined by commas"""
    with open(path, "w") as fh:
        fh.write("#" + "\t".join(SWEEP_COLUMNS) + "\n")
        for r in rows:
            fh.write("%d\t%d\t%d\t%d\t%r\t%r\t%s\n" % (r["K"], r["iterations"], 1 if r["converged"] else 0, r["empty_clusters"],
                                                         float(r["inertia"]), float(r["silhouette_mean"]), ",".join("%d" % x for x in r["sizes"])))


def sweep_best(rows):
    """the row of a sweep that wins: the largest mean silhouette, a tie goes to the smaller K, a NaN never wins; None if all are NaN"""
    best = None
    for r in sorted(rows, key=lambda r: r["K"]):
        m = r["silhouette_mean"]
        if m == m and (best is None or m > best["silhouette_mean"]):
            best = r
    return best


def silhouette_cluster_means(values, labels, k):
    """per cluster the mean of its members' silhouette values (host, float64), None for a cluster without a member"""
    values, labels = np.asarray(values, dtype=np.float64), np.asarray(labels)
    return [float(values[labels == c].mean()) if (labels == c).any() else None for c in range(k)]


def _kmedoids_mode(params, frequencies):
    """--kmedoids / --kmedoids-sweep: the dense matrix computed into device memory (po_pairwise_dev) once, clustered there
    (po_kmedoids_dev) for the one K or for every K of the range, each clustering scored there (po_silhouette_dev) when the run
    reports it; only labels, silhouette values and scalars come back"""
    n = frequencies.shape[0]
    sweep = _sweep_range(params)
    if sweep is None:
        ks_wanted = [params.kmedoids]
        if not 1 <= params.kmedoids <= n:
            refuse("Error, --kmedoids K needs 1 <= K <= number of contigs (got K = %d for %d contigs)" % (params.kmedoids, n))
    else:
        ks_wanted = list(range(sweep[0], sweep[1] + 1))
        if sweep[1] > n:
            refuse("Error, --kmedoids-sweep LO:HI needs 2 <= LO <= HI <= number of contigs (got %d:%d for %d contigs)" % (sweep[0], sweep[1], n))
    ctx = _context()
    buf, _, st = _device_matrix(params, ctx, frequencies, params.kmedoids_dtype == "float32", "--kmedoids", "--kmedoids-dtype float32")
    scored = sweep is not None or params.silhouette is not None or bool(params.json_stats)      # the mean costs one matrix read
    runs = []
    for k in ks_wanted:
        t0 = time.perf_counter()
        try:
            d_labels, medoids, ks = ctx.kmedoids(buf[:, :n], k, max_iter=params.kmedoids_iter, want_stats=True)
        except api._lib.PhyloligoError as e:
            refuse("Error, --kmedoids: %s" % e)
        labels, medoids = d_labels.cpu().numpy(), medoids.cpu().numpy()
        t1 = time.perf_counter()
        run = {"labels": labels, "values": None,
               "stats": {"kmedoids": k, "kmedoids_medoids": [int(x) for x in medoids], "kmedoids_iterations": ks["iterations"],
                         "kmedoids_converged": ks["converged"], "kmedoids_sizes": [int(x) for x in np.bincount(labels, minlength=k)],
                         "kmedoids_ms": (t1 - t0) * 1e3, "kmedoids_inertia": ks["inertia"], "kmedoids_dtype": params.kmedoids_dtype,
                         "kmedoids_phases_ms": {p: ks[p + "_ms"] for p in ("start", "rowsum", "assign", "update")}}}
        mean = float("nan")
        if scored:
            try:
                values, ss = ctx.silhouette(buf[:, :n], d_labels, k, want_stats=True)
                run["values"] = values.cpu().numpy()
                mean = ss["mean"]
                run["stats"].update(silhouette_mean=mean, silhouette_cluster_means=silhouette_cluster_means(run["values"], labels, k),
                                    silhouette_ms=(time.perf_counter() - t1) * 1e3, silhouette_passes=ss["passes"])
            except api._lib.PhyloligoError as e:             # fewer than two clusters with a member: no silhouette
                if sweep is None and params.silhouette is not None:
                    refuse("Error, --silhouette: %s" % e)
                run["stats"].update(silhouette_mean=None, silhouette_cluster_means=None, silhouette_ms=None, silhouette_passes=None)
        run["row"] = {"K": k, "iterations": ks["iterations"], "converged": ks["converged"], "empty_clusters": ks["empty_clusters"],
                      "inertia": ks["inertia"], "silhouette_mean": mean, "sizes": run["stats"]["kmedoids_sizes"]}
        runs.append(run)
    rows = [r["row"] for r in runs]
    if sweep is None:
        best = runs[0]
        stats = best["stats"]
    else:
        won = sweep_best(rows)
        if won is None:
            refuse("Error, --kmedoids-sweep %s: the mean silhouette of every K is NaN (the matrix holds undefined distances)" % params.kmedoids_sweep)
        best = next(r for r in runs if r["row"] is won)
        stats = dict(best["stats"], kmedoids_sweep=rows, kmedoids_sweep_best=won["K"])

    def write():
        write_labels(params.out_file, best["labels"])
        if params.silhouette is not None:
            write_silhouette(params.silhouette, best["values"])
        if sweep is not None and params.sweep_out is not None:
            write_sweep_table(params.sweep_out, rows)

    return "matrix + k-medoids", "Writing cluster labels", write, dict(st, rows=[0, n]), stats


def write_core(path, core):
    """one line per contig, in input order: 1 for a core contig, 0 for any other"""
    with open(path, "w") as fh:
        fh.write("".join("1\n" if x else "0\n" for x in core))


def _dbscan_mode(params, frequencies):
    """--dbscan: the dense matrix computed into device memory (po_pairwise_dev), its neighbourhoods counted and its core contigs
    joined there (po_eps_degrees_dev, po_dbscan_dev); only the labels, the core mask and the degrees come back"""
    n = frequencies.shape[0]
    ctx = _context()
    eps, m = params.dbscan, params.dbscan_min_samples
    if n < 1:
        refuse("Error, --dbscan needs at least 1 contig (got %d)" % n)
    buf, _, st = _device_matrix(params, ctx, frequencies, params.dbscan_dtype == "float32", "--dbscan", "--dbscan-dtype float32")
    t0 = time.perf_counter()
    try:
        d_labels, d_core, ds = ctx.dbscan(buf[:, :n], eps, m, want_stats=True)
        degree = ctx.eps_degrees(buf[:, :n], eps).cpu().numpy() if params.json_stats else None
    except api._lib.PhyloligoError as e:
        refuse("Error, --dbscan: %s" % e)
    labels, core = d_labels.cpu().numpy(), d_core.cpu().numpy()
    stats = {"dbscan_eps": eps, "dbscan_min_samples": m, "dbscan_dtype": params.dbscan_dtype, "dbscan_clusters": ds["clusters"],
             "dbscan_core": ds["core"], "dbscan_border": ds["border"], "dbscan_noise": ds["noise"], "dbscan_passes": ds["passes"],
             "dbscan_sizes": [int(x) for x in np.bincount(labels[labels >= 0], minlength=ds["clusters"])],
             "dbscan_ms": (time.perf_counter() - t0) * 1e3,
             "dbscan_phases_ms": {p: ds[p + "_ms"] for p in ("degree", "label", "finish")}}
    if degree is not None:
        stats.update(dbscan_degree_min=int(degree.min()), dbscan_degree_median=float(np.median(degree)), dbscan_degree_max=int(degree.max()))

    def write():
        write_labels(params.out_file, labels)
        if params.dbscan_core is not None:
            write_core(params.dbscan_core, core)

    return "matrix + DBSCAN", "Writing cluster labels", write, dict(st, rows=[0, n]), stats


def main(argv=None, params=None):
    """phyloligo.py:1036-1068 around whichever mode the options choose.  params: the command line as `python -m phyloligo_amd`
    has parsed it already."""
    global INGEST_PHASES
    if params is None:
        params = get_cmd(argv)
    if type(params.pattern) == int:                      # :1040-1041
        params.pattern = str("1") * params.pattern
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        from .cli_ranks import main_distributed
        return main_distributed(params)
    refuse(refusal(params))
    t_start = time.perf_counter()
    print("Using pattern {}".format(params.pattern))
    if not os.path.isdir(params.workdir):
        os.makedirs(params.workdir)
    print("Computing frequencies")
    INGEST_PHASES = bool(params.json_stats)              # the phase times of the ingest go into the JSON record
    frequencies, freq_name = compute_frequencies(params.mthdrun, params.large, params.genome, params.pattern,
                                                 params.strand, params.distchunksize, params.threads_max,
                                                 params.workdir)
    t_freq = time.perf_counter()
    if frequencies is not None and params.dist not in METRICS:
        refuse("Error, unknown metric methodfor joblib: {}".format(params.dist))
    clipped = {}
    if frequencies is not None and _clip_active(params):
        frequencies, clipped = _clip(params, frequencies)
    print("Computing Pairwise distances")
    t_dist0 = time.perf_counter()
    if frequencies is None:                              # an unknown --method: compute_frequencies has said so (:995 only prints)
        return 0
    mode = (_kmedoids_mode if params.kmedoids is not None or params.kmedoids_sweep is not None else
            _dbscan_mode if getattr(params, "dbscan", None) is not None else
            _tsne_mode if params.tsne is not None else _knn_mode if params.knn is not None else _matrix_mode)
    label, announce, write, stage2, stats = mode(params, frequencies)
    t_dist = time.perf_counter()
    _timing("single process: %s %.3f s" % (label, t_dist - t_dist0))
    _write_freq(params, lambda: np.asarray(frequencies))
    if announce:
        print(announce)
        write()
    if params.json_stats:
        _write_json_stats(params, frequencies, t_freq - t_start, t_dist - t_dist0, time.perf_counter() - t_dist, time.perf_counter() - t_start,
                          stage2=stage2, stats=dict(stats, **clipped))
    return 0


def _write_json_stats(params, frequencies, freq_s, dist_s, write_s, total_s, gpus=1, stage2=None, stats={}):
    """--json-stats ("keep the same five lines for CLI fidelity; add --json-stats"): the run's sizes and times, the
    stats of its first stage-2 call, then the keys of its mode and of the clip.  frequencies: anything with the matrix's shape."""
    import json
    from . import _lib
    n, dim = (int(x) for x in frequencies.shape)
    record = {"library": _lib.load().po_version().decode(), "device": _context().device_name, "gpus": gpus,
              "assembly": os.path.abspath(params.genome), "contigs": n, "words": dim, "pattern": str(params.pattern),
              "strand": params.strand, "metric": params.dist, "large": params.large, "pairs": n * (n - 1) // 2,
              "seconds": {"frequencies": freq_s, "distances" + ("_and_container" if params.large in ("memmap", "h5py") else ""): dist_s,
                          "writing": write_s, "total": total_s},
              "stage2_first_call": stage2, **stats,
              "ingest_phases_ms": None if LAST_INGEST is None else {k: round(v, 3) for k, v in LAST_INGEST.items()}}
    with open(params.json_stats, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
    sys.exit(0)
