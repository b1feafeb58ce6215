"""`python -m phyloligo_amd` as one of several ranks (WORLD_SIZE > 1; phyloligo.main() imports this module only then).

The reference spreads row slices over joblib workers that all see the frequency matrix (gen_even_slices,
phyloligo.py:424,516).  Here every rank profiles its own block of contigs, ONE all-gather moves the exact count
matrix, the block grid is dealt out like a round-robin tournament (dist.RowBlockPlan: every unordered pair evaluated
once in the whole job), the transposed blocks go to the ranks whose rows they complete, and every rank writes its
rows of the output: straight into its byte range of the float32 container (--large memmap / h5py), or in rank order into the
text matrix.  PO_CLI_REHEARSAL=1: all ranks on GPU 0 with gloo collectives, which move host tensors (a one-GPU box can run the
code path); every step that differs for it says so where it does.
"""
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

from . import api
from ._lib import METRICS, STRANDS
from .phyloligo import (_bc_memmap_diagonal, _context, _hdf5_or_refuse, _open_raw_container, _pwrite_rows, _timing, _write_freq,
                        _write_json_stats, _write_knn, read_fasta, read_fasta_device, refusal, refuse)


class _BlockWriter:
    """Device blocks of one rank -> their byte ranges of the shared float32 container (the multi-GPU form of
    _write_raw_f32): two pinned host buffers; the device-to-host copy of chunk k + 1 runs on a side stream while
    po_pwrite_rows (parallel pwrite) puts chunk k into the file from a background thread."""

    def __init__(self, fd, n, device, chunk_bytes=256 << 20, writers=8, base=0):
        import concurrent.futures as cf
        import torch
        self.torch, self.fd, self.n, self.writers, self.base = torch, fd, n, writers, base
        self.chunk = chunk_bytes
        self.stage = [torch.empty(chunk_bytes // 4, dtype=torch.float32, pin_memory=True) for _ in range(2)]
        self.pending = [None, None]
        self.stream = torch.cuda.Stream(device)
        self.pool = cf.ThreadPoolExecutor(max_workers=1)
        self.k = 0

    def put(self, t, row0, col0, fix=None):
        """t[R, C] float32 on the device -> rows row0.., columns col0.. of the file"""
        torch = self.torch
        R, C = t.shape
        if R == 0 or C == 0:
            return
        per = max(1, self.chunk // (C * 4))
        self.stream.wait_stream(torch.cuda.current_stream(t.device))
        for a in range(0, R, per):
            b = min(R, a + per)
            which = self.k & 1
            self.k += 1
            if self.pending[which] is not None:                  # the chunk written from this buffer two rounds ago
                self.pending[which].result()
            view = self.stage[which][:(b - a) * C].view(b - a, C)
            with torch.cuda.stream(self.stream):
                view.copy_(t[a:b], non_blocking=True)
            self.stream.synchronize()                            # (the previous chunk is being written meanwhile)
            host = view.numpy()
            if fix is not None:
                fix(host, row0 + a, row0 + b)
            self.pending[which] = self.pool.submit(_pwrite_rows, self.fd, host, row0 + a, col0, self.n, self.writers, self.base)

    def close(self):
        try:
            for f in self.pending:
                if f is not None:
                    f.result()
        finally:
            self.pool.shutdown(wait=True)


def _setup(params):
    """Refusals (rank 0 speaks), the process group, this rank's context, its share of the ingest and the all-gather of the
    profiles: everything the three writers below share, as one record."""
    import torch
    import torch.distributed as tdist
    from .dist import RowBlockPlan, first_contact
    s = SimpleNamespace(t_start=time.perf_counter(), tdist=tdist, rank=int(os.environ["RANK"]), world=int(os.environ["WORLD_SIZE"]),
                        rehearsal=os.environ.get("PO_CLI_REHEARSAL") == "1")
    local = 0 if s.rehearsal else int(os.environ.get("LOCAL_RANK", "0"))
    speak = s.rank == 0
    if params.mthdrun not in ("joblib", "hip"):
        refuse("Error, the multi-GPU run supports --method joblib|hip", speak)
    if params.large == "h5py":
        _hdf5_or_refuse(speak)
    if params.strand not in STRANDS or params.dist not in METRICS:
        sys.exit(1)
    refuse(refusal(params), speak)
    first_contact("cuda.set_device", torch.cuda.set_device, local)
    if s.rehearsal:
        first_contact("init_process_group", tdist.init_process_group, "gloo")
    else:
        first_contact("init_process_group", tdist.init_process_group, "nccl", device_id=torch.device("cuda", local))
    s.ctx, s.dev = _context(local), torch.device("cuda", local)
    say = print if speak else (lambda *a, **k: None)
    say("Using pattern {}".format(params.pattern))
    if speak and not os.path.isdir(params.workdir):
        os.makedirs(params.workdir)
    say("Computing frequencies")
    ingest = read_fasta_device(params.genome)
    if ingest is not None:
        d_seq, d_off, _ = ingest
    else:
        seq, offsets, _ = read_fasta(params.genome)
        d_seq, d_off = torch.from_numpy(seq).to(s.dev), torch.from_numpy(offsets.astype(np.int64)).to(s.dev)
    s.n = int(d_off.numel()) - 1
    s.plan = RowBlockPlan(s.n, s.world)
    s.lo, s.hi = lo, hi = s.plan.rows(s.rank)
    my_off = (d_off[lo:hi + 1] - d_off[lo]).contiguous()
    my_seq = d_seq[int(d_off[lo]):int(d_off[hi])]
    if my_seq.data_ptr() % 16:                                  # the kernels read aligned 16-byte vectors
        my_seq = my_seq.clone()
    my_counts, my_totals = s.ctx.count_profiles(my_seq, my_off, params.pattern, params.strand)
    host = (lambda t: t.cpu()) if s.rehearsal else (lambda t: t)      # rehearsal: host tensors through the collective, and back

    def gather():                         # the ranks' first collective: a failure surfaces at the synchronize at the latest
        c, t = s.plan.all_gather_profiles(host(my_counts), host(my_totals), tdist)
        torch.cuda.synchronize(s.dev)
        return c.to(s.dev), t.to(s.dev)

    s.counts, s.totals = first_contact("all_gather_profiles", gather)
    say("Computing Pairwise distances")
    s.t_dist0 = time.perf_counter()
    return s


def _complete_rows(s, slab, mirrors):
    """the row-completing exchange: afterwards this rank's slab holds ITS ROWS of the matrix whole"""
    import torch
    if s.rehearsal:                                             # host tensors through gloo; the slab stays on the device
        mirrors[:] = [None if m is None else m.cpu() for m in mirrors]
    s.plan.complete_rows(s.rank, slab, mirrors, s.tdist, stage_device="cpu" if s.rehearsal else None)
    del mirrors[:]
    torch.cuda.synchronize(s.dev)


def _frequencies(s):
    return s.ctx.frequencies(s.counts, s.totals).cpu().numpy()


def _finish(params, s, t_computed, t_written, **stats):
    """rank 0 writes --json-stats (the time between t_computed and t_written is the writing); the group is taken down"""
    if params.json_stats and s.rank == 0:
        t_end = time.perf_counter()
        _write_json_stats(params, SimpleNamespace(shape=(s.n, int(s.counts.shape[1]))), s.t_dist0 - s.t_start, t_computed - s.t_dist0,
                          t_written - t_computed, t_end - s.t_start, gpus=s.world, **stats)
    s.tdist.destroy_process_group()
    return 0


def _write_container(params, s, slab, mirrors, t_computed):
    """--large memmap / h5py.  The row-completing exchange runs first (point to point over xGMI: cheap next to any file system), so
    that every rank holds its rows whole and writes one contiguous byte range of the file in large pieces.  Measured
    on one MI355X node (tools/ubench/container_write_modes.cpp, page cache of overlay/ext4, 3.6 GB): buffered writes
    take the inode lock, so ranks that each pwrite their 60 kB pieces of every row reach 4.7 GB/s between two of them and
    2.5 GB/s between eight (the lock changes hands at every call; round 3 did exactly that, 0.82 s for this file),
    a shared mapping written with memcpy 0.6 - 2.7 GB/s, while contiguous row slabs in large pieces reach 11 GB/s from
    two and 15.6 GB/s from eight processes."""
    n, lo, hi, tdist = s.n, s.lo, s.hi, s.tdist
    _write_freq(params, lambda: _frequencies(s), s.rank == 0)
    base = [0]
    if s.rank == 0:
        if params.large == "h5py":                              # libhdf5 creates and sizes the file; the ranks fill the dataset's data range
            base[0] = _hdf5_or_refuse().create_f32_dataset(params.out_file, "distances", n, n)
        else:
            os.close(_open_raw_container(params.out_file, n * n * 4))
    tdist.broadcast_object_list(base, src=0)                    # where the matrix starts in the file
    empty = (s.totals.cpu().numpy() == 0) if params.dist == "BC" else None

    def diag_fix(host, a, b):                                   # rows [a, b) of the matrix, whole
        _bc_memmap_diagonal(host, a, b, np.flatnonzero(empty[a:b]) + a)

    fix = diag_fix if (empty is not None and empty[lo:hi].any()) else None
    _complete_rows(s, slab, mirrors)
    t_exchanged = time.perf_counter()
    tdist.barrier()                                             # the file exists and has its size
    fd = os.open(params.out_file, os.O_RDWR)
    # (two pinned chunks of at most 256 MB; pinning costs ~0.07 s per GB, a small job does not pay for more than its slab)
    writer = _BlockWriter(fd, n, s.dev, chunk_bytes=min(256 << 20, max(1 << 20, (hi - lo) * n * 4)), base=int(base[0]))
    try:
        writer.put(slab, lo, 0, fix=fix)                        # device -> pinned host chunks -> parallel pwrite, overlapped
    finally:
        try:
            writer.close()
        finally:
            os.close(fd)
    tdist.barrier()
    t_end = time.perf_counter()
    _timing("rank %d of %d: distances + container %.3f s (allocate + compute %.3f, row-completing exchange %.3f, copy + write %.3f)"
            % (s.rank, s.world, t_end - s.t_dist0, t_computed - s.t_dist0, t_exchanged - t_computed, t_end - t_exchanged))
    return _finish(params, s, t_end, t_end)                     # (the container is part of "distances_and_container")


def _write_text(params, s, slab, mirrors, t_computed):
    """the text matrix: rows have to be complete, and the ranks append theirs in rank order = row order"""
    n, lo, hi = s.n, s.lo, s.hi
    _complete_rows(s, slab, mirrors)
    step = max(1, (256 << 20) // max(1, n * slab.element_size()))     # rows per host copy: the slab never sits on the host whole
    _write_freq(params, lambda: _frequencies(s), s.rank == 0)
    if s.rank == 0:
        print("Writing distance matrix")
    for r in range(s.world):
        if r == s.rank:
            if r == 0 and hi == lo:
                api.write_mat_text(params.out_file, np.zeros((0, n)))
            for a in range(0, hi - lo, step):
                api.write_mat_text(params.out_file, slab[a:min(hi - lo, a + step)].cpu().numpy(), append=(r > 0 or a > 0))
        s.tdist.barrier()
    return _finish(params, s, t_computed, time.perf_counter())


def _knn_distributed(params, s):
    """--knn on several GPUs: every rank selects from the blocks of its tournament work list (partial lists over all n rows),
    rank 0 gathers the lists, merges them and writes the graph.  No row-completing exchange: the lists are [n, K], not rows."""
    import torch
    idx, val, st = s.ctx.knn_blocks(s.counts, s.totals, params.knn, s.plan.work(s.rank), params.dist, "float64", want_stats=True)
    torch.cuda.synchronize()
    t_computed = time.perf_counter()
    if s.rehearsal:                                             # host tensors through gloo
        idx, val = idx.cpu(), val.cpu()
    idx_all = [torch.empty_like(idx) for _ in range(s.world)]
    val_all = [torch.empty_like(val) for _ in range(s.world)]
    s.tdist.all_gather(idx_all, idx)
    s.tdist.all_gather(val_all, val)
    _write_freq(params, lambda: _frequencies(s), s.rank == 0)
    if s.rank == 0:
        print("Writing distance matrix")
        m_idx, m_val = s.ctx.knn_merge(torch.stack(idx_all).to(s.dev), torch.stack(val_all).to(s.dev), params.dist)
        _write_knn(params, s.counts.cpu().numpy(), m_idx.cpu().numpy(), m_val.cpu().numpy())
    t_written = time.perf_counter()
    s.tdist.barrier()
    return _finish(params, s, t_computed, t_written, stage2=dict(st, rows=[0, s.n]), stats={"knn": params.knn, "knn_select_ms": st.get("select_ms")})


def main_distributed(params):
    """the job of phyloligo.main() as one rank of several"""
    import torch
    s = _setup(params)
    if params.knn is not None:
        return _knn_distributed(params, s)
    container = params.large in ("memmap", "h5py")
    slab, mirrors = s.plan.allocate(s.rank, s.dev, torch.float32 if container else torch.float64)
    s.plan.compute(s.ctx, s.counts, s.totals, params.dist, s.rank, slab, mirrors)
    torch.cuda.synchronize(s.dev)
    return (_write_container if container else _write_text)(params, s, slab, mirrors, time.perf_counter())
