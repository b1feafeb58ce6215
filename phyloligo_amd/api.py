"""Thin Python face of the C ABI: numpy arrays (host entry points) or torch CUDA tensors
(device entry points) in, the same out.  All arithmetic happens in libphyloligo_amd.so.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import (METRICS, STRANDS, PO_F32, PO_F64, PO_FLAG_NO_SYMMETRY, PO_FLAG_NO_TABLE_PATH, PO_FLAG_NO_RC_FOLD, PO_FLAG_PAIRDOT_I8, PO_FLAG_NO_PAIRDOT, PO_KNN_MAX_K, PoBlock, PoDbscanResult, PoKmedoidsResult, PoSilhouetteResult, PoStats, PoTsneParams, PoTsneResult,
                   check)


def normalise_pattern(pattern):
    """-k N and -p PATTERN share one destination in the reference CLI
    (bin/phyloligo.py:1006,1027); an int means the contiguous pattern "1"*N (:1040-1041)."""
    if isinstance(pattern, (int, np.integer)) and not isinstance(pattern, bool):
        pattern = "1" * int(pattern)
    return str(pattern)


def pattern_info(pattern):
    lib = _lib.load()
    w, k, d = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    check(lib.po_pattern_info(normalise_pattern(pattern).encode(), ctypes.byref(w), ctypes.byref(k), ctypes.byref(d)))
    return w.value, k.value, d.value


def device_count():
    return _lib.load().po_device_count()


def _np_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class Context:
    """One po_ctx = one GPU.  Device-tensor calls run on torch's current stream."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        self.device = int(device)
        check(self._lib.po_ctx_create(ctypes.byref(self._h), self.device))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.po_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        check(self._lib.po_ctx_device_name(self._h, buf, 256))
        return buf.value.decode()

    def synchronize(self):
        check(self._lib.po_ctx_synchronize(self._h))

    def trim(self):
        """free the device workspaces this context has grown (po_ctx_trim); the next call allocates again"""
        check(self._lib.po_ctx_trim(self._h))

    def _use_torch_stream(self):
        import torch
        check(self._lib.po_ctx_set_stream(self._h, ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    # ---- stage 1 ---------------------------------------------------------------------------
    def count_profiles(self, seq, offsets, pattern="1111", strand="both"):
        """seq: uint8 concatenated sequence bytes, offsets: uint64[n+1].  numpy in -> numpy out
        (uint32 counts[n, 4^k], uint64 totals[n]); torch CUDA tensors in -> torch CUDA tensors out."""
        pat = normalise_pattern(pattern)
        _, _, dim = pattern_info(pat)
        if strand not in STRANDS:
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "strand must be one of both/plus/minus (got %r)" % (strand,))
        if _is_torch(seq):
            import torch
            n = offsets.numel() - 1
            assert seq.dtype == torch.uint8 and seq.is_cuda and seq.is_contiguous()
            assert offsets.dtype == torch.int64 and offsets.is_cuda and offsets.is_contiguous()
            if seq.device.index != self.device or offsets.device != seq.device:
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "tensors are on %s / %s, this context drives cuda:%d"
                                          % (seq.device, offsets.device, self.device))
            counts = torch.empty((n, dim), dtype=torch.int32, device=seq.device)
            totals = torch.empty((n,), dtype=torch.int64, device=seq.device)
            self._use_torch_stream()
            check(self._lib.po_count_profiles_dev(self._h, seq.data_ptr(), offsets.data_ptr(), n, seq.numel(),
                                                  pat.encode(), STRANDS[strand], counts.data_ptr(), totals.data_ptr()))
            return counts, totals
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.shape[0] - 1
        counts = np.zeros((n, dim), dtype=np.uint32)
        totals = np.zeros((n,), dtype=np.uint64)
        check(self._lib.po_count_profiles(self._h, _np_ptr(seq), _np_ptr(offsets), n, pat.encode(), STRANDS[strand],
                                          _np_ptr(counts), _np_ptr(totals)))
        return counts, totals

    def count_profiles_ranges(self, seq, begins, ends, pattern="1111", strand="both"):
        """Profiles of arbitrary (overlapping) byte ranges [begins[i], ends[i]) of one sequence buffer --
        Kount.py's sliding windows.  numpy in -> numpy out; torch CUDA tensors in -> torch CUDA tensors out."""
        pat = normalise_pattern(pattern)
        _, _, dim = pattern_info(pat)
        if strand not in STRANDS:
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "strand must be one of both/plus/minus (got %r)" % (strand,))
        if _is_torch(seq):
            import torch
            self._check_device(seq, begins, ends)
            assert seq.dtype == torch.uint8 and seq.is_contiguous()
            assert begins.dtype == torch.int64 and ends.dtype == torch.int64 and begins.is_contiguous() and ends.is_contiguous()
            n = begins.numel()
            counts = torch.empty((n, dim), dtype=torch.int32, device=seq.device)
            totals = torch.empty((n,), dtype=torch.int64, device=seq.device)
            sum_lengths = int((ends - begins).sum().item()) if n else 0
            self._use_torch_stream()
            check(self._lib.po_count_profiles_ranges_dev(self._h, seq.data_ptr(), seq.numel(), begins.data_ptr(), ends.data_ptr(), n,
                                                         sum_lengths, pat.encode(), STRANDS[strand], counts.data_ptr(),
                                                         totals.data_ptr()))
            return counts, totals
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        begins = np.ascontiguousarray(begins, dtype=np.uint64)
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        n = begins.shape[0]
        counts = np.zeros((n, dim), dtype=np.uint32)
        totals = np.zeros((n,), dtype=np.uint64)
        check(self._lib.po_count_profiles_ranges(self._h, _np_ptr(seq), seq.shape[0], _np_ptr(begins), _np_ptr(ends), n,
                                                 pat.encode(), STRANDS[strand], _np_ptr(counts), _np_ptr(totals)))
        return counts, totals

    def _check_device(self, *tensors):
        for t in tensors:
            if t.device.type != "cuda" or t.device.index != self.device:
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "tensor is on %s, this context drives cuda:%d" % (t.device, self.device))

    def count_byte_ranges(self, seq, begins, ends, byte):
        """Occurrences of one byte value in every range (device tensors): the numerator of Kount.py's N gate."""
        import torch
        self._check_device(seq, begins, ends)
        assert seq.dtype == torch.uint8 and begins.dtype == torch.int64 and ends.dtype == torch.int64
        out = torch.empty((begins.numel(),), dtype=torch.int64, device=seq.device)
        self._use_torch_stream()
        check(self._lib.po_count_byte_ranges_dev(self._h, seq.data_ptr(), seq.numel(), begins.data_ptr(), ends.data_ptr(),
                                                 begins.numel(), int(byte), out.data_ptr()))
        return out

    def profile_distances(self, counts, totals, proto, metric="JSD"):
        """Distance of every profile to ONE prototype frequency vector (Kount.py's JSD / KL / Eucl, unscaled)."""
        code = {"Eucl": 0, "JSD": 1, "KL": _lib.PO_KL}.get(metric)
        if code is None:
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "metric must be JSD, KL or Eucl (got %r)" % (metric,))
        if _is_torch(counts):
            import torch
            self._check_device(counts, totals)
            n, dim = counts.shape
            assert counts.dtype == torch.int32 and totals.dtype == torch.int64 and counts.is_contiguous()
            d_proto = proto if _is_torch(proto) else torch.from_numpy(np.ascontiguousarray(proto, dtype=np.float64)).to(counts.device)
            assert d_proto.dtype == torch.float64 and d_proto.numel() == dim
            out = torch.empty((n,), dtype=torch.float64, device=counts.device)
            self._use_torch_stream()
            check(self._lib.po_profile_distances_dev(self._h, counts.data_ptr(), totals.data_ptr(), n, dim, d_proto.data_ptr(),
                                                     code, out.data_ptr()))
            return out
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        totals = np.ascontiguousarray(totals, dtype=np.uint64)
        proto = np.ascontiguousarray(proto, dtype=np.float64)
        n, dim = counts.shape
        assert proto.shape == (dim,)
        out = np.zeros(n, dtype=np.float64)
        check(self._lib.po_profile_distances(self._h, _np_ptr(counts), _np_ptr(totals), n, dim, _np_ptr(proto), code,
                                             _np_ptr(out)))
        return out

    def frequencies(self, counts, totals):
        if _is_torch(counts):
            import torch
            n, dim = counts.shape
            out = torch.empty((n, dim), dtype=torch.float64, device=counts.device)
            self._use_torch_stream()
            check(self._lib.po_frequencies_dev(self._h, counts.data_ptr(), totals.data_ptr(), n, dim, out.data_ptr()))
            return out
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        totals = np.ascontiguousarray(totals, dtype=np.uint64)
        n, dim = counts.shape
        out = np.zeros((n, dim), dtype=np.float64)
        check(self._lib.po_frequencies(self._h, _np_ptr(counts), _np_ptr(totals), n, dim, _np_ptr(out)))
        return out

    # ---- stage 2 ---------------------------------------------------------------------------
    def reserve(self, n, dim, metric):
        check(self._lib.po_pairwise_reserve(self._h, n, dim, METRICS[metric]))

    def pairwise(self, counts, totals, metric="Eucl", row_begin=0, row_end=None, dtype="float64", symmetric=True,
                 out=None, want_stats=False, table_path=True, rc_fold=True, pairdot_i8=False, pairdot=True):
        """Rows [row_begin,row_end) x all columns of the distance matrix from integer profiles.
        table_path=False forces the general JSD kernel even for record blocks with equal totals;
        rc_fold=False keeps every word even when the profiles are reverse-complement symmetric;
        pairdot_i8=True keeps the materialised KT / BC operand as int8 instead of FP4 (same results);
        pairdot=False leaves KT / BC to the vector-ALU kernels (SAD / O(D^2) Kendall)."""
        return self._pairwise(counts, totals, None, metric, row_begin, row_end, dtype, symmetric, out, want_stats,
                              (0 if table_path else PO_FLAG_NO_TABLE_PATH) | (0 if rc_fold else PO_FLAG_NO_RC_FOLD) |
                              (PO_FLAG_PAIRDOT_I8 if pairdot_i8 else 0) | (0 if pairdot else PO_FLAG_NO_PAIRDOT))

    def pairwise_freq(self, freq, metric="Eucl", row_begin=0, row_end=None, dtype="float64", symmetric=True,
                      out=None, want_stats=False, rc_fold=True, table_path=True):
        """The same from a float64 frequency matrix (the reference's `frequencies` argument).  Frequencies that are
        count / total bit for bit (count2freq output) are traced back to the integer profiles on the device and take
        the same kernels as `pairwise`; table_path=False keeps the general float64 kernels."""
        return self._pairwise(None, None, freq, metric, row_begin, row_end, dtype, symmetric, out, want_stats,
                              (0 if rc_fold else PO_FLAG_NO_RC_FOLD) | (0 if table_path else PO_FLAG_NO_TABLE_PATH))

    def pairwise_blocks(self, counts, totals, metric, blocks, dtype="float64", want_stats=False, table_path=True,
                        rc_fold=True, pairdot_i8=False):
        """Several rectangular blocks of one matrix in one call (device tensors only).  `blocks` is a
        list of dicts: rows=(lo,hi), cols=(lo,hi), out=<2-D tensor [rows, cols]>, optional
        mirror=<2-D tensor [cols, rows]>, optional triangular=True (rows == cols)."""
        import torch
        f32 = str(dtype) in ("float32", "torch.float32", "f32")
        want = torch.float32 if f32 else torch.float64
        arr = (PoBlock * max(1, len(blocks)))()
        for k, b in zip(arr, blocks):
            (k.row_begin, k.row_end), (k.col_begin, k.col_end) = b["rows"], b["cols"]
            out = b["out"]
            assert out.dtype == want and out.is_cuda and out.dim() == 2 and out.stride(1) == 1
            assert out.shape[0] >= k.row_end - k.row_begin and out.shape[1] >= k.col_end - k.col_begin
            k.out, k.ld_out = out.data_ptr(), out.stride(0)
            m = b.get("mirror")
            if m is not None:
                assert m.dtype == want and m.is_cuda and m.dim() == 2 and m.stride(1) == 1
                assert m.shape[0] >= k.col_end - k.col_begin and m.shape[1] >= k.row_end - k.row_begin
                k.mirror, k.ld_mirror = m.data_ptr(), m.stride(0)
            k.triangular = 1 if b.get("triangular") else 0
        n, dim = counts.shape
        stats = PoStats()
        self._use_torch_stream()
        check(self._lib.po_pairwise_blocks_dev(self._h, counts.data_ptr(), totals.data_ptr(), n, dim, METRICS[metric],
                                               PO_F32 if f32 else PO_F64, arr, len(blocks),
                                               (0 if table_path else PO_FLAG_NO_TABLE_PATH) |
                                               (0 if rc_fold else PO_FLAG_NO_RC_FOLD) |
                                               (PO_FLAG_PAIRDOT_I8 if pairdot_i8 else 0),
                                               ctypes.byref(stats) if want_stats else None))
        if want_stats:
            return {"prep_ms": stats.prep_ms, "kernel_ms": stats.kernel_ms, "total_ms": stats.total_ms,
                    "pairs": stats.pairs, "tiles": stats.tiles, "kernel_id": stats.kernel_id,
                    "rc_folded": bool(stats.rc_folded)}
        return None

    # ---- k nearest neighbours -----------------------------------------------------------------
    def knn(self, counts, totals, k, metric="JSD", dtype="float64", panel_rows=0, want_stats=False, table_path=True,
            rc_fold=True):
        """The k_eff = min(k, n - 1) nearest records of every record: idx int32 [n, k_eff], val [n, k_eff] (po_knn*), ordered
        by value (descending for KT), NaN last, ties by the smaller index; val[i, c] is the entry (i, idx[i, c]) of
        pairwise(counts, totals, metric, dtype=dtype) bit for bit.  numpy in -> numpy out; torch CUDA tensors in -> tensors out.
        Returns (idx, val), or (idx, val, stats) with want_stats (stats["select_ms"]: the selection kernels)."""
        code, k, f32 = _knn_args(metric, k, dtype)
        n, dim = counts.shape
        k_eff = min(k, max(n - 1, 0))
        flags = (0 if table_path else PO_FLAG_NO_TABLE_PATH) | (0 if rc_fold else PO_FLAG_NO_RC_FOLD)
        stats = PoStats()
        sp = ctypes.byref(stats) if want_stats else None
        if _is_torch(counts):
            import torch
            self._check_device(counts, totals)
            assert counts.dtype == torch.int32 and totals.dtype == torch.int64
            assert counts.is_contiguous() and totals.is_contiguous()
            idx = torch.empty((n, k_eff), dtype=torch.int32, device=counts.device)
            val = torch.empty((n, k_eff), dtype=torch.float32 if f32 else torch.float64, device=counts.device)
            self._use_torch_stream()
            check(self._lib.po_knn_dev(self._h, counts.data_ptr(), totals.data_ptr(), n, dim, code, k, PO_F32 if f32 else PO_F64,
                                       int(panel_rows), idx.data_ptr(), val.data_ptr(), flags, sp))
        else:
            counts = np.ascontiguousarray(counts, dtype=np.uint32)
            totals = np.ascontiguousarray(totals, dtype=np.uint64)
            idx = np.zeros((n, k_eff), dtype=np.int32)
            val = np.zeros((n, k_eff), dtype=np.float32 if f32 else np.float64)
            check(self._lib.po_knn(self._h, _np_ptr(counts), _np_ptr(totals), n, dim, code, k, PO_F32 if f32 else PO_F64,
                                   int(panel_rows), _np_ptr(idx), _np_ptr(val), flags, sp))
        if want_stats:
            return idx, val, _knn_stats(stats)
        return idx, val

    def knn_blocks(self, counts, totals, k, blocks, metric="JSD", dtype="float64", panel_rows=0, want_stats=False):
        """Partial lists [n, k_eff] from a work list of blocks (device tensors; po_knn_blocks_dev).  `blocks`: dicts with
        rows=(lo, hi), cols=(lo, hi), optional triangular=True - or the (rows, cols, kind, peer) items of RowBlockPlan.work(rank).
        Returns (idx, val); idx -1 marks an entry no pair of the blocks filled."""
        import torch
        code, k, f32 = _knn_args(metric, k, dtype)
        self._check_device(counts, totals)
        assert counts.dtype == torch.int32 and totals.dtype == torch.int64 and counts.is_contiguous() and totals.is_contiguous()
        n, dim = counts.shape
        k_eff = min(k, max(n - 1, 0))
        arr = (PoBlock * max(1, len(blocks)))()
        for q, b in zip(arr, blocks):
            if isinstance(b, dict):
                rows, cols, tri = b["rows"], b["cols"], bool(b.get("triangular"))
            else:
                rows, cols, tri = b[0], b[1], b[2] == "diag"
            (q.row_begin, q.row_end), (q.col_begin, q.col_end) = rows, cols
            q.triangular = 1 if tri else 0
        idx = torch.empty((n, k_eff), dtype=torch.int32, device=counts.device)
        val = torch.empty((n, k_eff), dtype=torch.float32 if f32 else torch.float64, device=counts.device)
        stats = PoStats()
        self._use_torch_stream()
        check(self._lib.po_knn_blocks_dev(self._h, counts.data_ptr(), totals.data_ptr(), n, dim, code, k, PO_F32 if f32 else PO_F64,
                                          int(panel_rows), arr, len(blocks), idx.data_ptr(), val.data_ptr(), 0,
                                          ctypes.byref(stats) if want_stats else None))
        if want_stats:
            return idx, val, _knn_stats(stats)
        return idx, val

    def knn_merge(self, idx_lists, val_lists, metric="JSD"):
        """Merge m partial lists (device tensors [n, k] each, or stacked [m, n, k]) into one [n, k] (po_knn_merge_dev)."""
        import torch
        idx_in = idx_lists if _is_torch(idx_lists) else torch.stack(list(idx_lists))
        val_in = val_lists if _is_torch(val_lists) else torch.stack(list(val_lists))
        idx_in, val_in = idx_in.contiguous(), val_in.contiguous()
        assert idx_in.dim() == 3 and idx_in.shape == val_in.shape and idx_in.dtype == torch.int32
        assert val_in.dtype in (torch.float32, torch.float64)
        m, n, k = idx_in.shape
        f32 = val_in.dtype == torch.float32
        code, _, _ = _knn_args(metric, max(k, 1), "float32" if f32 else "float64")
        self._check_device(idx_in, val_in)
        idx = torch.empty((n, k), dtype=torch.int32, device=idx_in.device)
        val = torch.empty((n, k), dtype=val_in.dtype, device=idx_in.device)
        if k == 0 or n == 0:
            return idx, val
        self._use_torch_stream()
        check(self._lib.po_knn_merge_dev(self._h, n, k, code, PO_F32 if f32 else PO_F64, idx_in.data_ptr(), val_in.data_ptr(), m,
                                         idx.data_ptr(), val.data_ptr()))
        return idx, val

    # ---- t-SNE of the k-NN graph ---------------------------------------------------------------
    def tsne_affinities(self, idx, val, perplexity, metric="Eucl"):
        """scikit-learn's joint probabilities from the lists of knn() with k = tsne_neighbours(n, perplexity)
        (po_tsne_affinities_dev): a dict with beta [n] and cond [n, k] (float64: the precision found per row and the
        conditional probabilities), and the CSR of P = (C + C^T) / sum: rowptr int64 [n + 1], col int32 [nnz] (ascending in
        every row), p float32 [nnz].  numpy in -> numpy out; torch CUDA tensors in -> tensors out."""
        import torch
        as_numpy = not _is_torch(idx)
        if as_numpy:
            idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda(self.device)
            val = torch.from_numpy(np.ascontiguousarray(val)).cuda(self.device)
        n, k = idx.shape
        code, f32 = _tsne_list_args(metric, val, perplexity)
        self._check_device(idx, val)
        assert idx.dtype == torch.int32 and idx.is_contiguous() and val.is_contiguous() and val.shape == idx.shape
        dev = idx.device
        cap = 2 * n * k
        beta = torch.empty((n,), dtype=torch.float64, device=dev)
        cond = torch.empty((n, k), dtype=torch.float64, device=dev)
        rowptr = torch.empty((n + 1,), dtype=torch.int64, device=dev)
        col = torch.empty((cap,), dtype=torch.int32, device=dev)
        p = torch.empty((cap,), dtype=torch.float32, device=dev)
        nnz = ctypes.c_uint64()
        self._use_torch_stream()
        check(self._lib.po_tsne_affinities_dev(self._h, n, k, code, PO_F32 if f32 else PO_F64, idx.data_ptr(), val.data_ptr(),
                                               float(perplexity), beta.data_ptr(), cond.data_ptr(), rowptr.data_ptr(),
                                               col.data_ptr(), p.data_ptr(), cap, ctypes.byref(nnz)))
        out = {"beta": beta, "cond": cond, "rowptr": rowptr, "col": col[:nnz.value].clone(), "p": p[:nnz.value].clone()}
        if as_numpy:
            out = {key: t.cpu().numpy() for key, t in out.items()}
        return out

    def tsne_gradient(self, rowptr, col, p, y, exaggeration=1.0):
        """Gradient of KL(exaggeration * P || Q) at the embedding y float32 [n, 2] (po_tsne_gradient_dev): (grad float32
        [n, 2], Z, KL) with Z = sum over i != j of 1 / (1 + |y_i - y_j|^2), summed exactly over all pairs."""
        import torch
        as_numpy = not _is_torch(y)
        if as_numpy:
            rowptr, col, p, y = (torch.from_numpy(np.ascontiguousarray(a, dtype=t)).cuda(self.device)
                                 for a, t in ((rowptr, np.int64), (col, np.int32), (p, np.float32), (y, np.float32)))
        self._check_device(rowptr, col, p, y)
        assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and p.dtype == torch.float32 and y.dtype == torch.float32
        assert all(t.is_contiguous() for t in (rowptr, col, p, y)) and y.dim() == 2 and y.shape[1] == 2
        n = y.shape[0]
        assert rowptr.numel() == n + 1 and col.numel() == p.numel()
        grad = torch.empty_like(y)
        z, kl = ctypes.c_double(), ctypes.c_double()
        self._use_torch_stream()
        check(self._lib.po_tsne_gradient_dev(self._h, n, rowptr.data_ptr(), col.data_ptr(), p.data_ptr(), col.numel(), y.data_ptr(),
                                             float(exaggeration), grad.data_ptr(), ctypes.byref(z), ctypes.byref(kl)))
        return (grad.cpu().numpy() if as_numpy else grad), z.value, kl.value

    def tsne_optimise(self, rowptr, col, p, y0, max_iter=1000, exploration_iter=None, want_stats=False, time_kernels=False):
        """scikit-learn's gradient descent from y0 on the CSR of tsne_affinities (po_tsne_dev; device tensors).  time_kernels:
        the stats carry repulsion_ms / attraction_ms / rest_ms, medians per iteration from device events."""
        import torch
        self._check_device(rowptr, col, p, y0)
        assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and p.dtype == torch.float32 and y0.dtype == torch.float32
        assert all(t.is_contiguous() for t in (rowptr, col, p, y0)) and y0.dim() == 2 and y0.shape[1] == 2
        n = y0.shape[0]
        assert rowptr.numel() == n + 1 and col.numel() == p.numel()
        params, hist = _tsne_params(max_iter, exploration_iter)
        params.time_kernels = 1 if time_kernels else 0
        res = PoTsneResult()
        y = torch.empty_like(y0)
        self._use_torch_stream()
        check(self._lib.po_tsne_dev(self._h, n, rowptr.data_ptr(), col.data_ptr(), p.data_ptr(), col.numel(), y0.data_ptr(),
                                    ctypes.byref(params), y.data_ptr(), ctypes.byref(res)))
        return (y, _tsne_stats(res, hist)) if want_stats else y

    def tsne(self, idx, val, perplexity, seed=0, max_iter=1000, y0=None, want_stats=False, metric="Eucl", exploration_iter=None):
        """The 2-D t-SNE embedding float32 [n, 2] of the points whose k = tsne_neighbours(n, perplexity) nearest neighbours
        knn() listed: what sklearn.manifold.TSNE(n_components=2, perplexity=perplexity, metric="precomputed", init="random",
        random_state=seed, method="barnes_hut", angle=0.0) computes from the whole matrix (bin/phyloselect.py:381-398), with
        the repulsive force summed exactly on the GPU.  y0 (float32 [n, 2]) replaces the seeded start.  metric: the metric of
        the lists (KT, a correlation, is refused).  numpy in -> numpy out (po_tsne); torch CUDA tensors in -> tensor out
        (po_tsne_affinities_dev + po_tsne_dev), the same bytes.  want_stats: (y, stats) with kl, iterations, grad_norm,
        history [(iteration, kl, grad_norm) of every check] and, for numpy input, affinities_ms / optimise_ms."""
        n, k = idx.shape
        code, f32 = _tsne_list_args(metric, val, perplexity)
        if y0 is None:
            y0 = tsne_start(n, seed)
        if _is_torch(idx):
            import torch
            if not _is_torch(y0):
                y0 = torch.from_numpy(np.ascontiguousarray(y0, dtype=np.float32)).to(idx.device)
            a = self.tsne_affinities(idx, val, perplexity, metric)
            return self.tsne_optimise(a["rowptr"], a["col"], a["p"], y0.contiguous(), max_iter, exploration_iter, want_stats)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float32 if f32 else np.float64)
        y0 = np.ascontiguousarray(y0, dtype=np.float32)
        if y0.shape != (n, 2):
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "y0 must have shape (%d, 2), got %r" % (n, y0.shape))
        params, hist = _tsne_params(max_iter, exploration_iter)
        res = PoTsneResult()
        y = np.zeros((n, 2), dtype=np.float32)
        check(self._lib.po_tsne(self._h, n, k, code, PO_F32 if f32 else PO_F64, _np_ptr(idx), _np_ptr(val), float(perplexity),
                                _np_ptr(y0), ctypes.byref(params), _np_ptr(y), ctypes.byref(res)))
        return (y, _tsne_stats(res, hist)) if want_stats else y

    # ---- arguments of the calls that take a distance matrix (k-medoids, silhouettes, row medians) ----
    def _matrix_arg(self, matrix, square=True):
        """(is_torch, matrix, dtype code, n, ld) of a 2-D float32 / float64 matrix with unit inner stride and row stride >= n;
        square=False: any [rows, n] (the row count is matrix.shape[0])"""
        if _is_torch(matrix):
            import torch
            self._check_device(matrix)
            if matrix.dim() != 2 or (square and matrix.shape[0] != matrix.shape[1]) or matrix.dtype not in (torch.float32, torch.float64):
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "matrix must be a %s float32 / float64 tensor (got %s %s)"
                                          % ("square" if square else "2-D", tuple(matrix.shape), matrix.dtype))
            rows, n = matrix.shape
            if n > 1 and matrix.stride(1) != 1:
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "matrix must have unit inner stride (strides %r)" % (tuple(matrix.stride()),))
            ld = matrix.stride(0) if rows > 1 else max(n, 1)
            return True, matrix, PO_F32 if matrix.dtype == torch.float32 else PO_F64, n, ld
        if not isinstance(matrix, np.ndarray) or matrix.dtype not in (np.float32, np.float64):
            matrix = np.asarray(matrix, dtype=np.float64)
        if matrix.ndim != 2 or (square and matrix.shape[0] != matrix.shape[1]):
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "matrix must be %s (got shape %r)" % ("square" if square else "2-D", matrix.shape))
        rows, n = matrix.shape
        if (n > 1 or rows > 1) and (matrix.strides[1] != matrix.itemsize or matrix.strides[0] % matrix.itemsize or matrix.strides[0] < 0):
            matrix = np.ascontiguousarray(matrix)
        ld = matrix.strides[0] // matrix.itemsize if rows > 1 else max(n, 1)
        return False, matrix, PO_F32 if matrix.dtype == np.float32 else PO_F64, n, ld

    def _matrix_on_device(self, matrix, square=True):
        import torch
        is_t, matrix, code, n, ld = self._matrix_arg(matrix, square)
        if not is_t:
            matrix = torch.from_numpy(matrix).cuda(self.device)      # a strided view arrives with its row stride
            ld = matrix.stride(0) if matrix.shape[0] > 1 else max(n, 1)
        return is_t, matrix, code, n, ld

    def _labels_on_device(self, labels, n, dev):
        import torch
        labels = labels if _is_torch(labels) else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
        self._check_device(labels)
        if labels.dtype != torch.int32 or labels.shape != (n,):
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "labels must be int32 [%d] (got %s %s)" % (n, labels.dtype, tuple(labels.shape)))
        return labels.contiguous()

    def _index_list_on_device(self, x, name, dev):
        import torch
        x = x if _is_torch(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
        self._check_device(x)
        if x.dtype != torch.int32 or x.dim() != 1:
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "%s must be a 1-D int32 index list" % name)
        return x.contiguous()

    @staticmethod
    def _check_n_clusters(n_clusters, n):
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)) or not 1 <= int(n_clusters) <= n:
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "n_clusters must be an integer in 1..n = %d (got %r)" % (n, n_clusters))
        return int(n_clusters)

    # ---- k-medoids on a distance matrix --------------------------------------------------------
    def kmedoids(self, matrix, n_clusters=8, max_iter=300, init="heuristic", want_stats=False):
        """k-medoids of a precomputed distance matrix [n, n] (float32 / float64, unit inner stride, any row stride >= n): what
        the reference's KMedoids(n_clusters, distance_metric="precomputed", max_iter=max_iter).fit(matrix) decides
        (bin/phyloselect.py:37-309), on the GPU with float64 sums.  init: "heuristic" (the rows with the smallest sums) or
        n_clusters distinct row indices - RandomState(seed).permutation(n)[:n_clusters] is the reference's init="random".
        Returns (labels int32 [n], medoids int32 [n_clusters]); with want_stats also a dict (iterations, converged, inertia,
        empty_clusters, start_ms / rowsum_ms / assign_ms / update_ms).  numpy in -> numpy out (po_kmedoids: the matrix is
        copied to the device); torch CUDA tensor in -> tensors out on torch's current stream (po_kmedoids_dev).  With the
        heuristic start a row that sums to NaN is refused (PO_EINVAL); with explicit rows a NaN gives an unspecified result."""
        is_t, matrix, code, n, ld = self._matrix_arg(matrix)
        k = self._check_n_clusters(n_clusters, n)
        if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or int(max_iter) < 1:
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "max_iter must be at least 1 (got %r)" % (max_iter,))
        start = None
        if not (isinstance(init, str) and init == "heuristic"):
            if isinstance(init, str):
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "init must be \"heuristic\" or %d row indices (got %r)" % (k, init))
            start = init.cpu().numpy() if _is_torch(init) else np.asarray(init)
            if start.shape != (k,) or start.dtype.kind not in "iu" or (start.size and (start.min() < 0 or start.max() >= n)):
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "init must be %d integer row indices in 0..%d (got %r)" % (k, n - 1, init))
            start = np.ascontiguousarray(start, dtype=np.int32)
        sp = _np_ptr(start) if start is not None else None
        res = PoKmedoidsResult()
        rp = ctypes.byref(res) if want_stats else None
        if is_t:
            import torch
            labels = torch.empty((n,), dtype=torch.int32, device=matrix.device)
            medoids = torch.empty((k,), dtype=torch.int32, device=matrix.device)
            self._use_torch_stream()
            check(self._lib.po_kmedoids_dev(self._h, matrix.data_ptr(), code, n, ld, k, sp, int(max_iter), labels.data_ptr(),
                                            medoids.data_ptr(), rp))
        else:
            labels = np.zeros(n, dtype=np.int32)
            medoids = np.zeros(k, dtype=np.int32)
            check(self._lib.po_kmedoids(self._h, _np_ptr(matrix), code, n, ld, k, sp, int(max_iter), _np_ptr(labels), _np_ptr(medoids), rp))
        if want_stats:
            return labels, medoids, {"iterations": res.iterations, "converged": bool(res.converged), "inertia": res.inertia,
                                     "empty_clusters": res.empty_clusters, "start_ms": res.start_ms, "rowsum_ms": res.rowsum_ms,
                                     "assign_ms": res.assign_ms, "update_ms": res.update_ms}
        return labels, medoids

    def kmedoids_costs(self, matrix, labels, rows=None):
        """float64 [n]: for every row i the sum of matrix[i, j] over the columns j with labels[j] == labels[i] - the candidate
        costs of one k-medoids update (po_kmedoids_costs_dev).  rows: only these rows, in this order; the bytes of a row's cost
        are the same either way.  numpy in -> numpy out; torch CUDA tensors in -> tensor out."""
        import torch
        is_t, matrix, code, n, ld = self._matrix_on_device(matrix)
        dev = matrix.device
        labels = self._labels_on_device(labels, n, dev)
        d_rows, count = None, n
        if rows is not None:
            d_rows = self._index_list_on_device(rows, "rows", dev)
            count = d_rows.numel()
        out = torch.empty((count,), dtype=torch.float64, device=dev)
        self._use_torch_stream()
        check(self._lib.po_kmedoids_costs_dev(self._h, matrix.data_ptr(), code, n, ld, labels.data_ptr(),
                                              d_rows.data_ptr() if d_rows is not None else None, count if d_rows is not None else 0,
                                              out.data_ptr()))
        return out if is_t else out.cpu().numpy()

    def kmedoids_assign(self, matrix, medoids):
        """int32 [n]: labels[j] = argmin over c of matrix[medoids[c], j], the smaller c wins a tie (po_kmedoids_assign_dev).
        numpy in -> numpy out; torch CUDA tensors in -> tensor out."""
        import torch
        is_t, matrix, code, n, ld = self._matrix_on_device(matrix)
        dev = matrix.device
        medoids = self._index_list_on_device(medoids, "medoids", dev)
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        self._use_torch_stream()
        check(self._lib.po_kmedoids_assign_dev(self._h, matrix.data_ptr(), code, n, ld, medoids.numel(), medoids.data_ptr(),
                                               labels.data_ptr()))
        return labels if is_t else labels.cpu().numpy()

    # ---- silhouettes of a clustering of a distance matrix -------------------------------------------
    def _sil_clusters(self, labels, n, n_clusters):
        """the cluster count of a call: n_clusters, or max(labels) + 1 when it is None"""
        if n_clusters is None:
            if labels.shape[0] == 0:
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "labels are empty")
            n_clusters = int(labels.max()) + 1
        return self._check_n_clusters(n_clusters, n)

    def cluster_sums(self, matrix, labels, n_clusters=None):
        """float64 [n, n_clusters]: S[i, c] = the sum of matrix[i, j] over the columns j with labels[j] == c, in float64 and in
        the order of the k-medoids row sums (po_cluster_sums_dev): S[i, labels[i]] has the bytes of kmedoids_costs, and a
        column's bytes do not depend on n_clusters.  labels: int32 [n] in 0..n_clusters-1 (checked); n_clusters=None means
        max(labels) + 1.  Takes a torch CUDA tensor (numpy is copied to the device) and returns a torch CUDA tensor."""
        import torch
        _, matrix, code, n, ld = self._matrix_on_device(matrix)
        labels = self._labels_on_device(labels, n, matrix.device)
        k = self._sil_clusters(labels, n, n_clusters)
        out = torch.empty((n, k), dtype=torch.float64, device=matrix.device)
        self._use_torch_stream()
        check(self._lib.po_cluster_sums_dev(self._h, matrix.data_ptr(), code, n, ld, labels.data_ptr(), k, out.data_ptr()))
        return out

    def silhouette(self, matrix, labels, n_clusters=None, want_stats=False):
        """float64 [n]: the silhouette value of every record for a precomputed distance matrix [n, n] and labels int32 [n] in
        0..n_clusters-1 - sklearn.metrics.silhouette_samples(matrix, labels, metric="precomputed"), with float64 sums, except
        that clusters without a member are skipped and a record with a NaN sum over a non-empty cluster gets NaN where
        scikit-learn prints 0 (include/phyloligo_amd.h has the definitions).  n_clusters=None means max(labels) + 1; fewer
        than two non-empty clusters are refused.  numpy in -> numpy out (po_silhouette: the matrix is copied to the device);
        torch CUDA tensor in -> tensor out on torch's current stream (po_silhouette_dev).  want_stats: also a dict (mean,
        nonempty_clusters, passes = matrix reads made, sums_ms, finish_ms)."""
        is_t, matrix, code, n, ld = self._matrix_arg(matrix)
        res = PoSilhouetteResult()
        rp = ctypes.byref(res) if want_stats else None
        if is_t:
            import torch
            labels = self._labels_on_device(labels, n, matrix.device)
            k = self._sil_clusters(labels, n, n_clusters)
            values = torch.empty((n,), dtype=torch.float64, device=matrix.device)
            self._use_torch_stream()
            check(self._lib.po_silhouette_dev(self._h, matrix.data_ptr(), code, n, ld, labels.data_ptr(), k, values.data_ptr(), rp))
        else:
            labels = labels.cpu().numpy() if _is_torch(labels) else np.asarray(labels)
            if labels.shape != (n,) or labels.dtype.kind not in "iu":
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "labels must be %d integers (got %s %r)" % (n, labels.dtype, labels.shape))
            labels = np.ascontiguousarray(labels, dtype=np.int32)
            k = self._sil_clusters(labels, n, n_clusters)
            values = np.zeros(n, dtype=np.float64)
            check(self._lib.po_silhouette(self._h, _np_ptr(matrix), code, n, ld, _np_ptr(labels), k, _np_ptr(values), rp))
        if want_stats:
            return values, {"mean": res.mean, "nonempty_clusters": res.nonempty_clusters, "passes": res.passes,
                            "sums_ms": res.sums_ms, "finish_ms": res.finish_ms}
        return values

    # ---- DBSCAN on a distance matrix ---------------------------------------------------------------
    def eps_degrees(self, matrix, eps):
        """int32 [n]: for every row of a distance matrix [n, n] the number of entries <= eps, the diagonal as stored, a NaN never
        (po_eps_degrees_dev): the neighbourhood sizes DBSCAN compares with min_samples.  numpy in -> numpy out (the matrix is
        copied to the device); torch CUDA tensor in -> tensor out on torch's current stream."""
        import torch
        is_t, matrix, code, n, ld = self._matrix_on_device(matrix)
        out = torch.empty((n,), dtype=torch.int32, device=matrix.device)
        self._use_torch_stream()
        check(self._lib.po_eps_degrees_dev(self._h, matrix.data_ptr(), code, n, ld, float(eps), out.data_ptr()))
        return out if is_t else out.cpu().numpy()

    def dbscan(self, matrix, eps, min_samples=5, want_stats=False):
        """DBSCAN of a precomputed distance matrix [n, n] (float32 / float64, unit inner stride, any row stride >= n; symmetric):
        the labels_ and core samples of sklearn.cluster.DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(matrix),
        numbering and border ties included (include/phyloligo_amd.h has the six rules).  An entry <= eps makes two records
        neighbours, compared as float64; a NaN never does, where scikit-learn raises.  Returns (labels int32 [n], -1 = noise;
        core mask bool [n]); with want_stats also a dict (clusters, core, border, noise, passes = propagation rounds, degree_ms /
        label_ms / finish_ms).  numpy in -> numpy out (po_dbscan: the matrix is copied to the device); torch CUDA tensor in ->
        tensors out on torch's current stream (po_dbscan_dev)."""
        is_t, matrix, code, n, ld = self._matrix_arg(matrix)
        if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)):
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "min_samples must be an integer (got %r)" % (min_samples,))
        res = PoDbscanResult()
        rp = ctypes.byref(res) if want_stats else None
        if is_t:
            import torch
            labels = torch.empty((n,), dtype=torch.int32, device=matrix.device)
            core = torch.empty((n,), dtype=torch.uint8, device=matrix.device)
            self._use_torch_stream()
            check(self._lib.po_dbscan_dev(self._h, matrix.data_ptr(), code, n, ld, float(eps), int(min_samples), labels.data_ptr(),
                                          core.data_ptr(), rp))
            core = core.view(torch.bool)
        else:
            labels = np.zeros(n, dtype=np.int32)
            core = np.zeros(n, dtype=np.uint8)
            check(self._lib.po_dbscan(self._h, _np_ptr(matrix), code, n, ld, float(eps), int(min_samples), _np_ptr(labels), _np_ptr(core), rp))
            core = core.view(np.bool_)
        if want_stats:
            return labels, core, {"clusters": res.clusters, "core": res.core, "border": res.border, "noise": res.noise,
                                  "passes": res.passes, "degree_ms": res.degree_ms, "label_ms": res.label_ms, "finish_ms": res.finish_ms}
        return labels, core

    # ---- row medians of a matrix (the reference's outlier clip) -----------------------------------
    def row_medians(self, matrix):
        """float64 [rows]: the median of every row of matrix [rows, n] (float32 / float64, unit inner stride, any row stride >= n),
        over all n columns: numpy.median(matrix.astype(float64), axis=1), exactly - R's apply(dist_matrix, 1, median) of
        bin/phyloselect.R:339-357 (po_row_medians_dev).  A row that holds a NaN gives NaN.  numpy in -> numpy out (the matrix is
        copied to the device); torch CUDA tensor in -> tensor out on torch's current stream."""
        import torch
        is_t, matrix, code, n, ld = self._matrix_on_device(matrix, square=False)
        rows = matrix.shape[0]
        out = torch.empty((rows,), dtype=torch.float64, device=matrix.device)
        self._use_torch_stream()
        check(self._lib.po_row_medians_dev(self._h, matrix.data_ptr(), code, rows, n, ld, out.data_ptr()))
        if n == 0:
            out.fill_(float("nan"))                      # numpy.median of an empty row
        return out if is_t else out.cpu().numpy()

    def row_medians_passes(self):
        """row reads of the last row_medians call, summed over its rows (po_row_medians_passes)"""
        v = ctypes.c_uint64()
        check(self._lib.po_row_medians_passes(self._h, ctypes.byref(v)))
        return v.value

    def _pairwise(self, counts, totals, freq, metric, row_begin, row_end, dtype, symmetric, out, want_stats,
                  extra_flags=0):
        if metric not in METRICS:
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "unknown metric %r" % (metric,))
        src = freq if freq is not None else counts
        n, dim = src.shape
        row_end = n if row_end is None else row_end
        rows = max(0, row_end - row_begin)
        f32 = str(dtype) in ("float32", "torch.float32", "f32")
        code = PO_F32 if f32 else PO_F64
        flags = (0 if symmetric else PO_FLAG_NO_SYMMETRY) | extra_flags
        stats = PoStats()
        sp = ctypes.byref(stats) if want_stats else None
        if _is_torch(src):
            import torch
            want = torch.float32 if f32 else torch.float64
            if src.device.type != "cuda" or src.device.index != self.device:
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "input tensor is on %s, this context drives cuda:%d" % (src.device, self.device))
            if out is None:
                out = torch.empty((rows, n), dtype=want, device=src.device)
            elif not (_is_torch(out) and out.dtype == want and out.device == src.device and out.dim() == 2 and
                      out.shape[0] >= rows and out.shape[1] >= n and (out.stride(1) == 1 or out.shape[1] <= 1)):
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "out must be a %s tensor [>=%d, >=%d] with unit inner stride on %s"
                                          % (want, rows, n, src.device))
            ld = out.stride(0) if rows > 1 else max(n, out.stride(0) if out.dim() == 2 else n)
            self._use_torch_stream()
            if freq is not None:
                assert freq.dtype == torch.float64 and freq.is_contiguous()
                check(self._lib.po_pairwise_freq_dev(self._h, freq.data_ptr(), n, dim, METRICS[metric], row_begin,
                                                     row_end, code, out.data_ptr(), ld, flags, sp))
            else:
                assert counts.dtype == torch.int32 and totals.dtype == torch.int64
                assert counts.is_contiguous() and totals.is_contiguous()
                check(self._lib.po_pairwise_dev(self._h, counts.data_ptr(), totals.data_ptr(), n, dim, METRICS[metric],
                                                row_begin, row_end, code, out.data_ptr(), ld, flags, sp))
        else:
            want = np.float32 if f32 else np.float64
            if out is None:
                out = np.zeros((rows, n), dtype=want)
            elif not (isinstance(out, np.ndarray) and out.dtype == want and out.ndim == 2 and out.flags.writeable and
                      out.shape[0] >= rows and out.shape[1] >= n and
                      (out.strides[1] == out.itemsize or out.shape[1] <= 1) and out.strides[0] % out.itemsize == 0 and
                      (out.strides[0] >= n * out.itemsize or rows <= 1)):
                raise _lib.PhyloligoError(_lib.PO_EINVAL, "out must be a writeable %s array [>=%d, >=%d] with unit inner stride"
                                          % (np.dtype(want).name, rows, n))
            ld = out.strides[0] // out.itemsize if rows > 0 and n > 0 else n
            if freq is not None:
                freq = np.ascontiguousarray(freq, dtype=np.float64)
                check(self._lib.po_pairwise_freq(self._h, _np_ptr(freq), n, dim, METRICS[metric], row_begin, row_end,
                                                 code, _np_ptr(out), max(ld, n), flags, sp))
            else:
                counts = np.ascontiguousarray(counts, dtype=np.uint32)
                totals = np.ascontiguousarray(totals, dtype=np.uint64)
                check(self._lib.po_pairwise(self._h, _np_ptr(counts), _np_ptr(totals), n, dim, METRICS[metric],
                                            row_begin, row_end, code, _np_ptr(out), max(ld, n), flags, sp))
        if want_stats:
            return out, {"prep_ms": stats.prep_ms, "kernel_ms": stats.kernel_ms, "total_ms": stats.total_ms,
                         "pairs": stats.pairs, "tiles": stats.tiles, "kernel_id": stats.kernel_id,
                    "rc_folded": bool(stats.rc_folded)}
        return out


def clip_threshold(medians, percentile):
    """The reference's clip threshold quantile(medians, probs=percentile) (bin/phyloselect.R:341), R's default type 7: with x the
    sorted medians and idx = (n - 1) * percentile, x[floor(idx)] when idx is whole, else the two neighbours interpolated.
    Host arithmetic on n doubles.  PO_EINVAL: percentile outside [0, 1], no medians, a NaN among them (the message names the row)."""
    x = np.asarray(medians, dtype=np.float64).ravel()
    if not 0.0 <= percentile <= 1.0:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "clip percentile must lie in [0, 1] (got %r)" % (percentile,))
    if x.size == 0:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "clip threshold of no medians")
    bad = np.flatnonzero(np.isnan(x))
    if bad.size:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "the median of row %d is NaN (the row holds a NaN, e.g. Bray-Curtis of an empty "
                                                  "record): the clip cannot order it" % int(bad[0]))
    x = np.sort(x)
    idx = (x.size - 1) * float(percentile)
    lo, hi = int(np.floor(idx)), int(np.ceil(idx))
    h = idx - lo
    if h == 0 or x[hi] == x[lo]:                         # (R interpolates only where the neighbours differ: ties at the threshold stay)
        return float(x[lo])
    return float((1.0 - h) * x[lo] + h * x[hi])


def clip_keep(medians, percentile, lengths=None, min_size=0):
    """int64 ascending indices of the records that survive the reference's two filters in its order (bin/phyloselect.R:339-357):
    first medians <= clip_threshold(medians, percentile), skipped when percentile == 1; then lengths >= min_size among the
    survivors, skipped when min_size == 0 (so a short record still takes part in the quantile)."""
    med = np.asarray(medians, dtype=np.float64).ravel()
    if not 0.0 <= percentile <= 1.0:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "clip percentile must lie in [0, 1] (got %r)" % (percentile,))
    if min_size < 0:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "min_size must not be negative (got %r)" % (min_size,))
    keep = np.arange(med.size, dtype=np.int64)
    if percentile != 1 and med.size:
        keep = keep[med <= clip_threshold(med, percentile)]
    if min_size != 0:
        if lengths is None or len(lengths) != med.size:
            raise _lib.PhyloligoError(_lib.PO_EINVAL, "min_size needs the length of every record (%d medians)" % med.size)
        keep = keep[np.asarray(lengths)[keep] >= min_size]
    return keep


def tsne_neighbours(n, perplexity):
    """neighbours per point t-SNE reads at this perplexity: min(n - 1, int(3 * perplexity + 1)), scikit-learn's n_neighbors"""
    return min(n - 1, int(3.0 * perplexity + 1))


def check_tsne_perplexity(perplexity):
    """perplexity of the t-SNE entry points: 1 <= p and int(3 p + 1) <= PO_KNN_MAX_K (PO_EINVAL otherwise)"""
    try:
        p = float(perplexity)
    except (TypeError, ValueError):
        p = float("nan")
    if not p >= 1.0 or int(3.0 * p + 1) > PO_KNN_MAX_K:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "perplexity must satisfy 1 <= perplexity and int(3 * perplexity + 1) <= %d, "
                                  "i.e. at most %d (got %r)" % (PO_KNN_MAX_K, (PO_KNN_MAX_K - 1) // 3, perplexity))
    return p


def tsne_start(n, seed=0):
    """scikit-learn's init="random": 1e-4 * RandomState(seed).standard_normal((n, 2)) as float32"""
    return (1e-4 * np.random.RandomState(seed).standard_normal(size=(n, 2))).astype(np.float32)


def _tsne_list_args(metric, val, perplexity):
    if metric not in METRICS:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "unknown metric %r" % (metric,))
    check_tsne_perplexity(perplexity)
    return METRICS[metric], str(val.dtype) in ("float32", "torch.float32")


def _tsne_params(max_iter, exploration_iter):
    params = PoTsneParams()
    params.max_iter = int(max_iter)
    params.exploration_iter = 0 if exploration_iter is None else int(exploration_iter)
    if int(max_iter) < 1 or params.exploration_iter < 0:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "max_iter must be at least 1 (got %r)" % (max_iter,))
    cap = int(max_iter) // 50 + 2
    hist = (ctypes.c_double * (3 * cap))()
    params.history = ctypes.cast(hist, ctypes.POINTER(ctypes.c_double))
    params.history_cap = cap
    return params, hist


def _tsne_stats(res, hist):
    m = min(res.history_len, len(hist) // 3)
    return {"kl": res.kl, "iterations": res.iterations, "grad_norm": res.grad_norm, "z": res.z,
            "history": [(int(hist[3 * i]), hist[3 * i + 1], hist[3 * i + 2]) for i in range(m)],
            "affinities_ms": res.affinities_ms, "optimise_ms": res.optimise_ms, "repulsion_ms": res.repulsion_ms,
            "attraction_ms": res.attraction_ms, "rest_ms": res.rest_ms}


def check_knn_k(k):
    """k of the k-NN entry points: an integer in 1..1024 (PO_EINVAL otherwise, as the library answers)"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= PO_KNN_MAX_K:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "k must be an integer in 1..%d (got %r)" % (PO_KNN_MAX_K, k))
    return int(k)


def _knn_args(metric, k, dtype):
    if metric not in METRICS:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "unknown metric %r" % (metric,))
    return METRICS[metric], check_knn_k(k), str(dtype) in ("float32", "torch.float32", "f32")


def _knn_stats(stats):
    return {"prep_ms": stats.prep_ms, "kernel_ms": stats.kernel_ms, "total_ms": stats.total_ms,
            "select_ms": max(0.0, stats.total_ms - stats.prep_ms - stats.kernel_ms), "pairs": stats.pairs,
            "tiles": stats.tiles, "kernel_id": stats.kernel_id, "rc_folded": bool(stats.rc_folded)}


def knn_self_values(metric, val, totals=None, counts=None):
    """The diagonal of the dense matrix for every record (what write_knn_npz puts first in each row): 0, except KT, whose
    diagonal is 1 - or 0 for a record whose profile is constant (all words tied)."""
    n = val.shape[0]
    out = np.zeros(n, dtype=val.dtype)
    if metric == "KT":
        c = np.asarray(counts)
        out[:] = 1
        if n:
            out[(c == c[:, :1]).all(axis=1)] = 0
    return out


def write_knn_npz(path, idx, val, self_value):
    """The k-NN graph as the CSR container scipy.sparse.save_npz writes (keys data, indices, indptr, format, shape): row i
    holds i itself with self_value (a scalar or one value per row: the dense diagonal) and then its neighbours in order.
    Written to exactly `path` (a file object, so that numpy does not append ".npz"); no scipy needed."""
    idx = np.asarray(idx)
    val = np.asarray(val)
    n, k = idx.shape
    data = np.empty((n, k + 1), dtype=val.dtype)
    indices = np.empty((n, k + 1), dtype=np.int32)
    data[:, 0] = self_value
    data[:, 1:] = val
    indices[:, 0] = np.arange(n, dtype=np.int32)
    indices[:, 1:] = idx
    indptr = np.arange(0, n * (k + 1) + 1, k + 1, dtype=np.int32 if n * (k + 1) < 2 ** 31 else np.int64)
    import zipfile
    # numpy.savez's layout (one .npy member per key, stored) with a fixed member time stamp: the same graph gives the same bytes
    with open(path, "wb") as fh, zipfile.ZipFile(fh, mode="w", compression=zipfile.ZIP_STORED, allowZip64=True) as zf:
        for key, arr in (("indices", indices.reshape(-1)), ("indptr", indptr), ("format", np.array("csr")),
                         ("shape", np.array([n, n], dtype=np.int64)), ("data", data.reshape(-1))):
            with zf.open(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w", force_zip64=True) as fid:
                np.lib.format.write_array(fid, np.asanyarray(arr), allow_pickle=False)


# ---- host formats -------------------------------------------------------------------------------
class _Titles:
    """Record titles of a FASTA file, decoded on demand (50 000 Python strings cost more than the parse)."""

    def __init__(self, blob, bounds):
        self._blob, self._bounds = blob, bounds

    def __len__(self):
        return len(self._bounds) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._blob[int(self._bounds[i]):int(self._bounds[i + 1])].tobytes().decode("latin-1")

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __eq__(self, other):
        return list(self) == list(other)


def fasta_index(data):
    """bytes / numpy uint8 of a FASTA file -> (seq uint8[total], offsets uint64[n+1], titles sequence)."""
    lib = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    buf = np.ascontiguousarray(buf)
    nrec, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.po_fasta_scan(_np_ptr(buf), buf.shape[0], ctypes.byref(nrec), ctypes.byref(nbytes)))
    seq = np.empty(nbytes.value, dtype=np.uint8)
    offsets = np.zeros(nrec.value + 1, dtype=np.uint64)
    tb = np.zeros(nrec.value, dtype=np.uint64)
    te = np.zeros(nrec.value, dtype=np.uint64)
    check(lib.po_fasta_extract(_np_ptr(buf), buf.shape[0], _np_ptr(seq), _np_ptr(offsets), _np_ptr(tb), _np_ptr(te)))
    # title bytes gathered into one blob (the file buffer may be a memmap that goes away)
    lens = (te - tb).astype(np.int64)
    bounds = np.zeros(nrec.value + 1, dtype=np.int64)
    np.cumsum(lens, out=bounds[1:])
    idx = np.repeat(tb.astype(np.int64) - bounds[:-1], lens) + np.arange(int(bounds[-1]), dtype=np.int64)
    return seq, offsets, _Titles(np.asarray(buf[idx]) if idx.size else np.zeros(0, np.uint8), bounds)


class _LineTitles:
    """Record titles of a device-parsed FASTA file: spans [begin, line end) into the host copy of the file bytes,
    right-stripped when decoded (the device leaves the trailing white space to whoever reads a title)."""

    def __init__(self, buf, begins, ends):
        self._buf, self._b, self._e = buf, begins, ends

    def __len__(self):
        return len(self._b)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._buf[int(self._b[i]):int(self._e[i])].tobytes().rstrip(b" \t\n\r\x0b\x0c").decode("latin-1")

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __eq__(self, other):
        return list(self) == list(other)


def fasta_index_dev(ctx, path, phases=None):
    """FASTA file -> (seq uint8 CUDA tensor, offsets int64 CUDA tensor [n+1], titles): the file bytes go to HBM as they
    are and are parsed there (po_fasta_scan_dev / po_fasta_extract_dev).  Raises PhyloligoError(PO_EUNSUPPORTED) for the
    one construct left to the host parser (tabs on sequence lines): callers fall back to fasta_index().
    phases: a dict that receives the wall time of every step in ms (the device is synchronised between steps only then)."""
    import os
    import time
    import torch
    lib = _lib.load()
    size = os.path.getsize(path)
    dev = torch.device("cuda", ctx.device)

    t_last = [time.perf_counter()]

    def mark(name):
        if phases is not None:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            phases[name] = phases.get(name, 0.0) + (now - t_last[0]) * 1e3
            t_last[0] = now

    buf = np.empty(size, dtype=np.uint8)
    check(lib.po_file_read(str(path).encode(), _np_ptr(buf), size))
    mark("file_read_ms")
    raw = torch.from_numpy(buf).to(dev)
    mark("file_h2d_ms")
    nrec, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
    ctx._use_torch_stream()
    check(lib.po_fasta_scan_dev(ctx._h, raw.data_ptr(), size, ctypes.byref(nrec), ctypes.byref(nbytes)))
    mark("fasta_scan_ms")
    seq = torch.empty(((nbytes.value + 15) // 16 * 16 or 16,), dtype=torch.uint8, device=dev)
    offsets = torch.zeros((nrec.value + 1,), dtype=torch.int64, device=dev)
    tb = torch.empty((max(1, nrec.value),), dtype=torch.int64, device=dev)
    te = torch.empty((max(1, nrec.value),), dtype=torch.int64, device=dev)
    mark("device_alloc_ms")
    check(lib.po_fasta_extract_dev(ctx._h, raw.data_ptr(), size, seq.data_ptr(), offsets.data_ptr(), tb.data_ptr(), te.data_ptr()))
    mark("fasta_extract_ms")
    titles = _LineTitles(buf, tb[:nrec.value].cpu().numpy(), te[:nrec.value].cpu().numpy())
    mark("title_spans_d2h_ms")
    return seq[:nbytes.value], offsets, titles


def write_mat_text(path, m, append=False):
    """numpy.savetxt(path, m, delimiter="\\t") byte for byte (bin/phyloligo.py:1061,1066)."""
    lib = _lib.load()
    if m is None:
        raise _lib.PhyloligoError(_lib.PO_EINVAL, "write_mat_text: no matrix to write (got None)")
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.ndim == 1:
        m = m.reshape(-1, 1)      # savetxt writes a 1-D array one value per line
    rows, cols = m.shape
    check(lib.po_write_mat_text(_np_ptr(m), rows, cols, cols, str(path).encode(), 1 if append else 0))
