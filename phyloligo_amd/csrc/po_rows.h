// Internal: what the translation units that read a matrix in HBM row by row share (po_kmedoids.hip, po_silhouette.hip,
// po_rowmedian.hip; po_knn.hip takes the vector type).
//
// The summation order of a row.  The masked and unmasked row sums of k-medoids (kmed_rowsum_kernel) and the per-cluster sums of
// the silhouettes (sil_sums_kernel) promise the same bytes for the same (row, labels, cluster, n) - whatever the launch, the rows
// that share a workgroup, the other clusters a thread accumulates, the leading dimension or the alignment of the row.  Both
// kernels keep that promise by building a sum from the steps below and from nothing else:
//   - columns are cut into groups of V = 16 bytes / element size (4 float32, 2 float64); group g belongs to thread g mod 256
//     of the row's workgroup, which walks its groups in ascending order and keeps one float64 accumulator per position
//     inside the group (V independent chains); the last, partial group is a short group on thread (n / V) mod 256, added after
//     that thread's whole groups;
//   - rows on 16-byte boundaries (base and leading dimension, po_rows_aligned) are read with one 16-byte load per group, any
//     other layout with V element loads of the same group (po_load_group): same order, same bytes out;
//   - excluded entries are replaced by +0 with a select, never multiplied, so a NaN outside the cluster stays outside; every
//     value is converted to float64 before it is added;
//   - a thread ends with ((a0 + a1) + (a2 + a3)) (po_thread_tree), a wave with the fixed shuffle tree (po_wave_sum_fixed), the
//     four waves with ((w0 + w1) + (w2 + w3)) (po_block_tree).
#pragma once

#include "po_internal.h"

#if defined(__HIPCC__)
template <typename T> struct po_vec16;
template <> struct po_vec16<float> { using type = float4; };
template <> struct po_vec16<double> { using type = double2; };
template <int V> struct po_ivec;
template <> struct po_ivec<4> { using type = int4; };
template <> struct po_ivec<2> { using type = int2; };

__device__ __forceinline__ double po_wave_sum_fixed(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                                              // lane 0 holds the sum
}

// v = the V elements of the group that starts at column j0: one 16-byte load (row + j0 on a 16-byte boundary) or V element loads
template <typename T, bool ALIGNED, int V>
__device__ __forceinline__ void po_load_group(const T* row, uint32_t j0, T (&v)[V]) {
    static_assert(V * sizeof(T) == 16, "a group is 16 bytes");
    if (ALIGNED) {
        const typename po_vec16<T>::type q = *reinterpret_cast<const typename po_vec16<T>::type*>(row + j0);
        const T* qp = reinterpret_cast<const T*>(&q);
#pragma unroll
        for (uint32_t u = 0; u < V; ++u) v[u] = qp[u];
    } else {
#pragma unroll
        for (uint32_t u = 0; u < V; ++u) v[u] = row[j0 + u];
    }
}

// l = labels[j0 .. j0 + V) in one load; labels starts on a 16-byte boundary and j0 is a multiple of V
template <int V>
__device__ __forceinline__ void po_load_labels(const int32_t* labels, uint32_t j0, int32_t (&l)[V]) {
    const typename po_ivec<V>::type q = *reinterpret_cast<const typename po_ivec<V>::type*>(labels + j0);
    const int32_t* qp = reinterpret_cast<const int32_t*>(&q);
#pragma unroll
    for (uint32_t u = 0; u < V; ++u) l[u] = qp[u];
}

template <int V>
__device__ __forceinline__ double po_thread_tree(const double (&a)[V]) {
    static_assert(V == 4 || V == 2, "4 float32 or 2 float64 positions");
    if constexpr (V == 4) return (a[0] + a[1]) + (a[2] + a[3]);
    else return a[0] + a[1];
}

__device__ __forceinline__ double po_block_tree(const double (&w)[4]) { return (w[0] + w[1]) + (w[2] + w[3]); }

// The end of the one-workgroup kernels (1024 threads, all of which call this once): the sum of every thread's v by the wave
// tree, sixteen wave totals in LDS and a serial add of the sixteen in index order.  Thread 0 holds the sum.
__device__ __forceinline__ double po_block1024_sum(double v) {
    __shared__ double part[16];
    const uint32_t tid = threadIdx.x;
    v = po_wave_sum_fixed(v);
    if ((tid & 63u) == 0) part[tid >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (tid == 0)
        for (int w = 0; w < 16; ++w) t += part[w];
    return t;
}
#endif

// ---- host side ------------------------------------------------------------------------------------------------------------------
// rows of the matrix on 16-byte boundaries: the one-load-per-group kernels
inline bool po_rows_aligned(const void* d, uint64_t ld, size_t esz) { return (reinterpret_cast<uintptr_t>(d) & 15u) == 0 && (ld * esz) % 16 == 0; }

// the checks every entry point makes of a square n x n matrix argument (device or host pointer)
inline int po_check_matrix_args(const char* who, po_ctx* ctx, const void* m, int dtype, uint64_t n, uint64_t ld) {
    PO_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    PO_REQUIRE(dtype == PO_F64 || dtype == PO_F32, "%s: dtype must be PO_F64 or PO_F32 (got %d)", who, dtype);
    PO_REQUIRE(n >= 1 && n < (1ull << 31), "%s: n = %llu outside 1 .. 2^31 - 1", who, (unsigned long long)n);
    PO_REQUIRE(ld >= n, "%s: ld = %llu is smaller than n = %llu", who, (unsigned long long)ld, (unsigned long long)n);
    PO_REQUIRE(m != nullptr, "%s: the matrix pointer is NULL", who);
    const size_t esz = dtype == PO_F32 ? 4 : 8;
    PO_REQUIRE((reinterpret_cast<uintptr_t>(m) % esz) == 0, "%s: the matrix pointer is not aligned to its element size", who);
    return PO_OK;
}

// device values v[count] all inside [0, limit)?  d_flag_word: a device word of the caller's workspace, h_word: a pinned host
// word.  One synchronisation.  *bad: the first offending position or 0xFFFFFFFF.  (po_kmedoids.hip)
int po_check_index_range(po_ctx* ctx, uint32_t* d_flag_word, uint32_t* h_word, const int32_t* v, uint32_t count, uint32_t limit, uint32_t* bad);

// The host-pointer entry points: ctx->ws_io = [the n x n matrix on 16-byte rows | extra_bytes], the matrix copy enqueued.
inline int po_stage_host_matrix(const char* who, po_ctx* ctx, const void* matrix, int dtype, uint64_t n, uint64_t ld, size_t extra_bytes,
                                void** d_matrix, uint64_t* ld_dev, uint8_t** d_extra) {
    const size_t esz = dtype == PO_F32 ? 4 : 8;
    *ld_dev = po_round_up(n, 16 / esz);
    const size_t b_mat = po_round_up(n * *ld_dev * esz, 256);
    const int rc = po_buf_reserve(ctx, &ctx->ws_io, b_mat + extra_bytes);
    if (rc == PO_ENOMEM) {
        po_set_error("%s: the %llu x %llu %s matrix (%.1f GB) does not fit the device memory that is free%s", who, (unsigned long long)n,
                     (unsigned long long)n, dtype == PO_F32 ? "float32" : "float64", (double)b_mat / 1e9,
                     dtype == PO_F32 ? "" : "; a float32 matrix takes half");
        return PO_ENOMEM;
    }
    if (rc) return rc;
    uint8_t* base = static_cast<uint8_t*>(ctx->ws_io.p);
    *d_matrix = base;
    *d_extra = base + b_mat;
    PO_HIP(hipMemcpy2DAsync(base, *ld_dev * esz, matrix, ld * esz, n * esz, n, hipMemcpyHostToDevice, ctx->stream));
    return PO_OK;
}
