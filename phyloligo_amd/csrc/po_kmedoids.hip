// k-medoids on a distance matrix in HBM (po_kmedoids*, include/phyloligo_amd.h): the KMedoids class of the reference's
// bin/phyloselect.py:37-309 as it is called there (distance_metric="precomputed", :578-595, :647), decision for decision.
//
// One iteration is   assign -> masked row sums -> per-cluster argmin -> medoid update   and one 4-byte flag read back:
//   assign     label[j] = argmin_c D[medoid[c]][j], one thread per column, the smaller c wins a tie            K n reads
//   row sums   for every pair (row, target):  sum over j with label[j] == target of D[row][j], float64      (n + K) n reads
//              the n pairs (i, label[i]) are the candidate costs of the update, the K pairs (medoid[c], c) the current
//              costs; the heuristic start is the same kernel without a mask.  This is the hot path: it only reads, so its
//              roof is the HBM read rate.
//   argmin     order-preserving 64-bit keys of the costs, integer atomicMin per cluster, then the smallest index among the
//              rows that hold the minimum - no floating-point atomics anywhere
//   update     medoid[c] <- that row if its cost is strictly below the current cost; a changed-flag for the host
//
// The row-sum kernel.  A row's sum depends on the row, the labels and n only - not on the launch, the rows that share a
// workgroup, the leading dimension or the alignment of the row: it keeps the summation order written at the top of po_rows.h,
// and takes every step of it from there.
// A workgroup carries R rows (4 float32 / 2 float64: 0.8 MB of matrix per workgroup at 50 000 columns) through the same
// groups, so the labels of a group - 4 bytes per column, from L2 - are loaded once for R rows of matrix from HBM.
#include "po_rows.h"

#include <algorithm>
#include <vector>

namespace {

constexpr uint32_t kThreads = 256;
// pair p: row prow[p] (NULL: p), target ptgt[p] (NULL: labels[row]); MASKED = false: every column counts (labels unused)
template <typename T, int R, bool ALIGNED, bool MASKED>
__global__ __launch_bounds__(kThreads) void kmed_rowsum_kernel(const T* __restrict__ D, uint64_t ld, uint32_t n,
                                                               const int32_t* __restrict__ prow, const int32_t* __restrict__ ptgt,
                                                               const int32_t* __restrict__ labels, uint32_t npairs,
                                                               double* __restrict__ out) {
    constexpr uint32_t V = 16 / sizeof(T);
    __shared__ double wsum[R][kThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint32_t p0 = blockIdx.x * R;
    const T* s[R];
    int32_t tgt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t p = p0 + r < npairs ? p0 + r : npairs - 1;           // a short last workgroup repeats its last pair
        const uint32_t row = prow ? static_cast<uint32_t>(prow[p]) : p;
        s[r] = D + static_cast<uint64_t>(row) * ld;
        tgt[r] = MASKED ? (ptgt ? ptgt[p] : labels[row]) : 0;
    }
    double acc[R][V];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (uint32_t u = 0; u < V; ++u) acc[r][u] = 0.0;

    const uint32_t full = n / V;                                            // whole groups
    for (uint32_t g = tid; g < full; g += kThreads) {
        const uint32_t j0 = g * V;
        int32_t lab[V];
        if (MASKED) po_load_labels<V>(labels, j0, lab);
        T v[R][V];
#pragma unroll
        for (int r = 0; r < R; ++r) po_load_group<T, ALIGNED>(s[r], j0, v[r]);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (uint32_t u = 0; u < V; ++u) {
                const T x = (!MASKED || lab[u] == tgt[r]) ? v[r][u] : T(0);
                acc[r][u] += static_cast<double>(x);
            }
    }
    if (tid == (full & (kThreads - 1))) {                                   // the short group, after the thread's whole ones
#pragma unroll
        for (uint32_t u = 0; u + 1 < V; ++u) {
            const uint32_t j = full * V + u;
            if (j < n) {
                const int32_t lab = MASKED ? labels[j] : 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const T x = (!MASKED || lab == tgt[r]) ? s[r][j] : T(0);
                    acc[r][u] += static_cast<double>(x);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double t = po_wave_sum_fixed(po_thread_tree(acc[r]));
        if ((tid & 63u) == 0) wsum[r][tid >> 6] = t;
    }
    __syncthreads();
    if (tid < R && p0 + tid < npairs) out[p0 + tid] = po_block_tree(wsum[tid]);
}

// prow[0, n) = row index, ptgt[n, n + K) = cluster index: the fixed halves of the pair list
__global__ __launch_bounds__(kThreads) void kmed_iota_kernel(int32_t* __restrict__ prow, int32_t* __restrict__ ptgt, uint32_t n, uint32_t K) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) prow[i] = static_cast<int32_t>(i);
    if (i < K) ptgt[n + i] = static_cast<int32_t>(i);
}

// label[j] = argmin_c D[med[c]][j]: strict <, so the first minimum (the smaller c) wins and a NaN never does
template <typename T>
__global__ __launch_bounds__(kThreads) void kmed_assign_kernel(const T* __restrict__ D, uint64_t ld, uint32_t n, const int32_t* __restrict__ med,
                                                               uint32_t K, int32_t* __restrict__ labels) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    T best = D[static_cast<uint64_t>(static_cast<uint32_t>(med[0])) * ld + j];
    int32_t arg = 0;
    for (uint32_t c = 1; c < K; ++c) {
        const T v = D[static_cast<uint64_t>(static_cast<uint32_t>(med[c])) * ld + j];
        if (v < best) {
            best = v;
            arg = static_cast<int32_t>(c);
        }
    }
    labels[j] = arg;
}

// per cluster: the smallest order-preserving key (po_order_key: -0 = +0, NaN above +inf) among its members' costs ...
__global__ __launch_bounds__(kThreads) void kmed_best_kernel(const double* __restrict__ cost, const int32_t* __restrict__ labels, uint32_t n,
                                                             uint32_t K, unsigned long long* __restrict__ best) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = static_cast<uint32_t>(labels[i]);
    if (c >= K) return;
    // the minimum only ever falls, so a key that does not beat what the word holds now (even a stale view of it) cannot
    // beat the final value either: most rows skip the atomic, which K words would otherwise serialise
    const unsigned long long key = po_order_key(cost[i], false);
    if (key < *reinterpret_cast<volatile unsigned long long*>(&best[c])) atomicMin(&best[c], key);
}

// ... and the smallest row that holds it
__global__ __launch_bounds__(kThreads) void kmed_best_row_kernel(const double* __restrict__ cost, const int32_t* __restrict__ labels, uint32_t n,
                                                                 uint32_t K, const unsigned long long* __restrict__ best,
                                                                 uint32_t* __restrict__ best_row) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = static_cast<uint32_t>(labels[i]);
    if (c < K && best[c] == po_order_key(cost[i], false)) atomicMin(&best_row[c], i);
}

// cost[n + c]: the current medoid's sum over the cluster.  An empty cluster (no row lowered best_row) keeps its medoid.
__global__ __launch_bounds__(kThreads) void kmed_update_kernel(const double* __restrict__ cost, uint32_t n, uint32_t K,
                                                               const uint32_t* __restrict__ best_row, int32_t* __restrict__ med,
                                                               uint32_t* __restrict__ changed) {
    const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= K) return;
    const uint32_t i = best_row[c];
    if (i >= n) return;
    if (cost[i] < cost[n + c] && med[c] != static_cast<int32_t>(i)) {
        med[c] = static_cast<int32_t>(i);
        atomicOr(changed, 1u);
    }
}

// first position whose value is outside [0, limit)
__global__ __launch_bounds__(kThreads) void kmed_check_range_kernel(const int32_t* __restrict__ v, uint32_t count, uint32_t limit,
                                                                    uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < count && (v[i] < 0 || static_cast<uint32_t>(v[i]) >= limit)) atomicMin(err, i);
}

// One workgroup: inertia = sum_j D[med[label[j]]][j] (per-thread strided partial sums, po_block1024_sum) and the number of clusters
// without a member.  cnt [K] is zero on entry.
template <typename T>
__global__ __launch_bounds__(1024) void kmed_finish_kernel(const T* __restrict__ D, uint64_t ld, uint32_t n, const int32_t* __restrict__ med,
                                                           const int32_t* __restrict__ labels, uint32_t K, uint32_t* __restrict__ cnt,
                                                           double* __restrict__ inertia, uint32_t* __restrict__ n_empty) {
    __shared__ uint32_t empties;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) empties = 0;
    double acc = 0.0;
    for (uint32_t j = tid; j < n; j += 1024) {
        const uint32_t c = static_cast<uint32_t>(labels[j]);
        acc += static_cast<double>(D[static_cast<uint64_t>(static_cast<uint32_t>(med[c])) * ld + j]);
        atomicAdd(&cnt[c], 1u);
    }
    __threadfence();
    const double total = po_block1024_sum(acc);                             // (its barrier also stands between the two uses of cnt)
    uint32_t mine = 0;
    for (uint32_t c = tid; c < K; c += 1024) mine += atomicAdd(&cnt[c], 0u) == 0 ? 1u : 0u;
    if (mine) atomicAdd(&empties, mine);
    __syncthreads();
    if (tid == 0) {
        *inertia = total;
        *n_empty = empties;
    }
}

// ---- workspace of one problem (ctx->ws_kmed) ----------------------------------------------------------------------------------
struct kmed_ws {
    int32_t* prow;                  // [n + K]: 0 .. n-1, then the medoids
    int32_t* ptgt;                  // [n + K]: the labels, then 0 .. K-1
    double* cost;                   // [n + K]
    unsigned long long* best;       // [K]
    uint32_t* best_row;             // [K]   (directly behind best: one memset fills both)
    uint32_t* cnt;                  // [K]
    uint32_t* flag;                 // [4]: changed, range error, empty clusters
    double* scal;                   // [2]: inertia
    size_t fill_bytes;              // best + best_row
};

size_t kmed_ws_layout(uint64_t n, uint32_t K, uint8_t* base, kmed_ws* w) {
    po_carver ws{base};
    const uint64_t m = n + K;
    uint8_t* a = ws.take(m * 4);
    uint8_t* b = ws.take(m * 4);
    uint8_t* c = ws.take(m * 8);
    uint8_t* d = ws.take((size_t)K * 8 + (size_t)K * 4);
    uint8_t* e = ws.take((size_t)K * 4);
    uint8_t* f = ws.take(16);
    uint8_t* g = ws.take(16);
    if (w) {
        w->prow = reinterpret_cast<int32_t*>(a);
        w->ptgt = reinterpret_cast<int32_t*>(b);
        w->cost = reinterpret_cast<double*>(c);
        w->best = reinterpret_cast<unsigned long long*>(d);
        w->best_row = reinterpret_cast<uint32_t*>(d + (size_t)K * 8);
        w->cnt = reinterpret_cast<uint32_t*>(e);
        w->flag = reinterpret_cast<uint32_t*>(f);
        w->scal = reinterpret_cast<double*>(g);
        w->fill_bytes = (size_t)K * 12;
    }
    return ws.off;
}

int kmed_pinned(po_ctx* ctx) {
    if (!ctx->h_kmed) PO_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_kmed), 8 * sizeof(double), hipHostMallocDefault));
    return PO_OK;
}

int kmed_workspace(po_ctx* ctx, uint64_t n, uint32_t K, kmed_ws* w) {
    int rc = kmed_pinned(ctx);
    if (rc) return rc;
    rc = po_buf_reserve(ctx, &ctx->ws_kmed, kmed_ws_layout(n, K, nullptr, nullptr));
    if (rc) return rc;
    kmed_ws_layout(n, K, static_cast<uint8_t*>(ctx->ws_kmed.p), w);
    return PO_OK;
}

template <typename T, int R>
int launch_rowsum_t(po_ctx* ctx, const T* D, uint64_t ld, uint32_t n, const int32_t* prow, const int32_t* ptgt, const int32_t* labels,
                    uint32_t npairs, double* out) {
    const dim3 grid((npairs + R - 1) / R), block(kThreads);
    const bool al = po_rows_aligned(D, ld, sizeof(T));
    if (labels) {
        if (al) hipLaunchKernelGGL((kmed_rowsum_kernel<T, R, true, true>), grid, block, 0, ctx->stream, D, ld, n, prow, ptgt, labels, npairs, out);
        else hipLaunchKernelGGL((kmed_rowsum_kernel<T, R, false, true>), grid, block, 0, ctx->stream, D, ld, n, prow, ptgt, labels, npairs, out);
    } else {
        if (al) hipLaunchKernelGGL((kmed_rowsum_kernel<T, R, true, false>), grid, block, 0, ctx->stream, D, ld, n, prow, ptgt, labels, npairs, out);
        else hipLaunchKernelGGL((kmed_rowsum_kernel<T, R, false, false>), grid, block, 0, ctx->stream, D, ld, n, prow, ptgt, labels, npairs, out);
    }
    PO_CHECK_LAUNCH("kmed_rowsum_kernel");
    return PO_OK;
}

// labels NULL: plain row sums.  labels must start on a 16-byte boundary (the workspace's do).
int launch_rowsum(po_ctx* ctx, const void* D, int f32, uint64_t ld, uint32_t n, const int32_t* prow, const int32_t* ptgt,
                  const int32_t* labels, uint32_t npairs, double* out) {
    if (npairs == 0) return PO_OK;
    if (f32) return launch_rowsum_t<float, 4>(ctx, static_cast<const float*>(D), ld, n, prow, ptgt, labels, npairs, out);
    return launch_rowsum_t<double, 2>(ctx, static_cast<const double*>(D), ld, n, prow, ptgt, labels, npairs, out);
}

int launch_assign(po_ctx* ctx, const void* D, int f32, uint64_t ld, uint32_t n, const int32_t* med, uint32_t K, int32_t* labels) {
    const dim3 grid((n + kThreads - 1) / kThreads), block(kThreads);
    if (f32) hipLaunchKernelGGL(kmed_assign_kernel<float>, grid, block, 0, ctx->stream, static_cast<const float*>(D), ld, n, med, K, labels);
    else hipLaunchKernelGGL(kmed_assign_kernel<double>, grid, block, 0, ctx->stream, static_cast<const double*>(D), ld, n, med, K, labels);
    PO_CHECK_LAUNCH("kmed_assign_kernel");
    return PO_OK;
}

}  // namespace

int po_check_index_range(po_ctx* ctx, uint32_t* d_flag_word, uint32_t* h_word, const int32_t* v, uint32_t count, uint32_t limit, uint32_t* bad) {
    PO_HIP(hipMemsetAsync(d_flag_word, 0xFF, 4, ctx->stream));
    hipLaunchKernelGGL(kmed_check_range_kernel, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, v, count, limit, d_flag_word);
    PO_CHECK_LAUNCH("kmed_check_range_kernel");
    PO_HIP(hipMemcpyAsync(h_word, d_flag_word, 4, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    *bad = *h_word;
    return PO_OK;
}

extern "C" int po_kmedoids_costs_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, const int32_t* d_labels,
                                     const int32_t* d_rows, uint64_t n_rows, double* d_costs) {
    const char* who = "po_kmedoids_costs_dev";
    int rc = po_check_matrix_args(who, ctx, d_matrix, dtype, n, ld);
    if (rc) return rc;
    PO_REQUIRE(d_labels != nullptr && d_costs != nullptr, "%s: NULL buffer", who);
    PO_REQUIRE(d_rows != nullptr || n_rows == 0 || n_rows == n, "%s: n_rows = %llu without a row list (pass 0 or n)", who,
               (unsigned long long)n_rows);
    PO_REQUIRE(n_rows < (1ull << 31), "%s: n_rows = %llu is too large", who, (unsigned long long)n_rows);
    PO_HIP(hipSetDevice(ctx->device));
    kmed_ws w;
    rc = kmed_workspace(ctx, n, 1, &w);
    if (rc) return rc;
    const uint32_t count = d_rows ? (uint32_t)n_rows : (uint32_t)n;
    if (d_rows && count) {
        uint32_t bad = 0;
        rc = po_check_index_range(ctx, w.flag + 1, reinterpret_cast<uint32_t*>(ctx->h_kmed), d_rows, count, (uint32_t)n, &bad);
        if (rc) return rc;
        PO_REQUIRE(bad == 0xFFFFFFFFu, "%s: rows[%u] is outside 0 .. n-1", who, bad);
    }
    PO_HIP(hipMemcpyAsync(w.ptgt, d_labels, n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    return launch_rowsum(ctx, d_matrix, dtype == PO_F32, ld, (uint32_t)n, d_rows, nullptr, w.ptgt, count, d_costs);
}

extern "C" int po_kmedoids_assign_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, uint32_t n_clusters,
                                      const int32_t* d_medoids, int32_t* d_labels) {
    const char* who = "po_kmedoids_assign_dev";
    int rc = po_check_matrix_args(who, ctx, d_matrix, dtype, n, ld);
    if (rc) return rc;
    PO_REQUIRE(n_clusters >= 1 && n_clusters <= n, "%s: n_clusters = %u outside 1 .. n = %llu", who, n_clusters, (unsigned long long)n);
    PO_REQUIRE(d_medoids != nullptr && d_labels != nullptr, "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    kmed_ws w;
    rc = kmed_workspace(ctx, n, n_clusters, &w);
    if (rc) return rc;
    uint32_t bad = 0;
    rc = po_check_index_range(ctx, w.flag + 1, reinterpret_cast<uint32_t*>(ctx->h_kmed), d_medoids, n_clusters, (uint32_t)n, &bad);
    if (rc) return rc;
    PO_REQUIRE(bad == 0xFFFFFFFFu, "%s: medoids[%u] is outside 0 .. n-1", who, bad);
    return launch_assign(ctx, d_matrix, dtype == PO_F32, ld, (uint32_t)n, d_medoids, n_clusters, d_labels);
}

extern "C" int po_kmedoids_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, uint32_t n_clusters,
                               const int32_t* init_medoids, uint32_t max_iter, int32_t* d_labels, int32_t* d_medoids,
                               po_kmedoids_result* result) {
    const char* who = "po_kmedoids_dev";
    if (result) memset(result, 0, sizeof(*result));
    int rc = po_check_matrix_args(who, ctx, d_matrix, dtype, n, ld);
    if (rc) return rc;
    const uint32_t K = n_clusters, N = (uint32_t)n;
    PO_REQUIRE(K >= 1 && K <= n, "%s: n_clusters = %u outside 1 .. n = %llu", who, K, (unsigned long long)n);
    PO_REQUIRE(max_iter >= 1, "%s: max_iter must be at least 1", who);
    PO_REQUIRE(d_labels != nullptr && d_medoids != nullptr, "%s: NULL buffer", who);
    if (init_medoids) {
        std::vector<int32_t> seen(init_medoids, init_medoids + K);
        for (uint32_t c = 0; c < K; ++c)
            PO_REQUIRE(seen[c] >= 0 && (uint64_t)seen[c] < n, "%s: init_medoids[%u] = %d is outside 0 .. n-1", who, c, seen[c]);
        std::sort(seen.begin(), seen.end());
        for (uint32_t c = 1; c < K; ++c) PO_REQUIRE(seen[c] != seen[c - 1], "%s: init_medoids names row %d twice", who, seen[c]);
    }
    PO_HIP(hipSetDevice(ctx->device));
    kmed_ws w;
    rc = kmed_workspace(ctx, n, K, &w);
    if (rc) return rc;
    const int f32 = dtype == PO_F32;
    const bool timed = result != nullptr;
    float ms = 0.0f;
    int32_t* med = w.prow + n;
    int32_t* labels = w.ptgt;

    // ---- start ----
    if (timed) PO_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    hipLaunchKernelGGL(kmed_iota_kernel, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, w.prow, w.ptgt, N, K);
    PO_CHECK_LAUNCH("kmed_iota_kernel");
    std::vector<int32_t> start(K);
    if (init_medoids) {
        std::copy(init_medoids, init_medoids + K, start.begin());
    } else {
        // the K rows with the smallest sums, ascending, ties to the smaller row: numpy.argsort(numpy.sum(D, axis=1))[:K]
        rc = launch_rowsum(ctx, d_matrix, f32, ld, N, nullptr, nullptr, nullptr, N, w.cost);
        if (rc) return rc;
        std::vector<double> sums(n);
        PO_HIP(hipMemcpyAsync(sums.data(), w.cost, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipStreamSynchronize(ctx->stream));
        for (uint64_t i = 0; i < n; ++i)
            PO_REQUIRE(sums[i] == sums[i], "%s: row %llu of the matrix sums to NaN: the heuristic start cannot order it "
                       "(Bray-Curtis of an empty record is 0/0; drop the record or pass init_medoids)", who, (unsigned long long)i);
        std::vector<int32_t> order(n);
        for (uint64_t i = 0; i < n; ++i) order[i] = (int32_t)i;
        std::partial_sort(order.begin(), order.begin() + K, order.end(),
                          [&](int32_t a, int32_t b) { return sums[a] < sums[b] || (sums[a] == sums[b] && a < b); });
        std::copy(order.begin(), order.begin() + K, start.begin());
    }
    PO_HIP(hipMemcpyAsync(med, start.data(), (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));                              // `start` is pageable host memory
    if (timed) {
        PO_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
        PO_HIP(hipEventSynchronize(ctx->ev[1]));
        PO_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        result->start_ms = ms;
    }

    // ---- iterations ----
    uint32_t* h_flag = reinterpret_cast<uint32_t*>(ctx->h_kmed);
    uint32_t iterations = 0, converged = 0;
    const dim3 ngrid((N + kThreads - 1) / kThreads), kgrid((K + kThreads - 1) / kThreads), block(kThreads);
    double t_assign = 0.0, t_rowsum = 0.0, t_update = 0.0;
    for (;;) {
        ++iterations;
        if (timed) PO_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
        rc = launch_assign(ctx, d_matrix, f32, ld, N, med, K, labels);
        if (rc) return rc;
        if (timed) PO_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
        rc = launch_rowsum(ctx, d_matrix, f32, ld, N, w.prow, w.ptgt, labels, N + K, w.cost);
        if (rc) return rc;
        if (timed) PO_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
        PO_HIP(hipMemsetAsync(w.best, 0xFF, w.fill_bytes, ctx->stream));
        PO_HIP(hipMemsetAsync(w.flag, 0, 4, ctx->stream));
        hipLaunchKernelGGL(kmed_best_kernel, ngrid, block, 0, ctx->stream, w.cost, labels, N, K, w.best);
        PO_CHECK_LAUNCH("kmed_best_kernel");
        hipLaunchKernelGGL(kmed_best_row_kernel, ngrid, block, 0, ctx->stream, w.cost, labels, N, K, w.best, w.best_row);
        PO_CHECK_LAUNCH("kmed_best_row_kernel");
        hipLaunchKernelGGL(kmed_update_kernel, kgrid, block, 0, ctx->stream, w.cost, N, K, w.best_row, med, w.flag);
        PO_CHECK_LAUNCH("kmed_update_kernel");
        if (timed) PO_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
        PO_HIP(hipMemcpyAsync(h_flag, w.flag, 4, hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipStreamSynchronize(ctx->stream));
        if (timed) {
            PO_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
            t_assign += ms;
            PO_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
            t_rowsum += ms;
            PO_HIP(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]));
            t_update += ms;
        }
        if (h_flag[0] == 0) {
            converged = 1;
            break;
        }
        if (iterations >= max_iter) break;
    }

    // ---- results: the labels of the last assignment, the medoids after the last update ----
    PO_HIP(hipMemcpyAsync(d_labels, labels, n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    PO_HIP(hipMemcpyAsync(d_medoids, med, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    if (result) {
        PO_HIP(hipMemsetAsync(w.cnt, 0, (size_t)K * 4, ctx->stream));
        if (f32)
            hipLaunchKernelGGL(kmed_finish_kernel<float>, dim3(1), dim3(1024), 0, ctx->stream, static_cast<const float*>(d_matrix), ld, N, med,
                               labels, K, w.cnt, w.scal, w.flag + 2);
        else
            hipLaunchKernelGGL(kmed_finish_kernel<double>, dim3(1), dim3(1024), 0, ctx->stream, static_cast<const double*>(d_matrix), ld, N, med,
                               labels, K, w.cnt, w.scal, w.flag + 2);
        PO_CHECK_LAUNCH("kmed_finish_kernel");
        PO_HIP(hipMemcpyAsync(ctx->h_kmed, w.scal, 8, hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipMemcpyAsync(ctx->h_kmed + 1, w.flag + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipStreamSynchronize(ctx->stream));
        result->inertia = ctx->h_kmed[0];
        result->empty_clusters = *reinterpret_cast<uint32_t*>(ctx->h_kmed + 1);
        result->iterations = iterations;
        result->converged = converged;
        result->assign_ms = t_assign;
        result->rowsum_ms = t_rowsum;
        result->update_ms = t_update;
    }
    return PO_OK;
}

extern "C" int po_kmedoids(po_ctx* ctx, const void* matrix, int dtype, uint64_t n, uint64_t ld, uint32_t n_clusters,
                           const int32_t* init_medoids, uint32_t max_iter, int32_t* labels, int32_t* medoids, po_kmedoids_result* result) {
    const char* who = "po_kmedoids";
    if (result) memset(result, 0, sizeof(*result));
    int rc = po_check_matrix_args(who, ctx, matrix, dtype, n, ld);
    if (rc) return rc;
    PO_REQUIRE(n_clusters >= 1 && n_clusters <= n, "%s: n_clusters = %u outside 1 .. n = %llu", who, n_clusters, (unsigned long long)n);
    PO_REQUIRE(max_iter >= 1, "%s: max_iter must be at least 1", who);
    PO_REQUIRE(labels != nullptr && medoids != nullptr, "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    const size_t b_lab = po_round_up(n * 4, 256), b_med = po_round_up((size_t)n_clusters * 4, 256);
    void* base;
    uint64_t ld_dev;
    uint8_t* extra;
    rc = po_stage_host_matrix(who, ctx, matrix, dtype, n, ld, b_lab + b_med, &base, &ld_dev, &extra);
    if (rc) return rc;
    int32_t* d_labels = reinterpret_cast<int32_t*>(extra);
    int32_t* d_medoids = reinterpret_cast<int32_t*>(extra + b_lab);
    rc = po_kmedoids_dev(ctx, base, dtype, n, ld_dev, n_clusters, init_medoids, max_iter, d_labels, d_medoids, result);
    if (rc) return rc;
    PO_HIP(hipMemcpyAsync(labels, d_labels, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipMemcpyAsync(medoids, d_medoids, (size_t)n_clusters * 4, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    return PO_OK;
}
