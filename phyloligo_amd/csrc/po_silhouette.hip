// Silhouettes of a clustering of a distance matrix in HBM (po_cluster_sums_dev / po_silhouette*, include/phyloligo_amd.h): what
// sklearn.metrics.silhouette_samples(D, labels, metric="precomputed") computes, with the two rules of the header block that
// scikit-learn does not have (empty clusters are skipped, a NaN sum gives NaN).
//
//   histogram   sizes[c] = number of columns with label c (integer atomics) and the first label outside 0 .. K-1      n reads
//   sums        S[i][c] = float64 sum over j with label[j] == c of D[i][j], for a chunk of up to kChunk clusters
//               at a time: K <= kChunk reads the matrix once, a larger K ceil(K / kChunk) times.  The hot path.      n n reads
//   fold        after every pass, per row: the own cluster's sum if it is in the chunk, and the running minimum of
//               S[i][c] / sizes[c] over the other non-empty clusters of the chunk                                n kChunk reads
//   finish      s[i] from the two, and their mean: one workgroup, per-thread strided sums and a fixed tree
//
// The sums kernel keeps the summation order written at the top of po_rows.h, per cluster, and takes every step of it from there.
// An entry of another cluster is replaced by +0 with a select.  A cluster's chains see the same operands in the same order
// whatever else the thread accumulates, so S[i][labels[i]] has the bytes po_kmedoids_costs_dev gives, and the bytes of S[i][c]
// depend on the row, the labels and n alone: not on K, the chunk c falls in, the kernel variant, ld or the alignment.
//
// Registers.  A thread holds C x V accumulators per row (V = 4 float32 / 2 float64 positions).  The kernel is compiled for
// C = 4, 8 and kChunk = 16 clusters and a pass takes the smallest that holds its clusters (each element costs C compares shared
// by the workgroup's rows, and per row C selects and C float64 adds: a run with K <= 8 should not pay for 16).  The rows per
// workgroup R are chosen so that C x V x R <= 64 doubles = 128 VGPRs: float32 R = 4 / 2 / 1, float64 R = 4 / 4 / 2.  With the
// group in flight (loaded while the current one is added) the compiler reports 108 - 192 VGPRs and no scratch (DESIGN.md has the
// table): two or three waves per SIMD, each with its next 16-byte loads outstanding while it works through C x V x R selects and adds.
#include "po_rows.h"

#include <algorithm>

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kChunk = PO_SILHOUETTE_CHUNK;

// out[i * out_ld + c] = S[i][c0 + c] for c < nc <= C and every row i < n.  labels starts on a 16-byte boundary.
template <typename T, int C, int R, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void sil_sums_kernel(const T* __restrict__ D, uint64_t ld, uint32_t n, const int32_t* __restrict__ labels,
                                                            int32_t c0, uint32_t nc, double* __restrict__ out, uint64_t out_ld) {
    constexpr uint32_t V = 16 / sizeof(T);
    __shared__ double wsum[R][C][kThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint32_t i0 = blockIdx.x * R;
    const T* s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = D + static_cast<uint64_t>(i0 + r < n ? i0 + r : n - 1) * ld;   // a short last workgroup repeats the last row
    double acc[R][C][V];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (uint32_t u = 0; u < V; ++u) acc[r][c][u] = 0.0;

    const uint32_t full = n / V;                                            // whole groups
    uint32_t g = tid;
    if (g < full) {
        struct group {
            int32_t lab[V];                                                 // labels of the group's columns, relative to c0
            T v[R][V];
        } cur, next;
        auto load = [&](uint32_t grp, group& dst) {
            const uint32_t j0 = grp * V;
            int32_t l[V];
            po_load_labels<V>(labels, j0, l);
#pragma unroll
            for (uint32_t u = 0; u < V; ++u) dst.lab[u] = l[u] - c0;
#pragma unroll
            for (int r = 0; r < R; ++r) po_load_group<T, ALIGNED>(s[r], j0, dst.v[r]);
        };
        load(g, cur);
        for (;;) {                                                          // the next group is on its way while this one is added
            const uint32_t gn = g + kThreads;
            const bool more = gn < full;
            if (more) load(gn, next);
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (uint32_t u = 0; u < V; ++u) {
                    const bool in = cur.lab[u] == c;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const T x = in ? cur.v[r][u] : T(0);
                        acc[r][c][u] += static_cast<double>(x);
                    }
                }
            if (!more) break;
            g = gn;
            cur = next;
        }
    }
    if (tid == (full & (kThreads - 1))) {                                   // the short group, after the thread's whole ones
#pragma unroll
        for (uint32_t u = 0; u + 1 < V; ++u) {
            const uint32_t j = full * V + u;
            if (j < n) {
                const int32_t lab = labels[j] - c0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const T e = s[r][j];
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const T x = lab == c ? e : T(0);
                        acc[r][c][u] += static_cast<double>(x);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double t = po_wave_sum_fixed(po_thread_tree(acc[r][c]));
            if ((tid & 63u) == 0) wsum[r][c][tid >> 6] = t;
        }
    __syncthreads();
    if (tid < R * C) {
        const uint32_t r = tid / C, c = tid % C;
        if (i0 + r < n && c < nc) out[static_cast<uint64_t>(i0 + r) * out_ld + c] = po_block_tree(wsum[r][c]);
    }
}

// sizes[c] += 1 per column of cluster c; err = the first position whose label is outside [0, K).  sizes is zero, err all ones on entry.
__global__ __launch_bounds__(kThreads) void sil_hist_kernel(const int32_t* __restrict__ labels, uint32_t n, uint32_t K, uint32_t* __restrict__ sizes,
                                                            uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t l = labels[i];
    if (l < 0 || static_cast<uint32_t>(l) >= K) atomicMin(err, i);
    else atomicAdd(&sizes[l], 1u);
}

__global__ __launch_bounds__(kThreads) void sil_nonempty_kernel(const uint32_t* __restrict__ sizes, uint32_t K, uint32_t* __restrict__ count) {
    const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
    if (c < K && sizes[c] != 0) atomicAdd(count, 1u);
}

__global__ __launch_bounds__(kThreads) void sil_init_kernel(double* __restrict__ own, double* __restrict__ other, uint32_t n) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    own[i] = 0.0;
    other[i] = __longlong_as_double(0x7FF0000000000000ll);                  // +inf: no other cluster seen yet
}

// one pass's sums chunk[i][c] = S[i][c0 + c], c < nc: own[i] = the sum over the row's own cluster, other[i] = the smallest mean
// over the other non-empty clusters so far - a NaN mean stays (the row's value is NaN then)
__global__ __launch_bounds__(kThreads) void sil_fold_kernel(const double* __restrict__ chunk, const int32_t* __restrict__ labels,
                                                            const uint32_t* __restrict__ sizes, uint32_t n, uint32_t c0, uint32_t nc,
                                                            double* __restrict__ own, double* __restrict__ other) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t mine = static_cast<uint32_t>(labels[i]);
    double b = other[i];
    for (uint32_t c = 0; c < nc; ++c) {
        const uint32_t sz = sizes[c0 + c];
        if (sz == 0) continue;                                              // an empty cluster is no neighbour
        const double sum = chunk[static_cast<uint64_t>(i) * kChunk + c];
        if (c0 + c == mine) {
            own[i] = sum;
        } else {
            const double m = sum / static_cast<double>(sz);
            if (b == b && (m != m || m < b)) b = m;
        }
    }
    other[i] = b;
}

// One workgroup: s[i] of every row and mean = (sum of s) / n (per-thread strided partial sums, po_block1024_sum).
__global__ __launch_bounds__(1024) void sil_finish_kernel(const double* __restrict__ own, const double* __restrict__ other,
                                                          const int32_t* __restrict__ labels, const uint32_t* __restrict__ sizes, uint32_t n,
                                                          double* __restrict__ values, double* __restrict__ mean) {
    const uint32_t tid = threadIdx.x;
    double acc = 0.0;
    for (uint32_t i = tid; i < n; i += 1024) {
        const uint32_t sz = sizes[labels[i]];
        const double sum = own[i], b = other[i];
        double v;
        if (sum != sum || b != b) {
            v = __longlong_as_double(0x7FF8000000000000ll);                // an undefined distance: NaN, not scikit-learn's 0
        } else if (sz <= 1) {
            v = 0.0;                                                        // a cluster of one
        } else {
            const double a = sum / static_cast<double>(sz - 1);
            const double m = a > b ? a : b;
            v = m == 0.0 ? 0.0 : (b - a) / m;                               // duplicates: 0 / 0 is 0 (scikit-learn's nan_to_num)
        }
        values[i] = v;
        acc += v;
    }
    const double total = po_block1024_sum(acc);
    if (tid == 0) *mean = total / static_cast<double>(n);
}

// ---- workspace of one problem (ctx->ws_sil) -----------------------------------------------------------------------------------
struct sil_ws {
    int32_t* labels;                // [n]: the caller's labels on a 16-byte boundary
    uint32_t* sizes;                // [K]
    double* chunk;                  // [n][kChunk]: the sums of one pass (po_silhouette* only)
    double* own;                    // [n]
    double* other;                  // [n]
    uint32_t* flag;                 // [4]: first bad label, non-empty clusters
    double* scal;                   // [2]: mean
};

size_t sil_ws_layout(uint64_t n, uint32_t K, bool values, uint8_t* base, sil_ws* w) {
    po_carver ws{base};
    uint8_t* a = ws.take(n * 4);
    uint8_t* b = ws.take((size_t)K * 4);
    uint8_t* f = ws.take(16);
    uint8_t* g = ws.take(16);
    uint8_t* c = values ? ws.take(n * kChunk * 8) : nullptr;
    uint8_t* d = values ? ws.take(n * 8) : nullptr;
    uint8_t* e = values ? ws.take(n * 8) : nullptr;
    if (w) {
        w->labels = reinterpret_cast<int32_t*>(a);
        w->sizes = reinterpret_cast<uint32_t*>(b);
        w->flag = reinterpret_cast<uint32_t*>(f);
        w->scal = reinterpret_cast<double*>(g);
        w->chunk = reinterpret_cast<double*>(c);
        w->own = reinterpret_cast<double*>(d);
        w->other = reinterpret_cast<double*>(e);
    }
    return ws.off;
}

int sil_workspace(po_ctx* ctx, uint64_t n, uint32_t K, bool values, sil_ws* w) {
    if (!ctx->h_sil) PO_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_sil), 8 * sizeof(double), hipHostMallocDefault));
    int rc = po_buf_reserve(ctx, &ctx->ws_sil, sil_ws_layout(n, K, values, nullptr, nullptr));
    if (rc) return rc;
    sil_ws_layout(n, K, values, static_cast<uint8_t*>(ctx->ws_sil.p), w);
    return PO_OK;
}

template <typename T, int C, int R>
int launch_sums_t(po_ctx* ctx, const T* D, uint64_t ld, uint32_t n, const int32_t* labels, uint32_t c0, uint32_t nc, double* out, uint64_t out_ld) {
    const dim3 grid((n + R - 1) / R), block(kThreads);
    const bool al = po_rows_aligned(D, ld, sizeof(T));
    if (al) hipLaunchKernelGGL((sil_sums_kernel<T, C, R, true>), grid, block, 0, ctx->stream, D, ld, n, labels, (int32_t)c0, nc, out, out_ld);
    else hipLaunchKernelGGL((sil_sums_kernel<T, C, R, false>), grid, block, 0, ctx->stream, D, ld, n, labels, (int32_t)c0, nc, out, out_ld);
    PO_CHECK_LAUNCH("sil_sums_kernel");
    return PO_OK;
}

// one pass: clusters c0 .. c0 + nc - 1 (nc <= kChunk), by the smallest variant that holds them
int launch_sums(po_ctx* ctx, const void* D, int f32, uint64_t ld, uint32_t n, const int32_t* labels, uint32_t c0, uint32_t nc, double* out,
                uint64_t out_ld) {
    if (f32) {
        const float* d = static_cast<const float*>(D);
        if (nc <= 4) return launch_sums_t<float, 4, 4>(ctx, d, ld, n, labels, c0, nc, out, out_ld);
        if (nc <= 8) return launch_sums_t<float, 8, 2>(ctx, d, ld, n, labels, c0, nc, out, out_ld);
        return launch_sums_t<float, 16, 1>(ctx, d, ld, n, labels, c0, nc, out, out_ld);
    }
    const double* d = static_cast<const double*>(D);
    if (nc <= 4) return launch_sums_t<double, 4, 4>(ctx, d, ld, n, labels, c0, nc, out, out_ld);
    if (nc <= 8) return launch_sums_t<double, 8, 4>(ctx, d, ld, n, labels, c0, nc, out, out_ld);
    return launch_sums_t<double, 16, 2>(ctx, d, ld, n, labels, c0, nc, out, out_ld);
}

int check_args(const char* who, po_ctx* ctx, const void* m, int dtype, uint64_t n, uint64_t ld, uint32_t K) {
    const int rc = po_check_matrix_args(who, ctx, m, dtype, n, ld);
    if (rc) return rc;
    PO_REQUIRE(K >= 1 && K <= n, "%s: n_clusters = %u outside 1 .. n = %llu", who, K, (unsigned long long)n);
    return PO_OK;
}

// the labels into the workspace, their histogram, and the check of their range.  One synchronisation.
int take_labels(const char* who, po_ctx* ctx, const sil_ws& w, const int32_t* d_labels, uint32_t n, uint32_t K, uint32_t* nonempty) {
    uint32_t* h = reinterpret_cast<uint32_t*>(ctx->h_sil);
    PO_HIP(hipMemcpyAsync(w.labels, d_labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    PO_HIP(hipMemsetAsync(w.sizes, 0, (size_t)K * 4, ctx->stream));
    PO_HIP(hipMemsetAsync(w.flag, 0xFF, 4, ctx->stream));
    PO_HIP(hipMemsetAsync(w.flag + 1, 0, 4, ctx->stream));
    hipLaunchKernelGGL(sil_hist_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, w.labels, n, K, w.sizes, w.flag);
    PO_CHECK_LAUNCH("sil_hist_kernel");
    hipLaunchKernelGGL(sil_nonempty_kernel, dim3((K + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, w.sizes, K, w.flag + 1);
    PO_CHECK_LAUNCH("sil_nonempty_kernel");
    PO_HIP(hipMemcpyAsync(h, w.flag, 8, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    PO_REQUIRE(h[0] == 0xFFFFFFFFu, "%s: labels[%u] is outside 0 .. n_clusters-1 = %u", who, h[0], K - 1);
    *nonempty = h[1];
    return PO_OK;
}

}  // namespace

extern "C" int po_cluster_sums_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, const int32_t* d_labels,
                                   uint32_t n_clusters, double* d_sums) {
    const char* who = "po_cluster_sums_dev";
    int rc = check_args(who, ctx, d_matrix, dtype, n, ld, n_clusters);
    if (rc) return rc;
    PO_REQUIRE(d_labels != nullptr && d_sums != nullptr, "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    sil_ws w;
    rc = sil_workspace(ctx, n, n_clusters, false, &w);
    if (rc) return rc;
    uint32_t nonempty = 0;
    rc = take_labels(who, ctx, w, d_labels, (uint32_t)n, n_clusters, &nonempty);
    if (rc) return rc;
    for (uint32_t c0 = 0; c0 < n_clusters; c0 += kChunk) {
        rc = launch_sums(ctx, d_matrix, dtype == PO_F32, ld, (uint32_t)n, w.labels, c0, std::min(kChunk, n_clusters - c0), d_sums + c0, n_clusters);
        if (rc) return rc;
    }
    return PO_OK;
}

extern "C" int po_silhouette_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, const int32_t* d_labels,
                                 uint32_t n_clusters, double* d_values, po_silhouette_result* result) {
    const char* who = "po_silhouette_dev";
    if (result) memset(result, 0, sizeof(*result));
    int rc = check_args(who, ctx, d_matrix, dtype, n, ld, n_clusters);
    if (rc) return rc;
    PO_REQUIRE(d_labels != nullptr && d_values != nullptr, "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    const uint32_t N = (uint32_t)n, K = n_clusters;
    sil_ws w;
    rc = sil_workspace(ctx, n, K, true, &w);
    if (rc) return rc;
    const bool timed = result != nullptr;
    float ms = 0.0f;
    double t_sums = 0.0, t_finish = 0.0;
    if (timed) PO_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    uint32_t nonempty = 0;
    rc = take_labels(who, ctx, w, d_labels, N, K, &nonempty);
    if (rc) return rc;
    PO_REQUIRE(nonempty >= 2, "%s: the labels name %u non-empty cluster%s: a silhouette needs at least 2", who, nonempty, nonempty == 1 ? "" : "s");
    const dim3 ngrid((N + kThreads - 1) / kThreads), block(kThreads);
    hipLaunchKernelGGL(sil_init_kernel, ngrid, block, 0, ctx->stream, w.own, w.other, N);
    PO_CHECK_LAUNCH("sil_init_kernel");
    if (timed) {
        PO_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
        PO_HIP(hipEventSynchronize(ctx->ev[1]));
        PO_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        t_finish += ms;
    }
    uint32_t passes = 0;
    for (uint32_t c0 = 0; c0 < K; c0 += kChunk) {
        const uint32_t nc = std::min(kChunk, K - c0);
        if (timed) PO_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
        rc = launch_sums(ctx, d_matrix, dtype == PO_F32, ld, N, w.labels, c0, nc, w.chunk, kChunk);
        if (rc) return rc;
        if (timed) PO_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
        hipLaunchKernelGGL(sil_fold_kernel, ngrid, block, 0, ctx->stream, w.chunk, w.labels, w.sizes, N, c0, nc, w.own, w.other);
        PO_CHECK_LAUNCH("sil_fold_kernel");
        ++passes;
        if (timed) {
            PO_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
            PO_HIP(hipEventSynchronize(ctx->ev[2]));
            PO_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
            t_sums += ms;
            PO_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
            t_finish += ms;
        }
    }
    if (timed) PO_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    hipLaunchKernelGGL(sil_finish_kernel, dim3(1), dim3(1024), 0, ctx->stream, w.own, w.other, w.labels, w.sizes, N, d_values, w.scal);
    PO_CHECK_LAUNCH("sil_finish_kernel");
    if (result) {
        PO_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
        PO_HIP(hipMemcpyAsync(ctx->h_sil, w.scal, 8, hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipStreamSynchronize(ctx->stream));
        PO_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        t_finish += ms;
        result->mean = ctx->h_sil[0];
        result->nonempty_clusters = nonempty;
        result->passes = passes;
        result->sums_ms = t_sums;
        result->finish_ms = t_finish;
    }
    return PO_OK;
}

extern "C" int po_silhouette(po_ctx* ctx, const void* matrix, int dtype, uint64_t n, uint64_t ld, const int32_t* labels, uint32_t n_clusters,
                             double* values, po_silhouette_result* result) {
    const char* who = "po_silhouette";
    if (result) memset(result, 0, sizeof(*result));
    int rc = check_args(who, ctx, matrix, dtype, n, ld, n_clusters);
    if (rc) return rc;
    PO_REQUIRE(labels != nullptr && values != nullptr, "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    const size_t b_lab = po_round_up(n * 4, 256), b_val = po_round_up(n * 8, 256);
    void* base;
    uint64_t ld_dev;
    uint8_t* extra;
    rc = po_stage_host_matrix(who, ctx, matrix, dtype, n, ld, b_lab + b_val, &base, &ld_dev, &extra);
    if (rc) return rc;
    int32_t* d_labels = reinterpret_cast<int32_t*>(extra);
    double* d_values = reinterpret_cast<double*>(extra + b_lab);
    PO_HIP(hipMemcpyAsync(d_labels, labels, n * 4, hipMemcpyHostToDevice, ctx->stream));
    rc = po_silhouette_dev(ctx, base, dtype, n, ld_dev, d_labels, n_clusters, d_values, result);
    if (rc) return rc;
    PO_HIP(hipMemcpyAsync(values, d_values, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    return PO_OK;
}
