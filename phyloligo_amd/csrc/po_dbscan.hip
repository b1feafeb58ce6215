// DBSCAN on a distance matrix in HBM (po_eps_degrees_dev, po_dbscan*, include/phyloligo_amd.h): the labels and core records of
// sklearn.cluster.DBSCAN(eps, min_samples, metric="precomputed"), stated without a visiting order (the header has the six rules).
//
//   degree     degree[i] = #{j : D[i][j] <= eps}, every row read once                                              n n reads
//   partition  core = degree >= min_samples; the core rows and the other rows as two ascending lists; lab[i] = i for a core
//              record, the sentinel for any other                                                                   one workgroup
//   round      m[i] = min of lab[j] over the columns within eps, for the core rows (the same kernel as `border`)   n_core n reads
//              new[i] = min(lab[i], m[i]);  hook: atomicMin(&new[lab[i]], new[i]), so a root hears of a smaller label;
//              jump: new[i] = the end of the chain new[new[..]], and a changed-flag; the host reads that one word
//   border     m[i] for the rows that are not core, once, after the loop                                   (n - n_core) n reads
//   finish     roots ranked into ids by a scan over n flags, the labels, the four counts                            one workgroup
//
// Everything is integer counting and integer minima: no order of execution changes a result, and there are no floating-point
// atomics.  The comparison is made in the matrix's own type against the largest value of that type that is <= eps, which for a
// float32 entry x decides exactly what (double)x <= eps decides.
//
// Why the loop ends where it should.  lab[i] <= i always, lab[i] is a core record of i's component, and after a jump every label
// is a root (lab[lab[i]] == lab[i]).  A round never raises a label.  If a link i - j had lab[j] < lab[i], new[i] would fall below
// lab[i] and the flag would be set; so a round that changes nothing leaves one label per component, and as that label r has
// lab[r] == r <= every member, it is the component's smallest core index.  Hooking lets a whole tree follow its root in the next
// jump, which is what takes a chain of n records from n / 2 rounds to about log n.
#include "po_rows.h"

#include <cmath>
#include <utility>

namespace {

constexpr uint32_t kThreads = 256;
constexpr int32_t kNone = 0x7FFFFFFF;                                      // the label of a column that is not core

__device__ __forceinline__ int32_t wave_min(int32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_down(v, off, 64));
    return v;                                                              // lane 0 holds the minimum
}

__device__ __forceinline__ int32_t wave_add(int32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// COUNT: out[row] = the number of columns j with D[row][j] <= thr.   !COUNT: out[row] = the minimum of lab[j] over those columns
// (kNone if there is none).  Row p of the launch is rows[p] (NULL: p).  A NaN is never <= thr.
template <typename T, int R, bool ALIGNED, bool COUNT>
__global__ __launch_bounds__(kThreads) void dbscan_rows_kernel(const T* __restrict__ D, uint64_t ld, uint32_t n, T thr,
                                                               const int32_t* __restrict__ rows, uint32_t nrows,
                                                               const int32_t* __restrict__ lab, int32_t* __restrict__ out) {
    constexpr uint32_t V = 16 / sizeof(T);
    __shared__ int32_t wpart[R][kThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint32_t p0 = blockIdx.x * R;
    const T* s[R];
    uint32_t row[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t p = p0 + r < nrows ? p0 + r : nrows - 1;             // a short last workgroup repeats its last row
        row[r] = rows ? static_cast<uint32_t>(rows[p]) : p;
        s[r] = D + static_cast<uint64_t>(row[r]) * ld;
    }
    int32_t acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = COUNT ? 0 : kNone;

    const uint32_t full = n / V;                                            // whole groups
    for (uint32_t g = tid; g < full; g += kThreads) {
        const uint32_t j0 = g * V;
        int32_t l[V];
        if (!COUNT) po_load_labels<V>(lab, j0, l);
        T v[R][V];
#pragma unroll
        for (int r = 0; r < R; ++r) po_load_group<T, ALIGNED>(s[r], j0, v[r]);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (uint32_t u = 0; u < V; ++u) {
                if (COUNT) acc[r] += v[r][u] <= thr ? 1 : 0;
                else acc[r] = min(acc[r], v[r][u] <= thr ? l[u] : kNone);
            }
    }
    if (tid == (full & (kThreads - 1))) {                                   // the short group
#pragma unroll
        for (uint32_t u = 0; u + 1 < V; ++u) {
            const uint32_t j = full * V + u;
            if (j < n) {
                const int32_t lj = COUNT ? 0 : lab[j];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (COUNT) acc[r] += s[r][j] <= thr ? 1 : 0;
                    else acc[r] = min(acc[r], s[r][j] <= thr ? lj : kNone);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int32_t t = COUNT ? wave_add(acc[r]) : wave_min(acc[r]);
        if ((tid & 63u) == 0) wpart[r][tid >> 6] = t;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r)                                             // (row[] stays in registers: no index that varies by thread)
        if (tid == r && p0 + r < nrows) {
            const int32_t* w = wpart[r];
            out[row[r]] = COUNT ? (w[0] + w[1]) + (w[2] + w[3]) : min(min(w[0], w[1]), min(w[2], w[3]));
        }
}

// One workgroup of 1024 threads, all of which call this: the number of set flags among the threads before this one, and the
// workgroup's total.  part: 16 words of LDS, free again after the call returns (it ends with a barrier).
__device__ __forceinline__ uint32_t block1024_rank(bool flag, uint32_t* part, uint32_t* total) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) part[wave] = static_cast<uint32_t>(__popcll(b));
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < 16; ++w) {
        const uint32_t c = part[w];
        before += w < wave ? c : 0;
        all += c;
    }
    __syncthreads();
    *total = all;
    return before + static_cast<uint32_t>(__popcll(b & ((1ull << lane) - 1ull)));
}

// One workgroup.  core[i] = degree[i] >= min_samples (min_samples > n: nobody); list[0, n_core) the core rows and list[n_core, n)
// the others, each ascending; lab[i] = i or kNone; counts[0] = n_core; mask (may be NULL) the core records as bytes.
__global__ __launch_bounds__(1024) void dbscan_partition_kernel(const int32_t* __restrict__ degree, uint32_t n, int64_t min_samples,
                                                                int32_t* __restrict__ list, int32_t* __restrict__ lab,
                                                                uint8_t* __restrict__ mask, uint32_t* __restrict__ counts) {
    __shared__ uint32_t part[16];
    const uint32_t tid = threadIdx.x;
    uint32_t n_core = 0;
    for (uint32_t base = 0; base < n; base += 1024) {                       // the count first: the second list starts behind it
        const uint32_t i = base + tid;
        uint32_t total;
        block1024_rank(i < n && degree[i] >= min_samples, part, &total);
        n_core += total;
    }
    uint32_t seen = 0;
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + tid;
        const bool core = i < n && degree[i] >= min_samples;
        uint32_t total;
        const uint32_t k = seen + block1024_rank(core, part, &total);
        if (i < n) {
            list[core ? k : n_core + (i - k)] = static_cast<int32_t>(i);
            lab[i] = core ? static_cast<int32_t>(i) : kNone;
            if (mask) mask[i] = core ? 1 : 0;
        }
        seen += total;
    }
    if (tid == 0) counts[0] = n_core;
}

// nw[i] = min(lab[i], m[i]) for a core record (lab[i] != kNone), kNone for any other
__global__ __launch_bounds__(kThreads) void dbscan_lower_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ m, uint32_t n,
                                                                int32_t* __restrict__ nw) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t l = lab[i];
    nw[i] = l == kNone ? kNone : min(l, m[i]);
}

// a root learns of the smallest label any record of its tree has seen
__global__ __launch_bounds__(kThreads) void dbscan_hook_kernel(const int32_t* __restrict__ lab, uint32_t n, int32_t* __restrict__ nw) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t l = lab[i];
    if (l == kNone) return;
    const int32_t v = __atomic_load_n(&nw[i], __ATOMIC_RELAXED);           // (nw[i] may itself be lowered by another record's hook:
    if (v < l) atomicMin(&nw[l], v);                                       //  any value it has held is a label of the component)
}

// nw[i] = the end of i's chain.  nw[x] <= x with equality only at a root, so a chain falls strictly until it ends; the writes of
// other threads only replace a link by the end of the same chain, and a root is never written: every thread finds the same end
// whatever the others have done.  changed: some label differs from the round's start.
__global__ __launch_bounds__(kThreads) void dbscan_jump_kernel(const int32_t* __restrict__ lab, uint32_t n, int32_t* __restrict__ nw,
                                                               uint32_t* __restrict__ changed) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t l = lab[i];
    if (l == kNone) return;
    int32_t r = __atomic_load_n(&nw[i], __ATOMIC_RELAXED);
    for (;;) {
        const int32_t up = __atomic_load_n(&nw[r], __ATOMIC_RELAXED);
        if (up == r) break;
        r = up;
    }
    __atomic_store_n(&nw[i], r, __ATOMIC_RELAXED);
    if (r != l) atomicOr(changed, 1u);
}

// One workgroup.  rank[r] = the number of roots (lab[r] == r) below r; labels[i] = rank[lab[i]] for a core record, rank[m[i]] for
// a record that is not core and has a core neighbour (m[i]: the smallest root among them - ids ascend with the roots), else -1.
// counts[1..4] = clusters, core, border, noise.
__global__ __launch_bounds__(1024) void dbscan_finish_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ m, uint32_t n,
                                                             int32_t* __restrict__ rank, int32_t* __restrict__ labels,
                                                             uint32_t* __restrict__ counts) {
    __shared__ uint32_t part[16];
    __shared__ uint32_t tally[3];
    const uint32_t tid = threadIdx.x;
    if (tid < 3) tally[tid] = 0;
    uint32_t seen = 0;
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + tid;
        uint32_t total;
        const uint32_t k = seen + block1024_rank(i < n && lab[i] == static_cast<int32_t>(i), part, &total);
        if (i < n) rank[i] = static_cast<int32_t>(k);
        seen += total;
    }
    __threadfence_block();
    __syncthreads();                                                        // rank is written, tally is zero
    uint32_t core = 0, border = 0, noise = 0;
    for (uint32_t i = tid; i < n; i += 1024) {
        const int32_t l = lab[i];
        const int32_t root = l != kNone ? l : m[i];
        labels[i] = root != kNone ? rank[root] : -1;
        core += l != kNone ? 1u : 0u;
        border += l == kNone && root != kNone ? 1u : 0u;
        noise += root == kNone ? 1u : 0u;
    }
    atomicAdd(&tally[0], core);
    atomicAdd(&tally[1], border);
    atomicAdd(&tally[2], noise);
    __syncthreads();
    if (tid == 0) {
        counts[1] = seen;
        counts[2] = tally[0];
        counts[3] = tally[1];
        counts[4] = tally[2];
    }
}

// ---- workspace of one problem (ctx->ws_dbscan): O(n) integers ---------------------------------------------------------------------
struct dbscan_ws {
    int32_t* degree;                // [n]
    int32_t* list;                  // [n]: the core rows, then the others
    int32_t* lab;                   // [n] and
    int32_t* nw;                    // [n]: the labels of a round and the next ones, swapped after every round; then the ranks
    int32_t* m;                     // [n]: the minimum a row has seen
    uint32_t* counts;               // [8]: n_core, clusters, core, border, noise
    uint32_t* flag;                 // [4]: changed
};

size_t dbscan_ws_layout(uint64_t n, uint8_t* base, dbscan_ws* w) {
    po_carver ws{base};
    int32_t* a = ws.array<int32_t>(n);
    int32_t* b = ws.array<int32_t>(n);
    int32_t* c = ws.array<int32_t>(n);
    int32_t* d = ws.array<int32_t>(n);
    int32_t* e = ws.array<int32_t>(n);
    uint32_t* f = ws.array<uint32_t>(8);
    uint32_t* g = ws.array<uint32_t>(4);
    if (w) *w = dbscan_ws{a, b, c, d, e, f, g};
    return ws.off;
}

int dbscan_workspace(po_ctx* ctx, uint64_t n, dbscan_ws* w) {
    if (!ctx->h_dbscan) PO_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_dbscan), 8 * sizeof(uint32_t), hipHostMallocDefault));
    PO_TRY(po_buf_reserve(ctx, &ctx->ws_dbscan, dbscan_ws_layout(n, nullptr, nullptr)));
    dbscan_ws_layout(n, static_cast<uint8_t*>(ctx->ws_dbscan.p), w);
    return PO_OK;
}

// the largest value of T that is <= eps (eps >= 0, +inf included): for a T x,  x <= that value  iff  (double)x <= eps
template <typename T> T threshold(double eps);
template <> double threshold<double>(double eps) { return eps; }
template <> float threshold<float>(double eps) {
    float f = static_cast<float>(eps);
    if (static_cast<double>(f) > eps) f = nextafterf(f, -INFINITY);
    return f;
}

template <typename T, int R, bool COUNT>
int launch_rows_t(po_ctx* ctx, const T* D, uint64_t ld, uint32_t n, double eps, const int32_t* rows, uint32_t nrows, const int32_t* lab,
                  int32_t* out) {
    const dim3 grid((nrows + R - 1) / R), block(kThreads);
    const T thr = threshold<T>(eps);
    if (po_rows_aligned(D, ld, sizeof(T)))
        hipLaunchKernelGGL((dbscan_rows_kernel<T, R, true, COUNT>), grid, block, 0, ctx->stream, D, ld, n, thr, rows, nrows, lab, out);
    else
        hipLaunchKernelGGL((dbscan_rows_kernel<T, R, false, COUNT>), grid, block, 0, ctx->stream, D, ld, n, thr, rows, nrows, lab, out);
    PO_CHECK_LAUNCH("dbscan_rows_kernel");
    return PO_OK;
}

// lab NULL: the degrees of all n rows.  Else the minimum label within eps of the rows rows[0, nrows); lab starts on a 16-byte
// boundary (the workspace's does).
int launch_rows(po_ctx* ctx, const void* D, int f32, uint64_t ld, uint32_t n, double eps, const int32_t* rows, uint32_t nrows,
                const int32_t* lab, int32_t* out) {
    if (nrows == 0) return PO_OK;
    if (f32) {
        const float* d = static_cast<const float*>(D);
        return lab ? launch_rows_t<float, 4, false>(ctx, d, ld, n, eps, rows, nrows, lab, out)
                   : launch_rows_t<float, 4, true>(ctx, d, ld, n, eps, rows, nrows, lab, out);
    }
    const double* d = static_cast<const double*>(D);
    return lab ? launch_rows_t<double, 2, false>(ctx, d, ld, n, eps, rows, nrows, lab, out)
               : launch_rows_t<double, 2, true>(ctx, d, ld, n, eps, rows, nrows, lab, out);
}

// the checks of every entry point of this file; n == 0 passes them without a matrix
int dbscan_check(const char* who, po_ctx* ctx, const void* m, int dtype, uint64_t n, uint64_t ld, double eps, int64_t min_samples) {
    PO_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    PO_REQUIRE(dtype == PO_F64 || dtype == PO_F32, "%s: dtype must be PO_F64 or PO_F32 (got %d)", who, dtype);
    PO_REQUIRE(n < (1ull << 31), "%s: n = %llu outside 0 .. 2^31 - 1", who, (unsigned long long)n);
    PO_REQUIRE(ld >= n, "%s: ld = %llu is smaller than n = %llu", who, (unsigned long long)ld, (unsigned long long)n);
    PO_REQUIRE(eps >= 0.0, "%s: eps = %g is not a distance: it must be 0 or more (+inf is allowed)", who, eps);
    PO_REQUIRE(min_samples >= 1, "%s: min_samples = %lld must be at least 1", who, (long long)min_samples);
    if (n == 0) return PO_OK;
    PO_REQUIRE(m != nullptr, "%s: the matrix pointer is NULL", who);
    const size_t esz = dtype == PO_F32 ? 4 : 8;
    PO_REQUIRE((reinterpret_cast<uintptr_t>(m) % esz) == 0, "%s: the matrix pointer is not aligned to its element size", who);
    return PO_OK;
}

}  // namespace

extern "C" int po_eps_degrees_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, double eps, int32_t* d_degree) {
    const char* who = "po_eps_degrees_dev";
    PO_TRY(dbscan_check(who, ctx, d_matrix, dtype, n, ld, eps, 1));
    if (n == 0) return PO_OK;
    PO_REQUIRE(d_degree != nullptr, "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    return launch_rows(ctx, d_matrix, dtype == PO_F32, ld, (uint32_t)n, eps, nullptr, (uint32_t)n, nullptr, d_degree);
}

extern "C" int po_dbscan_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, double eps, int64_t min_samples,
                             int32_t* d_labels, uint8_t* d_core, po_dbscan_result* result) {
    const char* who = "po_dbscan_dev";
    if (result) memset(result, 0, sizeof(*result));
    PO_TRY(dbscan_check(who, ctx, d_matrix, dtype, n, ld, eps, min_samples));
    if (n == 0) return PO_OK;
    PO_REQUIRE(d_labels != nullptr, "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    dbscan_ws w;
    PO_TRY(dbscan_workspace(ctx, n, &w));
    const int f32 = dtype == PO_F32;
    const uint32_t N = (uint32_t)n;
    const bool timed = result != nullptr;
    const dim3 ngrid((N + kThreads - 1) / kThreads), block(kThreads);
    uint32_t* h = ctx->h_dbscan;
    float ms = 0.0f;

    // ---- degrees, core records, the two row lists ----
    if (timed) PO_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    PO_TRY(launch_rows(ctx, d_matrix, f32, ld, N, eps, nullptr, N, nullptr, w.degree));
    hipLaunchKernelGGL(dbscan_partition_kernel, dim3(1), dim3(1024), 0, ctx->stream, w.degree, N, min_samples, w.list, w.lab, d_core, w.counts);
    PO_CHECK_LAUNCH("dbscan_partition_kernel");
    if (timed) PO_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
    PO_HIP(hipMemcpyAsync(h, w.counts, 4, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    const uint32_t n_core = h[0];
    if (timed) {
        PO_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        result->degree_ms = ms;
    }

    // ---- components of the core records ----
    int32_t *lab = w.lab, *nw = w.nw;
    uint32_t passes = 0;
    double t_label = 0.0;
    while (n_core) {
        ++passes;
        if (timed) PO_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
        PO_HIP(hipMemsetAsync(w.flag, 0, 4, ctx->stream));
        PO_TRY(launch_rows(ctx, d_matrix, f32, ld, N, eps, w.list, n_core, lab, w.m));
        hipLaunchKernelGGL(dbscan_lower_kernel, ngrid, block, 0, ctx->stream, lab, w.m, N, nw);
        PO_CHECK_LAUNCH("dbscan_lower_kernel");
        hipLaunchKernelGGL(dbscan_hook_kernel, ngrid, block, 0, ctx->stream, lab, N, nw);
        PO_CHECK_LAUNCH("dbscan_hook_kernel");
        hipLaunchKernelGGL(dbscan_jump_kernel, ngrid, block, 0, ctx->stream, lab, N, nw, w.flag);
        PO_CHECK_LAUNCH("dbscan_jump_kernel");
        if (timed) PO_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
        PO_HIP(hipMemcpyAsync(h, w.flag, 4, hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipStreamSynchronize(ctx->stream));
        if (timed) {
            PO_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
            t_label += ms;
        }
        std::swap(lab, nw);
        if (h[0] == 0) break;
    }

    // ---- border records, ids, labels ----
    if (timed) PO_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    PO_TRY(launch_rows(ctx, d_matrix, f32, ld, N, eps, w.list + n_core, N - n_core, lab, w.m));
    if (timed) PO_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
    hipLaunchKernelGGL(dbscan_finish_kernel, dim3(1), dim3(1024), 0, ctx->stream, lab, w.m, N, nw, d_labels, w.counts);
    PO_CHECK_LAUNCH("dbscan_finish_kernel");
    if (timed) {
        PO_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
        PO_HIP(hipMemcpyAsync(h, w.counts, 5 * 4, hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipStreamSynchronize(ctx->stream));
        PO_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        result->label_ms = t_label + ms;
        PO_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
        result->finish_ms = ms;
        result->clusters = h[1];
        result->core = h[2];
        result->border = h[3];
        result->noise = h[4];
        result->passes = passes;
    }
    return PO_OK;
}

extern "C" int po_dbscan(po_ctx* ctx, const void* matrix, int dtype, uint64_t n, uint64_t ld, double eps, int64_t min_samples, int32_t* labels,
                         uint8_t* core, po_dbscan_result* result) {
    const char* who = "po_dbscan";
    if (result) memset(result, 0, sizeof(*result));
    PO_TRY(dbscan_check(who, ctx, matrix, dtype, n, ld, eps, min_samples));
    if (n == 0) return PO_OK;
    PO_REQUIRE(labels != nullptr, "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    const size_t b_lab = po_round_up(n * 4, 256), b_core = po_round_up(n, 256);
    void* base;
    uint64_t ld_dev;
    uint8_t* extra;
    PO_TRY(po_stage_host_matrix(who, ctx, matrix, dtype, n, ld, b_lab + b_core, &base, &ld_dev, &extra));
    int32_t* d_labels = reinterpret_cast<int32_t*>(extra);
    uint8_t* d_core = extra + b_lab;
    PO_TRY(po_dbscan_dev(ctx, base, dtype, n, ld_dev, eps, min_samples, d_labels, core ? d_core : nullptr, result));
    PO_HIP(hipMemcpyAsync(labels, d_labels, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (core) PO_HIP(hipMemcpyAsync(core, d_core, n, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    return PO_OK;
}
