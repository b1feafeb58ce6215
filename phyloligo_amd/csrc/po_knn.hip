// K nearest neighbours of every record, selected on the device (po_knn*, include/phyloligo_amd.h).
//
// Every list row keeps its best K candidates in HBM, idx int32 [n][K] and val [n][K] (float32 / float64, the dtype of the matrix
// the values come from), sorted by the total order of the ABI: ascending value (descending for Kendall's tau, a similarity), NaN
// after every number, ties by the smaller column; an unused entry has idx -1 and sorts after everything.  One launch of
// knn_select_kernel merges one batch of candidate rows into those lists, one workgroup per list row:
//   1. the row's threshold is its entry K-1 (the K-th best so far, or "empty" while the list is short);
//   2. the candidates stream in with 16-byte loads (row starts on 16-byte boundaries; the merge of lists, whose rows are
//      not, takes scalar loads) and each is compared with the threshold as a (key, column) pair;
//   3. the survivors are compacted into an LDS buffer by wave ballots and mbcnt prefix sums plus one exclusive scan over the
//      four waves - no per-element LDS atomics, so the buffer's content does not depend on timing;
//   4. when the buffer would overflow, and at the end of the batch if anything survived, the list (read from HBM on first
//      use) and the buffer are sorted together in LDS by a bitonic network over (key, column) pairs, the first K are kept
//      and the threshold tightens.  A batch in which nothing beats the threshold reads one entry of the list and writes none.
// The keys map values to an order-preserving unsigned integer: float32 / float64 bits with the sign folded in (negative:
// all bits flipped; positive: sign bit set), -0 read as +0 so that the two zeros tie as numbers do, every NaN one key above
// +inf, the unused entry the largest key.  Kendall's tau is negated before the mapping.  Since (key, column) is a total
// order over distinct columns, the lists do not depend on how the candidates are cut into batches, panels or ranks.
//
// LDS per workgroup: cap entries of (key 8 B, column 4 B, value 4 / 8 B), cap = 2 max(Kp, chunk), Kp = K rounded up to a power
// of two, chunk = 256 threads x one 16-byte load (1 024 float32 / 512 float64 values).  At K = 1 024: 2 048 x 20 B = 40 KiB
// (float64), 32 KiB (float32) - four workgroups fit the 160 KiB of a CU.
#include "po_rows.h"

#include <vector>

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint64_t kEmptyKey = ~0ull;
constexpr uint32_t kEmptyCol = 0xFFFFFFFFu;

__device__ inline bool pair_less(uint64_t ka, uint32_t ca, uint64_t kb, uint32_t cb) {
    return ka < kb || (ka == kb && ca < cb);
}

// One batch: list rows row0 + blockIdx.x; candidate t of that row is src[blockIdx.x * ld + t], 0 <= t < len, at column
// col0 + t, or at column cidx[blockIdx.x * ldc + t] when cidx is given (the merge: -1 = no candidate).  diag: column == row
// is not a candidate.
template <typename T>
__global__ __launch_bounds__(kThreads) void knn_select_kernel(int32_t* __restrict__ lidx, T* __restrict__ lval, uint32_t K,
                                                             uint32_t Kp, uint32_t cap, const T* __restrict__ src, uint64_t ld,
                                                             const int32_t* __restrict__ cidx, uint64_t ldc, uint64_t row0,
                                                             uint32_t len, uint32_t col0, int diag, int desc) {
    extern __shared__ uint64_t smem[];
    uint64_t* sk = smem;                                                   // [cap] keys
    T* sv = reinterpret_cast<T*>(smem + cap);                              // [cap] values as they came
    uint32_t* sc = reinterpret_cast<uint32_t*>(sv + cap);                  // [cap] columns
    __shared__ uint32_t wave_cnt[kWaves];

    constexpr uint32_t V = 16 / sizeof(T);
    constexpr uint32_t CH = kThreads * V;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t r = row0 + blockIdx.x;
    int32_t* li = lidx + r * K;
    T* lv = lval + r * K;
    const T* s = src + blockIdx.x * ld;
    const int32_t* ci = cidx ? cidx + blockIdx.x * ldc : nullptr;
    const bool aligned = !ci && (reinterpret_cast<uintptr_t>(s) & 15u) == 0;

    const int32_t last = li[K - 1];
    uint64_t thr_k = last < 0 ? kEmptyKey : po_order_key(lv[K - 1], desc != 0);
    uint32_t thr_c = last < 0 ? kEmptyCol : static_cast<uint32_t>(last);
    bool loaded = false;
    uint32_t cnt = 0;                                                      // entries in the buffer [Kp, Kp + cnt)

    // sort list + buffer, keep K, new threshold; leaves [K, Kp) empty
    auto flush = [&]() {
        if (!loaded) {
            for (uint32_t j = tid; j < Kp; j += kThreads) {
                const int32_t x = j < K ? li[j] : -1;
                const T v = j < K ? lv[j] : T(0);
                sk[j] = x < 0 ? kEmptyKey : po_order_key(v, desc != 0);
                sc[j] = x < 0 ? kEmptyCol : static_cast<uint32_t>(x);
                sv[j] = v;
            }
            loaded = true;
        }
        uint32_t P = 1;
        while (P < Kp + cnt) P <<= 1;
        for (uint32_t j = Kp + cnt + tid; j < P; j += kThreads) {
            sk[j] = kEmptyKey;
            sc[j] = kEmptyCol;
        }
        __syncthreads();
        for (uint32_t k = 2; k <= P; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < P; i += kThreads) {
                    const uint32_t p = i ^ j;
                    if (p > i) {
                        const uint64_t ka = sk[i], kb = sk[p];
                        const uint32_t ca = sc[i], cb = sc[p];
                        const bool up = (i & k) == 0;
                        if (pair_less(kb, cb, ka, ca) == up) {
                            sk[i] = kb; sk[p] = ka;
                            sc[i] = cb; sc[p] = ca;
                            const T t = sv[i]; sv[i] = sv[p]; sv[p] = t;
                        }
                    }
                }
                __syncthreads();
            }
        }
        thr_k = sk[K - 1];
        thr_c = sc[K - 1];
        for (uint32_t j = K + tid; j < Kp; j += kThreads) {
            sk[j] = kEmptyKey;
            sc[j] = kEmptyCol;
        }
        cnt = 0;
        __syncthreads();
    };

    for (uint32_t c0 = 0; c0 < len; c0 += CH) {
        const uint32_t e0 = c0 + tid * V;
        T v[V];
        if (aligned && e0 + V <= len) {
            const typename po_vec16<T>::type q = *reinterpret_cast<const typename po_vec16<T>::type*>(s + e0);
            const T* qp = reinterpret_cast<const T*>(&q);
#pragma unroll
            for (uint32_t u = 0; u < V; ++u) v[u] = qp[u];
        } else {
#pragma unroll
            for (uint32_t u = 0; u < V; ++u) v[u] = e0 + u < len ? s[e0 + u] : T(0);
        }
        uint64_t key[V];
        uint32_t col[V], pos[V];
        bool ok[V];
        uint32_t wsum = 0;
#pragma unroll
        for (uint32_t u = 0; u < V; ++u) {
            const uint32_t e = e0 + u;
            const int32_t c = e < len ? (ci ? ci[e] : static_cast<int32_t>(col0 + e)) : -1;
            key[u] = po_order_key(v[u], desc != 0);
            col[u] = static_cast<uint32_t>(c);
            ok[u] = c >= 0 && !(diag && static_cast<uint64_t>(c) == r) && pair_less(key[u], col[u], thr_k, thr_c);
            const uint64_t m = __ballot(ok[u]);
            pos[u] = wsum + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
            wsum += static_cast<uint32_t>(__popcll(m));
        }
        if (lane == 0) wave_cnt[wave] = wsum;
        __syncthreads();
        uint32_t woff = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            const uint32_t x = wave_cnt[w];
            woff += w < wave ? x : 0u;
            total += x;
        }
        __syncthreads();                                                   // wave_cnt is written again by the next chunk
        if (total == 0) continue;                                          // (uniform)
        if (cnt + total > cap - Kp) flush();
#pragma unroll
        for (uint32_t u = 0; u < V; ++u) {
            if (ok[u]) {
                const uint32_t j = Kp + cnt + woff + pos[u];
                sk[j] = key[u];
                sc[j] = col[u];
                sv[j] = v[u];
            }
        }
        cnt += total;
        __syncthreads();
    }
    if (cnt == 0) return;                                                  // nothing beat the threshold: the list stands
    flush();
    for (uint32_t j = tid; j < K; j += kThreads) {
        const uint32_t c = sc[j];
        li[j] = c == kEmptyCol ? -1 : static_cast<int32_t>(c);
        lv[j] = c == kEmptyCol ? T(0) : sv[j];
    }
}

uint32_t pow2_at_least(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace

size_t po_knn_select_shmem(uint32_t k, int val_f32) {
    const uint32_t chunk = kThreads * (val_f32 ? 4u : 2u);
    const uint32_t kp = pow2_at_least(k);
    const size_t cap = 2 * (size_t)(kp > chunk ? kp : chunk);
    return cap * (8 + 4 + (val_f32 ? 4 : 8));
}

int po_launch_knn_select(po_ctx* ctx, int32_t* d_idx, void* d_val, uint32_t k, int val_f32, int desc, const po_knn_batch& b) {
    if (b.rows == 0 || b.len == 0) return PO_OK;
    PO_REQUIRE(k >= 1 && k <= PO_KNN_MAX_K, "knn selection: k = %u outside 1..%u", k, PO_KNN_MAX_K);
    const uint32_t chunk = kThreads * (val_f32 ? 4u : 2u);
    const uint32_t kp = pow2_at_least(k);
    const uint32_t cap = 2 * (kp > chunk ? kp : chunk);
    const size_t shmem = po_knn_select_shmem(k, val_f32);
    const dim3 grid(static_cast<uint32_t>(b.rows)), block(kThreads);
    if (val_f32) {
        PO_SHMEM(ctx, knn_select_kernel<float>, shmem);
        hipLaunchKernelGGL(knn_select_kernel<float>, grid, block, shmem, ctx->stream, d_idx, static_cast<float*>(d_val), k, kp, cap,
                           static_cast<const float*>(b.src), b.ld, b.cidx, b.ldc, b.row0, b.len, b.col0, b.diag, desc);
    } else {
        PO_SHMEM(ctx, knn_select_kernel<double>, shmem);
        hipLaunchKernelGGL(knn_select_kernel<double>, grid, block, shmem, ctx->stream, d_idx, static_cast<double*>(d_val), k, kp, cap,
                           static_cast<const double*>(b.src), b.ld, b.cidx, b.ldc, b.row0, b.len, b.col0, b.diag, desc);
    }
    PO_CHECK_LAUNCH("knn_select_kernel");
    return PO_OK;
}

// ---- the entry points ----------------------------------------------------------------------------------------------------
// The lists are selected from panels of the matrix that po_pairwise_run computes into the context's workspace (ws_knn): a
// triangular block [a,b) becomes row panels [lo,hi) = one triangular block plus the rectangle [lo,hi) x [hi,b) with its
// mirror, a rectangular block becomes row strips with their mirrors.  Behind the kernels of the last block of a panel, the
// panel's rows (slab) and the rows of its columns (mirror) are merged into the lists; the next panel reuses the
// workspace.  Every ordered pair is fed exactly once, with the value the dense matrix holds.
static const uint64_t kKnnPanelBytes = 256ull << 20;    // slab + mirror of one panel: about the Infinity Cache

struct knn_feed {
    po_knn_batch rows, cols;   // the panel's rows from the slab, the rows of its columns from the mirror (rows == 0: none)
};

struct knn_run {
    po_ctx* ctx;
    int32_t* idx;
    void* val;
    uint32_t k;
    int f32, desc;
    std::vector<po_block> panels;             // the blocks po_pairwise_run computes
    std::vector<knn_feed> feeds;              // one per panel
    std::vector<hipEvent_t> ev;               // selection start / end per panel when timed
    std::vector<uint8_t> fed;
    ~knn_run() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

static int knn_after_block(void* user, uint32_t b) {
    knn_run* r = static_cast<knn_run*>(user);
    const knn_feed& f = r->feeds[b];
    if (f.rows.rows == 0 && f.cols.rows == 0) return PO_OK;
    if (!r->ev.empty()) PO_HIP(hipEventRecord(r->ev[2 * b], r->ctx->stream));
    PO_TRY(po_launch_knn_select(r->ctx, r->idx, r->val, r->k, r->f32, r->desc, f.rows));
    PO_TRY(po_launch_knn_select(r->ctx, r->idx, r->val, r->k, r->f32, r->desc, f.cols));
    if (!r->ev.empty()) {
        PO_HIP(hipEventRecord(r->ev[2 * b + 1], r->ctx->stream));
        r->fed[b] = 1;
    }
    return PO_OK;
}

// the blocks of a work list: inside 0..n, beginning on tile edges, triangular or off the diagonal; the tallest and the widest
static int knn_check_blocks(const char* who, const po_block* blocks, uint32_t n_blocks, uint64_t n, uint64_t* max_rows, uint64_t* max_cols) {
    *max_rows = *max_cols = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const po_block& q = blocks[b];
        PO_REQUIRE(po_block_inside(q, n), "%s: block %u outside 0..%llu", who, b, (unsigned long long)n);
        PO_REQUIRE(q.row_begin % PO_PAD_ROWS == 0 && q.col_begin % PO_PAD_ROWS == 0,
                   "%s: block %u does not begin on a multiple of %llu", who, b, (unsigned long long)PO_PAD_ROWS);
        if (q.triangular)
            PO_TRY(po_check_triangular_block(who, b, q));
        else
            PO_REQUIRE(q.row_end <= q.col_begin || q.col_end <= q.row_begin,
                       "%s: rectangular block %u overlaps the diagonal (rows and columns must be disjoint)", who, b);
        if (q.row_end - q.row_begin > *max_rows) *max_rows = q.row_end - q.row_begin;
        if (q.col_end - q.col_begin > *max_cols) *max_cols = q.col_end - q.col_begin;
    }
    return PO_OK;
}

// cuts the work list into panels of h rows over the slab (row stride ld_s) and the mirror (ld_m), with what each feeds
static void knn_plan_panels(knn_run& run, const po_block* blocks, uint32_t n_blocks, uint64_t h, uint8_t* slab, uint64_t ld_s,
                            uint8_t* mirror, uint64_t ld_m, size_t esz) {
    auto batch = [&](const uint8_t* src, uint64_t ld, uint64_t row0, uint64_t rows, uint64_t col0, uint64_t len, int diag) {
        po_knn_batch q;
        memset(&q, 0, sizeof(q));
        q.src = src; q.ld = ld; q.row0 = row0; q.rows = rows;
        q.col0 = (uint32_t)col0; q.len = (uint32_t)len; q.diag = diag;
        return q;
    };
    auto add = [&](uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint64_t out_col, bool tri, bool with_mirror, const knn_feed& f) {
        po_block q;
        memset(&q, 0, sizeof(q));
        q.row_begin = r0; q.row_end = r1; q.col_begin = c0; q.col_end = c1;
        q.out = slab + out_col * esz;
        q.ld_out = ld_s;
        q.mirror = with_mirror ? mirror : nullptr;
        q.ld_mirror = ld_m;
        q.triangular = tri ? 1u : 0u;
        run.panels.push_back(q);
        run.feeds.push_back(f);
    };
    const knn_feed none = {};
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const po_block& q = blocks[b];
        if (po_block_empty(q)) continue;
        if (q.triangular) {
            const uint64_t a = q.row_begin, e = q.row_end;
            for (uint64_t lo = a; lo < e; lo += h) {
                const uint64_t hi = lo + h < e ? lo + h : e;
                knn_feed f;
                f.rows = batch(slab, ld_s, lo, hi - lo, lo, e - lo, 1);
                f.cols = batch(mirror, ld_m, hi, e - hi, lo, hi - lo, 0);
                if (hi == e) {
                    add(lo, hi, lo, hi, 0, true, false, f);
                } else {
                    add(lo, hi, lo, hi, 0, true, false, none);
                    add(lo, hi, hi, e, hi - lo, false, true, f);
                }
            }
        } else {
            for (uint64_t s = q.row_begin; s < q.row_end; s += h) {
                const uint64_t t = s + h < q.row_end ? s + h : q.row_end;
                knn_feed f;
                f.rows = batch(slab, ld_s, s, t - s, q.col_begin, q.col_end - q.col_begin, 0);
                f.cols = batch(mirror, ld_m, q.col_begin, q.col_end - q.col_begin, s, t - s, 0);
                add(s, t, q.col_begin, q.col_end, 0, false, true, f);
            }
        }
    }
}

// k_eff of the ABI: min(k, n - 1), 0 for n <= 1 (an empty result)
static uint32_t knn_k_eff(uint64_t n, uint32_t k) { return n > 1 ? (uint32_t)(k < n - 1 ? k : n - 1) : 0; }

// knn over a list of blocks (pair ranges, out / mirror ignored); the lists [n][k_eff] are emptied first
static int knn_core(po_ctx* ctx, const char* who, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n, uint32_t dim,
                    int metric, uint32_t k, int val_dtype, uint64_t panel_rows, const po_block* blocks, uint32_t n_blocks,
                    int32_t* d_idx, void* d_val, uint32_t flags, po_stats* stats) {
    PO_TRY(po_check_ctx(who, ctx));
    if (stats) memset(stats, 0, sizeof(*stats));
    PO_TRY(po_check_metric(metric));
    PO_TRY(po_check_knn_k(who, k));
    PO_TRY(po_check_dtype(who, "val_dtype", val_dtype));
    PO_REQUIRE(panel_rows % PO_PAD_ROWS == 0, "%s: panel_rows (%llu) is not a multiple of %llu", who,
               (unsigned long long)panel_rows, (unsigned long long)PO_PAD_ROWS);
    PO_REQUIRE(blocks != nullptr || n_blocks == 0, "%s: NULL block list", who);
    PO_REQUIRE(n < (1ull << 31), "%s: n (%llu) does not fit the int32 neighbour indices", who, (unsigned long long)n);
    const uint32_t k_eff = knn_k_eff(n, k);
    if (k_eff == 0) return PO_OK;
    PO_REQUIRE(d_counts != nullptr && d_totals != nullptr && d_idx != nullptr && d_val != nullptr, "%s: NULL buffer", who);
    PO_TRY(po_check_dim(who, dim));
    uint64_t max_rows = 0, max_cols = 0;
    PO_TRY(knn_check_blocks(who, blocks, n_blocks, n, &max_rows, &max_cols));
    PO_HIP(hipSetDevice(ctx->device));
    const size_t esz = val_dtype == PO_F32 ? 4 : 8;
    PO_HIP(hipMemsetAsync(d_idx, 0xFF, n * (uint64_t)k_eff * sizeof(int32_t), ctx->stream));      // every entry unused
    PO_HIP(hipMemsetAsync(d_val, 0, n * (uint64_t)k_eff * esz, ctx->stream));
    if (max_rows == 0 || max_cols == 0) return PO_OK;

    // panel height: given, or the slab + mirror near kKnnPanelBytes (a multiple of the tile edge, so that the tiles are those of
    // the dense matrix), never more than the tallest block
    const uint64_t ld_s = po_round_up(max_cols, 32);
    uint64_t h = panel_rows;
    if (h == 0) {
        h = kKnnPanelBytes / (esz * (ld_s + max_cols)) / PO_PAD_ROWS * PO_PAD_ROWS;
        if (h < PO_PAD_ROWS) h = PO_PAD_ROWS;
    }
    if (h > po_round_up(max_rows, PO_PAD_ROWS)) h = po_round_up(max_rows, PO_PAD_ROWS);
    const uint64_t ld_m = po_round_up(h, 32);
    const size_t slab_bytes = po_round_up(h * ld_s * esz, 256);
    PO_TRY(po_buf_reserve(ctx, &ctx->ws_knn, slab_bytes + max_cols * ld_m * esz));
    uint8_t* slab = static_cast<uint8_t*>(ctx->ws_knn.p);

    knn_run run;
    run.ctx = ctx; run.idx = d_idx; run.val = d_val; run.k = k_eff;
    run.f32 = val_dtype == PO_F32; run.desc = metric == PO_KT;
    knn_plan_panels(run, blocks, n_blocks, h, slab, ld_s, slab + slab_bytes, ld_m, esz);
    if (stats) {
        run.ev.resize(2 * run.panels.size(), nullptr);
        run.fed.assign(run.panels.size(), 0);
        for (hipEvent_t& e : run.ev)
            if (hipEventCreate(&e) != hipSuccess) {
                po_set_error("%s: hipEventCreate failed", who);
                return PO_EHIP;
            }
    }
    // the dense symmetric path's convention: pairs are evaluated once; PO_FLAG_NO_SYMMETRY does not apply to a list
    const int rc = po_pairwise_run(ctx, who, d_counts, d_totals, nullptr, n, dim, metric, val_dtype, run.panels.data(),
                                   (uint32_t)run.panels.size(), flags & ~PO_FLAG_NO_SYMMETRY, stats, knn_after_block, &run);
    if (stats && rc == PO_OK) {       // kernel_ms is the tile kernels alone: take the selections out
        double sel = 0.0;
        for (size_t b = 0; b < run.fed.size(); ++b) {
            if (!run.fed[b]) continue;
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, run.ev[2 * b], run.ev[2 * b + 1]) == hipSuccess) sel += ms;
        }
        stats->kernel_ms = stats->kernel_ms > sel ? stats->kernel_ms - sel : 0.0;
    }
    return rc;
}

extern "C" int po_knn_dev(po_ctx* ctx, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n, uint32_t dim, int metric,
                          uint32_t k, int val_dtype, uint64_t panel_rows, int32_t* d_idx, void* d_val, uint32_t flags,
                          po_stats* stats) {
    po_block whole;
    memset(&whole, 0, sizeof(whole));
    whole.row_end = whole.col_end = n;
    whole.triangular = 1;
    return knn_core(ctx, "po_knn_dev", d_counts, d_totals, n, dim, metric, k, val_dtype, panel_rows, &whole, 1, d_idx, d_val,
                    flags, stats);
}

extern "C" int po_knn_blocks_dev(po_ctx* ctx, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n, uint32_t dim,
                                 int metric, uint32_t k, int val_dtype, uint64_t panel_rows, const po_block* blocks,
                                 uint32_t n_blocks, int32_t* d_idx, void* d_val, uint32_t flags, po_stats* stats) {
    return knn_core(ctx, "po_knn_blocks_dev", d_counts, d_totals, n, dim, metric, k, val_dtype, panel_rows, blocks, n_blocks,
                    d_idx, d_val, flags, stats);
}

extern "C" int po_knn_merge_dev(po_ctx* ctx, uint64_t n, uint32_t k, int metric, int val_dtype, const int32_t* d_idx_in,
                                const void* d_val_in, uint32_t m, int32_t* d_idx, void* d_val) {
    PO_TRY(po_check_ctx("po_knn_merge_dev", ctx));
    PO_TRY(po_check_metric(metric));
    PO_TRY(po_check_knn_k("po_knn_merge_dev", k));
    PO_TRY(po_check_dtype("po_knn_merge_dev", "val_dtype", val_dtype));
    if (n == 0) return PO_OK;
    PO_REQUIRE(d_idx != nullptr && d_val != nullptr && (m == 0 || (d_idx_in != nullptr && d_val_in != nullptr)),
               "po_knn_merge_dev: NULL buffer");
    PO_HIP(hipSetDevice(ctx->device));
    const size_t esz = val_dtype == PO_F32 ? 4 : 8;
    PO_HIP(hipMemsetAsync(d_idx, 0xFF, n * (uint64_t)k * sizeof(int32_t), ctx->stream));
    PO_HIP(hipMemsetAsync(d_val, 0, n * (uint64_t)k * esz, ctx->stream));
    for (uint32_t i = 0; i < m; ++i) {
        po_knn_batch q;
        memset(&q, 0, sizeof(q));
        q.src = static_cast<const uint8_t*>(d_val_in) + (uint64_t)i * n * k * esz;
        q.ld = k;
        q.cidx = d_idx_in + (uint64_t)i * n * k;
        q.ldc = k;
        q.row0 = 0;
        q.rows = n;
        q.len = k;
        PO_TRY(po_launch_knn_select(ctx, d_idx, d_val, k, val_dtype == PO_F32, metric == PO_KT, q));
    }
    return PO_OK;
}

// The host-pointer form stages and calls po_knn_dev.  The checks that come before the staging (it needs k_eff and the buffers)
// name this entry point; everything after them is po_knn_dev's to refuse.
extern "C" int po_knn(po_ctx* ctx, const uint32_t* counts, const uint64_t* totals, uint64_t n, uint32_t dim, int metric, uint32_t k,
                      int val_dtype, uint64_t panel_rows, int32_t* idx, void* val, uint32_t flags, po_stats* stats) {
    PO_TRY(po_check_ctx("po_knn", ctx));
    if (stats) memset(stats, 0, sizeof(*stats));
    PO_TRY(po_check_metric(metric));
    PO_TRY(po_check_knn_k("po_knn", k));
    PO_TRY(po_check_dtype("po_knn", "val_dtype", val_dtype));
    const uint32_t k_eff = knn_k_eff(n, k);
    if (k_eff == 0) return PO_OK;
    PO_REQUIRE(counts != nullptr && totals != nullptr && idx != nullptr && val != nullptr, "po_knn: NULL buffer");
    PO_TRY(po_check_dim("po_knn", dim));
    PO_HIP(hipSetDevice(ctx->device));
    const size_t esz = val_dtype == PO_F32 ? 4 : 8;
    const uint64_t entries = n * (uint64_t)k_eff;
    uint32_t* d_in = nullptr;
    uint64_t* d_tot = nullptr;
    int32_t* d_idx = nullptr;
    uint8_t* d_val = nullptr;
    PO_TRY(po_stage(ctx, &ctx->ws_io, [&](po_carver& ws) {
        d_in = ws.array<uint32_t>(n * (uint64_t)dim);
        d_tot = ws.array<uint64_t>(n);
        d_idx = ws.array<int32_t>(entries);
        d_val = ws.take(entries * esz);
    }));
    PO_TRY(po_upload_profiles(ctx, n, dim, counts, totals, d_in, d_tot));
    PO_TRY(po_knn_dev(ctx, d_in, d_tot, n, dim, metric, k, val_dtype, panel_rows, d_idx, d_val, flags, stats));
    PO_HIP(hipMemcpyAsync(idx, d_idx, entries * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipMemcpyAsync(val, d_val, entries * esz, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    return PO_OK;
}
