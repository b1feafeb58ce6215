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
