// Exact median of every row of a matrix in HBM (po_row_medians_dev, include/phyloligo_amd.h): the first step of the reference's
// outlier clip, medians = apply(dist_matrix, 1, median) of bin/phyloselect.R:339-357.
//
// One workgroup of 256 threads per row, a most-significant-digit radix select over the order-preserving 64-bit keys of the k-NN
// selection (po_order_key: float64 bits with the sign folded in, -0 = +0, NaN above +inf; a float32 matrix is widened first, which
// is exact).  The wanted ranks are k1 = (n-1)/2 and k2 = n/2.  State of a row: the key bits fixed so far (prefix / mask), the
// number m of elements that carry them, and k1, k2 relative to those.  Then, until the key is known:
//   collect    once m <= 2 048 the candidates are copied into LDS (16 KiB) and every later pass reads LDS, not memory;
//   histogram  a 4 096-bin LDS histogram of the next 12 key bits over the candidates (12 + 12 + 12 + 12 + 12 + 4 bits), scanned by
//              the workgroup for the bins that hold k1 and k2;
//   same bin   the digit joins the prefix (all 64 bits fixed: lo = hi = the key);
//   two bins   (even n only) k1 is the last element of its bin and k2 the first of the next occupied one: one more pass takes the
//              largest key of the first and the smallest key of the second, and the row is done.
// The first digit is sign + exponent, the second the top 12 mantissa bits: a row of distances typically leaves a few dozen
// candidates after two histograms, so it is read three times (histogram, histogram, collect); a row of up to 2 048 columns once.
// The worst case (every element equal down to the last bits) is seven reads.  Everything is integer counting on keys: the result is
// exact and depends on the row alone, whatever order LDS atomics arrive in.
//
// Histogram traffic: an LDS atomic per element would serialise on the few exponent bins a distance row occupies, so a wave first
// peels its two most common digits (ballot of the lanes that share the first lane's digit, one add of the popcount) and only the
// lanes left over add one by one.  LDS: 16 KiB histogram + 16 KiB candidates per workgroup, 5 workgroups (20 waves) per CU.
#include "po_rows.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kDigitBits = 12;
constexpr uint32_t kBins = 1u << kDigitBits;
constexpr uint32_t kCap = 2048;                 // candidates held in LDS
constexpr uint32_t kUnroll = 4;                 // 16-byte loads in flight per thread

__device__ inline double key_value(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double(static_cast<long long>(b));
}

__device__ inline uint32_t lane_rank(uint64_t m) {          // set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
}

// f(key, valid) for every element of the row, called by all threads of the workgroup the same number of times (so f may use wave
// ballots): columns in groups of V = 16 bytes / element size, group g read by thread g mod 256 with one 16-byte load (ALIGNED) or V
// element loads; the last, partial group is a short group read element by element.
template <typename T, bool ALIGNED, typename F>
__device__ __forceinline__ void sweep_row(const T* __restrict__ s, uint32_t n, uint32_t tid, F&& f) {
    constexpr uint32_t V = 16 / sizeof(T);
    using vecT = typename po_vec16<T>::type;
    const uint32_t full = n / V, groups = (n + V - 1) / V;
    for (uint32_t g0 = 0; g0 < groups; g0 += kThreads * kUnroll) {
        T v[kUnroll][V];
        uint32_t cnt[kUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u) {
            const uint32_t g = g0 + u * kThreads + tid;
            cnt[u] = g < full ? V : (g == full ? n - full * V : 0u);
            const uint64_t j0 = static_cast<uint64_t>(g) * V;
            if (ALIGNED && g < full) {
                const vecT q = *reinterpret_cast<const vecT*>(s + j0);
                const T* qp = reinterpret_cast<const T*>(&q);
#pragma unroll
                for (uint32_t e = 0; e < V; ++e) v[u][e] = qp[e];
            } else {
#pragma unroll
                for (uint32_t e = 0; e < V; ++e) v[u][e] = e < cnt[u] ? s[j0 + e] : T(0);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u)
#pragma unroll
            for (uint32_t e = 0; e < V; ++e) f(po_order_key(static_cast<double>(v[u][e]), false), e < cnt[u]);
    }
}

// hist[digit] += 1 for the lanes with `take`; called by whole waves
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t digit, bool take, uint32_t lane) {
    uint64_t left = __ballot(take);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (left == 0) break;                                              // (wave-uniform)
        const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(left))) - 1u;
        const uint32_t d = static_cast<uint32_t>(__shfl(static_cast<int>(digit), static_cast<int>(leader), 64));
        const bool same = take && digit == d;
        const uint64_t ms = __ballot(same);
        if (lane == leader) atomicAdd(&hist[d], static_cast<uint32_t>(__popcll(ms)));
        take = take && !same;
        left &= ~ms;
    }
    if (take) atomicAdd(&hist[digit], 1u);
}

// the bins that hold ranks k1 and k2 of the histogram: res = {bin, elements in lower bins, elements in the bin} x 2
__device__ __forceinline__ void find_bins(const uint32_t* hist, uint32_t tid, uint32_t k1, uint32_t k2, uint32_t* wtot, uint32_t* res) {
    constexpr uint32_t per = kBins / kThreads;                             // 16 consecutive bins per thread
    uint32_t c[per];
#pragma unroll
    for (uint32_t q = 0; q < per / 4; ++q) {
        const uint4 x = reinterpret_cast<const uint4*>(hist)[tid * (per / 4) + q];
        c[4 * q] = x.x; c[4 * q + 1] = x.y; c[4 * q + 2] = x.z; c[4 * q + 3] = x.w;
    }
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < per; ++i) sum += c[i];
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    uint32_t incl = sum;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t y = static_cast<uint32_t>(__shfl_up(static_cast<int>(incl), off, 64));
        if (lane >= off) incl += y;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t ex = incl - sum;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) ex += w < wave ? wtot[w] : 0u;
#pragma unroll
    for (uint32_t which = 0; which < 2; ++which) {
        const uint32_t k = which ? k2 : k1;
        if (k >= ex && k - ex < sum) {
            uint32_t acc = ex, bin = 0, below = 0, inbin = 0;
            bool found = false;
#pragma unroll
            for (uint32_t i = 0; i < per; ++i) {
                if (!found && k - acc < c[i]) {
                    found = true;
                    bin = tid * per + i;
                    below = acc;
                    inbin = c[i];
                }
                acc += found ? 0u : c[i];
            }
            res[3 * which] = bin;
            res[3 * which + 1] = below;
            res[3 * which + 2] = inbin;
        }
    }
    __syncthreads();
}

__device__ inline uint64_t wave_max(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t y = static_cast<uint64_t>(__shfl_xor(static_cast<long long>(v), off, 64));
        v = y > v ? y : v;
    }
    return v;
}

__device__ inline uint64_t wave_min(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t y = static_cast<uint64_t>(__shfl_xor(static_cast<long long>(v), off, 64));
        v = y < v ? y : v;
    }
    return v;
}

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void rowmed_kernel(const T* __restrict__ D, uint64_t ld, uint32_t n, double* __restrict__ out,
                                                          unsigned long long* __restrict__ passes) {
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[kBins];
    __shared__ uint64_t s_cand[kCap];
    __shared__ uint32_t s_wtot[kWaves];
    __shared__ uint32_t s_res[6];
    __shared__ uint32_t s_cnt, s_nan;
    __shared__ unsigned long long s_lo, s_hi;

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const T* s = D + static_cast<uint64_t>(blockIdx.x) * ld;
    uint32_t k1 = (n - 1) / 2, k2 = n / 2, m = n, mc = 0, bits_left = 64, reads = 0;
    uint64_t prefix = 0, mask = 0, lo = 0, hi = 0;
    bool in_lds = false, nan = false;
    if (tid == 0) {
        s_cnt = 0;
        s_nan = 0;
        s_lo = 0;
        s_hi = ~0ull;
    }
    __syncthreads();

    for (;;) {
        if (!in_lds && m <= kCap) {
            // collect: the candidates move into LDS (their order there is immaterial)
            sweep_row<T, ALIGNED>(s, n, tid, [&](uint64_t key, bool valid) {
                nan = nan || (valid && key == PO_NAN_KEY);
                const bool take = valid && ((key ^ prefix) & mask) == 0;
                const uint64_t mt = __ballot(take);
                if (mt != 0) {                                             // (wave-uniform)
                    const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(mt))) - 1u;
                    uint32_t base = 0;
                    if (lane == leader) base = atomicAdd(&s_cnt, static_cast<uint32_t>(__popcll(mt)));
                    base = static_cast<uint32_t>(__shfl(static_cast<int>(base), static_cast<int>(leader), 64));
                    const uint32_t pos = base + lane_rank(mt);
                    if (take && pos < kCap) s_cand[pos] = key;             // (pos < m <= kCap by the histogram's count)
                }
            });
            ++reads;
            in_lds = true;
            mc = m;
            __syncthreads();
        }
        const uint32_t width = bits_left < kDigitBits ? bits_left : kDigitBits;
        const uint32_t shift = bits_left - width;
        const uint32_t dmask = (1u << width) - 1u;
        for (uint32_t i = tid; i < kBins; i += kThreads) s_hist[i] = 0;
        __syncthreads();
        if (in_lds) {
            for (uint32_t i0 = 0; i0 < mc; i0 += kThreads) {
                const uint32_t i = i0 + tid;
                const uint64_t key = i < mc ? s_cand[i] : 0;
                hist_add(s_hist, static_cast<uint32_t>(key >> shift) & dmask, i < mc && ((key ^ prefix) & mask) == 0, lane);
            }
        } else {
            sweep_row<T, ALIGNED>(s, n, tid, [&](uint64_t key, bool valid) {
                nan = nan || (valid && key == PO_NAN_KEY);
                hist_add(s_hist, static_cast<uint32_t>(key >> shift) & dmask, valid && ((key ^ prefix) & mask) == 0, lane);
            });
            ++reads;
        }
        __syncthreads();
        find_bins(s_hist, tid, k1, k2, s_wtot, s_res);
        const uint32_t b1 = s_res[0], below1 = s_res[1], cnt1 = s_res[2], b2 = s_res[3];
        const uint64_t digit_mask = static_cast<uint64_t>(dmask) << shift;
        if (b1 == b2) {
            prefix |= static_cast<uint64_t>(b1) << shift;
            mask |= digit_mask;
            k1 -= below1;
            k2 -= below1;
            m = cnt1;
            bits_left -= width;
            __syncthreads();                                               // s_res is written again by the next digit
            if (bits_left == 0) {
                lo = hi = prefix;
                break;
            }
            continue;
        }
        // the two ranks part here: lo is the largest key under (prefix, b1), hi the smallest under (prefix, b2)
        const uint64_t p1 = prefix | (static_cast<uint64_t>(b1) << shift), p2 = prefix | (static_cast<uint64_t>(b2) << shift);
        const uint64_t mask2 = mask | digit_mask;
        uint64_t mx = 0, mn = ~0ull;
        auto see = [&](uint64_t key, bool valid) {
            if (valid && ((key ^ p1) & mask2) == 0) mx = key > mx ? key : mx;
            if (valid && ((key ^ p2) & mask2) == 0) mn = key < mn ? key : mn;
        };
        if (in_lds) {
            for (uint32_t i = tid; i < mc; i += kThreads) see(s_cand[i], true);
        } else {
            sweep_row<T, ALIGNED>(s, n, tid, see);
            ++reads;
        }
        mx = wave_max(mx);
        mn = wave_min(mn);
        if (lane == 0) {
            atomicMax(&s_lo, static_cast<unsigned long long>(mx));
            atomicMin(&s_hi, static_cast<unsigned long long>(mn));
        }
        __syncthreads();
        lo = s_lo;
        hi = s_hi;
        break;
    }
    if (nan) atomicOr(&s_nan, 1u);
    __syncthreads();
    if (tid == 0) {
        const double a = key_value(lo), b = key_value(hi);
        double r = (n & 1u) ? a : (a + b) * 0.5;
        if (s_nan) r = __longlong_as_double(0x7FF8000000000000ll);
        out[blockIdx.x] = r;
        atomicAdd(passes, static_cast<unsigned long long>(reads));
    }
}

template <typename T>
int launch_rowmed(po_ctx* ctx, const T* D, uint64_t ld, uint32_t n, uint32_t rows, double* out, unsigned long long* passes) {
    const dim3 grid(rows), block(kThreads);
    if (po_rows_aligned(D, ld, sizeof(T))) hipLaunchKernelGGL((rowmed_kernel<T, true>), grid, block, 0, ctx->stream, D, ld, n, out, passes);
    else hipLaunchKernelGGL((rowmed_kernel<T, false>), grid, block, 0, ctx->stream, D, ld, n, out, passes);
    PO_CHECK_LAUNCH("rowmed_kernel");
    return PO_OK;
}

}  // namespace

extern "C" int po_row_medians_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t rows, uint64_t n, uint64_t ld, double* d_out) {
    const char* who = "po_row_medians_dev";
    PO_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    PO_REQUIRE(dtype == PO_F64 || dtype == PO_F32, "%s: dtype must be PO_F64 or PO_F32 (got %d)", who, dtype);
    PO_REQUIRE(n < (1ull << 31), "%s: n = %llu is above 2^31 - 1", who, (unsigned long long)n);
    PO_HIP(hipSetDevice(ctx->device));
    int rc = po_buf_reserve(ctx, &ctx->ws_rowmed, 256);
    if (rc) return rc;
    unsigned long long* passes = static_cast<unsigned long long*>(ctx->ws_rowmed.p);
    PO_HIP(hipMemsetAsync(passes, 0, 8, ctx->stream));
    if (rows == 0 || n == 0) return PO_OK;
    PO_REQUIRE(ld >= n, "%s: ld = %llu is smaller than n = %llu", who, (unsigned long long)ld, (unsigned long long)n);
    PO_REQUIRE(d_matrix != nullptr && d_out != nullptr, "%s: NULL buffer", who);
    const size_t esz = dtype == PO_F32 ? 4 : 8;
    PO_REQUIRE((reinterpret_cast<uintptr_t>(d_matrix) % esz) == 0, "%s: the matrix pointer is not aligned to its element size", who);
    const uint64_t step = 1ull << 30;                                      // rows per launch: one workgroup each
    for (uint64_t r0 = 0; r0 < rows; r0 += step) {
        const uint32_t cnt = static_cast<uint32_t>(rows - r0 < step ? rows - r0 : step);
        const uint8_t* base = static_cast<const uint8_t*>(d_matrix) + r0 * ld * esz;
        if (dtype == PO_F32) rc = launch_rowmed<float>(ctx, reinterpret_cast<const float*>(base), ld, (uint32_t)n, cnt, d_out + r0, passes);
        else rc = launch_rowmed<double>(ctx, reinterpret_cast<const double*>(base), ld, (uint32_t)n, cnt, d_out + r0, passes);
        if (rc) return rc;
    }
    return PO_OK;
}

extern "C" int po_row_medians_passes(po_ctx* ctx, uint64_t* passes) {
    const char* who = "po_row_medians_passes";
    PO_REQUIRE(ctx != nullptr && passes != nullptr, "%s: NULL argument", who);
    *passes = 0;
    if (!ctx->ws_rowmed.p) return PO_OK;
    PO_HIP(hipSetDevice(ctx->device));
    PO_HIP(hipMemcpyAsync(passes, ctx->ws_rowmed.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    return PO_OK;
}
