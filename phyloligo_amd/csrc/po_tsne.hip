// t-SNE of the k-NN graph (po_tsne*, include/phyloligo_amd.h): scikit-learn's algorithm (manifold/_t_sne.py, _utils.pyx) with
// the repulsive sum taken exactly over all pairs instead of through a Barnes-Hut tree.
//
// Affinities (tsne_affinity_kernel, one wave per row): the squared neighbour values, rounded to float32 as scikit-learn holds
// them, sit in LDS; the binary search for beta runs in float64 (at most 100 steps, |H - log perplexity| <= 1e-5); the row's
// conditional probabilities go to HBM as float64 [n][K].  A NaN / negative value or a neighbour index outside 0..n-1 lowers
// an error word to the first offending row (integer atomicMin: the answer does not depend on timing).
//
// Joint probabilities P = (C + C^T) / sum: every row gets its own K entries and, behind them, the entries of the rows that
// list it (in-degree counted with integer atomics, so a hub row is as long as it needs to be - nothing is sized by K).  The
// transposed entries arrive in any order; an entry whose partner is in the row's own list is added to it and dropped, and
// the survivors are placed by rank (number of smaller columns in the row), so that the CSR - rowptr int64 [n+1], columns
// int32 ascending within a row, values float32 - holds the same bytes on every call.
//
// Gradient: tsne_repulse_kernel is the hot loop.  A workgroup owns 256 x IPT points i (IPT per lane, in registers) and a
// range of j tiles; a tile of 256 points goes through LDS and every lane reads the same j (broadcast, 16 bytes = two points
// per read).  Per pair: 2 subtractions, 2 fma for 1 + d^2, v_rcp_f32, one add for Z, one multiply and 2 fma for the force.
// Sums run in float32 within a tile and in float64 across tiles; the partial forces of the S j-ranges go to HBM as float64
// [S][n][2] and the partial Z of every workgroup to [S][row blocks]: both are added up later in a fixed order.  The point
// itself is not skipped inside the loop (q = 1 exactly, force 0 exactly): n is taken off Z at the reduction.
// tsne_attract_kernel (one wave per point) adds the attraction over the point's CSR row, the S partial repulsions, forms
// grad = 4 (attraction - repulsion / Z), and - in the optimiser - applies scikit-learn's gains / momentum update in float32,
// writing the next embedding into the other of two buffers.  KL and |grad|^2 are per-point float64 terms summed by
// reduce_sum_kernel (one workgroup, fixed order).  No floating-point atomics anywhere.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "po_internal.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTile = 256;                 // j points per LDS tile of the repulsion kernel
constexpr double kPerplexityTolerance = 1e-5;   // _utils.pyx
constexpr double kEpsilonDbl = 1e-8;            // _utils.pyx: a row sum of 0

template <typename T>
__device__ inline T wave_sum(T v) {             // xor butterfly: the same order on every call
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---- affinities ----------------------------------------------------------------------------------------------------------
// err[0]: first row with a NaN value, err[1]: with a negative value, err[2]: with a neighbour index outside 0..n-1 or equal to the row
template <typename T>
__global__ __launch_bounds__(64) void tsne_affinity_kernel(const int32_t* __restrict__ idx, const T* __restrict__ val, uint32_t n,
                                                           uint32_t k, double log_perp, double* __restrict__ beta_out,
                                                           double* __restrict__ cond, double* __restrict__ rowsum,
                                                           uint32_t* __restrict__ err) {
    extern __shared__ double sh[];              // d2[k], p[k]
    double* d2 = sh;
    double* p = sh + k;
    const uint32_t row = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)row * k;
    bool bad_nan = false, bad_neg = false, bad_idx = false;
    for (uint32_t c = lane; c < k; c += 64) {
        const double d = (double)val[base + c];
        const int32_t j = idx[base + c];
        bad_nan |= d != d;
        bad_neg |= d < 0.0;
        bad_idx |= j < 0 || (uint32_t)j >= n || (uint32_t)j == row;
        d2[c] = (double)(float)(d * d);         // distances_nn.data **= 2, then float32 (_joint_probabilities_nn)
    }
    if (bad_nan) atomicMin(&err[0], row);
    if (bad_neg) atomicMin(&err[1], row);
    if (bad_idx) atomicMin(&err[2], row);
    __syncthreads();
    double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY, sum_pi = 1.0;
    for (int step = 0; step < 100; ++step) {
        double s = 0.0;
        for (uint32_t c = lane; c < k; c += 64) {
            const double e = exp(-d2[c] * beta);
            p[c] = e;
            s += e;
        }
        sum_pi = wave_sum(s);
        if (sum_pi == 0.0) sum_pi = kEpsilonDbl;
        double sd = 0.0;
        for (uint32_t c = lane; c < k; c += 64) {
            const double q = p[c] / sum_pi;
            p[c] = q;
            sd += d2[c] * q;
        }
        sd = wave_sum(sd);
        const double diff = log(sum_pi) + beta * sd - log_perp;
        if (fabs(diff) <= kPerplexityTolerance) break;
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
    double s = 0.0;
    for (uint32_t c = lane; c < k; c += 64) {
        cond[base + c] = p[c];
        s += p[c];
    }
    s = wave_sum(s);
    if (lane == 0) {
        rowsum[row] = s;
        if (beta_out) beta_out[row] = beta;
    }
}

// out[0] = max(sum(in[0..count)) * scale - subtract, floor_): one workgroup, every thread a strided share, then a tree
__global__ __launch_bounds__(1024) void reduce_sum_kernel(const double* __restrict__ in, uint64_t count, double scale, double subtract,
                                                          double floor_, double* __restrict__ out) {
    __shared__ double sh[1024];
    double s = 0.0;
    for (uint64_t i = threadIdx.x; i < count; i += 1024) s += in[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t m = 512; m >= 1; m >>= 1) {
        if (threadIdx.x < m) sh[threadIdx.x] += sh[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double v = sh[0] * scale - subtract;
        out[0] = v > floor_ ? v : floor_;
    }
}

// ---- joint probabilities: CSR of (C + C^T) / sum ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_indeg_kernel(const int32_t* __restrict__ idx, uint64_t total, uint32_t* __restrict__ indeg) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) atomicAdd(&indeg[idx[e]], 1u);
}

// ptr[i] = sum over t < i of (cnt[t] + add), ptr[n] = the total
__global__ __launch_bounds__(1024) void tsne_scan_kernel(const uint32_t* __restrict__ cnt, uint32_t add, uint32_t n,
                                                         int64_t* __restrict__ ptr) {
    __shared__ int64_t part[1024];
    const uint32_t per = (n + 1023) / 1024;
    const uint32_t lo = threadIdx.x * per < n ? threadIdx.x * per : n;
    const uint32_t hi = lo + per < n ? lo + per : n;
    int64_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += (int64_t)cnt[i] + add;
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (uint32_t t = 0; t < 1024; ++t) {
            const int64_t v = part[t];
            part[t] = run;
            run += v;
        }
        ptr[n] = run;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (uint32_t i = lo; i < hi; ++i) {
        ptr[i] = run;
        run += (int64_t)cnt[i] + add;
    }
}

// row i: its own K entries first (in list order), then the entries of the rows that list i, in the order their atomics landed
__global__ __launch_bounds__(256) void tsne_fill_kernel(const int32_t* __restrict__ idx, const double* __restrict__ cond, uint32_t k,
                                                        uint64_t total, const int64_t* __restrict__ tptr, uint32_t* __restrict__ cursor,
                                                        int32_t* __restrict__ tcol, double* __restrict__ tval) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const uint32_t i = (uint32_t)(e / k), c = (uint32_t)(e % k);
    const int32_t j = idx[e];
    const double v = cond[e];
    tcol[tptr[i] + c] = j;
    tval[tptr[i] + c] = v;
    const uint32_t pos = atomicAdd(&cursor[j], 1u);
    tcol[tptr[j] + k + pos] = (int32_t)i;
    tval[tptr[j] + k + pos] = v;
}

// one workgroup per row: a transposed entry whose column is in the row's own list is added to that entry and dropped (-1);
// err_dup is lowered to the first row whose own list names a neighbour twice (the caller then stops before the placement)
__global__ __launch_bounds__(256) void tsne_mark_kernel(uint32_t k, const int64_t* __restrict__ tptr, int32_t* __restrict__ tcol,
                                                        double* __restrict__ tval, uint32_t* __restrict__ rowcnt,
                                                        uint32_t* __restrict__ err_dup) {
    __shared__ int32_t own[PO_KNN_MAX_K];
    __shared__ uint32_t live;
    const uint32_t row = blockIdx.x;
    const int64_t base = tptr[row];
    const uint32_t len = (uint32_t)(tptr[row + 1] - base);
    for (uint32_t c = threadIdx.x; c < k; c += 256) own[c] = tcol[base + c];
    if (threadIdx.x == 0) live = 0;
    __syncthreads();
    // a neighbour listed twice in the row's own list would give some other row two entries for one column
    bool dup = false;
    for (uint32_t c = threadIdx.x; c < k; c += 256)
        for (uint32_t c2 = 0; c2 < c; ++c2) dup |= own[c2] == own[c];
    if (dup) atomicMin(err_dup, row);
    uint32_t mine = 0;
    for (uint32_t t = k + threadIdx.x; t < len; t += 256) {
        const int32_t i = tcol[base + t];
        uint32_t hit = k;
        for (uint32_t c = 0; c < k; ++c)
            if (own[c] == i) hit = c;
        if (hit < k) {
            tval[base + hit] += tval[base + t];     // the only writer of this entry: (i -> row) exists once
            tcol[base + t] = -1;
        } else {
            ++mine;
        }
    }
    if (mine) atomicAdd(&live, mine);
    __syncthreads();
    if (threadIdx.x == 0) rowcnt[row] = live;       // the scan adds the k own entries
}

// one workgroup per row: every surviving entry goes to the place of its rank among the row's surviving columns
__global__ __launch_bounds__(256) void tsne_place_kernel(const int64_t* __restrict__ tptr, const int32_t* __restrict__ tcol,
                                                         const double* __restrict__ tval, const double* __restrict__ total,
                                                         const int64_t* __restrict__ rowptr, int32_t* __restrict__ col,
                                                         float* __restrict__ pval) {
    const uint32_t row = blockIdx.x;
    const int64_t base = tptr[row];
    const uint32_t len = (uint32_t)(tptr[row + 1] - base);
    const int64_t out = rowptr[row];
    const double sum = total[0];
    for (uint32_t e = threadIdx.x; e < len; e += 256) {
        const int32_t ce = tcol[base + e];
        if (ce < 0) continue;
        uint32_t rank = 0;
        for (uint32_t t = 0; t < len; ++t) {
            const int32_t ct = tcol[base + t];
            rank += (ct >= 0 && ct < ce) ? 1u : 0u;
        }
        col[out + rank] = ce;
        pval[out + rank] = (float)(tval[base + e] / sum);
    }
}

// ---- gradient --------------------------------------------------------------------------------------------------------------
__device__ inline void repulse_pair(float xi, float yi, float xj, float yj, float& fx, float& fy, float& z) {
    const float dx = xi - xj, dy = yi - yj;
    const float d = __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, 1.0f));
    const float q = __builtin_amdgcn_rcpf(d);
    z += q;
    const float q2 = q * q;
    fx = __builtin_fmaf(q2, dx, fx);
    fy = __builtin_fmaf(q2, dy, fy);
}

// grid (row blocks, S): workgroup (rb, s) owns points rb * 256 * IPT + m * 256 + lane (m < IPT) and j tiles
// [s * tiles_per_split, (s + 1) * tiles_per_split)
template <int IPT>
__global__ __launch_bounds__(256) void tsne_repulse_kernel(const float2* __restrict__ y, uint32_t n, uint32_t tiles_per_split,
                                                           double* __restrict__ part_f, double* __restrict__ part_z) {
    __shared__ float4 tile[kTile / 2];
    __shared__ double zw[kThreads / 64];
    const uint32_t tid = threadIdx.x, rb = blockIdx.x, s = blockIdx.y;
    const uint32_t n_tiles = (n + kTile - 1) / kTile;
    const uint32_t t_begin = s * tiles_per_split;
    const uint32_t t_end = t_begin + tiles_per_split < n_tiles ? t_begin + tiles_per_split : n_tiles;
    float xi[IPT], yi[IPT];
    double acc_x[IPT], acc_y[IPT], acc_z = 0.0;
#pragma unroll
    for (int m = 0; m < IPT; ++m) {
        const uint32_t i = rb * kThreads * IPT + m * kThreads + tid;
        const float2 p = y[i < n ? i : n - 1];
        xi[m] = p.x;
        yi[m] = p.y;
        acc_x[m] = acc_y[m] = 0.0;
    }
    for (uint32_t t = t_begin; t < t_end; ++t) {
        const uint32_t j0 = t * kTile;
        const uint32_t cnt = n - j0 < kTile ? n - j0 : kTile;
        const float2 pj = j0 + tid < n ? y[j0 + tid] : make_float2(0.0f, 0.0f);
        __syncthreads();
        reinterpret_cast<float2*>(tile)[tid] = pj;
        __syncthreads();
        float fx[IPT], fy[IPT], z[IPT];
#pragma unroll
        for (int m = 0; m < IPT; ++m) fx[m] = fy[m] = z[m] = 0.0f;
        if (cnt == kTile) {
#pragma unroll 4
            for (uint32_t u = 0; u < kTile / 2; ++u) {
                const float4 q = tile[u];
#pragma unroll
                for (int m = 0; m < IPT; ++m) {
                    repulse_pair(xi[m], yi[m], q.x, q.y, fx[m], fy[m], z[m]);
                    repulse_pair(xi[m], yi[m], q.z, q.w, fx[m], fy[m], z[m]);
                }
            }
        } else {
            for (uint32_t u = 0; u < cnt; ++u) {
                const float2 q = reinterpret_cast<const float2*>(tile)[u];
#pragma unroll
                for (int m = 0; m < IPT; ++m) repulse_pair(xi[m], yi[m], q.x, q.y, fx[m], fy[m], z[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < IPT; ++m) {
            const uint32_t i = rb * kThreads * IPT + m * kThreads + tid;
            acc_x[m] += (double)fx[m];
            acc_y[m] += (double)fy[m];
            if (i < n) acc_z += (double)z[m];
        }
    }
#pragma unroll
    for (int m = 0; m < IPT; ++m) {
        const uint32_t i = rb * kThreads * IPT + m * kThreads + tid;
        if (i < n) {
            double2 f;
            f.x = acc_x[m];
            f.y = acc_y[m];
            reinterpret_cast<double2*>(part_f)[(size_t)s * n + i] = f;
        }
    }
    acc_z = wave_sum(acc_z);
    if ((tid & 63) == 0) zw[tid >> 6] = acc_z;
    __syncthreads();
    if (tid == 0) part_z[(size_t)s * gridDim.x + rb] = ((zw[0] + zw[1]) + zw[2]) + zw[3];
}

struct tsne_step {
    float momentum, lr, min_gain;
};

// One wave per point: attraction over the CSR row, the S partial repulsions, grad = 4 (attraction - repulsion / Z).
// UPDATE: gains / momentum step into y_out (y itself is only read: other waves still need the old neighbours); else the
// gradient goes to grad_out.  klrow / gnrow (may be NULL): the point's terms of the KL divergence and of |grad|^2.
template <bool UPDATE>
__global__ __launch_bounds__(256) void tsne_attract_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           const float* __restrict__ pval, const float2* __restrict__ y, uint32_t n,
                                                           float exaggeration, const double* __restrict__ part_f, uint32_t splits,
                                                           const double* __restrict__ zp, float2* __restrict__ grad_out,
                                                           float2* __restrict__ y_out, float2* __restrict__ upd,
                                                           float2* __restrict__ gains, tsne_step st, double* __restrict__ klrow,
                                                           double* __restrict__ gnrow) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const float2 yi = y[row];
    const double z = zp[0];
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    float ax = 0.0f, ay = 0.0f;
    double kl = 0.0;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const float2 yj = y[col[e]];
        const float p = pval[e] * exaggeration;
        const float dx = yi.x - yj.x, dy = yi.y - yj.y;
        const float q = __builtin_amdgcn_rcpf(__builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, 1.0f)));
        const float pq = p * q;
        ax = __builtin_fmaf(pq, dx, ax);
        ay = __builtin_fmaf(pq, dy, ay);
        if (klrow) {
            const double pd = (double)p, qn = (double)q / z;
            kl += pd * log((pd > (double)FLT_MIN ? pd : (double)FLT_MIN) / (qn > (double)FLT_MIN ? qn : (double)FLT_MIN));
        }
    }
    double rx = 0.0, ry = 0.0;
    if (lane < splits) {
        const double2 f = reinterpret_cast<const double2*>(part_f)[(size_t)lane * n + row];
        rx = f.x;
        ry = f.y;
    }
    const double sax = wave_sum((double)ax), say = wave_sum((double)ay);
    rx = wave_sum(rx);
    ry = wave_sum(ry);
    if (klrow) kl = wave_sum(kl);
    if (lane != 0) return;
    float gx = (float)(4.0 * (sax - rx / z)), gy = (float)(4.0 * (say - ry / z));
    if (klrow) klrow[row] = kl;
    if (UPDATE) {
        float2 u = upd[row], g = gains[row];
        g.x = u.x * gx < 0.0f ? g.x + 0.2f : g.x * 0.8f;
        g.y = u.y * gy < 0.0f ? g.y + 0.2f : g.y * 0.8f;
        g.x = g.x < st.min_gain ? st.min_gain : g.x;
        g.y = g.y < st.min_gain ? st.min_gain : g.y;
        gx *= g.x;
        gy *= g.y;
        u.x = st.momentum * u.x - st.lr * gx;
        u.y = st.momentum * u.y - st.lr * gy;
        gains[row] = g;
        upd[row] = u;
        y_out[row] = make_float2(yi.x + u.x, yi.y + u.y);
    } else {
        grad_out[row] = make_float2(gx, gy);
    }
    if (gnrow) gnrow[row] = (double)gx * (double)gx + (double)gy * (double)gy;
}

__global__ __launch_bounds__(256) void tsne_check_csr_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, uint32_t n,
                                                             uint64_t nnz, uint32_t* __restrict__ err) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    bool bad = e0 < 0 || e1 < e0 || (uint64_t)e1 > nnz || (row == 0 && e0 != 0);
    if (!bad)
        for (int64_t e = e0; e < e1; ++e) bad |= col[e] < 0 || (uint32_t)col[e] >= n;
    if (bad) atomicMin(&err[0], row);
}

uint32_t repulse_ipt(uint64_t n) { return n >= 16384 ? 4u : 1u; }

}  // namespace

// ---- launchers -------------------------------------------------------------------------------------------------------------
void po_tsne_split(uint64_t n, uint32_t* row_blocks, uint32_t* splits, uint32_t* tiles_per_split) {
    const uint32_t ipt = repulse_ipt(n);
    const uint32_t rbs = (uint32_t)((n + kThreads * ipt - 1) / (kThreads * ipt));
    const uint32_t n_tiles = (uint32_t)((n + kTile - 1) / kTile);
    // about 1 024 workgroups (four per CU of the 256): a property of the problem size alone, so that the summation order is too
    uint32_t want = (1024 + rbs - 1) / rbs;
    if (want > 64) want = 64;                    // the attraction kernel adds the partials with one lane each
    if (want > n_tiles) want = n_tiles;
    if (want < 1) want = 1;
    const uint32_t tps = (n_tiles + want - 1) / want;
    *row_blocks = rbs;
    *tiles_per_split = tps;
    *splits = (n_tiles + tps - 1) / tps;
}

size_t po_tsne_grad_workspace(uint64_t n) {
    uint32_t rbs, s, tps;
    po_tsne_split(n, &rbs, &s, &tps);
    // part_f [S][n][2], part_z [S][rbs], klrow [n], gnrow [n], scalars [8]
    return ((size_t)s * n * 2 + (size_t)s * rbs + 2 * n + 8) * sizeof(double);
}

// gradient of one embedding; ws: po_tsne_grad_workspace(n) bytes.  d_scalars = ws scalars: [0] Z, [1] KL, [2] |grad|^2
int po_launch_tsne_gradient(po_ctx* ctx, const int64_t* d_rowptr, const int32_t* d_col, const float* d_p, const float* d_y, uint64_t n,
                            double exaggeration, void* ws, bool update, float* d_grad, float* d_y_out, float* d_upd, float* d_gains,
                            double momentum, double lr, double min_gain, bool want_kl, bool want_gn, double** d_scalars,
                            hipEvent_t* ev) {
    uint32_t rbs, splits, tps;
    po_tsne_split(n, &rbs, &splits, &tps);
    double* part_f = static_cast<double*>(ws);
    double* part_z = part_f + (size_t)splits * n * 2;
    double* klrow = part_z + (size_t)splits * rbs;
    double* gnrow = klrow + n;
    double* scal = gnrow + n;
    *d_scalars = scal;
    const float2* y = reinterpret_cast<const float2*>(d_y);
    const dim3 grid(rbs, splits), block(kThreads);
    if (ev) PO_HIP(hipEventRecord(ev[0], ctx->stream));
    if (repulse_ipt(n) == 4)
        hipLaunchKernelGGL(tsne_repulse_kernel<4>, grid, block, 0, ctx->stream, y, (uint32_t)n, tps, part_f, part_z);
    else
        hipLaunchKernelGGL(tsne_repulse_kernel<1>, grid, block, 0, ctx->stream, y, (uint32_t)n, tps, part_f, part_z);
    PO_CHECK_LAUNCH("tsne_repulse_kernel");
    if (ev) PO_HIP(hipEventRecord(ev[1], ctx->stream));
    hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, part_z, (uint64_t)splits * rbs, 1.0, (double)n, DBL_EPSILON,
                       scal);
    PO_CHECK_LAUNCH("reduce_sum_kernel");
    if (ev) PO_HIP(hipEventRecord(ev[2], ctx->stream));
    tsne_step st;
    st.momentum = (float)momentum;
    st.lr = (float)lr;
    st.min_gain = (float)min_gain;
    const dim3 agrid((uint32_t)((n + 3) / 4));
    if (update)
        hipLaunchKernelGGL(tsne_attract_kernel<true>, agrid, block, 0, ctx->stream, d_rowptr, d_col, d_p, y, (uint32_t)n, (float)exaggeration,
                           part_f, splits, scal, (float2*)nullptr, reinterpret_cast<float2*>(d_y_out), reinterpret_cast<float2*>(d_upd),
                           reinterpret_cast<float2*>(d_gains), st, want_kl ? klrow : nullptr, want_gn ? gnrow : nullptr);
    else
        hipLaunchKernelGGL(tsne_attract_kernel<false>, agrid, block, 0, ctx->stream, d_rowptr, d_col, d_p, y, (uint32_t)n, (float)exaggeration,
                           part_f, splits, scal, reinterpret_cast<float2*>(d_grad), (float2*)nullptr, (float2*)nullptr, (float2*)nullptr, st,
                           want_kl ? klrow : nullptr, want_gn ? gnrow : nullptr);
    PO_CHECK_LAUNCH("tsne_attract_kernel");
    if (ev) PO_HIP(hipEventRecord(ev[3], ctx->stream));
    if (want_kl) {
        hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, klrow, n, 1.0, 0.0, -DBL_MAX, scal + 1);
        PO_CHECK_LAUNCH("reduce_sum_kernel");
    }
    if (want_gn) {
        hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, gnrow, n, 1.0, 0.0, -DBL_MAX, scal + 2);
        PO_CHECK_LAUNCH("reduce_sum_kernel");
    }
    return PO_OK;
}

// rows, columns and extents of a caller's CSR: err word lowered to the first bad row (the gradient kernels index y with col)
int po_launch_tsne_check_csr(po_ctx* ctx, const int64_t* d_rowptr, const int32_t* d_col, uint64_t n, uint64_t nnz, uint32_t* d_err) {
    hipLaunchKernelGGL(tsne_check_csr_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_rowptr, d_col, (uint32_t)n, nnz,
                       d_err);
    PO_CHECK_LAUNCH("tsne_check_csr_kernel");
    return PO_OK;
}

size_t po_tsne_affinity_workspace(uint64_t n, uint32_t k) {
    const uint64_t e = n * (uint64_t)k;
    // cond [n][k] f64, rowsum [n] f64, total [2] f64, tptr [n+1] i64, tval [2e] f64, tcol [2e] i32, indeg / cursor / rowcnt [n] u32 each, err [4]
    return e * 8 + n * 8 + 16 + (n + 1) * 8 + 2 * e * 8 + 2 * e * 4 + 3 * n * 4 + 16 + 256;
}

// Stage 1 of po_tsne_affinities_dev: search + validation; the three error words are copied to h_err (pinned) and the stream is
// waited for.  d_cond (may be NULL): the caller's copy of the conditional probabilities.
int po_launch_tsne_affinities(po_ctx* ctx, uint64_t n, uint32_t k, int val_f32, const int32_t* d_idx, const void* d_val, double perplexity,
                              double* d_beta, double* d_cond, void* ws, uint32_t* h_err) {
    const uint64_t e = n * (uint64_t)k;
    double* cond = static_cast<double*>(ws);
    double* rowsum = cond + e;
    double* total = rowsum + n;
    uint8_t* tail = reinterpret_cast<uint8_t*>(total + 2) + (n + 1) * 8 + 2 * e * 8 + 2 * e * 4 + 3 * n * 4;
    uint32_t* err = reinterpret_cast<uint32_t*>(tail);
    PO_HIP(hipMemsetAsync(err, 0xFF, 16, ctx->stream));
    const size_t shmem = 2 * (size_t)k * sizeof(double);
    if (val_f32)
        hipLaunchKernelGGL(tsne_affinity_kernel<float>, dim3((uint32_t)n), dim3(64), shmem, ctx->stream, d_idx, static_cast<const float*>(d_val),
                           (uint32_t)n, k, log(perplexity), d_beta, cond, rowsum, err);
    else
        hipLaunchKernelGGL(tsne_affinity_kernel<double>, dim3((uint32_t)n), dim3(64), shmem, ctx->stream, d_idx,
                           static_cast<const double*>(d_val), (uint32_t)n, k, log(perplexity), d_beta, cond, rowsum, err);
    PO_CHECK_LAUNCH("tsne_affinity_kernel");
    if (d_cond) PO_HIP(hipMemcpyAsync(d_cond, cond, e * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    PO_HIP(hipMemcpyAsync(h_err, err, 16, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    return PO_OK;
}

// Stage 2: the CSR.  Two steps, because the caller's buffers must hold *nnz entries before anything is written to them:
// step 0 builds the temporary rows and row pointers and reads nnz back (one synchronisation), step 1 places the entries.
int po_launch_tsne_joint(po_ctx* ctx, uint64_t n, uint32_t k, const int32_t* d_idx, void* ws, int64_t* d_rowptr, int32_t* d_col, float* d_p,
                         int step, int64_t* h_nnz, uint32_t* h_dup) {
    const uint64_t e = n * (uint64_t)k;
    double* cond = static_cast<double*>(ws);
    double* rowsum = cond + e;
    double* total = rowsum + n;
    int64_t* tptr = reinterpret_cast<int64_t*>(total + 2);
    double* tval = reinterpret_cast<double*>(tptr + n + 1);
    int32_t* tcol = reinterpret_cast<int32_t*>(tval + 2 * e);
    uint32_t* indeg = reinterpret_cast<uint32_t*>(tcol + 2 * e);
    uint32_t* cursor = indeg + n;
    uint32_t* rowcnt = cursor + n;
    uint32_t* err = rowcnt + n;                  // the four error words po_launch_tsne_affinities reset; [3]: duplicate neighbour
    const dim3 egrid((uint32_t)((e + 255) / 256));
    if (step == 0) {
        PO_HIP(hipMemsetAsync(indeg, 0, 2 * n * sizeof(uint32_t), ctx->stream));      // indeg and cursor
        hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, rowsum, n, 2.0, 0.0, DBL_EPSILON, total);
        PO_CHECK_LAUNCH("reduce_sum_kernel");
        hipLaunchKernelGGL(tsne_indeg_kernel, egrid, dim3(256), 0, ctx->stream, d_idx, e, indeg);
        PO_CHECK_LAUNCH("tsne_indeg_kernel");
        hipLaunchKernelGGL(tsne_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, indeg, k, (uint32_t)n, tptr);
        PO_CHECK_LAUNCH("tsne_scan_kernel");
        hipLaunchKernelGGL(tsne_fill_kernel, egrid, dim3(256), 0, ctx->stream, d_idx, cond, k, e, tptr, cursor, tcol, tval);
        PO_CHECK_LAUNCH("tsne_fill_kernel");
        hipLaunchKernelGGL(tsne_mark_kernel, dim3((uint32_t)n), dim3(256), 0, ctx->stream, k, tptr, tcol, tval, rowcnt, err + 3);
        PO_CHECK_LAUNCH("tsne_mark_kernel");
        hipLaunchKernelGGL(tsne_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, rowcnt, k, (uint32_t)n, d_rowptr);
        PO_CHECK_LAUNCH("tsne_scan_kernel");
        PO_HIP(hipMemcpyAsync(h_nnz, d_rowptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipMemcpyAsync(h_dup, err + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipStreamSynchronize(ctx->stream));
        return PO_OK;
    }
    hipLaunchKernelGGL(tsne_place_kernel, dim3((uint32_t)n), dim3(256), 0, ctx->stream, tptr, tcol, tval, total, d_rowptr, d_col, d_p);
    PO_CHECK_LAUNCH("tsne_place_kernel");
    return PO_OK;
}

// ---- the entry points ----------------------------------------------------------------------------------------------------
static int tsne_pinned(po_ctx* ctx) {
    if (!ctx->h_tsne) PO_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_tsne), 8 * sizeof(double), hipHostMallocDefault));
    return PO_OK;
}

static int check_tsne_lists(const char* who, uint64_t n, uint32_t k, int metric, int val_dtype, double perplexity) {
    PO_TRY(po_check_metric(metric));
    PO_REQUIRE(metric != PO_KT, "%s: metric KT is a correlation (lists ordered descending), not a distance: t-SNE cannot take it", who);
    PO_TRY(po_check_dtype(who, "val_dtype", val_dtype));
    PO_REQUIRE(perplexity >= 1.0, "%s: perplexity %g is below 1", who, perplexity);      // NaN fails this too
    PO_REQUIRE(3.0 * perplexity + 1.0 < (double)PO_KNN_MAX_K + 1.0,
               "%s: perplexity %g needs int(3 * perplexity + 1) = %.0f neighbours, more than PO_KNN_MAX_K = %u (perplexity <= %u)", who,
               perplexity, floor(3.0 * perplexity + 1.0), PO_KNN_MAX_K, (PO_KNN_MAX_K - 1) / 3);
    PO_REQUIRE(n >= 4, "%s: n = %llu, t-SNE needs at least 4 points", who, (unsigned long long)n);
    PO_REQUIRE(n < (1ull << 31), "%s: n = %llu does not fit int32 indices", who, (unsigned long long)n);
    const uint64_t want = (uint64_t)(3.0 * perplexity + 1.0);
    const uint64_t k_want = want < n - 1 ? want : n - 1;
    PO_REQUIRE(k == k_want, "%s: k = %u, but perplexity %g on %llu points takes min(n - 1, int(3 * perplexity + 1)) = %llu neighbours", who,
               k, perplexity, (unsigned long long)n, (unsigned long long)k_want);
    return PO_OK;
}

extern "C" int po_tsne_affinities_dev(po_ctx* ctx, uint64_t n, uint32_t k, int metric, int val_dtype, const int32_t* d_idx,
                                      const void* d_val, double perplexity, double* d_beta, double* d_cond, int64_t* d_rowptr,
                                      int32_t* d_col, float* d_p, uint64_t cap, uint64_t* nnz) {
    const char* who = "po_tsne_affinities_dev";
    PO_TRY(po_check_ctx(who, ctx));
    if (nnz) *nnz = 0;
    PO_TRY(check_tsne_lists(who, n, k, metric, val_dtype, perplexity));
    PO_REQUIRE(d_idx != nullptr && d_val != nullptr && d_rowptr != nullptr && d_col != nullptr && d_p != nullptr && nnz != nullptr,
               "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    PO_TRY(tsne_pinned(ctx));
    PO_TRY(po_buf_reserve(ctx, &ctx->ws_tsne_aff, po_tsne_affinity_workspace(n, k)));
    uint32_t* h_err = reinterpret_cast<uint32_t*>(ctx->h_tsne);
    PO_TRY(po_launch_tsne_affinities(ctx, n, k, val_dtype == PO_F32, d_idx, d_val, perplexity, d_beta, d_cond, ctx->ws_tsne_aff.p, h_err));
    PO_REQUIRE(h_err[2] == 0xFFFFFFFFu, "%s: row %u lists a neighbour index outside 0..n-1 or itself (an unfilled list?)", who, h_err[2]);
    PO_REQUIRE(h_err[0] == 0xFFFFFFFFu, "%s: row %u has a NaN neighbour value (an empty record under BC / SC?)", who, h_err[0]);
    PO_REQUIRE(h_err[1] == 0xFFFFFFFFu, "%s: row %u has a negative neighbour value: t-SNE needs distances", who, h_err[1]);
    int64_t* h_nnz = reinterpret_cast<int64_t*>(ctx->h_tsne + 2);
    uint32_t* h_dup = reinterpret_cast<uint32_t*>(ctx->h_tsne + 3);
    PO_TRY(po_launch_tsne_joint(ctx, n, k, d_idx, ctx->ws_tsne_aff.p, d_rowptr, d_col, d_p, 0, h_nnz, h_dup));
    PO_REQUIRE(*h_dup == 0xFFFFFFFFu, "%s: row %u lists a neighbour twice", who, *h_dup);
    *nnz = (uint64_t)*h_nnz;
    PO_REQUIRE(*nnz <= cap, "%s: the CSR has %llu entries, col / p hold %llu", who, (unsigned long long)*nnz, (unsigned long long)cap);
    return po_launch_tsne_joint(ctx, n, k, d_idx, ctx->ws_tsne_aff.p, d_rowptr, d_col, d_p, 1, h_nnz, h_dup);
}

// the caller's CSR indexes y: its extents and columns are checked on the device before a kernel follows them
static int tsne_check_csr(po_ctx* ctx, const char* who, uint64_t n, const int64_t* d_rowptr, const int32_t* d_col, uint64_t nnz, void* ws) {
    uint32_t* d_err = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws) + po_tsne_grad_workspace(n));
    uint32_t* h_err = reinterpret_cast<uint32_t*>(ctx->h_tsne);
    PO_HIP(hipMemsetAsync(d_err, 0xFF, 4, ctx->stream));
    PO_TRY(po_launch_tsne_check_csr(ctx, d_rowptr, d_col, n, nnz, d_err));
    PO_HIP(hipMemcpyAsync(h_err, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    PO_REQUIRE(h_err[0] == 0xFFFFFFFFu, "%s: row %u of the CSR has row pointers outside 0..nnz or a column outside 0..n-1", who, h_err[0]);
    return PO_OK;
}

extern "C" int po_tsne_gradient_dev(po_ctx* ctx, uint64_t n, const int64_t* d_rowptr, const int32_t* d_col, const float* d_p, uint64_t nnz,
                                    const float* d_y, double exaggeration, float* d_grad, double* z, double* kl) {
    const char* who = "po_tsne_gradient_dev";
    PO_TRY(po_check_ctx(who, ctx));
    PO_REQUIRE(n >= 1 && n < (1ull << 31), "%s: n = %llu out of range", who, (unsigned long long)n);
    PO_REQUIRE(d_rowptr != nullptr && d_y != nullptr && d_grad != nullptr && (nnz == 0 || (d_col != nullptr && d_p != nullptr)),
               "%s: NULL buffer", who);
    PO_REQUIRE(exaggeration > 0.0, "%s: exaggeration must be positive", who);
    PO_HIP(hipSetDevice(ctx->device));
    PO_TRY(tsne_pinned(ctx));
    PO_TRY(po_buf_reserve(ctx, &ctx->ws_tsne, po_tsne_grad_workspace(n) + 256));
    PO_TRY(tsne_check_csr(ctx, who, n, d_rowptr, d_col, nnz, ctx->ws_tsne.p));
    double* scal = nullptr;
    PO_TRY(po_launch_tsne_gradient(ctx, d_rowptr, d_col, d_p, d_y, n, exaggeration, ctx->ws_tsne.p, false, d_grad, nullptr, nullptr, nullptr,
                                   0.0, 0.0, 0.0, kl != nullptr, false, &scal, nullptr));
    if (z || kl) {
        PO_HIP(hipMemcpyAsync(ctx->h_tsne, scal, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipStreamSynchronize(ctx->stream));
        if (z) *z = ctx->h_tsne[0];
        if (kl) *kl = ctx->h_tsne[1];
    }
    return PO_OK;
}

// a zero in po_tsne_params selects scikit-learn's value
static int tsne_params(const char* who, uint64_t n, const po_tsne_params* params, po_tsne_params* out) {
    po_tsne_params p;
    memset(&p, 0, sizeof(p));
    if (params) p = *params;
    if (p.max_iter == 0) p.max_iter = 1000;
    if (p.exploration_iter == 0) p.exploration_iter = 250;
    if (p.n_iter_check == 0) p.n_iter_check = 50;
    if (p.n_iter_without_progress == 0) p.n_iter_without_progress = 300;
    if (p.early_exaggeration == 0.0) p.early_exaggeration = 12.0;
    if (p.min_grad_norm == 0.0) p.min_grad_norm = 1e-7;
    PO_REQUIRE(p.early_exaggeration >= 1.0, "%s: early_exaggeration %g is below 1", who, p.early_exaggeration);
    if (p.learning_rate == 0.0) {
        p.learning_rate = (double)n / p.early_exaggeration / 4.0;
        if (p.learning_rate < 50.0) p.learning_rate = 50.0;
    }
    PO_REQUIRE(p.learning_rate > 0.0 && p.min_grad_norm > 0.0, "%s: learning_rate and min_grad_norm must be positive", who);
    *out = p;
    return PO_OK;
}

// time_kernels: four events per iteration, read after the loop (no extra synchronisation inside it)
struct tsne_events {
    std::vector<hipEvent_t> ev;
    ~tsne_events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    int add4() {
        for (int q = 0; q < 4; ++q) {
            hipEvent_t e;
            PO_HIP(hipEventCreate(&e));
            ev.push_back(e);
        }
        return PO_OK;
    }
    // medians over the iterations; the rest of an iteration: start to the next start, less the two kernels
    int medians(uint32_t steps, po_tsne_result* result) const {
        std::vector<float> rep, att, rest;
        for (uint32_t i = 0; i + 1 < steps; ++i) {
            float a = 0.0f, b = 0.0f, c = 0.0f;
            PO_HIP(hipEventElapsedTime(&a, ev[4 * i], ev[4 * i + 1]));
            PO_HIP(hipEventElapsedTime(&b, ev[4 * i + 2], ev[4 * i + 3]));
            PO_HIP(hipEventElapsedTime(&c, ev[4 * i], ev[4 * i + 4]));
            rep.push_back(a);
            att.push_back(b);
            rest.push_back(c - a - b);
        }
        auto median = [](std::vector<float>& v) { std::sort(v.begin(), v.end()); return (double)v[v.size() / 2]; };
        result->repulsion_ms = median(rep);
        result->attraction_ms = median(att);
        result->rest_ms = median(rest);
        return PO_OK;
    }
};

// csr_checked: the CSR was built by po_tsne_affinities_dev in this call (po_tsne), so it is not validated again
static int tsne_run(po_ctx* ctx, const char* who, uint64_t n, const int64_t* d_rowptr, const int32_t* d_col, const float* d_p, uint64_t nnz,
                    const float* d_y0, const po_tsne_params* params, float* d_y, po_tsne_result* result, bool csr_checked) {
    PO_TRY(po_check_ctx(who, ctx));
    if (result) memset(result, 0, sizeof(*result));
    PO_REQUIRE(n >= 4 && n < (1ull << 31), "%s: n = %llu, t-SNE needs at least 4 points (and int32 indices)", who, (unsigned long long)n);
    PO_REQUIRE(d_rowptr != nullptr && d_y0 != nullptr && d_y != nullptr && (nnz == 0 || (d_col != nullptr && d_p != nullptr)),
               "%s: NULL buffer", who);
    po_tsne_params p;
    PO_TRY(tsne_params(who, n, params, &p));
    PO_HIP(hipSetDevice(ctx->device));
    PO_TRY(tsne_pinned(ctx));
    uint8_t* base = nullptr;                   // the gradient's workspace, then two embeddings, the update and the gains
    float *ybuf[2] = {nullptr, nullptr}, *upd = nullptr, *gains = nullptr;
    PO_TRY(po_stage(ctx, &ctx->ws_tsne, [&](po_carver& ws) {
        base = ws.take(po_tsne_grad_workspace(n) + 256);
        ybuf[0] = ws.array<float>(n * 2);
        ybuf[1] = ws.array<float>(n * 2);
        upd = ws.array<float>(n * 2);
        gains = ws.array<float>(n * 2);
    }));
    if (!csr_checked) PO_TRY(tsne_check_csr(ctx, who, n, d_rowptr, d_col, nnz, base));
    PO_HIP(hipMemcpyAsync(ybuf[0], d_y0, n * 2 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    PO_HIP(hipMemsetAsync(upd, 0, n * 2 * sizeof(float), ctx->stream));
    {   // gains start at 1: fill through the host staging of one float pattern
        const float one = 1.0f;
        uint32_t bits;
        memcpy(&bits, &one, 4);
        PO_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(gains), (int)bits, n * 2, ctx->stream));
    }
    // scikit-learn's two calls of _gradient_descent: `it` carries over, best_error starts afresh in the second
    int cur = 0;
    uint32_t steps = 0, checks = 0;
    double grad_norm = 0.0;
    double* scal = nullptr;
    uint32_t it = 0;
    tsne_events timing;
    for (int phase = 0; phase < 2; ++phase) {
        const uint32_t stop_at = phase == 0 ? (p.exploration_iter < p.max_iter ? p.exploration_iter : p.max_iter) : p.max_iter;
        const double exaggeration = phase == 0 ? p.early_exaggeration : 1.0, momentum = phase == 0 ? 0.5 : 0.8;
        const uint32_t patience = phase == 0 ? p.exploration_iter : p.n_iter_without_progress;
        double best = DBL_MAX;
        uint32_t best_iter = it;
        for (; it < stop_at; ++it) {
            const bool check = (it + 1) % p.n_iter_check == 0;
            hipEvent_t* ev = nullptr;
            if (p.time_kernels) {
                PO_TRY(timing.add4());
                ev = &timing.ev[timing.ev.size() - 4];
            }
            PO_TRY(po_launch_tsne_gradient(ctx, d_rowptr, d_col, d_p, ybuf[cur], n, exaggeration, base, true, nullptr, ybuf[cur ^ 1], upd, gains,
                                           momentum, p.learning_rate, 0.01, check, check, &scal, ev));
            cur ^= 1;
            ++steps;
            if (!check) continue;
            PO_HIP(hipMemcpyAsync(ctx->h_tsne, scal, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            PO_HIP(hipStreamSynchronize(ctx->stream));
            const double err = ctx->h_tsne[1];
            grad_norm = sqrt(ctx->h_tsne[2]);
            if (p.history && checks < p.history_cap) {
                p.history[3 * checks] = (double)(it + 1);
                p.history[3 * checks + 1] = err;
                p.history[3 * checks + 2] = grad_norm;
            }
            ++checks;
            PO_REQUIRE(err == err && grad_norm == grad_norm, "%s: the embedding is not finite at iteration %u (NaN in y0 or P?)", who, it + 1);
            if (err < best) {
                best = err;
                best_iter = it;
            } else if (it - best_iter > patience) {
                ++it;
                break;
            }
            if (grad_norm <= p.min_grad_norm) {
                ++it;
                break;
            }
        }
    }
    // KL, Z of the embedding that is returned (scikit-learn reports the error of the step before the last update)
    PO_TRY(po_launch_tsne_gradient(ctx, d_rowptr, d_col, d_p, ybuf[cur], n, 1.0, base, false, upd, nullptr, nullptr, nullptr, 0.0, 0.0, 0.0, true,
                                   false, &scal, nullptr));
    PO_HIP(hipMemcpyAsync(d_y, ybuf[cur], n * 2 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    PO_HIP(hipMemcpyAsync(ctx->h_tsne, scal, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    if (result) {
        result->z = ctx->h_tsne[0];
        result->kl = ctx->h_tsne[1];
        result->grad_norm = grad_norm;
        result->iterations = steps;
        result->history_len = checks;
        if (steps >= 2 && timing.ev.size() == 4 * (size_t)steps) PO_TRY(timing.medians(steps, result));
    }
    return PO_OK;
}

extern "C" int po_tsne_dev(po_ctx* ctx, uint64_t n, const int64_t* d_rowptr, const int32_t* d_col, const float* d_p, uint64_t nnz,
                           const float* d_y0, const po_tsne_params* params, float* d_y, po_tsne_result* result) {
    return tsne_run(ctx, "po_tsne_dev", n, d_rowptr, d_col, d_p, nnz, d_y0, params, d_y, result, false);
}

// The host-pointer form: the lists, the CSR and the embeddings in ws_tsne_csr, then po_tsne_affinities_dev and tsne_run.  The list
// rules are asked here first, under this entry point's name, because the staging is sized by them.
extern "C" int po_tsne(po_ctx* ctx, uint64_t n, uint32_t k, int metric, int val_dtype, const int32_t* idx, const void* val,
                       double perplexity, const float* y0, const po_tsne_params* params, float* y, po_tsne_result* result) {
    const char* who = "po_tsne";
    PO_TRY(po_check_ctx(who, ctx));
    if (result) memset(result, 0, sizeof(*result));
    PO_TRY(check_tsne_lists(who, n, k, metric, val_dtype, perplexity));
    PO_REQUIRE(idx != nullptr && val != nullptr && y0 != nullptr && y != nullptr, "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    const size_t esz = val_dtype == PO_F32 ? 4 : 8;
    const uint64_t e = n * (uint64_t)k, cap = 2 * e;
    int32_t *d_idx = nullptr, *d_col = nullptr;
    uint8_t* d_val = nullptr;
    int64_t* d_rowptr = nullptr;
    float *d_p = nullptr, *d_y0 = nullptr, *d_y = nullptr;
    PO_TRY(po_stage(ctx, &ctx->ws_tsne_csr, [&](po_carver& ws) {
        d_idx = ws.array<int32_t>(e);
        d_val = ws.take(e * esz);
        d_rowptr = ws.array<int64_t>(n + 1);
        d_col = ws.array<int32_t>(cap);
        d_p = ws.array<float>(cap);
        d_y0 = ws.array<float>(n * 2);
        d_y = ws.array<float>(n * 2);
    }));
    PO_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    PO_HIP(hipMemcpyAsync(d_idx, idx, e * 4, hipMemcpyHostToDevice, ctx->stream));
    PO_HIP(hipMemcpyAsync(d_val, val, e * esz, hipMemcpyHostToDevice, ctx->stream));
    PO_HIP(hipMemcpyAsync(d_y0, y0, n * 2 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    uint64_t nnz = 0;
    PO_TRY(po_tsne_affinities_dev(ctx, n, k, metric, val_dtype, d_idx, d_val, perplexity, nullptr, nullptr, d_rowptr, d_col, d_p, cap, &nnz));
    PO_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
    PO_TRY(tsne_run(ctx, who, n, d_rowptr, d_col, d_p, nnz, d_y0, params, d_y, result, true));
    PO_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    PO_HIP(hipMemcpyAsync(y, d_y, n * 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    if (result) {
        float ms = 0.0f;
        PO_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        result->affinities_ms = ms;
        PO_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
        result->optimise_ms = ms;
    }
    return PO_OK;
}
