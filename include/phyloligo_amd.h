/*
 * phyloligo_amd.h -- C ABI of the MI355X-native PhylOligo all-by-all contig distance path.
 *
 * The reference (itsmeludo/PhylOligo) is pure Python and has no FFI of its own; its seam for
 * this path is two dispatcher functions keyed by the `--method` string plus a metric-name
 * registry (paths relative to /root/reference/phylopackage/):
 *
 *   compute_frequencies(mthdrun, large, genome, pattern, strand, ...)   bin/phyloligo.py:980-997
 *   compute_distances(mthdrun, large, frequencies, ..., dist, ...)      bin/phyloligo.py:536-553
 *   call_dist = {"Eucl","JSD","KT","BC","SC"}                           bin/phyloligo.py:381
 *   numpy.savetxt(out_file, res, delimiter="\t")                        bin/phyloligo.py:1059-1066
 *
 * Each entry point below names the reference function(s) it replaces.  The binding a
 * PhylOligo maintainer would add (a ctypes stub selected by `--method hip`) is shown in
 * INTEGRATION.md.  Plain pointers and sizes only; no torch / numpy types cross this line.
 *
 * Conventions
 *   - every function returns PO_OK (0) or a negative po_status; po_last_error() gives the
 *     message of the calling thread's last failure;
 *   - `*_dev` entry points take DEVICE pointers and enqueue on the context's stream without
 *     synchronising (the caller owns the stream: po_ctx_set_stream / po_ctx_synchronize);
 *     the un-suffixed forms take HOST pointers, copy in, run the same kernels, copy out and
 *     return when the result is in the caller's buffer;
 *   - a profile is an exact integer count vector in the reference's word order
 *     (itertools.product("CGAT", repeat=k), bin/phyloligo.py:653: C=0,G=1,A=2,T=3, first
 *     letter most significant) plus the number of counted words of the record;
 *   - there is NO CPU fallback: without a HIP device every compute call fails with PO_ENODEV.
 */
#ifndef PHYLOLIGO_AMD_H
#define PHYLOLIGO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PO_ABI_VERSION 1

typedef struct po_ctx po_ctx;

typedef enum po_status {
    PO_OK = 0,
    PO_EINVAL = -1,       /* bad argument (unknown strand / metric / pattern, null pointer, bad range) */
    PO_ENODEV = -2,       /* no usable HIP device */
    PO_ENOMEM = -3,       /* host or device allocation failed */
    PO_EHIP = -4,         /* a HIP runtime call or kernel launch failed */
    PO_EUNSUPPORTED = -5, /* valid request outside the implemented envelope (window > 64, k > 8) */
    PO_EIO = -6,          /* file could not be opened / written, malformed FASTA */
} po_status;

/* -s/--strand choices, bin/phyloligo.py:1010 and select_strand :124-149 */
typedef enum po_strand { PO_STRAND_BOTH = 0, PO_STRAND_PLUS = 1, PO_STRAND_MINUS = 2 } po_strand;

/* -d/--distance choices, bin/phyloligo.py:1012; functions in core/phylodist.py:36-85 */
typedef enum po_metric { PO_EUCL = 0, PO_JSD = 1, PO_KT = 2, PO_BC = 3, PO_SC = 4,
                         PO_KL = 5 /* Kount.py only (po_profile_distances), bin/Kount.py:69-85 */ } po_metric;

/* element type of the distance matrix: float64 is what compute_distances_joblib returns
 * (bin/phyloligo.py:364-392); float32 is the container type of the --large memmap variant
 * (bin/phyloligo.py:413) -- values are computed in float64 and rounded once on store. */
typedef enum po_dtype { PO_F64 = 0, PO_F32 = 1 } po_dtype;

/* flags of po_pairwise* */
#define PO_FLAG_NO_SYMMETRY 1u /* compute every (i,j) independently even for the full matrix
                                  (what sklearn does for n_jobs>1); default mirrors j<i from i<j */

#define PO_FLAG_NO_TABLE_PATH 2u /* general kernels only: no integer-sum table kernel for JSD record blocks with
                                   equal word totals, no exact int8-MFMA kernel for Eucl / SC,
                                   no packed-byte SAD kernel for BC, no int8-MFMA kernel for KT, and frequency
                                   input is not traced back to integer profiles (po_pairwise_freq*: by default
                                   a matrix whose every entry is count / total bit for bit, i.e. count2freq output,
                                   is; that check reads one flag word back)                              */

#define PO_FLAG_NO_RC_FOLD 4u /* JSD / BC / KT: do not look for reverse-complement symmetric profiles.  By default
                                 the input is checked on the device (count[w] == count[rc(w)] for every record
                                 and word - what `-s both` with a palindromic pattern produces,
                                 bin/phyloligo.py:141) and, if it holds, the sums over words run over one word
                                 per {w, rc(w)} orbit: same result up to summation order, about half
                                 the work.  The check reads one flag word back, i.e. it synchronises the
                                 stream once per call; this flag avoids that.                             */

#define PO_FLAG_PAIRDOT_I8 8u /* KT (dim <= 256) and BC on thermometer planes: keep the materialised {-1,0,1} operand as
                                int8 and use v_mfma_i32_32x32x32_i8 instead of the default FP4 (E2M1) operand with
                                v_mfma_scale_f32_32x32x64_f8f6f4.  Both are exact; results are bit-identical.   */

#define PO_FLAG_NO_PAIRDOT 16u /* KT / BC: do not materialise pair-sign / thermometer operands for the matrix cores; BC then
                                 takes the packed-byte SAD kernel (equal-total blocks) and the general kernel, KT at
                                 dim <= 256 the O(D^2) vector kernel.  For cross-checks and timing comparisons.      */

/* Filled by po_pairwise* when non-NULL.  Times are HIP-event times on the context's stream;
 * asking for them makes the call synchronise. */
typedef struct po_stats {
    double prep_ms;        /* counts -> device working layout (+ per-row terms)                  */
    double kernel_ms;      /* the tile kernel(s) of the metric                                    */
    double total_ms;       /* prep + kernel + anything between                                    */
    uint64_t pairs;        /* matrix entries written / 2 (unordered pairs incl. half the diagonal) */
    uint64_t tiles;        /* workgroup tiles launched                                            */
    uint32_t kernel_id;    /* which tile kernel ran (PO_KERNEL_*)                                 */
    uint32_t rc_folded;    /* 1 if the reverse-complement folded operands were used (PO_FLAG_NO_RC_FOLD)  */
} po_stats;

#define PO_KERNEL_VALU_JSD 1u
#define PO_KERNEL_VALU_BC 2u
#define PO_KERNEL_MFMA_F64_GRAM 3u
#define PO_KERNEL_MFMA_I8_GRAM 4u  /* exact int8 kernels (counts <= 2097151, dim <= 32768; Spearman ranks, dim <= 16384), else the float64 one */
#define PO_KERNEL_VALU_KT 5u
#define PO_KERNEL_MFMA_I8_KT 8u /* Kendall tau as an exact matrix-core Gram over pair-sign vectors (FP4 / int8 operands) */
#define PO_KERNEL_MFMA_BC 9u    /* Bray-Curtis as s_a + s_b - 2 <thermometer(a), thermometer(b)> on the matrix cores   */
#define PO_KERNEL_SAD_BC 7u    /* packed-byte SAD kernel (equal-total blocks) + general kernel for the rest */
#define PO_KERNEL_LUT_JSD 6u   /* integer-sum table kernel (equal-total blocks, counts <= 255) + general kernel for the remaining tiles */

/* ---- library / context ------------------------------------------------------------------ */
const char* po_version(void);   /* "phyloligo_amd 0.1 (gfx950) src <16 hex digits>": the hash of the sources it was built from */
int po_abi_version(void);
const char* po_last_error(void);
const char* po_status_string(int status);
int po_device_count(void);                              /* 0 when no HIP device is visible      */
int po_ctx_create(po_ctx** out, int device_id);         /* one context per GPU / per process rank */
void po_ctx_destroy(po_ctx* ctx);
int po_ctx_set_stream(po_ctx* ctx, void* hip_stream);   /* hipStream_t of the caller; NULL = default */
int po_ctx_synchronize(po_ctx* ctx);
int po_ctx_device_name(po_ctx* ctx, char* buf, size_t len);
/* Frees every device workspace the context has grown (operand matrices, the materialised Kendall / Bray-Curtis
 * operand of up to 96 GB, staging of the host-pointer forms); the next call allocates again.  The reference's
 * workers hold nothing between calls (joblib processes, bin/phyloligo.py:386-390): this is the way back to that. */
int po_ctx_trim(po_ctx* ctx);

/* ---- pattern ---------------------------------------------------------------------------- *
 * `pattern` is the -p string of '1'/'0' (bin/phyloligo.py:1027); -k N is "1"*N (:1040-1041).
 * window = len(pattern) <= 64, k = number of '1' <= 8, dim = 4^k.  (The reference takes any length and any k,
 * bin/phyloligo.py:622-628; 4^9 columns and beyond are impractical anywhere, wider seeds than 64 return
 * PO_EUNSUPPORTED.)                                                                           */
int po_pattern_info(const char* pattern, uint32_t* window, uint32_t* k, uint64_t* dim);

/* ---- stage 1: profiles ------------------------------------------------------------------ *
 * Replaces compute_frequencies_joblib (bin/phyloligo.py:847-877), i.e. per record
 * select_strand (:124-149) -> upper() (:683) -> cut_sequence_and_count_pattern (:601-631) ->
 * the dense C,G,A,T ordering of count2freq (:653); the division count/total of :656 is left
 * to the consumer (po_frequencies*, po_pairwise*) so that the canonical result is exact.
 *   seq      concatenated sequence bytes of all records, in file order, line ends / blanks
 *            already removed, case preserved (any byte that is not ACGTacgt separates words)
 *   offsets  n_seqs+1 byte offsets into seq (offsets[0]=0, non-decreasing)
 *   counts   [n_seqs][dim] uint32, row major          totals  [n_seqs] uint64                 */
int po_count_profiles(po_ctx* ctx, const uint8_t* seq, const uint64_t* offsets, uint64_t n_seqs,
                      const char* pattern, int strand, uint32_t* counts, uint64_t* totals);
int po_count_profiles_dev(po_ctx* ctx, const uint8_t* d_seq, const uint64_t* d_offsets, uint64_t n_seqs,
                          uint64_t total_bytes, const char* pattern, int strand,
                          uint32_t* d_counts, uint64_t* d_totals);

/* count2freq (bin/phyloligo.py:633-661): freq[i][w] = counts[i][w] / totals[i] in float64
 * (0 for an empty record); this is the matrix -q/--outfreq writes (:1059-1061).               */
int po_frequencies(po_ctx* ctx, const uint32_t* counts, const uint64_t* totals, uint64_t n, uint32_t dim,
                   double* freq);
int po_frequencies_dev(po_ctx* ctx, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n,
                       uint32_t dim, double* d_freq);

/* ---- sliding windows against a prototype (bin/Kount.py, the ContaLocate front end) ----------- *
 * Profiles of arbitrary, possibly overlapping byte ranges [begins[i], ends[i]) of one sequence buffer:
 * the windows that make_genome_chunk cuts (bin/Kount.py:343-407), each counted exactly like a record
 * (cut_sequence_and_count_pattern with the strand handling inside, bin/Kount.py:208-243).
 * sum_lengths (device form) is an upper bound of sum(ends[i]-begins[i]).                          */
int po_count_profiles_ranges(po_ctx* ctx, const uint8_t* seq, uint64_t total_bytes, const uint64_t* begins,
                             const uint64_t* ends, uint64_t n_ranges, const char* pattern, int strand,
                             uint32_t* counts, uint64_t* totals);
int po_count_profiles_ranges_dev(po_ctx* ctx, const uint8_t* d_seq, uint64_t total_bytes, const uint64_t* d_begins,
                                 const uint64_t* d_ends, uint64_t n_ranges, uint64_t sum_lengths, const char* pattern,
                                 int strand, uint32_t* d_counts, uint64_t* d_totals);
/* Distance of every profile to ONE prototype frequency vector proto[dim] (compute_distance_joblib,
 * bin/Kount.py:322-330): PO_JSD / PO_EUCL / PO_KL of bin/Kount.py:69-123 WITHOUT their x1000 display
 * scaling (the host mirror applies it).  out[n] float64.                                           */
int po_profile_distances(po_ctx* ctx, const uint32_t* counts, const uint64_t* totals, uint64_t n, uint32_t dim,
                         const double* proto, int metric, double* out);
int po_profile_distances_dev(po_ctx* ctx, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n,
                             uint32_t dim, const double* d_proto, int metric, double* d_out);
/* Occurrences of one byte value in every range - the numerator of Kount.py's N gate, seq.count("N") / len(seq)
 * (bin/Kount.py:295), for the same windows, without a pass over the genome on the host.  Device pointers.       */
int po_count_byte_ranges_dev(po_ctx* ctx, const uint8_t* d_seq, uint64_t total_bytes, const uint64_t* d_begins,
                             const uint64_t* d_ends, uint64_t n_ranges, int byte, uint64_t* d_out);

/* ---- stage 2: pairwise matrix ----------------------------------------------------------- *
 * Replaces compute_distances_joblib (bin/phyloligo.py:364-392) = sklearn pairwise_distances
 * over phylodist.Eucl / JSD / KT / SC (core/phylodist.py:36-85) and SciPy 'braycurtis'.
 * Computes rows [row_begin,row_end) x all n columns:
 *     out[(i-row_begin)*ld_out + j]   0 <= j < n,   ld_out >= n  (elements, not bytes)
 * Diagonal as the reference produces it: Eucl/JSD/BC/SC 0, KT 1 (0 for a constant row).
 * Row blocks are independent, which is how the matrix shards over GPUs (one context each).
 * Layout of a DEVICE result and speed: any ld_out >= n is correct.  Rows that start on 16-byte boundaries (d_out 16-byte aligned and
 * ld_out a multiple of 4 float32 / 2 float64 entries) leave as 16-byte stores; rows on whole 128-byte lines (ld_out a multiple of 32
 * float32 / 16 float64 entries) are written ~25 % faster still, and an odd float32 leading dimension costs about 2 x (every 512-byte
 * row piece of a tile then begins and ends inside a 32-byte sector that a neighbouring tile also writes).  The host-pointer forms
 * below keep their device copy of the result on 128-byte rows whatever n is.  The metric of the largest matrices here, Eucl on the
 * exact int8 path, makes ONE host synchronisation per call from 8 192 records on (it reads 4 bytes per 128 records back to deal the
 * tiles to the kernels of their class); JSD and BC make one for the fold decision, as before.                                        */
int po_pairwise(po_ctx* ctx, const uint32_t* counts, const uint64_t* totals, uint64_t n, uint32_t dim,
                int metric, uint64_t row_begin, uint64_t row_end, int out_dtype, void* out, uint64_t ld_out,
                uint32_t flags, po_stats* stats);
int po_pairwise_dev(po_ctx* ctx, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n, uint32_t dim,
                    int metric, uint64_t row_begin, uint64_t row_end, int out_dtype, void* d_out,
                    uint64_t ld_out, uint32_t flags, po_stats* stats);

/* The same from a float64 frequency matrix freq[n][dim] (row major) -- literally the
 * `frequencies` argument of compute_distances / compute_distances_joblib
 * (bin/phyloligo.py:536-553, :364-392), for callers that hold frequencies rather than counts. */
int po_pairwise_freq(po_ctx* ctx, const double* freq, uint64_t n, uint32_t dim, int metric, uint64_t row_begin,
                     uint64_t row_end, int out_dtype, void* out, uint64_t ld_out, uint32_t flags, po_stats* stats);
int po_pairwise_freq_dev(po_ctx* ctx, const double* d_freq, uint64_t n, uint32_t dim, int metric,
                         uint64_t row_begin, uint64_t row_end, int out_dtype, void* d_out, uint64_t ld_out,
                         uint32_t flags, po_stats* stats);

/* Several rectangular blocks of one matrix in one call (the per-rank work list of a multi-GPU run):
 * the working layout is prepared once, then every block is launched.
 *   out[(i-row_begin)*ld_out + (j-col_begin)]                      row_begin <= i < row_end, col_begin <= j < col_end
 *   mirror[(j-col_begin)*ld_mirror + (i-row_begin)]  (if not NULL)  the transposed block, same values
 * triangular != 0 requires rows == columns: only pairs i <= j are evaluated and the lower half is
 * filled by symmetry inside `out` (mirror / ld_mirror are ignored).                                    */
typedef struct po_block {
    uint64_t row_begin, row_end, col_begin, col_end;
    void* out;
    uint64_t ld_out;
    void* mirror;
    uint64_t ld_mirror;
    uint32_t triangular;
    uint32_t reserved;
} po_block;
int po_pairwise_blocks_dev(po_ctx* ctx, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n, uint32_t dim,
                           int metric, int out_dtype, const po_block* blocks, uint32_t n_blocks, uint32_t flags,
                           po_stats* stats);

/* ---- k nearest neighbours: a sparse graph instead of the dense matrix ------------------------------------------------ *
 * The reference hands the whole matrix to its next step (phyloselect.py reads it with numpy.loadtxt / a memmap and gives it to
 * t-SNE with metric="precomputed", which only looks at the 3 perplexity + 1 nearest neighbours of each point; HDBSCAN's core
 * distance is one neighbour).  These entry points select, for every record i of the n given, its k_eff = min(k, n - 1) nearest
 * records j != i from the matrix po_pairwise_dev computes for the same input, metric and out dtype (val_dtype): v[i][j] below is
 * bit for bit that matrix's (i, j) entry.  The matrix is evaluated panel by panel on the device and never leaves it whole.
 *   idx int32 [n][k_eff]   val [n][k_eff] (float64 / float32)      row i in this order:
 *     ascending v (PO_KT: descending, Kendall's tau is a similarity), NaN after every number, equal values by the smaller j
 *   i.e. numpy.argsort(key, kind="stable")[:k_eff] over row i without its diagonal, key = v (-v for KT), NaN last.
 * k: 1 .. 1024 (else PO_EINVAL); n <= 1 gives an empty result.  panel_rows: rows per panel, a multiple of 128 (0 = the slab and
 * mirror of a panel near 256 MiB); the result does not depend on it.  The panel workspace is held by the context (po_ctx_trim).
 * flags: those of po_pairwise* (PO_FLAG_NO_SYMMETRY is ignored: every pair is evaluated once, as in the dense symmetric path).
 * stats: prep_ms and total_ms as po_pairwise*; kernel_ms is the tile kernels alone, the selection is total - prep - kernel.  */
#define PO_KNN_MAX_K 1024u
int po_knn(po_ctx* ctx, const uint32_t* counts, const uint64_t* totals, uint64_t n, uint32_t dim, int metric, uint32_t k,
           int val_dtype, uint64_t panel_rows, int32_t* idx, void* val, uint32_t flags, po_stats* stats);
int po_knn_dev(po_ctx* ctx, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n, uint32_t dim, int metric, uint32_t k,
               int val_dtype, uint64_t panel_rows, int32_t* d_idx, void* d_val, uint32_t flags, po_stats* stats);
/* The same over a work list of blocks of the matrix (a rank's share, as a multi-GPU plan deals it; out / mirror / ld_* of the
 * blocks are ignored, row_begin / col_begin must be multiples of 128): a triangular block feeds both directions within itself,
 * a rectangular block (rows and columns disjoint) feeds its rows, and its columns through the transposed copy.  The lists
 * [n][k_eff] cover all n rows and are emptied first (idx -1 = unused entry): they are partial when the blocks do not cover the
 * matrix, and po_knn_merge_dev combines the partial lists of several work lists.                                            */
int po_knn_blocks_dev(po_ctx* ctx, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n, uint32_t dim, int metric,
                      uint32_t k, int val_dtype, uint64_t panel_rows, const po_block* blocks, uint32_t n_blocks, int32_t* d_idx,
                      void* d_val, uint32_t flags, po_stats* stats);
/* m lists of shape [n][k] (idx_in / val_in: [m][n][k], each ordered as above, from disjoint pairs) -> one list [n][k] of the
 * best k of each row, same order.  The reduction of a multi-rank k-NN run; metric gives the direction (PO_KT descending).     */
int po_knn_merge_dev(po_ctx* ctx, uint64_t n, uint32_t k, int metric, int val_dtype, const int32_t* d_idx_in, const void* d_val_in,
                     uint32_t m, int32_t* d_idx, void* d_val);

/* ---- t-SNE of the k-NN graph: the 2-D map phyloselect.py clusters on ------------------------------------------------------ *
 * Replaces transform_matrix_tsne (bin/phyloselect.py:381-398): sklearn.manifold.TSNE(n_components=2, random_state=0,
 * perplexity=p, metric="precomputed") on the distance matrix.  t-SNE looks at the K = min(n - 1, int(3 p + 1)) nearest
 * neighbours of every point only, so the lists of po_knn* are its whole input and the matrix never exists.  scikit-learn's
 * algorithm (1.7: manifold/_t_sne.py, _utils.pyx) step for step, except that the repulsive force is summed exactly over all
 * pairs (method="barnes_hut" with angle=0.0) and that init is "random".  Three steps, each an entry point of its own.
 * The same inputs give the same bytes on every call.  The un-suffixed form takes host pointers.
 *
 * 1. po_tsne_affinities_dev: lists idx int32 [n][k] / val [n][k] (val_dtype; distances, squared here) -> per row the precision
 *    beta [n] (float64, may be NULL) found by scikit-learn's binary search, the conditional probabilities cond float64 [n][k]
 *    (may be NULL), and the joint probabilities P = (C + C^T) / sum(C + C^T) as CSR: rowptr int64 [n + 1], col int32 and
 *    p float32 [*nnz], columns ascending in every row.  cap: entries col / p can hold; 2 n k is always enough, less gives
 *    PO_EINVAL with the number needed in *nnz.  Synchronises the stream (validation and nnz are read back).
 *    PO_EINVAL: perplexity < 1 or int(3 perplexity + 1) > PO_KNN_MAX_K; n < 4; k != min(n - 1, int(3 perplexity + 1));
 *    metric PO_KT (a similarity, ordered descending); a NaN or negative value, or a neighbour index outside 0..n-1 or equal
 *    to its row, or a neighbour listed twice in a row - checked on the device, the message names the first offending row.
 * 2. po_tsne_gradient_dev: CSR P, embedding y float32 [n][2], exaggeration -> grad float32 [n][2] of the KL divergence
 *    between exaggeration * P and Q, *z = sum over i != j of 1 / (1 + |y_i - y_j|^2) and *kl (host doubles, any may be NULL).
 *    The CSR indexes y, so its row pointers and columns are checked on the device first (PO_EINVAL names the first bad row):
 *    every call synchronises the stream once for that, and once more when z or kl is asked for.
 * 3. po_tsne_dev: CSR P and the start y0 float32 [n][2] -> the embedding y float32 [n][2] after scikit-learn's
 *    _gradient_descent.  A zero in po_tsne_params selects scikit-learn's value.  The CSR is checked as in 2. (one synchronisation
 *    before the loop; po_tsne, which has just built it, skips that).  Every n_iter_check iterations KL and the gradient norm
 *    are read back (the loop's only synchronisation).  Returns when y is complete.                        */
typedef struct po_tsne_params {
    uint32_t max_iter;                 /* 0: 1000 */
    uint32_t exploration_iter;         /* 0: 250 iterations with early_exaggeration and momentum 0.5, then 1 and 0.8 */
    uint32_t n_iter_check;             /* 0: 50 */
    uint32_t n_iter_without_progress;  /* 0: 300 */
    double early_exaggeration;         /* 0: 12 */
    double learning_rate;              /* 0: max(n / early_exaggeration / 4, 50) */
    double min_grad_norm;              /* 0: 1e-7 */
    double* history;                   /* host, may be NULL: per check (iteration, KL, gradient norm), history_cap triples */
    uint32_t history_cap;
    uint32_t time_kernels;             /* != 0: device events around the kernels of every iteration (po_tsne_result *_ms below) */
} po_tsne_params;
typedef struct po_tsne_result {
    double kl;                         /* KL divergence of the returned embedding (exaggeration 1) */
    double grad_norm;                  /* gradient norm at the last check (0 if there was none) */
    double z;                          /* sum of q over all pairs of the returned embedding */
    uint32_t iterations;               /* update steps made */
    uint32_t history_len;              /* checks made (entries written to history: min(history_len, history_cap)) */
    double affinities_ms, optimise_ms; /* po_tsne only: HIP-event times of the two parts */
    double repulsion_ms, attraction_ms, rest_ms; /* time_kernels: median per iteration of the repulsion kernel, of the attraction +
                                          update kernel, and of the rest of an iteration (Z reduction, gaps between launches) */
} po_tsne_result;
int po_tsne_affinities_dev(po_ctx* ctx, uint64_t n, uint32_t k, int metric, int val_dtype, const int32_t* d_idx, const void* d_val,
                           double perplexity, double* d_beta, double* d_cond, int64_t* d_rowptr, int32_t* d_col, float* d_p,
                           uint64_t cap, uint64_t* nnz);
int po_tsne_gradient_dev(po_ctx* ctx, uint64_t n, const int64_t* d_rowptr, const int32_t* d_col, const float* d_p, uint64_t nnz,
                         const float* d_y, double exaggeration, float* d_grad, double* z, double* kl);
int po_tsne_dev(po_ctx* ctx, uint64_t n, const int64_t* d_rowptr, const int32_t* d_col, const float* d_p, uint64_t nnz,
                const float* d_y0, const po_tsne_params* params, float* d_y, po_tsne_result* result);
int po_tsne(po_ctx* ctx, uint64_t n, uint32_t k, int metric, int val_dtype, const int32_t* idx, const void* val, double perplexity,
            const float* y0, const po_tsne_params* params, float* y, po_tsne_result* result);

/* ---- k-medoids on the distance matrix: the clusters phyloselect.py writes out ------------------------------------------------ *
 * Replaces the KMedoids class the reference ships (bin/phyloselect.py:37-309) as phyloselect.py calls it:
 * KMedoids(n_clusters, distance_metric="precomputed").fit(matrix) on the whole matrix (:578-595, :647).  Decision for decision:
 *   start    init_medoids == NULL: init="heuristic" (_get_initial_medoid_indices, :298-302) - the n_clusters rows with the smallest
 *            row sums, ascending, ties to the smaller row.  Else n_clusters distinct rows, a HOST array in both forms (init="random",
 *            :293-296, is RandomState(seed).permutation(n)[:n_clusters] computed by the caller).
 *   assign   label[j] = argmin_c matrix[medoid[c]][j], the smaller c wins a tie (_get_cluster_ics, :190-198)
 *   update   per cluster, against those labels: the member with the smallest sum over the members (ties: the smaller row) replaces
 *            the medoid if that sum is strictly below the medoid's own; an empty cluster keeps its medoid
 *            (_update_medoid_ics_in_place, :200-240)
 *   loop     until no medoid changed or max_iter passes ran (fit, :143-168; the reference's default is 300).  labels are those of
 *            the LAST assignment: when max_iter ends the loop they do not reflect the last update, as in the reference.
 * matrix: [n][n] float32 / float64 (dtype), row major, leading dimension ld >= n elements; read by rows, never written.  Every sum
 * accumulates in float64 whatever dtype is, and a row's sum depends on the row, the labels and n alone (fixed order, no
 * floating-point atomics): the same input gives the same bytes.  Rows on 16-byte boundaries (pointer and ld) are read with 16-byte
 * loads, any other layout element by element with the same result.  The host reads back one flag word per iteration; with the
 * heuristic start also the n row sums, once.  PO_EINVAL: n_clusters < 1 or > n, max_iter < 1, ld < n, an init row outside 0..n-1
 * or given twice, and - heuristic start only - a row whose sum is NaN (Bray-Curtis gives 0/0 for two empty records); the message
 * names the first such row.  With init_medoids the result for a matrix that holds NaN is unspecified (a NaN never wins the
 * assignment, and sorts after every number in the update).
 *   d_labels int32 [n], d_medoids int32 [n_clusters]     result (may be NULL; asking for it adds one small kernel and device events) */
typedef struct po_kmedoids_result {
    uint32_t iterations;       /* assignment passes made (the reference's n_iter_) */
    uint32_t converged;        /* 1: the last update changed no medoid; 0: max_iter ended the loop */
    uint32_t empty_clusters;   /* clusters without a member in the returned labels */
    uint32_t reserved;
    double inertia;            /* sum over j of matrix[medoid[label[j]]][j] for the returned labels and medoids */
    double start_ms;           /* HIP-event times: the start (row sums + selection on the host) ... */
    double rowsum_ms, assign_ms, update_ms;   /* ... and, summed over the iterations, the three steps of an iteration */
} po_kmedoids_result;
int po_kmedoids_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, uint32_t n_clusters,
                    const int32_t* init_medoids, uint32_t max_iter, int32_t* d_labels, int32_t* d_medoids, po_kmedoids_result* result);
/* Host pointers: the matrix is copied to the device (PO_ENOMEM, with the size in the message, when it does not fit). */
int po_kmedoids(po_ctx* ctx, const void* matrix, int dtype, uint64_t n, uint64_t ld, uint32_t n_clusters, const int32_t* init_medoids,
                uint32_t max_iter, int32_t* labels, int32_t* medoids, po_kmedoids_result* result);
/* The two pieces the loop is made of.  Costs: d_costs[t] = sum over j with d_labels[j] == d_labels[r] of matrix[r][j], float64, for
 * r = d_rows[t], t < n_rows - or for every row r = t < n when d_rows is NULL (n_rows 0 or n): numpy.sum(D_in, axis=1) of :218-223 for
 * all clusters at once.  The bytes of a row's cost do not depend on which other rows are asked for.  Labels are any int32.
 * Assign: d_labels [n] for the medoids d_medoids [n_clusters] (device; rows of the matrix, checked: PO_EINVAL names the first
 * outside 0..n-1).  Both synchronise the stream once when they check a device index list.                                     */
int po_kmedoids_costs_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, const int32_t* d_labels,
                          const int32_t* d_rows, uint64_t n_rows, double* d_costs);
int po_kmedoids_assign_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, uint32_t n_clusters,
                           const int32_t* d_medoids, int32_t* d_labels);

/* ---- silhouettes of a clustering of the distance matrix: is K a good choice, which records sit between two clusters ------------ *
 * What sklearn.metrics.silhouette_samples(matrix, labels, metric="precomputed") computes, the score the scikit-learn stack under
 * phyloselect.py offers for the question its --interactive loop ("perform an other run? ... change nbk") leaves to the user's eye.
 * matrix: as for k-medoids ([n][n] float32 / float64, ld >= n elements, read by rows, never written); the diagonal is expected to
 * be 0.  d_labels: int32 [n], every value in 0 .. n_clusters-1 (checked on the device: PO_EINVAL names the first position outside).
 *   sizes[c]   the number of columns with label c
 *   S[i][c]    the float64 sum of matrix[i][j] over the columns j with label c: every entry widened to float64 before it is added,
 *              the row taken as stored (matrix[i][i] included, as scikit-learn includes it), an entry of another cluster replaced by
 *              +0 with a select and never multiplied, so a NaN outside a cluster stays outside it.  Summed in the order of the
 *              k-medoids row sums: S[i][d_labels[i]] has the bytes po_kmedoids_costs_dev gives for row i, and the bytes of S[i][c]
 *              depend on row i, the labels and n alone - not on n_clusters, ld, the alignment or the other rows.
 *   s[i]       with own = d_labels[i]: 0 when sizes[own] == 1; otherwise a = S[i][own] / (sizes[own] - 1), b = the smallest
 *              S[i][c] / sizes[c] over c != own with sizes[c] > 0, m = max(a, b), s = (b - a) / m, or 0 when m == 0 (duplicate
 *              records; scikit-learn's nan_to_num of 0 / 0 gives 0 too).
 *   NaN        if S[i][c] of any non-empty cluster is NaN, s[i] is NaN (a cluster of one included) and so is the mean.  scikit-learn
 *              prints 0 there; a silent 0 for a record whose distance is undefined is worse than NaN.
 *   empty      clusters without a member (k-medoids can return them) are skipped; fewer than two non-empty clusters: PO_EINVAL
 *              (scikit-learn raises).
 *   mean       (sum of s[i]) / n, a float64 sum with a fixed reduction tree.  No floating-point atomics anywhere.
 * The clusters are handled PO_SILHOUETTE_CHUNK at a time: n_clusters <= PO_SILHOUETTE_CHUNK reads the matrix once, a larger
 * n_clusters ceil(n_clusters / PO_SILHOUETTE_CHUNK) times; the n x n_clusters sums are never stored by po_silhouette* (workspace:
 * n x PO_SILHOUETTE_CHUNK doubles, held by the context).  Every entry point synchronises the stream once, for the label check.
 * po_cluster_sums_dev: d_sums [n][n_clusters] = S, for any 1 <= n_clusters <= n (no rule about empty clusters applies).
 *   d_values float64 [n] = s     result (may be NULL; asking for it adds device events and one more synchronisation per pass)    */
#define PO_SILHOUETTE_CHUNK 16
int po_cluster_sums_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, const int32_t* d_labels,
                        uint32_t n_clusters, double* d_sums);
typedef struct po_silhouette_result {
    double mean;                   /* (sum of the n values) / n */
    uint32_t nonempty_clusters;    /* clusters with at least one member */
    uint32_t passes;               /* matrix reads made: ceil(n_clusters / PO_SILHOUETTE_CHUNK) */
    double sums_ms, finish_ms;     /* HIP-event times: the passes over the matrix; everything else (histogram, folds, the values) */
} po_silhouette_result;
int po_silhouette_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, const int32_t* d_labels, uint32_t n_clusters,
                      double* d_values, po_silhouette_result* result);
/* Host pointers: the matrix is copied to the device (PO_ENOMEM, with the size in the message, when it does not fit). */
int po_silhouette(po_ctx* ctx, const void* matrix, int dtype, uint64_t n, uint64_t ld, const int32_t* labels, uint32_t n_clusters,
                  double* values, po_silhouette_result* result);

/* ---- DBSCAN on the distance matrix: clusters by density, and a label for the records that belong to none ----------------------- *
 * The labels_ and core_sample_indices_ of sklearn.cluster.DBSCAN(eps, min_samples, metric="precomputed").fit(matrix), numbering and
 * border ties included, stated without a visiting order.  The label -1, "no cluster", is what the reference's recommended run
 * (phyloselect.py -m hdbscan) sends to data_fasta_unclust.fa (bin/phyloselect.py:565-570) and k-medoids cannot give.
 * matrix: as for k-medoids ([n][n] float32 / float64, ld >= n elements, read by rows, never written); expected to be symmetric,
 * which is not checked - the result for an asymmetric matrix is unspecified.  Every entry counts as its float64 value.
 *   neighbours   j is a neighbour of i iff matrix[i][j] <= eps.  The diagonal is taken as stored: a record counts itself through its
 *                0.  A NaN is never <= eps: a record with an undefined distance is nobody's neighbour (scikit-learn raises).
 *   degree[i]    the number of neighbours of row i (po_eps_degrees_dev gives just these)
 *   core[i]      degree[i] >= min_samples
 *   components   two core records are in one component iff a chain of core records joins them, each link <= eps; a component's
 *                root is its smallest core index
 *   ids          0, 1, ... in ascending order of the root (scikit-learn opens clusters in index order of their first core record)
 *   labels       a core record: its component's id.  Any other record with a core neighbour (a border record): the smallest id
 *                among its core neighbours' clusters (the first cluster opened that reaches it).  Any other record: -1, noise.
 * Integer counts and integer minima only: no order of execution changes a result, and the same input gives the same bytes.
 * The components come from rounds of: the smallest label within eps of every core row (one read of those rows), hooking of each
 * tree's root onto the smallest label its members saw, pointer jumping; the host reads one flag word per round and the loop ends
 * with the round that changes nothing (a chain of 4 096 records takes about ten).  Workspace: 5 n integers held by the context.
 * PO_EINVAL: eps negative or NaN (+inf is allowed: every entry that is not NaN is then a neighbour), min_samples < 1, ld < n,
 * n > 2^31 - 1, a dtype other than PO_F32 / PO_F64.  n == 0: nothing is done.  po_eps_degrees_dev works on the context's stream
 * without synchronising it.
 *   d_degree int32 [n]    d_labels int32 [n]    d_core uint8 [n], 1 = core (may be NULL)
 *   result (may be NULL; asking for it adds device events and one more synchronisation)                                           */
typedef struct po_dbscan_result {
    uint32_t clusters, core, border, noise;   /* core + border + noise = n */
    uint32_t passes;           /* propagation rounds, the one that changed nothing included (not the degree pass, not the border pass) */
    uint32_t reserved;
    double degree_ms;          /* HIP-event times: the degree pass and the split into core and other rows ... */
    double label_ms;           /* ... the rounds, plus the pass over the rows that are not core ... */
    double finish_ms;          /* ... the ids, the labels and the counts */
} po_dbscan_result;
int po_eps_degrees_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, double eps, int32_t* d_degree);
int po_dbscan_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t n, uint64_t ld, double eps, int64_t min_samples,
                  int32_t* d_labels, uint8_t* d_core, po_dbscan_result* result);
/* Host pointers: the matrix is copied to the device (PO_ENOMEM, with the size in the message, when it does not fit). */
int po_dbscan(po_ctx* ctx, const void* matrix, int dtype, uint64_t n, uint64_t ld, double eps, int64_t min_samples, int32_t* labels,
              uint8_t* core, po_dbscan_result* result);

/* ---- row medians of a matrix in HBM ---------------------------------------------------------- *
 * d_out[i] = median of row i of d_matrix [rows][n] (float32 / float64, row major, leading dimension ld >= n elements; read,
 * never written), over all n columns - the diagonal of a distance matrix included: R's apply(dist_matrix, 1, median), the first
 * step of the reference's outlier clip (bin/phyloselect.R:339-357).  The values are widened to float64 and ordered as numbers
 * (-0 = +0); lo is the value at rank (n-1)/2, hi the value at rank n/2 (0-based); the median is lo for odd n and (lo + hi) * 0.5
 * for even n: numpy.median(m.astype(float64), axis=1).  A row that holds a NaN gives NaN; +-inf are ordinary values.  The result
 * is exact (an element of the row or the mean of two), so it depends on nothing but the row: not on ld, the alignment (rows on
 * 16-byte boundaries are read with 16-byte loads, any other layout element by element) or the launch.  Works on the context's
 * stream without synchronising it.  rows == 0 or n == 0: nothing is done.  PO_EINVAL: n > 2^31 - 1, ld < n, a dtype other than
 * PO_F32 / PO_F64.
 * po_row_medians_passes: how many times the last po_row_medians_dev call of this context read a row from memory, summed over
 * its rows (the selection re-reads a row once per radix digit it needs; passes / rows is the bytes read per matrix byte).
 * Synchronises the stream.                                                                                                  */
int po_row_medians_dev(po_ctx* ctx, const void* d_matrix, int dtype, uint64_t rows, uint64_t n, uint64_t ld, double* d_out);
int po_row_medians_passes(po_ctx* ctx, uint64_t* passes);

/* bytes of device workspace po_pairwise_dev will hold for this problem (allocated lazily on
 * first use and kept by the context; call once before timing to keep hipMalloc out of it)    */
int po_pairwise_reserve(po_ctx* ctx, uint64_t n, uint32_t dim, int metric);

/* ---- host-side formats either side of the path ------------------------------------------ *
 * FASTA ingest with the semantics of Bio.SeqIO.parse(genome, "fasta") as used at
 * bin/phyloligo.py:869: '>' at line start opens a record, sequence lines are right-stripped
 * and joined, ' ' and '\r' removed.  Two calls: sizes first, then fill.                      */
int po_fasta_scan(const uint8_t* data, uint64_t len, uint64_t* n_records, uint64_t* seq_bytes);
int po_fasta_extract(const uint8_t* data, uint64_t len, uint8_t* seq_out, uint64_t* offsets_out,
                     uint64_t* title_begin, uint64_t* title_end);

/* ---- FASTA ingest on the device ------------------------------------------------------------ *
 * The same records as po_fasta_scan / po_fasta_extract, from the raw file bytes already in HBM (16-byte aligned
 * buffer): what Bio.SeqIO.parse(genome, "fasta") yields at bin/phyloligo.py:869, without a pass over the file on
 * the host.  po_fasta_scan_dev sizes the outputs (it synchronises the stream once) and must precede
 * po_fasta_extract_dev on the same buffer.  Title spans [title_begin, title_end) end at the line end: strip trailing
 * white space when decoding a title.  Returns PO_EIO for text before the first record, PO_EUNSUPPORTED for a tab /
 * vertical tab / form feed on a sequence line (rstrip() semantics that need the host parser).                   */
int po_file_read(const char* path, uint8_t* buf, uint64_t len);   /* first len bytes of a file, read in parallel (host) */
int po_fasta_scan_dev(po_ctx* ctx, const uint8_t* d_data, uint64_t len, uint64_t* n_records, uint64_t* seq_bytes);
int po_fasta_extract_dev(po_ctx* ctx, const uint8_t* d_data, uint64_t len, uint8_t* d_seq, uint64_t* d_offsets,
                         uint64_t* d_title_begin, uint64_t* d_title_end);

/* numpy.savetxt(path, m, delimiter="\t") of bin/phyloligo.py:1061,1066: "%.18e" values, '\t'
 * between columns, '\n' after each row, "nan"/"inf" spelled as numpy spells them.  A regular file that exists is
 * overwritten in place and cut to the new length at the end (append = 1: continued at its end); the rows are formatted and
 * written by the host threads the job may use.  Any other kind of file (pipe, /dev/null) gets the bytes in order.          */
int po_write_mat_text(const double* m, uint64_t rows, uint64_t cols, uint64_t ld, const char* path, int append);

/* The write side of the raw float32 container of `--large memmap` (bin/phyloligo.py:394-427: row slices assigned into a
 * numpy.memmap of the output file, :200-217; read back by phyloligo_comparemat.py:16-24 and phyloselect.py:606-614):
 * `rows` pieces of row_bytes bytes, piece r taken from src + r * src_pitch, go to byte offset file_offset + r * file_pitch
 * of the OPEN file descriptor fd through up to `threads` parallel pwrite(2) callers (<= 0: 8; never more than the CPUs the
 * job may use).  Whole rows of the matrix (row_bytes == src_pitch == file_pitch) are written as one contiguous range; a
 * rectangular block of a multi-GPU work list (some columns of some rows) is one pwrite per row.  Host only: no po_ctx, no
 * GPU.  Several processes may write disjoint ranges of one file at once.  Returns PO_EIO with the errno text on failure. */
int po_pwrite_rows(int fd, const void* src, uint64_t rows, uint64_t row_bytes, uint64_t src_pitch,
                   uint64_t file_offset, uint64_t file_pitch, int threads);

#ifdef __cplusplus
}
#endif
#endif /* PHYLOLIGO_AMD_H */
