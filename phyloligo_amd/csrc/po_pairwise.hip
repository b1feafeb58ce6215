// Stage 2 of the C ABI (po_pairwise*, include/phyloligo_amd.h): one call is checked (check_blocks), prepared once into a
// po_pairwise_plan (prepare: a shared front, then one function per metric) and launched block by block (launch_block: one
// function per metric).  The plan lives for the call only.  po_pairwise_run is the driver; the k-NN drivers (po_knn.hip) run
// their panels through it.
#include "po_internal.h"
#include "po_host.h"

#include <sys/mman.h>

// with_operand: also reserve the materialised Kendall pair-sign operand (up to 96 GB, FP4, folded layout).  Only
// po_pairwise_reserve asks for that - it cannot know the flags of the calls to come; a compute call reserves exactly what its
// own path uses inside po_launch_kt_pairdot_prep (PO_FLAG_NO_PAIRDOT / NO_TABLE_PATH / int8 operands / the panel kernel never
// touch this buffer, and must not fail with PO_ENOMEM because of it).  A failed reservation of the operand is not an error
// here either: the call that needs it falls back to the panel kernel.
static int reserve_pairwise(po_ctx* ctx, uint64_t n, uint32_t dim, int metric, bool with_operand) {
    const uint64_t npad = po_round_up(n ? n : 1, PO_PAD_ROWS);
    PO_TRY(po_buf_reserve(ctx, &ctx->ws_rowstat, 4 * npad * sizeof(double)));
    if (metric != PO_KT) {
        PO_TRY(po_buf_reserve(ctx, &ctx->ws_freq, po_round_up(dim, 8) * npad * sizeof(double)));
    } else {
        PO_TRY(po_buf_reserve(ctx, &ctx->ws_aux, n * (uint64_t)dim * sizeof(uint32_t)));
        size_t kt_ws = 0;
        if (po_kt_pairdot_supported(dim)) kt_ws = po_kt_pairdot_rank_bytes(n, dim);          // ranks of the pair-dot path
        if (po_kt_panel_supported(dim) && po_kt_panel_workspace(n, dim) > kt_ws) kt_ws = po_kt_panel_workspace(n, dim);
        if (kt_ws) PO_TRY(po_buf_reserve(ctx, &ctx->ws_freq, kt_ws));
        // the materialised pair-sign operand: sized for the reverse-complement folded layout when the word space is 4^k
        // (what `-s both` gives), else for all words; a call that needs more grows it lazily
        if (with_operand && po_kt_pairdot_supported(dim)) {
            const uint32_t selfs = po_fold_selfs(dim);
            const bool fold = selfs != 0xFFFFFFFFu;
            const size_t opb = po_kt_pairdot_operand_bytes(n, dim, fold ? selfs + (dim - selfs) / 2 : dim, fold ? selfs : 0, fold, 1);
            if (opb <= PO_PAIRDOT_MAX_OPERAND) (void)po_buf_reserve(ctx, &ctx->ws_pairdot, opb);
        }
    }
    // the pair-dot operand of an earlier Kendall / Bray-Curtis call (up to 96 GB) is dead weight for the other metrics
    if (metric != PO_KT && metric != PO_BC && ctx->ws_pairdot.cap > (1ull << 30)) {
        PO_HIP(hipStreamSynchronize(ctx->stream));
        po_buf_free(&ctx->ws_pairdot);
    }
    if (metric == PO_JSD) {
        PO_TRY(po_logtab_init(ctx));
        PO_TRY(po_buf_reserve(ctx, &ctx->ws_aux, po_jsd_lut_workspace(n, dim)));
    }
    if (metric == PO_EUCL || (metric == PO_SC && po_gram_i8_sc_supported(dim)))
        PO_TRY(po_buf_reserve(ctx, &ctx->ws_aux, po_gram_i8_workspace(n, dim)));
    if (metric == PO_BC) PO_TRY(po_buf_reserve(ctx, &ctx->ws_aux, po_bc_sad_workspace(n, dim)));
    return PO_OK;
}

extern "C" int po_pairwise_reserve(po_ctx* ctx, uint64_t n, uint32_t dim, int metric) {
    PO_TRY(po_check_ctx("po_pairwise_reserve", ctx));
    PO_TRY(po_check_metric(metric));
    PO_HIP(hipSetDevice(ctx->device));
    return reserve_pairwise(ctx, n, dim, metric, true);
}

// ---- the plan: what prepare leaves for launch_block -------------------------------------------------------------------------
// One part per metric, holding what that metric's launch function reads.
struct plan_eucl {
    const uint32_t* i8flag;     // device word with the largest count: the int8 kernels are candidates (NULL: float64 only)
    const uint32_t* i8_hmax;    // host copy of the largest counts per 128-record block (n >= 8192), else NULL
    uint32_t i8_upto;           // largest count the int8 kernels take
    bool i8_only;               // decided on the host: the float64 operand, norms and kernel are not needed
};
struct plan_equal_total {       // JSD, BC: the kernels for 128-record blocks with one common word total
    const unsigned long long* cls;   // the blocks' classes, NULL: those kernels are not launched
    bool own_every_tile;             // the fold pass established that the general kernel has no tile left
};
struct plan_bc {
    plan_equal_total sad;
    bool thermo;                // the thermometer-plane Gram owns the matrix
    po_pairdot_plan thermo_plan;
    double inv_n;
};
struct plan_kt {
    uint32_t* lessrank;
    bool mfma, panel;           // pair-dot Gram / rank-panel kernel; neither: the VALU kernel
    po_pairdot_plan pairdot;
    po_kt_panel_plan panel_plan;
};
struct po_pairwise_plan {
    po_ctx* ctx;
    int metric;
    uint32_t flags;
    bool out_f32;
    // the working profiles: the caller's, or recovered from frequencies, or folded (exactly one of counts / freq)
    const uint32_t* counts; const uint64_t* totals; const double* freq;
    uint64_t n, npad;
    uint32_t dim;
    double *ft, *rowstat;       // ws_freq: the float64 operand [dim8][npad]; ws_rowstat [4][npad]
    uint32_t dbl_at = PO_NO_DOUBLING;
    bool folded;
    uint32_t fold_flags = 0xFFFFFFFFu;      // PO_FOLD_*; all set = unknown: launch every candidate kernel
    // the profiles as the caller gave them - not folded - for the pass behind the JSD tile kernels (po_jsd_exact.hip)
    const uint32_t* in_counts; const uint64_t* in_totals; const double* in_freq; uint32_t in_dim;
    plan_eucl eucl;
    plan_equal_total jsd;
    plan_bc bc;
    bool sc_i8;                 // Spearman: the doubled centred ranks go through the exact int8 kernel
    plan_kt kt;
    uint32_t kernel_id;

    bool table_path() const { return !(flags & PO_FLAG_NO_TABLE_PATH); }
    // the fold pass may have established that no 128-record block can have one common total (a ragged assembly).  The
    // equal-total kernels would then be prepared and launched to own no tile - 1.4 ms of empty workgroups at N = 50 000
    bool no_equal_block() const { return fold_flags != 0xFFFFFFFFu && !(fold_flags & PO_FOLD_SOME_EQUAL); }
};

// ---- step 1: the blocks ------------------------------------------------------------------------------------------------------
// *entries: matrix entries the call writes (a mirror counts)
static int check_blocks(const char* who, const po_block* blocks, uint32_t n_blocks, uint64_t n, uint64_t* entries) {
    *entries = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const po_block& k = blocks[b];
        PO_REQUIRE(po_block_inside(k, n), "%s: block %u [%llu,%llu) x [%llu,%llu) outside 0..%llu", who, b, (unsigned long long)k.row_begin,
                   (unsigned long long)k.row_end, (unsigned long long)k.col_begin, (unsigned long long)k.col_end, (unsigned long long)n);
        if (po_block_empty(k)) continue;
        PO_REQUIRE(k.out != nullptr, "%s: block %u has no output buffer", who, b);
        PO_REQUIRE(k.ld_out >= k.col_end - k.col_begin, "%s: block %u: ld_out (%llu) < columns (%llu)", who, b,
                   (unsigned long long)k.ld_out, (unsigned long long)(k.col_end - k.col_begin));
        if (k.triangular)
            PO_TRY(po_check_triangular_block(who, b, k));
        else if (k.mirror)
            PO_REQUIRE(k.ld_mirror >= k.row_end - k.row_begin, "%s: block %u: ld_mirror (%llu) < rows (%llu)", who, b,
                       (unsigned long long)k.ld_mirror, (unsigned long long)(k.row_end - k.row_begin));
        *entries += (k.row_end - k.row_begin) * (k.col_end - k.col_begin) * ((k.mirror && !k.triangular) ? 2 : 1);
    }
    return PO_OK;
}

// ---- step 2: prepare ---------------------------------------------------------------------------------------------------------
// The float64 operand matrix Ft from the working profiles.  skip_flag: see po_launch_prep.
static int launch_operand(const po_pairwise_plan& p, const uint32_t* skip_flag) {
    return p.freq ? po_launch_prep_freq(p.ctx, p.freq, p.n, p.dim, p.npad, p.ft)
                  : po_launch_prep(p.ctx, p.counts, p.totals, p.n, p.dim, p.npad, p.ft, skip_flag, po_gram_i8_value_limit(p.dim));
}

// The shared front.  Frequencies that are count2freq output go back to the exact integer profiles (po_recover.hip); then
// strand-symmetric profiles keep one word per reverse-complement orbit (JSD, BC; po_fold.hip).
static int prepare_front(po_pairwise_plan& p) {
    po_ctx* ctx = p.ctx;
    if (p.freq && p.table_path()) {
        bool recovered = false;
        const uint32_t* rc_counts = nullptr;
        const uint64_t* rc_totals = nullptr;
        PO_TRY(po_recover_counts(ctx, p.freq, p.n, p.dim, &recovered, &rc_counts, &rc_totals));
        if (recovered) {
            p.counts = rc_counts; p.totals = rc_totals; p.freq = nullptr;
        }
    }
    p.in_counts = p.counts; p.in_totals = p.totals; p.in_freq = p.freq; p.in_dim = p.dim;
    if ((p.metric == PO_JSD || p.metric == PO_BC) && !(p.flags & PO_FLAG_NO_RC_FOLD)) {
        uint32_t dim_f = 0, at = PO_NO_DOUBLING;
        PO_TRY(po_rc_fold(ctx, p.counts, p.freq, p.totals, p.n, p.dim, p.metric == PO_BC ? 32u : 8u, &p.folded, &dim_f, &at, &p.fold_flags));
        if (p.folded) {
            if (p.counts) p.counts = static_cast<const uint32_t*>(ctx->ws_fold.p);
            else p.freq = static_cast<const double*>(ctx->ws_fold.p);
            p.dim = dim_f;
            p.dbl_at = at;
        }
    }
    return PO_OK;
}

// Eucl: int8 digit planes (integer profiles) -> host-read block maxima (n >= 8192) -> float64 operand -> norms
static int prepare_eucl(po_pairwise_plan& p) {
    po_ctx* ctx = p.ctx;
    plan_eucl& e = p.eucl;
    e.i8_upto = po_gram_i8_value_limit(p.dim);
    // profiles that fit int8 go through the exact integer MFMA kernel; both tile kernels are launched and the device-side
    // flag decides which one does the work (and whether the float64 operand matrix is built at all)
    if (p.counts && p.table_path()) PO_TRY(po_launch_gram_i8_prep(ctx, p.counts, p.totals, false, p.n, p.dim, p.npad, ctx->ws_aux.p, &e.i8flag));
    // From ~2 000 tiles on, the largest counts (whole matrix and per 128-record block: 4 bytes per block) are read back - the
    // path's one host synchronisation for this metric, ~15 us - and the host launches what is needed: the float64 operand,
    // its norms and its tile kernel only for a matrix beyond the int8 limit, the int8 tile kernels over exactly the tiles of their
    // class.  Before, every candidate was launched over all tiles to find out on the device that it had nothing to do: four
    // launches of 76 000 workgroups that leave at once are 0.2 ms of a 2 ms float32 matrix at N = 50 000.  Small matrices keep
    // the device-side decision (their empty launches cost less than the synchronisation).
    if (e.i8flag && p.n >= 8192) {
        PO_TRY(po_gram_i8_block_maxima(ctx, ctx->ws_aux.p, p.npad, p.dim, &e.i8_hmax));
        e.i8_only = e.i8_hmax[0] <= e.i8_upto;
        if (!e.i8_only) e.i8flag = nullptr;                // the float64 kernels run unconditionally
    }
    if (!e.i8_only) {
        PO_TRY(launch_operand(p, e.i8flag));
        PO_TRY(po_launch_gram_norms(ctx, p.ft, p.dim, p.npad, p.rowstat, e.i8flag, e.i8_upto));
    }
    p.kernel_id = e.i8flag ? PO_KERNEL_MFMA_I8_GRAM : PO_KERNEL_MFMA_F64_GRAM;
    return PO_OK;
}

// JSD, BC: the float64 operand and the per-record terms from it - or, when the fold pass established that the equal-total
// kernels own every tile, no operand at all and the terms straight from the counts.  logtab: JSD's entropies by the table log.
static int prepare_rowstat(po_pairwise_plan& p, plan_equal_total& q, uint32_t not_all_bit, const void* logtab) {
    q.own_every_tile = p.counts && p.table_path() && !(p.fold_flags & not_all_bit);
    if (q.own_every_tile) return po_launch_rowstat_counts(p.ctx, p.counts, p.totals, p.n, p.dim, p.npad, p.rowstat, logtab != nullptr, p.dbl_at);
    PO_TRY(launch_operand(p, nullptr));
    return po_launch_rowstat(p.ctx, p.ft, p.n, p.dim, p.npad, p.rowstat, logtab, p.dbl_at);
}

// JSD: operand (unless the table kernel owns every tile) -> per-record terms -> table prep (unless no block has one total)
static int prepare_jsd(po_pairwise_plan& p) {
    PO_TRY(prepare_rowstat(p, p.jsd, PO_FOLD_NOT_ALL_TABLE, p.ctx->ws_logtab.p));
    // record blocks with one common word total go through the integer-sum table kernel, the rest through the general
    // float64 kernel; each launch skips the other's tiles (decided on device)
    if (p.counts && p.table_path() && !p.no_equal_block())
        PO_TRY(po_launch_jsd_lut_prep(p.ctx, p.counts, p.totals, p.n, p.dim, p.npad, p.rowstat + p.npad, p.ctx->ws_aux.p, &p.jsd.cls));
    p.kernel_id = p.jsd.cls ? PO_KERNEL_LUT_JSD : PO_KERNEL_VALU_JSD;
    return PO_OK;
}

// BC: operand (unless the SAD kernel owns every tile) -> per-record terms -> SAD prep -> thermometer prep
static int prepare_bc(po_pairwise_plan& p) {
    po_ctx* ctx = p.ctx;
    plan_bc& q = p.bc;
    PO_TRY(prepare_rowstat(p, q.sad, PO_FOLD_NOT_ALL_SAD, nullptr));
    if (p.counts && p.table_path() && !p.no_equal_block()) {
        // the same split as JSD: equal-total record blocks with byte-sized counts take the packed SAD kernel
        PO_TRY(po_launch_bc_sad_prep(ctx, p.counts, p.totals, p.n, p.dim, p.npad, ctx->ws_aux.p, &q.sad.cls));
        // one common word total and few count levels per word: sum of min as a matrix-core Gram over thermometer
        // planes (po_pairdot.hip); decided from a small header read back from the device
        const uint32_t* p8t = nullptr;
        uint32_t gp = 0;
        po_bc_sad_view(ctx->ws_aux.p, p.npad, p.dim, &p8t, &gp);
        if (!(p.flags & PO_FLAG_NO_PAIRDOT))
            PO_TRY(po_launch_bc_thermo_prep(ctx, p8t, gp, q.sad.cls, p.n, p.dim, p.npad, p.dbl_at, (p.flags & PO_FLAG_PAIRDOT_I8) ? 0 : 1,
                                            &q.thermo, &q.thermo_plan, &q.inv_n));
    }
    p.kernel_id = q.thermo ? PO_KERNEL_MFMA_BC : q.sad.cls ? PO_KERNEL_SAD_BC : PO_KERNEL_VALU_BC;
    return PO_OK;
}

// SC: ranks -> int8 digit planes of the doubled centred ranks, or the float64 centred ranks and their norms
static int prepare_sc(po_pairwise_plan& p) {
    po_ctx* ctx = p.ctx;
    const uint32_t* counts = p.freq ? nullptr : p.counts;
    // the doubled centred ranks are small integers -> the same exact int8 kernel as Eucl (two digit planes)
    p.sc_i8 = po_gram_i8_sc_supported(p.dim) && p.table_path();
    p.kernel_id = p.sc_i8 ? PO_KERNEL_MFMA_I8_GRAM : PO_KERNEL_MFMA_F64_GRAM;
    if (p.sc_i8) {
        int32_t* r2 = static_cast<int32_t*>(ctx->ws_freq.p);           // the float64 operand buffer is free on this path
        PO_TRY(po_launch_ranks(ctx, counts, p.freq, p.n, p.dim, p.npad, nullptr, nullptr, r2, p.rowstat));
        return po_launch_gram_i8_prep(ctx, reinterpret_cast<const uint32_t*>(r2), nullptr, true, p.n, p.dim, p.npad, ctx->ws_aux.p, nullptr);
    }
    PO_TRY(po_launch_ranks(ctx, counts, p.freq, p.n, p.dim, p.npad, p.ft, nullptr, nullptr, p.rowstat));
    return po_launch_gram_norms(ctx, p.ft, p.dim, p.npad, p.rowstat, nullptr, po_gram_i8_value_limit(p.dim));
}

// KT: ranks -> fold (one word per reverse-complement orbit, weighted; po_fold.hip) -> the pair-dot operand, or without room for
// it (PO_ENOMEM) or support the rank panels, or neither: the VALU kernel reads the ranks
static int prepare_kt(po_pairwise_plan& p) {
    po_ctx* ctx = p.ctx;
    plan_kt& q = p.kt;
    q.lessrank = static_cast<uint32_t*>(ctx->ws_aux.p);
    PO_TRY(po_launch_ranks(ctx, p.freq ? nullptr : p.counts, p.freq, p.n, p.dim, p.npad, nullptr, q.lessrank, nullptr, p.rowstat));
    q.mfma = po_kt_pairdot_supported(p.dim) && !(p.flags & (PO_FLAG_NO_TABLE_PATH | PO_FLAG_NO_PAIRDOT));
    const bool panel_ok = po_kt_panel_supported(p.dim) && p.table_path();
    p.kernel_id = PO_KERNEL_VALU_KT;
    if (!q.mfma && !panel_ok) return PO_OK;
    const uint32_t selfs = po_fold_selfs(p.dim);
    const uint32_t* fold_src = nullptr;
    uint32_t fold_len = 0;
    const bool can_fold = selfs != 0xFFFFFFFFu && (q.mfma || po_kt_panel_fold_supported(p.dim, selfs));
    if (!(p.flags & PO_FLAG_NO_RC_FOLD) && can_fold) {
        uint32_t at = 0;
        PO_TRY(po_rc_fold(ctx, p.counts, p.freq, nullptr, p.n, p.dim, PO_FOLD_SELFS_FIRST, &p.folded, &fold_len, &at, nullptr));
        if (p.folded) fold_src = static_cast<const uint32_t*>(ctx->ws_fold_src.p);
    }
    const uint32_t n_pairs = fold_src ? (p.dim - selfs) / 2 : 0;
    const int want_fp4 = (p.flags & PO_FLAG_PAIRDOT_I8) ? 0 : 1;
    // the materialised operand must stay within bounds (it grows with D^2: 1 MB per record at folded k = 6)
    if (q.mfma && po_kt_pairdot_operand_bytes(p.n, p.dim, fold_src ? selfs + n_pairs : p.dim, selfs, fold_src != nullptr, want_fp4) >
                      PO_PAIRDOT_MAX_OPERAND)
        q.mfma = false;
    if (q.mfma) {
        const int rc = po_launch_kt_pairdot_prep(ctx, q.lessrank, p.n, p.dim, p.npad, fold_src, selfs, n_pairs, want_fp4, &q.pairdot);
        if (rc == PO_ENOMEM) q.mfma = false;               // no room for the operand: the panel / VALU kernel does without
        else if (rc) return rc;
    }
    q.panel = !q.mfma && panel_ok;
    if (q.panel && fold_src && !po_kt_panel_fold_supported(p.dim, selfs)) { fold_src = nullptr; p.folded = false; }
    if (q.panel) PO_TRY(po_launch_kt_panel_prep(ctx, q.lessrank, p.n, p.dim, p.npad, ctx->ws_freq.p, fold_src, fold_len, selfs, n_pairs, &q.panel_plan));
    if (q.mfma || q.panel) p.kernel_id = PO_KERNEL_MFMA_I8_KT;
    return PO_OK;
}

static int prepare(po_pairwise_plan& p) {
    PO_TRY(prepare_front(p));
    switch (p.metric) {
        case PO_EUCL: return prepare_eucl(p);
        case PO_JSD: return prepare_jsd(p);
        case PO_BC: return prepare_bc(p);
        case PO_SC: return prepare_sc(p);
        default: return prepare_kt(p);
    }
}

// ---- step 3: one block ----------------------------------------------------------------------------------------------------
// the equal-total kernel over its tiles, the general kernel over the rest (JSD, BC)
template <typename F>
static int launch_equal_total(const po_pairwise_plan& p, const plan_equal_total& q, const po_tile_args& a, uint64_t* tiles, F&& equal_total_tiles) {
    if (q.cls) PO_TRY(equal_total_tiles());
    if (q.cls && q.own_every_tile) return PO_OK;
    return po_launch_valu_tiles(p.ctx, p.metric, a, q.cls, q.cls ? nullptr : tiles);
}

static int launch_jsd(const po_pairwise_plan& p, po_tile_args& a, uint64_t* tiles) {
    PO_TRY(po_jsd_exact_reset(p.ctx, &a.fix));
    PO_TRY(launch_equal_total(p, p.jsd, a, tiles, [&] { return po_launch_jsd_lut_tiles(p.ctx, a, p.n, p.ctx->ws_aux.p, tiles); }));
    return po_launch_jsd_exact(p.ctx, a, p.in_counts, p.in_totals, p.in_freq, p.in_dim);   // values at cancellation level, once more
}

static int launch_bc(const po_pairwise_plan& p, const po_tile_args& a, uint64_t* tiles) {
    if (p.bc.thermo) return po_launch_bc_thermo_tiles(p.ctx, a, p.bc.thermo_plan, p.bc.inv_n, tiles);
    return launch_equal_total(p, p.bc.sad, a, tiles, [&] { return po_launch_bc_sad_tiles(p.ctx, a, p.ctx->ws_aux.p, tiles); });
}

static int launch_eucl(const po_pairwise_plan& p, const po_tile_args& a, uint64_t* tiles) {
    const plan_eucl& e = p.eucl;
    if (e.i8flag) PO_TRY(po_launch_gram_i8_tiles(p.ctx, PO_EUCL, a, p.ctx->ws_aux.p, e.i8_hmax, tiles));
    if (e.i8_only) return PO_OK;
    return po_launch_gram_f64(p.ctx, PO_EUCL, a, e.i8flag, e.i8_upto, e.i8flag ? nullptr : tiles);
}

static int launch_sc(const po_pairwise_plan& p, const po_tile_args& a, uint64_t* tiles) {
    if (p.sc_i8) return po_launch_gram_i8_tiles(p.ctx, PO_SC, a, p.ctx->ws_aux.p, nullptr, tiles);
    return po_launch_gram_f64(p.ctx, PO_SC, a, nullptr, 0, tiles);
}

static int launch_kt(const po_pairwise_plan& p, const po_tile_args& a, uint64_t* tiles) {
    if (p.kt.mfma) return po_launch_kt_pairdot_tiles(p.ctx, a, p.kt.pairdot, tiles);
    if (p.kt.panel) return po_launch_kt_panel_tiles(p.ctx, a, p.ctx->ws_freq.p, p.kt.panel_plan, tiles);
    return po_launch_kt(p.ctx, p.kt.lessrank, p.n, p.dim, a, tiles);
}

static int launch_block(const po_pairwise_plan& p, const po_block& k, uint64_t* tiles) {
    po_tile_args a;
    a.ft = p.ft; a.rowstat = p.rowstat;
    a.n = p.n; a.npad = p.npad; a.dim = p.dim;
    a.row_begin = k.row_begin; a.row_end = k.row_end;
    a.col_begin = k.col_begin; a.col_end = k.col_end;
    a.out = k.out; a.ld_out = k.ld_out;
    a.triangular = k.triangular ? 1 : 0;
    a.mirror = k.triangular ? k.out : k.mirror;
    a.ld_mirror = k.triangular ? k.ld_out : k.ld_mirror;
    a.out_f32 = p.out_f32; a.dbl_at = p.dbl_at;
    a.fix = nullptr;
    switch (p.metric) {
        case PO_JSD: return launch_jsd(p, a, tiles);
        case PO_BC: return launch_bc(p, a, tiles);
        case PO_EUCL: return launch_eucl(p, a, tiles);
        case PO_SC: return launch_sc(p, a, tiles);
        default: return launch_kt(p, a, tiles);
    }
}

// ---- the driver ---------------------------------------------------------------------------------------------------------------
int po_pairwise_run(po_ctx* ctx, const char* who, const uint32_t* d_counts, const uint64_t* d_totals, const double* d_freq, uint64_t n,
                    uint32_t dim, int metric, int out_dtype, const po_block* blocks, uint32_t n_blocks, uint32_t flags, po_stats* stats,
                    po_after_block_fn after_block, void* after_user) {
    PO_TRY(po_check_ctx(who, ctx));
    PO_TRY(po_check_metric(metric));
    PO_TRY(po_check_dtype(who, "out_dtype", out_dtype));
    PO_TRY(po_check_dim(who, dim));
    PO_REQUIRE(blocks != nullptr || n_blocks == 0, "%s: NULL block list", who);
    if (stats) memset(stats, 0, sizeof(*stats));
    uint64_t entries = 0;
    PO_TRY(check_blocks(who, blocks, n_blocks, n, &entries));
    if (n == 0 || entries == 0) return PO_OK;
    PO_REQUIRE(d_freq != nullptr || (d_counts != nullptr && d_totals != nullptr), "%s: NULL buffer", who);
    PO_HIP(hipSetDevice(ctx->device));
    PO_TRY(reserve_pairwise(ctx, n, dim, metric, false));

    po_pairwise_plan plan{};
    plan.ctx = ctx; plan.metric = metric; plan.flags = flags; plan.out_f32 = out_dtype == PO_F32;
    plan.counts = d_counts; plan.totals = d_totals; plan.freq = d_freq;
    plan.n = n; plan.npad = po_round_up(n, PO_PAD_ROWS); plan.dim = dim;
    plan.ft = static_cast<double*>(ctx->ws_freq.p);
    plan.rowstat = static_cast<double*>(ctx->ws_rowstat.p);
    if (stats) PO_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    PO_TRY(prepare(plan));
    if (stats) PO_HIP(hipEventRecord(ctx->ev[1], ctx->stream));

    uint64_t tiles = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        if (po_block_empty(blocks[b])) continue;
        PO_TRY(launch_block(plan, blocks[b], &tiles));
        if (after_block) PO_TRY(after_block(after_user, b));
    }
    if (stats) {
        PO_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
        PO_HIP(hipEventSynchronize(ctx->ev[2]));
        float prep = 0.f, kernel = 0.f, total = 0.f;
        PO_HIP(hipEventElapsedTime(&prep, ctx->ev[0], ctx->ev[1]));
        PO_HIP(hipEventElapsedTime(&kernel, ctx->ev[1], ctx->ev[2]));
        PO_HIP(hipEventElapsedTime(&total, ctx->ev[0], ctx->ev[2]));
        stats->prep_ms = prep; stats->kernel_ms = kernel; stats->total_ms = total;
        stats->pairs = entries / 2;
        stats->tiles = tiles;
        stats->kernel_id = plan.kernel_id;
        stats->rc_folded = plan.folded ? 1u : 0u;
    }
    return PO_OK;
}

// ---- entry points over rows [row_begin,row_end) x all columns -----------------------------------------------------------------
// one block; the full matrix is one triangular block
static po_block rows_block(uint64_t n, uint64_t row_begin, uint64_t row_end, void* out, uint64_t ld_out, uint32_t flags) {
    po_block k;
    memset(&k, 0, sizeof(k));
    k.row_begin = row_begin; k.row_end = row_end;
    k.col_begin = 0; k.col_end = n;
    k.out = out; k.ld_out = ld_out;
    k.triangular = (row_begin == 0 && row_end == n && !(flags & PO_FLAG_NO_SYMMETRY)) ? 1u : 0u;
    return k;
}

static int check_row_range(const char* who, uint64_t n, uint64_t row_begin, uint64_t row_end) {
    PO_REQUIRE(row_begin <= row_end && row_end <= n, "%s: row range [%llu,%llu) outside 0..%llu", who,
               (unsigned long long)row_begin, (unsigned long long)row_end, (unsigned long long)n);
    return PO_OK;
}

// The device forms.  They refuse in an order of their own - stats emptied, the row range, the result, the profiles, and only
// then what po_pairwise_run checks - so those checks stay here.
static int pairwise_dev(po_ctx* ctx, const char* who, const uint32_t* d_counts, const uint64_t* d_totals, const double* d_freq, uint64_t n,
                        uint32_t dim, int metric, uint64_t row_begin, uint64_t row_end, int out_dtype, void* d_out, uint64_t ld_out,
                        uint32_t flags, po_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    PO_TRY(check_row_range(who, n, row_begin, row_end));
    if (n && row_begin != row_end) {
        PO_REQUIRE(d_out != nullptr, "%s: NULL buffer", who);
        PO_REQUIRE(ld_out >= n, "%s: ld_out (%llu) < n (%llu)", who, (unsigned long long)ld_out, (unsigned long long)n);
        PO_REQUIRE(d_freq != nullptr || (d_counts != nullptr && d_totals != nullptr), "%s: NULL buffer", who);
    }
    const po_block k = rows_block(n, row_begin, row_end, d_out, ld_out, flags);
    return po_pairwise_run(ctx, who, d_counts, d_totals, d_freq, n, dim, metric, out_dtype, &k, 1, flags, stats);
}

extern "C" int po_pairwise_dev(po_ctx* ctx, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n, uint32_t dim, int metric,
                               uint64_t row_begin, uint64_t row_end, int out_dtype, void* d_out, uint64_t ld_out, uint32_t flags, po_stats* stats) {
    return pairwise_dev(ctx, "po_pairwise_dev", d_counts, d_totals, nullptr, n, dim, metric, row_begin, row_end, out_dtype, d_out, ld_out, flags, stats);
}

extern "C" int po_pairwise_freq_dev(po_ctx* ctx, const double* d_freq, uint64_t n, uint32_t dim, int metric, uint64_t row_begin, uint64_t row_end,
                                    int out_dtype, void* d_out, uint64_t ld_out, uint32_t flags, po_stats* stats) {
    return pairwise_dev(ctx, "po_pairwise_freq_dev", nullptr, nullptr, d_freq, n, dim, metric, row_begin, row_end, out_dtype, d_out, ld_out, flags, stats);
}

extern "C" int po_pairwise_blocks_dev(po_ctx* ctx, const uint32_t* d_counts, const uint64_t* d_totals, uint64_t n, uint32_t dim, int metric,
                                      int out_dtype, const po_block* blocks, uint32_t n_blocks, uint32_t flags, po_stats* stats) {
    return po_pairwise_run(ctx, "po_pairwise_blocks_dev", d_counts, d_totals, nullptr, n, dim, metric, out_dtype, blocks, n_blocks, flags, stats);
}

// Device rows -> pageable host rows through two pinned staging buffers: the DMA of chunk c+1 runs while host
// threads copy chunk c into the caller's memory.  Measured on the gpurun box for 6 GB (tools/ubench/d2h_paths.hip):
// plain hipMemcpy into fresh pageable memory 18 GB/s; hipHostRegister of the destination + copy 15-17 GB/s all
// in (registering costs 0.3 s); hipHostMalloc of a pinned result 7 GB/s all in (0.8 s to allocate, 0.5 s to free);
// this ring into 4 KiB pages 15 GB/s, into transparent huge pages 43 GB/s (the link itself does 57 GB/s).
static int copy_rows_to_host(po_ctx* ctx, const uint8_t* d_src, size_t src_pitch, size_t row_bytes, uint64_t rows,
                             uint8_t* dst, size_t dst_pitch) {
    const size_t kStage = 32u << 20;
    if (rows == 0 || row_bytes == 0) return PO_OK;
    if (rows * row_bytes < (64u << 20) || row_bytes > kStage) {      // small result (or absurdly long rows): one plain copy
        PO_HIP(hipMemcpy2DAsync(dst, dst_pitch, d_src, src_pitch, row_bytes, rows, hipMemcpyDeviceToHost, ctx->stream));
        PO_HIP(hipStreamSynchronize(ctx->stream));
        return PO_OK;
    }
    // A freshly allocated destination (numpy.zeros / numpy.empty: untouched anonymous pages) is first touched by the
    // copy threads below; with 4 KiB pages that is 1.8 million page faults for a 7 GB matrix and caps the copy at
    // ~15 GB/s.  Asking for transparent huge pages first (harmless if the range is already populated or the kernel
    // declines) measured 43 GB/s on the same box (tools/ubench/d2h_paths.hip: ring 2 x 32 MB, 8 threads, THP).
    {
        const uintptr_t lo = (reinterpret_cast<uintptr_t>(dst) + 4095u) & ~(uintptr_t)4095u;
        const uintptr_t hi = (reinterpret_cast<uintptr_t>(dst) + (rows - 1) * dst_pitch + row_bytes) & ~(uintptr_t)4095u;
        if (hi > lo) (void)madvise(reinterpret_cast<void*>(lo), hi - lo, MADV_HUGEPAGE);
    }
    if (!ctx->h_stage[0]) {
        PO_HIP(hipHostMalloc(&ctx->h_stage[0], kStage, hipHostMallocDefault));
        PO_HIP(hipHostMalloc(&ctx->h_stage[1], kStage, hipHostMallocDefault));
    }
    // the ring itself is host code (po_ring_copy_rows, po_io.cpp: it also runs under the thread sanitizer, `make san`);
    // here only the two HIP calls it is built around
    struct d2h_src { po_ctx* ctx; const uint8_t* d_src; size_t src_pitch, row_bytes; hipError_t err; } u{ctx, d_src, src_pitch, row_bytes, hipSuccess};
    po_ring_source ring;
    ring.user = &u;
    ring.issue = [](void* p, uint64_t, void* stage, uint64_t r0, uint64_t nr) -> int {
        d2h_src* s = static_cast<d2h_src*>(p);
        s->err = hipMemcpy2DAsync(stage, s->row_bytes, s->d_src + r0 * s->src_pitch, s->src_pitch, s->row_bytes, nr,
                                  hipMemcpyDeviceToHost, s->ctx->stream);
        return s->err == hipSuccess ? PO_OK : PO_EHIP;
    };
    ring.wait = [](void* p) -> int {
        d2h_src* s = static_cast<d2h_src*>(p);
        s->err = hipStreamSynchronize(s->ctx->stream);
        return s->err == hipSuccess ? PO_OK : PO_EHIP;
    };
    const int rc = po_ring_copy_rows(ring, ctx->h_stage, kStage, row_bytes, rows, dst, dst_pitch, po_host_threads(14));
    if (rc == PO_EHIP) po_set_error("device to host copy: %s", hipGetErrorString(u.err));
    return rc;
}

// The host-pointer forms: stage in ws_io, run the driver, copy the rows back.  Their refusals come in another order than the
// driver's (the profiles first, before even the context; the row range before the buffers; dim last), so their checks stay here.
static int pairwise_host(po_ctx* ctx, const char* who, const uint32_t* counts, const uint64_t* totals, const double* freq, uint64_t n, uint32_t dim,
                         int metric, uint64_t row_begin, uint64_t row_end, int out_dtype, void* out, uint64_t ld_out, uint32_t flags, po_stats* stats) {
    const bool have_profiles = freq != nullptr || (counts != nullptr && totals != nullptr);
    PO_REQUIRE(have_profiles || n == 0 || row_begin == row_end, "%s: NULL buffer", who);
    PO_TRY(po_check_ctx(who, ctx));
    PO_TRY(po_check_metric(metric));
    PO_TRY(po_check_dtype(who, "out_dtype", out_dtype));
    PO_TRY(check_row_range(who, n, row_begin, row_end));
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0 || row_begin == row_end) return PO_OK;
    PO_REQUIRE(out != nullptr, "%s: NULL buffer", who);
    PO_REQUIRE(ld_out >= n, "%s: ld_out (%llu) < n (%llu)", who, (unsigned long long)ld_out, (unsigned long long)n);
    PO_TRY(po_check_dim(who, dim));
    PO_HIP(hipSetDevice(ctx->device));

    const size_t esz = (out_dtype == PO_F32) ? 4 : 8;
    const uint64_t rows = row_end - row_begin;
    // the device copy of the result has its rows on 128-byte boundaries whatever n is (row stride rounded up to 32 entries): the
    // tile kernels' 16-byte stores want aligned rows, and row pieces that start on a line boundary are written ~25 % faster
    const uint64_t ld_dev = po_round_up(n, 32);
    uint8_t *d_in = nullptr, *d_out = nullptr;
    uint64_t* d_tot = nullptr;
    PO_TRY(po_stage(ctx, &ctx->ws_io, [&](po_carver& ws) {
        d_in = ws.take(n * (uint64_t)dim * (freq ? sizeof(double) : sizeof(uint32_t)));
        d_tot = ws.array<uint64_t>(n);
        d_out = ws.take(rows * ld_dev * esz);
    }));
    if (freq) PO_HIP(hipMemcpyAsync(d_in, freq, n * (uint64_t)dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    else PO_TRY(po_upload_profiles(ctx, n, dim, counts, totals, reinterpret_cast<uint32_t*>(d_in), d_tot));
    const po_block k = rows_block(n, row_begin, row_end, d_out, ld_dev, flags);
    PO_TRY(po_pairwise_run(ctx, who, freq ? nullptr : reinterpret_cast<const uint32_t*>(d_in), freq ? nullptr : d_tot,
                           freq ? reinterpret_cast<const double*>(d_in) : nullptr, n, dim, metric, out_dtype, &k, 1, flags, stats));
    return copy_rows_to_host(ctx, d_out, ld_dev * esz, n * esz, rows, static_cast<uint8_t*>(out), ld_out * esz);
}

extern "C" int po_pairwise(po_ctx* ctx, const uint32_t* counts, const uint64_t* totals, uint64_t n, uint32_t dim, int metric, uint64_t row_begin,
                           uint64_t row_end, int out_dtype, void* out, uint64_t ld_out, uint32_t flags, po_stats* stats) {
    return pairwise_host(ctx, "po_pairwise", counts, totals, nullptr, n, dim, metric, row_begin, row_end, out_dtype, out, ld_out, flags, stats);
}

extern "C" int po_pairwise_freq(po_ctx* ctx, const double* freq, uint64_t n, uint32_t dim, int metric, uint64_t row_begin, uint64_t row_end,
                                int out_dtype, void* out, uint64_t ld_out, uint32_t flags, po_stats* stats) {
    return pairwise_host(ctx, "po_pairwise_freq", nullptr, nullptr, freq, n, dim, metric, row_begin, row_end, out_dtype, out, ld_out, flags, stats);
}
