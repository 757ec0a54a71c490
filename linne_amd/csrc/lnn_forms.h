/* lnn_forms.h -- which form of a kernel a call, a chunk and a layer get, as pure host code: the one place where a reader finds
 * "which form at which size and why".  lnn_device.hip asks here and launches what the answer says; nothing in this header touches a
 * GPU, and it compiles in a translation unit that has never seen hip/hip_runtime.h (the class predicates below are also device code
 * when hipcc compiles them: the kernels call these same hist_takes / fwd_loss_takes / search_long_takes, so host and kernels
 * cannot drift apart).  Four parts: the knobs, the class bookkeeping of a call, the split of a call into chunks over streams, the
 * forms of an encode chunk and of a decode call.  Every rule keeps the measurement it came from. */
#ifndef LNN_FORMS_H_INCLUDED
#define LNN_FORMS_H_INCLUDED

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "linne_amd.h"

#if defined(__HIPCC__)
#define LNN_HD __host__ __device__ __forceinline__
#else
#define LNN_HD inline
#endif

#define LNN_MAXT        8       /* unit-count trials per layer: u = 1,2,...,128 */
#define LNN_MAXU        128
#define LNN_MAXP        128
#define LNN_MAXL        3
#define LNN_MAXR        4
#define LNN_MAXCLS      16
#define LNN_MAXCH       8
#define LNN_ACW         256     /* autocorrelation words per (job, trial): P + u <= 256 */
#define LNN_MAXSUB      8
#define LNN_META        8
#define LNN_FIR_TILE 2048u               /* samples per block of the search / forward kernels (lnn_k_fir.h FIR_TILE) */
/* what the rules below need to know of the kernels' tiling (lnn_device.hip asserts that they are the kernels' own) */
#define LNN_FIR_WAVES   4u              /* waves of a search / forward block: FIR_THREADS / 64 */
#define LNN_SELW_MAXPART 64u            /* partial sums k_select_wave can hold per (job, trial): SELW_MAXPART */
#define LNN_SEARCH_JOB_MIN 8u           /* SEARCH_JOB_MIN */
#define LNN_LEV_MAXRIDE 3u              /* short Levinson trials that ride with the one-unit trial: LEV_MAXRIDE */
#define LEV_LDS(np_) (sizeof(double) * 64 * (size_t)(2 * (np_) + 3))       /* LDS columns of one Levinson problem set of order np_ */
#define LEV_LDS_BUDGET ((size_t)160 * 1024)                                   /* LDS of a CU */
#define LNN_SUB_TILE_SMALL 16u          /* tile depth of the small-LDS k_autocorr_sub (every other caller of autocorr_rows: 32) */
#define LNN_SUB_SMALL_LDS ((size_t)8 * (2 * LNN_SUB_TILE_SMALL * 65 + 2 * LNN_MAXT * 32))      /* its static LDS: tile[2][16][65] + wts_mem, 20 736 bytes */
#define LNN_LEV_BESIDE_MIN 32768u       /* jobs of a chunk from which the order-128 Levinson launch runs beside the lag kernels */
#define LNN_LEV_BESIDE_DEFAULT 1        /* the size rule is in force (0: only LINNE_AMD_LEV_BESIDE=1 turns the form on) */

/* one distinct frame length of a batch (full frames, the ragged tail, ...) */
struct DevClass {
    uint32_t n;                         /* valid samples                                             */
    uint32_t na;                        /* analysis length (linne_encoder.c:644-655)                 */
    uint32_t sin_off;                   /* offset of this class's SIN window table                   */
    uint32_t pad;
    uint32_t ntrials[LNN_MAXL];
    uint32_t trial_u[LNN_MAXL][LNN_MAXT];
    double   trial_div[LNN_MAXL][LNN_MAXT];   /* 4*pow(na/u - 1, -2) from the host libm (lpc.c:199)  */
    uint32_t wt_off[LNN_MAXL][LNN_MAXT];      /* offset of the trial's Welch weight table (padded unit: n + max(p,4) entries) */
};

/* Rows of a chunk (channel-frames, or jobs) cut into runs of one length class, so that the kernels that put 64 rows on
 * the lanes of a wave see blocks of one class and may take their wave-uniform fast paths; a ragged last frame gets a
 * block of its own.  Run i = rows [row_begin[i], row_begin[i+1]) = blocks [blk_begin[i], blk_begin[i+1]) of 64 rows.
 * The host hands the frames of a call to the kernels sorted by class (Plan.frame_map leads back to the caller's order), so a
 * chunk never has more runs than there are classes.  Only with the sort switched off (LINNE_AMD_SORT=0, a test knob) can a
 * chunk exceed LNN_MAXRUN runs: then one run covers everything (blocks may mix classes: slower, same results). */
#define LNN_MAXRUN LNN_MAXCLS
struct RowRuns { uint32_t n; uint32_t mixed; uint32_t row_begin[LNN_MAXRUN + 1]; uint32_t blk_begin[LNN_MAXRUN + 1]; };   /* mixed: the one-run fallback */

/* what a preset means: layers, their orders, regularisers (lnn_preset_info) */
struct HostShape { uint32_t L, R, P[LNN_MAXL], coef_off[LNN_MAXL], maxP; double regs[LNN_MAXR]; };

/* ------------------------------------------------------------------------------------------------
 * class predicates: which frames the lanes = jobs kernels take.  One definition for the kernels (PlanT = Plan, lnn_dev_common.h)
 * and for the host rules below (PlanT = LnnPlanView): a host copy that drifted from the device's would make the host skip a
 * fallback launch that the kernels still expect.
 * ---------------------------------------------------------------------------------------------- */
struct LnnPlanView { uint32_t L, S, hist, search_long, fused_last, P[LNN_MAXL]; };     /* what the predicates read of a Plan */

/* does k_search_long (lnn_k_search.h) produce this job's unit-count search of `layer`?  The long layer (64 / 128 taps) of a preset
 * with a layer behind it, every trial present, the analysis length whole 2048-sample tiles (all full 10240-sample frames);
 * k_fir2<2> keeps the other frames */
template <class PlanT> LNN_HD bool search_long_takes(const PlanT &p, uint32_t layer, const DevClass &c)
{
    const uint32_t P = p.P[layer];
    uint32_t nt = 0; for (uint32_t u = 1; u <= P && u <= (uint32_t)LNN_MAXU; u <<= 1) nt++;
    return p.search_long && layer > 0 && layer + 1 < p.L && (P == 128u || P == 64u) && c.ntrials[layer] == nt && (c.na % LNN_FIR_TILE) == 0;
}

/* does k_fwd_loss (lnn_k_fwdloss.h) produce this job's last-layer loss?  (na: the job's analysis length) */
template <class PlanT> LNN_HD bool fwd_loss_takes(const PlanT &p, uint32_t layer, uint32_t na) { return p.fused_last && layer + 1 == p.L && (na % (4u * p.P[layer])) == 0; }

/* Which frames k_autocorr_hist / k_autocorr_sub (lnn_k_autocorr_hist.h) take (the others stay with k_autocorr2, which skips
 * the ones taken there): every trial present,
 * every unit a whole number of 16-sample tiles, the finest unit at least one weight tile long, rows 16-byte aligned. */
template <class PlanT> LNN_HD bool hist_takes(const PlanT &p, uint32_t layer, const DevClass &c)
{
    const uint32_t P = p.P[layer];
    uint32_t nt = 0; for (uint32_t u = 1; u <= P && u <= (uint32_t)LNN_MAXU; u <<= 1) nt++;
    return p.hist && P >= 64u && c.ntrials[layer] == nt && (c.na % (16u << (nt - 1))) == 0 && (c.na >> (nt - 1)) >= 32u && (p.S & 3u) == 0;
}
static inline uint32_t lnn_all_trials(uint32_t P) { uint32_t nt = 0; for (uint32_t u = 1; u <= P && u <= (uint32_t)LNN_MAXU; u <<= 1) nt++; return nt; }

/* ------------------------------------------------------------------------------------------------
 * knobs: every environment variable that selects a kernel form.  Production sets none and gets the size rules.
 * ---------------------------------------------------------------------------------------------- */
struct LnnKnobs {
    /* read once, when the context is created (lnn_knobs_read_context) */
    int fwd_loss;                       /* LINNE_AMD_FWD_LOSS: last layer's forward pass and loss in one kernel (k_fwd_loss); -1 = by batch size */
    int lev_ride;                       /* short Levinson trials ride along with the one-unit trial (LINNE_AMD_LEV_RIDE, default 1) */
    int lev_beside;                     /* LINNE_AMD_LEV_BESIDE: the long layer's order-128 Levinson launch on the chunk's sibling stream beside the short-trial lags; 0 / 1 never / always, -1 = by chunk size; 2 (a measuring knob) = the same launches -- riders moved, small-LDS lag form -- all on the chunk's own stream, nothing overlapped */
    int lev_wave;                       /* batches of <= 64 jobs: a wave per Levinson problem (LINNE_AMD_LEV_WAVE, default 1) */
    int search_two;                     /* k_search_long in two passes over the window, five waves per SIMD (LINNE_AMD_SEARCH_TWO) */
    int search_job;                     /* k_search_long with one block per job that walks the job's tiles: 1 always, 0 never ((jobs, tiles) blocks), -1 by the size of the batch (LINNE_AMD_SEARCH_JOB, default -1) */
    int fir_small;                      /* LINNE_AMD_FIR_SMALL (default 1): register-window search kernel for layers of <= 16 taps */
    int fir_spec;                       /* LINNE_AMD_SPECULATE (default 1): fuse the one-unit forward into the search of layers 0 .. L-2 */
    int force_exact;                    /* LINNE_AMD_EXACT=1: every unit-count search runs the exact ordered chains (diff against the certified search) */
    /* read per CALL (lnn_knobs_read_call: once at the top of an encode / decode call, never inside the chunk loop) */
    int sort, l0_products, wide, search_long, rows16, prep_general;
    int stats_rows;                     /* -1 = by batch size */
    int hist;                           /* -1 = by batch size */
    int decode_kernel;                  /* 0 = by batch size, 1 = wave, 2 = lanes, 3 = pipe, 4 = rows */
    int rows8;                          /* LINNE_AMD_DECODE_ROWS8: -1 = by batch size */
    int streams;                        /* LINNE_AMD_STREAMS of this call, 0 = not given */
    int nostats;
    int fwd_loss_mw;                    /* LINNE_AMD_FWD_LOSS_MW (default 1): chunks below 65 536 jobs take the five-wave form of k_fwd_loss */
    int prep_defer;                     /* LINNE_AMD_PREP_DEFER (default 1): inexact pre-emphasis sums go to k_prep_slow */
    int last_layer;                     /* LINNE_AMD_LAST_LAYER (default 1): the last layer's search, forward pass and loss in one launch (k_last_layer) where it takes the chunk */
    int decode_fused;                   /* LINNE_AMD_DECODE_FUSED (default 1): layer 0 + de-emphasis + MS -> LR in one launch */
    uint32_t dbg_maxtr;
};
static inline int lnn_env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
static inline void lnn_knobs_read_context(LnnKnobs *k)
{
    k->force_exact = lnn_env_int("LINNE_AMD_EXACT", 0);
    k->fir_spec = lnn_env_int("LINNE_AMD_SPECULATE", 1);
    k->lev_ride = lnn_env_int("LINNE_AMD_LEV_RIDE", 1);
    k->lev_wave = lnn_env_int("LINNE_AMD_LEV_WAVE", 1);
    k->lev_beside = lnn_env_int("LINNE_AMD_LEV_BESIDE", -1);
    k->search_two = lnn_env_int("LINNE_AMD_SEARCH_TWO", 1);
    k->search_job = lnn_env_int("LINNE_AMD_SEARCH_JOB", -1);
    k->fwd_loss = lnn_env_int("LINNE_AMD_FWD_LOSS", -1);
    k->fir_small = lnn_env_int("LINNE_AMD_FIR_SMALL", 1);
}
static inline void lnn_knobs_read_call(LnnKnobs *k)
{
    k->sort = lnn_env_int("LINNE_AMD_SORT", 1);
    k->l0_products = lnn_env_int("LINNE_AMD_L0_PRODUCTS", 1);
    k->wide = lnn_env_int("LINNE_AMD_WIDE", 1);
    k->search_long = lnn_env_int("LINNE_AMD_SEARCH_LONG", 1);
    k->rows16 = lnn_env_int("LINNE_AMD_ROWS16", 1);
    k->prep_general = lnn_env_int("LINNE_AMD_PREP_GENERAL", 0);
    k->prep_defer = lnn_env_int("LINNE_AMD_PREP_DEFER", 1);
    k->fwd_loss_mw = lnn_env_int("LINNE_AMD_FWD_LOSS_MW", 1);
    k->last_layer = lnn_env_int("LINNE_AMD_LAST_LAYER", 1);
    k->stats_rows = lnn_env_int("LINNE_AMD_STATS_ROWS", -1);
    { const char *e = getenv("LINNE_AMD_HIST"); k->hist = e ? (atoi(e) != 0) : -1; }
    k->rows8 = lnn_env_int("LINNE_AMD_DECODE_ROWS8", -1);
    k->decode_fused = lnn_env_int("LINNE_AMD_DECODE_FUSED", 1);
    { const char *e = getenv("LINNE_AMD_DECODE_KERNEL"); k->decode_kernel = !e ? 0 : (strcmp(e, "wave") == 0 ? 1 : (strcmp(e, "pipe") == 0 ? 3 : (strcmp(e, "rows") == 0 ? 4 : 2))); }
    /* LINNE_AMD_STREAMS per call: a call may use fewer compute sub-streams than the context created (bench.py times one step on
     * one stream so that its per-kernel spans do not overlap); it cannot use more */
    k->streams = lnn_env_int("LINNE_AMD_STREAMS", 0);
    if (k->streams < 0) k->streams = 0;
#ifdef LNN_TIMING_EXPERIMENTS       /* builds for timing experiments only (make EXPERIMENTS=1): with these set the results are WRONG */
    k->dbg_maxtr = (uint32_t)lnn_env_int("LINNE_AMD_DBG_MAXTR", 0);
    k->nostats = lnn_env_int("LINNE_AMD_DBG_NOSTATS", 0);
#else
    k->dbg_maxtr = 0; k->nostats = 0;
#endif
}

/* the compute sub-streams a context creates at its first encode call: LINNE_AMD_STREAMS, two by default, none for 1 (the analysis
 * then always runs on the context's own stream, as small batches do anyway); *forced: the variable was given */
static inline int lnn_context_streams(int *forced)
{
    const char *env = getenv("LINNE_AMD_STREAMS");
    int ns = env ? atoi(env) : 2;
    *forced = env != NULL;
    if (ns < 1) ns = 1;
    if (ns > LNN_MAXSUB) ns = LNN_MAXSUB;
    return ns >= 2 ? ns : 0;
}

/* ------------------------------------------------------------------------------------------------
 * class bookkeeping of an encode call
 * ---------------------------------------------------------------------------------------------- */
static inline double lnn_welch_div(uint32_t unit_samples) { return 4.0 * pow((double)(unit_samples - 1u), -2.0); }                         /* lpc.c:199 */

/* one length class: analysis length, the unit counts each layer may try, their Welch divisors (host libm, lpc.c:199) and
 * the offsets of its tables */
static inline void lnn_make_class(const HostShape *hs, uint32_t S, uint32_t n, uint64_t *sin_total, uint64_t *wt_total, DevClass *out)
{
    DevClass c; memset(&c, 0, sizeof(c));
    c.n = n;
    uint32_t na = ((n + 7u) / 8u) * 8u;             /* linne_encoder.c:652-654 */
    if (na < hs->maxP) na = hs->maxP;
    if (na > S) na = S;
    c.na = na;
    c.sin_off = (uint32_t)*sin_total; *sin_total += n;
    for (uint32_t l = 0; l < hs->L; l++) {
        const uint32_t maxu = hs->P[l] < 128u ? hs->P[l] : 128u;    /* linne_network.c:586,594 */
        uint32_t nt = 0;
        for (uint32_t u = 1; u <= maxu; u <<= 1) {
            if ((hs->P[l] % u) != 0 || (na % u) != 0) continue;      /* linne_network.c:291-294 */
            c.trial_u[l][nt] = u;
            c.trial_div[l][nt] = lnn_welch_div(na / u);                   /* lpc.c:199 */
            c.wt_off[l][nt] = (uint32_t)*wt_total;
            { const uint32_t pu = hs->P[l] / u; *wt_total += na / u + (pu > 4 ? pu : 4); *wt_total = (*wt_total + 3u) & ~(uint64_t)3u; }   /* tables start 32-byte aligned */
            nt++;
        }
        c.ntrials[l] = nt;
    }
    *out = c;
}

/* The resident class table of a context.  It is CUMULATIVE: a length seen in an earlier call of the same shape keeps its slot, so a
 * caller that alternates between batches with and without a ragged tail (a pipelined stream, chunk after chunk) uploads tables once
 * per new length and never again. */
struct LnnClassTable { DevClass cls[LNN_MAXCLS]; struct LINNEAmdShape shape; int valid; uint32_t ncls; uint64_t sin_total, wt_total; };
enum { LNN_CLS_FIRST = 0, LNN_CLS_REUSE = 1, LNN_CLS_APPEND = 2, LNN_CLS_RESTART_SHAPE = 3, LNN_CLS_RESTART_OVERFLOW = 4 };
enum { LNN_CLS_OK = 0, LNN_CLS_BAD_LENGTH = 1, LNN_CLS_TOO_MANY = 2 };
struct LnnCallClasses {
    int error; uint32_t error_frame;    /* LNN_CLS_BAD_LENGTH: the frame whose length is 0 or above the block */
    int branch;                         /* what became of the resident table (LNN_CLS_*); anything but REUSE: its tables go to the device again */
    uint32_t nlen, lens[LNN_MAXCLS], slot_of[LNN_MAXCLS];       /* the distinct lengths of the call in order of first appearance, and their slots */
    uint32_t na_max;                    /* largest analysis length of the call */
    int prod_ok;                        /* bit l: layer l's lags may come from k_autocorr_prod (short layers) / k_autocorr_wide (long ones) */
};

/* The classes of one call and the class-sorted order the kernels work in: sorted row i is the caller's frame map[i]; rows of one
 * class are contiguous (stable: the caller's order inside a class), so that whatever the order of lengths in the batch -- many tracks
 * back to back, each with its ragged tail -- a chunk has at most one run per class and the lanes = rows kernels see class-homogeneous
 * blocks.  idx, map, raw: F words each (idx and map back to back in the caller's buffer; raw is scratch).  Returns out->error. */
static inline int lnn_call_classes(LnnClassTable *tab, const struct LINNEAmdShape *shape, const HostShape *hs, const LnnKnobs *k,
        const uint32_t *h_num_samples, uint32_t F, uint32_t *idx, uint32_t *map, uint32_t *raw, LnnCallClasses *out)
{
    const uint32_t S = shape->num_samples_per_block;
    uint32_t *lens = out->lens, *slot_of = out->slot_of, nlen = 0;
    memset(out, 0, sizeof(*out));
    /* pass 1: the distinct lengths of this call (raw[f] = index into lens[]) */
    {
        uint32_t last_n = 0, last_k = 0;
        for (uint32_t f = 0; f < F; f++) {
            const uint32_t n = h_num_samples ? h_num_samples[f] : S;
            if (n == 0 || n > S) { out->error_frame = f; return out->error = LNN_CLS_BAD_LENGTH; }
            uint32_t kk = last_k;
            if (n != last_n || nlen == 0) {
                for (kk = 0; kk < nlen; kk++) if (lens[kk] == n) break;
                if (kk == nlen) {
                    if (nlen == LNN_MAXCLS) return out->error = LNN_CLS_TOO_MANY;
                    lens[nlen++] = n;
                }
                last_n = n; last_k = kk;
            }
            raw[f] = kk;
        }
    }
    out->nlen = nlen;
    /* the resident table: keep it if it has (room for) every length of this call, else start over with this call's lengths */
    const bool same_shape = tab->valid && memcmp(&tab->shape, shape, sizeof(*shape)) == 0;
    uint32_t missing = 0;
    for (uint32_t kk = 0; kk < nlen; kk++) {
        uint32_t j = 0;
        if (same_shape) for (; j < tab->ncls; j++) if (tab->cls[j].n == lens[kk]) break;
        slot_of[kk] = (same_shape && j < tab->ncls) ? j : 0xFFFFFFFFu;
        if (slot_of[kk] == 0xFFFFFFFFu) missing++;
    }
    out->branch = LNN_CLS_REUSE;
    if (missing) {
        out->branch = LNN_CLS_APPEND;
        if (!same_shape || tab->ncls + missing > LNN_MAXCLS) {
            out->branch = same_shape ? LNN_CLS_RESTART_OVERFLOW : (tab->valid ? LNN_CLS_RESTART_SHAPE : LNN_CLS_FIRST);
            tab->ncls = 0; tab->sin_total = 0; tab->wt_total = 0;
            memset(tab->cls, 0, sizeof(tab->cls));
            for (uint32_t kk = 0; kk < nlen; kk++) slot_of[kk] = 0xFFFFFFFFu;
        }
        for (uint32_t kk = 0; kk < nlen; kk++) if (slot_of[kk] == 0xFFFFFFFFu) {
            lnn_make_class(hs, S, lens[kk], &tab->sin_total, &tab->wt_total, &tab->cls[tab->ncls]);
            slot_of[kk] = tab->ncls++;
        }
        tab->shape = *shape; tab->valid = 1;        /* (the caller invalidates the table if its upload fails) */
    }
    /* pass 2: class slots in order of first appearance in this call, stable counting sort by class
     * (LINNE_AMD_SORT=0: the caller's order, for tests of the mixed-run fallback) */
    for (uint32_t kk = 0; kk < nlen; kk++) if (tab->cls[slot_of[kk]].na > out->na_max) out->na_max = tab->cls[slot_of[kk]].na;
    if (k->sort == 0) { for (uint32_t f = 0; f < F; f++) { idx[f] = slot_of[raw[f]]; map[f] = f; } }
    else {
        uint32_t count[LNN_MAXCLS + 1];
        memset(count, 0, sizeof(count));
        for (uint32_t f = 0; f < F; f++) count[raw[f] + 1]++;
        for (uint32_t kk = 0; kk < nlen; kk++) count[kk + 1] += count[kk];
        for (uint32_t f = 0; f < F; f++) { const uint32_t pos = count[raw[f]]++; idx[pos] = slot_of[raw[f]]; map[pos] = f; }
    }
    /* short layers by products (k_autocorr_prod): all trials present and every unit length even, in every class of this call */
    for (uint32_t l = 0; l < hs->L; l++) {
        if (hs->P[l] > 16u || !k->l0_products) continue;
        uint32_t nt = 0; for (uint32_t u = 1; u <= hs->P[l]; u <<= 1) nt++;
        int ok = 1;
        for (uint32_t kk = 0; kk < nlen; kk++) { const DevClass &c = tab->cls[slot_of[kk]]; if (c.ntrials[l] != nt || (c.na % (1u << nt)) != 0) ok = 0; }
        if (ok) out->prod_ok |= 1 << l;
    }
    /* long layers by lanes = lags (k_autocorr_wide): a small batch (at most 64 rows), and every unit length of every trial a class has even */
    for (uint32_t l = 0; l < hs->L; l++) {
        if (hs->P[l] < 32u || hs->P[l] > 128u || !k->wide || (uint64_t)F * shape->num_channels * (l == 0 ? 1u : hs->R) > 64u) continue;
        int ok = 1;
        for (uint32_t kk = 0; kk < nlen; kk++) { const DevClass &c = tab->cls[slot_of[kk]]; if (c.ntrials[l] == 0 || (c.na % (1u << c.ntrials[l])) != 0) ok = 0; }
        if (ok) out->prod_ok |= 1 << l;
    }
    return LNN_CLS_OK;
}

/* RowRuns of a chunk of frames whose rows are `rpf` per frame */
static inline void lnn_build_runs(RowRuns *rr, const uint32_t *idx, uint32_t F, uint32_t rpf)
{
    uint32_t n = 0, f = 0;
    rr->row_begin[0] = 0; rr->blk_begin[0] = 0;
    while (f < F) {
        uint32_t g = f + 1;
        while (g < F && idx[g] == idx[f]) g++;
        if (n == LNN_MAXRUN) { n = 0; break; }                  /* too many runs: one run over everything */
        rr->row_begin[n + 1] = g * rpf;
        rr->blk_begin[n + 1] = rr->blk_begin[n] + ((g - f) * rpf + 63u) / 64u;
        n++; f = g;
    }
    rr->mixed = 0;
    if (n == 0) { n = 1; rr->mixed = 1; rr->row_begin[1] = F * rpf; rr->blk_begin[1] = (F * rpf + 63u) / 64u; }
    rr->n = n;
}

/* ------------------------------------------------------------------------------------------------
 * the split of an encode call: frame groups ("chunks") rotate over nsub streams, each with its own slice of the arena
 * ---------------------------------------------------------------------------------------------- */
struct LnnSplit { uint32_t nsub; uint64_t part_bytes, chunk; bool streams_forced, use_sub; };
/* ctx_nsub: the compute sub-streams the context created; ctx_forced: LINNE_AMD_STREAMS was given when it created them */
static inline LnnSplit lnn_call_split(uint64_t arena_bytes, uint64_t per_frame, uint32_t num_frames, uint32_t C, uint32_t R,
        int ctx_nsub, bool ctx_forced, const LnnKnobs *k)
{
    LnnSplit s;
    uint32_t nsub = ctx_nsub > 0 ? (uint32_t)ctx_nsub : 1u;
    s.streams_forced = ctx_forced || k->streams > 0;
    if (k->streams > 0 && (uint32_t)k->streams < nsub) nsub = (uint32_t)k->streams;
    while (nsub > 1 && ((arena_bytes - 65536) / nsub < per_frame * 2 || num_frames < nsub * 512u)) nsub--;
    /* By default a call is cut in two only if each half still fills the chip and keeps every large-batch kernel form (the chunk rules
     * go by the jobs of a chunk: k_fwd_loss from 24 576): the halves' latency-bound kernels (Levinson-Durbin, the short layers' search,
     * the selections) then run beside the other half's vector-unit-bound ones -- 83.1 -> 80.1 ms per step on the 60-minute batch
     * (tools/streams_ab.sh).  Smaller batches keep one stream and the context's own (no fork / join around a block-at-a-time call). */
    if (!s.streams_forced) while (nsub > 1 && (uint64_t)(num_frames / nsub) * C * R < 32768u) nsub--;
    s.nsub = nsub;
    s.part_bytes = ((arena_bytes - 65536) / nsub) & ~(uint64_t)255;
    uint64_t chunk = s.part_bytes / per_frame;
    if (chunk == 0) chunk = 1;
    {   /* even split over the streams; every kernel carries the job index in grid.x: J = chunk * C * R is kept below 2^22 */
        const uint64_t even = (num_frames + nsub - 1) / nsub;
        if (chunk > even) chunk = even;
        const uint64_t lim = 4194304u / ((uint64_t)C * R);
        if (chunk > lim) chunk = lim;
        /* chunks of equal size (a multiple of the stream count): a small last chunk would run the latency-bound kernels
         * nearly empty */
        uint64_t nchunks = (num_frames + chunk - 1) / chunk;
        nchunks = ((nchunks + nsub - 1) / nsub) * nsub;
        chunk = (num_frames + nchunks - 1) / nchunks;
    }
    s.chunk = chunk;
    s.use_sub = ctx_nsub > 0 && (nsub > 1 || (s.streams_forced && k->streams != 1));
    return s;
}

/* block-type statistics.  Batches: lanes = channel-frames (k_stats_rows); a few channel-frames: a block each (k_stats finishes one
 * block sooner).  LINNE_AMD_STATS_ROWS forces either; the rows form needs 16-byte rows and a layer 0 of 2 or 4 taps */
static inline bool lnn_stats_rows_form(const LnnKnobs *k, uint32_t num_frames, uint32_t C, uint32_t S, uint32_t P0)
{
    const bool rows_form = k->stats_rows >= 0 ? (k->stats_rows != 0) : ((uint64_t)num_frames * C >= 1024u);
    return rows_form && (S & 3u) == 0 && (P0 == 2u || P0 == 4u);
}

/* ------------------------------------------------------------------------------------------------
 * the forms of one encode chunk
 * ---------------------------------------------------------------------------------------------- */
struct LnnLevLaunch { uint32_t t, u, threads, ride; size_t lds; };        /* one k_levinson_lds launch: trial t, u units of order P / u */
struct LnnLayerForms {
    bool fir_spec;                      /* the search also writes the one-unit trial's forward output; the forward pass skips those jobs */
    bool hist_layer, hist_all;          /* lanes = jobs lag kernels launched / they take every frame of the chunk (no general kernel then) */
    bool beside;                        /* the general lag kernel runs beside them on the side stream */
    bool lev_wave;                      /* k_levinson_wave: all trials in one launch */
    bool lev_inline;                    /* ... the same launches in the same order, but lev[0] on the chunk's own stream (LINNE_AMD_LEV_BESIDE=2: what the forms cost without the overlap) */
    bool lev_beside;                    /* lev[0] (order 128, no riders) runs on the chunk's sibling stream beside k_autocorr_hist<P,1> and the small-LDS k_autocorr_sub */
    uint32_t lev_carrier;               /* index in lev[] of the launch the riding waves go with: 0, or 1 when lev_beside (LNN_MAXT: none rides) */
    uint32_t nlev; LnnLevLaunch lev[LNN_MAXT];          /* else: these k_levinson_lds launches */
    bool last_layer;                    /* k_last_layer + k_select(2), nothing else of this layer's search and loss */
    bool long_any, long_all;            /* k_search_long is launched / takes every frame (no other search kernel then) */
    uint32_t long_mask;                 /* bit s: k_search_long takes the frames of class slot s */
    int search_form;                    /* k_search_long: 2 one block per job, two passes; 1 (jobs, tiles) blocks, two passes; 0 one pass */
    bool fir_small;                     /* the other search kernel is k_fir_small (else k_fir2<2>, per leftover run when long_any) */
    bool sel_wave;                      /* k_select_wave for k_fir2<0>'s fallback and the selection */
    bool fwd_loss, fwd_loss_mw;         /* k_fwd_loss / its five-wave form after the selection */
    bool forward, forward_walk;         /* k_fir2<1> is launched / one block per job walks the tiles */
};
struct LnnChunkForms {
    bool fwd_loss_on, fuse_cfg, fuse_all, last_layer_all, prep_defer, hist;
    uint32_t present;                   /* bit s: the chunk holds frames of class slot s */
    bool chain_sum, chain_sum_wave;     /* the last layer's loss by k_chain_sum / a wave per row */
    bool cascade_walk;                  /* k_fir_cascade: one block per channel-frame walks its tiles */
    LnnLayerForms layer[LNN_MAXL];
};
struct LnnChunkIn {
    const HostShape *hs; uint32_t C, S, Fc;
    const DevClass *cls; const uint32_t *idx;           /* the resident classes; class slot of each of the chunk's Fc frames */
    const LnnKnobs *k; bool use_sub, has_side; uint32_t af_iters, learning;
    bool final_pass;                    /* the real final pass of -a N: one job per channel-frame, general kernels, no lanes = jobs forms */
};

static inline void lnn_chunk_forms(const LnnChunkIn *in, LnnChunkForms *cf)
{
    const HostShape &hs = *in->hs; const LnnKnobs &k = *in->k;
    const uint32_t S = in->S, Fc = in->Fc, L = hs.L, Plast = hs.P[L - 1];
    const bool fin = in->final_pass;
    const uint64_t CF = (uint64_t)Fc * in->C, J = CF * (fin ? 1u : hs.R);
    memset(cf, 0, sizeof(*cf));
    for (uint32_t f = 0; f < Fc; f++) cf->present |= 1u << in->idx[f];
    /* per class slot in the chunk: which lanes = jobs kernels would take its frames, were their form switched on */
    LnnPlanView pv; memset(&pv, 0, sizeof(pv));
    pv.L = L; pv.S = S; pv.hist = 1; pv.fused_last = 1; pv.search_long = k.search_long ? 1u : 0u;
    for (uint32_t l = 0; l < L; l++) pv.P[l] = hs.P[l];
    uint32_t fwd_mask = 0, lastnt_mask = 0, hist_mask[LNN_MAXL] = { 0, 0, 0 }, long_mask[LNN_MAXL] = { 0, 0, 0 };
    for (uint32_t s = 0; s < LNN_MAXCLS; s++) if ((cf->present >> s) & 1u) {
        const DevClass &c = in->cls[s];
        if (fwd_loss_takes(pv, L - 1, c.na)) fwd_mask |= 1u << s;
        if (c.ntrials[L - 1] == lnn_all_trials(Plast)) lastnt_mask |= 1u << s;
        for (uint32_t l = 0; l < L; l++) {
            if (hist_takes(pv, l, c)) hist_mask[l] |= 1u << s;
            if (search_long_takes(pv, l, c)) long_mask[l] |= 1u << s;
        }
    }
    /* The lanes = jobs kernels need a batch that fills the chip with 64-job waves: below ~24 k jobs (k_fwd_loss: one wave per
     * 64 jobs) / ~12 k jobs (k_autocorr_hist: one block per 64 jobs and trial) the block-per-job kernels finish sooner --
     * a single stereo frame takes 2.6 ms with them, 6.2 ms without this rule.  The environment forces either form. */
    cf->fwd_loss_on = !fin && ((k.fwd_loss < 0) ? (J >= 24576u) : (k.fwd_loss != 0));
    /* last layer: forward pass + loss in one kernel for the jobs it takes (fwd_loss_takes); the two-kernel form runs only
     * when the chunk holds frames it does not take */
    cf->fuse_cfg = cf->fwd_loss_on && L > 1 && (Plast == 2u || Plast == 4u || Plast == 8u || Plast == 16u);
    cf->fuse_all = cf->fuse_cfg && (cf->present & ~fwd_mask) == 0;
    /* k_last_layer (search + forward pass + loss of the last layer in one launch) takes a chunk whole or not at all: every frame
     * k_fwd_loss's and with every trial (LINNE_AMD_EXACT keeps the certified search's exact fallback in use: that knob compares the two) */
    /* (from 49 152 jobs on, or when LINNE_AMD_LAST_LAYER=2 says always: with lanes = jobs and a wave per 64 of them a chunk of J jobs is
     * J / 64 waves on 1024 SIMDs, and a lone wave walks its frames in 4.1 ms however few they are -- the 31 008 jobs of a group of
     * EncodeWhole took 4.1 ms here and 1.8 in the three kernels: 108 -> 110.5 ms per 60-minute stream) */
    /* (a chunk alone on the GPU has nothing beside its lone waves: it pays from ~78 k jobs on -- 124 k x 4.1 / 6.6) */
    /* (the every-trial term cannot fail once fuse_all holds -- an analysis length that is a multiple of 4 x P divides by every unit count
     * up to P -- it states what the kernel relies on) */
    cf->last_layer_all = cf->fuse_all && k.last_layer && !k.force_exact && !in->af_iters && !in->learning
            && (J >= (in->use_sub ? 49152u : 81920u) || (k.last_layer == 2 && J > 256u)) && (cf->present & ~lastnt_mask) == 0;
    /* (k_prep_slow addresses xtmp with 32-bit byte offsets) */
    cf->prep_defer = k.prep_defer && !k.prep_general && (S & 3u) == 0 && CF * S * sizeof(int32_t) <= 0xFFFFFFFFull;
    RowRuns rr; lnn_build_runs(&rr, in->idx, Fc, in->C * hs.R);
    cf->hist = !fin && (k.hist >= 0 ? (k.hist != 0) : (J >= 12288u));
    if (rr.mixed) cf->hist = false;                            /* more class runs than RowRuns holds: blocks may mix classes, which only the general kernels serve */
    const uint32_t tiles = (S + LNN_FIR_TILE - 1) / LNN_FIR_TILE;
    for (uint32_t l = 0; l < L; l++) {
        LnnLayerForms &lf = cf->layer[l];
        const uint32_t P = hs.P[l], maxu = P < 128u ? P : 128u;
        const bool last = l + 1 == L;
        /* the first two layers nearly always keep one unit: their search pass also writes that trial's forward output */
        lf.fir_spec = !fin && k.fir_spec && !last;
        lf.hist_layer = cf->hist && P >= 64u;
        lf.hist_all = cf->hist && (cf->present & ~hist_mask[l]) == 0;   /* (hist_mask holds only layers of >= 64 taps) */
        /* the general kernels serve what the lanes = jobs kernels do not take -- usually one ragged frame, a launch that is
         * all latency: it runs beside them on the side stream */
        lf.beside = lf.hist_layer && !lf.hist_all && in->has_side;
        /* Levinson-Durbin.  A handful of jobs: a wave per problem, all trials in one launch.  Else one launch per trial, every
         * order on LDS columns -- except that the short trials whose columns fit beside the one-unit trial's ride along with it on
         * a second wave (k_levinson_lds) */
        lf.lev_wave = J <= 64u && k.lev_wave;
        lf.lev_carrier = LNN_MAXT;
        if (!lf.lev_wave) {
            uint32_t ride = LNN_MAXT;
            for (uint32_t t = 1, u = 2; u <= maxu && k.lev_ride; u <<= 1, t++)
                if (LEV_LDS(P) + LNN_LEV_MAXRIDE * LEV_LDS(P / u) <= LEV_LDS_BUDGET) { ride = t; break; }
            /* The order-128 launch is one 130 KB block per CU, a lone wave on one of its four SIMDs: 2.8 ms of the 60-minute step with
             * the chip nearly empty.  It needs only trial 0's lags (k_autocorr_hist<P,0>), so it runs on the chunk's sibling stream
             * beside k_autocorr_hist<P,1> and k_autocorr_sub, whose small-LDS form (LNN_SUB_SMALL_LDS) fits in the 31 232 bytes the
             * solver leaves.  The riding waves need k_autocorr_sub's lags: they move to the trial-1 launch.  Only where the lanes = jobs lag
             * kernels run (hist_layer), only for order 128 (an order-64 solver block is 67 KB: the lag kernels fit beside it as
             * they are), and only for a chunk whose solver has more than a block per CU to hide -- LNN_LEV_BESIDE_MIN jobs.
             * Measured (profiles/ab_lev_beside.txt; two streams, three alternating runs each against the build without the form, every
             * run with the form ahead of every run without): the 60-minute batch, two chunks of 62 016 jobs, 70.56 -> 69.01 ms per
             * step; a 32-minute batch, two chunks of 33 076 jobs -- the smallest a two-stream call makes are 32 768 (lnn_call_split) --
             * 40.83 -> 40.25.  The threshold is that smallest two-stream chunk: a smaller chunk runs alone on one stream, where the
             * overlap gave 0.2-0.5 ms at 124 032 jobs and was not measured below; a group of EncodeWhole (31 008 jobs) and block-at-a-
             * time calls keep the launches they had.  The forms alone cost 0.67 ms of the 60-minute step (LINNE_AMD_LEV_BESIDE=2: the
             * riders with the trial-1 launch, the 16-position tiles of k_autocorr_sub), the overlap gives 2.2 back.
             * LINNE_AMD_LEV_BESIDE=0/1 forces the size term either way. */
            const bool beside_size = k.lev_beside >= 0 ? (k.lev_beside != 0) : (LNN_LEV_BESIDE_DEFAULT && J >= LNN_LEV_BESIDE_MIN);
            lf.lev_beside = beside_size && lf.hist_layer && P == 128u && in->has_side && ride >= 2u && ride < LNN_MAXT
                    && LEV_LDS(P / 2u) + LNN_LEV_MAXRIDE * LEV_LDS(P >> ride) <= LEV_LDS_BUDGET && LEV_LDS(P) + LNN_SUB_SMALL_LDS <= LEV_LDS_BUDGET;
            lf.lev_inline = lf.lev_beside && k.lev_beside == 2;
            if (ride < LNN_MAXT) lf.lev_carrier = lf.lev_beside ? 1u : 0u;
            for (uint32_t t = 0, u = 1; u <= maxu && t < (ride < LNN_MAXT ? ride : LNN_MAXT); u <<= 1, t++) {
                const bool carry = (t == lf.lev_carrier);
                LnnLevLaunch &v = lf.lev[lf.nlev++];
                v.t = t; v.u = u;
                v.lds = LEV_LDS(P / u) + (carry ? LNN_LEV_MAXRIDE * LEV_LDS(P >> ride) : 0);
                v.threads = carry ? 64 * (1 + LNN_LEV_MAXRIDE) : 64;
                v.ride = carry ? ride : (uint32_t)LNN_MAXT;
            }
        }
        /* the last layer of a chunk k_last_layer takes: search, selection, forward pass and loss from one pass over the input */
        lf.last_layer = cf->last_layer_all && last;
        if (!lf.last_layer) {
            /* unit-count search.  Short layers: the register-window kernel.  The long layer: k_search_long for the frames it takes
             * (search_long_takes), k_fir2<2> for the others (it returns at once for the jobs taken there) */
            lf.long_mask = (lf.fir_spec && !fin) ? long_mask[l] : 0u;
            lf.long_any = (cf->present & lf.long_mask) != 0;
            lf.long_all = (cf->present & ~lf.long_mask) == 0;
            /* one block per job that walks its tiles (coefficients, bookkeeping and reductions once per job) where the jobs alone
             * are at least SEARCH_JOB_MIN; (jobs, tiles) blocks below that.  The one-pass kernel has the latter form only. */
            const bool per_job = k.search_two && (k.search_job < 0 ? J >= LNN_SEARCH_JOB_MIN : k.search_job != 0);
            lf.search_form = per_job ? 2 : (k.search_two ? 1 : 0);
            lf.fir_small = P <= 16u && k.fir_small;
            lf.sel_wave = J <= 256u && (uint64_t)tiles * LNN_FIR_WAVES <= LNN_SELW_MAXPART;       /* a handful of jobs: a wave per job */
            /* the last layer's output is only ever summed: layers of <= 16 taps do the forward pass and the ordered loss in one
             * kernel and write nothing else */
            lf.fwd_loss = last && cf->fuse_cfg;
            /* fewer than 1024 waves of 64 jobs: each would be alone on its SIMD (1.4 ms per launch however few) -- five waves per 64 jobs then (k_fwd_loss_mw) */
            lf.fwd_loss_mw = lf.fwd_loss && J < 65536u && k.fwd_loss_mw;
        }
        /* the final pass needs no output of the last layer: only its parameters */
        lf.forward = !(fin && last) && !(last && cf->fuse_all);
        lf.forward_walk = lf.forward && lf.fir_spec && J >= 4096u;      /* forward pass in batches: a block per job walks the tiles (few jobs have any work) */
    }
    cf->chain_sum = !fin && !cf->fuse_all;
    cf->chain_sum_wave = cf->chain_sum && J <= 1024u;          /* few rows: a wave per row */
    cf->cascade_walk = CF >= 1024u;
}

/* the frames k_search_long leaves -- usually the one ragged tail -- are runs of consecutive rows (the chunk is sorted by class): the
 * next such run [*f, *g) at or after frame `from` of the chunk, false when there is none */
static inline bool lnn_next_left_run(const LnnLayerForms *lf, const uint32_t *idx, uint32_t Fc, uint32_t from, uint32_t *f, uint32_t *g)
{
    uint32_t a = from;
    while (a < Fc && ((lf->long_mask >> idx[a]) & 1u)) a++;
    if (a >= Fc) return false;
    uint32_t b = a + 1;
    while (b < Fc && !((lf->long_mask >> idx[b]) & 1u)) b++;
    *f = a; *g = b;
    return true;
}

/* ------------------------------------------------------------------------------------------------
 * the forms of a decode call
 * ---------------------------------------------------------------------------------------------- */
enum { LNN_DEC_LAYERS = 0, LNN_DEC_WAVE = 1, LNN_DEC_PIPE = 2 };
enum { LNN_DL_FUSED_L0 = 0, LNN_DL_ROWS = 1, LNN_DL_ROWS8 = 2, LNN_DL_SMALL = 3, LNN_DL_BIG = 4, LNN_DL_GENERAL = 5 };
struct LnnDecLayer {
    int form;                           /* LNN_DL_* */
    int nch;                            /* k_synth_rows<NCH>: 0 short layer, 1 / 3 / 7 for 32 / 64 / 128 taps */
    uint32_t pb;                        /* taps the instantiation is built for: rows<0, 4> (0: its default), rows8<4 | 8 | 16>, small<P>, big<P> */
    bool de;                            /* layer 0: the de-emphasis comes with it (fused_l0, small) or behind it (rows: k_deemph_lr) */
    bool ms_fold;                       /* ... and MS -> LR with the de-emphasis, no k_ms_to_lr */
};
struct LnnDecodeForms { int call; LnnDecLayer layer[LNN_MAXL]; bool ms_separate; };
/* rows_ptr_ok: the samples lie 16-byte aligned; pipe_fits: a frame fits k_synth_pipe's LDS image */
static inline void lnn_decode_forms(const HostShape *hs, uint32_t C, uint32_t S, uint32_t ms, uint32_t num_frames, bool rows_ptr_ok, bool pipe_fits,
        const LnnKnobs *k, LnnDecodeForms *df)
{
    memset(df, 0, sizeof(*df));
    const uint32_t CF = num_frames * C;
    /* The lanes = channel-frames kernels have few, long-running waves: a pass over a short layer takes the time of one
     * wave's 10240-step recurrence however small the batch.  Below a few thousand channel-frames the one-wave-per-
     * channel-frame kernel (all layers and the de-emphasis in one launch) finishes sooner. */
    /* LINNE_AMD_DECODE_KERNEL = "wave" / "lanes" / "pipe": for tests and measurements.  Small batches -- block-at-a-time calls
     * above all -- take the pipelined latency form (k_synth_pipe: a wave per stage of the cascade, 16-sample blocks) when the
     * frame fits its LDS image; k_synthesize is its fallback for longer frames */
    /* (tools/decode_crossover.py: the pipelined form costs 0.85 ms per 1024 channel-frames, the throughput form 1.25 ms up to ~4000 and
     * 0.12 per 1024 beyond: they cross at 1536; the lanes form the throughput form falls back to, 5.1 ms whatever the batch: at 6144) */
    const bool rows_fit = (S & 3u) == 0u && rows_ptr_ok;
    const int form = k->decode_kernel ? k->decode_kernel : (CF < (rows_fit ? 1536u : 6144u) ? 3 : 0);
    const bool ms_foldable = ms && C >= 2u && C <= 64u && (C & (C - 1u)) == 0u;       /* a block of 64 rows holds whole frames */
    df->ms_separate = ms != 0;
    if (form == 3 && pipe_fits) { df->call = LNN_DEC_PIPE; return; }
    if (form == 1 || form == 3) { df->call = LNN_DEC_WAVE; return; }
    df->call = LNN_DEC_LAYERS;
    for (uint32_t l = 0; l < hs->L; l++) {
        LnnDecLayer &d = df->layer[l];
        const uint32_t P = hs->P[l];
        d.de = (l == 0);
        /* k_synth_rows (four channel-frames per wave, the old taps on the matrix unit) takes the layers without de-emphasis whose
         * order is a preset's, when the samples can travel as 16-byte groups (LINNE_AMD_DECODE_KERNEL=lanes: none) */
        d.nch = P <= 16u ? 0 : (P == 32u ? 1 : (P == 64u ? 3 : (P == 128u ? 7 : -1)));
        if (d.de && d.nch == 0 && form != 2 && rows_fit && P <= 4u && k->decode_fused) {
            /* the end of the cascade in ONE launch: layer 0, the de-emphasis and MS -> LR on tiles in LDS (lnn_k_decode_fused.h) */
            d.form = LNN_DL_FUSED_L0; d.ms_fold = ms_foldable;
        } else if (d.nch >= 0 && form != 2 && rows_fit) {
            d.form = LNN_DL_ROWS; d.pb = (d.nch == 0 && P <= 4u) ? 4u : 0u;
            /* (LINNE_AMD_DECODE_ROWS8=0 / 1: the four- / eight-channel-frame form whatever the batch; eight per wave are twice the blocks
             * per wave: they pay once the four-per-wave form fills the SIMDs, tools/decode_crossover.py) */
            if (d.nch == 0 && (k->rows8 < 0 ? CF >= 20480u : k->rows8 != 0)) { d.form = LNN_DL_ROWS8; d.pb = P <= 4u ? 4u : (P <= 8u ? 8u : 16u); }
            d.ms_fold = d.de && ms_foldable;            /* the de-emphasis behind layer 0 (k_deemph_lr), MS -> LR on its way out */
        } else {
            d.pb = P;
            d.form = (P == 2u || P == 4u || P == 8u || P == 16u) ? LNN_DL_SMALL : ((P == 32u || P == 64u || P == 128u) ? LNN_DL_BIG : LNN_DL_GENERAL);   /* general: not a preset size */
        }
        if (d.ms_fold) df->ms_separate = false;
    }
}
#endif
