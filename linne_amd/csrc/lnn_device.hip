/*
 * lnn_device.hip -- gfx950 (MI355X) kernels of the LINNE per-frame prediction path and their C-ABI
 * launchers (declared in include/linne_amd.h).
 *
 * Bit-exactness rules (DESIGN.md "Arithmetic contract"):
 *   - this TU is compiled with -ffp-contract=off: every double multiply and add is a separate, correctly
 *     rounded IEEE-754 operation, issued in the reference's order.  A sum that the reference evaluates as
 *     one chain is owned by ONE thread here; parallelism comes only from independent chains (lags, units,
 *     unit-count trials, regulariser passes, samples, channels, frames).
 *   - libm values the reference takes from glibc (Welch divisor pow(n-1,-2), the SIN window) are computed
 *     on the host and passed in as tables.
 *   - int32 filters use 32-bit wrap-around arithmetic (uint32 multiply/add, arithmetic shift).
 *
 * Citations are file:line under /root/reference.
 */
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <new>
#include <vector>

#include "linne_amd.h"
#include "lnn_common.h"
#include "lnn_host.h"
#include "linne_decoder.h"
#include "linne_encoder.h"

/* the kernels, in pipeline order */
#include "lnn_dev_common.h"             /* (brings lnn_forms.h: the shared structs, and which kernel form a call, a chunk, a layer gets) */
#include "lnn_k_prep.h"
#include "lnn_k_autocorr.h"
#include "lnn_k_levinson.h"
#include "lnn_k_fir.h"
#include "lnn_k_search.h"
#include "lnn_k_fwdloss.h"
#include "lnn_k_lastlayer.h"
#include "lnn_k_af.h"
#include "lnn_k_train.h"
#include "lnn_k_decode.h"
#include "lnn_k_decode_rows.h"
#include "lnn_k_decode_fused.h"
#include "lnn_k_finalize.h"
#include "lnn_k_rice.h"
#include "lnn_k_stream.h"
#include "lnn_k_index_batch.h"
#include "lnn_k_windows.h"              /* (brings lnn_windows_plan.h: the host's plan of a windows call) */
#include "lnn_k_compare.h"
#include "lnn_k_measure.h"
#include "lnn_k_digest.h"
#include "lnn_k_quiet.h"
#include "lnn_k_histogram.h"
#include "lnn_k_relate.h"
#include "lnn_k_mix.h"
#include "lnn_k_resample.h"
#include "lnn_k_overlay.h"
#include "lnn_k_lags.h"
#include "lnn_k_project.h"
#include "lnn_k_stream_enc.h"
#include "lnn_stream_batch.h"
#include "lnn_block_scan.h"             /* where the lists of the index's and the repair call's block-head scan lie */
#include "lnn_k_splice.h"              /* (brings lnn_splice.h: the host's plan of a splice call) */
#include "lnn_repair.h"                 /* the host's plan of a repair call */
#include "lnn_k_repair.h"
/* what lnn_forms.h knows of the kernels' tiling is the kernels' own */
/* the two timing kinds linne_amd.h numbers by their place behind kind 68 */
static_assert(LINNE_AMD_T_IB_HEADERS == 69 && LINNE_AMD_T_IB_BEHIND == 70, "the index batch's timing kinds are 69 and 70");
static_assert(LINNE_AMD_SPLICE_T_COPY == 71 && LINNE_AMD_SPLICE_T_HEADER == 72, "the splice call's timing kinds are 71 and 72");
static_assert(LINNE_AMD_REPAIR_T_SOUND == 73 && LINNE_AMD_REPAIR_T_RUNS == 78, "the repair call's timing kinds are 73 to 78");
static_assert(LINNE_AMD_COMPARE_T_COMPARE == 79, "the compare call's timing kind is 79");
static_assert(LINNE_AMD_MEASURE_T_MEASURE == 80 && LINNE_AMD_MEASURE_T_COMMIT == 82, "the measure call's timing kinds are 80 to 82");
static_assert(LINNE_AMD_DIGEST_T_DIGEST == 83 && LINNE_AMD_DIGEST_T_COMMIT == 85, "the digest call's timing kinds are 83 to 85");
static_assert(LINNE_AMD_QUIET_T_QUIET == 86 && LINNE_AMD_QUIET_T_ENDS == 91 && LINNE_AMD_QUIET_EXTRA_LAUNCHES == 5, "the quiet call's timing kinds are 86 to 91: the pass kind and five launches per call");
static_assert(LINNE_AMD_HISTOGRAM_T_HISTOGRAM == 92 && LINNE_AMD_HISTOGRAM_T_COMMIT == 94, "the histogram call's timing kinds are 92 to 94");
static_assert(LINNE_AMD_RELATE_T_RELATE == 95 && LINNE_AMD_RELATE_T_COMMIT == 97, "the relate call's timing kinds are 95 to 97");
static_assert(LINNE_AMD_MIX_T_MIX == 98, "the mix call's timing kind is 98");
static_assert(LINNE_AMD_RESAMPLE_T_PRESET == 99 && LINNE_AMD_RESAMPLE_T_RESAMPLE == 100, "the resample call's timing kinds are 99 and 100");
static_assert(LINNE_AMD_OVERLAY_T_OVERLAY == 101, "the overlay call's timing kind is 101");
static_assert(LINNE_AMD_LAGS_T_LAGS == 102 && LINNE_AMD_LAGS_T_COMMIT == 103, "the lag call's timing kinds are 102 and 103");
static_assert(LINNE_AMD_PROJECT_T_PRESET == 104 && LINNE_AMD_PROJECT_T_PROJECT == 105, "the project call's timing kinds are 104 and 105");
static_assert(LNN_FIR_TILE == FIR_TILE && LNN_FIR_WAVES == FIR_THREADS / 64 && LNN_SELW_MAXPART == SELW_MAXPART && LNN_SEARCH_JOB_MIN == SEARCH_JOB_MIN && LNN_LEV_MAXRIDE == LEV_MAXRIDE, "lnn_forms.h and the kernels disagree");

/* ================================================================================================
 * host side of this TU: context, scratch arena, launch sequences, C-ABI
 * ============================================================================================== */
#define LNN_RICE_STREAMS 4
struct LINNEAmdContext {
    int device;
    hipStream_t stream; int own_stream;
    void *arena; uint64_t arena_bytes;
    char err[256];
    int timing;
    uint32_t na_max;                    /* largest analysis length of the current batch */
    hipEvent_t ev[2]; int ev_valid;
    /* per-kernel spans of the last call (timing enabled): HIP events on the launch stream */
    hipEvent_t *span_ev; int *span_kind; int nspans, span_cap;
    /* cached class tables */
    uint32_t *d_ucount;
    /* frame groups of one call rotate over these streams so that the latency-bound phases of one group (short
     * layers, Levinson, ordered sums) overlap the throughput-bound phases of another */
    hipStream_t sub[LNN_MAXSUB]; hipEvent_t sub_done[LNN_MAXSUB]; hipEvent_t ev_start; int nsub, nsub_forced /* LINNE_AMD_STREAMS was given */;
    int enc_streams_done;
    hipStream_t side; hipEvent_t side_done; int has_side;     /* block-type statistics run beside the analysis */
    /* Sibling streams: what a chunk runs beside its own stream's work -- the general autocorrelation kernel for the few frames the lanes =
     * jobs kernels do not take, and the long layer's order-128 Levinson launch (LnnLayerForms.lev_beside).  Two of them, sib[0] the side
     * stream: the chunk in stream slot s forks to sib[s & 1], so that a call keeps at most four streams busy (two halves, a sibling
     * each).  Events per slot: the halves of a call never share a pair. */
    hipStream_t sib[2]; int sib1_tried;
    hipEvent_t fork_ev[LNN_MAXSUB], join_ev[LNN_MAXSUB], lev_fork_ev[LNN_MAXSUB], lev_join_ev[LNN_MAXSUB];
    DevClass *d_cls; double *d_sin; uint64_t sin_cap; double *d_wt; uint64_t wt_cap; uint32_t *d_clsidx; uint64_t clsidx_cap; uint32_t *d_map;   /* class index per sorted row, then the sorted row's frame (same buffer) */ uint32_t *d_nsmp; uint64_t nsmp_cap;
    /* what the resident class tables were built for: a call with the same shape and frame lengths re-uses them */
    LnnClassTable tab;
    /* pinned ring for the per-call frame metadata (class index, length), so that a call enqueues without a host sync */
    int last_search_form;               /* the form of the call's last k_search_long launch: 0 (jobs, tiles), 1 per job, -1 none (LINNEAmd_GetLastSearchLongForm) */
    const uint32_t *cur_idx;            /* class index per frame of the call being enqueued (host copy, in the meta ring) */
    uint32_t *meta_h[LNN_META]; uint64_t meta_cap[LNN_META]; hipEvent_t meta_ev[LNN_META]; int meta_used[LNN_META]; int meta_next;
    /* copy streams of the staging slots (H2D of the next group and D2H of the previous one overlap the kernels) */
    hipStream_t copy_in, copy_out; int has_copy;
    /* decode slots in stream mode: the Rice decoders of a stream's groups run side by side on these (a launch is a few dozen waves
     * walking their blocks for ~8 ms), the slots take them in turn */
    hipStream_t rice_pool[LNN_RICE_STREAMS]; int n_rice_pool, rice_next;
    uint32_t *d_plan_nsmp; uint64_t plan_nsmp_cap; double rice_steps[32]; uint32_t rice_nsteps;
    int prod_ok;                        /* set per batch by build_classes, bit l: in layer l every class has all its trials and even unit lengths (k_autocorr_prod) */
    uint32_t learning;                  /* -l: the SGD trainer after the analysis (LINNEAmd_SetLearning), 0 = off */
    uint32_t af_iters;                  /* -a N: auxiliary-function iterations of the final pass (LINNEAmd_SetAfIterations), 0 = off */
    double *af_h; uint32_t af_h_cap;    /* pinned: a Cholesky step's pivots on their way through the host's pow() */
    int pcm16_next;                     /* the next EncodeFramesDevice call reads narrow samples: 1 int16, 2 packed 3-byte (set by the staging slots, cleared by the call) */
    int capture_on;                     /* LINNEAmd_SetSearchCapture: the encode calls leave what k_select decided from (tests; off: Plan.capture is NULL) */
    double *d_capture; uint64_t capture_cap, capture_n;      /* its records on the device: capacity, and those of the last call */
    void *sdec; uint64_t sdec_cap;      /* the windows calls: the buffers of one pass (wx_scratch).  The block-head scan (IbScan): its rows' counts and offsets */
    void *senc; uint64_t senc_cap;      /* scratch of EncodeStreamDevice: the buffers of one pass */
    void *wdec; uint64_t wdec_cap;      /* the windows calls: fail words, window and block records of one call.  The block-head scan: its lists (lnn_block_scan.h) */
    void *wstage; uint64_t wstage_cap;  /* pinned: the same lists on the host, at the same offsets; what the device answers comes back into it */
    int64_t senc_count[4];              /* the last EncodeStreamDevice call: COMPRESS, SILENT, RAW blocks, host-settled Rice plans */
    int64_t sbatch_count[3];            /* the last EncodeStreamsDevice call: shape groups, passes, EncodeFramesDevice calls */
    void *xcand; uint64_t xcand_cap;    /* behind the block-head scan, laid out by its caller: StreamIndexesCreate's candidates and pointer-doubling levels; RepairStreamsDevice's, with its sound candidates, chain blocks and run records */
    int64_t ibatch_count[5];            /* the last StreamIndexesCreate call: streams, indexes built, K, host synchronisations, device allocations */
    int span_keep;                      /* EncodeFramesDevice inside EncodeStream(s)Device: keep the call's spans and start event */
    double rice_guard;                  /* guard band of k_rice_plan (0: LNN_RICE_GUARD); set by EncodeStreamDevice's test knob */
    void *hstage; uint64_t hstage_cap;  /* device staging of the host-buffer forms (EncodeFramesHost / DecodeFramesHost: block-at-a-time calls), kept between calls */
    void *spl; uint64_t spl_cap;        /* SpliceStreamsDevice: the fragments' PCM and scratch streams, then the run table and the headers of one call.  RepairStreamsDevice: its run table and fill bytes */
    void *spl_stage; uint64_t spl_stage_cap;    /* pinned: the run table and what lies behind it on the host, uploaded in one copy; RepairStreamsDevice fetches its run records into it first */
    int64_t splice_count[6];            /* the last SpliceStreamsDevice call: outputs written, copied blocks, re-encoded blocks, copy runs, bytes copied, its own host synchronisations */
    int outer_keep;                     /* DecodeWindowsDevice / EncodeStreamsDevice inside SpliceStreamsDevice: keep the call's spans and start event */
    int64_t repair_count[7];            /* the last RepairStreamsDevice call: outputs written, kept blocks, fill blocks, gaps, copy runs, host synchronisations, kernel launches */
    struct LINNEAmdGap *rp_gaps; uint64_t *rp_gap0; uint32_t rp_streams;     /* its gaps, stream i's are [rp_gap0[i], rp_gap0[i + 1]) (LINNEAmd_GetLastRepairGaps; host memory) */
    LnnKnobs knob;                      /* every form-selecting knob (lnn_forms.h): some read when the context is created, the others at the top of each call */
};

#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { snprintf((ctx)->err, sizeof((ctx)->err), "%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); return LNN_NG; } } while (0)

static const uint32_t k_layers_a[] = { 2, 32 }, k_layers_b[] = { 4, 64, 8 }, k_layers_c[] = { 4, 128, 16 };
static const double k_regs_1[] = { 0.0 }, k_regs_2[] = { 0.0, 1.0 / 512.0 }, k_regs_4[] = { 0.0, 1.0 / 2048.0, 1.0 / 512.0, 1.0 / 128.0 };

extern "C" int lnn_preset_info(uint32_t preset, uint32_t *num_layers, uint32_t *layers, uint32_t *num_regs, double *regs)
{   /* libs/linne_internal/src/linne_internal.c:16-41 */
    const uint32_t *L; const double *R; uint32_t nl, nr;
    if (preset >= 8) return -1;
    if (preset < 2) { L = k_layers_a; nl = 2; } else if (preset < 5) { L = k_layers_b; nl = 3; } else { L = k_layers_c; nl = 3; }
    switch (preset) { case 0: case 2: case 5: R = k_regs_1; nr = 1; break; case 1: case 3: case 6: R = k_regs_2; nr = 2; break; default: R = k_regs_4; nr = 4; }
    if (num_layers) *num_layers = nl;
    if (layers) for (uint32_t i = 0; i < nl; i++) layers[i] = L[i];
    if (num_regs) *num_regs = nr;
    if (regs) for (uint32_t i = 0; i < nr; i++) regs[i] = R[i];
    return 0;
}

/* A HIP stream is multiplexed onto one of a few hardware queues -- four per process by default -- and streams that share a
 * queue execute in submission order whatever their events allow.  A context pipelines over four streams (analysis, block-type
 * statistics, copy-in, copy-out) next to whatever the host application uses (torch has its own); when copy-in and copy-out
 * shared a queue, the H2D of group g + 1 sat behind the Rice emission of group g, which waits for the analysis of g: the
 * staging pipeline ran serially (measured: 28 ms per group instead of 23).  The runtime reads GPU_MAX_HW_QUEUES when it
 * initialises, i.e. at the first HIP call of the process; loading this library comes before that.  A value the user set is
 * left alone.  Round 4 tried more: DecodeWhole keeps eight groups in flight, and with a stream per slot 8 queues were too few -- a
 * slot's stream shared one with the copy-out stream and its Rice decoder started 3 ms late behind another group's D2H
 * (profiles/r04_decode_timeline.txt; 55 ms per 60-minute stream with 8 queues, 42 with 16, 37 with 24) -- but with 24 queues
 * EncodeWhole lost a quarter of its rate inside a process that holds other contexts (bench.py: 142 k -> 107 k frames/s, every
 * kernel of the analysis 6 % slower: profiles/r04_encode_whole_queues.txt).  So the count stays at 8 and the decoder asks for LESS:
 * its context creates no encode-side streams (ctx_encode_streams) and four pooled streams carry the Rice decoders
 * (LNN_RICE_STREAMS), so that what runs side by side in a decode -- synthesis, copy-in, copy-out, four decoders -- are seven streams
 * created one after the other: seven different queues out of eight. */
__attribute__((constructor)) static void lnn_more_hw_queues(void) { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

extern "C" int LINNEAmd_GetDeviceCount(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* The streams only the ENCODE side uses -- the compute sub-streams of a large call and the side stream of the block-type statistics --
 * are created at the first encode call, not with the context: a stream takes the next of the process's few hardware queues in turn
 * (GPU_MAX_HW_QUEUES), and a decoder's context that never encodes should not push its own streams -- the synthesis, the copy-out, the
 * Rice decoders -- onto queues that collide (round 4: DecodeWhole's Rice decoders started milliseconds late behind another group's D2H). */
static int ctx_encode_streams(LINNEAmdContext *ctx)
{
    if (ctx->enc_streams_done) return LNN_OK;
    ctx->enc_streams_done = 1;
    {
        int forced = 0;
        const int ns = lnn_context_streams(&forced);     /* (two by default since round 3: see lnn_call_split) */
        ctx->nsub_forced = forced;
        /* One stream of a process maps onto one of a few hardware queues (four by default); streams that share a queue run in
         * order whatever their events say.  A context therefore creates as few streams as it needs: two compute sub-streams
         * (LINNE_AMD_STREAMS=1: none -- the analysis then always runs on the context's own stream, as small batches do anyway). */
        ctx->nsub = 0;
        for (int i = 0; i < ns; i++) {
            if (hipStreamCreateWithFlags(&ctx->sub[i], hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ctx->sub_done[i], hipEventDisableTiming) != hipSuccess) break;
            ctx->nsub++;
        }
        const bool have_start = hipEventCreateWithFlags(&ctx->ev_start, hipEventDisableTiming) == hipSuccess;
        if (!have_start) ctx->nsub = 0;
        ctx->has_side = have_start && hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking) == hipSuccess
                && hipEventCreateWithFlags(&ctx->side_done, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < LNN_MAXSUB && ctx->has_side; i++)
            ctx->has_side = hipEventCreateWithFlags(&ctx->fork_ev[i], hipEventDisableTiming) == hipSuccess
                    && hipEventCreateWithFlags(&ctx->join_ev[i], hipEventDisableTiming) == hipSuccess
                    && hipEventCreateWithFlags(&ctx->lev_fork_ev[i], hipEventDisableTiming) == hipSuccess
                    && hipEventCreateWithFlags(&ctx->lev_join_ev[i], hipEventDisableTiming) == hipSuccess;
        /* (the second sibling is created when a chunk first sends its Levinson launch there -- sibling_for_levinson: a context whose calls
         * stay below that size keeps the streams, and so the hardware queues, it always had) */
        if (ctx->has_side) { ctx->sib[0] = ctx->side; ctx->sib[1] = ctx->side; }
    }
    return LNN_OK;
}

extern "C" struct LINNEAmdContext *LINNEAmd_ContextCreate(int device, uint64_t scratch_bytes)
{
    int n = 0;
    hipError_t e;
#define CC_FAIL(what) do { fprintf(stderr, "liblinne_amd: ContextCreate(device=%d): %s: %s\n", device, what, hipGetErrorString(e)); } while (0)
    if ((e = hipGetDeviceCount(&n)) != hipSuccess) { CC_FAIL("hipGetDeviceCount"); return NULL; }
    if (n <= 0 || device < 0 || device >= n) { fprintf(stderr, "liblinne_amd: ContextCreate(device=%d): %d HIP device(s) visible\n", device, n); return NULL; }
    if ((e = hipSetDevice(device)) != hipSuccess) { CC_FAIL("hipSetDevice"); return NULL; }
    LINNEAmdContext *ctx = (LINNEAmdContext *)calloc(1, sizeof(*ctx));
    if (!ctx) return NULL;
    ctx->device = device;
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) { CC_FAIL("hipStreamCreate"); free(ctx); return NULL; }
    ctx->own_stream = 1;
    if (scratch_bytes == 0) scratch_bytes = 6ull << 30;
    if ((e = hipMalloc(&ctx->arena, scratch_bytes)) != hipSuccess) { CC_FAIL("hipMalloc(arena)"); hipStreamDestroy(ctx->stream); free(ctx); return NULL; }
    ctx->arena_bytes = scratch_bytes;
    if ((e = hipMalloc((void **)&ctx->d_cls, sizeof(DevClass) * LNN_MAXCLS)) != hipSuccess) { CC_FAIL("hipMalloc(classes)"); hipFree(ctx->arena); hipStreamDestroy(ctx->stream); free(ctx); return NULL; }
    if ((e = hipMalloc((void **)&ctx->d_ucount, 4 * sizeof(uint32_t))) != hipSuccess) { CC_FAIL("hipMalloc(counter)"); }
    lnn_knobs_read_context(&ctx->knob); ctx->last_search_form = -1;
    (void)hipFuncSetAttribute((const void *)k_levinson_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LEV_LDS_BUDGET);
    (void)hipFuncSetAttribute((const void *)k_synth_pipe, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LEV_LDS_BUDGET);
    if ((e = hipEventCreate(&ctx->ev[0])) != hipSuccess || (e = hipEventCreate(&ctx->ev[1])) != hipSuccess) { CC_FAIL("hipEventCreate"); }
#undef CC_FAIL
    return ctx;
}

extern "C" void LINNEAmd_ContextDestroy(struct LINNEAmdContext *ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (ctx->arena) hipFree(ctx->arena);
    if (ctx->d_cls) hipFree(ctx->d_cls);
    if (ctx->d_ucount) hipFree(ctx->d_ucount);
    if (ctx->d_capture) hipFree(ctx->d_capture);
    for (int i = 0; i < ctx->nsub; i++) { hipStreamSynchronize(ctx->sub[i]); hipStreamDestroy(ctx->sub[i]); hipEventDestroy(ctx->sub_done[i]); }
    if (ctx->ev_start) hipEventDestroy(ctx->ev_start);
    if (ctx->has_side && ctx->sib[1] != ctx->side) { hipStreamSynchronize(ctx->sib[1]); hipStreamDestroy(ctx->sib[1]); }
    if (ctx->has_side) { hipStreamSynchronize(ctx->side); hipStreamDestroy(ctx->side); hipEventDestroy(ctx->side_done); }
    for (int i = 0; i < LNN_MAXSUB; i++) {
        if (ctx->fork_ev[i]) hipEventDestroy(ctx->fork_ev[i]);
        if (ctx->join_ev[i]) hipEventDestroy(ctx->join_ev[i]);
        if (ctx->lev_fork_ev[i]) hipEventDestroy(ctx->lev_fork_ev[i]);
        if (ctx->lev_join_ev[i]) hipEventDestroy(ctx->lev_join_ev[i]);
    }
    if (ctx->d_sin) hipFree(ctx->d_sin);
    if (ctx->d_wt) hipFree(ctx->d_wt);
    if (ctx->d_clsidx) hipFree(ctx->d_clsidx);
    if (ctx->d_nsmp) hipFree(ctx->d_nsmp);
    if (ctx->d_plan_nsmp) hipFree(ctx->d_plan_nsmp);
    if (ctx->hstage) hipFree(ctx->hstage);
    if (ctx->sdec) hipFree(ctx->sdec);
    if (ctx->senc) hipFree(ctx->senc);
    if (ctx->wdec) hipFree(ctx->wdec);
    if (ctx->xcand) hipFree(ctx->xcand);
    if (ctx->spl) hipFree(ctx->spl);
    if (ctx->spl_stage) hipHostFree(ctx->spl_stage);
    if (ctx->wstage) hipHostFree(ctx->wstage);
    if (ctx->af_h) hipHostFree(ctx->af_h);
    for (int i = 0; i < LNN_META; i++) { if (ctx->meta_h[i]) hipHostFree(ctx->meta_h[i]); if (ctx->meta_ev[i]) hipEventDestroy(ctx->meta_ev[i]); }
    for (int i = 0; i < ctx->n_rice_pool; i++) { hipStreamSynchronize(ctx->rice_pool[i]); hipStreamDestroy(ctx->rice_pool[i]); }
    if (ctx->has_copy) { hipStreamSynchronize(ctx->copy_in); hipStreamSynchronize(ctx->copy_out); hipStreamDestroy(ctx->copy_in); hipStreamDestroy(ctx->copy_out); }
    hipEventDestroy(ctx->ev[0]); hipEventDestroy(ctx->ev[1]);
    for (int i = 0; i < 2 * ctx->span_cap; i++) hipEventDestroy(ctx->span_ev[i]);
    free(ctx->span_ev); free(ctx->span_kind);
    if (ctx->own_stream) hipStreamDestroy(ctx->stream);
    free(ctx->rp_gaps); free(ctx->rp_gap0);
    free(ctx);
}

extern "C" const char *LINNEAmd_GetLastError(const struct LINNEAmdContext *ctx) { return ctx ? ctx->err : "no context"; }

extern "C" int LINNEAmd_SetStream(struct LINNEAmdContext *ctx, void *hip_stream)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream) { HIPCHK(ctx, hipStreamDestroy(ctx->stream)); ctx->own_stream = 0; }
    ctx->stream = (hipStream_t)hip_stream;              /* NULL is the device's default (null) stream */
    return LNN_OK;
}

extern "C" int LINNEAmd_ReserveScratch(struct LINNEAmdContext *ctx, uint64_t bytes)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    if (ctx->arena_bytes >= bytes) return LNN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    void *fresh = NULL;
    if (hipMalloc(&fresh, bytes) != hipSuccess) { (void)hipGetLastError(); snprintf(ctx->err, sizeof(ctx->err), "cannot reserve %llu bytes of scratch", (unsigned long long)bytes); return LNN_NG; }
    if (ctx->arena) HIPCHK(ctx, hipFree(ctx->arena));
    ctx->arena = fresh; ctx->arena_bytes = bytes;
    return LNN_OK;
}

extern "C" int64_t LINNEAmd_GetLastFallbackCount(struct LINNEAmdContext *ctx)
{
    if (!ctx) return -1;
    uint32_t v = 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess
            || hipMemcpy(&v, ctx->d_ucount, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
}

extern "C" double LINNEAmd_GetLastMinMargin(struct LINNEAmdContext *ctx)
{
    if (!ctx) return -1.0;
    double v = -1.0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess
            || hipMemcpy(&v, ctx->d_ucount + 2, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
    return v;
}

extern "C" int LINNEAmd_SetSearchCapture(struct LINNEAmdContext *ctx, int enable)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->capture_on = enable ? 1 : 0;
    return LNN_OK;
}

extern "C" int64_t LINNEAmd_GetLastSearchCapture(struct LINNEAmdContext *ctx, double *host, uint64_t capacity_records)
{
    if (!ctx) return -1;
    const uint64_t n = ctx->capture_n < capacity_records ? ctx->capture_n : capacity_records;
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
    if (n && (!host || hipMemcpy(host, ctx->d_capture, n * LNN_CAP_WORDS * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)) return -1;
    return (int64_t)ctx->capture_n;
}

extern "C" int LINNEAmd_Synchronize(struct LINNEAmdContext *ctx)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LNN_OK;
}

extern "C" int LINNEAmd_SetLearning(struct LINNEAmdContext *ctx, uint32_t enable)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->learning = enable ? 1u : 0u;
    return LNN_OK;
}
extern "C" int LINNEAmd_SetAfIterations(struct LINNEAmdContext *ctx, uint32_t iterations)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->af_iters = iterations;
    return LNN_OK;
}
extern "C" int LINNEAmd_EnableTiming(struct LINNEAmdContext *ctx, int enable) { if (!ctx) return LNN_INVALID_ARGUMENT; ctx->timing = enable; return LNN_OK; }
/* span bookkeeping: span_begin/span_end bracket one kernel launch with events when timing is on */
static int span_begin(LINNEAmdContext *ctx, int kind, hipStream_t st)
{
    if (!ctx->timing) return -1;
    if (ctx->nspans == ctx->span_cap) {
        const int ncap = ctx->span_cap ? ctx->span_cap * 2 : 256;
        hipEvent_t *ne = (hipEvent_t *)realloc(ctx->span_ev, sizeof(hipEvent_t) * 2 * ncap);
        if (!ne) return -1;
        ctx->span_ev = ne;
        int *nk = (int *)realloc(ctx->span_kind, sizeof(int) * ncap);
        if (!nk) return -1;
        ctx->span_kind = nk;
        for (int i = 2 * ctx->span_cap; i < 2 * ncap; i++) if (hipEventCreate(&ctx->span_ev[i]) != hipSuccess) return -1;
        ctx->span_cap = ncap;
    }
    const int id = ctx->nspans++;
    ctx->span_kind[id] = kind;
    (void)hipEventRecord(ctx->span_ev[2 * id], st);
    return id;
}
static void span_end(LINNEAmdContext *ctx, int id, hipStream_t st) { if (id >= 0) (void)hipEventRecord(ctx->span_ev[2 * id + 1], st); }

extern "C" double LINNEAmd_GetLastTimingMs(struct LINNEAmdContext *ctx, int which)
{
    if (!ctx || which < 0) return -1.0;
    if (which == 0) {
        float ms = -1.0f;
        if (!ctx->ev_valid) return -1.0;
        if (hipEventSynchronize(ctx->ev[1]) != hipSuccess || hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) != hipSuccess) return -1.0;
        return ms;
    }
    double sum = 0.0; int cnt = 0;
    for (int i = 0; i < ctx->nspans; i++) if (ctx->span_kind[i] == which) {
        float ms = 0.0f;
        if (hipEventSynchronize(ctx->span_ev[2 * i + 1]) != hipSuccess || hipEventElapsedTime(&ms, ctx->span_ev[2 * i], ctx->span_ev[2 * i + 1]) != hipSuccess) return -1.0;
        sum += ms; cnt++;
    }
    return cnt ? sum : -1.0;
}
extern "C" int LINNEAmd_GetLastSearchLongForm(struct LINNEAmdContext *ctx) { return ctx ? ctx->last_search_form : -1; }
extern "C" int LINNEAmd_GetLastTimingLaunches(struct LINNEAmdContext *ctx, int which)
{
    if (!ctx) return 0;
    int cnt = 0;
    for (int i = 0; i < ctx->nspans; i++) if (ctx->span_kind[i] == which) cnt++;
    return cnt;
}

/* What a call counts of its own work, each in a slot of its *_count[]: waits for the stream, device allocations, kernel launches.
 * A NULL slot, or no tally at all, counts nothing. */
struct LnnTally { int64_t *waits, *allocs, *launches; };
static inline void tally_launch(const LnnTally *t) { if (t && t->launches) ++*t->launches; }
static int tally_wait(LINNEAmdContext *ctx, const LnnTally *t)
{
    if (t && t->waits) ++*t->waits;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LNN_OK;
}

/* a buffer of the context, device or pinned, that holds `need` bytes from here on: one that grows waits for the stream first */
static int ensure_buf(LINNEAmdContext *ctx, void **ptr, uint64_t *cap, uint64_t need, bool pinned = false, const LnnTally *t = NULL)
{
    if (*cap >= need) return LNN_OK;
    if (t && t->allocs) ++*t->allocs;
    const int ret = tally_wait(ctx, t);
    if (ret != LNN_OK) return ret;
    if (*ptr) HIPCHK(ctx, pinned ? hipHostFree(*ptr) : hipFree(*ptr));
    *ptr = NULL; *cap = 0;
    if (pinned) HIPCHK(ctx, hipHostMalloc(ptr, need, hipHostMallocDefault)); else HIPCHK(ctx, hipMalloc(ptr, need));
    *cap = need;
    return LNN_OK;
}

/* the stream parameters a header names */
static struct LINNEAmdShape header_shape(const struct LINNEHeader *h)
{
    struct LINNEAmdShape s;
    s.num_channels = h->num_channels; s.bits_per_sample = h->bits_per_sample; s.num_samples_per_block = h->num_samples_per_block;
    s.preset = h->preset; s.ch_process_method = (uint32_t)h->ch_process_method;
    return s;
}

static int shape_info(const struct LINNEAmdShape *s, HostShape *h)
{
    if (!s || s->preset >= 8 || s->num_channels == 0 || s->num_channels > LNN_MAXCH || s->bits_per_sample == 0 || s->bits_per_sample > 32
            || s->num_samples_per_block == 0 || s->ch_process_method > 1 || (s->ch_process_method == 1 && s->num_channels < 2)) return LNN_INVALID_FORMAT;
    lnn_preset_info(s->preset, &h->L, h->P, &h->R, h->regs);
    uint32_t off = 0; h->maxP = 0;
    for (uint32_t l = 0; l < h->L; l++) { h->coef_off[l] = off; off += h->P[l]; if (h->P[l] > h->maxP) h->maxP = h->P[l]; }
    for (uint32_t l = 0; l < h->L; l++) if (s->num_samples_per_block <= h->P[l]) return LNN_INVALID_FORMAT;   /* linne_encoder.c:176-181 */
    return LNN_OK;
}

/* next buffer of the pinned metadata ring, holding at least 4 * F words; waits for the copy that last read it */
static int meta_acquire(LINNEAmdContext *ctx, uint32_t F, int *m_out)
{
    const int m = ctx->meta_next;
    ctx->meta_next = (m + 1) % LNN_META;
    if (ctx->meta_used[m]) { HIPCHK(ctx, hipEventSynchronize(ctx->meta_ev[m])); ctx->meta_used[m] = 0; }
    if (!ctx->meta_ev[m]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->meta_ev[m], hipEventDisableTiming));
    if (ctx->meta_cap[m] < 4ull * F) {
        const uint64_t cap = 4ull * (F < 4096u ? 4096u : F);
        if (ctx->meta_h[m]) { HIPCHK(ctx, hipHostFree(ctx->meta_h[m])); ctx->meta_h[m] = NULL; ctx->meta_cap[m] = 0; }
        HIPCHK(ctx, hipHostMalloc((void **)&ctx->meta_h[m], sizeof(uint32_t) * cap, hipHostMallocDefault));
        ctx->meta_cap[m] = cap;
    }
    *m_out = m;
    return LNN_OK;
}

/* a call's per-frame lengths into dst[F] (NULL: every frame is a whole block); a length of 0 or beyond the block size is refused */
static int copy_lengths(LINNEAmdContext *ctx, const struct LINNEAmdShape *shape, const uint32_t *h_num_samples, uint32_t F, uint32_t *dst)
{
    const uint32_t S = shape->num_samples_per_block;
    for (uint32_t f = 0; f < F; f++) {
        const uint32_t n = h_num_samples ? h_num_samples[f] : S;
        if (n == 0 || n > S) { snprintf(ctx->err, sizeof(ctx->err), "frame %u: num_samples %u out of range", f, n); return LNN_INVALID_ARGUMENT; }
        dst[f] = n;
    }
    return LNN_OK;
}

/* frame lengths of a decode call: the synthesis kernels need nothing but each frame's length (any number of distinct
 * lengths: a stream written by EncodeBlock calls of varying num_samples, linne_decoder.c:671-742), so no class tables
 * are built and the encode side's resident tables stay valid */
static int upload_lengths(LINNEAmdContext *ctx, const struct LINNEAmdShape *shape, const uint32_t *h_num_samples, uint32_t F)
{
    int m, ret;
    if ((ret = meta_acquire(ctx, F, &m)) != LNN_OK) return ret;
    uint32_t *nsm = ctx->meta_h[m];
    if ((ret = copy_lengths(ctx, shape, h_num_samples, F, nsm)) != LNN_OK) return ret;
    if ((ret = ensure_buf(ctx, (void **)&ctx->d_nsmp, &ctx->nsmp_cap, sizeof(uint32_t) * (uint64_t)(F ? F : 1))) != LNN_OK) return ret;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_nsmp, nsm, sizeof(uint32_t) * F, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->meta_ev[m], ctx->stream));
    ctx->meta_used[m] = 1;
    return LNN_OK;
}

/* The libm values of the path, behind names of their own so that a test can compare the box's libm with the committed
 * values of the build container (tests/golden/libm_values.json): were they ever to differ, the test names the cause where the
 * parity tests would only show hashes that do not match. */
extern "C" double lnn_welch_divisor(uint32_t unit_samples) { return lnn_welch_div(unit_samples); }                        /* lpc.c:199 */
extern "C" double lnn_sin_window(uint32_t s, uint32_t n) { return sin((3.1415926535897932384626433832795029 * s) / (n - 1)); }            /* lpc.c:192 */
extern "C" double lnn_cholesky_pivot(double sum) { return pow(sum, -0.5); }                                                                /* lpc.c:421 */

/* Builds the per-length classes of an encode batch and the class-sorted order the kernels work in (lnn_call_classes has the
 * bookkeeping), fills the tables of new classes (host libm values) and uploads them: only a call with a new length
 * synchronises the host.  The per-frame class index and the map go through a pinned ring. */
static int build_classes(LINNEAmdContext *ctx, const struct LINNEAmdShape *shape, const HostShape *hs,
        const uint32_t *h_num_samples, uint32_t F)
{
    int m, ret;
    { const int r_ = meta_acquire(ctx, F, &m); if (r_ != LNN_OK) return r_; }
    uint32_t *idx = ctx->meta_h[m], *map = ctx->meta_h[m] + F, *raw = ctx->meta_h[m] + 2 * (size_t)F;
    ctx->cur_idx = idx;
    LnnClassTable &tab = ctx->tab;
    LnnCallClasses cc;
    switch (lnn_call_classes(&tab, shape, hs, &ctx->knob, h_num_samples, F, idx, map, raw, &cc)) {
    case LNN_CLS_BAD_LENGTH: snprintf(ctx->err, sizeof(ctx->err), "frame %u: num_samples %u out of range", cc.error_frame, h_num_samples[cc.error_frame]); return LNN_INVALID_ARGUMENT;
    case LNN_CLS_TOO_MANY: snprintf(ctx->err, sizeof(ctx->err), "more than %d distinct frame lengths in one batch", LNN_MAXCLS); return LNN_INVALID_ARGUMENT;
    default: break;
    }
    ctx->na_max = cc.na_max; ctx->prod_ok = cc.prod_ok;
    if (cc.branch != LNN_CLS_REUSE) {
        /* (re)build and upload the tables of every resident class */
        const uint64_t sin_total = tab.sin_total, wt_total = tab.wt_total;
        double *sintab = (double *)malloc(sizeof(double) * (sin_total ? sin_total : 1));
        double *wt = (double *)calloc(wt_total ? wt_total : 1, sizeof(double));
        if (!sintab || !wt) { free(sintab); free(wt); tab.valid = 0; tab.ncls = 0; snprintf(ctx->err, sizeof(ctx->err), "out of host memory"); return LNN_NG; }
        for (uint32_t k = 0; k < tab.ncls; k++) {
            const DevClass &c = tab.cls[k];
            const uint32_t n = c.n;
            for (uint32_t s = 0; s < n; s++) sintab[c.sin_off + s] = lnn_sin_window(s, n);   /* lpc.c:192 */
            /* Welch weights per trial over one padded unit (lpc.c:199-204): w[loc] = (div * h) * (n-1-h), h = min(loc, n-1-loc);
             * zero in the zero zone; the (never written) middle of an odd unit is handled on the device (Q1) */
            for (uint32_t l = 0; l < hs->L; l++)
                for (uint32_t t = 0; t < c.ntrials[l]; t++) {
                    const uint32_t u = c.trial_u[l][t], nu = c.na / u;
                    const double div = c.trial_div[l][t];
                    double *w = wt + c.wt_off[l][t];
                    for (uint32_t loc = 0; loc < nu; loc++) {
                        const uint32_t h = (loc < (nu >> 1)) ? loc : (nu - 1 - loc);
                        w[loc] = div * (double)h * (double)(nu - 1 - h);
                    }
                }
        }
        /* the old tables may still be read by work enqueued on the sub-streams / side stream of an earlier call */
        hipError_t e = hipDeviceSynchronize();
        ret = (e == hipSuccess) ? ensure_buf(ctx, (void **)&ctx->d_sin, &ctx->sin_cap, sizeof(double) * (sin_total ? sin_total : 1)) : LNN_NG;
        if (ret == LNN_OK) ret = ensure_buf(ctx, (void **)&ctx->d_wt, &ctx->wt_cap, sizeof(double) * (wt_total ? wt_total : 1));
        if (ret != LNN_OK) { free(sintab); free(wt); tab.valid = 0; tab.ncls = 0; return ret; }
        e = hipMemcpyAsync(ctx->d_sin, sintab, sizeof(double) * sin_total, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_wt, wt, sizeof(double) * wt_total, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_cls, tab.cls, sizeof(DevClass) * LNN_MAXCLS, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);          /* sintab / wt are freed here */
        free(sintab); free(wt);
        if (e != hipSuccess) { tab.valid = 0; tab.ncls = 0; snprintf(ctx->err, sizeof(ctx->err), "class table upload: %s", hipGetErrorString(e)); return LNN_NG; }
    }
    if ((ret = ensure_buf(ctx, (void **)&ctx->d_clsidx, &ctx->clsidx_cap, sizeof(uint32_t) * 2 * (uint64_t)(F ? F : 1))) != LNN_OK) return ret;
    ctx->d_map = ctx->d_clsidx + F;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_clsidx, idx, sizeof(uint32_t) * 2 * (size_t)F, hipMemcpyHostToDevice, ctx->stream));    /* class index and map, back to back */
    HIPCHK(ctx, hipEventRecord(ctx->meta_ev[m], ctx->stream));
    ctx->meta_used[m] = 1;
    return LNN_OK;
}

static uint64_t align_up(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }

/* bytes of scratch one frame needs (C channel-frames, R passes each) */
static uint64_t frame_scratch_bytes(const struct LINNEAmdShape *shape, const HostShape *hs, uint32_t af_iters = 0, uint32_t learning = 0)
{
    const uint64_t C = shape->num_channels, S = shape->num_samples_per_block, J = C * hs->R;
    uint64_t b = 0;
    b += 2 * C * S * sizeof(int32_t);
    b += J * 2 * S * sizeof(double);
    b += J * LNN_MAXT * LNN_ACW * sizeof(double);
    b += J * LNN_MAXT * LNN_MAXP * sizeof(double);
    b += J * LNN_MAXT * LNN_MAXU * (sizeof(double) + 1);
    b += J * LNN_MAXT * sizeof(double) * (1 + (uint64_t)((S + FIR_TILE - 1) / FIR_TILE) * (FIR_THREADS / 64)) + J;
    b += J * sizeof(double) * (uint64_t)((S + FIR_TILE - 1) / FIR_TILE) * (FIR_THREADS / 64) + 256;
    b += J * LNN_MAXT * sizeof(double) + 256;
    b += J * LNN_MAXL * LNN_MAXP * sizeof(double);
    b += J * LNN_MAXL * sizeof(uint32_t);
    b += J * 2 * sizeof(double);
    b += C * sizeof(uint32_t) + 512;                        /* k_prep_slow's list */
    if (af_iters)       /* the auxiliary-function pass: per channel-frame the normal matrices, reciprocals, vectors, problem lists */
        b += C * (sizeof(double) * ((uint64_t)hs->maxP * hs->maxP + S + 3 * LNN_MAXP + 3 * LNN_MAXU + 2) + sizeof(uint32_t) * (2 * LNN_MAXU + 1)) + 8192;
    if (af_iters || learning) b += C * (sizeof(uint32_t) + 2 * sizeof(double)) + 1024;        /* the winners of the search passes */
    if (learning)       /* the trainer: two layer inputs and a gradient-signal buffer per layer (TR_NBUF), gradients and momenta per channel-frame */
        b += C * (sizeof(double) * ((2 + LNN_MAXL) * S + 2 * LNN_MAXL * LNN_MAXP + 2) + sizeof(uint32_t)) + 4096;
    return b + 4096;
}

extern "C" uint64_t LINNEAmd_ScratchBytesPerFrame(const struct LINNEAmdShape *shape)
{
    HostShape hs;
    if (shape_info(shape, &hs) != LNN_OK) return 0;
    return frame_scratch_bytes(shape, &hs);
}

/* ------------------------------------------------------------------------------------------------
 * dispatch helpers: one per kernel family, from run-time orders and flags to the template instantiation
 * ---------------------------------------------------------------------------------------------- */
/* a kernel template over the order of a short layer (2 / 4 / 8 / 16 taps) */
#define LNN_BY_ORDER(P_, LAUNCH_) do { switch (P_) { case 2: LAUNCH_(2); break; case 4: LAUNCH_(4); break; case 8: LAUNCH_(8); break; default: LAUNCH_(16); break; } } while (0)
/* a kernel template over <layer 0 reads the int32 channel, the search writes / the forward skips the one-unit trial> */
#define LNN_BY_L0_SPEC(l0_, spec_, LAUNCH_) do { if (l0_) { if (spec_) LAUNCH_(true, true); else LAUNCH_(true, false); } else { if (spec_) LAUNCH_(false, true); else LAUNCH_(false, false); } } while (0)

/* k_fir2 launcher: layer 0 reads the int32 channel (L0); `spec` = the search also writes the one-unit trial's forward output
 * (MODE 2) / the forward pass skips the jobs that chose one unit (MODE 1) */
template <int MODE> static void launch_fir(hipStream_t st, const Plan &p, uint32_t l, uint32_t cur, uint32_t J, uint32_t grid_y, bool spec)
{
    const dim3 grid(J, grid_y), blk(FIR_THREADS);
#define LNN_F2(L0_, SPEC_) hipLaunchKernelGGL((k_fir2<MODE, L0_, SPEC_>), grid, blk, 0, st, p, l, cur)
    LNN_BY_L0_SPEC(l == 0, spec, LNN_F2);
#undef LNN_F2
}

/* search of a short layer (P <= 16): register-window kernel */
template <int PP> static void launch_fir_small_p(hipStream_t st, const Plan &p, uint32_t l, uint32_t cur, const dim3 grid, bool spec)
{
#define LNN_FS(L0_, SPEC_) hipLaunchKernelGGL((k_fir_small<PP, L0_, SPEC_>), grid, dim3(FIR_THREADS), 0, st, p, l, cur)
    LNN_BY_L0_SPEC(l == 0, spec, LNN_FS);
#undef LNN_FS
}
static void launch_fir_small_search(hipStream_t st, const Plan &p, uint32_t l, uint32_t cur, uint32_t J, uint32_t tiles, bool spec, uint32_t P)
{
    const dim3 grid(l == 0 ? J / p.R : J, tiles);      /* layer 0: one block serves the R jobs of a channel-frame */
#define LNN_FSP(PP_) launch_fir_small_p<PP_>(st, p, l, cur, grid, spec)
    LNN_BY_ORDER(P, LNN_FSP);
#undef LNN_FSP
}

static void launch_last_layer(hipStream_t st, const Plan &q, uint32_t l, uint32_t cur, uint32_t J)
{
#define LNN_LL(PP_) hipLaunchKernelGGL(k_last_layer<PP_>, dim3((J + 63) / 64), dim3(64), 0, st, q, l, cur)
    LNN_BY_ORDER(q.P[l], LNN_LL);
#undef LNN_LL
}

/* k_fwd_loss: a wave per 64 jobs; mw: its five-wave form */
static void launch_fwd_loss(hipStream_t st, const Plan &q, uint32_t l, uint32_t cur, uint32_t J, bool mw)
{
    const dim3 g((J + 63) / 64);
#define LNN_FLM(PP_) hipLaunchKernelGGL(k_fwd_loss_mw<PP_>, g, dim3(320), 0, st, q, l, cur)
#define LNN_FL(PP_) hipLaunchKernelGGL(k_fwd_loss<PP_>, g, dim3(64), 0, st, q, l, cur)
    if (mw) LNN_BY_ORDER(q.P[l], LNN_FLM); else LNN_BY_ORDER(q.P[l], LNN_FL);
#undef LNN_FLM
#undef LNN_FL
}

/* k_search_long<P, two passes, one block per job>; form: LnnLayerForms.search_form */
static void launch_search_long(hipStream_t st, const Plan &q, uint32_t l, uint32_t cur, uint32_t J, uint32_t tiles, int form)
{
    const dim3 grid(J, form == 2 ? 1u : tiles), blk(FIR_THREADS);
#define LNN_SL(TWO_, JOB_) do { if (q.P[l] == 128u) hipLaunchKernelGGL((k_search_long<128, TWO_, JOB_>), grid, blk, 0, st, q, l, cur); else hipLaunchKernelGGL((k_search_long<64, TWO_, JOB_>), grid, blk, 0, st, q, l, cur); } while (0)
    if (form == 2) LNN_SL(true, true); else if (form == 1) LNN_SL(true, false); else LNN_SL(false, false);
#undef LNN_SL
}

/* ------------------------------------------------------------------------------------------------
 * the encode call: what its launchers share, and the launchers in pipeline order
 * ---------------------------------------------------------------------------------------------- */
struct EncodeCall {             /* one LINNEAmd_EncodeFramesDevice call */
    const struct LINNEAmdShape *shape; HostShape hs; uint32_t C, S, num_frames, pcm16;
    const int32_t *d_pcm; int32_t *d_residual, *d_params; double *d_stats;
    LnnSplit split;
};
struct Chunk {                  /* one chunk of it on its stream */
    LINNEAmdContext *ctx; hipStream_t st; const HostShape *hs;
    hipStream_t sib; uint32_t slot;     /* its sibling stream (valid when the context has a side stream) and its stream slot: the index of its events */
    uint32_t C, S, f0, Fc; uint64_t CF, J;
    const uint32_t *idx;        /* class slot of each of its frames (host copy) */
    Plan p; LnnChunkForms forms;
    uint8_t *abase; uint64_t part_bytes;                /* its slice of the arena */
    uint32_t *af_best; double *af_loss, *af_reg; TrainArgs tr;
};
struct Pass {                   /* the layers of one pass over the jobs of plan q: the R search passes, or the real final pass of -a N */
    const Plan *q; const LnnChunkForms *forms; uint32_t J, af_iters;
    uint32_t cur;               /* which half of `sig` holds the current layer's input */
};

static void fill_plan(Plan &p, const EncodeCall &e, uint32_t F)
{
    memset(&p, 0, sizeof(p));
    p.C = e.C; p.S = e.S; p.bits = e.shape->bits_per_sample; p.L = e.hs.L; p.R = e.hs.R; p.F = F;
    for (uint32_t l = 0; l < e.hs.L; l++) p.P[l] = e.hs.P[l];
    p.scale = ldexp(1.0, -(int)(e.shape->bits_per_sample - 1));
    p.pcm = e.d_pcm; p.pcm16 = e.pcm16; p.stats = e.d_stats;
}

/* statistics of every frame of the call: one launch beside the analysis */
static int launch_stats(LINNEAmdContext *ctx, const EncodeCall &e)
{
    Plan ps; fill_plan(ps, e, e.num_frames);
    ps.cls_of_frame = ctx->d_clsidx; ps.frame_map = ctx->d_map; ps.cls = ctx->d_cls; ps.sintab = ctx->d_sin;
    hipStream_t ss = ctx->stream;
    if (ctx->has_side) { ss = ctx->side; HIPCHK(ctx, hipStreamWaitEvent(ss, ctx->ev_start, 0)); }
    if (!ctx->knob.nostats) {      /* (always, except in a build for timing experiments: without the statistics the block types are wrong) */
        const int sp_ = span_begin(ctx, LINNE_AMD_T_STATS, ss);
        if (lnn_stats_rows_form(&ctx->knob, e.num_frames, e.C, e.S, e.hs.P[0])) {
            const dim3 g((e.num_frames * e.C + 63u) / 64u);
#define LNN_SR(W_, T_) do { if (e.pcm16 == 1u) hipLaunchKernelGGL((k_stats_rows<W_, 1>), g, dim3(T_), 0, ss, ps); else if (e.pcm16 == 2u) hipLaunchKernelGGL((k_stats_rows<W_, 2>), g, dim3(T_), 0, ss, ps); else hipLaunchKernelGGL((k_stats_rows<W_, 0>), g, dim3(T_), 0, ss, ps); } while (0)
            if (e.hs.P[0] == 4u) LNN_SR(5, 320); else LNN_SR(3, 192);
#undef LNN_SR
        }
        else hipLaunchKernelGGL(k_stats, dim3(e.num_frames, e.C), dim3(STAT_THREADS), 0, ss, ps);
        span_end(ctx, sp_, ss);
    }
    if (ss != ctx->stream) HIPCHK(ctx, hipEventRecord(ctx->side_done, ss));
    return LNN_OK;
}

/* the chunk's plan, its forms and the carve-up of its slice of the arena */
static int chunk_setup(Chunk &k, LINNEAmdContext *ctx, const EncodeCall &e, uint32_t f0, uint32_t slot)
{
    const uint32_t S = e.S;
    k.ctx = ctx; k.hs = &e.hs; k.C = e.C; k.S = S; k.f0 = f0;
    k.st = e.split.use_sub ? ctx->sub[slot] : ctx->stream;
    k.slot = slot; k.sib = ctx->sib[slot & 1u];
    k.Fc = (e.num_frames - f0 < e.split.chunk) ? (e.num_frames - f0) : (uint32_t)e.split.chunk;
    k.CF = (uint64_t)k.Fc * e.C; k.J = k.CF * e.hs.R;
    k.idx = ctx->cur_idx + f0;
    const uint64_t CF = k.CF, J = k.J;
    const LnnChunkIn in = { &e.hs, e.C, S, k.Fc, ctx->tab.cls, k.idx, &ctx->knob, e.split.use_sub, ctx->has_side != 0, ctx->af_iters, ctx->learning, false };
    lnn_chunk_forms(&in, &k.forms);
    Plan &p = k.p;
    fill_plan(p, e, k.Fc);
    p.ms = e.shape->ch_process_method; p.J = (uint32_t)J;
    for (uint32_t l = 0; l < e.hs.L; l++) p.coef_off[l] = e.hs.coef_off[l];
    for (uint32_t r = 0; r < e.hs.R; r++) p.regs[r] = e.hs.regs[r];
    p.resid = e.d_residual; p.prm = e.d_params;      /* the caller's arrays: rows of the class-sorted chunk reach them through frame_map */
    p.fused_last = k.forms.fuse_cfg ? 1u : 0u;
    p.search_long = ctx->knob.search_long ? 1u : 0u;
    p.rows16 = ctx->knob.rows16 ? 1u : 0u;
    p.prep_general = ctx->knob.prep_general ? 1u : 0u;
    p.prep_defer = k.forms.prep_defer ? 1u : 0u;
    lnn_build_runs(&p.runs[0], k.idx, k.Fc, e.C); lnn_build_runs(&p.runs[1], k.idx, k.Fc, e.C * e.hs.R);
    p.hist = k.forms.hist ? 1u : 0u;
    p.cls_of_frame = ctx->d_clsidx + f0; p.frame_map = ctx->d_map + f0; p.cls = ctx->d_cls; p.sintab = ctx->d_sin; p.wtab = ctx->d_wt; p.ucount = ctx->d_ucount; p.min_margin = (unsigned long long *)(ctx->d_ucount + 2); p.force_exact = ctx->knob.force_exact ? 1u : 0u; p.dbg_maxtr = ctx->knob.dbg_maxtr;
    p.capture = ctx->capture_n ? ctx->d_capture : NULL;
    k.part_bytes = e.split.part_bytes;
    k.abase = (uint8_t *)ctx->arena + (size_t)slot * k.part_bytes;
    uint8_t *a = k.abase;
#define TAKE(ptr, type, count) do { ptr = (type *)a; a += align_up(sizeof(type) * (uint64_t)(count)); } while (0)
    TAKE(p.xint, int32_t, CF * S); TAKE(p.xtmp, int32_t, CF * S);
    TAKE(p.sig, double, J * 2 * S);
    TAKE(p.acorr, double, J * LNN_MAXT * LNN_ACW); TAKE(p.tcoef, double, J * LNN_MAXT * LNN_MAXP);
    TAKE(p.ptail, double, J * LNN_MAXT * LNN_MAXU); TAKE(p.ptail_set, uint8_t, J * LNN_MAXT * LNN_MAXU);
    TAKE(p.tloss, double, J * LNN_MAXT); p.npart = ((S + FIR_TILE - 1) / FIR_TILE) * (FIR_THREADS / 64); TAKE(p.tsum, double, J * LNN_MAXT * p.npart); TAKE(p.txmax, double, J * p.npart); TAKE(p.thsum, double, J * LNN_MAXT); TAKE(p.uncertain, uint8_t, J); TAKE(p.lparams, double, J * LNN_MAXL * LNN_MAXP);
    TAKE(p.lunits, uint32_t, J * LNN_MAXL); TAKE(p.jloss, double, J); TAKE(p.jtail, double, J);
    TAKE(p.prep_slow_n, uint32_t, 64); TAKE(p.prep_slow_rows, uint32_t, CF);
    k.af_best = NULL; k.af_loss = NULL; k.af_reg = NULL;
    memset(&k.tr, 0, sizeof(k.tr));
    TrainArgs &tr = k.tr;
    if (ctx->af_iters || ctx->learning) { TAKE(k.af_best, uint32_t, CF); TAKE(k.af_loss, double, CF); TAKE(k.af_reg, double, CF); }
    if (ctx->learning) {
        TAKE(tr.buf, double, CF * TR_NBUF * S); TAKE(tr.dparams, double, CF * LNN_MAXL * LNN_MAXP); TAKE(tr.momentum, double, CF * LNN_MAXL * LNN_MAXP);
        TAKE(tr.loss, double, CF); TAKE(tr.prev, double, CF); TAKE(tr.active, uint32_t, CF); TAKE(tr.nactive, uint32_t, 64);
    }
    if (ctx->af_iters) {      /* the final pass works on CF jobs */
        TAKE(p.af_a, double, CF * LNN_MAXP); TAKE(p.af_inv, double, CF * S); p.af_Rstride = e.hs.maxP * e.hs.maxP; TAKE(p.af_R, double, CF * p.af_Rstride);
        TAKE(p.af_rv, double, CF * LNN_MAXP); TAKE(p.af_invd, double, CF * LNN_MAXP);
        TAKE(p.af_obj, double, CF * LNN_MAXU); TAKE(p.af_prev, double, CF * LNN_MAXU); TAKE(p.af_state, uint32_t, CF * LNN_MAXU);
        TAKE(p.af_prob, uint32_t, CF * LNN_MAXU); TAKE(p.af_nprob, uint32_t, 64); TAKE(p.af_pivot, double, CF * LNN_MAXU);
    }
#undef TAKE
    if ((uint64_t)(a - k.abase) > k.part_bytes) { snprintf(ctx->err, sizeof(ctx->err), "internal: arena overflow"); return LNN_NG; }
    return LNN_OK;
}

/* k_prep, and behind it k_prep_slow for the channel-frames it listed (none for 16-bit material: its blocks leave at once) */
static int launch_prep(Chunk &k)
{
    LINNEAmdContext *ctx = k.ctx; hipStream_t st = k.st; const Plan &p = k.p;
    if (p.prep_defer) HIPCHK(ctx, hipMemsetAsync(p.prep_slow_n, 0, sizeof(uint32_t), st));
    const int sp_ = span_begin(ctx, LINNE_AMD_T_PREP, st);
    hipLaunchKernelGGL(k_prep, dim3(k.Fc, k.C), dim3(PREP_THREADS), 0, st, p);
    if (p.prep_defer) hipLaunchKernelGGL(k_prep_slow, dim3((uint32_t)((k.CF + 63) / 64)), dim3(256), 0, st, p);
    span_end(ctx, sp_, st);
    return LNN_OK;
}

/* the sibling stream of a chunk whose order-128 Levinson launch runs beside its lag kernels: the odd stream slots get a stream of
 * their own at the first such chunk (failing that they share the side stream: slower, same results) */
static void sibling_for_levinson(Chunk &k)
{
    LINNEAmdContext *ctx = k.ctx;
    if ((k.slot & 1u) && ctx->sib[1] == ctx->side && !ctx->sib1_tried) {
        ctx->sib1_tried = 1;
        if (hipStreamCreateWithFlags(&ctx->sib[1], hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ctx->sib[1] = ctx->side; }
    }
    k.sib = ctx->sib[k.slot & 1u];
}

/* lags of layer l: the lanes = jobs kernels for the frames they take (hist_takes), the general kernels for the others */
static int launch_lags(Chunk &k, const Pass &ps, uint32_t l)
{
    LINNEAmdContext *ctx = k.ctx; hipStream_t st = k.st; const Plan &q = *ps.q; const LnnLayerForms &lf = ps.forms->layer[l];
    const uint32_t P = k.hs->P[l];
    if (lf.lev_beside && !lf.lev_inline) sibling_for_levinson(k);
    if (lf.beside) {
        HIPCHK(ctx, hipEventRecord(ctx->fork_ev[k.slot], st)); HIPCHK(ctx, hipStreamWaitEvent(k.sib, ctx->fork_ev[k.slot], 0));
        const int sp_ = span_begin(ctx, LINNE_AMD_T_AUTOCORR, k.sib); dispatch_autocorr2(k.sib, q, l, ps.cur, ctx->na_max, (ctx->prod_ok >> l) & 1); span_end(ctx, sp_, k.sib);
        HIPCHK(ctx, hipEventRecord(ctx->join_ev[k.slot], k.sib));
    }
    if (lf.hist_layer) {
        for (int w = 0; w < 3; w++) {
            if (P == 64u && w == 1) continue;
            const int sp_ = span_begin(ctx, LINNE_AMD_T_HIST_P + w, st); (void)launch_autocorr_hist(st, q, l, ps.cur, w, w == 2 && lf.lev_beside); span_end(ctx, sp_, st);
            if (w == 0 && lf.lev_beside) {
                /* Trial 0's lags are there (those of the frames the general kernel has: in stream order on the sibling, in front of the
                 * solver): the order-128 Levinson launch starts on the sibling, BEFORE the lag kernels behind this one are
                 * launched.  Its 130 KB blocks and k_autocorr_hist<P,1>'s 66 KB blocks cannot share a CU: while that kernel runs the
                 * two compete for whole CUs; once k_autocorr_sub follows, its small-LDS blocks fit in beside the solver's.  It takes
                 * no timing span of its own; launch_levinson joins.  (lev_inline: the solver on the chunk's own stream -- behind
                 * the general kernel's lags too, which only an event orders there.) */
                const LnnLevLaunch &v = lf.lev[0];
                const hipStream_t ls = lf.lev_inline ? st : k.sib;
                if (lf.lev_inline && lf.beside) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->join_ev[k.slot], 0));
                if (!lf.lev_inline) { HIPCHK(ctx, hipEventRecord(ctx->lev_fork_ev[k.slot], st)); HIPCHK(ctx, hipStreamWaitEvent(k.sib, ctx->lev_fork_ev[k.slot], 0)); }
                hipLaunchKernelGGL(k_levinson_lds, dim3((ps.J + 63) / 64, v.u), dim3(v.threads), v.lds, ls, q, l, v.t, v.ride);
                if (!lf.lev_inline) HIPCHK(ctx, hipEventRecord(ctx->lev_join_ev[k.slot], k.sib));
            }
        }
    }
    if (lf.beside) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->join_ev[k.slot], 0));
    else if (!lf.hist_all) {
        const int sp_ = span_begin(ctx, (P >= 32u) ? LINNE_AMD_T_AUTOCORR : LINNE_AMD_T_AUTOCORR_SHORT, st); dispatch_autocorr2(st, q, l, ps.cur, ctx->na_max, (ctx->prod_ok >> l) & 1); span_end(ctx, sp_, st);
    }
    return LNN_OK;
}

static void launch_levinson(Chunk &k, const Pass &ps, uint32_t l)
{
    LINNEAmdContext *ctx = k.ctx; hipStream_t st = k.st; const Plan &q = *ps.q; const LnnLayerForms &lf = ps.forms->layer[l];
    const uint32_t P = k.hs->P[l], maxu = P < 128u ? P : 128u;
    if (lf.lev_beside && !lf.lev_inline) (void)hipStreamWaitEvent(st, ctx->lev_join_ev[k.slot], 0);      /* lev[0] went ahead on the sibling (launch_lags) */
    const int sp_ = span_begin(ctx, LINNE_AMD_T_LEVINSON, st);
    if (lf.lev_wave) hipLaunchKernelGGL(k_levinson_wave, dim3(ps.J, 2u * maxu - 1u), dim3(64), 0, st, q, l);
    else for (uint32_t i = lf.lev_beside ? 1u : 0u; i < lf.nlev; i++) {
        const LnnLevLaunch &v = lf.lev[i];
        hipLaunchKernelGGL(k_levinson_lds, dim3((ps.J + 63) / 64, v.u), dim3(v.threads), v.lds, st, q, l, v.t, v.ride);
    }
    span_end(ctx, sp_, st);
}

/* unit-count search of layer l: k_search_long for the frames it takes, the register-window kernel / k_fir2<2> for the others */
static void launch_search(Chunk &k, const Pass &ps, uint32_t l)
{
    LINNEAmdContext *ctx = k.ctx; hipStream_t st = k.st; const Plan &q = *ps.q; const LnnLayerForms &lf = ps.forms->layer[l];
    const uint32_t tiles = (k.S + FIR_TILE - 1) / FIR_TILE;
    if (lf.long_any) {
        const int sp_ = span_begin(ctx, LINNE_AMD_T_SEARCH_LONG, st);
        ctx->last_search_form = lf.search_form == 2 ? 1 : 0;
        launch_search_long(st, q, l, ps.cur, ps.J, tiles, lf.search_form);
        span_end(ctx, sp_, st);
    }
    if (lf.long_any && lf.long_all) return;
    const int sp_ = span_begin(ctx, (l == 0) ? LINNE_AMD_T_SEARCH_L0 : (lf.fir_spec ? LINNE_AMD_T_SEARCH : LINNE_AMD_T_SEARCH_PLAIN), st);
    if (lf.fir_small) launch_fir_small_search(st, q, l, ps.cur, ps.J, tiles, lf.fir_spec, k.hs->P[l]);
    else if (lf.long_any) {
        /* a launch per run of frames k_search_long leaves, not 620 k blocks of which all but a handful look up their job and go (0.7 ms) */
        const uint32_t rpf = ps.J / k.Fc;
        for (uint32_t f = 0, g = 0; lnn_next_left_run(&lf, k.idx, k.Fc, g, &f, &g); ) {
            Plan qq = q; qq.job_off = f * rpf;
            launch_fir<2>(st, qq, l, ps.cur, (g - f) * rpf, tiles, lf.fir_spec);
        }
    }
    else launch_fir<2>(st, q, l, ps.cur, ps.J, tiles, lf.fir_spec);
    span_end(ctx, sp_, st);
}

/* the selection, then the exact ordered chains for the (rare) jobs the certified search flagged (everything else exits at once) and
 * the selection among those */
static void launch_select(Chunk &k, const Pass &ps, uint32_t l)
{
    LINNEAmdContext *ctx = k.ctx; hipStream_t st = k.st; const Plan &q = *ps.q; const LnnLayerForms &lf = ps.forms->layer[l];
    for (uint32_t exact = 0; exact < 2; exact++) {
        const int sp_ = span_begin(ctx, exact ? LINNE_AMD_T_EXACT : LINNE_AMD_T_SELECT, st);
        if (exact) { if (l == 0) hipLaunchKernelGGL((k_fir2<0, true, false>), dim3(ps.J, 1), dim3(FIR_THREADS), 0, st, q, l, ps.cur); else hipLaunchKernelGGL((k_fir2<0, false, false>), dim3(ps.J, 1), dim3(FIR_THREADS), 0, st, q, l, ps.cur); }
        if (lf.sel_wave) hipLaunchKernelGGL(k_select_wave, dim3(ps.J), dim3(64), 0, st, q, l, exact);
        else hipLaunchKernelGGL(k_select, dim3((ps.J + 63) / 64), dim3(64), 0, st, q, l, exact);
        span_end(ctx, sp_, st);
    }
}

/* -a N: the auxiliary-function iterations on the coefficients k_select kept for layer l (lnn_k_af.h); synchronous: every
 * Cholesky pivot goes through the host's pow() */
static int run_af(Chunk &k, const Pass &ps, uint32_t l)
{
    LINNEAmdContext *ctx = k.ctx; hipStream_t st = k.st; const Plan &q = *ps.q;
    const uint32_t P = k.hs->P[l], S = k.S, Jq = ps.J, cur = ps.cur;
    HIPCHK(ctx, hipMemsetAsync(q.af_nprob, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_af_init, dim3((Jq + 255) / 256), dim3(256), 0, st, q, l);
    uint32_t nprob = 0;
    HIPCHK(ctx, hipMemcpyAsync(&nprob, q.af_nprob, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (nprob == 0) return LNN_OK;
    if (ctx->af_h_cap < nprob) {
        if (ctx->af_h) HIPCHK(ctx, hipHostFree(ctx->af_h));
        ctx->af_h = NULL; ctx->af_h_cap = 0;
        HIPCHK(ctx, hipHostMalloc((void **)&ctx->af_h, sizeof(double) * (size_t)nprob, hipHostMallocDefault));
        ctx->af_h_cap = nprob;
    }
    uint32_t mblocks = 0;                                                      /* k_af_matrix: blocks per job, whatever unit count it chose */
    for (uint32_t uu = 1; uu <= P; uu <<= 1) { const uint32_t b_ = uu * afm_blocks_per_unit(P / uu); if (b_ > mblocks) mblocks = b_; }
    for (uint32_t it = 0; it < ps.af_iters; it++) {
        hipLaunchKernelGGL(k_af_resid, dim3(Jq, (S + AFR_THREADS * 4 - 1) / (AFR_THREADS * 4)), dim3(AFR_THREADS), 0, st, q, l, cur);
        hipLaunchKernelGGL(k_af_obj, dim3(nprob), dim3(64), 0, st, q, l, cur);
        hipLaunchKernelGGL(k_af_matrix, dim3(Jq, mblocks), dim3(AFM_THREADS), 0, st, q, l, cur);
        for (uint32_t i = 0; i < P; i++) {
            hipLaunchKernelGGL(k_af_pivot, dim3((nprob + 63) / 64), dim3(64), 0, st, q, l, i);
            HIPCHK(ctx, hipMemcpyAsync(ctx->af_h, q.af_pivot, sizeof(double) * (size_t)nprob, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipStreamSynchronize(st));
            for (uint32_t j = 0; j < nprob; j++) { const double v = ctx->af_h[j]; ctx->af_h[j] = (v <= 0.0) ? -1.0 : lnn_cholesky_pivot(v); }      /* lpc.c:418-421, host libm */
            HIPCHK(ctx, hipMemcpyAsync(q.af_pivot, ctx->af_h, sizeof(double) * (size_t)nprob, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_af_column, dim3(nprob), dim3(128), 0, st, q, l, i);
        }
        hipLaunchKernelGGL(k_af_solve, dim3((nprob + 63) / 64), dim3(64), 0, st, q, l);
    }
    hipLaunchKernelGGL(k_af_finish, dim3((Jq + 255) / 256), dim3(256), 0, st, q, l);
    HIPCHK(ctx, hipGetLastError());
    return LNN_OK;
}

/* the layers of one pass (linne_network.c:582-602): lags, Levinson-Durbin, the unit-count search, [the auxiliary-function refinement
 * of the chosen coefficients], the forward pass.  Returns LNN_*; ps.cur = which half of `sig` holds the last layer's output */
static int run_layers(Chunk &k, Pass &ps)
{
    LINNEAmdContext *ctx = k.ctx; hipStream_t st = k.st; const Plan &q = *ps.q;
    const uint32_t L = k.hs->L, tiles = (k.S + FIR_TILE - 1) / FIR_TILE;
    int ret;
    ps.cur = 0;
    for (uint32_t l = 0; l < L; l++) {
        const LnnLayerForms &lf = ps.forms->layer[l];
        if ((ret = launch_lags(k, ps, l)) != LNN_OK) return ret;
        launch_levinson(k, ps, l);
        if (lf.last_layer) {        /* search, selection, forward pass and loss from one pass over the input */
            { const int sp_ = span_begin(ctx, LINNE_AMD_T_FWD_LOSS, st); launch_last_layer(st, q, l, ps.cur, ps.J); span_end(ctx, sp_, st); }
            { const int sp_ = span_begin(ctx, LINNE_AMD_T_SELECT, st); hipLaunchKernelGGL(k_select, dim3((ps.J + 63) / 64), dim3(64), 0, st, q, l, 2u); span_end(ctx, sp_, st); }
        } else {
            launch_search(k, ps, l);
            launch_select(k, ps, l);
            if (lf.fwd_loss) { const int sp_ = span_begin(ctx, LINNE_AMD_T_FWD_LOSS, st); launch_fwd_loss(st, q, l, ps.cur, ps.J, lf.fwd_loss_mw); span_end(ctx, sp_, st); }
        }
        if (ps.af_iters && (ret = run_af(k, ps, l)) != LNN_OK) return ret;
        if (lf.forward) {
            const int sp_ = span_begin(ctx, (l == 0) ? LINNE_AMD_T_FORWARD_L0 : (lf.fir_spec ? LINNE_AMD_T_FORWARD : LINNE_AMD_T_FORWARD_PLAIN), st);
            launch_fir<1>(st, q, l, ps.cur, ps.J, lf.forward_walk ? 1u : tiles, lf.fir_spec);
            span_end(ctx, sp_, st);
        }
        ps.cur ^= 1u;
    }
    return LNN_OK;
}

/* -l: LINNENetworkTrainer_Train on the parameters the analysis left (lnn_k_train.h); synchronous: the host reads after every
 * step how many channel-frames go on */
static int run_train(Chunk &k, const Plan &q, const uint32_t *best)
{
    LINNEAmdContext *ctx = k.ctx; hipStream_t st = k.st; TrainArgs &tr = k.tr;
    const uint32_t CF = (uint32_t)k.CF, L = k.hs->L;
    tr.p = q; tr.best = best; tr.CF = CF;
    const uint32_t tiles = (k.S + TR_TILE - 1) / TR_TILE;
    const int sp_ = span_begin(ctx, LINNE_AMD_T_TRAIN, st);
    hipLaunchKernelGGL(k_tr_init, dim3((CF + 255) / 256), dim3(256), 0, st, tr);
    for (uint32_t it = 0; it < 2000u; it++) {                      /* LINNE_TRAINING_PARAMETER_MAX_NUM_ITRATION, linne_internal.h:29 */
        HIPCHK(ctx, hipMemsetAsync(tr.nactive, 0, sizeof(uint32_t), st));
        for (uint32_t l = 0; l < L; l++) hipLaunchKernelGGL(k_tr_forward, dim3(CF, tiles), dim3(TR_THREADS), 0, st, tr, l);
        hipLaunchKernelGGL(k_tr_loss, dim3(CF), dim3(64), 0, st, tr);                                   /* the loss and, in place, its gradient */
        for (uint32_t l = L - 1; l >= 1; l--) hipLaunchKernelGGL(k_tr_back, dim3(CF, tiles), dim3(TR_THREADS), 0, st, tr, l);
        hipLaunchKernelGGL(k_tr_gradp, dim3(CF, L), dim3(128), 0, st, tr);
        hipLaunchKernelGGL(k_tr_update, dim3(CF), dim3(128), 0, st, tr, (double)0.8f, (double)0.1f, 1.0e-7);     /* linne_network.c:829, linne_internal.h:31-33 */
        uint32_t left = 0;
        HIPCHK(ctx, hipMemcpyAsync(&left, tr.nactive, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (left == 0) break;
    }
    span_end(ctx, sp_, st);
    HIPCHK(ctx, hipGetLastError());
    return LNN_OK;
}

/* quantise + cascade: the parameter records and the residual */
static void launch_finish(Chunk &k, const Plan &q)
{
    const uint32_t CF = (uint32_t)k.CF;
    const int sp_ = span_begin(k.ctx, LINNE_AMD_T_FINALIZE, k.st);
    hipLaunchKernelGGL(k_quantize, dim3(CF), dim3(64), 0, k.st, q);
    hipLaunchKernelGGL(k_fir_cascade, dim3(CF, k.forms.cascade_walk ? 1u : (k.S + FIN_TILE - 1) / FIN_TILE), dim3(FIN_THREADS), 0, k.st, q);
    span_end(k.ctx, sp_, k.st);
}

/* -a N: the final pass is real -- the winner's regulariser, the refinement after every layer's search, and therefore new inputs (and
 * possibly new unit counts) for the layers behind it.  One job per channel-frame, general kernels: the same rules, asked with R = 1. */
static int run_final_pass(Chunk &k)
{
    LINNEAmdContext *ctx = k.ctx; hipStream_t st = k.st; const Plan &p = k.p;
    const uint32_t CF = (uint32_t)k.CF;
    int ret;
    Plan q = p;
    q.R = 1; q.J = CF; q.regs[0] = 0.0;
    q.hist = 0; q.fused_last = 0; q.search_long = 0;
    q.capture = NULL;                                       /* the final pass does not search: it refines the winner */
    lnn_build_runs(&q.runs[1], k.idx, k.Fc, k.C);
    q.job_reg = k.af_reg; q.af_best = k.af_best; q.af_loss = k.af_loss;
    hipLaunchKernelGGL(k_af_best, dim3((CF + 255) / 256), dim3(256), 0, st, p, k.af_best, k.af_loss, k.af_reg);
    const LnnChunkIn in = { k.hs, k.C, k.S, k.Fc, ctx->tab.cls, k.idx, &ctx->knob, false, ctx->has_side != 0, ctx->af_iters, ctx->learning, true };
    LnnChunkForms ff;
    lnn_chunk_forms(&in, &ff);
    Pass fp = { &q, &ff, CF, ctx->af_iters, 0 };
    const int sp_ = span_begin(ctx, LINNE_AMD_T_AF_PASS, st);
    if ((ret = run_layers(k, fp)) != LNN_OK) return ret;
    span_end(ctx, sp_, st);
    if (ctx->learning && (ret = run_train(k, q, NULL)) != LNN_OK) return ret;
    launch_finish(k, q);
    return LNN_OK;
}

/* everything of one chunk, on its stream */
static int enqueue_chunk(Chunk &k)
{
    LINNEAmdContext *ctx = k.ctx; hipStream_t st = k.st; const Plan &p = k.p;
    int ret;
    if ((ret = launch_prep(k)) != LNN_OK) return ret;
    Pass sp = { &p, &k.forms, (uint32_t)k.J, 0u, 0 };
    if ((ret = run_layers(k, sp)) != LNN_OK) return ret;
    if (k.forms.chain_sum) {
        const int sp_ = span_begin(ctx, LINNE_AMD_T_FINAL_LOSS, st);
        if (k.forms.chain_sum_wave) hipLaunchKernelGGL(k_chain_sum_wave<1>, dim3((uint32_t)k.J), dim3(64), 0, st, p, 0u, sp.cur);
        else hipLaunchKernelGGL(k_chain_sum<1>, dim3(((uint32_t)k.J + 63) / 64), dim3(SUM_THREADS), 0, st, p, 0u, sp.cur);
        span_end(ctx, sp_, st);
    }
    if (ctx->af_iters) { if ((ret = run_final_pass(k)) != LNN_OK) return ret; }
    else {                      /* the final pass of linne_network.c:628-629 repeats the winning pass bit for bit: skipped */
        if (ctx->learning) {
            hipLaunchKernelGGL(k_af_best, dim3(((uint32_t)k.CF + 255) / 256), dim3(256), 0, st, p, k.af_best, k.af_loss, k.af_reg);
            if ((ret = run_train(k, p, k.af_best)) != LNN_OK) return ret;
        }
        launch_finish(k, p);
    }
    HIPCHK(ctx, hipGetLastError());
    return LNN_OK;
}

/* the chunks are enqueued inside one function so that EVERY way out of the loop -- a failing HIP call, a failing layer pass --
 * comes by the join in LINNEAmd_EncodeFramesDevice: with sub-streams forked off, the caller may only reuse its buffers once they
 * have drained */
static int enqueue_chunks(LINNEAmdContext *ctx, const EncodeCall &e)
{
    uint32_t chunk_index = 0;
    for (uint32_t f0 = 0; f0 < e.num_frames; f0 += (uint32_t)e.split.chunk, chunk_index++) {
        Chunk k;
        int ret = chunk_setup(k, ctx, e, f0, chunk_index % e.split.nsub);
        if (ret == LNN_OK) ret = enqueue_chunk(k);
        if (ret != LNN_OK) return ret;
    }
    return LNN_OK;
}

extern "C" int LINNEAmd_EncodeFramesDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        const int32_t *d_pcm, const uint32_t *h_num_samples, uint32_t num_frames,
        int32_t *d_residual, int32_t *d_params, double *d_stats)
{
    /* validate */
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->err[0] = 0;
    EncodeCall e;
    e.pcm16 = (uint32_t)ctx->pcm16_next;        /* 0 int32, 1 int16, 2 packed 3-byte samples (set by the staging slots) */
    ctx->pcm16_next = 0;
    if (!shape || !d_pcm || !d_residual || !d_params || !d_stats) { snprintf(ctx->err, sizeof(ctx->err), "null argument"); return LNN_INVALID_ARGUMENT; }
    if (num_frames == 0) return LNN_OK;
    int ret = shape_info(shape, &e.hs);
    if (ret != LNN_OK) { snprintf(ctx->err, sizeof(ctx->err), "invalid shape"); return ret; }
    e.shape = shape; e.C = shape->num_channels; e.S = shape->num_samples_per_block; e.num_frames = num_frames;
    e.d_pcm = d_pcm; e.d_residual = d_residual; e.d_params = d_params; e.d_stats = d_stats;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((ret = ctx_encode_streams(ctx)) != LNN_OK) return ret;
    lnn_knobs_read_call(&ctx->knob);
    /* classes */
    if ((ret = build_classes(ctx, shape, &e.hs, h_num_samples, num_frames)) != LNN_OK) return ret;
    /* split */
    const uint64_t per_frame = frame_scratch_bytes(shape, &e.hs, ctx->af_iters, ctx->learning);
    if (ctx->arena_bytes < per_frame * 4 + 65536) {       /* grow the arena to hold at least a few frames */
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipFree(ctx->arena)); ctx->arena = NULL; ctx->arena_bytes = 0;
        HIPCHK(ctx, hipMalloc(&ctx->arena, per_frame * 4 + 65536));
        ctx->arena_bytes = per_frame * 4 + 65536;
    }
    e.split = lnn_call_split(ctx->arena_bytes, per_frame, num_frames, e.C, e.hs.R, ctx->nsub, ctx->nsub_forced != 0, &ctx->knob);
    const LnnSplit &sp = e.split;
    if (!ctx->span_keep) ctx->nspans = 0;
    ctx->last_search_form = -1;
    ctx->capture_n = 0;
    if (ctx->capture_on) {          /* one record per (frame, channel, pass, layer, trial slot) in the caller's order; slots no search fills stay NaN */
        const uint64_t nrec = (uint64_t)num_frames * e.C * e.hs.R * e.hs.L * LNN_MAXT;
        if (ctx->capture_cap < nrec) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            if (ctx->d_capture) HIPCHK(ctx, hipFree(ctx->d_capture));
            ctx->d_capture = NULL; ctx->capture_cap = 0;
            HIPCHK(ctx, hipMalloc((void **)&ctx->d_capture, nrec * LNN_CAP_WORDS * sizeof(double)));
            ctx->capture_cap = nrec;
        }
        HIPCHK(ctx, hipMemsetAsync(ctx->d_capture, 0xFF, nrec * LNN_CAP_WORDS * sizeof(double), ctx->stream));
        ctx->capture_n = nrec;
    }
    HIPCHK(ctx, hipMemsetAsync(ctx->d_ucount, 0, sizeof(uint32_t), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_ucount + 2, 0x7F, 2 * sizeof(uint32_t), ctx->stream));      /* min margin: a huge double (0x7F7F...) */
    if (ctx->timing && !ctx->span_keep) { HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream)); }
    if (sp.use_sub || ctx->has_side) HIPCHK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    if (sp.use_sub) for (uint32_t i = 0; i < sp.nsub; i++) HIPCHK(ctx, hipStreamWaitEvent(ctx->sub[i], ctx->ev_start, 0));
    /* statistics launch, loop over chunks */
    if ((ret = launch_stats(ctx, e)) != LNN_OK) return ret;
    const int loop_ret = enqueue_chunks(ctx, e);
    /* join */
    if (loop_ret != LNN_OK) {       /* what was forked is waited for before the error goes back (the callers synchronise ctx->stream only) */
        if (sp.use_sub) for (uint32_t i = 0; i < sp.nsub; i++) (void)hipStreamSynchronize(ctx->sub[i]);
        if (ctx->has_side) { (void)hipStreamSynchronize(ctx->side); (void)hipStreamSynchronize(ctx->sib[1]); }
        return loop_ret;
    }
    if (ctx->has_side) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->side_done, 0));
    if (sp.use_sub) {
        for (uint32_t i = 0; i < sp.nsub; i++) { HIPCHK(ctx, hipEventRecord(ctx->sub_done[i], ctx->sub[i])); HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->sub_done[i], 0)); }
    }
    if (ctx->timing) { HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream)); ctx->ev_valid = 1; }
    return LNN_OK;
}

/* The throughput and latency forms of the synthesis carry a coefficient as int8 (the format's range: the coefficients are 8-bit
 * Huffman symbols, linne_decoder.c:452-470); the lanes form would take any int32.  A parameter record with a coefficient outside
 * [-128, 127] is no LINNE stream's: the entry points that see the records on the HOST refuse it, so that the result never depends on
 * which form the batch size picked (include/linne_amd.h states the contract for records that are already in HBM). */
static int params_in_range(LINNEAmdContext *ctx, const HostShape *hs, uint32_t C, const int32_t *h_params, uint32_t num_frames)
{
    uint32_t ncoef = 0;
    for (uint32_t l = 0; l < hs->L; l++) ncoef += hs->P[l];
    const uint64_t rows = (uint64_t)num_frames * C;
    uint32_t bad = 0;
    for (uint64_t r = 0; r < rows; r++) {
        const int32_t *c = h_params + r * LINNE_AMD_PARAM_WORDS + LINNE_AMD_PRM_COEF;
        uint32_t acc = 0;
        for (uint32_t i = 0; i < ncoef; i++) acc |= (uint32_t)(c[i] + 128) & ~255u;
        bad |= acc;
    }
    if (bad) { snprintf(ctx->err, sizeof(ctx->err), "a coefficient outside [-128, 127] in the parameter records (not a LINNE stream's)"); return LNN_INVALID_FORMAT; }
    return LNN_OK;
}

/* dispatch helpers of the synthesis kernels */
static void launch_synth_rows(hipStream_t st, const DecPlan &p, uint32_t l, const LnnDecLayer &d, uint32_t CF)
{
    const dim3 grows((CF + 3) / 4), grows8((CF + 7) / 8), b(64);
    if (d.form == LNN_DL_ROWS8) switch (d.pb) {
    case 4: hipLaunchKernelGGL((k_synth_rows8<4>), grows8, b, 0, st, p, l); break;
    case 8: hipLaunchKernelGGL((k_synth_rows8<8>), grows8, b, 0, st, p, l); break;
    default: hipLaunchKernelGGL((k_synth_rows8<16>), grows8, b, 0, st, p, l); break;
    }
    else switch (d.nch) {
    case 0: if (d.pb == 4u) hipLaunchKernelGGL((k_synth_rows<0, 4>), grows, b, 0, st, p, l); else hipLaunchKernelGGL((k_synth_rows<0>), grows, b, 0, st, p, l); break;
    case 1: hipLaunchKernelGGL((k_synth_rows<1>), grows, b, 0, st, p, l); break;
    case 3: hipLaunchKernelGGL((k_synth_rows<3>), grows, b, 0, st, p, l); break;
    default: hipLaunchKernelGGL((k_synth_rows<7>), grows, b, 0, st, p, l); break;
    }
}
template <int PP> static void launch_synth_small_p(hipStream_t st, const DecPlan &p, uint32_t l, bool de, uint32_t CF)
{
    if (de) hipLaunchKernelGGL((k_synth_small<PP, true>), dim3((CF + 63) / 64), dim3(64), 0, st, p, l); else hipLaunchKernelGGL((k_synth_small<PP, false>), dim3((CF + 63) / 64), dim3(64), 0, st, p, l);
}
/* the lanes forms: short layers with lanes = channel-frames (and the de-emphasis on layer 0's pass), long ones a wave per 16 */
static void launch_synth_lanes(hipStream_t st, const DecPlan &p, uint32_t l, const LnnDecLayer &d, uint32_t CF)
{
#define LNN_SS(PP_) launch_synth_small_p<PP_>(st, p, l, d.de, CF)
    if (d.form == LNN_DL_SMALL) LNN_BY_ORDER(d.pb, LNN_SS);
#undef LNN_SS
    else if (d.form == LNN_DL_BIG) switch (d.pb) {
    case 32:  hipLaunchKernelGGL((k_synth_big<32>), dim3((CF + 15) / 16), dim3(64), 0, st, p, l); break;
    case 64:  hipLaunchKernelGGL((k_synth_big<64>), dim3((CF + 15) / 16), dim3(64), 0, st, p, l); break;
    default: hipLaunchKernelGGL((k_synth_big<128>), dim3((CF + 15) / 16), dim3(64), 0, st, p, l); break;
    }
    else hipLaunchKernelGGL(k_synthesize, dim3(CF), dim3(64), 0, st, p, l, 0u);      /* not a preset size */
}

/* the synthesis of num_frames frames whose lengths are in device memory (d_nsmp): enqueued on the context's stream behind what is
 * there; records the call's end event when timing is on.  The caller has read the call's knobs and started its spans.  Layers in
 * reverse order (linne_decoder.c:503-509); which form each takes: lnn_decode_forms */
static int decode_frames_dev(LINNEAmdContext *ctx, const struct LINNEAmdShape *shape, const HostShape &hs,
        int32_t *d_data, const uint32_t *d_nsmp, uint32_t num_frames, const int32_t *d_params)
{
    DecPlan p; memset(&p, 0, sizeof(p));
    p.C = shape->num_channels; p.S = shape->num_samples_per_block; p.L = hs.L; p.ms = shape->ch_process_method; p.F = num_frames;
    for (uint32_t l = 0; l < hs.L; l++) { p.P[l] = hs.P[l]; p.coef_off[l] = hs.coef_off[l]; }
    p.data = d_data; p.prm = d_params; p.nsmp = d_nsmp;
    hipStream_t st = ctx->stream;
    const uint32_t CF = num_frames * p.C, gsmall = (CF + 63) / 64;
    if (hs.P[0] > 16) { snprintf(ctx->err, sizeof(ctx->err), "internal: layer 0 of order %u", hs.P[0]); return LNN_NG; }
    LnnDecodeForms df;
    lnn_decode_forms(&hs, p.C, p.S, p.ms, num_frames, ((uintptr_t)d_data & 15u) == 0u, SP_LDS_BYTES(p.S) <= LEV_LDS_BUDGET, &ctx->knob, &df);
    if (df.call == LNN_DEC_PIPE) { const int sp_ = span_begin(ctx, LINNE_AMD_T_SYNTH_PIPE, st); hipLaunchKernelGGL(k_synth_pipe, dim3(CF), dim3(64 * (hs.L + 1)), SP_LDS_BYTES(p.S), st, p); span_end(ctx, sp_, st); }
    else if (df.call == LNN_DEC_WAVE) { const int sp_ = span_begin(ctx, LINNE_AMD_T_SYNTH, st); hipLaunchKernelGGL(k_synthesize, dim3(CF), dim3(64), 0, st, p, 0xFFFFFFFFu, 1u); span_end(ctx, sp_, st); }
    else for (int32_t li = (int32_t)hs.L - 1; li >= 0; li--) {
        const uint32_t l = (uint32_t)li;
        const LnnDecLayer &d = df.layer[l];
        if (d.form == LNN_DL_FUSED_L0) {
            const int sp_ = span_begin(ctx, LINNE_AMD_T_SYNTH_L0_DE, st);
            if (d.ms_fold) hipLaunchKernelGGL((k_synth_l0_de<true>), dim3(gsmall), dim3(64 * SF_WAVES), 0, st, p); else hipLaunchKernelGGL((k_synth_l0_de<false>), dim3(gsmall), dim3(64 * SF_WAVES), 0, st, p);
            span_end(ctx, sp_, st);
        } else if (d.form == LNN_DL_ROWS || d.form == LNN_DL_ROWS8) {
            const int sp_ = span_begin(ctx, d.nch > 0 ? LINNE_AMD_T_SYNTH_ROWS : LINNE_AMD_T_SYNTH_ROWS_SHORT, st);
            launch_synth_rows(st, p, l, d, CF);
            span_end(ctx, sp_, st);
            if (d.de) {
                const int sd_ = span_begin(ctx, LINNE_AMD_T_DEEMPH_LR, st);
                if (d.ms_fold) hipLaunchKernelGGL((k_deemph_lr<true>), dim3(gsmall), dim3(64 * (2 + DL_STORERS)), 0, st, p); else hipLaunchKernelGGL((k_deemph_lr<false>), dim3(gsmall), dim3(64 * (2 + DL_STORERS)), 0, st, p);
                span_end(ctx, sd_, st);
            }
        } else {
            const int sp_ = span_begin(ctx, d.form == LNN_DL_SMALL ? LINNE_AMD_T_SYNTH_SMALL : (d.form == LNN_DL_BIG ? LINNE_AMD_T_SYNTH_BIG : LINNE_AMD_T_SYNTH), st);
            launch_synth_lanes(st, p, l, d, CF);
            span_end(ctx, sp_, st);
        }
    }
    if (df.ms_separate)
        { const int sp_ = span_begin(ctx, LINNE_AMD_T_MS_TO_LR, st); hipLaunchKernelGGL(k_ms_to_lr, dim3(num_frames, (p.S + 255) / 256), dim3(256), 0, st, p); span_end(ctx, sp_, st); }
    HIPCHK(ctx, hipGetLastError());
    if (ctx->timing) { HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream)); ctx->ev_valid = 1; }
    return LNN_OK;
}

extern "C" int LINNEAmd_DecodeFramesDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        int32_t *d_data, const uint32_t *h_num_samples, uint32_t num_frames, const int32_t *d_params)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->err[0] = 0;
    if (!shape || !d_data || !d_params) { snprintf(ctx->err, sizeof(ctx->err), "null argument"); return LNN_INVALID_ARGUMENT; }
    if (num_frames == 0) return LNN_OK;
    HostShape hs;
    int ret = shape_info(shape, &hs);
    if (ret != LNN_OK) { snprintf(ctx->err, sizeof(ctx->err), "invalid shape"); return ret; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    lnn_knobs_read_call(&ctx->knob);
    if ((ret = upload_lengths(ctx, shape, h_num_samples, num_frames)) != LNN_OK) return ret;
    ctx->nspans = 0;
    if (ctx->timing) { HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream)); }
    return decode_frames_dev(ctx, shape, hs, d_data, ctx->d_nsmp, num_frames, d_params);
}

/* device staging of the host-buffer forms: one allocation kept between calls (a block-at-a-time caller pays no hipMalloc /
 * hipFree -- and with it no device-wide synchronisation -- per block); batches beyond HSTAGE_KEEP get a transient one */
#define HSTAGE_KEEP ((uint64_t)64 << 20)
static int hstage_get(LINNEAmdContext *ctx, uint64_t bytes, void **out, int *transient)
{
    *transient = 0;
    if (bytes > HSTAGE_KEEP) {
        if (hipMalloc(out, bytes) != hipSuccess) { (void)hipGetLastError(); snprintf(ctx->err, sizeof(ctx->err), "hipMalloc of staging buffers failed"); return LNN_NG; }
        *transient = 1;
        return LNN_OK;
    }
    if (ctx->hstage_cap < bytes) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->hstage) { HIPCHK(ctx, hipFree(ctx->hstage)); ctx->hstage = NULL; ctx->hstage_cap = 0; }
        uint64_t cap = bytes < ((uint64_t)1 << 20) ? ((uint64_t)1 << 20) : bytes;
        if (hipMalloc(&ctx->hstage, cap) != hipSuccess) { (void)hipGetLastError(); ctx->hstage = NULL; snprintf(ctx->err, sizeof(ctx->err), "hipMalloc of staging buffers failed"); return LNN_NG; }
        ctx->hstage_cap = cap;
    }
    *out = ctx->hstage;
    return LNN_OK;
}

/* host-buffer forms (what the block-at-a-time API calls; batch callers use the device entry points or the staging slots) */
extern "C" int LINNEAmd_EncodeFramesHost(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        const int32_t *pcm, const uint32_t *num_samples, uint32_t num_frames,
        int32_t *residual, int32_t *params, double *stats)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    if (!shape || !pcm || !residual || !params || !stats) return LNN_INVALID_ARGUMENT;
    if (num_frames == 0) return LNN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t CS = (uint64_t)shape->num_channels * shape->num_samples_per_block;
    const uint64_t nb = sizeof(int32_t) * CS * num_frames, pb = sizeof(int32_t) * LINNE_AMD_PARAM_WORDS * (uint64_t)shape->num_channels * num_frames,
                   sb = sizeof(double) * LINNE_AMD_STAT_WORDS * (uint64_t)shape->num_channels * num_frames;
    int32_t *d_pcm = NULL, *d_res = NULL, *d_prm = NULL; double *d_st = NULL;
    void *stage = NULL; int transient = 0;
    const uint64_t nb_a = align_up(nb), pb_a = align_up(pb);
    int ret = hstage_get(ctx, 2 * nb_a + pb_a + align_up(sb), &stage, &transient);
    if (ret != LNN_OK) return ret;
    d_pcm = (int32_t *)stage; d_res = (int32_t *)((uint8_t *)stage + nb_a); d_prm = (int32_t *)((uint8_t *)stage + 2 * nb_a); d_st = (double *)((uint8_t *)stage + 2 * nb_a + pb_a);
    ret = LNN_NG;
    if (hipMemcpyAsync(d_pcm, pcm, nb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "H2D failed"); goto done; }
    if (hipMemsetAsync(d_prm, 0, pb, ctx->stream) != hipSuccess || hipMemsetAsync(d_st, 0, sb, ctx->stream) != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "memset failed"); goto done; }
    ret = LINNEAmd_EncodeFramesDevice(ctx, shape, d_pcm, num_samples, num_frames, d_res, d_prm, d_st);
    if (ret != LNN_OK) goto done;
    ret = LNN_NG;
    if (hipMemcpyAsync(residual, d_res, nb, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess
            || hipMemcpyAsync(params, d_prm, pb, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess
            || hipMemcpyAsync(stats, d_st, sb, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "D2H failed"); goto done; }
    {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "stream sync: %s", hipGetErrorString(e)); goto done; }
    }
    ret = LNN_OK;
done:
    if (ret != LNN_OK || transient) hipStreamSynchronize(ctx->stream);
    if (transient) hipFree(stage);
    return ret;
}

extern "C" int LINNEAmd_DecodeFramesHost(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        int32_t *data, const uint32_t *num_samples, uint32_t num_frames, const int32_t *params)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    if (!shape || !data || !params) return LNN_INVALID_ARGUMENT;
    if (num_frames == 0) return LNN_OK;
    { HostShape hs_; int r_ = shape_info(shape, &hs_); if (r_ != LNN_OK) { snprintf(ctx->err, sizeof(ctx->err), "invalid shape"); return r_; }
      if ((r_ = params_in_range(ctx, &hs_, shape->num_channels, params, num_frames)) != LNN_OK) return r_; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t CS = (uint64_t)shape->num_channels * shape->num_samples_per_block;
    const uint64_t nb = sizeof(int32_t) * CS * num_frames, pb = sizeof(int32_t) * LINNE_AMD_PARAM_WORDS * (uint64_t)shape->num_channels * num_frames;
    int32_t *d_data = NULL, *d_prm = NULL;
    void *stage = NULL; int transient = 0;
    int ret = hstage_get(ctx, align_up(nb) + pb, &stage, &transient);
    if (ret != LNN_OK) return ret;
    d_data = (int32_t *)stage; d_prm = (int32_t *)((uint8_t *)stage + align_up(nb));
    ret = LNN_NG;
    if (hipMemcpyAsync(d_data, data, nb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess
            || hipMemcpyAsync(d_prm, params, pb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "H2D failed"); goto done; }
    ret = LINNEAmd_DecodeFramesDevice(ctx, shape, d_data, num_samples, num_frames, d_prm);
    if (ret != LNN_OK) goto done;
    ret = LNN_NG;
    if (hipMemcpyAsync(data, d_data, nb, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "D2H failed"); goto done; }
    {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "stream sync: %s", hipGetErrorString(e)); goto done; }
    }
    ret = LNN_OK;
done:
    if (ret != LNN_OK || transient) hipStreamSynchronize(ctx->stream);
    if (transient) hipFree(stage);
    return ret;
}


extern "C" int LINNEAmd_RicePlanDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        const int32_t *d_residual, const uint32_t *h_num_samples, uint32_t num_frames, uint8_t *d_plan)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->err[0] = 0;
    if (!shape || !d_residual || !d_plan) { snprintf(ctx->err, sizeof(ctx->err), "null argument"); return LNN_INVALID_ARGUMENT; }
    if (num_frames == 0) return LNN_OK;
    HostShape hs;
    int ret = shape_info(shape, &hs);
    if (ret != LNN_OK) { snprintf(ctx->err, sizeof(ctx->err), "invalid shape"); return ret; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->rice_nsteps == 0) ctx->rice_nsteps = lnn_rice_k2_steps(ctx->rice_steps);
    int m;
    if ((ret = meta_acquire(ctx, num_frames, &m)) != LNN_OK) return ret;
    uint32_t *nsm = ctx->meta_h[m];
    if ((ret = copy_lengths(ctx, shape, h_num_samples, num_frames, nsm)) != LNN_OK) return ret;
    if ((ret = ensure_buf(ctx, (void **)&ctx->d_plan_nsmp, &ctx->plan_nsmp_cap, sizeof(uint32_t) * (uint64_t)num_frames)) != LNN_OK) return ret;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_plan_nsmp, nsm, sizeof(uint32_t) * num_frames, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->meta_ev[m], ctx->stream));
    ctx->meta_used[m] = 1;
    RicePlanArgs a; memset(&a, 0, sizeof(a));
    a.resid = d_residual; a.nsmp = ctx->d_plan_nsmp; a.plan = d_plan; a.C = shape->num_channels; a.S = shape->num_samples_per_block;
    a.nsteps = ctx->rice_nsteps;
    for (uint32_t i = 0; i < 32; i++) a.steps[i] = ctx->rice_steps[i];
    a.guard = ctx->rice_guard > 0.0 ? ctx->rice_guard : LNN_RICE_GUARD;
    const uint64_t CF = (uint64_t)num_frames * shape->num_channels;
    for (uint64_t c0 = 0; c0 < CF; ) {        /* grid.x limit: split very large batches on frame boundaries */
        uint64_t cnt = CF - c0;
        const uint64_t lim = (0x7FFFFFFFull / a.C) * a.C;
        if (cnt > lim) cnt = lim;
        RicePlanArgs b = a;
        b.resid = d_residual + c0 * a.S; b.plan = d_plan + c0 * LINNE_AMD_RICE_PLAN_BYTES; b.nsmp = ctx->d_plan_nsmp + c0 / a.C;
        const int sp_ = span_begin(ctx, LINNE_AMD_T_RICE_PLAN, ctx->stream);
        if (b.S <= REMIT_LDS_SAMPLES) hipLaunchKernelGGL(k_rice_plan<true>, dim3((uint32_t)cnt), dim3(RICE_THREADS), sizeof(uint32_t) * (b.S + 1025u), ctx->stream, b);
        else hipLaunchKernelGGL(k_rice_plan<false>, dim3((uint32_t)cnt), dim3(RICE_THREADS), 0, ctx->stream, b);
        span_end(ctx, sp_, ctx->stream);
        c0 += cnt;
    }
    HIPCHK(ctx, hipGetLastError());
    return LNN_OK;
}

/* Rice emission on the device: see lnn_k_rice.h.  d_plan is RicePlanDevice's output for the same batch (it carries every
 * channel's code length); enqueues the scan and the emission on the context's stream. */
extern "C" int LINNEAmd_RiceEmitDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        const int32_t *d_residual, uint32_t num_frames, const uint8_t *d_plan,
        uint32_t *d_offsets, uint8_t *d_packed, uint64_t packed_capacity)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->err[0] = 0;
    if (!shape || !d_residual || !d_plan || !d_offsets || !d_packed) { snprintf(ctx->err, sizeof(ctx->err), "null argument"); return LNN_INVALID_ARGUMENT; }
    if (num_frames == 0) return LNN_OK;
    const uint64_t CF = (uint64_t)num_frames * shape->num_channels;
    if (CF > 0x7FFFFFFFull || ctx->plan_nsmp_cap < sizeof(uint32_t) * (uint64_t)num_frames) { snprintf(ctx->err, sizeof(ctx->err), "RiceEmitDevice: call RicePlanDevice for the same batch first"); return LNN_INVALID_ARGUMENT; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RiceEmitArgs a; memset(&a, 0, sizeof(a));
    a.resid = d_residual; a.nsmp = ctx->d_plan_nsmp; a.plan = d_plan; a.offsets = d_offsets; a.packed = d_packed;
    a.packed_cap = packed_capacity & ~(uint64_t)15; a.C = shape->num_channels; a.S = shape->num_samples_per_block; a.CF = (uint32_t)CF;
    a.cap_bytes = shape->num_samples_per_block * 4u;
    { const char *e_ = getenv("LINNE_AMD_RICE_EMIT_CAP"); if (e_) a.cap_bytes = (uint32_t)atol(e_); }      /* test knob: forces the host fallback */
    { const int sp_ = span_begin(ctx, LINNE_AMD_T_RICE_EMIT, ctx->stream);
      hipLaunchKernelGGL(k_rice_scan, dim3(1), dim3(RSCAN_THREADS), 0, ctx->stream, a);
      if (a.S <= REMIT_LDS_SAMPLES) hipLaunchKernelGGL(k_rice_emit<true>, dim3((uint32_t)CF), dim3(REMIT_THREADS), sizeof(uint32_t) * (a.S + REMIT_THREADS + 1u), ctx->stream, a);
      else hipLaunchKernelGGL(k_rice_emit<false>, dim3((uint32_t)CF), dim3(REMIT_THREADS), 0, ctx->stream, a);
      span_end(ctx, sp_, ctx->stream); }
    HIPCHK(ctx, hipGetLastError());
    return LNN_OK;
}

/* k_rice_decode over the F frames of one segment (seg: 4-byte aligned, nbytes of it valid, zero padded to 8 bytes), under its span,
 * on st.  bitend may be NULL: the codes may run to the segment's end */
static int rice_decode_launch(LINNEAmdContext *ctx, hipStream_t st, const struct LINNEAmdShape *shape, const uint8_t *seg, uint64_t nbytes,
        const uint64_t *bitpos, const uint64_t *bitend, const uint32_t *nsmp, uint32_t F, int32_t *resid, uint64_t *endbit)
{
    RiceDecodeArgs a; memset(&a, 0, sizeof(a));
    a.words = (const uint32_t *)seg; a.nbytes = nbytes; a.bitpos = bitpos; a.bitend = bitend; a.nsmp = nsmp; a.resid = resid; a.endbit = endbit;
    a.F = F; a.C = shape->num_channels; a.S = shape->num_samples_per_block;
    const int sp_ = span_begin(ctx, LINNE_AMD_T_RICE_DECODE, st);
    hipLaunchKernelGGL(k_rice_decode, dim3((F + RDEC_THREADS - 1u) / RDEC_THREADS), dim3(RDEC_THREADS), 0, st, a);
    span_end(ctx, sp_, st);
    HIPCHK(ctx, hipGetLastError());
    return LNN_OK;
}

/* Rice decoding on the device: see lnn_k_rice.h.  d_stream: the bytes of a group of blocks (4-byte aligned; stream_bytes of it
 * valid, readable up to the next multiple of 8); d_bitpos[f]: where frame f's first channel's code starts (~0: skip the frame);
 * d_endbit[f] receives the bit position behind its last channel's code (~0: the stream held something no encoder writes: the host
 * must decode this group itself).  Enqueues on the context's stream. */
extern "C" int LINNEAmd_RiceDecodeDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_bitpos, const uint32_t *h_num_samples, uint32_t num_frames,
        int32_t *d_residual, uint64_t *d_endbit)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->err[0] = 0;
    if (!shape || !d_stream || !d_bitpos || !d_residual || !d_endbit || ((uintptr_t)d_stream & 3u)) { snprintf(ctx->err, sizeof(ctx->err), "RiceDecodeDevice: null or misaligned argument"); return LNN_INVALID_ARGUMENT; }
    if (num_frames == 0) return LNN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int ret = upload_lengths(ctx, shape, h_num_samples, num_frames);
    if (ret != LNN_OK) return ret;
    return rice_decode_launch(ctx, ctx->stream, shape, d_stream, stream_bytes, d_bitpos, NULL, ctx->d_nsmp, num_frames, d_residual, d_endbit);
}

/* ================================================================================================
 * staging slots: pinned host buffers + device buffers for a group of frames.  Submit enqueues H2D (copy-in
 * stream), the kernels (context stream) and D2H (copy-out stream) chained by events and returns at once, so a
 * caller that rotates over a few slots overlaps its own host work (entropy stage), PCIe and the kernels.
 * ============================================================================================== */
struct LINNEAmdSlot {
    LINNEAmdContext *ctx; struct LINNEAmdShape shape; uint32_t max_frames; int for_encode; uint32_t flags;
    int32_t *h_pcm, *h_data, *h_prm; double *h_st; uint8_t *h_plan;
    int32_t *d_pcm, *d_data, *d_prm; double *d_st; uint8_t *d_plan;
    /* emit mode: the channels' Rice code, packed back to back, instead of the residual */
    uint8_t *h_packed, *d_packed; uint64_t packed_cap; uint32_t *h_offsets, *d_offsets;
    /* decode, stream mode: the blocks' bytes instead of the residual; PCM optionally as int16 */
    uint8_t *h_stream, *d_stream; uint64_t stream_cap; uint64_t *h_bitpos, *d_bitpos, *h_endbit, *d_endbit; int16_t *h_out16, *d_out16; uint32_t *d_flag, *h_flag;
    hipStream_t in_stream;      /* stream mode: the stream of this slot's Rice decoder, one of the context's pool (not owned) */
    hipEvent_t ev_in, ev_k, ev_done; int pending;
};

static int ctx_copy_streams(LINNEAmdContext *ctx)
{
    if (ctx->has_copy) return LNN_OK;
    /* The three kinds of work a staging pipeline overlaps must sit on different hardware queues: streams that share one run in order
     * whatever their events allow (an H2D behind a kernel that waits for another group's decoder: DecodeWhole took 67 ms in one process
     * and 25 in another, by which queue the copy-in stream had drawn).  Which queue of a priority level's pool a stream gets is
     * round-robin over everything the process ever created at that level -- so the copy-in stream (and the Rice decoders' streams) are
     * created at HIGH priority and the copy-out stream at LOW: three pools, and in each only this library's streams. */
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);          /* (numerically lowest = highest priority) */
    if (hipStreamCreateWithPriority(&ctx->copy_in, hipStreamNonBlocking, prio_hi) != hipSuccess) {        /* (a runtime without priorities: plain streams) */
        (void)hipGetLastError();
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking));
    }
    if (hipStreamCreateWithPriority(&ctx->copy_out, hipStreamNonBlocking, prio_lo) != hipSuccess) {
        (void)hipGetLastError();
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking));
    }
    ctx->has_copy = 1;
    return LNN_OK;
}

extern "C" void LINNEAmd_SlotDestroy(struct LINNEAmdSlot *s)
{
    if (!s) return;
    hipSetDevice(s->ctx->device);
    if (s->pending) hipEventSynchronize(s->ev_done);
    if (s->in_stream) hipStreamSynchronize(s->in_stream);
    if (s->h_pcm) hipHostFree(s->h_pcm);
    if (s->h_data) hipHostFree(s->h_data);
    if (s->h_prm) hipHostFree(s->h_prm);
    if (s->h_st) hipHostFree(s->h_st);
    if (s->h_plan) hipHostFree(s->h_plan);
    if (s->d_plan) hipFree(s->d_plan);
    if (s->h_packed) hipHostFree(s->h_packed);
    if (s->d_packed) hipFree(s->d_packed);
    if (s->h_offsets) hipHostFree(s->h_offsets);
    if (s->d_offsets) hipFree(s->d_offsets);
    if (s->h_stream) hipHostFree(s->h_stream);
    if (s->d_stream) hipFree(s->d_stream);
    if (s->h_bitpos) hipHostFree(s->h_bitpos);
    if (s->d_bitpos) hipFree(s->d_bitpos);
    if (s->h_endbit) hipHostFree(s->h_endbit);
    if (s->d_endbit) hipFree(s->d_endbit);
    if (s->h_out16) hipHostFree(s->h_out16);
    if (s->d_out16) hipFree(s->d_out16);
    if (s->h_flag) hipHostFree(s->h_flag);
    if (s->d_flag) hipFree(s->d_flag);
    if (s->d_pcm) hipFree(s->d_pcm);
    if (s->d_data) hipFree(s->d_data);
    if (s->d_prm) hipFree(s->d_prm);
    if (s->d_st) hipFree(s->d_st);
    if (s->ev_in) hipEventDestroy(s->ev_in);
    if (s->ev_k) hipEventDestroy(s->ev_k);
    if (s->ev_done) hipEventDestroy(s->ev_done);
    free(s);
}

extern "C" struct LINNEAmdSlot *LINNEAmd_SlotCreate(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        uint32_t max_frames, int for_encode)
{
    return LINNEAmd_SlotCreateEx(ctx, shape, max_frames, for_encode, 0u);
}

extern "C" struct LINNEAmdSlot *LINNEAmd_SlotCreateEx(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        uint32_t max_frames, int for_encode, uint32_t flags)
{
    HostShape hs;
    if (!ctx) return NULL;
    ctx->err[0] = 0;
    if (!shape || max_frames == 0 || shape_info(shape, &hs) != LNN_OK) { snprintf(ctx->err, sizeof(ctx->err), "SlotCreate: invalid shape"); return NULL; }
    if (hipSetDevice(ctx->device) != hipSuccess || ctx_copy_streams(ctx) != LNN_OK) return NULL;
    LINNEAmdSlot *s = (LINNEAmdSlot *)calloc(1, sizeof(*s));
    if (!s) return NULL;
    if (!for_encode) flags &= (LINNE_AMD_SLOT_STREAM | LINNE_AMD_SLOT_PCM16); else flags &= ~(uint32_t)LINNE_AMD_SLOT_STREAM;
    if (shape->bits_per_sample > 24) flags &= ~(uint32_t)LINNE_AMD_SLOT_PCM16;          /* narrow staging: 2 bytes up to 16 bits, 3 packed bytes up to 24 */
    s->ctx = ctx; s->shape = *shape; s->max_frames = max_frames; s->for_encode = for_encode; s->flags = flags;
    const uint64_t CS = (uint64_t)shape->num_channels * shape->num_samples_per_block;
    const uint64_t nb = sizeof(int32_t) * CS * max_frames, pb = sizeof(int32_t) * LINNE_AMD_PARAM_WORDS * (uint64_t)shape->num_channels * max_frames,
                   sb = sizeof(double) * LINNE_AMD_STAT_WORDS * (uint64_t)shape->num_channels * max_frames;
    hipError_t e = hipSuccess;
    const bool emit = (flags & LINNE_AMD_SLOT_EMIT) != 0, pcm16 = (flags & LINNE_AMD_SLOT_PCM16) != 0;
    const uint64_t nbn = pcm16 ? nb / 4u * (shape->bits_per_sample <= 16 ? 2u : 3u) : nb;      /* bytes of the narrow PCM image */
    /* emit mode: the residual stays on the device; stream-mode decode with int16 PCM: the int32 PCM is only fetched when a block's
     * samples leave the 16-bit range (LINNEAmd_SlotFetchPcm32 allocates then) */
    const bool lazy_data = !for_encode && (flags & LINNE_AMD_SLOT_STREAM) && pcm16;
    if (e == hipSuccess && !emit && !lazy_data) e = hipHostMalloc((void **)&s->h_data, nb, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_prm, pb, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_data, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_prm, pb);
    if (for_encode) {
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_pcm, nbn, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_st, sb, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_pcm, nbn);
        if (emit) {
            /* room for the code of a group: what the samples' own width would take, a little more than any audio that is
             * not emitted RAW anyway needs; channels that do not fit fall back to the host (offset 0xFFFFFFFF) */
            const uint64_t CF = (uint64_t)shape->num_channels * max_frames;
            s->packed_cap = (CF * ((uint64_t)shape->num_samples_per_block * ((shape->bits_per_sample + 7u) / 8u) + 64u) + 4095u) & ~(uint64_t)4095u;
            if (s->packed_cap > 0xFFFFFFF0ull) s->packed_cap = 0xFFFFF000ull;
            if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_packed, s->packed_cap, hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc((void **)&s->d_packed, s->packed_cap);
            if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_offsets, sizeof(uint32_t) * (CF + 1), hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc((void **)&s->d_offsets, sizeof(uint32_t) * (CF + 1));
        }
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_st, sb);
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_plan, (uint64_t)LINNE_AMD_RICE_PLAN_BYTES * shape->num_channels * max_frames, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_plan, (uint64_t)LINNE_AMD_RICE_PLAN_BYTES * shape->num_channels * max_frames);
    }
    if (!for_encode && (flags & LINNE_AMD_SLOT_STREAM)) {
        /* room for the blocks' bytes: what RAW blocks take, and a little more (a COMPRESS block is chosen on an estimate and may
         * come out larger: a group that does not fit is decoded the other way, lnn_api.c) */
        s->stream_cap = ((uint64_t)max_frames * (CS * ((shape->bits_per_sample + 7u) / 8u) + CS / 8u + 1024u) + 4095u) & ~(uint64_t)4095u;
        if (e == hipSuccess) {
            const int k = ctx->rice_next++ % LNN_RICE_STREAMS;
            if (k >= ctx->n_rice_pool) {
                /* HIGH priority: the runtime keeps a pool of hardware queues per priority level, so these streams cannot land on the
                 * queue of the synthesis or of a copy stream whatever else the process created before (which of the normal pool's
                 * queues a stream gets is round-robin over the process's whole history: DecodeWhole took 25 ms in one process and
                 * 67 ms in another before this) -- and a launch of a few dozen latency-bound waves is what should go first anyway */
                int lo = 0, hi = 0;
                (void)hipDeviceGetStreamPriorityRange(&lo, &hi);      /* (numerically lowest = highest priority) */
                e = hipStreamCreateWithPriority(&ctx->rice_pool[k], hipStreamNonBlocking, hi);
                if (e != hipSuccess) { (void)hipGetLastError(); e = hipStreamCreateWithFlags(&ctx->rice_pool[k], hipStreamNonBlocking); }
                if (e == hipSuccess) ctx->n_rice_pool = k + 1;
            }
            if (e == hipSuccess) s->in_stream = ctx->rice_pool[k];
        }
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_stream, s->stream_cap + 16, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_stream, s->stream_cap + 16);
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_bitpos, (2 * sizeof(uint64_t) + sizeof(uint32_t)) * max_frames, hipHostMallocDefault);      /* positions, the blocks' ends, the frames' lengths */
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_bitpos, (2 * sizeof(uint64_t) + sizeof(uint32_t)) * max_frames);
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_endbit, sizeof(uint64_t) * max_frames, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_endbit, sizeof(uint64_t) * max_frames);
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_flag, sizeof(uint32_t) * 4, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_flag, sizeof(uint32_t) * 4);
        if (flags & LINNE_AMD_SLOT_PCM16) {
            if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_out16, nbn, hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc((void **)&s->d_out16, nbn);
        }
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_k, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming);
    if (e != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "SlotCreate: %s", hipGetErrorString(e)); LINNEAmd_SlotDestroy(s); return NULL; }
    return s;
}

extern "C" int32_t *LINNEAmd_SlotPcm(struct LINNEAmdSlot *s) { return (s && !(s->flags & LINNE_AMD_SLOT_PCM16)) ? s->h_pcm : NULL; }
extern "C" int16_t *LINNEAmd_SlotPcm16(struct LINNEAmdSlot *s) { return (s && (s->flags & LINNE_AMD_SLOT_PCM16)) ? (s->for_encode ? (int16_t *)s->h_pcm : s->h_out16) : NULL; }
extern "C" uint32_t LINNEAmd_SlotPcmWidth(const struct LINNEAmdSlot *s) { return !s ? 0u : (!(s->flags & LINNE_AMD_SLOT_PCM16) ? 4u : (s->shape.bits_per_sample <= 16 ? 2u : 3u)); }
extern "C" uint8_t *LINNEAmd_SlotStream(struct LINNEAmdSlot *s) { return s ? s->h_stream : NULL; }
extern "C" uint64_t LINNEAmd_SlotStreamCapacity(const struct LINNEAmdSlot *s) { return s ? s->stream_cap : 0; }
extern "C" uint64_t *LINNEAmd_SlotBitPos(struct LINNEAmdSlot *s) { return s ? s->h_bitpos : NULL; }
extern "C" uint64_t *LINNEAmd_SlotBitEnd(struct LINNEAmdSlot *s) { return (s && s->h_bitpos) ? s->h_bitpos + s->max_frames : NULL; }
extern "C" const uint64_t *LINNEAmd_SlotEndBits(struct LINNEAmdSlot *s) { return s ? s->h_endbit : NULL; }
extern "C" int LINNEAmd_SlotPcm16Valid(const struct LINNEAmdSlot *s) { return (s && s->h_out16 && s->h_flag) ? (s->h_flag[0] == 0u) : 0; }
extern "C" const uint8_t *LINNEAmd_SlotPacked(struct LINNEAmdSlot *s) { return s ? s->h_packed : NULL; }
extern "C" const uint32_t *LINNEAmd_SlotOffsets(struct LINNEAmdSlot *s) { return s ? s->h_offsets : NULL; }
extern "C" uint32_t LINNEAmd_SlotFlags(const struct LINNEAmdSlot *s) { return s ? s->flags : 0; }

/* emit mode keeps the residual on the device; the host asks for a frame's residual only when it has to code a channel
 * itself (flagged plan, code that did not fit): synchronous, valid until the slot is submitted again */
extern "C" int LINNEAmd_SlotFetchResidual(struct LINNEAmdSlot *s, uint32_t frame, int32_t *dst)
{
    if (!s || !dst || !s->for_encode || frame >= s->max_frames) return LNN_INVALID_ARGUMENT;
    const uint64_t fb = sizeof(int32_t) * (uint64_t)s->shape.num_channels * s->shape.num_samples_per_block;
    if (hipSetDevice(s->ctx->device) != hipSuccess || hipMemcpy(dst, (const uint8_t *)s->d_data + fb * frame, fb, hipMemcpyDeviceToHost) != hipSuccess) return LNN_NG;
    return LNN_OK;
}
extern "C" int32_t *LINNEAmd_SlotData(struct LINNEAmdSlot *s) { return s ? s->h_data : NULL; }
extern "C" int32_t *LINNEAmd_SlotParams(struct LINNEAmdSlot *s) { return s ? s->h_prm : NULL; }
extern "C" double *LINNEAmd_SlotStats(struct LINNEAmdSlot *s) { return s ? s->h_st : NULL; }
extern "C" uint8_t *LINNEAmd_SlotRicePlan(struct LINNEAmdSlot *s) { return s ? s->h_plan : NULL; }
extern "C" uint32_t LINNEAmd_SlotCapacity(const struct LINNEAmdSlot *s) { return s ? s->max_frames : 0; }

extern "C" int LINNEAmd_SlotWait(struct LINNEAmdSlot *s)
{
    if (!s) return LNN_INVALID_ARGUMENT;
    if (!s->pending) return LNN_OK;
    HIPCHK(s->ctx, hipEventSynchronize(s->ev_done));
    s->pending = 0;
    return LNN_OK;
}

extern "C" int LINNEAmd_SlotEncodeSubmit(struct LINNEAmdSlot *s, const uint32_t *num_samples, uint32_t num_frames)
{
    if (!s || !s->for_encode) return LNN_INVALID_ARGUMENT;
    LINNEAmdContext *ctx = s->ctx;
    if (num_frames == 0 || num_frames > s->max_frames) { snprintf(ctx->err, sizeof(ctx->err), "SlotEncodeSubmit: %u frames in a slot of %u", num_frames, s->max_frames); return LNN_INVALID_ARGUMENT; }
    int ret = LINNEAmd_SlotWait(s);
    if (ret != LNN_OK) return ret;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t C = s->shape.num_channels, CS = C * s->shape.num_samples_per_block;
    const uint64_t nb = sizeof(int32_t) * CS * num_frames, pb = sizeof(int32_t) * LINNE_AMD_PARAM_WORDS * C * num_frames, sb = sizeof(double) * LINNE_AMD_STAT_WORDS * C * num_frames;
    const bool emit = (s->flags & LINNE_AMD_SLOT_EMIT) != 0, pcm16 = (s->flags & LINNE_AMD_SLOT_PCM16) != 0;
    const uint32_t width = LINNEAmd_SlotPcmWidth(s);
    HIPCHK(ctx, hipMemcpyAsync(s->d_pcm, s->h_pcm, nb / 4u * width, hipMemcpyHostToDevice, ctx->copy_in));
    HIPCHK(ctx, hipEventRecord(s->ev_in, ctx->copy_in));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, s->ev_in, 0));
    HIPCHK(ctx, hipMemsetAsync(s->d_st, 0, sb, ctx->stream));
    ctx->pcm16_next = pcm16 ? (width == 2u ? 1 : 2) : 0;
    if ((ret = LINNEAmd_EncodeFramesDevice(ctx, &s->shape, s->d_pcm, num_samples, num_frames, s->d_data, s->d_prm, s->d_st)) != LNN_OK) return ret;
    /* The Rice planning and emission are light integer kernels behind the analysis: they run on the copy-out stream, where
     * they overlap the next group's (FP64-bound) analysis instead of delaying it; the slots of a context share that stream,
     * so their use of the context's plan metadata stays ordered. */
    HIPCHK(ctx, hipEventRecord(s->ev_k, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_out, s->ev_k, 0));
    {
        hipStream_t keep = ctx->stream;
        ctx->stream = ctx->copy_out;
        ret = LINNEAmd_RicePlanDevice(ctx, &s->shape, s->d_data, num_samples, num_frames, s->d_plan);
        if (ret == LNN_OK && emit) ret = LINNEAmd_RiceEmitDevice(ctx, &s->shape, s->d_data, num_frames, s->d_plan, s->d_offsets, s->d_packed, s->packed_cap);
        ctx->stream = keep;
        if (ret != LNN_OK) return ret;
    }
    if (emit) {         /* the code's used bytes (a size only the device knows so far) by a copy kernel, then the offsets */
        hipLaunchKernelGGL(k_copy_out, dim3(96), dim3(256), 0, ctx->copy_out, (const uint4 *)s->d_packed, (uint4 *)s->h_packed, (const uint32_t *)(s->d_offsets + (size_t)C * num_frames));
        HIPCHK(ctx, hipMemcpyAsync(s->h_offsets, s->d_offsets, sizeof(uint32_t) * (C * num_frames + 1), hipMemcpyDeviceToHost, ctx->copy_out));
    } else
    HIPCHK(ctx, hipMemcpyAsync(s->h_data, s->d_data, nb, hipMemcpyDeviceToHost, ctx->copy_out));
    HIPCHK(ctx, hipMemcpyAsync(s->h_prm, s->d_prm, pb, hipMemcpyDeviceToHost, ctx->copy_out));
    HIPCHK(ctx, hipMemcpyAsync(s->h_st, s->d_st, sb, hipMemcpyDeviceToHost, ctx->copy_out));
    HIPCHK(ctx, hipMemcpyAsync(s->h_plan, s->d_plan, (uint64_t)LINNE_AMD_RICE_PLAN_BYTES * C * num_frames, hipMemcpyDeviceToHost, ctx->copy_out));
    HIPCHK(ctx, hipEventRecord(s->ev_done, ctx->copy_out));
    s->pending = 1;
    return LNN_OK;
}

extern "C" int LINNEAmd_SlotDecodeSubmit(struct LINNEAmdSlot *s, const uint32_t *num_samples, uint32_t num_frames)
{
    if (!s) return LNN_INVALID_ARGUMENT;
    LINNEAmdContext *ctx = s->ctx;
    if (num_frames == 0 || num_frames > s->max_frames) { snprintf(ctx->err, sizeof(ctx->err), "SlotDecodeSubmit: %u frames in a slot of %u", num_frames, s->max_frames); return LNN_INVALID_ARGUMENT; }
    int ret = LINNEAmd_SlotWait(s);
    if (ret != LNN_OK) return ret;
    { HostShape hs_; if ((ret = shape_info(&s->shape, &hs_)) != LNN_OK || (ret = params_in_range(ctx, &hs_, s->shape.num_channels, s->h_prm, num_frames)) != LNN_OK) return ret; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t C = s->shape.num_channels, CS = C * s->shape.num_samples_per_block;
    const uint64_t nb = sizeof(int32_t) * CS * num_frames, pb = sizeof(int32_t) * LINNE_AMD_PARAM_WORDS * C * num_frames;
    HIPCHK(ctx, hipMemcpyAsync(s->d_data, s->h_data, nb, hipMemcpyHostToDevice, ctx->copy_in));
    HIPCHK(ctx, hipMemcpyAsync(s->d_prm, s->h_prm, pb, hipMemcpyHostToDevice, ctx->copy_in));
    HIPCHK(ctx, hipEventRecord(s->ev_in, ctx->copy_in));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, s->ev_in, 0));
    if ((ret = LINNEAmd_DecodeFramesDevice(ctx, &s->shape, s->d_data, num_samples, num_frames, s->d_prm)) != LNN_OK) return ret;
    HIPCHK(ctx, hipEventRecord(s->ev_k, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_out, s->ev_k, 0));
    HIPCHK(ctx, hipMemcpyAsync(s->h_data, s->d_data, nb, hipMemcpyDeviceToHost, ctx->copy_out));
    HIPCHK(ctx, hipEventRecord(s->ev_done, ctx->copy_out));
    s->pending = 1;
    return LNN_OK;
}

/* decode slot in stream mode: SlotStream holds the blocks' bytes (stream_bytes of them), SlotBitPos[f] where frame f's Rice code
 * starts, SlotParams the parameters; H2D, Rice decoding, synthesis, [int16 narrowing], D2H are enqueued; after SlotWait:
 * SlotEndBits (~0 anywhere: decode this group on the host instead), SlotData or -- if SlotPcm16Valid -- SlotPcm16 */
extern "C" int LINNEAmd_SlotDecodeStreamSubmit(struct LINNEAmdSlot *s, uint64_t stream_bytes, const uint32_t *num_samples, uint32_t num_frames)
{
    if (!s || s->for_encode || !s->h_stream) return LNN_INVALID_ARGUMENT;
    LINNEAmdContext *ctx = s->ctx;
    if (num_frames == 0 || num_frames > s->max_frames || stream_bytes > s->stream_cap) { snprintf(ctx->err, sizeof(ctx->err), "SlotDecodeStreamSubmit: %u frames / %llu bytes in a slot of %u / %llu", num_frames, (unsigned long long)stream_bytes, s->max_frames, (unsigned long long)s->stream_cap); return LNN_INVALID_ARGUMENT; }
    int ret = LINNEAmd_SlotWait(s);
    if (ret != LNN_OK) return ret;
    { HostShape hs_; if ((ret = shape_info(&s->shape, &hs_)) != LNN_OK || (ret = params_in_range(ctx, &hs_, s->shape.num_channels, s->h_prm, num_frames)) != LNN_OK) return ret; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    /* the copies in on the context's copy-in stream, one group behind the other; the Rice decoder on one of the pooled streams, so that
     * the groups' decoders run side by side (a pooled stream is shared by every fourth group: its decoder waits for the one four groups
     * back, which has had 9 ms by then) */
    hipStream_t cin = ctx->copy_in, rst = s->in_stream ? s->in_stream : ctx->copy_in;
    const uint64_t C = s->shape.num_channels, CS = C * s->shape.num_samples_per_block;
    const uint64_t nb = sizeof(int32_t) * CS * num_frames, pb = sizeof(int32_t) * LINNE_AMD_PARAM_WORDS * C * num_frames;
    memset(s->h_stream + stream_bytes, 0, 16);                 /* the reader loads whole 8-byte words */
    HIPCHK(ctx, hipMemcpyAsync(s->d_stream, s->h_stream, (stream_bytes + 15u) & ~(uint64_t)7u, hipMemcpyHostToDevice, cin));
    /* the frames' lengths travel with the bit positions: the Rice decoder runs on the copy-in stream, beside the synthesis of the
     * group before (k_rice_decode has a wave per 64 frames -- a few dozen waves -- and leaves the chip to it) */
    if ((ret = copy_lengths(ctx, &s->shape, num_samples, num_frames, (uint32_t *)(s->h_bitpos + 2 * (size_t)s->max_frames))) != LNN_OK) return ret;
    HIPCHK(ctx, hipMemcpyAsync(s->d_bitpos, s->h_bitpos, 2 * sizeof(uint64_t) * s->max_frames + sizeof(uint32_t) * num_frames, hipMemcpyHostToDevice, cin));
    HIPCHK(ctx, hipMemcpyAsync(s->d_prm, s->h_prm, pb, hipMemcpyHostToDevice, cin));
    if (rst != cin) { HIPCHK(ctx, hipEventRecord(s->ev_in, cin)); HIPCHK(ctx, hipStreamWaitEvent(rst, s->ev_in, 0)); }
    if ((ret = rice_decode_launch(ctx, rst, &s->shape, s->d_stream, stream_bytes, s->d_bitpos, s->d_bitpos + s->max_frames,
            (const uint32_t *)(s->d_bitpos + 2 * (size_t)s->max_frames), num_frames, s->d_data, s->d_endbit)) != LNN_OK) return ret;
    HIPCHK(ctx, hipEventRecord(s->ev_in, rst));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, s->ev_in, 0));
    if ((ret = LINNEAmd_DecodeFramesDevice(ctx, &s->shape, s->d_data, num_samples, num_frames, s->d_prm)) != LNN_OK) return ret;
    if (s->d_out16) {
        HIPCHK(ctx, hipMemsetAsync(s->d_flag, 0, sizeof(uint32_t), ctx->stream));
        if (LINNEAmd_SlotPcmWidth(s) == 2u)
            hipLaunchKernelGGL(k_narrow16, dim3(1024), dim3(256), 0, ctx->stream, (const int32_t *)s->d_data, s->d_out16, CS * num_frames, s->d_flag,
                    (const uint32_t *)(s->d_bitpos + 2 * (size_t)s->max_frames), (uint32_t)C, s->shape.num_samples_per_block);
        else
            hipLaunchKernelGGL(k_narrow24, dim3(1024), dim3(256), 0, ctx->stream, (const int32_t *)s->d_data, (uint8_t *)s->d_out16, CS * num_frames, s->d_flag,
                    (const uint32_t *)(s->d_bitpos + 2 * (size_t)s->max_frames), (uint32_t)C, s->shape.num_samples_per_block);
    }
    HIPCHK(ctx, hipEventRecord(s->ev_k, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_out, s->ev_k, 0));
    HIPCHK(ctx, hipMemcpyAsync(s->h_endbit, s->d_endbit, sizeof(uint64_t) * num_frames, hipMemcpyDeviceToHost, ctx->copy_out));
    if (s->d_out16) {
        HIPCHK(ctx, hipMemcpyAsync(s->h_flag, s->d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->copy_out));
        HIPCHK(ctx, hipMemcpyAsync(s->h_out16, s->d_out16, nb / 4u * LINNEAmd_SlotPcmWidth(s), hipMemcpyDeviceToHost, ctx->copy_out));
    } else
        HIPCHK(ctx, hipMemcpyAsync(s->h_data, s->d_data, nb, hipMemcpyDeviceToHost, ctx->copy_out));
    HIPCHK(ctx, hipEventRecord(s->ev_done, ctx->copy_out));
    s->pending = 1;
    return LNN_OK;
}

/* the int32 PCM of a stream-mode decode slot whose int16 copy is not valid (LINNEAmd_SlotPcm16Valid == 0): synchronous */
extern "C" int LINNEAmd_SlotFetchPcm32(struct LINNEAmdSlot *s, uint32_t num_frames)
{
    if (!s || s->for_encode || num_frames > s->max_frames) return LNN_INVALID_ARGUMENT;
    const uint64_t nb = sizeof(int32_t) * (uint64_t)s->shape.num_channels * s->shape.num_samples_per_block * num_frames;
    if (hipSetDevice(s->ctx->device) != hipSuccess) return LNN_NG;
    if (!s->h_data && hipHostMalloc((void **)&s->h_data, sizeof(int32_t) * (uint64_t)s->shape.num_channels * s->shape.num_samples_per_block * s->max_frames, hipHostMallocDefault) != hipSuccess) { s->h_data = NULL; return LNN_NG; }
    if (hipMemcpy(s->h_data, s->d_data, nb, hipMemcpyDeviceToHost) != hipSuccess) return LNN_NG;
    return LNN_OK;
}

/* ================================================================================================
 * .lnn streams in device memory (lnn_k_stream.h): a block index built once, then decodes of sample ranges
 * ============================================================================================== */
struct LINNEAmdStreamIndex {
    int device;
    struct LINNEHeader header; struct LINNEAmdShape shape;
    uint64_t stream_bytes;
    uint32_t nb;                        /* the blocks a whole decode walks: up to the one that reaches num_samples */
    uint64_t covered;                   /* the samples they hold (first sample of block nb) */
    int64_t fail_block;                 /* lowest failing block (nb: the place behind the last one), -1: none */
    int fail_code; uint64_t fail_off;
    uint64_t *h_off, *h_first; uint32_t *h_size, *h_type, *h_nsmp;           /* host copies */
    uint64_t *d_off, *d_first; uint32_t *d_size, *d_type, *d_nsmp; int32_t *d_status; SxTables *d_tab;
    struct SxSlab *slab;                /* the tables above are parts of the call's two allocations, freed with the last index of the call */
};
/* what the indexes of one StreamIndexesCreate call share (a StreamIndexCreate call: its one index) */
struct SxSlab { std::atomic<uint32_t> refs; int device; void *dev, *host; };
static void sx_slab_release(SxSlab *s)
{
    if (s->refs.fetch_sub(1u) != 1u) return;
    (void)hipSetDevice(s->device);
    if (s->dev) (void)hipFree(s->dev);
    free(s->host);
    delete s;
}

extern "C" void LINNEAmd_StreamIndexDestroy(struct LINNEAmdStreamIndex *x)
{
    if (!x) return;
    if (x->slab) sx_slab_release(x->slab);                         /* (NULL: an index without tables yet, as ib_open leaves it) */
    free(x);
}

/* device -> host, synchronous, behind the context's stream */
static int sx_fetch(LINNEAmdContext *ctx, void *dst, const void *src, uint64_t bytes)
{
    if (!bytes) return LNN_OK;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LNN_OK;
}
#define SX_TRY(call) do { const int r_ = (call); if (r_ != LNN_OK) return r_; } while (0)
/* a launch on the context's stream inside its span; tally: the calling call's (const LnnTally *, NULL for none) */
#define SX_LAUNCH(tally, kind, ...) do { tally_launch(tally); const int sp_ = span_begin(ctx, (kind), ctx->stream); hipLaunchKernelGGL(__VA_ARGS__); span_end(ctx, sp_, ctx->stream); HIPCHK(ctx, hipGetLastError()); } while (0)

/* ---- how the calls over many items (streams, windows, tracks, splices, repairs) end ---- */
/* the body of such a call, which may run out of host memory */
template <class Body> static int items_try(LINNEAmdContext *ctx, Body body)
{
    try { return body(); }
    catch (const std::bad_alloc &) { snprintf(ctx->err, sizeof(ctx->err), "out of host memory"); return LNN_NG; }
}
/* Behind the body and its `ret`: the end event if `record` (a body that fetches results behind its last launch records its own), the
 * wait for whatever was enqueued if `wait` (it reads the context's buffers; counted in *waits), and behind a failure of the whole
 * call every item marked.  who: the call's name in the texts of a failed wait and of a failure that left none (NULL: the body leaves
 * one with every failure).  LNN_OK or LNN_NG */
template <class Mark> static int items_end(LINNEAmdContext *ctx, const char *who, int ret, bool record, bool wait, int64_t *waits, uint32_t n, Mark mark_failed)
{
    if (record && ctx->timing) { (void)hipEventRecord(ctx->ev[1], ctx->stream); ctx->ev_valid = 1; }
    if (wait) {
        if (waits) ++*waits;
        if (hipStreamSynchronize(ctx->stream) != hipSuccess && ret == LNN_OK) { snprintf(ctx->err, sizeof(ctx->err), "%s: hipStreamSynchronize failed", who); ret = LNN_NG; }
    }
    if (ret == LNN_OK) return LNN_OK;
    if (who && !ctx->err[0]) snprintf(ctx->err, sizeof(ctx->err), "%s: failed with %d", who, ret);
    for (uint32_t i = 0; i < n; i++) mark_failed(i);
    return LNN_NG;
}
/* the text of the lowest-numbered failing item in ctx->err: behind its noun and number, bare where the call is the single one */
static void items_first_text(LINNEAmdContext *ctx, const char *noun, uint32_t i, bool single, const char *text)
{
    if (single) snprintf(ctx->err, sizeof(ctx->err), "%s", text);
    else snprintf(ctx->err, sizeof(ctx->err), "%s %u: %.*s", noun, i, (int)sizeof(ctx->err) - 24, text);
}

static void sx_tables(SxTables *t)
{
    lnn_stream_tables(t->crc, &t->root, t->child);
    /* feeding one zero byte to the CRC state c: (c >> 8) ^ crc[c & 0xFF], a linear map; level k + 1 = level k applied twice */
    for (uint32_t j = 0; j < 16u; j++) { const uint32_t c = 1u << j; t->shift[0][j] = (uint16_t)((c >> 8) ^ t->crc[c & 0xFFu]); }
    for (uint32_t k = 1; k < SX_CRC_LEVELS; k++)
        for (uint32_t j = 0; j < 16u; j++) {
            uint32_t v = t->shift[k - 1][j], r = 0;
            for (uint32_t i = 0; i < 16u; i++) if ((v >> i) & 1u) r ^= t->shift[k - 1][i];
            t->shift[k][j] = (uint16_t)r;
        }
}

extern "C" int LINNEAmd_StreamIndexHeader(const struct LINNEAmdStreamIndex *index, struct LINNEHeader *header)
{
    if (!index || !header) return LNN_INVALID_ARGUMENT;
    *header = index->header;
    return LNN_OK;
}
extern "C" uint32_t LINNEAmd_StreamIndexNumBlocks(const struct LINNEAmdStreamIndex *index) { return index ? index->nb : 0u; }

extern "C" int LINNEAmd_StreamIndexBlocks(const struct LINNEAmdStreamIndex *index, const uint64_t **off, const uint64_t **first,
        const uint32_t **size, const uint32_t **type, const uint32_t **nsmp)
{
    if (!index) return LNN_INVALID_ARGUMENT;
    if (off) *off = index->h_off;
    if (first) *first = index->h_first;
    if (size) *size = index->h_size;
    if (type) *type = index->h_type;
    if (nsmp) *nsmp = index->h_nsmp;
    return LNN_OK;
}
extern "C" int LINNEAmd_StreamIndexFailure(const struct LINNEAmdStreamIndex *index, int64_t *block, int32_t *code, uint64_t *byte)
{
    if (!index) return LNN_INVALID_ARGUMENT;
    if (block) *block = index->fail_block;
    if (code) *code = index->fail_block < 0 ? LNN_OK : index->fail_code;
    if (byte) *byte = index->fail_block < 0 ? 0u : index->fail_off;
    return LNN_OK;
}

/* ================================================================================================
 * the block indexes of many resident streams in one call (lnn_k_index_batch.h)
 * ============================================================================================== */
extern "C" int64_t LINNEAmd_GetLastIndexBatchCount(struct LINNEAmdContext *ctx, int which)
{
    if (!ctx || which < 0 || which > 4) return -1;
    return ctx->ibatch_count[which];
}

/* a stream's header, on header bytes that are on the host, as DecodeWhole reads it: LINNEDecoder_DecodeHeader, then SetHeader's checks on
 * a decoder with room for it.  *out = an index without tables, or NULL with the stream's code and text; *whole_call: the failure is no
 * answer about the stream (no host memory) and fails the call */
static int ib_open(int device, const uint8_t *hb, uint64_t stream_bytes, LINNEAmdStreamIndex **out, char *text, size_t cap, bool *whole_call)
{
    struct LINNEHeader h;
    const uint64_t hn = stream_bytes < LINNE_HEADER_SIZE ? stream_bytes : LINNE_HEADER_SIZE;
    int ret;
    *out = NULL; text[0] = 0; *whole_call = false;
    if ((ret = (int)LINNEDecoder_DecodeHeader(hb, (uint32_t)hn, &h)) != LNN_OK) { snprintf(text, cap, "stream header: LINNEDecoder_DecodeHeader -> %d", ret); return ret; }
    {
        struct LINNEDecoderConfig cfg;
        memset(&cfg, 0, sizeof(cfg));
        cfg.max_num_channels = h.num_channels ? h.num_channels : 1u; cfg.max_num_layers = LINNE_AMD_MAX_LAYERS; cfg.max_num_parameters_per_layer = 128; cfg.check_crc = 1;
        struct LINNEDecoder *dec = LINNEDecoder_Create(&cfg, NULL, 0);
        if (!dec) { snprintf(text, cap, "LINNEDecoder_Create failed"); *whole_call = true; return LNN_NG; }
        ret = (int)LINNEDecoder_SetHeader(dec, &h);
        LINNEDecoder_Destroy(dec);
        if (ret != LNN_OK) { snprintf(text, cap, "stream header: LINNEDecoder_SetHeader -> %d", ret); return ret; }
    }
    LINNEAmdStreamIndex *x = (LINNEAmdStreamIndex *)calloc(1, sizeof(LINNEAmdStreamIndex));
    if (!x) { snprintf(text, cap, "out of host memory"); *whole_call = true; return LNN_NG; }
    x->device = device; x->header = h; x->stream_bytes = stream_bytes;
    x->shape = header_shape(&h);
    HostShape hs;
    if (shape_info(&x->shape, &hs) != LNN_OK) {
        snprintf(text, cap, "stream header: a shape the device decoder does not take (%u bits, %u samples per block)", h.bits_per_sample, h.num_samples_per_block);
        free(x); return LNN_INVALID_FORMAT;
    }
    x->fail_block = -1; x->fail_code = LNN_OK;
    *out = x;
    return LNN_OK;
}

/* ---- the block-head scan of the T streams of one call: StreamIndexesCreate's, and RepairStreamsDevice's first half ----
 * Its steps, in the caller's order: ib_scan_lists, ib_scan_headers, ib_scan_candidates; then, the caller's candidate buffers (xcand)
 * being there, ib_scan_write, the caller's own successor pass, ib_scan_jumps, the caller's own chain lengths, ib_scan_chains.  The
 * scan owns the lists (pinned wstage, device wdec: lnn_block_scan.h) and the rows' counts and offsets (sdec); waits, growing buffers
 * and launches go to the caller's tally. */
struct IbScan {
    LINNEAmdContext *ctx; const char *who; bool bare;      /* the call's name in its texts; bare: a failure of the whole call inside ib_open keeps ib_open's text as it is */
    uint32_t T; LnnTally tally;
    IbLists at; uint8_t *hl, *dl;                           /* the lists on the host and on the device */
    IbStream *h_st; uint64_t *h_row0, *h_crow, *h_seg, *h_len;
    const IbStream *d_st; const uint64_t *d_row0, *d_crow; uint64_t *d_seg, *d_len;
    uint64_t nrows, M, nchain; const uint64_t *cofs;       /* (stream, wave) rows and their candidates' offsets; candidates; chain blocks */
    uint32_t K, M32, gT, gM, grow;                          /* pointer-doubling levels; the grids over streams, candidates, rows */
};

/* the lists with the caller's own parts, and the call's start: its spans and start event */
static int ib_scan_lists(IbScan &s, LINNEAmdContext *ctx, const char *who, bool bare, uint32_t T, const LnnTally &tally, uint64_t early_bytes, uint64_t late_bytes)
{
    s.ctx = ctx; s.who = who; s.bare = bare; s.T = T; s.tally = tally;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    s.at = ib_lists(T, sizeof(IbStream), IB_HDR_SLOT, early_bytes, late_bytes);
    const LnnTally wait_only = { tally.waits, NULL, NULL };       /* (the pinned list is no device allocation) */
    SX_TRY(ensure_buf(ctx, &ctx->wstage, &ctx->wstage_cap, s.at.bytes, true, &wait_only));
    SX_TRY(ensure_buf(ctx, &ctx->wdec, &ctx->wdec_cap, s.at.bytes, false, &s.tally));
    uint8_t *hl = s.hl = (uint8_t *)ctx->wstage, *dl = s.dl = (uint8_t *)ctx->wdec;
    s.h_st = (IbStream *)(hl + s.at.o_st); s.d_st = (const IbStream *)(dl + s.at.o_st);
    s.h_row0 = (uint64_t *)(hl + s.at.o_row0); s.d_row0 = (const uint64_t *)(dl + s.at.o_row0);
    s.h_crow = (uint64_t *)(hl + s.at.o_crow); s.d_crow = (const uint64_t *)(dl + s.at.o_crow);
    s.h_seg = (uint64_t *)(hl + s.at.o_seg); s.d_seg = (uint64_t *)(dl + s.at.o_seg);
    s.h_len = (uint64_t *)(hl + s.at.o_len); s.d_len = (uint64_t *)(dl + s.at.o_len);
    s.gT = (uint32_t)(((uint64_t)T + 256u) / 256u);
    s.nrows = s.M = s.nchain = 0; s.cofs = NULL; s.K = s.M32 = s.gM = s.grow = 0;
    ctx->nspans = 0;
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    return LNN_OK;
}

/* 1. the headers: one gather, one fetch, one wait; then the host reads them as DecodeWhole does (ib_open), and the streams, row0 and
 * the caller's early part go up.  bytes_of(i, &N): stream i's bytes, or NULL for a stream the caller has refused already.
 * opened(i, code, text, x): what ib_open says of stream i -- x an index without tables that is the caller's from here on (the stream's
 * record h_st[i] is filled in by then), or NULL with the stream's code and text. */
template <class BytesOf, class Opened> static int ib_scan_headers(IbScan &s, BytesOf bytes_of, Opened opened)
{
    LINNEAmdContext *ctx = s.ctx;
    const uint32_t T = s.T;
    const LnnTally *tl = &s.tally;
    char text[sizeof(ctx->err)];
    memset(s.h_st, 0, sizeof(IbStream) * (uint64_t)T);
    for (uint32_t i = 0; i < T; i++) { uint64_t N = 0; s.h_st[i].b = bytes_of(i, &N); s.h_st[i].N = s.h_st[i].b ? N : 0u; }
    HIPCHK(ctx, hipMemcpyAsync(s.dl + s.at.o_st, s.hl + s.at.o_st, sizeof(IbStream) * (uint64_t)T, hipMemcpyHostToDevice, ctx->stream));
    SX_LAUNCH(tl, LINNE_AMD_T_IB_HEADERS, k_ib_headers, dim3((uint32_t)(((uint64_t)T * IB_HDR_SLOT + 255u) / 256u)), dim3(256), 0, ctx->stream, s.d_st, T, s.dl + s.at.o_hdr);
    HIPCHK(ctx, hipMemcpyAsync(s.hl + s.at.o_hdr, s.dl + s.at.o_hdr, (uint64_t)IB_HDR_SLOT * T, hipMemcpyDeviceToHost, ctx->stream));
    SX_TRY(tally_wait(ctx, tl));
    uint64_t nrows = 0;
    for (uint32_t i = 0; i < T; i++) {
        IbStream &st = s.h_st[i];
        s.h_row0[i] = nrows;
        if (!st.b) continue;
        LINNEAmdStreamIndex *x = NULL;
        bool whole_call;
        const uint64_t N = st.N;
        const int r = ib_open(ctx->device, s.hl + s.at.o_hdr + (uint64_t)IB_HDR_SLOT * i, N, &x, text, sizeof(text), &whole_call);
        if (whole_call) {                                         /* (the single call's texts are older than the batch call and stay as they were) */
            if (s.bare) snprintf(ctx->err, sizeof(ctx->err), "%s", text);
            else snprintf(ctx->err, sizeof(ctx->err), "%s: %.*s", s.who, (int)sizeof(ctx->err) - 32, text);
            return LNN_NG;
        }
        if (r != LNN_OK) { st.b = NULL; st.N = 0; opened(i, r, text, (LINNEAmdStreamIndex *)NULL); continue; }
        st.num_samples = x->header.num_samples; st.C = x->shape.num_channels; st.S = x->shape.num_samples_per_block; st.bits = x->shape.bits_per_sample;
        opened(i, LNN_OK, text, x);
        if (N > SX_FIRST_BLOCK) nrows += (N - SX_FIRST_BLOCK + SX_WAVE_POS - 1u) / SX_WAVE_POS;
    }
    s.h_row0[T] = s.nrows = nrows;
    if (nrows >= 0x1FFFFFFFCull) { snprintf(ctx->err, sizeof(ctx->err), "%s: %llu stream bytes in one call: too many", s.who, (unsigned long long)(nrows * SX_WAVE_POS)); return LNN_NG; }
    HIPCHK(ctx, hipMemcpyAsync(s.dl + s.at.o_st, s.hl + s.at.o_st, s.at.o_crow - s.at.o_st, hipMemcpyHostToDevice, ctx->stream));
    return LNN_OK;
}

/* 2. candidates over (stream, wave) rows, numbered over the whole call; the T + 1 segment bounds come back behind one wait, and with
 * them M, and K with 2^K > the longest segment: K levels of pointer doubling cover any chain */
static int ib_scan_candidates(IbScan &s)
{
    LINNEAmdContext *ctx = s.ctx;
    const uint32_t T = s.T;
    const LnnTally *tl = &s.tally;
    const uint64_t nrows = s.nrows, o_counts = 0, o_cofs = align_up(sizeof(uint32_t) * nrows);
    SX_TRY(ensure_buf(ctx, &ctx->sdec, &ctx->sdec_cap, align_up(o_cofs + sizeof(uint64_t) * (nrows + 1u)), false, tl));
    uint32_t *counts = (uint32_t *)((uint8_t *)ctx->sdec + o_counts);
    uint64_t *cofs = (uint64_t *)((uint8_t *)ctx->sdec + o_cofs);
    s.cofs = cofs; s.grow = (uint32_t)((nrows + 3u) / 4u);
    if (nrows) SX_LAUNCH(tl, LINNE_AMD_T_SX_COUNT, k_ib_count, dim3(s.grow), dim3(256), 0, ctx->stream, s.d_st, s.d_row0, T, nrows, counts);
    SX_LAUNCH(tl, LINNE_AMD_T_SX_SCAN, k_sx_scan, dim3(1), dim3(SX_SCAN_THREADS), 0, ctx->stream, (const uint32_t *)counts, nrows, cofs);
    SX_LAUNCH(tl, LINNE_AMD_T_SX_SCAN, k_ib_seg, dim3(s.gT), dim3(256), 0, ctx->stream, (const uint64_t *)cofs, s.d_row0, T, s.d_seg);
    HIPCHK(ctx, hipMemcpyAsync(s.h_seg, s.d_seg, sizeof(uint64_t) * (T + 1ull), hipMemcpyDeviceToHost, ctx->stream));
    SX_TRY(tally_wait(ctx, tl));
    const uint64_t M = s.h_seg[T];
    if (M >= 0xFFFFFFFFull) { snprintf(ctx->err, sizeof(ctx->err), "%llu block candidates: too many", (unsigned long long)M); return LNN_NG; }
    uint64_t Mmax = 0;
    for (uint32_t i = 0; i < T; i++) if (s.h_seg[i + 1] - s.h_seg[i] > Mmax) Mmax = s.h_seg[i + 1] - s.h_seg[i];
    uint32_t K = 1;
    while ((1ull << K) <= Mmax) K++;
    s.M = M; s.K = K; s.M32 = (uint32_t)M; s.gM = (uint32_t)((M + 1u + 255u) / 256u);
    return LNN_OK;
}

/* 3. the candidates' positions into cand (M + 1 entries); the levels of jump (K of M + 1 entries) above the caller's level 0; the
 * chains' lengths, which the caller's pass has left in d_len, come back behind one wait: crow = their prefix sums, nchain their sum */
static int ib_scan_write(IbScan &s, uint64_t *cand)
{
    LINNEAmdContext *ctx = s.ctx;
    SX_LAUNCH(&s.tally, LINNE_AMD_T_SX_WRITE, k_ib_write, dim3(s.grow), dim3(256), 0, ctx->stream, s.d_st, s.d_row0, s.T, s.nrows, s.cofs, cand);
    return LNN_OK;
}
static int ib_scan_jumps(IbScan &s, uint32_t *jump)
{
    LINNEAmdContext *ctx = s.ctx;
    for (uint32_t k = 1; k < s.K; k++)
        SX_LAUNCH(&s.tally, LINNE_AMD_T_SX_JUMP, k_sx_jump, dim3(s.gM), dim3(256), 0, ctx->stream, (const uint32_t *)(jump + (uint64_t)(k - 1u) * (s.M + 1u)), jump + (uint64_t)k * (s.M + 1u), s.M32);
    return LNN_OK;
}
static int ib_scan_chains(IbScan &s)
{
    LINNEAmdContext *ctx = s.ctx;
    HIPCHK(ctx, hipMemcpyAsync(s.h_len, s.d_len, sizeof(uint64_t) * (uint64_t)s.T, hipMemcpyDeviceToHost, ctx->stream));
    SX_TRY(tally_wait(ctx, &s.tally));
    uint64_t nchain = 0;
    for (uint32_t i = 0; i < s.T; i++) { s.h_crow[i] = nchain; nchain += s.h_len[i]; }
    s.h_crow[s.T] = s.nchain = nchain;
    return LNN_OK;
}

/* The block-head scan (IbScan), then the index's own: successors, chains, first samples, checks and the slab of tables; the call's
 * waits and device allocations are counted (LINNEAmd_GetLastIndexBatchCount 3 and 4).
 * LNN_OK: every stream has its index or its own code, the lowest-numbered failing stream's text is in ctx->err (behind its number
 * unless the call is the single one) and its code in *first_code; anything else fails the whole call, and the caller destroys what
 * indexes[] holds by then */
static int ib_build(LINNEAmdContext *ctx, const uint8_t *const *d_streams, const uint64_t *stream_bytes, uint32_t T, bool single,
        struct LINNEAmdStreamIndex **indexes, int32_t *results, SxSlab **slab_out, int *first_code)
{
    const char *who = single ? "StreamIndexCreate" : "StreamIndexesCreate";
    char text[sizeof(ctx->err)];
    int64_t first_fail = -1;
    auto fail_stream = [&](uint32_t i, int code, const char *why) {
        results[i] = code;
        if (first_fail < 0 || (int64_t)i < first_fail) {
            first_fail = (int64_t)i; *first_code = code;
            items_first_text(ctx, "stream", i, single, why);
        }
    };
    /* 1. 2. the scan (the tables wait in its lists' late part for the slab); an opened stream's index is the stream's from here on */
    const LnnTally tally = { &ctx->ibatch_count[3], &ctx->ibatch_count[4], NULL }, *tl = &tally;
    IbScan s;
    SX_TRY(ib_scan_lists(s, ctx, who, single, T, tally, 0, sizeof(SxTables)));
    SX_TRY(ib_scan_headers(s,
            [&](uint32_t i, uint64_t *N) { if (!d_streams[i]) fail_stream(i, LNN_INVALID_ARGUMENT, "null stream pointer"); *N = stream_bytes[i]; return d_streams[i]; },
            [&](uint32_t i, int code, const char *why, LINNEAmdStreamIndex *x) { if (x) indexes[i] = x; else fail_stream(i, code, why); }));
    SX_TRY(ib_scan_candidates(s));
    const uint32_t K = s.K, M32 = s.M32, gT = s.gT;
    const uint64_t M = s.M, o_tab = s.at.o_late;
    uint8_t *hl = s.hl;
    const IbStream *d_st = s.d_st;
    const uint64_t *d_crow = s.d_crow, *d_seg = s.d_seg, *h_crow = s.h_crow, *h_len = s.h_len;
    ctx->ibatch_count[2] = K;
    /* 3. successors inside the segments, pointer doubling over the global array, the chains' lengths.  cand has M + 1 entries: the
     * scan of the chains' sample counts takes its place once the chains are read (no more chain blocks than candidates) */
    const uint64_t o_cand = 0, o_jump = align_up(sizeof(uint64_t) * (M + 1u));
    SX_TRY(ensure_buf(ctx, &ctx->xcand, &ctx->xcand_cap, align_up(o_jump + sizeof(uint32_t) * (uint64_t)K * (M + 1u)), false, tl));
    uint64_t *cand = (uint64_t *)((uint8_t *)ctx->xcand + o_cand);
    uint32_t *jump = (uint32_t *)((uint8_t *)ctx->xcand + o_jump);
    if (M) {
        SX_TRY(ib_scan_write(s, cand));
        SX_LAUNCH(tl, LINNE_AMD_T_SX_SUCC, k_ib_succ, dim3(s.gM), dim3(256), 0, ctx->stream, d_st, d_seg, T, (const uint64_t *)cand, M32, jump);
        SX_TRY(ib_scan_jumps(s, jump));
    }
    SX_LAUNCH(tl, LINNE_AMD_T_SX_CHAIN_LEN, k_ib_chain_len, dim3(gT), dim3(256), 0, ctx->stream, d_seg, T, (const uint64_t *)cand, (const uint32_t *)jump, K, M32, s.d_len);
    SX_TRY(ib_scan_chains(s));
    const uint64_t nchain = s.nchain;
    /* 4. the tables of all indexes: one device allocation (the CRC and Huffman tables first) and one on the host, laid out alike from
     * `off` on: off | first (a stream's len + 1 entries from crow[i] + i on) | size | type | nsmp | status | behind */
    const uint64_t nfirst = nchain + T, s_off = align_up(sizeof(SxTables)), s_first = s_off + sizeof(uint64_t) * (nchain + 1u), s_size = s_first + sizeof(uint64_t) * (nfirst + 1u),
            s_type = s_size + sizeof(uint32_t) * (nchain + 1u), s_nsmp = s_type + sizeof(uint32_t) * (nchain + 1u), s_status = s_nsmp + sizeof(uint32_t) * (nchain + 1u),
            s_behind = s_status + sizeof(int32_t) * (nchain + 1u), s_end = s_behind + sizeof(int32_t) * (uint64_t)T;
    SxSlab *slab = new (std::nothrow) SxSlab;
    if (!slab) { snprintf(ctx->err, sizeof(ctx->err), "out of host memory"); return LNN_NG; }
    slab->refs.store(1u); slab->device = ctx->device; slab->dev = NULL; slab->host = NULL;
    *slab_out = slab;
    slab->host = malloc(s_end - s_off);
    if (!slab->host) { snprintf(ctx->err, sizeof(ctx->err), "out of host memory"); return LNN_NG; }
    ctx->ibatch_count[4]++;
    HIPCHK(ctx, hipMalloc(&slab->dev, s_end));
    uint8_t *ds = (uint8_t *)slab->dev;
    auto hp = [&](uint64_t o) { return (uint8_t *)slab->host + (o - s_off); };          /* the host copy of the part at o */
    uint64_t *d_off = (uint64_t *)(ds + s_off), *d_first = (uint64_t *)(ds + s_first);
    uint32_t *d_size = (uint32_t *)(ds + s_size), *d_type = (uint32_t *)(ds + s_type), *d_nsmp = (uint32_t *)(ds + s_nsmp);
    int32_t *d_status = (int32_t *)(ds + s_status), *d_behind = (int32_t *)(ds + s_behind);
    sx_tables((SxTables *)(hl + o_tab));
    HIPCHK(ctx, hipMemcpyAsync(ds, hl + o_tab, sizeof(SxTables), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s.dl + s.at.o_crow, hl + s.at.o_crow, sizeof(uint64_t) * (T + 1ull), hipMemcpyHostToDevice, ctx->stream));
    if (nchain) {
        SX_LAUNCH(tl, LINNE_AMD_T_SX_CHAIN, k_ib_chain, dim3((uint32_t)((nchain + 255u) / 256u)), dim3(256), 0, ctx->stream, d_st, d_seg, d_crow, T, (const uint64_t *)cand,
                (const uint32_t *)jump, K, M32, nchain, d_off, d_size, d_type, d_nsmp);
    }
    uint64_t *scan = cand;                                         /* (the candidates are read: see 3.) */
    SX_LAUNCH(tl, LINNE_AMD_T_SX_SCAN, k_sx_scan, dim3(1), dim3(SX_SCAN_THREADS), 0, ctx->stream, (const uint32_t *)d_nsmp, nchain, scan);
    SX_LAUNCH(tl, LINNE_AMD_T_SX_SCAN, k_ib_first, dim3((uint32_t)((nfirst + 255u) / 256u)), dim3(256), 0, ctx->stream, (const uint64_t *)scan, d_crow, T, nfirst, d_first);
    if (nchain) {
        IbCheckArgs a;
        a.st = d_st; a.crow = d_crow; a.T = T; a.nchain = nchain; a.off = d_off; a.first = d_first; a.size = d_size; a.type = d_type; a.nsmp = d_nsmp;
        a.tab = (const SxTables *)ds; a.status = d_status;
        SX_LAUNCH(tl, LINNE_AMD_T_SX_CHECK, k_ib_check, dim3((uint32_t)((nchain + 3u) / 4u)), dim3(256), 0, ctx->stream, a);
    }
    SX_LAUNCH(tl, LINNE_AMD_T_IB_BEHIND, k_ib_behind, dim3(gT), dim3(256), 0, ctx->stream, d_st, d_crow, T, (const uint64_t *)d_off, (const uint32_t *)d_size, (const uint64_t *)d_first, d_behind);
    /* 5. everything comes back in one copy behind the call's last wait */
    HIPCHK(ctx, hipMemcpyAsync(slab->host, ds + s_off, s_end - s_off, hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->timing) { HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream)); ctx->ev_valid = 1; }
    SX_TRY(tally_wait(ctx, tl));
    const int32_t *h_status = (const int32_t *)(hp(s_status)), *h_behind = (const int32_t *)(hp(s_behind));
    for (uint32_t i = 0; i < T; i++) {
        LINNEAmdStreamIndex *x = indexes[i];
        if (!x) continue;
        const uint64_t c0 = h_crow[i], len = h_len[i], ns = x->header.num_samples, N = x->stream_bytes;
        x->slab = slab; slab->refs.fetch_add(1u);
        x->d_tab = (SxTables *)ds;
        x->d_off = d_off + c0; x->d_first = d_first + c0 + i; x->d_size = d_size + c0; x->d_type = d_type + c0; x->d_nsmp = d_nsmp + c0; x->d_status = d_status + c0;
        x->h_off = (uint64_t *)(hp(s_off)) + c0; x->h_first = (uint64_t *)(hp(s_first)) + c0 + i;
        x->h_size = (uint32_t *)(hp(s_size)) + c0; x->h_type = (uint32_t *)(hp(s_type)) + c0; x->h_nsmp = (uint32_t *)(hp(s_nsmp)) + c0;
        /* DecodeWhole's loop ends once the samples reach the header's count (lnn_api.c LINNEDecoder_DecodeWhole) */
        uint64_t nb = 0;
        while (nb < len && x->h_first[nb] < ns) nb++;
        x->nb = (uint32_t)nb; x->covered = x->h_first[nb];
        for (uint64_t r = 0; r < nb; r++) if (h_status[c0 + r] != LNN_OK) { x->fail_block = (int64_t)r; x->fail_code = h_status[c0 + r]; x->fail_off = x->h_off[r]; break; }
        if (x->fail_block < 0 && nb == len && x->covered < ns) {
            const uint64_t q = nb ? x->h_off[nb - 1] + x->h_size[nb - 1] + 6u : SX_FIRST_BLOCK;
            if (q < N) {
                if (h_behind[i] == LNN_NG || h_behind[i] == 0) {
                    snprintf(text, sizeof(text), "internal: a block head at byte %llu the index did not find", (unsigned long long)q);
                    fail_stream(i, LNN_NG, text);
                    LINNEAmd_StreamIndexDestroy(x); indexes[i] = NULL;
                    continue;
                }
                x->fail_block = (int64_t)nb; x->fail_code = h_behind[i]; x->fail_off = q;
            }
        }
        ctx->ibatch_count[1]++;
    }
    return LNN_OK;
}

/* Both entry points behind their own first checks: the streams' indexes and results, then the call's -- the lowest-numbered failing
 * stream's code, with its text in ctx->err (behind the stream's number unless the call is the single one) */
static int ib_call(LINNEAmdContext *ctx, const uint8_t *const *d_streams, const uint64_t *stream_bytes, uint32_t num_streams,
        struct LINNEAmdStreamIndex **indexes, int32_t *results, bool single)
{
    ctx->err[0] = 0;
    for (int i = 0; i < 5; i++) ctx->ibatch_count[i] = 0;
    if (num_streams == 0) return LNN_OK;
    if (!d_streams || !stream_bytes || !indexes || !results) { snprintf(ctx->err, sizeof(ctx->err), "StreamIndexesCreate: null argument"); return LNN_INVALID_ARGUMENT; }
    ctx->ibatch_count[0] = num_streams;
    for (uint32_t i = 0; i < num_streams; i++) { indexes[i] = NULL; results[i] = LNN_OK; }
    SxSlab *slab = NULL;
    int first_code = LNN_OK;
    int ret = ib_build(ctx, d_streams, stream_bytes, num_streams, single, indexes, results, &slab, &first_code);
    /* a HIP error, no memory: the whole call fails (ib_build has waited and recorded where it did not) */
    ret = items_end(ctx, NULL, ret, false, ret != LNN_OK, NULL, num_streams, [&](uint32_t i) { LINNEAmd_StreamIndexDestroy(indexes[i]); indexes[i] = NULL; results[i] = LNN_NG; });
    if (ret != LNN_OK) ctx->ibatch_count[1] = 0;
    if (slab) sx_slab_release(slab);                               /* the call's own reference */
    return ret != LNN_OK ? LNN_NG : first_code;
}

extern "C" int LINNEAmd_StreamIndexesCreate(struct LINNEAmdContext *ctx, const uint8_t *const *d_streams, const uint64_t *stream_bytes, uint32_t num_streams,
        struct LINNEAmdStreamIndex **indexes, int32_t *results)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    return ib_call(ctx, d_streams, stream_bytes, num_streams, indexes, results, false);
}

/* one stream: indexes[0] and results[0] of the call above */
extern "C" struct LINNEAmdStreamIndex *LINNEAmd_StreamIndexCreate(struct LINNEAmdContext *ctx, const uint8_t *d_stream,
        uint64_t stream_bytes, int *result)
{
    int dummy;
    if (!result) result = &dummy;
    if (!ctx || !d_stream) { *result = LNN_INVALID_ARGUMENT; return NULL; }
    ctx->err[0] = 0;
    if (hipSetDevice(ctx->device) != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "hipSetDevice(%d) failed", ctx->device); *result = LNN_NG; return NULL; }
    struct LINNEAmdStreamIndex *x = NULL;
    int32_t r = LNN_OK;
    (void)ib_call(ctx, &d_stream, &stream_bytes, 1, &x, &r, true);
    *result = r;
    return x;
}

/* ================================================================================================
 * sample windows of resident streams: many in one call, or one (lnn_k_windows.h; the plan: lnn_windows_plan.h)
 * ============================================================================================== */
struct WxCall;
/* what a consumer's launches read beside a pass's WxPlaceArgs: its per-window records, its accumulators (behind every pass's scratch,
 * acc_prefix units of its own in front of them) and its words behind the fail and saturation words */
struct WxLaunch {
    const WxBucket *side; const WxMix *mix; const WxWindow *wins; uint8_t *acc; uint32_t *back; const uint32_t *fail; uint32_t nwin; uint64_t nacc, nout, nmask;
    const WxResample *rs; const WxTile *tiles; const uint32_t *coef; uint64_t ntile; uint32_t *sat;        /* the resampling consumer's */
    const WxOvOutput *ov_outs; const WxOvSource *ov_srcs;          /* the overlaying consumer's, beside tiles, ntile and sat */
    const WxLagTile *lg_tiles; const uint32_t *lg_runs; const WxLagProbe *lg_probes; const WxLagImage *lg_imgs; uint64_t nlgrun, lg_part;     /* the lag consumer's, beside ntile */
    const WxProject *pj; const WxProjTile *pj_tiles; const WxProjTable *pj_tabs; const int32_t *pj_rsum; const int16_t *pj_raw; uint32_t pj_ntab; uint64_t pj_plane0, pj_cells;   /* the projecting consumer's, beside ntile and sat */
};
/* What a windows call does with its windows' samples: k_wx_place's place in a pass, and what goes with it.  The eleven calls are the
 * eleven constant instances below; a launch that a consumer does not have is NULL */
struct WxConsumer {
    const char *name;                   /* in the call's texts */
    uint32_t back_words;                /* 32-bit words per window behind the fail and saturation words, which come back with them */
    void (*back_preset)(uint32_t *back, uint32_t W);
    WxBucketing bucketing;              /* buckets: a WxBucket beside every window record, accumulators preset in front of the first pass and committed behind the last */
    uint64_t acc_unit, acc_prefix;      /* an accumulator's bytes; units in front of the accumulators */
    int (*check)(const WxCall &c, uint32_t i, char *err, size_t cap);      /* the window's own arguments, behind the range check */
    void (*describe)(const WxCall &c, uint32_t i, WxRange &r);             /* where its samples go: its WxWindow's fields, its bucket spec */
    int (*preset)(LINNEAmdContext *ctx, const WxLaunch &l);
    int (*pass)(LINNEAmdContext *ctx, const WxLaunch &l, const WxPlaceArgs &la);
    int (*commit)(LINNEAmdContext *ctx, const WxLaunch &l);
    /* an OK window's answer into the caller's arrays; words: all that came back (fail words first), NULL for a window that took no pass */
    void (*read_back)(const WxCall &c, uint32_t i, const uint32_t *words);
    bool mixes;                         /* a WxMix beside every window record, from the windows' struct LINNEAmdMixSpec (a consumer without buckets) */
    bool resamples;                     /* a WxResample beside every window record, from the windows' struct LINNEAmdResampleSpec: the passes place the
                                         * windows' input ranges into images among the accumulators, the commit filters them (a consumer without buckets) */
    bool overlays;                      /* the windows are the sources of the call's outputs (WxCall.ov_*): the passes place them into images among the
                                         * accumulators, the commit sums the outputs from them (a consumer without buckets) */
    bool lags;                          /* the windows are the needles and haystacks of the call's probes (WxCall.lag_*): the passes place them into images
                                         * among the accumulators, the commit slides them (a consumer without buckets) */
    bool projects;                      /* a WxProject beside every window record, from the windows' struct LINNEAmdProjectSpec: the passes place the
                                         * windows' input ranges into images among the accumulators, the commit projects their frames (a consumer without buckets) */
};
struct WxCall {
    const WxConsumer *use;
    bool single;                        /* the call is LINNEAmd_DecodeStreamDevice, which its texts then name */
    struct LINNEAmdWindow *win; uint32_t W, group_frames;
    const void *specs;                  /* [W] of the consumer's: place, compare and mix struct LINNEAmdPcmLayout (NULL: int32 planar, pcm_stride), measure, digest, quiet, histogram and relate their specs */
    void *answers;                      /* [W] of the consumer's: place and mix the layouts again (`saturated`; NULL: not reported), compare struct LINNEAmdDiff, quiet struct LINNEAmdQuiet */
    const struct LINNEAmdMixSpec *mix;  /* [W], mix alone: its specs go beside its layouts */
    const struct LINNEAmdResampleSpec *rs;      /* [W], resample alone, likewise */
    const struct LINNEAmdOverlaySource *const *ov_src; const WxOvOut *ov_outs; uint32_t ov_O;      /* overlay alone: window i's source [W]; the outputs [ov_O] */
    const WxLagIn *lag_in; uint32_t lag_Q;      /* lags alone: the probes [lag_Q] */
    struct LINNEAmdProjectSpec *pj;     /* [W], project alone: in (the spec) and out (`saturated`) */
};
static WxCall wx_call(const WxConsumer *use, struct LINNEAmdWindow *win, uint32_t W, uint32_t group_frames, const void *specs, void *answers)
{
    WxCall c;
    c.use = use; c.single = false; c.win = win; c.W = W; c.group_frames = group_frames; c.specs = specs; c.answers = answers; c.mix = NULL; c.rs = NULL;
    c.ov_src = NULL; c.ov_outs = NULL; c.ov_O = 0; c.lag_in = NULL; c.lag_Q = 0; c.pj = NULL;
    return c;
}
/* a lane per unit, in a grid-stride kernel */
/* the most workgroups of SX_PLACE_THREADS (256) threads a launch takes: fewer than 2^32 threads in all */
#define WX_LAUNCH_GROUPS 0xFFFFFFu
static dim3 wx_grid(uint64_t n) { const uint64_t g = (n + WXB_THREADS - 1u) / WXB_THREADS; return dim3((uint32_t)(g < 65536u ? g : 65536u)); }

/* ---- place, and compare, which reads the PCM that place writes (LINNE_AMD_PCM_F32 is refused as on encode) ---- */
static int wx_pcm_check(const WxCall &c, uint32_t i, uint32_t C, bool writes, char *err, size_t cap)
{
    const struct LINNEAmdWindow *w = &c.win[i];
    if (c.specs) {
        const struct LINNEAmdPcmLayout *ly = (const struct LINNEAmdPcmLayout *)c.specs + i;
        const int why = sb_layout_check(ly->format, ly->channel_stride, ly->sample_stride, (uint64_t)(uintptr_t)w->d_pcm, C, w->num_samples, writes);
        if (why != SB_LY_OK) { snprintf(err, cap, "DecodeStreamDevice: %s", sb_layout_text(why)); return LNN_INVALID_ARGUMENT; }
    } else if (C > 1u && w->pcm_stride < w->num_samples) { snprintf(err, cap, "DecodeStreamDevice: pcm_stride %llu < %llu samples", (unsigned long long)w->pcm_stride, (unsigned long long)w->num_samples); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}
static int wx_place_check(const WxCall &c, uint32_t i, char *err, size_t cap) { return wx_pcm_check(c, i, c.win[i].index->shape.num_channels, true, err, cap); }
static int wx_compare_check(const WxCall &c, uint32_t i, char *err, size_t cap) { return wx_pcm_check(c, i, c.win[i].index->shape.num_channels, false, err, cap); }
static void wx_pcm_describe(const WxCall &c, uint32_t i, WxRange &r)
{
    const struct LINNEAmdPcmLayout *ly = (const struct LINNEAmdPcmLayout *)c.specs;
    r.out = c.win[i].d_pcm;
    if (ly) { r.fmt = ly[i].format; r.stride = ly[i].channel_stride; r.sstride = ly[i].sample_stride; }
    else { r.fmt = LINNE_AMD_PCM_S32; r.stride = c.win[i].pcm_stride; r.sstride = 1u; }
}
static int wx_place_pass(LINNEAmdContext *ctx, const WxLaunch &, const WxPlaceArgs &la) { SX_LAUNCH(NULL, LINNE_AMD_T_WX_PLACE, k_wx_place, dim3(la.nrec * la.xch), dim3(SX_PLACE_THREADS), 0, ctx->stream, la); return LNN_OK; }
/* (a failing window's `saturated` stays as the caller left it; the saturation words lie behind the fail words) */
static void wx_place_read_back(const WxCall &c, uint32_t i, const uint32_t *words) { if (c.answers) ((struct LINNEAmdPcmLayout *)c.answers)[i].saturated = (words && words[c.W + i]) ? 1u : 0u; }
/* compare: two 64-bit words per window, its count of differing elements (0) and their least key (~0) */
static void wx_compare_back_preset(uint32_t *back, uint32_t W) { uint64_t *d = (uint64_t *)back; for (uint32_t i = 0; i < W; i++) { d[2u * i] = 0u; d[2u * i + 1u] = ~(uint64_t)0; } }
static int wx_compare_pass(LINNEAmdContext *ctx, const WxLaunch &l, const WxPlaceArgs &la)
{
    WxCompareArgs ca; ca.p = la; ca.diff = (unsigned long long *)l.back;
    SX_LAUNCH(NULL, LINNE_AMD_COMPARE_T_COMPARE, k_wx_compare, dim3(la.nrec * la.xch), dim3(SX_PLACE_THREADS), 0, ctx->stream, ca);
    return LNN_OK;
}
/* (a failing window's diffs[i] stays too; an OK window of no samples took no pass and differs nowhere) */
static void wx_compare_read_back(const WxCall &c, uint32_t i, const uint32_t *words)
{
    const uint64_t *dw = words ? (const uint64_t *)(words + 2u * (uint64_t)c.W) + 2u * (uint64_t)i : NULL;
    const uint64_t cnt = dw ? dw[0] : 0u;
    struct LINNEAmdDiff &d = ((struct LINNEAmdDiff *)c.answers)[i];
    d.num_differing = cnt; d.first_sample = cnt ? c.win[i].first_sample + (dw[1] >> 3) : 0u; d.first_channel = cnt ? (uint32_t)(dw[1] & 7u) : 0u; d.reserved = 0u;
}

/* ---- measure and digest: the window's d_pcm and pcm_stride are not looked at; its spec names buckets and a table ---- */
static int wx_bucket_check(const char *who, uint64_t n, uint64_t b, const void *d_out, char *err, size_t cap)
{
    const uint64_t nb = wx_buckets(n, b);
    if (!d_out && nb) { snprintf(err, cap, "%s: null d_out", who); return LNN_INVALID_ARGUMENT; }
    if ((uint64_t)(uintptr_t)d_out & 7u) { snprintf(err, cap, "%s: d_out is not 8-byte aligned", who); return LNN_INVALID_ARGUMENT; }
    if (nb > 0xFFFFFFFFull) { snprintf(err, cap, "%s: %llu buckets in one window: too many", who, (unsigned long long)nb); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}
static int wx_measure_check(const WxCall &c, uint32_t i, char *err, size_t cap)
{
    const struct LINNEAmdMeasureSpec &ms = ((const struct LINNEAmdMeasureSpec *)c.specs)[i];
    const uint64_t nb = wx_buckets(c.win[i].num_samples, ms.bucket_samples);
    SX_TRY(wx_bucket_check(c.use->name, c.win[i].num_samples, ms.bucket_samples, ms.d_out, err, cap));
    if (ms.channel_stride < nb) { snprintf(err, cap, "%s: channel_stride %llu < %llu buckets", c.use->name, (unsigned long long)ms.channel_stride, (unsigned long long)nb); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}
static int wx_digest_check(const WxCall &c, uint32_t i, char *err, size_t cap)
{
    const struct LINNEAmdDigestSpec &ds = ((const struct LINNEAmdDigestSpec *)c.specs)[i];
    return wx_bucket_check(c.use->name, c.win[i].num_samples, ds.bucket_samples, ds.d_out, err, cap);
}
static void wx_measure_describe(const WxCall &c, uint32_t i, WxRange &r)
{
    const struct LINNEAmdMeasureSpec &ms = ((const struct LINNEAmdMeasureSpec *)c.specs)[i];
    r.bucket_samples = ms.bucket_samples; r.bucket_out = ms.d_out; r.bucket_cstride = ms.channel_stride;
}
static void wx_digest_describe(const WxCall &c, uint32_t i, WxRange &r)
{
    const struct LINNEAmdDigestSpec &ds = ((const struct LINNEAmdDigestSpec *)c.specs)[i];
    r.bucket_samples = ds.bucket_samples; r.bucket_out = ds.d_out;
}
static int wx_measure_preset(LINNEAmdContext *ctx, const WxLaunch &l) { SX_LAUNCH(NULL, LINNE_AMD_MEASURE_T_PRESET, k_wx_measure_preset, wx_grid(l.nacc), dim3(WXB_THREADS), 0, ctx->stream, (struct LINNEAmdMeasure *)l.acc, l.nacc); return LNN_OK; }
static int wx_measure_pass(LINNEAmdContext *ctx, const WxLaunch &l, const WxPlaceArgs &la)
{
    WxMeasureArgs ma; ma.p = la; ma.mwin = l.side; ma.acc = (struct LINNEAmdMeasure *)l.acc;
    SX_LAUNCH(NULL, LINNE_AMD_MEASURE_T_MEASURE, k_wx_measure, dim3(la.nrec * la.xch), dim3(SX_PLACE_THREADS), 0, ctx->stream, ma);
    return LNN_OK;
}
static int wx_measure_commit(LINNEAmdContext *ctx, const WxLaunch &l) { SX_LAUNCH(NULL, LINNE_AMD_MEASURE_T_COMMIT, k_wx_measure_commit, wx_grid(l.nout), dim3(WXB_THREADS), 0, ctx->stream, l.side, l.nwin, (const struct LINNEAmdMeasure *)l.acc, l.fail, l.nout); return LNN_OK; }
/* digest: the tables of powers (WXD_POW_WORDS words), then the 32-bit accumulators */
static int wx_digest_preset(LINNEAmdContext *ctx, const WxLaunch &l)
{
    uint32_t *pow = (uint32_t *)l.acc;
    SX_LAUNCH(NULL, LINNE_AMD_DIGEST_T_PRESET, k_wx_digest_preset, wx_grid(l.nacc + WXD_POW_WORDS), dim3(WXB_THREADS), 0, ctx->stream, pow, pow + WXD_POW_WORDS, l.nacc);
    return LNN_OK;
}
static int wx_digest_pass(LINNEAmdContext *ctx, const WxLaunch &l, const WxPlaceArgs &la)
{
    WxDigestArgs da; da.p = la; da.dwin = l.side; da.pow = (const uint32_t *)l.acc; da.acc = (uint32_t *)l.acc + WXD_POW_WORDS;
    SX_LAUNCH(NULL, LINNE_AMD_DIGEST_T_DIGEST, k_wx_digest, dim3(la.nrec * la.xch), dim3(SX_PLACE_THREADS), 0, ctx->stream, da);
    return LNN_OK;
}
static int wx_digest_commit(LINNEAmdContext *ctx, const WxLaunch &l)
{
    const uint32_t *pow = (const uint32_t *)l.acc;
    SX_LAUNCH(NULL, LINNE_AMD_DIGEST_T_COMMIT, k_wx_digest_commit, wx_grid(l.nout), dim3(WXB_THREADS), 0, ctx->stream, l.side, l.nwin, pow + WXD_POW_WORDS, pow, l.fail, l.nout);
    return LNN_OK;
}


/* ---- quiet: a bit per frame in the scratch, runs extracted behind the last pass (lnn_k_quiet.h); four 64-bit words per window come
 * back: the loud extent (~0, 0), the runs found and the sum of their lengths ---- */
static int wx_quiet_check(const WxCall &c, uint32_t i, char *err, size_t cap)
{
    const struct LINNEAmdQuietSpec &qs = ((const struct LINNEAmdQuietSpec *)c.specs)[i];
    if (!qs.d_out && qs.capacity) { snprintf(err, cap, "%s: null d_out with capacity %llu", c.use->name, (unsigned long long)qs.capacity); return LNN_INVALID_ARGUMENT; }
    if ((uint64_t)(uintptr_t)qs.d_out & 7u) { snprintf(err, cap, "%s: d_out is not 8-byte aligned", c.use->name); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}
static void wx_quiet_describe(const WxCall &c, uint32_t i, WxRange &r)
{
    const struct LINNEAmdQuietSpec &qs = ((const struct LINNEAmdQuietSpec *)c.specs)[i];
    r.bucket_out = qs.d_out; r.quiet_min = qs.min_samples ? qs.min_samples : 1u; r.quiet_capacity = qs.capacity; r.quiet_threshold = qs.threshold;
}
static void wx_quiet_back_preset(uint32_t *back, uint32_t W)
{
    uint64_t *d = (uint64_t *)back;
    for (uint32_t i = 0; i < W; i++) { d[4u * i + WXQ_LOUD_LO] = ~(uint64_t)0; d[4u * i + WXQ_LOUD_HI] = 0u; d[4u * i + WXQ_RUNS] = 0u; d[4u * i + WXQ_QUIET] = 0u; }
}
static int wx_quiet_preset(LINNEAmdContext *ctx, const WxLaunch &l) { SX_LAUNCH(NULL, LINNE_AMD_QUIET_T_PRESET, k_wx_quiet_preset, wx_grid(l.nmask), dim3(WXB_THREADS), 0, ctx->stream, (unsigned long long *)l.acc, l.nmask); return LNN_OK; }
static int wx_quiet_pass(LINNEAmdContext *ctx, const WxLaunch &l, const WxPlaceArgs &la)
{
    WxQuietArgs qa; qa.p = la; qa.qwin = l.side; qa.mask = (unsigned long long *)l.acc;
    SX_LAUNCH(NULL, LINNE_AMD_QUIET_T_QUIET, k_wx_quiet, dim3(la.nrec * la.xch), dim3(SX_PLACE_THREADS), 0, ctx->stream, qa);
    return LNN_OK;
}
/* behind the masks (lnn_windows_plan.h wxq_chunk_units): the prefix sums, then the counts */
static int wx_quiet_commit(LINNEAmdContext *ctx, const WxLaunch &l)
{
    WxQuietCommitArgs a;
    uint64_t *ofs = (uint64_t *)l.acc + l.nmask;
    a.qwin = l.side; a.wins = l.wins; a.nwin = l.nwin; a.mask = (const unsigned long long *)l.acc; a.fail = l.fail; a.nchunks = l.nout;
    a.counts = (uint32_t *)(ofs + 2u * l.nout + 1u); a.ofs = ofs; a.back = (unsigned long long *)l.back;
    const dim3 grid((uint32_t)(l.nout < WX_MAX_TILES ? l.nout : WX_MAX_TILES));      /* (the kernels walk the chunks in steps of the grid) */
    SX_LAUNCH(NULL, LINNE_AMD_QUIET_T_COUNT, k_wx_quiet_runs<WXQ_COUNT>, grid, dim3(WXB_THREADS), 0, ctx->stream, a);
    SX_LAUNCH(NULL, LINNE_AMD_QUIET_T_SCAN, k_sx_scan, dim3(1), dim3(SX_SCAN_THREADS), 0, ctx->stream, (const uint32_t *)a.counts, 2u * l.nout, ofs);
    SX_LAUNCH(NULL, LINNE_AMD_QUIET_T_STARTS, k_wx_quiet_runs<WXQ_STARTS>, grid, dim3(WXB_THREADS), 0, ctx->stream, a);
    SX_LAUNCH(NULL, LINNE_AMD_QUIET_T_ENDS, k_wx_quiet_runs<WXQ_ENDS>, grid, dim3(WXB_THREADS), 0, ctx->stream, a);
    return LNN_OK;
}
/* (a failing window's answers[i] stays as the caller left it; an OK window of no samples took no pass: all four are 0) */
static void wx_quiet_read_back(const WxCall &c, uint32_t i, const uint32_t *words)
{
    struct LINNEAmdQuiet &q = ((struct LINNEAmdQuiet *)c.answers)[i];
    if (!words) { q.num_runs = q.quiet_samples = q.lead_samples = q.trail_samples = 0u; return; }
    const uint64_t *d = (const uint64_t *)(words + 2u * (uint64_t)c.W) + 4u * (uint64_t)i, n = c.win[i].num_samples;
    const bool none_loud = d[WXQ_LOUD_HI] == 0u;
    q.num_runs = d[WXQ_RUNS]; q.quiet_samples = d[WXQ_QUIET];
    q.lead_samples = none_loud ? n : d[WXQ_LOUD_LO]; q.trail_samples = none_loud ? n : n - d[WXQ_LOUD_HI];
}

/* ---- histogram: measure's buckets with num_bins 32-bit counters where that has a record (lnn_k_histogram.h) ---- */
static int wx_histogram_check(const WxCall &c, uint32_t i, char *err, size_t cap)
{
    const struct LINNEAmdHistogramSpec &hs = ((const struct LINNEAmdHistogramSpec *)c.specs)[i];
    const uint64_t nb = wx_buckets(c.win[i].num_samples, hs.bucket_samples);
    if (hs.num_bins == 0u || hs.num_bins > LINNE_AMD_HIST_MAX_BINS) { snprintf(err, cap, "%s: num_bins %u is not in 1 .. %d", c.use->name, hs.num_bins, LINNE_AMD_HIST_MAX_BINS); return LNN_INVALID_ARGUMENT; }
    if (hs.shift > 31u) { snprintf(err, cap, "%s: shift %u > 31", c.use->name, hs.shift); return LNN_INVALID_ARGUMENT; }
    if (hs.scale != LINNE_AMD_HIST_LINEAR && hs.scale != LINNE_AMD_HIST_LOG2) { snprintf(err, cap, "%s: unknown scale %u", c.use->name, hs.scale); return LNN_INVALID_ARGUMENT; }
    if (hs.reserved != 0u) { snprintf(err, cap, "%s: reserved is not 0", c.use->name); return LNN_INVALID_ARGUMENT; }
    SX_TRY(wx_bucket_check(c.use->name, c.win[i].num_samples, hs.bucket_samples, hs.d_out, err, cap));
    if (hs.channel_stride < nb) { snprintf(err, cap, "%s: channel_stride %llu < %llu buckets", c.use->name, (unsigned long long)hs.channel_stride, (unsigned long long)nb); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}
static void wx_histogram_describe(const WxCall &c, uint32_t i, WxRange &r)
{
    const struct LINNEAmdHistogramSpec &hs = ((const struct LINNEAmdHistogramSpec *)c.specs)[i];
    r.bucket_samples = hs.bucket_samples; r.bucket_out = hs.d_out; r.bucket_cstride = hs.channel_stride; r.hist = WXH_SPEC(hs.num_bins, hs.shift, hs.scale);
}
static int wx_histogram_preset(LINNEAmdContext *ctx, const WxLaunch &l) { SX_LAUNCH(NULL, LINNE_AMD_HISTOGRAM_T_PRESET, k_wx_histogram_preset, wx_grid(l.nacc), dim3(WXB_THREADS), 0, ctx->stream, (uint32_t *)l.acc, l.nacc); return LNN_OK; }
static int wx_histogram_pass(LINNEAmdContext *ctx, const WxLaunch &l, const WxPlaceArgs &la)
{
    WxHistogramArgs ha; ha.p = la; ha.hwin = l.side; ha.acc = (uint32_t *)l.acc;
    SX_LAUNCH(NULL, LINNE_AMD_HISTOGRAM_T_HISTOGRAM, k_wx_histogram, dim3(la.nrec * la.xch), dim3(SX_PLACE_THREADS), 0, ctx->stream, ha);
    return LNN_OK;
}
static int wx_histogram_commit(LINNEAmdContext *ctx, const WxLaunch &l) { SX_LAUNCH(NULL, LINNE_AMD_HISTOGRAM_T_COMMIT, k_wx_histogram_commit, wx_grid(l.nout), dim3(WXB_THREADS), 0, ctx->stream, l.side, l.nwin, (const uint32_t *)l.acc, l.fail, l.nout); return LNN_OK; }

/* ---- relate: measure's buckets with a record per channel pair where that has one per channel (lnn_k_relate.h) ---- */
static int wx_relate_check(const WxCall &c, uint32_t i, char *err, size_t cap)
{
    const struct LINNEAmdRelateSpec &rs = ((const struct LINNEAmdRelateSpec *)c.specs)[i];
    const uint64_t nb = wx_buckets(c.win[i].num_samples, rs.bucket_samples);
    SX_TRY(wx_bucket_check(c.use->name, c.win[i].num_samples, rs.bucket_samples, rs.d_out, err, cap));
    if (rs.pair_stride < nb) { snprintf(err, cap, "%s: pair_stride %llu < %llu buckets", c.use->name, (unsigned long long)rs.pair_stride, (unsigned long long)nb); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}
static void wx_relate_describe(const WxCall &c, uint32_t i, WxRange &r)
{
    const struct LINNEAmdRelateSpec &rs = ((const struct LINNEAmdRelateSpec *)c.specs)[i];
    r.bucket_samples = rs.bucket_samples; r.bucket_out = rs.d_out; r.bucket_cstride = rs.pair_stride;
}
static int wx_relate_preset(LINNEAmdContext *ctx, const WxLaunch &l) { SX_LAUNCH(NULL, LINNE_AMD_RELATE_T_PRESET, k_wx_relate_preset, wx_grid(l.nacc), dim3(WXB_THREADS), 0, ctx->stream, (struct LINNEAmdRelation *)l.acc, l.nacc); return LNN_OK; }
static int wx_relate_pass(LINNEAmdContext *ctx, const WxLaunch &l, const WxPlaceArgs &la)
{
    WxRelateArgs ra; ra.p = la; ra.rwin = l.side; ra.acc = (struct LINNEAmdRelation *)l.acc;
    SX_LAUNCH(NULL, LINNE_AMD_RELATE_T_RELATE, k_wx_relate, dim3(la.nrec * la.xch), dim3(SX_PLACE_THREADS), 0, ctx->stream, ra);
    return LNN_OK;
}
static int wx_relate_commit(LINNEAmdContext *ctx, const WxLaunch &l) { SX_LAUNCH(NULL, LINNE_AMD_RELATE_T_COMMIT, k_wx_relate_commit, wx_grid(l.nout), dim3(WXB_THREADS), 0, ctx->stream, l.side, l.nwin, (const struct LINNEAmdRelation *)l.acc, l.fail, l.nout); return LNN_OK; }

/* ---- mix: place with the window's channel matrix between the samples and the PCM (lnn_k_mix.h); the PCM has the matrix' Co channels ---- */
static int wx_mix_check(const WxCall &c, uint32_t i, char *err, size_t cap)
{
    const struct LINNEAmdMixSpec &ms = c.mix[i];
    if (ms.out_channels < 1u || ms.out_channels > LINNE_MAX_NUM_CHANNELS) { snprintf(err, cap, "%s: out_channels %u is not 1 .. %u", c.use->name, ms.out_channels, (unsigned)LINNE_MAX_NUM_CHANNELS); return LNN_INVALID_ARGUMENT; }
    if (ms.shift > 31u) { snprintf(err, cap, "%s: shift %u > 31", c.use->name, ms.shift); return LNN_INVALID_ARGUMENT; }
    if (ms.clip_bits == 1u || ms.clip_bits > 32u) { snprintf(err, cap, "%s: clip_bits %u is neither 0 nor 2 .. 32", c.use->name, ms.clip_bits); return LNN_INVALID_ARGUMENT; }
    if (ms.reserved != 0u) { snprintf(err, cap, "%s: reserved is not 0", c.use->name); return LNN_INVALID_ARGUMENT; }
    return wx_pcm_check(c, i, ms.out_channels, true, err, cap);
}
static void wx_mix_describe(const WxCall &c, uint32_t i, WxRange &r) { wx_pcm_describe(c, i, r); r.mix = c.mix + i; }
static int wx_mix_pass(LINNEAmdContext *ctx, const WxLaunch &l, const WxPlaceArgs &la)
{
    WxMixArgs ma; ma.p = la; ma.mwin = l.mix;
    SX_LAUNCH(NULL, LINNE_AMD_MIX_T_MIX, k_wx_mix, dim3(la.nrec * la.xch), dim3(SX_PLACE_THREADS), 0, ctx->stream, ma);
    return LNN_OK;
}

/* ---- resample: the passes place the windows' input ranges into images; the commit filters the outputs from them (lnn_k_resample.h) ---- */
/* the spec's own bounds, which the range check needs in front of it */
static int wx_resample_spec_check(const WxCall &c, uint32_t i, char *err, size_t cap)
{
    const struct LINNEAmdResampleSpec &s = c.rs[i];
    const char *who = c.use->name;
    if (s.up < 1u || s.up > LINNE_AMD_RESAMPLE_MAX_RATIO || s.down < 1u || s.down > LINNE_AMD_RESAMPLE_MAX_RATIO) { snprintf(err, cap, "%s: up %u / down %u is not 1 .. %u", who, s.up, s.down, (unsigned)LINNE_AMD_RESAMPLE_MAX_RATIO); return LNN_INVALID_ARGUMENT; }
    if (s.taps < 1u || s.taps > LINNE_AMD_RESAMPLE_MAX_TAPS) { snprintf(err, cap, "%s: taps %u is not 1 .. %u", who, s.taps, (unsigned)LINNE_AMD_RESAMPLE_MAX_TAPS); return LNN_INVALID_ARGUMENT; }
    if ((uint64_t)s.up * s.taps > LINNE_AMD_RESAMPLE_MAX_COEFS) { snprintf(err, cap, "%s: up %u * taps %u > %u coefficients", who, s.up, s.taps, (unsigned)LINNE_AMD_RESAMPLE_MAX_COEFS); return LNN_INVALID_ARGUMENT; }
    if (s.before > s.taps - 1u) { snprintf(err, cap, "%s: before %u > taps - 1", who, s.before); return LNN_INVALID_ARGUMENT; }
    if (s.shift > 31u) { snprintf(err, cap, "%s: shift %u > 31", who, s.shift); return LNN_INVALID_ARGUMENT; }
    if (s.clip_bits == 1u || s.clip_bits > 32u) { snprintf(err, cap, "%s: clip_bits %u is neither 0 nor 2 .. 32", who, s.clip_bits); return LNN_INVALID_ARGUMENT; }
    if (s.reserved != 0u) { snprintf(err, cap, "%s: reserved is not 0", who); return LNN_INVALID_ARGUMENT; }
    if (!s.coef) { snprintf(err, cap, "%s: null coef", who); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}
static int wx_resample_check(const WxCall &c, uint32_t i, char *err, size_t cap) { return wx_pcm_check(c, i, c.win[i].index->shape.num_channels, true, err, cap); }
/* (behind wx_decode's own: the planned range becomes the window's input range) */
static void wx_resample_describe(const WxCall &c, uint32_t i, WxRange &r)
{
    wx_pcm_describe(c, i, r);
    r.rs = c.rs + i; r.m_lo = r.lo; r.m_n = r.n;
    const WxrInput in = wxr_input(r.m_lo, r.m_n, c.rs[i], c.win[i].index->header.num_samples);
    r.lo = in.lo; r.n = in.hi - in.lo;
}
static int wx_resample_preset(LINNEAmdContext *ctx, const WxLaunch &l) { SX_LAUNCH(NULL, LINNE_AMD_RESAMPLE_T_PRESET, k_wx_resample_preset, wx_grid(l.nacc / 4u), dim3(WXB_THREADS), 0, ctx->stream, (uint4 *)l.acc, l.nacc / 4u); return LNN_OK; }
static int wx_resample_commit(LINNEAmdContext *ctx, const WxLaunch &l)
{
    WxResampleArgs ra;
    ra.tiles = l.tiles; ra.ntiles = (uint32_t)l.ntile; ra.rwin = l.rs; ra.fail = l.fail; ra.sat = l.sat; ra.acc = (const int32_t *)l.acc; ra.coef = l.coef;
    SX_LAUNCH(NULL, LINNE_AMD_RESAMPLE_T_RESAMPLE, k_wx_resample, dim3(ra.ntiles), dim3(WXR_TILE), 0, ctx->stream, ra);
    return LNN_OK;
}

/* ---- overlay: the passes place the sources' ranges into images; the commit sums the outputs from them (lnn_k_overlay.h) ---- */
static int wx_overlay_check(const WxCall &, uint32_t, char *, size_t) { return LNN_OK; }   /* (the outputs' checks came in front of the windows') */
static void wx_overlay_describe(const WxCall &c, uint32_t i, WxRange &r) { r.ov = c.ov_src[i]; }
static int wx_overlay_commit(LINNEAmdContext *ctx, const WxLaunch &l)
{
    WxOverlayArgs oa;
    oa.tiles = l.tiles; oa.ntiles = (uint32_t)l.ntile; oa.outs = l.ov_outs; oa.srcs = l.ov_srcs; oa.fail = l.fail; oa.sat = l.sat; oa.acc = (const int32_t *)l.acc;
    /* (a call whose live sources all belong to outputs with a failing source has no tile: its one workgroup returns at once) */
    SX_LAUNCH(NULL, LINNE_AMD_OVERLAY_T_OVERLAY, k_wx_overlay, dim3(oa.ntiles ? oa.ntiles : 1u), dim3(WXR_TILE), 0, ctx->stream, oa);
    return LNN_OK;
}

/* ---- lags: the passes place the needles' and the haystacks' ranges into images; two launches slide them (lnn_k_lags.h) ---- */
static int wx_lags_check(const WxCall &, uint32_t, char *, size_t) { return LNN_OK; }      /* (the probes' checks came in front of the windows') */
static void wx_lags_describe(const WxCall &, uint32_t, WxRange &) {}
static int wx_lags_commit(LINNEAmdContext *ctx, const WxLaunch &l)
{
    WxLagsArgs ga;
    ga.tiles = l.lg_tiles; ga.ntiles = (uint32_t)l.ntile; ga.runs = l.lg_runs; ga.nruns = (uint32_t)l.nlgrun; ga.probes = l.lg_probes; ga.imgs = l.lg_imgs;
    ga.fail = l.fail; ga.acc = (const int32_t *)l.acc; ga.part = (uint64_t *)((int32_t *)l.acc + l.lg_part);
    /* (a call whose live windows all belong to probes with a window the host refused has no tile: the one workgroup returns at once) */
    SX_LAUNCH(NULL, LINNE_AMD_LAGS_T_LAGS, k_wx_lags, dim3(ga.ntiles ? ga.ntiles : 1u), dim3(WXL_LAGS), 0, ctx->stream, ga);
    SX_LAUNCH(NULL, LINNE_AMD_LAGS_T_COMMIT, k_wx_lags_commit, dim3(ga.nruns ? ga.nruns : 1u), dim3(WXL_LAGS), 0, ctx->stream, ga);
    return LNN_OK;
}

/* ---- project: the passes place the windows' input ranges into images; the commit projects their frames on the basis rows (lnn_k_project.h) ---- */
/* the spec's own bounds, which the range check needs in front of it */
static int wx_project_spec_check(const WxCall &c, uint32_t i, char *err, size_t cap)
{
    const struct LINNEAmdProjectSpec &s = c.pj[i];
    const char *who = c.use->name;
    if (s.frame_len < 1u || s.frame_len > LINNE_AMD_PROJECT_MAX_FRAME) { snprintf(err, cap, "%s: frame_len %u is not 1 .. %u", who, s.frame_len, (unsigned)LINNE_AMD_PROJECT_MAX_FRAME); return LNN_INVALID_ARGUMENT; }
    if (s.hop < 1u || s.hop > LINNE_AMD_PROJECT_MAX_HOP) { snprintf(err, cap, "%s: hop %u is not 1 .. %u", who, s.hop, (unsigned)LINNE_AMD_PROJECT_MAX_HOP); return LNN_INVALID_ARGUMENT; }
    if (s.num_rows < 1u || s.num_rows > LINNE_AMD_PROJECT_MAX_ROWS) { snprintf(err, cap, "%s: num_rows %u is not 1 .. %u", who, s.num_rows, (unsigned)LINNE_AMD_PROJECT_MAX_ROWS); return LNN_INVALID_ARGUMENT; }
    if (s.before > s.frame_len - 1u) { snprintf(err, cap, "%s: before %u > frame_len - 1", who, s.before); return LNN_INVALID_ARGUMENT; }
    if (s.shift > 31u) { snprintf(err, cap, "%s: shift %u > 31", who, s.shift); return LNN_INVALID_ARGUMENT; }
    if (s.clip_bits == 1u || s.clip_bits > 32u) { snprintf(err, cap, "%s: clip_bits %u is neither 0 nor 2 .. 32", who, s.clip_bits); return LNN_INVALID_ARGUMENT; }
    if (s.format != LINNE_AMD_PCM_S32 && s.format != LINNE_AMD_PCM_F32) { snprintf(err, cap, "%s: format %u is neither S32 nor F32", who, s.format); return LNN_INVALID_ARGUMENT; }
    if (s.float_exp > 63u || (s.float_exp != 0u && s.format == LINNE_AMD_PCM_S32)) { snprintf(err, cap, "%s: float_exp %u is not 0 .. 63, or not 0 with S32", who, s.float_exp); return LNN_INVALID_ARGUMENT; }
    if (s.reserved != 0u) { snprintf(err, cap, "%s: reserved is not 0", who); return LNN_INVALID_ARGUMENT; }
    if (!s.basis) { snprintf(err, cap, "%s: null basis", who); return LNN_INVALID_ARGUMENT; }
    if (!c.win[i].d_pcm) { snprintf(err, cap, "%s: null d_pcm", who); return LNN_INVALID_ARGUMENT; }
    if ((uint64_t)(uintptr_t)c.win[i].d_pcm & 3u) { snprintf(err, cap, "%s: d_pcm is not 4-byte aligned", who); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}
/* what needs the stream's channel count, still in front of the range check: the products' cap and the injective output map */
static int wx_project_shape_check(const WxCall &c, uint32_t i, uint32_t C, char *err, size_t cap)
{
    const struct LINNEAmdProjectSpec &s = c.pj[i];
    const char *who = c.use->name;
    const uint64_t n = c.win[i].num_samples;
    if (!wxp_products_fit(n, s.num_rows, s.frame_len, C)) { snprintf(err, cap, "%s: %llu frames * %u rows * %u samples * %u channels > 2^40 products", who, (unsigned long long)n, s.num_rows, s.frame_len, C); return LNN_INVALID_ARGUMENT; }
    if (!wxp_injective(s.channel_stride, C, s.frame_stride, n, s.row_stride, s.num_rows)) { snprintf(err, cap, "%s: channel_stride %llu, frame_stride %llu and row_stride %llu do not keep %u channels, %llu frames and %u rows apart", who, (unsigned long long)s.channel_stride, (unsigned long long)s.frame_stride, (unsigned long long)s.row_stride, C, (unsigned long long)n, s.num_rows); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}
static int wx_project_check(const WxCall &, uint32_t, char *, size_t) { return LNN_OK; }   /* (the window's own checks came in front of the range check) */
/* (behind wx_decode's own: the planned range becomes the window's input range) */
static void wx_project_describe(const WxCall &c, uint32_t i, WxRange &r)
{
    r.out = c.win[i].d_pcm; r.fmt = c.pj[i].format; r.stride = c.pj[i].channel_stride; r.sstride = c.pj[i].frame_stride;
    r.pj = c.pj + i; r.m_lo = r.lo; r.m_n = r.n;
    const WxpInput in = wxp_input(r.m_lo, r.m_n, c.pj[i], c.win[i].index->header.num_samples);
    r.lo = in.lo; r.n = in.hi - in.lo;
}
static int wx_project_preset(LINNEAmdContext *ctx, const WxLaunch &l)
{
    WxProjectPresetArgs pa;
    pa.acc = (uint4 *)l.acc; pa.n16 = l.pj_plane0 / 4u; pa.tabs = l.pj_tabs; pa.ntab = l.pj_ntab; pa.raw = l.pj_raw; pa.planes = (int8_t *)((int32_t *)l.acc + l.pj_plane0);
    SX_LAUNCH(NULL, LINNE_AMD_PROJECT_T_PRESET, k_wx_project_preset, wx_grid(pa.n16 > l.pj_cells ? pa.n16 : l.pj_cells), dim3(WXB_THREADS), 0, ctx->stream, pa);
    return LNN_OK;
}
static int wx_project_commit(LINNEAmdContext *ctx, const WxLaunch &l)
{
    WxProjectArgs pa;
    pa.tiles = l.pj_tiles; pa.ntiles = (uint32_t)l.ntile; pa.pwin = l.pj; pa.fail = l.fail; pa.sat = l.sat; pa.acc = (const int32_t *)l.acc;
    pa.planes = (const int8_t *)((const int32_t *)l.acc + l.pj_plane0); pa.raw = l.pj_raw; pa.rsum = l.pj_rsum;
    SX_LAUNCH(NULL, LINNE_AMD_PROJECT_T_PROJECT, k_wx_project, dim3(pa.ntiles ? pa.ntiles : 1u), dim3(WXP_THREADS), 0, ctx->stream, pa);
    return LNN_OK;
}
/* (a failing window's `saturated` stays as the caller left it) */
static void wx_project_read_back(const WxCall &c, uint32_t i, const uint32_t *words) { c.pj[i].saturated = (words && words[c.W + i]) ? 1u : 0u; }

static const WxConsumer WX_PLACE = { "DecodeWindowsDevice", 0u, NULL, WX_NO_BUCKETS, 0u, 0u, wx_place_check, wx_pcm_describe, NULL, wx_place_pass, NULL, wx_place_read_back, false, false };
static const WxConsumer WX_COMPARE = { "CompareWindowsDevice", 4u, wx_compare_back_preset, WX_NO_BUCKETS, 0u, 0u, wx_compare_check, wx_pcm_describe, NULL, wx_compare_pass, NULL, wx_compare_read_back, false, false };
static const WxConsumer WX_MEASURE = { "MeasureWindowsDevice", 0u, NULL, WX_BUCKETS_PER_CHANNEL, sizeof(struct LINNEAmdMeasure), 0u, wx_measure_check, wx_measure_describe, wx_measure_preset, wx_measure_pass, wx_measure_commit, NULL, false, false };
static const WxConsumer WX_DIGEST = { "DigestWindowsDevice", 0u, NULL, WX_BUCKETS_PER_FRAME, sizeof(uint32_t), WXD_POW_WORDS, wx_digest_check, wx_digest_describe, wx_digest_preset, wx_digest_pass, wx_digest_commit, NULL, false, false };
static const WxConsumer WX_QUIET = { "QuietWindowsDevice", WXQ_BACK_WORDS, wx_quiet_back_preset, WX_BITMASK, sizeof(uint64_t), 0u, wx_quiet_check, wx_quiet_describe, wx_quiet_preset, wx_quiet_pass, wx_quiet_commit, wx_quiet_read_back, false, false };
static const WxConsumer WX_HISTOGRAM = { "HistogramWindowsDevice", 0u, NULL, WX_BUCKETS_PER_BIN, sizeof(uint32_t), 0u, wx_histogram_check, wx_histogram_describe, wx_histogram_preset, wx_histogram_pass, wx_histogram_commit, NULL, false, false };
static const WxConsumer WX_RELATE = { "RelateWindowsDevice", 0u, NULL, WX_BUCKETS_PER_PAIR, sizeof(struct LINNEAmdRelation), 0u, wx_relate_check, wx_relate_describe, wx_relate_preset, wx_relate_pass, wx_relate_commit, NULL, false, false };
static const WxConsumer WX_MIX = { "MixWindowsDevice", 0u, NULL, WX_NO_BUCKETS, 0u, 0u, wx_mix_check, wx_mix_describe, NULL, wx_mix_pass, NULL, wx_place_read_back, true, false };
static const WxConsumer WX_RESAMPLE = { "ResampleWindowsDevice", 0u, NULL, WX_NO_BUCKETS, sizeof(int32_t), 0u, wx_resample_check, wx_resample_describe, wx_resample_preset, wx_place_pass, wx_resample_commit, wx_place_read_back, false, true };
static const WxConsumer WX_OVERLAY = { "OverlayWindowsDevice", 0u, NULL, WX_NO_BUCKETS, sizeof(int32_t), 0u, wx_overlay_check, wx_overlay_describe, NULL, wx_place_pass, wx_overlay_commit, NULL, false, false, true };
static const WxConsumer WX_LAGS = { "LagWindowsDevice", 0u, NULL, WX_NO_BUCKETS, sizeof(int32_t), 0u, wx_lags_check, wx_lags_describe, NULL, wx_place_pass, wx_lags_commit, NULL, false, false, false, true };
static const WxConsumer WX_PROJECT = { "ProjectWindowsDevice", 0u, NULL, WX_NO_BUCKETS, sizeof(int32_t), 0u, wx_project_check, wx_project_describe, wx_project_preset, wx_place_pass, wx_project_commit, wx_project_read_back, false, false, false, false, true };

/* the argument and index checks on window i, with their codes and texts (they name LINNEAmd_DecodeStreamDevice, whose arguments a
 * window's fields are; the consumer's own name its call).  *r1 = the last block the window overlaps (nb: it reaches behind the last
 * block); not set for a window of 0 samples */
static int wx_check_window(const LINNEAmdContext *ctx, const WxCall &c, uint32_t i, char *err, size_t cap, uint64_t *r1)
{
    const struct LINNEAmdWindow *w = &c.win[i];
    const LINNEAmdStreamIndex *x = w->index;
    err[0] = 0;
    if (c.rs) SX_TRY(wx_resample_spec_check(c, i, err, cap));      /* (in front of everything: the range check needs the ratio) */
    if (c.pj) SX_TRY(wx_project_spec_check(c, i, err, cap));       /* (likewise: the range check needs the hop) */
    if (!x || !w->d_stream) { snprintf(err, cap, "DecodeStreamDevice: null argument"); return LNN_INVALID_ARGUMENT; }
    if (c.use->bucketing == WX_NO_BUCKETS && !w->d_pcm && w->num_samples) { snprintf(err, cap, "DecodeStreamDevice: null argument"); return LNN_INVALID_ARGUMENT; }
    if (x->device != ctx->device) { snprintf(err, cap, "DecodeStreamDevice: the index belongs to device %d, the context to %d", x->device, ctx->device); return LNN_INVALID_ARGUMENT; }
    uint64_t total = x->header.num_samples;
    if (c.rs) total = wxr_length(total, c.rs[i].up, c.rs[i].down);         /* the range is one of the resampled stream */
    if (c.pj) { SX_TRY(wx_project_shape_check(c, i, x->shape.num_channels, err, cap)); total = wxp_length(total, c.pj[i].hop); }   /* the range is one of the stream's frames */
    if (w->first_sample > total || w->num_samples > total - w->first_sample) { snprintf(err, cap, "DecodeStreamDevice: samples [%llu, %llu) beyond the stream's %llu", (unsigned long long)w->first_sample, (unsigned long long)(w->first_sample + w->num_samples), (unsigned long long)total); return LNN_INVALID_ARGUMENT; }
    SX_TRY(c.use->check(c, i, err, cap));
    if (w->num_samples == 0) return LNN_OK;
    const uint64_t hi = c.rs ? wxr_input(w->first_sample, w->num_samples, c.rs[i], x->header.num_samples).hi
                      : c.pj ? wxp_input(w->first_sample, w->num_samples, c.pj[i], x->header.num_samples).hi : w->first_sample + w->num_samples;
    *r1 = (hi - 1u < x->covered) ? wx_block_of(x->h_first, x->nb, hi - 1u) : x->nb;
    if (x->fail_block >= 0 && (uint64_t)x->fail_block <= *r1) {
        snprintf(err, cap, "block %lld (byte %llu of the stream): %s", (long long)x->fail_block, (unsigned long long)x->fail_off,
                x->fail_code == LNN_NG ? "a block no encoder writes" : "damaged or truncated stream");
        return x->fail_code;
    }
    return LNN_OK;
}

/* LNN_OK: every window has its result (the words that came back, the Rice fail words first, are in fail_out); anything else fails
 * the whole call.  The plan (lnn_windows_plan.h) says which records go into which pass; a pass gathers, parses, Rice-decodes and
 * checks its COMPRESS blocks, synthesises them unless it is check-only, and hands its records to the call's consumer */
static int wx_decode(LINNEAmdContext *ctx, const WxCall &c, WxPlanned &pl, const uint32_t **fail_out)
{
    const WxConsumer &u = *c.use;
    const uint32_t W = c.W;
    const char *who = c.single ? "DecodeStreamDevice" : u.name, *advice = c.single ? "decode the range in parts" : "give group_frames";
    char text[sizeof(ctx->err)];
    *fail_out = NULL;
    /* 1. the checks per window; the live ones get their blocks, their group and their passes */
    std::vector<WxRange> rg(W);
    for (uint32_t i = 0; i < W; i++) {
        const struct LINNEAmdWindow &w = c.win[i];
        WxRange &r = rg[i];
        c.win[i].result = wx_check_window(ctx, c, i, text, sizeof(text), &r.r1);
        if (w.result != LNN_OK || w.num_samples == 0) continue;
        const LINNEAmdStreamIndex *x = w.index;
        r.live = 1; r.stream = w.d_stream; r.lo = w.first_sample; r.n = w.num_samples;
        r.x.shape = x->shape; r.x.nb = x->nb; r.x.covered = x->covered; r.x.stream_bytes = x->stream_bytes;
        r.x.h_off = x->h_off; r.x.h_first = x->h_first; r.x.h_size = x->h_size; r.x.h_type = x->h_type; r.x.h_nsmp = x->h_nsmp;
        u.describe(c, i, r);
    }
    switch (wx_plan_count(rg.data(), W, c.group_frames, pl)) {
    case WXP_SHAPES: snprintf(ctx->err, sizeof(ctx->err), "%s: more than %d stream shapes in one call", who, WX_MAXGROUPS); return LNN_NG;
    case WXP_BLOCKS: snprintf(ctx->err, sizeof(ctx->err), "%s: %llu blocks in one call: too many", who, (unsigned long long)pl.total_rec); return LNN_NG;
    default: break;
    }
    if (!pl.nlive) return LNN_OK;
    if (u.resamples) {
        wx_resample_count(rg.data(), W, pl);
        if (pl.rs_tiles > WX_MAX_TILES) { snprintf(ctx->err, sizeof(ctx->err), "%s: %llu tiles of outputs in one call: too many", who, (unsigned long long)pl.rs_tiles); return LNN_NG; }
    }
    if (u.overlays) {
        wx_overlay_count(c.ov_outs, c.ov_O, pl);
        if (pl.rs_tiles > WX_MAX_TILES) { snprintf(ctx->err, sizeof(ctx->err), "%s: %llu tiles of outputs in one call: too many", who, (unsigned long long)pl.rs_tiles); return LNN_NG; }
    }
    if (u.projects) {
        wx_project_count(rg.data(), W, pl);
        if (pl.rs_tiles > WX_MAX_TILES) { snprintf(ctx->err, sizeof(ctx->err), "%s: %llu tiles of outputs in one call: too many", who, (unsigned long long)pl.rs_tiles); return LNN_NG; }
    }
    if (u.lags) {
        wx_lag_count(c.lag_in, c.lag_Q, pl);
        if (pl.rs_tiles > WX_MAX_TILES) { snprintf(ctx->err, sizeof(ctx->err), "%s: %llu tiles of lags in one call: too many", who, (unsigned long long)pl.rs_tiles); return LNN_NG; }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    lnn_knobs_read_call(&ctx->knob);
    /* 2. the lists, in pinned memory */
    const WxLists ls = wx_lists(pl, W, u.back_words, u.bucketing != WX_NO_BUCKETS ? sizeof(WxBucket) : u.mixes ? sizeof(WxMix) : u.resamples ? sizeof(WxResample) : u.projects ? sizeof(WxProject) : 0u, u.resamples, u.overlays, u.lags, u.projects);
    SX_TRY(ensure_buf(ctx, &ctx->wstage, &ctx->wstage_cap, ls.bytes, true));
    uint8_t *hs_ = (uint8_t *)ctx->wstage;
    uint32_t *h_fail = (uint32_t *)(hs_ + ls.o_fail);
    for (uint32_t i = 0; i < W; i++) { h_fail[i] = WX_NOFAIL; h_fail[W + i] = 0u; }
    if (u.back_preset) u.back_preset((uint32_t *)(hs_ + ls.o_back), W);
    const WxProjLists pjl = { (WxProject *)(hs_ + ls.o_side), (WxProjTile *)(hs_ + ls.o_tile), (WxProjTable *)(hs_ + ls.o_pjtab), (int32_t *)(hs_ + ls.o_pjrsum), (int16_t *)(hs_ + ls.o_pjraw) };
    wx_plan_fill(rg.data(), W, c.group_frames, u.bucketing, pl, (WxWindow *)(hs_ + ls.o_win), u.bucketing != WX_NO_BUCKETS ? (WxBucket *)(hs_ + ls.o_side) : NULL,
            (WxBlock *)(hs_ + ls.o_rec), (uint32_t *)(hs_ + ls.o_crec), u.mixes ? (WxMix *)(hs_ + ls.o_side) : NULL,
            u.resamples ? (WxResample *)(hs_ + ls.o_side) : NULL, u.resamples ? (WxTile *)(hs_ + ls.o_tile) : NULL, u.resamples ? (uint32_t *)(hs_ + ls.o_coef) : NULL,
            u.overlays ? (WxOvSource *)memset(hs_ + ls.o_ovsrc, 0, sizeof(WxOvSource) * W) : NULL,
            u.lags ? (WxLagImage *)memset(hs_ + ls.o_lgimg, 0, sizeof(WxLagImage) * W) : NULL, u.projects ? &pjl : NULL);
    if (u.lags) wx_lag_fill(c.lag_in, c.lag_Q, pl, (WxLagProbe *)(hs_ + ls.o_lgprobe), (WxLagTile *)(hs_ + ls.o_tile), (uint32_t *)(hs_ + ls.o_lgrun));
    if (u.overlays) wx_overlay_fill(c.ov_outs, c.ov_O, rg.data(), pl, (WxOvOutput *)(hs_ + ls.o_ovout), (WxTile *)(hs_ + ls.o_tile));
    for (const WxPass &p : pl.passes) if (p.seg_bytes >= ((uint64_t)1 << 33)) { snprintf(ctx->err, sizeof(ctx->err), "%s: a pass of %llu stream bytes: %s", who, (unsigned long long)p.seg_bytes, advice); return LNN_NG; }
    /* 3. device memory (a buffer that grows waits for the stream first), then the one upload */
    SX_TRY(ensure_buf(ctx, &ctx->wdec, &ctx->wdec_cap, ls.bytes));
    const uint64_t o_acc = align_up(pl.scratch_bytes);             /* (the accumulators lie behind every pass's scratch) */
    SX_TRY(ensure_buf(ctx, &ctx->sdec, &ctx->sdec_cap, o_acc + (u.bucketing != WX_NO_BUCKETS || u.resamples || u.overlays || u.lags || u.projects ? u.acc_unit * (u.acc_prefix + pl.nacc) : 0u)));
    uint8_t *wd = (uint8_t *)ctx->wdec, *sd = (uint8_t *)ctx->sdec;
    uint32_t *d_fail = (uint32_t *)(wd + ls.o_fail);
    const WxWindow *d_win = (const WxWindow *)(wd + ls.o_win);
    WxLaunch ln;
    ln.side = (const WxBucket *)(wd + ls.o_side); ln.mix = (const WxMix *)(wd + ls.o_side); ln.wins = d_win; ln.acc = sd + o_acc; ln.back = (uint32_t *)(wd + ls.o_back); ln.fail = d_fail;
    ln.nwin = pl.nwin; ln.nacc = pl.nacc; ln.nout = pl.nout; ln.nmask = pl.nmask;
    ln.rs = (const WxResample *)(wd + ls.o_side); ln.tiles = (const WxTile *)(wd + ls.o_tile); ln.coef = (const uint32_t *)(wd + ls.o_coef); ln.ntile = pl.ntile; ln.sat = d_fail + W;
    ln.ov_outs = (const WxOvOutput *)(wd + ls.o_ovout); ln.ov_srcs = (const WxOvSource *)(wd + ls.o_ovsrc);
    ln.lg_tiles = (const WxLagTile *)(wd + ls.o_tile); ln.lg_runs = (const uint32_t *)(wd + ls.o_lgrun); ln.lg_probes = (const WxLagProbe *)(wd + ls.o_lgprobe);
    ln.lg_imgs = (const WxLagImage *)(wd + ls.o_lgimg); ln.nlgrun = pl.nlgrun; ln.lg_part = pl.lg_part;
    ln.pj = (const WxProject *)(wd + ls.o_side); ln.pj_tiles = (const WxProjTile *)(wd + ls.o_tile); ln.pj_tabs = (const WxProjTable *)(wd + ls.o_pjtab);
    ln.pj_rsum = (const int32_t *)(wd + ls.o_pjrsum); ln.pj_raw = (const int16_t *)(wd + ls.o_pjraw); ln.pj_ntab = (uint32_t)pl.pj_tabs.size(); ln.pj_plane0 = pl.pj_plane0; ln.pj_cells = 0;
    for (const WxProjTable &tb : pl.pj_tabs) { const uint64_t cells = (uint64_t)tb.Kpad * tb.Npad; if (cells > ln.pj_cells) ln.pj_cells = cells; }
    if (u.resamples || u.overlays || u.lags || u.projects) {        /* the plan named the images by their offsets: now they have an address */
        WxWindow *h_win = (WxWindow *)(hs_ + ls.o_win);
        for (uint32_t k = 0; k < pl.nwin; k++) h_win[k].out = ln.acc + (uintptr_t)h_win[k].out;
    }
    if (!ctx->outer_keep) ctx->nspans = 0;
    if (ctx->timing && !ctx->outer_keep) HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(wd, hs_, ls.bytes, hipMemcpyHostToDevice, ctx->stream));
    /* 4. the passes */
    if (u.preset) SX_TRY(u.preset(ctx, ln));
    for (const WxPass &p : pl.passes) {
        const LINNEAmdStreamIndex *x = c.win[pl.gwin[p.group]].index;
        const uint32_t C = x->shape.num_channels, S = x->shape.num_samples_per_block;
        HostShape hs;
        SX_TRY(shape_info(&x->shape, &hs));
        const WxScratch sc = wx_scratch(p.nc, C, S, p.seg_bytes);
        const WxBlock *d_rec = (const WxBlock *)(wd + ls.o_rec) + p.rec0;
        const uint32_t *d_crec = (const uint32_t *)(wd + ls.o_crec) + p.c0;
        uint32_t *d_nsmp = (uint32_t *)(sd + sc.o_nsmp);
        uint64_t *d_bpos = (uint64_t *)(sd + sc.o_bpos), *d_bend = (uint64_t *)(sd + sc.o_bend), *d_eb = (uint64_t *)(sd + sc.o_eb);
        int32_t *d_prm = (int32_t *)(sd + sc.o_prm), *d_data = (int32_t *)(sd + sc.o_data);
        uint8_t *d_seg = sd + sc.o_seg;
        if (p.nc) {
            SX_LAUNCH(NULL, LINNE_AMD_T_WX_GATHER, k_wx_gather, dim3(p.nc), dim3(WX_GATHER_THREADS), 0, ctx->stream, d_rec, d_crec, p.nc, d_seg);
            WxParamArgs pa; memset(&pa, 0, sizeof(pa));
            pa.recs = d_rec; pa.crec = d_crec; pa.ncomp = p.nc; pa.C = C; pa.bits = x->shape.bits_per_sample; pa.L = hs.L;
            for (uint32_t l = 0; l < hs.L; l++) { pa.P[l] = hs.P[l]; pa.coef_off[l] = hs.coef_off[l]; }
            pa.tab = x->d_tab; pa.prm = d_prm; pa.bitpos = d_bpos; pa.bitend = d_bend; pa.out_nsmp = d_nsmp;
            SX_LAUNCH(NULL, LINNE_AMD_T_WX_PARAMS, k_wx_params, dim3((p.nc + 63u) / 64u), dim3(64), 0, ctx->stream, pa);
            SX_TRY(rice_decode_launch(ctx, ctx->stream, &x->shape, d_seg, p.seg_bytes, d_bpos, d_bend, d_nsmp, p.nc, d_data, d_eb));
            SX_LAUNCH(NULL, LINNE_AMD_T_WX_RICE_CHECK, k_wx_rice_check, dim3((p.nc + 255u) / 256u), dim3(256), 0, ctx->stream, (const uint64_t *)d_eb, d_rec, d_crec, d_win, p.nc, d_fail);
            if (!p.check_only) SX_TRY(decode_frames_dev(ctx, &x->shape, hs, d_data, d_nsmp, p.nc, d_prm));
        }
        if (p.check_only) continue;
        WxPlaceArgs la; memset(&la, 0, sizeof(la));
        la.recs = d_rec; la.nrec = p.nrec; la.wins = d_win; la.fail = d_fail; la.C = C; la.S = S; la.bits = x->shape.bits_per_sample; la.pcm = d_data;
        la.sat = d_fail + W; la.scale = ldexpf(1.0f, 1 - (int)x->shape.bits_per_sample);
        la.xch = (S + SX_PLACE_THREADS - 1u) / SX_PLACE_THREADS;
        /* A launch takes fewer than 2^32 threads: a grid beyond that is not refused, its thread count wraps and the records behind the
         * wrap are never visited.  So the consumer takes the pass's records in runs of at most WX_LAUNCH_GROUPS / xch -- 65535 blocks
         * of 65535 samples; a record's workgroups read nothing but their own record, the pass's synthesis and the windows' lists */
        if (la.xch > WX_LAUNCH_GROUPS) la.xch = WX_LAUNCH_GROUPS;      /* (a record's workgroups stride over its pieces: fewer of them visit the same) */
        const uint32_t run = WX_LAUNCH_GROUPS / la.xch;
        for (uint32_t r0 = 0; r0 < p.nrec; r0 += run) {
            la.recs = d_rec + r0; la.nrec = p.nrec - r0 < run ? p.nrec - r0 : run;
            SX_TRY(u.pass(ctx, ln, la));
        }
    }
    if (u.commit) SX_TRY(u.commit(ctx, ln));
    /* 5. the fail words and what lies behind them, with the call's one wait */
    HIPCHK(ctx, hipMemcpyAsync(h_fail, d_fail, ls.back_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->timing) { HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream)); ctx->ev_valid = 1; }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < W; i++) if (pl.win[i].group >= 0 && h_fail[i] != WX_NOFAIL) c.win[i].result = LNN_NG;
    *fail_out = h_fail;
    return LNN_OK;
}

/* Every entry point behind its argument checks: the windows' results, then the call's -- the lowest-numbered failing window's code,
 * with its text in ctx->err (behind the window's number unless the call is the single one) */
static int wx_run(LINNEAmdContext *ctx, const WxCall &c)
{
    ctx->err[0] = 0;
    const uint32_t *fail = NULL;
    WxPlanned pl;
    int ret = items_try(ctx, [&] { return wx_decode(ctx, c, pl, &fail); });
    /* a HIP error, no memory: the whole call fails (wx_decode has waited and recorded where it did not) */
    if (items_end(ctx, NULL, ret, false, ret != LNN_OK, NULL, c.W, [&](uint32_t i) { c.win[i].result = LNN_NG; }) != LNN_OK) return LNN_NG;
    if (c.use->read_back) for (uint32_t i = 0; i < c.W; i++)
        if (c.win[i].result == LNN_OK) c.use->read_back(c, i, pl.win[i].group >= 0 ? fail : NULL);
    for (uint32_t i = 0; i < c.W; i++) {
        if (c.win[i].result == LNN_OK) continue;
        char text[sizeof(ctx->err)]; uint64_t r1;
        if (pl.win[i].group >= 0 && fail)
            snprintf(text, sizeof(text), "block %u (byte %llu of the stream): its Rice codes do not end where its size field says (a block no encoder writes)",
                    fail[i], (unsigned long long)c.win[i].index->h_off[fail[i]]);
        else (void)wx_check_window(ctx, c, i, text, sizeof(text), &r1);
        items_first_text(ctx, "window", i, c.single, text);
        return c.win[i].result;
    }
    return LNN_OK;
}
/* the windows calls' own argument checks */
static int wx_entry(LINNEAmdContext *ctx, WxCall c, bool complete)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->err[0] = 0;
    if (c.W == 0) return LNN_OK;
    if (!complete) { snprintf(ctx->err, sizeof(ctx->err), "%s: null argument", c.use->name); return LNN_INVALID_ARGUMENT; }
    return wx_run(ctx, c);
}

extern "C" int LINNEAmd_DecodeWindowsDeviceLayout(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, struct LINNEAmdPcmLayout *layouts,
        uint32_t num_windows, uint32_t group_frames)
{
    return wx_entry(ctx, wx_call(&WX_PLACE, windows, num_windows, group_frames, layouts, layouts), windows != NULL);
}
/* int32 planar windows: the call above without layouts */
extern "C" int LINNEAmd_DecodeWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, uint32_t num_windows, uint32_t group_frames)
{
    return LINNEAmd_DecodeWindowsDeviceLayout(ctx, windows, NULL, num_windows, group_frames);
}

/* the windows compared with the PCM they name instead of written into it */
extern "C" int LINNEAmd_CompareWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, const struct LINNEAmdPcmLayout *layouts,
        struct LINNEAmdDiff *diffs, uint32_t num_windows, uint32_t group_frames)
{
    return wx_entry(ctx, wx_call(&WX_COMPARE, windows, num_windows, group_frames, layouts, diffs), windows && diffs);
}

/* the windows reduced to a table per window instead of written */
extern "C" int LINNEAmd_MeasureWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, const struct LINNEAmdMeasureSpec *specs,
        uint32_t num_windows, uint32_t group_frames)
{
    return wx_entry(ctx, wx_call(&WX_MEASURE, windows, num_windows, group_frames, specs, NULL), windows && specs);
}

/* the windows hashed to a table per window instead of written */
extern "C" int LINNEAmd_DigestWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, const struct LINNEAmdDigestSpec *specs,
        uint32_t num_windows, uint32_t group_frames)
{
    return wx_entry(ctx, wx_call(&WX_DIGEST, windows, num_windows, group_frames, specs, NULL), windows && specs);
}

/* the windows' quiet runs listed in a table per window instead of their samples written */
extern "C" int LINNEAmd_QuietWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, const struct LINNEAmdQuietSpec *specs,
        struct LINNEAmdQuiet *answers, uint32_t num_windows, uint32_t group_frames)
{
    return wx_entry(ctx, wx_call(&WX_QUIET, windows, num_windows, group_frames, specs, answers), windows && specs && answers);
}

/* the windows' sample levels counted into a table per window instead of their samples written */
extern "C" int LINNEAmd_HistogramWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, const struct LINNEAmdHistogramSpec *specs,
        uint32_t num_windows, uint32_t group_frames)
{
    return wx_entry(ctx, wx_call(&WX_HISTOGRAM, windows, num_windows, group_frames, specs, NULL), windows && specs);
}

/* the windows' channel pairs reduced into a table per window instead of their samples written */
extern "C" int LINNEAmd_RelateWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, const struct LINNEAmdRelateSpec *specs,
        uint32_t num_windows, uint32_t group_frames)
{
    return wx_entry(ctx, wx_call(&WX_RELATE, windows, num_windows, group_frames, specs, NULL), windows && specs);
}

/* the windows' channels through a matrix per window on their way into the PCM */
extern "C" int LINNEAmd_MixWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, const struct LINNEAmdMixSpec *specs,
        struct LINNEAmdPcmLayout *layouts, uint32_t num_windows, uint32_t group_frames)
{
    WxCall c = wx_call(&WX_MIX, windows, num_windows, group_frames, layouts, layouts);
    c.mix = specs;
    return wx_entry(ctx, c, windows && specs);
}

/* the windows are ranges of the stream resampled by a ratio per window, through a polyphase FIR per window, on their way into the PCM */
extern "C" int LINNEAmd_ResampleWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, const struct LINNEAmdResampleSpec *specs,
        struct LINNEAmdPcmLayout *layouts, uint32_t num_windows, uint32_t group_frames)
{
    WxCall c = wx_call(&WX_RESAMPLE, windows, num_windows, group_frames, layouts, layouts);
    c.rs = specs;
    return wx_entry(ctx, c, windows && specs);
}
extern "C" uint64_t LINNEAmd_ResampleLength(uint64_t num_samples, uint32_t up, uint32_t down) { return wxr_length(num_samples, up, down); }

/* the windows are ranges of the stream's frames, every frame projected on the rows of the window's int16 basis, into a table per window */
extern "C" int LINNEAmd_ProjectWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows, struct LINNEAmdProjectSpec *specs,
        uint32_t num_windows, uint32_t group_frames)
{
    WxCall c = wx_call(&WX_PROJECT, windows, num_windows, group_frames, NULL, NULL);
    c.pj = specs;
    return wx_entry(ctx, c, windows && specs);
}
extern "C" uint64_t LINNEAmd_ProjectLength(uint64_t num_samples, uint32_t hop) { return wxp_length(num_samples, hop); }

/* ---- LINNEAmd_OverlayWindowsDevice: the sources of all outputs are the windows of one windows call ---- */
/* the gain (q + step * i) >> 32 lies in int16: in 128 bits */
static bool ov_gain_fits(int64_t q, int64_t step, uint64_t i)
{
    const __int128 g = ((__int128)q + (__int128)step * (__int128)(unsigned __int128)i) >> 32;
    return g >= -32768 && g <= 32767;
}
/* the checks on output o alone, in front of its sources' window checks; *C: the channel count its sources share */
static int ov_check_output(const struct LINNEAmdOverlay &o, const struct LINNEAmdPcmLayout *ly, char *err, size_t cap, uint32_t *C)
{
    const char *who = "OverlayWindowsDevice";
    err[0] = 0;
    if (o.num_sources < 1u || o.num_sources > LINNE_AMD_OVERLAY_MAX_SOURCES) { snprintf(err, cap, "%s: num_sources %u is not 1 .. %u", who, o.num_sources, (unsigned)LINNE_AMD_OVERLAY_MAX_SOURCES); return LNN_INVALID_ARGUMENT; }
    if (!o.sources) { snprintf(err, cap, "%s: null sources", who); return LNN_INVALID_ARGUMENT; }
    if (o.shift > 31u) { snprintf(err, cap, "%s: shift %u > 31", who, o.shift); return LNN_INVALID_ARGUMENT; }
    if (o.clip_bits == 1u || o.clip_bits > 32u) { snprintf(err, cap, "%s: clip_bits %u is neither 0 nor 2 .. 32", who, o.clip_bits); return LNN_INVALID_ARGUMENT; }
    if (o.reserved != 0u) { snprintf(err, cap, "%s: reserved is not 0", who); return LNN_INVALID_ARGUMENT; }
    for (uint32_t j = 0; j < o.num_sources; j++) {
        const struct LINNEAmdOverlaySource &s = o.sources[j];
        if (!s.index || !s.d_stream) { snprintf(err, cap, "%s: source %u: null argument", who, j); return LNN_INVALID_ARGUMENT; }
        if (s.reserved != 0u) { snprintf(err, cap, "%s: source %u: reserved is not 0", who, j); return LNN_INVALID_ARGUMENT; }
        if (s.num_samples == 0u) { snprintf(err, cap, "%s: source %u: num_samples 0", who, j); return LNN_INVALID_ARGUMENT; }
        if (s.at > o.num_samples || s.num_samples > o.num_samples - s.at) { snprintf(err, cap, "%s: source %u: at %llu + %llu samples beyond the output's %llu", who, j, (unsigned long long)s.at, (unsigned long long)s.num_samples, (unsigned long long)o.num_samples); return LNN_INVALID_ARGUMENT; }
        if (!ov_gain_fits(s.gain_q32, s.step_q32, 0u) || !ov_gain_fits(s.gain_q32, s.step_q32, s.num_samples - 1u)) { snprintf(err, cap, "%s: source %u: a gain outside -32768 .. 32767", who, j); return LNN_INVALID_ARGUMENT; }
    }
    *C = o.sources[0].index->shape.num_channels;
    for (uint32_t j = 1; j < o.num_sources; j++)
        if (o.sources[j].index->shape.num_channels != *C) { snprintf(err, cap, "%s: source %u: %u channels, source 0 has %u", who, j, o.sources[j].index->shape.num_channels, *C); return LNN_INVALID_ARGUMENT; }
    if (!o.d_pcm) { snprintf(err, cap, "%s: null d_pcm", who); return LNN_INVALID_ARGUMENT; }
    if (ly) {
        const int why = sb_layout_check(ly->format, ly->channel_stride, ly->sample_stride, (uint64_t)(uintptr_t)o.d_pcm, *C, o.num_samples, true);
        if (why != SB_LY_OK) { snprintf(err, cap, "%s: %s", who, sb_layout_text(why)); return LNN_INVALID_ARGUMENT; }
    } else if (*C > 1u && o.pcm_stride < o.num_samples) { snprintf(err, cap, "%s: pcm_stride %llu < %llu samples", who, (unsigned long long)o.pcm_stride, (unsigned long long)o.num_samples); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}

extern "C" int LINNEAmd_OverlayWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdOverlay *outputs, struct LINNEAmdPcmLayout *layouts,
        uint32_t num_outputs, uint32_t group_frames)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->err[0] = 0;
    const uint32_t O = num_outputs;
    if (O == 0) return LNN_OK;
    if (!outputs) { snprintf(ctx->err, sizeof(ctx->err), "OverlayWindowsDevice: null argument"); return LNN_INVALID_ARGUMENT; }
    char text[sizeof(ctx->err)];
    std::vector<WxOvOut> outs;
    std::vector<struct LINNEAmdWindow> wins;
    std::vector<const struct LINNEAmdOverlaySource *> srcs;
    const uint32_t *fail = NULL;
    WxPlanned pl;
    WxCall c = wx_call(&WX_OVERLAY, NULL, 0, group_frames, NULL, NULL);
    int ret = items_try(ctx, [&] {
        /* 1. the outputs' own checks; the sources of those that pass become the call's windows */
        outs.resize(O);
        for (uint32_t k = 0; k < O; k++) {
            struct LINNEAmdOverlay &o = outputs[k];
            WxOvOut &d = outs[k];
            uint32_t C = 0;
            memset(&d, 0, sizeof(d));
            d.w0 = (uint32_t)wins.size();
            o.result = ov_check_output(o, layouts ? layouts + k : NULL, text, sizeof(text), &C);
            if (o.result != LNN_OK) continue;
            d.checked = 1; d.nsrc = o.num_sources; d.n = o.num_samples; d.out = o.d_pcm; d.shift = o.shift; d.clip_bits = o.clip_bits;
            if (layouts) { d.fmt = layouts[k].format; d.stride = layouts[k].channel_stride; d.sstride = layouts[k].sample_stride; }
            else { d.fmt = LINNE_AMD_PCM_S32; d.stride = o.pcm_stride; d.sstride = 1u; }
            for (uint32_t j = 0; j < o.num_sources; j++) {
                const struct LINNEAmdOverlaySource &s = o.sources[j];
                struct LINNEAmdWindow w;
                w.index = s.index; w.d_stream = s.d_stream; w.first_sample = s.first_sample; w.num_samples = s.num_samples;
                w.d_pcm = o.d_pcm; w.pcm_stride = 0u; w.result = LNN_OK;   /* (the passes write the source's image, not this) */
                wins.push_back(w); srcs.push_back(&s);
                /* A source the host refuses ends the output's windows: the output cannot be written any more, and only the sources in
                 * front of this one can still change its code, by failing their Rice check */
                const WxCall one = wx_call(&WX_OVERLAY, &w, 1, 0, NULL, NULL);
                uint64_t r1;
                if (wx_check_window(ctx, one, 0, text, sizeof(text), &r1) != LNN_OK) { d.nsrc = j + 1u; break; }
            }
        }
        if (wins.size() >= 0xFFFFFFFFull) { snprintf(ctx->err, sizeof(ctx->err), "OverlayWindowsDevice: %llu sources in one call: too many", (unsigned long long)wins.size()); return (int)LNN_NG; }
        c.win = wins.data(); c.W = (uint32_t)wins.size(); c.ov_src = srcs.data(); c.ov_outs = outs.data(); c.ov_O = O;
        /* 2. the windows call over all sources */
        return wx_decode(ctx, c, pl, &fail);
    });
    if (items_end(ctx, NULL, ret, false, ret != LNN_OK, NULL, O, [&](uint32_t k) { outputs[k].result = LNN_NG; }) != LNN_OK) return LNN_NG;
    /* 3. an output has the result of its lowest-numbered failing source; the call that of its lowest-numbered failing output */
    int first = LNN_OK;
    for (uint32_t k = 0; k < O; k++) {
        struct LINNEAmdOverlay &o = outputs[k];
        const WxOvOut &d = outs[k];
        uint32_t C, j = 0;
        if (d.checked) {
            while (j < d.nsrc && wins[d.w0 + j].result == LNN_OK) j++;
            if (j == d.nsrc) { if (layouts) layouts[k].saturated = (fail && fail[c.W + d.w0]) ? 1u : 0u; continue; }
            o.result = wins[d.w0 + j].result;
        }
        if (first != LNN_OK) continue;
        first = o.result;
        if (!d.checked) (void)ov_check_output(o, layouts ? layouts + k : NULL, text, sizeof(text), &C);
        else {
            const uint32_t i = d.w0 + j;
            char inner[sizeof(ctx->err)]; uint64_t r1;
            if (pl.win[i].group >= 0 && fail)
                snprintf(inner, sizeof(inner), "block %u (byte %llu of the stream): its Rice codes do not end where its size field says (a block no encoder writes)",
                        fail[i], (unsigned long long)wins[i].index->h_off[fail[i]]);
            else (void)wx_check_window(ctx, c, i, inner, sizeof(inner), &r1);
            snprintf(text, sizeof(text), "source %u: %.*s", j, (int)sizeof(text) - 24, inner);
        }
        items_first_text(ctx, "output", k, false, text);
    }
    return first;
}

/* ---- LINNEAmd_LagWindowsDevice: the needles and the clipped haystacks of all probes are the windows of one windows call ---- */
/* the checks on probe q alone, in front of its windows' checks */
static int lg_check_probe(const struct LINNEAmdLagProbe &q, char *err, size_t cap)
{
    const char *who = "LagWindowsDevice";
    err[0] = 0;
    if (!q.index_a || !q.d_stream_a || !q.index_b || !q.d_stream_b) { snprintf(err, cap, "%s: null argument", who); return LNN_INVALID_ARGUMENT; }
    if (!q.d_out) { snprintf(err, cap, "%s: null d_out", who); return LNN_INVALID_ARGUMENT; }
    if (q.reserved != 0u) { snprintf(err, cap, "%s: reserved is not 0", who); return LNN_INVALID_ARGUMENT; }
    if (q.num_samples == 0u) { snprintf(err, cap, "%s: num_samples 0", who); return LNN_INVALID_ARGUMENT; }
    if (q.num_lags < 1u || q.num_lags > LINNE_AMD_LAG_MAX_LAGS) { snprintf(err, cap, "%s: num_lags %u is not 1 .. %u", who, q.num_lags, (unsigned)LINNE_AMD_LAG_MAX_LAGS); return LNN_INVALID_ARGUMENT; }
    if (q.num_pairs < 1u || q.num_pairs > LINNE_MAX_NUM_CHANNELS) { snprintf(err, cap, "%s: num_pairs %u is not 1 .. %u", who, q.num_pairs, (unsigned)LINNE_MAX_NUM_CHANNELS); return LNN_INVALID_ARGUMENT; }
    if ((unsigned __int128)q.num_samples * q.num_lags * q.num_pairs > (unsigned __int128)LINNE_AMD_LAG_MAX_PRODUCTS) {
        snprintf(err, cap, "%s: %llu samples * %u lags * %u pairs > 2^38 products", who, (unsigned long long)q.num_samples, q.num_lags, q.num_pairs);
        return LNN_INVALID_ARGUMENT;
    }
    for (uint32_t p = 0; p < q.num_pairs; p++) {
        if (q.chan_a[p] >= q.index_a->shape.num_channels) { snprintf(err, cap, "%s: pair %u: channel %u of a needle of %u", who, p, q.chan_a[p], q.index_a->shape.num_channels); return LNN_INVALID_ARGUMENT; }
        if (q.chan_b[p] >= q.index_b->shape.num_channels) { snprintf(err, cap, "%s: pair %u: channel %u of a haystack of %u", who, p, q.chan_b[p], q.index_b->shape.num_channels); return LNN_INVALID_ARGUMENT; }
    }
    if ((uint64_t)(uintptr_t)q.d_out & 7u) { snprintf(err, cap, "%s: d_out is not 8-byte aligned", who); return LNN_INVALID_ARGUMENT; }
    if ((uint64_t)(uintptr_t)q.d_a_sq & 7u) { snprintf(err, cap, "%s: d_a_sq is not 8-byte aligned", who); return LNN_INVALID_ARGUMENT; }
    if (q.pair_stride < q.num_lags) { snprintf(err, cap, "%s: pair_stride %llu < %u lags", who, (unsigned long long)q.pair_stride, q.num_lags); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}
/* the haystack samples probe q reads, clipped to the stream's [0, N_b): [*lo, *lo + *n), *n 0 when the range misses the stream; *b0:
 * first_b + lag_first relative to *lo, never positive.  In 128 bits */
static void lg_haystack(const struct LINNEAmdLagProbe &q, uint64_t *lo, uint64_t *n, int64_t *b0)
{
    const __int128 S = (__int128)(unsigned __int128)q.first_b + q.lag_first, E = S + (q.num_lags - 1u) + (__int128)(unsigned __int128)q.num_samples;
    const __int128 N = (__int128)(unsigned __int128)q.index_b->header.num_samples;
    const __int128 a = S < 0 ? (__int128)0 : S, b = E > N ? N : E;
    *b0 = S < 0 ? (int64_t)S : 0;       /* (>= -2^63: first_b is not negative) */
    *lo = 0u; *n = 0u;
    if (a < b) { *lo = (uint64_t)a; *n = (uint64_t)(b - a); }
}

extern "C" int LINNEAmd_LagWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdLagProbe *probes, uint32_t num_probes, uint32_t group_frames)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->err[0] = 0;
    const uint32_t Q = num_probes;
    if (Q == 0) return LNN_OK;
    if (!probes) { snprintf(ctx->err, sizeof(ctx->err), "LagWindowsDevice: null argument"); return LNN_INVALID_ARGUMENT; }
    char text[sizeof(ctx->err)];
    std::vector<WxLagIn> in;
    std::vector<struct LINNEAmdWindow> wins;
    const uint32_t *fail = NULL;
    WxPlanned pl;
    WxCall c = wx_call(&WX_LAGS, NULL, 0, group_frames, NULL, NULL);
    int ret = items_try(ctx, [&] {
        /* 1. the probes' own checks; the needle and the clipped haystack of those that pass become the call's windows */
        in.resize(Q);
        for (uint32_t k = 0; k < Q; k++) {
            struct LINNEAmdLagProbe &q = probes[k];
            WxLagIn &d = in[k];
            memset(&d, 0, sizeof(d));
            d.wa = (uint32_t)wins.size(); d.wb = WXL_NOWIN;
            q.result = lg_check_probe(q, text, sizeof(text));
            if (q.result != LNN_OK) continue;
            d.checked = 1; d.n = q.num_samples; d.nlags = q.num_lags; d.npair = q.num_pairs; d.out = q.d_out; d.pstride = q.pair_stride; d.a_sq = q.d_a_sq;
            memcpy(d.ca, q.chan_a, sizeof(d.ca)); memcpy(d.cb, q.chan_b, sizeof(d.cb));
            struct LINNEAmdWindow w;
            w.index = q.index_a; w.d_stream = q.d_stream_a; w.first_sample = q.first_a; w.num_samples = q.num_samples;
            w.d_pcm = (int32_t *)q.d_out; w.pcm_stride = 0u; w.result = LNN_OK;    /* (the passes write the window's image, not this) */
            wins.push_back(w);
            /* a needle the host refuses ends the probe's windows: the probe cannot be answered any more */
            const WxCall one = wx_call(&WX_LAGS, &w, 1, 0, NULL, NULL);
            uint64_t r1, lo, n;
            if (wx_check_window(ctx, one, 0, text, sizeof(text), &r1) != LNN_OK) continue;
            lg_haystack(q, &lo, &n, &d.b0);
            if (n == 0) continue;
            d.wb = (uint32_t)wins.size();
            w.index = q.index_b; w.d_stream = q.d_stream_b; w.first_sample = lo; w.num_samples = n;
            wins.push_back(w);
        }
        if (wins.size() >= 0xFFFFFFFFull) { snprintf(ctx->err, sizeof(ctx->err), "LagWindowsDevice: %llu windows in one call: too many", (unsigned long long)wins.size()); return (int)LNN_NG; }
        c.win = wins.data(); c.W = (uint32_t)wins.size(); c.lag_in = in.data(); c.lag_Q = Q;
        /* 2. the windows call over all needles and haystacks */
        return wx_decode(ctx, c, pl, &fail);
    });
    if (items_end(ctx, NULL, ret, false, ret != LNN_OK, NULL, Q, [&](uint32_t k) { probes[k].result = LNN_NG; }) != LNN_OK) return LNN_NG;
    /* 3. a probe has the result of its needle, then of its haystack; the call that of its lowest-numbered failing probe */
    int first = LNN_OK;
    for (uint32_t k = 0; k < Q; k++) {
        struct LINNEAmdLagProbe &q = probes[k];
        const WxLagIn &d = in[k];
        uint32_t i = d.wa; const char *what = "needle";
        if (d.checked) {
            if (wins[i].result == LNN_OK && d.wb != WXL_NOWIN) { i = d.wb; what = "haystack"; }
            if (wins[i].result == LNN_OK) continue;
            q.result = wins[i].result;
        }
        if (first != LNN_OK) continue;
        first = q.result;
        if (!d.checked) (void)lg_check_probe(q, text, sizeof(text));
        else {
            char inner[sizeof(ctx->err)]; uint64_t r1;
            if (pl.win[i].group >= 0 && fail)
                snprintf(inner, sizeof(inner), "block %u (byte %llu of the stream): its Rice codes do not end where its size field says (a block no encoder writes)",
                        fail[i], (unsigned long long)wins[i].index->h_off[fail[i]]);
            else (void)wx_check_window(ctx, c, i, inner, sizeof(inner), &r1);
            snprintf(text, sizeof(text), "%s: %.*s", what, (int)sizeof(text) - 24, inner);
        }
        items_first_text(ctx, "probe", k, false, text);
    }
    return first;
}

/* one window of one stream */
extern "C" int LINNEAmd_DecodeStreamDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdStreamIndex *x, const uint8_t *d_stream,
        uint64_t first_sample, uint64_t num_samples, int32_t *d_pcm, uint64_t pcm_stride)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    struct LINNEAmdWindow w;
    w.index = x; w.d_stream = d_stream; w.first_sample = first_sample; w.num_samples = num_samples; w.d_pcm = d_pcm; w.pcm_stride = pcm_stride; w.result = LNN_OK;
    WxCall c = wx_call(&WX_PLACE, &w, 1, 0, NULL, NULL);
    c.single = true;
    return wx_run(ctx, c);
}


/* ================================================================================================
 * PCM in device memory -> .lnn streams in device memory: many tracks in one call, and one track as the one-track case of it
 * (lnn_k_stream_enc.h, lnn_stream_batch.h)
 * ============================================================================================== */
extern "C" uint64_t LINNEAmd_EncodeStreamBound(const struct LINNEHeader *header)
{
    if (!header || header->num_samples_per_block == 0) return 0;
    const uint64_t S = header->num_samples_per_block, blocks = ((uint64_t)header->num_samples + S - 1u) / S;
    return LINNE_HEADER_SIZE + blocks * (64u + (uint64_t)header->num_channels * S * 8u);
}

extern "C" int64_t LINNEAmd_GetLastStreamEncodeCount(struct LINNEAmdContext *ctx, int which)
{
    if (!ctx || which < 0 || which > 3) return -1;
    return ctx->senc_count[which];
}

/* LINNEEncoder_SetEncodeParameter's checks (lnn_api.c), in its order, on an encoder with room for the header */
static int se_parameter_code(const struct LINNEHeader *h)
{
    struct lnn_layers ly;
    if (h->num_channels == 0 || h->bits_per_sample == 0 || h->sampling_rate == 0 || h->num_samples_per_block == 0
            || h->preset >= LINNE_NUM_PARAMETER_PRESETS || (int)h->ch_process_method >= (int)LINNE_CH_PROCESS_METHOD_INVALID
            || (int)h->ch_process_method < 0) return LNN_INVALID_FORMAT;
    const struct LINNEAmdShape shape = header_shape(h);
    if (lnn_shape_layers(&shape, &ly) != 0) return LNN_INVALID_FORMAT;
    for (uint32_t l = 0; l < ly.num_layers; l++) if (h->num_samples_per_block <= ly.size[l]) return LNN_INVALID_FORMAT;
    if (h->num_channels > LINNE_MAX_NUM_CHANNELS) return LNN_INSUFFICIENT_BUFFER;
    return LNN_OK;
}

static_assert(SB_MAXLEN == LNN_MAXCLS, "lnn_stream_batch.h cuts the rows of a pass by the analysis' limit");

extern "C" int64_t LINNEAmd_GetLastStreamBatchCount(struct LINNEAmdContext *ctx, int which)
{
    if (!ctx || which < 0 || which > 2) return -1;
    return ctx->sbatch_count[which];
}

/* a track of the call on the host */
struct SbHost {
    int32_t result; char text[160];
    struct LINNEAmdShape shape;
    bool live;                          /* it passed its checks and no block of it was refused so far */
    bool writing; uint64_t pos, room; double state;
    uint32_t id;                        /* its number in its shape group */
    uint32_t fmt; uint64_t cs, ss;      /* its PCM's layout */
};

/* the argument and header checks of one track, with the codes, the texts and the order LINNEAmd_EncodeStreamDevice documents */
static int sb_check_track(struct LINNEAmdTrack *t, const struct LINNEAmdPcmLayout *ly, SbHost *h)
{
    char *err = h->text; const size_t cap = sizeof(h->text);
    const struct LINNEHeader *header = &t->header;
    err[0] = 0;
    if (!t->d_pcm || !t->d_out) { snprintf(err, cap, "EncodeStreamDevice: null argument"); return LNN_INVALID_ARGUMENT; }
    if ((uintptr_t)t->d_out & 3u) { snprintf(err, cap, "EncodeStreamDevice: d_out is not 4-byte aligned"); return LNN_INVALID_ARGUMENT; }
    if (ly) {
        const int why = sb_layout_check(ly->format, ly->channel_stride, ly->sample_stride, (uint64_t)(uintptr_t)t->d_pcm, header->num_channels, header->num_samples, false);
        if (why != SB_LY_OK) { snprintf(err, cap, "EncodeStreamDevice: %s", sb_layout_text(why)); return LNN_INVALID_ARGUMENT; }
        h->fmt = ly->format; h->cs = ly->channel_stride; h->ss = ly->sample_stride;
    } else { h->fmt = LINNE_AMD_PCM_S32; h->cs = t->pcm_stride; h->ss = 1u; }
    t->out_bytes = 0;
    int ret = se_parameter_code(header);
    if (ret != LNN_OK) { snprintf(err, cap, "EncodeStreamDevice: header refused by SetEncodeParameter's checks"); return ret; }
    {
        uint8_t hb[LINNE_HEADER_SIZE];
        ret = (int)LINNEEncoder_EncodeHeader(header, hb, LINNE_HEADER_SIZE);
        if (ret != LNN_OK) { snprintf(err, cap, "EncodeStreamDevice: header refused by EncodeHeader"); return t->capacity < LINNE_HEADER_SIZE ? LNN_INSUFFICIENT_BUFFER : ret; }
    }
    h->shape = header_shape(header);
    HostShape hs;
    if ((ret = shape_info(&h->shape, &hs)) != LNN_OK) { snprintf(err, cap, "EncodeStreamDevice: a shape the device path does not take"); return ret; }
    if (!ly && h->shape.num_channels > 1u && t->pcm_stride < header->num_samples) { snprintf(err, cap, "EncodeStreamDevice: pcm_stride %llu < %u samples", (unsigned long long)t->pcm_stride, header->num_samples); return LNN_INVALID_ARGUMENT; }
    return LNN_OK;
}

/* The tracks `members` (numbers in `tracks`, all of `shape`, all live) through their passes.  LNN_OK: every member has its result in
 * host[]; anything else fails the whole call. */
static int sb_group_run(LINNEAmdContext *ctx, struct LINNEAmdTrack *tracks, SbHost *host, const std::vector<uint32_t> &members,
        const struct LINNEAmdShape &shape, uint32_t group_frames)
{
    HostShape hs;
    SX_TRY(shape_info(&shape, &hs));
    const uint32_t C = shape.num_channels, S = shape.num_samples_per_block, n = (uint32_t)members.size();
    const uint64_t CS = (uint64_t)C * S;
    std::vector<uint64_t> samples(n);
    uint64_t F = 0;
    for (uint32_t k = 0; k < n; k++) { samples[k] = tracks[members[k]].header.num_samples; F += sb_frames(samples[k], S); host[members[k]].id = k; }
    uint64_t G = group_frames ? (group_frames < F ? group_frames : F) : F;
    if (G * C > 0x7FFFFFFFull) G = 0x7FFFFFFFull / C;              /* grid.x of the channel-frame kernels */
    const uint64_t T = n < G ? n : G;                               /* the tracks of a pass: each has a frame in it */
    /* scratch of one pass */
    uint64_t at = 0;
    const uint64_t o_frames = at; at = align_up(at + sizeof(int32_t) * CS * G);
    const uint64_t o_resid = at; at = align_up(at + sizeof(int32_t) * CS * G);
    const uint64_t o_prm = at; at = align_up(at + sizeof(int32_t) * LINNE_AMD_PARAM_WORDS * C * G);
    const uint64_t o_st = at; at = align_up(at + sizeof(double) * LINNE_AMD_STAT_WORDS * C * G);
    const uint64_t o_plan = at; at = align_up(at + (uint64_t)LINNE_AMD_RICE_PLAN_BYTES * C * G);
    const uint64_t o_nz = at; at = align_up(at + sizeof(uint32_t) * G);
    const uint64_t o_cmp = at; at = align_up(at + sizeof(uint2) * C * G);
    const uint64_t o_types = at; at = align_up(at + G);
    const uint64_t o_size = at; at = align_up(at + sizeof(uint32_t) * G);
    const uint64_t o_status = at; at = align_up(at + sizeof(int32_t) * G);
    const uint64_t o_off = at; at = align_up(at + sizeof(uint64_t) * (G + 1u));
    const uint64_t o_cfbit = at; at = align_up(at + sizeof(uint64_t) * C * G);
    const uint64_t o_fail = at; at = align_up(at + sizeof(uint32_t) * (uint64_t)n);                /* a word per track */
    const uint64_t o_tab = at; at = align_up(at + sizeof(SeTables));
    const uint64_t tables_bytes = align_up(sizeof(SbTrack) * T) + sizeof(SbRow) * G;
    const uint64_t o_tables = at; at = align_up(at + tables_bytes);             /* SbTrack[T], then SbRow[G] */
    const uint64_t o_tout = at; at = align_up(at + sizeof(SbTrackOut) * T);
    const uint64_t o_hdr = at; at = align_up(at + (sizeof(uint8_t *) + 32u) * (uint64_t)n);     /* n pointers, then n * 32 bytes */
    SX_TRY(ensure_buf(ctx, &ctx->senc, &ctx->senc_cap, at));
    uint8_t *sd = (uint8_t *)ctx->senc;
    int32_t *d_frames = (int32_t *)(sd + o_frames), *d_resid = (int32_t *)(sd + o_resid), *d_prm = (int32_t *)(sd + o_prm), *d_status = (int32_t *)(sd + o_status);
    double *d_st = (double *)(sd + o_st);
    uint8_t *d_plan = sd + o_plan, *d_types = sd + o_types;
    uint32_t *d_nz = (uint32_t *)(sd + o_nz), *d_size = (uint32_t *)(sd + o_size), *d_fail = (uint32_t *)(sd + o_fail);
    uint2 *d_cmp = (uint2 *)(sd + o_cmp);
    uint64_t *d_off = (uint64_t *)(sd + o_off), *d_cfbit = (uint64_t *)(sd + o_cfbit);
    SeTables *d_tab = (SeTables *)(sd + o_tab);
    SbTrack *d_trk = (SbTrack *)(sd + o_tables);
    SbRow *d_rows = (SbRow *)(sd + o_tables + align_up(sizeof(SbTrack) * T));
    SbTrackOut *d_tout = (SbTrackOut *)(sd + o_tout);
    /* host buffers (std::bad_alloc is the caller's to catch): per row, per slot, per track of a pass */
    std::vector<uint2> h_cmp(C * G);
    std::vector<double> h_st(LINNE_AMD_STAT_WORDS * C * G), s_st(LINNE_AMD_STAT_WORDS * C * G);
    std::vector<uint32_t> h_nz(G), h_nsmp(G), s_nsmp(G), h_settle(C * G), h_settle_n(C * G), h_bad(n);
    std::vector<uint8_t> s_nz(G), s_types(G), h_types(G), h_tables(tables_bytes), h_plans;
    std::vector<int32_t> h_res;
    std::vector<SbTrack> h_trk2(T);                                 /* the second upload of a pass (pos, write) has a buffer of its own */
    std::vector<SbTrackOut> h_tout(T);
    {
        SeTables t;
        sx_tables(&t.sx);
        lnn_huff_code_table(t.code, t.len);
        HIPCHK(ctx, hipMemcpyAsync(d_tab, &t, sizeof(t), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_fail, 0, sizeof(uint32_t) * (uint64_t)n, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));         /* (t lives on this frame) */
    }
    ctx->sbatch_count[0]++;
    SbPlanner planner;
    sb_planner_init(&planner, samples.data(), n, S);
    SbPassPlan pp;
    uint32_t live = n;                                              /* tracks no block of which was refused so far */
    while (F && live && sb_next_pass(&planner, G, &pp)) {
        const uint32_t Fp = (uint32_t)pp.rows.size(), Tp = (uint32_t)pp.segs.size(), CF = Fp * C;
        ctx->sbatch_count[1]++;
        /* 0. the tables of the pass, in one copy */
        SbTrack *h_trk = (SbTrack *)h_tables.data();
        SbRow *h_rows = (SbRow *)(h_tables.data() + align_up(sizeof(SbTrack) * T));
        for (uint32_t k = 0; k < Tp; k++) {
            const SbPlanSeg &sg = pp.segs[k];
            const struct LINNEAmdTrack &tr = tracks[members[sg.track]];
            SbTrack &d = h_trk[k];
            const SbHost &th = host[members[sg.track]];
            d.pcm = tr.d_pcm; d.stride = th.cs; d.sstride = th.ss; d.fmt = th.fmt; d.pad = 0; d.total = samples[sg.track]; d.out = tr.d_out; d.pos = host[members[sg.track]].pos;
            d.slot0 = sg.slot0; d.nslots = sg.nslots; d.write = 0; d.id = sg.track;
        }
        for (uint32_t r = 0; r < Fp; r++) {
            const SbPlanRow &pr = pp.rows[r];
            h_rows[r].track = pr.seg; h_rows[r].slot = pr.slot; h_rows[r].first = pr.first;
            h_nsmp[r] = pr.nsmp; s_nsmp[pr.slot] = pr.nsmp;
        }
        HIPCHK(ctx, hipMemcpyAsync(sd + o_tables, h_tables.data(), align_up(sizeof(SbTrack) * T) + sizeof(SbRow) * Fp, hipMemcpyHostToDevice, ctx->stream));
        /* 1. gather */
        HIPCHK(ctx, hipMemsetAsync(d_nz, 0, sizeof(uint32_t) * Fp, ctx->stream));
        {
            SeGatherArgs g;
            g.frames = d_frames; g.nonzero = d_nz; g.F = Fp; g.C = C; g.S = S;
            SX_LAUNCH(NULL, LINNE_AMD_T_SB_GATHER, k_sb_gather, dim3(CF), dim3(SE_THREADS), 0, ctx->stream, g, (const SbRow *)d_rows, (const SbTrack *)d_trk);
        }
        /* 2. analysis, a call per slice of at most LNN_MAXCLS distinct lengths; the Rice plan of all rows */
        for (size_t k = 0; k + 1 < pp.slice.size(); k++) {
            const uint32_t r0 = pp.slice[k], cnt = pp.slice[k + 1] - r0;
            SX_TRY(LINNEAmd_EncodeFramesDevice(ctx, &shape, d_frames + CS * r0, h_nsmp.data() + r0, cnt, d_resid + CS * r0,
                    d_prm + (uint64_t)LINNE_AMD_PARAM_WORDS * C * r0, d_st + (uint64_t)LINNE_AMD_STAT_WORDS * C * r0));
            ctx->sbatch_count[2]++;
        }
        SX_TRY(LINNEAmd_RicePlanDevice(ctx, &shape, d_resid, h_nsmp.data(), Fp, d_plan));
        const uint32_t *d_nsmp = ctx->d_plan_nsmp;                 /* (RicePlanDevice's copy of this pass's lengths, by row) */
        SX_LAUNCH(NULL, LINNE_AMD_T_SE_COMPACT, k_se_compact, dim3((CF + SE_THREADS - 1u) / SE_THREADS), dim3(SE_THREADS), 0, ctx->stream, (const uint8_t *)d_plan, CF, d_cmp);
        /* 3. the host step: per track, in stream order, with the track's own state */
        HIPCHK(ctx, hipMemcpyAsync(h_cmp.data(), d_cmp, sizeof(uint2) * CF, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(h_st.data(), d_st, sizeof(double) * LINNE_AMD_STAT_WORDS * CF, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(h_nz.data(), d_nz, sizeof(uint32_t) * Fp, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        const size_t stw = (size_t)LINNE_AMD_STAT_WORDS * C;
        for (uint32_t r = 0; r < Fp; r++) {
            const uint32_t slot = pp.rows[r].slot;
            memcpy(&s_st[stw * slot], &h_st[stw * r], sizeof(double) * stw);
            s_nz[slot] = h_nz[r] ? 1u : 0u;
        }
        for (uint32_t k = 0; k < Tp; k++) {
            const SbPlanSeg &sg = pp.segs[k];
            SbHost &th = host[members[sg.track]];
            if (!th.live) { memset(&s_types[sg.slot0], LNN_BLOCK_SILENT, sg.nslots); continue; }       /* (an 11-byte block nobody writes) */
            if (lnn_decide_block_types(&shape, &s_nsmp[sg.slot0], sg.nslots, &s_st[stw * sg.slot0], &s_nz[sg.slot0], &s_types[sg.slot0], &th.state) != 0) { snprintf(ctx->err, sizeof(ctx->err), "block types: invalid shape"); return LNN_NG; }
        }
        uint32_t nsettle = 0;
        for (uint32_t r = 0; r < Fp; r++) {
            const uint8_t type = s_types[pp.rows[r].slot];
            h_types[r] = type;
            if (!host[members[pp.segs[pp.rows[r].seg].track]].live) continue;
            ctx->senc_count[type == LNN_BLOCK_COMPRESS ? 0 : (type == LNN_BLOCK_SILENT ? 1 : 2)]++;
            if (type != LNN_BLOCK_COMPRESS) continue;
            for (uint32_t ch = 0; ch < C; ch++) {
                const uint2 q = h_cmp[r * C + ch];
                const uint32_t order = q.x & 0xFFu, flag = (q.x >> 8) & 0xFFu;
                if (flag || order > 10u || (h_nsmp[r] % (1u << order)) != 0u) { h_settle[nsettle] = r * C + ch; h_settle_n[nsettle] = h_nsmp[r]; nsettle++; }
            }
        }
        ctx->senc_count[3] += nsettle;
        if (nsettle) {
            if (h_res.size() < (uint64_t)nsettle * S) { h_res.resize((uint64_t)nsettle * S); h_plans.resize((uint64_t)LINNE_AMD_RICE_PLAN_BYTES * nsettle); }
            for (uint32_t k = 0; k < nsettle; k++)
                HIPCHK(ctx, hipMemcpyAsync(h_res.data() + (uint64_t)k * S, d_resid + (uint64_t)h_settle[k] * S, sizeof(int32_t) * h_settle_n[k], hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            if (lnn_rice_plan_host(h_res.data(), S, h_settle_n.data(), nsettle, h_plans.data()) != 0) { snprintf(ctx->err, sizeof(ctx->err), "host Rice search failed"); return LNN_NG; }
            for (uint32_t k = 0; k < nsettle; k++) {
                const uint8_t *rec = h_plans.data() + (uint64_t)k * LINNE_AMD_RICE_PLAN_BYTES;
                HIPCHK(ctx, hipMemcpyAsync(d_plan + (uint64_t)h_settle[k] * LINNE_AMD_RICE_PLAN_BYTES, rec, LINNE_AMD_RICE_PLAN_K2 + (1u << rec[0]), hipMemcpyHostToDevice, ctx->stream));
            }
        }
        HIPCHK(ctx, hipMemcpyAsync(d_types, h_types.data(), Fp, hipMemcpyHostToDevice, ctx->stream));
        /* 4. sizes into slots, offsets over stream order, the tracks' totals and failures in one copy */
        SeBlockArgs a; memset(&a, 0, sizeof(a));
        a.types = d_types; a.nsmp = d_nsmp; a.prm = d_prm; a.plan = d_plan; a.resid = d_resid; a.tab = d_tab;
        a.F = Fp; a.C = C; a.S = S; a.bits = shape.bits_per_sample; a.L = hs.L;
        for (uint32_t l = 0; l < hs.L; l++) { a.P[l] = hs.P[l]; a.coef_off[l] = hs.coef_off[l]; }
        a.size = d_size; a.status = d_status; a.fail = d_fail; a.cfbit = d_cfbit; a.off = d_off; a.rows = d_rows; a.trk = d_trk;
        a.xch = (S + SE_THREADS - 1u) / SE_THREADS;
        SX_LAUNCH(NULL, LINNE_AMD_T_SB_SIZE, k_se_size, dim3((Fp + SE_THREADS - 1u) / SE_THREADS), dim3(SE_THREADS), 0, ctx->stream, a);
        SX_LAUNCH(NULL, LINNE_AMD_T_SE_SCAN, k_sx_scan, dim3(1), dim3(SX_SCAN_THREADS), 0, ctx->stream, (const uint32_t *)d_size, (uint64_t)Fp, d_off);
        SX_LAUNCH(NULL, LINNE_AMD_T_SB_REDUCE, k_sb_reduce, dim3(Tp), dim3(64), 0, ctx->stream, (const SbTrack *)d_trk, Tp, (const int32_t *)d_status, (const uint64_t *)d_off, d_tout);
        SX_TRY(sx_fetch(ctx, h_tout.data(), d_tout, sizeof(SbTrackOut) * Tp));
        /* the host decides per track: a refused block ends it; a track that no longer fits goes on being measured */
        uint64_t most = 0; bool any = false;
        for (uint32_t k = 0; k < Tp; k++) {
            const SbPlanSeg &sg = pp.segs[k];
            struct LINNEAmdTrack &tr = tracks[members[sg.track]];
            SbHost &th = host[members[sg.track]];
            h_trk2[k] = h_trk[k];
            if (!th.live) continue;
            const SbTrackOut &o = h_tout[k];
            if (o.fail != 0xFFFFFFFFu) {
                snprintf(th.text, sizeof(th.text), "block %llu: %s", (unsigned long long)(sg.frame0 + o.fail),
                        o.status == LNN_INVALID_FORMAT ? "a RAW block at a width other than 8, 16 or 24 bits" : "longer than the host stitcher's 64 + C * S * 8 bytes");
                live--; th.live = false; th.result = tr.capacity < LINNE_HEADER_SIZE ? LNN_INSUFFICIENT_BUFFER : o.status; tr.out_bytes = 0;
                continue;
            }
            if (th.writing && th.pos + o.bytes > th.room) th.writing = false;
            if (th.writing) { h_trk2[k].write = 1u; any = true; if (o.bytes > most) most = o.bytes; }
            th.pos += o.bytes;
        }
        /* 5. 6. the writers and the CRC, into the zeroed regions of the tracks that are written */
        if (any) {
            const uint64_t xz = (most + SB_ZERO_CHUNK - 1u) / SB_ZERO_CHUNK;
            if (xz * Tp > 0x7FFFFFFFull) { snprintf(ctx->err, sizeof(ctx->err), "EncodeStreamsDevice: a pass of %u tracks with up to %llu bytes each: give group_frames", Tp, (unsigned long long)most); return LNN_NG; }
            HIPCHK(ctx, hipMemcpyAsync(d_trk, h_trk2.data(), sizeof(SbTrack) * Tp, hipMemcpyHostToDevice, ctx->stream));
            SX_LAUNCH(NULL, LINNE_AMD_T_SB_ZERO, k_sb_zero, dim3((uint32_t)(xz * Tp)), dim3(SB_ZERO_THREADS), 0, ctx->stream, (const SbTrack *)d_trk, (const SbTrackOut *)d_tout, (uint32_t)xz);
            SX_LAUNCH(NULL, LINNE_AMD_T_SB_PARAMS, k_se_params, dim3((Fp + 63u) / 64u), dim3(64), 0, ctx->stream, a);
            if (S <= REMIT_LDS_SAMPLES) SX_LAUNCH(NULL, LINNE_AMD_T_SB_RICE, k_se_rice<true>, dim3(CF), dim3(REMIT_THREADS), sizeof(uint32_t) * (S + REMIT_THREADS + 1u), ctx->stream, a);
            else SX_LAUNCH(NULL, LINNE_AMD_T_SB_RICE, k_se_rice<false>, dim3(CF), dim3(REMIT_THREADS), 0, ctx->stream, a);
            SX_LAUNCH(NULL, LINNE_AMD_T_SB_RAW, k_se_raw, dim3(Fp * a.xch), dim3(SE_THREADS), 0, ctx->stream, a, (const int32_t *)d_frames);
            SX_LAUNCH(NULL, LINNE_AMD_T_SB_CRC, k_se_crc, dim3((Fp + 3u) / 4u), dim3(256), 0, ctx->stream, a);
        }
    }
    /* 7. the tracks' ends: does it fit, the length check of the Rice writers, the header */
    SX_TRY(sx_fetch(ctx, h_bad.data(), d_fail, sizeof(uint32_t) * (uint64_t)n));
    std::vector<uint8_t> h_hdr((sizeof(uint8_t *) + 32u) * (uint64_t)n);
    uint8_t **h_dst = (uint8_t **)h_hdr.data();
    uint32_t nh = 0;
    for (uint32_t k = 0; k < n; k++) {
        struct LINNEAmdTrack &tr = tracks[members[k]];
        SbHost &th = host[members[k]];
        if (!th.live) continue;
        tr.out_bytes = th.pos;
        if (!th.writing || th.pos > th.room) {
            snprintf(th.text, sizeof(th.text), "the stream takes %llu bytes, the buffer holds %llu", (unsigned long long)th.pos, (unsigned long long)tr.capacity);
            th.result = LNN_INSUFFICIENT_BUFFER; continue;
        }
        if (h_bad[k]) { snprintf(th.text, sizeof(th.text), "a Rice code's length is not its plan's (a wrapped 32-bit length count)"); th.result = LNN_NG; continue; }
        SX_TRY((int)LINNEEncoder_EncodeHeader(&tr.header, h_hdr.data() + sizeof(uint8_t *) * (uint64_t)n + 32u * (uint64_t)nh, LINNE_HEADER_SIZE));
        h_dst[nh++] = tr.d_out;
        th.result = LNN_OK;
    }
    if (nh) {
        /* (the bytes of entry i lie at n pointers + 32 * i, whatever nh is) */
        HIPCHK(ctx, hipMemcpyAsync(sd + o_hdr, h_hdr.data(), h_hdr.size(), hipMemcpyHostToDevice, ctx->stream));
        SX_LAUNCH(NULL, LINNE_AMD_T_SB_HEADER, k_sb_header, dim3((nh * 32u + 255u) / 256u), dim3(256), 0, ctx->stream, (uint8_t *const *)(sd + o_hdr), (const uint8_t *)(sd + o_hdr + sizeof(uint8_t *) * (uint64_t)n), nh);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));         /* (h_hdr lives on this frame) */
    }
    return LNN_OK;
}

static int sb_run(LINNEAmdContext *ctx, struct LINNEAmdTrack *tracks, const struct LINNEAmdPcmLayout *layouts, uint32_t num_tracks, uint32_t group_frames, std::vector<SbHost> &host)
{
    struct Group { struct LINNEAmdShape shape; std::vector<uint32_t> members; };
    std::vector<Group> groups;
    host.resize(num_tracks);
    uint64_t frames = 0;
    for (uint32_t i = 0; i < num_tracks; i++) {
        SbHost &h = host[i];
        memset(&h, 0, sizeof(h));
        h.result = sb_check_track(&tracks[i], layouts ? &layouts[i] : NULL, &h);
        if (h.result != LNN_OK) continue;
        h.live = true; h.pos = LINNE_HEADER_SIZE; h.state = tracks[i].parcor_state;
        h.room = tracks[i].capacity < 0xFFFFFFFFull ? tracks[i].capacity : 0xFFFFFFFFull;     /* EncodeWhole's buffer size is a uint32 */
        h.writing = tracks[i].capacity >= LINNE_HEADER_SIZE;
        frames += sb_frames(tracks[i].header.num_samples, h.shape.num_samples_per_block);
        size_t g = 0;
        while (g < groups.size() && memcmp(&groups[g].shape, &h.shape, sizeof(h.shape)) != 0) g++;
        if (g == groups.size()) { groups.emplace_back(); groups[g].shape = h.shape; }
        groups[g].members.push_back(i);
    }
    if (frames > 0x7FFFFFFFull) { snprintf(ctx->err, sizeof(ctx->err), "EncodeStreamsDevice: %llu frames in one call: too many", (unsigned long long)frames); return LNN_NG; }
    if (groups.empty()) return LNN_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    { const char *g = getenv("LINNE_AMD_RICE_GUARD"); ctx->rice_guard = g ? atof(g) : 0.0; }      /* test knob: wider guard band, more plans for the host */
    if (!ctx->outer_keep) ctx->nspans = 0;
    ctx->span_keep = 1;
    if (ctx->timing && !ctx->outer_keep) (void)hipEventRecord(ctx->ev[0], ctx->stream);
    int ret = LNN_OK;
    for (size_t g = 0; ret == LNN_OK && g < groups.size(); g++) ret = sb_group_run(ctx, tracks, host.data(), groups[g].members, groups[g].shape, group_frames);
    if (ret != LNN_OK && !ctx->err[0]) snprintf(ctx->err, sizeof(ctx->err), "EncodeStreamsDevice: a pass failed with %d", ret);
    return ret == LNN_OK ? LNN_OK : LNN_NG;
}

/* Both pairs of entry points behind their context check: the tracks' results, then the call's -- the lowest-numbered failing
 * track's code, with its text in ctx->err (behind the track's number unless the call is the single one) */
static int sb_call(LINNEAmdContext *ctx, struct LINNEAmdTrack *tracks, const struct LINNEAmdPcmLayout *layouts, uint32_t num_tracks, uint32_t group_frames, bool single)
{
    ctx->err[0] = 0;
    for (int i = 0; i < 4; i++) ctx->senc_count[i] = 0;
    for (int i = 0; i < 3; i++) ctx->sbatch_count[i] = 0;
    if (num_tracks == 0) return LNN_OK;
    if (!tracks) { snprintf(ctx->err, sizeof(ctx->err), "EncodeStreamsDevice: null argument"); return LNN_INVALID_ARGUMENT; }
    std::vector<SbHost> host;
    const int ret = items_try(ctx, [&] { return sb_run(ctx, tracks, layouts, num_tracks, group_frames, host); });
    const bool began = ctx->span_keep != 0;
    ctx->span_keep = 0; ctx->rice_guard = 0.0;
    if (items_end(ctx, single ? "EncodeStreamDevice" : "EncodeStreamsDevice", ret, began, began, NULL, num_tracks, [&](uint32_t i) { tracks[i].result = LNN_NG; }) != LNN_OK) return LNN_NG;
    int first = -1;
    for (uint32_t i = 0; i < num_tracks; i++) {
        tracks[i].result = host[i].result;
        if (host[i].result == LNN_OK) tracks[i].parcor_state = host[i].state;
        else if (first < 0) first = (int)i;
    }
    if (first < 0) return LNN_OK;
    items_first_text(ctx, "track", (uint32_t)first, single, host[first].text);
    return host[first].result;
}

/* int32 planar tracks: the call below without layouts */
extern "C" int LINNEAmd_EncodeStreamsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdTrack *tracks, uint32_t num_tracks, uint32_t group_frames)
{
    return LINNEAmd_EncodeStreamsDeviceLayout(ctx, tracks, NULL, num_tracks, group_frames);
}

extern "C" int LINNEAmd_EncodeStreamsDeviceLayout(struct LINNEAmdContext *ctx, struct LINNEAmdTrack *tracks, const struct LINNEAmdPcmLayout *layouts,
        uint32_t num_tracks, uint32_t group_frames)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    return sb_call(ctx, tracks, layouts, num_tracks, group_frames, false);
}

/* One track, int32 planar with pcm_stride (layout NULL) or as its layout says.  A NULL header or out_bytes leaves the track without
 * its d_pcm, which its check reports as the null argument it is; *out_bytes and *parcor_state are the track's, the state only on OK. */
static int se_single(struct LINNEAmdContext *ctx, const struct LINNEHeader *header, const void *d_pcm, uint64_t pcm_stride,
        const struct LINNEAmdPcmLayout *layout, uint32_t group_frames, uint8_t *d_out, uint64_t capacity, uint64_t *out_bytes, double *parcor_state)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    struct LINNEAmdTrack t;
    memset(&t, 0, sizeof(t));
    if (header && out_bytes) { t.header = *header; t.d_pcm = (const int32_t *)d_pcm; }
    if (out_bytes) t.out_bytes = *out_bytes;
    t.pcm_stride = pcm_stride; t.d_out = d_out; t.capacity = capacity; t.parcor_state = parcor_state ? *parcor_state : 0.0;
    const int ret = sb_call(ctx, &t, layout, 1, group_frames, true);
    if (out_bytes) *out_bytes = t.out_bytes;
    if (ret == LNN_OK && parcor_state) *parcor_state = t.parcor_state;
    return ret;
}
extern "C" int LINNEAmd_EncodeStreamDevice(struct LINNEAmdContext *ctx, const struct LINNEHeader *header,
        const int32_t *d_pcm, uint64_t pcm_stride, uint32_t group_frames,
        uint8_t *d_out, uint64_t capacity, uint64_t *out_bytes, double *parcor_state)
{
    return se_single(ctx, header, d_pcm, pcm_stride, NULL, group_frames, d_out, capacity, out_bytes, parcor_state);
}
extern "C" int LINNEAmd_EncodeStreamDeviceLayout(struct LINNEAmdContext *ctx, const struct LINNEHeader *header,
        const void *d_pcm, const struct LINNEAmdPcmLayout *layout, uint32_t group_frames,
        uint8_t *d_out, uint64_t capacity, uint64_t *out_bytes, double *parcor_state)
{
    return se_single(ctx, header, d_pcm, 0, layout, group_frames, d_out, capacity, out_bytes, parcor_state);
}


/* ================================================================================================
 * cutting and joining resident streams (lnn_splice.h, lnn_k_splice.h)
 * ============================================================================================== */
extern "C" int64_t LINNEAmd_GetLastSpliceCount(struct LINNEAmdContext *ctx, int which)
{
    if (!ctx || which < 0 || which > 5) return -1;
    return ctx->splice_count[which];
}

struct SpHost { char text[200]; };

/* LNN_OK: every output has its result in outs[] / host[]; anything else fails the whole call */
static int sp_run(LINNEAmdContext *ctx, struct LINNEAmdSplice *splices, uint32_t N, uint32_t group_frames, std::vector<SpOutput> &outs, std::vector<SpHost> &host)
{
    /* 1. the plan's inputs: the distinct indexes as streams, the cuts, the outputs */
    std::vector<SpStream> streams;
    std::vector<const LINNEAmdStreamIndex *> sx;
    std::vector<SpCut> cuts;
    std::vector<const uint8_t *> cut_bytes;
    outs.resize(N); host.resize(N);
    for (uint32_t k = 0; k < N; k++) {
        const struct LINNEAmdSplice &s = splices[k];
        SpOutput &o = outs[k];
        memset(&o, 0, sizeof(o)); host[k].text[0] = 0;
        o.cut0 = (uint32_t)cuts.size(); o.ncuts = 0; o.capacity = s.capacity;
        o.why0 = (!s.d_out || (!s.cuts && s.num_cuts)) ? SP_WHY_NULL : (((uintptr_t)s.d_out & 3u) ? SP_WHY_ALIGN : SP_WHY_NONE);
        if (o.why0 || !s.num_cuts) continue;
        if ((uint64_t)cuts.size() + s.num_cuts > 0x7FFFFFFFull) { snprintf(ctx->err, sizeof(ctx->err), "SpliceStreamsDevice: too many cuts in one call"); return LNN_NG; }
        o.ncuts = s.num_cuts;
        for (uint32_t i = 0; i < s.num_cuts; i++) {
            const struct LINNEAmdCut &c = s.cuts[i];
            SpCut pc; pc.stream = -1; pc.first = c.first_sample; pc.n = c.num_samples;
            if (c.index && c.d_stream) {
                if (c.index->device != ctx->device) o.why0 = SP_WHY_DEVICE;
                size_t j = sx.size();
                /* (the cuts of a call mostly name few streams, and neighbours the same one) */
                while (j > 0 && sx[j - 1] != c.index) j--;
                if (j == 0) {
                    const LINNEAmdStreamIndex *x = c.index;
                    SpStream st;
                    st.off = x->h_off; st.first = x->h_first; st.size = x->h_size; st.nsmp = x->h_nsmp; st.nb = x->nb; st.num_samples = x->header.num_samples;
                    st.channels = x->header.num_channels; st.bits = x->header.bits_per_sample; st.rate = x->header.sampling_rate;
                    st.block = x->header.num_samples_per_block; st.preset = x->header.preset; st.ms = (uint32_t)x->header.ch_process_method;
                    st.fail_block = x->fail_block; st.fail_code = x->fail_code;
                    sx.push_back(x); streams.push_back(st); j = sx.size();
                }
                pc.stream = (int32_t)(j - 1);
            }
            cuts.push_back(pc); cut_bytes.push_back(c.d_stream);
        }
    }
    std::vector<SpPiece> pieces;
    sp_plan(streams.data(), cuts.data(), outs.data(), N, pieces);
    auto refuse = [&](uint32_t k, int code, const char *text) {
        outs[k].result = code; outs[k].copied_blocks = outs[k].encoded_blocks = 0; outs[k].bytes = 0;
        snprintf(host[k].text, sizeof(host[k].text), "%s", text);
    };
    for (uint32_t k = 0; k < N; k++) {
        const SpOutput &o = outs[k];
        if (o.result == LNN_OK) continue;
        if (o.result == LNN_INVALID_ARGUMENT && o.why) snprintf(host[k].text, sizeof(host[k].text), "SpliceStreamsDevice: %s", sp_why_text(o.why));
        else {
            const LINNEAmdStreamIndex *x = sx[cuts[o.cut0 + o.fail_cut].stream];
            snprintf(host[k].text, sizeof(host[k].text), "cut %u: block %lld (byte %llu of the stream): %s", o.fail_cut, (long long)x->fail_block, (unsigned long long)x->fail_off,
                    x->fail_code == LNN_NG ? "a block no encoder writes" : "damaged or truncated stream");
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->nspans = 0; ctx->outer_keep = 1;
    if (ctx->timing) (void)hipEventRecord(ctx->ev[0], ctx->stream);
    /* 2. the fragments: decoded as windows into scratch, int32 planar, and encoded as tracks into scratch streams */
    std::vector<uint32_t> frag;                                 /* the fragment pieces of the live outputs */
    uint64_t runs_max = 0, live = 0;
    for (uint32_t k = 0; k < N; k++) if (outs[k].result == LNN_OK) { live++; runs_max += outs[k].npieces; }
    for (uint32_t i = 0; i < pieces.size(); i++) if (pieces[i].frag) frag.push_back(i);
    if (!live) return LNN_OK;
    const uint32_t nfrag = (uint32_t)frag.size();
    /* scratch: per fragment C * n samples and a stream of EncodeStreamBound's bytes, 16-byte aligned; then the run table and the headers */
    std::vector<uint64_t> o_pcm(nfrag), o_str(nfrag), room(nfrag);
    uint64_t at = 0;
    for (uint32_t f = 0; f < nfrag; f++) {
        const SpPiece &p = pieces[frag[f]];
        const SpStream &st = streams[cuts[outs[p.out].cut0 + p.cut].stream];
        o_pcm[f] = at; at = (at + sizeof(int32_t) * (uint64_t)st.channels * (p.b - p.a) + 15u) & ~(uint64_t)15u;
        room[f] = LINNE_HEADER_SIZE + 64u + (uint64_t)st.channels * st.block * 8u;
        o_str[f] = at; at = (at + room[f] + 15u) & ~(uint64_t)15u;
    }
    const uint64_t o_runs = at; at = align_up(at + sizeof(SpRun) * (runs_max + 1u));
    const uint64_t o_hptr = at; at = align_up(at + sizeof(uint8_t *) * live);
    const uint64_t o_hbytes = at; at = align_up(at + 32u * live);
    const uint64_t stage_bytes = at - o_runs;
    const LnnTally tally = { &ctx->splice_count[5], NULL, NULL };  /* the waits of its growing buffers are the call's own */
    SX_TRY(ensure_buf(ctx, &ctx->spl, &ctx->spl_cap, at, false, &tally));
    SX_TRY(ensure_buf(ctx, &ctx->spl_stage, &ctx->spl_stage_cap, stage_bytes, true, &tally));
    uint8_t *sd = (uint8_t *)ctx->spl, *hs_ = (uint8_t *)ctx->spl_stage;
    if (nfrag) {
        std::vector<struct LINNEAmdWindow> win(nfrag);
        for (uint32_t f = 0; f < nfrag; f++) {
            const SpPiece &p = pieces[frag[f]];
            const uint32_t ci = outs[p.out].cut0 + p.cut;
            win[f].index = sx[cuts[ci].stream]; win[f].d_stream = cut_bytes[ci]; win[f].first_sample = p.a; win[f].num_samples = p.b - p.a;
            win[f].d_pcm = (int32_t *)(sd + o_pcm[f]); win[f].pcm_stride = p.b - p.a; win[f].result = LNN_OK;
        }
        int ret = LINNEAmd_DecodeWindowsDevice(ctx, win.data(), nfrag, group_frames);
        if (ret != LNN_OK && strncmp(ctx->err, "window ", 7) != 0) return LNN_NG;         /* (a failing window's text starts with its number) */
        for (uint32_t f = 0; f < nfrag; f++) {
            const SpPiece &p = pieces[frag[f]];
            if (win[f].result != LNN_OK && outs[p.out].result == LNN_OK) {
                char text[sizeof(host[0].text)];
                snprintf(text, sizeof(text), "cut %u, samples [%llu, %llu): DecodeWindowsDevice -> %d (a block whose Rice codes do not end where its size field says)", p.cut,
                        (unsigned long long)p.a, (unsigned long long)p.b, win[f].result);
                refuse(p.out, win[f].result, text);
            }
        }
        std::vector<struct LINNEAmdTrack> trk;
        std::vector<uint32_t> trk_frag;
        for (uint32_t f = 0; f < nfrag; f++) {
            const SpPiece &p = pieces[frag[f]];
            if (outs[p.out].result != LNN_OK) continue;
            struct LINNEAmdTrack t; memset(&t, 0, sizeof(t));
            t.header = sx[cuts[outs[p.out].cut0 + p.cut].stream]->header; t.header.num_samples = (uint32_t)(p.b - p.a);
            t.d_pcm = (const int32_t *)(sd + o_pcm[f]); t.pcm_stride = p.b - p.a; t.d_out = sd + o_str[f]; t.capacity = room[f];
            t.parcor_state = 0.0;                               /* a fresh encoder (quirk Q2) */
            trk.push_back(t); trk_frag.push_back(f);
        }
        if (!trk.empty()) {
            ret = LINNEAmd_EncodeStreamsDevice(ctx, trk.data(), (uint32_t)trk.size(), group_frames);
            if (ret != LNN_OK && strncmp(ctx->err, "track ", 6) != 0) return LNN_NG;      /* (a failing track's text starts with its number) */
            for (size_t j = 0; j < trk.size(); j++) {
                SpPiece &p = pieces[frag[trk_frag[j]]];
                if (trk[j].result == LNN_OK) { p.bytes = trk[j].out_bytes - LINNE_HEADER_SIZE; continue; }
                if (outs[p.out].result != LNN_OK) continue;
                char text[sizeof(host[0].text)];
                snprintf(text, sizeof(text), "cut %u, samples [%llu, %llu): EncodeStreamDevice refuses the edge block with %d", p.cut, (unsigned long long)p.a, (unsigned long long)p.b, trk[j].result);
                refuse(p.out, trk[j].result, text);
            }
        }
        ctx->err[0] = 0;
    }
    /* 3. where everything lands, which outputs fit; then one copy launch and one header launch for those */
    sp_place(outs.data(), N, pieces.data());
    SpRun *h_runs = (SpRun *)hs_;
    uint8_t **h_hptr = (uint8_t **)(hs_ + (o_hptr - o_runs));
    uint8_t *h_hbytes = hs_ + (o_hbytes - o_runs);
    uint32_t nruns = 0, nh = 0; uint64_t nchunks = 0;
    std::vector<uint32_t> frag_of(pieces.size(), 0u);
    for (uint32_t f = 0; f < nfrag; f++) frag_of[frag[f]] = f;
    for (uint32_t k = 0; k < N; k++) {
        SpOutput &o = outs[k];
        if (o.result == LNN_INSUFFICIENT_BUFFER) {
            snprintf(host[k].text, sizeof(host[k].text), "the stream takes %llu bytes, the buffer holds %llu", (unsigned long long)o.bytes, (unsigned long long)o.capacity);
            o.copied_blocks = o.encoded_blocks = 0;
        }
        if (o.result != LNN_OK) continue;
        struct LINNEHeader h = sx[cuts[o.cut0].stream]->header;
        h.num_samples = (uint32_t)o.total_samples;
        SX_TRY((int)LINNEEncoder_EncodeHeader(&h, h_hbytes + 32u * (uint64_t)nh, LINNE_HEADER_SIZE));
        h_hptr[nh++] = splices[k].d_out;
        for (uint32_t i = 0; i < o.npieces; i++) {
            const SpPiece &p = pieces[o.piece0 + i];
            if (!p.bytes) continue;
            SpRun &r = h_runs[nruns++];
            r.src = p.frag ? sd + o_str[frag_of[o.piece0 + i]] + LINNE_HEADER_SIZE : cut_bytes[o.cut0 + p.cut] + p.a;
            r.dst = splices[k].d_out + p.dst; r.n = p.bytes; r.chunk0 = nchunks;
            nchunks += sp_run_chunks((uint64_t)(uintptr_t)r.dst, r.n);
            ctx->splice_count[4] += (int64_t)p.bytes;
        }
        ctx->splice_count[0]++; ctx->splice_count[1] += o.copied_blocks; ctx->splice_count[2] += o.encoded_blocks;
    }
    ctx->splice_count[3] = nruns;
    if (nh) {
        memset(&h_runs[nruns], 0, sizeof(SpRun)); h_runs[nruns].chunk0 = nchunks;
        HIPCHK(ctx, hipMemcpyAsync(sd + o_runs, hs_, stage_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (nruns) {
            const uint32_t grid = nchunks < SP_MAX_GRID ? (uint32_t)nchunks : SP_MAX_GRID;
            SX_LAUNCH(NULL, LINNE_AMD_SPLICE_T_COPY, k_sp_copy, dim3(grid), dim3(SP_THREADS), 0, ctx->stream, (const SpRun *)(sd + o_runs), nruns, nchunks);
        }
        SX_LAUNCH(NULL, LINNE_AMD_SPLICE_T_HEADER, k_sb_header, dim3((nh * 32u + 255u) / 256u), dim3(256), 0, ctx->stream, (uint8_t *const *)(sd + o_hptr), (const uint8_t *)(sd + o_hbytes), nh);
    }
    return LNN_OK;
}

extern "C" int LINNEAmd_SpliceStreamsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdSplice *splices, uint32_t num_splices, uint32_t group_frames)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->err[0] = 0;
    for (int i = 0; i < 6; i++) ctx->splice_count[i] = 0;
    if (num_splices == 0) return LNN_OK;
    if (!splices) { snprintf(ctx->err, sizeof(ctx->err), "SpliceStreamsDevice: null argument"); return LNN_INVALID_ARGUMENT; }
    std::vector<SpOutput> outs;
    std::vector<SpHost> host;
    const int ret = items_try(ctx, [&] { return sp_run(ctx, splices, num_splices, group_frames, outs, host); });
    const bool began = ctx->outer_keep != 0;
    ctx->outer_keep = 0; ctx->span_keep = 0;
    /* (the wait is the call's one wait of its own) */
    if (items_end(ctx, "SpliceStreamsDevice", ret, began, began, &ctx->splice_count[5], num_splices,
            [&](uint32_t i) { splices[i].result = LNN_NG; splices[i].out_bytes = 0; splices[i].copied_blocks = splices[i].encoded_blocks = 0; }) != LNN_OK) {
        for (int i = 0; i < 5; i++) ctx->splice_count[i] = 0;
        return LNN_NG;
    }
    int first = -1;
    for (uint32_t i = 0; i < num_splices; i++) {
        const SpOutput &o = outs[i];
        splices[i].result = o.result;
        splices[i].out_bytes = (o.result == LNN_OK || o.result == LNN_INSUFFICIENT_BUFFER) ? o.bytes : 0u;
        splices[i].copied_blocks = o.result == LNN_OK ? o.copied_blocks : 0u;
        splices[i].encoded_blocks = o.result == LNN_OK ? o.encoded_blocks : 0u;
        if (o.result != LNN_OK && first < 0) first = (int)i;
    }
    if (first < 0) return LNN_OK;
    items_first_text(ctx, "splice", (uint32_t)first, false, host[first].text);
    return outs[first].result;
}

/* test infrastructure (like lnn_forms_query: exported, not in include/): lnn_splice.h's plan on host tables, without a GPU.
 * streams: per stream 10 words { nb, num_samples, channels, bits, rate, block, preset, ms, fail_block (as int64), fail_code }, its
 * tables tab[s] = { off, first, size, nsmp } (size and nsmp widened to uint64).  cuts: per cut { stream (as int64, -1: NULL), first, n }.
 * outputs: per output { cut0, ncuts, capacity, why0 }.  frag_bytes: the size of every fragment's block, in the order the plan lists
 * the fragments (read up to nfrag_bytes of them; a missing one counts as 0).  out_rec: per output 8 words { result, why, bytes,
 * total samples, copied blocks, encoded blocks, piece0, npieces }; piece_rec: per piece 8 words { out, cut, frag, blocks, a, b, bytes,
 * dst }, up to piece_cap pieces.  Returns the number of pieces. */
extern "C" int64_t lnn_splice_plan(const uint64_t *stream_rec, const uint64_t *const *tabs, uint32_t nstreams, const uint64_t *cut_rec, uint32_t ncuts,
        const uint64_t *out_in, uint32_t nouts, const uint64_t *frag_bytes, uint32_t nfrag_bytes, uint64_t *out_rec, uint64_t *piece_rec, uint64_t piece_cap)
{
    try {
        std::vector<SpStream> streams(nstreams);
        std::vector<std::vector<uint32_t>> narrow(2 * (size_t)nstreams);
        for (uint32_t s = 0; s < nstreams; s++) {
            const uint64_t *r = stream_rec + 10u * (uint64_t)s;
            SpStream &st = streams[s];
            st.nb = (uint32_t)r[0]; st.num_samples = r[1]; st.channels = (uint32_t)r[2]; st.bits = (uint32_t)r[3]; st.rate = (uint32_t)r[4]; st.block = (uint32_t)r[5];
            st.preset = (uint32_t)r[6]; st.ms = (uint32_t)r[7]; st.fail_block = (int64_t)r[8]; st.fail_code = (int32_t)r[9];
            st.off = tabs[4u * s]; st.first = tabs[4u * s + 1u];
            for (int w = 0; w < 2; w++) { std::vector<uint32_t> &v = narrow[2u * s + w]; v.resize(st.nb); for (uint32_t i = 0; i < st.nb; i++) v[i] = (uint32_t)tabs[4u * s + 2u + w][i]; }
            st.size = narrow[2u * s].data(); st.nsmp = narrow[2u * s + 1u].data();
        }
        std::vector<SpCut> cuts(ncuts);
        for (uint32_t i = 0; i < ncuts; i++) { cuts[i].stream = (int32_t)(int64_t)cut_rec[3u * i]; cuts[i].first = cut_rec[3u * i + 1u]; cuts[i].n = cut_rec[3u * i + 2u]; }
        std::vector<SpOutput> outs(nouts);
        for (uint32_t k = 0; k < nouts; k++) { memset(&outs[k], 0, sizeof(SpOutput)); outs[k].cut0 = (uint32_t)out_in[4u * k]; outs[k].ncuts = (uint32_t)out_in[4u * k + 1u]; outs[k].capacity = out_in[4u * k + 2u]; outs[k].why0 = (int)out_in[4u * k + 3u]; }
        std::vector<SpPiece> pieces;
        sp_plan(streams.data(), cuts.data(), outs.data(), nouts, pieces);
        uint32_t f = 0;
        for (SpPiece &p : pieces) if (p.frag) { p.bytes = f < nfrag_bytes ? frag_bytes[f] : 0u; f++; }
        sp_place(outs.data(), nouts, pieces.data());
        for (uint32_t k = 0; k < nouts; k++) {
            const SpOutput &o = outs[k]; uint64_t *r = out_rec + 8u * (uint64_t)k;
            r[0] = (uint64_t)(int64_t)o.result; r[1] = (uint64_t)o.why; r[2] = o.bytes; r[3] = o.total_samples; r[4] = o.copied_blocks; r[5] = o.encoded_blocks; r[6] = o.piece0; r[7] = o.npieces;
        }
        for (size_t i = 0; i < pieces.size() && i < piece_cap; i++) {
            const SpPiece &p = pieces[i]; uint64_t *r = piece_rec + 8u * i;
            r[0] = p.out; r[1] = p.cut; r[2] = p.frag; r[3] = p.blocks; r[4] = p.a; r[5] = p.b; r[6] = p.bytes; r[7] = p.dst;
        }
        return (int64_t)pieces.size();
    } catch (const std::bad_alloc &) { return -1; }
}


/* ================================================================================================
 * repairing damaged resident streams (lnn_repair.h, lnn_k_repair.h)
 * ============================================================================================== */
extern "C" int64_t LINNEAmd_GetLastRepairCount(struct LINNEAmdContext *ctx, int which)
{
    if (!ctx || which < 0 || which > 6) return -1;
    return ctx->repair_count[which];
}

extern "C" int LINNEAmd_GetLastRepairGaps(struct LINNEAmdContext *ctx, uint32_t stream, const struct LINNEAmdGap **gaps, uint32_t *num_gaps)
{
    if (!ctx || !gaps || !num_gaps || stream >= ctx->rp_streams || !ctx->rp_gap0) return LNN_INVALID_ARGUMENT;
    *gaps = ctx->rp_gaps + ctx->rp_gap0[stream];
    *num_gaps = (uint32_t)(ctx->rp_gap0[stream + 1u] - ctx->rp_gap0[stream]);
    return LNN_OK;
}

struct RpHost { int32_t result; char text[200]; };

/* The block-head scan (IbScan), then the repair's own: sound candidates, their chains, the runs of kept blocks, the host's plan and
 * the copy launch (run table and fill bytes in spl / spl_stage).
 * LNN_OK: every stream has its result in host[] and, where that is OK or INSUFFICIENT_BUFFER, its plan; anything else fails the
 * whole call */
static int rp_run(LINNEAmdContext *ctx, struct LINNEAmdRepair *rep, uint32_t T, std::vector<RpHost> &host, std::vector<RpPlan> &plans)
{
    char text[sizeof(ctx->err)];
    host.resize(T); plans.resize(T);
    for (uint32_t i = 0; i < T; i++) { host[i].result = LNN_OK; host[i].text[0] = 0; plans[i].result = RP_OK; plans[i].bytes = 0; }
    /* 1. 2. the index's scan over the call's streams, through its host code and in its buffers (ib_scan_*).  Behind row0 its lists
     * carry the streams' block bounds and the tables, which go up with them; at their end the segment bounds of the sound candidates
     * and of the runs.  An opened stream's index is read for its shape and freed.  The call's waits and launches are counted
     * (LINNEAmd_GetLastRepairCount 5 and 6) */
    const LnnTally tally = { &ctx->repair_count[5], NULL, &ctx->repair_count[6] }, *tl = &tally;
    const uint64_t e_tab = align_up(sizeof(uint64_t) * (uint64_t)T), l_rseg = align_up(sizeof(uint64_t) * (T + 1ull));
    IbScan s;
    SX_TRY(ib_scan_lists(s, ctx, "RepairStreamsDevice", false, T, tally, e_tab + sizeof(SxTables), l_rseg + sizeof(uint64_t) * (T + 1ull)));
    uint8_t *hl = s.hl, *dl = s.dl;
    uint64_t *h_bound = (uint64_t *)(hl + s.at.o_early), *h_rseg = (uint64_t *)(hl + s.at.o_late + l_rseg);
    const uint64_t *d_bound = (const uint64_t *)(dl + s.at.o_early);
    uint64_t *d_sseg = (uint64_t *)(dl + s.at.o_late), *d_rseg = (uint64_t *)(dl + s.at.o_late + l_rseg);
    sx_tables((SxTables *)(hl + s.at.o_early + e_tab));
    SX_TRY(ib_scan_headers(s,
            [&](uint32_t i, uint64_t *N) -> const uint8_t * {
                h_bound[i] = 0;
                if (!rep[i].d_stream || !rep[i].d_out) { host[i].result = LNN_INVALID_ARGUMENT; snprintf(host[i].text, sizeof(host[i].text), "RepairStreamsDevice: null argument"); return NULL; }
                *N = rep[i].stream_bytes; return rep[i].d_stream;
            },
            [&](uint32_t i, int code, const char *why, LINNEAmdStreamIndex *x) {
                if (!x) { host[i].result = code; snprintf(host[i].text, sizeof(host[i].text), "%.*s", (int)sizeof(host[i].text) - 1, why); return; }
                uint32_t L = 0, P[LINNE_AMD_MAX_LAYERS] = { 0, 0, 0 }, sum = 0;
                (void)lnn_preset_info(x->shape.preset, &L, P, NULL, NULL);
                for (uint32_t l = 0; l < L; l++) sum += P[l];
                h_bound[i] = rp_block_bound(s.h_st[i].C, s.h_st[i].S, s.h_st[i].bits, L, sum);
                free(x);
            }));
    SX_TRY(ib_scan_candidates(s));
    const uint32_t K = s.K, M32 = s.M32, gT = s.gT, gM = s.gM;
    const uint64_t M = s.M;
    const IbStream *h_st = s.h_st, *d_st = s.d_st;
    const uint64_t *d_crow = s.d_crow, *d_seg = s.d_seg;
    /* 3. the sound candidates, their successors, pointer doubling, the chains' lengths.  No more sound candidates than candidates
     * and no more chain blocks than sound candidates: every table below has room for M of them, so nothing waits for a count */
    uint64_t at = 0;
    auto part = [&](uint64_t bytes) { const uint64_t o = at; at = align_up(at + bytes); return o; };
    const uint64_t o_cand = part(sizeof(uint64_t) * (M + 1u)), o_flag = part(sizeof(uint32_t) * (M + 1u)), o_sofs = part(sizeof(uint64_t) * (M + 2u)),
            o_spos = part(sizeof(uint64_t) * (M + 1u)), o_jump = part(sizeof(uint32_t) * (uint64_t)K * (M + 1u)), o_off = part(sizeof(uint64_t) * (M + 1u)),
            o_size = part(sizeof(uint32_t) * (M + 1u)), o_type = part(sizeof(uint32_t) * (M + 1u)), o_nsmp = part(sizeof(uint32_t) * (M + 1u)),
            o_scan = part(sizeof(uint64_t) * (M + 2u)), o_mark = part(sizeof(uint32_t) * (M + 1u)), o_rofs = part(sizeof(uint64_t) * (M + 2u)),
            o_rec = part(sizeof(RpRunRec) * (M + 1u));
    SX_TRY(ensure_buf(ctx, &ctx->xcand, &ctx->xcand_cap, at, false, tl));
    uint8_t *xc = (uint8_t *)ctx->xcand;
    uint64_t *cand = (uint64_t *)(xc + o_cand), *sofs = (uint64_t *)(xc + o_sofs), *spos = (uint64_t *)(xc + o_spos), *c_off = (uint64_t *)(xc + o_off),
            *scan = (uint64_t *)(xc + o_scan), *rofs = (uint64_t *)(xc + o_rofs);
    uint32_t *flag = (uint32_t *)(xc + o_flag), *jump = (uint32_t *)(xc + o_jump), *c_size = (uint32_t *)(xc + o_size), *c_type = (uint32_t *)(xc + o_type),
            *c_nsmp = (uint32_t *)(xc + o_nsmp), *mark = (uint32_t *)(xc + o_mark);
    RpRunRec *rec = (RpRunRec *)(xc + o_rec);
    for (uint32_t i = 0; i <= T; i++) s.h_crow[i] = 0;
    if (M) {
        SX_TRY(ib_scan_write(s, cand));
        RpSoundArgs sa;
        sa.st = d_st; sa.bound = d_bound; sa.seg = s.d_seg; sa.T = T; sa.M = M32; sa.cand = cand; sa.tab = (const SxTables *)(dl + s.at.o_early + e_tab); sa.flag = flag;
        SX_LAUNCH(tl, LINNE_AMD_REPAIR_T_SOUND, k_rp_sound, dim3((uint32_t)((M + 3u) / 4u)), dim3(256), 0, ctx->stream, sa);
        SX_LAUNCH(tl, LINNE_AMD_T_SX_SCAN, k_sx_scan, dim3(1), dim3(SX_SCAN_THREADS), 0, ctx->stream, (const uint32_t *)flag, M, sofs);
        SX_LAUNCH(tl, LINNE_AMD_REPAIR_T_COMPACT, k_rp_compact, dim3(gM), dim3(256), 0, ctx->stream, (const uint32_t *)flag, (const uint64_t *)sofs, (const uint64_t *)cand, M32, spos);
        SX_LAUNCH(tl, LINNE_AMD_T_SX_SCAN, k_ib_seg, dim3(gT), dim3(256), 0, ctx->stream, (const uint64_t *)sofs, d_seg, T, d_sseg);
        SX_LAUNCH(tl, LINNE_AMD_REPAIR_T_SUCC, k_rp_succ, dim3(gM), dim3(256), 0, ctx->stream, d_st, (const uint64_t *)d_sseg, T, (const uint64_t *)spos, M32, jump);
        SX_TRY(ib_scan_jumps(s, jump));
        SX_LAUNCH(tl, LINNE_AMD_REPAIR_T_CHAIN_LEN, k_rp_chain_len, dim3(gT), dim3(256), 0, ctx->stream, (const uint64_t *)d_sseg, T, (const uint32_t *)jump, K, M32, s.d_len);
        SX_TRY(ib_scan_chains(s));
        if (s.nchain > M) { snprintf(ctx->err, sizeof(ctx->err), "internal: %llu chain blocks of %llu candidates", (unsigned long long)s.nchain, (unsigned long long)M); return LNN_NG; }
    }
    const uint64_t nchain = s.nchain;
    /* 4. the chains' blocks, the cut at the headers' sample counts, a record per run of adjacent kept blocks: one fetch */
    std::vector<std::vector<RpPiece>> pieces(T);
    if (nchain) {
        SX_TRY(ensure_buf(ctx, &ctx->spl_stage, &ctx->spl_stage_cap, sizeof(RpRunRec) * nchain, true, tl));
        HIPCHK(ctx, hipMemcpyAsync(dl + s.at.o_crow, hl + s.at.o_crow, sizeof(uint64_t) * (T + 1ull), hipMemcpyHostToDevice, ctx->stream));
        SX_LAUNCH(tl, LINNE_AMD_T_SX_CHAIN, k_ib_chain, dim3((uint32_t)((nchain + 255u) / 256u)), dim3(256), 0, ctx->stream, d_st, (const uint64_t *)d_sseg, d_crow, T, (const uint64_t *)spos,
                (const uint32_t *)jump, K, M32, nchain, c_off, c_size, c_type, c_nsmp);
        SX_LAUNCH(tl, LINNE_AMD_T_SX_SCAN, k_sx_scan, dim3(1), dim3(SX_SCAN_THREADS), 0, ctx->stream, (const uint32_t *)c_nsmp, nchain, scan);
        RpRunArgs ra;
        ra.st = d_st; ra.crow = d_crow; ra.T = T; ra.nchain = nchain; ra.off = c_off; ra.size = c_size; ra.scan = scan; ra.mark = mark; ra.rofs = rofs; ra.rec = rec;
        const uint32_t gc = (uint32_t)((nchain + 255u) / 256u);
        SX_LAUNCH(tl, LINNE_AMD_REPAIR_T_MARK, k_rp_mark, dim3(gc), dim3(256), 0, ctx->stream, ra);
        SX_LAUNCH(tl, LINNE_AMD_T_SX_SCAN, k_sx_scan, dim3(1), dim3(SX_SCAN_THREADS), 0, ctx->stream, (const uint32_t *)mark, nchain, rofs);
        SX_LAUNCH(tl, LINNE_AMD_REPAIR_T_RUNS, k_rp_runs, dim3(gc), dim3(256), 0, ctx->stream, ra);
        SX_LAUNCH(tl, LINNE_AMD_T_SX_SCAN, k_ib_seg, dim3(gT), dim3(256), 0, ctx->stream, (const uint64_t *)rofs, d_crow, T, d_rseg);
        HIPCHK(ctx, hipMemcpyAsync(h_rseg, d_rseg, sizeof(uint64_t) * (T + 1ull), hipMemcpyDeviceToHost, ctx->stream));
        /* (no more runs than chain blocks: the records of all of them come back without waiting for their count) */
        HIPCHK(ctx, hipMemcpyAsync(ctx->spl_stage, rec, sizeof(RpRunRec) * nchain, hipMemcpyDeviceToHost, ctx->stream));
        SX_TRY(tally_wait(ctx, tl));
        const RpRunRec *h_rec = (const RpRunRec *)ctx->spl_stage;
        if (h_rseg[T] > nchain) { snprintf(ctx->err, sizeof(ctx->err), "internal: %llu runs of %llu chain blocks", (unsigned long long)h_rseg[T], (unsigned long long)nchain); return LNN_NG; }
        for (uint32_t i = 0; i < T; i++)
            for (uint64_t j = h_rseg[i]; j < h_rseg[i + 1]; j++) {
                const RpRunRec &r = h_rec[j];
                const RpPiece q = { r.off0, r.off1 - r.off0, r.smp1 - r.smp0, (uint64_t)(r.rank1 - r.rank0) };
                pieces[i].push_back(q);
            }
    }
    /* 5. the host's plan; one upload of the run table and the fill bytes; one copy launch */
    lnn_tables_init();                                              /* (lnn_crc16's table) */
    uint64_t nruns = 0, fill_bytes = 0;
    for (uint32_t i = 0; i < T; i++) {
        if (host[i].result != LNN_OK) continue;
        RpPlan &p = plans[i];
        rp_plan(pieces[i].data(), pieces[i].size(), h_st[i].num_samples, h_st[i].S, rep[i].stream_bytes, rep[i].capacity, lnn_crc16, p);
        host[i].result = p.result;
        if (p.result != RP_OK) { snprintf(host[i].text, sizeof(host[i].text), "the stream takes %llu bytes, the buffer holds %llu", (unsigned long long)p.bytes, (unsigned long long)rep[i].capacity); continue; }
        nruns += p.runs.size(); fill_bytes += p.fill.size();
    }
    if (nruns >= 0xFFFFFFFFull) { snprintf(ctx->err, sizeof(ctx->err), "RepairStreamsDevice: too many runs in one call"); return LNN_NG; }
    if (nruns) {
        const uint64_t o_fill = align_up(sizeof(SpRun) * (nruns + 1u)), stage_bytes = align_up(o_fill + fill_bytes);
        SX_TRY(ensure_buf(ctx, &ctx->spl, &ctx->spl_cap, stage_bytes, false, tl));
        SX_TRY(ensure_buf(ctx, &ctx->spl_stage, &ctx->spl_stage_cap, stage_bytes, true, tl));
        uint8_t *sd = (uint8_t *)ctx->spl, *hs_ = (uint8_t *)ctx->spl_stage;
        SpRun *h_runs = (SpRun *)hs_;
        uint64_t r = 0, f = o_fill, nchunks = 0;
        for (uint32_t i = 0; i < T; i++) {
            if (host[i].result != LNN_OK) continue;
            const RpPlan &p = plans[i];
            if (!p.fill.empty()) memcpy(hs_ + f, p.fill.data(), p.fill.size());
            for (const RpRun &q : p.runs) {
                SpRun &o = h_runs[r++];
                o.src = q.fill ? sd + f + q.src : rep[i].d_stream + q.src; o.dst = rep[i].d_out + q.dst; o.n = q.bytes; o.chunk0 = nchunks;
                nchunks += sp_run_chunks((uint64_t)(uintptr_t)o.dst, o.n);
            }
            f += p.fill.size();
        }
        memset(&h_runs[nruns], 0, sizeof(SpRun)); h_runs[nruns].chunk0 = nchunks;
        HIPCHK(ctx, hipMemcpyAsync(sd, hs_, stage_bytes, hipMemcpyHostToDevice, ctx->stream));
        const uint32_t grid = nchunks < SP_MAX_GRID ? (uint32_t)nchunks : SP_MAX_GRID;
        SX_LAUNCH(tl, LINNE_AMD_SPLICE_T_COPY, k_sp_copy, dim3(grid), dim3(SP_THREADS), 0, ctx->stream, (const SpRun *)sd, (uint32_t)nruns, nchunks);
    }
    ctx->repair_count[4] = (int64_t)nruns;
    /* room for the gaps LINNEAmd_GetLastRepairGaps hands out (filled behind the call's last wait) */
    uint64_t ngaps = 0;
    for (uint32_t i = 0; i < T; i++) if (host[i].result == LNN_OK) ngaps += plans[i].gaps.size();
    ctx->rp_gaps = (struct LINNEAmdGap *)malloc(sizeof(struct LINNEAmdGap) * (ngaps + 1u));
    ctx->rp_gap0 = (uint64_t *)malloc(sizeof(uint64_t) * ((uint64_t)T + 1u));
    if (!ctx->rp_gaps || !ctx->rp_gap0) { free(ctx->rp_gaps); free(ctx->rp_gap0); ctx->rp_gaps = NULL; ctx->rp_gap0 = NULL; snprintf(ctx->err, sizeof(ctx->err), "out of host memory"); return LNN_NG; }
    return LNN_OK;
}

extern "C" int LINNEAmd_RepairStreamsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdRepair *streams, uint32_t num_streams)
{
    if (!ctx) return LNN_INVALID_ARGUMENT;
    ctx->err[0] = 0;
    for (int i = 0; i < 7; i++) ctx->repair_count[i] = 0;
    free(ctx->rp_gaps); free(ctx->rp_gap0); ctx->rp_gaps = NULL; ctx->rp_gap0 = NULL; ctx->rp_streams = 0;
    if (num_streams == 0) return LNN_OK;
    if (!streams) { snprintf(ctx->err, sizeof(ctx->err), "RepairStreamsDevice: null argument"); return LNN_INVALID_ARGUMENT; }
    std::vector<RpHost> host;
    std::vector<RpPlan> plans;
    const int ret = items_try(ctx, [&] { return rp_run(ctx, streams, num_streams, host, plans); });
    /* (the wait is the call's last) */
    if (items_end(ctx, "RepairStreamsDevice", ret, ret == LNN_OK, true, &ctx->repair_count[5], num_streams, [&](uint32_t i) {
                streams[i].result = LNN_NG; streams[i].out_bytes = streams[i].lost_samples = 0;
                streams[i].kept_blocks = streams[i].fill_blocks = streams[i].num_gaps = streams[i].exact = 0;
            }) != LNN_OK) {
        for (int i = 0; i < 5; i++) ctx->repair_count[i] = 0;
        return LNN_NG;
    }
    int first = -1;
    uint64_t g = 0;
    for (uint32_t i = 0; i < num_streams; i++) {
        struct LINNEAmdRepair &s = streams[i];
        const RpPlan &p = plans[i];
        const bool ok = host[i].result == LNN_OK;
        ctx->rp_gap0[i] = g;
        s.result = host[i].result;
        s.out_bytes = (ok || host[i].result == LNN_INSUFFICIENT_BUFFER) ? p.bytes : 0u;
        s.lost_samples = ok ? p.lost_samples : 0u;
        s.kept_blocks = ok ? (uint32_t)p.kept_blocks : 0u; s.fill_blocks = ok ? (uint32_t)p.fill_blocks : 0u;
        s.num_gaps = ok ? (uint32_t)p.gaps.size() : 0u; s.exact = ok ? p.exact : 0u;
        if (!ok) { if (first < 0) first = (int)i; continue; }
        for (const RpGap &q : p.gaps) {
            struct LINNEAmdGap &o = ctx->rp_gaps[g++];
            o.first_sample = q.first_sample; o.num_samples = q.num_samples; o.src_offset = q.src_off; o.src_bytes = q.src_bytes; o.fill_blocks = (uint32_t)q.fill_blocks; o.reserved = 0;
        }
        ctx->repair_count[0]++; ctx->repair_count[1] += (int64_t)p.kept_blocks; ctx->repair_count[2] += (int64_t)p.fill_blocks; ctx->repair_count[3] += (int64_t)p.gaps.size();
    }
    ctx->rp_gap0[num_streams] = g; ctx->rp_streams = num_streams;
    if (first < 0) return LNN_OK;
    items_first_text(ctx, "repair", (uint32_t)first, false, host[first].text);
    return host[first].result;
}

/* test infrastructure (like lnn_splice_plan: exported, not in include/): lnn_repair.h's plan on host tables, without a GPU.
 * in: { N, S, stream_bytes, capacity }; blocks: per kept block { offset, size field, samples }.  out_rec: 9 words { result, bytes,
 * kept blocks, fill blocks, gaps, lost samples, exact, runs, fill bytes }; gap_rec: per gap 6 words { first sample, samples, source
 * offset, source bytes, fill blocks, offset in the fill bytes }; run_rec: per run 4 words { fill, src, dst, bytes }; fill: the fill
 * bytes.  Nothing is written beyond the capacities given.  Returns 0, -1 on a bad argument or without memory. */
extern "C" int64_t lnn_repair_plan(const uint64_t *in, const uint64_t *blocks, uint64_t nblocks, uint64_t *out_rec, uint64_t *gap_rec, uint64_t gap_cap,
        uint64_t *run_rec, uint64_t run_cap, uint8_t *fill, uint64_t fill_cap)
{
    if (!in || !out_rec || in[1] == 0u || (nblocks && !blocks)) return -1;
    try {
        lnn_tables_init();                                          /* (lnn_crc16's table) */
        std::vector<RpPiece> pieces(nblocks);
        for (uint64_t i = 0; i < nblocks; i++) { const RpPiece q = { blocks[3u * i], blocks[3u * i + 1u] + 6u, blocks[3u * i + 2u], 1u }; pieces[i] = q; }
        RpPlan p;
        rp_plan(pieces.data(), nblocks, in[0], in[1], in[2], in[3], lnn_crc16, p);
        out_rec[0] = (uint64_t)(int64_t)p.result; out_rec[1] = p.bytes; out_rec[2] = p.kept_blocks; out_rec[3] = p.fill_blocks; out_rec[4] = p.gaps.size();
        out_rec[5] = p.lost_samples; out_rec[6] = p.exact; out_rec[7] = p.runs.size(); out_rec[8] = p.fill.size();
        for (size_t i = 0; i < p.gaps.size() && i < gap_cap && gap_rec; i++) {
            const RpGap &g = p.gaps[i]; uint64_t *r = gap_rec + 6u * i;
            r[0] = g.first_sample; r[1] = g.num_samples; r[2] = g.src_off; r[3] = g.src_bytes; r[4] = g.fill_blocks; r[5] = g.fill_at;
        }
        for (size_t i = 0; i < p.runs.size() && i < run_cap && run_rec; i++) {
            const RpRun &q = p.runs[i]; uint64_t *r = run_rec + 4u * i;
            r[0] = q.fill; r[1] = q.src; r[2] = q.dst; r[3] = q.bytes;
        }
        if (fill) for (size_t i = 0; i < p.fill.size() && i < fill_cap; i++) fill[i] = p.fill[i];
        return 0;
    } catch (const std::bad_alloc &) { return -1; }
}


/* ------------------------------------------------------------------------------------------------
 * test infrastructure (like lnn_preset_info: exported, not in include/): what the rules of lnn_forms.h say for a call, without a GPU
 * ---------------------------------------------------------------------------------------------- */
#define LNN_Q_HEADER 48         /* words of the call record */
#define LNN_Q_CHUNK 16          /* words of a chunk record; LNN_Q_LAYER words per layer follow it */
#define LNN_Q_LAYER 24
/* mode 0: an encode call -- class bookkeeping, split and the forms of every chunk, as a fresh context would decide them with the
 * knobs of the environment.  ctx_streams: the compute sub-streams of the context (-1: what LINNE_AMD_STREAMS makes it create);
 * arena_bytes 0: the default arena.  out: the call record (layout: tests/test_forms_cpu.py CALL_FIELDS), then per chunk a chunk
 * record and hs.L layer records (CHUNK_FIELDS, LAYER_FIELDS); with -a N a second such group per chunk, the final pass's.
 * mode 1: a decode call of num_frames frames (data_aligned: the samples lie 16-byte aligned): out = call form, ms_separate, then per
 * layer form, nch, pb, de, ms_fold.  Returns the words written, -1 on a bad argument or too small a buffer. */
extern "C" int64_t lnn_forms_query(int mode, const struct LINNEAmdShape *shape, const uint32_t *num_samples, uint32_t num_frames,
        uint64_t arena_bytes, int ctx_streams, int has_side, uint32_t af_iters, uint32_t learning, int data_aligned, int64_t *out, uint64_t cap)
{
    HostShape hs;
    if (!out || num_frames == 0 || shape_info(shape, &hs) != LNN_OK) return -1;
    LnnKnobs knob; memset(&knob, 0, sizeof(knob));
    lnn_knobs_read_context(&knob); lnn_knobs_read_call(&knob);
    const uint32_t C = shape->num_channels, S = shape->num_samples_per_block;
    uint64_t n = 0;
    uint32_t *meta = NULL; LnnClassTable *tab = NULL;
#define PUT(v) do { if (n >= cap) { free(meta); free(tab); return -1; } out[n++] = (int64_t)(v); } while (0)
    if (mode == 1) {
        LnnDecodeForms df;
        lnn_decode_forms(&hs, C, S, shape->ch_process_method, num_frames, data_aligned != 0, SP_LDS_BYTES(S) <= LEV_LDS_BUDGET, &knob, &df);
        PUT(df.call); PUT(df.ms_separate);
        for (uint32_t l = 0; l < hs.L; l++) { const LnnDecLayer &d = df.layer[l]; PUT(d.form); PUT(d.nch); PUT(d.pb); PUT(d.de); PUT(d.ms_fold); }
        return (int64_t)n;
    }
    int forced = 0;
    if (ctx_streams < 0) ctx_streams = lnn_context_streams(&forced);
    meta = (uint32_t *)malloc(sizeof(uint32_t) * 3 * (size_t)num_frames);
    tab = (LnnClassTable *)calloc(1, sizeof(LnnClassTable));
    LnnCallClasses cc;
    if (!meta || !tab || lnn_call_classes(tab, shape, &hs, &knob, num_samples, num_frames, meta, meta + num_frames, meta + 2 * (size_t)num_frames, &cc) != LNN_CLS_OK) { free(meta); free(tab); return -1; }
    const uint64_t per_frame = frame_scratch_bytes(shape, &hs, af_iters, learning);
    if (arena_bytes == 0) arena_bytes = 6ull << 30;
    if (arena_bytes < per_frame * 4 + 65536) arena_bytes = per_frame * 4 + 65536;
    const LnnSplit sp = lnn_call_split(arena_bytes, per_frame, num_frames, C, hs.R, ctx_streams, forced != 0, &knob);
    PUT(cc.branch); PUT(cc.nlen); PUT(cc.na_max); PUT(cc.prod_ok); PUT(sp.nsub); PUT(sp.use_sub); PUT(sp.chunk); PUT(sp.part_bytes);
    PUT((num_frames + sp.chunk - 1) / sp.chunk); PUT(lnn_stats_rows_form(&knob, num_frames, C, S, hs.P[0])); PUT(per_frame); PUT(hs.L);
    PUT(sp.streams_forced); PUT(0); PUT(0); PUT(0);
    for (uint32_t i = 0; i < LNN_MAXCLS; i++) PUT(i < cc.nlen ? cc.lens[i] : 0);
    for (uint32_t i = 0; i < LNN_MAXCLS; i++) PUT(i < cc.nlen ? cc.slot_of[i] : 0);
    for (uint32_t f0 = 0; f0 < num_frames; f0 += (uint32_t)sp.chunk) {
        const uint32_t Fc = (num_frames - f0 < sp.chunk) ? (num_frames - f0) : (uint32_t)sp.chunk;
        for (int fin = 0; fin < (af_iters ? 2 : 1); fin++) {
            const LnnChunkIn in = { &hs, C, S, Fc, tab->cls, meta + f0, &knob, sp.use_sub, has_side != 0, af_iters, learning, fin != 0 };
            LnnChunkForms cf;
            lnn_chunk_forms(&in, &cf);
            RowRuns rr; lnn_build_runs(&rr, meta + f0, Fc, C * hs.R);
            PUT(f0); PUT(Fc); PUT((uint64_t)Fc * C * (fin ? 1u : hs.R)); PUT(fin); PUT(cf.fwd_loss_on); PUT(cf.fuse_cfg); PUT(cf.fuse_all); PUT(cf.last_layer_all);
            PUT(cf.prep_defer); PUT(cf.hist); PUT(cf.chain_sum); PUT(cf.chain_sum_wave); PUT(cf.cascade_walk); PUT(rr.mixed); PUT(rr.n); PUT(cf.present);
            for (uint32_t l = 0; l < hs.L; l++) {
                const LnnLayerForms &lf = cf.layer[l];
                uint32_t nleft = 0, left_first = 0, left_frames = 0;
                if (lf.long_any && !lf.long_all && !lf.fir_small)
                    for (uint32_t f = 0, g = 0; lnn_next_left_run(&lf, meta + f0, Fc, g, &f, &g); nleft++) { if (!nleft) left_first = f; left_frames += g - f; }
                PUT(lf.fir_spec); PUT(lf.hist_layer); PUT(lf.hist_all); PUT(lf.beside); PUT(lf.lev_wave); PUT(lf.nlev); PUT(lf.nlev ? lf.lev[0].ride : 0); PUT(lf.last_layer);
                PUT(lf.long_any); PUT(lf.long_all); PUT(lf.search_form); PUT(lf.fir_small); PUT(lf.sel_wave); PUT(lf.fwd_loss); PUT(lf.fwd_loss_mw); PUT(lf.forward);
                PUT(lf.forward_walk); PUT(nleft); PUT(left_first); PUT(left_frames); PUT(lf.long_mask); PUT(lf.lev_beside); PUT(lf.lev_carrier); PUT(lf.lev_carrier < lf.nlev ? lf.lev[lf.lev_carrier].ride : LNN_MAXT);
            }
        }
    }
    free(meta); free(tab);
    return (int64_t)n;
#undef PUT
}

/* the class bookkeeping of a LIST of encode calls on one context: call i has shape shapes[i] and the counts[i] next lengths of
 * `lengths`.  out: per call 2 + LNN_MAXCLS words -- the branch taken (LNN_CLS_*), the resident classes after it, their lengths in
 * slot order.  Returns the words written, -1 on a bad argument or a call the encoder would refuse. */
extern "C" int64_t lnn_classes_replay(const struct LINNEAmdShape *shapes, const uint32_t *lengths, const uint32_t *counts, uint32_t num_calls, int64_t *out, uint64_t cap)
{
    if (!shapes || !lengths || !counts || !out || cap < (uint64_t)num_calls * (2 + LNN_MAXCLS)) return -1;
    LnnKnobs knob; memset(&knob, 0, sizeof(knob));
    lnn_knobs_read_context(&knob); lnn_knobs_read_call(&knob);
    LnnClassTable *tab = (LnnClassTable *)calloc(1, sizeof(LnnClassTable));
    if (!tab) return -1;
    uint64_t n = 0;
    for (uint32_t i = 0; i < num_calls; i++) {
        HostShape hs; LnnCallClasses cc;
        uint32_t *meta = (uint32_t *)malloc(sizeof(uint32_t) * 3 * (size_t)(counts[i] ? counts[i] : 1));
        const bool ok = meta && shape_info(&shapes[i], &hs) == LNN_OK
                && lnn_call_classes(tab, &shapes[i], &hs, &knob, lengths, counts[i], meta, meta + counts[i], meta + 2 * (size_t)counts[i], &cc) == LNN_CLS_OK;
        free(meta);
        if (!ok) { free(tab); return -1; }
        out[n++] = cc.branch; out[n++] = tab->ncls;
        for (uint32_t s = 0; s < LNN_MAXCLS; s++) out[n++] = s < tab->ncls ? tab->cls[s].n : 0;
        lengths += counts[i];
    }
    free(tab);
    return (int64_t)n;
}
