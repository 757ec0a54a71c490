/*
 * linne_amd.h -- C-ABI of the MI355X (gfx950) per-frame prediction path, batch form.
 *
 * The reference has no FFI for this path: its caller reaches it through LINNEEncoder_EncodeBlock /
 * LINNEDecoder_DecodeBlock (include/linne_encoder.h:49-54, include/linne_decoder.h:38-43), one block per
 * call.  liblinne_amd.so keeps those 13 public symbols (include/linne_encoder.h, include/linne_decoder.h
 * in this directory) and adds the entry points below, which are what those functions call internally and
 * what a maintainer would bind to feed many frames at once.  Plain pointers and sizes
 * only; no torch types.  Every function returns a LINNEApiResult value (0 = OK) unless noted.
 *
 * Units: a "frame" is one LINNE block (num_samples_per_block samples per channel); a "channel-frame" is
 * one channel of one frame -- the independent unit of work.
 *
 * Data layout (all device buffers are SoA, frame-major, planar):
 *   pcm / residual : int32_t [num_frames][num_channels][stride]        stride = num_samples_per_block
 *   params         : int32_t [num_frames][num_channels][LINNE_AMD_PARAM_WORDS]
 *   stats          : double  [num_frames][num_channels][LINNE_AMD_STAT_WORDS]
 */
#ifndef LINNE_AMD_H_INCLUDED
#define LINNE_AMD_H_INCLUDED

#include <stdint.h>
#include "linne.h"                        /* struct LINNEHeader, a member of struct LINNEAmdTrack */

#define LINNE_AMD_MAX_LAYERS      3
#define LINNE_AMD_MAX_PARAMS      128
#define LINNE_AMD_PARAM_WORDS     160     /* per channel-frame, see offsets below */
#define LINNE_AMD_STAT_WORDS      8

/* params record (int32 words) of one channel-frame:
 *   [0..1]  pre-emphasis prev (first sample of each stage's input; linne_encoder.c:637,707-709)
 *   [2..3]  pre-emphasis coefficient, 0..15            (linne_utility.c:158-193)
 *   [4..6]  number of units per layer (power of two)   (linne_network.c:268-347)
 *   [7..9]  coefficient right shift per layer          (lpc.c:981-1040)
 *   [10..]  quantised coefficients, layers back to back (sum of the preset's layer sizes <= 148),
 *           in filter order (index 0 multiplies the oldest sample; linne_network.c:310-316) */
#define LINNE_AMD_PRM_PREV    0
#define LINNE_AMD_PRM_PCOEF   2
#define LINNE_AMD_PRM_UNITS   4
#define LINNE_AMD_PRM_RSHIFT  7
#define LINNE_AMD_PRM_COEF    10

/* stats record (doubles) of one channel-frame, inputs of the host-side block-type decision
 * (linne_encoder.c:480-529, lpc.c:810-865):
 *   [0] r0        SIN-window autocorrelation lag 0 of the raw channel
 *   [1..3] k1..k3 PARCOR coefficients 1..order-1 of that analysis (order = layer-0 size)
 *   [4] zero_path 1.0 if that Levinson call took the all-zero branch (lpc.c:271-276), else 0.0
 *   [5] tail      value the channel's analysis leaves in parcor[order] (oracle quirk Q2)
 *   [6] best_pass index of the winning regulariser
 *   [7] loss      its L1 loss */
#define LINNE_AMD_ST_R0     0
#define LINNE_AMD_ST_K1     1
#define LINNE_AMD_ST_ZERO   4
#define LINNE_AMD_ST_TAIL   5
#define LINNE_AMD_ST_BEST   6
#define LINNE_AMD_ST_LOSS   7

struct LINNEAmdShape {                  /* batch-wide stream parameters (struct LINNEEncodeParameter) */
    uint32_t num_channels;
    uint32_t bits_per_sample;
    uint32_t num_samples_per_block;     /* = row stride of pcm / residual */
    uint32_t preset;
    uint32_t ch_process_method;         /* 0 none, 1 mid/side */
};

struct LINNEAmdContext;

#ifdef __cplusplus
extern "C" {
#endif

/* number of visible HIP devices (0 when there is none); never fails */
int LINNEAmd_GetDeviceCount(void);

/* Creates a context on `device`: a scratch arena of about scratch_bytes (0 = default 6 GiB, grown on
 * demand) and the stream work is issued on.  Returns NULL when the HIP runtime or the device is
 * unavailable -- there is no CPU fallback. */
struct LINNEAmdContext *LINNEAmd_ContextCreate(int device, uint64_t scratch_bytes);
void LINNEAmd_ContextDestroy(struct LINNEAmdContext *ctx);
/* message of the last failure on this context ("" if none) */
const char *LINNEAmd_GetLastError(const struct LINNEAmdContext *ctx);
/* grows the scratch arena to at least `bytes` (bigger arena = more frames per launch) */
int LINNEAmd_ReserveScratch(struct LINNEAmdContext *ctx, uint64_t bytes);
/* scratch one frame of this shape needs inside EncodeFramesDevice (0 for an invalid shape): frames x this = the arena that holds a
 * batch in one launch chunk */
uint64_t LINNEAmd_ScratchBytesPerFrame(const struct LINNEAmdShape *shape);
/* issue all subsequent work on an existing hipStream_t (e.g. torch's current stream); NULL names the device's
 * default (null) stream.  Until this is called the context uses a stream of its own. */
int LINNEAmd_SetStream(struct LINNEAmdContext *ctx, void *hip_stream);

/* `-a N` (struct LINNEEncodeParameter.num_afmethod_iterations; lpc.c:578-633): the number of auxiliary-function iterations that
 * refine every layer's coefficients in the final pass of LINNENetwork_SetUnitsAndParameters (linne_network.c:605-630).  Applies to
 * the following EncodeFramesDevice / Host calls of this context; 0 (the default) = off.  With N > 0 a call synchronises the
 * host: every Cholesky pivot's pow(x, -0.5) is taken from the host's libm, whose bits no device routine can promise. */
int LINNEAmd_SetAfIterations(struct LINNEAmdContext *ctx, uint32_t iterations);
/* `-l` (struct LINNEEncodeParameter.enable_learning; linne_encoder.c:669-675): after the analysis every channel-frame's parameters go
 * through LINNENetworkTrainer_Train (linne_network.c:805-873: up to 2000 momentum-SGD steps on the L1 loss).  Synchronises the host. */
int LINNEAmd_SetLearning(struct LINNEAmdContext *ctx, uint32_t enable);

/* ENCODE hot path, device resident.  Replaces, for every frame of the batch, the numeric core of
 * LINNEEncoder_EncodeCompressData (linne_encoder.c:613-696) and the analysis half of
 * LINNEEncoder_DecideBlockDataType (linne_encoder.c:494-503):
 *   MS (linne_utility.c:120-132) -> 2x pre-emphasis (:158-212) -> per regulariser { per layer { Welch window,
 *   autocorrelation, Levinson-Durbin (lpc.c:176-366) for every unit count; residual L1 search
 *   (linne_network.c:268-347); forward (linne_network.c:165-210) } } -> best regulariser (linne_network.c:605-630)
 *   -> quantisation (lpc.c:981-1040) -> int32 FIR cascade (linne_lpc_predict.c:7-38).
 * d_pcm: right-justified signed PCM; h_num_samples[f] <= stride is frame f's valid length (host array,
 * NULL = all frames full).  Work is enqueued on the context's stream; the call returns without
 * synchronising unless it has to grow the arena. */
int LINNEAmd_EncodeFramesDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        const int32_t *d_pcm, const uint32_t *h_num_samples, uint32_t num_frames,
        int32_t *d_residual, int32_t *d_params, double *d_stats);

/* DECODE hot path, device resident, in place: d_data holds the entropy-decoded residual on entry and PCM on
 * return.  Replaces linne_decoder.c:503-522: per channel the int32 synthesis cascade in reverse layer order
 * (linne_lpc_synthesize.c:8-83), two-stage de-emphasis (linne_utility.c:215-241), then MS->LR
 * (linne_utility.c:135-147).  d_params' coefficients must lie in [-128, 127], the range the stream's 8-bit coefficient code can
 * express (lnn_parse_block delivers nothing else): the synthesis kernels multiply them on 8-bit / exact-FP64 paths. */
int LINNEAmd_DecodeFramesDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        int32_t *d_data, const uint32_t *h_num_samples, uint32_t num_frames, const int32_t *d_params);

/* Same two paths on host buffers (H2D, kernels, D2H, synchronous); what EncodeBlock / DecodeBlock use.  Where the parameter records
 * are in HOST memory -- here and in the staging slots' decode submits -- the [-128, 127] contract of the coefficients is CHECKED:
 * a record outside it is refused with LINNE_APIRESULT_INVALID_FORMAT's value (2), so that no result depends on which form of the
 * synthesis the batch size picks. */
int LINNEAmd_EncodeFramesHost(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        const int32_t *pcm, const uint32_t *num_samples, uint32_t num_frames,
        int32_t *residual, int32_t *params, double *stats);
int LINNEAmd_DecodeFramesHost(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        int32_t *data, const uint32_t *num_samples, uint32_t num_frames, const int32_t *params);

/* Rice planning on the device (linne_coder.c:217-279): for every channel-frame of a batch, the
 * partition means of the zig-zagged residual, the parameter of every partition at every partition order, the code length
 * of every order and the argmin -- everything of LINNECoder_EncodePartitionedRecursiveRice except writing the bits.
 * Plan record per channel-frame, LINNE_AMD_RICE_PLAN_BYTES bytes: [0] partition order, [1] 1 if some mean fell inside the
 * guard band of a parameter step (the host then runs its own search for this channel-frame; the libm expression decides),
 * [16 ..] the parameter of each partition of the chosen order.  Enqueues on the context's stream. */
#define LINNE_AMD_RICE_PLAN_BYTES  1040
#define LINNE_AMD_RICE_PLAN_NBITS  4       /* uint32 at this byte offset: length of the channel's whole Rice code in bits (0xFFFFFFFF when flagged) */
#define LINNE_AMD_RICE_PLAN_K2     16
int LINNEAmd_RicePlanDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        const int32_t *d_residual, const uint32_t *h_num_samples, uint32_t num_frames, uint8_t *d_plan);

/* Rice EMISSION on the device (beyond step 2): writes every channel-frame's partitioned recursive Rice code
 * (linne_coder.c:281-302 with the bit order of bit_stream.h:240-282) from the residual and the plan RicePlanDevice made for the
 * same batch (call it first).  d_offsets [F * C + 1] receives each code's byte offset in d_packed (8-byte aligned; 0xFFFFFFFF
 * for a channel-frame whose plan is flagged or whose code does not fit), the last entry the bytes used.  The host stage then
 * appends the codes at their bit positions instead of coding the residual (LINNEAmd_PackFramesEmitted). */
int LINNEAmd_RiceEmitDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        const int32_t *d_residual, uint32_t num_frames, const uint8_t *d_plan,
        uint32_t *d_offsets, uint8_t *d_packed, uint64_t packed_capacity);

/* Rice DECODING on the device (linne_coder.c:306-327): lanes = frames, every lane walks its block's channels from d_bitpos[f] on.
 * d_stream must be 4-byte aligned and readable up to the next multiple of 8 behind stream_bytes.  d_endbit[f] = the bit position
 * behind the frame's last code, ~0 for a frame whose code holds something no encoder writes (decode it on the host). */
int LINNEAmd_RiceDecodeDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_bitpos, const uint32_t *h_num_samples, uint32_t num_frames,
        int32_t *d_residual, uint64_t *d_endbit);

/* Staging slots: what a whole-stream caller (LINNEEncoder_EncodeWhole / LINNEDecoder_DecodeWhole,
 * linne_encoder.c:865-932, linne_decoder.c:671-742) uses instead of the synchronous host forms.  A slot owns pinned
 * host buffers and device buffers for up to max_frames frames of one shape.  The caller fills SlotPcm (encode) or
 * SlotData + SlotParams (decode), submits, and later waits; Submit only enqueues (H2D on a copy stream, the kernels on
 * the context stream, D2H on a second copy stream, chained by events), so rotating over two or three slots overlaps
 * the host entropy stage, PCIe and the kernels.  After SlotWait: encode -> SlotData = residual, SlotParams, SlotStats;
 * decode -> SlotData = PCM.  A slot must be destroyed before its context. */
struct LINNEAmdSlot;
struct LINNEAmdSlot *LINNEAmd_SlotCreate(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        uint32_t max_frames, int for_encode);
/* Encode slots with less PCIe traffic (what LINNEEncoder_EncodeWhole uses):
 *   LINNE_AMD_SLOT_PCM16  the input is staged NARROW (SlotPcm16; LINNEAmd_SlotPcmWidth bytes per sample: int16 up to 16 bits per sample,
 *                         packed little-endian 3-byte samples up to 24, ignored above) and widened on the device;
 *   LINNE_AMD_SLOT_EMIT   the device also WRITES the residual's Rice code (linne_coder.c:281-302; LINNEAmd_RiceEmitDevice): after
 *                         SlotWait, SlotPacked holds the channels' codes back to back, SlotOffsets[cf] the byte offset of
 *                         channel-frame cf's code (0xFFFFFFFF: not emitted -- flagged plan or no room; the host then fetches that
 *                         frame's residual with SlotFetchResidual and codes it itself), SlotRicePlan the plans with each code's
 *                         bit length at LINNE_AMD_RICE_PLAN_NBITS.  The residual is not copied to the host (SlotData is NULL). */
#define LINNE_AMD_SLOT_PCM16  1u
#define LINNE_AMD_SLOT_EMIT   2u
#define LINNE_AMD_SLOT_STREAM 4u       /* decode slots: see LINNEAmd_SlotDecodeStreamSubmit */
struct LINNEAmdSlot *LINNEAmd_SlotCreateEx(struct LINNEAmdContext *ctx, const struct LINNEAmdShape *shape,
        uint32_t max_frames, int for_encode, uint32_t flags);
uint32_t  LINNEAmd_SlotFlags(const struct LINNEAmdSlot *slot);
int16_t  *LINNEAmd_SlotPcm16(struct LINNEAmdSlot *slot);                   /* [F][C][S] int16 (NULL unless LINNE_AMD_SLOT_PCM16 took effect; SlotPcm is NULL then) */
const uint8_t  *LINNEAmd_SlotPacked(struct LINNEAmdSlot *slot);
const uint32_t *LINNEAmd_SlotOffsets(struct LINNEAmdSlot *slot);           /* [F * C + 1], the last entry = bytes used */
int LINNEAmd_SlotFetchResidual(struct LINNEAmdSlot *slot, uint32_t frame, int32_t *dst /* [C][S] */);
/* Decode slots with less PCIe traffic and no Rice decoding on the host (what LINNEDecoder_DecodeWhole uses for streams whose CRCs
 * it checks): created with LINNE_AMD_SLOT_STREAM (| LINNE_AMD_SLOT_PCM16 for <= 16-bit audio).  The caller copies the bytes of a group
 * of blocks into SlotStream, sets SlotBitPos[f] = the bit offset in that buffer at which frame f's first channel's Rice code starts
 * (behind the parameter bits; lnn_parse_block_head), fills SlotParams, and submits: H2D, LINNEAmd_RiceDecodeDevice, the synthesis
 * kernels, D2H.  After SlotWait: SlotEndBits[f] = the bit position behind frame f's last code (from which the bytes the block
 * consumed follow, linne_decoder.c:495-499), or ~0 when the stream held something no encoder writes -- the host must then decode
 * the group itself (SlotDecodeSubmit); PCM in SlotData, or in SlotPcm16 when SlotPcm16Valid (every sample fitted). */
uint8_t  *LINNEAmd_SlotStream(struct LINNEAmdSlot *slot);
uint64_t  LINNEAmd_SlotStreamCapacity(const struct LINNEAmdSlot *slot);
uint64_t *LINNEAmd_SlotBitPos(struct LINNEAmdSlot *slot);
/* [max_frames] where every block ends (bit position in the slot's stream buffer): the device's decoder reads a block's codes no further */
uint64_t *LINNEAmd_SlotBitEnd(struct LINNEAmdSlot *slot);
const uint64_t *LINNEAmd_SlotEndBits(struct LINNEAmdSlot *slot);
int LINNEAmd_SlotPcm16Valid(const struct LINNEAmdSlot *slot);
/* bytes per staged PCM sample of this slot: 4 (int32), 2 (int16) or 3 (packed little-endian: a LINNE_AMD_SLOT_PCM16 slot of 17 .. 24-bit
 * audio; SlotPcm16 then points at bytes) */
uint32_t LINNEAmd_SlotPcmWidth(const struct LINNEAmdSlot *slot);
int LINNEAmd_SlotDecodeStreamSubmit(struct LINNEAmdSlot *slot, uint64_t stream_bytes, const uint32_t *num_samples, uint32_t num_frames);
int LINNEAmd_SlotFetchPcm32(struct LINNEAmdSlot *slot, uint32_t num_frames);
void      LINNEAmd_SlotDestroy(struct LINNEAmdSlot *slot);
int32_t  *LINNEAmd_SlotPcm(struct LINNEAmdSlot *slot);       /* [F][C][S] int32, encode input (NULL for a decode slot) */
int32_t  *LINNEAmd_SlotData(struct LINNEAmdSlot *slot);      /* [F][C][S] int32, residual (encode out, decode in) / PCM (decode out) */
int32_t  *LINNEAmd_SlotParams(struct LINNEAmdSlot *slot);    /* [F][C][LINNE_AMD_PARAM_WORDS] */
double   *LINNEAmd_SlotStats(struct LINNEAmdSlot *slot);     /* [F][C][LINNE_AMD_STAT_WORDS] (NULL for a decode slot) */
uint8_t  *LINNEAmd_SlotRicePlan(struct LINNEAmdSlot *slot);  /* [F][C][LINNE_AMD_RICE_PLAN_BYTES] (NULL for a decode slot) */
uint32_t  LINNEAmd_SlotCapacity(const struct LINNEAmdSlot *slot);
int LINNEAmd_SlotEncodeSubmit(struct LINNEAmdSlot *slot, const uint32_t *num_samples, uint32_t num_frames);
int LINNEAmd_SlotDecodeSubmit(struct LINNEAmdSlot *slot, const uint32_t *num_samples, uint32_t num_frames);
int LINNEAmd_SlotWait(struct LINNEAmdSlot *slot);

/* Several GPUs from ONE process (the "direct per-GPU H2D/D2H" transport).  The reference has nothing like
 * it: its caller loops over blocks in one thread (tools/linne_codec/linne_codec.c:133-161).  Frames are independent on this path
 * (linne_encoder.c:637), so a batch on host memory is cut into groups of group_frames frames (0 = a default that gives every
 * device a few throughput-sized groups), group g goes to device g mod G, one host thread per device drives that device's staging
 * slots -- H2D and D2H on each GPU's own PCIe link, two or three groups in flight per device -- and the results land in the
 * caller's arrays in the caller's frame order.  No data ever moves between GPUs.
 *   devices == NULL / num_devices == 0: LINNE_AMD_DEVICES="0,1,..." if set, else every visible device.  The same device may be
 *   listed more than once (two contexts on one GPU: what the one-GPU tests do).
 * The whole-stream API functions (LINNEEncoder_EncodeWhole / LINNEDecoder_DecodeWhole) fan out the same way when
 * LINNE_AMD_DEVICES names several devices; their .lnn bytes do not depend on it. */
struct LINNEAmdMulti;
struct LINNEAmdMulti *LINNEAmd_MultiCreate(const int *devices, uint32_t num_devices, uint64_t scratch_bytes_per_device);
void LINNEAmd_MultiDestroy(struct LINNEAmdMulti *multi);
uint32_t LINNEAmd_MultiNumDevices(const struct LINNEAmdMulti *multi);
int LINNEAmd_MultiDevice(const struct LINNEAmdMulti *multi, uint32_t index);                       /* HIP device id of member `index`, -1 if out of range */
struct LINNEAmdContext *LINNEAmd_MultiContext(struct LINNEAmdMulti *multi, uint32_t index);       /* the member's context (timing, telemetry) */
const char *LINNEAmd_MultiGetLastError(const struct LINNEAmdMulti *multi);
/* pcm / residual [F][C][S], params [F][C][LINNE_AMD_PARAM_WORDS], stats [F][C][LINNE_AMD_STAT_WORDS] on the host;
 * rice_plan (may be NULL) [F][C][LINNE_AMD_RICE_PLAN_BYTES].  Synchronous.  Returns LINNEApiResult. */
int LINNEAmd_MultiEncodeFramesHost(struct LINNEAmdMulti *multi, const struct LINNEAmdShape *shape, const int32_t *pcm,
        const uint32_t *num_samples, uint32_t num_frames, int32_t *residual, int32_t *params, double *stats, uint8_t *rice_plan,
        uint32_t group_frames);
/* in place: data holds the residual on entry, PCM on return */
int LINNEAmd_MultiDecodeFramesHost(struct LINNEAmdMulti *multi, const struct LINNEAmdShape *shape, int32_t *data,
        const uint32_t *num_samples, uint32_t num_frames, const int32_t *params, uint32_t group_frames);

/* Number of (job, layer) unit-count searches of the last EncodeFramesDevice call that the certified order-free
 * search could not decide and that therefore ran the exact ordered sums (synchronises; -1 on error). */
int64_t LINNEAmd_GetLastFallbackCount(struct LINNEAmdContext *ctx);

/* Telemetry of the certified search (linne_network.c:338-341): over all (job, layer) searches of the last EncodeFramesDevice
 * call that the certificate decided, the smallest gap between the winning trial's upper bound and the runner-up's lower bound,
 * relative to the winning mean (synchronises; a huge value when no search had two trials; -1 on error).  LINNE_AMD_EXACT=1 in
 * the environment of ContextCreate makes every search take the exact ordered chains instead (for diffing the two paths). */
double LINNEAmd_GetLastMinMargin(struct LINNEAmdContext *ctx);

/* Test instrument of the certified search (off by default; nothing in production enables it): what the selection kernels decided
 * every unit-count search FROM.  After SetSearchCapture(ctx, 1) every EncodeFramesDevice call leaves LINNE_AMD_CAPTURE_WORDS doubles
 * per trial slot, indexed [frame][channel][regulariser pass][layer][LINNE_AMD_CAPTURE_TRIALS] with the frames in the CALLER's order
 * (whatever chunks, streams and class-sorted rows the call was cut into), trial t of a layer of P coefficients being the one with
 * 2^t units:
 *   [0] the mean of the order-free sum exactly as the certificate compared it    [1] its slack   [2] rel   [3] max |input|
 *   [4] the largest L1 norm of a unit's coefficients   [5] how the search was decided: 0 by the certificate, 1 by the exact
 *   ordered chains after the certificate refused (or LINNE_AMD_EXACT=1), 2 by k_last_layer's exact chains (then [0]..[4] were
 *   never computed)   [6] the ordered mean, where the exact chains ran   [7] the trial's unit count.
 * A word that was not computed, and every word of a slot without a trial, is NaN (all bits set).  The searches inside the real final
 * pass of -a N are not recorded.  Enabled or not, the call's results, telemetry and kernel choices are the same; disabled, the
 * kernels see a null pointer and write nothing.
 * GetLastSearchCapture synchronises, copies min(records, capacity_records) records (LINNE_AMD_CAPTURE_WORDS doubles each) of the
 * last encode call to host and returns the number of records that call left (0: capture was off; -1 on error). */
#define LINNE_AMD_CAPTURE_WORDS   8
#define LINNE_AMD_CAPTURE_TRIALS  8
int LINNEAmd_SetSearchCapture(struct LINNEAmdContext *ctx, int enable);
int64_t LINNEAmd_GetLastSearchCapture(struct LINNEAmdContext *ctx, double *host, uint64_t capacity_records);

/* blocks until everything enqueued on the context's stream has finished */
int LINNEAmd_Synchronize(struct LINNEAmdContext *ctx);

/* Per-kernel timing of the last Encode/DecodeFramesDevice call, measured with HIP events recorded on the
 * context's stream around each launch (only while timing is enabled).  GetLastTimingMs returns the summed
 * milliseconds of all launches of one kernel kind (negative if none was recorded), GetLastTimingLaunches their
 * count.  `which` is one of the kinds below; the numbers are ABI (callers pass them as plain integers). */
enum LINNEAmdTimingKind {
    LINNE_AMD_T_CALL = 0,               /* the whole call */
    LINNE_AMD_T_PREP = 1,               /* prep (k_prep, and k_prep_slow behind it) */
    LINNE_AMD_T_WINDOW = 2,             /* window */
    LINNE_AMD_T_AUTOCORR = 3,           /* autocorrelation: the long layer's kernel */
    LINNE_AMD_T_LEVINSON = 4,           /* levinson */
    LINNE_AMD_T_SEARCH = 5,             /* trial residual (the double-input instantiation with the fused one-unit forward: layers behind layer 0) */
    LINNE_AMD_T_EXACT = 6,              /* loss sum: the exact ordered chains and the selection after them */
    LINNE_AMD_T_SELECT = 7,             /* select */
    LINNE_AMD_T_FORWARD = 8,            /* forward (double input, behind a search with the fused one-unit forward) */
    LINNE_AMD_T_FINAL_LOSS = 9,         /* final loss */
    LINNE_AMD_T_FINALIZE = 10,          /* finalize (quantise + FIR cascade) */
    LINNE_AMD_T_SYNTH = 11,             /* synthesis: the one-launch form (k_synthesize) */
    LINNE_AMD_T_MS_TO_LR = 12,          /* MS->LR */
    LINNE_AMD_T_STATS = 13,             /* block-type statistics (runs on a side stream beside the analysis) */
    LINNE_AMD_T_AUTOCORR_SHORT = 14,    /* autocorrelation of the short layers */
    LINNE_AMD_T_SEARCH_L0 = 15,         /* trial residual of layer 0 (int32 input) */
    LINNE_AMD_T_FORWARD_L0 = 16,        /* forward of layer 0 (int32 input) */
    LINNE_AMD_T_RICE_PLAN = 17,         /* Rice plan */
    LINNE_AMD_T_SEARCH_PLAIN = 18,      /* trial residual without the fused one-unit forward (the last layer, or LINNE_AMD_SPECULATE=0): a different kernel from 5 */
    LINNE_AMD_T_FORWARD_PLAIN = 19,     /* forward behind such a search: a different kernel from 8 */
    LINNE_AMD_T_FWD_LOSS = 20,          /* the last layer's forward pass fused with its loss (k_fwd_loss, k_fwd_loss_mw, k_last_layer; replaces 19 + 9 for the frames it takes) */
    LINNE_AMD_T_HIST_P = 21,            /* the long layer's autocorrelation with lanes = jobs: k_autocorr_hist for the trials of order P ... */
    LINNE_AMD_T_HIST_P2 = 22,           /* ... and P/2 ... */
    LINNE_AMD_T_HIST_SUB = 23,          /* ... k_autocorr_sub for the shorter ones (21-23 replace 3 for the frames they take) */
    LINNE_AMD_T_RICE_EMIT = 24,         /* Rice scan + emission */
    LINNE_AMD_T_SEARCH_LONG = 25,       /* the long layer's search in one window pass (k_search_long; replaces 5 for the frames it takes) */
    LINNE_AMD_T_AF_PASS = 26,           /* the real final pass of -a N */
    LINNE_AMD_T_TRAIN = 27,             /* the -l trainer */
    LINNE_AMD_T_RICE_DECODE = 28,       /* Rice decoding */
    LINNE_AMD_T_SYNTH_BIG = 30,         /* the synthesis of the long layer (k_synth_big) */
    LINNE_AMD_T_SYNTH_SMALL = 31,       /* ... of the short layers and the de-emphasis (k_synth_small) */
    LINNE_AMD_T_SYNTH_PIPE = 32,        /* the pipelined latency form (k_synth_pipe: small batches) */
    LINNE_AMD_T_SYNTH_ROWS = 33,        /* the throughput form of a long layer (k_synth_rows<NCH > 0>: four channel-frames per wave, what large batches take) */
    LINNE_AMD_T_DEEMPH_LR = 34,         /* the de-emphasis behind it (k_deemph_lr; it includes MS->LR when whole frames lie in a block of 64 rows: no kind 12 then) */
    LINNE_AMD_T_SYNTH_L0_DE = 35,       /* layer 0 + de-emphasis + MS->LR in one launch (k_synth_l0_de) */
    LINNE_AMD_T_SYNTH_ROWS_SHORT = 36,  /* the throughput form of a short layer (k_synth_rows<0> / k_synth_rows8: four or eight channel-frames per wave) */
    /* the stream indexes (LINNEAmd_StreamIndexesCreate, and LINNEAmd_StreamIndexCreate as its one-stream case; a call of its own,
     * with 69 and 70 below) */
    LINNE_AMD_T_SX_COUNT = 37,          /* counting the block candidates (k_ib_count) */
    LINNE_AMD_T_SX_WRITE = 38,          /* writing them (k_ib_write) */
    LINNE_AMD_T_SX_SCAN = 39,           /* prefix sums and what reads them per stream (k_sx_scan, k_ib_seg, k_ib_first) */
    LINNE_AMD_T_SX_SUCC = 40,           /* successors (k_ib_succ) */
    LINNE_AMD_T_SX_JUMP = 41,           /* pointer doubling (k_sx_jump, a launch per level) */
    LINNE_AMD_T_SX_CHAIN_LEN = 42,      /* the chains' lengths (k_ib_chain_len) */
    LINNE_AMD_T_SX_CHAIN = 43,          /* their blocks (k_ib_chain) */
    LINNE_AMD_T_SX_CHECK = 44,          /* CRC16 and block checks (k_ib_check) */
    /* 45-47 were the kinds of LINNEAmd_DecodeStreamDevice's own kernels, which are gone (it reports 56-59 now); the numbers are not
     * reused, so that recorded profiles stay readable */
    /* the stream encoders (LINNEAmd_EncodeStreamsDevice, and LINNEAmd_EncodeStreamDevice as its one-track case; the analysis and
     * the Rice plan report as the kinds above); a launch of each per pass.  48, 50 and 52-55 were the kinds of the single call's own
     * launches, which are gone (it reports 60-68 now); the numbers are not reused, so that recorded profiles stay readable */
    LINNE_AMD_T_SE_COMPACT = 49,        /* compacting the Rice plans for the host step (k_se_compact) */
    LINNE_AMD_T_SE_SCAN = 51,           /* the blocks' offsets (k_sx_scan) */
    /* sample windows of indexed streams (LINNEAmd_DecodeWindowsDevice, and LINNEAmd_DecodeStreamDevice as its one-window case; a
     * launch of each per pass, with 28 and the synthesis' kinds 11-12, 30-36 between them) */
    LINNE_AMD_T_WX_GATHER = 56,         /* gathering the COMPRESS blocks' bytes into the packed segment (k_wx_gather) */
    LINNE_AMD_T_WX_PARAMS = 57,         /* parameter records (k_wx_params) */
    LINNE_AMD_T_WX_RICE_CHECK = 58,     /* the consumption check per window (k_wx_rice_check) */
    LINNE_AMD_T_WX_PLACE = 59,          /* placing every window's samples (k_wx_place) */
    /* ... and the rest of them (both calls; per pass a launch of each of 60-67, with 49, 51, the analysis' kinds and 17 between
     * them; 68 once per shape) */
    LINNE_AMD_T_SB_GATHER = 60,         /* gathering the rows of a pass from their tracks (k_sb_gather) */
    LINNE_AMD_T_SB_SIZE = 61,           /* block sizes into stream-order slots (k_se_size) */
    LINNE_AMD_T_SB_REDUCE = 62,         /* per track: bytes, lowest failing block (k_sb_reduce) */
    LINNE_AMD_T_SB_ZERO = 63,           /* zeroing the written tracks' regions (k_sb_zero) */
    LINNE_AMD_T_SB_PARAMS = 64,         /* parameter bits (k_se_params) */
    LINNE_AMD_T_SB_RICE = 65,           /* Rice codes (k_se_rice) */
    LINNE_AMD_T_SB_RAW = 66,            /* RAW payloads (k_se_raw) */
    LINNE_AMD_T_SB_CRC = 67,            /* CRC16 and block headers (k_se_crc) */
    LINNE_AMD_T_SB_HEADER = 68,         /* the finished tracks' stream headers (k_sb_header) */
    /* the rest of the stream indexes' kinds (both calls), numbered on from the kind above (lnn_device.hip asserts 69 and 70: a kind
     * put between them and 68 does not compile) */
    LINNE_AMD_T_IB_HEADERS,             /* 69: gathering every stream's header bytes (k_ib_headers) */
    LINNE_AMD_T_IB_BEHIND               /* 70: the place behind a chain that ends early (k_ib_behind) */
};
/* further kinds, numbered on (`which` is a plain integer): cutting and joining streams (LINNEAmd_SpliceStreamsDevice, a call of its own:
 * the kinds of LINNEAmd_DecodeWindowsDevice and LINNEAmd_EncodeStreamsDevice for its edge blocks, then one launch of each of these) */
enum LINNEAmdSpliceTimingKind {
    LINNE_AMD_SPLICE_T_COPY = 71,           /* every run of bytes of every output (k_sp_copy) */
    LINNE_AMD_SPLICE_T_HEADER = 72          /* the outputs' stream headers (k_sb_header) */
};
/* repairing damaged streams (LINNEAmd_RepairStreamsDevice, a call of its own: the batch index's kinds 37-39, 41, 43 and 69 for the
 * kernels it shares with it, 71 for its one copy launch, and one launch of each of these) */
enum LINNEAmdRepairTimingKind {
    LINNE_AMD_REPAIR_T_SOUND = 73,          /* which candidates are sound blocks: size bound, CRC16, structure (k_rp_sound) */
    LINNE_AMD_REPAIR_T_COMPACT = 74,        /* the sound ones in stream order (k_rp_compact) */
    LINNE_AMD_REPAIR_T_SUCC = 75,           /* their successors in the salvage chain (k_rp_succ) */
    LINNE_AMD_REPAIR_T_CHAIN_LEN = 76,      /* the chains' lengths (k_rp_chain_len) */
    LINNE_AMD_REPAIR_T_MARK = 77,           /* the cut at the header's sample count, where runs of adjacent kept blocks begin (k_rp_mark) */
    LINNE_AMD_REPAIR_T_RUNS = 78            /* a record per run (k_rp_runs) */
};
/* comparing windows with resident PCM (LINNEAmd_CompareWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice, with a launch of
 * this one wherever that call has one of kind 59) */
enum LINNEAmdCompareTimingKind {
    LINNE_AMD_COMPARE_T_COMPARE = 79        /* comparing every window's samples with the caller's PCM (k_wx_compare) */
};
/* measuring windows (LINNEAmd_MeasureWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice, with a launch of kind 80 wherever that
 * call has one of kind 59, and one launch each of kinds 81 and 82 per call that takes a pass) */
enum LINNEAmdMeasureTimingKind {
    LINNE_AMD_MEASURE_T_MEASURE = 80,       /* reducing every window's samples into its buckets' accumulators (k_wx_measure) */
    LINNE_AMD_MEASURE_T_PRESET = 81,        /* the call's accumulators preset, once, in front of the first pass (k_wx_measure_preset) */
    LINNE_AMD_MEASURE_T_COMMIT = 82         /* the tables of the windows that did not fail written to their d_out, once, behind the last pass (k_wx_measure_commit) */
};
/* digesting windows (LINNEAmd_DigestWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice, with a launch of kind 83 wherever that
 * call has one of kind 59, and one launch each of kinds 84 and 85 per call that takes a pass) */
enum LINNEAmdDigestTimingKind {
    LINNE_AMD_DIGEST_T_DIGEST = 83,         /* hashing every window's samples into its buckets' accumulators (k_wx_digest) */
    LINNE_AMD_DIGEST_T_PRESET = 84,         /* the call's accumulators zeroed and the tables of powers filled, once, in front of the first pass (k_wx_digest_preset) */
    LINNE_AMD_DIGEST_T_COMMIT = 85          /* the answers of the windows that did not fail written to their d_out, once, behind the last pass (k_wx_digest_commit) */
};
/* finding quiet runs in windows (LINNEAmd_QuietWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice, with a launch of kind 86
 * wherever that call has one of kind 59, and one launch each of kinds 87 to 91 per call that takes a pass) */
enum LINNEAmdQuietTimingKind {
    LINNE_AMD_QUIET_T_QUIET = 86,           /* a bit per sample frame of every window into its mask (k_wx_quiet) */
    LINNE_AMD_QUIET_T_PRESET = 87,          /* the call's masks zeroed, once, in front of the first pass (k_wx_quiet_preset) */
    LINNE_AMD_QUIET_T_COUNT = 88,           /* behind the last pass: the runs of every chunk of every mask counted (k_wx_quiet_runs) */
    LINNE_AMD_QUIET_T_SCAN = 89,            /* ... the counts' prefix sums (k_sx_scan) */
    LINNE_AMD_QUIET_T_STARTS = 90,          /* ... the runs' first samples into the tables of the windows that did not fail (k_wx_quiet_runs) */
    LINNE_AMD_QUIET_T_ENDS = 91             /* ... and their lengths (k_wx_quiet_runs) */
};
#define LINNE_AMD_QUIET_EXTRA_LAUNCHES 5    /* kinds 87 to 91, one launch each */
/* histogramming windows (LINNEAmd_HistogramWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice, with a launch of kind 92 wherever
 * that call has one of kind 59, and one launch each of kinds 93 and 94 per call that takes a pass) */
enum LINNEAmdHistogramTimingKind {
    LINNE_AMD_HISTOGRAM_T_HISTOGRAM = 92,   /* counting every window's samples into its bins' accumulators (k_wx_histogram) */
    LINNE_AMD_HISTOGRAM_T_PRESET = 93,      /* the call's accumulators zeroed, once, in front of the first pass (k_wx_histogram_preset) */
    LINNE_AMD_HISTOGRAM_T_COMMIT = 94       /* the tables of the windows that did not fail written to their d_out, once, behind the last pass (k_wx_histogram_commit) */
};
/* relating the channels of windows (LINNEAmd_RelateWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice, with a launch of kind 95 wherever
 * that call has one of kind 59, and one launch each of kinds 96 and 97 per call that takes a pass) */
enum LINNEAmdRelateTimingKind {
    LINNE_AMD_RELATE_T_RELATE = 95,         /* every window's channel pairs reduced into their buckets' accumulators (k_wx_relate) */
    LINNE_AMD_RELATE_T_PRESET = 96,         /* the call's accumulators zeroed, once, in front of the first pass (k_wx_relate_preset) */
    LINNE_AMD_RELATE_T_COMMIT = 97          /* the tables of the windows that did not fail written to their d_out, once, behind the last pass (k_wx_relate_commit) */
};
/* mixing the channels of windows (LINNEAmd_MixWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice, with a launch of this one wherever
 * that call has one of kind 59, and nothing else) */
enum LINNEAmdMixTimingKind {
    LINNE_AMD_MIX_T_MIX = 98                /* every window's sample frames through its channel matrix into its output (k_wx_mix) */
};
/* resampling windows (LINNEAmd_ResampleWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice -- its kind 59 places the windows' input
 * samples into the call's scratch --, and one launch each of kinds 99 and 100 per call that takes a pass) */
enum LINNEAmdResampleTimingKind {
    LINNE_AMD_RESAMPLE_T_PRESET = 99,       /* the call's input images zeroed, once, in front of the first pass (k_wx_resample_preset) */
    LINNE_AMD_RESAMPLE_T_RESAMPLE = 100     /* the outputs of the windows that did not fail filtered from their input images, once, behind the last pass (k_wx_resample) */
};
/* overlaying windows (LINNEAmd_OverlayWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice -- its kind 59 places the sources'
 * samples into the call's scratch --, and one launch of kind 101 per call that takes a pass) */
enum LINNEAmdOverlayTimingKind {
    LINNE_AMD_OVERLAY_T_OVERLAY = 101       /* the outputs whose sources did not fail summed from their sources' images, once, behind the last pass (k_wx_overlay) */
};
/* lag correlation of windows (LINNEAmd_LagWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice -- its kind 59 places the needles'
 * and the haystacks' samples into the call's scratch --, and one launch each of kinds 102 and 103 per call that takes a pass) */
enum LINNEAmdLagsTimingKind {
    LINNE_AMD_LAGS_T_LAGS = 102,            /* the sliding products of every tile (probe, pair, 256 lags, a chunk of the needle) into its partial sums, once, behind the last pass (k_wx_lags) */
    LINNE_AMD_LAGS_T_COMMIT = 103           /* the partial sums added per lag and the tables of the probes that did not fail written, once, behind kind 102 (k_wx_lags_commit) */
};
/* projecting frames of windows (LINNEAmd_ProjectWindowsDevice: the kinds of LINNEAmd_DecodeWindowsDevice -- its kind 59 places the windows'
 * input samples into the call's scratch --, and one launch each of kinds 104 and 105 per call that takes a pass) */
enum LINNEAmdProjectTimingKind {
    LINNE_AMD_PROJECT_T_PRESET = 104,       /* the call's input images zeroed and its basis tables cut into digit planes, once, in front of the first pass (k_wx_project_preset) */
    LINNE_AMD_PROJECT_T_PROJECT = 105       /* the frames of the windows that did not fail projected from their input images, once, behind the last pass (k_wx_project) */
};
double LINNEAmd_GetLastTimingMs(struct LINNEAmdContext *ctx, int which);
int LINNEAmd_GetLastTimingLaunches(struct LINNEAmdContext *ctx, int which);
/* The grid form of the last k_search_long launch (kind 25) of the most recent encode call: 0 a block per (job, tile), 1 one block
 * per job that walks the job's tiles (chosen by the launch's job count; LINNE_AMD_SEARCH_JOB=0 / 1 forces either), -1 if the call
 * did not launch the kernel. */
int LINNEAmd_GetLastSearchLongForm(struct LINNEAmdContext *ctx);
int LINNEAmd_EnableTiming(struct LINNEAmdContext *ctx, int enable);

/* Host entropy stage, batch form (thread pool over frames): serialises analysed frames to .lnn blocks exactly
 * as linne_encoder.c:698-749,806-855 does.  blocks_out receives the blocks back to back; block_sizes[f] their
 * byte counts.  pcm is needed for RAW blocks.  parcor_state (in/out, may be NULL = 0.0) carries oracle quirk Q2
 * across calls.  Returns LINNEApiResult. */
int LINNEAmd_PackFrames(const struct LINNEAmdShape *shape, const int32_t *pcm, const uint32_t *num_samples,
        uint32_t num_frames, const int32_t *residual, const int32_t *params, const double *stats,
        uint8_t *blocks_out, uint64_t blocks_capacity, uint32_t *block_sizes, double *parcor_state,
        uint32_t num_threads);
/* The same with the device's Rice plan (LINNEAmd_RicePlanDevice; NULL = search on the host): the host then only writes bits. */
int LINNEAmd_PackFramesPlanned(const struct LINNEAmdShape *shape, const int32_t *pcm, const uint32_t *num_samples,
        uint32_t num_frames, const int32_t *residual, const int32_t *params, const double *stats, const uint8_t *rice_plan,
        uint8_t *blocks_out, uint64_t blocks_capacity, uint32_t *block_sizes, double *parcor_state,
        uint32_t num_threads);

/* How the calling thread's last LINNEDecoder_DecodeWhole ran.  Bit 0: it finished with the device decoding the Rice codes
 * (LINNEAmd_SlotDecodeStreamSubmit; the default for CRC-checked streams, LINNE_AMD_DECODE_STREAM=0 turns it off).  Bit 1: it had
 * started that way, met a block no encoder writes (or 16-bit PCM out of range) and went over the stream again with the host's Rice
 * decoder, which is the reference's decoder restated (linne_coder.c:304-345). */
uint32_t LINNEAmd_LastDecodeWholeMode(void);

/* The host stage when the device wrote the Rice codes (LINNEAmd_RiceEmitDevice, or an encode slot with LINNE_AMD_SLOT_EMIT): block
 * types in stream order, then per block the header, the parameter bits (linne_encoder.c:698-735), the channels' codes appended at
 * the running bit position, padding and CRC16 (:743-749, :848-855).  PCM is read in place from the caller's planes (frame f of
 * the batch starts at sample first_sample + f * num_samples_per_block of every plane; needed for the SILENT test and RAW blocks).
 * fetch(arg, frame, dst[C][S]) must deliver a frame's residual; it is called for the (rare) channel-frames without a device code
 * (offset 0xFFFFFFFF).  Same bytes as LINNEAmd_PackFrames. */
int LINNEAmd_PackFramesEmitted(const struct LINNEAmdShape *shape, const int32_t *const *planes, uint64_t first_sample,
        const uint32_t *num_samples, uint32_t num_frames, const int32_t *params, const double *stats, const uint8_t *rice_plan,
        const uint8_t *packed, const uint32_t *offsets, int (*fetch)(void *arg, uint32_t frame, int32_t *dst), void *fetch_arg,
        uint8_t *blocks_out, uint64_t blocks_capacity, uint32_t *block_sizes, double *parcor_state, uint32_t num_threads);

/* ---- .lnn streams held in device memory: a block index built once, then decodes of sample ranges ----
 * LINNEAmd_StreamIndexCreate reads the 30-byte header through LINNEDecoder_DecodeHeader (the header errors of
 * LINNEDecoder_DecodeWhole), finds the chain of blocks, checks every block's CRC16 and the checks lnn's block parser makes
 * after it, all on the device.  d_stream: the device bytes of a whole stream, at any alignment.  Synchronous; returns NULL and
 * *result = LINNEApiResult when it fails (a NULL result is tolerated; a NULL ctx or d_stream is INVALID_ARGUMENT and writes no
 * text).  The call is the one-stream case of LINNEAmd_StreamIndexesCreate below, run by the same code: indexes[0] and results[0] of
 * that call, GetLastError's text without "stream 0: " before it.  The index holds O(blocks) memory, one device and one host
 * allocation freed by LINNEAmd_StreamIndexDestroy; building it uses scratch kept by the context, at the sizes stated there, and
 * counts as a call of one stream in LINNEAmd_GetLastIndexBatchCount.  The stream's bytes stay the caller's and must be passed again,
 * unchanged, to every decode.
 *
 * LINNEAmd_DecodeStreamDevice writes samples [first_sample, first_sample + num_samples) of every channel ch to
 * d_pcm[ch * pcm_stride + i], int32.  Enqueued on the context's stream and synchronous.  The result:
 *   - whole range [0, header.num_samples): the LINNEApiResult of LINNEDecoder_DecodeWhole with the CRC check on and a buffer of
 *     exactly num_samples per channel, and when that is OK the same PCM (samples the stream's blocks do not reach are 0).  The one
 *     exception: a CRC-valid block no encoder writes (a payload other than its size field says, Rice codes that do not end
 *     where the block does) may give LINNE_APIRESULT_NG instead; GetLastError names the block.
 *   - any range: the first failure among blocks 0 .. the last block the range overlaps (damage behind the range does not matter,
 *     damage before it does: earlier blocks fix where later samples sit); otherwise OK and that slice of the whole decode.  The
 *     Rice decoder's consumption is checked on the blocks the range decodes.
 *   - a range beyond num_samples: LINNE_APIRESULT_INVALID_ARGUMENT.
 * The CRC is always checked.  The call is the one-window case of LINNEAmd_DecodeWindowsDevice below (group_frames 0), run by the same
 * code: scratch (kept by the context) is as described there, and a range whose COMPRESS blocks hold 2^33 bytes or more is refused
 * with LINNE_APIRESULT_NG (decode it in parts).  Neither call writes any of d_pcm when the result is a block's failure. */
struct LINNEAmdStreamIndex;
struct LINNEHeader;
struct LINNEAmdStreamIndex *LINNEAmd_StreamIndexCreate(struct LINNEAmdContext *ctx, const uint8_t *d_stream,
        uint64_t stream_bytes, int *result);
void     LINNEAmd_StreamIndexDestroy(struct LINNEAmdStreamIndex *index);
int      LINNEAmd_StreamIndexHeader(const struct LINNEAmdStreamIndex *index, struct LINNEHeader *header);
uint32_t LINNEAmd_StreamIndexNumBlocks(const struct LINNEAmdStreamIndex *index);   /* the blocks a whole decode walks */
int LINNEAmd_DecodeStreamDevice(struct LINNEAmdContext *ctx, const struct LINNEAmdStreamIndex *index,
        const uint8_t *d_stream, uint64_t first_sample, uint64_t num_samples, int32_t *d_pcm, uint64_t pcm_stride);
/* host tables of the blocks a whole decode walks, NumBlocks entries each (first: NumBlocks + 1), valid until Destroy: a block's byte
 * offset in the stream, first sample, size field (the block holds size + 6 bytes), type (0 COMPRESS, 1 SILENT, 2 RAW) and samples.
 * Any of the out pointers may be NULL; a NULL index is INVALID_ARGUMENT */
int LINNEAmd_StreamIndexBlocks(const struct LINNEAmdStreamIndex *index, const uint64_t **off, const uint64_t **first,
        const uint32_t **size, const uint32_t **type, const uint32_t **nsmp);
/* the lowest failing block (-1: none; NumBlocks: the place behind the last block), its LINNEApiResult and byte offset */
int LINNEAmd_StreamIndexFailure(const struct LINNEAmdStreamIndex *index, int64_t *block, int32_t *code, uint64_t *byte);

/* ---- the indexes of many resident streams in one call ----
 * LINNEAmd_StreamIndexesCreate builds the indexes of num_streams streams.  For every stream i, indexes[i] and results[i] are what
 * LINNEAmd_StreamIndexCreate(ctx, d_streams[i], stream_bytes[i], &r) returns for it alone: a header error gives NULL and the single
 * call's code for that stream only, damage in the blocks an index with the same failing block, code and byte offset
 * (LINNEAmd_StreamIndexFailure); a NULL d_streams[i] is that stream's INVALID_ARGUMENT.  A failing stream does not disturb the
 * others.  Streams of different shapes may be mixed, a stream may be named twice (two independent indexes), and streams may be
 * adjacent views of one buffer at any alignment: every read of stream i is a byte load inside [0, stream_bytes[i]).
 * Returns LINNE_APIRESULT_OK when every stream is OK, otherwise the result of the lowest-numbered failing stream; GetLastError then
 * reads "stream <i>: " and the single call's text.  A HIP error or running out of memory fails the whole call: LINNE_APIRESULT_NG, in
 * every results[i] too, every indexes[i] NULL, nothing kept.  num_streams == 0 is OK; a NULL ctx, or NULL arrays with num_streams
 * > 0, INVALID_ARGUMENT; more than 2^32 - 2 block candidates (FF FF sync words with a plausible size field) over the whole call,
 * LINNE_APIRESULT_NG.
 * Every index is an ordinary one: it serves LINNEAmd_DecodeStreamDevice / LINNEAmd_DecodeWindowsDevice(Layout) next to indexes of
 * the single call and is destroyed with LINNEAmd_StreamIndexDestroy on its own, in any order, at any time (the indexes of a call
 * share one device and one host allocation, which the last of them frees).
 * The number of kernel launches, copies, host synchronisations (four once the scratch has grown) and device allocations (one once the
 * scratch has grown) does not depend on num_streams;
 * only the pointer-doubling depth K does on the streams: the smallest K with 2^K > the largest candidate count of one stream, K - 1
 * launches of kind 41.  Scratch, kept by the context and grown (an allocation and a wait more) when a call needs more than any
 * before it: about 12 bytes per 4096 stream bytes, 8 + 4 K bytes per candidate, and 128 bytes per stream in a pinned host buffer and
 * its device copy.
 * LINNEAmd_GetLastIndexBatchCount: of the last such call (a LINNEAmd_StreamIndexCreate call is one, of one stream), which = 0 the streams given, 1 the indexes built, 2 K, 3 its host
 * synchronisations, 4 its device allocations; -1 for a NULL ctx or any other `which`. */
int LINNEAmd_StreamIndexesCreate(struct LINNEAmdContext *ctx, const uint8_t *const *d_streams, const uint64_t *stream_bytes,
        uint32_t num_streams, struct LINNEAmdStreamIndex **indexes /* out [num_streams] */, int32_t *results /* out [num_streams] */);
int64_t LINNEAmd_GetLastIndexBatchCount(struct LINNEAmdContext *ctx, int which);

/* ---- many sample windows of resident streams in one call ----
 * LINNEAmd_DecodeWindowsDevice decodes num_windows windows, each a sample range of some stream with a built index; streams of
 * different shapes (channels, bits, block size, preset, MS) may be mixed, windows may overlap, repeat and name the same stream (a
 * block two windows share is decoded twice).  Every window's `result` and PCM are what LINNEAmd_DecodeStreamDevice(ctx, index,
 * d_stream, first_sample, num_samples, d_pcm, pcm_stride) returns and writes for it alone -- its argument checks, the index's
 * failing block at or before the range, the Rice consumption check; a failing window's d_pcm is never written, as in the single
 * call -- and a failing window does not disturb the others.  Returns LINNE_APIRESULT_OK when every window is OK, otherwise the result of the
 * lowest-numbered failing window; GetLastError then reads "window <i>: " and the single call's text.  A HIP error or running out of
 * memory fails the whole call: LINNE_APIRESULT_NG, in every `result` too.  num_windows == 0 is OK; a NULL ctx, or NULL windows with
 * num_windows > 0, INVALID_ARGUMENT.
 * The windows of one shape are decoded together: the number of kernel launches, copies and host synchronisations does not depend
 * on num_windows.  group_frames bounds the COMPRESS blocks of one pass (scratch, kept by the context: about 8 + 4 * C * S bytes per
 * COMPRESS block of the pass plus its stream bytes, and 64 bytes per block of the call in a pinned host buffer and its device copy);
 * 0 = one pass per shape, which is refused with LINNE_APIRESULT_NG when its COMPRESS blocks hold 2^33 bytes or more.  It never changes a result: windows are kept whole in a pass where they
 * fit, and a window of more COMPRESS blocks than group_frames has its Rice codes checked in passes of their own before any of its
 * samples is placed.  Enqueued on the context's stream and synchronous. */
struct LINNEAmdWindow {
    const struct LINNEAmdStreamIndex *index;   /* of the stream below, same device as the context */
    const uint8_t *d_stream;                   /* the stream's device bytes, any alignment */
    uint64_t first_sample, num_samples;
    int32_t *d_pcm; uint64_t pcm_stride;       /* channel ch, sample i -> d_pcm[ch * pcm_stride + i] */
    int32_t result;                            /* out: the LINNEApiResult of this window */
};
int LINNEAmd_DecodeWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        uint32_t num_windows, uint32_t group_frames);

/* ---- planar PCM held in device memory -> a .lnn stream in device memory ----
 * (the one-track case of the call below: the same code, so a track there and a call here cannot come apart)
 * LINNEAmd_EncodeStreamDevice encodes header->num_samples samples of every channel ch, read from d_pcm + ch * pcm_stride (int32,
 * right-justified; any element offset), into d_out[0, *out_bytes).  header's num_channels, num_samples, sampling_rate,
 * bits_per_sample, num_samples_per_block, preset and ch_process_method are used (the version fields are not); -a / -l come from
 * the context (LINNEAmd_SetAfIterations / SetLearning).  The result is the LINNEApiResult LINNEEncoder_EncodeWhole returns on a fresh
 * encoder (room for the header) given the same fields and settings and a buffer of `capacity` bytes, and when that is OK
 * d_out[0, *out_bytes) holds exactly its bytes:
 *   - the header checks of SetEncodeParameter, then EncodeHeader's (a capacity under 30 bytes, then the fields), with their codes;
 *   - LINNE_APIRESULT_INVALID_FORMAT when a block comes out RAW at a width other than 8, 16 or 24 bits, INSUFFICIENT_BUFFER when a
 *     block is over the host stitcher's 64 + C * S * 8 bytes -- the first such block in stream order; such a block takes precedence
 *     over a stream that does not fit (EncodeWhole meets the two in the order of its groups; with one group, in this order);
 *   - LINNE_APIRESULT_INSUFFICIENT_BUFFER when the stream is longer than `capacity` (or than 2^32 - 1 bytes): nothing is written at
 *     or beyond `capacity`, and *out_bytes is the size the stream needs (0 after a header or block error).
 * *parcor_state (may be NULL: start from 0.0 like a fresh encoder) is read, and on OK replaced by the value the host stitcher would
 * carry to the next call (oracle quirk Q2): two calls that thread it give the blocks of two EncodeWhole calls on one encoder.
 * group_frames bounds the frames of one analysis pass (device memory ~ 8 * C * S bytes per frame of a pass); 0 = the whole stream in
 * one pass.  It never changes the bytes.  d_out must be 4-byte aligned (INVALID_ARGUMENT otherwise): the bit fields are ORed into
 * 32-bit words, and the last word of the stream may be touched by an OR that leaves the bytes behind it as they are.  Enqueued on
 * the context's stream and synchronous: every pass has one host step (block types with the host's libm, Rice plans the device
 * left to the host).  The environment variable LINNE_AMD_RICE_GUARD (a test knob; default 1e-9) widens the device's guard band for
 * this entry point, sending more plans to the host; the bytes do not change. */
uint64_t LINNEAmd_EncodeStreamBound(const struct LINNEHeader *header);      /* 30 + blocks * (64 + C * S * 8): always enough */
int LINNEAmd_EncodeStreamDevice(struct LINNEAmdContext *ctx, const struct LINNEHeader *header,
        const int32_t *d_pcm, uint64_t pcm_stride, uint32_t group_frames,
        uint8_t *d_out, uint64_t capacity, uint64_t *out_bytes, double *parcor_state);
/* how the last EncodeStream(s)Device call of this context went (many tracks: the sums over the call): which 0 / 1 / 2 = its COMPRESS / SILENT / RAW blocks, 3 = the
 * channel-frames whose Rice plan the host settled (a mean in a guard band); -1 for a NULL context or another `which` */
int64_t LINNEAmd_GetLastStreamEncodeCount(struct LINNEAmdContext *ctx, int which);

/* ---- many tracks of planar PCM in device memory -> their .lnn streams in device memory, in one call ----
 * LINNEAmd_EncodeStreamsDevice encodes num_tracks tracks; tracks of different shapes (channels, bits, block size, preset, MS) may be
 * mixed, and two tracks may read the same PCM.  Every track's `result`, `out_bytes`, new `parcor_state` and bytes
 * d_out[0, out_bytes) are what LINNEAmd_EncodeStreamDevice(ctx, &header, d_pcm, pcm_stride, g, d_out, capacity, &out_bytes,
 * &parcor_state) returns and writes for it alone, for any g -- its argument checks (a NULL pointer or a misaligned d_out of one track
 * is that track's INVALID_ARGUMENT, its out_bytes left as it was), its header codes, its first refused block with that block's code
 * (out_bytes 0 after a header or block error), INSUFFICIENT_BUFFER with the needed size in out_bytes and nothing written at or beyond
 * `capacity`; parcor_state is replaced only on OK -- and a failing track does not disturb the others.  Returns LINNE_APIRESULT_OK when
 * every track is OK, otherwise the result of the lowest-numbered failing track; GetLastError then reads "track <i>: " and the single
 * call's text.  A HIP error or running out of memory fails the whole call: LINNE_APIRESULT_NG, in every `result` too.  num_tracks == 0
 * is OK; a NULL ctx, or NULL tracks with num_tracks > 0, INVALID_ARGUMENT; more than 2^31 - 1 frames in one call, NG.
 * -a / -l come from the context and apply to every track; LINNE_AMD_RICE_GUARD applies as in the single call;
 * LINNEAmd_GetLastStreamEncodeCount reports the sums over the call.
 * The tracks of one shape are encoded together: their frames, in the caller's track order, form one list that is cut into passes of
 * group_frames frames (0 = one pass per shape; a track may span passes); group_frames never changes a byte.  The kernel launches,
 * memsets, copies and host synchronisations of a pass do not depend on how many tracks it holds, with one exception: the analysis
 * (LINNEAmd_EncodeFramesDevice) takes at most 16 distinct frame lengths per call, so a pass whose frames have d distinct lengths
 * takes 1 call when d <= 16 and 1 + ceil((d - 16) / 16) otherwise.  Scratch (kept by the context) is about 8 * C * S bytes per frame
 * of a pass, plus 16 bytes per frame and about 100 per track, for the single call too.  The tracks' output buffers must be 4-byte aligned and must not overlap.
 * Enqueued on the context's stream and synchronous. */
struct LINNEAmdTrack {
    struct LINNEHeader header;                 /* as EncodeStreamDevice's header argument */
    const int32_t *d_pcm; uint64_t pcm_stride; /* channel ch at d_pcm + ch * pcm_stride */
    uint8_t *d_out; uint64_t capacity;         /* 4-byte aligned; the tracks' buffers do not overlap */
    uint64_t out_bytes;                        /* out */
    double parcor_state;                       /* in/out, quirk Q2; 0.0 = a fresh encoder */
    int32_t result;                            /* out: this track's LINNEApiResult */
};
int LINNEAmd_EncodeStreamsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdTrack *tracks,
        uint32_t num_tracks, uint32_t group_frames);
/* how the last EncodeStream(s)Device call of this context went: which 0 = its shape groups, 1 = its passes, 2 = its EncodeFramesDevice
 * calls (after a single call: 1 group, its passes, one analysis call per pass; 0, 0, 0 when the track failed its argument or header
 * checks); -1 for a NULL context or another `which` */
int64_t LINNEAmd_GetLastStreamBatchCount(struct LINNEAmdContext *ctx, int which);

/* ---- resident streams from and into int16, packed 24-bit and float PCM, planar or interleaved ----
 * A struct LINNEAmdPcmLayout names how the caller's PCM lies in device memory: sample i of channel ch is element
 * ch * channel_stride + i * sample_stride from the base pointer, the strides counted in elements of the format (an S24 element is
 * 3 bytes, little-endian).  Planar is (stride, 1), interleaved is (1, C); padded variants of both are legal.  With a layout the
 * track's or window's d_pcm (the single call's d_pcm) is that base pointer, whatever its declared type, and pcm_stride is ignored.
 * The three calls below are the calls above with a layout per track / window (the single call: one); `layout(s) == NULL` is
 * exactly the call above, which is that case of the same code.
 *   encode  the samples are sign-extended from the format and taken as right-justified values: result, out_bytes, parcor_state and
 *           bytes are those of the call above on an int32 planar copy of the same values (header.bits_per_sample is independent of
 *           the format).  LINNE_AMD_PCM_F32, or an unknown format, is that track's INVALID_ARGUMENT.
 *   decode  every window's result and samples are those of LINNEAmd_DecodeStreamDevice, converted: S32 as is; S16 and S24
 *           saturated to the format's range, `saturated` = 1 when some sample of the window lay outside it; F32 =
 *           (float)v * 2^-(bits_per_sample - 1), the conversion rounding to nearest-even (exact up to 25 bits).  `saturated` is 0
 *           otherwise and left untouched for a failing window, whose memory is still never written.
 * Checked per track / window (INVALID_ARGUMENT for it alone, out_bytes left as it was): the base is aligned to the element (2 bytes
 * for S16, 4 for S32 and F32, any for S24), and for C > 1 channels of n samples the index map is injective in one of two ways:
 * sample_stride >= 1 && channel_stride >= n * sample_stride, or channel_stride >= 1 && sample_stride >= C * channel_stride (C == 1:
 * sample_stride >= 1).  No load or store touches a byte outside the elements the layout names; an element is written by plain
 * stores that touch no byte of another element's owner.  Tracks and windows of one stream shape stay in one shape group and one
 * pass whatever their layouts: the launches, copies and synchronisations of a pass are those of the int32 planar call. */
enum { LINNE_AMD_PCM_S32 = 0, LINNE_AMD_PCM_S16 = 1, LINNE_AMD_PCM_S24 = 2 /* packed 3-byte little-endian */, LINNE_AMD_PCM_F32 = 3 /* decode only */ };
struct LINNEAmdPcmLayout {
    uint32_t format;
    uint32_t saturated;                 /* out, decode only: 1 if some sample of the window lay outside the format's range */
    uint64_t channel_stride, sample_stride;   /* in elements of the format (an S24 element is 3 bytes) */
};
int LINNEAmd_EncodeStreamDeviceLayout(struct LINNEAmdContext *ctx, const struct LINNEHeader *header,
        const void *d_pcm, const struct LINNEAmdPcmLayout *layout, uint32_t group_frames,
        uint8_t *d_out, uint64_t capacity, uint64_t *out_bytes, double *parcor_state);
int LINNEAmd_EncodeStreamsDeviceLayout(struct LINNEAmdContext *ctx, struct LINNEAmdTrack *tracks,
        const struct LINNEAmdPcmLayout *layouts /* [num_tracks] */, uint32_t num_tracks, uint32_t group_frames);
int LINNEAmd_DecodeWindowsDeviceLayout(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        struct LINNEAmdPcmLayout *layouts /* [num_windows], in/out */, uint32_t num_windows, uint32_t group_frames);

/* ---- comparing sample windows of resident streams with resident PCM: the proof that a stream holds the samples it was made from ----
 * LINNEAmd_CompareWindowsDevice takes the windows and layouts of LINNEAmd_DecodeWindowsDeviceLayout (layouts == NULL: int32 planar,
 * pcm_stride) and, instead of writing every window's samples to its d_pcm, compares them with what d_pcm holds.
 * Every window's `result` is what LINNEAmd_DecodeWindowsDeviceLayout gives it -- its argument, layout and alignment checks, the
 * index's failing block at or before the range, the Rice consumption check -- with one exception: LINNE_AMD_PCM_F32 is that window's
 * INVALID_ARGUMENT, as on encode.  For an OK window diffs[i] describes the difference between what that call would have written and
 * what d_pcm holds: num_differing counts the (sample, channel) elements that differ, first_sample / first_channel name the first of
 * them -- the lowest sample, then the lowest channel; both 0 when there is none.  A window that differs is still LINNE_APIRESULT_OK:
 * a difference is an answer, not an error.  S32 elements are compared as they are; S16 and S24 elements are sign-extended and
 * compared with the decoded value, nothing is saturated: a decoded sample outside the format's range differs from every element
 * (where the decode call would have clipped and set `saturated`).  A failing window's diffs[i] is left as it was, and a failing
 * window does not disturb the others.
 * d_pcm is only read -- no load touches a byte outside the elements the layout names -- and layouts[i].saturated is not written.
 * Shape groups, passes, group_frames, scratch and whole-call failures are the decode call's: LINNE_APIRESULT_OK when every window is
 * OK, otherwise the result of the lowest-numbered failing window, with "window <i>: " and the single call's text in GetLastError; a
 * HIP error or running out of memory fails the whole call (LINNE_APIRESULT_NG, in every `result` too, diffs untouched).  The number
 * of kernel launches, copies (one upload, one fetch) and host synchronisations (one) does not depend on num_windows; a pass has the
 * decode call's launches with kind 79 in place of kind 59, and a window that spans passes collects its answer over them.
 * num_windows == 0 is OK; a NULL ctx, or NULL windows or NULL diffs with num_windows > 0, INVALID_ARGUMENT.  Enqueued on the
 * context's stream and synchronous. */
struct LINNEAmdDiff {
    uint64_t num_differing;             /* (sample, channel) elements of the window that differ */
    uint64_t first_sample;              /* stream sample index of the first one: lowest sample, then lowest channel; 0 when none */
    uint32_t first_channel;             /* 0 when none */
    uint32_t reserved;
};
int LINNEAmd_CompareWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        const struct LINNEAmdPcmLayout *layouts /* [num_windows]; NULL: int32 planar, pcm_stride */,
        struct LINNEAmdDiff *diffs /* [num_windows], out */, uint32_t num_windows, uint32_t group_frames);

/* ---- measuring sample windows of resident streams: min, max, sum and energy per channel and bucket, no PCM written ----
 * LINNEAmd_MeasureWindowsDevice takes the windows of LINNEAmd_DecodeWindowsDevice and, instead of writing every window's samples,
 * reduces them: the only output is a table of struct LINNEAmdMeasure per window, in device memory.  A window of n samples with
 * specs[i].bucket_samples = b > 0 has nb = ceil(n / b) buckets, bucket k holding the window's samples [k * b, min((k + 1) * b, n))
 * (the last one may be short); b == 0 is one bucket of the whole window; a window of no samples has no buckets and nothing is
 * written.  The samples are exactly those LINNEAmd_DecodeStreamDevice writes for the range -- int32, nothing saturated, the zeros of
 * SILENT blocks and of the range behind the stream's last block included -- and every number is exact integer arithmetic: the sum
 * of squares is kept as a 128-bit unsigned integer.  The windows' d_pcm and pcm_stride are ignored and may be NULL and 0.
 * Every window's `result` is what LINNEAmd_DecodeWindowsDevice gives it (its argument checks but those of d_pcm and pcm_stride, the
 * index's failing block at or before the range, the Rice consumption check), and for that window alone INVALID_ARGUMENT when d_out
 * is NULL (with n > 0) or not 8-byte aligned, when channel_stride < nb, or when nb > 2^32 - 1.  A failing window's d_out is never
 * written, and a failing window does not disturb the others.  No byte outside d_out[ch * channel_stride + k], ch < channels,
 * k < nb, is written; the outputs of different windows must not overlap; the streams are only read.
 * Shape groups, passes, group_frames, scratch and whole-call failures are the decode call's: LINNE_APIRESULT_OK when every window is
 * OK, otherwise the result of the lowest-numbered failing window, with "window <i>: " and the single call's text in GetLastError; a
 * HIP error or running out of memory fails the whole call (LINNE_APIRESULT_NG, in every `result` too).  A pass has the decode
 * call's launches with kind 80 in place of kind 59; a call that takes at least one pass adds exactly two launches, whatever
 * num_windows is: kind 81 in front of the first pass (the accumulators preset) and kind 82 behind the last (the tables of the windows
 * whose Rice check passed written to their d_out); a window that spans passes collects its answer over them.  Copies (one upload,
 * one fetch) and host synchronisations (one) do not depend on num_windows.  The accumulators live in the context's scratch: one
 * record per (channel, bucket) of every window, times up to 64 for windows whose buckets are 8192 samples or longer (so that the
 * workgroups of a long bucket do not queue on one address) -- at most 1/32 of the windows' int32 PCM for those.
 * num_windows == 0 is OK; a NULL ctx, or NULL windows or NULL specs with num_windows > 0, INVALID_ARGUMENT.  Enqueued on the
 * context's stream and synchronous. */
struct LINNEAmdMeasure {                /* 32 bytes: one channel of one bucket of one window */
    int32_t min, max;                   /* over the bucket's samples */
    int64_t sum;                        /* exact */
    uint64_t sumsq_lo, sumsq_hi;        /* the exact sum of squares, a 128-bit unsigned integer */
};
struct LINNEAmdMeasureSpec {
    uint64_t bucket_samples;            /* 0: the whole window is one bucket */
    struct LINNEAmdMeasure *d_out;      /* device, 8-byte aligned: channel ch, bucket k at d_out[ch * channel_stride + k] */
    uint64_t channel_stride;            /* in records, >= the window's bucket count */
};
int LINNEAmd_MeasureWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        const struct LINNEAmdMeasureSpec *specs /* [num_windows] */, uint32_t num_windows, uint32_t group_frames);

/* ---- digesting sample windows of resident streams: the CRC-32 of the decoded PCM per bucket, no PCM written ----
 * LINNEAmd_DigestWindowsDevice takes the windows of LINNEAmd_DecodeWindowsDevice and, instead of writing every window's samples,
 * hashes them: the only output is a table of struct LINNEAmdDigest per window, in device memory.  The digest of a whole stream
 * equals zlib's crc32() of the `data` chunk of the WAV file that the reference's `linne -d` (and linne_amd_cli -d) writes for it.
 * The byte string of the samples [first, first + n) of a stream of C channels and `bits` bits per sample: the samples in sample
 * order and, within a sample, in channel order (interleaved); every value in w = ceil(bits / 8) bytes, little-endian, the low w
 * bytes of the two's-complement int32 that LINNEAmd_DecodeStreamDevice writes; for w == 1 the byte is (v + 128) & 0xFF, WAV's 8-bit
 * form being unsigned (libs/wav/src/wav.c, the writer's 8/16/24/32 cases).  Nothing is saturated: a value outside the width is
 * truncated, as in the reference's writer.  The zeros of SILENT blocks and of the range behind the stream's last block are part of
 * the string (for 8-bit streams they are 0x80 bytes, not nothing).
 * Buckets are LINNEAmd_MeasureWindowsDevice's: specs[i].bucket_samples = b > 0 gives nb = ceil(n / b) buckets, bucket k covering the
 * window's samples [k * b, min((k + 1) * b, n)), all channels (the last one may be short); b == 0 is one bucket of the whole window;
 * a window of no samples has no buckets and nothing is written.  Bucket k's answer, at d_out[k]: crc32, the zlib / IEEE 802.3
 * CRC-32 of the bucket's byte string (reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF), and num_bytes, the
 * string's length.  CRC-32 is linear over GF(2): the pieces of a bucket are hashed independently and folded with XOR in any order,
 * so the answer is exact and does not depend on the order the device takes them in.
 * Everything LINNEAmd_MeasureWindowsDevice says about results holds unchanged: the windows' d_pcm and pcm_stride are ignored;
 * every window's `result` is what LINNEAmd_DecodeWindowsDevice gives it, and for that window alone INVALID_ARGUMENT when d_out is
 * NULL (with n > 0) or not 8-byte aligned, or when nb > 2^32 - 1.  A failing window's d_out is never written, and a failing window
 * does not disturb the others.  No byte outside d_out[0 .. nb) is written; the outputs of different windows must not overlap; the
 * streams are only read.  Shape groups, passes, group_frames, scratch and whole-call failures are the decode call's, with
 * "window <i>: " and the single call's text in GetLastError.  A pass has the decode call's launches with kind 83 in place of
 * kind 59; a call that takes at least one pass adds exactly two launches, whatever num_windows is: kind 84 in front of the first
 * pass and kind 85 behind the last; a window that spans passes collects its answer over them.  Copies (one upload, one fetch) and
 * host synchronisations (one) are the measure call's.  The accumulators live in the context's scratch: one 32-bit word per bucket
 * of every window, times up to 64 (16 words apart) for windows whose buckets are 8192 samples or longer, behind 40 KiB of tables.
 * num_windows == 0 is OK; a NULL ctx, or NULL windows or NULL specs with num_windows > 0, INVALID_ARGUMENT.  Enqueued on the
 * context's stream and synchronous. */
struct LINNEAmdDigest {                 /* 16 bytes: one bucket of one window */
    uint32_t crc32;                     /* of the bucket's byte string, as zlib's crc32() gives it */
    uint32_t reserved;                  /* 0 */
    uint64_t num_bytes;                 /* the byte string's length */
};
struct LINNEAmdDigestSpec {
    uint64_t bucket_samples;            /* 0: the whole window is one bucket */
    struct LINNEAmdDigest *d_out;       /* device, 8-byte aligned: bucket k at d_out[k] */
};
int LINNEAmd_DigestWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        const struct LINNEAmdDigestSpec *specs /* [num_windows] */, uint32_t num_windows, uint32_t group_frames);

/* ---- finding the quiet runs of sample windows of resident streams: where is the silence?  No PCM written ----
 * LINNEAmd_QuietWindowsDevice takes the windows of LINNEAmd_DecodeWindowsDevice and, instead of writing every window's samples,
 * lists the window's quiet runs: the only output in device memory is a table of struct LINNEAmdRun per window.  The samples are
 * exactly those LINNEAmd_DecodeStreamDevice writes for the range -- int32, L/R after MS, nothing saturated, the zeros of SILENT blocks
 * and of the range behind the stream's last block included.  A sample frame is quiet when |v| <= specs[i].threshold in EVERY
 * channel; |v| is taken in 64 bits, so INT32_MIN has magnitude 2^31 and is quiet only for threshold >= 2^31.  A run is a maximal
 * stretch of consecutive quiet frames inside the window: it ends at the window's ends, whatever lies outside.  The runs of at least
 * max(min_samples, 1) frames are reported in ascending order: answers[i].num_runs counts them and quiet_samples adds their lengths,
 * whether or not they fitted, and the first min(num_runs, capacity) of them are written to d_out; no byte of d_out behind those
 * records is touched.  num_runs > capacity is not an error: count first (capacity 0, d_out NULL), then call again with room.
 * lead_samples and trail_samples are the quiet frames at the window's start and at its end, whatever min_samples is; both are the
 * window's length when no frame of it is loud.  A window of no samples is OK with all four answers 0.
 * Everything LINNEAmd_MeasureWindowsDevice says about results holds unchanged: the windows' d_pcm and pcm_stride are ignored;
 * every window's `result` is what LINNEAmd_DecodeWindowsDevice gives it, and for that window alone INVALID_ARGUMENT when d_out is
 * NULL with capacity > 0 or not 8-byte aligned.  A failing window's d_out and answers[i] are never written, and a failing window
 * does not disturb the others.  The outputs of different windows must not overlap; the streams are only read.  Shape groups, passes,
 * group_frames, scratch and whole-call failures are the decode call's, with "window <i>: " and the single call's text in
 * GetLastError.  A pass has the decode call's launches with kind 86 in place of kind 59; a call that takes at least one pass adds
 * exactly LINNE_AMD_QUIET_EXTRA_LAUNCHES = 5 launches, whatever num_windows is: kind 87 in front of the first pass (the masks
 * zeroed) and kinds 88, 89, 90 and 91 behind the last (the runs counted per chunk, the counts' prefix sums, the runs' first samples
 * and their lengths written for the windows whose Rice check passed); a window that spans passes collects its mask over them.
 * Copies (one upload, one fetch) and host synchronisations (one) do not depend on num_windows.  The context's scratch holds one bit
 * per sample frame of every window, rounded up to 64 per window, and 24 bytes per 16384 frames (a commit workgroup's chunk) for the
 * counts and their prefix sums: 1/32 of ONE channel's int32 PCM, and never a word per sample or per run.  A test of min_samples walks
 * at most min_samples bits of its run in one lane, 64 at a time: a call with min_samples in the millions on material that has such
 * runs spends that walk's time in kinds 88, 90 and 91.
 * num_windows == 0 is OK; a NULL ctx, or NULL windows, NULL specs or NULL answers with num_windows > 0, INVALID_ARGUMENT.  Enqueued
 * on the context's stream and synchronous. */
struct LINNEAmdRun {                    /* 16 bytes: one quiet run of one window */
    uint64_t first_sample, num_samples; /* stream sample index; length */
};
struct LINNEAmdQuietSpec {
    uint32_t threshold, reserved;       /* a sample frame is quiet when |v| <= threshold in EVERY channel */
    uint64_t min_samples;               /* report runs of at least this many frames; 0 is taken as 1 */
    struct LINNEAmdRun *d_out;          /* device, 8-byte aligned; may be NULL when capacity == 0 */
    uint64_t capacity;                  /* records d_out has room for */
};
struct LINNEAmdQuiet {                  /* host, out, per window */
    uint64_t num_runs;                  /* runs found, whether or not they fitted */
    uint64_t quiet_samples;             /* the sum of their lengths */
    uint64_t lead_samples, trail_samples;   /* quiet frames at the window's start / end, whatever min_samples is; both n when no frame is loud */
};
int LINNEAmd_QuietWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        const struct LINNEAmdQuietSpec *specs /* [num_windows] */, struct LINNEAmdQuiet *answers /* [num_windows], out */,
        uint32_t num_windows, uint32_t group_frames);

/* ---- histogramming the sample levels of windows of resident streams: how are the magnitudes distributed?  No PCM written ----
 * LINNEAmd_HistogramWindowsDevice takes the windows of LINNEAmd_DecodeWindowsDevice and, instead of writing every window's samples,
 * counts them by level: the only output is a table of uint64_t counts per window, in device memory, num_bins of them per channel and
 * bucket.  The samples are exactly those LINNEAmd_DecodeStreamDevice writes for the range -- int32, L/R after MS, nothing saturated,
 * the zeros of SILENT blocks and of the range behind the stream's last block included.  The bin of a sample v: m = |v| >> shift, |v|
 * taken in 64 bits (INT32_MIN has magnitude 2^31); x = m for LINNE_AMD_HIST_LINEAR, x = the bit length of m for LINNE_AMD_HIST_LOG2
 * (0 for m == 0, otherwise floor(log2 m) + 1: INT32_MIN at shift 0 has x = 32); the bin is min(x, num_bins - 1), so the last bin
 * catches everything above.  Every count is exact, and the bins of one (channel, bucket) add up to the bucket's samples.
 * Buckets are LINNEAmd_MeasureWindowsDevice's: specs[i].bucket_samples = b > 0 gives nb = ceil(n / b) buckets, bucket k holding the
 * window's samples [k * b, min((k + 1) * b, n)) (the last one may be short); b == 0 is one bucket of the whole window; a window of no
 * samples has no buckets and nothing is written.  The windows of one call may differ in every field of their specs.
 * Everything LINNEAmd_MeasureWindowsDevice says about results holds unchanged: the windows' d_pcm and pcm_stride are ignored;
 * every window's `result` is what LINNEAmd_DecodeWindowsDevice gives it, and for that window alone INVALID_ARGUMENT when num_bins is 0
 * or above LINNE_AMD_HIST_MAX_BINS, shift > 31, scale is neither of the two, reserved != 0, d_out is NULL (with n > 0) or not 8-byte
 * aligned, channel_stride < nb, or nb > 2^32 - 1.  A failing window's d_out is never written, and a failing window does not disturb
 * the others.  No byte outside d_out[(ch * channel_stride + k) * num_bins + j], ch < channels, k < nb, j < num_bins, is written; the
 * outputs of different windows must not overlap; the streams are only read.  Shape groups, passes, group_frames, scratch and
 * whole-call failures are the decode call's, with "window <i>: " and the single call's text in GetLastError.  A pass has the decode
 * call's launches with kind 92 in place of kind 59; a call that takes at least one pass adds exactly two launches, whatever
 * num_windows is: kind 93 in front of the first pass (the accumulators zeroed) and kind 94 behind the last (the slots added up and the
 * tables of the windows whose Rice check passed written to their d_out); a window that spans passes collects its counts over them.
 * Copies (one upload, one fetch) and host synchronisations (one) are the measure call's.  The accumulators live in the context's
 * scratch: one 32-bit counter per (channel, bucket, bin) of every window -- a stream holds at most 2^32 - 1 samples, so none can
 * overflow -- half the bytes of the table itself -- times up to 64 for windows whose buckets are 8192 samples or longer (a bucket
 * of b samples has at most b / 4096 such copies: at most num_bins / 1024 bytes per sample and channel, a quarter of the int32 PCM).
 * num_windows == 0 is OK; a NULL ctx, or NULL windows or NULL specs with num_windows > 0, INVALID_ARGUMENT.  Enqueued on the
 * context's stream and synchronous. */
enum { LINNE_AMD_HIST_LINEAR = 0, LINNE_AMD_HIST_LOG2 = 1 };
#define LINNE_AMD_HIST_MAX_BINS 1024
struct LINNEAmdHistogramSpec {
    uint64_t bucket_samples;            /* 0: the whole window is one bucket */
    uint32_t num_bins;                  /* 1 .. LINNE_AMD_HIST_MAX_BINS */
    uint32_t shift;                     /* 0 .. 31 */
    uint32_t scale;                     /* LINNE_AMD_HIST_LINEAR / LINNE_AMD_HIST_LOG2 */
    uint32_t reserved;                  /* 0 */
    uint64_t *d_out;                    /* device, 8-byte aligned: bin j of channel ch, bucket k at d_out[(ch * channel_stride + k) * num_bins + j] */
    uint64_t channel_stride;            /* in buckets, >= the window's bucket count */
};
int LINNEAmd_HistogramWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        const struct LINNEAmdHistogramSpec *specs /* [num_windows] */, uint32_t num_windows, uint32_t group_frames);

/* ---- relating the channels of windows of resident streams: dual mono?  Polarity turned?  Correlation?  No PCM written ----
 * LINNEAmd_RelateWindowsDevice takes the windows of LINNEAmd_DecodeWindowsDevice and, instead of writing every window's samples,
 * reduces the products of its channels: the only output is a table of struct LINNEAmdRelation per window, in device memory, one
 * record per bucket and channel pair (i <= j) -- a Gram matrix per bucket, in exact integers.  The samples are exactly those
 * LINNEAmd_DecodeStreamDevice writes for the range -- int32, L/R after MS, nothing saturated, the zeros of SILENT blocks and of the
 * range behind the stream's last block included.  Per pair and bucket, over the bucket's sample frames: dot, the sum of a_i * a_j
 * as a 128-bit two's-complement integer (dot_hi * 2^64 + dot_lo; one product is at most 2^62 in magnitude, and no stream is long
 * enough to pass 2^127); num_equal, the frames with a_i == a_j; num_opposite, the frames with (int64)a_i + (int64)a_j == 0
 * (INT32_MIN is nobody's opposite, not even its own).  A frame of zeros counts in both.  The diagonal pairs are part of the table on
 * purpose: dot(i, i) is channel i's sum of squares (LINNEAmd_MeasureWindowsDevice's sumsq), num_equal(i, i) the bucket's frame count
 * and num_opposite(i, i) the channel's count of zero samples, so one call gives dot(i, j) / sqrt(dot(i, i) * dot(j, j)) without a
 * second decode.  The pairs are the upper triangle row by row: with C channels, LINNE_AMD_NUM_PAIRS(C) of them, pair (i, j) at
 * LINNE_AMD_PAIR(C, i, j) -- (0,0) (0,1) .. (0,C-1) (1,1) .. (C-1,C-1).
 * Buckets are LINNEAmd_MeasureWindowsDevice's: specs[i].bucket_samples = b > 0 gives nb = ceil(n / b) buckets, bucket k holding the
 * window's samples [k * b, min((k + 1) * b, n)) (the last one may be short); b == 0 is one bucket of the whole window; a window of no
 * samples has no buckets and nothing is written.  The windows of one call may differ in every field of their specs.
 * Everything LINNEAmd_MeasureWindowsDevice says about results holds unchanged: the windows' d_pcm and pcm_stride are ignored;
 * every window's `result` is what LINNEAmd_DecodeWindowsDevice gives it, and for that window alone INVALID_ARGUMENT when d_out is
 * NULL (with n > 0) or not 8-byte aligned, pair_stride < nb, or nb > 2^32 - 1.  A failing window's d_out is never written, and a
 * failing window does not disturb the others.  No byte outside d_out[p * pair_stride + k], p < LINNE_AMD_NUM_PAIRS(channels), k < nb,
 * is written; the outputs of different windows must not overlap; the streams are only read.  Shape groups, passes, group_frames,
 * scratch and whole-call failures are the decode call's, with "window <i>: " and the single call's text in GetLastError.  A pass has
 * the decode call's launches with kind 95 in place of kind 59; a call that takes at least one pass adds exactly two launches,
 * whatever num_windows is: kind 96 in front of the first pass (the accumulators zeroed) and kind 97 behind the last (the slots added
 * up with carries and the tables of the windows whose Rice check passed written to their d_out); a window that spans passes collects
 * its sums over them.  Copies (one upload, one fetch) and host synchronisations (one) are the measure call's.  The accumulators live
 * in the context's scratch: one struct LINNEAmdRelation per (pair, bucket) of every window -- the bytes of the table itself -- times
 * up to 64 for windows whose buckets are 8192 samples or longer (a bucket of b samples has at most b / 4096 such copies: at most
 * 32 * P / 4096 bytes per sample frame, under 0.3 bytes at 8 channels).  num_windows == 0 is OK; a NULL ctx, or NULL windows or NULL
 * specs with num_windows > 0, INVALID_ARGUMENT.  Enqueued on the context's stream and synchronous. */
#define LINNE_AMD_NUM_PAIRS(C)      ((C) * ((C) + 1u) / 2u)                      /* 36 at 8 channels */
#define LINNE_AMD_PAIR(C, i, j)     ((i) * (C) - (i) * ((i) - 1u) / 2u + ((j) - (i)))   /* i <= j < C: the upper triangle, row by row */
struct LINNEAmdRelation {               /* 32 bytes: one channel pair (i <= j) of one bucket of one window */
    uint64_t dot_lo; int64_t dot_hi;    /* the exact sum of a_i * a_j over the bucket's frames: a 128-bit two's-complement integer */
    uint64_t num_equal;                 /* frames with a_i == a_j */
    uint64_t num_opposite;              /* frames with (int64)a_i + (int64)a_j == 0 (INT32_MIN is nobody's opposite) */
};
struct LINNEAmdRelateSpec {
    uint64_t bucket_samples;            /* 0: the whole window is one bucket */
    struct LINNEAmdRelation *d_out;     /* device, 8-byte aligned: pair p, bucket k at d_out[p * pair_stride + k] */
    uint64_t pair_stride;               /* in buckets, >= the window's bucket count */
};
int LINNEAmd_RelateWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        const struct LINNEAmdRelateSpec *specs /* [num_windows] */, uint32_t num_windows, uint32_t group_frames);

/* ---- mixing the channels of windows of resident streams: a downmix, a channel swap, a polarity fix, on decode ----
 * LINNEAmd_MixWindowsDevice takes the windows and layouts of LINNEAmd_DecodeWindowsDeviceLayout and writes, instead of every window's C
 * channels, the Co = specs[i].out_channels channels its exact integer matrix makes of them.  With v[c] the values
 * LINNEAmd_DecodeStreamDevice gives for a sample frame, output channel o of that frame is
 *   1. the sum    acc = sum over c < C of (int64)coef[o][c] * v[c]   (a product is at most 2^46 in magnitude, eight of them 2^49:
 *                 nothing wraps);
 *   2. the shift  y = shift ? (acc + (1 << (shift - 1))) >> shift : acc, the shift arithmetic: halves round towards plus infinity;
 *   3. the clip   y clipped to [-2^(B - 1), 2^(B - 1) - 1], B = clip_bits, or 32 where clip_bits is 0;
 *   4. the layout's conversion of the clipped value, as LINNEAmd_DecodeWindowsDeviceLayout converts: S32 as it is, S16 and S24 saturated
 *      to the format's range, F32 (float)y * 2^-(Bf - 1), Bf = clip_bits, or the stream's bits_per_sample where clip_bits is 0.
 * layouts[i].saturated is 1 when step 3 or step 4 clipped an element of window i, otherwise 0; a failing window's stays as it was.
 * coef[o][c] with o >= Co or c >= C is never read into the result.  The identity matrix with shift 0 and clip_bits 0 writes what
 * LINNEAmd_DecodeWindowsDeviceLayout writes.
 * The rest of the contract is LINNEAmd_DecodeWindowsDeviceLayout's, word for word, with Co where that has the stream's channel count
 * in what it says of the output (the elements written, the layout's checks -- injectivity, alignment --, pcm_stride >= num_samples
 * when Co > 1 and layouts is NULL): per-window results ("window <i>: MixWindowsDevice: ..." for this call's own checks), a failing
 * window's memory never written and the others undisturbed, the lowest failing window's code returned, shape groups (the stream's
 * shape: windows of different C, Co and matrices share a pass), passes, group_frames, scratch, copies, the one host synchronisation
 * and whole-call failures.  For window i alone INVALID_ARGUMENT when out_channels is outside 1 .. 8, shift > 31, clip_bits is 1 or
 * above 32, or reserved is not 0.  A pass has the decode call's launches with kind 98 in place of kind 59 and nothing more, whatever
 * num_windows is.  num_windows == 0 is OK; a NULL ctx, or NULL windows or NULL specs with num_windows > 0, INVALID_ARGUMENT.
 * Enqueued on the context's stream and synchronous. */
struct LINNEAmdMixSpec {
    uint32_t out_channels;              /* Co, 1 .. 8 */
    uint32_t shift;                     /* 0 .. 31 */
    uint32_t clip_bits;                 /* 0 (32), or 2 .. 32 */
    uint32_t reserved;                  /* 0 */
    int16_t coef[LINNE_MAX_NUM_CHANNELS][LINNE_MAX_NUM_CHANNELS];       /* [o][c] */
};
int LINNEAmd_MixWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        const struct LINNEAmdMixSpec *specs /* [num_windows] */,
        struct LINNEAmdPcmLayout *layouts /* [num_windows] in/out; NULL: int32 planar, pcm_stride */,
        uint32_t num_windows, uint32_t group_frames);

/* ---- resampling windows of resident streams: a rational rate change L/M through an exact int16 polyphase FIR, on decode ----
 * LINNEAmd_ResampleWindowsDevice takes the windows and layouts of LINNEAmd_DecodeWindowsDeviceLayout, but a window's first_sample and
 * num_samples count OUTPUT samples of the resampled stream, which has LINNEAmd_ResampleLength(N, L, M) = ceil(N * L / M) samples, N the
 * header's num_samples, L = specs[i].up, M = specs[i].down.  With x[c][i] the values LINNEAmd_DecodeStreamDevice gives for channel c,
 * sample i of the stream, and x = 0 for i < 0 and i >= N, output sample m of channel c of the resampled stream is, with all index
 * arithmetic in 64 bits,
 *   1. the place  t = m * M, p = t % L, n = t / L;
 *   2. the sum    acc = sum over k < P of (int64)coef[p * P + k] * x[c][n - before + k], P = taps   (a product is at most 2^46 in
 *                 magnitude, 64 of them 2^52: nothing wraps);
 *   3. the shift, the clip and the layout's conversion: steps 2 to 4 of LINNEAmd_MixWindowsDevice, word for word, and its rule for
 *      layouts[i].saturated.
 * Zero-stuffed samples are never formed: this is the polyphase form.  With L = M = P = 1, coef = {1} and shift 0 the call writes what
 * LINNEAmd_DecodeWindowsDeviceLayout writes.  The output has the stream's channel count.  The rest of the contract is
 * LINNEAmd_DecodeWindowsDeviceLayout's: per-window results ("window <i>: ResampleWindowsDevice: ..." for this call's own checks), a
 * failing window's memory never written and the others undisturbed, the lowest failing window's code returned, shape groups, passes,
 * group_frames (which never changes a byte), copies, the one host synchronisation and whole-call failures -- with two rules adapted:
 * the range check uses the resampled length where that call uses N, and the index's failing block fails a window when it lies at or
 * before the last INPUT sample the window reads (sample n - before + P - 1 of its last output, or N - 1 where that lies behind the
 * stream).  For window i alone INVALID_ARGUMENT when up or down is outside 1 .. LINNE_AMD_RESAMPLE_MAX_RATIO, taps outside
 * 1 .. LINNE_AMD_RESAMPLE_MAX_TAPS, up * taps > LINNE_AMD_RESAMPLE_MAX_COEFS, before > taps - 1, shift > 31, clip_bits is 1 or above
 * 32, coef is NULL or reserved is not 0; these are checked in front of the range.  Windows with different specs, ratios and stream
 * shapes may share a call; windows that name the same (coef, up, taps) share one device copy of the table, which is read during the
 * call only.
 * Scratch: beside a pass's, the call keeps an int32 image of every live window's input range, halo included --
 * 4 * C * (n(last) - n(first) + P, rounded up to 4) bytes per window -- in the context's scratch; where that cannot be had the whole
 * call fails with NG and nothing is written.  A pass has the decode call's launches (its kind 59 writes the images); a call that takes
 * a pass adds one launch of kind 99 in front of the first pass and one of kind 100 behind the last, whatever num_windows, L, M and P
 * are.  num_windows == 0 is OK; a NULL ctx, or NULL windows or NULL specs with num_windows > 0, INVALID_ARGUMENT.  Enqueued on the
 * context's stream and synchronous. */
#define LINNE_AMD_RESAMPLE_MAX_TAPS   64      /* P: taps per phase */
#define LINNE_AMD_RESAMPLE_MAX_RATIO  1024    /* L and M */
#define LINNE_AMD_RESAMPLE_MAX_COEFS  16384   /* L * P */
struct LINNEAmdResampleSpec {
    uint32_t up, down;                  /* L, M: 1 .. LINNE_AMD_RESAMPLE_MAX_RATIO; need not be coprime */
    uint32_t taps;                      /* P: 1 .. LINNE_AMD_RESAMPLE_MAX_TAPS */
    uint32_t before;                    /* 0 .. P - 1: input samples the filter reaches back */
    uint32_t shift;                     /* 0 .. 31 */
    uint32_t clip_bits;                 /* 0 (32), or 2 .. 32, as in struct LINNEAmdMixSpec */
    uint64_t reserved;                  /* 0 */
    const int16_t *coef;                /* HOST memory, [L][P]: coef[p * P + k] */
};
int LINNEAmd_ResampleWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        const struct LINNEAmdResampleSpec *specs /* [num_windows] */,
        struct LINNEAmdPcmLayout *layouts /* [num_windows] in/out; NULL: int32 planar, pcm_stride */,
        uint32_t num_windows, uint32_t group_frames);
/* ceil(num_samples * up / down), 0 where down is 0; the product is formed in 128 bits, and a quotient no uint64 holds gives UINT64_MAX */
uint64_t LINNEAmd_ResampleLength(uint64_t num_samples, uint32_t up, uint32_t down);
/* A filter for the call above: a Kaiser-windowed sinc prototype of up * taps points (beta 8) with its cutoff at the lower of the two
 * Nyquist rates, split into `up` phases of `taps` coefficients and quantised to int16 so that every phase sums to exactly 1 << *shift
 * (the rounding remainder goes to the phase's largest tap): a constant input gives the same constant.  *before centres the filter:
 * (taps - 1) / 2.  up, down and taps are checked as the spec's are (INVALID_ARGUMENT, as for a NULL pointer); otherwise OK.  Pure host
 * code: no device is needed. */
int LINNEAmd_ResampleDesign(uint32_t up, uint32_t down, uint32_t taps, int16_t *coef /* [up][taps] */, uint32_t *shift, uint32_t *before);

/* ---- overlaying windows of several resident streams: a mix-down, a fade, a crossfade at a join, on decode ----
 * LINNEAmd_OverlayWindowsDevice writes num_outputs outputs, each the sum of up to LINNE_AMD_OVERLAY_MAX_SOURCES sources: ranges of
 * indexed streams, each laid at an output sample of its own under a gain that moves linearly over its samples.  For source s, sample
 * i of its range (0 <= i < n_s = num_samples), the gain is
 *   g_s(i) = (gain_q32 + step_q32 * i) >> 32, the sum formed in 64 bits and the shift arithmetic: the floor.
 * g_s(0) and g_s(n_s - 1) must lie in [-32768, 32767]; the host checks both in 128 bits, and the ramp being linear every gain between
 * them lies there too: nothing in the kernel can wrap.  With x_s[c][j] the values LINNEAmd_DecodeStreamDevice gives for channel c,
 * sample j of source s's stream, output sample t of channel c is
 *   1. the sum    acc = sum over the sources with at_s <= t < at_s + n_s of (int64)g_s(t - at_s) * x_s[c][first_s + t - at_s]   (a
 *                 product is at most 2^46 in magnitude, 64 of them 2^52: nothing wraps); a sample no source covers has acc = 0;
 *   2. the shift, the clip and the layout's conversion: steps 2 to 4 of LINNEAmd_MixWindowsDevice, word for word, and its rule for
 *      layouts[i].saturated.  For F32 with clip_bits 0, Bf is the bits_per_sample of the stream of the output's first source.
 * One source with at = 0, gain_q32 = 1 << 32, step_q32 = 0, shift 0 and clip_bits 0 writes what LINNEAmd_DecodeWindowsDeviceLayout
 * writes.  The output has the channel count C its sources' streams share; the streams may differ in everything else (bits, block
 * size, preset, MS, rate), and two sources may name the same stream and overlap.  An output's d_pcm, pcm_stride and layouts[i] are
 * what a window's are in LINNEAmd_DecodeWindowsDeviceLayout, for num_samples samples of C channels: all of them are written, zeros
 * where no source lies.
 * Results: outputs[i].result.  For output i alone INVALID_ARGUMENT ("output <i>: OverlayWindowsDevice: ..." in GetLastError) when
 * num_sources is outside 1 .. LINNE_AMD_OVERLAY_MAX_SOURCES or sources is NULL, shift > 31, clip_bits is 1 or above 32, reserved (the
 * output's or a source's) is not 0, a source is NULL in index or d_stream or has num_samples 0, at + num_samples lies beyond the
 * output's num_samples (or wraps), a gain end lies outside int16, the sources' streams differ in channel count, d_pcm is NULL, or the
 * layout's checks (with C) fail.  These come first; every source is then checked as a struct LINNEAmdWindow of
 * LINNEAmd_DecodeWindowsDevice is ("output <i>: source <j>: ..."): its range, its index's failing block at or before its range, and,
 * on the device, its Rice codes.  An output fails with the code of its lowest-numbered failing source; a failing output's memory is
 * never written and the others are undisturbed; the call returns the lowest failing output's code.  Whole-call failures are the decode
 * call's.
 * Every source is a window of the decode call's plan: shape groups, passes, group_frames (which never changes a byte), copies and the
 * one host synchronisation are that call's, over all sources of all outputs.  The passes place every source's samples into an int32
 * image in the context's scratch -- 4 * C * (n_s rounded up to 4) bytes per source --; where that cannot be had the whole call fails
 * with NG and nothing is written.  A pass has the decode call's launches (its kind 59 writes the images); a call that takes a pass
 * adds one launch of kind 101 behind the last pass and nothing else, whatever the numbers of outputs and sources are.
 * num_outputs == 0 is OK; a NULL ctx, or NULL outputs with num_outputs > 0, INVALID_ARGUMENT.  Enqueued on the context's stream and
 * synchronous. */
#define LINNE_AMD_OVERLAY_MAX_SOURCES 64
struct LINNEAmdOverlaySource {          /* 64 bytes */
    const struct LINNEAmdStreamIndex *index;    /* as in struct LINNEAmdWindow */
    const uint8_t *d_stream;
    uint64_t first_sample, num_samples; /* the source's range in ITS stream; num_samples >= 1 */
    uint64_t at;                        /* the output sample its first sample lands on */
    int64_t gain_q32, step_q32;         /* the gain at its first sample and its change per sample, in units of 2^-32 */
    uint64_t reserved;                  /* 0 */
};
struct LINNEAmdOverlay {
    const struct LINNEAmdOverlaySource *sources; uint32_t num_sources;  /* HOST memory; 1 .. LINNE_AMD_OVERLAY_MAX_SOURCES */
    uint32_t shift, clip_bits, reserved;        /* as in struct LINNEAmdMixSpec */
    uint64_t num_samples;               /* of the output */
    int32_t *d_pcm; uint64_t pcm_stride;        /* as in struct LINNEAmdWindow, when layouts is NULL */
    int32_t result;                     /* out */
};
int LINNEAmd_OverlayWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdOverlay *outputs,
        struct LINNEAmdPcmLayout *layouts /* [num_outputs] in/out; NULL: int32 planar, pcm_stride */,
        uint32_t num_outputs, uint32_t group_frames);

/* ---- sliding one resident stream over another: the exact lag correlation, which finds the `at` an overlay needs ----
 * LINNEAmd_LagWindowsDevice answers num_probes probes.  A probe slides n = num_samples samples of stream A, the needle, from
 * first_a on, over stream B, the haystack, at the num_lags lags L = lag_first + l, 0 <= l < num_lags, for num_pairs channel pairs
 * (ca, cb) = (chan_a[p], chan_b[p]).  With a[c][j] and b[c][j] the values LINNEAmd_DecodeStreamDevice gives for the two streams, and
 * b = 0 FOR EVERY j OUTSIDE [0, N_b), N_b the sample count of B's header -- a range off the haystack's ends is no error --, record
 * (p, l) of the table holds
 *   dot  = sum over i < n of a[ca][first_a + i] * b[cb][first_b + L + i]       a 128-bit two's-complement sum, dot_hi * 2^64 + dot_lo;
 *   b_sq = sum over i < n of b[cb][first_b + L + i]^2                          unsigned 128 bits;
 * and d_a_sq, where it is given, gets a_sq = sum over i < n of a[ca][first_a + i]^2 once per pair, low word then high word: the three
 * give the exact dot / sqrt(a_sq * b_sq) of every lag without a second decode.  Every index is formed in 128 bits on the host; A and
 * B may be one stream (the autocorrelation), a pair may name a channel twice, and two pairs may be the same.
 * Results: probes[i].result.  For probe i alone INVALID_ARGUMENT ("probe <i>: LagWindowsDevice: ..." in GetLastError) when a pointer
 * (index_a, d_stream_a, index_b, d_stream_b, d_out) is NULL, reserved is not 0, num_samples is 0, num_lags is 0 or above
 * LINNE_AMD_LAG_MAX_LAGS, num_pairs is outside 1 .. 8, num_samples * num_lags * num_pairs is above LINNE_AMD_LAG_MAX_PRODUCTS (which
 * keeps one mistaken call from occupying a shared device for minutes: the device multiplies num_samples * num_pairs * (num_lags rounded
 * up to 64) times, a wave of 64 lags being the least it works on, so at most 64 times the products counted), a channel is not one of its stream's, d_out or d_a_sq is not
 * 8-byte aligned, or pair_stride < num_lags.  These come first.  A is then checked as a struct LINNEAmdWindow of
 * LINNEAmd_DecodeWindowsDevice is ("probe <i>: needle: ..."): its range, its index's failing block at or before its range and, on the
 * device, its Rice codes; B likewise ("probe <i>: haystack: ...") for the part of [first_b + lag_first, first_b + lag_first +
 * num_lags - 1 + n) that lies inside [0, N_b).  A probe whose B range misses the stream entirely is valid and writes zeros; its A is
 * still decoded, for a_sq.  A failing probe's memory is never written and the others are undisturbed; the call returns the lowest
 * failing probe's code.  No byte outside the table elements named above is written; the streams are only read.  Whole-call failures
 * are the decode call's.
 * Every probe brings one or two windows into the decode call's plan -- A's range and B's clipped range --: shape groups, passes,
 * group_frames (which never changes a byte), copies and the one host synchronisation are that call's.  The passes place the windows
 * into int32 images in the context's scratch, 4 * C * (samples rounded up to 4) bytes each, beside 16 bytes of partial sums per lag of
 * every tile (a probe's pair, 256 lags, 65536 needle samples) and 32 per tile; where that cannot be had the whole call fails with NG and nothing is
 * written.  A pass has the decode call's launches (its kind 59 writes the images); a call that takes a pass adds one launch of kind
 * 102 and one of kind 103 behind the last pass and nothing else, whatever the numbers of probes, pairs and lags are.  No atomics: a
 * tile writes its own partial sums, and the result does not depend on scheduling.
 * num_probes == 0 is OK; a NULL ctx, or NULL probes with num_probes > 0, INVALID_ARGUMENT.  Enqueued on the context's stream and
 * synchronous. */
#define LINNE_AMD_LAG_MAX_LAGS 65536u
#define LINNE_AMD_LAG_MAX_PRODUCTS ((uint64_t)1 << 38)
struct LINNEAmdLagSum {                 /* 32 bytes: one channel pair at one lag */
    uint64_t dot_lo; int64_t dot_hi;    /* the sum of a * b: dot_hi * 2^64 + dot_lo */
    uint64_t b_sq_lo; uint64_t b_sq_hi; /* the sum of b^2 under the needle at this lag */
};
struct LINNEAmdLagProbe {
    const struct LINNEAmdStreamIndex *index_a; const uint8_t *d_stream_a;       /* the needle's stream, as in struct LINNEAmdWindow */
    uint64_t first_a, num_samples;      /* the needle's range, num_samples >= 1, inside stream A */
    const struct LINNEAmdStreamIndex *index_b; const uint8_t *d_stream_b;       /* the haystack; may be stream A */
    uint64_t first_b; int64_t lag_first; uint32_t num_lags;     /* lags lag_first .. lag_first + num_lags - 1 */
    uint32_t num_pairs; uint8_t chan_a[8], chan_b[8];   /* 1 .. 8 channel pairs */
    struct LINNEAmdLagSum *d_out; uint64_t pair_stride; /* device, 8-byte aligned: pair p, lag l at d_out[p * pair_stride + l] */
    uint64_t *d_a_sq;                   /* device, 8-byte aligned, or NULL: [num_pairs][2], low word then high word */
    uint64_t reserved;                  /* 0 */
    int32_t result;                     /* out */
};
int LINNEAmd_LagWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdLagProbe *probes, uint32_t num_probes, uint32_t group_frames);

/* ---- projecting frames of windows of resident streams on int16 basis rows: an exact STFT, a filter bank, a band-energy front end ----
 * LINNEAmd_ProjectWindowsDevice cuts a stream into overlapping frames of N = frame_len samples, H = hop samples apart, and writes every
 * frame's inner product with each of K = num_rows rows of an int16 basis: a frames x rows table per channel.  A window's first_sample
 * and num_samples count output FRAMES of its stream, which has LINNEAmd_ProjectLength(N_s, H) = ceil(N_s / H) of them, N_s the header's
 * num_samples (this is how LINNEAmd_ResampleWindowsDevice counts outputs); d_pcm is the output's base, an int32_t* or a float*, and
 * pcm_stride is ignored.  With x[c][i] the values LINNEAmd_DecodeStreamDevice gives for channel c, sample i of the stream, and x = 0 for
 * i < 0 and i >= N_s, element (c, f, k) -- channel c, frame f of the stream, row k -- is
 *   1. the sum    acc = sum over n < N of (int64)basis[k * N + n] * x[c][f * H - before + n], the index arithmetic in 64 bits   (a
 *                 product is at most 2^46 in magnitude, 4096 of them 2^58: nothing wraps);
 *   2. the shift  y = shift ? (acc + (1 << (shift - 1))) >> shift : acc, the shift arithmetic: halves round towards plus infinity;
 *   3. the clip   y clipped to [-2^(B - 1), 2^(B - 1) - 1], B = clip_bits, or 32 where clip_bits is 0
 *                 (steps 2 and 3 of LINNEAmd_MixWindowsDevice, word for word);
 *   4. the store  LINNE_AMD_PCM_S32 stores y; LINNE_AMD_PCM_F32 stores (float)y, rounded to nearest-even, times 2^-float_exp, which is
 *                 exact scaling;
 * at d_pcm[c * channel_stride + (f - first_sample) * frame_stride + k * row_stride], in elements.  specs[i].saturated is 1 when step 3
 * changed an element of window i, otherwise 0; a failing window's stays as it was.
 * For window i alone INVALID_ARGUMENT ("window <i>: ProjectWindowsDevice: ...") when frame_len, hop or num_rows is outside 1 .. its
 * LINNE_AMD_PROJECT_MAX_*, before > frame_len - 1, shift > 31, clip_bits is 1 or above 32, format is neither S32 nor F32, float_exp > 63
 * or nonzero with S32, reserved is not 0, basis is NULL, d_pcm is NULL or not 4-byte aligned, frames * K * N * C (formed in 128 bits) is
 * above LINNE_AMD_PROJECT_MAX_PRODUCTS, or the output map is not injective: with the three (stride, extent) pairs -- extents C,
 * num_samples and K -- sorted by stride and pairs of extent 1 left out, the smallest stride must be at least 1 and each later one at
 * least the one before it times that one's extent.  These come in front of the range check, which uses LINNEAmd_ProjectLength; the
 * index's failing block fails a window when it lies at or before the last INPUT sample the window reads,
 * min(N_s - 1, (first_sample + num_samples - 1) * H - before + N - 1).  Halo samples off either end of the stream are zeros, not errors.
 * The rest of the contract is LINNEAmd_DecodeWindowsDeviceLayout's: per-window results, a failing window's memory never written and the
 * others undisturbed, the lowest failing window's code returned, shape groups, passes, group_frames (which never changes a byte), the
 * one host synchronisation and whole-call failures.  Windows with different specs and stream shapes may share a call; windows that name
 * the same (basis, K, N) share one device copy of the table, which is read during the call only.
 * Scratch: beside a pass's, the call keeps an int32 planar image of every live window's input range, halo included -- 4 * C * (span
 * rounded up to 4) bytes, span = (num_samples - 1) * H + N -- and its tables as digit planes (2 * (K rounded up to 16) * (N rounded up
 * to 64) bytes each) in the context's scratch; where that cannot be had the whole call fails with NG and nothing is written.  A pass has
 * the decode call's launches (its kind 59 writes the images); a call that takes a pass adds one launch of kind 104 in front of the
 * first pass and one of kind 105 behind the last, whatever the numbers of windows, frames, rows and taps are.  num_windows == 0 is OK; a
 * NULL ctx, or NULL windows or NULL specs with num_windows > 0, INVALID_ARGUMENT.  Enqueued on the context's stream and synchronous. */
#define LINNE_AMD_PROJECT_MAX_FRAME   4096u                   /* N */
#define LINNE_AMD_PROJECT_MAX_ROWS    2048u                   /* K */
#define LINNE_AMD_PROJECT_MAX_HOP     65536u                  /* H */
#define LINNE_AMD_PROJECT_MAX_PRODUCTS ((uint64_t)1 << 40)    /* frames * K * N * C of one window */
struct LINNEAmdProjectSpec {
    uint32_t frame_len, hop, num_rows;  /* N, H, K */
    uint32_t before;                    /* 0 .. N - 1: samples a frame reaches back from f * H */
    uint32_t shift, clip_bits;          /* as in struct LINNEAmdMixSpec */
    uint32_t format;                    /* LINNE_AMD_PCM_S32 or LINNE_AMD_PCM_F32 only */
    uint32_t float_exp;                 /* 0 .. 63: F32 = (float)y * 2^-float_exp */
    uint64_t channel_stride, frame_stride, row_stride;   /* elements: (c, f, k) -> d_pcm[c*cs + (f - first)*fs + k*rs] */
    uint32_t saturated;                 /* out */
    uint32_t reserved;                  /* 0 */
    const int16_t *basis;               /* HOST memory, [K][N] */
};
int LINNEAmd_ProjectWindowsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdWindow *windows,
        struct LINNEAmdProjectSpec *specs /* [num_windows], in/out */, uint32_t num_windows, uint32_t group_frames);
/* ceil(num_samples / hop), 0 where hop is 0 */
uint64_t LINNEAmd_ProjectLength(uint64_t num_samples, uint32_t hop);
/* A DFT basis for the call above: row 2 j is round_half_even(32767 * w[n] * cos(2 pi j n / N)), row 2 j + 1 is
 * round_half_even(-32767 * w[n] * sin(2 pi j n / N)), j < bins, n < N = frame_len; window 0: w = 1 (rectangular), 1: the periodic Hann
 * window w[n] = 0.5 - 0.5 cos(2 pi n / N).  Needs 1 <= frame_len <= LINNE_AMD_PROJECT_MAX_FRAME, 1 <= bins <= N / 2 + 1,
 * 2 * bins <= LINNE_AMD_PROJECT_MAX_ROWS and window 0 or 1; INVALID_ARGUMENT otherwise, and for a NULL pointer.  Pure host code: no
 * device is needed. */
int LINNEAmd_ProjectDesign(uint32_t frame_len, uint32_t bins, uint32_t window /* 0 rectangular, 1 periodic Hann */,
        int16_t *basis /* [2*bins][frame_len] */);

/* ---- cutting and joining resident streams, re-encoding only the blocks a cut goes through ----
 * LINNEAmd_SpliceStreamsDevice writes num_splices output streams, each made of the cuts of indexed streams it names.  The decoder
 * carries nothing from one block to the next (linne_decoder.c:564-668: a block brings its own sample count, parameters and
 * de-emphasis history), so a stream that keeps untouched blocks byte for byte is a valid .lnn stream; only the blocks a cut's ends
 * lie inside are decoded and encoded again.
 * The stream: output k holds the 30 bytes LINNEEncoder_EncodeHeader writes from the header of its first cut's stream with num_samples
 * set to the sum of its cuts, then, cut by cut and in sample order, one block per source block the cut overlaps:
 *   - a source block that lies wholly inside the cut is its size + 6 bytes, unchanged (COMPRESS, SILENT and RAW alike);
 *   - a source block the cut covers partly becomes one new block of exactly the covered samples: bytes [30, end) of what
 *     LINNEEncoder_EncodeWhole writes on a fresh encoder (quirk Q2: its parcor state starts at 0.0) for those samples alone, with the
 *     stream's shape and the context's -a / -l settings (LINNEAmd_SetAfIterations / SetLearning).
 * A cut inside one source block gives one such block; the neighbouring edge blocks of two cuts are not merged; a cut of 0 samples
 * contributes nothing.  An edge block of no more samples than the preset's largest layer (32 at -m 0..1, 64 at -m 2..4, 128 at -m
 * 5..7) is outside the contract, as such a tail is for the encoder (the reference's own encoder crashes on it); this call refuses an
 * output that needs one with INVALID_ARGUMENT.
 * Per output, for it alone (`result`):
 *   - INVALID_ARGUMENT: a NULL d_out, cuts, index or d_stream; a d_out that is not 4-byte aligned; an index of another device;
 *     num_cuts == 0 or 0 samples in all; more than 2^32 - 1 samples in all; a cut beyond its stream's num_samples, or beyond the
 *     samples the blocks of an undamaged stream reach; cuts whose streams differ in channels, bits, rate, block size, preset or MS;
 *     an edge block outside the contract (above).  These are checked first, over all cuts of the output;
 *   - then damage, cut by cut: the code of the index's failing block when that block lies at or before the last block the cut
 *     overlaps (LINNEAmd_DecodeStreamDevice's rule: damage behind the cut does not matter).  An edge block whose Rice codes do not
 *     end where its size field says gives DecodeStreamDevice's LINNE_APIRESULT_NG;
 *   - an edge block the encoder refuses gives the code LINNEAmd_EncodeStreamDevice gives for it;
 *   - INSUFFICIENT_BUFFER with the needed size in out_bytes when the stream is longer than `capacity` (or than 2^32 - 1 bytes).
 * A failing output has no byte of d_out written and out_bytes 0 (INSUFFICIENT_BUFFER: the needed size), copied_blocks and
 * encoded_blocks 0, and does not disturb the others.  On OK, copied_blocks and encoded_blocks count the output's blocks of either kind.
 * The call returns LINNE_APIRESULT_OK when every output is OK, otherwise the result of the lowest-numbered failing output;
 * GetLastError then reads "splice <i>: " and that output's text.  A HIP error or running out of memory fails the whole call:
 * LINNE_APIRESULT_NG, in every `result` too.  num_splices == 0 is OK; a NULL ctx, or NULL splices with num_splices > 0,
 * INVALID_ARGUMENT.
 * Cost: the edge blocks of all outputs are decoded by ONE LINNEAmd_DecodeWindowsDevice call and encoded by ONE
 * LINNEAmd_EncodeStreamsDevice call, whose passes cost what those calls document (an analysis call per 16 distinct edge lengths of a
 * pass); group_frames is handed to both and never changes a byte.  Behind them one copy launch (kind 71) places every run of bytes
 * of every output -- a cut's whole blocks are contiguous in their source: one run; an edge block: one run -- and one launch (kind 72)
 * writes the headers, after one upload; then the call's one wait.  Launches, copies, waits and allocations of the call's own steps
 * do not depend on the number of outputs or cuts.  Scratch (kept by the context, grown with a wait and an allocation more when a
 * call needs more than any before it): per edge block its samples as int32 and EncodeStreamBound's bytes, 32 bytes per run, 40 per
 * output.  LINNEAmd_GetLastStreamEncodeCount / GetLastStreamBatchCount report the edge blocks' encode.
 * Memory: no byte outside [0, stream_bytes) of a source is read, no byte outside [0, out_bytes) of an output is written.  d_out
 * must be 4-byte aligned; the outputs must not overlap each other or any source.  Enqueued on the context's stream and synchronous.
 * LINNEAmd_GetLastSpliceCount: of the last such call, which = 0 the outputs written, 1 their copied blocks, 2 their re-encoded
 * blocks, 3 the copy runs, 4 the bytes they moved, 5 the host synchronisations of the call's own steps (1 once the scratch has grown;
 * the two calls above add theirs); -1 for a NULL ctx or any other `which`. */
struct LINNEAmdCut {                            /* samples [first_sample, first_sample + num_samples) of one indexed stream */
    const struct LINNEAmdStreamIndex *index;    /* of the stream below, same device as the context */
    const uint8_t *d_stream;                    /* the stream's device bytes, any alignment */
    uint64_t first_sample, num_samples;
};
struct LINNEAmdSplice {                         /* one output stream: its cuts, in order */
    const struct LINNEAmdCut *cuts; uint32_t num_cuts;
    uint8_t *d_out; uint64_t capacity;          /* 4-byte aligned; outputs do not overlap each other or any source */
    uint64_t out_bytes;                         /* out */
    uint32_t copied_blocks, encoded_blocks;     /* out */
    int32_t result;                             /* out: this output's LINNEApiResult */
};
int LINNEAmd_SpliceStreamsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdSplice *splices, uint32_t num_splices, uint32_t group_frames);
int64_t LINNEAmd_GetLastSpliceCount(struct LINNEAmdContext *ctx, int which);

/* ---- repairing damaged resident streams: sound blocks kept byte for byte, lost stretches replaced by SILENT blocks ----
 * The index and every call on it stop at the first damaged block (LINNEAmd_DecodeStreamDevice: "damage before [the range] does"
 * matter), as the reference's decoder does.  LINNEAmd_RepairStreamsDevice turns num_streams damaged streams into valid .lnn streams:
 * the index finds no failing block in an output, LINNEAmd_DecodeWindowsDevice and LINNEAmd_SpliceStreamsDevice take it, the reference
 * decodes it.  It rests on what the splice call rests on: a block brings everything its decoding needs, so a stream that keeps
 * untouched blocks and holds blocks of fewer than S samples between them is a valid stream.
 * Per stream (N: the header's sample count, S its block size, C its channels):
 *   1. Header.  Read as LINNEAmd_StreamIndexCreate reads it; a header error is that stream's result, with the index's code, nothing
 *      is written and out_bytes is 0.  A damaged header is out of scope.
 *   2. Sound block.  A candidate is a position p >= 30 that passes the checks lnn's block parser makes before the CRC with
 *      left = stream_bytes - p: FF FF, size + 6 <= left, size >= 5.  It is sound when size + 6 <= B, its CRC16 matches, and it passes
 *      the parser's checks behind the CRC with the room replaced by S: type 0 .. 2, 1 <= samples <= S, a RAW block at 8, 16 or 24
 *      bits, a RAW or SILENT payload exactly as long as the size field says.
 *      B bounds the bytes the reference's encoder can write for one block of the stream's shape:
 *          B = 11 + ceil(C * (2 * (bits + 5) + 7 * L + 32 * P + 15 + 36 * S) / 8)
 *      with L the layers and P the coefficients per channel of the header's preset (DESIGN.md derives it).  It keeps the CRC work
 *      linear in the stream: a false candidate carries a random size field.  A true block larger than B -- none the reference's
 *      encoder or this library's writes -- is treated as damage.
 *   3. The salvage chain.  Its first block is the lowest sound candidate; the block behind a block at p with size field z is the
 *      lowest sound candidate at byte >= p + z + 6.  The chain stops before the block with which the kept samples would exceed N (as
 *      the decoder's loop stops at N); what lies behind is dropped and is no gap.  On an undamaged stream this is the index's chain.
 *   4. Gaps.  A gap lies before the first kept block when that is not at byte 30, between two kept blocks that are not adjacent, and
 *      behind the last kept block when the kept samples are fewer than N and bytes lie behind it or there is no other gap (alone, this
 *      trailing gap may hold 0 bytes: a stream cut at a block boundary; where a gap lies before a last block that ends the stream, that
 *      gap stands for the missing samples; a stream without a sound block is one trailing gap from byte 30 on).  M = N - kept samples are lost in all.  One
 *      gap gets all of M and exact = 1.  Several gaps: gap i of b_i source bytes gets floor(M * b_i / sum b), the last gap the
 *      remainder (with sum b == 0, everything), and exact = 0: the kept runs between the gaps are then placed by estimate, not by
 *      proof.  A gap given 0 samples gets no fill: junk bytes between sound blocks are dropped.  No gap: exact = 1.
 *   5. Fill.  A gap of g samples becomes ceil(g / min(S, 65535)) SILENT blocks of 11 bytes (size field 5), every one full but the
 *      last.
 *   6. Output.  The source's 30 header bytes, then kept runs and fills in order.  It holds out_bytes bytes; when capacity is smaller
 *      (or the output longer than 2^32 - 1 bytes) the result is LINNE_APIRESULT_INSUFFICIENT_BUFFER, out_bytes the size needed, no
 *      byte is written and the other out fields are 0.  Damage is no failure: a stream with gaps returns OK and the out fields say
 *      what happened; a stream without a sound block returns OK with kept_blocks = 0.
 *   7. An undamaged stream whose blocks reach N gives bytes [0, end of the last block a whole decode walks) of the input,
 *      num_gaps = 0, exact = 1.
 * Two limits.  A CRC-valid block whose Rice codes do not end where the block does is kept as it is: the output then fails where the
 * input did.  A false candidate inside a LOST stretch passes CRC16 with chance 2^-16 and is then kept as a block (inside a sound
 * block it is skipped: the chain continues behind that block's end).
 * A NULL d_stream or d_out is that stream's INVALID_ARGUMENT.  d_out may lie at any alignment; the outputs must not overlap each
 * other or any source.  Streams of different shapes may be mixed; streams may lie at any alignment and be adjacent views of one
 * buffer: every read of stream i is a byte load inside [0, stream_bytes[i]), no byte outside [0, out_bytes) of an output is written.
 * A failing stream does not disturb the others.  The call returns LINNE_APIRESULT_OK when every stream is OK, otherwise the result of
 * the lowest-numbered failing stream; GetLastError then reads "repair <i>: " and that stream's text.  A HIP error or running out of
 * memory fails the whole call: LINNE_APIRESULT_NG, in every `result` too.  num_streams == 0 is OK; a NULL ctx, or NULL streams with
 * num_streams > 0, INVALID_ARGUMENT.
 * Cost: kernel launches, copies, host synchronisations (five once the scratch has grown) and device allocations do not depend on
 * the number of streams or gaps; only the pointer-doubling depth K does on the streams (the batch index's K: K - 1 launches of kind
 * 41).  One copy launch (kind 71) places every run and fill of every output, after one upload of the fill bytes and the run table.
 * Scratch is kept by the context and grown as the batch index grows it: about 120 + 4 K bytes per candidate.  Enqueued on the
 * context's stream and synchronous.
 * LINNEAmd_GetLastRepairGaps: the gaps of stream i of the context's last repair call (none for a failing stream), valid until its
 * next one.  LINNEAmd_GetLastRepairCount: of the last such call, which = 0 the outputs written, 1 their kept blocks, 2 their fill
 * blocks, 3 their gaps, 4 the copy runs, 5 its host synchronisations, 6 its kernel launches; -1 for a NULL ctx or any other `which`. */
struct LINNEAmdGap {
    uint64_t first_sample, num_samples;         /* in the output's timeline */
    uint64_t src_offset, src_bytes;             /* the bytes of the source it stands for */
    uint32_t fill_blocks, reserved;             /* the SILENT blocks written for it */
};
struct LINNEAmdRepair {
    const uint8_t *d_stream; uint64_t stream_bytes;     /* the damaged stream's device bytes, any alignment */
    uint8_t *d_out; uint64_t capacity;
    uint64_t out_bytes, lost_samples;           /* out */
    uint32_t kept_blocks, fill_blocks, num_gaps, exact;     /* out */
    int32_t result;                             /* out: this stream's LINNEApiResult */
};
int LINNEAmd_RepairStreamsDevice(struct LINNEAmdContext *ctx, struct LINNEAmdRepair *streams, uint32_t num_streams);
int LINNEAmd_GetLastRepairGaps(struct LINNEAmdContext *ctx, uint32_t stream, const struct LINNEAmdGap **gaps, uint32_t *num_gaps);
int64_t LINNEAmd_GetLastRepairCount(struct LINNEAmdContext *ctx, int which);

#ifdef __cplusplus
}
#endif

#endif /* LINNE_AMD_H_INCLUDED */
