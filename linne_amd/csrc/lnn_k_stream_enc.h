/* lnn_k_stream_enc.h -- encoding PCM that lies in device memory into .lnn streams in device memory
 * (LINNEAmd_EncodeStreamsDevice, and LINNEAmd_EncodeStreamDevice as its one-track case; DESIGN.md section 5, "Encoding into a
 * stream in HBM" and "Encoding many tracks in one call").
 *
 * Per pass of frames (between the analysis and the writers sits the one host step: block types, flagged Rice plans):
 *   k_sb_gather    the input (int32 planar, or any struct LINNEAmdPcmLayout: int16 / packed 24-bit, interleaved, padded) -> the
 *                  [F][C][S] frame layout of the analysis, a track's last frame zero-padded; per frame a flag "some sample is not
 *                  0" (the SILENT test of the block-type decision)
 *   k_se_compact   each channel-frame's plan flag, partition order and code length in 8 bytes (what the host step reads)
 *   k_se_size      each block's size, where each channel's Rice code starts in it, and the host stitcher's per-block errors
 *   k_sx_scan      (lnn_k_stream.h) the blocks' offsets
 *   k_se_params    the parameter bits of every COMPRESS block (linne_encoder.c:698-735), a lane per block
 *   k_se_rice      every channel's Rice code at its final bit position (k_rice_emit with the writer started at any bit)
 *   k_se_raw       RAW payloads: zig-zag, big-endian, channels interleaved (linne_encoder.c:532-591)
 *   k_se_crc       a wave per block: CRC16 over [p + 8, p + 6 + size) from lane partials, then the 11 header bytes
 *
 * The shared-word rule.  The region of a pass is zeroed before the writers run, and bits are ORed into it.  Neighbouring bit
 * fields -- one channel's code and the next, the parameter bits and the first code of a block -- share 32-bit words, and the
 * workgroups that write them may sit on different XCDs.  So every word a writer may share is written with atomicOr (a
 * device-scope vector global atomic); a plain store goes only to a word whose 32 bits all belong to the writing thread (RiceBW's
 * rule).  Byte stores (RAW payloads, block headers) go to bytes no other writer of the same launch touches: a RAW payload shares
 * no word with any code (11 header bytes lie between blocks), and the header bytes, whose words the codes of the block before and
 * after may share, are written by k_se_crc, a launch of its own after every writer of the pass.
 *
 * Rows, slots and tracks.  The rows of a pass are frames of one or several tracks, full frames first, the ragged ones sorted by
 * length behind them; a per-row table (SbRow: the track, the row's slot in stream order, the frame's first sample) and a per-track
 * table (SbTrack) connect rows to streams.  The analysis, the Rice plan and every kernel above work per row; sizes, statuses and
 * offsets are indexed by SLOT, so that the scan runs over stream order, and the writers place a row at
 * track.out + track.pos + (off[slot] - off[track.slot0]) and skip the rows of a track that is not written.  Beside them:
 *   k_sb_reduce    a wave per track of the pass: its bytes, its lowest failing block and that block's status (one copy to the host)
 *   k_sb_zero      zeroes exactly [pos, pos + bytes) of every written track: whole words where all four bytes are the region's,
 *                  byte stores at its edges
 *   k_sb_header    the 30 header bytes of every finished track, from an uploaded table, by byte stores
 * The shared-word rule holds unchanged inside a track.  Across tracks it holds because the tracks' buffers are 4-byte aligned and
 * do not overlap: a 32-bit word belongs to one track only, and the one word two launches of a track may both touch by bytes (the
 * edge of a pass's region, the word holding header bytes 28-29 and stream bytes 30-31) is touched by launches that follow each
 * other on the stream.
 */
#ifndef LNN_K_STREAM_ENC_H_INCLUDED
#define LNN_K_STREAM_ENC_H_INCLUDED

#include "lnn_k_pcm_load.h"

#define SE_THREADS 256u

/* the device tables of the stream encoder: the decoder's (CRC byte table, shift matrices, Huffman tree) and the Huffman code */
struct SeTables {
    SxTables sx;
    uint32_t code[256];                 /* code word of each coefficient symbol (lnn_entropy.c huff_walk), its low len[sym] bits */
    uint8_t len[256];
};

/* the tables of a pass */
struct SbRow { uint32_t track, slot; uint64_t first; };        /* index into the pass's SbTrack table; slot in stream order; the frame's first sample in its track */
struct SbTrack {
    const void *pcm; uint64_t stride, total;                    /* element (ch, i) at pcm + (ch * stride + i * sstride) elements; samples per channel */
    uint8_t *out; uint64_t pos;                                 /* the track's stream and the byte at which this pass's blocks start */
    uint32_t slot0, nslots;                                     /* its slots in this pass: [slot0, slot0 + nslots) */
    uint32_t write, id;                                         /* write 0: the track is not written (it failed, or does not fit); id: its number in its shape group */
    uint64_t sstride; uint32_t fmt, pad;                        /* the layout: sample stride, LINNE_AMD_PCM_* (int32 planar: 1, S32) */
};
struct SbTrackOut { uint64_t bytes; uint32_t fail; int32_t status; };  /* of a track in a pass: bytes; lowest failing slot - slot0 (~0: none), its status */

struct SeGatherArgs {
    int32_t *frames;                            /* [F][C][S] */
    uint32_t *nonzero;                          /* [F], zeroed */
    uint32_t F, C, S;
};

/* (reading PCM of any layout: ly_word / ly_load4 / ly_load1 of lnn_k_pcm_load.h) */
/* Workgroup x of frame f's C, for a layout other than int32 with sample stride 1: the frame has n samples from `first` of a track
 * of `total`.  Returns "one of my samples is not 0".
 *   sample stride 1 (planar)   x is a channel: its n elements are contiguous and read four at a time (ly_load4) into row (f, x)
 *   otherwise                  x is a quarter-aligned C-th of the frame's samples with all their channels.  Packed interleaved
 *                              (channel stride 1, sample stride C): those are contiguous too, read four at a time and scattered to
 *                              the C rows; any other strides: element by element, the channels of a sample on neighbouring lanes
 * Samples n .. S of the rows are zeroed as the int32 planar path zeroes them. */
__device__ __forceinline__ int se_gather_layout(const void *pcm, uint32_t fmt, uint64_t cs, uint64_t ss, uint64_t total, uint64_t first,
        uint32_t n, int32_t *frames, uint32_t f, uint32_t x, uint32_t C, uint32_t S)
{
    const uint32_t es = fmt == LINNE_AMD_PCM_S16 ? 2u : (fmt == LINNE_AMD_PCM_S24 ? 3u : 4u);
    const uint8_t *base = (const uint8_t *)pcm;
    int32_t *rows = frames + (uint64_t)f * C * S;
    int any = 0;
    if (ss == 1u) {
        const uint8_t *lo = base + (uint64_t)x * cs * es, *hi = lo + total * es, *p = lo + first * es;
        int32_t *dst = rows + (uint64_t)x * S;
        for (uint32_t k0 = threadIdx.x * 4u; k0 < S; k0 += SE_THREADS * 4u) {
            int32_t v[4] = { 0, 0, 0, 0 };
            if (k0 < n) ly_load4(p + (uint64_t)k0 * es, lo, hi, fmt, (n - k0 < 4u) ? n - k0 : 4u, v);
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) if (k0 + i < S) { dst[k0 + i] = v[i]; any |= (v[i] != 0); }
        }
        return any;
    }
    const uint32_t chunk = ((S + C - 1u) / C + 3u) & ~3u, s_lo = x * chunk;
    if (s_lo >= S) return 0;
    const uint32_t s_hi = (S - s_lo < chunk) ? S : s_lo + chunk;
    const uint32_t ne = (s_hi - s_lo) * C, live = (n > s_lo) ? ((n < s_hi ? n : s_hi) - s_lo) * C : 0u;       /* elements to write, and those of them the track holds */
    if (cs == 1u && ss == C) {
        const uint8_t *lo = base, *hi = base + total * C * es, *p = base + (first + s_lo) * C * es;
        for (uint32_t k0 = threadIdx.x * 4u; k0 < ne; k0 += SE_THREADS * 4u) {
            int32_t v[4] = { 0, 0, 0, 0 };
            if (k0 < live) ly_load4(p + (uint64_t)k0 * es, lo, hi, fmt, (live - k0 < 4u) ? live - k0 : 4u, v);
            uint32_t smp = k0 / C, ch = k0 - smp * C;
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) {
                if (k0 + i < ne) { rows[(uint64_t)ch * S + s_lo + smp] = v[i]; any |= (v[i] != 0); }
                if (++ch == C) { ch = 0; smp++; }
            }
        }
        return any;
    }
    for (uint32_t k = threadIdx.x; k < ne; k += SE_THREADS) {
        const uint32_t smp = k / C, ch = k - smp * C;
        const int32_t v = (k < live) ? ly_load1(base + ((uint64_t)ch * cs + (first + s_lo + smp) * ss) * es, fmt) : 0;
        rows[(uint64_t)ch * S + s_lo + smp] = v;
        any |= (v != 0);
    }
    return any;
}

/* a workgroup per channel-frame: row f's source is its track's */
__global__ __launch_bounds__(SE_THREADS) void k_sb_gather(SeGatherArgs a, const SbRow *rows, const SbTrack *trk)
{
    const uint32_t cf = blockIdx.x, f = cf / a.C, ch = cf - f * a.C;
    const SbRow r = rows[f];
    const SbTrack &t = trk[r.track];
    const uint32_t n = (t.total - r.first < a.S) ? (uint32_t)(t.total - r.first) : a.S;
    int any = 0;
    if (t.fmt == LINNE_AMD_PCM_S32 && t.sstride == 1u) {
        const int32_t *src = (const int32_t *)t.pcm + (uint64_t)ch * t.stride + r.first;
        int32_t *dst = a.frames + (uint64_t)cf * a.S;
        for (uint32_t s = threadIdx.x; s < a.S; s += SE_THREADS) {
            const int32_t v = (s < n) ? src[s] : 0;
            dst[s] = v;
            any |= (v != 0);
        }
    } else any = se_gather_layout(t.pcm, t.fmt, t.stride, t.sstride, t.total, r.first, n, a.frames, f, ch, a.C, a.S);        /* block-uniform */
    if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(&a.nonzero[f], 1u);
}

/* out[cf] = (order | flag << 8, code length in bits) of k_rice_plan's record */
__global__ __launch_bounds__(SE_THREADS) void k_se_compact(const uint8_t *plan, uint32_t CF, uint2 *out)
{
    const uint32_t cf = blockIdx.x * SE_THREADS + threadIdx.x;
    if (cf >= CF) return;
    const uint8_t *rec = plan + (uint64_t)cf * LINNE_AMD_RICE_PLAN_BYTES;
    out[cf] = make_uint2((uint32_t)rec[0] | ((uint32_t)rec[1] << 8), *(const uint32_t *)(rec + LINNE_AMD_RICE_PLAN_NBITS));
}

__device__ __forceinline__ uint32_t se_zz(int32_t v) { const uint32_t d = (uint32_t)v << 1; return (v < 0) ? ((0u - d) - 1u) : d; }
__device__ __forceinline__ uint32_t se_ceil_log2(uint32_t x) { const uint32_t y = x - 1u; return y ? 32u - (uint32_t)__clz((int)y) : 0u; }

struct SeBlockArgs {
    const uint8_t *types; const uint32_t *nsmp;
    const int32_t *prm; const uint8_t *plan; const int32_t *resid; const SeTables *tab;
    uint32_t F, C, S, bits, L, P[LNN_MAXL], coef_off[LNN_MAXL];
    uint32_t *size;                     /* [F] bytes of each block (k_se_size) */
    int32_t *status;                    /* [F] LNN_* of each block (k_se_size) */
    uint32_t *fail;                     /* a word per track of the shape group, set when a Rice code's length is not its plan's */
    uint64_t *cfbit;                    /* [F * C] bit offset of each channel's code from its block's first byte */
    const uint64_t *off;                /* [F + 1] offsets of the slots' blocks from the first one's (k_sx_scan) */
    uint32_t xch;                       /* k_se_raw: workgroups per block */
    const SbRow *rows; const SbTrack *trk;      /* (size, status and off are indexed by slot, everything else by row) */
};

/* where row f's block goes: the stream, the block's first byte in it, the row's slot; false: the row's track is not written */
__device__ __forceinline__ bool se_where(const SeBlockArgs &a, uint32_t f, uint8_t *&out, uint64_t &p, uint32_t &slot)
{
    const SbRow r = a.rows[f];
    const SbTrack &t = a.trk[r.track];
    out = t.out; p = t.pos + (a.off[r.slot] - a.off[t.slot0]); slot = r.slot;
    return t.write != 0u;
}

/* the parameter bits of one channel-frame's record, as pack_block writes them (lnn_entropy.c) */
__device__ __forceinline__ uint64_t se_param_bits(const SeBlockArgs &a, const int32_t *rec)
{
    uint64_t b = 2u * (a.bits + 1u + 4u);
    for (uint32_t l = 0; l < a.L; l++) {
        b += 7u;
        for (uint32_t i = 0; i < a.P[l]; i++) b += a.tab->len[se_zz(rec[LINNE_AMD_PRM_COEF + a.coef_off[l] + i]) & 255u];
    }
    return b;
}

/* a lane per block: its size, the start of every channel's code, the host stitcher's per-block errors (lnn_entropy.c pack_block:
 * a RAW block at a width other than 8, 16 or 24 bits; a block over its 64 + C * S * 8 bytes; a size field over 32 bits) */
__global__ __launch_bounds__(SE_THREADS) void k_se_size(SeBlockArgs a)
{
    const uint32_t f = blockIdx.x * SE_THREADS + threadIdx.x;
    if (f >= a.F) return;
    const uint32_t type = a.types[f], n = a.nsmp[f];
    uint64_t bytes = 11u;
    int32_t st = LNN_OK;
    if (type == SX_RAW) {
        if (a.bits != 8u && a.bits != 16u && a.bits != 24u) st = LNN_INVALID_FORMAT;
        else bytes += ((uint64_t)a.bits * n * a.C) / 8u;
    } else if (type == SX_COMPRESS) {
        uint64_t pb = 0;
        for (uint32_t ch = 0; ch < a.C; ch++) pb += se_param_bits(a, a.prm + ((uint64_t)f * a.C + ch) * LINNE_AMD_PARAM_WORDS);
        uint64_t at = 88u + pb;
        for (uint32_t ch = 0; ch < a.C; ch++) {
            const uint64_t cf = (uint64_t)f * a.C + ch;
            a.cfbit[cf] = at;
            at += *(const uint32_t *)(a.plan + cf * LINNE_AMD_RICE_PLAN_BYTES + LINNE_AMD_RICE_PLAN_NBITS);
        }
        bytes = (at + 7u) >> 3;
        if (bytes > 64u + (uint64_t)a.C * a.S * 8u || bytes - 11u + 5u > 0xFFFFFFFFull) st = LNN_INSUFFICIENT_BUFFER;
    }
    const uint32_t slot = a.rows[f].slot;
    a.status[slot] = st;
    a.size[slot] = (st == LNN_OK) ? (uint32_t)bytes : 0u;
}

/* a lane per COMPRESS block: the parameter bits (linne_encoder.c:698-735) from bit 88 of the block on */
__global__ __launch_bounds__(64) void k_se_params(SeBlockArgs a)
{
    __shared__ uint32_t code[256];
    __shared__ uint8_t len[256];
    for (uint32_t i = threadIdx.x; i < 256u; i += 64u) { code[i] = a.tab->code[i]; len[i] = a.tab->len[i]; }
    __syncthreads();
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f >= a.F || a.types[f] != SX_COMPRESS) return;
    uint8_t *out; uint64_t p; uint32_t slot;
    if (!se_where(a, f, out, p, slot)) return;
    const uint64_t start = p * 8u + 88u;
    RiceBW bw; bw.dst = (uint32_t *)out; bw.w = bw.first_w = (uint32_t)(start >> 5); bw.fill = (uint32_t)(start & 31u); bw.cur = 0;
    auto put = [&](uint32_t v, uint32_t nb) { if (nb) bw.put(v & (0xFFFFFFFFu >> (32u - nb)), nb); };
    const int32_t *base = a.prm + (uint64_t)f * a.C * LINNE_AMD_PARAM_WORDS;
    for (uint32_t ch = 0; ch < a.C; ch++) {
        const int32_t *rec = base + (uint64_t)ch * LINNE_AMD_PARAM_WORDS;
        for (uint32_t l = 0; l < 2u; l++) { put(se_zz(rec[LINNE_AMD_PRM_PREV + l]), a.bits + 1u); put((uint32_t)rec[LINNE_AMD_PRM_PCOEF + l], 4u); }
    }
    for (uint32_t ch = 0; ch < a.C; ch++) {
        const int32_t *rec = base + (uint64_t)ch * LINNE_AMD_PARAM_WORDS;
        for (uint32_t l = 0; l < a.L; l++) {
            put(se_ceil_log2((uint32_t)rec[LINNE_AMD_PRM_UNITS + l]), 3u);
            put((uint32_t)rec[LINNE_AMD_PRM_RSHIFT + l], 4u);
            for (uint32_t i = 0; i < a.P[l]; i++) { const uint32_t sym = se_zz(rec[LINNE_AMD_PRM_COEF + a.coef_off[l] + i]) & 255u; put(code[sym], len[sym]); }
        }
    }
    bw.finish();
}

/* A workgroup per channel-frame of a COMPRESS block: k_rice_emit's two passes (lengths, then codes) with the writer started at the
 * channel's bit in the stream.  The code's length must be its plan's (the block's size was computed from it): a channel whose code
 * would come out longer or shorter writes nothing and raises its track's fail word (the track then fails; only a uint32
 * wrap-around of the reference's length count could do it). */
template <bool LDS> __global__ __launch_bounds__(REMIT_THREADS) void k_se_rice(SeBlockArgs a)
{
    extern __shared__ uint32_t zbuf[];
    __shared__ uint8_t kk[1024];
    __shared__ uint64_t wsum[REMIT_THREADS / 64];
    const uint32_t cf = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t f = cf / a.C;
    if (a.types[f] != SX_COMPRESS) return;                    /* block-uniform */
    uint8_t *out; uint64_t p; uint32_t slot;
    if (!se_where(a, f, out, p, slot)) return;        /* block-uniform */
    const uint8_t *rec = a.plan + (uint64_t)cf * LINNE_AMD_RICE_PLAN_BYTES;
    const uint32_t nbits = *(const uint32_t *)(rec + LINNE_AMD_RICE_PLAN_NBITS);
    const uint32_t n = a.nsmp[f], best = rec[0], ns = n >> best, parts = 1u << best;
    const int32_t *x = a.resid + (uint64_t)cf * a.S;
    const uint32_t ipt = (n + REMIT_THREADS - 1) / REMIT_THREADS;
    for (uint32_t p = tid; p < parts; p += REMIT_THREADS) kk[p] = rec[LINNE_AMD_RICE_PLAN_K2 + p];
    if (LDS) for (uint32_t s = tid; s < n; s += REMIT_THREADS) zbuf[s + s / ipt] = rp_zz(x[s]);
    __syncthreads();
    const uint32_t s0 = tid * ipt < n ? tid * ipt : n, s1 = (s0 + ipt < n) ? s0 + ipt : n;
    const uint32_t *zrun = zbuf + (size_t)tid * (ipt + 1u);
    uint64_t mybits = 0;
    {
        uint32_t part = ns ? s0 / ns : 0, loc = ns ? s0 - part * ns : 0;
        for (uint32_t s = s0; s < s1; s++) {
            const uint32_t k2 = kk[part], k1 = k2 + 1u, k1pow = 1u << (k1 & 31u);
            if (loc == 0) mybits += part ? rp_gamma_len(rp_zz((int32_t)k2 - (int32_t)kk[part - 1])) : 15u;
            const uint32_t v = LDS ? zrun[s - s0] : rp_zz(x[s]);
            mybits += (v < k1pow) ? (k1 + 1u) : (uint64_t)(((v - k1pow) >> k2) + 2u + k2);
            if (++loc == ns) { loc = 0; part++; }
        }
    }
    uint64_t incl = mybits;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint64_t v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t start = incl - mybits, total = 0;
    for (uint32_t w = 0; w < REMIT_THREADS / 64; w++) { if (w < wave) start += wsum[w]; total += wsum[w]; }
    if (total != nbits) { if (tid == 0) atomicOr(&a.fail[a.trk[a.rows[f].track].id], 1u); return; }          /* block-uniform */
    if (s0 >= s1) return;
    start += p * 8u + a.cfbit[cf];
    RiceBW bw; bw.dst = (uint32_t *)out; bw.w = bw.first_w = (uint32_t)(start >> 5); bw.fill = (uint32_t)(start & 31u); bw.cur = 0;
    {
        uint32_t part = ns ? s0 / ns : 0, loc = ns ? s0 - part * ns : 0;
        for (uint32_t s = s0; s < s1; s++) {
            const uint32_t k2 = kk[part], k1 = k2 + 1u, k1pow = 1u << (k1 & 31u);
            if (loc == 0) {
                if (part == 0) bw.put((best << 5) | k2, 15u);
                else {
                    const uint32_t g = rp_zz((int32_t)k2 - (int32_t)kk[part - 1]);
                    if (g == 0) bw.put(1u, 1u);
                    else { const uint32_t nd = 32u - (uint32_t)__clz((int)(g + 1u)); bw.zeros(nd - 1u); bw.put(g + 1u, nd); }
                }
            }
            const uint32_t v = LDS ? zrun[s - s0] : rp_zz(x[s]);
            if (v < k1pow) { bw.put(1u, 1u); bw.put((k1 == 32u) ? v : (v & ((1u << (k1 & 31u)) - 1u)), k1); }
            else {
                const uint32_t d = v - k1pow;
                bw.zeros((uint64_t)(d >> k2) + 1u);
                bw.put((1u << k2) | (d & ((1u << k2) - 1u)), k2 + 1u);
            }
            if (++loc == ns) { loc = 0; part++; }
        }
    }
    bw.finish();
}

/* xch workgroups per block: the samples of RAW blocks, zig-zagged, big-endian, channels interleaved; `pcm` is the pass's [F][C][S] */
__global__ __launch_bounds__(SE_THREADS) void k_se_raw(SeBlockArgs a, const int32_t *pcm)
{
    const uint32_t f = blockIdx.x / a.xch, x = blockIdx.x % a.xch;
    if (a.types[f] != SX_RAW) return;
    uint8_t *out; uint64_t p; uint32_t slot;
    if (!se_where(a, f, out, p, slot)) return;
    const uint32_t n = a.nsmp[f], w = a.bits >> 3;
    uint8_t *dst = out + p + 11u;
    for (uint32_t s = x * SE_THREADS + threadIdx.x; s < n; s += a.xch * SE_THREADS)
        for (uint32_t ch = 0; ch < a.C; ch++) {
            const uint32_t u = se_zz(pcm[((uint64_t)f * a.C + ch) * a.S + s]);
            uint8_t *q = dst + ((uint64_t)s * a.C + ch) * w;
            for (uint32_t j = 0; j < w; j++) q[j] = (uint8_t)(u >> (8u * (w - 1u - j)));
        }
}

/* A wave per block (four per workgroup), after every other writer of the pass: the CRC16 over [p + 8, p + 6 + size) -- the type and
 * sample count, which this launch writes, taken from registers, the payload from memory -- from lane partials shifted by the bytes
 * behind them (k_ib_check), then the 11 header bytes: FF FF, size - 6, CRC, type, n (linne_encoder.c:806-855). */
__global__ __launch_bounds__(256) void k_se_crc(SeBlockArgs a)
{
    __shared__ uint16_t crc_t[256];
    __shared__ uint16_t shift_t[SX_CRC_LEVELS][16];
    for (uint32_t i = threadIdx.x; i < 256u; i += 256u) crc_t[i] = a.tab->sx.crc[i];
    for (uint32_t i = threadIdx.x; i < SX_CRC_LEVELS * 16u; i += 256u) shift_t[i >> 4][i & 15u] = a.tab->sx.shift[i >> 4][i & 15u];
    __syncthreads();
    const uint32_t f = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (f >= a.F) return;
    uint8_t *out; uint64_t p; uint32_t slot;
    if (!se_where(a, f, out, p, slot)) return;        /* wave-uniform */
    const uint32_t size = a.size[slot], type = a.types[f], n = a.nsmp[f];
    const uint32_t h0 = type & 0xFFu, h1 = (n >> 8) & 0xFFu, h2 = n & 0xFFu;
    const uint64_t len = (uint64_t)size - 8u;                      /* 3 header bytes + the payload */
    const uint64_t chunk = (len + 63u) >> 6, s = (uint64_t)lane * chunk, e = (s + chunk < len) ? s + chunk : len;
    const uint8_t *q = out + p + 8u;
    uint32_t crc = 0;
    if (s < len) {
        uint64_t i = s;
        for (; i < e && i < 3u; i++) crc = (crc >> 8) ^ crc_t[(crc ^ (i == 0u ? h0 : (i == 1u ? h1 : h2))) & 0xFFu];
        for (; i + 4u <= e; i += 4u) {
            const uint32_t b0 = q[i], b1 = q[i + 1], b2 = q[i + 2], b3 = q[i + 3];
            crc = (crc >> 8) ^ crc_t[(crc ^ b0) & 0xFFu];
            crc = (crc >> 8) ^ crc_t[(crc ^ b1) & 0xFFu];
            crc = (crc >> 8) ^ crc_t[(crc ^ b2) & 0xFFu];
            crc = (crc >> 8) ^ crc_t[(crc ^ b3) & 0xFFu];
        }
        for (; i < e; i++) crc = (crc >> 8) ^ crc_t[(crc ^ q[i]) & 0xFFu];
        uint64_t behind = len - e;
        for (uint32_t k = 0; behind != 0u && k < SX_CRC_LEVELS; k++, behind >>= 1) if (behind & 1u) crc = sx_apply(shift_t[k], crc);
    }
    for (uint32_t m = 32; m >= 1u; m >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, (int)m, 64);
    if (lane != 0u) return;
    uint8_t *h = out + p;
    const uint32_t field = size - 6u;
    h[0] = 0xFFu; h[1] = 0xFFu;
    h[2] = (uint8_t)(field >> 24); h[3] = (uint8_t)(field >> 16); h[4] = (uint8_t)(field >> 8); h[5] = (uint8_t)field;
    h[6] = (uint8_t)(crc >> 8); h[7] = (uint8_t)crc;
    h[8] = (uint8_t)h0; h[9] = (uint8_t)h1; h[10] = (uint8_t)h2;
}

/* ---- per track of a pass ---- */
#define SB_ZERO_THREADS 256u
#define SB_ZERO_CHUNK 65536u            /* bytes a workgroup of k_sb_zero clears */

/* A wave per track of the pass, behind k_se_size and the scan: the bytes of the track's blocks, the lowest slot whose block
 * the host stitcher refuses (relative to the track's first slot) and that block's status. */
__global__ __launch_bounds__(64) void k_sb_reduce(const SbTrack *trk, uint32_t ntrk, const int32_t *status, const uint64_t *off, SbTrackOut *out)
{
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (t >= ntrk) return;
    const uint32_t s0 = trk[t].slot0, n = trk[t].nslots;
    uint32_t low = 0xFFFFFFFFu;
    for (uint32_t i = lane; i < n; i += 64u) if (status[s0 + i] != LNN_OK) { low = i; break; }        /* (a lane's slots ascend) */
    for (uint32_t m = 32; m >= 1u; m >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)low, (int)m, 64); low = o < low ? o : low; }
    if (lane != 0u) return;
    SbTrackOut r;
    r.bytes = off[s0 + n] - off[s0]; r.fail = low; r.status = (low != 0xFFFFFFFFu) ? status[s0 + low] : LNN_OK;
    out[t] = r;
}

/* xz workgroups per track of the pass; workgroup x of a written track clears bytes [x * SB_ZERO_CHUNK, (x + 1) * SB_ZERO_CHUNK)
 * of the track's region [pos, pos + bytes): 32-bit stores to the words that lie wholly inside the region (the track's buffer is
 * 4-byte aligned, so these are words of this track alone), byte stores to the up to three bytes at either edge. */
__global__ __launch_bounds__(SB_ZERO_THREADS) void k_sb_zero(const SbTrack *trk, const SbTrackOut *res, uint32_t xz)
{
    const uint32_t t = blockIdx.x / xz, x = blockIdx.x - t * xz;
    if (!trk[t].write) return;
    const uint64_t lo = trk[t].pos, hi = lo + res[t].bytes;
    const uint64_t c0 = lo + (uint64_t)x * SB_ZERO_CHUNK;
    if (c0 >= hi) return;
    const uint64_t c1 = (hi - c0 > SB_ZERO_CHUNK) ? c0 + SB_ZERO_CHUNK : hi;      /* this workgroup's bytes [c0, c1) */
    uint8_t *out = trk[t].out;
    uint64_t w0 = (c0 + 3u) & ~(uint64_t)3u, w1 = c1 & ~(uint64_t)3u;           /* whole words [w0, w1) */
    if (w0 > w1) w0 = w1 = c1;                                                  /* fewer than four bytes inside one word */
    if (threadIdx.x < 3u && c0 + threadIdx.x < (w0 < c1 ? w0 : c1)) out[c0 + threadIdx.x] = 0u;
    if (threadIdx.x < 3u && w1 + threadIdx.x < c1 && w1 >= w0) out[w1 + threadIdx.x] = 0u;
    uint32_t *w = (uint32_t *)(out + w0);
    const uint64_t nw = (w1 - w0) >> 2;
    for (uint64_t i = threadIdx.x; i < nw; i += SB_ZERO_THREADS) w[i] = 0u;
}

/* the stream headers of the finished tracks: entry i is 30 bytes of `bytes` (stride 32) for the stream dst[i]; a thread per byte */
__global__ __launch_bounds__(256) void k_sb_header(uint8_t *const *dst, const uint8_t *bytes, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, t = i >> 5, b = i & 31u;
    if (t >= n || b >= 30u) return;
    dst[t][b] = bytes[(uint64_t)t * 32u + b];
}

#endif
