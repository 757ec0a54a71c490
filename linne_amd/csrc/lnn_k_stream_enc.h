/* lnn_k_stream_enc.h -- encoding planar PCM that lies in device memory into a .lnn stream in device memory
 * (LINNEAmd_EncodeStreamDevice; DESIGN.md section 5, "Encoding into a stream in HBM").
 *
 * Per pass of frames (between the analysis and the writers sits the one host step: block types, flagged Rice plans):
 *   k_se_gather    planar input -> the [F][C][S] frame layout of the analysis, the last frame zero-padded; per frame a flag
 *                  "some sample is not 0" (the SILENT test of the block-type decision)
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
 */
#ifndef LNN_K_STREAM_ENC_H_INCLUDED
#define LNN_K_STREAM_ENC_H_INCLUDED

#define SE_THREADS 256u

/* the device tables of the stream encoder: the decoder's (CRC byte table, shift matrices, Huffman tree) and the Huffman code */
struct SeTables {
    SxTables sx;
    uint32_t code[256];                 /* code word of each coefficient symbol (lnn_entropy.c huff_walk), its low len[sym] bits */
    uint8_t len[256];
};

struct SeGatherArgs {
    const int32_t *pcm; uint64_t stride;        /* channel ch at pcm + ch * stride */
    uint64_t first, total;                      /* the pass's first sample, the stream's samples per channel */
    int32_t *frames;                            /* [F][C][S] */
    uint32_t *nonzero;                          /* [F], zeroed */
    uint32_t F, C, S;
};
/* a workgroup per channel-frame */
__global__ __launch_bounds__(SE_THREADS) void k_se_gather(SeGatherArgs a)
{
    const uint32_t cf = blockIdx.x, f = cf / a.C, ch = cf - f * a.C;
    const uint64_t s0 = a.first + (uint64_t)f * a.S;
    const uint32_t n = (a.total - s0 < a.S) ? (uint32_t)(a.total - s0) : a.S;
    const int32_t *src = a.pcm + (uint64_t)ch * a.stride + s0;
    int32_t *dst = a.frames + (uint64_t)cf * a.S;
    int any = 0;
    for (uint32_t s = threadIdx.x; s < a.S; s += SE_THREADS) {
        const int32_t v = (s < n) ? src[s] : 0;
        dst[s] = v;
        any |= (v != 0);
    }
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
    uint32_t *fail;                     /* [0] lowest failing block (atomicMin), [1] set when a Rice code's length is not its plan's */
    uint64_t *cfbit;                    /* [F * C] bit offset of each channel's code from its block's first byte */
    const uint64_t *off;                /* [F + 1] offsets of the blocks from `base` (k_sx_scan) */
    uint8_t *out; uint64_t base;        /* the stream and the pass's first byte in it */
    uint32_t xch;                       /* k_se_raw: workgroups per block */
};

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
    a.status[f] = st;
    a.size[f] = (st == LNN_OK) ? (uint32_t)bytes : 0u;
    if (st != LNN_OK) atomicMin(&a.fail[0], f);
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
    const uint64_t start = (a.base + a.off[f]) * 8u + 88u;
    RiceBW bw; bw.dst = (uint32_t *)a.out; bw.w = bw.first_w = (uint32_t)(start >> 5); bw.fill = (uint32_t)(start & 31u); bw.cur = 0;
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
 * would come out longer or shorter writes nothing and raises fail[1] (the call then fails; only a uint32 wrap-around of the
 * reference's length count could do it). */
template <bool LDS> __global__ __launch_bounds__(REMIT_THREADS) void k_se_rice(SeBlockArgs a)
{
    extern __shared__ uint32_t zbuf[];
    __shared__ uint8_t kk[1024];
    __shared__ uint64_t wsum[REMIT_THREADS / 64];
    const uint32_t cf = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t f = cf / a.C;
    if (a.types[f] != SX_COMPRESS) return;                    /* block-uniform */
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
    if (total != nbits) { if (tid == 0) atomicOr(&a.fail[1], 1u); return; }          /* block-uniform */
    if (s0 >= s1) return;
    start += (a.base + a.off[f]) * 8u + a.cfbit[cf];
    RiceBW bw; bw.dst = (uint32_t *)a.out; bw.w = bw.first_w = (uint32_t)(start >> 5); bw.fill = (uint32_t)(start & 31u); bw.cur = 0;
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
    const uint32_t n = a.nsmp[f], w = a.bits >> 3;
    uint8_t *dst = a.out + a.base + a.off[f] + 11u;
    for (uint32_t s = x * SE_THREADS + threadIdx.x; s < n; s += a.xch * SE_THREADS)
        for (uint32_t ch = 0; ch < a.C; ch++) {
            const uint32_t u = se_zz(pcm[((uint64_t)f * a.C + ch) * a.S + s]);
            uint8_t *q = dst + ((uint64_t)s * a.C + ch) * w;
            for (uint32_t j = 0; j < w; j++) q[j] = (uint8_t)(u >> (8u * (w - 1u - j)));
        }
}

/* A wave per block (four per workgroup), after every other writer of the pass: the CRC16 over [p + 8, p + 6 + size) -- the type and
 * sample count, which this launch writes, taken from registers, the payload from memory -- from lane partials shifted by the bytes
 * behind them (k_sx_check), then the 11 header bytes: FF FF, size - 6, CRC, type, n (linne_encoder.c:806-855). */
__global__ __launch_bounds__(256) void k_se_crc(SeBlockArgs a)
{
    __shared__ uint16_t crc_t[256];
    __shared__ uint16_t shift_t[SX_CRC_LEVELS][16];
    for (uint32_t i = threadIdx.x; i < 256u; i += 256u) crc_t[i] = a.tab->sx.crc[i];
    for (uint32_t i = threadIdx.x; i < SX_CRC_LEVELS * 16u; i += 256u) shift_t[i >> 4][i & 15u] = a.tab->sx.shift[i >> 4][i & 15u];
    __syncthreads();
    const uint32_t f = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (f >= a.F) return;
    const uint64_t p = a.base + a.off[f];
    const uint32_t size = a.size[f], type = a.types[f], n = a.nsmp[f];
    const uint32_t h0 = type & 0xFFu, h1 = (n >> 8) & 0xFFu, h2 = n & 0xFFu;
    const uint64_t len = (uint64_t)size - 8u;                      /* 3 header bytes + the payload */
    const uint64_t chunk = (len + 63u) >> 6, s = (uint64_t)lane * chunk, e = (s + chunk < len) ? s + chunk : len;
    const uint8_t *q = a.out + p + 8u;
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
    uint8_t *h = a.out + p;
    const uint32_t field = size - 6u;
    h[0] = 0xFFu; h[1] = 0xFFu;
    h[2] = (uint8_t)(field >> 24); h[3] = (uint8_t)(field >> 16); h[4] = (uint8_t)(field >> 8); h[5] = (uint8_t)field;
    h[6] = (uint8_t)(crc >> 8); h[7] = (uint8_t)crc;
    h[8] = (uint8_t)h0; h[9] = (uint8_t)h1; h[10] = (uint8_t)h2;
}

#endif
