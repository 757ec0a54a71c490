/* lnn_k_windows.h -- decoding sample windows of resident .lnn streams with their block indexes (lnn_k_stream.h): many windows of
 * many streams in one call (LINNEAmd_DecodeWindowsDevice) or one (LINNEAmd_DecodeStreamDevice, the same with one window); DESIGN.md
 * section 5, "Many windows in one call".
 *
 * The host flattens the windows of one stream shape into block records (one per block of every window, in window order) and
 * window records, uploads them once, and launches per pass:
 *   k_wx_gather               the bytes of the pass's COMPRESS blocks, each from its own stream, into one packed segment the Rice
 *                             decoder reads as words
 *   k_wx_params               a lane per COMPRESS block: its parameter records, where its Rice code starts and ends in the
 *                             packed segment
 *   (k_rice_decode of lnn_k_rice.h)
 *   k_wx_rice_check           did the Rice decoder consume exactly the bytes the block's size field names?  The lowest failing
 *                             block's number goes into its window's fail word
 *   (the synthesis kernels of lnn_k_decode*.h)
 *   k_wx_place                every record's samples, cropped to its window, into that window's planar output; a record of type
 *                             WX_TAIL is the part of a window beyond the stream's last block (zeros).  The records of a window whose
 *                             fail word is set are skipped: a failing window's output is not written
 * As in lnn_k_stream.h, no read of a stream leaves [0, stream_bytes): RAW samples are un-zig-zagged straight from the stream.
 */
#ifndef LNN_K_WINDOWS_H_INCLUDED
#define LNN_K_WINDOWS_H_INCLUDED

#define WX_TAIL 3u                      /* record type beside SX_COMPRESS / SX_SILENT / SX_RAW: a window's samples in [covered, hi) */
#define WX_GATHER_THREADS 256u
#define WX_NOFAIL 0xFFFFFFFFu

/* one block of one window (64 bytes) */
struct WxBlock {
    const uint8_t *b; uint64_t N;       /* the block's stream and its length */
    uint64_t off;                       /* the block's position in it */
    uint64_t first;                     /* its first sample */
    uint64_t dst;                       /* COMPRESS: where its first byte lies in the pass's packed segment; (dst & 15) == ((b + off) & 15) */
    uint32_t size, type, nsmp;          /* the size field, SX_* / WX_TAIL, samples */
    uint32_t win;                       /* its window's record */
    uint32_t cidx;                      /* index among the pass's COMPRESS blocks, or ~0 */
    uint32_t blk;                       /* its number in its stream */
};
/* one window (48 bytes) */
struct WxWindow {
    uint64_t lo, hi, covered;           /* the range [lo, hi); the samples the stream's blocks hold */
    int32_t *out; uint64_t stride;
    uint32_t fidx, pad;                 /* its fail word */
};

/* Workgroup k copies COMPRESS block k's size + 6 bytes to seg + dst.  Source and destination have the same address modulo 16 (the
 * host chose dst so): the 16-byte groups that lie wholly inside the block travel as one load and one store, the two at its ends
 * are put together from bytes, with zeros where the block does not reach -- so every byte of the block's slot
 * [dst & ~15, (dst + size + 6 + 15) & ~15) is written, and the segment, a sequence of such slots, holds no stale byte. */
__global__ __launch_bounds__(WX_GATHER_THREADS) void k_wx_gather(const WxBlock *recs, const uint32_t *crec, uint32_t ncomp, uint8_t *seg)
{
    const uint32_t k = blockIdx.x;
    if (k >= ncomp) return;
    const WxBlock rc = recs[crec[k]];
    uint64_t len = (uint64_t)rc.size + 6u;
    if (rc.off >= rc.N) return;
    if (len > rc.N - rc.off) len = rc.N - rc.off;                  /* (a candidate's size + 6 fits: sx_candidate) */
    const uint8_t *src = rc.b + rc.off;
    const uint64_t s0 = rc.dst & ~(uint64_t)15u, end = rc.dst + len, ngroups = (end + 15u - s0) >> 4;
    for (uint64_t j = threadIdx.x; j < ngroups; j += WX_GATHER_THREADS) {
        const uint64_t c = s0 + (j << 4);
        uint4 v;
        if (c >= rc.dst && c + 16u <= end) v = *(const uint4 *)(src + (c - rc.dst));
        else {
            uint32_t w[4] = { 0u, 0u, 0u, 0u };
            for (uint32_t t = 0; t < 16u; t++) {
                const uint64_t p = c + t;
                if (p >= rc.dst && p < end) w[t >> 2] |= (uint32_t)src[p - rc.dst] << (8u * (t & 3u));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *(uint4 *)(seg + c) = v;
    }
}

struct WxParamArgs {
    const WxBlock *recs; const uint32_t *crec;
    uint32_t ncomp, C, bits, L, P[LNN_MAXL], coef_off[LNN_MAXL];
    const SxTables *tab;
    int32_t *prm;                       /* [ncomp][C][LINNE_AMD_PARAM_WORDS] */
    uint64_t *bitpos, *bitend;          /* [ncomp], bits from the packed segment's start */
    uint32_t *out_nsmp;                 /* [ncomp] */
};
/* a lane per COMPRESS block of the pass; the bits are read from the block's own stream, not from the packed segment */
__global__ __launch_bounds__(64) void k_wx_params(WxParamArgs a)
{
    __shared__ uint16_t child[512][2];
    for (uint32_t i = threadIdx.x; i < 512u; i += 64u) { child[i][0] = a.tab->child[i][0]; child[i][1] = a.tab->child[i][1]; }
    __syncthreads();
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= a.ncomp) return;
    const WxBlock *rc = a.recs + a.crec[k];
    SxBits r; r.open(rc->b, rc->N, rc->off + 11u);
    sx_parse_params(r, child, a.tab->root, a.C, a.bits, a.L, a.P, a.coef_off, a.prm + (uint64_t)k * a.C * LINNE_AMD_PARAM_WORDS);
    a.bitpos[k] = rc->dst * 8u + 88u + r.consumed;
    a.bitend[k] = (rc->dst + (uint64_t)rc->size + 6u) * 8u;
    a.out_nsmp[k] = rc->nsmp;
}

/* DecodeWhole's test of the device's Rice decoder (lnn_api.c:860-868): the codes must end in the block's last byte.  fail[window] =
 * the lowest block number of the window's stream that fails it (preset to WX_NOFAIL) */
__global__ __launch_bounds__(256) void k_wx_rice_check(const uint64_t *endbit, const WxBlock *recs, const uint32_t *crec, const WxWindow *wins,
        uint32_t ncomp, uint32_t *fail)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= ncomp) return;
    const WxBlock *rc = recs + crec[k];
    const uint64_t eb = endbit[k], pay = (rc->dst + 11u) * 8u;
    if (eb == ~0ull || eb < pay || 11u + ((eb - pay + 7u) >> 3) != (uint64_t)rc->size + 6u) atomicMin(fail + wins[rc->win].fidx, rc->blk);
}

struct WxPlaceArgs {
    const WxBlock *recs; uint32_t nrec;
    const WxWindow *wins; const uint32_t *fail;
    uint32_t C, S, bits;
    const int32_t *pcm;                 /* [ncomp][C][S]: the synthesis' output */
    uint32_t xch;                       /* workgroups per record */
};
/* nrec * xch workgroups: the y-th xch of them place record y */
__global__ __launch_bounds__(SX_PLACE_THREADS) void k_wx_place(WxPlaceArgs a)
{
    const uint32_t y = blockIdx.x / a.xch, x = blockIdx.x % a.xch;
    if (y >= a.nrec) return;
    const WxBlock *rc = a.recs + y;
    const WxWindow w = a.wins[rc->win];
    if (a.fail[w.fidx] != WX_NOFAIL) return;
    const uint32_t type = rc->type;
    if (type == WX_TAIL) {
        const uint64_t z0 = w.covered > w.lo ? w.covered : w.lo;
        for (uint64_t s = z0 + (uint64_t)x * SX_PLACE_THREADS + threadIdx.x; s < w.hi; s += (uint64_t)a.xch * SX_PLACE_THREADS)
            for (uint32_t ch = 0; ch < a.C; ch++) w.out[(uint64_t)ch * w.stride + (s - w.lo)] = 0;
        return;
    }
    const uint32_t n = rc->nsmp;
    const uint64_t f0 = rc->first;
    for (uint32_t i = x * SX_PLACE_THREADS + threadIdx.x; i < n; i += a.xch * SX_PLACE_THREADS) {
        const uint64_t s = f0 + i;
        if (s < w.lo || s >= w.hi) continue;
        int32_t *dst = w.out + (s - w.lo);
        if (type == SX_COMPRESS) {
            const int32_t *src = a.pcm + (uint64_t)rc->cidx * a.C * a.S + i;
            for (uint32_t ch = 0; ch < a.C; ch++) dst[(uint64_t)ch * w.stride] = src[(uint64_t)ch * a.S];
        } else if (type == SX_RAW) {
            const uint32_t wd = a.bits >> 3;
            uint64_t q = rc->off + 11u + (uint64_t)i * a.C * wd;
            for (uint32_t ch = 0; ch < a.C; ch++, q += wd) {
                uint32_t u = 0;
                for (uint32_t j = 0; j < wd; j++) u = (u << 8) | rc->b[q + j];
                dst[(uint64_t)ch * w.stride] = sx_unzz(u);
            }
        } else
            for (uint32_t ch = 0; ch < a.C; ch++) dst[(uint64_t)ch * w.stride] = 0;
    }
}

#endif
