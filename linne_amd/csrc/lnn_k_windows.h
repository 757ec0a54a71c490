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
 *   k_wx_place                every record's samples, cropped to its window, into that window's output (int32 planar, or converted
 *                             to the window's struct LINNEAmdPcmLayout: int16, packed 24-bit, float32; interleaved, padded); a record of type
 *                             WX_TAIL is the part of a window beyond the stream's last block (zeros).  The records of a window whose
 *                             fail word is set are skipped: a failing window's output is not written
 * k_wx_place and the kernels that stand in its place in the sibling calls -- k_wx_compare (lnn_k_compare.h), k_wx_measure
 * (lnn_k_measure.h), k_wx_digest (lnn_k_digest.h), k_wx_mix (lnn_k_mix.h, which writes PCM too: wx_place_layout_from) -- begin with wx_prologue and cut their record into pieces with wx_walk, below;
 * they differ in what they do with a piece.
 * As in lnn_k_stream.h, no read of a stream leaves [0, stream_bytes): RAW samples are un-zig-zagged straight from the stream.
 */
#ifndef LNN_K_WINDOWS_H_INCLUDED
#define LNN_K_WINDOWS_H_INCLUDED

#include "lnn_windows_plan.h"          /* the records the host's plan fills: WxBlock, WxWindow, WX_TAIL, WX_NOFAIL */

#define WX_GATHER_THREADS 256u

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
    uint32_t *sat;                      /* [W] beside the fail words: set when a sample of the window lay outside its format's range */
    float scale;                        /* 2^-(bits - 1): the F32 format's */
};

/* ---- writing PCM of any layout (include/linne_amd.h struct LINNEAmdPcmLayout) ---- */
#define WX_IMG_BYTES (SX_PLACE_THREADS * LINNE_MAX_NUM_CHANNELS * 4u + 8u * LINNE_MAX_NUM_CHANNELS)

/* sample s (block sample i) of channel ch of record rc, as the int32 planar path takes it */
__device__ __forceinline__ int32_t wx_value(const WxPlaceArgs &a, const WxBlock *rc, uint32_t type, uint32_t i, uint32_t ch)
{
    if (type == SX_COMPRESS) return a.pcm[((uint64_t)rc->cidx * a.C + ch) * a.S + i];
    if (type == SX_RAW) {
        const uint32_t wd = a.bits >> 3;
        const uint64_t q = rc->off + 11u + ((uint64_t)i * a.C + ch) * wd;
        uint32_t u = 0;
        for (uint32_t j = 0; j < wd; j++) u = (u << 8) | rc->b[q + j];
        return sx_unzz(u);
    }
    return 0;
}
/* v in the window's format: the element's bits (its low 2, 3 or 4 bytes); sat is set when v had to be clipped */
__device__ __forceinline__ uint32_t wx_convert(int32_t v, uint32_t fmt, float scale, int &sat)
{
    if (fmt == LINNE_AMD_PCM_F32) return __float_as_uint((float)v * scale);
    if (fmt == LINNE_AMD_PCM_S32) return (uint32_t)v;
    const int32_t top = (fmt == LINNE_AMD_PCM_S16) ? 32767 : 8388607;
    const int32_t c = v > top ? top : (v < -top - 1 ? -top - 1 : v);
    sat |= (c != v);
    return (uint32_t)c;
}
/* an element of es bytes at p, aligned to the element (S24: to nothing), in global memory or LDS: stores of its own bytes only */
__device__ __forceinline__ void wx_store1(uint8_t *p, uint32_t u, uint32_t es)
{
    if (es == 4u) *(uint32_t *)p = u;
    else if (es == 2u) *(uint16_t *)p = (uint16_t)u;
    else { p[0] = (uint8_t)u; p[1] = (uint8_t)(u >> 8); p[2] = (uint8_t)(u >> 16); }
}

/* The workgroup places sample frames [sa, sb) (at most SX_PLACE_THREADS, inside the window) of C channels in a layout other than int32
 * with sample stride 1.  The elements come from src: src.frame(smp) names frame sa + smp, src.get(ch, sat) then gives channel ch of it
 * in the window's format (the element's bits, as wx_convert gives them).  Where the elements of this piece are contiguous in memory --
 * every channel's for sample stride 1, the whole piece's for packed interleaved (channel stride 1, sample stride C) -- they are first
 * laid out in LDS at their address modulo 4 and then stored as aligned 32-bit words; a word that reaches outside the run [A, A + len)
 * holds elements other workgroups (or nobody) write, and only its bytes inside the run are stored, one by one.  With any other strides
 * every element is stored by itself.  Returns (to every thread) whether a sample was clipped. */
template <class Source> __device__ __forceinline__ int wx_place_layout_from(const WxWindow &w, uint32_t C, uint64_t sa, uint64_t sb, uint8_t *img, Source src)
{
    const uint32_t fmt = w.fmt, es = fmt == LINNE_AMD_PCM_S16 ? 2u : (fmt == LINNE_AMD_PCM_S24 ? 3u : 4u);
    const uint32_t m = (uint32_t)(sb - sa), t = threadIdx.x;
    uint8_t *base = (uint8_t *)w.out;
    const bool packed = (w.stride == 1u && w.sstride == C), planar = (w.sstride == 1u);
    int sat = 0;
    if (!packed && !planar) {
        for (uint32_t k = t; k < m * C; k += SX_PLACE_THREADS) {
            const uint32_t smp = k / C, ch = k - smp * C;
            src.frame(smp);
            const uint32_t u = src.get(ch, sat);
            wx_store1(base + ((uint64_t)ch * w.stride + (sa + smp - w.lo) * w.sstride) * es, u, es);
        }
        return __syncthreads_or(sat);
    }
    /* runs: planar C of m elements, packed one of m * C; run r starts at byte A(r) and lies in LDS at r * pitch + (A(r) & 3) */
    const uint32_t nrun = planar ? C : 1u, len = (planar ? m : m * C) * es, pitch = ((len + 3u) & ~3u) + 8u;
    if (t < m) {
        src.frame(t);
        for (uint32_t ch = 0; ch < C; ch++) {
            const uint32_t u = src.get(ch, sat);
            const uint32_t r = planar ? ch : 0u;
            const uint64_t A = (uint64_t)(uintptr_t)base + ((uint64_t)r * w.stride + (sa - w.lo) * w.sstride) * es;
            wx_store1(img + r * pitch + (uint32_t)(A & 3u) + (planar ? t : t * C + ch) * es, u, es);
        }
    }
    sat = __syncthreads_or(sat);
    for (uint32_t r = 0; r < nrun; r++) {
        const uint64_t A = (uint64_t)(uintptr_t)base + ((uint64_t)r * w.stride + (sa - w.lo) * w.sstride) * es, E = A + len, W0 = A & ~(uint64_t)3u;
        const uint32_t nw = (uint32_t)((E + 3u - W0) >> 2);
        const uint32_t *src = (const uint32_t *)(img + r * pitch);
        for (uint32_t k = t; k < nw; k += SX_PLACE_THREADS) {
            const uint64_t g = W0 + 4u * (uint64_t)k;
            const uint32_t v = src[k];
            if (g >= A && g + 4u <= E) *(uint32_t *)(uintptr_t)g = v;
            else for (uint32_t j = 0; j < 4u; j++) if (g + j >= A && g + j < E) *(uint8_t *)(uintptr_t)(g + j) = (uint8_t)(v >> (8u * j));
        }
    }
    __syncthreads();                    /* (the image is filled again by the next piece) */
    return sat;
}
/* k_wx_place's source: the record's own samples, channel for channel; sample 0 of record rc is stream sample f0 */
struct WxPlaceSource {
    const WxPlaceArgs &a; const WxBlock *rc; uint32_t type, fmt; uint64_t f0, sa; uint32_t smp;
    __device__ __forceinline__ void frame(uint32_t smp_) { smp = smp_; }
    __device__ __forceinline__ uint32_t get(uint32_t ch, int &sat) const { return wx_convert(wx_value(a, rc, type, (uint32_t)(sa + smp - f0), ch), fmt, a.scale, sat); }
};
__device__ __forceinline__ int wx_place_layout(const WxPlaceArgs &a, const WxWindow &w, const WxBlock *rc, uint32_t type, uint64_t f0,
        uint64_t sa, uint64_t sb, uint8_t *img)
{
    WxPlaceSource src = { a, rc, type, w.fmt, f0, sa, 0u };
    return wx_place_layout_from(w, a.C, sa, sb, img, src);
}

/* ---- the record walk k_wx_place and its siblings (lnn_k_compare.h, lnn_k_measure.h, lnn_k_digest.h) share ---- */
/* What workgroup blockIdx.x of a grid of nrec * xch starts with: the y-th xch workgroups take record y, this one as its x-th.  false:
 * nothing to do -- no such record, or its window's fail word is set.  Every exit is block-uniform */
struct WxRecord { const WxBlock *rc; WxWindow w; uint32_t type, x; };
__device__ __forceinline__ bool wx_prologue(const WxPlaceArgs &a, WxRecord &r)
{
    const uint32_t y = blockIdx.x / a.xch;
    r.x = blockIdx.x % a.xch;
    if (y >= a.nrec) return false;
    r.rc = a.recs + y;
    r.w = a.wins[r.rc->win];
    if (a.fail[r.w.fidx] != WX_NOFAIL) return false;
    r.type = r.rc->type;
    return true;
}
/* piece(f0, sa, sb) for every piece of record rc that this workgroup takes: samples [sa, sb) of the stream, at most SX_PLACE_THREADS
 * of them and inside the window, of a record whose sample 0 is stream sample f0.  A WX_TAIL record is cut from max(covered, lo) on
 * (f0 = sa: its "block" begins with the piece); a block record is cut from its first sample on and every piece cropped to [lo, hi).
 * sa and sb are block-uniform, so a piece may hold barriers */
template <class Piece> __device__ __forceinline__ void wx_walk(const WxPlaceArgs &a, const WxBlock *rc, const WxWindow &w, uint32_t type, uint32_t x, Piece piece)
{
    if (type == WX_TAIL) {
        const uint64_t z0 = w.covered > w.lo ? w.covered : w.lo;
        for (uint64_t s = z0 + (uint64_t)x * SX_PLACE_THREADS; s < w.hi; s += (uint64_t)a.xch * SX_PLACE_THREADS)
            piece(s, s, (w.hi - s < SX_PLACE_THREADS) ? w.hi : s + SX_PLACE_THREADS);
    } else {
        const uint64_t f0 = rc->first, e = f0 + rc->nsmp;
        for (uint64_t s = f0 + (uint64_t)x * SX_PLACE_THREADS; s < e; s += (uint64_t)a.xch * SX_PLACE_THREADS) {
            const uint64_t s1 = (e - s < SX_PLACE_THREADS) ? e : s + SX_PLACE_THREADS;
            const uint64_t sa = s > w.lo ? s : w.lo, sb = s1 < w.hi ? s1 : w.hi;
            if (sa < sb) piece(f0, sa, sb);
        }
    }
}

/* nrec * xch workgroups: the y-th xch of them place record y.  Held to the 96 scalar registers it had before the layout branch went
 * through wx_walk: 256-thread workgroups are admitted per CU by their scalar registers in steps of 16, seven at 96 and six at the 102
 * the compiler takes otherwise, and the int32 path, a thread per sample and bound by how many workgroups are in flight, is a tenth
 * slower with six (profiles/ab_windows_shared_walk.txt has both; nothing spills under the cap) */
__global__ __launch_bounds__(SX_PLACE_THREADS) __attribute__((amdgpu_num_sgpr(96))) void k_wx_place(WxPlaceArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t img[WX_IMG_BYTES];
    WxRecord r;
    if (!wx_prologue(a, r)) return;
    const WxBlock *rc = r.rc;
    const WxWindow w = r.w;
    const uint32_t type = r.type, x = r.x;
    if (w.fmt != LINNE_AMD_PCM_S32 || w.sstride != 1u) {         /* block-uniform */
        int sat = 0;
        wx_walk(a, rc, w, type, x, [&](uint64_t f0, uint64_t sa, uint64_t sb) { sat |= wx_place_layout(a, w, rc, type, f0, sa, sb, img); });
        if (sat && threadIdx.x == 0) atomicOr(&a.sat[w.fidx], 1u);
        return;
    }
    /* int32 with sample stride 1: a thread per sample, no pieces */
    int32_t *out = (int32_t *)w.out;
    if (type == WX_TAIL) {
        const uint64_t z0 = w.covered > w.lo ? w.covered : w.lo;
        for (uint64_t s = z0 + (uint64_t)x * SX_PLACE_THREADS + threadIdx.x; s < w.hi; s += (uint64_t)a.xch * SX_PLACE_THREADS)
            for (uint32_t ch = 0; ch < a.C; ch++) out[(uint64_t)ch * w.stride + (s - w.lo)] = 0;
        return;
    }
    const uint32_t n = rc->nsmp;
    const uint64_t f0 = rc->first;
    for (uint32_t i = x * SX_PLACE_THREADS + threadIdx.x; i < n; i += a.xch * SX_PLACE_THREADS) {
        const uint64_t s = f0 + i;
        if (s < w.lo || s >= w.hi) continue;
        int32_t *dst = out + (s - w.lo);
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
