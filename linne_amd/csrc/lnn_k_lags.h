/* lnn_k_lags.h -- sliding sample windows of one resident .lnn stream over another: per channel pair and lag the exact 128-bit sum of
 * a[i] * b[i + lag] and the sum of b^2 under the needle, and the needle's own sum of squares (LINNEAmd_LagWindowsDevice, which states
 * the arithmetic; DESIGN.md section 5, "Sliding instead of placing").
 *
 * A lag's sum depends on two ranges, which no record walk sees together: so the passes of the call place every probe's needle and its
 * clipped haystack into int32 planar images behind the passes' scratch (k_wx_place, exactly as an overlay's sources), and two launches
 * behind the last pass work from the images.  wx_value gives 0 for SILENT blocks and the tail: the passes write every word of an image
 * that is read, and nothing zeroes them.
 *   k_wx_lags          a workgroup per tile (the host's tile list: a probe's pair, WXL_LAGS lags from l0 on, a chunk of at most WXL_CHUNK
 *                      needle samples), a lane per lag, four waves.  The chunk goes through LDS in sub-tiles of WXL_SUB needle words and
 *                      the WXL_SUB + WXL_LAGS - 1 haystack words they meet; a haystack word whose index falls outside the image is
 *                      staged as 0, which is how a range off the stream's ends costs the inner loop nothing.  The inner loop is
 *                      acc += (int64)a[i] * b[i + lane]: the needle word is one LDS address for the whole wave, a broadcast, and the
 *                      haystack words are consecutive per lane.  WXL_BLOCK needle words are fetched at a time (one 16-byte broadcast
 *                      read for four of them); WXL_BLOCK 1 is the plain loop.  Exactness is relate's rule (WXR_NARROW's reasoning):
 *                      where every word of a sub-tile, needle and haystack, lies within +-2^WXL_NARROW -- the staging lanes tell, and
 *                      the barrier that ends the staging carries the answer to all four waves --, the products go into one int64 per
 *                      lane (a product is at most 2^46, the 65536 of a chunk at most 2^62); otherwise into (lo, hi) with carries.  The
 *                      choice rests on the values alone.  The staging lanes also square what they stage: the chunk's share of b^2 at
 *                      the tile's first lag and of a^2.  A tile WRITES its partial sums into its own place among the accumulators:
 *                      no atomics, no zeroing launch, and nothing depends on the order in which tiles run.  A tile of a probe whose
 *                      needle or haystack has its fail word set returns at once (block-uniform).  A wave whose 64 lags all lie behind
 *                      the probe's last one stages and waits with the others and skips the inner loop: with few lags the device does
 *                      n * (num_lags rounded up to 64) products per pair, not 256 per lag asked for.  a^2 is squared and reduced by
 *                      the tiles of a pair's first run alone, the only ones the commit reads it from.
 *   k_wx_lags_commit   a workgroup per run of tiles (a probe's pair, WXL_LAGS lags; the chunks of a run follow each other), a lane per
 *                      lag: the chunks' partial dots added with carries; b^2 at the run's first lag from the chunks' shares, and at the
 *                      following lags by the square that enters minus the square that leaves, as a 128-bit prefix sum over the lanes;
 *                      a^2 by the first run of a pair.  Nothing is written for a probe with a fail word set.
 * Plain C++ and vector stores only.
 */
#ifndef LNN_K_LAGS_H_INCLUDED
#define LNN_K_LAGS_H_INCLUDED

#include "lnn_k_windows.h"

#ifndef WXL_NARROW                      /* (tools/stream_lags.py times a build with 0, which takes (lo, hi) on all but -1, 0 and 1) */
#define WXL_NARROW 23                   /* values within +-2^23: the 65536 products of a chunk fit one int64 */
#endif
#ifndef WXL_BLOCK                       /* needle words fetched per step of the inner loop: 1 (plain) or 4 */
#define WXL_BLOCK 4
#endif
#define WXL_SUB 1024u                   /* needle words of a sub-tile */
static_assert(WXL_NARROW >= 0 && WXL_NARROW <= 23, "WXL_CHUNK products of two values within +-2^WXL_NARROW fit one int64");
static_assert(WXL_BLOCK == 1 || WXL_BLOCK == 4, "the inner loop takes 1 or 4 needle words per step");
static_assert(WXL_SUB % 4u == 0 && WXL_CHUNK % WXL_SUB == 0 && WXL_SUB % WXL_LAGS == 0, "whole steps, whole sub-tiles, whole staging rounds");
static_assert(sizeof(struct LINNEAmdLagSum) == 32, "a table element is four 64-bit words");

struct WxLagsArgs {
    const WxLagTile *tiles; uint32_t ntiles;
    const uint32_t *runs; uint32_t nruns;       /* the commit's: the first tile of every run */
    const WxLagProbe *probes;
    const WxLagImage *imgs;             /* [W] a record per window of the call */
    const uint32_t *fail;
    const int32_t *acc;                 /* the images */
    uint64_t *part;                     /* the partial sums: WXL_PART_WORDS words per tile */
};

__device__ __forceinline__ void wxl_add(uint64_t &lo, uint64_t &hi, uint64_t olo, uint64_t ohi) { lo += olo; hi += ohi + (uint64_t)(lo < olo); }
__device__ __forceinline__ void wxl_add_square(uint64_t &lo, uint64_t &hi, int32_t v) { const uint64_t q = (uint64_t)((int64_t)v * (int64_t)v); lo += q; hi += (uint64_t)(lo < q); }
__device__ __forceinline__ void wxl_add_product(uint64_t &lo, uint64_t &hi, int32_t x, int32_t y) { const int64_t q = (int64_t)x * (int64_t)y; wxl_add(lo, hi, (uint64_t)q, (uint64_t)(q >> 63)); }
__device__ __forceinline__ bool wxl_wide(int32_t v) { return (uint32_t)v + (1u << WXL_NARROW) > (2u << WXL_NARROW); }
/* a probe with a fail word set: the same answer in every lane */
__device__ __forceinline__ bool wxl_failed(const WxLagsArgs &a, const WxLagProbe *q) { return a.fail[q->wa] != WX_NOFAIL || (q->wb != WXL_NOWIN && a.fail[q->wb] != WX_NOFAIL); }
/* the whole workgroup's 128-bit sum of (lo, hi), in every lane; red has a slot per wave */
__device__ __forceinline__ void wxl_block_sum(uint64_t &lo, uint64_t &hi, uint64_t (*red)[2])
{
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t olo = (uint64_t)__shfl_xor((unsigned long long)lo, o), ohi = (uint64_t)__shfl_xor((unsigned long long)hi, o);
        wxl_add(lo, hi, olo, ohi);
    }
    __syncthreads();                    /* (red may still be read from the sum before) */
    if ((threadIdx.x & 63u) == 0u) { red[threadIdx.x >> 6][0] = lo; red[threadIdx.x >> 6][1] = hi; }
    __syncthreads();
    lo = red[0][0]; hi = red[0][1];
    for (uint32_t w = 1; w < WXL_LAGS / 64u; w++) wxl_add(lo, hi, red[w][0], red[w][1]);
}

__global__ __launch_bounds__(WXL_LAGS) void k_wx_lags(WxLagsArgs a)
{
    __shared__ __attribute__((aligned(16))) int32_t as[WXL_SUB];
    __shared__ __attribute__((aligned(16))) int32_t bs[WXL_SUB + WXL_LAGS - 1u];
    __shared__ uint64_t red[WXL_LAGS / 64u][2];
    if (blockIdx.x >= a.ntiles) return;
    const WxLagTile t = a.tiles[blockIdx.x];
    const WxLagProbe *q = a.probes + t.probe;
    if (wxl_failed(a, q)) return;
    const uint32_t tid = threadIdx.x;
    const WxLagImage ia = a.imgs[q->wa];
    const bool has_b = q->wb != WXL_NOWIN;                             /* block-uniform */
    const uint64_t nb = has_b ? a.imgs[q->wb].n : 0u;
    const int32_t *pa = a.acc + ia.img + (uint64_t)q->ca[t.pair] * ia.istride;
    const int32_t *pb = has_b ? a.acc + a.imgs[q->wb].img + (uint64_t)q->cb[t.pair] * a.imgs[q->wb].istride : a.acc;
    const uint64_t i0 = (uint64_t)t.chunk * WXL_CHUNK;
    const uint32_t len = (q->n - i0 < WXL_CHUNK) ? (uint32_t)(q->n - i0) : WXL_CHUNK;
    const int64_t j0 = q->b0 + (int64_t)t.l0 + (int64_t)i0;            /* the haystack word under needle word i0 at the tile's first lag */
    const bool first_run = t.l0 == 0u;                                 /* block-uniform: the commit reads a^2 from a pair's first run alone */
    /* a wave whose lags all lie behind the probe's last takes part in the staging and the barriers and skips the products */
    const bool idle = t.l0 + (tid & ~63u) >= q->nlags;                 /* wave-uniform */
    int64_t narrow_sum = 0;
    uint64_t lo = 0u, hi = 0u, a_lo = 0u, a_hi = 0u, b_lo = 0u, b_hi = 0u;
    for (uint32_t s0 = 0; s0 < len; s0 += WXL_SUB) {
        const uint32_t sub = (len - s0 < WXL_SUB) ? len - s0 : WXL_SUB;
        bool wide = false;
        for (uint32_t k = tid; k < WXL_SUB; k += WXL_LAGS) {
            const int32_t v = (k < sub) ? pa[i0 + s0 + k] : 0;
            as[k] = v; wide |= wxl_wide(v);
            if (first_run) wxl_add_square(a_lo, a_hi, v);
        }
        for (uint32_t k = tid; k < WXL_SUB + WXL_LAGS - 1u; k += WXL_LAGS) {   /* (the words the inner loop reads, no more) */
            const int64_t j = j0 + (int64_t)s0 + (int64_t)k;
            const int32_t v = (j >= 0 && (uint64_t)j < nb) ? pb[j] : 0;
            bs[k] = v; wide |= wxl_wide(v);
            if (k < sub) wxl_add_square(b_lo, b_hi, v);
        }
        const bool narrow = !__syncthreads_or(wide);                   /* block-uniform; and the sub-tile is there */
        const int32_t *bl = bs + tid;
        const uint32_t kend = (sub + 3u) & ~3u;                        /* (the needle words behind `sub` are zeros) */
        if (idle) {
        } else if (narrow) {
            int64_t s = 0;
#if WXL_BLOCK == 4
            for (uint32_t k = 0; k < kend; k += 4u) {
                const int4 av = *(const int4 *)(as + k);
                s += (int64_t)av.x * (int64_t)bl[k] + (int64_t)av.y * (int64_t)bl[k + 1u] + (int64_t)av.z * (int64_t)bl[k + 2u] + (int64_t)av.w * (int64_t)bl[k + 3u];
            }
#else
            for (uint32_t k = 0; k < kend; k++) s += (int64_t)as[k] * (int64_t)bl[k];
#endif
            narrow_sum += s;
        } else {
#if WXL_BLOCK == 4
            for (uint32_t k = 0; k < kend; k += 4u) {
                const int4 av = *(const int4 *)(as + k);
                wxl_add_product(lo, hi, av.x, bl[k]); wxl_add_product(lo, hi, av.y, bl[k + 1u]);
                wxl_add_product(lo, hi, av.z, bl[k + 2u]); wxl_add_product(lo, hi, av.w, bl[k + 3u]);
            }
#else
            for (uint32_t k = 0; k < kend; k++) wxl_add_product(lo, hi, as[k], bl[k]);
#endif
        }
        __syncthreads();                /* (the next sub-tile overwrites this one) */
    }
    wxl_add(lo, hi, (uint64_t)narrow_sum, (uint64_t)(narrow_sum >> 63));
    uint64_t *part = a.part + (uint64_t)blockIdx.x * WXL_PART_WORDS;
    part[2u * tid] = lo; part[2u * tid + 1u] = hi;
    wxl_block_sum(b_lo, b_hi, red);
    if (first_run) wxl_block_sum(a_lo, a_hi, red);
    if (tid == 0) { uint64_t *side = part + 2u * WXL_LAGS; side[0] = b_lo; side[1] = b_hi; side[2] = a_lo; side[3] = a_hi; }
}

__global__ __launch_bounds__(WXL_LAGS) void k_wx_lags_commit(WxLagsArgs a)
{
    __shared__ uint64_t scan[2][WXL_LAGS][2];
    if (blockIdx.x >= a.nruns) return;
    const uint32_t k0 = a.runs[blockIdx.x];
    const WxLagTile t = a.tiles[k0];
    const WxLagProbe *q = a.probes + t.probe;
    if (wxl_failed(a, q)) return;
    const uint32_t tid = threadIdx.x, nchunk = q->nchunk;
    const uint64_t *part = a.part + (uint64_t)k0 * WXL_PART_WORDS;
    uint64_t lo = 0u, hi = 0u, a_lo = 0u, a_hi = 0u, b_lo = 0u, b_hi = 0u;
    for (uint32_t c = 0; c < nchunk; c++, part += WXL_PART_WORDS) wxl_add(lo, hi, part[2u * tid], part[2u * tid + 1u]);
    if (tid == 0) {
        /* b^2 at the run's first lag; the lanes behind it bring the square that enters minus the square that leaves */
        const uint64_t *side = a.part + (uint64_t)k0 * WXL_PART_WORDS + 2u * WXL_LAGS;
        for (uint32_t c = 0; c < nchunk; c++, side += WXL_PART_WORDS) { wxl_add(b_lo, b_hi, side[0], side[1]); wxl_add(a_lo, a_hi, side[2], side[3]); }
    } else if (q->wb != WXL_NOWIN) {
        const WxLagImage ib = a.imgs[q->wb];
        const int32_t *pb = a.acc + ib.img + (uint64_t)q->cb[t.pair] * ib.istride;
        const int64_t leaves = q->b0 + (int64_t)t.l0 + (int64_t)tid - 1, enters = leaves + (int64_t)q->n;
        const int32_t ve = (enters >= 0 && (uint64_t)enters < ib.n) ? pb[enters] : 0, vl = (leaves >= 0 && (uint64_t)leaves < ib.n) ? pb[leaves] : 0;
        const uint64_t qe = (uint64_t)((int64_t)ve * (int64_t)ve), ql = (uint64_t)((int64_t)vl * (int64_t)vl);
        b_lo = qe - ql; b_hi = (uint64_t)0 - (uint64_t)(qe < ql);     /* modulo 2^128: the prefix sums are the b^2 themselves, never negative */
    }
    uint32_t cur = 0;
    scan[0][tid][0] = b_lo; scan[0][tid][1] = b_hi;
    __syncthreads();
    for (uint32_t d = 1; d < WXL_LAGS; d <<= 1, cur ^= 1u) {
        uint64_t slo = scan[cur][tid][0], shi = scan[cur][tid][1];
        if (tid >= d) wxl_add(slo, shi, scan[cur][tid - d][0], scan[cur][tid - d][1]);
        scan[cur ^ 1u][tid][0] = slo; scan[cur ^ 1u][tid][1] = shi;
        __syncthreads();
    }
    if (t.l0 + tid < q->nlags) {
        uint64_t *o = (uint64_t *)((struct LINNEAmdLagSum *)q->out + ((uint64_t)t.pair * q->pstride + t.l0 + tid));
        o[0] = lo; o[1] = hi; o[2] = scan[cur][tid][0]; o[3] = scan[cur][tid][1];
    }
    if (tid == 0 && t.l0 == 0u && q->a_sq) { q->a_sq[2u * t.pair] = a_lo; q->a_sq[2u * t.pair + 1u] = a_hi; }
}

#endif
