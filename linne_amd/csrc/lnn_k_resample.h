/* lnn_k_resample.h -- resampling sample windows of resident .lnn streams: a rational rate change L/M through the window's exact int16
 * polyphase FIR (LINNEAmd_ResampleWindowsDevice, which states the arithmetic; DESIGN.md section 5, "Resampling instead of placing").
 *
 * The filter reads across block boundaries, which no record walk does: so the passes of the call place every window's INPUT range,
 * halo included, into an int32 planar image behind the passes' scratch (k_wx_place, with the image as its target), and one launch
 * behind the last pass filters all windows from their images:
 *   k_wx_resample_preset      the images zeroed: the zeros in front of sample 0, behind the stream's last sample and in the rounding
 *                             of a channel's stride
 *   k_wx_resample             a workgroup per tile of WXR_TILE outputs of one window (the host's tile list: the grid does not depend
 *                             on a loop over windows).  A lane owns one output sample m: its phase p = (m * M) % L and its first
 *                             input sample follow from the tile's (p0, n0) with 32-bit arithmetic.  The workgroup stages
 *                               - the coefficients (pairs of int16 in 32-bit words), at a row stride of prow | 1 words: neighbouring
 *                                 lanes read different rows when L > 1, and an odd stride spreads them over all banks whatever P
 *                                 is.  Where the window's whole table fits the rows' memory (L * (prow | 1) <= 8448 words: every
 *                                 1/M decimation, where all lanes share the one row, 160/441 and 160/147 at 32 taps) it is copied
 *                                 as it lies, L * prow coalesced words, and a lane reads row p; otherwise a row per lane, the row
 *                                 of its phase.  (WXR_WHOLE_TABLE=0 builds the second form alone: DESIGN.md has both measured);
 *                               - per channel, the tile's input span ((cnt - 1) * M + p0) / L + P samples of the image, where that
 *                                 fits WXR_XCAP words (a decimation beyond that reads the image directly: its lanes' taps are far
 *                                 apart and shared by nobody);
 *                             then every lane forms its sum -- int16 x int32 into int64, one 64-bit multiply-add per tap --, shifts
 *                             and clips it as k_wx_mix does, and the tile leaves through wx_place_layout_from / wx_convert: every
 *                             layout, the aligned word stores and `saturated` are the code k_wx_place has.  int32 with sample stride 1
 *                             is stored straight from the registers.  A tile of a window whose fail word is set is skipped.
 * Plain C++ and vector stores only.
 */
#ifndef LNN_K_RESAMPLE_H_INCLUDED
#define LNN_K_RESAMPLE_H_INCLUDED

#include "lnn_k_windows.h"

#ifndef WXR_WHOLE_TABLE
#define WXR_WHOLE_TABLE 1
#endif
#define WXR_XCAP 4096u                  /* words of a channel's input span a workgroup stages */
#define WXR_CROW ((LINNE_AMD_RESAMPLE_MAX_TAPS / 2u) | 1u)      /* the longest padded coefficient row, in words */
static_assert(WXR_TILE == SX_PLACE_THREADS, "a tile is a piece of wx_place_layout_from");

struct WxResampleArgs {
    const WxTile *tiles; uint32_t ntiles;
    const WxResample *rwin;             /* [nwin] beside the window records */
    const uint32_t *fail; uint32_t *sat;
    const int32_t *acc;                 /* the images */
    const uint32_t *coef;               /* the call's tables */
};

__global__ __launch_bounds__(256) void k_wx_resample_preset(uint4 *acc, uint64_t n16)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * 256u) acc[i] = make_uint4(0u, 0u, 0u, 0u);
}

/* the sum over a lane's taps: row its coefficient pairs (in LDS), x its first input sample */
__device__ __forceinline__ int64_t wxr_dot(const uint32_t *row, const int32_t *x, uint32_t P)
{
    int64_t acc = 0;
    for (uint32_t k = 0; 2u * k < P; k++) {                         /* block-uniform */
        const uint32_t pair = row[k];
        acc += (int64_t)(int16_t)pair * (int64_t)x[2u * k];
        if (2u * k + 1u < P) acc += (int64_t)(int16_t)(pair >> 16) * (int64_t)x[2u * k + 1u];
    }
    return acc;
}

/* wx_place_layout_from's source: the tile's clipped results, [channel][lane] in LDS */
struct WxResampleSource {
    const int32_t *res; uint32_t fmt; float scale; uint32_t smp;
    __device__ __forceinline__ void frame(uint32_t smp_) { smp = smp_; }
    __device__ __forceinline__ uint32_t get(uint32_t ch, int &sat) const { return wx_convert(res[ch * WXR_TILE + smp], fmt, scale, sat); }
};

__global__ __launch_bounds__(WXR_TILE) void k_wx_resample(WxResampleArgs a)
{
    __shared__ uint32_t cf[WXR_TILE * WXR_CROW];
    __shared__ __attribute__((aligned(16))) int32_t xs[WXR_XCAP];
    __shared__ int32_t res[LINNE_MAX_NUM_CHANNELS * WXR_TILE];
    uint8_t *img = (uint8_t *)xs;       /* the layouts' image: needed when the last span has been read */
    uint32_t *ph = (uint32_t *)res;     /* the lanes' phases: needed until their rows are staged, in front of the first result */
    static_assert(sizeof(xs) >= WX_IMG_BYTES, "the layouts' image lies where the spans lay");
    if (blockIdx.x >= a.ntiles) return;
    const WxTile t = a.tiles[blockIdx.x];
    const WxResample *r = a.rwin + t.win;
    if (a.fail[r->fidx] != WX_NOFAIL) return;                       /* block-uniform */
    const uint32_t tid = threadIdx.x;
    const uint32_t L = r->up, M = r->down, P = r->taps, C = r->C, prow = r->prow, crow = prow | 1u, shift = r->shift, fmt = r->fmt;
    const int64_t lo = r->lo, hi = r->hi;
    const uint64_t m_lo = r->m_lo, m_hi = r->m_hi, istride = r->istride, stride = r->stride;
    const uint32_t cnt = (m_hi - t.m0 < WXR_TILE) ? (uint32_t)(m_hi - t.m0) : WXR_TILE;
    const uint32_t lane = tid < cnt ? tid : cnt - 1u;               /* (a lane without an output does the last one's work again, and stores nothing) */
    const uint32_t u = t.p0 + lane * M, p = u % L, j = u / L;       /* (p0 < L <= 1024, 255 * M < 2^18) */
    const uint32_t span = (t.p0 + (cnt - 1u) * M) / L + P;          /* the input samples of the tile, per channel */
    const int32_t *image = a.acc + r->img + (t.n0 - r->n_first);    /* the tile's first input sample, channel 0 */
    /* the coefficients: the whole table, or the lanes' rows */
    const uint32_t *tab = a.coef + r->coef;
    const bool whole = WXR_WHOLE_TABLE && L * crow <= WXR_TILE * WXR_CROW;      /* block-uniform */
    if (whole) {
        for (uint32_t i = tid; i < L * prow; i += WXR_TILE) {
            const uint32_t row = i / prow, w = i - row * prow;
            cf[row * crow + w] = tab[i];
        }
    } else {
        ph[tid] = p;
        __syncthreads();
        for (uint32_t i = tid; i < cnt * prow; i += WXR_TILE) {
            const uint32_t row = i / prow, w = i - row * prow;
            cf[row * crow + w] = tab[ph[row] * prow + w];
        }
    }
    const uint32_t *mine = cf + (whole ? p : lane) * crow;
    const bool staged = span <= WXR_XCAP, direct = (fmt == LINNE_AMD_PCM_S32 && r->sstride == 1u);   /* block-uniform */
    int32_t *out = (int32_t *)r->out + (t.m0 - m_lo) + tid;
    int sat = 0;
    for (uint32_t c = 0; c < C; c++) {
        const int32_t *src = image + (uint64_t)c * istride;
        int64_t acc;
        __syncthreads();                /* (the rows are there; the last channel's span has been read) */
        if (staged) {
            for (uint32_t i = tid; i < span; i += WXR_TILE) xs[i] = src[i];
            __syncthreads();
            acc = wxr_dot(mine, xs + j, P);
        } else
            acc = wxr_dot(mine, src + j, P);
        if (shift) acc = (acc + ((int64_t)1 << (shift - 1u))) >> shift;
        const int64_t y = acc > hi ? hi : (acc < lo ? lo : acc);
        sat |= (y != acc);
        if (!direct) res[c * WXR_TILE + tid] = (int32_t)y;
        else if (tid < cnt) out[(uint64_t)c * stride] = (int32_t)y;
    }
    sat = __syncthreads_or(sat);        /* (and the results are there) */
    if (!direct) {
        WxWindow w;
        w.lo = m_lo; w.hi = m_hi; w.covered = 0u; w.out = r->out; w.stride = stride; w.fidx = r->fidx; w.fmt = fmt; w.sstride = r->sstride;
        const WxResampleSource from = { res, fmt, __uint_as_float(r->scale_bits), 0u };
        sat |= wx_place_layout_from(w, C, t.m0, t.m0 + cnt, img, from);
    }
    if (sat && tid == 0) atomicOr(&a.sat[r->fidx], 1u);
}

#endif
