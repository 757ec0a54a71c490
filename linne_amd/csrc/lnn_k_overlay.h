/* lnn_k_overlay.h -- overlaying sample windows of several resident .lnn streams: every output sample is the sum of the sources that
 * cover it, each under a gain that moves linearly over the source (LINNEAmd_OverlayWindowsDevice, which states the arithmetic;
 * DESIGN.md section 5, "Overlaying instead of placing").
 *
 * An output depends on several streams, which no record walk sees together: so the passes of the call place every SOURCE's range into
 * an int32 planar image behind the passes' scratch (k_wx_place, with the image as its target, exactly as a resampled window's), and
 * one launch behind the last pass sums all outputs from their sources' images.  A source's range lies inside its stream, and
 * wx_value gives 0 for SILENT blocks and the tail: the passes write every word of an image that is read, and nothing zeroes them.
 *   k_wx_overlay              a workgroup per tile of WXR_TILE output samples of one output (the host's tile list: the grid does not
 *                             depend on a loop over outputs).  The workgroup first reads the fail words of the output's sources, a
 *                             lane each: one set, and the tile is skipped.  A lane owns output sample t and keeps the C <= 8 sums in
 *                             registers.  The source loop is outside -- a source that does not meet the tile is skipped by the whole
 *                             workgroup, and a lane's gain, one 64-bit multiply-add and a shift, is formed once per source --, the
 *                             channel loop inside: int16 x int32 into int64.  The images are read straight from global memory:
 *                             consecutive lanes read consecutive words and no word is read twice, so there is nothing to stage.
 *                             Shift, clip and `saturated` are k_wx_resample's tail: int32 with sample stride 1 is stored from the
 *                             registers, every other layout leaves through wx_place_layout_from / wx_convert.
 * Plain C++ and vector stores only.
 */
#ifndef LNN_K_OVERLAY_H_INCLUDED
#define LNN_K_OVERLAY_H_INCLUDED

#include "lnn_k_resample.h"

static_assert(LINNE_AMD_OVERLAY_MAX_SOURCES <= WXR_TILE, "a lane per source reads the fail words");

struct WxOverlayArgs {
    const WxTile *tiles; uint32_t ntiles;
    const WxOvOutput *outs;             /* the outputs that have tiles */
    const WxOvSource *srcs;             /* [W] a record per window of the call */
    const uint32_t *fail; uint32_t *sat;
    const int32_t *acc;                 /* the images */
};

__global__ __launch_bounds__(WXR_TILE) void k_wx_overlay(WxOverlayArgs a)
{
    __shared__ int32_t res[LINNE_MAX_NUM_CHANNELS * WXR_TILE];
    __shared__ __attribute__((aligned(16))) uint8_t img[WX_IMG_BYTES];
    if (blockIdx.x >= a.ntiles) return;
    const WxTile t = a.tiles[blockIdx.x];
    const WxOvOutput *o = a.outs + t.win;
    const uint32_t tid = threadIdx.x, nsrc = o->nsrc, src0 = o->src0;
    if (__syncthreads_or(tid < nsrc && a.fail[src0 + tid] != WX_NOFAIL)) return;    /* block-uniform */
    const uint32_t C = o->C, shift = o->shift, fmt = o->fmt;
    const int64_t lo = o->lo, hi = o->hi;
    const uint64_t n = o->n, stride = o->stride, t0 = t.m0;
    const uint32_t cnt = (n - t0 < WXR_TILE) ? (uint32_t)(n - t0) : WXR_TILE;
    const uint64_t mine = t0 + tid;
    int64_t acc[LINNE_MAX_NUM_CHANNELS];
#pragma unroll
    for (uint32_t c = 0; c < LINNE_MAX_NUM_CHANNELS; c++) acc[c] = 0;
    for (uint32_t k = 0; k < nsrc; k++) {
        const WxOvSource *s = a.srcs + src0 + k;
        const uint64_t at = s->at, ns = s->n;
        if (at + ns <= t0 || at >= t0 + cnt) continue;              /* block-uniform */
        if (tid < cnt && mine >= at && mine - at < ns) {
            const uint64_t i = mine - at, istride = s->istride;
            const int32_t g = (int32_t)((s->gain + s->step * (int64_t)i) >> 32);    /* (in int16: the host checked the ramp's ends) */
            const int32_t *x = a.acc + s->img + i;
#pragma unroll
            for (uint32_t c = 0; c < LINNE_MAX_NUM_CHANNELS; c++)
                if (c < C) acc[c] += (int64_t)g * (int64_t)x[(uint64_t)c * istride];
        }
    }
    const bool direct = (fmt == LINNE_AMD_PCM_S32 && o->sstride == 1u);     /* block-uniform */
    int32_t *out = (int32_t *)o->out + mine;
    int sat = 0;
#pragma unroll
    for (uint32_t c = 0; c < LINNE_MAX_NUM_CHANNELS; c++) {
        if (c >= C) continue;
        int64_t v = acc[c];
        if (shift) v = (v + ((int64_t)1 << (shift - 1u))) >> shift;
        const int64_t y = v > hi ? hi : (v < lo ? lo : v);
        sat |= (y != v);
        if (!direct) res[c * WXR_TILE + tid] = (int32_t)y;
        else if (tid < cnt) out[(uint64_t)c * stride] = (int32_t)y;
    }
    sat = __syncthreads_or(sat);        /* (and the results are there) */
    if (!direct) {
        WxWindow w;
        w.lo = 0u; w.hi = n; w.covered = 0u; w.out = o->out; w.stride = stride; w.fidx = src0; w.fmt = fmt; w.sstride = o->sstride;
        const WxResampleSource from = { res, fmt, __uint_as_float(o->scale_bits), 0u };
        sat |= wx_place_layout_from(w, C, t0, t0 + cnt, img, from);
    }
    if (sat && tid == 0) atomicOr(&a.sat[src0], 1u);
}

#endif
