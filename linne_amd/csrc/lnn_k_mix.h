/* lnn_k_mix.h -- mixing the channels of sample windows of resident .lnn streams: every sample frame through the window's exact integer
 * matrix into the window's output, Co channels where the stream has C (LINNEAmd_MixWindowsDevice, which states the arithmetic; DESIGN.md
 * section 5, "Mixing channels instead of placing").
 *
 * k_wx_mix is the sibling of k_wx_place (lnn_k_windows.h): its grid, its prologue and record walk, its values (wx_value), its layouts
 * (wx_place_layout_from: the LDS image and the aligned word stores, with Co channels and this kernel's value source) -- but a lane keeps
 * all C values of its sample frame, as in lnn_k_relate.h, and forms the Co results from them in registers.  The window's matrix is one
 * WxMix record (lnn_windows_plan.h) beside its window record; it is the same for the whole workgroup, which reads it once, into LDS:
 * a row of eight int16 coefficients is then one 16-byte LDS read at an address every lane shares.  Rows >= Co and columns >= C of the
 * record hold zeros (the plan copies nothing else), so garbage in the caller's spec never reaches a product.
 *   - int32 with sample stride 1: a thread per sample frame, Co coalesced word stores, no image;
 *   - any other layout: the pieces of k_wx_place, through wx_place_layout_from;
 *   - a SILENT or WX_TAIL record holds zeros, and a matrix makes zeros of zeros: they are stored without a load or a product.
 * Plain C++ and vector stores only.
 */
#ifndef LNN_K_MIX_H_INCLUDED
#define LNN_K_MIX_H_INCLUDED

#include "lnn_k_windows.h"

struct WxMixArgs {
    WxPlaceArgs p;                      /* the walk's arguments (scale is not used: a window's own is in its WxMix) */
    const WxMix *mwin;                  /* [nwin] beside the window records */
};

/* what the workgroup keeps of its window's record in registers: the same in every lane */
struct WxMixRule { uint32_t Co, shift; int32_t lo, hi; float scale; };

/* output channel o of the frame whose values are v: sum, shift, clip (LINNEAmd_MixWindowsDevice steps 1 to 3); sat is set when the
 * clip changed the value.  mx is the record in LDS; v[c] is 0 for c >= C */
__device__ __forceinline__ int32_t wx_mix_row(const WxMix *mx, const WxMixRule &q, uint32_t C, uint32_t o, const int32_t (&v)[LINNE_MAX_NUM_CHANNELS], int &sat)
{
    const uint4 row = *(const uint4 *)mx->coef[o];
    const uint32_t pair[4] = { row.x, row.y, row.z, row.w };
    int64_t acc = 0;
#pragma unroll
    for (uint32_t c = 0; c < LINNE_MAX_NUM_CHANNELS; c++)
        if (c < C) acc += (int64_t)(int16_t)(pair[c >> 1] >> (16u * (c & 1u))) * (int64_t)v[c];      /* block-uniform */
    if (q.shift) acc = (acc + ((int64_t)1 << (q.shift - 1u))) >> q.shift;
    const int64_t y = acc > (int64_t)q.hi ? (int64_t)q.hi : (acc < (int64_t)q.lo ? (int64_t)q.lo : acc);
    sat |= (y != acc);
    return (int32_t)y;
}
/* the C values of sample i of record rc (COMPRESS or RAW) */
__device__ __forceinline__ void wx_mix_load(const WxPlaceArgs &a, const WxBlock *rc, uint32_t type, uint32_t i, int32_t (&v)[LINNE_MAX_NUM_CHANNELS])
{
#pragma unroll
    for (uint32_t c = 0; c < LINNE_MAX_NUM_CHANNELS; c++) v[c] = (c < a.C) ? wx_value(a, rc, type, i, c) : 0;
}

/* wx_place_layout_from's source: the frame's C values once, a row of the matrix per element asked for */
struct WxMixSource {
    const WxPlaceArgs &a; const WxBlock *rc; const WxMix *mx; const WxMixRule &q; uint32_t type, fmt; bool zero; uint64_t f0, sa;
    int32_t v[LINNE_MAX_NUM_CHANNELS];
    __device__ __forceinline__ void frame(uint32_t smp) { if (!zero) wx_mix_load(a, rc, type, (uint32_t)(sa + smp - f0), v); }
    __device__ __forceinline__ uint32_t get(uint32_t o, int &sat) const
    {
        if (zero) return 0u;            /* (0 in every format, the float's included) */
        return wx_convert(wx_mix_row(mx, q, a.C, o, v, sat), fmt, q.scale, sat);
    }
};

/* nrec * xch workgroups: the y-th xch of them mix record y, piece by piece as k_wx_place places it */
__global__ __launch_bounds__(SX_PLACE_THREADS) void k_wx_mix(WxMixArgs ma)
{
    __shared__ __attribute__((aligned(16))) uint8_t img[WX_IMG_BYTES];
    __shared__ __attribute__((aligned(16))) WxMix mx;
    const WxPlaceArgs &a = ma.p;
    WxRecord r;
    if (!wx_prologue(a, r)) return;
    const WxBlock *rc = r.rc;
    const WxWindow w = r.w;
    const uint32_t type = r.type, x = r.x;
    if (threadIdx.x < sizeof(WxMix) / 4u) ((uint32_t *)&mx)[threadIdx.x] = ((const uint32_t *)(ma.mwin + rc->win))[threadIdx.x];
    __syncthreads();
    WxMixRule q;
    q.Co = __builtin_amdgcn_readfirstlane(mx.Co); q.shift = __builtin_amdgcn_readfirstlane(mx.shift);
    q.lo = __builtin_amdgcn_readfirstlane(mx.lo); q.hi = __builtin_amdgcn_readfirstlane(mx.hi);
    q.scale = __uint_as_float(__builtin_amdgcn_readfirstlane(mx.scale_bits));
    const bool zero = (type != SX_COMPRESS && type != SX_RAW);     /* block-uniform */
    int sat = 0;
    if (w.fmt != LINNE_AMD_PCM_S32 || w.sstride != 1u) {         /* block-uniform */
        wx_walk(a, rc, w, type, x, [&](uint64_t f0, uint64_t sa, uint64_t sb) {
            const WxMixSource src = { a, rc, &mx, q, type, w.fmt, zero, f0, sa, {} };
            sat |= wx_place_layout_from(w, q.Co, sa, sb, img, src);
        });
        if (sat && threadIdx.x == 0) atomicOr(&a.sat[w.fidx], 1u);
        return;
    }
    /* int32 with sample stride 1: a thread per sample frame, no pieces */
    int32_t *out = (int32_t *)w.out;
    if (type == WX_TAIL) {
        const uint64_t z0 = w.covered > w.lo ? w.covered : w.lo;
        for (uint64_t s = z0 + (uint64_t)x * SX_PLACE_THREADS + threadIdx.x; s < w.hi; s += (uint64_t)a.xch * SX_PLACE_THREADS)
            for (uint32_t o = 0; o < q.Co; o++) out[(uint64_t)o * w.stride + (s - w.lo)] = 0;
        return;
    }
    const uint32_t n = rc->nsmp;
    const uint64_t f0 = rc->first;
    for (uint32_t i = x * SX_PLACE_THREADS + threadIdx.x; i < n; i += a.xch * SX_PLACE_THREADS) {
        const uint64_t s = f0 + i;
        if (s < w.lo || s >= w.hi) continue;
        int32_t *dst = out + (s - w.lo);
        if (zero) { for (uint32_t o = 0; o < q.Co; o++) dst[(uint64_t)o * w.stride] = 0; continue; }
        int32_t v[LINNE_MAX_NUM_CHANNELS];
        wx_mix_load(a, rc, type, i, v);
        for (uint32_t o = 0; o < q.Co; o++) dst[(uint64_t)o * w.stride] = wx_mix_row(&mx, q, a.C, o, v, sat);
    }
    /* (every thread comes here: the loop above leaves nobody behind) */
    if (__syncthreads_or(sat) && threadIdx.x == 0) atomicOr(&a.sat[w.fidx], 1u);
}

#endif
