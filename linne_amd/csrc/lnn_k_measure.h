/* lnn_k_measure.h -- measuring sample windows of resident .lnn streams: min, max, sum and sum of squares per channel and bucket,
 * nothing of the window's size written (LINNEAmd_MeasureWindowsDevice; DESIGN.md section 5, "Reducing instead of placing").
 *
 * k_wx_measure is the sibling of k_wx_place (lnn_k_windows.h): its grid, its prologue and record walk, its values (wx_value) -- but a
 * sample that leaves the synthesis is reduced, not stored.  The buckets, the pieces among them, the slots of a long bucket and the
 * commit behind the last pass are those of lnn_k_buckets.h; this file adds the reduction.  Bucket k of channel ch owns one
 * accumulator record (struct LINNEAmdMeasure) in the context's scratch -- slot s of a window at abase + s * C * nb -- preset by
 * k_wx_measure_preset to (INT32_MAX, INT32_MIN, 0, 0, 0).  A piece:
 *   - a SILENT or WX_TAIL record holds zeros: one lane per bucket of the piece lowers its min and raises its max to 0, no more;
 *   - few buckets: the lanes of a bucket are folded across the wave with shuffles and across the four waves through LDS, and lane
 *     (g, ch) issues channel ch's atomics on bucket k0 + g's accumulator;
 *   - many: the first lane of every bucket walks its bucket's samples in LDS, channel by channel.
 * All of it is integer arithmetic, so the order of the atomics does not show: atomicMin and atomicMax on the 32-bit fields (skipped
 * when a plain load shows they would change nothing: the fields only ever move one way), atomicAdd on sum, and atomicAdd on sumsq_lo
 * whose returned value tells whether the addition carried into sumsq_hi.  One square fits 64 bits ((2^31)^2 = 2^62); a thread keeps
 * the sum of squares as (lo, hi) with lo += q; hi += lo < q.  Plain C++ and vector stores only.
 */
#ifndef LNN_K_MEASURE_H_INCLUDED
#define LNN_K_MEASURE_H_INCLUDED

#include "lnn_k_buckets.h"

static_assert(sizeof(struct LINNEAmdMeasure) == 32, "an accumulator is one struct LINNEAmdMeasure");

struct WxMeasureArgs {
    WxPlaceArgs p;                      /* the walk's arguments (sat and scale are not used) */
    const WxBucket *mwin;               /* per channel: cstride and C are set */
    struct LINNEAmdMeasure *acc;
};

struct WxAcc { int32_t mn, mx; int64_t sum; uint64_t qlo, qhi; };
__device__ __forceinline__ void wxm_clear(WxAcc &r) { r.mn = INT32_MAX; r.mx = INT32_MIN; r.sum = 0; r.qlo = 0u; r.qhi = 0u; }
__device__ __forceinline__ void wxm_note(WxAcc &r, int32_t v)
{
    const uint64_t q = (uint64_t)((int64_t)v * (int64_t)v);
    r.mn = v < r.mn ? v : r.mn; r.mx = v > r.mx ? v : r.mx; r.sum += v;
    r.qlo += q; r.qhi += (r.qlo < q);
}
__device__ __forceinline__ void wxm_fold(WxAcc &r, int32_t mn, int32_t mx, int64_t sum, uint64_t qlo, uint64_t qhi)
{
    r.mn = mn < r.mn ? mn : r.mn; r.mx = mx > r.mx ? mx : r.mx; r.sum += sum;
    r.qlo += qlo; r.qhi += qhi + (r.qlo < qlo);
}
/* r into the accumulator at p: the fields the addition would not change are left alone */
__device__ __forceinline__ void wxm_atomics(struct LINNEAmdMeasure *p, const WxAcc &r)
{
    if (r.mn < *(volatile int32_t *)&p->min) atomicMin(&p->min, r.mn);
    if (r.mx > *(volatile int32_t *)&p->max) atomicMax(&p->max, r.mx);
    if (r.sum) atomicAdd((unsigned long long *)&p->sum, (unsigned long long)r.sum);
    uint64_t hi = r.qhi;
    if (r.qlo) { const uint64_t old = atomicAdd((unsigned long long *)&p->sumsq_lo, (unsigned long long)r.qlo); hi += (old + r.qlo < old); }
    if (hi) atomicAdd((unsigned long long *)&p->sumsq_hi, (unsigned long long)hi);
}

/* The workgroup measures samples [sa, sb) (at most SX_PLACE_THREADS, inside the window) of record rc, whose sample 0 is stream
 * sample f0.  Every barrier in here is passed by the whole workgroup: sa, sb and the buckets are block-uniform. */
__device__ __forceinline__ void wx_measure_piece(const WxMeasureArgs &ma, const WxWindow &w, const WxBucket &m, const WxBlock *rc, uint32_t type,
        uint64_t f0, uint64_t sa, uint64_t sb, WxAcc (*part)[SX_PLACE_THREADS / 64u][LINNE_MAX_NUM_CHANNELS], int32_t *vals)
{
    const WxPlaceArgs &a = ma.p;
    const WxPiece pc = wx_piece(w, m, sa, sb);
    const uint32_t t = threadIdx.x, C = a.C, len = pc.len, nseg = pc.nseg;
    const uint64_t k0 = pc.k0;
    struct LINNEAmdMeasure *acc = ma.acc + m.abase + (uint64_t)pc.slot * C * m.nb;
    if (type != SX_COMPRESS && type != SX_RAW) {
        /* zeros */
        for (uint32_t j = t; j < nseg * C; j += SX_PLACE_THREADS) {
            const uint32_t ch = j / nseg, g = j - ch * nseg;
            struct LINNEAmdMeasure *p = acc + (uint64_t)ch * m.nb + (k0 + g);
            if (0 < *(volatile int32_t *)&p->min) atomicMin(&p->min, 0);
            if (0 > *(volatile int32_t *)&p->max) atomicMax(&p->max, 0);
        }
        return;
    }
    const uint32_t i0 = (uint32_t)(sa - f0);
    if (nseg <= WXB_SEGMENTS) {
        for (uint32_t ch = 0; ch < C; ch++) {
            const int32_t v = (t < len) ? wx_value(a, rc, type, i0 + t, ch) : 0;
            for (uint32_t g = 0; g < nseg; g++) {
                uint32_t ta, te;
                pc.lanes(k0 + g, ta, te);
                const bool mine = (t >= ta && t < te);
                WxAcc r; wxm_clear(r);
                if (__ballot(mine) != 0ull) {                       /* wave-uniform */
                    if (mine) wxm_note(r, v);
                    for (int o = 32; o > 0; o >>= 1)
                        wxm_fold(r, __shfl_xor(r.mn, o), __shfl_xor(r.mx, o), (int64_t)__shfl_xor((long long)r.sum, o),
                                (uint64_t)__shfl_xor((unsigned long long)r.qlo, o), (uint64_t)__shfl_xor((unsigned long long)r.qhi, o));
                }
                if ((t & 63u) == 0u) part[g][t >> 6][ch] = r;
            }
        }
        __syncthreads();
        if (t < nseg * C) {
            const uint32_t g = t / C, ch = t - g * C;
            WxAcc r = part[g][0][ch];
            for (uint32_t k = 1; k < SX_PLACE_THREADS / 64u; k++) { const WxAcc &o = part[g][k][ch]; wxm_fold(r, o.mn, o.mx, o.sum, o.qlo, o.qhi); }
            wxm_atomics(acc + (uint64_t)ch * m.nb + (k0 + g), r);
        }
        __syncthreads();                                            /* (part is written again by the next piece) */
        return;
    }
    /* many short buckets: the piece's values in LDS, channel by channel, and the first lane of every bucket walks its samples */
    if (t < len)
        for (uint32_t ch = 0; ch < C; ch++) vals[ch * SX_PLACE_THREADS + t] = wx_value(a, rc, type, i0 + t, ch);
    __syncthreads();
    if (t < len) {
        const uint64_t k = (pc.ra + t) / m.b;
        uint32_t ta, te;
        pc.lanes(k, ta, te);
        if (t == ta) {
            for (uint32_t ch = 0; ch < C; ch++) {
                WxAcc r; wxm_clear(r);
                for (uint32_t j = ta; j < te; j++) wxm_note(r, vals[ch * SX_PLACE_THREADS + j]);
                wxm_atomics(acc + (uint64_t)ch * m.nb + k, r);
            }
        }
    }
    __syncthreads();                                                /* (vals is filled again by the next piece) */
}

/* nrec * xch workgroups: the y-th xch of them measure record y, piece by piece as k_wx_place places it */
__global__ __launch_bounds__(SX_PLACE_THREADS) void k_wx_measure(WxMeasureArgs ma)
{
    __shared__ WxAcc part[WXB_SEGMENTS][SX_PLACE_THREADS / 64u][LINNE_MAX_NUM_CHANNELS];
    __shared__ int32_t vals[LINNE_MAX_NUM_CHANNELS * SX_PLACE_THREADS];
    WxRecord r;
    if (!wx_prologue(ma.p, r)) return;
    const WxBucket m = ma.mwin[r.rc->win];
    wx_walk(ma.p, r.rc, r.w, r.type, r.x, [&](uint64_t f0, uint64_t sa, uint64_t sb) { wx_measure_piece(ma, r.w, m, r.rc, r.type, f0, sa, sb, part, vals); });
}

/* every accumulator of the call to the operations' identities */
__global__ __launch_bounds__(WXB_THREADS) void k_wx_measure_preset(struct LINNEAmdMeasure *acc, uint64_t total)
{
    struct LINNEAmdMeasure z; z.min = INT32_MAX; z.max = INT32_MIN; z.sum = 0; z.sumsq_lo = 0u; z.sumsq_hi = 0u;
    for (uint64_t g = (uint64_t)blockIdx.x * WXB_THREADS + threadIdx.x; g < total; g += (uint64_t)gridDim.x * WXB_THREADS) acc[g] = z;
}

/* A lane per (channel, bucket) of every measured window, numbered through the windows in their records' order (obase): the
 * window's slots folded and the record stored in the caller's table, unless the window's fail word is set */
__global__ __launch_bounds__(WXB_THREADS) void k_wx_measure_commit(const WxBucket *mwin, uint32_t nwin, const struct LINNEAmdMeasure *acc, const uint32_t *fail, uint64_t total)
{
    for (uint64_t g = (uint64_t)blockIdx.x * WXB_THREADS + threadIdx.x; g < total; g += (uint64_t)gridDim.x * WXB_THREADS) {
        const WxBucket m = mwin[wx_bucket_window(mwin, nwin, g)];
        if (fail[m.fidx] != WX_NOFAIL) continue;
        const uint64_t e = g - m.obase, ch = e / m.nb, k = e - ch * m.nb, C = m.C;
        const struct LINNEAmdMeasure *p = acc + m.abase + e;
        WxAcc r; wxm_clear(r);
        for (uint32_t s = 0; s < m.ns; s++, p += C * m.nb) wxm_fold(r, p->min, p->max, p->sum, p->sumsq_lo, p->sumsq_hi);
        struct LINNEAmdMeasure o; o.min = r.mn; o.max = r.mx; o.sum = r.sum; o.sumsq_lo = r.qlo; o.sumsq_hi = r.qhi;
        ((struct LINNEAmdMeasure *)m.out)[ch * m.cstride + k] = o;
    }
}

#endif
