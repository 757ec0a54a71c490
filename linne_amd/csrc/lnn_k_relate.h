/* lnn_k_relate.h -- relating the channels of sample windows of resident .lnn streams: per bucket and channel pair (i <= j) the exact
 * 128-bit sum of a_i * a_j and the counts of frames with a_i == a_j and with a_i + a_j == 0, nothing of the window's size written
 * (LINNEAmd_RelateWindowsDevice; DESIGN.md section 5, "Combining channels instead of placing").
 *
 * k_wx_relate is the sibling of k_wx_measure (lnn_k_measure.h): its grid, its prologue and record walk, its values (wx_value), its
 * buckets, pieces and slots (lnn_k_buckets.h) -- but a lane keeps all C values of its sample frame and reduces their products.  Pair
 * p = LINNE_AMD_PAIR(C, i, j) of bucket k owns one accumulator record (struct LINNEAmdRelation) in the context's scratch -- slot s of
 * a window at abase + (s * P + p) * nb + k, P = LINNE_AMD_NUM_PAIRS(C) -- zeroed by k_wx_relate_preset.  A piece:
 *   - a SILENT or WX_TAIL record holds zeros: one lane per (bucket of the piece, pair) adds the overlap's length to num_equal and to
 *     num_opposite, no more (a frame of zeros is equal and opposite in every pair; its products are 0);
 *   - few buckets: bucket after bucket and pair after pair, the two counts are the population counts of two ballots (no shuffle), and
 *     the products are folded across the wave with shuffles -- as one int64 where a ballot says that every value the wave holds lies
 *     within +-2^23 (a product is then at most 2^46 and 64 of them at most 2^52), as (lo, hi) with carries otherwise.  The choice rests
 *     on the values alone: a stream's bits_per_sample says nothing about what a crafted block decodes to.  The four waves meet in LDS,
 *     and lane (g, p) issues pair p's atomics on bucket k0 + g;
 *   - many (more than WXB_SEGMENTS, a short bucket): the lanes' values go to LDS, and the first lane of every bucket walks its bucket's
 *     frames there, pair after pair.
 * The sum is a 128-bit two's-complement integer: a product q is (uint64_t)q with q >> 63 above it, additions carry from the low
 * word, and all of it is arithmetic modulo 2^128 -- so the order of the atomics does not show.  The accumulator takes it as two 64-bit
 * atomicAdds, the value the first returns telling whether the low word carried.  Additions that would add nothing are skipped.  Plain
 * C++ and vector stores only.
 */
#ifndef LNN_K_RELATE_H_INCLUDED
#define LNN_K_RELATE_H_INCLUDED

#include "lnn_k_buckets.h"

static_assert(sizeof(struct LINNEAmdRelation) == 32, "an accumulator is one struct LINNEAmdRelation");
#define WXR_MAXPAIRS LINNE_AMD_NUM_PAIRS(LINNE_MAX_NUM_CHANNELS)
#ifndef WXR_NARROW                      /* (tools/stream_relate.py times a build with 0, which folds (lo, hi) on all but -1, 0 and 1) */
#define WXR_NARROW 23                   /* values within +-2^23: 64 products fit one int64 with room to spare */
#endif
static_assert(WXR_NARROW >= 0 && WXR_NARROW <= 28, "64 products of two values within +-2^WXR_NARROW fit one int64");
static_assert(WXB_SEGMENTS * WXR_MAXPAIRS <= SX_PLACE_THREADS, "one lane per (bucket of a piece, pair) issues the atomics, without a loop");

struct WxRelateArgs {
    WxPlaceArgs p;                      /* the walk's arguments (sat and scale are not used) */
    const WxBucket *rwin;               /* per pair: cstride (the pair stride), C and npair are set */
    struct LINNEAmdRelation *acc;
};

/* what a wave, a workgroup or a lane has of one pair of one bucket; counts of a piece fit 32 bits */
struct WxRel { uint64_t lo; int64_t hi; uint32_t eq, opp; };
__device__ __forceinline__ void wxr_add(uint64_t &lo, int64_t &hi, uint64_t olo, int64_t ohi) { lo += olo; hi += ohi + (int64_t)(lo < olo); }
/* r into the accumulator at p: the fields the addition would not change are left alone */
__device__ __forceinline__ void wxr_atomics(struct LINNEAmdRelation *p, const WxRel &r)
{
    uint64_t hi = (uint64_t)r.hi;
    if (r.lo) { const uint64_t old = atomicAdd((unsigned long long *)&p->dot_lo, (unsigned long long)r.lo); hi += (old + r.lo < old); }
    if (hi) atomicAdd((unsigned long long *)&p->dot_hi, (unsigned long long)hi);
    if (r.eq) atomicAdd((unsigned long long *)&p->num_equal, (unsigned long long)r.eq);
    if (r.opp) atomicAdd((unsigned long long *)&p->num_opposite, (unsigned long long)r.opp);
}

/* The workgroup relates sample frames [sa, sb) (at most SX_PLACE_THREADS, inside the window) of record rc, whose sample 0 is stream
 * sample f0.  Every barrier in here is passed by the whole workgroup: sa, sb and the buckets are block-uniform. */
__device__ __forceinline__ void wx_relate_piece(const WxRelateArgs &ra, const WxWindow &w, const WxBucket &m, const WxBlock *rc, uint32_t type,
        uint64_t f0, uint64_t sa, uint64_t sb, WxRel (*part)[SX_PLACE_THREADS / 64u][WXR_MAXPAIRS], int32_t *vals)
{
    const WxPlaceArgs &a = ra.p;
    const WxPiece pc = wx_piece(w, m, sa, sb);
    const uint32_t t = threadIdx.x, C = a.C, P = m.npair, len = pc.len, nseg = pc.nseg;
    const uint64_t k0 = pc.k0;
    struct LINNEAmdRelation *acc = ra.acc + m.abase + (uint64_t)pc.slot * P * m.nb;
    if (type != SX_COMPRESS && type != SX_RAW) {
        /* zeros */
        for (uint32_t j = t; j < nseg * P; j += SX_PLACE_THREADS) {
            const uint32_t p = j / nseg, g = j - p * nseg;
            uint32_t ta, te;
            pc.lanes(k0 + g, ta, te);
            WxRel r; r.lo = 0u; r.hi = 0; r.eq = r.opp = te - ta;
            wxr_atomics(acc + (uint64_t)p * m.nb + (k0 + g), r);
        }
        return;
    }
    const uint32_t i0 = (uint32_t)(sa - f0);
    if (nseg <= WXB_SEGMENTS) {
        int32_t v[LINNE_MAX_NUM_CHANNELS];
        bool wide = false;
#pragma unroll
        for (uint32_t ch = 0; ch < LINNE_MAX_NUM_CHANNELS; ch++) {
            v[ch] = (ch < C && t < len) ? wx_value(a, rc, type, i0 + t, ch) : 0;
            wide |= (uint32_t)v[ch] + (1u << WXR_NARROW) > (2u << WXR_NARROW);
        }
        const bool narrow = __ballot(wide) == 0ull;                 /* wave-uniform: every value of this wave's 64 frames is within +-2^23 */
        for (uint32_t g = 0; g < nseg; g++) {
            uint32_t ta, te;
            pc.lanes(k0 + g, ta, te);
            const bool mine = (t >= ta && t < te);
            const bool any = __ballot(mine) != 0ull;                /* wave-uniform */
#pragma unroll
            for (uint32_t i = 0; i < LINNE_MAX_NUM_CHANNELS; i++) {
#pragma unroll
                for (uint32_t j = i; j < LINNE_MAX_NUM_CHANNELS; j++) {
                    if (j >= C) continue;                           /* block-uniform */
                    WxRel r; r.lo = 0u; r.hi = 0; r.eq = r.opp = 0u;
                    if (any) {
                        r.eq = (uint32_t)__popcll(__ballot(mine && v[i] == v[j]));
                        r.opp = (uint32_t)__popcll(__ballot(mine && (int64_t)v[i] + (int64_t)v[j] == 0));
                        const int64_t q = mine ? (int64_t)v[i] * (int64_t)v[j] : 0;
                        if (narrow) {
                            int64_t s = q;
                            for (int o = 32; o > 0; o >>= 1) s += (int64_t)__shfl_xor((long long)s, o);
                            r.lo = (uint64_t)s; r.hi = s >> 63;
                        } else {
                            r.lo = (uint64_t)q; r.hi = q >> 63;
                            for (int o = 32; o > 0; o >>= 1) {
                                const uint64_t olo = (uint64_t)__shfl_xor((unsigned long long)r.lo, o);
                                const int64_t ohi = (int64_t)__shfl_xor((long long)r.hi, o);
                                wxr_add(r.lo, r.hi, olo, ohi);
                            }
                        }
                    }
                    if ((t & 63u) == 0u) part[g][t >> 6][LINNE_AMD_PAIR(C, i, j)] = r;
                }
            }
        }
        __syncthreads();
        if (t < nseg * P) {
            const uint32_t g = t / P, p = t - g * P;
            WxRel r = part[g][0][p];
            for (uint32_t k = 1; k < SX_PLACE_THREADS / 64u; k++) { const WxRel &o = part[g][k][p]; wxr_add(r.lo, r.hi, o.lo, o.hi); r.eq += o.eq; r.opp += o.opp; }
            wxr_atomics(acc + (uint64_t)p * m.nb + (k0 + g), r);
        }
        __syncthreads();                                            /* (part is written again by the next piece) */
        return;
    }
    /* many short buckets: the piece's values in LDS, channel by channel, and the first lane of every bucket walks its frames */
    if (t < len)
        for (uint32_t ch = 0; ch < C; ch++) vals[ch * SX_PLACE_THREADS + t] = wx_value(a, rc, type, i0 + t, ch);
    __syncthreads();
    if (t < len) {
        const uint64_t k = (pc.ra + t) / m.b;
        uint32_t ta, te;
        pc.lanes(k, ta, te);
        if (t == ta) {
            uint32_t p = 0;
            for (uint32_t i = 0; i < C; i++)
                for (uint32_t j = i; j < C; j++, p++) {
                    const int32_t *x = vals + i * SX_PLACE_THREADS, *y = vals + j * SX_PLACE_THREADS;
                    WxRel r; r.lo = 0u; r.hi = 0; r.eq = r.opp = 0u;
                    for (uint32_t s = ta; s < te; s++) {
                        const int64_t q = (int64_t)x[s] * (int64_t)y[s];
                        wxr_add(r.lo, r.hi, (uint64_t)q, q >> 63);
                        r.eq += (x[s] == y[s]); r.opp += ((int64_t)x[s] + (int64_t)y[s] == 0);
                    }
                    wxr_atomics(acc + (uint64_t)p * m.nb + k, r);
                }
        }
    }
    __syncthreads();                                                /* (vals is filled again by the next piece) */
}

/* nrec * xch workgroups: the y-th xch of them relate record y, piece by piece as k_wx_place places it */
__global__ __launch_bounds__(SX_PLACE_THREADS) void k_wx_relate(WxRelateArgs ra)
{
    __shared__ WxRel part[WXB_SEGMENTS][SX_PLACE_THREADS / 64u][WXR_MAXPAIRS];
    __shared__ int32_t vals[LINNE_MAX_NUM_CHANNELS * SX_PLACE_THREADS];
    WxRecord r;
    if (!wx_prologue(ra.p, r)) return;
    const WxBucket m = ra.rwin[r.rc->win];
    wx_walk(ra.p, r.rc, r.w, r.type, r.x, [&](uint64_t f0, uint64_t sa, uint64_t sb) { wx_relate_piece(ra, r.w, m, r.rc, r.type, f0, sa, sb, part, vals); });
}

/* every accumulator of the call to zero */
__global__ __launch_bounds__(WXB_THREADS) void k_wx_relate_preset(struct LINNEAmdRelation *acc, uint64_t total)
{
    struct LINNEAmdRelation z; z.dot_lo = 0u; z.dot_hi = 0; z.num_equal = 0u; z.num_opposite = 0u;
    for (uint64_t g = (uint64_t)blockIdx.x * WXB_THREADS + threadIdx.x; g < total; g += (uint64_t)gridDim.x * WXB_THREADS) acc[g] = z;
}

/* A lane per (pair, bucket) of every related window, numbered through the windows in their records' order (obase): the window's
 * slots added up with carries and the record stored in the caller's table, unless the window's fail word is set */
__global__ __launch_bounds__(WXB_THREADS) void k_wx_relate_commit(const WxBucket *rwin, uint32_t nwin, const struct LINNEAmdRelation *acc, const uint32_t *fail, uint64_t total)
{
    for (uint64_t g = (uint64_t)blockIdx.x * WXB_THREADS + threadIdx.x; g < total; g += (uint64_t)gridDim.x * WXB_THREADS) {
        const WxBucket m = rwin[wx_bucket_window(rwin, nwin, g)];
        if (fail[m.fidx] != WX_NOFAIL) continue;
        const uint64_t e = g - m.obase, p = e / m.nb, k = e - p * m.nb;
        const struct LINNEAmdRelation *s = acc + m.abase + e;
        struct LINNEAmdRelation o; o.dot_lo = 0u; o.dot_hi = 0; o.num_equal = 0u; o.num_opposite = 0u;
        for (uint32_t n = 0; n < m.ns; n++, s += (uint64_t)m.npair * m.nb) {
            wxr_add(o.dot_lo, o.dot_hi, s->dot_lo, s->dot_hi);
            o.num_equal += s->num_equal; o.num_opposite += s->num_opposite;
        }
        ((struct LINNEAmdRelation *)m.out)[p * m.cstride + k] = o;
    }
}

#endif
