/* lnn_k_compare.h -- comparing sample windows of resident .lnn streams with the caller's resident PCM (LINNEAmd_CompareWindowsDevice;
 * DESIGN.md section 5, "Comparing instead of placing").
 *
 * k_wx_compare is the sibling of k_wx_place (lnn_k_windows.h): its grid, its prologue and record walk (wx_prologue, wx_walk), its
 * values (wx_value) -- but where k_wx_place converts and stores a sample, this kernel loads the caller's element (lnn_k_pcm_load.h) and compares.  Per
 * window the call wants two numbers: how many (sample, channel) elements differ, and the first of them -- lowest sample, then lowest
 * channel, which is the least key (s - lo) * 8 + ch (LINNE_MAX_NUM_CHANNELS is 8).  A thread keeps a count and a least key, a wave
 * reduces them across its lanes, the workgroup through LDS, and only a workgroup that found a difference touches global memory: one
 * 64-bit atomicAdd on its window's count and one 64-bit atomicMin on its window's key.  Equal windows -- the case a verified encode
 * meets -- issue no atomic and no store at all.  Nothing here writes the caller's PCM.
 *
 * An S16 or S24 element is sign-extended and compared with the decoded int32 value as it is: nothing is saturated, so a decoded value
 * outside the format's range differs from every element.
 */
#ifndef LNN_K_COMPARE_H_INCLUDED
#define LNN_K_COMPARE_H_INCLUDED

#include "lnn_k_pcm_load.h"

static_assert(LINNE_MAX_NUM_CHANNELS == 8, "a difference's key is (s - lo) * 8 + ch");
static_assert(SX_PLACE_THREADS == 256u, "k_wx_compare reduces over four waves of 64");

struct WxCompareArgs {
    WxPlaceArgs p;                      /* the walk's arguments (sat and scale are not used) */
    unsigned long long *diff;           /* [W][2] beside the fail words: a window's count of differing elements (0), its least key (~0) */
};

struct WxDiff { uint32_t cnt; uint64_t key; };
__device__ __forceinline__ void wx_diff_note(WxDiff &d, bool differs, uint64_t rel, uint32_t ch)
{
    if (!differs) return;
    const uint64_t k = rel * 8u + ch;
    d.cnt++;
    if (k < d.key) d.key = k;
}

/* The workgroup compares samples [sa, sb) (at most SX_PLACE_THREADS, inside the window) of record rc, whose sample 0 is stream sample
 * f0.  The pieces k_wx_place_layout lays out in LDS are contiguous runs here too: every channel's for sample stride 1 (the run: that
 * channel's elements of the window), the whole piece's for packed interleaved (the run: the window); they are read through ly_load4
 * with the run's bounds -- four elements a lane for S16 and S24, one for S32, whose elements are whole aligned words.  Any other
 * strides: ly_load1 per element. */
__device__ __forceinline__ void wx_compare_piece(const WxPlaceArgs &a, const WxWindow &w, const WxBlock *rc, uint32_t type, uint64_t f0,
        uint64_t sa, uint64_t sb, WxDiff &d)
{
    const uint32_t fmt = w.fmt, es = fmt == LINNE_AMD_PCM_S16 ? 2u : (fmt == LINNE_AMD_PCM_S24 ? 3u : 4u);
    const uint32_t m = (uint32_t)(sb - sa), t = threadIdx.x, C = a.C;
    const uint8_t *base = (const uint8_t *)w.out;
    const uint64_t n = w.hi - w.lo, r0 = sa - w.lo;
    const uint32_t i0 = (uint32_t)(sa - f0);
    const bool packed = (w.stride == 1u && w.sstride == C), planar = (w.sstride == 1u);
    if (!packed && !planar) {
        for (uint32_t k = t; k < m * C; k += SX_PLACE_THREADS) {
            const uint32_t smp = k / C, ch = k - smp * C;
            const int32_t v = ly_load1(base + ((uint64_t)ch * w.stride + (r0 + smp) * w.sstride) * es, fmt);
            wx_diff_note(d, v != wx_value(a, rc, type, i0 + smp, ch), r0 + smp, ch);
        }
        return;
    }
    const uint32_t per = (fmt == LINNE_AMD_PCM_S32) ? 1u : 4u;
    int32_t v[4];
    if (planar) {
        const uint32_t nq = (m + per - 1u) / per;
        for (uint32_t k = t; k < nq * C; k += SX_PLACE_THREADS) {
            const uint32_t ch = k / nq, q0 = (k - ch * nq) * per, cnt = (m - q0 < per) ? m - q0 : per;
            const uint8_t *lo = base + (uint64_t)ch * w.stride * es, *hi = lo + n * es;
            ly_load4(lo + (r0 + q0) * es, lo, hi, fmt, cnt, v);
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++)
                if (j < cnt) wx_diff_note(d, v[j] != wx_value(a, rc, type, i0 + q0 + j, ch), r0 + q0 + j, ch);
        }
        return;
    }
    const uint8_t *lo = base, *hi = base + n * C * es;
    const uint32_t ne = m * C;
    for (uint32_t k0 = t * per; k0 < ne; k0 += SX_PLACE_THREADS * per) {
        const uint32_t cnt = (ne - k0 < per) ? ne - k0 : per;
        ly_load4(lo + (r0 * C + k0) * es, lo, hi, fmt, cnt, v);
        uint32_t smp = k0 / C, ch = k0 - smp * C;
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            if (j < cnt) wx_diff_note(d, v[j] != wx_value(a, rc, type, i0 + smp, ch), r0 + smp, ch);
            if (++ch == C) { ch = 0; smp++; }
        }
    }
}

/* nrec * xch workgroups: the y-th xch of them compare record y, piece by piece as k_wx_place places it */
__global__ __launch_bounds__(SX_PLACE_THREADS) void k_wx_compare(WxCompareArgs ca)
{
    __shared__ uint32_t s_cnt[SX_PLACE_THREADS / 64u];
    __shared__ uint64_t s_key[SX_PLACE_THREADS / 64u];
    const WxPlaceArgs &a = ca.p;
    WxRecord r;
    if (!wx_prologue(a, r)) return;                                /* block-uniform, as every exit before the barrier below */
    const WxWindow &w = r.w;
    WxDiff d; d.cnt = 0u; d.key = ~(uint64_t)0;
    wx_walk(a, r.rc, w, r.type, r.x, [&](uint64_t f0, uint64_t sa, uint64_t sb) { wx_compare_piece(a, w, r.rc, r.type, f0, sa, sb, d); });
    if (!__syncthreads_or(d.cnt != 0u)) return;                    /* equal: nothing more */
    for (int o = 32; o > 0; o >>= 1) {
        d.cnt += (uint32_t)__shfl_xor((int)d.cnt, o);
        const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)d.key, o);
        d.key = other < d.key ? other : d.key;
    }
    if ((threadIdx.x & 63u) == 0u) { s_cnt[threadIdx.x >> 6] = d.cnt; s_key[threadIdx.x >> 6] = d.key; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint64_t cnt = 0, key = ~(uint64_t)0;
        for (uint32_t k = 0; k < SX_PLACE_THREADS / 64u; k++) { cnt += s_cnt[k]; key = s_key[k] < key ? s_key[k] : key; }
        atomicAdd(ca.diff + 2u * (uint64_t)w.fidx, (unsigned long long)cnt);
        atomicMin(ca.diff + 2u * (uint64_t)w.fidx + 1u, (unsigned long long)key);
    }
}

#endif
