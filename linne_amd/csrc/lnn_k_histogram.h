/* lnn_k_histogram.h -- histogramming the sample levels of windows of resident .lnn streams: a count per channel, bucket and bin of
 * |v| >> shift (or of its bit length), nothing of the window's size written (LINNEAmd_HistogramWindowsDevice; DESIGN.md section 5,
 * "Counting instead of placing").
 *
 * k_wx_histogram is the sibling of k_wx_measure (lnn_k_measure.h): its grid, its prologue and record walk, its values (wx_value), its
 * buckets, pieces and slots (lnn_k_buckets.h) -- but a sample that leaves the synthesis is counted, not reduced.  Bin j of channel ch,
 * bucket k owns one 32-bit counter in the context's scratch -- slot s of a window at abase + ((s * C + ch) * nb + k) * num_bins + j --
 * zeroed by k_wx_histogram_preset.  32 bits are enough: a stream's header holds a 32-bit sample count, so a window has at most
 * 2^32 - 1 samples and no counter, nor the sum of a bin's slots, can pass that.  A piece:
 *   - a SILENT or WX_TAIL record holds zeros: one lane per (bucket of the piece, channel) adds the overlap's length to bin 0, no more;
 *   - few buckets: bucket after bucket, the lanes of the bucket count into a histogram in LDS (C * num_bins counters, all zero
 *     between the pieces), a wave first adding up the lanes that share a bin (below).  The lane whose LDS addition found the counter
 *     at zero owns that bin for this bucket of the piece: behind the barrier it reads the counter, zeroes it again and adds it to
 *     the accumulator.  So a bin costs one global atomic per piece however many of the piece's samples fell into it, the bins that
 *     stayed empty cost nothing, and no pass over the C * num_bins counters is made, neither to zero nor to flush them;
 *   - many (more than WXB_SEGMENTS, a short bucket): a lane adds 1 to its sample's counter in the scratch, channel by channel.
 * A workgroup takes one piece of a block record (the grid has a workgroup per 256 samples of a block), so there is no run of pieces
 * to keep the LDS histogram over: it is flushed per piece, and the pieces of a long bucket meet in the accumulators, spread over the
 * window's slots as the measure kernel's are.
 * A wave whose lanes hit one LDS counter would queue there: digital near-silence, DC, a clipped plateau, log2 bins.  wxh_count therefore
 * asks first how many lanes share the first lane's bin; where that is WXH_SHARE or more, one lane adds their number and they retire,
 * and the question is put again to the lanes that are left, WXH_ROUNDS times at the most.  The lanes still active then add 1 each.
 * On spread-out material the first ballot fails and costs two wave operations.
 * All of it is integer additions, so the order of the atomics does not show.  Plain C++ and vector stores only.
 */
#ifndef LNN_K_HISTOGRAM_H_INCLUDED
#define LNN_K_HISTOGRAM_H_INCLUDED

#include "lnn_k_buckets.h"

#ifndef WXH_SHARE                       /* (tools/stream_histogram.py times a build with 65, which never adds up in the wave) */
#define WXH_SHARE 8                     /* lanes of a wave on one bin from which they are added up in the wave */
#endif
#define WXH_ROUNDS 4u                   /* bins a wave peels off that way */
static_assert(LINNE_AMD_HIST_MAX_BINS * LINNE_MAX_NUM_CHANNELS * sizeof(uint32_t) <= 32768u && LINNE_AMD_HIST_MAX_BINS <= 0xFFFFu,
        "the LDS histogram is at most 32 KiB, and WXH_SPEC keeps num_bins in 16 bits");

struct WxHistogramArgs {
    WxPlaceArgs p;                      /* the walk's arguments (sat and scale are not used) */
    const WxBucket *hwin;               /* per bin: cstride, C and hist are set */
    uint32_t *acc;
};

/* the bin of sample v: m = |v| >> shift with |v| taken beyond 32 bits (INT32_MIN has 2^31), x = m or m's bit length, min(x, last) */
__device__ __forceinline__ uint32_t wxh_bin(int32_t v, uint32_t shift, uint32_t log2, uint32_t last)
{
    const uint32_t mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    const uint32_t m = mag >> shift;
    const uint32_t x = log2 ? (m ? 32u - (uint32_t)__builtin_clz(m) : 0u) : m;
    return x < last ? x : last;
}

/* Every lane with `mine` counts once into h[bin]; true for the lane that found the counter at zero.  Called by whole waves */
__device__ __forceinline__ bool wxh_count(uint32_t *h, uint32_t bin, bool mine)
{
    bool own = false;
    for (uint32_t r = 0; r < WXH_ROUNDS; r++) {
        const unsigned long long act = __ballot(mine);
        if (act == 0ull) return own;                                /* wave-uniform */
        const int lead = __ffsll(act) - 1;
        const unsigned long long same = __ballot(mine && bin == (uint32_t)__shfl((int)bin, lead));
        if (__popcll(same) < WXH_SHARE) break;                      /* wave-uniform */
        if (mine && (int)(threadIdx.x & 63u) == lead) own = atomicAdd(h + bin, (uint32_t)__popcll(same)) == 0u;
        if ((same >> (threadIdx.x & 63u)) & 1ull) mine = false;
    }
    if (mine) own = atomicAdd(h + bin, 1u) == 0u;
    return own;
}

/* The workgroup counts samples [sa, sb) (at most SX_PLACE_THREADS, inside the window) of record rc, whose sample 0 is stream sample
 * f0.  Every barrier in here is passed by the whole workgroup: sa, sb and the buckets are block-uniform.  hist: C * num_bins counters,
 * zero on entry and on return */
__device__ __forceinline__ void wx_histogram_piece(const WxHistogramArgs &ha, const WxWindow &w, const WxBucket &m, const WxBlock *rc, uint32_t type,
        uint64_t f0, uint64_t sa, uint64_t sb, uint32_t *hist)
{
    const WxPlaceArgs &a = ha.p;
    const WxPiece pc = wx_piece(w, m, sa, sb);
    const uint32_t t = threadIdx.x, C = a.C, len = pc.len, nseg = pc.nseg;
    const uint32_t bins = WXH_BINS(m.hist), shift = WXH_SHIFT(m.hist), log2 = WXH_LOG2(m.hist), last = bins - 1u;
    const uint64_t k0 = pc.k0;
    uint32_t *acc = ha.acc + m.abase + (uint64_t)pc.slot * C * m.nb * bins;
    if (type != SX_COMPRESS && type != SX_RAW) {
        /* zeros */
        for (uint32_t j = t; j < nseg * C; j += SX_PLACE_THREADS) {
            const uint32_t ch = j / nseg, g = j - ch * nseg;
            uint32_t ta, te;
            pc.lanes(k0 + g, ta, te);
            atomicAdd(acc + ((uint64_t)ch * m.nb + (k0 + g)) * bins, te - ta);
        }
        return;
    }
    const uint32_t i0 = (uint32_t)(sa - f0);
    if (nseg > WXB_SEGMENTS) {
        /* many short buckets: nothing shares a counter for long */
        if (t < len) {
            const uint64_t k = (pc.ra + t) / m.b;
            for (uint32_t ch = 0; ch < C; ch++)
                atomicAdd(acc + ((uint64_t)ch * m.nb + k) * bins + wxh_bin(wx_value(a, rc, type, i0 + t, ch), shift, log2, last), 1u);
        }
        return;
    }
    uint32_t bin[LINNE_MAX_NUM_CHANNELS];
#pragma unroll
    for (uint32_t ch = 0; ch < LINNE_MAX_NUM_CHANNELS; ch++)
        bin[ch] = (ch < C && t < len) ? wxh_bin(wx_value(a, rc, type, i0 + t, ch), shift, log2, last) : 0u;
    for (uint32_t g = 0; g < nseg; g++) {
        uint32_t ta, te;
        pc.lanes(k0 + g, ta, te);
        const bool mine = (t >= ta && t < te);
        uint32_t own = 0u;
#pragma unroll
        for (uint32_t ch = 0; ch < LINNE_MAX_NUM_CHANNELS; ch++)
            if (ch < C && wxh_count(hist + ch * bins, bin[ch], mine)) own |= 1u << ch;
        __syncthreads();
#pragma unroll
        for (uint32_t ch = 0; ch < LINNE_MAX_NUM_CHANNELS; ch++)
            if ((own >> ch) & 1u) {
                uint32_t *h = hist + ch * bins + bin[ch];
                const uint32_t n = *h;
                *h = 0u;
                atomicAdd(acc + ((uint64_t)ch * m.nb + (k0 + g)) * bins + bin[ch], n);
            }
        __syncthreads();                                            /* (the counters are used again by the next bucket and the next piece) */
    }
}

/* nrec * xch workgroups: the y-th xch of them count record y, piece by piece as k_wx_place places it */
__global__ __launch_bounds__(SX_PLACE_THREADS) void k_wx_histogram(WxHistogramArgs ha)
{
    __shared__ uint32_t hist[LINNE_MAX_NUM_CHANNELS * LINNE_AMD_HIST_MAX_BINS];
    WxRecord r;
    if (!wx_prologue(ha.p, r)) return;
    const WxBucket m = ha.hwin[r.rc->win];
    if (r.type == SX_COMPRESS || r.type == SX_RAW) {                /* block-uniform */
        for (uint32_t j = threadIdx.x; j < ha.p.C * WXH_BINS(m.hist); j += SX_PLACE_THREADS) hist[j] = 0u;
        __syncthreads();
    }
    wx_walk(ha.p, r.rc, r.w, r.type, r.x, [&](uint64_t f0, uint64_t sa, uint64_t sb) { wx_histogram_piece(ha, r.w, m, r.rc, r.type, f0, sa, sb, hist); });
}

/* every counter of the call to zero */
__global__ __launch_bounds__(WXB_THREADS) void k_wx_histogram_preset(uint32_t *acc, uint64_t total)
{
    for (uint64_t g = (uint64_t)blockIdx.x * WXB_THREADS + threadIdx.x; g < total; g += (uint64_t)gridDim.x * WXB_THREADS) acc[g] = 0u;
}

/* A lane per (channel, bucket, bin) of every histogrammed window, numbered through the windows in their records' order (obase): the
 * bin's slots added up and the count stored in the caller's table, unless the window's fail word is set */
__global__ __launch_bounds__(WXB_THREADS) void k_wx_histogram_commit(const WxBucket *hwin, uint32_t nwin, const uint32_t *acc, const uint32_t *fail, uint64_t total)
{
    for (uint64_t g = (uint64_t)blockIdx.x * WXB_THREADS + threadIdx.x; g < total; g += (uint64_t)gridDim.x * WXB_THREADS) {
        const WxBucket m = hwin[wx_bucket_window(hwin, nwin, g)];
        if (fail[m.fidx] != WX_NOFAIL) continue;
        const uint64_t bins = WXH_BINS(m.hist), e = g - m.obase, rec = e / bins, j = e - rec * bins, ch = rec / m.nb, k = rec - ch * m.nb;
        const uint32_t *p = acc + m.abase + e;
        uint64_t n = 0;
        for (uint32_t s = 0; s < m.ns; s++, p += (uint64_t)m.C * m.nb * bins) n += *p;
        ((uint64_t *)m.out)[(ch * m.cstride + k) * bins + j] = n;
    }
}

#endif
