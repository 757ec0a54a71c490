/* lnn_k_quiet.h -- finding the quiet runs of sample windows of resident .lnn streams: a list of (first sample, length) per window,
 * no PCM written (LINNEAmd_QuietWindowsDevice; DESIGN.md section 5, "A bitmask instead of buckets").  A sample frame is quiet when
 * |v| <= threshold in every channel, |v| taken in 64 bits; a run is a maximal stretch of quiet frames inside the window.
 *
 * k_wx_quiet is the sibling of k_wx_place (lnn_k_windows.h): its grid, its prologue and record walk, its values (wx_value) -- but a
 * frame that leaves the synthesis becomes one bit.  Every window owns ceil(n / 64) 64-bit words in the context's scratch, zeroed by
 * k_wx_quiet_preset; bit r of them is the window's frame r.  Lane t of a piece holds the piece's frame t, a wave's ballot is 64
 * consecutive bits of the mask, and they lie at bit (sa - lo) + 64 * wave, which is unaligned in general: lane 0 of the wave issues
 * one atomicOr on the word the ballot begins in and one on the next where it reaches into it, none for a ballot of zeros.  Pieces
 * cover disjoint bits, so the mask does not depend on the order of the pieces or on the passes a window is spread over.  A piece has
 * no barrier and no LDS, and the kernel stores nothing to the caller's memory.  The window's loud extent -- its lowest loud frame
 * (preset ~0) and its highest loud frame + 1 (preset 0), from which the host takes lead_samples and trail_samples -- is NOT kept here:
 * the workgroups of a grid run roughly in ascending order, so the highest loud frame moves with nearly every wave, and an atomicMax
 * per wave on one address made the kernel of a 60-minute stream 22 ms long where k_wx_place takes 0.9.  The extent is a property of
 * the mask's zero bits and is taken from them in the commit stage, one atomicMin and one atomicMax per chunk of 16384 frames.
 *
 * The commit stage runs behind the last pass, for the windows whose fail word is clear.  A workgroup takes a chunk of
 * WXQ_CHUNK_WORDS mask words of one window, a lane one word of it (with the last bit of the word before and the first of the word
 * behind).  A qualified start is a 1 bit behind a 0 (or the window's edge) that has min_run - 1 ones behind it; a qualified end is the
 * last 1 bit in front of a 0 (or the window's edge) that has min_run - 1 ones in front of it.  Either test walks at most min_run bits
 * of the run, a word at a time, so all tests together read no more than the masks twice, and the k-th qualified start and the k-th
 * qualified end of a window belong to the same run.
 *   k_wx_quiet_runs<WXQ_COUNT>   per chunk: its qualified starts and its qualified ends, into two halves of one array of counts;
 *                                per window (atomics, one per chunk that has any): the runs, and the sum of the ends minus the sum
 *                                of the starts, which in wrapping 64-bit arithmetic is the sum of the runs' lengths; the lowest and
 *                                the highest zero bit of the chunk into the window's loud extent (whatever min_run is)
 *   (k_sx_scan of lnn_k_stream.h) the prefix sums of both halves in one launch
 *   k_wx_quiet_runs<WXQ_STARTS>  the start of run k into record k of the caller's table, where k < capacity
 *   k_wx_quiet_runs<WXQ_ENDS>    the end of run k, minus the start the launch before stored, into record k's length
 * No list of runs is kept in between, and a chunk whose first run lies at or behind the capacity returns before it reads its words: a
 * call that only counts (capacity 0) pays the two writing launches and nothing in them.  Plain C++ and vector stores only.
 */
#ifndef LNN_K_QUIET_H_INCLUDED
#define LNN_K_QUIET_H_INCLUDED

#include "lnn_k_buckets.h"             /* wx_bucket_window */

static_assert(sizeof(struct LINNEAmdRun) == 16, "a record of the caller's table is two 64-bit words");
static_assert(SX_PLACE_THREADS == 256u && WXQ_CHUNK_WORDS == WXB_THREADS, "a piece is four ballots of 64 lanes; a commit lane takes one word of its chunk");

#define WXQ_BACK_WORDS 8u               /* per window behind the fail and saturation words: four 64-bit words */
enum { WXQ_LOUD_LO = 0, WXQ_LOUD_HI = 1, WXQ_RUNS = 2, WXQ_QUIET = 3 };
enum { WXQ_COUNT = 0, WXQ_STARTS = 1, WXQ_ENDS = 2 };

struct WxQuietArgs {
    WxPlaceArgs p;                      /* the walk's arguments (sat and scale are not used) */
    const WxBucket *qwin;               /* bitmask: threshold and abase are read here */
    unsigned long long *mask;           /* the call's mask words */
};

/* The workgroup marks frames [sa, sb) (at most SX_PLACE_THREADS, inside the window) of record rc, whose sample 0 is stream sample f0.
 * No barrier: every step is a wave's own */
__device__ __forceinline__ void wx_quiet_piece(const WxQuietArgs &qa, const WxWindow &w, const WxBucket &m, const WxBlock *rc, uint32_t type,
        uint64_t f0, uint64_t sa, uint64_t sb)
{
    const WxPlaceArgs &a = qa.p;
    const uint32_t t = threadIdx.x, len = (uint32_t)(sb - sa), i0 = (uint32_t)(sa - f0), wb = t & ~63u;
    bool quiet = false;
    if (t < len) {
        quiet = true;
        for (uint32_t ch = 0; ch < a.C; ch++) {
            const int64_t v = wx_value(a, rc, type, i0 + t, ch);
            quiet = quiet && (uint64_t)(v < 0 ? -v : v) <= (uint64_t)m.threshold;
        }
    }
    const uint64_t q = __ballot(quiet);
    if (t != wb || !q) return;                                      /* lane 0 of a wave that holds quiet frames goes on */
    /* the ballot's set bits are frames of the piece, which lie inside the window: a word that receives one is one of the window's */
    const uint64_t p = (sa - w.lo) + wb;                            /* the window's frame in the ballot's bit 0 */
    unsigned long long *word = qa.mask + m.abase + (p >> 6);
    const uint32_t sh = (uint32_t)(p & 63u);
    atomicOr(word, (unsigned long long)(q << sh));
    if (sh && (q >> (64u - sh))) atomicOr(word + 1, (unsigned long long)(q >> (64u - sh)));
}

/* nrec * xch workgroups: the y-th xch of them mark record y, piece by piece as k_wx_place places it */
__global__ __launch_bounds__(SX_PLACE_THREADS) void k_wx_quiet(WxQuietArgs qa)
{
    WxRecord r;
    if (!wx_prologue(qa.p, r)) return;
    const WxBucket m = qa.qwin[r.rc->win];
    wx_walk(qa.p, r.rc, r.w, r.type, r.x, [&](uint64_t f0, uint64_t sa, uint64_t sb) { wx_quiet_piece(qa, r.w, m, r.rc, r.type, f0, sa, sb); });
}

/* every mask word of the call to zero */
__global__ __launch_bounds__(WXB_THREADS) void k_wx_quiet_preset(unsigned long long *mask, uint64_t nwords)
{
    for (uint64_t g = (uint64_t)blockIdx.x * WXB_THREADS + threadIdx.x; g < nwords; g += (uint64_t)gridDim.x * WXB_THREADS) mask[g] = 0ull;
}

/* ---- the commit stage ---- */
/* the ones in a row from bit P (a 1) upward: exact when below `want`, otherwise some number >= want.  At most want / 64 + 2 words of
 * the window's nwords are read */
__device__ __forceinline__ uint64_t wxq_ones_up(const unsigned long long *mask, uint64_t nwords, uint64_t P, uint64_t want)
{
    uint64_t j = P >> 6;
    const uint32_t sh = (uint32_t)(P & 63u);
    const uint64_t inv = ~(mask[j] >> sh);                          /* (the sh bits shifted in read as the run's end) */
    uint64_t got = inv ? (uint64_t)__builtin_ctzll(inv) : 64u;
    if (got < 64u - sh) return got;
    got = 64u - sh;
    while (got < want && ++j < nwords) {
        const uint64_t x = ~mask[j];
        if (x) return got + (uint64_t)__builtin_ctzll(x);
        got += 64u;
    }
    return got;
}
/* the ones in a row from bit P (a 1) downward, likewise */
__device__ __forceinline__ uint64_t wxq_ones_down(const unsigned long long *mask, uint64_t P, uint64_t want)
{
    uint64_t j = P >> 6;
    const uint32_t sh = (uint32_t)(P & 63u);
    const uint64_t inv = ~(mask[j] << (63u - sh));
    uint64_t got = inv ? (uint64_t)__builtin_clzll(inv) : 64u;
    if (got < sh + 1u) return got;
    got = sh + 1u;
    while (got < want && j-- > 0u) {
        const uint64_t x = ~mask[j];
        if (x) return got + (uint64_t)__builtin_clzll(x);
        got += 64u;
    }
    return got;
}
/* word j of a window's mask: the bits where a run of at least min_run frames starts (ends false) or has its last frame (ends true) */
__device__ __forceinline__ uint64_t wxq_events(const unsigned long long *mask, uint64_t nwords, uint64_t j, uint64_t min_run, bool ends)
{
    const uint64_t w = mask[j];
    if (!w) return 0u;
    uint64_t e;
    if (!ends) e = w & ~((w << 1) | (j ? mask[j - 1u] >> 63 : 0ull));
    else e = w & ~((w >> 1) | (j + 1u < nwords ? mask[j + 1u] << 63 : 0ull));
    if (min_run <= 1u) return e;
    uint64_t keep = 0u;
    for (uint64_t rest = e; rest; rest &= rest - 1u) {
        const uint32_t b = (uint32_t)__builtin_ctzll(rest);
        const uint64_t P = (j << 6) + b;
        if ((ends ? wxq_ones_down(mask, P, min_run) : wxq_ones_up(mask, nwords, P, min_run)) >= min_run) keep |= 1ull << b;
    }
    return keep;
}

struct WxQuietCommitArgs {
    const WxBucket *qwin; const WxWindow *wins; uint32_t nwin;
    const unsigned long long *mask;
    const uint32_t *fail;
    uint64_t nchunks;                   /* of all windows: chunk c belongs to the last window whose obase <= c */
    uint32_t *counts;                   /* [2][nchunks]: qualified starts, qualified ends */
    const uint64_t *ofs;                /* [2 * nchunks + 1]: the exclusive prefix sums of counts */
    unsigned long long *back;           /* [W][4] beside the fail words: WXQ_LOUD_LO .. WXQ_QUIET */
};

/* A workgroup per chunk (grid-stride over the chunks; every exit and barrier is block-uniform), a lane per mask word */
template <int MODE> __global__ __launch_bounds__(WXB_THREADS) void k_wx_quiet_runs(WxQuietCommitArgs a)
{
    __shared__ uint32_t s_cnt[2][WXB_THREADS / 64u];
    __shared__ uint64_t s_sum[WXB_THREADS / 64u], s_lo[WXB_THREADS / 64u], s_hi[WXB_THREADS / 64u];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    for (uint64_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
        const uint32_t wi = wx_bucket_window(a.qwin, a.nwin, c);
        const WxBucket m = a.qwin[wi];
        const bool failed = a.fail[m.fidx] != WX_NOFAIL;
        if (MODE == WXQ_COUNT && failed) {
            if (t == 0u) { a.counts[c] = 0u; a.counts[a.nchunks + c] = 0u; }
            continue;
        }
        if (failed) continue;
        const uint64_t half = (MODE == WXQ_ENDS) ? a.nchunks : 0u;
        const uint64_t k0 = (MODE == WXQ_COUNT) ? 0u : a.ofs[half + c] - a.ofs[half + m.obase];   /* the runs of the window's chunks before this one */
        if (MODE != WXQ_COUNT && k0 >= m.capacity) continue;
        const unsigned long long *mask = a.mask + m.abase;
        const uint64_t nwords = (m.n >> 6) + ((m.n & 63u) != 0u), j = (c - m.obase) * WXQ_CHUNK_WORDS + t;
        if (MODE == WXQ_COUNT) {
            uint64_t qs = 0u, qe = 0u, sum = 0u, lo = ~0ull, hi = 0u;
            if (j < nwords) {
                qs = wxq_events(mask, nwords, j, m.min_run, false); qe = wxq_events(mask, nwords, j, m.min_run, true);
                /* the word's loud frames: its zero bits below the window's end */
                const uint64_t loud = ~mask[j] & ((j + 1u == nwords && (m.n & 63u)) ? (1ull << (m.n & 63u)) - 1u : ~0ull);
                if (loud) { lo = (j << 6) + (uint32_t)__builtin_ctzll(loud); hi = (j << 6) + 64u - (uint32_t)__builtin_clzll(loud); }
            }
            uint32_t cs = (uint32_t)__popcll(qs), ce = (uint32_t)__popcll(qe);
            for (uint64_t rest = qe; rest; rest &= rest - 1u) sum += (j << 6) + (uint32_t)__builtin_ctzll(rest) + 1u;
            for (uint64_t rest = qs; rest; rest &= rest - 1u) sum -= (j << 6) + (uint32_t)__builtin_ctzll(rest);
            for (int o = 32; o > 0; o >>= 1) {
                cs += (uint32_t)__shfl_xor((int)cs, o); ce += (uint32_t)__shfl_xor((int)ce, o);
                sum += (uint64_t)__shfl_xor((unsigned long long)sum, o);
                const uint64_t olo = (uint64_t)__shfl_xor((unsigned long long)lo, o), ohi = (uint64_t)__shfl_xor((unsigned long long)hi, o);
                lo = olo < lo ? olo : lo; hi = ohi > hi ? ohi : hi;
            }
            if (lane == 0u) { s_cnt[0][wv] = cs; s_cnt[1][wv] = ce; s_sum[wv] = sum; s_lo[wv] = lo; s_hi[wv] = hi; }
            __syncthreads();
            if (t == 0u) {
                uint32_t ts = 0u, te = 0u; uint64_t tq = 0u, tlo = ~0ull, thi = 0u;
                for (uint32_t k = 0; k < WXB_THREADS / 64u; k++) {
                    ts += s_cnt[0][k]; te += s_cnt[1][k]; tq += s_sum[k];
                    tlo = s_lo[k] < tlo ? s_lo[k] : tlo; thi = s_hi[k] > thi ? s_hi[k] : thi;
                }
                a.counts[c] = ts; a.counts[a.nchunks + c] = te;
                unsigned long long *ans = a.back + 4u * (uint64_t)m.fidx;
                if (ts) atomicAdd(&ans[WXQ_RUNS], (unsigned long long)ts);
                if (tq) atomicAdd(&ans[WXQ_QUIET], (unsigned long long)tq);
                if (thi) { atomicMin(&ans[WXQ_LOUD_LO], (unsigned long long)tlo); atomicMax(&ans[WXQ_LOUD_HI], (unsigned long long)thi); }
            }
            __syncthreads();                                        /* (the partial sums are written again by the next chunk) */
        } else {
            const uint64_t q = (j < nwords) ? wxq_events(mask, nwords, j, m.min_run, MODE == WXQ_ENDS) : 0u;
            const uint32_t v = (uint32_t)__popcll(q);
            uint32_t x = v;                                         /* inclusive scan within the wave */
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
                if (lane >= d) x += y;
            }
            if (lane == 63u) s_cnt[0][wv] = x;
            __syncthreads();
            uint64_t k = k0 + x - v;
            for (uint32_t i = 0; i < wv; i++) k += s_cnt[0][i];
            struct LINNEAmdRun *out = (struct LINNEAmdRun *)m.out;
            const uint64_t lo = a.wins[wi].lo;
            for (uint64_t rest = q; rest && k < m.capacity; rest &= rest - 1u, k++) {
                const uint64_t P = (j << 6) + (uint32_t)__builtin_ctzll(rest);
                if (MODE == WXQ_STARTS) out[k].first_sample = lo + P;
                else out[k].num_samples = lo + P + 1u - out[k].first_sample;
            }
            __syncthreads();                                        /* (the waves' totals are written again by the next chunk) */
        }
    }
}

#endif
