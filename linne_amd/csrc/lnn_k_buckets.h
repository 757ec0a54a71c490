/* lnn_k_buckets.h -- what the windows calls that reduce a window per bucket share (k_wx_measure of lnn_k_measure.h, k_wx_digest of
 * lnn_k_digest.h; DESIGN.md section 5, "Consumers that keep buckets").  A window of n samples with bucket length b has
 * nb = ceil(n / b) buckets; its WxBucket record (lnn_windows_plan.h, filled by the host's plan) says where its accumulators lie in
 * the context's scratch and where its answers go.
 *
 * A piece of the record walk (wx_walk: at most 256 samples, lane t the piece's sample t) lies in the buckets [k0, k0 + nseg).  With
 * at most WXB_SEGMENTS of them the whole workgroup reduces bucket after bucket, the lanes outside a bucket carrying the reduction's
 * identity; with more (a small b) the lanes' values go to LDS and the first lane of every bucket walks its bucket's there.  Either
 * way one lane per (piece, bucket) issues the atomics, and no reduction crosses a bucket's boundary.
 *
 * Where a bucket is long, thousands of workgroups would queue on one address.  Such a window gets ns > 1 slots (wx_slots), copies of
 * its accumulators, and the piece at samples [256 j, 256 j + 256) of the window adds into slot j % ns.  A commit kernel, once per call
 * behind the last pass, folds a bucket's slots and writes the answer to the caller's table -- only for windows whose fail word is
 * clear.  Its lanes are numbered through the output records of all windows; wx_bucket_window finds a lane's window.
 */
#ifndef LNN_K_BUCKETS_H_INCLUDED
#define LNN_K_BUCKETS_H_INCLUDED

static_assert(SX_PLACE_THREADS == 256u, "a piece is reduced over four waves of 64, and a slot takes pieces of 256 samples");

/* samples [sa, sb) of window w among its buckets */
struct WxPiece {
    uint64_t ra, b, k0;                 /* the piece's first sample in the window; the bucket length; its first bucket */
    uint32_t len, nseg, slot;           /* samples; buckets, <= 256; the slot it adds into */
    /* the lanes [ta, te) of bucket k */
    __device__ __forceinline__ void lanes(uint64_t k, uint32_t &ta, uint32_t &te) const
    {
        const uint64_t ba = k * b, e = ba + b - ra;
        ta = ba > ra ? (uint32_t)(ba - ra) : 0u; te = e > len ? len : (uint32_t)e;
    }
};
__device__ __forceinline__ WxPiece wx_piece(const WxWindow &w, const WxBucket &m, uint64_t sa, uint64_t sb)
{
    WxPiece p;
    p.ra = sa - w.lo; p.b = m.b; p.len = (uint32_t)(sb - sa);
    p.k0 = p.ra / m.b;
    p.nseg = (uint32_t)((p.ra + p.len - 1u) / m.b - p.k0) + 1u;
    p.slot = (uint32_t)(p.ra / SX_PLACE_THREADS) & (m.ns - 1u);
    return p;
}

/* the window of output record g: the last one whose obase <= g */
__device__ __forceinline__ uint32_t wx_bucket_window(const WxBucket *bwin, uint32_t nwin, uint64_t g)
{
    uint32_t lo = 0, hi = nwin;
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (bwin[mid].obase <= g) lo = mid; else hi = mid; }
    return lo;
}

#endif
