/* lnn_k_digest.h -- the CRC-32 of the decoded PCM of sample windows of resident .lnn streams, per bucket, nothing of the window's size
 * written (LINNEAmd_DigestWindowsDevice; DESIGN.md section 5, "Hashing instead of placing").
 *
 * k_wx_digest is the sibling of k_wx_place (lnn_k_windows.h): its grid, its prologue and record walk, its values (wx_value) -- but a
 * sample that leaves the synthesis is hashed, not stored.  The buckets, the pieces among them, the slots of a long bucket and the
 * commit behind the last pass are those of lnn_k_buckets.h, as for k_wx_measure (lnn_k_measure.h); this file adds the hash.  It is the zlib / IEEE 802.3 CRC-32 of the bytes a WAV writer gives the samples (include/linne_amd.h has the byte string).
 *
 * The algebra, in the reflected representation (bit 31 is x^0; a (x) b is the product modulo P = 0xEDB88320, wxd_mul): with raw(M)
 * the CRC register behind M from the initial value 0 and without the final XOR, a bucket whose string is M = M_0 || ... || M_k,
 * piece i at byte offset o_i with l_i bytes, has
 *     crc32(M) = XOR_i [ raw(M_i) (x) x^(8 (|M| - o_i - l_i)) ]  XOR  (0xFFFFFFFF (x) x^(8 |M|))  XOR  0xFFFFFFFF.
 * A term depends on its piece's bytes and on how many bytes lie between the piece's end and the bucket's end, nothing else, and the
 * terms fold with XOR: atomicXor on a 32-bit accumulator in the context's scratch gives an answer the order of the atomics does not
 * show.  The last two terms need |M| alone; k_wx_digest_commit applies them.
 *
 * A lane takes one sample frame (C channels of w = ceil(bits / 8) bytes, F = C w <= 32 bytes), computes its raw() bit by bit -- the
 * register shifted once per bit, a few integer operations a bit and no table: random byte-table reads would queue on the LDS banks --
 * and multiplies it by x^(8 F d), d < 256 the frames from its own to the end of its bucket's part of the piece, read from a table
 * in the scratch.  A piece of at most 256 frames lies in the buckets [k0, k1]:
 *   - at most WXB_SEGMENTS buckets: for every bucket the lanes of that bucket (the others carry 0) are XORed across the wave with
 *     shuffles and across the four waves through LDS, and lane g multiplies bucket k0 + g's word by x^(8 R), R the bytes from the
 *     part's end to the bucket's end, and issues the one atomicXor of that (piece, bucket);
 *   - more buckets (a small b): the terms go to LDS, and the first lane of every bucket XORs its bucket's terms there.
 * x^(8 R) is the product of at most eight entries of a second table, x^(8 v 256^k), one per non-zero byte of R.  Both tables
 * (WXD_POW_WORDS words in front of the accumulators) are filled by k_wx_digest_preset, which also zeroes the call's accumulators, in
 * front of the first pass: gfx950 has no carry-less multiply, a product is 32 shift-and-XOR steps, and so it stays out of the
 * per-byte path: one per lane, one per (piece, bucket) and non-zero byte of R.
 * Zero-valued records (SILENT, WX_TAIL) contribute nothing when w >= 2 -- raw() of zeros is 0 -- and are skipped; with w == 1 a zero
 * is the byte 0x80 and is hashed like any other.
 *
 * A window's slots lie 64 bytes or more apart (sstride words, no two in one line).  A term is
 * taken to the bucket's end whichever slot it lands in, so k_wx_digest_commit, once per call behind the last pass, XORs a bucket's
 * slots, applies the length terms and writes {crc32, 0, num_bytes} to the caller's d_out -- only for windows whose fail word is
 * clear, so a failing window's d_out is never written.  Plain C++ and vector stores and atomics only.
 */
#ifndef LNN_K_DIGEST_H_INCLUDED
#define LNN_K_DIGEST_H_INCLUDED

#include "lnn_k_buckets.h"

static_assert(SX_PLACE_THREADS == 256u, "a lane's power table has 256 entries");
static_assert(sizeof(struct LINNEAmdDigest) == 16, "a bucket's answer is one struct LINNEAmdDigest");
#define WXD_POLY 0xEDB88320u
#define WXD_ONE 0x80000000u             /* x^0 */
#define WXD_X8 0x00800000u              /* x^8 */
#define WXD_MAXFRAME (LINNE_MAX_NUM_CHANNELS * 4u)
#define WXD_TF_WORDS (WXD_MAXFRAME * 256u)      /* pow[(F - 1) * 256 + d] = x^(8 F d), F <= WXD_MAXFRAME, d < 256 */
#define WXD_TB_WORDS (8u * 256u)                /* pow[WXD_TF_WORDS + k * 256 + v] = x^(8 v 256^k), k < 8, v < 256 */
#define WXD_POW_WORDS (WXD_TF_WORDS + WXD_TB_WORDS)

struct WxDigestArgs {
    WxPlaceArgs p;                      /* the walk's arguments (sat and scale are not used) */
    const WxBucket *dwin;               /* per frame: n, F and sstride are set; slot s, bucket k at abase + s * sstride + k */
    uint32_t *acc;
    const uint32_t *pow;                /* the two tables of powers */
};

/* a (x) b */
__device__ __forceinline__ uint32_t wxd_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0u;
    for (uint32_t i = 0; i < 32u; i++) { p ^= b & (0u - ((a >> (31u - i)) & 1u)); b = (b >> 1) ^ (WXD_POLY & (0u - (b & 1u))); }
    return p;
}
/* x^(8 e), by square and multiply */
__device__ __forceinline__ uint32_t wxd_xpow8(uint64_t e)
{
    uint32_t p = WXD_ONE, s = WXD_X8;
    for (; e; e >>= 1) { if (e & 1u) p = wxd_mul(p, s); s = wxd_mul(s, s); }
    return p;
}
/* x^(8 R) from the table of byte powers tb */
__device__ __forceinline__ uint32_t wxd_pow(const uint32_t *tb, uint64_t R)
{
    uint32_t p = WXD_ONE;
    for (uint32_t k = 0; R; k++, R >>= 8) { const uint32_t v = (uint32_t)R & 255u; if (v) p = wxd_mul(p, tb[k * 256u + v]); }
    return p;
}
/* the register c behind the low nbits bits of u, least significant bit first (whole little-endian bytes) */
__device__ __forceinline__ uint32_t wxd_feed(uint32_t c, uint32_t u, uint32_t nbits)
{
    c ^= u;
    for (uint32_t i = 0; i < nbits; i++) c = (c >> 1) ^ (WXD_POLY & (0u - (c & 1u)));
    return c;
}
/* raw() of block sample i's frame of record rc: every channel's low wd bytes, 8-bit samples unsigned */
__device__ __forceinline__ uint32_t wxd_frame(const WxPlaceArgs &a, const WxBlock *rc, uint32_t type, uint32_t i, uint32_t wd)
{
    uint32_t c = 0u;
    for (uint32_t ch = 0; ch < a.C; ch++) {
        const uint32_t v = (uint32_t)wx_value(a, rc, type, i, ch);
        const uint32_t u = wd == 1u ? ((v + 128u) & 0xFFu) : wd == 4u ? v : (v & ((1u << (8u * wd)) - 1u));
        c = wxd_feed(c, u, 8u * wd);
    }
    return c;
}

/* The workgroup hashes samples [sa, sb) (at most SX_PLACE_THREADS, inside the window) of record rc, whose sample 0 is stream
 * sample f0.  Every barrier in here is passed by the whole workgroup: sa, sb and the buckets are block-uniform. */
__device__ __forceinline__ void wx_digest_piece(const WxDigestArgs &da, const WxWindow &w, const WxBucket &m, const WxBlock *rc, uint32_t type,
        uint64_t f0, uint64_t sa, uint64_t sb, uint32_t wd, uint32_t (*part)[SX_PLACE_THREADS / 64u], uint32_t *terms)
{
    const WxPlaceArgs &a = da.p;
    const WxPiece pc = wx_piece(w, m, sa, sb);
    const uint32_t t = threadIdx.x, len = pc.len, nseg = pc.nseg;
    const uint64_t ra = pc.ra, k0 = pc.k0;
    uint32_t *acc = da.acc + m.abase + (uint64_t)pc.slot * m.sstride;
    const uint32_t *tf = da.pow + (m.F - 1u) * 256u, *tb = da.pow + WXD_TF_WORDS;
    const uint32_t i0 = (uint32_t)(sa - f0);
    if (nseg <= WXB_SEGMENTS) {
        uint32_t end = 0u;                                          /* where the lane's bucket ends in the piece */
        uint32_t ta, te;
        for (uint32_t g = 0; g < nseg; g++) { pc.lanes(k0 + g, ta, te); if (t >= ta && t < te) end = te; }
        const uint32_t term = (t < len) ? wxd_mul(wxd_frame(a, rc, type, i0 + t, wd), tf[end - 1u - t]) : 0u;
        for (uint32_t g = 0; g < nseg; g++) {
            pc.lanes(k0 + g, ta, te);
            uint32_t r = (t >= ta && t < te) ? term : 0u;
            for (int o = 32; o > 0; o >>= 1) r ^= __shfl_xor(r, o);
            if ((t & 63u) == 0u) part[g][t >> 6] = r;
        }
        __syncthreads();
        if (t < nseg) {
            const uint64_t ba = (k0 + t) * m.b, be = ba + m.b < m.n ? ba + m.b : m.n;
            pc.lanes(k0 + t, ta, te);
            uint32_t r = part[t][0];
            for (uint32_t k = 1; k < SX_PLACE_THREADS / 64u; k++) r ^= part[t][k];
            const uint64_t R = (be - (ra + te)) * m.F;
            if (r && R) r = wxd_mul(r, wxd_pow(tb, R));
            if (r) atomicXor(acc + (k0 + t), r);
        }
        __syncthreads();                                            /* (part is written again by the next piece) */
        return;
    }
    /* many short buckets: the piece's terms in LDS, and the first lane of every bucket XORs its bucket's */
    uint64_t k = 0u;
    uint32_t ta = 0u, te = 0u;
    if (t < len) {
        k = (ra + t) / m.b;
        pc.lanes(k, ta, te);
        terms[t] = wxd_mul(wxd_frame(a, rc, type, i0 + t, wd), tf[te - 1u - t]);
    }
    __syncthreads();
    if (t < len && t == ta) {
        uint32_t r = 0u;
        for (uint32_t j = ta; j < te; j++) r ^= terms[j];
        const uint64_t ba = k * m.b, be = ba + m.b < m.n ? ba + m.b : m.n, R = (be - (ra + te)) * m.F;
        if (r && R) r = wxd_mul(r, wxd_pow(tb, R));
        if (r) atomicXor(acc + k, r);
    }
    __syncthreads();                                                /* (terms is filled again by the next piece) */
}

/* nrec * xch workgroups: the y-th xch of them hash record y, piece by piece as k_wx_place places it */
__global__ __launch_bounds__(SX_PLACE_THREADS) void k_wx_digest(WxDigestArgs da)
{
    __shared__ uint32_t part[WXB_SEGMENTS][SX_PLACE_THREADS / 64u];
    __shared__ uint32_t terms[SX_PLACE_THREADS];
    WxRecord r;
    if (!wx_prologue(da.p, r)) return;                             /* block-uniform, as every exit */
    const uint32_t wd = (da.p.bits + 7u) >> 3;
    if (wd > 1u && r.type != SX_COMPRESS && r.type != SX_RAW) return;      /* zeros of two bytes or more: raw() is 0 */
    const WxBucket m = da.dwin[r.rc->win];
    wx_walk(da.p, r.rc, r.w, r.type, r.x, [&](uint64_t f0, uint64_t sa, uint64_t sb) { wx_digest_piece(da, r.w, m, r.rc, r.type, f0, sa, sb, wd, part, terms); });
}

/* the two tables of powers filled and every accumulator of the call zeroed: a lane per word */
__global__ __launch_bounds__(WXB_THREADS) void k_wx_digest_preset(uint32_t *pow, uint32_t *acc, uint64_t total)
{
    for (uint64_t g = (uint64_t)blockIdx.x * WXB_THREADS + threadIdx.x; g < total + WXD_POW_WORDS; g += (uint64_t)gridDim.x * WXB_THREADS) {
        if (g >= WXD_POW_WORDS) acc[g - WXD_POW_WORDS] = 0u;
        else if (g < WXD_TF_WORDS) pow[g] = wxd_xpow8((uint64_t)((uint32_t)g / 256u + 1u) * ((uint32_t)g & 255u));
        else { const uint32_t j = (uint32_t)g - WXD_TF_WORDS; pow[g] = wxd_xpow8((uint64_t)(j & 255u) << (8u * (j / 256u))); }
    }
}

/* A lane per bucket of every digested window, numbered through the windows in their records' order (obase): the bucket's slots
 * XORed, the length terms applied and the answer stored in the caller's table, unless the window's fail word is set */
__global__ __launch_bounds__(WXB_THREADS) void k_wx_digest_commit(const WxBucket *dwin, uint32_t nwin, const uint32_t *acc, const uint32_t *pow, const uint32_t *fail, uint64_t total)
{
    for (uint64_t g = (uint64_t)blockIdx.x * WXB_THREADS + threadIdx.x; g < total; g += (uint64_t)gridDim.x * WXB_THREADS) {
        const WxBucket m = dwin[wx_bucket_window(dwin, nwin, g)];
        if (fail[m.fidx] != WX_NOFAIL) continue;
        const uint64_t k = g - m.obase, ba = k * m.b, bytes = ((ba + m.b < m.n ? ba + m.b : m.n) - ba) * m.F;
        const uint32_t *p = acc + m.abase + k;
        uint32_t r = 0u;
        for (uint32_t s = 0; s < m.ns; s++, p += m.sstride) r ^= *p;
        struct LINNEAmdDigest o;
        o.crc32 = r ^ wxd_mul(0xFFFFFFFFu, wxd_pow(pow + WXD_TF_WORDS, bytes)) ^ 0xFFFFFFFFu; o.reserved = 0u; o.num_bytes = bytes;
        ((struct LINNEAmdDigest *)m.out)[k] = o;
    }
}

#endif
