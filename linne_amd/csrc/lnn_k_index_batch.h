/* lnn_k_index_batch.h -- the block indexes of the resident .lnn streams of one call, all streams at once (LINNEAmd_StreamIndexesCreate,
 * and LINNEAmd_StreamIndexCreate as its one-stream case).
 *
 *   k_ib_headers              every stream's header bytes, gathered for the host
 *   k_ib_count / k_ib_write   every position from the first block on that passes sx_candidate is a candidate; a wave scans 4096
 *                             positions of one stream, counts, and after a scan of the counts (k_sx_scan, k_ib_seg) writes its
 *                             candidates in stream order
 *   k_ib_succ                 a candidate's successor: the candidate of its stream at position + size + 6 (binary search), or none
 *   k_sx_jump                 pointer doubling: level k + 1 = level k applied twice
 *   k_ib_chain_len, k_ib_chain  a stream's chain from its head (position 30) enumerated by its ranks: rank r is the head's
 *                             successor taken r times, read off the levels by the bits of r.  A false candidate (FF FF inside a
 *                             payload) is never the successor of a node the head reaches, so the chain never holds one
 *   k_sx_scan, k_ib_first     the blocks' first samples
 *   k_ib_check                a wave per block: CRC16 over lanes (partial CRCs shifted by the bytes behind them and XORed), then the
 *                             checks lnn_parse_block_head makes after the CRC, in its order
 *   k_ib_behind               what stands behind a chain that ends before the header's sample count
 *
 * Three prefix tables of T + 1 entries place a thread in its stream (ib_owner, a binary search):
 *   row0   the 4096-position waves of the streams before it (host: from the streams' lengths)
 *   seg    the candidates of the streams before it (device: the scan of the rows' counts, read at row0): candidates are numbered
 *          over the whole call, stream i's are [seg[i], seg[i + 1]), their positions are bytes of their own stream
 *   crow   the chain blocks of the streams before it (host: from the chain lengths)
 * A successor is searched inside the candidate's own segment and "none" is the one global sentinel M, so the levels of the pointer
 * doubling are plain arrays over [0, M] (k_sx_jump as it is) and no chain ever leaves its stream.  A stream has a chain only when its
 * first candidate lies at byte 30.
 * Every read of stream i is a byte load inside [0, N_i).  A stream that dropped out of the call has b = NULL and N = 0: no rows, no
 * candidates, no chain.
 */
#ifndef LNN_K_INDEX_BATCH_H_INCLUDED
#define LNN_K_INDEX_BATCH_H_INCLUDED

#define IB_HDR_SLOT 32u                 /* a stream's slot in the gathered headers (SX_FIRST_BLOCK bytes used) */

struct IbStream {
    const uint8_t *b; uint64_t N;
    uint64_t num_samples; uint32_t C, S, bits, pad;                /* of its header (zero until the host has read it) */
};

/* the i < T with tab[i] + i * step <= v < tab[i + 1] + (i + 1) * step; tab is non-decreasing, tab[0] = 0 and v lies below the last
 * entry (a stream with nothing in the table owns no v) */
__device__ __forceinline__ uint32_t ib_owner(const uint64_t *tab, uint32_t T, uint64_t v, uint64_t step)
{
    uint32_t lo = 0, hi = T;
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (tab[mid] + mid * step <= v) lo = mid; else hi = mid; }
    return lo;
}

/* every stream's first min(30, N) bytes, zeros behind them */
__global__ __launch_bounds__(256) void k_ib_headers(const IbStream *st, uint32_t T, uint8_t *out)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)T * IB_HDR_SLOT) return;
    const uint32_t i = (uint32_t)(t / IB_HDR_SLOT), j = (uint32_t)(t % IB_HDR_SLOT);
    const uint8_t *b = st[i].b;
    out[t] = (b && j < SX_FIRST_BLOCK && j < st[i].N) ? b[j] : (uint8_t)0;
}

/* the candidates of (stream, wave) rows: counted, then written in stream order from the scan of the counts on */
__global__ __launch_bounds__(256) void k_ib_count(const IbStream *st, const uint64_t *row0, uint32_t T, uint64_t nrows, uint32_t *counts)
{
    const uint64_t w = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (w >= nrows) return;
    const uint32_t i = ib_owner(row0, T, w, 0);
    const uint8_t *b = st[i].b; const uint64_t N = st[i].N;
    const uint64_t base = SX_FIRST_BLOCK + (w - row0[i]) * SX_WAVE_POS;
    uint32_t cnt = 0;
    for (uint32_t it = 0; it < SX_WAVE_POS / 64u; it++) cnt += (uint32_t)__popcll(__ballot(sx_candidate(b, N, base + it * 64u + lane)));
    if (lane == 0) counts[w] = cnt;
}

__global__ __launch_bounds__(256) void k_ib_write(const IbStream *st, const uint64_t *row0, uint32_t T, uint64_t nrows, const uint64_t *first, uint64_t *cand)
{
    const uint64_t w = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (w >= nrows) return;
    const uint32_t i = ib_owner(row0, T, w, 0);
    const uint8_t *b = st[i].b; const uint64_t N = st[i].N;
    const uint64_t base = SX_FIRST_BLOCK + (w - row0[i]) * SX_WAVE_POS;
    const uint64_t below = (lane == 0u) ? 0ull : (~0ull >> (64u - lane));
    uint64_t at = first[w];
    for (uint32_t it = 0; it < SX_WAVE_POS / 64u; it++) {
        const uint64_t p = base + it * 64u + lane;
        const bool c = sx_candidate(b, N, p);
        const uint64_t m = __ballot(c);
        if (c) cand[at + (uint64_t)__popcll(m & below)] = p;
        at += (uint64_t)__popcll(m);
    }
}

/* seg[i] = cofs[row0[i]], i <= T */
__global__ __launch_bounds__(256) void k_ib_seg(const uint64_t *cofs, const uint64_t *row0, uint32_t T, uint64_t *seg)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i <= T) seg[i] = cofs[row0[i]];
}

/* succ[g]: the candidate of g's own stream at cand[g] + size + 6, or M (none); succ[M] = M */
__global__ __launch_bounds__(256) void k_ib_succ(const IbStream *st, const uint64_t *seg, uint32_t T, const uint64_t *cand, uint32_t M, uint32_t *succ)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > M) return;
    if (g == M) { succ[M] = M; return; }
    const uint32_t i = ib_owner(seg, T, g, 0), end = (uint32_t)seg[i + 1];
    const uint64_t p = cand[g], q = p + (uint64_t)sx_be32(st[i].b, p + 2) + 6u;
    uint32_t lo = g + 1u, hi = end;                                /* first index in (g, end) whose position is >= q */
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (cand[mid] < q) lo = mid + 1u; else hi = mid; }
    succ[g] = (lo < end && cand[lo] == q) ? lo : M;
}

/* per stream: the blocks of the chain from its head (levels K - 1 .. 0, greedily: the steps to its end, and the head itself), 0 where
 * its first candidate is not at byte 30 */
__global__ __launch_bounds__(256) void k_ib_chain_len(const uint64_t *seg, uint32_t T, const uint64_t *cand, const uint32_t *jump, uint32_t K, uint32_t M, uint64_t *len)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= T) return;
    uint64_t d = 0;
    if (seg[i] < seg[i + 1] && cand[seg[i]] == SX_FIRST_BLOCK) {
        uint32_t node = (uint32_t)seg[i];
        for (int32_t k = (int32_t)K - 1; k >= 0; k--) {
            const uint32_t nx = jump[(uint64_t)k * (M + 1u) + node];
            if (nx != M) { node = nx; d += 1ull << k; }
        }
        d++;
    }
    len[i] = d;
}

/* chain block e of the call (rank e - crow[i] of stream i): its position, size field, type and sample count */
__global__ __launch_bounds__(256) void k_ib_chain(const IbStream *st, const uint64_t *seg, const uint64_t *crow, uint32_t T, const uint64_t *cand,
        const uint32_t *jump, uint32_t K, uint32_t M, uint64_t nchain, uint64_t *off, uint32_t *size, uint32_t *type, uint32_t *nsmp)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= nchain) return;
    const uint32_t i = ib_owner(crow, T, e, 0), r = (uint32_t)(e - crow[i]);
    uint32_t node = (uint32_t)seg[i];
    for (uint32_t k = 0; k < K; k++) if ((r >> k) & 1u) node = jump[(uint64_t)k * (M + 1u) + node];
    const uint8_t *b = st[i].b;
    const uint64_t p = cand[node];
    off[e] = p; size[e] = sx_be32(b, p + 2); type[e] = b[p + 8]; nsmp[e] = sx_be16(b, p + 9);
}

/* first samples: stream i has len_i + 1 entries from crow[i] + i on, the global scan of the sample counts minus its value at the
 * stream's start */
__global__ __launch_bounds__(256) void k_ib_first(const uint64_t *scan, const uint64_t *crow, uint32_t T, uint64_t nentries, uint64_t *first)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= nentries) return;
    const uint32_t i = ib_owner(crow, T, e, 1);
    first[e] = scan[e - i] - scan[crow[i]];
}

/* A wave per chain block of the call (four per workgroup): the CRC, then what lnn_parse_block_head checks after it, in its order, with
 * the consumption test DecodeWhole makes on RAW and SILENT blocks (a block whose payload is not what its size field says is one no
 * encoder writes: LNN_NG).  status[g] = LNN_*; only the blocks a whole decode walks (first sample below the header's count) are looked
 * at, the others read LNN_OK */
struct IbCheckArgs {
    const IbStream *st; const uint64_t *crow; uint32_t T; uint64_t nchain;
    const uint64_t *off, *first; const uint32_t *size, *type, *nsmp;
    const SxTables *tab;
    int32_t *status;
};
__global__ __launch_bounds__(256) void k_ib_check(IbCheckArgs a)
{
    __shared__ uint16_t crc_t[256];
    __shared__ uint16_t shift_t[SX_CRC_LEVELS][16];
    for (uint32_t i = threadIdx.x; i < 256u; i += 256u) crc_t[i] = a.tab->crc[i];
    for (uint32_t i = threadIdx.x; i < SX_CRC_LEVELS * 16u; i += 256u) shift_t[i >> 4][i & 15u] = a.tab->shift[i >> 4][i & 15u];
    __syncthreads();
    const uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (g >= a.nchain) return;
    const uint32_t si = ib_owner(a.crow, a.T, g, 0);
    const IbStream s = a.st[si];
    const uint64_t first = a.first[g + si];
    if (first >= s.num_samples) { if (lane == 0u) a.status[g] = LNN_OK; return; }
    const uint64_t p = a.off[g];
    const uint32_t bsize = a.size[g];
    const uint64_t len = (uint64_t)bsize - 2u;                     /* the CRC covers [p + 8, p + 6 + size) (size >= 5: a candidate) */
    const uint64_t chunk = (len + 63u) >> 6, lo = (uint64_t)lane * chunk, hi = (lo + chunk < len) ? lo + chunk : len;
    uint32_t crc = 0;
    if (lo < len) {
        const uint8_t *q = s.b + p + 8u;
        uint64_t i = lo;
        for (; i + 4u <= hi; i += 4u) {
            const uint32_t b0 = q[i], b1 = q[i + 1], b2 = q[i + 2], b3 = q[i + 3];
            crc = (crc >> 8) ^ crc_t[(crc ^ b0) & 0xFFu];
            crc = (crc >> 8) ^ crc_t[(crc ^ b1) & 0xFFu];
            crc = (crc >> 8) ^ crc_t[(crc ^ b2) & 0xFFu];
            crc = (crc >> 8) ^ crc_t[(crc ^ b3) & 0xFFu];
        }
        for (; i < hi; i++) crc = (crc >> 8) ^ crc_t[(crc ^ q[i]) & 0xFFu];
        uint64_t behind = len - hi;                                /* the CRC is linear (initial 0, no final XOR): the lane's part, then the bytes behind it */
        for (uint32_t k = 0; behind != 0u && k < SX_CRC_LEVELS; k++, behind >>= 1) if (behind & 1u) crc = sx_apply(shift_t[k], crc);
    }
    for (uint32_t m = 32; m >= 1u; m >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, (int)m, 64);
    if (lane != 0u) return;
    int32_t stt = LNN_OK;
    const uint32_t type = a.type[g], n = a.nsmp[g];
    const uint64_t room = s.num_samples - first, avail = s.N - p;
    if (crc != sx_be16(s.b, p + 6)) stt = LNN_DETECT_DATA_CORRUPTION;
    else if (n > room || n > s.S) stt = LNN_INSUFFICIENT_BUFFER;
    else if (type == SX_RAW) {
        const uint64_t payload = ((uint64_t)s.bits * n * s.C) / 8u;
        if (s.bits != 8u && s.bits != 16u && s.bits != 24u) stt = LNN_INVALID_FORMAT;
        else if (avail - 11u < payload) stt = LNN_INSUFFICIENT_DATA;
        else if (11u + payload != (uint64_t)bsize + 6u) stt = LNN_NG;
    } else if (type == SX_SILENT) { if (bsize != 5u) stt = LNN_NG; }
    else if (type == SX_COMPRESS) { if (n == 0u) stt = LNN_INVALID_FORMAT; }
    else stt = LNN_INVALID_FORMAT;
    a.status[g] = stt;
}

/* the place behind a chain that ends before the header's sample count, where it lies inside the stream: the checks of
 * lnn_parse_block_head before the CRC (no candidate is there, so one of them fails; LNN_NG would be a head the index missed).
 * 0: the stream has no such place */
__global__ __launch_bounds__(256) void k_ib_behind(const IbStream *st, const uint64_t *crow, uint32_t T, const uint64_t *off, const uint32_t *size,
        const uint64_t *first, int32_t *behind)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= T) return;
    const uint8_t *b = st[i].b; const uint64_t N = st[i].N;
    const uint64_t c0 = crow[i], n = crow[i + 1] - c0;
    const uint64_t q = n ? off[c0 + n - 1u] + (uint64_t)size[c0 + n - 1u] + 6u : (uint64_t)SX_FIRST_BLOCK;
    int32_t code = 0;
    if (b && first[c0 + i + n] < st[i].num_samples && q < N) {
        if (N - q < 11u) code = LNN_INSUFFICIENT_DATA;
        else if (b[q] != 0xFFu || b[q + 1] != 0xFFu) code = LNN_INVALID_FORMAT;
        else {
            const uint32_t bsize = sx_be32(b, q + 2);
            if ((uint64_t)bsize + 6u > N - q) code = LNN_INSUFFICIENT_DATA;
            else code = bsize < 5u ? LNN_INVALID_FORMAT : LNN_NG;
        }
    }
    behind[i] = code;
}

#endif
