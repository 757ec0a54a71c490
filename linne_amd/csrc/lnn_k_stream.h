/* lnn_k_stream.h -- the block index of a .lnn stream that lies in device memory (LINNEAmd_StreamIndexCreate),
 * and the bit reader and parameter walk that decoding its blocks shares with it.
 *
 * Block index, built once per stream:
 *   k_sx_count / k_sx_write   every position from the first block on that passes the checks lnn_parse_block_head makes before the
 *                             CRC (data left >= 11, FFFF sync, size + 6 <= left, size >= 5) is a candidate; a wave scans 4096
 *                             positions, counts, and after a scan of the counts writes its candidates in stream order
 *   k_sx_succ                 a candidate's successor: the candidate at position + size + 6 (binary search), or none
 *   k_sx_jump                 pointer doubling: level k + 1 = level k applied twice
 *   k_sx_chain_len, k_sx_chain  the chain from the head (position 30) enumerated by its ranks: rank r is the head's successor
 *                             taken r times, read off the levels by the bits of r.  A false candidate (FF FF inside a payload)
 *                             is never the successor of a node the head reaches, so the chain never holds one
 *   k_sx_scan                 exclusive prefix sums (one workgroup): candidate offsets, the blocks' first samples
 *   k_sx_check                a wave per block: CRC16 over lanes (partial CRCs shifted by the bytes behind them and XORed),
 *                             then the checks lnn_parse_block_head makes after the CRC, in its order
 * Decoding sample ranges with the index, one or many in a call: lnn_k_windows.h.
 * Every read of the stream is a byte load inside [0, stream_bytes): the caller's bytes may lie at any alignment.
 */
#ifndef LNN_K_STREAM_H_INCLUDED
#define LNN_K_STREAM_H_INCLUDED

#define SX_FIRST_BLOCK 30u              /* LINNE_HEADER_SIZE */
#define SX_WAVE_POS 4096u               /* positions one wave scans for candidates */
#define SX_SCAN_THREADS 1024u
#define SX_CRC_LEVELS 40u               /* shift matrices x^(8 * 2^k), k < 40: blocks of up to 2^40 bytes */
#define SX_PLACE_THREADS 256u
#define SX_COMPRESS 0u                  /* block types (lnn_host.h LNN_BLOCK_*) */
#define SX_SILENT 1u
#define SX_RAW 2u

/* the tables a stream decode needs in device memory (built on the host once per index) */
struct SxTables {
    uint16_t crc[256];                  /* CRC-16/ARC, reflected 0xA001 (lnn_entropy.c crc_init) */
    uint16_t shift[SX_CRC_LEVELS][16];  /* column j of the map "feed 2^k zero bytes" applied to the CRC state 1 << j */
    uint16_t child[512][2];             /* the static Huffman tree of the coefficients (lnn_entropy.c huff_init) */
    uint32_t root;
};

__device__ __forceinline__ uint32_t sx_byte(const uint8_t *b, uint64_t N, uint64_t p) { return p < N ? (uint32_t)b[p] : 0u; }
__device__ __forceinline__ uint32_t sx_be16(const uint8_t *b, uint64_t p) { return ((uint32_t)b[p] << 8) | b[p + 1]; }
__device__ __forceinline__ uint32_t sx_be32(const uint8_t *b, uint64_t p) { return ((uint32_t)b[p] << 24) | ((uint32_t)b[p + 1] << 16) | ((uint32_t)b[p + 2] << 8) | b[p + 3]; }
__device__ __forceinline__ int32_t sx_unzz(uint32_t u) { return (int32_t)((u >> 1) ^ (0u - (u & 1u))); }

/* the checks of lnn_parse_block_head before the CRC (lnn_entropy.c:881-885) */
__device__ __forceinline__ bool sx_candidate(const uint8_t *b, uint64_t N, uint64_t p)
{
    if (p + 11u > N) return false;
    if (b[p] != 0xFFu || b[p + 1] != 0xFFu) return false;
    const uint32_t size = sx_be32(b, p + 2);
    return (uint64_t)size + 6u <= N - p && size >= 5u;
}

__global__ __launch_bounds__(256) void k_sx_count(const uint8_t *b, uint64_t N, uint64_t nwaves, uint32_t *counts)
{
    const uint64_t w = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (w >= nwaves) return;
    const uint64_t base = SX_FIRST_BLOCK + w * SX_WAVE_POS;
    uint32_t cnt = 0;
    for (uint32_t it = 0; it < SX_WAVE_POS / 64u; it++) {
        const uint64_t p = base + it * 64u + lane;
        cnt += (uint32_t)__popcll(__ballot(sx_candidate(b, N, p)));
    }
    if (lane == 0) counts[w] = cnt;
}

__global__ __launch_bounds__(256) void k_sx_write(const uint8_t *b, uint64_t N, uint64_t nwaves, const uint64_t *first, uint64_t *cand)
{
    const uint64_t w = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (w >= nwaves) return;
    const uint64_t base = SX_FIRST_BLOCK + w * SX_WAVE_POS;
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

/* out[i] = in[0] + ... + in[i - 1] for i <= n (out[n]: the total); one workgroup of SX_SCAN_THREADS */
__global__ __launch_bounds__(SX_SCAN_THREADS) void k_sx_scan(const uint32_t *in, uint64_t n, uint64_t *out)
{
    __shared__ uint64_t wsum[SX_SCAN_THREADS / 64u];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < n; b0 += SX_SCAN_THREADS) {
        const uint64_t i = b0 + t;
        const uint64_t v = i < n ? (uint64_t)in[i] : 0ull;
        uint64_t x = v;                                            /* inclusive scan within the wave */
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t y = (uint64_t)__shfl_up((long long)x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63u) wsum[wv] = x;
        __syncthreads();
        uint64_t before = carry, tile = 0;
        for (uint32_t k = 0; k < SX_SCAN_THREADS / 64u; k++) { if (k < wv) before += wsum[k]; tile += wsum[k]; }
        if (i < n) out[i] = before + x - v;
        carry += tile;
        __syncthreads();
    }
    if (t == 0) out[n] = carry;
}

/* succ[i]: the candidate at cand[i] + size + 6, or M (none); succ[M] = M */
__global__ __launch_bounds__(256) void k_sx_succ(const uint8_t *b, const uint64_t *cand, uint32_t M, uint32_t *succ)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > M) return;
    if (i == M) { succ[M] = M; return; }
    const uint64_t p = cand[i], q = p + (uint64_t)sx_be32(b, p + 2) + 6u;
    uint32_t lo = i + 1u, hi = M;                                  /* first index in (i, M) whose position is >= q */
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (cand[mid] < q) lo = mid + 1u; else hi = mid; }
    succ[i] = (lo < M && cand[lo] == q) ? lo : M;
}

__global__ __launch_bounds__(256) void k_sx_jump(const uint32_t *src, uint32_t *dst, uint32_t M)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i <= M) dst[i] = src[src[i]];
}

/* the number of steps from the head (candidate 0) to the end of its chain: levels K - 1 .. 0, greedily */
__global__ void k_sx_chain_len(const uint32_t *jump, uint32_t K, uint32_t M, uint64_t *len)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t node = 0; uint64_t d = 0;
    for (int32_t k = (int32_t)K - 1; k >= 0; k--) {
        const uint32_t nx = jump[(uint64_t)k * (M + 1u) + node];
        if (nx != M) { node = nx; d += 1ull << k; }
    }
    *len = d;
}

/* rank r of the head's chain, r < nb: its position, size field, type and sample count */
__global__ __launch_bounds__(256) void k_sx_chain(const uint8_t *b, const uint64_t *cand, const uint32_t *jump, uint32_t K, uint32_t M,
        uint32_t nb, uint64_t *off, uint32_t *size, uint32_t *type, uint32_t *nsmp)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= nb) return;
    uint32_t node = 0;
    for (uint32_t k = 0; k < K; k++) if ((r >> k) & 1u) node = jump[(uint64_t)k * (M + 1u) + node];
    const uint64_t p = cand[node];
    off[r] = p; size[r] = sx_be32(b, p + 2); type[r] = b[p + 8]; nsmp[r] = sx_be16(b, p + 9);
}

__device__ __forceinline__ uint32_t sx_apply(const uint16_t *m, uint32_t v)
{
    uint32_t r = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) r ^= (0u - ((v >> j) & 1u)) & (uint32_t)m[j];
    return r;
}

/* A wave per block (four per workgroup): the CRC, then what lnn_parse_block_head checks after it, in its order (lnn_entropy.c:
 * 886-938), with the consumption test DecodeWhole makes on RAW and SILENT blocks (a block whose payload is not what its size field
 * says is one no encoder writes: LNN_NG).  status[r] = LNN_* */
struct SxCheckArgs {
    const uint8_t *b; uint64_t N;
    const uint64_t *off, *first; const uint32_t *size, *type, *nsmp;
    uint32_t nb, C, S, bits; uint64_t num_samples;
    const SxTables *tab;
    int32_t *status;
};
__global__ __launch_bounds__(256) void k_sx_check(SxCheckArgs a)
{
    __shared__ uint16_t crc_t[256];
    __shared__ uint16_t shift_t[SX_CRC_LEVELS][16];
    for (uint32_t i = threadIdx.x; i < 256u; i += 256u) crc_t[i] = a.tab->crc[i];
    for (uint32_t i = threadIdx.x; i < SX_CRC_LEVELS * 16u; i += 256u) shift_t[i >> 4][i & 15u] = a.tab->shift[i >> 4][i & 15u];
    __syncthreads();
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (r >= a.nb) return;
    const uint64_t p = a.off[r];
    const uint32_t bsize = a.size[r];
    const uint64_t len = (uint64_t)bsize - 2u;                     /* the CRC covers [p + 8, p + 6 + size) (size >= 5: a candidate) */
    const uint64_t chunk = (len + 63u) >> 6, s = (uint64_t)lane * chunk, e = (s + chunk < len) ? s + chunk : len;
    uint32_t crc = 0;
    if (s < len) {
        const uint8_t *q = a.b + p + 8u;
        uint64_t i = s;
        for (; i + 4u <= e; i += 4u) {
            const uint32_t b0 = q[i], b1 = q[i + 1], b2 = q[i + 2], b3 = q[i + 3];
            crc = (crc >> 8) ^ crc_t[(crc ^ b0) & 0xFFu];
            crc = (crc >> 8) ^ crc_t[(crc ^ b1) & 0xFFu];
            crc = (crc >> 8) ^ crc_t[(crc ^ b2) & 0xFFu];
            crc = (crc >> 8) ^ crc_t[(crc ^ b3) & 0xFFu];
        }
        for (; i < e; i++) crc = (crc >> 8) ^ crc_t[(crc ^ q[i]) & 0xFFu];
        /* the CRC is linear (initial value 0, no final XOR): the lane's part followed by the len - e bytes behind it */
        uint64_t behind = len - e;
        for (uint32_t k = 0; behind != 0u && k < SX_CRC_LEVELS; k++, behind >>= 1) if (behind & 1u) crc = sx_apply(shift_t[k], crc);
    }
    for (uint32_t m = 32; m >= 1u; m >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, (int)m, 64);
    if (lane != 0u) return;
    int32_t st = LNN_OK;
    const uint32_t type = a.type[r], n = a.nsmp[r];
    const uint64_t room = a.num_samples - a.first[r], avail = a.N - p;
    if (crc != sx_be16(a.b, p + 6)) st = LNN_DETECT_DATA_CORRUPTION;
    else if (n > room || n > a.S) st = LNN_INSUFFICIENT_BUFFER;
    else if (type == SX_RAW) {
        const uint64_t payload = ((uint64_t)a.bits * n * a.C) / 8u;
        if (a.bits != 8u && a.bits != 16u && a.bits != 24u) st = LNN_INVALID_FORMAT;
        else if (avail - 11u < payload) st = LNN_INSUFFICIENT_DATA;
        else if (11u + payload != (uint64_t)bsize + 6u) st = LNN_NG;
    } else if (type == SX_SILENT) { if (bsize != 5u) st = LNN_NG; }
    else if (type == SX_COMPRESS) { if (n == 0u) st = LNN_INVALID_FORMAT; }
    else st = LNN_INVALID_FORMAT;
    a.status[r] = st;
}

/* the host's bit reader (lnn_entropy.c struct bitr): MSB first, zeros beyond the stream's end */
struct SxBits {
    const uint8_t *b; uint64_t N, next; uint64_t win; uint32_t have; uint64_t consumed;
    __device__ __forceinline__ void open(const uint8_t *b_, uint64_t N_, uint64_t at) { b = b_; N = N_; next = at; win = 0; have = 0; consumed = 0; }
    __device__ __forceinline__ uint32_t get(uint32_t n) {          /* n <= 33: the low 32 bits of the next n bits, as br_get */
        if (n == 0u) return 0u;
        while (have < n) { win |= (uint64_t)sx_byte(b, N, next) << (56u - have); next++; have += 8u; }
        const uint32_t v = (uint32_t)(win >> (64u - n));
        win <<= n; have -= n; consumed += n;
        return v;
    }
};

/* lnn_parse_block_head's parameter part (lnn_entropy.c:912-932) of one block, read from r into base[C][LINNE_AMD_PARAM_WORDS]:
 * the records are serial within a block.  child: the Huffman tree (in LDS) */
__device__ __forceinline__ void sx_parse_params(SxBits &r, const uint16_t (*child)[2], uint32_t root, uint32_t C, uint32_t bits, uint32_t L,
        const uint32_t *P, const uint32_t *coef_off, int32_t *base)
{
    for (uint32_t ch = 0; ch < C; ch++) {
        int32_t *rec = base + (uint64_t)ch * LINNE_AMD_PARAM_WORDS;
        for (uint32_t w = 0; w < LINNE_AMD_PARAM_WORDS; w++) rec[w] = 0;
        for (uint32_t l = 0; l < 2u; l++) {
            rec[LINNE_AMD_PRM_PREV + l] = sx_unzz(r.get(bits + 1u));
            rec[LINNE_AMD_PRM_PCOEF + l] = (int32_t)r.get(4);
        }
    }
    for (uint32_t ch = 0; ch < C; ch++) {
        int32_t *rec = base + (uint64_t)ch * LINNE_AMD_PARAM_WORDS;
        for (uint32_t l = 0; l < L; l++) {
            rec[LINNE_AMD_PRM_UNITS + l] = (int32_t)(1u << r.get(3));
            rec[LINNE_AMD_PRM_RSHIFT + l] = (int32_t)r.get(4);
            for (uint32_t i = 0; i < P[l]; i++) {
                uint32_t node = root;
                do { node = child[node][r.get(1)]; } while (node >= 256u);
                rec[LINNE_AMD_PRM_COEF + coef_off[l] + i] = sx_unzz(node);
            }
        }
    }
}

#endif
