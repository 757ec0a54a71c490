/* lnn_k_stream.h -- what the kernels that read .lnn streams in device memory share: the tables, the test for a
 * block candidate, the prefix sum and the pointer-doubling step of the block index, the CRC shift, and the bit reader and parameter
 * walk of decoding a block.
 *
 *   sx_candidate              the checks lnn_parse_block_head makes before the CRC (data left >= 11, FFFF sync, size + 6 <= left,
 *                             size >= 5): a position that passes them is a block candidate
 *   k_sx_scan                 exclusive prefix sums (one workgroup): candidate offsets, the blocks' first samples, block offsets
 *   k_sx_jump                 pointer doubling: level k + 1 = level k applied twice
 *   sx_apply                  a CRC state fed 2^k zero bytes (a lane's partial CRC shifted by the bytes behind it)
 * The block index itself, for one stream or many in a call: lnn_k_index_batch.h.  Decoding sample ranges with it: lnn_k_windows.h.
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

__global__ __launch_bounds__(256) void k_sx_jump(const uint32_t *src, uint32_t *dst, uint32_t M)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i <= M) dst[i] = src[src[i]];
}

__device__ __forceinline__ uint32_t sx_apply(const uint16_t *m, uint32_t v)
{
    uint32_t r = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) r ^= (0u - ((v >> j) & 1u)) & (uint32_t)m[j];
    return r;
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
