/* lnn_k_repair.h -- the device side of LINNEAmd_RepairStreamsDevice (lnn_device.hip; DESIGN.md section 5, "Repairing damaged
 * resident streams"): the salvage chains of all streams of a call, segmented as the batch index is (lnn_k_index_batch.h: candidates
 * are numbered over the whole call, `seg` holds every stream's first one, ib_owner places a number in its stream).
 *
 *   k_rp_sound      a wave per candidate: 0 when its block is larger than the stream's bound B, else the CRC16 over 64 slices
 *                   (k_ib_check's: partial CRCs shifted by the bytes behind them and XORed) and the structural checks of rule 2
 *   k_rp_compact    the sound candidates' positions in stream order, behind a scan of the flags (k_sx_scan)
 *   k_rp_succ       a sound candidate's successor: the lowest sound candidate of its own stream at or behind its block's end
 *                   (lower bound by bisection), or M (none).  The levels above it are k_sx_jump's, unchanged
 *   k_rp_chain_len  per stream the blocks of the chain from its first sound candidate
 *   (k_ib_chain enumerates the chains by rank, k_sx_scan sums their sample counts)
 *   k_rp_mark       chain block e is kept while the samples up to and including it do not exceed the header's count; a kept block
 *                   that does not begin where the kept block before it ends begins a run
 *   k_rp_runs       one record per run, behind a scan of the marks: where it begins and ends in bytes, samples and ranks
 *
 * The sound candidates number at most M, the candidates; the host does not wait to learn how many there are: arrays over them have
 * M + 1 entries, the count is read on the device, and entries from the count on point to M like "none" does.
 * Every read of stream i is a byte load inside [0, N_i): a candidate's block lies inside its stream (sx_candidate).  Candidates may
 * overlap -- a false one lies inside a true block -- so the bytes two waves of k_rp_sound read are bounded by B each, not disjoint.
 */
#ifndef LNN_K_REPAIR_H_INCLUDED
#define LNN_K_REPAIR_H_INCLUDED

struct RpRunRec { uint64_t off0, off1, smp0, smp1; uint32_t rank0, rank1; };

struct RpSoundArgs {
    const IbStream *st; const uint64_t *bound;      /* per stream: B */
    const uint64_t *seg; uint32_t T; uint32_t M;
    const uint64_t *cand;
    const SxTables *tab;
    uint32_t *flag;
};
__global__ __launch_bounds__(256) void k_rp_sound(RpSoundArgs a)
{
    __shared__ uint16_t crc_t[256];
    __shared__ uint16_t shift_t[SX_CRC_LEVELS][16];
    for (uint32_t i = threadIdx.x; i < 256u; i += 256u) crc_t[i] = a.tab->crc[i];
    for (uint32_t i = threadIdx.x; i < SX_CRC_LEVELS * 16u; i += 256u) shift_t[i >> 4][i & 15u] = a.tab->shift[i >> 4][i & 15u];
    __syncthreads();
    const uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (g >= a.M) return;
    const uint32_t si = ib_owner(a.seg, a.T, g, 0);
    const IbStream s = a.st[si];
    const uint64_t p = a.cand[g];
    const uint32_t bsize = sx_be32(s.b, p + 2);                    /* >= 5 and p + bsize + 6 <= N: a candidate */
    if ((uint64_t)bsize + 6u > a.bound[si]) { if (lane == 0u) a.flag[g] = 0u; return; }
    const uint64_t len = (uint64_t)bsize - 2u;                     /* the CRC covers [p + 8, p + 6 + size) */
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
        uint64_t behind = len - hi;                                /* the lane's part followed by the bytes behind it (k_ib_check) */
        for (uint32_t k = 0; behind != 0u && k < SX_CRC_LEVELS; k++, behind >>= 1) if (behind & 1u) crc = sx_apply(shift_t[k], crc);
    }
    for (uint32_t m = 32; m >= 1u; m >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, (int)m, 64);
    if (lane != 0u) return;
    const uint32_t type = s.b[p + 8], n = sx_be16(s.b, p + 9);
    bool ok = crc == sx_be16(s.b, p + 6) && n >= 1u && n <= s.S;
    if (ok) {
        if (type == SX_RAW) ok = (s.bits == 8u || s.bits == 16u || s.bits == 24u) && 11u + ((uint64_t)s.bits * n * s.C) / 8u == (uint64_t)bsize + 6u;
        else if (type == SX_SILENT) ok = bsize == 5u;
        else ok = type == SX_COMPRESS;
    }
    a.flag[g] = ok ? 1u : 0u;
}

/* spos[sofs[g]] = cand[g] for the sound ones (sofs: the exclusive scan of the flags) */
__global__ __launch_bounds__(256) void k_rp_compact(const uint32_t *flag, const uint64_t *sofs, const uint64_t *cand, uint32_t M, uint64_t *spos)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < M && flag[g]) spos[sofs[g]] = cand[g];
}

/* succ[g], g <= M; sseg: every stream's first sound candidate, sseg[T] their count */
__global__ __launch_bounds__(256) void k_rp_succ(const IbStream *st, const uint64_t *sseg, uint32_t T, const uint64_t *spos, uint32_t M, uint32_t *succ)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > M) return;
    if ((uint64_t)g >= sseg[T]) { succ[g] = M; return; }
    const uint32_t i = ib_owner(sseg, T, g, 0), end = (uint32_t)sseg[i + 1];
    const uint64_t p = spos[g], q = p + (uint64_t)sx_be32(st[i].b, p + 2) + 6u;
    uint32_t lo = g + 1u, hi = end;                                /* first index in (g, end) whose position is >= q */
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (spos[mid] < q) lo = mid + 1u; else hi = mid; }
    succ[g] = lo < end ? lo : M;
}

__global__ __launch_bounds__(256) void k_rp_chain_len(const uint64_t *sseg, uint32_t T, const uint32_t *jump, uint32_t K, uint32_t M, uint64_t *len)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= T) return;
    uint64_t d = 0;
    if (sseg[i] < sseg[i + 1]) {
        uint32_t node = (uint32_t)sseg[i];
        for (int32_t k = (int32_t)K - 1; k >= 0; k--) {
            const uint32_t nx = jump[(uint64_t)k * (M + 1u) + node];
            if (nx != M) { node = nx; d += 1ull << k; }
        }
        d++;
    }
    len[i] = d;
}

/* scan: the exclusive scan of the chain blocks' sample counts over the whole call (nchain + 1 entries) */
__device__ __forceinline__ bool rp_kept(const IbStream *st, const uint64_t *crow, const uint64_t *scan, uint32_t i, uint64_t e)
{
    return scan[e + 1u] - scan[crow[i]] <= st[i].num_samples;
}

struct RpRunArgs {
    const IbStream *st; const uint64_t *crow; uint32_t T; uint64_t nchain;
    const uint64_t *off; const uint32_t *size; const uint64_t *scan;
    uint32_t *mark;                     /* k_rp_mark: 1 where a run begins */
    const uint64_t *rofs;               /* k_rp_runs: the exclusive scan of the marks */
    RpRunRec *rec;
};
__global__ __launch_bounds__(256) void k_rp_mark(RpRunArgs a)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= a.nchain) return;
    const uint32_t i = ib_owner(a.crow, a.T, e, 0);
    const bool begins = rp_kept(a.st, a.crow, a.scan, i, e) && (e == a.crow[i] || a.off[e] != a.off[e - 1u] + (uint64_t)a.size[e - 1u] + 6u);
    a.mark[e] = begins ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_rp_runs(RpRunArgs a)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= a.nchain) return;
    const uint32_t i = ib_owner(a.crow, a.T, e, 0);
    if (!rp_kept(a.st, a.crow, a.scan, i, e)) return;
    const uint64_t c0 = a.crow[i], end = a.off[e] + (uint64_t)a.size[e] + 6u;
    RpRunRec *r = a.rec + (a.rofs[e + 1u] - 1u);                    /* the run e lies in: the marks up to and including e, less one */
    if (a.mark[e]) { r->off0 = a.off[e]; r->smp0 = a.scan[e] - a.scan[c0]; r->rank0 = (uint32_t)(e - c0); }
    if (e + 1u == a.crow[i + 1u] || !rp_kept(a.st, a.crow, a.scan, i, e + 1u) || a.off[e + 1u] != end) {
        r->off1 = end; r->smp1 = a.scan[e + 1u] - a.scan[c0]; r->rank1 = (uint32_t)(e + 1u - c0);
    }
}

#endif
