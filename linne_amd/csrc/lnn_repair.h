/* lnn_repair.h -- the host's planning for LINNEAmd_RepairStreamsDevice ("Repairing damaged resident streams"):
 * from the blocks of a stream that are kept, the gaps between them, the samples every gap stands for, the SILENT blocks that fill it
 * and where every run of bytes of the output comes from and lands.  Plain host C++ with no HIP in it and no device pointer, so a small
 * stand-alone program -- or tests/test_repair_cpu.py through lnn_repair_plan -- can drive it.
 *
 * The rules are those of include/linne_amd.h (rules 4 to 6 of the repair section).  A "piece" is a kept block or a run of adjacent
 * kept blocks (the device hands over runs, a test hands over blocks): adjacent pieces are merged first, so both give one plan. */
#ifndef LNN_REPAIR_H_INCLUDED
#define LNN_REPAIR_H_INCLUDED

#include <stddef.h>
#include <stdint.h>
#include <vector>

#define RP_HEADER_BYTES 30u
#define RP_FILL_BYTES 11u               /* a SILENT block: FF FF, size field 5, CRC16, type 1, samples */
#define RP_OK 0
#define RP_INSUFFICIENT_BUFFER 3

/* B of rule 2: the bytes of the largest block the reference's encoder can write for one block of S samples of C channels at `bits`
 * bits per sample with a preset of L layers holding P coefficients in all (DESIGN.md derives it):
 *   11 bytes in front of the payload; per channel 2 * (bits + 1 + 4) bits of pre-emphasis, 7 bits per layer, at most 32 bits per
 *   coefficient (the width of the reference's Huffman code word), and a Rice code of at most 10 + 5 + 36 * S bits. */
static inline uint64_t rp_block_bound(uint64_t C, uint64_t S, uint64_t bits, uint64_t L, uint64_t P)
{
    const uint64_t per_channel = 2u * (bits + 5u) + 7u * L + 32u * P + 15u + 36u * S;
    return 11u + (C * per_channel + 7u) / 8u;
}

struct RpPiece { uint64_t off, bytes, samples; uint64_t blocks; };
struct RpGap {
    uint64_t first_sample, num_samples;         /* in the output's timeline */
    uint64_t src_off, src_bytes;                /* the bytes of the source it stands for */
    uint64_t fill_blocks, fill_at;              /* its SILENT blocks, and their offset in the stream's fill bytes */
};
struct RpRun { uint32_t fill; uint64_t src, dst, bytes; };     /* fill 0: bytes [src, src + bytes) of the source; 1: of the stream's fill bytes */
struct RpPlan {
    int32_t result;
    uint64_t bytes;                             /* the output's size (INSUFFICIENT_BUFFER: the size it needs) */
    uint64_t kept_blocks, fill_blocks, lost_samples;
    uint32_t exact;
    std::vector<RpGap> gaps;
    std::vector<RpRun> runs;                    /* none for an output that does not fit */
    std::vector<uint8_t> fill;                  /* the fill blocks of all gaps, gap by gap */
};

typedef uint16_t (*rp_crc_fn)(const uint8_t *data, uint64_t size);

static inline void rp_silent_block(uint8_t *out, uint32_t n, rp_crc_fn crc16)
{
    out[0] = 0xFFu; out[1] = 0xFFu; out[2] = out[3] = out[4] = 0u; out[5] = 5u;
    out[8] = 1u; out[9] = (uint8_t)(n >> 8); out[10] = (uint8_t)n;
    const uint16_t c = crc16(out + 8, 3);
    out[6] = (uint8_t)(c >> 8); out[7] = (uint8_t)c;
}

/* pieces: in stream order, not overlapping, at byte 30 or behind it, inside [0, stream_bytes), their samples no more than N in all */
static inline void rp_plan(const RpPiece *pieces, uint64_t npieces, uint64_t N, uint64_t S, uint64_t stream_bytes, uint64_t capacity,
        rp_crc_fn crc16, RpPlan &p)
{
    p.result = RP_OK; p.bytes = 0; p.kept_blocks = p.fill_blocks = p.lost_samples = 0; p.exact = 1u;
    p.gaps.clear(); p.runs.clear(); p.fill.clear();
    /* the runs of adjacent kept blocks */
    std::vector<RpPiece> kept;
    uint64_t kept_samples = 0;
    for (uint64_t i = 0; i < npieces; i++) {
        const RpPiece &q = pieces[i];
        if (!kept.empty() && kept.back().off + kept.back().bytes == q.off) { kept.back().bytes += q.bytes; kept.back().samples += q.samples; kept.back().blocks += q.blocks; }
        else kept.push_back(q);
        kept_samples += q.samples; p.kept_blocks += q.blocks;
    }
    const uint64_t M = N - kept_samples;
    p.lost_samples = M;
    /* rule 4: the gaps.  before[r]: the gap in front of run r (-1: none); the trailing gap is the last one */
    std::vector<int64_t> before(kept.size(), -1);
    uint64_t at = RP_HEADER_BYTES, sum_b = 0;
    for (size_t r = 0; r < kept.size(); r++) {
        if (kept[r].off != at) {
            RpGap g = { 0, 0, at, kept[r].off - at, 0, 0 };
            before[r] = (int64_t)p.gaps.size(); p.gaps.push_back(g); sum_b += g.src_bytes;
        }
        at = kept[r].off + kept[r].bytes;
    }
    const bool trailing = kept_samples < N && (stream_bytes > at || p.gaps.empty());     /* (0 bytes behind the last block and a gap before it: that gap stands for M) */
    if (trailing) { RpGap g = { 0, 0, at, stream_bytes - at, 0, 0 }; p.gaps.push_back(g); sum_b += g.src_bytes; }
    const size_t ng = p.gaps.size();
    p.exact = ng <= 1u ? 1u : 0u;
    if (ng == 1u) p.gaps[0].num_samples = M;
    else if (ng > 1u) {
        uint64_t given = 0;
        for (size_t i = 0; i + 1u < ng; i++) {
            const uint64_t g = sum_b ? (uint64_t)(((unsigned __int128)M * p.gaps[i].src_bytes) / sum_b) : 0u;
            p.gaps[i].num_samples = g; given += g;
        }
        p.gaps[ng - 1u].num_samples = M - given;           /* the remainder; with no bytes in any gap, everything */
    }
    /* rules 5 and 6: sizes first, then the verdict on the capacity, then the bytes */
    const uint64_t F = S < 65535u ? S : 65535u;
    uint64_t fill_at = 0, sample = 0, out = RP_HEADER_BYTES;
    auto size_gap = [&](RpGap &g) {
        g.first_sample = sample; sample += g.num_samples;
        g.fill_blocks = (g.num_samples + F - 1u) / F; g.fill_at = fill_at;
        fill_at += g.fill_blocks * RP_FILL_BYTES; out += g.fill_blocks * RP_FILL_BYTES; p.fill_blocks += g.fill_blocks;
    };
    for (size_t r = 0; r < kept.size(); r++) {
        if (before[r] >= 0) size_gap(p.gaps[(size_t)before[r]]);
        sample += kept[r].samples; out += kept[r].bytes;
    }
    if (trailing) size_gap(p.gaps[ng - 1u]);
    p.bytes = out;
    if (out > capacity || out > 0xFFFFFFFFull) { p.result = RP_INSUFFICIENT_BUFFER; return; }
    p.fill.resize((size_t)fill_at);
    uint64_t dst = 0;
    auto put = [&](uint32_t fill, uint64_t src, uint64_t bytes) {
        if (!bytes) return;
        if (!fill && !p.runs.empty() && !p.runs.back().fill && p.runs.back().src + p.runs.back().bytes == src) p.runs.back().bytes += bytes;
        else { RpRun r = { fill, src, dst, bytes }; p.runs.push_back(r); }
        dst += bytes;
    };
    auto put_gap = [&](const RpGap &g) {
        uint64_t left = g.num_samples;
        for (uint64_t k = 0; k < g.fill_blocks; k++) {
            const uint64_t n = left < F ? left : F;
            rp_silent_block(p.fill.data() + g.fill_at + k * RP_FILL_BYTES, (uint32_t)n, crc16);
            left -= n;
        }
        put(1u, g.fill_at, g.fill_blocks * RP_FILL_BYTES);
    };
    put(0u, 0u, RP_HEADER_BYTES);
    for (size_t r = 0; r < kept.size(); r++) {
        if (before[r] >= 0) put_gap(p.gaps[(size_t)before[r]]);
        put(0u, kept[r].off, kept[r].bytes);
    }
    if (trailing) put_gap(p.gaps[ng - 1u]);
}

#endif
