/* lnn_splice.h -- the host's planning for LINNEAmd_SpliceStreamsDevice ("Cutting and joining resident
 * streams"): which pieces every output is made of, and where they land.  Plain host C++ with no HIP in it and no device pointer:
 * it works on the host tables an index keeps of its stream's blocks (LINNEAmd_StreamIndexBlocks), so a small stand-alone program --
 * or tests/test_splice_cpu.py through lnn_splice_plan -- can drive it.
 *
 * A cut [first, first + n) of a stream gives, in sample order, at most three pieces: the fragment of the block its first sample lies
 * in (when the cut does not begin at that block's first sample, or ends inside it), ONE copy piece for the maximal run of blocks it
 * covers whole (contiguous bytes of the source), and the fragment of the block its last sample lies in.  A fragment is re-encoded by
 * the caller; once its block's size is known (SpPiece.bytes), sp_place gives every piece its offset in its output, every output its
 * size and the verdict on its capacity. */
#ifndef LNN_SPLICE_H_INCLUDED
#define LNN_SPLICE_H_INCLUDED

#include <stdint.h>
#include <vector>

#ifdef __HIPCC__
#define SP_HD __host__ __device__
#else
#define SP_HD
#endif

#define SP_HEADER_BYTES 30u
#define SP_CHUNK_UNITS 2048u            /* 16-byte destination units a workgroup of k_sp_copy moves per chunk: 32 KiB */
/* result codes (LINNEApiResult's values) */
#define SP_OK 0
#define SP_INVALID_ARGUMENT 1
#define SP_INSUFFICIENT_BUFFER 3

/* why an output is refused with INVALID_ARGUMENT (0: it is not) */
enum { SP_WHY_NONE = 0, SP_WHY_NULL, SP_WHY_ALIGN, SP_WHY_NO_CUTS, SP_WHY_RANGE, SP_WHY_UNREACHED, SP_WHY_SHAPE, SP_WHY_EMPTY, SP_WHY_TOTAL,
       SP_WHY_SHORT_FRAGMENT, SP_WHY_DEVICE };

static inline const char *sp_why_text(int why)
{
    switch (why) {
    case SP_WHY_NULL: return "null argument";
    case SP_WHY_ALIGN: return "d_out is not 4-byte aligned";
    case SP_WHY_NO_CUTS: return "no cuts";
    case SP_WHY_RANGE: return "a cut beyond its stream's samples";
    case SP_WHY_UNREACHED: return "a cut beyond the samples its stream's blocks reach";
    case SP_WHY_SHAPE: return "the cuts' streams differ in channels, bits, rate, block size, preset or MS";
    case SP_WHY_EMPTY: return "0 samples in all";
    case SP_WHY_TOTAL: return "more than 2^32 - 1 samples in all";
    case SP_WHY_SHORT_FRAGMENT: return "a cut leaves an edge block of no more samples than the preset's largest layer";
    case SP_WHY_DEVICE: return "an index belongs to another device";
    default: return "";
    }
}

/* a source stream as its index describes it */
struct SpStream {
    const uint64_t *off, *first;        /* [nb], [nb + 1] */
    const uint32_t *size, *nsmp;        /* [nb] */
    uint32_t nb;
    uint64_t num_samples;               /* the header's count */
    uint32_t channels, bits, rate, block, preset, ms;
    int64_t fail_block; int32_t fail_code;      /* the index's lowest failing block (-1: none) and its code */
};
struct SpCut { int32_t stream; uint64_t first, n; };            /* stream: number in the streams' list, -1 for a NULL index or stream pointer */
struct SpOutput {
    uint32_t cut0, ncuts;               /* its cuts in the cuts' list */
    int why0;                           /* SP_WHY_* of its own pointers (NULL, alignment, device), checked by the caller */
    uint64_t capacity;
    /* out */
    int32_t result; int why; int64_t fail_block; uint32_t fail_cut;
    uint64_t total_samples, bytes;
    uint32_t copied_blocks, encoded_blocks;
    uint32_t piece0, npieces;           /* its pieces in the pieces' list (none for a failing output) */
};
struct SpPiece {
    uint32_t out, cut;
    uint32_t frag;                      /* 0: bytes [a, b) of the cut's stream, `blocks` whole blocks; 1: its samples [a, b), to be re-encoded */
    uint32_t blocks;
    uint64_t a, b;
    uint64_t bytes;                     /* copy: b - a; fragment: set by the caller before sp_place */
    uint64_t dst;                       /* sp_place: its offset in its output */
};

static inline uint32_t sp_max_order(uint32_t preset) { return preset < 2u ? 32u : (preset < 5u ? 64u : 128u); }

/* the block holding sample s (s < first[nb]): the last r with first[r] <= s */
static inline uint32_t sp_block_of(const SpStream &x, uint64_t s)
{
    uint32_t lo = 0, hi = x.nb;
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (x.first[mid] <= s) lo = mid; else hi = mid; }
    return lo;
}

static inline bool sp_same_shape(const SpStream &a, const SpStream &b)
{
    return a.channels == b.channels && a.bits == b.bits && a.rate == b.rate && a.block == b.block && a.preset == b.preset && a.ms == b.ms;
}

/* Steps 1 and 2: every output's checks, in the header's order -- its own pointers, its cuts' arguments (all of them, before any
 * damage counts), then the first cut, in order, whose stream's failing block lies at or before the last block the cut overlaps --
 * and the pieces of the outputs that pass. */
static inline void sp_plan(const SpStream *streams, const SpCut *cuts, SpOutput *outs, uint32_t nouts, std::vector<SpPiece> &pieces)
{
    pieces.clear();
    for (uint32_t k = 0; k < nouts; k++) {
        SpOutput &o = outs[k];
        o.result = SP_OK; o.why = SP_WHY_NONE; o.fail_block = -1; o.fail_cut = 0; o.total_samples = 0; o.bytes = 0;
        o.copied_blocks = o.encoded_blocks = 0; o.piece0 = (uint32_t)pieces.size(); o.npieces = 0;
        int why = o.why0;
        if (!why && o.ncuts == 0) why = SP_WHY_NO_CUTS;
        uint64_t total = 0; bool over = false;
        for (uint32_t i = 0; !why && i < o.ncuts; i++) {
            const SpCut &c = cuts[o.cut0 + i];
            if (c.stream < 0) { why = SP_WHY_NULL; break; }
            const SpStream &x = streams[c.stream];
            if (c.first > x.num_samples || c.n > x.num_samples - c.first) { why = SP_WHY_RANGE; break; }
            if (!sp_same_shape(x, streams[cuts[o.cut0].stream])) { why = SP_WHY_SHAPE; break; }
            if (c.n && c.first + c.n > x.first[x.nb] && !(x.fail_block >= 0)) { why = SP_WHY_UNREACHED; break; }
            total += c.n; if (total > 0xFFFFFFFFull) over = true;
        }
        if (!why && over) why = SP_WHY_TOTAL;
        if (!why && total == 0) why = SP_WHY_EMPTY;
        if (why) { o.result = SP_INVALID_ARGUMENT; o.why = why; continue; }
        /* damage: DecodeStreamDevice's rule, cut by cut */
        for (uint32_t i = 0; i < o.ncuts && o.result == SP_OK; i++) {
            const SpCut &c = cuts[o.cut0 + i];
            if (c.n == 0) continue;
            const SpStream &x = streams[c.stream];
            const uint64_t hi = c.first + c.n;
            const uint64_t r1 = (hi - 1u < x.first[x.nb]) ? sp_block_of(x, hi - 1u) : x.nb;
            if (x.fail_block >= 0 && (uint64_t)x.fail_block <= r1) { o.result = x.fail_code; o.fail_block = x.fail_block; o.fail_cut = i; }
        }
        if (o.result != SP_OK) continue;
        /* the pieces */
        for (uint32_t i = 0; i < o.ncuts && !why; i++) {
            const SpCut &c = cuts[o.cut0 + i];
            if (c.n == 0) continue;
            const SpStream &x = streams[c.stream];
            const uint64_t lo = c.first, hi = c.first + c.n;
            const uint32_t r0 = sp_block_of(x, lo), r1 = sp_block_of(x, hi - 1u);
            uint32_t w0 = r0, w1 = r1 + 1u;                     /* the wholly covered blocks [w0, w1) */
            SpPiece p; p.out = k; p.cut = i; p.dst = 0;
            auto fragment = [&](uint64_t a, uint64_t b) {
                if (b - a <= sp_max_order(x.preset)) why = SP_WHY_SHORT_FRAGMENT;
                p.frag = 1u; p.blocks = 1u; p.a = a; p.b = b; p.bytes = 0; pieces.push_back(p); o.encoded_blocks++;
            };
            if (lo != x.first[r0] || (r0 == r1 && hi != x.first[r0 + 1u])) { fragment(lo, hi < x.first[r0 + 1u] ? hi : x.first[r0 + 1u]); w0 = r0 + 1u; }
            const bool tail = r1 >= w0 && hi != x.first[r1 + 1u];
            if (tail) w1 = r1;
            if (w1 > w0) {
                p.frag = 0u; p.blocks = w1 - w0; p.a = x.off[w0]; p.b = x.off[w1 - 1u] + x.size[w1 - 1u] + 6u; p.bytes = p.b - p.a;
                pieces.push_back(p); o.copied_blocks += p.blocks;
            }
            if (tail) fragment(x.first[r1], hi);
        }
        if (why) {
            pieces.resize(o.piece0); o.copied_blocks = o.encoded_blocks = 0;
            o.result = SP_INVALID_ARGUMENT; o.why = why; continue;
        }
        o.total_samples = total; o.npieces = (uint32_t)pieces.size() - o.piece0;
    }
}

/* Step 3, once every fragment's `bytes` is known: offsets, sizes and the capacity verdicts of the outputs that are still OK.  An
 * output that does not fit keeps its size in `bytes` (the needed size). */
static inline void sp_place(SpOutput *outs, uint32_t nouts, SpPiece *pieces)
{
    for (uint32_t k = 0; k < nouts; k++) {
        SpOutput &o = outs[k];
        if (o.result != SP_OK) continue;
        uint64_t at = SP_HEADER_BYTES;
        for (uint32_t i = 0; i < o.npieces; i++) { SpPiece &p = pieces[o.piece0 + i]; p.dst = at; at += p.bytes; }
        o.bytes = at;
        if (at > o.capacity || at > 0xFFFFFFFFull) o.result = SP_INSUFFICIENT_BUFFER;
    }
}

/* The chunks of k_sp_copy for a run of n bytes to the address dst: a head of up to 15 bytes to the next 16-byte boundary of the
 * destination, `body` whole 16-byte units, a tail of up to 15 bytes; a chunk is SP_CHUNK_UNITS units (the first chunk moves the
 * head as well, the last the tail; a run without a whole unit is one chunk). */
static inline SP_HD void sp_run_parts(uint64_t dst, uint64_t n, uint64_t *head, uint64_t *body, uint64_t *tail)
{
    uint64_t h = (16u - (dst & 15u)) & 15u;
    if (h > n) h = n;
    *head = h; *body = (n - h) >> 4; *tail = (n - h) & 15u;
}
static inline SP_HD uint64_t sp_run_chunks(uint64_t dst, uint64_t n)
{
    uint64_t h, b, t;
    sp_run_parts(dst, n, &h, &b, &t);
    return b ? (b + SP_CHUNK_UNITS - 1u) / SP_CHUNK_UNITS : 1u;
}

#endif
