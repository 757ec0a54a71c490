/* lnn_windows_plan.h -- the host's planning for the windows calls (LINNEAmd_DecodeWindowsDevice and its siblings that compare, measure,
 * digest, find quiet runs, histogram, relate, mix, resample, overlay, slide and project; DESIGN.md section 5, "Many windows in one call"): from the windows' ranges and their streams' block indexes, the groups
 * by stream shape, the passes under group_frames, the block, window and bucket records the kernels of lnn_k_windows.h read, and the
 * sizes of the lists and of a pass's scratch.  Plain host C++ with no HIP call and no context in it, so a small stand-alone program
 * (tests/test_windows_plan_cpu.py) can drive it.  The records' structs are here because the plan fills them.
 *
 * A call plans in two steps.  wx_plan_count: which group every live window belongs to, which of its stream's blocks it overlaps, and
 * how many block records and COMPRESS entries the lists must have room for.  The caller sizes the lists from that (wx_lists) and
 * hands their memory to wx_plan_fill, which writes the records pass by pass:
 *   - the windows of one shape form a group; a group's windows are taken in the caller's order;
 *   - a pass holds at most group_frames COMPRESS blocks (0: no limit); a window's blocks are not split from the window before it
 *     unless they have to be;
 *   - a window with more COMPRESS blocks than a pass takes first has all of them in check-only passes of its own (its Rice codes are
 *     checked, nothing is placed), so that no sample of it is written before all that its fail word can say is known;
 *   - a window that reaches beyond the samples its stream's blocks hold gets a WX_TAIL record in front of its blocks;
 *   - a COMPRESS block's bytes get a slot of whole 16-byte groups in the pass's packed segment, at the source's address modulo 16.
 */
#ifndef LNN_WINDOWS_PLAN_H_INCLUDED
#define LNN_WINDOWS_PLAN_H_INCLUDED

#include <assert.h>
#include <stdint.h>
#include <string.h>
#include <map>
#include <tuple>
#include <vector>

#include "linne_amd.h"

#ifndef SX_COMPRESS                     /* (lnn_k_stream.h has the block types too) */
#define SX_COMPRESS 0u
#define SX_SILENT 1u
#define SX_RAW 2u
#endif
#define WX_TAIL 3u                      /* record type beside SX_COMPRESS / SX_SILENT / SX_RAW: a window's samples in [covered, hi) */
#define WX_NOFAIL 0xFFFFFFFFu
#define WX_MAXGROUPS 64
/* the bucketed consumers (lnn_k_buckets.h) */
#define WXB_SEGMENTS 4u                 /* up to this many buckets in a piece are reduced by the whole workgroup, one after the other */
#define WXB_MAXSLOTS 64u
#define WXB_THREADS 256u
/* the bitmask consumer (lnn_k_quiet.h): a bit per sample frame in 64-bit words; a commit workgroup takes a chunk of this many words */
#define WXQ_CHUNK_WORDS 256u

/* one block of one window (64 bytes) */
struct WxBlock {
    const uint8_t *b; uint64_t N;       /* the block's stream and its length */
    uint64_t off;                       /* the block's position in it */
    uint64_t first;                     /* its first sample */
    uint64_t dst;                       /* COMPRESS: where its first byte lies in the pass's packed segment; (dst & 15) == ((b + off) & 15) */
    uint32_t size, type, nsmp;          /* the size field, SX_* / WX_TAIL, samples */
    uint32_t win;                       /* its window's record */
    uint32_t cidx;                      /* index among the pass's COMPRESS blocks, or ~0 */
    uint32_t blk;                       /* its number in its stream */
};
/* one window (56 bytes) */
struct WxWindow {
    uint64_t lo, hi, covered;           /* the range [lo, hi); the samples the stream's blocks hold */
    void *out; uint64_t stride;         /* element (ch, i) at out + (ch * stride + i * sstride) elements of fmt */
    uint32_t fidx, fmt;                 /* its fail word (its saturation word lies W words behind it); LINNE_AMD_PCM_* */
    uint64_t sstride;                   /* (int32 planar: fmt S32, sstride 1) */
};
/* one window's buckets (64 bytes), at its WxWindow's index: what a bucketed consumer keeps per window.  A consumer leaves zero what it
 * does not use.  The bitmask consumer has no buckets but keeps the same record: min_run, capacity and threshold are its spec, abase the
 * window's first mask word and obase the number of commit chunks of the windows before it */
struct WxBucket {
    void *out;                          /* the caller's table */
    union { uint64_t b, min_run; };     /* bucket length (the window's length for "one bucket"); bitmask: the shortest run reported, >= 1 */
    union { uint64_t nb, capacity; };   /* buckets; bitmask: the records the caller's table has room for */
    uint64_t abase;                     /* its accumulators in the scratch, in the consumer's units */
    uint64_t obase;                     /* the number of output records of the windows before it */
    union { uint64_t cstride, n; };     /* per channel: the caller's channel stride; per frame and bitmask: the window's samples */
    union { uint32_t ns, threshold; };  /* slots (a power of two); bitmask: the largest quiet magnitude */
    uint32_t fidx;                      /* its fail word */
    union { uint32_t C, F; };           /* per channel: channels; per frame: bytes per sample frame */
    union { uint32_t sstride, hist, npair; };   /* per frame: units from one slot to the next (per channel: C * nb, not kept); per bin: the window's bins, shift and scale (WXH_SPEC); per pair: P = C (C + 1) / 2 */
};
static_assert(sizeof(WxBlock) == 64 && sizeof(WxBucket) == 64, "a block record and a bucket record are 64 bytes");
/* one window's channel matrix (160 bytes), at its WxWindow's index: what the mixing consumer (lnn_k_mix.h) keeps per window -- struct
 * LINNEAmdMixSpec with everything the host can work out worked out: the clip bounds -2^(B - 1) and 2^(B - 1) - 1, and the F32 format's
 * scale 2^-(Bf - 1) as the bits of a float.  Rows >= Co and columns >= C hold zeros, whatever the caller's spec holds there */
struct WxMix {
    uint32_t Co, shift;                 /* output channels 1 .. 8; the shift 0 .. 31 */
    int32_t lo, hi;                     /* the clip */
    uint32_t scale_bits;                /* the float 2^-(Bf - 1), Bf = clip_bits or, where that is 0, the stream's bits_per_sample */
    uint32_t fidx;                      /* its fail word */
    uint32_t reserved[2];
    int16_t coef[LINNE_MAX_NUM_CHANNELS][LINNE_MAX_NUM_CHANNELS];  /* [o][c] */
};
static_assert(sizeof(WxMix) == 160 && sizeof(WxMix) % 16 == 0, "a mix record is 160 bytes");

/* one window's resampling (128 bytes), at its WxWindow's index: what the resampling consumer (lnn_k_resample.h) keeps per window.  That
 * consumer's WxWindow names the window's INPUT range and, as its output, the window's int32 planar image in the accumulators; the
 * PCM the caller named is here */
struct WxResample {
    void *out; uint64_t stride, sstride;        /* the caller's PCM: element (ch, i) at out + (ch * stride + i * sstride) elements of fmt */
    uint64_t m_lo, m_hi;                /* the output samples [m_lo, m_hi) of the resampled stream */
    uint64_t n_first;                   /* n of output m_lo: word j of a channel of the image is stream sample n_first - before + j */
    uint64_t img, istride;              /* the image's first word among the accumulators; words from one channel to the next */
    uint64_t coef;                      /* its table's first word in the call's coefficient area */
    uint32_t up, down, taps, shift;
    int32_t lo, hi;                     /* the clip */
    uint32_t scale_bits;                /* the float 2^-(Bf - 1), as in WxMix */
    uint32_t fidx, fmt, C;              /* its fail word; LINNE_AMD_PCM_*; the stream's channels */
    uint32_t prow;                      /* 32-bit words of a phase's row in the table: (taps + 1) / 2, a pair of coefficients each */
    uint32_t reserved[3];
};
/* 256 outputs of one window: output m0 reads from stream sample n0 - before on, through phase p0 (m0 * down = n0 * up + p0) */
struct WxTile { uint32_t win, p0; uint64_t m0, n0; };
static_assert(sizeof(WxResample) == 128 && sizeof(WxTile) == 24, "a resample record is 128 bytes, a tile 24");
#define WXR_TILE 256u

/* ---- the overlaying consumer (lnn_k_overlay.h): its windows are the SOURCES of its outputs, in the caller's order, output by output ----
 * one source (48 bytes), at its window's number in the call (not at its WxWindow's): its image, the int32 planar target of the passes,
 * and where and under which gains it lies in its output */
struct WxOvSource {
    uint64_t img, istride;              /* the image's first word among the accumulators; words from one channel to the next: n rounded up to 4 */
    uint64_t at, n;                     /* it covers output samples [at, at + n) */
    int64_t gain, step;                 /* sample i of it under (gain + step * i) >> 32 */
};
/* one output that none of the host's checks failed (80 bytes); its tiles are WxTile with `win` its record here and m0 the tile's
 * first output sample (p0 and n0 are 0) */
struct WxOvOutput {
    void *out; uint64_t stride, sstride;        /* the caller's PCM: element (ch, t) at out + (ch * stride + t * sstride) elements of fmt */
    uint64_t n;                         /* its samples */
    uint32_t src0, nsrc;                /* its sources' records, and their fail words: [src0, src0 + nsrc); its saturation word is src0's */
    uint32_t C, shift;
    int32_t lo, hi;                     /* the clip */
    uint32_t scale_bits;                /* the float 2^-(Bf - 1), as in WxMix */
    uint32_t fmt;                       /* LINNE_AMD_PCM_* */
    uint32_t reserved[4];
};
static_assert(sizeof(WxOvSource) == 48 && sizeof(WxOvOutput) == 80, "an overlay source record is 48 bytes, an output record 80");
/* what the plan reads of one output: its sources are windows [w0, w0 + nsrc) of the call (the caller leaves out those behind one that its
 * checks refuse); checked: the output's own checks passed */
struct WxOvOut { uint32_t w0, nsrc; int checked; uint64_t n; void *out; uint64_t stride, sstride; uint32_t fmt, shift, clip_bits; };

/* ---- the lag consumer (lnn_k_lags.h): its windows are the needles and the clipped haystacks of its probes, in the caller's order ----
 * one window's image (32 bytes), at its window's number in the call: the int32 planar target of the passes, as an overlay source's */
struct WxLagImage {
    uint64_t img, istride;              /* the image's first word among the accumulators; words from one channel to the next: n rounded up to 4 */
    uint64_t lo, n;                     /* it holds stream samples [lo, lo + n) */
};
/* one probe that none of the host's checks failed (80 bytes) */
struct WxLagProbe {
    void *out; uint64_t pstride;        /* the caller's table: pair p, lag l at out[p * pstride + l] (struct LINNEAmdLagSum) */
    uint64_t *a_sq;                     /* the caller's [npair][2], or NULL */
    uint64_t n;                         /* the needle's samples */
    int64_t b0;                         /* word b0 + l + i of the haystack's image meets needle sample i at lag number l; <= 0, and words outside the image are 0 */
    uint32_t wa, wb;                    /* the needle's and the haystack's windows in the call: their images and fail words; wb WXL_NOWIN: the haystack is all zeros */
    uint32_t nlags, npair, nchunk, ntl; /* lags, pairs, chunks of WXL_CHUNK needle samples, tiles of WXL_LAGS lags */
    uint8_t ca[LINNE_MAX_NUM_CHANNELS], cb[LINNE_MAX_NUM_CHANNELS];
};
/* a tile: WXL_LAGS lags from l0 on of one pair of one probe, over chunk `chunk` of the needle; the chunks of one (probe, pair, l0) follow
 * each other in the list, and the commit's list names the first of each such run */
struct WxLagTile { uint32_t probe, pair, l0, chunk; };
static_assert(sizeof(WxLagImage) == 32 && sizeof(WxLagProbe) == 80 && sizeof(WxLagTile) == 16, "a lag image is 32 bytes, a probe record 80, a tile 16");
#define WXL_LAGS 256u
#define WXL_CHUNK 65536u
#define WXL_NOWIN 0xFFFFFFFFu
/* the most tiles of outputs or of lags one call takes: every tile is a workgroup of 256 threads of one launch, and a launch of 2^32
 * threads or more is not refused -- the count wraps and the tiles behind the wrap are never visited */
#define WX_MAX_TILES 0xFFFFFFull
static_assert(WXL_LAGS == 256u && WXR_TILE == 256u && (WX_MAX_TILES + 1u) * 256u == (1ull << 32), "WX_MAX_TILES workgroups of a tile's threads stay below 2^32 threads");
/* a tile's partial sums among the accumulators, in 64-bit words: (lo, hi) of the dot per lag, then the chunk's sum of b^2 at the tile's
 * first lag and its sum of a^2, (lo, hi) each */
#define WXL_PART_WORDS (2u * WXL_LAGS + 4u)
/* what the plan reads of one probe: checked: its own checks and its windows' host checks passed; its needle is window wa of the call, its
 * clipped haystack window wb (WXL_NOWIN: the range misses the stream) */
struct WxLagIn {
    int checked; uint32_t wa, wb; uint64_t n; int64_t b0; uint32_t nlags, npair;
    void *out; uint64_t pstride; uint64_t *a_sq; uint8_t ca[LINNE_MAX_NUM_CHANNELS], cb[LINNE_MAX_NUM_CHANNELS];
};

/* ---- the projecting consumer (lnn_k_project.h): its WxWindow names the window's INPUT range and, as its output, the window's int32
 * planar image in the accumulators, as a resampled window's does; the table the caller named is here (144 bytes) */
struct WxProject {
    void *out; uint64_t cstride, fstride, rstride;      /* the caller's table: element (c, f, k) at out + c * cstride + (f - f_lo) * fstride + k * rstride elements */
    uint64_t f_lo, nframes;             /* the frames [f_lo, f_lo + nframes) of the stream */
    uint64_t img, istride;              /* the image's first word among the accumulators; words from one channel to the next; word j of a channel is stream sample f_lo * H - before + j */
    uint64_t planes;                    /* its basis' digit planes: their first byte in the call's plane area (behind the images) */
    uint64_t raw;                       /* its basis as the caller gave it: its first int16 in the lists' table area */
    uint64_t rsum;                      /* its rows' sums: their first word in the lists' sums area */
    uint32_t N, H, K, Npad, Kpad, shift;        /* Npad: N rounded up to 64; Kpad: K rounded up to 16 */
    int32_t lo, hi;                     /* the clip */
    uint32_t fmt, scale_bits;           /* LINNE_AMD_PCM_S32 / _F32; the float 2^-float_exp */
    uint32_t fidx, C;                   /* its fail word; the stream's channels */
    uint32_t reserved[2];
};
/* one basis of the call (32 bytes): K rows of N int16 at `raw`, to become two planes of Kpad rows of Npad bytes at `planes` */
struct WxProjTable { uint64_t raw, planes; uint32_t K, N, Kpad, Npad; };
/* WXP_FRAMES frames from f0 on (counted from the window's first) by WXP_ROWS rows from k0 on, of channel ch of one window */
struct WxProjTile { uint64_t f0; uint32_t win, ch, k0, reserved; };
static_assert(sizeof(WxProject) == 144 && sizeof(WxProjTable) == 32 && sizeof(WxProjTile) == 24, "a project record is 144 bytes, a table record 32, a tile 24");
#define WXP_FRAMES 64u
#define WXP_ROWS 64u
/* where wx_plan_fill writes the projecting consumer's lists */
struct WxProjLists { WxProject *rec; WxProjTile *tile; WxProjTable *tab; int32_t *rsum; int16_t *raw; };

/* the histogram's spec in one word: num_bins (1 .. 1024) | shift (0 .. 31) << 16 | scale (0 linear, 1 log2) << 24 */
#define WXH_SPEC(bins, shift, scale) ((uint32_t)(bins) | (uint32_t)(shift) << 16 | (uint32_t)(scale) << 24)
#define WXH_BINS(h) ((h) & 0xFFFFu)
#define WXH_SHIFT(h) (((h) >> 16) & 31u)
#define WXH_LOG2(h) (((h) >> 24) & 1u)

/* how a consumer keeps buckets: not at all; an accumulator per (channel, bucket), a window's slots C * nb apart (measure); one per
 * bucket, a window's slots padded to whole 64-byte lines of 16 units (digest); a bit per sample frame, in whole 64-bit words per window
 * (quiet: the units are those words, and the "output records" counted in obase and nout are the commit's chunks of WXQ_CHUNK_WORDS
 * words, of which every window has whole ones); a 32-bit counter per (channel, bucket, bin), laid out as per channel with the window's
 * num_bins units where that has one -- bin j of channel ch, bucket k, slot s at abase + ((s * C + ch) * nb + k) * num_bins + j -- and
 * an "output record" per bin, C * nb * num_bins of them: the commit has a lane per bin it stores (histogram); an accumulator per
 * (channel pair i <= j, bucket), laid out as per channel with the P = C (C + 1) / 2 pairs (LINNE_AMD_PAIR) where that has the
 * channels -- pair p, bucket k, slot s at abase + (s * P + p) * nb + k, a window's slots P * nb apart -- P * nb output records, and
 * cstride the caller's pair stride (relate) */
enum WxBucketing { WX_NO_BUCKETS = 0, WX_BUCKETS_PER_CHANNEL = 1, WX_BUCKETS_PER_FRAME = 2, WX_BITMASK = 3, WX_BUCKETS_PER_BIN = 4, WX_BUCKETS_PER_PAIR = 5 };

/* what the plan reads of a block index */
struct WxIndexView {
    struct LINNEAmdShape shape;
    uint32_t nb; uint64_t covered, stream_bytes;
    const uint64_t *h_off, *h_first; const uint32_t *h_size, *h_type, *h_nsmp;
};
/* one window of the call */
struct WxRange {
    WxIndexView x; const uint8_t *stream;       /* (the address is used modulo 16, nothing is read) */
    int live;                           /* it passed its checks and has samples: the fields below are set */
    uint64_t lo, n, r1;                 /* [lo, lo + n); the last block it overlaps (nb: it reaches behind the last block) */
    void *out; uint64_t stride, sstride; uint32_t fmt;          /* its WxWindow's */
    uint64_t bucket_samples, bucket_cstride; void *bucket_out;  /* bucketed consumers: its spec */
    uint64_t quiet_min, quiet_capacity; uint32_t quiet_threshold;       /* the bitmask consumer: its spec beside bucket_out (quiet_min >= 1) */
    uint32_t hist;                      /* the per-bin consumer: WXH_SPEC beside bucket_samples, bucket_cstride and bucket_out */
    const struct LINNEAmdMixSpec *mix;  /* the mixing consumer: its spec, checked (out_channels 1 .. 8, shift <= 31, clip_bits 0 or 2 .. 32) */
    const struct LINNEAmdResampleSpec *rs;      /* the resampling consumer: its spec, checked; [lo, lo + n) above is the window's INPUT range */
    uint64_t m_lo, m_n;                 /* ... and these its output samples, of the resampled stream */
    const struct LINNEAmdOverlaySource *ov;     /* the overlaying consumer: the source this window is, checked */
    const struct LINNEAmdProjectSpec *pj;       /* the projecting consumer: its spec, checked; [lo, lo + n) is the window's INPUT range, m_lo and m_n its frames */
};
struct WxPlan { uint32_t r0, nr, ncomp; int32_t group; };               /* a window's blocks [r0, r0 + nr), the COMPRESS ones among them; group -1: it takes no pass */
struct WxPass { uint32_t group, rec0, nrec, c0, nc; uint64_t seg_bytes; int check_only; };
struct WxPlanned {
    std::vector<WxPlan> win;            /* [W] */
    uint32_t ngroups, gwin[WX_MAXGROUPS];       /* a window of every group: its stream has the group's shape */
    uint64_t nlive, total_rec, total_crec;      /* what the lists are reserved for (wx_plan_count) */
    std::vector<WxPass> passes;
    uint32_t nwin, nrec, ncrec;         /* records written (wx_plan_fill): nwin == nlive, nrec <= total_rec, ncrec <= total_crec */
    uint64_t scratch_bytes;             /* the largest pass's */
    uint64_t nacc, nout;                /* bucketed consumers: accumulator units, output records */
    uint64_t nmask;                     /* the bitmask consumer: the mask words among nacc; behind them the commit's units per chunk (wxq_chunk_units) */
    /* the resampling consumer (wx_resample_count): every window's table in the coefficient area (windows of one (coef, up, taps) share
     * one), the area's words, the tiles of all live windows; ntile: the tiles written */
    std::vector<uint64_t> rs_coef; std::vector<uint8_t> rs_owner; uint64_t rs_words, rs_tiles, ntile;
    uint64_t ov_outs, nov;              /* the overlaying consumer (wx_overlay_count): the outputs that get tiles (counted in rs_tiles); nov: their records written */
    /* the lag consumer (wx_lag_count): the probes that get tiles (counted in rs_tiles) and the runs of tiles the commit takes; nlg and
     * nlgrun: those written; lg_part: the partial sums' first word among the accumulators (wx_lag_fill) */
    uint64_t lg_probes, lg_runs, nlg, nlgrun, lg_part;
    /* the projecting consumer (wx_project_count): every window's table among the call's (windows of one (basis, K, N) share one), the
     * tables' records, int16 elements, row sums and plane bytes the lists and the scratch must have room for (the tiles are counted in
     * rs_tiles); pj_plane0: the planes' first word among the accumulators (wx_plan_fill) */
    std::vector<uint32_t> pj_tab; std::vector<uint8_t> pj_owner; std::vector<WxProjTable> pj_tabs;
    uint64_t pj_raw, pj_rsum, pj_plane_bytes, pj_plane0;
};
enum { WXP_OK = 0, WXP_SHAPES = 1, WXP_BLOCKS = 2 };    /* wx_plan_count: more than WX_MAXGROUPS shapes; total_rec blocks are too many */

static inline uint64_t wx_align(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }
/* the block holding sample s (s < covered): the last r < nb with first[r] <= s */
static inline uint64_t wx_block_of(const uint64_t *first, uint64_t nb, uint64_t s)
{
    uint64_t lo = 0, hi = nb;
    while (hi - lo > 1u) { const uint64_t mid = lo + ((hi - lo) >> 1); if (first[mid] <= s) lo = mid; else hi = mid; }
    return lo;
}
/* the buckets of a window of n samples (0 for none) */
static inline uint64_t wx_buckets(uint64_t n, uint64_t b) { return n == 0 ? 0u : (b == 0 || b >= n) ? 1u : n / b + (n % b != 0); }
/* A bucket of L samples takes L / 256 pieces, each one atomic per accumulator: from 8192 samples on they are spread over L / 4096
 * slots, WXB_MAXSLOTS at most */
static inline uint32_t wx_slots(uint64_t b) { uint32_t ns = 1u; while (ns < WXB_MAXSLOTS && (b >> 12) >= 2u * ns) ns *= 2u; return ns; }

/* the 64-bit words of a window's mask, and the chunks the commit cuts them into */
static inline uint64_t wxq_words(uint64_t n) { return (n >> 6) + ((n & 63u) != 0); }
static inline uint64_t wxq_chunks(uint64_t n) { return (wxq_words(n) + WXQ_CHUNK_WORDS - 1u) / WXQ_CHUNK_WORDS; }
/* what the commit keeps for nchunks chunks, in 64-bit units behind the masks: the prefix sums of the chunks' counts of run starts and of
 * run ends (2 * nchunks + 1 words), then the counts themselves (2 * nchunks 32-bit words) */
static inline uint64_t wxq_chunk_units(uint64_t nchunks) { return 3u * nchunks + 1u; }

/* the buffers of one pass in the context's scratch */
struct WxScratch { uint64_t o_nsmp, o_bpos, o_bend, o_eb, o_prm, o_data, o_seg, bytes; };
static inline WxScratch wx_scratch(uint32_t nc, uint32_t C, uint32_t S, uint64_t seg_bytes)
{
    WxScratch s; uint64_t at = 0;
    s.o_nsmp = at; at = wx_align(at + sizeof(uint32_t) * (nc + 1u));
    s.o_bpos = at; at = wx_align(at + sizeof(uint64_t) * (nc + 1u));
    s.o_bend = at; at = wx_align(at + sizeof(uint64_t) * (nc + 1u));
    s.o_eb = at; at = wx_align(at + sizeof(uint64_t) * (nc + 1u));
    s.o_prm = at; at = wx_align(at + sizeof(int32_t) * LINNE_AMD_PARAM_WORDS * C * (uint64_t)nc);
    s.o_data = at; at = wx_align(at + sizeof(int32_t) * (uint64_t)C * S * nc);
    s.o_seg = at; at = wx_align(at + seg_bytes + 16u);
    s.bytes = at;
    return s;
}

/* the lists, in pinned memory and at the same offsets on the device: the words that come back (fail words, saturation words and
 * back_words 32-bit words per window of the consumer's own) | window records | the consumer's per-window records | block records |
 * the passes' COMPRESS records */
struct WxLists { uint64_t o_fail, o_back, back_bytes, o_win, o_side, o_rec, o_crec, bytes, o_tile, o_coef, o_ovout, o_ovsrc, o_lgrun, o_lgprobe, o_lgimg, o_pjtab, o_pjrsum, o_pjraw; };
static inline WxLists wx_lists(const WxPlanned &p, uint64_t W, uint64_t back_words, uint64_t side_bytes, bool resamples = false, bool overlays = false, bool lags = false, bool projects = false)
{
    WxLists l;
    l.o_fail = 0; l.o_back = 2u * sizeof(uint32_t) * W; l.back_bytes = l.o_back + sizeof(uint32_t) * back_words * W;
    l.o_win = wx_align(l.back_bytes);
    l.o_side = wx_align(l.o_win + sizeof(WxWindow) * p.nlive);
    l.o_rec = wx_align(l.o_side + side_bytes * p.nlive);
    l.o_crec = wx_align(l.o_rec + sizeof(WxBlock) * p.total_rec);
    l.bytes = wx_align(l.o_crec + sizeof(uint32_t) * (p.total_crec + 1u));
    l.o_tile = l.o_coef = l.bytes;
    if (resamples) {                    /* behind everything the other consumers have: the tiles | the coefficient tables */
        l.o_coef = wx_align(l.o_tile + sizeof(WxTile) * p.rs_tiles);
        l.bytes = wx_align(l.o_coef + sizeof(uint32_t) * p.rs_words);
    }
    l.o_ovout = l.o_ovsrc = l.bytes;
    if (overlays) {                     /* likewise: the tiles | the output records | a source record per window of the call */
        l.o_ovout = wx_align(l.o_tile + sizeof(WxTile) * p.rs_tiles);
        l.o_ovsrc = wx_align(l.o_ovout + sizeof(WxOvOutput) * p.ov_outs);
        l.bytes = wx_align(l.o_ovsrc + sizeof(WxOvSource) * W);
    }
    l.o_lgrun = l.o_lgprobe = l.o_lgimg = l.bytes;
    if (lags) {                         /* likewise: the tiles | the commit's runs | the probe records | an image record per window of the call */
        l.o_lgrun = wx_align(l.o_tile + sizeof(WxLagTile) * p.rs_tiles);
        l.o_lgprobe = wx_align(l.o_lgrun + sizeof(uint32_t) * p.lg_runs);
        l.o_lgimg = wx_align(l.o_lgprobe + sizeof(WxLagProbe) * p.lg_probes);
        l.bytes = wx_align(l.o_lgimg + sizeof(WxLagImage) * W);
    }
    l.o_pjtab = l.o_pjrsum = l.o_pjraw = l.bytes;
    if (projects) {                     /* likewise: the tiles | the table records | the rows' sums | the tables as the caller gave them */
        l.o_pjtab = wx_align(l.o_tile + sizeof(WxProjTile) * p.rs_tiles);
        l.o_pjrsum = wx_align(l.o_pjtab + sizeof(WxProjTable) * p.pj_tabs.size());
        l.o_pjraw = wx_align(l.o_pjrsum + sizeof(int32_t) * p.pj_rsum);
        l.bytes = wx_align(l.o_pjraw + sizeof(int16_t) * p.pj_raw);
    }
    return l;
}

/* step 1: the live windows get their blocks and the group of their shape */
static inline int wx_plan_count(const WxRange *rg, uint32_t W, uint32_t group_frames, WxPlanned &p)
{
    p.win.resize(W);
    p.ngroups = 0; p.nlive = p.total_rec = p.total_crec = 0;
    p.passes.clear(); p.nwin = p.nrec = p.ncrec = 0; p.scratch_bytes = p.nacc = p.nout = p.nmask = 0;
    p.rs_coef.clear(); p.rs_owner.clear(); p.rs_words = p.rs_tiles = p.ntile = 0; p.ov_outs = p.nov = 0;
    p.lg_probes = p.lg_runs = p.nlg = p.nlgrun = p.lg_part = 0;
    p.pj_tab.clear(); p.pj_owner.clear(); p.pj_tabs.clear(); p.pj_raw = p.pj_rsum = p.pj_plane_bytes = p.pj_plane0 = 0;
    for (uint32_t i = 0; i < W; i++) {
        WxPlan &pl = p.win[i];
        pl.group = -1; pl.r0 = pl.nr = pl.ncomp = 0;
        if (!rg[i].live) continue;
        const WxIndexView &x = rg[i].x;
        const uint64_t lo = rg[i].lo, r1 = rg[i].r1;
        const uint64_t r0 = (lo < x.covered) ? wx_block_of(x.h_first, x.nb, lo) : x.nb;
        const uint64_t nr = (r0 < x.nb) ? ((r1 < x.nb ? r1 : x.nb - 1u) - r0 + 1u) : 0u;
        uint32_t nc = 0;
        for (uint64_t y = 0; y < nr; y++) nc += (x.h_type[r0 + y] == SX_COMPRESS);
        uint32_t g = 0;
        while (g < p.ngroups && memcmp(&rg[p.gwin[g]].x.shape, &x.shape, sizeof(x.shape)) != 0) g++;
        if (g == p.ngroups) {
            if (p.ngroups == WX_MAXGROUPS) return WXP_SHAPES;
            p.gwin[p.ngroups++] = i;
        }
        pl.r0 = (uint32_t)r0; pl.nr = (uint32_t)nr; pl.ncomp = nc; pl.group = (int32_t)g;
        const bool big = group_frames && nc > group_frames;
        p.nlive++; p.total_rec += nr + 1u + (big ? nc : 0u); p.total_crec += (uint64_t)nc * (big ? 2u : 1u);
    }
    return (p.nlive && p.total_rec >= 0x7FFFFFFFull) ? WXP_BLOCKS : WXP_OK;
}

/* a window's mix record from its spec and its stream's shape */
static inline void wx_mix_record(const struct LINNEAmdMixSpec &s, const struct LINNEAmdShape &shape, uint32_t fidx, WxMix &m)
{
    const uint32_t B = s.clip_bits ? s.clip_bits : 32u, Bf = s.clip_bits ? s.clip_bits : shape.bits_per_sample;
    memset(&m, 0, sizeof(m));
    m.Co = s.out_channels; m.shift = s.shift; m.fidx = fidx;
    m.hi = (int32_t)(((uint64_t)1 << (B - 1u)) - 1u); m.lo = -m.hi - 1;
    m.scale_bits = (128u - Bf) << 23;   /* 2^-(Bf - 1): exponent field 127 - (Bf - 1), Bf <= 32 */
    for (uint32_t o = 0; o < s.out_channels && o < LINNE_MAX_NUM_CHANNELS; o++)
        for (uint32_t c = 0; c < shape.num_channels && c < LINNE_MAX_NUM_CHANNELS; c++) m.coef[o][c] = s.coef[o][c];
}

/* ---- the resampling consumer ---- */
static inline uint64_t wxr_length(uint64_t N, uint32_t L, uint32_t M)
{
    if (M == 0) return 0;
    const unsigned __int128 q = ((unsigned __int128)N * L + (M - 1u)) / M;
    return q > (unsigned __int128)~(uint64_t)0 ? ~(uint64_t)0 : (uint64_t)q;
}
/* what outputs [first, first + n), n >= 1, of a stream of N samples read: n(first), and the input range [lo, hi) inside the stream */
struct WxrInput { uint64_t n_first, n_last, lo, hi, istride; };
static inline WxrInput wxr_input(uint64_t first, uint64_t n, const struct LINNEAmdResampleSpec &s, uint64_t N)
{
    WxrInput r;
    r.n_first = (uint64_t)((unsigned __int128)first * s.down / s.up);
    r.n_last = (uint64_t)((unsigned __int128)(first + n - 1u) * s.down / s.up);
    r.lo = r.n_first > s.before ? r.n_first - s.before : 0u;
    r.hi = r.n_last + s.taps - s.before;                    /* (before <= taps - 1: at least n_last + 1) */
    if (r.hi > N) r.hi = N;
    r.istride = (r.n_last - r.n_first + s.taps + 3u) & ~(uint64_t)3u;
    return r;
}
/* between wx_plan_count and wx_lists: the tables and the tiles the lists must have room for */
static inline void wx_resample_count(const WxRange *rg, uint32_t W, WxPlanned &p)
{
    std::map<std::tuple<const int16_t *, uint32_t, uint32_t>, uint64_t> seen;
    p.rs_coef.assign(W, 0u); p.rs_owner.assign(W, 0u);
    for (uint32_t i = 0; i < W; i++) {
        if (p.win[i].group < 0) continue;
        const struct LINNEAmdResampleSpec &s = *rg[i].rs;
        p.rs_tiles += (rg[i].m_n + WXR_TILE - 1u) / WXR_TILE;
        const auto at = seen.emplace(std::make_tuple(s.coef, s.up, s.taps), p.rs_words);
        if (at.second) { p.rs_owner[i] = 1u; p.rs_words += (uint64_t)s.up * ((s.taps + 1u) / 2u); }
        p.rs_coef[i] = at.first->second;
    }
}
/* a window's resample record, its tiles and (where it is the first to name it) its table; the window record names the image */
static inline void wx_resample_record(const WxRange &w, const struct LINNEAmdShape &shape, uint32_t i, uint32_t wi, WxPlanned &p,
        WxWindow &ww, WxResample &m, WxTile *h_tile, uint32_t *h_coef)
{
    const struct LINNEAmdResampleSpec &s = *w.rs;
    const uint32_t B = s.clip_bits ? s.clip_bits : 32u, Bf = s.clip_bits ? s.clip_bits : shape.bits_per_sample;
    const uint64_t n_first = (uint64_t)((unsigned __int128)w.m_lo * s.down / s.up);
    const uint64_t n_last = (uint64_t)((unsigned __int128)(w.m_lo + w.m_n - 1u) * s.down / s.up);
    memset(&m, 0, sizeof(m));
    m.out = w.out; m.stride = w.stride; m.sstride = w.sstride; m.fmt = w.fmt;
    m.m_lo = w.m_lo; m.m_hi = w.m_lo + w.m_n; m.n_first = n_first;
    m.img = p.nacc; m.istride = (n_last - n_first + s.taps + 3u) & ~(uint64_t)3u;
    m.coef = p.rs_coef[i]; m.up = s.up; m.down = s.down; m.taps = s.taps; m.shift = s.shift; m.prow = (s.taps + 1u) / 2u;
    m.hi = (int32_t)(((uint64_t)1 << (B - 1u)) - 1u); m.lo = -m.hi - 1;
    m.scale_bits = (128u - Bf) << 23;
    m.fidx = i; m.C = shape.num_channels;
    p.nacc += m.istride * shape.num_channels;
    /* the passes place the input range into the image: the window record's output is the image, as an offset in bytes from the
     * accumulators' first byte (the caller of the plan adds their address) */
    ww.out = (void *)(uintptr_t)(sizeof(int32_t) * (m.img + (w.lo + s.before - n_first)));
    ww.fmt = LINNE_AMD_PCM_S32; ww.stride = m.istride; ww.sstride = 1u;
    for (uint64_t m0 = m.m_lo; m0 < m.m_hi; m0 += WXR_TILE) {
        assert(p.ntile < p.rs_tiles);
        WxTile &t = h_tile[p.ntile++];
        const unsigned __int128 at = (unsigned __int128)m0 * s.down;
        t.win = wi; t.m0 = m0; t.n0 = (uint64_t)(at / s.up); t.p0 = (uint32_t)(at % s.up);
    }
    if (p.rs_owner[i]) for (uint32_t ph = 0; ph < s.up; ph++)
        for (uint32_t k = 0; k < m.prow; k++) {
            const uint32_t a = (uint16_t)s.coef[(uint64_t)ph * s.taps + 2u * k], b = (2u * k + 1u < s.taps) ? (uint16_t)s.coef[(uint64_t)ph * s.taps + 2u * k + 1u] : 0u;
            h_coef[m.coef + (uint64_t)ph * m.prow + k] = a | b << 16;
        }
}

/* ---- the overlaying consumer ---- */
/* an output gets tiles when its own checks passed and every source of it is a live window of the plan */
static inline bool wx_overlay_live(const WxOvOut &o, const WxPlanned &p)
{
    if (!o.checked) return false;
    for (uint32_t j = 0; j < o.nsrc; j++) if (p.win[o.w0 + j].group < 0) return false;
    return true;
}
/* between wx_plan_count and wx_lists: the outputs and the tiles the lists must have room for */
static inline void wx_overlay_count(const WxOvOut *outs, uint32_t O, WxPlanned &p)
{
    for (uint32_t k = 0; k < O; k++) if (wx_overlay_live(outs[k], p)) { p.ov_outs++; p.rs_tiles += (outs[k].n + WXR_TILE - 1u) / WXR_TILE; }
}
/* a source's record (at its window's number i in the call); the window record names the image, as a resampled window's does */
static inline void wx_overlay_source(const WxRange &w, const struct LINNEAmdShape &shape, WxPlanned &p, WxWindow &ww, WxOvSource &m)
{
    m.img = p.nacc; m.istride = (w.n + 3u) & ~(uint64_t)3u;
    m.at = w.ov->at; m.n = w.n; m.gain = w.ov->gain_q32; m.step = w.ov->step_q32;
    p.nacc += m.istride * shape.num_channels;
    ww.out = (void *)(uintptr_t)(sizeof(int32_t) * m.img);
    ww.fmt = LINNE_AMD_PCM_S32; ww.stride = m.istride; ww.sstride = 1u;
}
/* behind wx_plan_fill: the records and the tiles of the outputs that get them, in the caller's order */
static inline void wx_overlay_fill(const WxOvOut *outs, uint32_t O, const WxRange *rg, WxPlanned &p, WxOvOutput *h_out, WxTile *h_tile)
{
    for (uint32_t k = 0; k < O; k++) {
        const WxOvOut &o = outs[k];
        if (!wx_overlay_live(o, p)) continue;
        assert(p.nov < p.ov_outs);
        const uint32_t oi = (uint32_t)p.nov++;
        const struct LINNEAmdShape &shape = rg[o.w0].x.shape;
        const uint32_t B = o.clip_bits ? o.clip_bits : 32u, Bf = o.clip_bits ? o.clip_bits : shape.bits_per_sample;
        WxOvOutput &m = h_out[oi];
        memset(&m, 0, sizeof(m));
        m.out = o.out; m.stride = o.stride; m.sstride = o.sstride; m.fmt = o.fmt; m.n = o.n;
        m.src0 = o.w0; m.nsrc = o.nsrc; m.C = shape.num_channels; m.shift = o.shift;
        m.hi = (int32_t)(((uint64_t)1 << (B - 1u)) - 1u); m.lo = -m.hi - 1;
        m.scale_bits = (128u - Bf) << 23;
        for (uint64_t t0 = 0; t0 < o.n; t0 += WXR_TILE) {
            assert(p.ntile < p.rs_tiles);
            WxTile &t = h_tile[p.ntile++];
            t.win = oi; t.p0 = 0u; t.m0 = t0; t.n0 = 0u;
        }
    }
}

/* ---- the lag consumer ---- */
/* a probe gets tiles when its checks passed and its windows are live windows of the plan */
static inline bool wx_lag_live(const WxLagIn &q, const WxPlanned &p)
{
    return q.checked && p.win[q.wa].group >= 0 && (q.wb == WXL_NOWIN || p.win[q.wb].group >= 0);
}
static inline uint64_t wxl_lag_tiles(uint32_t nlags) { return ((uint64_t)nlags + WXL_LAGS - 1u) / WXL_LAGS; }
static inline uint64_t wxl_chunks(uint64_t n) { return (n + WXL_CHUNK - 1u) / WXL_CHUNK; }
/* between wx_plan_count and wx_lists: the probes, the runs and the tiles the lists must have room for */
static inline void wx_lag_count(const WxLagIn *in, uint32_t Q, WxPlanned &p)
{
    for (uint32_t k = 0; k < Q; k++) if (wx_lag_live(in[k], p)) {
        const uint64_t runs = in[k].npair * wxl_lag_tiles(in[k].nlags);
        p.lg_probes++; p.lg_runs += runs; p.rs_tiles += runs * wxl_chunks(in[k].n);
    }
}
/* a window's image (at its window's number i in the call); the window record names the image, as an overlay source's does */
static inline void wx_lag_image(const WxRange &w, const struct LINNEAmdShape &shape, WxPlanned &p, WxWindow &ww, WxLagImage &m)
{
    m.img = p.nacc; m.istride = (w.n + 3u) & ~(uint64_t)3u; m.lo = w.lo; m.n = w.n;
    p.nacc += m.istride * shape.num_channels;
    ww.out = (void *)(uintptr_t)(sizeof(int32_t) * m.img);
    ww.fmt = LINNE_AMD_PCM_S32; ww.stride = m.istride; ww.sstride = 1u;
}
/* behind wx_plan_fill: the records, the tiles and the runs of the probes that get them, in the caller's order; the partial sums lie
 * behind the images, WXL_PART_WORDS 64-bit words per tile */
static inline void wx_lag_fill(const WxLagIn *in, uint32_t Q, WxPlanned &p, WxLagProbe *h_probe, WxLagTile *h_tile, uint32_t *h_run)
{
    for (uint32_t k = 0; k < Q; k++) {
        const WxLagIn &q = in[k];
        if (!wx_lag_live(q, p)) continue;
        assert(p.nlg < p.lg_probes);
        const uint32_t pi = (uint32_t)p.nlg++;
        WxLagProbe &m = h_probe[pi];
        memset(&m, 0, sizeof(m));
        m.out = q.out; m.pstride = q.pstride; m.a_sq = q.a_sq; m.n = q.n; m.b0 = q.b0; m.wa = q.wa; m.wb = q.wb;
        m.nlags = q.nlags; m.npair = q.npair; m.nchunk = (uint32_t)wxl_chunks(q.n); m.ntl = (uint32_t)wxl_lag_tiles(q.nlags);
        memcpy(m.ca, q.ca, sizeof(m.ca)); memcpy(m.cb, q.cb, sizeof(m.cb));
        for (uint32_t pr = 0; pr < m.npair; pr++)
            for (uint32_t lt = 0; lt < m.ntl; lt++) {
                assert(p.nlgrun < p.lg_runs);
                h_run[p.nlgrun++] = (uint32_t)p.ntile;
                for (uint32_t c = 0; c < m.nchunk; c++) {
                    assert(p.ntile < p.rs_tiles);
                    WxLagTile &t = h_tile[p.ntile++];
                    t.probe = pi; t.pair = pr; t.l0 = lt * WXL_LAGS; t.chunk = c;
                }
            }
    }
    p.lg_part = (p.nacc + 3u) & ~(uint64_t)3u;  /* (in the images' 32-bit words: 16-byte aligned) */
    p.nacc = p.lg_part + 2u * WXL_PART_WORDS * p.ntile;
}

/* ---- the projecting consumer ---- */
static inline uint64_t wxp_length(uint64_t N, uint32_t H) { return H == 0 ? 0u : N / H + (N % H != 0); }
/* frames * K * N * C of one window stays inside LINNE_AMD_PROJECT_MAX_PRODUCTS: formed in 128 bits */
static inline bool wxp_products_fit(uint64_t frames, uint32_t K, uint32_t N, uint32_t C)
{
    return (unsigned __int128)frames * K * N * C <= (unsigned __int128)LINNE_AMD_PROJECT_MAX_PRODUCTS;
}
/* the output map (c, f, k) -> c * cs + f * fs + k * rs is injective by the header's rule: the three (stride, extent) pairs sorted by
 * stride, pairs of extent 1 (or 0) left out, the smallest stride at least 1 and each later one at least the one before it times that
 * one's extent */
static inline bool wxp_injective(uint64_t cs, uint64_t C, uint64_t fs, uint64_t frames, uint64_t rs, uint64_t K)
{
    uint64_t st[3] = { cs, fs, rs }, ex[3] = { C, frames, K };
    for (int a = 0; a < 3; a++) for (int b = a + 1; b < 3; b++) if (st[b] < st[a]) { const uint64_t s = st[a], e = ex[a]; st[a] = st[b]; ex[a] = ex[b]; st[b] = s; ex[b] = e; }
    bool first = true; uint64_t ps = 0, pe = 0;
    for (int a = 0; a < 3; a++) {
        if (ex[a] <= 1u) continue;
        if (first ? st[a] < 1u : (unsigned __int128)st[a] < (unsigned __int128)ps * pe) return false;
        first = false; ps = st[a]; pe = ex[a];
    }
    return true;
}
/* what frames [first, first + n), n >= 1 and (first + n - 1) * H < N_s, of a stream of N_s samples read: the input range [lo, hi) inside
 * the stream (hi > lo), and the words of a channel of the image, which holds the halos off either end too */
struct WxpInput { uint64_t lo, hi, istride; };
static inline WxpInput wxp_input(uint64_t first, uint64_t n, const struct LINNEAmdProjectSpec &s, uint64_t N_s)
{
    WxpInput r;
    const uint64_t at = first * s.hop;                      /* (< N_s) */
    r.lo = at > s.before ? at - s.before : 0u;
    const unsigned __int128 hi = (unsigned __int128)(first + n - 1u) * s.hop + s.frame_len - s.before;
    r.hi = hi > N_s ? N_s : (uint64_t)hi;
    r.istride = ((n - 1u) * s.hop + s.frame_len + 3u) & ~(uint64_t)3u;
    return r;
}
/* between wx_plan_count and wx_lists: the tables and the tiles the lists must have room for */
static inline void wx_project_count(const WxRange *rg, uint32_t W, WxPlanned &p)
{
    std::map<std::tuple<const int16_t *, uint32_t, uint32_t>, uint32_t> seen;
    p.pj_tab.assign(W, 0u); p.pj_owner.assign(W, 0u);
    for (uint32_t i = 0; i < W; i++) {
        if (p.win[i].group < 0) continue;
        const struct LINNEAmdProjectSpec &s = *rg[i].pj;
        p.rs_tiles += rg[i].x.shape.num_channels * ((rg[i].m_n + WXP_FRAMES - 1u) / WXP_FRAMES) * ((s.num_rows + WXP_ROWS - 1u) / WXP_ROWS);
        const auto at = seen.emplace(std::make_tuple(s.basis, s.num_rows, s.frame_len), (uint32_t)p.pj_tabs.size());
        if (at.second) {
            WxProjTable t;
            t.K = s.num_rows; t.N = s.frame_len; t.Kpad = (t.K + 15u) & ~15u; t.Npad = (t.N + 63u) & ~63u;
            t.raw = p.pj_raw; t.planes = p.pj_plane_bytes;
            p.pj_owner[i] = 1u; p.pj_tabs.push_back(t);
            p.pj_raw += ((uint64_t)t.K * t.N + 7u) & ~(uint64_t)7u;         /* (every table 16-byte aligned) */
            p.pj_rsum += t.Kpad;
            p.pj_plane_bytes += 2u * (uint64_t)t.Kpad * t.Npad;
        }
        p.pj_tab[i] = at.first->second;
    }
}
/* a window's project record, its tiles and (where it is the first to name it) its table and its rows' sums; the window record names
 * the image.  Row k's sum is that of basis[k][n] - 128 over n < N: what the kernel's offset digits need (lnn_k_project.h) */
static inline void wx_project_record(const WxRange &w, const struct LINNEAmdShape &shape, uint32_t i, uint32_t wi, WxPlanned &p,
        WxWindow &ww, const WxProjLists &h)
{
    const struct LINNEAmdProjectSpec &s = *w.pj;
    const uint32_t B = s.clip_bits ? s.clip_bits : 32u;
    const WxProjTable &t = p.pj_tabs[p.pj_tab[i]];
    WxProject &m = h.rec[wi];
    memset(&m, 0, sizeof(m));
    m.out = w.out; m.cstride = s.channel_stride; m.fstride = s.frame_stride; m.rstride = s.row_stride; m.fmt = s.format;
    m.f_lo = w.m_lo; m.nframes = w.m_n;
    m.img = p.nacc; m.istride = ((w.m_n - 1u) * s.hop + s.frame_len + 3u) & ~(uint64_t)3u;
    m.planes = t.planes; m.raw = t.raw; m.rsum = 0;
    for (uint32_t j = 0; j < p.pj_tab[i]; j++) m.rsum += p.pj_tabs[j].Kpad;
    m.N = s.frame_len; m.H = s.hop; m.K = s.num_rows; m.Npad = t.Npad; m.Kpad = t.Kpad; m.shift = s.shift;
    m.hi = (int32_t)(((uint64_t)1 << (B - 1u)) - 1u); m.lo = -m.hi - 1;
    m.scale_bits = (127u - s.float_exp) << 23;            /* 2^-float_exp, float_exp <= 63 */
    m.fidx = i; m.C = shape.num_channels;
    p.nacc += m.istride * shape.num_channels;
    /* the passes place the input range into the image: word j of a channel is stream sample f_lo * H - before + j */
    ww.out = (void *)(uintptr_t)(sizeof(int32_t) * (m.img + (w.lo + s.before - w.m_lo * s.hop)));
    ww.fmt = LINNE_AMD_PCM_S32; ww.stride = m.istride; ww.sstride = 1u;
    for (uint32_t c = 0; c < shape.num_channels; c++)
        for (uint64_t f0 = 0; f0 < w.m_n; f0 += WXP_FRAMES)
            for (uint32_t k0 = 0; k0 < s.num_rows; k0 += WXP_ROWS) {
                assert(p.ntile < p.rs_tiles);
                WxProjTile &tl = h.tile[p.ntile++];
                tl.f0 = f0; tl.win = wi; tl.ch = c; tl.k0 = k0; tl.reserved = 0u;
            }
    if (p.pj_owner[i]) {
        h.tab[p.pj_tab[i]] = t;
        memcpy(h.raw + t.raw, s.basis, sizeof(int16_t) * (size_t)t.K * t.N);
        for (uint32_t k = 0; k < t.Kpad; k++) {
            int32_t sum = 0;
            if (k < t.K) for (uint32_t n = 0; n < t.N; n++) sum += (int32_t)s.basis[(size_t)k * t.N + n] - 128;
            h.rsum[m.rsum + k] = sum;
        }
    }
}

/* step 2: the records, into lists with room for nlive window (and bucket) records, total_rec block records and total_crec COMPRESS
 * entries; h_side NULL for WX_NO_BUCKETS; h_mix, where it is given, gets a mix record per window from the windows' mix specs; h_ov,
 * where it is given, has a record per window of the CALL (W of them, zeroed by the caller) and gets those of the live ones; h_lag
 * likewise */
static inline void wx_plan_fill(const WxRange *rg, uint32_t W, uint32_t group_frames, WxBucketing bucketing, WxPlanned &p,
        WxWindow *h_win, WxBucket *h_side, WxBlock *h_rec, uint32_t *h_crec, WxMix *h_mix = NULL,
        WxResample *h_rs = NULL, WxTile *h_tile = NULL, uint32_t *h_coef = NULL, WxOvSource *h_ov = NULL, WxLagImage *h_lag = NULL,
        const WxProjLists *h_pj = NULL)
{
    for (uint32_t g = 0; g < p.ngroups; g++) {
        const struct LINNEAmdShape &shape = rg[p.gwin[g]].x.shape;
        WxPass cur;
        auto fresh = [&](int check_only) { cur.group = g; cur.rec0 = p.nrec; cur.nrec = 0; cur.c0 = p.ncrec; cur.nc = 0; cur.seg_bytes = 0; cur.check_only = check_only; };
        auto close = [&](int check_only) {
            if (cur.nrec) {
                const WxScratch sc = wx_scratch(cur.nc, shape.num_channels, shape.num_samples_per_block, cur.seg_bytes);
                if (sc.bytes > p.scratch_bytes) p.scratch_bytes = sc.bytes;
                p.passes.push_back(cur);
            }
            fresh(check_only);
        };
        auto add = [&](const WxRange &w, uint32_t wi, uint32_t type, uint32_t r) {
            const WxIndexView &x = w.x;
            /* the counts of step 1 are what the lists were reserved for: nothing is written past them */
            assert(p.nrec < p.total_rec && (type != SX_COMPRESS || p.ncrec < p.total_crec));
            WxBlock &rc = h_rec[p.nrec++];
            memset(&rc, 0, sizeof(rc));
            rc.b = w.stream; rc.N = x.stream_bytes; rc.type = type; rc.win = wi; rc.cidx = 0xFFFFFFFFu; rc.blk = r;
            if (type != WX_TAIL) { rc.off = x.h_off[r]; rc.first = x.h_first[r]; rc.size = x.h_size[r]; rc.nsmp = x.h_nsmp[r]; }
            if (type == SX_COMPRESS) {
                /* the block's slot in the packed segment: whole 16-byte groups, the block at its source's address modulo 16 */
                rc.dst = cur.seg_bytes + ((uintptr_t)(w.stream + rc.off) & 15u);
                cur.seg_bytes = (rc.dst + (uint64_t)rc.size + 6u + 15u) & ~(uint64_t)15u;
                rc.cidx = cur.nc++;
                h_crec[p.ncrec++] = cur.nrec;
            }
            cur.nrec++;
        };
        fresh(0);
        for (uint32_t i = 0; i < W; i++) {
            const WxPlan &pl = p.win[i];
            if (pl.group != (int32_t)g) continue;
            const WxRange &w = rg[i];
            const WxIndexView &x = w.x;
            assert(p.nwin < p.nlive);
            const uint32_t wi = p.nwin++;
            WxWindow &ww = h_win[wi];
            ww.lo = w.lo; ww.hi = w.lo + w.n; ww.covered = x.covered; ww.out = w.out; ww.fidx = i;
            ww.fmt = w.fmt; ww.stride = w.stride; ww.sstride = w.sstride;
            if (h_mix) wx_mix_record(*w.mix, shape, i, h_mix[wi]);
            if (h_rs) wx_resample_record(w, shape, i, wi, p, ww, h_rs[wi], h_tile, h_coef);
            if (h_ov) wx_overlay_source(w, shape, p, ww, h_ov[i]);
            if (h_lag) wx_lag_image(w, shape, p, ww, h_lag[i]);
            if (h_pj) wx_project_record(w, shape, i, wi, p, ww, *h_pj);
            if (bucketing == WX_BITMASK) {
                WxBucket &m = h_side[wi];
                memset(&m, 0, sizeof(m));
                m.out = w.bucket_out; m.min_run = w.quiet_min; m.capacity = w.quiet_capacity; m.threshold = w.quiet_threshold;
                m.abase = p.nacc; m.obase = p.nout; m.n = w.n; m.fidx = i; m.C = shape.num_channels;
                p.nacc += wxq_words(w.n); p.nout += wxq_chunks(w.n);
            } else if (bucketing != WX_NO_BUCKETS) {
                WxBucket &m = h_side[wi];
                const uint64_t b = w.bucket_samples, C = shape.num_channels;
                memset(&m, 0, sizeof(m));
                m.out = w.bucket_out; m.b = (b == 0 || b > w.n) ? w.n : b; m.nb = wx_buckets(w.n, b); m.ns = wx_slots(m.b);
                m.abase = p.nacc; m.obase = p.nout; m.fidx = i;
                if (bucketing == WX_BUCKETS_PER_CHANNEL) {
                    m.cstride = w.bucket_cstride; m.C = (uint32_t)C;
                    p.nacc += m.ns * C * m.nb; p.nout += C * m.nb;
                } else if (bucketing == WX_BUCKETS_PER_BIN) {
                    m.cstride = w.bucket_cstride; m.C = (uint32_t)C; m.hist = w.hist;
                    p.nacc += m.ns * C * m.nb * WXH_BINS(w.hist); p.nout += C * m.nb * WXH_BINS(w.hist);
                } else if (bucketing == WX_BUCKETS_PER_PAIR) {
                    const uint64_t P = LINNE_AMD_NUM_PAIRS(C);
                    m.cstride = w.bucket_cstride; m.C = (uint32_t)C; m.npair = (uint32_t)P;
                    p.nacc += m.ns * P * m.nb; p.nout += P * m.nb;
                } else {
                    /* the slots lie 16 words or more apart, no two in one 64-byte line */
                    m.n = w.n; m.F = (uint32_t)C * ((shape.bits_per_sample + 7u) >> 3);
                    m.sstride = (uint32_t)((m.nb + 15u) & ~(uint64_t)15u);  /* (nb < 2^32 - 15 where ns > 1: such a bucket has 8192 samples) */
                    p.nacc += m.ns > 1u ? (uint64_t)m.ns * m.sstride : m.nb; p.nout += m.nb;
                }
            }
            const bool big = group_frames && pl.ncomp > group_frames;
            if (big) {
                close(1);
                for (uint32_t y = 0; y < pl.nr; y++) {
                    const uint32_t r = pl.r0 + y;
                    if (x.h_type[r] != SX_COMPRESS) continue;
                    if (cur.nc == group_frames) close(1);
                    add(w, wi, SX_COMPRESS, r);
                }
                close(0);
            } else if (group_frames && cur.nc + pl.ncomp > group_frames) close(0);
            if (ww.hi > ww.covered) add(w, wi, WX_TAIL, 0);
            for (uint32_t y = 0; y < pl.nr; y++) {
                const uint32_t r = pl.r0 + y, type = x.h_type[r];
                if (type == SX_COMPRESS && group_frames && cur.nc == group_frames) close(0);
                add(w, wi, type, r);
            }
            if (big) close(0);
        }
        close(0);
    }
    if (bucketing == WX_BITMASK) { p.nmask = p.nacc; p.nacc += wxq_chunk_units(p.nout); }
    if (h_pj) {                         /* the digit planes lie behind the images, 16-byte aligned, in the images' 32-bit words */
        p.pj_plane0 = (p.nacc + 3u) & ~(uint64_t)3u;
        p.nacc = p.pj_plane0 + (p.pj_plane_bytes + 3u) / 4u;
    }
}

#endif
