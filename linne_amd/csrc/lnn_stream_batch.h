/* lnn_stream_batch.h -- the host's planning for LINNEAmd_EncodeStreamsDevice ("Encoding many tracks in one
 * call"): which frames of which tracks a pass holds, the order of its rows, and the slices of rows the analysis takes per call.
 * Plain host C++ with no HIP in it, so that a small stand-alone program can drive it (under a sanitizer, say).
 *
 * The tracks of one shape, in the caller's order, form one list of frames (each track's frames in stream order); a pass is the next
 * max_frames of that list, so a track may span passes.  A frame's SLOT is its place in the pass in that stream order.  The ROWS of
 * the pass -- the order the analysis, the Rice plan and the writers work in -- are the full frames first, in stream order, then the
 * ragged frames (a track's last, shorter than a block) sorted by length: LINNEAmd_EncodeFramesDevice takes at most SB_MAXLEN
 * distinct lengths per call, so the rows are cut into contiguous slices of at most that many; sorted this way a pass of d distinct
 * lengths takes ceil(d / SB_MAXLEN) calls, the first of which holds the full frames. */
#ifndef LNN_STREAM_BATCH_H_INCLUDED
#define LNN_STREAM_BATCH_H_INCLUDED

#include <stdint.h>
#include <algorithm>
#include <vector>

#define SB_MAXLEN 16u                   /* = LNN_MAXCLS (lnn_forms.h) */

struct SbPlanSeg { uint32_t track; uint32_t slot0, nslots; uint64_t frame0; };     /* a track's part of a pass: its number in the group, its slots, its first frame here */
struct SbPlanRow { uint32_t seg, slot, nsmp; uint64_t first; };                    /* index into segs; the slot; the frame's length and first sample in its track */
struct SbPassPlan {
    std::vector<SbPlanSeg> segs;        /* in track order = slot order */
    std::vector<SbPlanRow> rows;
    std::vector<uint32_t> slice;        /* slice k = rows [slice[k], slice[k + 1]) */
    uint32_t distinct;                  /* distinct frame lengths of the pass */
};
struct SbPlanner {
    const uint64_t *samples; uint32_t ntracks, S;       /* samples per channel of every track of the group; the block size */
    uint32_t t; uint64_t f;                             /* the next frame: frame f of track t */
};

/* ---- the PCM layout of a track or window (include/linne_amd.h struct LINNEAmdPcmLayout) ----
 * formats as LINNE_AMD_PCM_*; SB_LY_* = why a layout is refused (0: it is taken) */
#define SB_PCM_S32 0u
#define SB_PCM_S16 1u
#define SB_PCM_S24 2u
#define SB_PCM_F32 3u
enum { SB_LY_OK = 0, SB_LY_FORMAT, SB_LY_ALIGN, SB_LY_STRIDES };

static inline uint32_t sb_elem_bytes(uint32_t format) { return format == SB_PCM_S16 ? 2u : (format == SB_PCM_S24 ? 3u : 4u); }

/* The argument check on a layout: `base` the PCM's address, C channels of n samples, decode: the call writes PCM (F32 is a decode
 * format only).  The strides must make (ch, i) -> ch * cs + i * ss injective in one of the two ways the header names: channels apart
 * by at least a channel's span (planar), or samples apart by at least C channels' span (interleaved). */
static inline int sb_layout_check(uint32_t format, uint64_t cs, uint64_t ss, uint64_t base, uint32_t C, uint64_t n, bool decode)
{
    if (format > SB_PCM_F32 || (format == SB_PCM_F32 && !decode)) return SB_LY_FORMAT;
    const uint64_t align = format == SB_PCM_S16 ? 2u : (format == SB_PCM_S24 ? 1u : 4u);
    if (base & (align - 1u)) return SB_LY_ALIGN;
    typedef unsigned __int128 u128;
    if (C <= 1u) { if (ss < 1u) return SB_LY_STRIDES; cs = 0; }
    else {
        const bool planar = ss >= 1u && (u128)cs >= (u128)n * ss;
        const bool interleaved = cs >= 1u && (u128)ss >= (u128)C * cs;
        if (!planar && !interleaved) return SB_LY_STRIDES;
    }
    /* the last element's byte offset must be a uint64 the kernels can add to the base */
    const u128 last = ((u128)(C ? C - 1u : 0u) * cs + (u128)(n ? n - 1u : 0u) * ss + 1u) * sb_elem_bytes(format);
    return last < ((u128)1 << 62) ? SB_LY_OK : SB_LY_STRIDES;
}
static inline const char *sb_layout_text(int why)
{
    return why == SB_LY_FORMAT ? "a PCM format this call does not take" : why == SB_LY_ALIGN ? "the PCM base is not aligned to its format's element"
         : "channel_stride and sample_stride let two samples share an element";
}

static inline uint64_t sb_frames(uint64_t samples, uint32_t S) { return (samples + S - 1u) / S; }

static inline void sb_planner_init(SbPlanner *pl, const uint64_t *samples, uint32_t ntracks, uint32_t S)
{
    pl->samples = samples; pl->ntracks = ntracks; pl->S = S; pl->t = 0; pl->f = 0;
}

/* the next pass of at most max_frames (>= 1) frames; false when no frame is left */
static inline bool sb_next_pass(SbPlanner *pl, uint64_t max_frames, SbPassPlan *p)
{
    const uint32_t S = pl->S;
    p->segs.clear(); p->rows.clear(); p->slice.clear(); p->distinct = 0;
    std::vector<SbPlanRow> ragged;
    uint32_t slot = 0;
    while (pl->t < pl->ntracks && slot < max_frames) {
        const uint64_t N = pl->samples[pl->t], F = sb_frames(N, S);
        if (pl->f >= F) { pl->t++; pl->f = 0; continue; }
        uint64_t take = F - pl->f;
        if (take > max_frames - slot) take = max_frames - slot;
        SbPlanSeg sg; sg.track = pl->t; sg.slot0 = slot; sg.nslots = (uint32_t)take; sg.frame0 = pl->f;
        const uint32_t si = (uint32_t)p->segs.size();
        p->segs.push_back(sg);
        for (uint64_t k = 0; k < take; k++, slot++) {
            SbPlanRow r; r.seg = si; r.slot = slot; r.first = (pl->f + k) * S;
            r.nsmp = (N - r.first < S) ? (uint32_t)(N - r.first) : S;
            if (r.nsmp == S) p->rows.push_back(r); else ragged.push_back(r);
        }
        pl->f += take;
    }
    if (slot == 0) return false;
    std::sort(ragged.begin(), ragged.end(), [](const SbPlanRow &a, const SbPlanRow &b) { return a.nsmp != b.nsmp ? a.nsmp < b.nsmp : a.slot < b.slot; });
    p->rows.insert(p->rows.end(), ragged.begin(), ragged.end());
    uint32_t in_slice = 0;
    for (uint32_t i = 0; i < p->rows.size(); i++) {
        if (i == 0 || p->rows[i].nsmp != p->rows[i - 1].nsmp) {        /* (equal lengths are neighbours) */
            p->distinct++;
            if (i == 0 || in_slice == SB_MAXLEN) { p->slice.push_back(i); in_slice = 0; }
            in_slice++;
        }
    }
    p->slice.push_back((uint32_t)p->rows.size());
    return true;
}

/* analysis calls of a pass of `distinct` lengths */
static inline uint32_t sb_analysis_calls(uint32_t distinct) { return distinct <= SB_MAXLEN ? 1u : 1u + (distinct - SB_MAXLEN + SB_MAXLEN - 1u) / SB_MAXLEN; }

#endif
