/* lnn_block_scan.h -- where the lists of one block-head scan lie ("The indexes of many streams in one call").
 * LINNEAmd_StreamIndexesCreate and LINNEAmd_RepairStreamsDevice run the same scan over the T streams of a call; its lists lie in
 * pinned host memory and at the same offsets in device memory.  Plain host C with no HIP in it, so that a small stand-alone program
 * can drive it.
 *
 * In this order, every part 256-byte aligned:
 *   st     T stream records               \
 *   row0   T + 1 first (stream, wave) rows | what goes up behind the headers step, in one copy: [o_st, o_crow)
 *   early  the caller's own, uploaded too /  (repair: the streams' block bounds, then the CRC and Huffman tables; the index: nothing)
 *   crow   T + 1 first chain rows
 *   hdr    T gathered headers, hdr_slot bytes each
 *   seg    T + 1 segment bounds of the candidates
 *   len    T chain lengths
 *   late   the caller's own (repair: the segment bounds of the sound candidates, then of the runs; the index: the tables, on their
 *          way from the host into its slab) */
#ifndef LNN_BLOCK_SCAN_H_INCLUDED
#define LNN_BLOCK_SCAN_H_INCLUDED

#include <stdint.h>

struct IbLists { uint64_t o_st, o_row0, o_early, o_crow, o_hdr, o_seg, o_len, o_late, bytes; };

static inline uint64_t ib_lists_align(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }

/* st_bytes: a stream record's size; early_bytes, late_bytes: the caller's own parts (aligned sums of what it puts there) */
static inline struct IbLists ib_lists(uint64_t T, uint64_t st_bytes, uint64_t hdr_slot, uint64_t early_bytes, uint64_t late_bytes)
{
    struct IbLists a;
    a.o_st = 0;
    a.o_row0 = ib_lists_align(a.o_st + st_bytes * T);
    a.o_early = ib_lists_align(a.o_row0 + sizeof(uint64_t) * (T + 1u));
    a.o_crow = ib_lists_align(a.o_early + early_bytes);
    a.o_hdr = ib_lists_align(a.o_crow + sizeof(uint64_t) * (T + 1u));
    a.o_seg = ib_lists_align(a.o_hdr + hdr_slot * T);
    a.o_len = ib_lists_align(a.o_seg + sizeof(uint64_t) * (T + 1u));
    a.o_late = ib_lists_align(a.o_len + sizeof(uint64_t) * T);
    a.bytes = ib_lists_align(a.o_late + late_bytes);
    return a;
}

#endif
