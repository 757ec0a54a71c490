/* lnn_k_splice.h -- the device side of LINNEAmd_SpliceStreamsDevice (lnn_device.hip; DESIGN.md section 5, "Cutting and joining
 * resident streams"): one launch copies every run of bytes of every output.
 *
 *   k_sp_copy   runs[r] = { src, dst, n, chunk0 }: n bytes from src (any alignment) to dst (any alignment).  The runs are cut into
 *               chunks of SP_CHUNK_UNITS 16-byte units of the DESTINATION (lnn_splice.h sp_run_parts: up to 15 head bytes to the
 *               destination's next 16-byte boundary, whole units, up to 15 tail bytes); chunk0 is the number of the run's first chunk
 *               among all chunks of the launch, runs[nruns].chunk0 their count.  A workgroup takes chunks blockIdx.x, + gridDim.x, ...
 *               and finds a chunk's run by bisection of chunk0, so what a workgroup does never depends on how long a run is.
 *
 * What touches memory:
 *   stores  a unit is one 16-byte store to a 16-byte-aligned address whose 16 bytes all belong to the run's destination; head and
 *           tail bytes are byte stores.  Two runs of one output meet at any byte: the word at their seam is written by the byte
 *           stores of either side, never by a wider store (the rule of k_sb_zero); outputs are 4-byte aligned and disjoint, so
 *           different outputs never share a word.
 *   loads   a unit whose source is 16-byte aligned is one 16-byte load inside the run.  Otherwise it is put together in registers
 *           from the two ALIGNED 16-byte vectors its source bytes lie in, when both lie wholly inside [src, src + n); a unit for which
 *           one of them does not (at most the first and the last unit of a run) is put together from 16 byte loads.  Head and tail
 *           are byte loads.  So no load touches a byte outside the source run. */
#ifndef LNN_K_SPLICE_H_INCLUDED
#define LNN_K_SPLICE_H_INCLUDED

#include "lnn_splice.h"

#define SP_THREADS 256u
#define SP_MAX_GRID 2048u               /* workgroups of a launch: 8 per CU; more chunks are walked by a grid stride */

struct SpRun { const uint8_t *src; uint8_t *dst; uint64_t n; uint64_t chunk0; };
/* the runs' pointers come out of a table: said to be global memory, so that the copies are global_load / global_store and not flat ones */
#define SP_GLOBAL __attribute__((address_space(1)))
typedef SP_GLOBAL const uint8_t *sp_src_t;
typedef SP_GLOBAL uint8_t *sp_dst_t;
typedef uint32_t sp_u4 __attribute__((ext_vector_type(4)));       /* 16 bytes, a plain vector (HIP's uint4 class has no copy between address spaces) */
typedef SP_GLOBAL const sp_u4 *sp_srcv_t;
typedef SP_GLOBAL sp_u4 *sp_dstv_t;

/* bytes [m, m + 16) of the 32 bytes x | y (m = 1 .. 15), little-endian words */
__device__ __forceinline__ sp_u4 sp_realign(sp_u4 x, sp_u4 y, uint32_t m)
{
    const uint32_t q = m >> 2, sh = (m & 3u) * 8u;
    const uint32_t a0 = q == 0u ? x.x : (q == 1u ? x.y : (q == 2u ? x.z : x.w));
    const uint32_t a1 = q == 0u ? x.y : (q == 1u ? x.z : (q == 2u ? x.w : y.x));
    const uint32_t a2 = q == 0u ? x.z : (q == 1u ? x.w : (q == 2u ? y.x : y.y));
    const uint32_t a3 = q == 0u ? x.w : (q == 1u ? y.x : (q == 2u ? y.y : y.z));
    const uint32_t a4 = q == 0u ? y.x : (q == 1u ? y.y : (q == 2u ? y.z : y.w));
    sp_u4 v;
    v.x = (uint32_t)((((uint64_t)a1 << 32) | a0) >> sh);
    v.y = (uint32_t)((((uint64_t)a2 << 32) | a1) >> sh);
    v.z = (uint32_t)((((uint64_t)a3 << 32) | a2) >> sh);
    v.w = (uint32_t)((((uint64_t)a4 << 32) | a3) >> sh);
    return v;
}

/* (volatile: sixteen byte loads, which the compiler may not merge into a wider one) */
__device__ __forceinline__ sp_u4 sp_load_bytes(SP_GLOBAL const volatile uint8_t *p)
{
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
    sp_u4 v;
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    return v;
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_copy(const SpRun *runs, uint32_t nruns, uint64_t nchunks)
{
    const uint32_t tid = threadIdx.x;
    for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        uint32_t lo = 0, hi = nruns;                            /* runs[lo].chunk0 <= c < runs[hi].chunk0 */
        while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (runs[mid].chunk0 <= c) lo = mid; else hi = mid; }
        sp_src_t src = (sp_src_t)runs[lo].src;
        sp_dst_t dst = (sp_dst_t)runs[lo].dst;
        const uint64_t n = runs[lo].n, k = c - runs[lo].chunk0;
        uint64_t head, body, tail;
        sp_run_parts((uint64_t)(uintptr_t)dst, n, &head, &body, &tail);
        const uint64_t u0 = k * SP_CHUNK_UNITS, u1 = (body - u0 > SP_CHUNK_UNITS) ? u0 + SP_CHUNK_UNITS : body;       /* this chunk's units [u0, u1); u0 <= body */
        if (k == 0u && tid < head) dst[tid] = src[tid];
        if (u1 == body && tid < tail) { const uint64_t at = head + (body << 4) + tid; dst[at] = src[at]; }
        sp_src_t sb = src + head;
        sp_dstv_t db = (sp_dstv_t)(dst + head);                     /* 16-byte aligned whenever body > 0 */
        const uint32_t m = (uint32_t)((uintptr_t)sb & 15u);
        if (m == 0u) {
            sp_srcv_t sv = (sp_srcv_t)sb;
#pragma unroll 4
            for (uint64_t u = u0 + tid; u < u1; u += SP_THREADS) db[u] = sv[u];
        } else {
            const uintptr_t s_lo = (uintptr_t)src, s_hi = s_lo + n;
#pragma unroll 4
            for (uint64_t u = u0 + tid; u < u1; u += SP_THREADS) {
                sp_src_t p = sb + (u << 4);
                const uintptr_t a = (uintptr_t)p - m;           /* the aligned vector p's first byte lies in */
                sp_u4 v;
                if (a >= s_lo && a + 32u <= s_hi) v = sp_realign(*(sp_srcv_t)a, *(sp_srcv_t)(a + 16u), m);
                else v = sp_load_bytes((SP_GLOBAL const volatile uint8_t *)p);
                db[u] = v;
            }
        }
    }
}

#endif
