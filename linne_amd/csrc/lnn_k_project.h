/* lnn_k_project.h -- projecting the frames of sample windows of resident .lnn streams on int16 basis rows: the exact integer STFT, a filter
 * bank, a band-energy front end (LINNEAmd_ProjectWindowsDevice, which states the arithmetic; DESIGN.md section 5, "Projecting instead of
 * placing").
 *
 * As for the resampling consumer, the passes of the call place every window's INPUT range, halo included, into an int32 planar image
 * behind the passes' scratch (k_wx_place, with the image as its target); two launches do the rest:
 *   k_wx_project_preset       the images zeroed (the zeros in front of sample 0, behind the stream's last sample and in the rounding of a
 *                             channel's stride), and every basis of the call cut into two planes of int8 digits, Kpad rows of Npad
 *                             bytes each (K rounded up to 16, N to 64; the padding is zero in both planes)
 *   k_wx_project              a workgroup per tile: WXP_FRAMES frames by WXP_ROWS rows of one channel of one window (the host's tile
 *                             list).  The sum over a frame's N samples runs on the MATRIX unit, v_mfma_i32_16x16x64_i8: one
 *                             instruction is 16 basis rows (operand A) by 16 frames (operand B) over 64 frame samples, and a wave owns
 *                             16 frames of the tile and all of its rows.
 *
 * The digits.  The call is not modular, so both operands are cut exactly:
 *   basis   v = 256 * hi + lo' + 128 with lo' = (v & 255) - 128 and hi = v >> 8: both in [-128, 127] for every int16.  The 128 times
 *           the frame's sample sum that this leaves over comes from one more operand A of ones (over n < N), shared by all rows;
 *   sample  x = sum over b < P of 256^b * d_b + c_P, with d = x ^ c_P cut into bytes, c_P = 0x80, 0x8080, 0x808080 for P = 2, 3, 4
 *           planes: the low P - 1 bytes are the unsigned bytes of x less 128, the top one is x's own signed byte.  Exact for every x
 *           that fits 8 P bits, and P = 4 takes all of int32.  c_P times the row's sum of (v - 128) is a table of the host's.
 *   P is chosen per tile from the values the tile reads (a pass over its span of the image in front of the sums): a 16-bit stream costs
 *   2 x 2 plane products, a 24-bit stream 2 x 3, anything beyond the full 2 x 4.  Every pair of planes keeps an int32 accumulator over the
 *   whole frame (a digit product is at most 2^14, 4096 of them 2^26) and they recombine in int64 as sum acc[a][b] << 8 (a + b).
 * The operands.  The frame runs through LDS in slices of WXP_SLICE samples.  A slice of the basis' planes is copied as it lies (16-byte
 * groups) and serves all four waves' frames.  The samples are staged UNFOLDED: frame j's slice lies at row j of the LDS array, cut into
 * digits on the way, so every 16-byte operand read is aligned whatever the hop is -- frame f's column starts at sample f * H of the image,
 * which no alignment survives -- and a hop longer than the frame needs no case of its own.  The price is that samples shared by
 * overlapping frames are read from the image (L2) once per frame, not once.  Rows are WXP_LROW = 144 bytes apart: the 16 lanes of an
 * operand read then cover all 64 banks once.  LDS: 4 x 64 x 144 + 2 x 64 x 144 = 55296 bytes.
 * Edges.  Ragged rows, frames and taps (K % 16, frames % 16, N % 64) are zeros in the operands: all sums run on the matrix unit, and
 * what a tile has no element for is computed and not stored.  -DWXP_MATRIX=0 builds the plain form alone, one 64-bit multiply-add per
 * product from the same tiles, for measuring the two against each other.
 * Stores.  A lane ends up with one frame and 4 consecutive rows of each 16-row group, 16 lanes with 16 consecutive frames: with
 * frame_stride 1 the lanes of a store are contiguous, with row_stride 1 a lane's four stores and its three neighbours' are one 64-byte run.
 * A tile of a window whose fail word is set is skipped.  Plain C++ and vector stores only; the one atomic is the OR into `saturated`.
 */
#ifndef LNN_K_PROJECT_H_INCLUDED
#define LNN_K_PROJECT_H_INCLUDED

#include "lnn_k_windows.h"

#ifndef WXP_MATRIX
#define WXP_MATRIX 1
#endif
#define WXP_THREADS 256u
#define WXP_SLICE 128u                  /* frame samples per trip through LDS: two steps of the matrix instruction */
#define WXP_LROW (WXP_SLICE + 16u)      /* bytes from one row of a staged slice to the next */
#define WXP_PSLICE 32u                  /* the plain form's slice */
static_assert(WXP_FRAMES == 64u && WXP_ROWS == 64u && WXP_THREADS == 256u, "a wave owns 16 frames of a tile, and a tile has four 16-row groups");

struct WxProjectArgs {
    const WxProjTile *tiles; uint32_t ntiles;
    const WxProject *pwin;              /* [nwin] beside the window records */
    const uint32_t *fail; uint32_t *sat;
    const int32_t *acc;                 /* the images */
    const int8_t *planes;               /* the call's digit planes */
    const int16_t *raw;                 /* the call's tables as the caller gave them */
    const int32_t *rsum;                /* their rows' sums of (v - 128) */
};
struct WxProjectPresetArgs { uint4 *acc; uint64_t n16; const WxProjTable *tabs; uint32_t ntab; const int16_t *raw; int8_t *planes; };

__global__ __launch_bounds__(WXB_THREADS) void k_wx_project_preset(WxProjectPresetArgs a)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * WXB_THREADS + threadIdx.x, step = (uint64_t)gridDim.x * WXB_THREADS;
    for (uint64_t i = t0; i < a.n16; i += step) a.acc[i] = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t t = 0; t < a.ntab; t++) {
        const WxProjTable tb = a.tabs[t];
        const uint64_t cnt = (uint64_t)tb.Kpad * tb.Npad;
        int8_t *lo = a.planes + tb.planes, *hi = lo + cnt;
        const int16_t *src = a.raw + tb.raw;
        for (uint64_t i = t0; i < cnt; i += step) {
            const uint32_t k = (uint32_t)(i / tb.Npad), n = (uint32_t)(i - (uint64_t)k * tb.Npad);
            int32_t l = 0, h = 0;
            if (k < tb.K && n < tb.N) { const int32_t v = src[(uint64_t)k * tb.N + n]; l = (v & 255) - 128; h = v >> 8; }
            lo[i] = (int8_t)l; hi[i] = (int8_t)h;
        }
    }
}

/* steps 2 to 4 of the call's arithmetic and the store of element (frame fr of the window, row k) */
__device__ __forceinline__ int wxp_finish(const WxProject *r, uint32_t ch, uint64_t fr, uint32_t k, int64_t acc)
{
    const uint32_t shift = r->shift;
    if (shift) acc = (acc + ((int64_t)1 << (shift - 1u))) >> shift;
    const int64_t lo = r->lo, hi = r->hi, y = acc > hi ? hi : (acc < lo ? lo : acc);
    uint32_t *out = (uint32_t *)r->out + ((uint64_t)ch * r->cstride + fr * r->fstride + (uint64_t)k * r->rstride);
    *out = (r->fmt == LINNE_AMD_PCM_F32) ? __float_as_uint((float)(int32_t)y * __uint_as_float(r->scale_bits)) : (uint32_t)(int32_t)y;
    return y != acc;
}

#if WXP_MATRIX
/* the sums of one wave's 16 frames by the tile's rows, over all slices, with P sample planes; then the wave's stores */
template <int P> __device__ __forceinline__ int wxp_matrix(const WxProjectArgs &a, const WxProjTile &t, const WxProject *r, const int32_t *image,
        int8_t (*xs)[WXP_FRAMES][WXP_LROW], int8_t (*bs)[WXP_ROWS][WXP_LROW], uint32_t cnt_f, uint32_t cnt_k)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, i = lane & 15u, g4 = lane >> 4;
    const uint32_t N = r->N, H = r->H, Npad = r->Npad, Kpad = r->Kpad;
    const uint32_t cmask = P == 2 ? 0x80u : (P == 3 ? 0x8080u : 0x808080u);
    const int8_t *plane = a.planes + r->planes;
    const uint64_t psize = (uint64_t)Kpad * Npad;
    const uint32_t ngrp = (cnt_k + 15u) / 16u;                     /* the tile's 16-row groups */
    const bool busy = 16u * wave < cnt_f;                           /* wave-uniform: the wave has a frame of the tile */
    lnn_v4i acc[4][2][P], ones[P];
#pragma unroll
    for (int g = 0; g < 4; g++)
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int b = 0; b < P; b++) acc[g][p][b] = lnn_v4i{ 0, 0, 0, 0 };
#pragma unroll
    for (int b = 0; b < P; b++) ones[b] = lnn_v4i{ 0, 0, 0, 0 };
    for (uint32_t s0 = 0; s0 < Npad; s0 += WXP_SLICE) {            /* block-uniform */
        __syncthreads();                /* (the slice before has been read) */
        /* the basis: 2 planes x 64 rows x 8 groups of 16 bytes, as they lie; zeros behind the table's rows and columns */
        for (uint32_t e = tid; e < 2u * WXP_ROWS * (WXP_SLICE / 16u); e += WXP_THREADS) {
            const uint32_t q = e & 7u, row = (e >> 3) & 63u, p = e >> 9;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (t.k0 + row < Kpad && s0 + 16u * q < Npad) v = *(const uint4 *)(plane + p * psize + (uint64_t)(t.k0 + row) * Npad + s0 + 16u * q);
            *(uint4 *)&bs[p][row][16u * q] = v;
        }
        /* the samples: 64 frames x 32 groups of 4, cut into P planes; zeros behind the tile's frames and the frame's samples */
        for (uint32_t e = tid; e < WXP_FRAMES * (WXP_SLICE / 4u); e += WXP_THREADS) {
            const uint32_t q = e & 31u, j = e >> 5, n = s0 + 4u * q;
            uint32_t d[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) d[u] = ((j < cnt_f && n + u < N) ? (uint32_t)image[(uint64_t)j * H + n + u] : 0u) ^ cmask;
#pragma unroll
            for (int b = 0; b < P; b++)
                *(uint32_t *)&xs[b][j][4u * q] = ((d[0] >> (8 * b)) & 255u) | ((d[1] >> (8 * b)) & 255u) << 8 | ((d[2] >> (8 * b)) & 255u) << 16 | ((d[3] >> (8 * b)) & 255u) << 24;
        }
        __syncthreads();
        if (!busy) continue;            /* (wave-uniform; the barriers above are reached by all) */
#pragma unroll
        for (uint32_t st = 0; st < WXP_SLICE / 64u; st++) {
            const uint32_t n0 = s0 + 64u * st + 16u * g4;          /* my 16 samples of the step */
            if (s0 + 64u * st >= Npad) break;                       /* block-uniform */
            lnn_v4i xv[P], one;
#pragma unroll
            for (int b = 0; b < P; b++) xv[b] = *(const lnn_v4i *)&xs[b][16u * wave + i][64u * st + 16u * g4];
            /* ones over n < N */
#pragma unroll
            for (uint32_t w = 0; w < 4u; w++) {
                const uint32_t at = n0 + 4u * w, m = at >= N ? 0u : (N - at < 4u ? N - at : 4u);
                one[w] = (int)(m == 0u ? 0u : 0x01010101u >> (8u * (4u - m)));
            }
#pragma unroll
            for (int b = 0; b < P; b++) ones[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(one, xv[b], ones[b], 0, 0, 0);
#pragma unroll
            for (uint32_t g = 0; g < 4u; g++) {
                if (g >= ngrp) break;                               /* block-uniform */
#pragma unroll
                for (uint32_t p = 0; p < 2u; p++) {
                    const lnn_v4i bv = *(const lnn_v4i *)&bs[p][16u * g + i][64u * st + 16u * g4];
#pragma unroll
                    for (int b = 0; b < P; b++) acc[g][p][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bv, xv[b], acc[g][p][b], 0, 0, 0);
                }
            }
        }
    }
    /* my frame is column i of the wave's 16; my rows are 4 g4 .. 4 g4 + 3 of every group */
    int sat = 0;
    const uint32_t j = 16u * wave + i;
    if (busy && j < cnt_f) {
        int64_t sx = 0;
#pragma unroll
        for (int b = 0; b < P; b++) sx += (int64_t)ones[b][0] << (8 * b);
        const int64_t shared = 128 * (sx + (int64_t)N * cmask);
        const int32_t *rsum = a.rsum + r->rsum;
#pragma unroll
        for (uint32_t g = 0; g < 4u; g++) {
            if (g >= ngrp) break;
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) {
                const uint32_t k = t.k0 + 16u * g + 4u * g4 + e;
                if (k >= r->K) continue;
                int64_t v = shared + (int64_t)cmask * rsum[k];
#pragma unroll
                for (int p = 0; p < 2; p++)
#pragma unroll
                    for (int b = 0; b < P; b++) v += (int64_t)acc[g][p][b][e] << (8 * (p + b));
                sat |= wxp_finish(r, t.ch, t.f0 + j, k, v);
            }
        }
    }
    return sat;
}
#endif

__global__ __launch_bounds__(WXP_THREADS) void k_wx_project(WxProjectArgs a)
{
    if (blockIdx.x >= a.ntiles) return;
    const WxProjTile t = a.tiles[blockIdx.x];
    const WxProject *r = a.pwin + t.win;
    if (a.fail[r->fidx] != WX_NOFAIL) return;                       /* block-uniform */
    const uint32_t tid = threadIdx.x;
    const uint32_t N = r->N, H = r->H, K = r->K;
    const uint32_t cnt_f = (r->nframes - t.f0 < WXP_FRAMES) ? (uint32_t)(r->nframes - t.f0) : WXP_FRAMES;
    const uint32_t cnt_k = (K - t.k0 < WXP_ROWS) ? K - t.k0 : WXP_ROWS;
    /* sample n of the tile's frame j: image[j * H + n]; the last one read is (cnt_f - 1) * H + N - 1, inside the channel's istride words */
    const int32_t *image = a.acc + r->img + (uint64_t)t.ch * r->istride + t.f0 * H;
    int sat = 0;
#if WXP_MATRIX
    __shared__ __attribute__((aligned(16))) int8_t xs[4][WXP_FRAMES][WXP_LROW];
    __shared__ __attribute__((aligned(16))) int8_t bs[2][WXP_ROWS][WXP_LROW];
    /* the planes the tile's values need: a value fits 8 P bits when v ^ (v >> 31) < 2^(8 P - 1) */
    uint32_t top = 0;
    if (H <= N) {                       /* the frames overlap or touch: one span */
        const uint64_t span = (uint64_t)(cnt_f - 1u) * H + N;
        for (uint64_t e = tid; e < span; e += WXP_THREADS) { const int32_t v = image[e]; top |= (uint32_t)(v ^ (v >> 31)); }
    } else {
        for (uint32_t j = 0; j < cnt_f; j++)
            for (uint32_t n = tid; n < N; n += WXP_THREADS) { const int32_t v = image[(uint64_t)j * H + n]; top |= (uint32_t)(v ^ (v >> 31)); }
    }
    const int wide = __syncthreads_or(top >= (1u << 23)), mid = __syncthreads_or(top >= (1u << 15));
    if (wide) sat = wxp_matrix<4>(a, t, r, image, xs, bs, cnt_f, cnt_k);
    else if (mid) sat = wxp_matrix<3>(a, t, r, image, xs, bs, cnt_f, cnt_k);
    else sat = wxp_matrix<2>(a, t, r, image, xs, bs, cnt_f, cnt_k);
#else
    /* the plain form: a lane owns one row and a wave 16 frames; slices of WXP_PSLICE samples of both through LDS */
    __shared__ int32_t xp[WXP_FRAMES][WXP_PSLICE + 1u];
    __shared__ int32_t bp[WXP_ROWS][WXP_PSLICE + 1u];
    const uint32_t row = tid & 63u, f16 = 16u * (tid >> 6);
    const int16_t *tab = a.raw + r->raw;
    int64_t acc[16];
#pragma unroll
    for (int m = 0; m < 16; m++) acc[m] = 0;
    for (uint32_t s0 = 0; s0 < N; s0 += WXP_PSLICE) {
        __syncthreads();
        for (uint32_t e = tid; e < WXP_FRAMES * WXP_PSLICE; e += WXP_THREADS) {
            const uint32_t q = e & (WXP_PSLICE - 1u), j = e / WXP_PSLICE, n = s0 + q;
            xp[j][q] = (j < cnt_f && n < N) ? image[(uint64_t)j * H + n] : 0;
            bp[j][q] = (j < cnt_k && n < N) ? (int32_t)tab[(uint64_t)(t.k0 + j) * N + n] : 0;
        }
        __syncthreads();
        for (uint32_t q = 0; q < WXP_PSLICE; q++) {
            const int64_t c = bp[row][q];
#pragma unroll
            for (int m = 0; m < 16; m++) acc[m] += c * (int64_t)xp[f16 + m][q];
        }
    }
    if (row < cnt_k)
#pragma unroll
        for (int m = 0; m < 16; m++) if (f16 + m < cnt_f) sat |= wxp_finish(r, t.ch, t.f0 + f16 + m, t.k0 + row, acc[m]);
#endif
    sat = __syncthreads_or(sat);
    if (sat && tid == 0) atomicOr(&a.sat[r->fidx], 1u);
}

#endif
