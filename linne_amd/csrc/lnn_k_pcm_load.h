/* lnn_k_pcm_load.h -- loads of the caller's PCM in any layout (include/linne_amd.h struct LINNEAmdPcmLayout), shared by the kernels
 * that read it: the stream encoder's gathers (lnn_k_stream_enc.h) and the windows' compare (lnn_k_compare.h). */
#ifndef LNN_K_PCM_LOAD_H_INCLUDED
#define LNN_K_PCM_LOAD_H_INCLUDED

/* ---- reading PCM of any layout (include/linne_amd.h struct LINNEAmdPcmLayout) ----
 * Four consecutive elements -- 8, 12 or 16 bytes at q, aligned to the element only -- from the aligned 32-bit words that hold them.
 * [lo, hi) are the bytes of the contiguous run of elements q lies in (a planar channel, or a whole packed interleaved track): a word
 * is loaded whole where all of it lies in the run and put together from the run's bytes where it does not (the run's two ends), so
 * no byte outside the run is touched.  Only the words that hold the first cnt (1 .. 4) elements are read; v[cnt ..] = 0. */
__device__ __forceinline__ uint32_t ly_word(const uint8_t *w, const uint8_t *lo, const uint8_t *hi)
{
    if (w >= lo && w + 4 <= hi) return *(const uint32_t *)w;
    uint32_t v = 0;
    for (uint32_t t = 0; t < 4u; t++) if (w + t >= lo && w + t < hi) v |= (uint32_t)w[t] << (8u * t);
    return v;
}
__device__ __forceinline__ void ly_load4(const uint8_t *q, const uint8_t *lo, const uint8_t *hi, uint32_t fmt, uint32_t cnt, int32_t v[4])
{
    const uint32_t es = fmt == LINNE_AMD_PCM_S16 ? 2u : (fmt == LINNE_AMD_PCM_S24 ? 3u : 4u);
    const uint32_t mis = (uint32_t)((uintptr_t)q & 3u), sh = mis * 8u, nw = (mis + cnt * es + 3u) >> 2;      /* nw <= 4 */
    const uint8_t *w0 = q - mis;
    uint32_t W[5], B[4];
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) W[i] = (i < nw) ? ly_word(w0 + 4u * i, lo, hi) : 0u;
    W[4] = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) B[i] = sh ? ((W[i] >> sh) | (W[i + 1] << (32u - sh))) : W[i];
    if (fmt == LINNE_AMD_PCM_S16) {
        v[0] = (int16_t)B[0]; v[1] = (int16_t)(B[0] >> 16); v[2] = (int16_t)B[1]; v[3] = (int16_t)(B[1] >> 16);
    } else if (fmt == LINNE_AMD_PCM_S24) {
        v[0] = (int32_t)(B[0] << 8) >> 8; v[1] = (int32_t)(((B[0] >> 24) | (B[1] << 8)) << 8) >> 8;
        v[2] = (int32_t)(((B[1] >> 16) | (B[2] << 16)) << 8) >> 8; v[3] = (int32_t)B[2] >> 8;
    } else { v[0] = (int32_t)B[0]; v[1] = (int32_t)B[1]; v[2] = (int32_t)B[2]; v[3] = (int32_t)B[3]; }
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) if (i >= cnt) v[i] = 0;
}
/* one element by loads of its own bytes */
__device__ __forceinline__ int32_t ly_load1(const uint8_t *q, uint32_t fmt)
{
    if (fmt == LINNE_AMD_PCM_S16) return *(const int16_t *)q;
    if (fmt == LINNE_AMD_PCM_S24) return (int32_t)(((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16)) << 8) >> 8;
    return *(const int32_t *)q;
}

#endif
