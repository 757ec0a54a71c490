/* lnn_host.h -- internal declarations of the host C side of liblinne_amd.so */
#ifndef LNN_HOST_H_INCLUDED
#define LNN_HOST_H_INCLUDED

#include <stdint.h>
#include "linne_amd.h"
#include "lnn_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* block types (libs/linne_internal/include/linne_internal.h:47-52) */
#define LNN_BLOCK_COMPRESS 0u
#define LNN_BLOCK_SILENT   1u
#define LNN_BLOCK_RAW      2u

struct lnn_layers {
    uint32_t num_layers, size[LINNE_AMD_MAX_LAYERS], offset[LINNE_AMD_MAX_LAYERS], total, max_size;
    uint32_t num_regs; double regs[4];
};

#define LNN_MAX_DEVICES 16
/* "0,1,2" -> device list (lnn_multi.c); returns the count, 0 when text is NULL or empty */
uint32_t lnn_parse_device_list(const char *text, int *devices, uint32_t max);

void lnn_tables_init(void);
uint16_t lnn_crc16(const uint8_t *data, uint64_t size);
int lnn_shape_layers(const struct LINNEAmdShape *shape, struct lnn_layers *out);
uint32_t lnn_decide_block_type(const struct LINNEAmdShape *shape, const struct lnn_layers *ly, uint32_t n,
        const int32_t *pcm_frame, const double *stats_frame, double *state);
void lnn_parallel_for(uint32_t count, uint32_t num_threads, void (*fn)(void *arg, uint32_t first, uint32_t count), void *arg);
int lnn_parse_block(const struct LINNEAmdShape *shape, const struct lnn_layers *ly, const uint8_t *data, uint64_t avail,
        int check_crc, uint32_t max_samples, uint32_t *type_out, uint32_t *n_out, uint32_t *consumed_out,
        int32_t *samples, int32_t *params);

int lnn_parse_block_head(const struct LINNEAmdShape *shape, const struct lnn_layers *ly, const uint8_t *data, uint64_t avail,
        int check_crc, uint32_t max_samples, uint32_t *type_out, uint32_t *n_out, uint32_t *consumed_out,
        int32_t *samples, int32_t *params, uint64_t *rice_bit_out);

/* the tables of the stream decoder on the device (LINNEAmd_StreamIndexCreate): the byte table of lnn_crc16 (CRC-16/ARC) and the
 * static Huffman tree of the coefficients as huff_init builds it (nodes below 256 are symbols) */
void lnn_stream_tables(uint16_t crc[256], uint32_t *huff_root, uint16_t huff_child[512][2]);
/* the encoder's side of that Huffman code: each symbol's code word (its low len[sym] bits, MSB first) and length */
void lnn_huff_code_table(uint32_t code[256], uint8_t len[256]);

/* the stream encoder on the device (LINNEAmd_EncodeStreamDevice): block types from per-frame silence flags, and the host's Rice plan
 * of the channel-frames the device could not settle (lnn_entropy.c) */
int lnn_decide_block_types(const struct LINNEAmdShape *shape, const uint32_t *num_samples, uint32_t num_frames, const double *stats,
        const uint8_t *nonzero, uint8_t *types, double *state);
int lnn_rice_plan_host(const int32_t *residual, uint64_t stride, const uint32_t *num_samples, uint32_t count, uint8_t *plans);

#ifdef __cplusplus
}
#endif

#endif
