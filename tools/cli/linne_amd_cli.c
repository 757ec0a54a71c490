/*
 * linne_amd_cli -- command line encoder/decoder on liblinne_amd.so.
 *
 * Same options and the same files as the reference's tools/linne_codec (linne_codec.c:15-33: -e -d -m -l -a -c -h -v,
 * INPUT OUTPUT), written from scratch with its own WAV reader/writer (wavio.c).  Differences, all additive:
 *   - whole streams go through LINNEEncoder_EncodeWhole / LINNEDecoder_DecodeWhole (pipelined over the GPU and the host
 *     threads; identical bytes); -B / --block-at-a-time walks LINNEEncoder_EncodeBlock like the reference tool does;
 *   - --batch DIR encodes (or decodes) every remaining argument into DIR with ONE handle, so the GPU context and the
 *     pinned staging slots are set up once (BASELINE config 4: many independent tracks);
 *   - -l and -a N are parsed and refused: the MI355X path does not offer them;
 *   - -r / --repair IN.lnn OUT.lnn repairs a damaged stream on the device (LINNEAmd_RepairStreamsDevice: sound blocks kept, lost
 *     stretches replaced by SILENT blocks), prints the report to stderr and exits 0 when the output was written;
 *   - -V / --verify (with -e) compares the encoded stream with the WAV's samples on the device (LINNEAmd_CompareWindowsDevice) before
 *     the output file is written, and writes nothing when they differ; -C / --compare STREAM.lnn PCM.wav does the same for a stream
 *     and a WAV file that exist: exit 0 and "identical", or exit 1 and the first differing sample;
 *   - -M / --measure [BUCKET] STREAM.lnn measures a stream on the device without decoding it into memory
 *     (LINNEAmd_MeasureWindowsDevice): per channel the minimum, maximum, exact sum and sum of squares, mean and RMS of the whole
 *     stream on stdout, or with BUCKET one such line per BUCKET samples and channel;
 *   - -D / --digest [BUCKET] STREAM.lnn digests a stream on the device without decoding it into memory
 *     (LINNEAmd_DigestWindowsDevice): "crc32 %08x bytes %llu" on stdout, the CRC-32 and length of the `data` chunk of the WAV file
 *     that -d writes for the stream, or with BUCKET one such line per BUCKET samples;
 *   - -S / --silence THRESHOLD[,MIN_SAMPLES] STREAM.lnn lists a stream's quiet runs on the device without decoding it into memory
 *     (LINNEAmd_QuietWindowsDevice): the stretches of at least MIN_SAMPLES (default 1) sample frames whose every channel stays within
 *     +-THRESHOLD, "run %llu: first %llu samples %llu seconds %.6f" per run on stdout, then "runs %llu quiet_samples %llu lead %llu
 *     trail %llu"; exit 0 when the stream decoded;
 *   - -L / --levels BINS[,SHIFT[,log2]] STREAM.lnn histograms a stream's sample levels on the device without decoding it into memory
 *     (LINNEAmd_HistogramWindowsDevice, the whole stream one bucket): bin min(x, BINS - 1) of x = |v| >> SHIFT, or with log2 of that
 *     value's bit length; "ch %u bin %u %llu..%llu %llu" per channel and non-empty bin on stdout -- the lowest and the highest |v| of the
 *     bin, "inf" for the last bin's, and the count -- then "samples %llu"; exit 0 when the stream decoded;
 *   - -R / --relate [BUCKET] STREAM.lnn relates a stream's channels on the device without decoding it into memory
 *     (LINNEAmd_RelateWindowsDevice): per channel pair i <= j "pair %u %u: samples %llu dot %s equal %llu opposite %llu correlation
 *     %.6f" on stdout -- the exact sum of a_i * a_j in decimal, the frames with a_i == a_j and with a_i == -a_j, and
 *     dot_ij / sqrt(dot_ii * dot_jj) ("nan" where a channel has no energy) -- followed by " identical" or " inverted" where every
 *     frame says so, and "channel %u: silent" for a channel of zeros; with BUCKET one such group per BUCKET samples, every line
 *     behind "bucket %llu ";
 *   - -X / --remix SPEC IN.lnn OUT.lnn writes a new stream whose channels are an integer matrix of IN's, on the device
 *     (LINNEAmd_MixWindowsDevice into device PCM, clipped to the stream's bits, then LINNEAmd_EncodeStreamsDevice with IN's header and
 *     the matrix' row count as its channels; one channel does not inherit MS).  SPEC: the rows separated by '/', a row's coefficients (int16) by ',', then optionally
 *     ">>SHIFT" (0 .. 31, halves round up): "1,1>>1" the mean of a stereo pair, "0,1/1,0" a channel swap.
 *   - -Z / --resample RATE[,TAPS] IN.lnn OUT.lnn writes IN at the sampling rate RATE, on the device (LINNEAmd_ResampleDesign's filter of
 *     TAPS coefficients per phase, 32 unless given; LINNEAmd_ResampleWindowsDevice into device PCM, clipped to the stream's bits; then
 *     LINNEAmd_EncodeStreamsDevice with IN's header but for the rate and the sample count): what Context.resample_streams writes.
 *   - -J / --join OTHER.lnn[,OVERLAP] IN.lnn OUT.lnn writes IN followed by OTHER, crossfaded over OVERLAP samples (0 unless given: a hard
 *     cut), on the device (LINNEAmd_OverlayWindowsDevice into device PCM -- the last OVERLAP samples of IN under a gain falling from
 *     16384, the first OVERLAP of OTHER under the one rising to it, shift 14, clipped to IN's bits --, then LINNEAmd_EncodeStreamsDevice
 *     with IN's header but for the sample count): what Context.crossfade_streams writes.
 *   - -A / --align OTHER.lnn[,MAX_LAG[,FIRST,N]] IN.lnn prints the lag at which OTHER best matches IN, per channel the two share and for
 *     all of them together, on the device (one LINNEAmd_LagWindowsDevice probe at the lags -MAX_LAG .. MAX_LAG, 4096 unless given; the
 *     needle N samples of IN from FIRST on, unless given the whole stream cut to the call's products limit): what Context.align_streams
 *     returns, compared as exactly.
 *   - -F / --spectrum N_FFT[,HOP[,FIRST,N]] IN.lnn prints the exact power spectrum of IN, a line per bin: the bin, its frequency in Hz and
 *     per channel the sum over the frames of re^2 + im^2 as an unsigned 128-bit decimal (LINNEAmd_ProjectDesign's Hann basis of all
 *     N_FFT / 2 + 1 bins, LINNEAmd_ProjectWindowsDevice on frames centred HOP apart -- N_FFT / 4 unless given --, shift 15, over the
 *     frames that begin in the N samples from FIRST on, the whole stream unless given): what Context.spectrum_streams returns.
 */
#include "linne_decoder.h"
#include "linne_encoder.h"
#include "linne_amd.h"
#include "wavio.h"

#include <hip/hip_runtime_api.h>

#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

struct options {
    int encode, decode, repair, verify, compare, measure, digest, silence, levels, relate, remix, resample, join, align, spectrum, no_crc, learning, block_at_a_time, help, version, quiet;
    long mode, af_iterations;
    const char *batch_dir, *silence_spec, *levels_spec, *remix_spec, *resample_spec, *join_spec, *align_spec, *spectrum_spec;
    const char *files[4096];
    int num_files;
};

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

static void usage(const char *argv0)
{
    printf("Usage: %s [options] INPUT_FILE_NAME OUTPUT_FILE_NAME \n", argv0);
    printf("       %s [options] --batch OUTPUT_DIRECTORY INPUT_FILE_NAME... \n", argv0);
    printf("       %s -C STREAM.lnn PCM.wav \n", argv0);
    printf("       %s -M [BUCKET_SAMPLES] STREAM.lnn \n", argv0);
    printf("       %s -D [BUCKET_SAMPLES] STREAM.lnn \n", argv0);
    printf("       %s -S THRESHOLD[,MIN_SAMPLES] STREAM.lnn \n", argv0);
    printf("       %s -L BINS[,SHIFT[,log2]] STREAM.lnn \n", argv0);
    printf("       %s -R [BUCKET_SAMPLES] STREAM.lnn \n", argv0);
    printf("       %s -X ROW[/ROW...][>>SHIFT] IN.lnn OUT.lnn \n", argv0);
    printf("       %s -Z RATE[,TAPS] IN.lnn OUT.lnn \n", argv0);
    printf("       %s -J OTHER.lnn[,OVERLAP] IN.lnn OUT.lnn \n", argv0);
    printf("options: \n"
           "  -e, --encode                           Encode mode \n"
           "  -d, --decode                           Decode mode \n"
           "  -r, --repair                           Repair a damaged .lnn stream into a valid one (report on stderr) \n"
           "  -V, --verify                           With -e: compare the stream with the input's samples on the device before writing it \n"
           "  -C, --compare                          Compare a .lnn stream with a WAV file's samples on the device (exit 0: identical) \n"
           "  -M, --measure                          Measure a .lnn stream on the device: min, max, sum, energy, mean, RMS per channel (and bucket) \n"
           "  -D, --digest                           Digest a .lnn stream on the device: the CRC-32 of the decoded PCM as -d writes it (per bucket) \n"
           "  -S, --silence THRESHOLD[,MIN_SAMPLES]  List a .lnn stream's quiet runs on the device: every channel within +-THRESHOLD \n"
           "  -L, --levels BINS[,SHIFT[,log2]]       Histogram a .lnn stream's sample levels on the device: |v| >> SHIFT, or its bit length \n"
           "  -R, --relate                           Relate a .lnn stream's channels on the device: dot products, equal and opposite frames, correlation per pair (and bucket) \n"
           "  -X, --remix ROW[/ROW...][>>SHIFT]      Write a .lnn stream whose channels are an integer matrix of the input's: rows of C coefficients \n"
           "  -Z, --resample RATE[,TAPS]             Write a .lnn stream at the sampling rate RATE: an exact polyphase FIR of TAPS (32) coefficients per phase \n"
           "  -J, --join OTHER.lnn[,OVERLAP]         Write IN followed by OTHER.lnn, crossfaded over OVERLAP (0) samples \n"
           "  -A, --align OTHER.lnn[,MAX_LAG[,FIRST,N]]  Print the lag at which OTHER.lnn best matches IN (-A OTHER.lnn[,MAX_LAG[,FIRST,N]] IN.lnn): \n"
           "                                         lags -MAX_LAG .. MAX_LAG (4096), the needle N samples of IN from FIRST on \n"
           "  -F, --spectrum N_FFT[,HOP[,FIRST,N]]   Print the exact power spectrum of IN (-F N_FFT[,HOP[,FIRST,N]] IN.lnn): per bin its frequency and, per channel, \n"
           "                                         the sum of re^2 + im^2 over the Hann frames HOP (N_FFT / 4) apart that begin in N samples from FIRST on \n"
           "  -m, --mode N                           Specify compress mode: 0(fast), ..., 7(high compression) (default:0) \n"
           "  -l, --enable-learning                  (not offered by the MI355X path) \n"
           "  -a, --auxiliary-function-iteration N   (not offered by the MI355X path unless N is 0) \n"
           "  -c, --no-crc-check                     Whether to NOT check CRC16 at decoding (default:no) \n"
           "  -B, --block-at-a-time                  Encode block by block (LINNEEncoder_EncodeBlock), as the reference tool does \n"
           "      --batch DIR                        Process every input into DIR with one handle (names keep their stem) \n"
           "  -q, --quiet                            No progress or summary lines \n"
           "  -h, --help                             Show command help message \n"
           "  -v, --version                          Show version information \n");
}

/* option with a value: "-m 7", "-m7", "--mode 7", "--mode=7" */
static int take_value(int argc, char **argv, int *i, const char *shortopt, const char *longopt, const char **value)
{
    const char *a = argv[*i];
    const size_t ll = strlen(longopt);
    if (strcmp(a, shortopt) == 0 || strcmp(a, longopt) == 0) {
        if (*i + 1 >= argc) { fprintf(stderr, "%s needs a value. \n", a); exit(1); }
        *value = argv[++*i];
        return 1;
    }
    if (strncmp(a, longopt, ll) == 0 && a[ll] == '=') { *value = a + ll + 1; return 1; }
    if (shortopt[0] && strncmp(a, shortopt, 2) == 0 && a[1] != '-' && a[2] != '\0') { *value = a + 2; return 1; }
    return 0;
}

static void parse(int argc, char **argv, struct options *o)
{
    int i;
    memset(o, 0, sizeof(*o));
    for (i = 1; i < argc; i++) {
        const char *a = argv[i], *v = NULL;
        if (strcmp(a, "-e") == 0 || strcmp(a, "--encode") == 0) o->encode = 1;
        else if (strcmp(a, "-d") == 0 || strcmp(a, "--decode") == 0) o->decode = 1;
        else if (strcmp(a, "-r") == 0 || strcmp(a, "--repair") == 0) o->repair = 1;
        else if (strcmp(a, "-V") == 0 || strcmp(a, "--verify") == 0) o->verify = 1;
        else if (strcmp(a, "-C") == 0 || strcmp(a, "--compare") == 0) o->compare = 1;
        else if (strcmp(a, "-M") == 0 || strcmp(a, "--measure") == 0) o->measure = 1;
        else if (strcmp(a, "-R") == 0 || strcmp(a, "--relate") == 0) o->relate = 1;
        else if (strcmp(a, "-D") == 0 || strcmp(a, "--digest") == 0) o->digest = 1;
        else if (strcmp(a, "-c") == 0 || strcmp(a, "--no-crc-check") == 0) o->no_crc = 1;
        else if (strcmp(a, "-l") == 0 || strcmp(a, "--enable-learning") == 0) o->learning = 1;
        else if (strcmp(a, "-B") == 0 || strcmp(a, "--block-at-a-time") == 0) o->block_at_a_time = 1;
        else if (strcmp(a, "-q") == 0 || strcmp(a, "--quiet") == 0) o->quiet = 1;
        else if (strcmp(a, "-h") == 0 || strcmp(a, "--help") == 0) o->help = 1;
        else if (strcmp(a, "-v") == 0 || strcmp(a, "--version") == 0) o->version = 1;
        else if (take_value(argc, argv, &i, "-m", "--mode", &v)) {
            char *end; o->mode = strtol(v, &end, 10);
            if (*end != '\0' || o->mode < 0 || o->mode >= LINNE_NUM_PARAMETER_PRESETS) { fprintf(stderr, "%s: Encode preset number is out of range. \n", argv[0]); exit(1); }
        } else if (take_value(argc, argv, &i, "-a", "--auxiliary-function-iteration", &v)) {
            char *end; o->af_iterations = strtol(v, &end, 10);
            if (*end != '\0' || o->af_iterations < 0 || o->af_iterations > 255) { fprintf(stderr, "%s: auxiliary function iteration count is out of range. \n", argv[0]); exit(1); }
        } else if (take_value(argc, argv, &i, "-S", "--silence", &v)) { o->silence = 1; o->silence_spec = v; }
        else if (take_value(argc, argv, &i, "-L", "--levels", &v)) { o->levels = 1; o->levels_spec = v; }
        else if (take_value(argc, argv, &i, "-X", "--remix", &v)) { o->remix = 1; o->remix_spec = v; }
        else if (take_value(argc, argv, &i, "-Z", "--resample", &v)) { o->resample = 1; o->resample_spec = v; }
        else if (take_value(argc, argv, &i, "-J", "--join", &v)) { o->join = 1; o->join_spec = v; }
        else if (take_value(argc, argv, &i, "-A", "--align", &v)) { o->align = 1; o->align_spec = v; }
        else if (take_value(argc, argv, &i, "-F", "--spectrum", &v)) { o->spectrum = 1; o->spectrum_spec = v; }
        else if (take_value(argc, argv, &i, "", "--batch", &v)) o->batch_dir = v;
        else if (a[0] == '-' && a[1] != '\0') { fprintf(stderr, "%s: unknown option %s \n", argv[0], a); exit(1); }
        else if (o->num_files < (int)(sizeof(o->files) / sizeof(o->files[0]))) o->files[o->num_files++] = a;
        else { fprintf(stderr, "%s: too many files. \n", argv[0]); exit(1); }
    }
}

/* DIR/stem.ext for a batch item */
static void batch_name(char *dst, size_t cap, const char *dir, const char *input, const char *ext)
{
    const char *base = strrchr(input, '/');
    const char *dot;
    size_t stem;
    base = base ? base + 1 : input;
    dot = strrchr(base, '.');
    stem = dot ? (size_t)(dot - base) : strlen(base);
    snprintf(dst, cap, "%s/%.*s%s", dir, (int)stem, base, ext);
}

static int read_file(const char *path, uint8_t **data, uint32_t *size)
{
    FILE *fp = fopen(path, "rb");
    long n;
    if (!fp) return -1;
    if (fseek(fp, 0, SEEK_END) != 0 || (n = ftell(fp)) < 0 || fseek(fp, 0, SEEK_SET) != 0 || (unsigned long)n > 0xFFFFFFFFul) { fclose(fp); return -1; }
    if (!(*data = malloc(n ? (size_t)n : 1))) { fclose(fp); return -1; }
    if (fread(*data, 1, (size_t)n, fp) != (size_t)n) { fclose(fp); free(*data); return -1; }
    fclose(fp);
    *size = (uint32_t)n;
    return 0;
}

/* A whole stream resident on the device 0, as -V, -C, -M, -D, -S, -L and -R want it: a context, the stream's bytes, its block index, `extra` bytes
 * beside it for what the call reads or writes, and the one window over all its samples */
struct resident {
    struct LINNEAmdContext *ctx;
    struct LINNEAmdStreamIndex *index;
    void *d_stream, *d_extra;
    struct LINNEAmdWindow w;
};
/* 0, or the stage that failed with its text in err: 1 the context, 2 the copies (`what` went to the device), 3 the index */
static int resident_open(struct resident *r, const uint8_t *stream, uint32_t size, uint64_t num_samples, uint64_t extra, const char *what, char *err, size_t cap)
{
    int ret = LINNE_APIRESULT_OK;
    memset(r, 0, sizeof(*r));
    if (!(r->ctx = LINNEAmd_ContextCreate(0, 0))) { snprintf(err, cap, "Failed to create a device context."); return 1; }
    if (hipMalloc(&r->d_stream, size ? size : 1) != hipSuccess || hipMemcpy(r->d_stream, stream, size, hipMemcpyHostToDevice) != hipSuccess
            || hipMalloc(&r->d_extra, extra ? extra : 1) != hipSuccess) { snprintf(err, cap, "Failed to copy %s to the device.", what); return 2; }
    if (!(r->index = LINNEAmd_StreamIndexCreate(r->ctx, r->d_stream, size, &ret))) { snprintf(err, cap, "the stream does not index: %d (%s)", ret, LINNEAmd_GetLastError(r->ctx)); return 3; }
    r->w.index = r->index; r->w.d_stream = r->d_stream; r->w.first_sample = 0; r->w.num_samples = num_samples;
    return 0;
}
static void resident_close(struct resident *r)
{
    if (r->index) LINNEAmd_StreamIndexDestroy(r->index);
    if (r->d_extra) (void)hipFree(r->d_extra);
    if (r->d_stream) (void)hipFree(r->d_stream);
    if (r->ctx) LINNEAmd_ContextDestroy(r->ctx);
}

/* The stream and the WAV's int32 planes go to the device; LINNEAmd_StreamIndexCreate and one LINNEAmd_CompareWindowsDevice window over
 * the whole stream answer.  0: *diff is the answer; 1: the stream does not index or decode, or the device failed (text in err) */
static int device_compare(const uint8_t *stream, uint32_t size, const struct wav_pcm *wav, struct LINNEAmdDiff *diff, char *err, size_t cap)
{
    struct resident r;
    const uint64_t n = wav->num_samples, plane = n * sizeof(int32_t);
    uint32_t ch;
    int ret, rc = 1;
    memset(diff, 0, sizeof(*diff));
    if (resident_open(&r, stream, size, n, plane * wav->num_channels, "the stream and the samples", err, cap) != 0) goto done;
    for (ch = 0; ch < wav->num_channels; ch++)
        if (plane && hipMemcpy((uint8_t *)r.d_extra + ch * plane, wav->plane[ch], plane, hipMemcpyHostToDevice) != hipSuccess) { snprintf(err, cap, "Failed to copy the stream and the samples to the device."); goto done; }
    r.w.d_pcm = r.d_extra; r.w.pcm_stride = n;
    if ((ret = LINNEAmd_CompareWindowsDevice(r.ctx, &r.w, NULL, diff, 1, 0)) != LINNE_APIRESULT_OK) { snprintf(err, cap, "the stream does not decode: %d (%s)", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    rc = 0;
done:
    resident_close(&r);
    return rc;
}

/* is the stream's header the WAV's format?  (0: yes; otherwise the text says what is not) */
static int header_matches(const struct LINNEHeader *h, const struct wav_pcm *wav, char *err, size_t cap)
{
    if (h->num_channels == wav->num_channels && h->bits_per_sample == wav->bits_per_sample && h->sampling_rate == wav->sampling_rate && h->num_samples == wav->num_samples) return 0;
    snprintf(err, cap, "the stream holds %u channels, %u bits, %u Hz, %u samples; the WAV file %u channels, %u bits, %u Hz, %u samples",
            (unsigned)h->num_channels, (unsigned)h->bits_per_sample, (unsigned)h->sampling_rate, (unsigned)h->num_samples,
            wav->num_channels, wav->bits_per_sample, wav->sampling_rate, wav->num_samples);
    return 1;
}

/* the verdict of -V and -C on stderr; 0: identical */
static int report_compare(const uint8_t *stream, uint32_t size, const struct wav_pcm *wav)
{
    struct LINNEHeader h;
    struct LINNEAmdDiff diff;
    char err[512];
    LINNEApiResult ret;
    if ((ret = LINNEDecoder_DecodeHeader(stream, size, &h)) != LINNE_APIRESULT_OK) { fprintf(stderr, "verification failed: the stream's header does not decode: %d \n", ret); return 1; }
    if (header_matches(&h, wav, err, sizeof(err)) != 0 || device_compare(stream, size, wav, &diff, err, sizeof(err)) != 0) { fprintf(stderr, "verification failed: %s \n", err); return 1; }
    if (diff.num_differing) {
        fprintf(stderr, "verification failed: sample %llu channel %u (%llu elements differ) \n", (unsigned long long)diff.first_sample, diff.first_channel, (unsigned long long)diff.num_differing);
        return 1;
    }
    return 0;
}

/* -C: a stream and a WAV file that exist */
static int compare_one(const char *lnn_path, const char *wav_path)
{
    uint8_t *buf = NULL;
    uint32_t size = 0;
    struct wav_pcm wav;
    char err[256];
    int rc;
    if (read_file(lnn_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", lnn_path); return 1; }
    if (wav_read(wav_path, &wav, err, sizeof(err)) != 0) { fprintf(stderr, "Failed to open %s. (%s) \n", wav_path, err); free(buf); return 1; }
    rc = report_compare(buf, size, &wav);
    if (rc == 0) printf("identical \n");
    free(buf); wav_free(&wav);
    return rc;
}

/* -M: the stream goes to the device; LINNEAmd_StreamIndexCreate and one LINNEAmd_MeasureWindowsDevice window over the whole stream
 * answer, and the table comes back: a line per channel, or with a bucket per bucket and channel */
static int measure_one(const char *lnn_path, uint64_t bucket)
{
    uint8_t *buf = NULL;
    uint32_t size = 0, ch;
    struct resident r;
    struct LINNEAmdMeasureSpec spec;
    struct LINNEAmdMeasure *tab = NULL;
    struct LINNEHeader h;
    char err[512];
    uint64_t n, nb, k;
    int ret, stage, rc = 1;
    if (read_file(lnn_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", lnn_path); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); free(buf); return 1; }
    n = h.num_samples;
    nb = n == 0 ? 0 : (bucket == 0 || bucket >= n) ? 1 : (n + bucket - 1) / bucket;
    if ((stage = resident_open(&r, buf, size, n, sizeof(*tab) * nb * h.num_channels, "the stream", err, sizeof(err))) != 0) { fprintf(stderr, stage == 3 ? "Failed to measure! %s \n" : "%s \n", err); goto done; }
    memset(&spec, 0, sizeof(spec));
    spec.bucket_samples = bucket; spec.d_out = r.d_extra; spec.channel_stride = nb;
    if ((ret = LINNEAmd_MeasureWindowsDevice(r.ctx, &r.w, &spec, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to measure! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    if (!(tab = malloc(nb ? sizeof(*tab) * nb * h.num_channels : 1)) || (nb && hipMemcpy(tab, r.d_extra, sizeof(*tab) * nb * h.num_channels, hipMemcpyDeviceToHost) != hipSuccess)) { fprintf(stderr, "Failed to fetch the table. \n"); goto done; }
    for (k = 0; k < nb; k++)
        for (ch = 0; ch < h.num_channels; ch++) {
            const struct LINNEAmdMeasure *m = tab + ch * nb + k;
            const uint64_t first = bucket ? k * bucket : 0, cnt = (bucket && first + bucket < n) ? bucket : n - first;
            const double energy = ldexp((double)m->sumsq_hi, 64) + (double)m->sumsq_lo;
            if (bucket) printf("bucket %llu ", (unsigned long long)k);
            printf("channel %u: samples %llu min %d max %d sum %lld sumsq_hi %llu sumsq_lo %llu mean %.6f rms %.6f \n", ch, (unsigned long long)cnt, m->min, m->max,
                    (long long)m->sum, (unsigned long long)m->sumsq_hi, (unsigned long long)m->sumsq_lo, (double)m->sum / (double)cnt, sqrt(energy / (double)cnt));
        }
    rc = 0;
done:
    resident_close(&r);
    free(tab); free(buf);
    return rc;
}

/* -D: the stream goes to the device; LINNEAmd_StreamIndexCreate and one LINNEAmd_DigestWindowsDevice window over the whole stream
 * answer, and the table comes back: one line, or with a bucket one line per bucket */
static int digest_one(const char *lnn_path, uint64_t bucket)
{
    uint8_t *buf = NULL;
    uint32_t size = 0;
    struct resident r;
    struct LINNEAmdDigestSpec spec;
    struct LINNEAmdDigest *tab = NULL;
    struct LINNEHeader h;
    char err[512];
    uint64_t n, nb, k;
    int ret, stage, rc = 1;
    if (read_file(lnn_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", lnn_path); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); free(buf); return 1; }
    n = h.num_samples;
    nb = n == 0 ? 0 : (bucket == 0 || bucket >= n) ? 1 : (n + bucket - 1) / bucket;
    if ((stage = resident_open(&r, buf, size, n, sizeof(*tab) * nb, "the stream", err, sizeof(err))) != 0) { fprintf(stderr, stage == 3 ? "Failed to digest! %s \n" : "%s \n", err); goto done; }
    memset(&spec, 0, sizeof(spec));
    spec.bucket_samples = bucket; spec.d_out = r.d_extra;
    if ((ret = LINNEAmd_DigestWindowsDevice(r.ctx, &r.w, &spec, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to digest! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    if (!(tab = malloc(nb ? sizeof(*tab) * nb : 1)) || (nb && hipMemcpy(tab, r.d_extra, sizeof(*tab) * nb, hipMemcpyDeviceToHost) != hipSuccess)) { fprintf(stderr, "Failed to fetch the table. \n"); goto done; }
    /* (a stream of no samples has the empty string's digest) */
    if (nb == 0) printf("crc32 %08x bytes %llu \n", 0u, 0ull);
    for (k = 0; k < nb; k++) printf("crc32 %08x bytes %llu \n", tab[k].crc32, (unsigned long long)tab[k].num_bytes);
    rc = 0;
done:
    resident_close(&r);
    free(tab); free(buf);
    return rc;
}

/* -S: the stream goes to the device; LINNEAmd_StreamIndexCreate and LINNEAmd_QuietWindowsDevice over the whole stream answer, first
 * with no table (the count), then with a table of exactly that many records, which comes back: a line per run and the summary */
static int silence_one(const char *lnn_path, uint32_t threshold, uint64_t min_samples)
{
    uint8_t *buf = NULL;
    uint32_t size = 0;
    struct resident r;
    struct LINNEAmdQuietSpec spec;
    struct LINNEAmdQuiet q;
    struct LINNEAmdRun *tab = NULL;
    void *d_tab = NULL;
    struct LINNEHeader h;
    char err[512];
    uint64_t k;
    int ret, stage, rc = 1;
    if (read_file(lnn_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", lnn_path); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); free(buf); return 1; }
    if ((stage = resident_open(&r, buf, size, h.num_samples, 0, "the stream", err, sizeof(err))) != 0) { fprintf(stderr, stage == 3 ? "Failed to find the silence! %s \n" : "%s \n", err); goto done; }
    memset(&spec, 0, sizeof(spec)); memset(&q, 0, sizeof(q));
    spec.threshold = threshold; spec.min_samples = min_samples;
    if ((ret = LINNEAmd_QuietWindowsDevice(r.ctx, &r.w, &spec, &q, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to find the silence! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    if (q.num_runs) {
        if (hipMalloc(&d_tab, sizeof(*tab) * q.num_runs) != hipSuccess) { fprintf(stderr, "Failed to allocate %llu records on the device. \n", (unsigned long long)q.num_runs); d_tab = NULL; goto done; }
        spec.d_out = d_tab; spec.capacity = q.num_runs;
        if ((ret = LINNEAmd_QuietWindowsDevice(r.ctx, &r.w, &spec, &q, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to find the silence! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
        if (q.num_runs != spec.capacity || !(tab = malloc(sizeof(*tab) * q.num_runs)) || hipMemcpy(tab, d_tab, sizeof(*tab) * q.num_runs, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "Failed to fetch the table. \n"); goto done; }
    }
    for (k = 0; k < q.num_runs; k++)
        printf("run %llu: first %llu samples %llu seconds %.6f \n", (unsigned long long)k, (unsigned long long)tab[k].first_sample, (unsigned long long)tab[k].num_samples,
                h.sampling_rate ? (double)tab[k].num_samples / (double)h.sampling_rate : 0.0);
    printf("runs %llu quiet_samples %llu lead %llu trail %llu \n", (unsigned long long)q.num_runs, (unsigned long long)q.quiet_samples, (unsigned long long)q.lead_samples, (unsigned long long)q.trail_samples);
    rc = 0;
done:
    if (d_tab) (void)hipFree(d_tab);
    resident_close(&r);
    free(tab); free(buf);
    return rc;
}

static int encode_one(struct LINNEEncoder *enc, const struct options *o, const char *in_path, const char *out_path)
{
    struct wav_pcm wav;
    struct LINNEEncodeParameter par;
    char err[256];
    uint8_t *buf = NULL;
    uint64_t cap;
    uint32_t out_size = 0;
    LINNEApiResult ret;
    FILE *fp;
    const double t0 = now_s();
    if (wav_read(in_path, &wav, err, sizeof(err)) != 0) { fprintf(stderr, "Failed to open %s. (%s) \n", in_path, err); return 1; }
    if (wav.num_channels > LINNE_MAX_NUM_CHANNELS) { fprintf(stderr, "%s: %u channels, at most %d are supported. \n", in_path, wav.num_channels, LINNE_MAX_NUM_CHANNELS); wav_free(&wav); return 1; }
    par.num_channels = (uint16_t)wav.num_channels; par.bits_per_sample = (uint16_t)wav.bits_per_sample; par.sampling_rate = wav.sampling_rate;
    par.num_samples_per_block = 5 * 2048;                          /* linne_codec.c:75-76 */
    par.ch_process_method = (wav.num_channels >= 2) ? LINNE_CH_PROCESS_METHOD_MS : LINNE_CH_PROCESS_METHOD_NONE;
    par.preset = (uint8_t)o->mode; par.enable_learning = (uint8_t)o->learning; par.num_afmethod_iterations = (uint8_t)o->af_iterations;
    if ((ret = LINNEEncoder_SetEncodeParameter(enc, &par)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to set encode parameter: %d \n", ret); wav_free(&wav); return 1; }
    cap = 2ull * ((uint64_t)wav.num_samples * wav.num_channels * (wav.bits_per_sample / 8) + 44) + 65536;     /* "twice the input", linne_codec.c:93-95 */
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    if (!(buf = malloc((size_t)cap))) { fprintf(stderr, "out of memory \n"); wav_free(&wav); return 1; }
    if (!o->block_at_a_time) {
        ret = LINNEEncoder_EncodeWhole(enc, (const int32_t *const *)wav.plane, wav.num_samples, buf, (uint32_t)cap, &out_size);
        if (ret != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to encode! ret:%d \n", ret); free(buf); wav_free(&wav); return 1; }
    } else {
        struct LINNEHeader h;
        uint32_t progress = 0, ch;
        memset(&h, 0, sizeof(h));
        h.num_channels = par.num_channels; h.num_samples = wav.num_samples; h.sampling_rate = par.sampling_rate; h.bits_per_sample = par.bits_per_sample;
        h.num_samples_per_block = par.num_samples_per_block; h.preset = par.preset; h.ch_process_method = par.ch_process_method;
        if ((ret = LINNEEncoder_EncodeHeader(&h, buf, (uint32_t)cap)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to encode header! ret:%d \n", ret); free(buf); wav_free(&wav); return 1; }
        out_size = LINNE_HEADER_SIZE;
        while (progress < wav.num_samples) {
            const int32_t *ptr[LINNE_MAX_NUM_CHANNELS];
            const uint32_t n = (wav.num_samples - progress < par.num_samples_per_block) ? (wav.num_samples - progress) : par.num_samples_per_block;
            uint32_t wrote = 0;
            for (ch = 0; ch < wav.num_channels; ch++) ptr[ch] = wav.plane[ch] + progress;
            if ((ret = LINNEEncoder_EncodeBlock(enc, ptr, n, buf + out_size, (uint32_t)cap - out_size, &wrote)) != LINNE_APIRESULT_OK) {
                fprintf(stderr, "Failed to encode! ret:%d \n", ret); free(buf); wav_free(&wav); return 1;
            }
            out_size += wrote; progress += n;
            if (!o->quiet) { printf("progress... %5.2f%% \r", (progress * 100.0f) / wav.num_samples); fflush(stdout); }
        }
    }
    if (o->verify && report_compare(buf, out_size, &wav) != 0) { free(buf); wav_free(&wav); return 1; }      /* nothing is written */
    if (!(fp = fopen(out_path, "wb")) || fwrite(buf, 1, out_size, fp) != out_size) { fprintf(stderr, "File output error! %s \n", out_path); if (fp) fclose(fp); free(buf); wav_free(&wav); return 1; }
    fclose(fp);
    if (!o->quiet) {
        const uint64_t in_bytes = (uint64_t)wav.num_samples * wav.num_channels * (wav.bits_per_sample / 8) + 44;
        printf("finished: %llu -> %u (%6.2f %%) in %.3f s%s \n", (unsigned long long)in_bytes, out_size, 100.0 * (double)out_size / (double)in_bytes, now_s() - t0, o->verify ? ", verified" : "");
    }
    free(buf); wav_free(&wav);
    return 0;
}

static int decode_one(struct LINNEDecoder *dec, const struct options *o, const char *in_path, const char *out_path)
{
    uint8_t *buf = NULL;
    uint32_t size = 0;
    struct LINNEHeader h;
    struct wav_pcm wav;
    char err[256];
    LINNEApiResult ret;
    const double t0 = now_s();
    if (read_file(in_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", in_path); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); free(buf); return 1; }
    memset(&wav, 0, sizeof(wav));
    wav.num_channels = h.num_channels; wav.sampling_rate = h.sampling_rate; wav.bits_per_sample = h.bits_per_sample; wav.num_samples = h.num_samples;
    if (wav_alloc(&wav) != 0) { fprintf(stderr, "Failed to create wav handle. \n"); free(buf); wav_free(&wav); return 1; }
    if ((ret = LINNEDecoder_DecodeWhole(dec, buf, size, wav.plane, wav.num_channels, wav.num_samples)) != LINNE_APIRESULT_OK) {
        fprintf(stderr, "Decoding error! %d \n", ret); free(buf); wav_free(&wav); return 1;
    }
    if (wav_write(out_path, &wav, err, sizeof(err)) != 0) { fprintf(stderr, "Failed to write wav file. (%s) \n", err); free(buf); wav_free(&wav); return 1; }
    if (!o->quiet) printf("finished: %u -> %llu in %.3f s \n", size, (unsigned long long)wav.num_samples * wav.num_channels * (wav.bits_per_sample / 8) + 44, now_s() - t0);
    free(buf); wav_free(&wav);
    return 0;
}

/* -r: the stream goes to the device, LINNEAmd_RepairStreamsDevice repairs it there, the result comes back */
static int repair_one(const char *in_path, const char *out_path)
{
    uint8_t *buf = NULL, *out = NULL;
    void *d_in = NULL, *d_out = NULL;
    uint32_t size = 0, i, ngaps = 0;
    struct LINNEHeader h;
    struct LINNEAmdContext *ctx = NULL;
    struct LINNEAmdRepair rep;
    const struct LINNEAmdGap *gaps = NULL;
    uint64_t cap;
    FILE *fp;
    int ret, rc = 1, pass;
    if (read_file(in_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", in_path); return 1; }
    cap = (uint64_t)size + 22;
    if (LINNEDecoder_DecodeHeader(buf, size, &h) == LINNE_APIRESULT_OK && h.num_samples_per_block > 0) {
        const uint32_t full = h.num_samples_per_block < 65535u ? h.num_samples_per_block : 65535u;
        cap = (uint64_t)size + 11ull * (h.num_samples / full + 2u);
    }
    if (!(ctx = LINNEAmd_ContextCreate(0, 0))) { fprintf(stderr, "Failed to create a device context. \n"); goto done; }
    if (hipMalloc(&d_in, size ? size : 1) != hipSuccess || hipMemcpy(d_in, buf, size, hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "Failed to copy the stream to the device. \n"); goto done; }
    memset(&rep, 0, sizeof(rep));
    for (pass = 0; pass < 2; pass++) {                             /* (a stream of many gaps may need more room: once more at its exact size) */
        if (hipMalloc(&d_out, cap) != hipSuccess) { fprintf(stderr, "Failed to allocate %llu bytes on the device. \n", (unsigned long long)cap); d_out = NULL; goto done; }
        rep.d_stream = d_in; rep.stream_bytes = size; rep.d_out = d_out; rep.capacity = cap;
        ret = LINNEAmd_RepairStreamsDevice(ctx, &rep, 1);
        if (ret != LINNE_APIRESULT_INSUFFICIENT_BUFFER || pass == 1) break;
        (void)hipFree(d_out); d_out = NULL; cap = rep.out_bytes;
    }
    if (ret != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to repair! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(ctx)); goto done; }
    if (!(out = malloc(rep.out_bytes ? (size_t)rep.out_bytes : 1)) || hipMemcpy(out, d_out, rep.out_bytes, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "Failed to fetch the repaired stream. \n"); goto done; }
    if (!(fp = fopen(out_path, "wb")) || fwrite(out, 1, (size_t)rep.out_bytes, fp) != rep.out_bytes) { fprintf(stderr, "File output error! %s \n", out_path); if (fp) fclose(fp); goto done; }
    fclose(fp);
    rc = 0;
    fprintf(stderr, "repaired: %u -> %llu bytes, kept blocks %u, fill blocks %u, gaps %u, lost samples %llu, exact %u \n", size, (unsigned long long)rep.out_bytes,
            rep.kept_blocks, rep.fill_blocks, rep.num_gaps, (unsigned long long)rep.lost_samples, rep.exact);
    if (LINNEAmd_GetLastRepairGaps(ctx, 0, &gaps, &ngaps) == LINNE_APIRESULT_OK)
        for (i = 0; i < ngaps; i++)
            fprintf(stderr, "gap %u: samples [%llu, %llu), source bytes [%llu, %llu), fill blocks %u \n", i, (unsigned long long)gaps[i].first_sample,
                    (unsigned long long)(gaps[i].first_sample + gaps[i].num_samples), (unsigned long long)gaps[i].src_offset,
                    (unsigned long long)(gaps[i].src_offset + gaps[i].src_bytes), gaps[i].fill_blocks);
done:
    if (d_out) (void)hipFree(d_out);
    if (d_in) (void)hipFree(d_in);
    if (ctx) LINNEAmd_ContextDestroy(ctx);
    free(out); free(buf);
    return rc;
}

/* -L: the stream goes to the device; LINNEAmd_StreamIndexCreate and one LINNEAmd_HistogramWindowsDevice window over the whole stream
 * in one bucket answer, and the table comes back: a line per channel and non-empty bin, then the sample count */
static int levels_one(const char *lnn_path, uint32_t bins, uint32_t shift, uint32_t scale)
{
    uint8_t *buf = NULL;
    uint32_t size = 0, ch, j;
    struct resident r;
    struct LINNEAmdHistogramSpec spec;
    uint64_t *tab = NULL;
    struct LINNEHeader h;
    char err[512];
    uint64_t n, nb;
    int ret, stage, rc = 1;
    if (read_file(lnn_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", lnn_path); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); free(buf); return 1; }
    n = h.num_samples;
    nb = n == 0 ? 0 : 1;
    if ((stage = resident_open(&r, buf, size, n, sizeof(*tab) * nb * bins * h.num_channels, "the stream", err, sizeof(err))) != 0) { fprintf(stderr, stage == 3 ? "Failed to histogram! %s \n" : "%s \n", err); goto done; }
    memset(&spec, 0, sizeof(spec));
    spec.num_bins = bins; spec.shift = shift; spec.scale = scale; spec.d_out = r.d_extra; spec.channel_stride = nb;
    if ((ret = LINNEAmd_HistogramWindowsDevice(r.ctx, &r.w, &spec, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to histogram! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    if (!(tab = malloc(nb ? sizeof(*tab) * bins * h.num_channels : 1)) || (nb && hipMemcpy(tab, r.d_extra, sizeof(*tab) * bins * h.num_channels, hipMemcpyDeviceToHost) != hipSuccess)) { fprintf(stderr, "Failed to fetch the table. \n"); goto done; }
    for (ch = 0; nb && ch < h.num_channels; ch++)
        for (j = 0; j < bins; j++) {
            /* bin j holds x == j: the values m = |v| >> shift in [mlo, mhi], |v| in [mlo << shift, ((mhi + 1) << shift) - 1] */
            const uint64_t cnt = tab[(uint64_t)ch * bins + j];
            const uint64_t mlo = scale == LINNE_AMD_HIST_LOG2 ? (j ? (uint64_t)1 << (j - 1u) : 0u) : j, mhi = scale == LINNE_AMD_HIST_LOG2 ? (j ? ((uint64_t)1 << j) - 1u : 0u) : j;
            if (!cnt) continue;
            printf("ch %u bin %u %llu..", ch, j, (unsigned long long)(mlo << shift));
            if (j == bins - 1u) printf("inf");
            else printf("%llu", (unsigned long long)(((mhi + 1u) << shift) - 1u));
            printf(" %llu \n", (unsigned long long)cnt);
        }
    printf("samples %llu \n", (unsigned long long)n);
    rc = 0;
done:
    resident_close(&r);
    free(tab); free(buf);
    return rc;
}

/* the 128-bit two's-complement integer hi * 2^64 + lo in decimal (at most 40 digits and a sign) */
static const char *decimal128(int64_t hi, uint64_t lo, char text[48])
{
    unsigned __int128 u = ((unsigned __int128)(uint64_t)hi << 64) | lo;
    const int neg = hi < 0;
    char *p = text + 47;
    if (neg) u = 0 - u;
    *p = '\0';
    do { *--p = (char)('0' + (int)(u % 10u)); u /= 10u; } while (u != 0);
    if (neg) *--p = '-';
    return p;
}

/* the same integer as a double: negated in integers first, so that a small negative sum (hi = -1, lo just below 2^64) does not cancel */
static double double128(int64_t hi, uint64_t lo)
{
    unsigned __int128 u = ((unsigned __int128)(uint64_t)hi << 64) | lo;
    const int neg = hi < 0;
    double mag;
    if (neg) u = 0 - u;
    mag = ldexp((double)(uint64_t)(u >> 64), 64) + (double)(uint64_t)u;
    return neg ? -mag : mag;
}

/* -R: the stream goes to the device; LINNEAmd_StreamIndexCreate and one LINNEAmd_RelateWindowsDevice window over the whole stream
 * answer, and the table comes back: a line per channel pair, or with a bucket per bucket and pair, and a line per silent channel */
static int relate_one(const char *lnn_path, uint64_t bucket)
{
    uint8_t *buf = NULL;
    uint32_t size = 0, i, j, C, P;
    struct resident r;
    struct LINNEAmdRelateSpec spec;
    struct LINNEAmdRelation *tab = NULL;
    struct LINNEHeader h;
    char err[512], text[48];
    uint64_t n, nb, k;
    int ret, stage, rc = 1;
    if (read_file(lnn_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", lnn_path); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); free(buf); return 1; }
    n = h.num_samples; C = h.num_channels; P = LINNE_AMD_NUM_PAIRS(C);
    nb = n == 0 ? 0 : (bucket == 0 || bucket >= n) ? 1 : (n + bucket - 1) / bucket;
    if ((stage = resident_open(&r, buf, size, n, sizeof(*tab) * nb * P, "the stream", err, sizeof(err))) != 0) { fprintf(stderr, stage == 3 ? "Failed to relate! %s \n" : "%s \n", err); goto done; }
    memset(&spec, 0, sizeof(spec));
    spec.bucket_samples = bucket; spec.d_out = r.d_extra; spec.pair_stride = nb;
    if ((ret = LINNEAmd_RelateWindowsDevice(r.ctx, &r.w, &spec, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to relate! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    if (!(tab = malloc(nb ? sizeof(*tab) * nb * P : 1)) || (nb && hipMemcpy(tab, r.d_extra, sizeof(*tab) * nb * P, hipMemcpyDeviceToHost) != hipSuccess)) { fprintf(stderr, "Failed to fetch the table. \n"); goto done; }
    for (k = 0; k < nb; k++) {
        const uint64_t cnt = tab[k].num_equal;                     /* pair (0, 0): every frame equals itself */
        for (i = 0; i < C; i++)
            for (j = i; j < C; j++) {
                const struct LINNEAmdRelation *m = tab + (uint64_t)LINNE_AMD_PAIR(C, i, j) * nb + k;
                const struct LINNEAmdRelation *a = tab + (uint64_t)LINNE_AMD_PAIR(C, i, i) * nb + k, *b = tab + (uint64_t)LINNE_AMD_PAIR(C, j, j) * nb + k;
                const double d = double128(m->dot_hi, m->dot_lo), ei = double128(a->dot_hi, a->dot_lo), ej = double128(b->dot_hi, b->dot_lo);
                if (bucket) printf("bucket %llu ", (unsigned long long)k);
                printf("pair %u %u: samples %llu dot %s equal %llu opposite %llu correlation ", i, j, (unsigned long long)cnt, decimal128(m->dot_hi, m->dot_lo, text),
                        (unsigned long long)m->num_equal, (unsigned long long)m->num_opposite);
                if (ei > 0.0 && ej > 0.0) printf("%.6f", d / sqrt(ei * ej));
                else printf("nan");
                if (i < j && m->num_equal == cnt) printf(" identical");
                else if (i < j && m->num_opposite == cnt && !(a->num_opposite == cnt && b->num_opposite == cnt)) printf(" inverted");
                printf(" \n");
            }
        for (i = 0; i < C; i++)
            if (tab[(uint64_t)LINNE_AMD_PAIR(C, i, i) * nb + k].num_opposite == cnt) {
                if (bucket) printf("bucket %llu ", (unsigned long long)k);
                printf("channel %u: silent \n", i);
            }
    }
    rc = 0;
done:
    resident_close(&r);
    free(tab); free(buf);
    return rc;
}

/* "1,1>>1", "0,1/1,0": rows by '/', coefficients by ',', an optional ">>shift" -> spec (out_channels the rows) and *cols, the length
 * every row has.  0, or a message in err */
static int parse_remix(const char *text, struct LINNEAmdMixSpec *spec, uint32_t *cols, char *err, size_t cap)
{
    const char *p = text;
    uint32_t o = 0, c = 0;
    memset(spec, 0, sizeof(*spec));
    *cols = 0;
    for (;;) {
        char *end;
        long v;
        if (!((*p >= '0' && *p <= '9') || ((*p == '-' || *p == '+') && p[1] >= '0' && p[1] <= '9'))) { snprintf(err, cap, "remix spec: a coefficient is expected at \"%s\"", p); return 1; }
        v = strtol(p, &end, 10);
        if (v < -32768 || v > 32767) { snprintf(err, cap, "remix spec: coefficient %ld is outside int16", v); return 1; }
        if (o >= LINNE_MAX_NUM_CHANNELS || c >= LINNE_MAX_NUM_CHANNELS) { snprintf(err, cap, "remix spec: more than %d rows or coefficients in a row", LINNE_MAX_NUM_CHANNELS); return 1; }
        spec->coef[o][c++] = (int16_t)v;
        p = end;
        if (*p == ',') { p++; continue; }
        if (o == 0) *cols = c;
        else if (c != *cols) { snprintf(err, cap, "remix spec: row %u has %u coefficients, row 0 has %u", o, c, *cols); return 1; }
        o++; c = 0;
        if (*p == '/') { p++; continue; }
        break;
    }
    spec->out_channels = o;
    if (p[0] == '>' && p[1] == '>' && p[2] >= '0' && p[2] <= '9') {
        char *end;
        const unsigned long sh = strtoul(p + 2, &end, 10);
        if (sh > 31) { snprintf(err, cap, "remix spec: shift %lu > 31", sh); return 1; }
        spec->shift = (uint32_t)sh;
        p = end;
    }
    if (*p != '\0') { snprintf(err, cap, "remix spec: malformed at \"%s\"", p); return 1; }
    return 0;
}

/* -X: the spec and the stream's header are checked on the host; then the stream goes to the device, LINNEAmd_StreamIndexCreate, one
 * LINNEAmd_MixWindowsDevice window over the whole stream into int32 planes beside it, and LINNEAmd_EncodeStreamsDevice make the output */
static int remix_one(const char *spec_text, const char *in_path, const char *out_path)
{
    uint8_t *buf = NULL, *out = NULL;
    void *d_out = NULL;
    uint32_t size = 0, cols = 0;
    struct resident r;
    struct LINNEAmdMixSpec spec;
    struct LINNEAmdTrack tr;
    struct LINNEHeader h;
    char err[512];
    uint64_t n, cap;
    FILE *fp;
    int ret, stage, rc = 1;
    memset(&r, 0, sizeof(r));
    if (parse_remix(spec_text, &spec, &cols, err, sizeof(err)) != 0) { fprintf(stderr, "%s \n", err); return 1; }
    if (read_file(in_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", in_path); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); free(buf); return 1; }
    if (cols != h.num_channels) { fprintf(stderr, "remix spec: its rows have %u coefficients, the stream has %u channels \n", cols, (unsigned)h.num_channels); free(buf); return 1; }
    n = h.num_samples;
    spec.clip_bits = h.bits_per_sample;
    if ((stage = resident_open(&r, buf, size, n, sizeof(int32_t) * n * spec.out_channels, "the stream", err, sizeof(err))) != 0) { fprintf(stderr, stage == 3 ? "Failed to remix! %s \n" : "%s \n", err); goto done; }
    r.w.d_pcm = r.d_extra; r.w.pcm_stride = n;
    if ((ret = LINNEAmd_MixWindowsDevice(r.ctx, &r.w, &spec, NULL, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to remix! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    memset(&tr, 0, sizeof(tr));
    tr.header = h; tr.header.num_channels = (uint16_t)spec.out_channels;
    if (spec.out_channels == 1) tr.header.ch_process_method = LINNE_CH_PROCESS_METHOD_NONE;    /* (one channel has no mid and side) */
    cap = LINNEAmd_EncodeStreamBound(&tr.header);
    if (hipMalloc(&d_out, cap ? cap : 1) != hipSuccess) { fprintf(stderr, "Failed to allocate %llu bytes on the device. \n", (unsigned long long)cap); d_out = NULL; goto done; }
    tr.d_pcm = r.d_extra; tr.pcm_stride = n; tr.d_out = d_out; tr.capacity = cap;
    if ((ret = LINNEAmd_EncodeStreamsDevice(r.ctx, &tr, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to encode! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    if (!(out = malloc(tr.out_bytes ? (size_t)tr.out_bytes : 1)) || hipMemcpy(out, d_out, tr.out_bytes, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "Failed to fetch the stream. \n"); goto done; }
    if (!(fp = fopen(out_path, "wb")) || fwrite(out, 1, (size_t)tr.out_bytes, fp) != tr.out_bytes) { fprintf(stderr, "File output error! %s \n", out_path); if (fp) fclose(fp); goto done; }
    fclose(fp);
    rc = 0;
done:
    if (d_out) (void)hipFree(d_out);
    resident_close(&r);
    free(out); free(buf);
    return rc;
}

/* "16000", "48000,64": the rate, then optionally the taps per phase -> *rate, *taps (32 unless given).  0, or a message in err */
static int parse_resample(const char *text, uint32_t *rate, uint32_t *taps, char *err, size_t cap)
{
    const char *p = text;
    char *end;
    unsigned long v;
    *taps = 32;
    if (!(*p >= '0' && *p <= '9')) { snprintf(err, cap, "resample spec: a sampling rate is expected at \"%s\"", p); return 1; }
    v = strtoul(p, &end, 10);
    if (v < 1 || v > 0xFFFFFFFFul) { snprintf(err, cap, "resample spec: sampling rate %lu is outside 1 .. 4294967295", v); return 1; }
    *rate = (uint32_t)v;
    p = end;
    if (*p == ',') {
        p++;
        if (!(*p >= '0' && *p <= '9')) { snprintf(err, cap, "resample spec: a tap count is expected at \"%s\"", p); return 1; }
        v = strtoul(p, &end, 10);
        if (v < 1 || v > LINNE_AMD_RESAMPLE_MAX_TAPS) { snprintf(err, cap, "resample spec: %lu taps are outside 1 .. %d", v, LINNE_AMD_RESAMPLE_MAX_TAPS); return 1; }
        *taps = (uint32_t)v;
        p = end;
    }
    if (*p != '\0') { snprintf(err, cap, "resample spec: malformed at \"%s\"", p); return 1; }
    return 0;
}
static uint32_t gcd32(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }

/* -Z: the spec and the stream's header are checked on the host and the filter designed there; then the stream goes to the device,
 * LINNEAmd_StreamIndexCreate, one LINNEAmd_ResampleWindowsDevice window over the whole resampled stream into int32 planes beside it, and
 * LINNEAmd_EncodeStreamsDevice make the output */
static int resample_one(const char *spec_text, const char *in_path, const char *out_path)
{
    uint8_t *buf = NULL, *out = NULL;
    int16_t *coef = NULL;
    void *d_out = NULL;
    uint32_t size = 0, rate = 0, taps = 0, g;
    struct resident r;
    struct LINNEAmdResampleSpec spec;
    struct LINNEAmdTrack tr;
    struct LINNEHeader h;
    char err[512];
    uint64_t n, cap, up, down;
    FILE *fp;
    int ret, stage, rc = 1;
    memset(&r, 0, sizeof(r));
    if (parse_resample(spec_text, &rate, &taps, err, sizeof(err)) != 0) { fprintf(stderr, "%s \n", err); return 1; }
    if (read_file(in_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", in_path); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); free(buf); return 1; }
    if (h.sampling_rate == 0) { fprintf(stderr, "resample spec: the stream names no sampling rate \n"); free(buf); return 1; }
    g = gcd32(h.sampling_rate, rate); up = rate / g; down = h.sampling_rate / g;
    memset(&spec, 0, sizeof(spec));
    if (up > LINNE_AMD_RESAMPLE_MAX_RATIO || down > LINNE_AMD_RESAMPLE_MAX_RATIO || up * taps > LINNE_AMD_RESAMPLE_MAX_COEFS) {
        fprintf(stderr, "resample spec: %u -> %u Hz is %llu/%llu with %u taps: beyond %d/%d or %d coefficients \n", (unsigned)h.sampling_rate, rate, (unsigned long long)up, (unsigned long long)down, taps,
                LINNE_AMD_RESAMPLE_MAX_RATIO, LINNE_AMD_RESAMPLE_MAX_RATIO, LINNE_AMD_RESAMPLE_MAX_COEFS);
        free(buf); return 1;
    }
    spec.up = (uint32_t)up; spec.down = (uint32_t)down; spec.taps = taps; spec.clip_bits = h.bits_per_sample;
    if (!(coef = malloc(sizeof(*coef) * up * taps)) || (ret = LINNEAmd_ResampleDesign(spec.up, spec.down, taps, coef, &spec.shift, &spec.before)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to design the filter: %d \n", coef ? ret : -1); goto done; }
    spec.coef = coef;
    n = LINNEAmd_ResampleLength(h.num_samples, spec.up, spec.down);
    if (n > 0xFFFFFFFFull) { fprintf(stderr, "resample spec: %llu samples are more than a header names \n", (unsigned long long)n); goto done; }
    if ((stage = resident_open(&r, buf, size, n, sizeof(int32_t) * n * h.num_channels, "the stream", err, sizeof(err))) != 0) { fprintf(stderr, stage == 3 ? "Failed to resample! %s \n" : "%s \n", err); goto done; }
    r.w.d_pcm = r.d_extra; r.w.pcm_stride = n;
    if ((ret = LINNEAmd_ResampleWindowsDevice(r.ctx, &r.w, &spec, NULL, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to resample! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    memset(&tr, 0, sizeof(tr));
    tr.header = h; tr.header.sampling_rate = rate; tr.header.num_samples = (uint32_t)n;
    cap = LINNEAmd_EncodeStreamBound(&tr.header);
    if (hipMalloc(&d_out, cap ? cap : 1) != hipSuccess) { fprintf(stderr, "Failed to allocate %llu bytes on the device. \n", (unsigned long long)cap); d_out = NULL; goto done; }
    tr.d_pcm = r.d_extra; tr.pcm_stride = n; tr.d_out = d_out; tr.capacity = cap;
    if ((ret = LINNEAmd_EncodeStreamsDevice(r.ctx, &tr, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to encode! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    if (!(out = malloc(tr.out_bytes ? (size_t)tr.out_bytes : 1)) || hipMemcpy(out, d_out, tr.out_bytes, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "Failed to fetch the stream. \n"); goto done; }
    if (!(fp = fopen(out_path, "wb")) || fwrite(out, 1, (size_t)tr.out_bytes, fp) != tr.out_bytes) { fprintf(stderr, "File output error! %s \n", out_path); if (fp) fclose(fp); goto done; }
    fclose(fp);
    rc = 0;
done:
    if (d_out) (void)hipFree(d_out);
    resident_close(&r);
    free(out); free(coef); free(buf);
    return rc;
}

/* "b.lnn", "b.lnn,4410": the other stream's file name, then optionally the overlap in samples, behind the LAST comma where digits
 * alone follow it -> path (a copy), *overlap (0 unless given).  0, or a message in err */
static int parse_join(const char *text, char *path, size_t path_cap, uint64_t *overlap, char *err, size_t cap)
{
    const char *comma = strrchr(text, ',');
    size_t len = strlen(text);
    *overlap = 0;
    if (comma) {
        const char *p = comma + 1;
        char *end;
        unsigned long long v;
        if (!(*p >= '0' && *p <= '9')) { snprintf(err, cap, "join spec: an overlap in samples is expected at \"%s\"", p); return 1; }
        v = strtoull(p, &end, 10);
        if (*end != '\0') { snprintf(err, cap, "join spec: malformed at \"%s\"", end); return 1; }
        if (v > 0xFFFFFFFFull) { snprintf(err, cap, "join spec: overlap %s is outside 0 .. 4294967295", p); return 1; }
        *overlap = v;
        len = (size_t)(comma - text);
    }
    if (len == 0) { snprintf(err, cap, "join spec: a file name is expected"); return 1; }
    if (len >= path_cap) { snprintf(err, cap, "join spec: the file name is too long"); return 1; }
    memcpy(path, text, len); path[len] = '\0';
    return 0;
}

/* -J: the spec and the two headers are checked on the host; then both streams go to the device, LINNEAmd_StreamIndexCreate each, one
 * LINNEAmd_OverlayWindowsDevice output of up to four sources into int32 planes beside them, and LINNEAmd_EncodeStreamsDevice make
 * the output */
static int join_one(const char *spec_text, const char *in_path, const char *out_path)
{
    enum { UNITY = 16384 };
    uint8_t *buf = NULL, *other = NULL, *out = NULL;
    void *d_out = NULL, *d_other = NULL;
    struct LINNEAmdStreamIndex *xo = NULL;
    uint32_t size = 0, osize = 0, k = 0;
    struct resident r;
    struct LINNEAmdOverlaySource src[4];
    struct LINNEAmdOverlay ov;
    struct LINNEAmdTrack tr;
    struct LINNEHeader h, ho;
    char err[512], path[4096];
    uint64_t n, cap, overlap, na, nb;
    int64_t fall = 0, step = 0;
    FILE *fp;
    int ret, stage, rc = 1;
    memset(&r, 0, sizeof(r));
    if (parse_join(spec_text, path, sizeof(path), &overlap, err, sizeof(err)) != 0) { fprintf(stderr, "%s \n", err); return 1; }
    if (read_file(in_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", in_path); return 1; }
    if (read_file(path, &other, &osize) != 0) { fprintf(stderr, "Failed to open %s. \n", path); free(buf); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK || (ret = LINNEDecoder_DecodeHeader(other, osize, &ho)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); goto done; }
    na = h.num_samples; nb = ho.num_samples;
    if (h.num_channels != ho.num_channels || h.sampling_rate != ho.sampling_rate) { fprintf(stderr, "join spec: %u channels at %u Hz cannot be joined with %u channels at %u Hz \n", (unsigned)h.num_channels, (unsigned)h.sampling_rate, (unsigned)ho.num_channels, (unsigned)ho.sampling_rate); goto done; }
    if (na < 1 || nb < 1 || overlap > na || overlap > nb) { fprintf(stderr, "join spec: an overlap of %llu samples between streams of %llu and %llu \n", (unsigned long long)overlap, (unsigned long long)na, (unsigned long long)nb); goto done; }
    n = na + nb - overlap;
    if (n > 0xFFFFFFFFull) { fprintf(stderr, "join spec: %llu samples are more than a header names \n", (unsigned long long)n); goto done; }
    if ((stage = resident_open(&r, buf, size, na, sizeof(int32_t) * n * h.num_channels, "the stream", err, sizeof(err))) != 0) { fprintf(stderr, stage == 3 ? "Failed to join! %s \n" : "%s \n", err); goto done; }
    if (hipMalloc(&d_other, osize ? osize : 1) != hipSuccess || hipMemcpy(d_other, other, osize, hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "Failed to copy %s to the device. \n", path); goto done; }
    if (!(xo = LINNEAmd_StreamIndexCreate(r.ctx, d_other, osize, &ret))) { fprintf(stderr, "Failed to join! %s does not index: %d (%s) \n", path, ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    /* the falling ramp is exactly UNITY at its first sample and would reach 0 one past its last; the rising one is its complement:
     * the two gains add up to UNITY at every sample (what linne_amd.crossfade makes) */
    if (overlap) { fall = ((int64_t)UNITY << 32) + ((int64_t)1 << 31); step = -(int64_t)((((uint64_t)UNITY) << 32) / overlap); }
    memset(src, 0, sizeof(src));
    if (na > overlap) { src[k].index = r.index; src[k].d_stream = r.d_stream; src[k].first_sample = 0; src[k].num_samples = na - overlap; src[k].at = 0; src[k].gain_q32 = (int64_t)UNITY << 32; k++; }
    if (overlap) {
        src[k].index = r.index; src[k].d_stream = r.d_stream; src[k].first_sample = na - overlap; src[k].num_samples = overlap; src[k].at = na - overlap; src[k].gain_q32 = fall; src[k].step_q32 = step; k++;
        src[k].index = xo; src[k].d_stream = d_other; src[k].first_sample = 0; src[k].num_samples = overlap; src[k].at = na - overlap;
        src[k].gain_q32 = ((int64_t)UNITY << 32) + (((int64_t)1 << 32) - 1) - fall; src[k].step_q32 = -step; k++;
    }
    if (nb > overlap) { src[k].index = xo; src[k].d_stream = d_other; src[k].first_sample = overlap; src[k].num_samples = nb - overlap; src[k].at = na; src[k].gain_q32 = (int64_t)UNITY << 32; k++; }
    memset(&ov, 0, sizeof(ov));
    ov.sources = src; ov.num_sources = k; ov.shift = 14; ov.clip_bits = h.bits_per_sample; ov.num_samples = n; ov.d_pcm = r.d_extra; ov.pcm_stride = n;
    if ((ret = LINNEAmd_OverlayWindowsDevice(r.ctx, &ov, NULL, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to join! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    memset(&tr, 0, sizeof(tr));
    tr.header = h; tr.header.num_samples = (uint32_t)n;
    cap = LINNEAmd_EncodeStreamBound(&tr.header);
    if (hipMalloc(&d_out, cap ? cap : 1) != hipSuccess) { fprintf(stderr, "Failed to allocate %llu bytes on the device. \n", (unsigned long long)cap); d_out = NULL; goto done; }
    tr.d_pcm = r.d_extra; tr.pcm_stride = n; tr.d_out = d_out; tr.capacity = cap;
    if ((ret = LINNEAmd_EncodeStreamsDevice(r.ctx, &tr, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to encode! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    if (!(out = malloc(tr.out_bytes ? (size_t)tr.out_bytes : 1)) || hipMemcpy(out, d_out, tr.out_bytes, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "Failed to fetch the stream. \n"); goto done; }
    if (!(fp = fopen(out_path, "wb")) || fwrite(out, 1, (size_t)tr.out_bytes, fp) != tr.out_bytes) { fprintf(stderr, "File output error! %s \n", out_path); if (fp) fclose(fp); goto done; }
    fclose(fp);
    rc = 0;
done:
    if (xo) LINNEAmd_StreamIndexDestroy(xo);
    if (d_out) (void)hipFree(d_out);
    if (d_other) (void)hipFree(d_other);
    resident_close(&r);
    free(out); free(other); free(buf);
    return rc;
}

/* "b.lnn", "b.lnn,4096", "b.lnn,4096,0,220500": the other stream's file name, then optionally the largest lag, then optionally the
 * needle's first sample and its length, which come together; numbers are the trailing fields that begin with a digit -> path (a
 * copy), *max_lag (4096 unless given), *has_needle, *first, *n.  0, or a message in err */
static int parse_align(const char *text, char *path, size_t path_cap, uint64_t *max_lag, int *has_needle, uint64_t *first, uint64_t *n, char *err, size_t cap)
{
    size_t len = strlen(text);
    unsigned long long v[3];
    int count = 0;
    *max_lag = 4096; *has_needle = 0; *first = *n = 0;
    if (memchr(text, ',', len)) {
        while (count < 3) {
            size_t at = len;
            const char *p;
            char *end;
            while (at > 0 && text[at - 1] != ',') at--;
            if (at == 0) break;                                 /* no comma in front: the file name */
            p = text + at;
            if (!(*p >= '0' && *p <= '9')) {
                if (count == 0) { snprintf(err, cap, "lag spec: a largest lag in samples is expected at \"%s\"", p); return 1; }
                break;
            }
            errno = 0;
            v[count] = strtoull(p, &end, 10);
            if (end != text + len) { snprintf(err, cap, "lag spec: malformed at \"%.*s\"", (int)(text + len - end), end); return 1; }
            if (errno != 0) { snprintf(err, cap, "lag spec: %.*s is outside 64 bits", (int)(len - at), p); return 1; }
            count++;
            len = at - 1;
        }
        if (count == 2) { snprintf(err, cap, "lag spec: the needle's first sample and its length come together, behind the largest lag"); return 1; }
        if (count == 1) *max_lag = v[0];
        if (count == 3) { *max_lag = v[2]; *first = v[1]; *n = v[0]; *has_needle = 1; }
    }
    if (*max_lag > (LINNE_AMD_LAG_MAX_LAGS - 1u) / 2u) { snprintf(err, cap, "lag spec: a largest lag of %llu is outside 0 .. %u", (unsigned long long)*max_lag, (unsigned)((LINNE_AMD_LAG_MAX_LAGS - 1u) / 2u)); return 1; }
    if (len == 0) { snprintf(err, cap, "lag spec: a file name is expected"); return 1; }
    if (len >= path_cap) { snprintf(err, cap, "lag spec: the file name is too long"); return 1; }
    memcpy(path, text, len); path[len] = '\0';
    return 0;
}

/* a * b * c in 384 bits, least significant limb first */
static void mul3(unsigned __int128 a, unsigned __int128 b, unsigned __int128 c, uint64_t out[6])
{
    const uint64_t x[3][2] = { { (uint64_t)a, (uint64_t)(a >> 64) }, { (uint64_t)b, (uint64_t)(b >> 64) }, { (uint64_t)c, (uint64_t)(c >> 64) } };
    uint64_t acc[6] = { x[0][0], x[0][1], 0, 0, 0, 0 }, next[6];
    int f, i, j;
    for (f = 1; f < 3; f++) {
        memset(next, 0, sizeof(next));
        for (i = 0; i < 6; i++)
            for (j = 0; j < 2 && i + j < 6; j++) {
                unsigned __int128 t = (unsigned __int128)acc[i] * x[f][j];
                int k = i + j;
                while (t != 0 && k < 6) { t += next[k]; next[k] = (uint64_t)t; t >>= 64; k++; }
            }
        memcpy(acc, next, sizeof(acc));
    }
    memcpy(out, acc, sizeof(acc));
}
/* is d_i / sqrt(e_i) above d_j / sqrt(e_j)?  (a lag without energy has the value 0.)  Exact: the squares cross-multiplied */
static int lag_above(__int128 di, unsigned __int128 ei, __int128 dj, unsigned __int128 ej)
{
    uint64_t l[6], r[6];
    int k;
    if (ei == 0) di = 0;
    if (ej == 0) dj = 0;
    if ((di > 0) != (dj > 0) || di == 0 || dj == 0) return di > dj;
    mul3((unsigned __int128)(di < 0 ? -di : di), (unsigned __int128)(di < 0 ? -di : di), ej, l);
    mul3((unsigned __int128)(dj < 0 ? -dj : dj), (unsigned __int128)(dj < 0 ? -dj : dj), ei, r);
    for (k = 5; k >= 0; k--) if (l[k] != r[k]) return di > 0 ? l[k] > r[k] : l[k] < r[k];
    return 0;
}
/* linne_amd.best_lag over pairs [p0, p1) of a table [pairs][lags]: the pairs' dots and energies added per lag; ties go to the smaller
 * |lag|, then to the negative lag -> the lag, *r = dot / sqrt(a_sq * b_sq) there (NaN where an energy is 0) */
static int64_t best_lag(const struct LINNEAmdLagSum *t, const uint64_t *a_sq, uint32_t p0, uint32_t p1, uint32_t lags, int64_t lag_first, double *r)
{
    __int128 bd = 0; unsigned __int128 be = 0, ea = 0;
    uint32_t best = 0, l, p;
    for (p = p0; p < p1; p++) ea += ((unsigned __int128)a_sq[2u * p + 1u] << 64) | a_sq[2u * p];
    for (l = 0; l < lags; l++) {
        __int128 d = 0; unsigned __int128 e = 0;
        for (p = p0; p < p1; p++) {
            const struct LINNEAmdLagSum *s = t + (size_t)p * lags + l;
            d += (__int128)(((unsigned __int128)(uint64_t)s->dot_hi << 64) | s->dot_lo);
            e += ((unsigned __int128)s->b_sq_hi << 64) | s->b_sq_lo;
        }
        if (l > 0) {
            const int64_t la = lag_first + l, lb = lag_first + best, ma = la < 0 ? -la : la, mb = lb < 0 ? -lb : lb;
            if (!(lag_above(d, e, bd, be) || (!lag_above(bd, be, d, e) && (ma < mb || (ma == mb && la < lb))))) continue;
        }
        best = l; bd = d; be = e;
    }
    *r = (ea > 0 && be > 0) ? (double)((long double)bd / sqrtl((long double)ea * (long double)be)) : NAN;
    return lag_first + best;
}

/* -A: the spec and the two headers are checked on the host; then both streams go to the device, LINNEAmd_StreamIndexCreate each and
 * one LINNEAmd_LagWindowsDevice probe over the channels the two share; the host reads the table as linne_amd.best_lag does */
static int align_one(const char *spec_text, const char *in_path)
{
    uint8_t *buf = NULL, *other = NULL;
    void *d_other = NULL;
    struct LINNEAmdStreamIndex *xo = NULL;
    struct LINNEAmdLagSum *table = NULL;
    uint64_t a_sq[16];
    uint32_t size = 0, osize = 0, P, L, p;
    struct resident r;
    struct LINNEAmdLagProbe q;
    struct LINNEHeader h, ho;
    char err[512], path[4096];
    uint64_t max_lag, first, n, room;
    int has_needle, ret, stage, rc = 1;
    double coef;
    int64_t lag;
    memset(&r, 0, sizeof(r));
    if (parse_align(spec_text, path, sizeof(path), &max_lag, &has_needle, &first, &n, err, sizeof(err)) != 0) { fprintf(stderr, "%s \n", err); return 1; }
    if (read_file(in_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", in_path); return 1; }
    if (read_file(path, &other, &osize) != 0) { fprintf(stderr, "Failed to open %s. \n", path); free(buf); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK || (ret = LINNEDecoder_DecodeHeader(other, osize, &ho)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); goto done; }
    P = h.num_channels < ho.num_channels ? h.num_channels : ho.num_channels;
    L = (uint32_t)(2u * max_lag + 1u);
    room = LINNE_AMD_LAG_MAX_PRODUCTS / ((uint64_t)L * P);
    if (!has_needle) { first = 0; n = h.num_samples < room ? h.num_samples : room; }     /* the whole stream, cut to the products limit */
    if (n < 1 || first > h.num_samples || n > h.num_samples - first) { fprintf(stderr, "lag spec: a needle of %llu samples from %llu on in a stream of %llu \n", (unsigned long long)n, (unsigned long long)first, (unsigned long long)h.num_samples); goto done; }
    if (n > room) { fprintf(stderr, "lag spec: %llu samples * %u lags * %u pairs are more than LINNE_AMD_LAG_MAX_PRODUCTS = 2^38: a needle of at most %llu samples \n", (unsigned long long)n, L, P, (unsigned long long)room); goto done; }
    if ((stage = resident_open(&r, buf, size, h.num_samples, sizeof(struct LINNEAmdLagSum) * (uint64_t)L * P + sizeof(a_sq), "the stream", err, sizeof(err))) != 0) { fprintf(stderr, stage == 3 ? "Failed to align! %s \n" : "%s \n", err); goto done; }
    if (hipMalloc(&d_other, osize ? osize : 1) != hipSuccess || hipMemcpy(d_other, other, osize, hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "Failed to copy %s to the device. \n", path); goto done; }
    if (!(xo = LINNEAmd_StreamIndexCreate(r.ctx, d_other, osize, &ret))) { fprintf(stderr, "Failed to align! %s does not index: %d (%s) \n", path, ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    memset(&q, 0, sizeof(q));
    q.index_a = r.index; q.d_stream_a = r.d_stream; q.first_a = first; q.num_samples = n;
    q.index_b = xo; q.d_stream_b = d_other; q.first_b = first; q.lag_first = -(int64_t)max_lag; q.num_lags = L; q.num_pairs = P;
    for (p = 0; p < P; p++) q.chan_a[p] = q.chan_b[p] = (uint8_t)p;
    q.d_out = r.d_extra; q.pair_stride = L; q.d_a_sq = (uint64_t *)((struct LINNEAmdLagSum *)r.d_extra + (size_t)L * P);
    if ((ret = LINNEAmd_LagWindowsDevice(r.ctx, &q, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to align! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
    if (!(table = malloc(sizeof(*table) * (size_t)L * P)) || hipMemcpy(table, q.d_out, sizeof(*table) * (size_t)L * P, hipMemcpyDeviceToHost) != hipSuccess
            || hipMemcpy(a_sq, q.d_a_sq, sizeof(uint64_t) * 2u * P, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "Failed to fetch the table. \n"); goto done; }
    for (p = 0; p < P; p++) {
        lag = best_lag(table, a_sq, p, p + 1u, L, q.lag_first, &coef);
        printf("channel %u: lag %lld correlation %.9f \n", p, (long long)lag, coef);
    }
    lag = best_lag(table, a_sq, 0, P, L, q.lag_first, &coef);
    printf("all %u channels: lag %lld correlation %.9f \n", P, (long long)lag, coef);
    rc = 0;
done:
    if (xo) LINNEAmd_StreamIndexDestroy(xo);
    if (d_other) (void)hipFree(d_other);
    resident_close(&r);
    free(table); free(other); free(buf);
    return rc;
}

/* "512", "512,128", "512,128,0,220500": the frame length, then optionally the hop (a quarter of the frame unless given), then optionally
 * the first sample and the sample count, which come together -> *n_fft, *hop, *has_range, *first, *n.  0, or a message in err */
static int parse_spectrum(const char *text, uint32_t *n_fft, uint32_t *hop, int *has_range, uint64_t *first, uint64_t *n, char *err, size_t cap)
{
    unsigned long long v[4];
    int count = 0;
    const char *p = text;
    *has_range = 0; *first = *n = 0;
    for (;;) {
        char *end;
        if (!(*p >= '0' && *p <= '9')) {
            snprintf(err, cap, "spectrum spec: %s is expected at \"%s\"", count == 0 ? "a frame length in samples" : count == 1 ? "a hop in samples" : "a sample number", p);
            return 1;
        }
        errno = 0;
        v[count] = strtoull(p, &end, 10);
        if (errno != 0) { snprintf(err, cap, "spectrum spec: %.*s is outside 64 bits", (int)(end - p), p); return 1; }
        count++;
        if (*end == '\0') break;
        if (*end != ',' || count == 4) { snprintf(err, cap, "spectrum spec: malformed at \"%s\"", end); return 1; }
        p = end + 1;
    }
    if (count == 3) { snprintf(err, cap, "spectrum spec: the first sample and the sample count come together, behind the hop"); return 1; }
    /* every bin of the frame is printed: 2 * (N_FFT / 2 + 1) rows within LINNE_AMD_PROJECT_MAX_ROWS */
    if (v[0] < 1u || v[0] > LINNE_AMD_PROJECT_MAX_ROWS - 1u) { snprintf(err, cap, "spectrum spec: a frame length of %llu is outside 1 .. %u", v[0], (unsigned)(LINNE_AMD_PROJECT_MAX_ROWS - 1u)); return 1; }
    *n_fft = (uint32_t)v[0];
    *hop = *n_fft / 4u ? *n_fft / 4u : 1u;
    if (count >= 2) {
        if (v[1] < 1u || v[1] > LINNE_AMD_PROJECT_MAX_HOP) { snprintf(err, cap, "spectrum spec: a hop of %llu is outside 1 .. %u", v[1], (unsigned)LINNE_AMD_PROJECT_MAX_HOP); return 1; }
        *hop = (uint32_t)v[1];
    }
    if (count == 4) { *first = v[2]; *n = v[3]; *has_range = 1; }
    return 0;
}

/* an unsigned 128-bit integer in decimal */
static void print_u128(unsigned __int128 v)
{
    char text[40];
    int at = 39;
    text[at] = '\0';
    do { text[--at] = (char)('0' + (int)(v % 10u)); v /= 10u; } while (v != 0);
    fputs(text + at, stdout);
}

/* -F: the spec and the header are checked on the host; then the stream goes to the device, LINNEAmd_StreamIndexCreate, and
 * LINNEAmd_ProjectWindowsDevice on the designed basis, in runs of frames that fit the call's products limit and a table of 256 MiB;
 * the host adds re^2 + im^2 per bin in 128 bits */
static int spectrum_one(const char *spec_text, const char *in_path)
{
    uint8_t *buf = NULL;
    int16_t *basis = NULL;
    int32_t *table = NULL;
    unsigned __int128 *sums = NULL;
    uint32_t size = 0, n_fft, hop, bins, K, C, c, j;
    struct resident r;
    struct LINNEAmdWindow w;
    struct LINNEAmdProjectSpec sp;
    struct LINNEHeader h;
    char err[512];
    uint64_t first, n, f0, f1, run, f, most;
    int has_range, ret, stage, rc = 1;
    memset(&r, 0, sizeof(r));
    if (parse_spectrum(spec_text, &n_fft, &hop, &has_range, &first, &n, err, sizeof(err)) != 0) { fprintf(stderr, "%s \n", err); return 1; }
    if (read_file(in_path, &buf, &size) != 0) { fprintf(stderr, "Failed to open %s. \n", in_path); return 1; }
    if ((ret = LINNEDecoder_DecodeHeader(buf, size, &h)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to get header information: %d \n", ret); goto done; }
    if (!has_range) { first = 0; n = h.num_samples; }
    if (first > h.num_samples || n > h.num_samples - first) { fprintf(stderr, "spectrum spec: %llu samples from %llu on in a stream of %llu \n", (unsigned long long)n, (unsigned long long)first, (unsigned long long)h.num_samples); goto done; }
    bins = n_fft / 2u + 1u; K = 2u * bins; C = h.num_channels;
    f0 = (first + hop - 1u) / hop; f1 = (first + n + hop - 1u) / hop;       /* the frames f with first <= f * hop < first + n */
    most = LINNE_AMD_PROJECT_MAX_PRODUCTS / ((uint64_t)K * n_fft * C);
    if (most > ((uint64_t)1 << 26) / ((uint64_t)K * C)) most = ((uint64_t)1 << 26) / ((uint64_t)K * C);
    if (most < 1u) most = 1u;
    run = f1 - f0 < most ? f1 - f0 : most;
    if (!(basis = malloc(sizeof(*basis) * (size_t)K * n_fft)) || !(sums = calloc((size_t)C * bins, sizeof(*sums))) || !(table = malloc(sizeof(*table) * (size_t)(C * (run ? run : 1u) * K)))) { fprintf(stderr, "Failed to allocate the tables. \n"); goto done; }
    if ((ret = LINNEAmd_ProjectDesign(n_fft, bins, 1, basis)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to design the basis: %d \n", ret); goto done; }
    if ((stage = resident_open(&r, buf, size, h.num_samples, sizeof(int32_t) * C * (run ? run : 1u) * K, "the stream", err, sizeof(err))) != 0) { fprintf(stderr, stage == 3 ? "Failed to project! %s \n" : "%s \n", err); goto done; }
    for (f = f0; f < f1; f += run) {
        const uint64_t cnt = f1 - f < run ? f1 - f : run;
        memset(&sp, 0, sizeof(sp));
        sp.frame_len = n_fft; sp.hop = hop; sp.num_rows = K; sp.before = n_fft / 2u; sp.shift = 15; sp.format = LINNE_AMD_PCM_S32;
        sp.channel_stride = cnt * K; sp.frame_stride = K; sp.row_stride = 1; sp.basis = basis;
        w = r.w; w.first_sample = f; w.num_samples = cnt; w.d_pcm = r.d_extra; w.pcm_stride = 0;
        if ((ret = LINNEAmd_ProjectWindowsDevice(r.ctx, &w, &sp, 1, 0)) != LINNE_APIRESULT_OK) { fprintf(stderr, "Failed to project! ret:%d (%s) \n", ret, LINNEAmd_GetLastError(r.ctx)); goto done; }
        if (sp.saturated) { fprintf(stderr, "Failed to project! a bin does not fit 32 bits at shift 15: the sums would not be exact \n"); goto done; }
        if (hipMemcpy(table, r.d_extra, sizeof(*table) * (size_t)(C * cnt * K), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "Failed to fetch the table. \n"); goto done; }
        for (c = 0; c < C; c++) {
            uint64_t g;
            for (g = 0; g < cnt; g++) {
                const int32_t *row = table + ((size_t)c * cnt + g) * K;
                for (j = 0; j < bins; j++) {
                    const int64_t re = row[2u * j], im = row[2u * j + 1u];
                    sums[(size_t)c * bins + j] += (unsigned __int128)(uint64_t)(re * re) + (unsigned __int128)(uint64_t)(im * im);
                }
            }
        }
    }
    for (j = 0; j < bins; j++) {
        printf("bin %u %.6f Hz:", j, (double)j * (double)h.sampling_rate / (double)n_fft);
        for (c = 0; c < C; c++) { putchar(' '); print_u128(sums[(size_t)c * bins + j]); }
        printf(" \n");
    }
    rc = 0;
done:
    resident_close(&r);
    free(table); free(sums); free(basis); free(buf);
    return rc;
}

int main(int argc, char **argv)
{
    struct options o;
    int i, rc = 0;
    if (argc == 1) { usage(argv[0]); printf("Type `%s -h` to display command helps. \n", argv[0]); return 1; }
    parse(argc, argv, &o);
    if (o.help) { usage(argv[0]); return 0; }
    if (o.version) { printf("LINNE -- LInear-predictive Neural Net Encoder Version.%d (liblinne_amd, MI355X) \n", LINNE_CODEC_VERSION); return 0; }
    if (o.spectrum) {
        if (o.align || o.join || o.encode || o.decode || o.repair || o.verify || o.compare || o.measure || o.digest || o.silence || o.levels || o.relate || o.remix || o.resample || o.batch_dir || o.num_files != 1) { fprintf(stderr, "%s: -F takes a frame length and an input file name and no other mode. \n", argv[0]); return 1; }
        return spectrum_one(o.spectrum_spec, o.files[0]);
    }
    if (o.align) {
        if (o.join || o.encode || o.decode || o.repair || o.verify || o.compare || o.measure || o.digest || o.silence || o.levels || o.relate || o.remix || o.resample || o.batch_dir || o.num_files != 1) { fprintf(stderr, "%s: -A takes another stream's file name and an input file name and no other mode. \n", argv[0]); return 1; }
        return align_one(o.align_spec, o.files[0]);
    }
    if (o.join) {
        if (o.encode || o.decode || o.repair || o.verify || o.compare || o.measure || o.digest || o.silence || o.levels || o.relate || o.remix || o.resample || o.batch_dir || o.num_files != 2) { fprintf(stderr, "%s: -J takes another stream's file name, an input and an output file name and no other mode. \n", argv[0]); return 1; }
        return join_one(o.join_spec, o.files[0], o.files[1]);
    }
    if (o.resample) {
        if (o.encode || o.decode || o.repair || o.verify || o.compare || o.measure || o.digest || o.silence || o.levels || o.relate || o.remix || o.batch_dir || o.num_files != 2) { fprintf(stderr, "%s: -Z takes a sampling rate, an input and an output file name and no other mode. \n", argv[0]); return 1; }
        return resample_one(o.resample_spec, o.files[0], o.files[1]);
    }
    if (o.remix) {
        if (o.encode || o.decode || o.repair || o.verify || o.compare || o.measure || o.digest || o.silence || o.levels || o.relate || o.batch_dir || o.num_files != 2) { fprintf(stderr, "%s: -X takes a matrix, an input and an output file name and no other mode. \n", argv[0]); return 1; }
        return remix_one(o.remix_spec, o.files[0], o.files[1]);
    }
    if (o.relate) {
        unsigned long long bucket = 0;
        if (o.encode || o.decode || o.repair || o.verify || o.compare || o.measure || o.digest || o.silence || o.levels || o.batch_dir || o.num_files < 1 || o.num_files > 2) { fprintf(stderr, "%s: -R takes an optional bucket sample count and a stream file name and no other mode. \n", argv[0]); return 1; }
        if (o.num_files == 2) {
            char *end; bucket = strtoull(o.files[0], &end, 10);
            if (*end != '\0' || o.files[0][0] < '0' || o.files[0][0] > '9' || bucket == 0) { fprintf(stderr, "%s: bucket sample count is out of range. \n", argv[0]); return 1; }
        }
        return relate_one(o.files[o.num_files - 1], bucket);
    }
    if (o.levels) {
        unsigned long long bins, shift = 0, scale = LINNE_AMD_HIST_LINEAR;
        char *end;
        if (o.encode || o.decode || o.repair || o.verify || o.compare || o.measure || o.digest || o.silence || o.batch_dir || o.num_files != 1) { fprintf(stderr, "%s: -L takes BINS[,SHIFT[,log2]] and a stream file name and no other mode. \n", argv[0]); return 1; }
        bins = strtoull(o.levels_spec, &end, 10);
        if (o.levels_spec[0] < '0' || o.levels_spec[0] > '9' || (*end != '\0' && *end != ',') || bins == 0 || bins > LINNE_AMD_HIST_MAX_BINS) { fprintf(stderr, "%s: bin count is out of range. \n", argv[0]); return 1; }
        if (*end == ',') {
            const char *m = end + 1;
            shift = strtoull(m, &end, 10);
            if (m[0] < '0' || m[0] > '9' || (*end != '\0' && *end != ',') || shift > 31) { fprintf(stderr, "%s: level shift is out of range. \n", argv[0]); return 1; }
            if (*end == ',') {
                if (strcmp(end + 1, "log2") == 0) scale = LINNE_AMD_HIST_LOG2;
                else if (strcmp(end + 1, "linear") != 0) { fprintf(stderr, "%s: level scale is neither linear nor log2. \n", argv[0]); return 1; }
            }
        }
        return levels_one(o.files[0], (uint32_t)bins, (uint32_t)shift, (uint32_t)scale);
    }
    if (o.silence) {
        unsigned long long threshold, min_samples = 1;
        char *end;
        if (o.encode || o.decode || o.repair || o.verify || o.compare || o.measure || o.digest || o.batch_dir || o.num_files != 1) { fprintf(stderr, "%s: -S takes THRESHOLD[,MIN_SAMPLES] and a stream file name and no other mode. \n", argv[0]); return 1; }
        threshold = strtoull(o.silence_spec, &end, 10);
        if (o.silence_spec[0] < '0' || o.silence_spec[0] > '9' || (*end != '\0' && *end != ',') || threshold > 0xFFFFFFFFull) { fprintf(stderr, "%s: silence threshold is out of range. \n", argv[0]); return 1; }
        if (*end == ',') {
            const char *m = end + 1;
            min_samples = strtoull(m, &end, 10);
            if (m[0] < '0' || m[0] > '9' || *end != '\0' || min_samples == 0) { fprintf(stderr, "%s: silence minimum sample count is out of range. \n", argv[0]); return 1; }
        }
        return silence_one(o.files[0], (uint32_t)threshold, min_samples);
    }
    if (o.repair) {
        if (o.encode || o.decode || o.compare || o.measure || o.digest || o.verify || o.batch_dir || o.num_files != 2) { fprintf(stderr, "%s: -r takes an input and an output file name and no other mode. \n", argv[0]); return 1; }
        return repair_one(o.files[0], o.files[1]);
    }
    if (o.compare) {
        if (o.encode || o.decode || o.measure || o.digest || o.verify || o.batch_dir || o.num_files != 2) { fprintf(stderr, "%s: -C takes a stream and a WAV file name and no other mode. \n", argv[0]); return 1; }
        return compare_one(o.files[0], o.files[1]);
    }
    if (o.measure) {
        unsigned long long bucket = 0;
        if (o.encode || o.decode || o.digest || o.verify || o.batch_dir || o.num_files < 1 || o.num_files > 2) { fprintf(stderr, "%s: -M takes an optional bucket sample count and a stream file name and no other mode. \n", argv[0]); return 1; }
        if (o.num_files == 2) {
            char *end; bucket = strtoull(o.files[0], &end, 10);
            if (*end != '\0' || o.files[0][0] < '0' || o.files[0][0] > '9' || bucket == 0) { fprintf(stderr, "%s: bucket sample count is out of range. \n", argv[0]); return 1; }
        }
        return measure_one(o.files[o.num_files - 1], bucket);
    }
    if (o.digest) {
        unsigned long long bucket = 0;
        if (o.encode || o.decode || o.verify || o.batch_dir || o.num_files < 1 || o.num_files > 2) { fprintf(stderr, "%s: -D takes an optional bucket sample count and a stream file name and no other mode. \n", argv[0]); return 1; }
        if (o.num_files == 2) {
            char *end; bucket = strtoull(o.files[0], &end, 10);
            if (*end != '\0' || o.files[0][0] < '0' || o.files[0][0] > '9' || bucket == 0) { fprintf(stderr, "%s: bucket sample count is out of range. \n", argv[0]); return 1; }
        }
        return digest_one(o.files[o.num_files - 1], bucket);
    }
    if (o.verify && !o.encode) { fprintf(stderr, "%s: -V goes with encode mode (-e) only. \n", argv[0]); return 1; }
    if (o.encode && o.decode) { fprintf(stderr, "%s: encode and decode mode cannot specify simultaneously. \n", argv[0]); return 1; }
    if (!o.encode && !o.decode) { fprintf(stderr, "%s: decode(-d) or encode(-e) option must be specified. \n", argv[0]); return 1; }
    if (o.batch_dir ? (o.num_files < 1) : (o.num_files != 2)) { fprintf(stderr, "%s: input and output file name must be specified. \n", argv[0]); return 1; }
    if (o.encode) {
        struct LINNEEncoderConfig cfg;
        struct LINNEEncoder *enc;
        cfg.max_num_channels = LINNE_MAX_NUM_CHANNELS; cfg.max_num_samples_per_block = 16 * 1024; cfg.max_num_layers = 5; cfg.max_num_parameters_per_layer = 128;
        if (!(enc = LINNEEncoder_Create(&cfg, NULL, 0))) { fprintf(stderr, "Failed to create encoder handle. \n"); return 1; }
        if (!o.batch_dir) rc = encode_one(enc, &o, o.files[0], o.files[1]);
        else for (i = 0; i < o.num_files && rc == 0; i++) { char out[4096]; batch_name(out, sizeof(out), o.batch_dir, o.files[i], ".lnn"); rc = encode_one(enc, &o, o.files[i], out); }
        LINNEEncoder_Destroy(enc);
    } else {
        struct LINNEDecoderConfig cfg;
        struct LINNEDecoder *dec;
        cfg.max_num_channels = LINNE_MAX_NUM_CHANNELS; cfg.max_num_layers = 5; cfg.max_num_parameters_per_layer = 128; cfg.check_crc = o.no_crc ? 0 : 1;
        if (!(dec = LINNEDecoder_Create(&cfg, NULL, 0))) { fprintf(stderr, "Failed to create decoder handle. \n"); return 1; }
        if (!o.batch_dir) rc = decode_one(dec, &o, o.files[0], o.files[1]);
        else for (i = 0; i < o.num_files && rc == 0; i++) { char out[4096]; batch_name(out, sizeof(out), o.batch_dir, o.files[i], ".wav"); rc = decode_one(dec, &o, o.files[i], out); }
        LINNEDecoder_Destroy(dec);
    }
    return rc;
}
