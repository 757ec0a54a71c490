"""linne_amd -- Python bindings (ctypes) of liblinne_amd.so, the MI355X-native implementation of the LINNE
per-frame prediction path behind LINNE's own C API.

The product is the shared library (linne_amd/csrc, built in-tree as linne_amd/liblinne_amd.so); this module
only loads it and wraps its two interfaces:

* ``api``      -- the 13 LINNE public functions (include/linne_encoder.h, include/linne_decoder.h), host buffers;
* ``Context``  -- the batch C-ABI of include/linne_amd.h on device-resident buffers (torch tensors are used
  only to own HBM and to name the HIP stream).

There is no CPU fallback: importing works without a GPU (so the symbol table can be checked), but any
compute call needs a HIP device, and a missing library raises ImportError.
"""
import contextlib
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LINNE_AMD_LIB") or os.path.join(_HERE, "liblinne_amd.so")     # (LINNE_AMD_LIB: another build of the library, for A/B runs on one box)

PARAM_WORDS = 160
STAT_WORDS = 8
RICE_PLAN_BYTES = 1040         # include/linne_amd.h: [0] order, [1] host-search flag, [16..] parameters
RICE_PLAN_NBITS = 4            # uint32 at this byte offset of a plan: the channel's whole Rice code in bits
PRM_PREV, PRM_PCOEF, PRM_UNITS, PRM_RSHIFT, PRM_COEF = 0, 2, 4, 7, 10
ST_R0, ST_K1, ST_ZERO, ST_TAIL, ST_BEST, ST_LOSS = 0, 1, 4, 5, 6, 7
PRESET_LAYERS = {0: (2, 32), 1: (2, 32), 2: (4, 64, 8), 3: (4, 64, 8), 4: (4, 64, 8),
                 5: (4, 128, 16), 6: (4, 128, 16), 7: (4, 128, 16)}
CAPTURE_WORDS, CAPTURE_TRIALS = 8, 8      # include/linne_amd.h LINNEAmd_GetLastSearchCapture
CAP_MEAN, CAP_SLACK, CAP_REL, CAP_XMAX, CAP_HSUM, CAP_HOW, CAP_ORDERED, CAP_UNITS = range(8)
PRESET_NUM_REGULARS = {0: 1, 1: 2, 2: 1, 3: 2, 4: 4, 5: 1, 6: 2, 7: 4}

# symbols include/*.h declare (checked by tests/test_abi.py)
API_SYMBOLS = [
    "LINNEEncoder_EncodeHeader", "LINNEEncoder_CalculateWorkSize", "LINNEEncoder_Create", "LINNEEncoder_Destroy",
    "LINNEEncoder_SetEncodeParameter", "LINNEEncoder_EncodeBlock", "LINNEEncoder_EncodeWhole",
    "LINNEDecoder_DecodeHeader", "LINNEDecoder_CalculateWorkSize", "LINNEDecoder_Create", "LINNEDecoder_Destroy",
    "LINNEDecoder_SetHeader", "LINNEDecoder_DecodeBlock", "LINNEDecoder_DecodeWhole",
]
AMD_SYMBOLS = [
    "LINNEAmd_GetDeviceCount", "LINNEAmd_ContextCreate", "LINNEAmd_ContextDestroy", "LINNEAmd_GetLastError",
    "LINNEAmd_ReserveScratch", "LINNEAmd_ScratchBytesPerFrame", "LINNEAmd_SetStream", "LINNEAmd_EncodeFramesDevice", "LINNEAmd_DecodeFramesDevice",
    "LINNEAmd_EncodeFramesHost", "LINNEAmd_DecodeFramesHost", "LINNEAmd_Synchronize", "LINNEAmd_GetLastFallbackCount", "LINNEAmd_GetLastTimingMs",
    "LINNEAmd_GetLastTimingLaunches", "LINNEAmd_GetLastSearchLongForm", "LINNEAmd_EnableTiming", "LINNEAmd_PackFrames",
    "LINNEAmd_GetLastMinMargin", "LINNEAmd_SetSearchCapture", "LINNEAmd_GetLastSearchCapture", "LINNEAmd_SetAfIterations", "LINNEAmd_SetLearning", "LINNEAmd_MultiCreate", "LINNEAmd_MultiDestroy", "LINNEAmd_MultiNumDevices", "LINNEAmd_MultiDevice",
    "LINNEAmd_MultiContext", "LINNEAmd_MultiGetLastError", "LINNEAmd_MultiEncodeFramesHost", "LINNEAmd_MultiDecodeFramesHost", "LINNEAmd_SlotCreate", "LINNEAmd_SlotDestroy", "LINNEAmd_SlotPcm", "LINNEAmd_SlotData", "LINNEAmd_SlotParams", "LINNEAmd_SlotStats",
    "LINNEAmd_SlotCapacity", "LINNEAmd_SlotRicePlan", "LINNEAmd_SlotCreateEx", "LINNEAmd_SlotFlags", "LINNEAmd_SlotPcm16", "LINNEAmd_SlotPacked", "LINNEAmd_SlotOffsets",
    "LINNEAmd_SlotFetchResidual", "LINNEAmd_SlotStream", "LINNEAmd_SlotStreamCapacity", "LINNEAmd_SlotBitPos", "LINNEAmd_SlotEndBits", "LINNEAmd_SlotPcm16Valid",
    "LINNEAmd_SlotPcmWidth", "LINNEAmd_SlotDecodeStreamSubmit", "LINNEAmd_SlotFetchPcm32", "LINNEAmd_RiceDecodeDevice", "LINNEAmd_SlotBitEnd", "LINNEAmd_LastDecodeWholeMode", "LINNEAmd_RiceEmitDevice", "LINNEAmd_PackFramesEmitted", "LINNEAmd_RicePlanDevice", "LINNEAmd_PackFramesPlanned", "LINNEAmd_SlotEncodeSubmit", "LINNEAmd_SlotDecodeSubmit", "LINNEAmd_SlotWait",
    "LINNEAmd_StreamIndexCreate", "LINNEAmd_StreamIndexDestroy", "LINNEAmd_StreamIndexHeader", "LINNEAmd_StreamIndexNumBlocks",
    "LINNEAmd_DecodeStreamDevice", "LINNEAmd_DecodeWindowsDevice", "LINNEAmd_EncodeStreamBound", "LINNEAmd_EncodeStreamDevice", "LINNEAmd_GetLastStreamEncodeCount",
    "LINNEAmd_EncodeStreamsDevice", "LINNEAmd_GetLastStreamBatchCount",
    "LINNEAmd_EncodeStreamDeviceLayout", "LINNEAmd_EncodeStreamsDeviceLayout", "LINNEAmd_DecodeWindowsDeviceLayout",
    "LINNEAmd_StreamIndexesCreate", "LINNEAmd_GetLastIndexBatchCount", "LINNEAmd_StreamIndexBlocks", "LINNEAmd_StreamIndexFailure",
    "LINNEAmd_SpliceStreamsDevice", "LINNEAmd_GetLastSpliceCount",
    "LINNEAmd_RepairStreamsDevice", "LINNEAmd_GetLastRepairGaps", "LINNEAmd_GetLastRepairCount",
    "LINNEAmd_CompareWindowsDevice",
    "LINNEAmd_MeasureWindowsDevice",
    "LINNEAmd_DigestWindowsDevice",
    "LINNEAmd_QuietWindowsDevice", "LINNEAmd_HistogramWindowsDevice", "LINNEAmd_RelateWindowsDevice",
    "LINNEAmd_MixWindowsDevice",
    "LINNEAmd_ResampleWindowsDevice", "LINNEAmd_ResampleLength", "LINNEAmd_ResampleDesign",
    "LINNEAmd_OverlayWindowsDevice",
    "LINNEAmd_LagWindowsDevice",
    "LINNEAmd_ProjectWindowsDevice", "LINNEAmd_ProjectLength", "LINNEAmd_ProjectDesign",
]
PCM_S32, PCM_S16, PCM_S24, PCM_F32 = 0, 1, 2, 3          # include/linne_amd.h LINNE_AMD_PCM_*


class Shape(C.Structure):
    _fields_ = [("num_channels", C.c_uint32), ("bits_per_sample", C.c_uint32), ("num_samples_per_block", C.c_uint32),
                ("preset", C.c_uint32), ("ch_process_method", C.c_uint32)]


class Header(C.Structure):
    """struct LINNEHeader (include/linne.h)"""
    _fields_ = [("format_version", C.c_uint32), ("codec_version", C.c_uint32), ("num_channels", C.c_uint16),
                ("num_samples", C.c_uint32), ("sampling_rate", C.c_uint32), ("bits_per_sample", C.c_uint16),
                ("num_samples_per_block", C.c_uint32), ("preset", C.c_uint8), ("ch_process_method", C.c_int)]


class Window(C.Structure):
    """struct LINNEAmdWindow (include/linne_amd.h)"""
    _fields_ = [("index", C.c_void_p), ("d_stream", C.c_void_p), ("first_sample", C.c_uint64), ("num_samples", C.c_uint64),
                ("d_pcm", C.c_void_p), ("pcm_stride", C.c_uint64), ("result", C.c_int32)]


class Track(C.Structure):
    """struct LINNEAmdTrack (include/linne_amd.h)"""
    _fields_ = [("header", Header), ("d_pcm", C.c_void_p), ("pcm_stride", C.c_uint64), ("d_out", C.c_void_p), ("capacity", C.c_uint64),
                ("out_bytes", C.c_uint64), ("parcor_state", C.c_double), ("result", C.c_int32)]


class Cut(C.Structure):
    """struct LINNEAmdCut (include/linne_amd.h)"""
    _fields_ = [("index", C.c_void_p), ("d_stream", C.c_void_p), ("first_sample", C.c_uint64), ("num_samples", C.c_uint64)]


class Splice(C.Structure):
    """struct LINNEAmdSplice (include/linne_amd.h)"""
    _fields_ = [("cuts", C.POINTER(Cut)), ("num_cuts", C.c_uint32), ("d_out", C.c_void_p), ("capacity", C.c_uint64), ("out_bytes", C.c_uint64),
                ("copied_blocks", C.c_uint32), ("encoded_blocks", C.c_uint32), ("result", C.c_int32)]


class Gap(C.Structure):
    """struct LINNEAmdGap (include/linne_amd.h)"""
    _fields_ = [("first_sample", C.c_uint64), ("num_samples", C.c_uint64), ("src_offset", C.c_uint64), ("src_bytes", C.c_uint64),
                ("fill_blocks", C.c_uint32), ("reserved", C.c_uint32)]


class Repair(C.Structure):
    """struct LINNEAmdRepair (include/linne_amd.h)"""
    _fields_ = [("d_stream", C.c_void_p), ("stream_bytes", C.c_uint64), ("d_out", C.c_void_p), ("capacity", C.c_uint64), ("out_bytes", C.c_uint64),
                ("lost_samples", C.c_uint64), ("kept_blocks", C.c_uint32), ("fill_blocks", C.c_uint32), ("num_gaps", C.c_uint32), ("exact", C.c_uint32),
                ("result", C.c_int32)]


class PcmLayout(C.Structure):
    """struct LINNEAmdPcmLayout (include/linne_amd.h)"""
    _fields_ = [("format", C.c_uint32), ("saturated", C.c_uint32), ("channel_stride", C.c_uint64), ("sample_stride", C.c_uint64)]


class Diff(C.Structure):
    """struct LINNEAmdDiff (include/linne_amd.h)"""
    _fields_ = [("num_differing", C.c_uint64), ("first_sample", C.c_uint64), ("first_channel", C.c_uint32), ("reserved", C.c_uint32)]


class Measure(C.Structure):
    """struct LINNEAmdMeasure (include/linne_amd.h): one channel of one bucket of one window"""
    _fields_ = [("min", C.c_int32), ("max", C.c_int32), ("sum", C.c_int64), ("sumsq_lo", C.c_uint64), ("sumsq_hi", C.c_uint64)]


class MeasureSpec(C.Structure):
    """struct LINNEAmdMeasureSpec (include/linne_amd.h)"""
    _fields_ = [("bucket_samples", C.c_uint64), ("d_out", C.c_void_p), ("channel_stride", C.c_uint64)]


MEASURE_DTYPE = np.dtype([("min", "<i4"), ("max", "<i4"), ("sum", "<i8"), ("sumsq_lo", "<u8"), ("sumsq_hi", "<u8")])


class Measurement:
    """one window's table of measure_windows: `records`, an int64 CUDA tensor (C, nb, 4) holding a struct LINNEAmdMeasure per channel
    and bucket, and strided views of it -- min, max (int32, (C, nb)), sum (int64), sumsq_lo / sumsq_hi (int64 views of the two
    unsigned words of the 128-bit sum of squares)"""

    def __init__(self, records, bucket_samples):
        import torch
        self.records, self.bucket_samples = records, bucket_samples
        w = records.view(torch.int32)                                  # (C, nb, 8)
        self.min, self.max = w[..., 0], w[..., 1]
        self.sum, self.sumsq_lo, self.sumsq_hi = records[..., 1], records[..., 2], records[..., 3]

    def energy(self):
        """the sum of squares as float64 (C, nb): hi * 2^64 + lo, lo taken as unsigned"""
        lo = self.sumsq_lo.double() + (self.sumsq_lo < 0).double() * 2.0 ** 64
        hi = self.sumsq_hi.double() + (self.sumsq_hi < 0).double() * 2.0 ** 64
        return hi * 2.0 ** 64 + lo

    def cpu(self):
        """-> a numpy structured array (C, nb) with the fields min, max, sum, sumsq_lo, sumsq_hi (the last two unsigned)"""
        a = np.ascontiguousarray(self.records.cpu().numpy())
        return a.view(MEASURE_DTYPE).reshape(a.shape[:2])


class Digest(C.Structure):
    """struct LINNEAmdDigest (include/linne_amd.h): one bucket of one window"""
    _fields_ = [("crc32", C.c_uint32), ("reserved", C.c_uint32), ("num_bytes", C.c_uint64)]


class DigestSpec(C.Structure):
    """struct LINNEAmdDigestSpec (include/linne_amd.h)"""
    _fields_ = [("bucket_samples", C.c_uint64), ("d_out", C.c_void_p)]


DIGEST_DTYPE = np.dtype([("crc32", "<u4"), ("reserved", "<u4"), ("num_bytes", "<u8")])


class DigestTable:
    """one window's table of digest_windows: `records`, an int64 CUDA tensor (nb, 2) holding a struct LINNEAmdDigest per bucket, and
    views of it -- crc32 and num_bytes (int64, (nb,); the reserved word behind crc32 is 0, so the 64-bit word is the CRC).  `header`
    is the stream's (channels, bits, samples), which same_audio compares beside the digests"""

    def __init__(self, records, bucket_samples, header):
        self.records, self.bucket_samples, self.header = records, bucket_samples, header
        self.crc32, self.num_bytes = records[:, 0], records[:, 1]

    def cpu(self):
        """-> a numpy structured array (nb,) with the fields crc32, reserved and num_bytes"""
        a = np.ascontiguousarray(self.records.cpu().numpy())
        return a.view(DIGEST_DTYPE).reshape(a.shape[0])


class Run(C.Structure):
    """struct LINNEAmdRun (include/linne_amd.h): one quiet run of one window"""
    _fields_ = [("first_sample", C.c_uint64), ("num_samples", C.c_uint64)]


class QuietSpec(C.Structure):
    """struct LINNEAmdQuietSpec (include/linne_amd.h)"""
    _fields_ = [("threshold", C.c_uint32), ("reserved", C.c_uint32), ("min_samples", C.c_uint64), ("d_out", C.c_void_p), ("capacity", C.c_uint64)]


class Quiet(C.Structure):
    """struct LINNEAmdQuiet (include/linne_amd.h): one window's answer on the host"""
    _fields_ = [("num_runs", C.c_uint64), ("quiet_samples", C.c_uint64), ("lead_samples", C.c_uint64), ("trail_samples", C.c_uint64)]


QUIET_DEFAULT_CAPACITY = 256   # quiet_windows(capacity=None): records per window in the first call; windows with more runs get a second one


class QuietRuns:
    """one window's answer of quiet_windows: `runs`, an int64 CUDA tensor (k, 2) of (first sample in the stream, length), ascending,
    k = min(num_runs, the capacity given); num_runs and quiet_samples describe all runs of at least min_samples frames whether or not
    they fitted; lead_samples and trail_samples are the quiet frames at the window's ends whatever min_samples is"""

    def __init__(self, runs, answer, threshold, min_samples):
        self.runs, self.threshold, self.min_samples = runs, threshold, min_samples
        self.num_runs, self.quiet_samples = int(answer.num_runs), int(answer.quiet_samples)
        self.lead_samples, self.trail_samples = int(answer.lead_samples), int(answer.trail_samples)

    def cpu(self):
        """-> the runs as a list of (first, n) of Python integers"""
        return [(int(a), int(b)) for a, b in self.runs.cpu().numpy()]


class HistogramSpec(C.Structure):
    """struct LINNEAmdHistogramSpec (include/linne_amd.h)"""
    _fields_ = [("bucket_samples", C.c_uint64), ("num_bins", C.c_uint32), ("shift", C.c_uint32), ("scale", C.c_uint32), ("reserved", C.c_uint32),
                ("d_out", C.c_void_p), ("channel_stride", C.c_uint64)]


HIST_LINEAR, HIST_LOG2, HIST_MAX_BINS = 0, 1, 1024


class Histogram:
    """one window's table of histogram_windows: `counts`, an int64 CUDA tensor (C, nb, num_bins) -- bin min(x, num_bins - 1) of
    x = |v| >> shift, or with log2 the bit length of that, per channel and bucket -- and the spec it was made with"""

    def __init__(self, counts, num_bins, shift, log2, bucket_samples):
        self.counts, self.num_bins, self.shift, self.log2, self.bucket_samples = counts, num_bins, shift, log2, bucket_samples

    def cpu(self):
        """-> the counts as a numpy int64 array (C, nb, num_bins)"""
        return np.ascontiguousarray(self.counts.cpu().numpy())


def level_threshold(counts, fraction, shift=0):
    """the level below which `fraction` of the samples lie, from a linear histogram of one channel or of the channels' sum: counts a
    sequence of num_bins counts (a Histogram's .cpu()[ch, k], or a sum of such rows) made with this shift -> the smallest
    T = ((j + 1) << shift) - 1 such that at least fraction of the samples have |v| <= T, or None when that bin is the last one, which
    holds everything above and so has no upper edge.  T is what quiet_streams takes as its threshold.  Pure host code"""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    assert len(c) >= 1 and all(v >= 0 for v in c) and 0.0 <= float(fraction) <= 1.0 and 0 <= int(shift) <= 31
    from fractions import Fraction
    need, run = Fraction(fraction) * sum(c), 0                  # (exact: the comparison below is made in rationals, not in floating point)
    for j, v in enumerate(c):
        run += v
        if run >= need:
            break
    return None if j == len(c) - 1 else ((j + 1) << int(shift)) - 1


class Relation(C.Structure):
    """struct LINNEAmdRelation (include/linne_amd.h): one channel pair (i <= j) of one bucket of one window"""
    _fields_ = [("dot_lo", C.c_uint64), ("dot_hi", C.c_int64), ("num_equal", C.c_uint64), ("num_opposite", C.c_uint64)]


class RelateSpec(C.Structure):
    """struct LINNEAmdRelateSpec (include/linne_amd.h)"""
    _fields_ = [("bucket_samples", C.c_uint64), ("d_out", C.c_void_p), ("pair_stride", C.c_uint64)]


class MixSpec(C.Structure):
    """struct LINNEAmdMixSpec (include/linne_amd.h)"""
    _fields_ = [("out_channels", C.c_uint32), ("shift", C.c_uint32), ("clip_bits", C.c_uint32), ("reserved", C.c_uint32),
                ("coef", (C.c_int16 * 8) * 8)]


class ResampleSpec(C.Structure):
    """struct LINNEAmdResampleSpec (include/linne_amd.h); coef is host memory"""
    _fields_ = [("up", C.c_uint32), ("down", C.c_uint32), ("taps", C.c_uint32), ("before", C.c_uint32), ("shift", C.c_uint32),
                ("clip_bits", C.c_uint32), ("reserved", C.c_uint64), ("coef", C.POINTER(C.c_int16))]


RESAMPLE_MAX_TAPS, RESAMPLE_MAX_RATIO, RESAMPLE_MAX_COEFS = 64, 1024, 16384     # include/linne_amd.h LINNE_AMD_RESAMPLE_MAX_*


def resample_ratio(rate_in, rate_out):
    """the rate change rate_in -> rate_out as (up, down), reduced by their greatest common divisor; ValueError when a rate is not
    positive or either of the two exceeds RESAMPLE_MAX_RATIO.  Pure host code"""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError(f"sampling rates are positive: {rate_in} -> {rate_out}")
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    if up > RESAMPLE_MAX_RATIO or down > RESAMPLE_MAX_RATIO:
        raise ValueError(f"{rate_in} -> {rate_out} is {up}/{down}: beyond {RESAMPLE_MAX_RATIO}")
    return up, down


def resample_length(num_samples, up, down):
    """LINNEAmd_ResampleLength: ceil(num_samples * up / down)"""
    return int(lib.LINNEAmd_ResampleLength(int(num_samples), int(up), int(down)))


def resample_design(up, down, taps=32):
    """LINNEAmd_ResampleDesign, the one designer there is -> (coef int16 (up, taps), shift, before); ValueError for arguments outside
    the call's bounds.  Pure host code: no device is needed"""
    up, down, taps = int(up), int(down), int(taps)
    if not (0 <= up < 1 << 32 and 0 <= down < 1 << 32 and 0 <= taps < 1 << 32):
        raise ValueError("up, down and taps are unsigned")
    fits = up * taps <= RESAMPLE_MAX_COEFS
    coef = np.zeros((max(up, 1), max(taps, 1)) if fits else (1, 1), dtype=np.int16)
    shift, before = C.c_uint32(0), C.c_uint32(0)
    ret = lib.LINNEAmd_ResampleDesign(up, down, taps, coef.ctypes.data_as(C.POINTER(C.c_int16)), C.byref(shift), C.byref(before))
    if ret != 0:
        raise ValueError(f"resample_design({up}, {down}, {taps}) -> {ret}: up and down are 1 .. {RESAMPLE_MAX_RATIO}, taps 1 .. {RESAMPLE_MAX_TAPS}, up * taps <= {RESAMPLE_MAX_COEFS}")
    return coef, int(shift.value), int(before.value)


class ProjectSpec(C.Structure):
    """struct LINNEAmdProjectSpec (include/linne_amd.h); basis is host memory"""
    _fields_ = [("frame_len", C.c_uint32), ("hop", C.c_uint32), ("num_rows", C.c_uint32), ("before", C.c_uint32), ("shift", C.c_uint32),
                ("clip_bits", C.c_uint32), ("format", C.c_uint32), ("float_exp", C.c_uint32), ("channel_stride", C.c_uint64),
                ("frame_stride", C.c_uint64), ("row_stride", C.c_uint64), ("saturated", C.c_uint32), ("reserved", C.c_uint32),
                ("basis", C.POINTER(C.c_int16))]


PROJECT_MAX_FRAME, PROJECT_MAX_ROWS, PROJECT_MAX_HOP, PROJECT_MAX_PRODUCTS = 4096, 2048, 65536, 1 << 40     # include/linne_amd.h LINNE_AMD_PROJECT_MAX_*
PROJECT_WINDOWS = {"rect": 0, "rectangular": 0, "hann": 1}


def project_length(num_samples, hop):
    """LINNEAmd_ProjectLength: the frames of a stream of num_samples samples, ceil(num_samples / hop)"""
    return int(lib.LINNEAmd_ProjectLength(int(num_samples), int(hop)))


def project_design(n_fft, bins=None, window="hann"):
    """LINNEAmd_ProjectDesign -> the DFT basis as int16 (2 * bins, n_fft): row 2 j the cosine of bin j, row 2 j + 1 its negated sine,
    under the periodic Hann window or none ("rect"), scaled by 32767.  bins None: n_fft // 2 + 1.  ValueError for arguments outside the
    call's bounds.  Pure host code: no device is needed"""
    n_fft = int(n_fft)
    bins = n_fft // 2 + 1 if bins is None else int(bins)
    if window not in PROJECT_WINDOWS:
        raise ValueError(f"window is one of {sorted(PROJECT_WINDOWS)}")
    if not (0 <= n_fft < 1 << 32 and 0 <= bins < 1 << 32):
        raise ValueError("n_fft and bins are unsigned")
    fits = 1 <= n_fft <= PROJECT_MAX_FRAME and 2 * bins <= PROJECT_MAX_ROWS
    basis = np.zeros((2 * max(bins, 1), n_fft) if fits else (1, 1), dtype=np.int16)
    ret = lib.LINNEAmd_ProjectDesign(n_fft, bins, PROJECT_WINDOWS[window], basis.ctypes.data_as(C.POINTER(C.c_int16)))
    if ret != 0:
        raise ValueError(f"project_design({n_fft}, {bins}) -> {ret}: n_fft is 1 .. {PROJECT_MAX_FRAME}, bins 1 .. n_fft // 2 + 1, 2 * bins <= {PROJECT_MAX_ROWS}")
    return basis


class OverlaySource(C.Structure):
    """struct LINNEAmdOverlaySource (include/linne_amd.h)"""
    _fields_ = [("index", C.c_void_p), ("d_stream", C.c_void_p), ("first_sample", C.c_uint64), ("num_samples", C.c_uint64),
                ("at", C.c_uint64), ("gain_q32", C.c_int64), ("step_q32", C.c_int64), ("reserved", C.c_uint64)]


class Overlay(C.Structure):
    """struct LINNEAmdOverlay (include/linne_amd.h); sources is host memory"""
    _fields_ = [("sources", C.POINTER(OverlaySource)), ("num_sources", C.c_uint32), ("shift", C.c_uint32), ("clip_bits", C.c_uint32),
                ("reserved", C.c_uint32), ("num_samples", C.c_uint64), ("d_pcm", C.c_void_p), ("pcm_stride", C.c_uint64), ("result", C.c_int32)]


OVERLAY_MAX_SOURCES = 64                # include/linne_amd.h LINNE_AMD_OVERLAY_MAX_SOURCES


def overlay_gain(gain_q32, step_q32, i):
    """the gain LINNEAmd_OverlayWindowsDevice gives sample i of a source: (gain_q32 + step_q32 * i) >> 32, the floor"""
    return (int(gain_q32) + int(step_q32) * int(i)) >> 32


def fade(g0, g1, n):
    """a linear ramp for overlay_windows -> (gain_q32, step_q32): exactly g0 at sample 0, and g1 reached at sample n, one past the last
    of the n samples it is for (the step is rounded towards g0, and half a unit of 2^-32 keeps the floor of sample 0 at g0 when the
    ramp falls); g0 and g1 are int16 gains and n is 1 .. 2^31 -- beyond that the rounded step could miss g1 by one --, anything else
    raises ValueError.  Pure host code"""
    g0, g1, n = int(g0), int(g1), int(n)
    if not 1 <= n <= 1 << 31 or not (-32768 <= g0 <= 32767 and -32768 <= g1 <= 32767):
        raise ValueError(f"fade({g0}, {g1}, {n}): the gains are int16, n is 1 .. 2^31")
    span = (g1 - g0) << 32
    step = span // n if span >= 0 else -((-span) // n)
    return (g0 << 32) + (1 << 31), step


def crossfade(n, unity):
    """the two ramps of a linear crossfade over n samples -> ((gain_q32, step_q32) of the stream that leaves, of the stream that
    comes): the first falls from `unity` towards 0, the second is (unity << 32) + (1 << 32) - 1 - the first with the negated step, so
    that the two gains add up to exactly `unity` at every one of the n samples.  Pure host code"""
    n, unity = int(n), int(unity)
    if not 1 <= n <= 1 << 31 or not 1 <= unity <= 32767:
        raise ValueError(f"crossfade({n}, {unity}): n is 1 .. 2^31, unity 1 .. 32767")
    a, step = fade(unity, 0, n)
    return (a, step), ((unity << 32) + (1 << 32) - 1 - a, -step)


class LagSum(C.Structure):
    """struct LINNEAmdLagSum (include/linne_amd.h): one channel pair at one lag"""
    _fields_ = [("dot_lo", C.c_uint64), ("dot_hi", C.c_int64), ("b_sq_lo", C.c_uint64), ("b_sq_hi", C.c_uint64)]


class LagProbe(C.Structure):
    """struct LINNEAmdLagProbe (include/linne_amd.h)"""
    _fields_ = [("index_a", C.c_void_p), ("d_stream_a", C.c_void_p), ("first_a", C.c_uint64), ("num_samples", C.c_uint64),
                ("index_b", C.c_void_p), ("d_stream_b", C.c_void_p), ("first_b", C.c_uint64), ("lag_first", C.c_int64), ("num_lags", C.c_uint32),
                ("num_pairs", C.c_uint32), ("chan_a", C.c_uint8 * 8), ("chan_b", C.c_uint8 * 8), ("d_out", C.c_void_p), ("pair_stride", C.c_uint64),
                ("d_a_sq", C.c_void_p), ("reserved", C.c_uint64), ("result", C.c_int32)]


LAG_MAX_LAGS, LAG_MAX_PRODUCTS = 65536, 1 << 38      # include/linne_amd.h LINNE_AMD_LAG_MAX_*
LAG_DTYPE = np.dtype([("dot_lo", "<u8"), ("dot_hi", "<i8"), ("b_sq_lo", "<u8"), ("b_sq_hi", "<u8")])


class LagSums:
    """one probe's table of lag_windows: `records`, an int64 CUDA tensor (P, num_lags, 4) holding a struct LINNEAmdLagSum per channel
    pair and lag, `a_sq`, an int64 CUDA tensor (P, 2) holding the needle's sum of squares per pair (low word, high word), and what
    the probe asked: lag_first and pairs, the (channel of a, channel of b) of every row"""

    def __init__(self, records, a_sq, lag_first, pairs):
        self.records, self.a_sq, self.lag_first, self.pairs = records, a_sq, int(lag_first), tuple(pairs)

    def cpu(self):
        """-> a numpy structured array (P, num_lags) with the fields dot_lo (unsigned), dot_hi, b_sq_lo and b_sq_hi (unsigned)"""
        a = np.ascontiguousarray(self.records.cpu().numpy())
        return a.view(LAG_DTYPE).reshape(a.shape[:2])

    def a_squares(self):
        """the needle's exact sums of squares: a list [P] of Python integers"""
        return [(int(hi) << 64) + int(lo) for lo, hi in np.ascontiguousarray(self.a_sq.cpu().numpy()).view(np.uint64).reshape(-1, 2)]


def _lag_table(table):
    """a LagSums or its .cpu() -> the structured array (P, num_lags)"""
    a = table.cpu() if isinstance(table, LagSums) else np.asarray(table)
    assert a.dtype == LAG_DTYPE and a.ndim == 2, "a lag table is a LagSums or a LAG_DTYPE array (P, num_lags)"
    return a


def lag_dots(table):
    """the exact sums of products of a LagSums or its .cpu(): a list [P][num_lags] of Python integers, dot_hi * 2^64 + dot_lo"""
    return [[(int(r["dot_hi"]) << 64) + int(r["dot_lo"]) for r in row] for row in _lag_table(table)]


def lag_energies(table):
    """the exact sums of b^2 under the needle, likewise: a list [P][num_lags] of Python integers"""
    return [[(int(r["b_sq_hi"]) << 64) + int(r["b_sq_lo"]) for r in row] for row in _lag_table(table)]


def lag_correlation(table, a_sq=None):
    """the correlation coefficients of a LagSums -> float64 (P, num_lags): dot / sqrt(a_sq * b_sq) per pair and lag, NaN where an energy
    is 0.  a_sq: the needle's sums of squares per pair (Python integers), needed where `table` is a .cpu() array and not the LagSums.
    The integers are divided as such, as `correlation` does.  Pure host code"""
    from fractions import Fraction
    if a_sq is None:
        assert isinstance(table, LagSums), "a_sq is needed beside a bare table"
        a_sq = table.a_squares()
    dots, bsq = lag_dots(table), lag_energies(table)
    out = np.full((len(dots), len(dots[0]) if dots else 0), np.nan, dtype=np.float64)
    for p, row in enumerate(dots):
        for l, d in enumerate(row):
            if a_sq[p] > 0 and bsq[p][l] > 0:
                r = math.sqrt(Fraction(d * d, int(a_sq[p]) * bsq[p][l]))
                out[p, l] = -r if d < 0 else r
    return out


def best_lag(table, lag_first=None, a_sq=None):
    """the lag at which the haystack best matches the needle -> (lag, coefficient).  The pairs' dots and energies are added per lag;
    the lag maximises dot / sqrt(b_sq), candidates compared exactly by cross-multiplied integers (a lag whose b_sq is 0 has the
    value 0); ties go to the smaller |lag|, then to the negative lag.  The coefficient is dot / sqrt(a_sq * b_sq) of the sums there,
    NaN where an energy is 0 or a_sq is not known.  lag_first and a_sq default to the LagSums' own.  Pure host code"""
    from fractions import Fraction
    if isinstance(table, LagSums):
        lag_first = table.lag_first if lag_first is None else lag_first
        a_sq = table.a_squares() if a_sq is None else a_sq
    assert lag_first is not None, "lag_first is needed beside a bare table"
    lag_first = int(lag_first)
    dots, bsq = lag_dots(table), lag_energies(table)
    assert dots and dots[0], "a table of at least one pair and one lag"
    d = [sum(row[l] for row in dots) for l in range(len(dots[0]))]
    e = [sum(row[l] for row in bsq) for l in range(len(dots[0]))]

    def above(i, j):
        """is d_i / sqrt(e_i) > d_j / sqrt(e_j)?  (0 where e is 0)"""
        di, dj = (d[i] if e[i] else 0), (d[j] if e[j] else 0)
        ei, ej = (e[i] or 1), (e[j] or 1)
        if (di > 0) != (dj > 0) or di == 0 or dj == 0:
            return di > dj
        lhs, rhs = di * di * ej, dj * dj * ei                      # both of one sign: compare the squares, the other way round below 0
        return lhs > rhs if di > 0 else lhs < rhs

    best = 0
    for l in range(1, len(d)):
        La, Lb = lag_first + l, lag_first + best
        if above(l, best) or (not above(best, l) and (abs(La), La) < (abs(Lb), Lb)):
            best = l
    ea = sum(int(v) for v in a_sq) if a_sq is not None else 0
    coef = float("nan")
    if ea > 0 and e[best] > 0:
        coef = math.sqrt(Fraction(d[best] * d[best], ea * e[best])) * (-1 if d[best] < 0 else 1)
    return lag_first + best, coef


RELATION_DTYPE = np.dtype([("dot_lo", "<u8"), ("dot_hi", "<i8"), ("num_equal", "<u8"), ("num_opposite", "<u8")])


def pair_index(C, i, j):
    """LINNE_AMD_PAIR (include/linne_amd.h): the place of channel pair (i, j), i <= j < C, in the upper triangle taken row by row"""
    C, i, j = int(C), int(i), int(j)
    assert 0 <= i <= j < C, "a pair is i <= j < C"
    return i * C - i * (i - 1) // 2 + (j - i)


def downmix_matrix(C):
    """the matrix and shift that make one channel, the mean, of C -> (matrix, shift) as mix_windows takes them: a row of ones and
    shift log2(C) where C is a power of two (the shift's rounding is the mean's: halves towards plus infinity), otherwise a row of
    round(2^15 / C) in Q15 and shift 15.  Pure host code"""
    C = int(C)
    assert 1 <= C <= 8, "1 .. 8 channels"
    if C & (C - 1) == 0:
        return ((1,) * C,), C.bit_length() - 1
    return ((int(round(32768 / C)),) * C,), 15


def select_matrix(C, channels):
    """the matrix that keeps the given channels of C, in the given order (a channel may repeat) -> a tuple of rows of 0 and 1"""
    C, channels = int(C), [int(c) for c in channels]
    assert 1 <= C <= 8 and 1 <= len(channels) <= 8 and all(0 <= c < C for c in channels), "1 .. 8 channels out of C <= 8"
    return tuple(tuple(int(c == k) for c in range(C)) for k in channels)


def fix_matrix(findings):
    """one bucket of channel_findings -> the matrix that acts on it: of an "identical" pair (i, j) channel j is dropped, of an
    "inverted" pair channel j is negated; every other channel is kept as it is.  A pair with a channel already dropped changes
    nothing further.  Pure host code"""
    C = len(findings["channels"])
    keep, sign = [True] * C, [1] * C
    for (i, j), what in sorted(findings["pairs"].items()):
        if not (keep[i] and keep[j]):
            continue
        if what == "identical":
            keep[j] = False
        elif what == "inverted":
            sign[j] = -1
    return tuple(tuple(sign[k] * int(c == k) for c in range(C)) for k in range(C) if keep[k])


def _pair_channels(P):
    """the channel count whose upper triangle has P pairs"""
    C = (math.isqrt(8 * int(P) + 1) - 1) // 2
    assert C >= 1 and C * (C + 1) // 2 == int(P), f"{P} is not a number of channel pairs"
    return C


class Relations:
    """one window's table of relate_windows: `records`, an int64 CUDA tensor (P, nb, 4) holding a struct LINNEAmdRelation per channel
    pair (pair_index) and bucket, and strided views of it -- dot_lo, dot_hi (the unsigned low and the signed high word of the 128-bit
    sum of a_i * a_j), num_equal and num_opposite, each int64 (P, nb)"""

    def __init__(self, records, bucket_samples):
        self.records, self.bucket_samples = records, bucket_samples
        self.dot_lo, self.dot_hi, self.num_equal, self.num_opposite = records[..., 0], records[..., 1], records[..., 2], records[..., 3]
        self.num_channels = _pair_channels(records.shape[0])

    def dot(self):
        """the sums of products as float64 (P, nb), within two units in the last place.  A negative sum is negated in integers first
        (hi * 2^64 + lo in floating point would cancel: a small negative sum has hi = -1 and lo just below 2^64)"""
        import torch
        neg = self.dot_hi < 0
        lo = torch.where(neg, -self.dot_lo, self.dot_lo)               # (int64 wraps: the low word of the magnitude)
        hi = torch.where(neg, ~self.dot_hi + (self.dot_lo == 0).to(torch.int64), self.dot_hi)
        mag = hi.double() * 2.0 ** 64 + lo.double() + (lo < 0).double() * 2.0 ** 64
        return torch.where(neg, -mag, mag)

    def cpu(self):
        """-> a numpy structured array (P, nb) with the fields dot_lo (unsigned), dot_hi, num_equal, num_opposite"""
        a = np.ascontiguousarray(self.records.cpu().numpy())
        return a.view(RELATION_DTYPE).reshape(a.shape[:2])


def _relation_table(relation):
    """a Relations or its .cpu() -> (the structured array (P, nb), C)"""
    a = relation.cpu() if isinstance(relation, Relations) else np.asarray(relation)
    assert a.dtype == RELATION_DTYPE and a.ndim == 2, "a relation is a Relations or a RELATION_DTYPE array (P, nb)"
    return a, _pair_channels(a.shape[0])


def relation_dots(relation):
    """the exact sums of products of a Relations or its .cpu(): a list [P][nb] of Python integers, dot_hi * 2^64 + dot_lo"""
    a, _ = _relation_table(relation)
    return [[(int(r["dot_hi"]) << 64) + int(r["dot_lo"]) for r in row] for row in a]


def correlation(relation):
    """the correlation coefficients of a Relations or its .cpu() -> float64 (C, C, nb), symmetric: dot_ij / sqrt(dot_ii * dot_jj) per
    bucket, NaN where a channel's energy is 0.  The integers are divided as such (a 128-bit sum has no exact float64).  Pure host
    code"""
    from fractions import Fraction
    a, C = _relation_table(relation)
    dots, nb = relation_dots(a), a.shape[1]
    out = np.full((C, C, nb), np.nan, dtype=np.float64)
    for i in range(C):
        for j in range(i, C):
            for k in range(nb):
                ei, ej = dots[pair_index(C, i, i)][k], dots[pair_index(C, j, j)][k]
                if ei > 0 and ej > 0:
                    d = dots[pair_index(C, i, j)][k]
                    r = math.sqrt(Fraction(d * d, ei * ej))
                    out[i, j, k] = out[j, i, k] = -r if d < 0 else r
    return out


def channel_findings(relation):
    """what a Relations or its .cpu() says in words -> a list, one dict per bucket: {"pairs": {(i, j): finding, i < j}, "channels":
    {i: finding}}.  A pair is "identical" when num_equal is the bucket's frame count, "inverted" when num_opposite is and the two
    channels are not all zero, otherwise None; a channel is "silent" when all its samples are zero (num_opposite(i, i) is the frame
    count), otherwise None.  Pure host code"""
    a, C = _relation_table(relation)
    out = []
    for k in range(a.shape[1]):
        frames = int(a[0, k]["num_equal"])
        silent = [int(a[pair_index(C, i, i), k]["num_opposite"]) == frames for i in range(C)]
        pairs = {}
        for i in range(C):
            for j in range(i + 1, C):
                r = a[pair_index(C, i, j), k]
                pairs[(i, j)] = ("identical" if int(r["num_equal"]) == frames else
                                 "inverted" if int(r["num_opposite"]) == frames and not (silent[i] and silent[j]) else None)
        out.append({"pairs": pairs, "channels": {i: ("silent" if silent[i] else None) for i in range(C)}})
    return out


def sound_segments(num_samples, runs, pad=0):
    """the complement of quiet runs inside [0, num_samples): runs a sequence of (first, n) (a QuietRuns' .cpu(), or an array (k, 2)) ->
    a list of (first, n) in ascending order, every segment widened by `pad` frames at both ends (not beyond [0, num_samples)) and
    segments that then touch or overlap merged: what splice_streams takes as the cuts that keep the sound.  Pure host code"""
    num_samples, pad = int(num_samples), int(pad)
    assert pad >= 0, "pad is a number of frames >= 0"
    quiet = sorted((max(int(a), 0), min(int(a) + int(n), num_samples)) for a, n in runs)
    loud, at = [], 0
    for a, b in quiet:
        if a > at:
            loud.append((at, a))
        at = max(at, b)
    if at < num_samples:
        loud.append((at, num_samples))
    out = []
    for a, b in loud:
        a, b = max(a - pad, 0), min(b + pad, num_samples)
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return [(a, b - a) for a, b in out]


def _load():
    # torch bundles its own HIP runtime (same soname as /opt/rocm's).  Importing torch FIRST makes
    # liblinne_amd.so bind to that already-loaded runtime, so both share one HIP context: torch tensors can
    # be handed to the C-ABI and torch.cuda streams/events see our work.  The other order loads two runtimes.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C linne_amd/csrc`). linne_amd has no pure-Python or CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.LINNEAmd_GetDeviceCount.restype = C.c_int
    L.LINNEAmd_ContextCreate.restype = C.c_void_p
    L.LINNEAmd_ContextCreate.argtypes = [C.c_int, C.c_uint64]
    L.LINNEAmd_ContextDestroy.argtypes = [C.c_void_p]
    L.LINNEAmd_GetLastError.restype = C.c_char_p
    L.LINNEAmd_GetLastError.argtypes = [C.c_void_p]
    L.LINNEAmd_ReserveScratch.argtypes = [C.c_void_p, C.c_uint64]
    L.LINNEAmd_ScratchBytesPerFrame.restype = C.c_uint64
    L.LINNEAmd_ScratchBytesPerFrame.argtypes = [C.POINTER(Shape)]
    L.LINNEAmd_SetStream.argtypes = [C.c_void_p, C.c_void_p]
    L.LINNEAmd_EncodeFramesDevice.argtypes = [C.c_void_p, C.POINTER(Shape), C.c_void_p, C.c_void_p, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.LINNEAmd_DecodeFramesDevice.argtypes = [C.c_void_p, C.POINTER(Shape), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.LINNEAmd_EncodeFramesHost.argtypes = [C.c_void_p, C.POINTER(Shape), C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
    L.LINNEAmd_DecodeFramesHost.argtypes = [C.c_void_p, C.POINTER(Shape), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.LINNEAmd_Synchronize.argtypes = [C.c_void_p]
    L.LINNEAmd_GetLastFallbackCount.restype = C.c_int64
    L.LINNEAmd_GetLastFallbackCount.argtypes = [C.c_void_p]
    L.LINNEAmd_SetAfIterations.argtypes = [C.c_void_p, C.c_uint32]
    L.LINNEAmd_SetLearning.argtypes = [C.c_void_p, C.c_uint32]
    L.LINNEAmd_GetLastMinMargin.restype = C.c_double
    L.LINNEAmd_GetLastMinMargin.argtypes = [C.c_void_p]
    L.LINNEAmd_SetSearchCapture.argtypes = [C.c_void_p, C.c_int]
    L.LINNEAmd_GetLastSearchCapture.restype = C.c_int64
    L.LINNEAmd_GetLastSearchCapture.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.LINNEAmd_GetLastTimingMs.restype = C.c_double
    L.LINNEAmd_GetLastTimingMs.argtypes = [C.c_void_p, C.c_int]
    L.LINNEAmd_EnableTiming.argtypes = [C.c_void_p, C.c_int]
    L.LINNEAmd_GetLastTimingLaunches.restype = C.c_int
    L.LINNEAmd_GetLastTimingLaunches.argtypes = [C.c_void_p, C.c_int]
    L.LINNEAmd_PackFrames.argtypes = [C.POINTER(Shape), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_double), C.c_uint32]
    L.LINNEAmd_PackFramesPlanned.argtypes = [C.POINTER(Shape), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_double), C.c_uint32]
    L.LINNEAmd_RicePlanDevice.argtypes = [C.c_void_p, C.POINTER(Shape), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.LINNEAmd_RiceEmitDevice.argtypes = [C.c_void_p, C.POINTER(Shape), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.LINNEAmd_PackFramesEmitted.argtypes = [C.POINTER(Shape), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                             C.POINTER(C.c_double), C.c_uint32]
    L.LINNEAmd_StreamIndexCreate.restype = C.c_void_p
    L.LINNEAmd_StreamIndexCreate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]
    L.LINNEAmd_StreamIndexDestroy.argtypes = [C.c_void_p]
    L.LINNEAmd_StreamIndexHeader.argtypes = [C.c_void_p, C.POINTER(Header)]
    L.LINNEAmd_StreamIndexNumBlocks.restype = C.c_uint32
    L.LINNEAmd_StreamIndexNumBlocks.argtypes = [C.c_void_p]
    L.LINNEAmd_DecodeStreamDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    L.LINNEAmd_StreamIndexesCreate.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
    L.LINNEAmd_GetLastIndexBatchCount.restype = C.c_int64
    L.LINNEAmd_GetLastIndexBatchCount.argtypes = [C.c_void_p, C.c_int]
    L.LINNEAmd_StreamIndexBlocks.argtypes = [C.c_void_p] + [C.POINTER(C.POINTER(C.c_uint64))] * 2 + [C.POINTER(C.POINTER(C.c_uint32))] * 3
    L.LINNEAmd_StreamIndexFailure.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    L.LINNEAmd_DecodeWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Window), C.c_uint32, C.c_uint32]
    L.LINNEAmd_EncodeStreamBound.restype = C.c_uint64
    L.LINNEAmd_EncodeStreamBound.argtypes = [C.POINTER(Header)]
    L.LINNEAmd_EncodeStreamDevice.argtypes = [C.c_void_p, C.POINTER(Header), C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    L.LINNEAmd_GetLastStreamEncodeCount.restype = C.c_int64
    L.LINNEAmd_GetLastStreamEncodeCount.argtypes = [C.c_void_p, C.c_int]
    L.LINNEAmd_EncodeStreamsDevice.argtypes = [C.c_void_p, C.POINTER(Track), C.c_uint32, C.c_uint32]
    L.LINNEAmd_EncodeStreamDeviceLayout.argtypes = [C.c_void_p, C.POINTER(Header), C.c_void_p, C.POINTER(PcmLayout), C.c_uint32, C.c_void_p, C.c_uint64,
                                                    C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    L.LINNEAmd_EncodeStreamsDeviceLayout.argtypes = [C.c_void_p, C.POINTER(Track), C.POINTER(PcmLayout), C.c_uint32, C.c_uint32]
    L.LINNEAmd_DecodeWindowsDeviceLayout.argtypes = [C.c_void_p, C.POINTER(Window), C.POINTER(PcmLayout), C.c_uint32, C.c_uint32]
    L.LINNEAmd_CompareWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Window), C.POINTER(PcmLayout), C.POINTER(Diff), C.c_uint32, C.c_uint32]
    L.LINNEAmd_MeasureWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Window), C.POINTER(MeasureSpec), C.c_uint32, C.c_uint32]
    L.LINNEAmd_DigestWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Window), C.POINTER(DigestSpec), C.c_uint32, C.c_uint32]
    L.LINNEAmd_QuietWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Window), C.POINTER(QuietSpec), C.POINTER(Quiet), C.c_uint32, C.c_uint32]
    L.LINNEAmd_HistogramWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Window), C.POINTER(HistogramSpec), C.c_uint32, C.c_uint32]
    L.LINNEAmd_RelateWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Window), C.POINTER(RelateSpec), C.c_uint32, C.c_uint32]
    L.LINNEAmd_MixWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Window), C.POINTER(MixSpec), C.POINTER(PcmLayout), C.c_uint32, C.c_uint32]
    L.LINNEAmd_ResampleWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Window), C.POINTER(ResampleSpec), C.POINTER(PcmLayout), C.c_uint32, C.c_uint32]
    L.LINNEAmd_ResampleLength.restype = C.c_uint64
    L.LINNEAmd_ResampleLength.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    L.LINNEAmd_ResampleDesign.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.LINNEAmd_ProjectWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Window), C.POINTER(ProjectSpec), C.c_uint32, C.c_uint32]
    L.LINNEAmd_ProjectLength.restype = C.c_uint64
    L.LINNEAmd_ProjectLength.argtypes = [C.c_uint64, C.c_uint32]
    L.LINNEAmd_ProjectDesign.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int16)]
    L.LINNEAmd_OverlayWindowsDevice.argtypes = [C.c_void_p, C.POINTER(Overlay), C.POINTER(PcmLayout), C.c_uint32, C.c_uint32]
    L.LINNEAmd_LagWindowsDevice.argtypes = [C.c_void_p, C.POINTER(LagProbe), C.c_uint32, C.c_uint32]
    L.LINNEAmd_SpliceStreamsDevice.argtypes = [C.c_void_p, C.POINTER(Splice), C.c_uint32, C.c_uint32]
    L.LINNEAmd_GetLastSpliceCount.restype = C.c_int64
    L.LINNEAmd_GetLastSpliceCount.argtypes = [C.c_void_p, C.c_int]
    L.LINNEAmd_RepairStreamsDevice.argtypes = [C.c_void_p, C.POINTER(Repair), C.c_uint32]
    L.LINNEAmd_GetLastRepairGaps.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(Gap)), C.POINTER(C.c_uint32)]
    L.LINNEAmd_GetLastRepairCount.restype = C.c_int64
    L.LINNEAmd_GetLastRepairCount.argtypes = [C.c_void_p, C.c_int]
    L.LINNEAmd_GetLastStreamBatchCount.restype = C.c_int64
    L.LINNEAmd_GetLastStreamBatchCount.argtypes = [C.c_void_p, C.c_int]
    L.LINNEAmd_MultiCreate.restype = C.c_void_p
    L.LINNEAmd_MultiCreate.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    L.LINNEAmd_MultiDestroy.argtypes = [C.c_void_p]
    L.LINNEAmd_MultiNumDevices.restype = C.c_uint32
    L.LINNEAmd_MultiNumDevices.argtypes = [C.c_void_p]
    L.LINNEAmd_MultiDevice.argtypes = [C.c_void_p, C.c_uint32]
    L.LINNEAmd_MultiContext.restype = C.c_void_p
    L.LINNEAmd_MultiContext.argtypes = [C.c_void_p, C.c_uint32]
    L.LINNEAmd_MultiGetLastError.restype = C.c_char_p
    L.LINNEAmd_MultiGetLastError.argtypes = [C.c_void_p]
    L.LINNEAmd_MultiEncodeFramesHost.argtypes = [C.c_void_p, C.POINTER(Shape), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_uint32]
    L.LINNEAmd_MultiDecodeFramesHost.argtypes = [C.c_void_p, C.POINTER(Shape), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    return L


lib = _load()


def device_count():
    return int(lib.LINNEAmd_GetDeviceCount())


class LinneAmdError(RuntimeError):
    """code: the LINNEApiResult of the failing call, where one is known; codes: those of a batch's members (decode_windows,
    encode_streams; a verified encode: 7 for a track that differs)"""

    def __init__(self, msg, code=None, codes=None):
        super().__init__(msg)
        self.code = code
        self.codes = codes


class StreamIndex:
    """the block index of one .lnn stream in device memory (Context.index_stream; include/linne_amd.h LINNEAmd_StreamIndexCreate)"""

    def __init__(self, handle, header, num_blocks, nbytes):
        self.h = handle
        self.header = header
        self.num_blocks = num_blocks
        self.nbytes = nbytes

    @classmethod
    def of(cls, handle, nbytes):
        """the StreamIndex of a handle the library gave for a stream of nbytes bytes"""
        hd = Header()
        lib.LINNEAmd_StreamIndexHeader(handle, C.byref(hd))
        return cls(handle, {k: int(getattr(hd, k)) for k, _ in Header._fields_}, int(lib.LINNEAmd_StreamIndexNumBlocks(handle)), nbytes)

    def blocks(self):
        """the blocks a whole decode walks -> numpy copies (off, first, size, type, nsmp): byte offsets, first samples (num_blocks + 1
        entries), size fields, types (0 COMPRESS, 1 SILENT, 2 RAW) and sample counts (LINNEAmd_StreamIndexBlocks)"""
        off, first = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        size, typ, nsmp = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        ret = lib.LINNEAmd_StreamIndexBlocks(self.h, C.byref(off), C.byref(first), C.byref(size), C.byref(typ), C.byref(nsmp))
        if ret != 0:
            raise LinneAmdError(f"StreamIndexBlocks -> {ret}", ret)
        n = self.num_blocks
        take = lambda p, k, dt: np.array(p[:k], dtype=dt)
        return take(off, n, np.uint64), take(first, n + 1, np.uint64), take(size, n, np.uint32), take(typ, n, np.uint32), take(nsmp, n, np.uint32)

    def failure(self):
        """(block, code, byte) of the lowest failing block: block -1 (code 0) when there is none, num_blocks for the place behind the
        last block (LINNEAmd_StreamIndexFailure)"""
        block, code, byte = C.c_int64(0), C.c_int32(0), C.c_uint64(0)
        ret = lib.LINNEAmd_StreamIndexFailure(self.h, C.byref(block), C.byref(code), C.byref(byte))
        if ret != 0:
            raise LinneAmdError(f"StreamIndexFailure -> {ret}", ret)
        return int(block.value), int(code.value), int(byte.value)

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.LINNEAmd_StreamIndexDestroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _per_window(value, W, what, lo=0, hi=None, scalars=(int, np.integer)):
    """an argument that is one value or one per window -> a list of W integers, each >= lo (None: any) and < hi (None: any)"""
    vs = [int(value)] * W if isinstance(value, scalars) else [int(v) for v in value]
    rule = "" if lo is None else f" >= {lo}" if hi is None else f" in {lo} .. 2^{hi.bit_length() - 1} - 1"
    assert len(vs) == W and all((lo is None or v >= lo) and (hi is None or v < hi) for v in vs), f"{what} is one value{rule}, or one per window"
    return vs


def _sample_range(index, nbytes, first, n, where, *at):
    """the range (first, n) of a stream of nbytes bytes against its index, n None: to the stream's end -> (first, n, the num_samples
    a C struct takes: a negative n as a count no stream has, which the call refuses).  where % at names the range in the assertion"""
    assert index.nbytes == nbytes, f"{where % at}: the index was built for a stream of another length"
    first = int(first)
    n = index.header["num_samples"] - first if n is None else int(n)
    return first, n, n if n >= 0 else (1 << 64) - 1


def _default_room(nch, ns, bits):
    """the bytes encode_stream and encode_streams give a track's stream at first: what the reference's command line tool allocates"""
    return 2 * nch * ns * ((bits + 7) // 8) + 30


# The windows calls that answer per bucket, as _bucket_windows runs them (tests/stream_consumers.py holds the same table for the tests):
# the spec struct; the C entry point; the 64-bit words of a bucket (None: the caller's, per window); the rows of a window's table in
# front of (buckets, words), from its channel count; the spec's stride field; the answer of a window from (its table, its bucket length,
# its index, the spec's further fields)
_BUCKET_CONSUMERS = {
    "measure": (MeasureSpec, "LINNEAmd_MeasureWindowsDevice", 4, lambda c: (c,), "channel_stride", lambda t, b, x: Measurement(t, b)),
    "digest": (DigestSpec, "LINNEAmd_DigestWindowsDevice", 2, lambda c: (), None, lambda t, b, x: DigestTable(t, b, x.header)),
    "histogram": (HistogramSpec, "LINNEAmd_HistogramWindowsDevice", None, lambda c: (c,), "channel_stride",
                  lambda t, b, x, bins, shift, scale: Histogram(t, bins, shift, bool(scale), b)),
    "relate": (RelateSpec, "LINNEAmd_RelateWindowsDevice", 4, lambda c: (c * (c + 1) // 2,), "pair_stride", lambda t, b, x: Relations(t, b)),
}


class Context:
    """Batch hot path on one GPU (include/linne_amd.h).  Tensors are torch int32/float64 CUDA(HIP) tensors."""

    def __init__(self, device=0, scratch_bytes=0, use_torch_stream=True):
        self.h = lib.LINNEAmd_ContextCreate(int(device), int(scratch_bytes))
        if not self.h:
            raise LinneAmdError(f"LINNEAmd_ContextCreate(device={device}) failed: no usable HIP device "
                                "(the prediction path has no CPU fallback)")
        self.device = int(device)
        self._verify = False
        # With its own stream the library's kernels are NOT ordered behind what torch enqueued on torch's stream -- the fill kernel of a
        # torch.zeros, a clone, a copy from the host: the binding then drains torch's stream before every call that touches tensors
        # (_fence).  It went unnoticed while both streams happened to share a hardware queue; with the library's 24 queues they do not.
        self._own_stream = not use_torch_stream
        if use_torch_stream:
            import torch
            s = torch.cuda.current_stream(self.device).cuda_stream
            self._check(lib.LINNEAmd_SetStream(self.h, C.c_void_p(s)), "SetStream")

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.LINNEAmd_ContextDestroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, ret, what):
        if ret != 0:
            raise LinneAmdError(f"{what} -> {ret}: {lib.LINNEAmd_GetLastError(self.h).decode()}", ret)

    def _fence(self):
        """own stream: everything torch has enqueued so far (allocations' fills, clones, H2D copies) is done before the library runs"""
        if self._own_stream:
            import torch
            torch.cuda.current_stream(self.device).synchronize()

    @staticmethod
    def shape(nch, bits, block, preset, ms):
        return Shape(nch, bits, block, preset, int(ms))

    def reserve(self, nbytes):
        self._check(lib.LINNEAmd_ReserveScratch(self.h, int(nbytes)), "ReserveScratch")

    def enable_timing(self, on=True):
        lib.LINNEAmd_EnableTiming(self.h, int(on))

    def last_ms(self, which=0):
        return float(lib.LINNEAmd_GetLastTimingMs(self.h, which))

    def last_launches(self, which):
        return int(lib.LINNEAmd_GetLastTimingLaunches(self.h, which))

    def last_fallback_count(self):
        return int(lib.LINNEAmd_GetLastFallbackCount(self.h))

    def set_learning(self, on):
        self._check(lib.LINNEAmd_SetLearning(self.h, int(bool(on))), "SetLearning")

    def set_verify(self, on):
        """a setting of the context like -l and -a N: encode_stream and encode_streams compare every stream they are about to return
        with the PCM it was made from (verify_streams) and raise LinneAmdError (code 7) when one differs.  (A setting, not a
        parameter of the two calls: their parameter lists are pinned.)  The bytes do not change"""
        self._verify = bool(on)

    def set_af_iterations(self, n):
        self._check(lib.LINNEAmd_SetAfIterations(self.h, int(n)), "SetAfIterations")

    def last_min_margin(self):
        return float(lib.LINNEAmd_GetLastMinMargin(self.h))

    def set_search_capture(self, on=True):
        """test instrument (include/linne_amd.h LINNEAmd_SetSearchCapture): the encode calls record what every unit-count search was decided from"""
        self._check(lib.LINNEAmd_SetSearchCapture(self.h, int(bool(on))), "SetSearchCapture")

    def last_search_capture(self, shape, num_frames):
        """the last encode call's records as float64 [F][C][R][L][CAPTURE_TRIALS][CAPTURE_WORDS] (words: CAP_*; NaN = not computed / no such trial)"""
        R, nl = PRESET_NUM_REGULARS[shape.preset], len(PRESET_LAYERS[shape.preset])
        out = np.full((int(num_frames), shape.num_channels, R, nl, CAPTURE_TRIALS, CAPTURE_WORDS), np.nan)
        n = int(lib.LINNEAmd_GetLastSearchCapture(self.h, out.ctypes.data, out.size // CAPTURE_WORDS))
        if n != out.size // CAPTURE_WORDS:
            raise LinneAmdError(f"GetLastSearchCapture -> {n} records, {out.size // CAPTURE_WORDS} expected "
                                f"(capture off, or another shape?): {lib.LINNEAmd_GetLastError(self.h).decode()}")
        return out

    def synchronize(self):
        self._check(lib.LINNEAmd_Synchronize(self.h), "Synchronize")

    def encode_frames(self, shape, pcm, num_samples=None, out=None):
        """pcm: int32 cuda tensor [F][C][S] -> (residual [F][C][S] int32, params [F][C][160] int32, stats [F][C][8] f64)"""
        import torch
        F, Cn, S = pcm.shape
        assert pcm.dtype == torch.int32 and pcm.is_cuda and pcm.is_contiguous()
        assert Cn == shape.num_channels and S == shape.num_samples_per_block
        if out is None:
            res = torch.empty_like(pcm)
            prm = torch.zeros((F, Cn, PARAM_WORDS), dtype=torch.int32, device=pcm.device)
            st = torch.zeros((F, Cn, STAT_WORDS), dtype=torch.float64, device=pcm.device)
        else:
            res, prm, st = out
        ns = None
        if num_samples is not None:
            ns = np.ascontiguousarray(num_samples, dtype=np.uint32)
            assert ns.shape == (F,)
        self._fence()
        self._check(lib.LINNEAmd_EncodeFramesDevice(self.h, C.byref(shape), pcm.data_ptr(), ns.ctypes.data if ns is not None else None,
                                                    F, res.data_ptr(), prm.data_ptr(), st.data_ptr()), "EncodeFramesDevice")
        return res, prm, st

    def rice_plan(self, shape, residual, num_samples=None):
        """residual: int32 cuda tensor [F][C][S] -> uint8 cuda tensor [F][C][RICE_PLAN_BYTES] (order, flag, parameters)"""
        import torch
        F, Cn, S = residual.shape
        assert residual.dtype == torch.int32 and residual.is_cuda and residual.is_contiguous()
        plan = torch.zeros((F, Cn, RICE_PLAN_BYTES), dtype=torch.uint8, device=residual.device)
        ns = np.ascontiguousarray(num_samples, dtype=np.uint32) if num_samples is not None else None
        self._fence()
        self._check(lib.LINNEAmd_RicePlanDevice(self.h, C.byref(shape), residual.data_ptr(), ns.ctypes.data if ns is not None else None,
                                                F, plan.data_ptr()), "RicePlanDevice")
        return plan

    def rice_emit(self, shape, residual, plan, capacity_bytes=None):
        """residual int32 cuda [F][C][S], plan = rice_plan(...) of the same batch -> (packed uint8 cuda [capacity], offsets uint32-as-int32
        cuda [F*C+1]): every channel-frame's Rice code, written by the device (include/linne_amd.h LINNEAmd_RiceEmitDevice)"""
        import torch
        F, Cn, S = residual.shape
        cap = int(capacity_bytes if capacity_bytes is not None else F * Cn * (S * 4 + 64))
        packed = torch.zeros(cap, dtype=torch.uint8, device=residual.device)
        offsets = torch.zeros(F * Cn + 1, dtype=torch.int32, device=residual.device)
        self._fence()
        self._check(lib.LINNEAmd_RiceEmitDevice(self.h, C.byref(shape), residual.data_ptr(), F, plan.data_ptr(), offsets.data_ptr(),
                                                packed.data_ptr(), cap), "RiceEmitDevice")
        return packed, offsets

    def decode_frames(self, shape, data, params, num_samples=None):
        """in place: data int32 cuda [F][C][S] residual -> PCM"""
        import torch
        F, Cn, S = data.shape
        assert data.dtype == torch.int32 and data.is_cuda and data.is_contiguous() and params.is_contiguous()
        ns = None
        if num_samples is not None:
            ns = np.ascontiguousarray(num_samples, dtype=np.uint32)
        self._fence()
        self._check(lib.LINNEAmd_DecodeFramesDevice(self.h, C.byref(shape), data.data_ptr(), ns.ctypes.data if ns is not None else None,
                                                    F, params.data_ptr()), "DecodeFramesDevice")
        return data

    def _stream_bytes(self, data):
        """a .lnn stream as a 1-D uint8 CUDA tensor on the context's device: tensors are taken as they are (any offset),
        bytes / numpy arrays are copied there"""
        import torch
        if isinstance(data, torch.Tensor):
            assert data.dtype == torch.uint8 and data.is_cuda and data.dim() == 1 and data.is_contiguous(), \
                "a stream tensor is a contiguous 1-D uint8 CUDA tensor"
            assert data.device.index == self.device, f"the stream is on {data.device}, the context on cuda:{self.device}"
            return data
        arr = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        return torch.from_numpy(arr.copy()).to(f"cuda:{self.device}")

    def index_stream(self, data):
        """block index of a whole .lnn stream (uint8 CUDA tensor, bytes or numpy) -> StreamIndex; raises LinneAmdError (.code =
        the LINNEApiResult, the header's errors are DecodeWhole's) when the header is unusable"""
        t = self._stream_bytes(data)
        self._fence()
        res = C.c_int(0)
        h = lib.LINNEAmd_StreamIndexCreate(self.h, C.c_void_p(t.data_ptr()), t.numel(), C.byref(res))
        if not h:
            raise LinneAmdError(f"StreamIndexCreate -> {res.value}: {lib.LINNEAmd_GetLastError(self.h).decode()}", res.value)
        return StreamIndex.of(h, t.numel())

    def index_streams(self, streams, return_codes=False):
        """the block indexes of many whole .lnn streams in one call (include/linne_amd.h LINNEAmd_StreamIndexesCreate).  streams: a
        sequence of uint8 CUDA tensors, bytes or numpy arrays (None: a NULL stream pointer) -> a list of StreamIndex, each what
        index_stream gives for its stream alone.  Raises LinneAmdError with .code = the call's result and .codes = the per-stream
        LINNEApiResults when a stream fails (the indexes that were built are closed); with return_codes -> (indexes, codes), a failed
        stream's index is None, and only a failure of the whole call raises"""
        T = len(streams)
        keep = [None if s is None else self._stream_bytes(s) for s in streams]
        ptrs, sizes = (C.c_void_p * max(T, 1))(), (C.c_uint64 * max(T, 1))()
        for i, t in enumerate(keep):
            ptrs[i], sizes[i] = (None, 0) if t is None else (t.data_ptr(), t.numel())
        handles, res = (C.c_void_p * max(T, 1))(), (C.c_int32 * max(T, 1))()
        self._fence()
        ret = lib.LINNEAmd_StreamIndexesCreate(self.h, ptrs, sizes, T, handles, res)
        codes = [int(res[i]) for i in range(T)]
        msg = lib.LINNEAmd_GetLastError(self.h).decode() if ret != 0 else ""
        out = [StreamIndex.of(handles[i], keep[i].numel()) if handles[i] else None for i in range(T)]
        whole_call = ret == 7 and all(x is None for x in out) and all(c == 7 for c in codes)      # LINNE_APIRESULT_NG everywhere, nothing built
        if ret != 0 and (not return_codes or whole_call):
            for x in out:
                if x is not None:
                    x.close()
            raise LinneAmdError(f"StreamIndexesCreate -> {ret}: {msg}", ret, codes)
        return (out, codes) if return_codes else out

    def last_index_batch_count(self, which):
        """the last index_streams call: 0 the streams given, 1 the indexes built, 2 the pointer-doubling depth K, 3 its host
        synchronisations, 4 its device allocations"""
        return int(lib.LINNEAmd_GetLastIndexBatchCount(self.h, int(which)))

    def decode_stream(self, data, first_sample=0, num_samples=None, index=None, dtype=None, channels_last=False, s24=False,
                      return_saturated=False):
        """samples [first_sample, first_sample + num_samples) of a .lnn stream in device memory -> int32 CUDA tensor (C, n), decoded
        on the device (include/linne_amd.h LINNEAmd_DecodeStreamDevice states the result contract).  Without an index a temporary
        one is built.  Raises LinneAmdError with .code = the LINNEApiResult.  dtype (torch.int32, int16 or float32), channels_last
        ((n, C)), s24 (packed 3-byte samples: uint8 (..., 3)) and return_saturated (-> (pcm, flag)) are decode_windows' for its one
        window"""
        import torch
        t = self._stream_bytes(data)
        own = index is None
        if own:
            index = self.index_stream(t)
        try:
            if dtype not in (None, torch.int32) or channels_last or s24 or return_saturated:
                assert index.nbytes == t.numel(), "the index was built for a stream of another length"
                r = self.decode_windows([(t, index, first_sample, num_samples)], dtype=dtype, channels_last=channels_last, s24=s24,
                                        return_saturated=return_saturated)
                return (r[0][0], r[1][0]) if return_saturated else r[0]
            assert index.nbytes == t.numel(), "the index was built for a stream of another length"
            total = index.header["num_samples"]
            n = total - int(first_sample) if num_samples is None else int(num_samples)
            nch = index.header["num_channels"]
            out = torch.empty((nch, max(n, 0)), dtype=torch.int32, device=t.device)
            self._fence()
            self._check(lib.LINNEAmd_DecodeStreamDevice(self.h, index.h, C.c_void_p(t.data_ptr()), int(first_sample), n if n >= 0 else (1 << 64) - 1,
                                                        C.c_void_p(out.data_ptr()), out.shape[1]), "DecodeStreamDevice")
            return out
        finally:
            if own:
                index.close()

    def _windows_array(self, windows, extra=0):
        """the Window array of a windows call.  windows: (stream, index, first_sample, num_samples) as decode_windows takes them,
        each followed by `extra` fields of the caller's own -> (the array, with no PCM named yet; the stream tensors, to be kept alive
        over the call; (index, first, n) per window, n the samples asked for, negative when the range is)"""
        arr = (Window * max(len(windows), 1))()
        keep, ranges = [], []
        for i, w in enumerate(windows):
            stream, index, first, n = w[:len(w) - extra]
            t = self._stream_bytes(stream)
            first, n, count = _sample_range(index, t.numel(), first, n, "window %d", i)
            keep.append(t)
            ranges.append((index, first, n))
            win = arr[i]
            win.index, win.d_stream, win.first_sample, win.num_samples, win.d_pcm, win.pcm_stride = index.h, t.data_ptr(), first, count, None, 0
        return arr, keep, ranges

    def _windows_codes(self, ret, arr, W, what, return_codes):
        """the per-window LINNEApiResults behind a windows call; raises LinneAmdError unless the call succeeded or, with return_codes,
        only windows failed"""
        codes = [int(arr[i].result) for i in range(W)]
        if ret != 0:
            msg = lib.LINNEAmd_GetLastError(self.h).decode()
            if not (return_codes and msg.startswith("window ")):       # (a failing window's text starts with its number)
                raise LinneAmdError(f"{what} -> {ret}: {msg}", ret, codes)
        return codes

    def _bucket_tables(self, buckets, ranges, words, rows):
        """the tables of a call that answers per bucket, from the windows' bucket lengths and 64-bit words per bucket -> (per window an
        int64 view rows(C) + (nb, words) of one allocation; the views' device addresses; the bucket counts nb)"""
        import torch
        counts = [0 if n <= 0 else (1 if b == 0 else -(-n // b)) for (_, _, n), b in zip(ranges, buckets)]
        shapes = [rows(x.header["num_channels"]) + (nb, wd) for (x, _, _), nb, wd in zip(ranges, counts, words)]
        sizes = [math.prod(shape) for shape in shapes]
        flat = torch.empty(max(sum(sizes), max(words, default=1)), dtype=torch.int64, device=f"cuda:{self.device}")
        views, addresses, at = [], [], 0
        for shape, size in zip(shapes, sizes):
            views.append(flat[at:at + size].view(*shape))
            addresses.append(flat.data_ptr() + 8 * at)                 # (an empty view has no address of its own)
            at += size
        return views, addresses, counts

    def _bucket_windows(self, name, windows, bucket_samples, group_frames, return_codes, words=None, **fields):
        """measure_, digest_, histogram_ and relate_windows: row `name` of _BUCKET_CONSUMERS over the windows.  words: the 64-bit words
        of a bucket per window, where the row names none; fields: the spec's further fields, each a list with a value per window"""
        spec, entry, row_words, rows, stride, answer = _BUCKET_CONSUMERS[name]
        W = len(windows)
        arr, keep, ranges = self._windows_array(windows)
        buckets = _per_window(bucket_samples, W, "bucket_samples")
        tables, addresses, counts = self._bucket_tables(buckets, ranges, [row_words] * W if words is None else words, rows)
        specs = (spec * max(W, 1))()
        for i in range(W):
            sp = specs[i]
            sp.bucket_samples, sp.d_out = buckets[i], addresses[i]
            if stride:
                setattr(sp, stride, counts[i])
            for field, values in fields.items():
                setattr(sp, field, values[i])
        self._fence()
        ret = getattr(lib, entry)(self.h, arr, specs, W, int(group_frames))
        codes = self._windows_codes(ret, arr, W, entry[len("LINNEAmd_"):], return_codes)
        own = list(zip(*fields.values())) if fields else [()] * W
        out = [answer(tables[i], buckets[i], ranges[i][0], *own[i]) if codes[i] == 0 else None for i in range(W)]
        return (out, codes) if return_codes else out

    @contextlib.contextmanager
    def _whole_streams(self, streams, return_codes=False):
        """one index_streams call over whole streams -> (the streams' tensors, their indexes, with return_codes the streams' codes --
        a failed stream's index is None -- otherwise None); the indexes are closed behind the block"""
        ts = [self._stream_bytes(s) for s in streams]
        indexes, codes = self.index_streams(ts, return_codes=True) if return_codes else (self.index_streams(ts), None)
        try:
            yield ts, indexes, codes
        finally:
            for x in indexes:
                if x is not None:
                    x.close()

    def _over_whole_streams(self, streams, call, **kw):
        """one index_streams call and one `call` over the whole streams"""
        if len(streams) == 0:
            return []
        with self._whole_streams(streams) as (ts, indexes, _):
            return call([(t, x, 0, None) for t, x in zip(ts, indexes)], **kw)

    def decode_windows(self, windows, out=None, group_frames=0, return_codes=False, dtype=None, channels_last=False, s24=False,
                       return_saturated=False):
        """many sample windows of resident .lnn streams in one call (include/linne_amd.h LINNEAmd_DecodeWindowsDevice).  windows: a
        sequence of (stream, index, first_sample, num_samples): a 1-D uint8 CUDA tensor, its StreamIndex, and the range (num_samples
        None: to the stream's end).  Without `out` -> a list of int32 CUDA tensors (C_w, n_w), views of one allocation; with `out`, an
        int32 CUDA tensor (W, C, n) whose last dimension is contiguous, every window must have that C and n, and `out` is returned
        (the form of a training batch).  Every window's PCM is what decode_stream gives for it alone; a failing window's is not
        written.  Raises LinneAmdError with .code = the call's result and .codes = the per-window LINNEApiResults when a window
        fails; with return_codes -> (pcm, codes), and only a failure of the whole call raises.  group_frames bounds the COMPRESS
        blocks decoded per pass (0: one pass per stream shape) and never changes the result.
        Other sample formats (LINNEAmd_DecodeWindowsDeviceLayout): dtype torch.int16 (saturating), torch.float32 (v * 2^-(bits - 1))
        or torch.int32 (the default); s24=True gives packed 3-byte little-endian samples (saturating) as uint8 tensors with a trailing
        dimension of 3; channels_last=True gives (n_w, C_w) windows, and says that `out` is (W, n, C).  `out` then has that dtype and
        any strides.  return_saturated appends the list of the windows' flags "a sample was clipped" to the result"""
        return self._place_windows(windows, None, out, group_frames, return_codes, dtype, channels_last, s24, return_saturated)

    def _place_windows(self, windows, specs, out, group_frames, return_codes, dtype, channels_last, s24, return_saturated):
        """decode_windows (specs None) and mix_windows (specs: the windows' MixSpec array, whose out_channels are the windows' channel
        counts): the outputs, the layouts, the call and what it returns"""
        import torch
        W = len(windows)
        arr, keep, ranges = self._windows_array(windows)
        mixes = specs is not None and specs._type_ is MixSpec      # (otherwise the specs are ResampleSpec: the stream's channels, ranges of output samples)
        shapes = [(int(specs[i].out_channels) if mixes else x.header["num_channels"], max(n, 0)) for i, (x, _, n) in enumerate(ranges)]
        pcm, lays, plain = self._pcm_targets(arr, shapes, specs is None, out, dtype, channels_last, s24, return_saturated)
        self._fence()
        if plain:
            ret = lib.LINNEAmd_DecodeWindowsDevice(self.h, arr, W, int(group_frames))
        elif specs is None:
            ret = lib.LINNEAmd_DecodeWindowsDeviceLayout(self.h, arr, lays, W, int(group_frames))
        elif mixes:
            ret = lib.LINNEAmd_MixWindowsDevice(self.h, arr, specs, lays, W, int(group_frames))
        else:
            ret = lib.LINNEAmd_ResampleWindowsDevice(self.h, arr, specs, lays, W, int(group_frames))
        codes = self._windows_codes(ret, arr, W, "DecodeWindowsDevice" if specs is None else "MixWindowsDevice" if mixes else "ResampleWindowsDevice", return_codes)
        res = (pcm,) + ((codes,) if return_codes else ()) + (([bool(lays[i].saturated) for i in range(W)],) if return_saturated else ())
        return res[0] if len(res) == 1 else res

    def _pcm_targets(self, arr, shapes, bare, out, dtype, channels_last, s24, return_saturated, noun="window"):
        """where a batch writer's PCM goes: arr's elements (Window, or Overlay) get their d_pcm and pcm_stride for the (C, n) of
        `shapes`, in `out` or in one new allocation -> (the PCM as the call returns it, the PcmLayout array, whether the call may be
        the one without layouts: `bare`, int32 planar, and nobody asks for `saturated`)"""
        import torch
        W = len(shapes)
        dev = f"cuda:{self.device}"
        if s24:
            assert dtype in (None, torch.uint8), "s24 samples are uint8 triples"
            fmt, tdtype, esize = PCM_S24, torch.uint8, 3
        else:
            tdtype = torch.int32 if dtype is None else dtype
            assert tdtype in (torch.int32, torch.int16, torch.float32), "dtype is torch.int32, torch.int16 or torch.float32"
            fmt, esize = {torch.int32: (PCM_S32, 4), torch.int16: (PCM_S16, 2), torch.float32: (PCM_F32, 4)}[tdtype]
        plain = bare and fmt == PCM_S32 and not channels_last and not return_saturated and (out is None or out.dim() != 3 or out.stride(2) == 1 or out.shape[2] <= 1)
        lays = (PcmLayout * max(W, 1))()
        cdim, sdim = (2, 1) if channels_last else (1, 2)
        if out is not None:
            if plain:
                assert out.dtype == torch.int32 and out.is_cuda and out.dim() == 3 and out.shape[0] == W and (out.stride(2) == 1 or out.shape[2] <= 1), \
                    "out is an int32 CUDA tensor (W, C, n), contiguous in its last dimension"
            else:
                assert out.dtype == tdtype and out.is_cuda and out.dim() == (4 if s24 else 3) and out.shape[0] == W, \
                    f"out is a {tdtype} CUDA tensor (W, C, n) or, channels_last, (W, n, C)" + (" with a trailing dimension of 3" if s24 else "")
                assert not s24 or (out.shape[3] == 3 and out.stride(3) == 1 and all(out.stride(d) % 3 == 0 for d in range(3))), \
                    "the three bytes of an s24 sample are contiguous, and samples lie whole samples apart"
            assert out.device.index == self.device, f"out is on {out.device}, the context on cuda:{self.device}"
            unit = 3 if s24 else 1
            for i, (c, n) in enumerate(shapes):
                assert (c, n) == (out.shape[cdim], out.shape[sdim]), f"{noun} {i} is {(c, n)}, out holds {tuple(out.shape[1:])} per {noun}"
                arr[i].d_pcm, arr[i].pcm_stride = out.data_ptr() + out.element_size() * i * out.stride(0), out.stride(1) if c > 1 else n
                lays[i].format, lays[i].channel_stride = fmt, out.stride(cdim) // unit if c > 1 else 0
                lays[i].sample_stride = out.stride(sdim) // unit if n > 1 else 1
            pcm = out
        else:
            flat = torch.empty(sum(c * n for c, n in shapes) * (3 if s24 else 1), dtype=tdtype, device=dev)
            pcm, at = [], 0
            for i, (c, n) in enumerate(shapes):
                v = flat[at:at + c * n * (3 if s24 else 1)].view(*((n, c) if channels_last else (c, n)), *((3,) if s24 else ()))
                at += c * n * (3 if s24 else 1)
                pcm.append(v)
                arr[i].d_pcm, arr[i].pcm_stride = v.data_ptr(), n
                lays[i].format = fmt
                lays[i].channel_stride, lays[i].sample_stride = (1, c) if channels_last else (n, 1)
        return pcm, lays, plain

    @staticmethod
    def _mix_specs(indexes, matrix, shift, clip_bits):
        """the MixSpec array of a mix call: matrix one (Co, C) integer array for all windows or a sequence of them, one per window;
        shift and clip_bits one value or one per window.  Values outside int16 raise ValueError"""
        W = len(indexes)
        one = isinstance(matrix, np.ndarray) and matrix.ndim == 2 or (not isinstance(matrix, np.ndarray) and len(matrix) > 0 and np.ndim(matrix[0]) == 1)
        mats = [matrix] * W if one else list(matrix)
        assert len(mats) == W, "matrix is one (Co, C) array, or one per window"
        shifts, clips = _per_window(shift, W, "shift", lo=None), _per_window(clip_bits, W, "clip_bits", lo=None)      # (their ranges: ValueError, below)
        specs = (MixSpec * max(W, 1))()
        for i, (x, m) in enumerate(zip(indexes, mats)):
            m = np.asarray(m)
            if m.ndim != 2 or m.dtype.kind not in "iu" or not 1 <= m.shape[0] <= 8 or m.shape[1] != x.header["num_channels"]:
                raise ValueError(f"window {i}: the matrix is an integer array (Co, {x.header['num_channels']}), Co 1 .. 8; got {m.dtype} {m.shape}")
            if m.size and (int(m.min()) < -32768 or int(m.max()) > 32767):
                raise ValueError(f"window {i}: a coefficient outside int16")
            if shifts[i] < 0 or clips[i] < 0 or shifts[i] >= 1 << 32 or clips[i] >= 1 << 32:
                raise ValueError(f"window {i}: shift and clip_bits are unsigned")
            specs[i].out_channels, specs[i].shift, specs[i].clip_bits, specs[i].reserved = m.shape[0], shifts[i], clips[i], 0
            for o in range(m.shape[0]):
                for c in range(m.shape[1]):
                    specs[i].coef[o][c] = int(m[o, c])
        return specs

    def mix_windows(self, windows, matrix, shift=0, clip_bits=0, out=None, group_frames=0, return_codes=False, dtype=None, channels_last=False,
                    s24=False, return_saturated=False):
        """decode_windows with an exact integer channel matrix between the samples and the PCM (include/linne_amd.h
        LINNEAmd_MixWindowsDevice states the arithmetic): output channel o of a frame is sum_c matrix[o][c] * v[c] in 64 bits, shifted
        right by `shift` with halves rounded up, clipped to clip_bits bits (0: 32), then converted as decode_windows converts (float32:
        times 2^-(clip_bits - 1), or 2^-(bits - 1) of the stream where clip_bits is 0).  matrix: one (Co, C) integer array for all
        windows, or a sequence of them, one per window; shift and clip_bits likewise one value or one per window; values outside int16
        raise ValueError before any call.  Everything else -- windows, out, dtype, channels_last, s24, return_codes, return_saturated,
        group_frames, errors -- is decode_windows', with Co channels where that has the stream's"""
        specs = self._mix_specs([w[1] for w in windows], matrix, shift, clip_bits)
        return self._place_windows(windows, specs, out, group_frames, return_codes, dtype, channels_last, s24, return_saturated)

    def remix_streams(self, streams, matrix, shift=0, bits=None, preset=None, block=None, ms=None, group_frames=0):
        """new .lnn streams whose channels are a matrix of the given streams' channels, without the PCM leaving the device: one
        index_streams call, one mix_windows call over the whole streams into one int32 allocation (clip_bits = the output's bits) and
        one encode_streams call.  matrix and shift as mix_windows takes them (one for all streams, or one per stream).  Every header
        field not given (bits, preset, block, ms) is the source stream's; num_channels is the matrix' row count, and an output of one
        channel does not inherit MS, which a mono header cannot carry.  -> a list of uint8 CUDA tensors"""
        if len(streams) == 0:
            return []
        with self._whole_streams(streams) as (ts, indexes, _):
            heads = [x.header for x in indexes]
            obits = [int(bits) if bits is not None else h["bits_per_sample"] for h in heads]
            pcms = self.mix_windows([(t, x, 0, None) for t, x in zip(ts, indexes)], matrix, shift=shift, clip_bits=obits, group_frames=group_frames)
            tracks = [(pcm, b, h["sampling_rate"], int(block) if block is not None else h["num_samples_per_block"],
                       int(preset) if preset is not None else h["preset"], int(ms) if ms is not None else (h["ch_process_method"] if pcm.shape[0] > 1 else 0))
                      for pcm, b, h in zip(pcms, obits, heads)]
            return self.encode_streams(tracks, group_frames=group_frames)

    def resample_windows(self, windows, up, down, coef=None, taps=32, before=None, shift=None, clip_bits=0, out=None, group_frames=0,
                         return_codes=False, dtype=None, channels_last=False, s24=False, return_saturated=False):
        """decode_windows at another sampling rate: a rational rate change up/down through an exact int16 polyphase FIR between the
        samples and the PCM (include/linne_amd.h LINNEAmd_ResampleWindowsDevice states the arithmetic).  A window's first_sample and
        num_samples count OUTPUT samples of the resampled stream, which has resample_length(N, up, down) of them; num_samples None: to
        its end.  up, down: one value for all windows or one per window.  coef: an int16 array (up, taps) for all windows, or a
        sequence of them, one per window, with `before` (default (taps - 1) // 2 of the array) and `shift` (default 0) one value or one
        per window; coef None designs the filter of `taps` coefficients per phase (resample_design) and takes its shift and before.
        clip_bits as mix_windows has it.  Values outside the call's bounds raise ValueError before any call.  Everything else --
        out, dtype, channels_last, s24, return_codes, return_saturated, group_frames, errors -- is decode_windows'"""
        W = len(windows)
        ups, downs = _per_window(up, W, "up", lo=None), _per_window(down, W, "down", lo=None)
        clips = _per_window(clip_bits, W, "clip_bits", lo=None)
        if coef is None:
            made = {}
            for u, d in zip(ups, downs):
                if (u, d) not in made:
                    made[(u, d)] = resample_design(u, d, taps)
            tables = [made[(u, d)][0] for u, d in zip(ups, downs)]
            shifts = [made[(u, d)][1] for u, d in zip(ups, downs)] if shift is None else _per_window(shift, W, "shift", lo=None)
            befores = [made[(u, d)][2] for u, d in zip(ups, downs)] if before is None else _per_window(before, W, "before", lo=None)
        else:
            one = isinstance(coef, np.ndarray) and coef.ndim == 2
            given = [coef] * W if one else list(coef)
            assert len(given) == W, "coef is one (up, taps) array, or one per window"
            tables, same = [], {}
            for i, m in enumerate(given):
                if id(m) not in same:                                # (windows that share an array share its device copy)
                    a = np.asarray(m)
                    if a.ndim != 2 or a.dtype.kind not in "iu" or a.size == 0:
                        raise ValueError(f"window {i}: coef is an integer array (up, taps); got {a.dtype} {a.shape}")
                    if int(a.min()) < -32768 or int(a.max()) > 32767:
                        raise ValueError(f"window {i}: a coefficient outside int16")
                    same[id(m)] = np.ascontiguousarray(a, dtype=np.int16)
                tables.append(same[id(m)])
            shifts = _per_window(0 if shift is None else shift, W, "shift", lo=None)
            befores = [(t.shape[1] - 1) // 2 for t in tables] if before is None else _per_window(before, W, "before", lo=None)
        specs = (ResampleSpec * max(W, 1))()
        ranged = []
        for i, w in enumerate(windows):
            t = tables[i]
            if t.shape[0] != ups[i]:
                raise ValueError(f"window {i}: coef has {t.shape[0]} phases, up is {ups[i]}")
            if not (1 <= ups[i] <= RESAMPLE_MAX_RATIO and 1 <= downs[i] <= RESAMPLE_MAX_RATIO and 1 <= t.shape[1] <= RESAMPLE_MAX_TAPS and t.size <= RESAMPLE_MAX_COEFS):
                raise ValueError(f"window {i}: up and down are 1 .. {RESAMPLE_MAX_RATIO}, taps 1 .. {RESAMPLE_MAX_TAPS}, up * taps <= {RESAMPLE_MAX_COEFS}")
            if not (0 <= befores[i] < t.shape[1] and 0 <= shifts[i] <= 31 and (clips[i] == 0 or 2 <= clips[i] <= 32)):
                raise ValueError(f"window {i}: before is 0 .. taps - 1, shift 0 .. 31, clip_bits 0 or 2 .. 32")
            sp = specs[i]
            sp.up, sp.down, sp.taps, sp.before, sp.shift, sp.clip_bits, sp.reserved = ups[i], downs[i], t.shape[1], befores[i], shifts[i], clips[i], 0
            sp.coef = t.ctypes.data_as(C.POINTER(C.c_int16))
            stream, index, first, n = w
            if n is None:
                n = resample_length(index.header["num_samples"], ups[i], downs[i]) - int(first)
            ranged.append((stream, index, first, n))
        return self._place_windows(ranged, specs, out, group_frames, return_codes, dtype, channels_last, s24, return_saturated)

    def resample_streams(self, streams, rate, taps=32, bits=None, preset=None, block=None, ms=None, group_frames=0):
        """new .lnn streams at the sampling rate `rate`, without the PCM leaving the device: one index_streams call, one
        resample_windows call over the whole streams into one int32 allocation (the designed filter of `taps` coefficients per phase,
        clip_bits = the output's bits) and one encode_streams call.  A stream already at `rate` goes the same way, with 1/1.  Every
        header field not given (bits, preset, block, ms) is the source stream's; sampling_rate is `rate`.  -> a list of uint8 CUDA
        tensors"""
        if len(streams) == 0:
            return []
        with self._whole_streams(streams) as (ts, indexes, _):
            heads = [x.header for x in indexes]
            obits = [int(bits) if bits is not None else h["bits_per_sample"] for h in heads]
            ratios = [resample_ratio(h["sampling_rate"], rate) for h in heads]
            pcms = self.resample_windows([(t, x, 0, None) for t, x in zip(ts, indexes)], [r[0] for r in ratios], [r[1] for r in ratios], taps=taps,
                                         clip_bits=obits, group_frames=group_frames)
            tracks = [(pcm, b, int(rate), int(block) if block is not None else h["num_samples_per_block"],
                       int(preset) if preset is not None else h["preset"], int(ms) if ms is not None else h["ch_process_method"])
                      for pcm, b, h in zip(pcms, obits, heads)]
            return self.encode_streams(tracks, group_frames=group_frames)

    def project_windows(self, windows, basis, hop, before=0, shift=0, clip_bits=0, dtype=None, float_exp=0, rows_first=False, out=None,
                        group_frames=0, return_codes=False, return_saturated=False):
        """the frames of windows of resident streams projected on the rows of an int16 basis: an exact STFT, a filter bank (include/linne_amd.h
        LINNEAmd_ProjectWindowsDevice states the arithmetic).  windows: (stream, index, first_frame, num_frames) -- a window counts
        FRAMES of its stream, which has project_length(N, hop) of them; num_frames None: to the last.  Frame f holds the n_fft =
        basis.shape[1] samples from f * hop - before on, zeros off either end of the stream; element (c, f, k) is the 64-bit sum of
        basis[k][n] * x[c][f * hop - before + n], shifted right by `shift` with halves rounded up and clipped to clip_bits bits (0: 32)
        as mix_windows has it.  basis: an integer array (K, n_fft) with values in int16.  dtype torch.int32 (the default) or torch.float32,
        which stores (float)y * 2^-float_exp.  -> one tensor (W, C, frames, K), or (W, C, K, frames) with rows_first: all windows then
        have one channel count and one frame count; `out` is such a tensor of any strides that keep its elements apart.  Values
        outside the call's bounds raise ValueError before any call.  return_codes, return_saturated, group_frames and errors are
        decode_windows'"""
        import torch
        W = len(windows)
        b = np.asarray(basis)
        if b.ndim != 2 or b.dtype.kind not in "iu" or b.size == 0:
            raise ValueError(f"basis is an integer array (K, n_fft); got {b.dtype} {b.shape}")
        if int(b.min()) < -32768 or int(b.max()) > 32767:
            raise ValueError("a basis value outside int16")
        b = np.ascontiguousarray(b, dtype=np.int16)
        K, N = b.shape
        hop, before, shift, clip_bits, float_exp = int(hop), int(before), int(shift), int(clip_bits), int(float_exp)
        tdtype = torch.int32 if dtype is None else dtype
        if tdtype not in (torch.int32, torch.float32):
            raise ValueError("dtype is torch.int32 or torch.float32")
        if not (1 <= N <= PROJECT_MAX_FRAME and 1 <= K <= PROJECT_MAX_ROWS and 1 <= hop <= PROJECT_MAX_HOP):
            raise ValueError(f"n_fft is 1 .. {PROJECT_MAX_FRAME}, the rows 1 .. {PROJECT_MAX_ROWS}, hop 1 .. {PROJECT_MAX_HOP}")
        if not (0 <= before < N and 0 <= shift <= 31 and (clip_bits == 0 or 2 <= clip_bits <= 32) and 0 <= float_exp <= 63 and (float_exp == 0 or tdtype is torch.float32)):
            raise ValueError("before is 0 .. n_fft - 1, shift 0 .. 31, clip_bits 0 or 2 .. 32, float_exp 0 .. 63 and 0 with torch.int32")
        ranged = []
        for stream, index, first, n in windows:
            if n is None:
                n = project_length(index.header["num_samples"], hop) - int(first)
            ranged.append((stream, index, first, n))
        arr, keep, ranges = self._windows_array(ranged)
        shapes = [(x.header["num_channels"], max(n, 0)) for x, _, n in ranges]
        assert len(set(shapes)) <= 1, f"the windows of one call have one channel count and one frame count; got {sorted(set(shapes))}"
        Cn, F = shapes[0] if shapes else (0, 0)
        fdim, kdim = (3, 2) if rows_first else (2, 3)
        if out is None:
            out = torch.empty((W, Cn, K, F) if rows_first else (W, Cn, F, K), dtype=tdtype, device=f"cuda:{self.device}")
        else:
            assert out.dtype == tdtype and out.is_cuda and out.dim() == 4 and out.device.index == self.device, f"out is a {tdtype} CUDA tensor of the context's device"
            assert tuple(out.shape) == ((W, Cn, K, F) if rows_first else (W, Cn, F, K)), f"out is {tuple(out.shape)}, the call gives {(W, Cn, K, F) if rows_first else (W, Cn, F, K)}"
        specs = (ProjectSpec * max(W, 1))()
        for i in range(W):
            sp = specs[i]
            sp.frame_len, sp.hop, sp.num_rows, sp.before, sp.shift, sp.clip_bits = N, hop, K, before, shift, clip_bits
            sp.format, sp.float_exp, sp.reserved = (PCM_F32 if tdtype is torch.float32 else PCM_S32), float_exp, 0
            sp.channel_stride, sp.frame_stride, sp.row_stride = out.stride(1), out.stride(fdim), out.stride(kdim)
            sp.basis = b.ctypes.data_as(C.POINTER(C.c_int16))
            arr[i].d_pcm, arr[i].pcm_stride = out.data_ptr() + out.element_size() * i * out.stride(0), 0
        self._fence()
        ret = lib.LINNEAmd_ProjectWindowsDevice(self.h, arr, specs, W, int(group_frames))
        codes = self._windows_codes(ret, arr, W, "ProjectWindowsDevice", return_codes)
        res = (out,) + ((codes,) if return_codes else ()) + (([bool(specs[i].saturated) for i in range(W)],) if return_saturated else ())
        return res[0] if len(res) == 1 else res

    def stft_windows(self, windows, n_fft, hop, window="hann", center=True, shift=15, dtype=None, float_exp=0, bins=None, clip_bits=0,
                     rows_first=False, group_frames=0, return_codes=False, return_saturated=False):
        """the exact integer short-time Fourier transform of windows of resident streams: project_windows on project_design(n_fft, bins,
        window).  windows: (stream, index, first_sample, num_samples) in SAMPLES (num_samples None: to the stream's end); they map to
        the frames f with first_sample <= f * hop < first_sample + num_samples.  center: frame f is centred on sample f * hop (before =
        n_fft // 2), otherwise it starts there.  The basis is scaled by 32767: shift 15 (the default) gives the transform in the
        samples' own units.  -> (W, C, frames, bins, 2), real and imaginary part last, or (W, C, bins, 2, frames) with rows_first"""
        basis = project_design(n_fft, bins, window)
        hop = int(hop)
        if not 1 <= hop <= PROJECT_MAX_HOP:
            raise ValueError(f"hop is 1 .. {PROJECT_MAX_HOP}")
        framed = []
        for stream, index, first, n in windows:
            first = int(first)
            n = index.header["num_samples"] - first if n is None else int(n)
            f0 = -(-first // hop)
            framed.append((stream, index, f0, -(-(first + n) // hop) - f0 if n >= 0 else n))
        res = self.project_windows(framed, basis, hop, before=n_fft // 2 if center else 0, shift=shift, clip_bits=clip_bits, dtype=dtype,
                                   float_exp=float_exp, rows_first=rows_first, group_frames=group_frames, return_codes=return_codes,
                                   return_saturated=return_saturated)
        many = isinstance(res, tuple)
        t = res[0] if many else res
        t = t.view(t.shape[0], t.shape[1], t.shape[2] // 2, 2, t.shape[3]) if rows_first else t.view(t.shape[0], t.shape[1], t.shape[2], t.shape[3] // 2, 2)
        return (t,) + tuple(res[1:]) if many else t

    def spectrum_streams(self, streams, n_fft, hop):
        """the exact power spectrum of whole resident streams: one index_streams call, one stft_windows call (its defaults: Hann, centred,
        shift 15, int32) per group of streams of one shape, and per stream, channel and bin the sum over all frames of re^2 + im^2 as
        a Python integer -> a list per stream of [channel][bin] integers.  A bin that does not fit int32 at shift 15 (a 24-bit stream
        under a long frame) would make the sums those of clipped values: OverflowError, naming the streams"""
        import torch
        if len(streams) == 0:
            return []
        with self._whole_streams(streams) as (ts, indexes, _):
            groups = {}
            for i, x in enumerate(indexes):
                groups.setdefault((x.header["num_channels"], project_length(x.header["num_samples"], hop)), []).append(i)
            out = [None] * len(streams)
            for members in groups.values():
                z, clipped = self.stft_windows([(ts[i], indexes[i], 0, None) for i in members], n_fft, hop, return_saturated=True)    # (W, C, frames, bins, 2)
                if any(clipped):
                    raise OverflowError(f"spectrum_streams: a bin of stream(s) {[i for i, c in zip(members, clipped) if c]} does not fit 32 bits at shift 15")
                z = z.to(torch.int64)
                # v = a * 2^16 + b, 0 <= b < 2^16: the three sums stay inside int64 and recombine exactly
                a, b = z >> 16, z & 0xFFFF
                saa, sab, sbb = ((u * v).sum(dim=(2, 4)).cpu().tolist() for u, v in ((a, a), (a, b), (b, b)))
                for w, i in enumerate(members):
                    out[i] = [[(int(p) << 32) + (int(q) << 17) + int(r) for p, q, r in zip(*rows)] for rows in zip(saa[w], sab[w], sbb[w])]
            return out

    def overlay_windows(self, outputs, shift=0, clip_bits=0, out=None, group_frames=0, return_codes=False, dtype=None, channels_last=False,
                        s24=False, return_saturated=False):
        """windows of several resident streams summed into each output under gains that move linearly over a source: a mix-down, a
        fade, a crossfade (include/linne_amd.h LINNEAmd_OverlayWindowsDevice states the arithmetic).  outputs: a sequence of
        (num_samples, sources), sources a sequence of (stream, index, first_sample, num_samples, at, gain): the range of the source in
        its stream (num_samples None: to the stream's end), the output sample its first sample lands on, and its gain -- an int, a
        constant gain, or a (gain_q32, step_q32) pair as fade and crossfade make them.  The sum is shifted right by `shift` with
        halves rounded up and clipped to clip_bits bits (0: 32), as mix_windows has it; shift and clip_bits are one value or one per
        output.  An output has the channel count its sources share.  Values outside the call's bounds raise ValueError before any
        call.  Everything else -- out, dtype, channels_last, s24, return_codes, return_saturated, group_frames, errors -- is
        decode_windows', with an output where that has a window"""
        O = len(outputs)
        shifts, clips = _per_window(shift, O, "shift", lo=None), _per_window(clip_bits, O, "clip_bits", lo=None)
        arr = (Overlay * max(O, 1))()
        keep, shapes = [], []
        for k, (n_out, sources) in enumerate(outputs):
            n_out, K = int(n_out), len(sources)
            if not 1 <= K <= OVERLAY_MAX_SOURCES:
                raise ValueError(f"output {k}: {K} sources: 1 .. {OVERLAY_MAX_SOURCES}")
            if not (0 <= shifts[k] <= 31 and (clips[k] == 0 or 2 <= clips[k] <= 32) and 0 <= n_out < 1 << 64):
                raise ValueError(f"output {k}: shift is 0 .. 31, clip_bits 0 or 2 .. 32, num_samples unsigned")
            srcs = (OverlaySource * K)()
            keep.append(srcs)
            for j, (stream, index, first, n, at, gain) in enumerate(sources):
                t = self._stream_bytes(stream)
                first, n, count = _sample_range(index, t.numel(), first, n, "output %d: source %d", k, j)
                q, step = (int(gain) << 32, 0) if isinstance(gain, (int, np.integer)) else (int(gain[0]), int(gain[1]))
                at = int(at)
                if n < 1 or at < 0 or at + n > n_out:
                    raise ValueError(f"output {k}: source {j}: {n} samples at {at} of an output of {n_out}")
                if not (-32768 <= overlay_gain(q, step, 0) <= 32767 and -32768 <= overlay_gain(q, step, n - 1) <= 32767):
                    raise ValueError(f"output {k}: source {j}: a gain outside int16")
                if index.header["num_channels"] != sources[0][1].header["num_channels"]:
                    raise ValueError(f"output {k}: source {j} has {index.header['num_channels']} channels, source 0 {sources[0][1].header['num_channels']}")
                keep.append(t)
                sc = srcs[j]
                sc.index, sc.d_stream, sc.first_sample, sc.num_samples, sc.at, sc.gain_q32, sc.step_q32, sc.reserved = index.h, t.data_ptr(), first, count, at, q, step, 0
            o = arr[k]
            o.sources, o.num_sources, o.shift, o.clip_bits, o.reserved, o.num_samples = srcs, K, shifts[k], clips[k], 0, n_out
            shapes.append((sources[0][1].header["num_channels"], n_out))
        pcm, lays, _ = self._pcm_targets(arr, shapes, False, out, dtype, channels_last, s24, return_saturated, noun="output")
        self._fence()
        ret = lib.LINNEAmd_OverlayWindowsDevice(self.h, arr, lays, O, int(group_frames))
        codes = [int(arr[k].result) for k in range(O)]
        if ret != 0:
            msg = lib.LINNEAmd_GetLastError(self.h).decode()
            if not (return_codes and msg.startswith("output ")):       # (a failing output's text starts with its number)
                raise LinneAmdError(f"OverlayWindowsDevice -> {ret}: {msg}", ret, codes)
        res = (pcm,) + ((codes,) if return_codes else ()) + (([bool(lays[k].saturated) for k in range(O)],) if return_saturated else ())
        return res[0] if len(res) == 1 else res

    def overlay_streams(self, jobs, shift, bits=None, preset=None, block=None, ms=None, group_frames=0):
        """new .lnn streams that are overlays of resident streams, without the PCM leaving the device: one index_streams call over the
        distinct streams named, one overlay_windows call into one int32 allocation (clip_bits = the output's bits) and one
        encode_streams call.  jobs: a sequence of (num_samples, sources), sources a sequence of (stream, first_sample, num_samples, at,
        gain) as overlay_windows takes them without the index; shift one value or one per job.  Every header field not given (bits,
        preset, block, ms) is the job's first source's, the sampling rate too: sources of one job with different rates raise
        ValueError.  -> a list of uint8 CUDA tensors"""
        if len(jobs) == 0:
            return []
        order, ts = {}, []
        for _, sources in jobs:
            for src in sources:
                if id(src[0]) not in order:                      # (a stream named twice is indexed once)
                    order[id(src[0])] = len(ts)
                    ts.append(self._stream_bytes(src[0]))
        with self._whole_streams(ts) as (ts, xs, _):
            paired = [(n_out, [(ts[order[id(src[0])]], xs[order[id(src[0])]]) + tuple(src[1:]) for src in sources]) for n_out, sources in jobs]
            return self._overlay_indexed(paired, shift, bits, preset, block, ms, group_frames)

    def _overlay_indexed(self, jobs, shift, bits, preset, block, ms, group_frames):
        """overlay_streams and crossfade_streams behind their index_streams call: jobs of (num_samples, sources), a source (stream, its
        index, first_sample, num_samples, at, gain) as overlay_windows takes it -- every source carries its own index, so nothing
        depends on the order in which streams were named -> the encoded streams"""
        heads = []
        for k, (_, sources) in enumerate(jobs):
            if len(sources) == 0:
                raise ValueError(f"job {k}: no sources")
            rates = sorted({src[1].header["sampling_rate"] for src in sources})
            if len(rates) > 1:
                raise ValueError(f"job {k}: its sources have the sampling rates {rates}")
            heads.append(sources[0][1].header)
        obits = [int(bits) if bits is not None else h["bits_per_sample"] for h in heads]
        pcms = self.overlay_windows(jobs, shift=shift, clip_bits=obits, group_frames=group_frames)
        tracks = [(pcm, b, h["sampling_rate"], int(block) if block is not None else h["num_samples_per_block"],
                   int(preset) if preset is not None else h["preset"], int(ms) if ms is not None else h["ch_process_method"])
                  for pcm, b, h in zip(pcms, obits, heads)]
        return self.encode_streams(tracks, group_frames=group_frames)

    def crossfade_streams(self, streams, overlap, bits=None, preset=None, block=None, ms=None, group_frames=0):
        """one new .lnn stream: the given streams in order, each join a linear crossfade over `overlap` samples -- the last `overlap`
        samples of a stream under the falling ramp of crossfade(overlap, 16384), the first `overlap` of the next under the rising one,
        everything else at 16384, shift 14.  overlap 0 is a hard cut: the PCM of a splice_streams join.  One index_streams call (a
        stream given twice is indexed twice: an index per position), then what overlay_streams does behind its own: one
        overlay_windows call of one output and one encode_streams call.  A stream is a source at overlap 0 and otherwise up to three,
        two at the ends (one where it lies wholly under a ramp), and an output takes OVERLAY_MAX_SOURCES = 64: 64 streams at overlap 0,
        22 with crossfades, or ValueError.  A stream shorter than the overlaps it takes part in raises ValueError too.  -> a uint8
        CUDA tensor"""
        overlap = int(overlap)
        if len(streams) == 0 or overlap < 0:
            raise ValueError("crossfade_streams: at least one stream, overlap >= 0")
        unity = 16384
        down, up = crossfade(overlap, unity) if overlap else (None, None)
        ts = [self._stream_bytes(s) for s in streams]
        with self._whole_streams(ts) as (ts, indexes, _):
            sources, at = [], 0
            for i, (t, x) in enumerate(zip(ts, indexes)):
                n = x.header["num_samples"]
                head, tail = overlap if i > 0 else 0, overlap if i + 1 < len(ts) else 0
                if n < head + tail or n < 1:
                    raise ValueError(f"stream {i}: {n} samples under crossfades of {overlap}")
                if head:
                    sources.append((t, x, 0, head, at, up))
                if n - head - tail:
                    sources.append((t, x, head, n - head - tail, at + head, unity))
                if tail:
                    sources.append((t, x, n - tail, tail, at + n - tail, down))
                at += n - tail
            if len(sources) > OVERLAY_MAX_SOURCES:
                raise ValueError(f"crossfade_streams: {len(sources)} sources in one output: at most {OVERLAY_MAX_SOURCES}")
            return self._overlay_indexed([(at, sources)], 14, bits, preset, block, ms, group_frames)[0]

    def lag_windows(self, probes, group_frames=0, return_codes=False):
        """slide ranges of resident .lnn streams over each other: per probe, channel pair and lag the exact sums of a * b and of b^2
        under the needle, and the needle's sum of squares, no PCM written (include/linne_amd.h LINNEAmd_LagWindowsDevice states the
        arithmetic).  probes: a sequence of (stream_a, index_a, first_a, n, stream_b, index_b, first_b, lag_first, num_lags, pairs):
        n samples of a from first_a on (None: to the stream's end), the needle, against b at the lags lag_first .. lag_first +
        num_lags - 1, where sample first_a + i of a meets sample first_b + lag + i of b and b is 0 outside the stream; pairs a
        sequence of (channel of a, channel of b), None: (c, c) for every channel the two streams share.  Values outside the call's
        bounds raise ValueError before any call.  -> a list of LagSums, views of one allocation; lag_dots, lag_correlation and
        best_lag read a table on the host.  Errors follow measure_windows: LinneAmdError with .code and .codes when a probe fails;
        with return_codes -> (answers, codes), a failing probe's answer is None, and only a failure of the whole call raises"""
        import torch
        Q = len(probes)
        arr = (LagProbe * max(Q, 1))()
        keep, asked, at = [], [], 0
        for k, (sa, xa, first_a, n, sb, xb, first_b, lag_first, num_lags, pairs) in enumerate(probes):
            ta, tb = self._stream_bytes(sa), self._stream_bytes(sb)
            first_a, n, _ = _sample_range(xa, ta.numel(), first_a, n, "probe %d: the needle", k)
            _sample_range(xb, tb.numel(), 0, 0, "probe %d: the haystack", k)
            ca, cb = xa.header["num_channels"], xb.header["num_channels"]
            pairs = [(c, c) for c in range(min(ca, cb))] if pairs is None else [(int(i), int(j)) for i, j in pairs]
            first_b, lag_first, num_lags = int(first_b), int(lag_first), int(num_lags)
            if not 1 <= num_lags <= LAG_MAX_LAGS or not 1 <= len(pairs) <= 8:
                raise ValueError(f"probe {k}: num_lags is 1 .. {LAG_MAX_LAGS}, pairs are 1 .. 8")
            if n < 1 or first_a < 0 or first_a + n > xa.header["num_samples"]:
                raise ValueError(f"probe {k}: the needle [{first_a}, {first_a + n}) is not a range of at least one sample of its stream's {xa.header['num_samples']}")
            if n * num_lags * len(pairs) > LAG_MAX_PRODUCTS:
                raise ValueError(f"probe {k}: {n} samples * {num_lags} lags * {len(pairs)} pairs is more than LAG_MAX_PRODUCTS = 2^38")
            if not (0 <= first_b < 1 << 64 and -(1 << 63) <= lag_first < 1 << 63):
                raise ValueError(f"probe {k}: first_b is unsigned, lag_first an int64")
            if any(not (0 <= i < ca and 0 <= j < cb) for i, j in pairs):
                raise ValueError(f"probe {k}: a pair names a channel its stream ({ca} and {cb} channels) does not have")
            keep += [ta, tb]
            asked.append((at, len(pairs), num_lags, lag_first, pairs))
            at += len(pairs) * (4 * num_lags + 2)
            q = arr[k]
            q.index_a, q.d_stream_a, q.first_a, q.num_samples = xa.h, ta.data_ptr(), first_a, n
            q.index_b, q.d_stream_b, q.first_b, q.lag_first, q.num_lags, q.num_pairs = xb.h, tb.data_ptr(), first_b, lag_first, num_lags, len(pairs)
            for p, (i, j) in enumerate(pairs):
                q.chan_a[p], q.chan_b[p] = i, j
            q.pair_stride, q.reserved = num_lags, 0
        flat = torch.zeros(max(at, 1), dtype=torch.int64, device=f"cuda:{self.device}")
        for k, (base, P, L, _, _) in enumerate(asked):
            arr[k].d_out, arr[k].d_a_sq = flat.data_ptr() + 8 * base, flat.data_ptr() + 8 * (base + 4 * P * L)
        self._fence()
        ret = lib.LINNEAmd_LagWindowsDevice(self.h, arr, Q, int(group_frames))
        codes = [int(arr[k].result) for k in range(Q)]
        if ret != 0:
            msg = lib.LINNEAmd_GetLastError(self.h).decode()
            if not (return_codes and msg.startswith("probe ")):        # (a failing probe's text starts with its number)
                raise LinneAmdError(f"LagWindowsDevice -> {ret}: {msg}", ret, codes)
        out = [LagSums(flat[base:base + 4 * P * L].view(P, L, 4), flat[base + 4 * P * L:base + 4 * P * L + 2 * P].view(P, 2), lag_first, pairs)
               if codes[k] == 0 else None for k, (base, P, L, lag_first, pairs) in enumerate(asked)]
        return (out, codes) if return_codes else out

    def align_streams(self, pairs_of_streams, max_lag, needle=None):
        """where does stream b best match stream a?  pairs_of_streams: a sequence of (stream_a, stream_b); for each, a needle of a --
        `needle` = (first, n), default the whole stream cut to what LAG_MAX_PRODUCTS allows at these lags -- is slid over b: needle sample first + i meets b's sample first + lag + i,
        lag in -max_lag .. max_lag, over every channel the two share.
        One index_streams call and one lag_windows call -> a list of (lag, coefficient) as best_lag gives them: b delayed by d
        samples against a gives lag d, and laying a at output sample d of an overlay with b at 0 lines the two up.  A `needle`
        given that with 2 * max_lag + 1 lags passes LAG_MAX_PRODUCTS raises ValueError naming the limit"""
        max_lag = int(max_lag)
        if not 0 <= max_lag <= (LAG_MAX_LAGS - 1) // 2:
            raise ValueError(f"align_streams: max_lag is 0 .. {(LAG_MAX_LAGS - 1) // 2}")
        if len(pairs_of_streams) == 0:
            return []
        flat = [s for pair in pairs_of_streams for s in pair]
        with self._whole_streams(flat) as (ts, xs, _):
            probes = []
            for k in range(len(pairs_of_streams)):
                ta, tb, xa, xb = ts[2 * k], ts[2 * k + 1], xs[2 * k], xs[2 * k + 1]
                P = min(xa.header["num_channels"], xb.header["num_channels"])
                room = LAG_MAX_PRODUCTS // ((2 * max_lag + 1) * P)
                first, n = (0, min(xa.header["num_samples"], room)) if needle is None else (int(needle[0]), int(needle[1]))
                if n > room:
                    raise ValueError(f"align_streams: pair {k}: {n} samples * {2 * max_lag + 1} lags * {P} pairs is more than LAG_MAX_PRODUCTS = 2^38: give a needle of at most {LAG_MAX_PRODUCTS // ((2 * max_lag + 1) * P)} samples")
                probes.append((ta, xa, first, n, tb, xb, first, -max_lag, 2 * max_lag + 1, None))
            return [best_lag(t) for t in self.lag_windows(probes)]

    def compare_windows(self, windows, group_frames=0, return_codes=False):
        """many sample windows of resident .lnn streams compared with resident PCM in one call, nothing decoded into memory of the
        caller's (include/linne_amd.h LINNEAmd_CompareWindowsDevice).  windows: a sequence of (stream, index, first_sample,
        num_samples, pcm): the first four as decode_windows takes them, pcm as encode_stream takes it -- an int32 or int16 CUDA tensor
        (C, n) with any strides, or a uint8 one (C, n, 3) of packed 24-bit samples -- of exactly the window's (C, n).  -> a list of
        (num_differing, first_sample, first_channel) per window: the (sample, channel) elements at which the PCM is not what
        decode_windows would have written, and the first of them (lowest stream sample, then lowest channel; 0, 0 when none).  A
        window that differs is not an error.  Errors follow decode_windows: LinneAmdError with .code and .codes when a window fails;
        with return_codes -> (answers, codes), a failing window's answer is None, and only a failure of the whole call raises.  The
        PCM is only read"""
        W = len(windows)
        arr, keep, ranges = self._windows_array(windows, extra=1)
        lays = (PcmLayout * max(W, 1))()
        diffs = (Diff * max(W, 1))()
        for i, ((index, _, n), w) in enumerate(zip(ranges, windows)):
            pcm = w[4]
            fmt, cs, ss, nch, ns, _ = self._pcm_layout(pcm, f"window {i}: pcm")
            assert pcm.device.index == self.device, f"window {i}: the PCM is on {pcm.device}, the context on cuda:{self.device}"
            assert (nch, ns) == (index.header["num_channels"], max(n, 0)), \
                f"window {i} is {(index.header['num_channels'], max(n, 0))}, its pcm holds {(nch, ns)}"
            arr[i].d_pcm, arr[i].pcm_stride = pcm.data_ptr(), ns
            lays[i].format, lays[i].channel_stride, lays[i].sample_stride = fmt, cs, ss
        self._fence()
        ret = lib.LINNEAmd_CompareWindowsDevice(self.h, arr, lays, diffs, W, int(group_frames))
        codes = self._windows_codes(ret, arr, W, "CompareWindowsDevice", return_codes)
        out = [(int(diffs[i].num_differing), int(diffs[i].first_sample), int(diffs[i].first_channel)) if codes[i] == 0 else None for i in range(W)]
        return (out, codes) if return_codes else out

    def measure_windows(self, windows, bucket_samples=0, group_frames=0, return_codes=False):
        """min, max, sum and sum of squares of many sample windows of resident .lnn streams in one call, per channel and per bucket
        of bucket_samples samples, no PCM written (include/linne_amd.h LINNEAmd_MeasureWindowsDevice).  windows: a sequence of
        (stream, index, first_sample, num_samples) as decode_windows takes them; bucket_samples: one value or one per window (0: the
        whole window is one bucket; the last bucket may be short).  -> a list of Measurement, one per window, views of one
        allocation.  Every number is exact and is what numpy gives on decode_windows' int32 samples.  Errors follow
        compare_windows: LinneAmdError with .code and .codes when a window fails; with return_codes -> (answers, codes), a failing
        window's answer is None, and only a failure of the whole call raises"""
        return self._bucket_windows("measure", windows, bucket_samples, group_frames, return_codes)

    def measure_streams(self, streams, bucket_samples=0, group_frames=0):
        """min, max, sum and sum of squares of whole resident .lnn streams, per channel and bucket: one index_streams call and one
        measure_windows call over the whole streams -> a list of Measurement.  streams as index_streams takes them; bucket_samples as
        measure_windows takes it.  Raises LinneAmdError when a stream does not index or decode"""
        return self._over_whole_streams(streams, self.measure_windows, bucket_samples=bucket_samples, group_frames=group_frames)

    def digest_windows(self, windows, bucket_samples=0, group_frames=0, return_codes=False):
        """the CRC-32 of the decoded PCM of many sample windows of resident .lnn streams in one call, per bucket of bucket_samples
        samples, no PCM written (include/linne_amd.h LINNEAmd_DigestWindowsDevice).  windows: a sequence of (stream, index,
        first_sample, num_samples) as decode_windows takes them; bucket_samples: one value or one per window (0: the whole window is
        one bucket; the last bucket may be short).  -> a list of DigestTable, one per window, views of one allocation.  A digest is
        zlib.crc32 of the window's samples as a WAV file holds them (interleaved, ceil(bits / 8) bytes little-endian, 8-bit
        unsigned).  Errors follow measure_windows: LinneAmdError with .code and .codes when a window fails; with return_codes ->
        (answers, codes), a failing window's answer is None, and only a failure of the whole call raises"""
        return self._bucket_windows("digest", windows, bucket_samples, group_frames, return_codes)

    def digest_streams(self, streams, bucket_samples=0, group_frames=0):
        """the CRC-32 of the decoded PCM of whole resident .lnn streams, per bucket: one index_streams call and one digest_windows
        call over the whole streams -> a list of DigestTable.  With one bucket a stream's crc32 is zlib.crc32 of the `data` chunk of
        the WAV file the decoder writes for it.  streams as index_streams takes them; bucket_samples as digest_windows takes it.
        Raises LinneAmdError when a stream does not index or decode"""
        return self._over_whole_streams(streams, self.digest_windows, bucket_samples=bucket_samples, group_frames=group_frames)

    def quiet_windows(self, windows, threshold, min_samples=1, capacity=None, group_frames=0, return_codes=False):
        """where is the silence?  The quiet runs of many sample windows of resident .lnn streams in one call, no PCM written
        (include/linne_amd.h LINNEAmd_QuietWindowsDevice).  windows: a sequence of (stream, index, first_sample, num_samples) as
        decode_windows takes them; threshold: a frame is quiet when |v| <= threshold in every channel; min_samples: runs of at least
        so many frames are reported (0 is taken as 1); both one value or one per window.  capacity: the records per window (one value
        or one per window) -- runs beyond it are counted but not written; None: QUIET_DEFAULT_CAPACITY records, and one more call, for
        the windows that had more runs, with exactly their num_runs, so that every run is returned.  -> a list of QuietRuns, one per
        window.  Errors follow measure_windows: LinneAmdError with .code and .codes when a window fails; with return_codes ->
        (answers, codes), a failing window's answer is None, and only a failure of the whole call raises"""
        import torch
        W = len(windows)
        arr, keep, ranges = self._windows_array(windows)
        thr, mins = _per_window(threshold, W, "threshold"), _per_window(min_samples, W, "min_samples")
        caps = _per_window(QUIET_DEFAULT_CAPACITY if capacity is None else capacity, W, "capacity")
        assert all(t < (1 << 32) for t in thr), "threshold is below 2^32"

        def call(which, caps):
            """the call over windows[which] -> (ret, the Window array, tables, answers)"""
            w = (Window * max(len(which), 1))()
            specs, answers = (QuietSpec * max(len(which), 1))(), (Quiet * max(len(which), 1))()
            flat = torch.empty((max(sum(caps), 1), 2), dtype=torch.int64, device=f"cuda:{self.device}")
            at = 0
            for j, i in enumerate(which):
                C.memmove(C.byref(w[j]), C.byref(arr[i]), C.sizeof(Window))
                specs[j].threshold, specs[j].min_samples, specs[j].capacity = thr[i], mins[i], caps[j]
                specs[j].d_out = flat.data_ptr() + 16 * at if caps[j] else None
                at += caps[j]
            self._fence()
            ret = lib.LINNEAmd_QuietWindowsDevice(self.h, w, specs, answers, len(which), int(group_frames))
            tables, at = [], 0
            for j in range(len(which)):
                tables.append(flat[at:at + min(caps[j], int(answers[j].num_runs) if w[j].result == 0 else 0)])
                at += caps[j]
            return ret, w, tables, answers
        ret, w, tables, answers = call(list(range(W)), caps)
        codes = self._windows_codes(ret, w, W, "QuietWindowsDevice", return_codes)
        if capacity is None:
            more = [i for i in range(W) if codes[i] == 0 and int(answers[i].num_runs) > caps[i]]
            if more:
                ret2, w2, tables2, answers2 = call(more, [int(answers[i].num_runs) for i in more])
                self._windows_codes(ret2, w2, len(more), "QuietWindowsDevice", False)
                for j, i in enumerate(more):
                    tables[i] = tables2[j]
        out = [QuietRuns(tables[i], answers[i], thr[i], mins[i]) if codes[i] == 0 else None for i in range(W)]
        return (out, codes) if return_codes else out

    def quiet_streams(self, streams, threshold, min_samples=1, capacity=None, group_frames=0):
        """the quiet runs of whole resident .lnn streams: one index_streams call and quiet_windows over the whole streams -> a list
        of QuietRuns.  streams as index_streams takes them; the rest as quiet_windows takes it.  sound_segments turns a stream's
        runs into the cuts splice_streams takes.  Raises LinneAmdError when a stream does not index or decode"""
        return self._over_whole_streams(streams, self.quiet_windows, threshold=threshold, min_samples=min_samples, capacity=capacity, group_frames=group_frames)

    def histogram_windows(self, windows, num_bins, shift=0, log2=False, bucket_samples=0, group_frames=0, return_codes=False):
        """how are the sample levels distributed?  Histograms of |v| of many sample windows of resident .lnn streams in one call, per
        channel and per bucket of bucket_samples samples, no PCM written (include/linne_amd.h LINNEAmd_HistogramWindowsDevice).
        windows: a sequence of (stream, index, first_sample, num_samples) as decode_windows takes them.  A sample v counts in bin
        min(x, num_bins - 1), x = |v| >> shift, or with log2 the bit length of |v| >> shift (0 for 0); num_bins (1 .. HIST_MAX_BINS),
        shift (0 .. 31), log2 and bucket_samples (0: the whole window is one bucket) are one value or one per window.  -> a list of
        Histogram, one per window, views of one allocation.  Every count is exact and is what numpy.bincount gives on
        decode_windows' int32 samples.  Errors follow measure_windows: LinneAmdError with .code and .codes when a window fails; with
        return_codes -> (answers, codes), a failing window's answer is None, and only a failure of the whole call raises"""
        bins, shifts, scales = (_per_window(v, len(windows), what, hi=1 << 32, scalars=(int, np.integer, np.bool_))
                                for v, what in ((num_bins, "num_bins"), (shift, "shift"), (log2, "log2")))
        # (a table is sized for bins the call will accept; a num_bins that it refuses gets no room)
        return self._bucket_windows("histogram", windows, bucket_samples, group_frames, return_codes, words=[b if b <= HIST_MAX_BINS else 0 for b in bins],
                                    num_bins=bins, shift=shifts, scale=scales)

    def histogram_streams(self, streams, num_bins, shift=0, log2=False, bucket_samples=0, group_frames=0):
        """histograms of |v| of whole resident .lnn streams, per channel and bucket: one index_streams call and one histogram_windows
        call over the whole streams -> a list of Histogram.  streams as index_streams takes them; the rest as histogram_windows takes
        it.  level_threshold turns a linear histogram into the threshold quiet_streams takes.  Raises LinneAmdError when a stream does
        not index or decode"""
        return self._over_whole_streams(streams, self.histogram_windows, num_bins=num_bins, shift=shift, log2=log2, bucket_samples=bucket_samples,
                                        group_frames=group_frames)

    def relate_windows(self, windows, bucket_samples=0, group_frames=0, return_codes=False):
        """how do the channels relate?  Per channel pair i <= j and per bucket of bucket_samples samples, the exact sum of a_i * a_j
        (128 bits) and the counts of frames with a_i == a_j and with a_i == -a_j, of many sample windows of resident .lnn streams in
        one call, no PCM written (include/linne_amd.h LINNEAmd_RelateWindowsDevice).  windows: a sequence of (stream, index,
        first_sample, num_samples) as decode_windows takes them; bucket_samples: one value or one per window (0: the whole window is
        one bucket; the last bucket may be short).  -> a list of Relations, one per window, views of one allocation, pair (i, j) in
        row pair_index(C, i, j).  Every number is exact and is what Python integers give on decode_windows' int32 samples;
        correlation and channel_findings read the table on the host.  Errors follow measure_windows: LinneAmdError with .code and
        .codes when a window fails; with return_codes -> (answers, codes), a failing window's answer is None, and only a failure of
        the whole call raises"""
        return self._bucket_windows("relate", windows, bucket_samples, group_frames, return_codes)

    def relate_streams(self, streams, bucket_samples=0, group_frames=0):
        """the channel relations of whole resident .lnn streams, per pair and bucket: one index_streams call and one relate_windows
        call over the whole streams -> a list of Relations.  streams as index_streams takes them; bucket_samples as relate_windows
        takes it.  Raises LinneAmdError when a stream does not index or decode"""
        return self._over_whole_streams(streams, self.relate_windows, bucket_samples=bucket_samples, group_frames=group_frames)

    def same_audio(self, stream_a, stream_b, bucket_samples=0):
        """do two resident .lnn streams hold the same samples, whatever their presets, block sizes and mid/side choices?  ->
        (True, None), or (False, k) with k the first bucket of bucket_samples samples whose digests differ, or (False, None) when
        the channels, bits or sample counts differ.  One digest_streams call; equal CRC-32s of different audio are possible, one
        case in 2^32 per bucket"""
        a, b = self.digest_streams([stream_a, stream_b], bucket_samples=bucket_samples)
        if any(a.header[k] != b.header[k] for k in ("num_channels", "bits_per_sample", "num_samples")):
            return False, None
        ne = ((a.records != b.records).any(dim=1)).nonzero()
        return (True, None) if ne.numel() == 0 else (False, int(ne[0, 0]))

    def verify_streams(self, pairs, group_frames=0):
        """do these .lnn streams hold exactly these samples?  pairs: a sequence of (stream, pcm), a whole stream (as index_streams
        takes it) and the PCM it should decode to (as compare_windows takes it).  One index_streams call and one compare_windows
        call over the whole streams -> a list of (num_differing, first_sample, first_channel, reason) per pair: (0, 0, 0, None) for a
        stream that holds its PCM; the count and the first differing element (reason None) for one that decodes to other samples;
        num_differing None with the reason as text for one that does not index or decode, or whose header names other channel or
        sample counts than the PCM has.  Only a failure of a whole call raises"""
        T = len(pairs)
        if T == 0:
            return []
        with self._whole_streams([s for s, _ in pairs], return_codes=True) as (streams, indexes, icodes):
            out, wins, at = [None] * T, [], []
            for i, (x, (_, pcm)) in enumerate(zip(indexes, pairs)):
                if x is None:
                    out[i] = (None, 0, 0, f"the stream does not index (LINNEApiResult {icodes[i]})")
                    continue
                _, _, _, nch, ns, _ = self._pcm_layout(pcm, f"pair {i}: pcm")
                if (x.header["num_channels"], x.header["num_samples"]) != (nch, ns):
                    out[i] = (None, 0, 0, f"the header names {x.header['num_channels']} channels of {x.header['num_samples']} samples, the PCM has {nch} of {ns}")
                    continue
                wins.append((streams[i], x, 0, ns, pcm))
                at.append(i)
            if wins:
                answers, codes = self.compare_windows(wins, group_frames=group_frames, return_codes=True)
                for i, a, c in zip(at, answers, codes):
                    out[i] = a + (None,) if c == 0 else (None, 0, 0, f"the stream does not decode (LINNEApiResult {c})")
            return out

    def _verified(self, streams, pcms, what):
        """set_verify(True) in encode_stream / encode_streams: raises when a stream that was encoded does not hold its track's PCM"""
        live = [i for i, s in enumerate(streams) if s is not None]
        res = self.verify_streams([(streams[i], pcms[i]) for i in live])
        codes, first = [0] * len(streams), None
        for i, (k, s, c, reason) in zip(live, res):
            if k == 0:
                continue
            codes[i] = 7                                               # LINNE_APIRESULT_NG
            if first is None:
                first = f"track {i}: verification failed: {reason}" if k is None else \
                    f"track {i}: verification failed at sample {s}, channel {c} ({k} elements differ)"
        if first is not None:
            raise LinneAmdError(f"{what} -> 7: {first}", 7, codes)

    @staticmethod
    def _pcm_layout(pcm, what="pcm"):
        """(format, channel stride, sample stride, channels, samples, plain) of a PCM tensor: int32 or int16 (C, N), or uint8 (C, N, 3)
        for packed 24-bit samples, with any strides (a channels-last view is x.T); plain: int32 with contiguous rows"""
        import torch
        assert pcm.is_cuda and pcm.dtype in (torch.int32, torch.int16, torch.uint8), \
            f"{what} is an int32 or int16 CUDA tensor (C, N), or a uint8 one (C, N, 3) of packed 24-bit samples"
        if pcm.dtype == torch.uint8:
            assert pcm.dim() == 3 and pcm.shape[2] == 3 and pcm.stride(2) == 1 and pcm.stride(0) % 3 == 0 and pcm.stride(1) % 3 == 0, \
                f"{what}: a uint8 tensor is (C, N, 3), the three bytes of a sample contiguous, samples whole samples apart"
            fmt, unit = PCM_S24, 3
        else:
            assert pcm.dim() == 2, f"{what} is (C, N)"
            fmt, unit = (PCM_S32 if pcm.dtype == torch.int32 else PCM_S16), 1
        nch, ns = int(pcm.shape[0]), int(pcm.shape[1])
        cs = pcm.stride(0) // unit if nch > 1 else 0
        ss = pcm.stride(1) // unit if ns > 1 else 1
        return fmt, cs, ss, nch, ns, (fmt == PCM_S32 and ss == 1)

    def encode_stream(self, pcm, bits, rate, block, preset, ms, group_frames=0, parcor_state=None, out=None):
        """PCM (an int32 or int16 CUDA tensor (C, N) with any strides -- x.T of a channels-last (N, C) one included --, a uint8 one
        (C, N, 3) of packed little-endian 24-bit samples, or numpy: copied to the device as int32) -> a .lnn stream encoded on the device,
        as a 1-D uint8 CUDA tensor (a view of `out` when one is given); with parcor_state (a float, the quirk-Q2 state) not None, the
        pair (stream, new state).  include/linne_amd.h LINNEAmd_EncodeStreamDevice states the result contract (the library runs it as
        the one-track case of encode_streams' call).  The default buffer is
        what the reference's command line tool allocates (twice the PCM's bytes at `bits` width, plus the header); a stream that does not
        fit is encoded again into a buffer of its exact size.  Raises LinneAmdError with .code = the LINNEApiResult.  After
        set_verify(True) the stream is compared with the PCM before it is returned (verify_streams): LinneAmdError with .code = 7
        (LINNE_APIRESULT_NG) and the text "track 0: verification failed at sample s, channel c (k elements differ)" when they differ"""
        import torch
        if not isinstance(pcm, torch.Tensor):
            pcm = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.int32)).to(f"cuda:{self.device}")
        fmt, cs, ss, nch, ns, plain = self._pcm_layout(pcm)
        assert pcm.device.index == self.device, f"the PCM is on {pcm.device}, the context on cuda:{self.device}"
        lay = PcmLayout(fmt, 0, cs, ss)
        hd = Header(1, 2, nch, ns, rate, bits, block, preset, int(bool(ms)))
        state = C.c_double(0.0 if parcor_state is None else float(parcor_state))
        nbytes = C.c_uint64(0)

        def run(buf):
            state.value = 0.0 if parcor_state is None else float(parcor_state)
            self._fence()
            if not plain:
                return lib.LINNEAmd_EncodeStreamDeviceLayout(self.h, C.byref(hd), C.c_void_p(pcm.data_ptr()), C.byref(lay), int(group_frames),
                                                             C.c_void_p(buf.data_ptr()), buf.numel(), C.byref(nbytes), C.byref(state))
            return lib.LINNEAmd_EncodeStreamDevice(self.h, C.byref(hd), C.c_void_p(pcm.data_ptr()), pcm.stride(0) if nch > 1 else ns,
                                                   int(group_frames), C.c_void_p(buf.data_ptr()), buf.numel(), C.byref(nbytes),
                                                   C.byref(state))
        if out is not None:
            assert out.dtype == torch.uint8 and out.is_cuda and out.dim() == 1 and out.is_contiguous()
            buf = out
        else:
            buf = torch.empty(_default_room(nch, ns, bits), dtype=torch.uint8, device=pcm.device)
        ret = run(buf)
        if ret == 3 and out is None and nbytes.value > 0:             # LINNE_APIRESULT_INSUFFICIENT_BUFFER: once more at the exact size
            buf = torch.empty(nbytes.value, dtype=torch.uint8, device=pcm.device)
            ret = run(buf)
        self._check(ret, "EncodeStreamDevice")
        stream = buf[:nbytes.value]
        if self._verify:
            self._verified([stream], [pcm], "EncodeStreamDevice")
        return stream if parcor_state is None else (stream, state.value)

    def last_stream_encode_count(self, which):
        """the last encode_stream or encode_streams call: 0 / 1 / 2 its COMPRESS / SILENT / RAW blocks, 3 the channel-frames whose Rice plan the host settled"""
        return int(lib.LINNEAmd_GetLastStreamEncodeCount(self.h, int(which)))

    def _write_streams(self, what, noun, struct, rooms, fill, call, read):
        """encode_streams, splice_streams and repair_streams: the C call `what`, whose error texts name an item `noun`, writes every
        item's stream into rooms[i] bytes at a 4-byte-aligned offset of one allocation; the items that did not fit are written once
        more, together, at their exact sizes into another one.  struct: the call's item, with d_out, capacity, out_bytes and result;
        fill(sub[j], i) writes the rest of item i into its place of a call; call(sub, which) makes the C call over the items `which`;
        read(i, j, sub[j], item i's stream or None) takes item i's answer, before any other library call.  -> (the items' LINNEApiResults; the
        LinneAmdError of the lowest failing item, which the caller raises unless it returns the codes, or None).  A failure of a whole
        call raises here, with the codes of that call's items"""
        import torch
        T = len(rooms)
        codes, nbytes = [0] * T, [0] * T

        def run(which, sizes):
            offs, at = [], 0
            for n in sizes:
                offs.append(at)
                at += (n + 3) & ~3
            flat = torch.empty(max(at, 4), dtype=torch.uint8, device=f"cuda:{self.device}")
            sub = (struct * max(len(which), 1))()
            for j, i in enumerate(which):
                item = sub[j]
                fill(item, i)
                item.d_out, item.capacity, item.out_bytes, item.result = flat.data_ptr() + offs[j], sizes[j], 0, 0
            self._fence()
            ret = call(sub, which)
            msg = lib.LINNEAmd_GetLastError(self.h).decode() if ret != 0 else ""
            if ret != 0 and not msg.startswith(noun + " "):              # (a failing item's text starts with its noun and number)
                raise LinneAmdError(f"{what} -> {ret}: {msg}", ret, [int(sub[j].result) for j in range(len(which))])
            for j, i in enumerate(which):
                item = sub[j]
                codes[i], nbytes[i] = int(item.result), int(item.out_bytes)
                read(i, j, item, flat[offs[j]:offs[j] + nbytes[i]] if codes[i] == 0 else None)
            return ret, msg

        ret, msg = run(list(range(T)), rooms)
        again = [i for i in range(T) if codes[i] == 3 and nbytes[i] > rooms[i]]      # LINNE_APIRESULT_INSUFFICIENT_BUFFER: once more at the exact size
        if again:
            run(again, [nbytes[i] for i in again])
            bad = [i for i in range(T) if codes[i] != 0]
            ret = codes[bad[0]] if bad else 0
            msg = f"{noun} {bad[0]} failed" if bad else ""
        return codes, LinneAmdError(f"{what} -> {ret}: {msg}", ret, codes) if ret != 0 else None

    def encode_streams(self, tracks, group_frames=0, parcor_states=None, return_codes=False):
        """many tracks into their .lnn streams in one call (include/linne_amd.h LINNEAmd_EncodeStreamsDevice).  tracks: a sequence of
        (pcm, bits, rate, block, preset, ms), pcm as in encode_stream (an int32 or int16 CUDA tensor (C, N) with any strides, a uint8
        one (C, N, 3) of packed 24-bit samples, or numpy); shapes and sample formats may be mixed.  -> a list of 1-D uint8 CUDA tensors, views of one allocation at 4-byte-aligned
        offsets (None for a track that failed); every stream is what encode_stream gives for its track alone.  Each track gets the
        default room encode_stream gives it; the tracks that do not fit are encoded once more, together, at their exact sizes.  With
        parcor_states (a list of floats, the tracks' quirk-Q2 states) -> (streams, new states).  Raises LinneAmdError with .code =
        the call's result and .codes = the per-track LINNEApiResults when a track fails; with return_codes the codes are appended
        to the result, and only a failure of the whole call raises.  group_frames bounds the frames of one pass (0: one pass per
        shape) and never changes a byte.  After set_verify(True) every encoded stream is compared with its track's PCM before anything is
        returned (one verify_streams call): LinneAmdError with .code = 7 (LINNE_APIRESULT_NG), .codes per track (7 where a track
        differs) and the text "track i: verification failed at sample s, channel c (k elements differ)" when one differs"""
        import torch
        dev = f"cuda:{self.device}"
        T = len(tracks)
        assert parcor_states is None or len(parcor_states) == T
        arr = (Track * max(T, 1))()
        lays = (PcmLayout * max(T, 1))()
        keep, rooms, all_plain = [], [], True
        for i, (pcm, bits, rate, block, preset, ms) in enumerate(tracks):
            if not isinstance(pcm, torch.Tensor):
                pcm = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.int32)).to(dev)
            if pcm.dtype == torch.int32 and pcm.is_cuda and pcm.dim() == 2 and pcm.stride(1) == 1:      # int32 planar: the call without layouts
                nch, ns = pcm.shape
                lays[i].channel_stride, lays[i].sample_stride = pcm.stride(0) if nch > 1 else 0, 1
            else:
                fmt, cs, ss, nch, ns, plain = self._pcm_layout(pcm, f"track {i}: pcm")
                lays[i].format, lays[i].channel_stride, lays[i].sample_stride = fmt, cs, ss
                all_plain = all_plain and plain
            assert pcm.device.index == self.device, f"track {i}: the PCM is on {pcm.device}, the context on cuda:{self.device}"
            keep.append(pcm)
            arr[i].header = Header(1, 2, nch, ns, rate, bits, block, preset, int(bool(ms)))
            arr[i].d_pcm, arr[i].pcm_stride = pcm.data_ptr(), pcm.stride(0) if nch > 1 else ns
            rooms.append(_default_room(nch, ns, bits))
        states, streams = [0.0] * T, [None] * T

        def fill(track, i):
            C.memmove(C.byref(track), C.byref(arr[i]), C.sizeof(Track))
            track.parcor_state = 0.0 if parcor_states is None else float(parcor_states[i])

        def call(sub, which):
            if all_plain:
                return lib.LINNEAmd_EncodeStreamsDevice(self.h, sub, len(which), int(group_frames))
            sublay = (PcmLayout * max(len(which), 1))(*[lays[i] for i in which])
            return lib.LINNEAmd_EncodeStreamsDeviceLayout(self.h, sub, sublay, len(which), int(group_frames))

        def read(i, j, track, stream):
            states[i], streams[i] = float(track.parcor_state), stream
        codes, failed = self._write_streams("EncodeStreamsDevice", "track", Track, rooms, fill, call, read)
        if failed and not return_codes:
            raise failed
        if self._verify:
            self._verified(streams, keep, "EncodeStreamsDevice")
        out = (streams,) if parcor_states is None else (streams, states)
        if return_codes:
            out += (codes,)
        return out[0] if len(out) == 1 else out

    def last_stream_batch_count(self, which):
        """the last encode_streams call (its second one, where tracks were encoded again): 0 its shape groups, 1 its passes, 2 its
        EncodeFramesDevice calls; after an encode_stream call: 1 group, its passes, one analysis call per pass"""
        return int(lib.LINNEAmd_GetLastStreamBatchCount(self.h, int(which)))

    def splice_streams(self, splices, group_frames=0, return_codes=False):
        """cuts of resident .lnn streams joined into new streams in one call, only the blocks a cut goes through re-encoded
        (include/linne_amd.h LINNEAmd_SpliceStreamsDevice).  splices: a sequence of outputs, each a list of cuts (data, index,
        first_sample, num_samples): a 1-D uint8 CUDA tensor, its StreamIndex and the range (num_samples None: to the stream's end).
        -> a list of 1-D uint8 CUDA tensors, views of one allocation at 4-byte-aligned offsets (None for an output that failed).
        Each output gets the room of its cuts' streams whole plus an edge block's bound per cut end; one that still does not fit is
        spliced once more at its exact size.  Raises LinneAmdError with .code = the call's result and .codes = the per-output
        LINNEApiResults when an output fails; with return_codes -> (streams, codes), and only a failure of the whole call raises.
        group_frames bounds the edge blocks decoded and encoded per pass and never changes a byte.  Afterwards self.last_splice_blocks
        holds every output's (copied, re-encoded) block counts"""
        keep, cutlists, rooms = [], [], []
        for k, cuts in enumerate(splices):
            cs = (Cut * max(len(cuts), 1))()
            room = 30
            for i, (data, index, first, n) in enumerate(cuts):
                t = self._stream_bytes(data)
                first, _, count = _sample_range(index, t.numel(), first, n, "splice %d, cut %d", k, i)
                cs[i].index, cs[i].d_stream, cs[i].first_sample, cs[i].num_samples = index.h, t.data_ptr(), first, count
                keep.append(t)
                room += t.numel() + 2 * (64 + index.header["num_channels"] * index.header["num_samples_per_block"] * 8)
            cutlists.append((cs, len(cuts)))
            rooms.append(room)
        streams, counts = [None] * len(splices), [(0, 0)] * len(splices)

        def fill(splice, k):
            splice.cuts, splice.num_cuts = cutlists[k]

        def read(k, j, splice, stream):
            streams[k], counts[k] = stream, (int(splice.copied_blocks), int(splice.encoded_blocks))
        codes, failed = self._write_streams("SpliceStreamsDevice", "splice", Splice, rooms, fill,
                                            lambda sub, which: lib.LINNEAmd_SpliceStreamsDevice(self.h, sub, len(which), int(group_frames)), read)
        self.last_splice_blocks = counts
        if failed and not return_codes:
            raise failed
        return (streams, codes) if return_codes else streams

    def last_splice_count(self, which):
        """the last splice_streams call (its second one, where outputs were spliced again): 0 the outputs written, 1 their copied
        blocks, 2 their re-encoded blocks, 3 the copy runs, 4 the bytes they moved, 5 the host synchronisations of the call's own steps"""
        return int(lib.LINNEAmd_GetLastSpliceCount(self.h, int(which)))

    def repair_streams(self, streams, return_codes=False):
        """damaged resident .lnn streams turned into valid ones in one call: sound blocks kept byte for byte, lost stretches replaced
        by SILENT blocks (include/linne_amd.h LINNEAmd_RepairStreamsDevice).  streams: a sequence of 1-D uint8 CUDA tensors, bytes
        or numpy arrays -> a list of (stream, report): stream a 1-D uint8 CUDA view of one allocation at a 4-byte-aligned offset
        (None for a stream that failed), report a dict of out_bytes, result, kept_blocks, fill_blocks, num_gaps, lost_samples, exact
        and gaps (a list of dicts: first_sample, num_samples, src_offset, src_bytes, fill_blocks).  Every stream gets the room of its
        own bytes plus the fill blocks of a wholly lost stream; one that still does not fit is repaired once more at its exact size.
        Raises LinneAmdError with .code = the call's result and .codes = the per-stream LINNEApiResults when a stream fails; with
        return_codes -> (list, codes), and only a failure of the whole call raises"""
        import torch
        T = len(streams)
        keep = [self._stream_bytes(s) for s in streams]
        whole = [k for k in range(T) if keep[k].numel() >= 30]              # the headers' sample counts and block sizes: one copy
        heads = torch.stack([keep[k][:30] for k in whole]).cpu().numpy() if whole else np.zeros((0, 30), np.uint8)
        rooms = [t.numel() + 22 for t in keep]
        for row, k in zip(heads, whole):
            n, s = int.from_bytes(bytes(row[14:18]), "big"), int.from_bytes(bytes(row[24:28]), "big")
            rooms[k] = keep[k].numel() + 11 * (n // max(min(s, 65535), 1) + 2)
        out = [(None, None)] * T

        def fill(r, k):
            r.d_stream, r.stream_bytes = keep[k].data_ptr(), keep[k].numel()

        def read(k, j, r, stream):
            report = {f: int(getattr(r, f)) for f in ("out_bytes", "result", "kept_blocks", "fill_blocks", "num_gaps", "lost_samples", "exact")}
            gaps, n = C.POINTER(Gap)(), C.c_uint32(0)
            self._check(lib.LINNEAmd_GetLastRepairGaps(self.h, j, C.byref(gaps), C.byref(n)), "GetLastRepairGaps")      # (j: the stream's number within that call)
            report["gaps"] = [{f: int(getattr(gaps[i], f)) for f in ("first_sample", "num_samples", "src_offset", "src_bytes", "fill_blocks")} for i in range(n.value)]
            out[k] = (stream, report)
        codes, failed = self._write_streams("RepairStreamsDevice", "repair", Repair, rooms, fill,
                                            lambda sub, which: lib.LINNEAmd_RepairStreamsDevice(self.h, sub, len(which)), read)
        if failed and not return_codes:
            raise failed
        return (out, codes) if return_codes else out

    def last_repair_count(self, which):
        """the last repair_streams call (its second one, where streams were repaired again): 0 the outputs written, 1 their kept
        blocks, 2 their fill blocks, 3 their gaps, 4 the copy runs, 5 its host synchronisations, 6 its kernel launches"""
        return int(lib.LINNEAmd_GetLastRepairCount(self.h, int(which)))

    def encode_frames_host(self, shape, pcm, num_samples=None):
        """numpy int32 [F][C][S] -> numpy (residual, params, stats)"""
        pcm = np.ascontiguousarray(pcm, dtype=np.int32)
        F, Cn, S = pcm.shape
        res = np.zeros_like(pcm)
        prm = np.zeros((F, Cn, PARAM_WORDS), dtype=np.int32)
        st = np.zeros((F, Cn, STAT_WORDS), dtype=np.float64)
        ns = np.ascontiguousarray(num_samples, dtype=np.uint32) if num_samples is not None else None
        self._check(lib.LINNEAmd_EncodeFramesHost(self.h, C.byref(shape), pcm.ctypes.data, ns.ctypes.data if ns is not None else None,
                                                  F, res.ctypes.data, prm.ctypes.data, st.ctypes.data), "EncodeFramesHost")
        return res, prm, st

    def decode_frames_host(self, shape, residual, params, num_samples=None):
        d = np.ascontiguousarray(residual, dtype=np.int32).copy()
        prm = np.ascontiguousarray(params, dtype=np.int32)
        ns = np.ascontiguousarray(num_samples, dtype=np.uint32) if num_samples is not None else None
        self._check(lib.LINNEAmd_DecodeFramesHost(self.h, C.byref(shape), d.ctypes.data, ns.ctypes.data if ns is not None else None,
                                                  d.shape[0], prm.ctypes.data), "DecodeFramesHost")
        return d


class Multi:
    """Several GPUs from one process (include/linne_amd.h LINNEAmd_Multi*): groups of frames fan out round-robin over per-GPU
    contexts, each GPU fed over its own PCIe link; host numpy arrays in and out, the caller's frame order kept."""

    def __init__(self, devices=None, scratch_bytes=0):
        if devices:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            self.h = lib.LINNEAmd_MultiCreate(arr, len(devices), int(scratch_bytes))
        else:
            self.h = lib.LINNEAmd_MultiCreate(None, 0, int(scratch_bytes))
        if not self.h:
            raise LinneAmdError(f"LINNEAmd_MultiCreate({devices}) failed: no usable HIP device (there is no CPU fallback)")

    @property
    def num_devices(self):
        return int(lib.LINNEAmd_MultiNumDevices(self.h))

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.LINNEAmd_MultiDestroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, ret, what):
        if ret != 0:
            raise LinneAmdError(f"{what} -> {ret}: {lib.LINNEAmd_MultiGetLastError(self.h).decode()}")

    def encode_frames_host(self, shape, pcm, num_samples=None, group_frames=0, want_plan=False, out=None):
        pcm = np.ascontiguousarray(pcm, dtype=np.int32)
        F, Cn, S = pcm.shape
        if out is None:
            res = np.empty_like(pcm)
            prm = np.zeros((F, Cn, PARAM_WORDS), dtype=np.int32)
            st = np.zeros((F, Cn, STAT_WORDS), dtype=np.float64)
        else:
            res, prm, st = out
        plan = np.zeros((F, Cn, RICE_PLAN_BYTES), dtype=np.uint8) if want_plan else None
        ns = np.ascontiguousarray(num_samples, dtype=np.uint32) if num_samples is not None else None
        self._check(lib.LINNEAmd_MultiEncodeFramesHost(self.h, C.byref(shape), pcm.ctypes.data, ns.ctypes.data if ns is not None else None, F,
                                                       res.ctypes.data, prm.ctypes.data, st.ctypes.data,
                                                       plan.ctypes.data if plan is not None else None, int(group_frames)), "MultiEncodeFramesHost")
        return (res, prm, st, plan) if want_plan else (res, prm, st)

    def decode_frames_host(self, shape, residual, params, num_samples=None, group_frames=0, in_place=False):
        d = np.ascontiguousarray(residual, dtype=np.int32)
        if not in_place:
            d = d.copy()
        prm = np.ascontiguousarray(params, dtype=np.int32)
        ns = np.ascontiguousarray(num_samples, dtype=np.uint32) if num_samples is not None else None
        self._check(lib.LINNEAmd_MultiDecodeFramesHost(self.h, C.byref(shape), d.ctypes.data, ns.ctypes.data if ns is not None else None,
                                                       d.shape[0], prm.ctypes.data, int(group_frames)), "MultiDecodeFramesHost")
        return d


def pack_frames_emitted(shape, planes, first_sample, params, stats, plan, packed, offsets, num_samples=None, parcor_state=0.0, threads=0, residual=None):
    """host stitch stage over the device's Rice codes (LINNEAmd_PackFramesEmitted): planes = int32 [C][total samples] (the caller's PCM),
    the batch's frames start at first_sample; residual [F][C][S] (numpy) serves the fetch callback for channel-frames without a code"""
    planes = np.ascontiguousarray(planes, dtype=np.int32)
    params = np.ascontiguousarray(params, dtype=np.int32)
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    plan = np.ascontiguousarray(plan, dtype=np.uint8)
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets).view(np.uint32)
    F, Cn = params.shape[0], params.shape[1]
    ptrs = (C.POINTER(C.c_int32) * Cn)(*[planes[ch].ctypes.data_as(C.POINTER(C.c_int32)) for ch in range(Cn)])
    cap = F * Cn * shape.num_samples_per_block * 8 + 64 * F + 64
    out = np.zeros(cap, dtype=np.uint8)
    sizes = np.zeros(F, dtype=np.uint32)
    ns = np.ascontiguousarray(num_samples, dtype=np.uint32) if num_samples is not None else None
    st = C.c_double(parcor_state)
    fetched = []
    FETCH = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32))

    def _fetch(arg, frame, dst):
        if residual is None:
            return 7
        fetched.append(int(frame))
        C.memmove(dst, np.ascontiguousarray(residual[frame], dtype=np.int32).ctypes.data, Cn * shape.num_samples_per_block * 4)
        return 0

    cb = FETCH(_fetch)
    ret = lib.LINNEAmd_PackFramesEmitted(C.byref(shape), ptrs, int(first_sample), ns.ctypes.data if ns is not None else None, F,
                                         params.ctypes.data, stats.ctypes.data, plan.ctypes.data, packed.ctypes.data, offsets.ctypes.data,
                                         C.cast(cb, C.c_void_p), None, out.ctypes.data, cap, sizes.ctypes.data, C.byref(st), threads or (os.cpu_count() or 1))
    if ret != 0:
        raise LinneAmdError(f"PackFramesEmitted -> {ret}")
    blocks, off = [], 0
    for s in sizes:
        blocks.append(out[off:off + int(s)].tobytes())
        off += int(s)
    return blocks, st.value, fetched


def pack_frames(shape, pcm, residual, params, stats, num_samples=None, parcor_state=0.0, threads=0, plan=None):
    """host entropy stage: numpy arrays of one batch -> (list of block bytes, new parcor_state); plan = the device's
    Rice plan (Context.rice_plan, as a numpy uint8 array) or None for the host search"""
    pcm = np.ascontiguousarray(pcm, dtype=np.int32)
    residual = np.ascontiguousarray(residual, dtype=np.int32)
    params = np.ascontiguousarray(params, dtype=np.int32)
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    F = pcm.shape[0]
    cap = pcm.size * 8 + 64 * F + 64
    out = np.zeros(cap, dtype=np.uint8)
    sizes = np.zeros(F, dtype=np.uint32)
    ns = np.ascontiguousarray(num_samples, dtype=np.uint32) if num_samples is not None else None
    st = C.c_double(parcor_state)
    if plan is not None:
        plan = np.ascontiguousarray(plan, dtype=np.uint8)
        assert plan.shape == (F, pcm.shape[1], RICE_PLAN_BYTES)
    ret = lib.LINNEAmd_PackFramesPlanned(C.byref(shape), pcm.ctypes.data, ns.ctypes.data if ns is not None else None, F,
                                         residual.ctypes.data, params.ctypes.data, stats.ctypes.data,
                                         plan.ctypes.data if plan is not None else None, out.ctypes.data, cap,
                                         sizes.ctypes.data, C.byref(st), threads or (os.cpu_count() or 1))
    if ret != 0:
        raise LinneAmdError(f"PackFrames -> {ret}")
    blocks, off = [], 0
    for s in sizes:
        blocks.append(out[off:off + int(s)].tobytes())
        off += int(s)
    return blocks, st.value
