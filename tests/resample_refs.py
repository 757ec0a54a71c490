"""The reference for resampling windows of resident .lnn streams (tests/test_stream_resample_cpu.py, tests/test_gpu_stream_resample.py):
what LINNEAmd_ResampleWindowsDevice must write, from numpy int64 on the oracle's decode of the same bytes, never from the library under
test -- a direct transcription of steps 1 to 3 of include/linne_amd.h and of the layouts' conversions.  Stated once, here;
tests/test_stream_resample_cpu.py holds it to hand-written values."""
import numpy as np

FORMATS = ("s32", "s16", "s24", "f32")
ELEMENT_BYTES = {"s32": 4, "s16": 2, "s24": 3, "f32": 4}


def resampled_length(N, up, down):
    return -(-(N * up) // down)


def resampled_values(full, first, n, coef, up, down, before, shift=0, clip_bits=0):
    """outputs [first, first + n) of the stream `full` (C, N) int32 resampled by up/down -> (y int64 (C, n), clipped?).  coef: (up, P)
    integers within int16"""
    full = np.asarray(full)
    assert full.dtype == np.int32 and full.ndim == 2
    coef = np.asarray(coef, dtype=np.int64)
    assert coef.ndim == 2 and coef.shape[0] == up and coef.min(initial=0) >= -32768 and coef.max(initial=0) <= 32767
    P = coef.shape[1]
    assert 1 <= up <= 1024 and 1 <= down <= 1024 and 1 <= P <= 64 and 0 <= before < P and 0 <= shift <= 31 and (clip_bits == 0 or 2 <= clip_bits <= 32)
    C, N = full.shape
    assert 0 <= first and first + n <= resampled_length(N, up, down)
    m = first + np.arange(n, dtype=np.int64)
    t = m * down
    p, nn = t % up, t // up
    idx = nn[:, None] - before + np.arange(P, dtype=np.int64)[None, :]            # (n, P): the input samples of every output
    inside = (idx >= 0) & (idx < N)
    x = np.where(inside[None], full.astype(np.int64)[:, np.clip(idx, 0, max(N - 1, 0))], 0)
    acc = (x * coef[p][None]).sum(axis=2)                           # |a product| <= 2^46, 64 of them 2^52: int64 holds it
    y = (acc + (1 << (shift - 1))) >> shift if shift else acc      # (numpy's >> on int64 is arithmetic)
    B = clip_bits or 32
    c = np.clip(y, -(1 << (B - 1)), (1 << (B - 1)) - 1)
    return c, bool((c != y).any())


def expected_resample(full, first, n, coef, up, down, before, shift=0, clip_bits=0, fmt="s32", bits=16):
    """... in the format fmt -> (the elements (C, n): int32, int16, uint8 (C, n, 3) little-endian, or float32; saturated).  bits: the
    stream's bits_per_sample, the float format's scale where clip_bits is 0"""
    assert fmt in FORMATS
    y, sat = resampled_values(full, first, n, coef, up, down, before, shift, clip_bits)
    if fmt == "s32":
        return y.astype(np.int32), sat
    if fmt == "f32":
        Bf = clip_bits or bits
        return y.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -(Bf - 1)), sat
    top = 32767 if fmt == "s16" else 8388607
    c = np.clip(y, -top - 1, top)
    sat = sat or bool((c != y).any())
    if fmt == "s16":
        return c.astype(np.int16), sat
    u = (c & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8), sat


def random_coef(rng, up, P):
    """(up, P) int16: random coefficients with the extremes among them"""
    c = rng.integers(-32768, 32768, size=(up, P))
    flat = c.reshape(-1)
    for at, x in zip(rng.permutation(flat.size), (32767, -32767, -32768, 0, 1, -1)):
        flat[at] = x
    return np.ascontiguousarray(c, dtype=np.int16)


KAISER_BETA = 8.0


def kaiser_prototype(up, down, taps, beta=KAISER_BETA):
    """the float64 prototype of LINNEAmd_ResampleDesign from the formula: up * taps points of sinc(d / max(up, down)) under a Kaiser
    window of the given beta, d the distance from the centre (up * taps - 1) / 2"""
    n = up * taps
    d = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
    r = d / (0.5 * (n - 1)) if n > 1 else np.zeros(1)
    return np.sinc(d / max(up, down)) * np.i0(beta * np.sqrt(np.clip(1.0 - r * r, 0.0, 1.0))) / np.i0(beta)


def prototype_of(coef):
    """the phases (up, P) put back into the prototype they were split from: point p + (P - 1 - k) * up is coef[p][k]"""
    coef = np.asarray(coef)
    return np.ascontiguousarray(coef[:, ::-1].T).reshape(-1)


def stopband_db(proto, up, down, taps, beta=KAISER_BETA):
    """the largest response of the prototype behind its stopband's edge, in dB below its response at 0.  The edge: the cutoff
    1 / (2 max(up, down)) cycles per point plus the Kaiser window's half main-lobe width sqrt(1 + (beta / pi)^2) / (up * taps)"""
    proto = np.asarray(proto, dtype=np.float64)
    nfft = 1 << int(np.ceil(np.log2(proto.size * 16)))
    H = np.abs(np.fft.rfft(proto, nfft))
    edge = 0.5 / max(up, down) + np.sqrt(1.0 + (beta / np.pi) ** 2) / (up * taps)
    k = int(np.ceil(edge * nfft))
    assert k < H.size
    return float(20.0 * np.log10(H[0] / H[k:].max()))
