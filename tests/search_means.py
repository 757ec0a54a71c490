"""What tests/test_search_means_cpu.py and tests/test_gpu_search_means.py share: the inputs, the interval a trial mean of the unit-count
search has to lie in, an independent high-precision evaluation of the means, and the comparison routine.

The interval is DESIGN.md section 4's ("The certified unit-count search"), as k_select applies it (lnn_k_fir.h): a mean m of the
search kernels' order-free sums on fused multiply-adds and the reference's ordered mean m_ref of the same trial differ by at most

    rel * m_ref + slack,    rel = (2 na + 8) 2^-53,    slack = 4 (np + 2) 2^-53 max|x| (1 + max_unit sum_k |h_k|)

with na the analysis length, np the taps of a unit of the trial, x the layer's input and h the trial's coefficients.  Both are
computed HERE from the oracle's quantities; nothing a kernel reports enters a bound.
"""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from signals import music_frames

EPS = 2.0 ** -53


def rel_of(na):
    return (2.0 * na + 8.0) * EPS


def slack_of(np_, xmax, hmax):
    return 4.0 * (np_ + 2.0) * EPS * xmax * (1.0 + hmax)


def bounds_of(search, ref_means=None):
    """the half-width of the interval around each trial's reference mean: rel * m_ref + slack, in longdouble"""
    m = np.asarray(search["mean"] if ref_means is None else ref_means, dtype=np.longdouble)
    np_ = search["P"] // search["units"].astype(np.float64)
    sl = np.array([slack_of(a, x, h) for a, x, h in zip(np_, search["xmax"], search["hmax"])], dtype=np.longdouble)
    return np.longdouble(rel_of(search["n"])) * m + sl


def violations(means, search, ref_means=None):
    """the comparison routine: [(trial, |m - m_ref|, bound)] for every trial whose mean lies outside the interval (or is not a number)"""
    ref = np.asarray(search["mean"] if ref_means is None else ref_means, dtype=np.longdouble)
    d = np.abs(np.asarray(means, dtype=np.longdouble) - ref)
    b = bounds_of(search, ref_means)
    return [(int(t), float(d[t]), float(b[t])) for t in range(len(ref)) if not d[t] <= b[t]]


def headroom(means, search):
    """the smallest bound / |m - m_ref| over the trials (inf where a mean equals the reference's)"""
    d = np.abs(np.asarray(means, dtype=np.longdouble) - search["mean"].astype(np.longdouble))
    b = bounds_of(search)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where(d > 0, b / d, np.inf)
    return float(np.min(h))


def exact_terms(x, h, units):
    """|residual| of every sample of one trial (linne_network.c:318-335: sample s of the frame is x[s] + sum_k h_unit[k] x[s - np + k],
    samples in front of the frame are absent, the frame's first sample counts nothing), every product and sum in longdouble"""
    n, P = len(x), len(h)
    np_, ns = P // units, n // units
    assert np_ * units == P and ns * units == n
    xl = np.concatenate([np.zeros(np_, dtype=np.longdouble), x.astype(np.longdouble)])
    win = np.lib.stride_tricks.sliding_window_view(xl, np_)[:n]          # win[s] = x[s - np .. s - 1]
    res = x.astype(np.longdouble).copy()
    hl = h.astype(np.longdouble)
    for un in range(units):
        res[un * ns:(un + 1) * ns] += win[un * ns:(un + 1) * ns] @ hl[un * np_:(un + 1) * np_]
    t = np.abs(res)
    t[0] = 0
    return t


def fsum_mean(terms):
    """mean of longdouble terms, summed by math.fsum over their double heads and tails: order-free and exact to the last rounding"""
    hi = terms.astype(np.float64)
    lo = (terms - hi.astype(np.longdouble)).astype(np.float64)
    return np.longdouble(math.fsum(hi.tolist() + lo.tolist())) / np.longdouble(len(terms))


def exact_means(search):
    return np.array([fsum_mean(exact_terms(search["input"], search["coef"][t], int(u))) for t, u in enumerate(search["units"])], dtype=np.longdouble)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs.  A batch cycles over a few distinct frames (music, then a frame of silence and a frame of a constant where the signal has
# them) and, with another period, over a list of lengths: the oracle runs once per distinct (frame, length), the batch can be as
# large as a kernel form needs, and neighbouring frames of the caller's order differ in length, so that a capture record that went
# to a neighbour's slot shows.
# ---------------------------------------------------------------------------------------------------------------------------------
def signal(preset, nch, bits, block, ms, seed, nmusic=4, specials=True, quiet=()):
    return {"preset": preset, "nch": nch, "bits": bits, "block": block, "ms": ms, "seed": seed, "nmusic": nmusic, "specials": specials, "quiet": tuple(quiet)}


MIX = [10240, 9280, 8192, 10240, 3001, 10240, 129]          # two lengths k_search_long takes, the ragged ones between and behind them
SIG7 = signal(7, 2, 16, 10240, True, 11)                     # (4, 128, 16), four regulariser passes
SIG3 = signal(3, 2, 16, 10240, True, 12)                     # (4, 64, 8), two
SIG5 = signal(5, 2, 16, 10240, True, 13)                     # (4, 128, 16), one
SIG7M = signal(7, 1, 16, 10240, False, 14, nmusic=2, specials=False)
SIG7S = signal(7, 2, 16, 3072, True, 15, nmusic=3)           # a block below 4096 that is not whole tiles
SIG1 = signal(1, 1, 8, 2048, False, 16, nmusic=3)            # (2, 32), 8-bit, mono
SIG5W = signal(5, 8, 24, 10240, False, 17, nmusic=2, specials=False)      # eight channels of loud 24-bit material
SIG3W = signal(3, 2, 24, 10240, True, 18, nmusic=4, specials=False, quiet=(1, 3))   # 24-bit, loud and quiet (1/64) frames
FULL = [10240]

# name, signal, frames, lengths, environment, what has to be seen.  kinds / absent: timing kinds (include/linne_amd.h) with / without
# launches; form: LINNEAmd_GetLastSearchLongForm; jobs_per_chunk: "wave" (<= 256 jobs: k_select_wave decides) or "select" (k_select);
# chunks: at least so many chunks (kind 1 has a launch per chunk); how: the only way searches may be decided (None: any)
CASES = [
    ("m7 per-job", SIG7, 42, MIX, {"LINNE_AMD_SEARCH_JOB": "1", "LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "form": 1, "decider": "select"}),
    ("m7 tiles", SIG7, 42, MIX, {"LINNE_AMD_SEARCH_JOB": "0", "LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "form": 0, "decider": "select"}),
    ("m7 one pass", SIG7, 42, MIX, {"LINNE_AMD_SEARCH_TWO": "0", "LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "form": 0, "decider": "select"}),
    ("m7 no fused forward", SIG7, 42, MIX, {"LINNE_AMD_SPECULATE": "0", "LINNE_AMD_STREAMS": "1"}, {"kinds": (15, 18, 7, 6), "absent": (25, 5), "form": -1, "decider": "select"}),
    ("m7 exact", SIG7, 7, MIX, {"LINNE_AMD_EXACT": "1", "LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "decider": "wave", "how": 1}),
    ("m7 small batch", SIG7, 7, MIX, {"LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "form": 1, "decider": "wave"}),
    ("m7 one mono block", SIG7M, 1, FULL, {"LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 15, 18, 7, 6), "absent": (5,), "form": 0, "decider": "wave"}),
    ("m7 two chunks", SIG7, 42, MIX, {"LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "chunks": 2, "arena": 0.55, "decider": "wave"}),
    ("m7 last layer", SIG7, 42, FULL, {"LINNE_AMD_LAST_LAYER": "2", "LINNE_AMD_FWD_LOSS": "1", "LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 15, 20, 7), "absent": (5, 18), "form": 1, "decider": "select", "last_how": 2}),
    ("m7 short blocks", SIG7S, 6, [3072, 3072, 1000], {"LINNE_AMD_STREAMS": "1"}, {"kinds": (5, 15, 18, 7, 6), "absent": (25,), "decider": "wave"}),
    ("m3 per-job", SIG3, 84, MIX, {"LINNE_AMD_SEARCH_JOB": "1", "LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "form": 1, "decider": "select"}),
    ("m3 tiles", SIG3, 84, MIX, {"LINNE_AMD_SEARCH_JOB": "0", "LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "form": 0, "decider": "select"}),
    ("m3 one pass", SIG3, 84, MIX, {"LINNE_AMD_SEARCH_TWO": "0", "LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "form": 0, "decider": "select"}),
    ("m3 last layer", SIG3, 84, FULL, {"LINNE_AMD_LAST_LAYER": "2", "LINNE_AMD_FWD_LOSS": "1", "LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 15, 20, 7), "absent": (5, 18), "form": 1, "decider": "select", "last_how": 2}),
    ("m3 24 bit", SIG3W, 8, MIX, {"LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "decider": "wave"}),
    ("m1 8 bit mono", SIG1, 12, [2048, 1000, 2048, 129], {"LINNE_AMD_STREAMS": "1"}, {"kinds": (15, 18, 7, 6), "absent": (25, 5), "decider": "wave"}),
    ("m5 8 channels 24 bit", SIG5W, 3, [10240, 9280, 3001], {"LINNE_AMD_STREAMS": "1"}, {"kinds": (25, 5, 15, 18, 7, 6), "decider": "wave"}),
    ("m5 two streams", SIG5, 1024, MIX, {"LINNE_AMD_STREAMS": "2"}, {"kinds": (25, 5, 15, 18, 7, 6), "chunks": 2, "decider": "select"}),
]
CASE_IDS = [c[0].replace(" ", "_") for c in CASES]


def bases_of(sig):
    """the distinct frames of a signal [nbase][C][block] and the indices of the silent and the constant one (None without them)"""
    b = music_frames(sig["nmusic"], sig["nch"], sig["block"], sig["bits"], seed=sig["seed"])
    for q in sig["quiet"]:
        b[q] //= 64
    if not sig["specials"]:
        return b, None, None
    sp = np.zeros((2,) + b.shape[1:], dtype=np.int32)
    sp[1] = 1000 if sig["bits"] > 8 else 100
    return np.concatenate([b, sp]), sig["nmusic"], sig["nmusic"] + 1


def build_batch(sig, F, lens):
    """([F][C][block] int32, lengths, base index per frame)"""
    bases, _, _ = bases_of(sig)
    bmap = np.arange(F) % len(bases)
    ns = np.array([lens[f % len(lens)] for f in range(F)], dtype=np.uint32)
    frames = bases[bmap].copy()
    for f in range(F):
        frames[f, :, int(ns[f]):] = 0
    return np.ascontiguousarray(frames), ns, bmap


def sig_key(sig):
    return tuple(sorted(sig.items()))


def oracle_searches(oracle, sig, frames, ns, bmap, cache, with_data=False):
    """the oracle's hot path with its trial tap, once per distinct (frame, length) of the batch, on a pool of threads: the tap is
    thread-local and Encoder.hotpath_trials sets and reads it inside the call, on the worker's own thread.
    -> {(base, n): (tap, residual, searches[ch][pass][layer])}"""
    keys = {}
    for f in range(len(ns)):
        keys.setdefault((int(bmap[f]), int(ns[f])), f)
    todo = [(k, f) for k, f in keys.items() if (sig_key(sig), with_data) + k not in cache]

    def one(kf):
        k, f = kf
        enc = oracle.encoder(sig["nch"], sig["bits"], 44100, sig["block"], sig["preset"], sig["ms"])
        out = enc.hotpath_trials(frames[f][:, :k[1]], with_data=with_data)
        enc.close()
        return k, out

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        for k, out in ex.map(one, todo):
            cache[(sig_key(sig), with_data) + k] = out
    return {k: cache[(sig_key(sig), with_data) + k] for k in keys}
