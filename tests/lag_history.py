"""The scenarios of tests/test_gpu_stream_lags_history.py, as plain data in the form of tests/stream_history.py: does the answer of a
lag_windows call depend on the calls the context served before it?  The windows calls share buffers of the context that grow and are
never cleared (the pinned lists, their device copy, the scratch with the images and partial sums behind it), so a lag call's images
and partial sums land where another consumer's samples, accumulators or images lay, and the other way round.  A scenario is a list of
steps that the GPU test runs in order on ONE context.  A step is a dict:

    {"call": "lags" or a sibling ("measure", "quiet", "mix", "resample", "overlay", "relate"), "gf": group_frames, "note": the stale
     state the step is written to meet; lags: "probes": [(stream a, first_a, n, stream b, first_b, lag_first, num_lags, pairs)];
     a sibling: "wins": [(stream name, first sample, samples)]}

The streams are stream_history's.  A lags step's expected answer comes from lag_refs on the oracle's decode, whatever ran before; a
sibling's step has to succeed -- its own history tests hold its answer."""
import numpy as np

from stream_history import NAMES, SPEC, num_samples

SIBLINGS = ["measure", "quiet", "mix", "resample", "overlay", "relate"]
CHANNELS = {name: SPEC[name][0] for name in NAMES}


def lags(probes, gf=0, note=""):
    return {"call": "lags", "probes": list(probes), "gf": gf, "note": note}


def sibling(call, wins, gf=0, note=""):
    return {"call": call, "wins": list(wins), "gf": gf, "note": note}


def pairs_of(a, b, k):
    """1 to 3 pairs of channels the two streams have, rotated by k"""
    ca, cb = CHANNELS[a], CHANNELS[b]
    return [((k + i) % ca, (2 * k + i) % cb) for i in range(1 + k % 3)]


def probes_of(k):
    """five probes over the six streams, rotated from call to call: an anchor with a long needle of the largest shape, haystacks off
    either end, a stream against itself, more than one lag tile"""
    nm = lambda i: NAMES[(k + i) % 6]
    out = [("loud", 1024 + k, (8 - k % 3) * 1024 - 24, "mixed", 900, -40 - k, 97 + 10 * k, pairs_of("loud", "mixed", k))]
    for i, (fa, n, fb, lf, L) in enumerate([(5, 300, 0, -200, 257), (100, 77, 0, 0, 1), (0, 1000, 2000, -30, 300), (33, 1, 50, -3, 7)]):
        a, b = nm(i), nm(i + 1 + i % 2)
        fb = fb if i != 2 else num_samples(b) - 500                 # (the range ends behind the haystack)
        out.append((a, fa + k, n, b if i != 1 else a, fb, lf, L, pairs_of(a, b if i != 1 else a, k + i)))
    return out


def windows_of(k, same_channels=False):
    names = [n for n in NAMES if not same_channels or CHANNELS[n] == 2]
    return [(names[(k + i) % len(names)], 10 * i + k, 700 + 300 * i) for i in range(4)]


def scenario_between():
    """lags before and after every sibling"""
    steps = [lags(probes_of(0), note="the context's first call")]
    for k, call in enumerate(SIBLINGS, 1):
        steps.append(sibling(call, windows_of(2 * k, call == "overlay"), note="behind the lag call: its accumulators, samples or images where that call's images and partial sums lay"))
        steps.append(lags(probes_of(2 * k + 1), gf=k % 2, note=f"behind {call}: its images and partial sums where that call's accumulators or scratch lay"))
    return steps


def scenario_large_small_large():
    name = "mixed"
    N = num_samples(name)
    whole = [(name, 0, N, name, 0, -600, 1201, [(0, 0), (1, 1), (0, 1)])]
    small = [(name, 5000, 64, "loud", 5000, -2, 5, [(1, 0)])]
    steps = [lags(whole, note="grows the lists and the scratch: two whole-stream images and 15 tiles of partial sums"),
             lags(small, note="its images and partial sums begin inside the whole-stream call's images"),
             lags(whole, gf=1, note="many passes in one scratch, its images where the small call's lay"),
             lags(small, note="the same 64 samples again: the same answer"),
             sibling("measure", [(name, 0, N)], note="accumulators of a whole stream over the images"),
             lags(whole, note="and the whole stream as at first")]
    rng = np.random.default_rng(12)
    many = []
    for i in range(64):
        a, b = NAMES[i % 6], NAMES[(i * 5 + 1) % 6]
        fa = int(rng.integers(0, num_samples(a) - 900))
        many.append((a, fa, int(rng.integers(1, 900)), b, int(rng.integers(0, num_samples(b))), -int(rng.integers(0, 300)), int(rng.integers(1, 600)), pairs_of(a, b, i)))
    return steps + [lags(many, note="64 probes of every shape: long lists, tables of every probe"),
                    lags([(name, 70, 150, name, 0, 0, 3, [(0, 0)])], note="one probe: its images inside the 64 probes' images"),
                    sibling("overlay", windows_of(3, True), note="an overlay's images over the lag call's"),
                    lags(many[::-1], gf=2, note="the 64 probes in the other order")]
