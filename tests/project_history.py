"""The scenarios of tests/test_gpu_stream_project_history.py, as plain data in the form of tests/stream_history.py: does the answer of a
project_windows call depend on the calls the context served before it?  The windows calls share buffers of the context that grow and are
never cleared (the pinned lists, their device copy, the scratch with the images and the digit planes behind them), so a project call's
images, tables and planes land where another consumer's samples, accumulators, images or partial sums lay, and the other way round.  A
scenario is a list of steps that the GPU test runs in order on ONE context.  A step is a dict:

    {"call": "project" or a sibling ("measure", "quiet", "mix", "resample", "overlay", "lags"), "gf": group_frames, "note": the stale
     state the step is written to meet; project: "wins": [(stream name, first frame, frames)] and "spec": (basis number, hop, before,
     shift, clip_bits, float32, rows_first); lags: "probes" as lag_history has them; another sibling: "wins": [(stream name, first
     sample, samples)]}

The streams are stream_history's.  A project step's expected answer comes from project_refs on the oracle's decode, whatever ran before;
a sibling's step has to succeed -- its own history tests hold its answer.  The windows of one project call that share a channel count and
a frame count go into one call of the Python form; the step's calls follow each other on the one context."""
import numpy as np

from lag_history import CHANNELS, probes_of, windows_of
from stream_history import NAMES, num_samples

SIBLINGS = ["measure", "quiet", "mix", "resample", "overlay", "lags"]
SHAPES = [(64, 16), (65, 17), (512, 70), (1, 1), (300, 3), (20, 130)]       # (frame_len, rows) of basis 0 .. 5


def bases():
    """the scenarios' bases: random int16 with a row of 32767 and a row of -32768 where there is room"""
    rng = np.random.default_rng(21)
    out = []
    for N, K in SHAPES:
        b = rng.integers(-32768, 32768, (K, N)).astype(np.int16)
        if K >= 3:
            b[0], b[K - 1] = 32767, -32768
        out.append(b)
    return out


def frames(name, hop):
    return -(-num_samples(name) // hop)


def project(wins, spec, gf=0, note=""):
    return {"call": "project", "wins": list(wins), "spec": spec, "gf": gf, "note": note}


def sibling(call, wins, gf=0, note=""):
    return {"call": call, "wins": list(wins), "gf": gf, "note": note}


def spec_of(k):
    """rotated from call to call: every basis, hops below, at and above the frame, both formats and both stride orders"""
    b = k % len(SHAPES)
    N = SHAPES[b][0]
    hop = (1, 7, N, N + 5, 64, 3)[k % 6]
    return (b, hop, (0, N - 1, N // 2)[k % 3], (0, 15, 31)[k % 3], (0, 16, 24)[(k // 2) % 3], k % 4 == 1, k % 2 == 1)


def wins_of(k, hop):
    """six windows over the six streams: the first frames with their halo in front of sample 0, the last with theirs behind the stream, a
    tile of 64 frames and one more, one frame"""
    out = []
    for i in range(6):
        name = NAMES[(k + i) % 6]
        F = frames(name, hop)
        n = (1, 17, 65, 40, 16, 15)[(k + i) % 6]
        n = min(n, F)
        first = (0, F - n, (F - n) // 2)[i % 3]
        out.append((name, first, n))
    return out


def scenario_between():
    """project before and after every sibling"""
    s0 = spec_of(0)
    steps = [project(wins_of(0, s0[1]), s0, note="the context's first call")]
    for k, call in enumerate(SIBLINGS, 1):
        if call == "lags":
            steps.append({"call": "lags", "probes": probes_of(k), "gf": 0, "note": "behind the project call: its images and partial sums where that call's images and planes lay"})
        else:
            steps.append(sibling(call, windows_of(2 * k, call == "overlay"), note="behind the project call: its accumulators, samples or images where that call's images and planes lay"))
        s = spec_of(2 * k + 1)
        steps.append(project(wins_of(2 * k + 1, s[1]), s, gf=k % 2, note=f"behind {call}: its images and planes where that call's accumulators or scratch lay"))
    return steps


def scenario_large_small_large():
    name = "mixed"
    big = (2, 128, 256, 15, 0, False, True)                       # 512 samples, 70 rows, hop 128: the whole stream
    tiny = (3, 1, 0, 0, 0, False, False)
    whole = [(name, 0, frames(name, 128))]
    small = [(name, 5000, 64)]
    steps = [project(whole, big, note="grows the lists and the scratch: a whole-stream image and a table of 70 rows"),
             project(small, tiny, note="its image and planes begin inside the whole-stream call's image"),
             project(whole, big, gf=1, note="many passes in one scratch, its image where the small call's lay"),
             project(small, tiny, note="the same 64 frames again: the same answer"),
             sibling("measure", [(name, 0, num_samples(name))], note="accumulators of a whole stream over the image and the planes"),
             project(whole, big, note="and the whole stream as at first")]
    many = []
    rng = np.random.default_rng(12)
    s = (1, 9, 30, 12, 24, True, False)
    for i in range(64):
        a = NAMES[i % 6]
        F = frames(a, 9)
        n = (5, 33)[i % 2]
        many.append((a, int(rng.integers(0, F - n)), n))
    return steps + [project(many, s, note="64 windows of every shape: long lists, one shared table"),
                    project([(name, 70, 3)], spec_of(5), note="one window: its image inside the 64 windows' images"),
                    sibling("overlay", windows_of(3, True), note="an overlay's images over the project call's"),
                    project(many[::-1], s, gf=2, note="the 64 windows in the other order")]
