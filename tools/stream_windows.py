"""Timing of Context.decode_windows (many sample windows of resident .lnn streams in one call) against the same windows as a loop
of Context.decode_stream calls and against one whole-stream decode.  Two cases, each 256 windows of 5 seconds at seeded random
offsets, decoded into one (256, 2, 220500) int32 tensor:
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS;
  (b) 64 streams of 3 minutes each of that shape (BASELINE configs[3]'s tracks), the windows spread over them.
The streams are encoded once on the device (Context.encode_stream) and stay resident with their indexes.  Every figure is the
median of --reps runs after a warm-up, each run ending in a device synchronise; the three figures of a case are taken in turn
within each repetition, and the runs' minimum and maximum are reported beside the median.  Prints one JSON line
(profiles/stream_windows.json holds the MI355X's)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import linne_amd
from bench import synth_track

ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=60.0)
ap.add_argument("--tracks", type=int, default=64)
ap.add_argument("--track-minutes", type=float, default=3.0)
ap.add_argument("--windows", type=int, default=256)
ap.add_argument("--window-seconds", type=float, default=5.0)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
nch, bits, rate, block, preset = 2, 16, 44100, 10240, 7
dev = torch.device("cuda", 0)
ctx = linne_amd.Context(0, use_torch_stream=True)
win = int(args.window_seconds * rate)
W = args.windows
KINDS = (56, 57, 28, 58, 32, 33, 34, 35, 36, 30, 31, 11, 12, 59)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def case(tracks, seed):
    """tracks: [(pcm on the device, stream on the device, index)] -> the case's figures"""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, len(tracks), size=W)
    firsts = [int(rng.integers(0, tracks[t][0].shape[1] - win)) for t in which]
    wins = [(tracks[t][1], tracks[t][2], a, win) for t, a in zip(which, firsts)]
    out = torch.empty((W, nch, win), dtype=torch.int32, device=dev)

    def batch():
        ctx.decode_windows(wins, out=out)

    def loop():
        for s, ix, a, n in wins:
            ctx.decode_stream(s, a, n, index=ix)

    def whole():
        ctx.decode_stream(tracks[0][1], index=tracks[0][2])

    out.fill_(-1)
    batch()
    exact_batch = all(torch.equal(out[i], tracks[t][0][:, a:a + win]) for i, (t, a) in enumerate(zip(which, firsts)))
    exact_loop = all(torch.equal(ctx.decode_stream(s, a, n, index=ix), out[i]) for i, (s, ix, a, n) in enumerate(wins))
    exact_whole = torch.equal(ctx.decode_stream(tracks[0][1], index=tracks[0][2]), tracks[0][0])
    loop(); whole()                                              # warm-up (batch() ran above)
    tb, tl, tw = [], [], []
    for _ in range(args.reps):
        tb.append(timed(batch)); tl.append(timed(loop)); tw.append(timed(whole))
    ctx.enable_timing(True)
    batch()
    kinds = {str(k): round(ctx.last_ms(k), 3) for k in KINDS if ctx.last_launches(k) > 0}
    launches = {str(k): ctx.last_launches(k) for k in KINDS if ctx.last_launches(k) > 0}
    call_ms = round(ctx.last_ms(0), 3)
    ctx.enable_timing(False)
    nblocks = sum(1 + (a + win - 1) // block - a // block for a in firsts)
    return {
        "streams": len(tracks), "windows": W, "window_samples": win, "blocks_in_the_batch": nblocks,
        "blocks_of_the_first_stream": tracks[0][2].num_blocks,
        "decode_windows": stats(tb), "loop_of_decode_stream": stats(tl), "decode_stream_whole_first_stream": stats(tw),
        "batch_over_whole": round(statistics.median(tb) / statistics.median(tw), 3),
        "loop_over_batch": round(statistics.median(tl) / statistics.median(tb), 2),
        "kernel_ms_one_batch": kinds, "launches_one_batch": launches, "device_ms_one_batch": call_ms,
        "exact": {"decode_windows": bool(exact_batch), "loop_equals_batch": bool(exact_loop), "whole": bool(exact_whole)},
    }


def make_tracks(count, minutes, seed0):
    tracks = []
    for t in range(count):
        x = synth_track(int(minutes * 60 * rate), nch, bits, seed0 + t, dev, rate=float(rate))
        s = ctx.encode_stream(x, bits, rate, block, preset, True).clone()
        tracks.append((x, s, ctx.index_stream(s)))
    return tracks


result = {"config": f"44.1 kHz int16 stereo, -m {preset}, block {block}, MS; {W} windows of {args.window_seconds:g} s", "reps": args.reps,
          "statistic": "median (min, max) ms of the runs, warm-up excluded, each run ends in a device synchronise; the figures of a case alternate within a repetition"}
one = make_tracks(1, args.minutes, 3)
result["one_stream"] = dict(case(one, 42), stream=f"{args.minutes:g} min (BASELINE configs[1])")
for _, _, ix in one:
    ix.close()
del one
many = make_tracks(args.tracks, args.track_minutes, 100)
result["many_streams"] = dict(case(many, 43), stream=f"{args.tracks} x {args.track_minutes:g} min (BASELINE configs[3]'s tracks)")
for _, _, ix in many:
    ix.close()
result["gate"] = {"rule": "one_stream: decode_windows median <= 1.25 x whole-stream decode_stream median",
                  "met": bool(result["one_stream"]["batch_over_whole"] <= 1.25)}
print(json.dumps(result))
ctx.close()
