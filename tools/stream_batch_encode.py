"""Timing of the many-tracks stream encoder (Context.encode_streams) against a loop of single calls (Context.encode_stream) on the
same context, PCM resident in HBM as planar int32: 44.1 kHz, 16 bit, stereo, -m 7, MS, block 10240.  Three sets, all windows of one
synthetic 60-minute signal:
  a  256 five-second clips of 256 different lengths      b  64 three-minute tracks, each with its own tail      c  one 60-minute track
Per set: the batch call; the loop of encode_stream calls (the baseline); for a and b, encode_stream of ONE stream holding the same
number of frames (the floor: what the analysis and the writers cost without any track boundary).  Median of --reps runs after a
warm-up, minimum and maximum beside it, each run ending in a device synchronise.  Records the passes and analysis calls of the batch
call, its kernel times by kind, and whether every batch stream equals its single-call stream.  Prints one JSON line
(profiles/stream_batch_encode.json holds the MI355X's)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import linne_amd
from bench import synth_track

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="a,b,c")
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
nch, bits, rate, block, preset, ms = 2, 16, 44100, 10240, 7, True
total = 60 * 60 * rate
base = synth_track(total, nch, bits, 3, torch.device("cuda", 0), rate=float(rate)).to(torch.int32).contiguous()
ctx = linne_amd.Context(0, use_torch_stream=True)
KINDS = (17, 21, 49, 51) + tuple(range(60, 69))


def stats_ms(fn, reps):
    fn()                                                      # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def windows(lengths):
    """tracks of these lengths cut from the base signal, spread over it"""
    step = max((total - max(lengths)) // max(len(lengths), 1), 0)
    return [base[:, i * step:i * step + n] for i, n in enumerate(lengths)]


SETS = {
    "a": ("256 five-second clips, 256 different lengths", [5 * rate + 13 * i for i in range(256)]),
    "b": ("64 three-minute tracks, each with its own tail", [180 * rate + 977 * i for i in range(64)]),
    "c": ("one 60-minute track", [total]),
}
result = {"config": "44.1 kHz int16 stereo, -m 7, block 10240, MS, PCM resident", "reps": args.reps,
          "statistic": "median / min / max ms over the runs, warm-up excluded, each run ends in a device synchronise", "sets": {}}
for key in args.sets.split(","):
    what, lengths = SETS[key]
    xs = windows(lengths)
    tracks = [(x, bits, rate, block, preset, ms) for x in xs]
    frames = sum((n + block - 1) // block for n in lengths)
    rec = {"what": what, "tracks": len(xs), "frames": frames, "distinct_frame_lengths": len({block} | {n % block for n in lengths if n % block})}
    batch = ctx.encode_streams(tracks)
    rec["passes"], rec["analysis_calls"] = ctx.last_stream_batch_count(1), ctx.last_stream_batch_count(2)
    single = [ctx.encode_stream(*t) for t in tracks]
    rec["every_batch_stream_equals_its_single_call_stream"] = all(bool(torch.equal(b, s)) for b, s in zip(batch, single))
    rec["stream_bytes"] = int(sum(b.numel() for b in batch))
    del batch, single
    rec["batch_call"] = stats_ms(lambda: ctx.encode_streams(tracks), args.reps)
    rec["loop_of_single_calls"] = stats_ms(lambda: [ctx.encode_stream(*t) for t in tracks], args.reps)
    if len(xs) > 1:
        one = base.repeat(1, -(-frames * block // total))[:, :frames * block].contiguous()      # (the base signal over again where it is too short)
        rec["one_stream_of_as_many_frames"] = stats_ms(lambda: ctx.encode_stream(one, bits, rate, block, preset, ms), args.reps)
    rec["loop_over_batch"] = round(rec["loop_of_single_calls"]["median_ms"] / rec["batch_call"]["median_ms"], 2)
    ctx.enable_timing(True)
    ctx.encode_streams(tracks)
    rec["kernel_ms_batch_call"] = {str(k): round(ctx.last_ms(k), 3) for k in KINDS if ctx.last_launches(k) > 0}
    rec["kernel_launches_batch_call"] = {str(k): ctx.last_launches(k) for k in KINDS if ctx.last_launches(k) > 0}
    ctx.enable_timing(False)
    if len(xs) > 1:
        del one
    result["sets"][key] = rec
print(json.dumps(result))
ctx.close()
