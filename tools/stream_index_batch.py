"""Timing of the many-streams index call (Context.index_streams) against a loop of single calls (Context.index_stream) over the same
device bytes, on one context: streams of 44.1 kHz, 16 bit, stereo, -m 7, MS, block 10240, encoded by Context.encode_streams from
windows of one synthetic 60-minute signal.  Three sets, the shapes of tools/stream_batch_encode.py:
  a  256 five-second clips of 256 different lengths      b  64 three-minute tracks, each with its own tail      c  one 60-minute track
Per set: median of --reps runs after a warm-up, minimum, maximum and the run-to-run spread (max - min) beside it, each run ending in
a device synchronise; the timed region builds the indexes, closing them happens outside it (and is timed separately: every index
of either call is a part of its call's two allocations, which the last index of the call frees).  Records LINNEAmd_GetLastIndexBatchCount, the batch call's kernel times by kind,
whether every batch index equals its single-call index, and the criterion: for a and b the batch median lies below the loop's by
more than the larger spread; for c the batch is no slower than the single call beyond that spread.  Prints one JSON line
(profiles/stream_index_batch.json holds the MI355X's)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import linne_amd
from bench import synth_track

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="a,b,c")
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
nch, bits, rate, block, preset, ms = 2, 16, 44100, 10240, 7, True
total = 60 * 60 * rate
base = synth_track(total, nch, bits, 3, torch.device("cuda", 0), rate=float(rate)).to(torch.int32).contiguous()
ctx = linne_amd.Context(0, use_torch_stream=True)
KINDS = tuple(range(37, 45)) + (69, 70)


def stats_ms(build, reps):
    """build() -> the indexes; they are closed behind the timed region"""
    def close(ixs):
        t0 = time.perf_counter()
        for ix in ixs:
            ix.close()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    close(build())                                            # warm-up
    ts, cs = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ixs = build()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        cs.append(close(ixs))
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
            "spread_ms": round(max(ts) - min(ts), 3), "close_median_ms": round(statistics.median(cs), 3)}


def facts(ix):
    return (ix.header, ix.num_blocks, [a.tolist() for a in ix.blocks()], ix.failure())


def windows(lengths):
    """tracks of these lengths cut from the base signal, spread over it"""
    step = max((total - max(lengths)) // max(len(lengths), 1), 0)
    return [base[:, i * step:i * step + n] for i, n in enumerate(lengths)]


SETS = {
    "a": ("256 five-second clips, 256 different lengths", [5 * rate + 13 * i for i in range(256)]),
    "b": ("64 three-minute tracks, each with its own tail", [180 * rate + 977 * i for i in range(64)]),
    "c": ("one 60-minute track", [total]),
}
result = {"config": "44.1 kHz int16 stereo, -m 7, block 10240, MS, streams resident", "reps": args.reps,
          "statistic": "median / min / max / spread (max - min) ms over the runs, warm-up excluded, each run ends in a device synchronise; closing the indexes is outside the timed region (close_median_ms)",
          "sets": {}}
for key in args.sets.split(","):
    what, lengths = SETS[key]
    streams = ctx.encode_streams([(x, bits, rate, block, preset, ms) for x in windows(lengths)])
    rec = {"what": what, "streams": len(streams), "stream_bytes": int(sum(s.numel() for s in streams))}
    batch = ctx.index_streams(streams)
    rec["index_batch_count"] = {name: ctx.last_index_batch_count(w) for w, name in enumerate(("streams", "indexes", "K", "host_synchronisations", "device_allocations"))}
    single = [ctx.index_stream(s) for s in streams]
    rec["blocks"] = int(sum(ix.num_blocks for ix in batch))
    rec["every_batch_index_equals_its_single_call_index"] = all(facts(b) == facts(s) for b, s in zip(batch, single))
    for ix in batch + single:
        ix.close()
    rec["batch_call"] = stats_ms(lambda: ctx.index_streams(streams), args.reps)
    rec["loop_of_single_calls"] = stats_ms(lambda: [ctx.index_stream(s) for s in streams], args.reps)
    b, l = rec["batch_call"], rec["loop_of_single_calls"]
    spread = max(b["spread_ms"], l["spread_ms"])
    rec["loop_over_batch"] = round(l["median_ms"] / b["median_ms"], 2)
    if len(streams) > 1:
        rec["criterion"] = "batch median below the loop's by more than the larger spread: " + ("MET" if l["median_ms"] - b["median_ms"] > spread else "MISSED")
    else:
        rec["criterion"] = "batch no slower than the single call beyond the larger spread: " + ("MET" if b["median_ms"] - l["median_ms"] <= spread else "MISSED")
    ctx.enable_timing(True)
    for ix in ctx.index_streams(streams):
        ix.close()
    rec["kernel_ms_batch_call"] = {str(k): round(ctx.last_ms(k), 3) for k in KINDS if ctx.last_launches(k) > 0}
    rec["kernel_launches_batch_call"] = {str(k): ctx.last_launches(k) for k in KINDS if ctx.last_launches(k) > 0}
    ctx.enable_timing(False)
    del streams
    result["sets"][key] = rec
    print(f"set {key}: batch {b['median_ms']} ms, loop {l['median_ms']} ms", file=sys.stderr, flush=True)
print(json.dumps(result))
ctx.close()
