"""Timing of the repair call (Context.repair_streams) on resident streams of 44.1 kHz, 16 bit, stereo, -m 7, MS, block 10240, encoded
by Context.encode_streams from one synthetic 60-minute signal (the shapes of tools/stream_index_batch.py):
  long   the 60-minute stream with 0, 1 and 64 damaged blocks (one payload byte flipped in each), beside Context.index_stream of the
         same bytes plus a device-to-device copy of them, timed in the same session: an intact stream costs the index's CRC work
         once more over the candidates outside the chain, and a copy of every byte, so the question is how far above index + copy the
         repair lies.  The repair's kernel times by kind show what the size bound B leaves k_rp_sound to do.
  clips  256 five-second clips, 16 of them damaged: one call against 256 single-stream calls; the criterion is the batch index's --
         the one call's median below the loop's by more than the larger spread.
Per measurement: median of --reps runs after a warm-up, minimum, maximum and the run-to-run spread (max - min), each run ending in a
device synchronise.  Prints one JSON line (profiles/stream_repair.json holds the MI355X's)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import linne_amd
from bench import synth_track

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="long,clips")
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
nch, bits, rate, block, preset, ms = 2, 16, 44100, 10240, 7, True
total = 60 * 60 * rate
base = synth_track(total, nch, bits, 3, torch.device("cuda", 0), rate=float(rate)).to(torch.int32).contiguous()
ctx = linne_amd.Context(0, use_torch_stream=True)
KINDS = (37, 38, 39, 41, 43, 69, 71) + tuple(range(73, 79))
COUNTS = ("outputs", "kept_blocks", "fill_blocks", "gaps", "copy_runs", "host_synchronisations", "kernel_launches")


def stats_ms(run, reps):
    run()                                                     # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = run()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del keep
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "spread_ms": round(max(ts) - min(ts), 3)}


def damaged(stream, which):
    """a copy of the stream with one payload byte flipped in each of the blocks `which`"""
    ix = ctx.index_stream(stream)
    off, _, size, _, _ = ix.blocks()
    ix.close()
    out = stream.clone()
    for r in which:
        out[int(off[r]) + 11 + (int(size[r]) - 5) // 2] ^= 0x10
    return out


def index_only(s):
    ctx.index_stream(s).close()


result = {"config": "44.1 kHz int16 stereo, -m 7, block 10240, MS, streams resident", "reps": args.reps,
          "statistic": "median / min / max / spread (max - min) ms over the runs, warm-up excluded, each run ends in a device synchronise", "sets": {}}
sets = args.sets.split(",")
if "long" in sets:
    stream = ctx.encode_streams([(base, bits, rate, block, preset, ms)])[0]
    nb = -(-total // block)
    rec = {"what": "one 60-minute stream", "stream_bytes": int(stream.numel()), "blocks": nb}
    dst = torch.empty_like(stream)
    rec["index_stream"] = stats_ms(lambda: index_only(stream), args.reps)
    rec["device_to_device_copy"] = stats_ms(lambda: dst.copy_(stream), args.reps)
    floor = rec["index_stream"]["median_ms"] + rec["device_to_device_copy"]["median_ms"]
    for ndam in (0, 1, 64):
        s = damaged(stream, [40 + (i * (nb - 80)) // max(ndam, 1) for i in range(ndam)])
        one = stats_ms(lambda: ctx.repair_streams([s]), args.reps)
        one["counts"] = {name: ctx.last_repair_count(w) for w, name in enumerate(COUNTS)}
        one["over_index_plus_copy"] = round(one["median_ms"] / floor, 2)
        ctx.enable_timing(True)
        ctx.repair_streams([s])
        one["kernel_ms"] = {str(k): round(ctx.last_ms(k), 3) for k in KINDS if ctx.last_launches(k) > 0}
        one["kernel_launches"] = {str(k): ctx.last_launches(k) for k in KINDS if ctx.last_launches(k) > 0}
        ctx.enable_timing(False)
        rec[f"repair_{ndam}_damaged_blocks"] = one
        del s
    del stream, dst
    result["sets"]["long"] = rec
    print(f"long: index + copy {round(floor, 3)} ms, repair {[rec[f'repair_{n}_damaged_blocks']['median_ms'] for n in (0, 1, 64)]} ms", file=sys.stderr, flush=True)
if "clips" in sets:
    lengths = [5 * rate + 13 * i for i in range(256)]
    step = (total - max(lengths)) // len(lengths)
    streams = ctx.encode_streams([(base[:, i * step:i * step + n], bits, rate, block, preset, ms) for i, n in enumerate(lengths)])
    streams = [damaged(s, [7]) if i % 16 == 5 else s for i, s in enumerate(streams)]
    rec = {"what": "256 five-second clips, 16 of them with a damaged block", "streams": len(streams), "stream_bytes": int(sum(s.numel() for s in streams))}
    batch = ctx.repair_streams(streams)
    rec["counts"] = {name: ctx.last_repair_count(w) for w, name in enumerate(COUNTS)}
    single = [ctx.repair_streams([s])[0] for s in streams]
    rec["every_output_equals_its_single_call_output"] = all(torch.equal(b[0], s[0]) and b[1] == s[1] for b, s in zip(batch, single))
    del batch, single
    rec["one_call"] = stats_ms(lambda: ctx.repair_streams(streams), args.reps)
    rec["loop_of_single_calls"] = stats_ms(lambda: [ctx.repair_streams([s]) for s in streams], args.reps)
    b, l = rec["one_call"], rec["loop_of_single_calls"]
    rec["loop_over_one_call"] = round(l["median_ms"] / b["median_ms"], 2)
    rec["criterion"] = "one call's median below the loop's by more than the larger spread: " + ("MET" if l["median_ms"] - b["median_ms"] > max(b["spread_ms"], l["spread_ms"]) else "MISSED")
    result["sets"]["clips"] = rec
    print(f"clips: one call {b['median_ms']} ms, loop {l['median_ms']} ms", file=sys.stderr, flush=True)
print(json.dumps(result))
ctx.close()
