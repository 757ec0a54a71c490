"""Timing and memory of Context.quiet_streams (the quiet runs of resident .lnn streams, nothing decoded into memory) against the
composition a user had before the call existed: index_streams + decode_windows (int32 planar) over the whole streams + torch
(abs() <= threshold, all over the channels, run extraction with diff and nonzero).  Two workloads, each with two settings --
threshold 0 / min_samples 1 (digital silence, every run) and 16 / 4410 (a musical setting: a tenth of a second within +-16):
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS;
  (b) 256 clips of 5 seconds of that shape, in one call.
Stretches of digital silence and of low-level noise (within +-8) are written into the PCM before it is encoded; `planted` records how
many and how long.  The streams are encoded once on the device and stay resident.  Both forms run on this build -- the decode path is
the parent commit's, launch for launch, which the suite holds.  Every figure is the median of --reps runs after a warm-up, each run
ending in a device synchronise, the forms of a case taken in turn within a repetition; minimum and maximum beside the median, spread
= max - min.  Peak device memory of a call = torch's peak allocation during it plus what the context's scratch grew by (free device
memory before and after, on a fresh context, less what torch's allocator reserved).  Kinds 86, 59 and 79 are HIP events around
k_wx_quiet, k_wx_place and k_wx_compare in a quiet_windows, a decode_windows and a compare_windows call over the same windows (one
pass each); kinds 87 to 91 are the quiet call's preset and commit stage, in a call whose tables hold every run.  quiet_streams itself is
timed as a user calls it, without a capacity: the streams of more runs than the default are asked once more.  Prints one JSON line (profiles/stream_quiet.json holds the
MI355X's)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import linne_amd
from bench import synth_track

ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=60.0)
ap.add_argument("--clips", type=int, default=256)
ap.add_argument("--clip-seconds", type=float, default=5.0)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
nch, bits, rate, block, preset = 2, 16, 44100, 10240, 7
dev = torch.device("cuda", 0)
SETTINGS = {"threshold_0_min_1": (0, 1), "threshold_16_min_4410": (16, 4410)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "spread_ms": round(max(ts) - min(ts), 3)}


def verdict(ok, text):
    return ("met: " if ok else "MISSED: ") + text


def plant(x, seed, every, lengths):
    """stretches of digital silence and of noise within +-8, alternately, every `every` samples, of the lengths given in turn ->
    what was planted"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n, done = x.shape[1], {"silence": [], "noise": []}
    for k, at in enumerate(range(every // 2, n, every)):
        m = min(lengths[k % len(lengths)], n - at)
        if k % 2 == 0:
            x[:, at:at + m] = 0
            done["silence"].append(m)
        else:
            x[:, at:at + m] = torch.randint(-8, 9, (x.shape[0], m), generator=g, dtype=torch.int32).to(x.device)
            done["noise"].append(m)
    return {kind: {"stretches": len(v), "samples": int(sum(v)), "shortest": min(v, default=0), "longest": max(v, default=0)} for kind, v in done.items()}


def torch_runs(pcm, thr, mn):
    """the composition's table of one stream: (k, 2) int64 of (first, length)"""
    q = (pcm.abs() <= thr).all(dim=0).to(torch.int8)
    zero = torch.zeros(1, dtype=torch.int8, device=pcm.device)
    edge = torch.diff(q, prepend=zero, append=zero)
    starts, ends = (edge == 1).nonzero().squeeze(1), (edge == -1).nonzero().squeeze(1)
    keep = (ends - starts) >= mn
    return torch.stack([starts[keep], (ends - starts)[keep]], dim=1)


def case(streams, thr, mn):
    def new(c):
        return c.quiet_streams(streams, thr, min_samples=mn)        # (capacity None: a second call for the streams of more runs than the default)

    def recipe(c):
        idx = c.index_streams(streams)
        got = c.decode_windows([(s, x, 0, None) for s, x in zip(streams, idx)])
        out = [torch_runs(g, thr, mn) for g in got]
        for x in idx:
            x.close()
        return out

    forms = {"quiet_streams": new, "recipe": recipe}
    answers, peaks = {}, {}
    for name, fn in forms.items():
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        c = linne_amd.Context(0, use_torch_stream=True)
        free0, res0, alloc0 = torch.cuda.mem_get_info(dev)[0], torch.cuda.memory_reserved(dev), torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        answers[name] = fn(c)
        torch.cuda.synchronize()
        torch_peak = torch.cuda.max_memory_allocated(dev) - alloc0
        scratch = (free0 - torch.cuda.mem_get_info(dev)[0]) - (torch.cuda.memory_reserved(dev) - res0)
        peaks[name] = {"torch_peak_bytes": int(torch_peak), "context_scratch_bytes": int(max(scratch, 0)), "peak_bytes": int(torch_peak + max(scratch, 0))}
        c.close()
    out = {"streams": len(streams), "threshold": thr, "min_samples": mn, "runs": int(sum(q.num_runs for q in answers["quiet_streams"])),
           "quiet_samples": int(sum(q.quiet_samples for q in answers["quiet_streams"])), "most_runs_in_a_stream": int(max(q.num_runs for q in answers["quiet_streams"]))}
    out["answers_equal"] = all(q.num_runs == r.shape[0] and torch.equal(q.runs, r) for q, r in zip(answers["quiet_streams"], answers["recipe"]))
    out["peak_memory"] = peaks
    ctx = linne_amd.Context(0, use_torch_stream=True)
    idx = ctx.index_streams(streams)
    out["decoded_pcm_bytes"] = sum(4 * x.header["num_channels"] * x.header["num_samples"] for x in idx)
    for fn in forms.values():
        fn(ctx)
    ts = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, fn in forms.items():
            ts[name].append(timed(lambda: fn(ctx)))
    for name in forms:
        out[name] = stats(ts[name])
    # kinds 86, 59 and 79 over the same windows, one pass each; the quiet call's preset and commit stage
    wins = [(s, x, 0, None) for s, x in zip(streams, idx)]
    pcms = ctx.decode_windows(wins)
    ctx.enable_timing(True)
    k86, k59, k79, calls = [], [], [], {}
    for _ in range(args.reps + 1):
        ctx.quiet_windows(wins, thr, mn, capacity=max(out["most_runs_in_a_stream"], 1))    # one call in which every run fits
        assert ctx.last_launches(86) == 1 and ctx.last_launches(59) == 0 and all(ctx.last_launches(k) == 1 for k in (87, 88, 89, 90, 91))
        k86.append(ctx.last_ms(86)); calls.setdefault("quiet_windows_device_ms", []).append(ctx.last_ms(0))
        calls.setdefault("kind_87_preset", []).append(ctx.last_ms(87))
        for k, name in ((88, "count"), (89, "scan"), (90, "starts"), (91, "ends")):
            calls.setdefault(f"kind_{k}_{name}", []).append(ctx.last_ms(k))
        calls.setdefault("commit_stage_kinds_88_to_91", []).append(sum(ctx.last_ms(k) for k in (88, 89, 90, 91)))
        ctx.decode_windows(wins)
        assert ctx.last_launches(59) == 1 and ctx.last_launches(86) == 0
        k59.append(ctx.last_ms(59)); calls.setdefault("decode_windows_device_ms", []).append(ctx.last_ms(0))
        ctx.compare_windows([w + (p,) for w, p in zip(wins, pcms)])
        assert ctx.last_launches(79) == 1
        k79.append(ctx.last_ms(79))
    ctx.enable_timing(False)
    out["kind_86_k_wx_quiet"], out["kind_59_k_wx_place"], out["kind_79_k_wx_compare"] = stats(k86[1:]), stats(k59[1:]), stats(k79[1:])
    out.update({k: stats(v[1:]) for k, v in calls.items()})
    del pcms
    for x in idx:
        x.close()
    ctx.close()
    slack = max(out["quiet_streams"]["spread_ms"], out["recipe"]["spread_ms"])
    out["criteria"] = {
        "faster_than_the_composition_beyond_the_spread": verdict(out["quiet_streams"]["median_ms"] + slack < out["recipe"]["median_ms"],
                                                                 f"quiet_streams {out['quiet_streams']['median_ms']} ms against the composition's {out['recipe']['median_ms']} ms (spread {slack} ms)"),
        "peak_memory_below_the_composition": verdict(peaks["quiet_streams"]["peak_bytes"] < peaks["recipe"]["peak_bytes"],
                                                     f"{peaks['quiet_streams']['peak_bytes']} bytes against {peaks['recipe']['peak_bytes']}; the decoded PCM is {out['decoded_pcm_bytes']}"),
    }
    return out


result = {"config": f"44.1 kHz int16 stereo, -m {preset}, block {block}, MS", "reps": args.reps,
          "statistic": "median (min, max, spread = max - min) ms of the runs, warm-up excluded, each run ends in a device synchronise; the forms of a case alternate within a repetition",
          "recipe_library": "this build: its decode path is the parent commit's, launch for launch"}
enc = linne_amd.Context(0, use_torch_stream=True)
x = synth_track(int(args.minutes * 60 * rate), nch, bits, 3, dev, rate=float(rate))
planted = plant(x, 1, 20 * rate, [2 * rate, 300, 5 * rate, 4410, 64, rate // 2])
s = enc.encode_stream(x, bits, rate, block, preset, True).clone()
del x
result["one_stream"] = {"stream": f"{args.minutes:g} min (BASELINE configs[1])", "planted": planted}
result["one_stream"].update({name: case([s], thr, mn) for name, (thr, mn) in SETTINGS.items()})
del s
n = int(args.clip_seconds * rate)
clips = [synth_track(n, nch, bits, 100 + t, dev, rate=float(rate)) for t in range(args.clips)]
planted = [plant(p, 100 + t, rate, [rate // 4, 4410, 100, rate // 2]) for t, p in enumerate(clips)]
streams = [t.clone() for t in enc.encode_streams([(p, bits, rate, block, preset, True) for p in clips])]
del clips
enc.close()
result["clips"] = {"stream": f"{args.clips} x {args.clip_seconds:g} s",
                   "planted": {kind: {"stretches": sum(p[kind]["stretches"] for p in planted), "samples": sum(p[kind]["samples"] for p in planted)} for kind in ("silence", "noise")}}
result["clips"].update({name: case(streams, thr, mn) for name, (thr, mn) in SETTINGS.items()})
print(json.dumps(result))
