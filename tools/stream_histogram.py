"""Timing and memory of Context.histogram_streams (the sample levels of resident .lnn streams counted per channel, bucket and bin,
nothing decoded into memory) against the composition a user had before the call existed: index_streams + decode_windows (int32 planar)
over the whole streams + torch (abs, shift, clamp -- or the bit length --, bincount per channel and bucket).  Two workloads, each with
two settings -- 1024 linear bins at shift 5 in one bucket, and 33 log2 bins in buckets of 441 samples:
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS;
  (b) 256 clips of 5 seconds of that shape, in one call.
One-bin material beside them: a 60-minute track of one constant value, and the 60-minute music with two log2 bins; there kind 92 is set
against kind 92 on the music with 1024 linear bins.  The streams are encoded once on the device and stay resident.  Both forms run on
this build -- the decode path is the parent commit's, launch for launch, which the suite holds.  Every figure is the median of --reps
runs after a warm-up, each run ending in a device synchronise, the forms of a case taken in turn within a repetition; minimum and
maximum beside the median, spread = max - min.  Peak device memory of a call = torch's peak allocation during it plus what the context's
scratch grew by (free device memory before and after, on a fresh context, less what torch's allocator reserved).  Kinds 92, 59 and 80 are
HIP events around k_wx_histogram, k_wx_place and k_wx_measure in a histogram_windows, a decode_windows and a measure_windows call over
the same windows (one pass each); kinds 93 and 94 are the histogram call's preset and commit.  The library is measured as it is built:
to see k_wx_histogram without the addition inside a wave, build with -DWXH_SHARE=65 (no wave has 65 lanes) and run this again with
--label.  Prints one JSON line (profiles/stream_histogram.json holds the MI355X's)."""
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
ap.add_argument("--label", default="as built (WXH_SHARE 8)")
args = ap.parse_args()
nch, bits, rate, block, preset = 2, 16, 44100, 10240, 7
dev = torch.device("cuda", 0)
SETTINGS = {"linear_1024_one_bucket": (1024, 5, False, 0), "log2_33_buckets_of_441": (33, 0, True, 441)}


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


def torch_histogram(pcm, bins, shift, log2, b):
    """the composition's table of one stream: (C, nb, bins) int64"""
    C, n = pcm.shape
    m = pcm.to(torch.int64).abs() >> shift
    x = torch.where(m > 0, torch.floor(torch.log2(m.double())).long() + 1, torch.zeros_like(m)) if log2 else m
    x = x.clamp(max=bins - 1)
    step = b if b else n
    nb = -(-n // step)
    x = x + (torch.arange(n, device=pcm.device) // step * bins)[None, :]
    return torch.stack([torch.bincount(x[ch], minlength=nb * bins).view(nb, bins) for ch in range(C)])


def kinds(ctx, wins, spec, reps):
    """kind 92 (and 93, 94) of a histogram call over wins, one pass"""
    bins, shift, log2, b = spec
    out = {}
    for _ in range(reps + 1):
        ctx.histogram_windows(wins, bins, shift, log2, b)
        assert ctx.last_launches(92) == 1 and ctx.last_launches(59) == 0 and ctx.last_launches(93) == 1 and ctx.last_launches(94) == 1
        for k, name in ((92, "kind_92_k_wx_histogram"), (93, "kind_93_preset"), (94, "kind_94_commit"), (0, "histogram_windows_device_ms")):
            out.setdefault(name, []).append(ctx.last_ms(k))
    return {k: stats(v[1:]) for k, v in out.items()}


def case(streams, spec):
    bins, shift, log2, b = spec

    def new(c):
        return c.histogram_streams(streams, bins, shift, log2, b)

    def recipe(c):
        idx = c.index_streams(streams)
        got = c.decode_windows([(s, x, 0, None) for s, x in zip(streams, idx)])
        out = [torch_histogram(g, bins, shift, log2, b) for g in got]
        for x in idx:
            x.close()
        return out

    forms = {"histogram_streams": new, "recipe": recipe}
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
    out = {"streams": len(streams), "num_bins": bins, "shift": shift, "log2": log2, "bucket_samples": b}
    out["answers_equal"] = all(torch.equal(h.counts, r) for h, r in zip(answers["histogram_streams"], answers["recipe"]))
    out["peak_memory"] = peaks
    del answers
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
    wins = [(s, x, 0, None) for s, x in zip(streams, idx)]
    ctx.enable_timing(True)
    out.update(kinds(ctx, wins, spec, args.reps))
    k59, k80 = [], []
    for _ in range(args.reps + 1):
        ctx.decode_windows(wins)
        assert ctx.last_launches(59) == 1 and ctx.last_launches(92) == 0
        k59.append(ctx.last_ms(59))
        ctx.measure_windows(wins, bucket_samples=b)
        assert ctx.last_launches(80) == 1
        k80.append(ctx.last_ms(80))
    ctx.enable_timing(False)
    out["kind_59_k_wx_place"], out["kind_80_k_wx_measure"] = stats(k59[1:]), stats(k80[1:])
    for x in idx:
        x.close()
    ctx.close()
    slack = max(out["histogram_streams"]["spread_ms"], out["recipe"]["spread_ms"])
    k92, k59m, k80m = out["kind_92_k_wx_histogram"]["median_ms"], out["kind_59_k_wx_place"]["median_ms"], out["kind_80_k_wx_measure"]["median_ms"]
    out["criteria"] = {
        "faster_than_the_composition_beyond_the_spread": verdict(out["histogram_streams"]["median_ms"] + slack < out["recipe"]["median_ms"],
                                                                 f"histogram_streams {out['histogram_streams']['median_ms']} ms against the composition's {out['recipe']['median_ms']} ms (spread {slack} ms)"),
        "peak_memory_below_the_composition": verdict(peaks["histogram_streams"]["peak_bytes"] < peaks["recipe"]["peak_bytes"],
                                                     f"{peaks['histogram_streams']['peak_bytes']} bytes against {peaks['recipe']['peak_bytes']}; the decoded PCM is {out['decoded_pcm_bytes']}"),
        "kind_92_between_place_and_measure_(a_guess,_not_a_criterion)": f"k_wx_place {k59m} ms, k_wx_histogram {k92} ms, k_wx_measure {k80m} ms",
    }
    return out


def one_bin(streams, spec, music_k92):
    ctx = linne_amd.Context(0, use_torch_stream=True)
    idx = ctx.index_streams(streams)
    wins = [(s, x, 0, None) for s, x in zip(streams, idx)]
    h = ctx.histogram_windows(wins, *spec)[0].counts
    ctx.enable_timing(True)
    out = kinds(ctx, wins, spec, args.reps)
    ctx.enable_timing(False)
    out["bins_in_use"] = int((h > 0).sum())
    out["largest_share_of_one_bin"] = round(float(h.max(dim=2).values.sum() / h.sum()), 6)
    for x in idx:
        x.close()
    ctx.close()
    k, slack = out["kind_92_k_wx_histogram"], max(out["kind_92_k_wx_histogram"]["spread_ms"], music_k92["spread_ms"])
    out["criterion_no_slower_than_on_music_beyond_the_spread"] = verdict(k["median_ms"] <= music_k92["median_ms"] + slack,
                                                                        f"kind 92 {k['median_ms']} ms against {music_k92['median_ms']} ms on the music with 1024 linear bins (spread {slack} ms)")
    return out


result = {"config": f"44.1 kHz int16 stereo, -m {preset}, block {block}, MS", "reps": args.reps, "library": args.label,
          "statistic": "median (min, max, spread = max - min) ms of the runs, warm-up excluded, each run ends in a device synchronise; the forms of a case alternate within a repetition",
          "recipe_library": "this build: its decode path is the parent commit's, launch for launch"}
enc = linne_amd.Context(0, use_torch_stream=True)
ns = int(args.minutes * 60 * rate)
x = synth_track(ns, nch, bits, 3, dev, rate=float(rate))
s = enc.encode_stream(x, bits, rate, block, preset, True).clone()
del x
result["one_stream"] = {"stream": f"{args.minutes:g} min (BASELINE configs[1])"}
result["one_stream"].update({name: case([s], spec) for name, spec in SETTINGS.items()})
music_k92 = result["one_stream"]["linear_1024_one_bucket"]["kind_92_k_wx_histogram"]
flat = enc.encode_stream(torch.full((nch, ns), 1000, dtype=torch.int32, device=dev), bits, rate, block, preset, True).clone()
result["one_bin"] = {"constant_track_linear_1024": one_bin([flat], (1024, 0, False, 0), music_k92),
                     "music_log2_2_bins": one_bin([s], (2, 0, True, 0), music_k92)}
del s, flat
n = int(args.clip_seconds * rate)
clips = [synth_track(n, nch, bits, 100 + t, dev, rate=float(rate)) for t in range(args.clips)]
streams = [t.clone() for t in enc.encode_streams([(p, bits, rate, block, preset, True) for p in clips])]
del clips
enc.close()
result["clips"] = {"stream": f"{args.clips} x {args.clip_seconds:g} s"}
result["clips"].update({name: case(streams, spec) for name, spec in SETTINGS.items()})
print(json.dumps(result))
