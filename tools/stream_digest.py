"""Timing and memory of Context.digest_streams (the CRC-32 of the decoded PCM of resident .lnn streams per bucket, nothing decoded into
memory) against what a user did before the call existed: index_streams + decode_windows into the WAV layout (dtype=int16,
channels_last=True) over the whole streams + a .cpu() copy + zlib.crc32 of every bucket's bytes on the host.  Two cases, each with
bucket_samples 0 (one bucket per stream) and 441 (10 ms):
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS;
  (b) 256 clips of 5 seconds of that shape, in one call.
The streams are encoded once on the device and stay resident.  Both forms run on this build -- the decode path is the parent
commit's, launch for launch, which the suite holds.  Every figure is the median of --reps runs after a warm-up, each run ending in a
device synchronise, the forms of a case taken in turn within a repetition; minimum and maximum beside the median, spread = max -
min.  Peak device memory of a call = torch's peak allocation during it plus what the context's scratch grew by (free device memory
before and after, on a fresh context, less what torch's allocator reserved).  Kinds 83, 59, 79 and 80 are HIP events around
k_wx_digest, k_wx_place, k_wx_compare and k_wx_measure in a digest_windows, a decode_windows, a compare_windows and a measure_windows
call over the same windows (one pass each).  Prints one JSON line (profiles/stream_digest.json holds the MI355X's)."""
import argparse, json, os, statistics, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import linne_amd
from bench import synth_track

ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=60.0)
ap.add_argument("--clips", type=int, default=256)
ap.add_argument("--clip-seconds", type=float, default=5.0)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
nch, bits, rate, block, preset = 2, 16, 44100, 10240, 7
dev = torch.device("cuda", 0)


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


def host_digest(pcm, b):
    """the recipe's table of one stream: [(crc32, bytes)] of an (n, C) int16 tensor on the host"""
    raw = memoryview(pcm.numpy()).cast("B")
    step = len(raw) if b == 0 else b * pcm.shape[1] * 2
    return [(zlib.crc32(raw[at:at + step]), len(raw[at:at + step])) for at in range(0, len(raw), step)]


def case(streams, b):
    def new(c):
        return c.digest_streams(streams, bucket_samples=b)

    def recipe(c):
        idx = c.index_streams(streams)
        got = c.decode_windows([(s, x, 0, None) for s, x in zip(streams, idx)], dtype=torch.int16, channels_last=True)
        out = [host_digest(g.cpu(), b) for g in got]
        for x in idx:
            x.close()
        return out

    forms = {"digest_streams": new, "recipe": recipe}
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
    out = {"streams": len(streams), "bucket_samples": b, "buckets_per_stream": int(answers["digest_streams"][0].crc32.shape[0])}
    out["answers_equal"] = all([(int(r["crc32"]), int(r["num_bytes"])) for r in d.cpu()] == r for d, r in zip(answers["digest_streams"], answers["recipe"]))
    out["peak_memory"] = peaks
    ctx = linne_amd.Context(0, use_torch_stream=True)
    idx = ctx.index_streams(streams)
    out["decoded_wav_bytes"] = sum(2 * x.header["num_channels"] * x.header["num_samples"] for x in idx)
    for fn in forms.values():
        fn(ctx)
    ts = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, fn in forms.items():
            ts[name].append(timed(lambda: fn(ctx)))
    for name in forms:
        out[name] = stats(ts[name])
    # kinds 83, 59, 79 and 80 over the same windows, one pass each
    wins = [(s, x, 0, None) for s, x in zip(streams, idx)]
    pcms = ctx.decode_windows(wins)
    ctx.enable_timing(True)
    k83, k59, k79, k80, calls = [], [], [], [], {}
    for _ in range(args.reps + 1):
        ctx.digest_windows(wins, bucket_samples=b)
        assert ctx.last_launches(83) == 1 and ctx.last_launches(59) == 0 and ctx.last_launches(84) == 1 and ctx.last_launches(85) == 1
        k83.append(ctx.last_ms(83)); calls.setdefault("digest_windows_device_ms", []).append(ctx.last_ms(0))
        calls.setdefault("kind_84_preset", []).append(ctx.last_ms(84)); calls.setdefault("kind_85_commit", []).append(ctx.last_ms(85))
        ctx.decode_windows(wins)
        assert ctx.last_launches(59) == 1 and ctx.last_launches(83) == 0
        k59.append(ctx.last_ms(59)); calls.setdefault("decode_windows_device_ms", []).append(ctx.last_ms(0))
        ctx.compare_windows([w + (p,) for w, p in zip(wins, pcms)])
        assert ctx.last_launches(79) == 1
        k79.append(ctx.last_ms(79))
        ctx.measure_windows(wins, bucket_samples=b)
        assert ctx.last_launches(80) == 1
        k80.append(ctx.last_ms(80))
    ctx.enable_timing(False)
    out["kind_83_k_wx_digest"], out["kind_59_k_wx_place"], out["kind_79_k_wx_compare"], out["kind_80_k_wx_measure"] = stats(k83[1:]), stats(k59[1:]), stats(k79[1:]), stats(k80[1:])
    out.update({k: stats(v[1:]) for k, v in calls.items()})
    samples = sum(x.header["num_channels"] * x.header["num_samples"] for x in idx)
    out["kind_83_ns_per_sample"] = round(out["kind_83_k_wx_digest"]["median_ms"] * 1e6 / samples, 6)
    del pcms
    for x in idx:
        x.close()
    ctx.close()
    slack = max(out["digest_streams"]["spread_ms"], out["recipe"]["spread_ms"])
    slack83 = max(out["kind_83_k_wx_digest"]["spread_ms"], out["kind_80_k_wx_measure"]["spread_ms"])
    out["criteria"] = {
        "faster_than_the_recipe_beyond_the_spread": verdict(out["digest_streams"]["median_ms"] + slack < out["recipe"]["median_ms"],
                                                            f"digest_streams {out['digest_streams']['median_ms']} ms against the recipe's {out['recipe']['median_ms']} ms (spread {slack} ms)"),
        "reported_kind_83_under_kind_80": verdict(out["kind_83_k_wx_digest"]["median_ms"] + slack83 < out["kind_80_k_wx_measure"]["median_ms"],
                                                  f"k_wx_digest {out['kind_83_k_wx_digest']['median_ms']} ms against k_wx_measure {out['kind_80_k_wx_measure']['median_ms']} ms (spread {slack83} ms); "
                                                  f"k_wx_place {out['kind_59_k_wx_place']['median_ms']} ms, k_wx_compare {out['kind_79_k_wx_compare']['median_ms']} ms"),
    }
    return out


result = {"config": f"44.1 kHz int16 stereo, -m {preset}, block {block}, MS", "reps": args.reps,
          "statistic": "median (min, max, spread = max - min) ms of the runs, warm-up excluded, each run ends in a device synchronise; the forms of a case alternate within a repetition",
          "recipe_library": "this build: its decode path is the parent commit's, launch for launch"}
enc = linne_amd.Context(0, use_torch_stream=True)
x = synth_track(int(args.minutes * 60 * rate), nch, bits, 3, dev, rate=float(rate))
s = enc.encode_stream(x, bits, rate, block, preset, True).clone()
del x
result["one_stream"] = {"stream": f"{args.minutes:g} min (BASELINE configs[1])", "bucket_0": case([s], 0), "bucket_441": case([s], 441)}
del s
n = int(args.clip_seconds * rate)
clips = [synth_track(n, nch, bits, 100 + t, dev, rate=float(rate)) for t in range(args.clips)]
streams = [t.clone() for t in enc.encode_streams([(p, bits, rate, block, preset, True) for p in clips])]
del clips
enc.close()
result["clips"] = {"stream": f"{args.clips} x {args.clip_seconds:g} s", "bucket_0": case(streams, 0), "bucket_441": case(streams, 441)}
print(json.dumps(result))
