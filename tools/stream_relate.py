"""Timing and memory of Context.relate_streams (per channel pair and bucket the exact sum of a_i * a_j and the counts of equal and of
opposite frames of resident .lnn streams, nothing decoded into memory) against the recipe a user wrote before the call existed:
index_streams + decode_windows (int32 planar) over the whole streams + the torch reductions that give the same numbers (per pair the
int64 sum of the int64 products and the two counts -- exact for 16-bit material; the library's sum is 128 bits wide).  Two cases, each
with bucket_samples 0 (one bucket per stream) and 441 (10 ms):
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS;
  (b) 256 clips of 5 seconds of that shape, in one call.
The streams are encoded once on the device and stay resident.  Both forms run on this build -- the decode path is the parent
commit's, launch for launch, which the suite holds.  Every figure is the median of --reps runs after a warm-up, each run ending in a
device synchronise, the forms of a case taken in turn within a repetition; minimum and maximum beside the median, spread = max -
min.  Peak device memory of a call = torch's peak allocation during it plus what the context's scratch grew by (free device memory
before and after, on a fresh context, less what torch's allocator reserved).  Kinds 95, 80 and 59 are HIP events around k_wx_relate,
k_wx_measure and k_wx_place in a relate_windows, a measure_windows and a decode_windows call over the same windows (one pass each);
k_wx_measure and k_wx_place are the parent commit's kernels, unchanged.  Prints one JSON line (profiles/stream_relate.json holds
the MI355X's; profiles/stream_relate_wide_fold.json the same run on a library built with -DWXR_NARROW=0, where every wave folds the
products as (lo, hi))."""
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


def reduce_pairs(x):
    """per channel pair i <= j over the last dimension of an int32 tensor (C, ..., n): (dot, its sign's extension, equal, opposite),
    int64 each -> (P, ..., 4)"""
    w = x.to(torch.int64)
    rows = []
    for i in range(w.shape[0]):
        for j in range(i, w.shape[0]):
            d = (w[i] * w[j]).sum(-1)
            rows.append(torch.stack([d, d >> 63, (w[i] == w[j]).sum(-1), (w[i] + w[j] == 0).sum(-1)], dim=-1))
    return torch.stack(rows, dim=0)


def torch_relate(pcm, b):
    """the recipe's table of one stream: (P, nb, 4) int64"""
    n = pcm.shape[1]
    if b == 0 or b >= n:
        return reduce_pairs(pcm).unsqueeze(1)
    full = n // b
    parts = [reduce_pairs(pcm[:, :full * b].view(pcm.shape[0], full, b))]
    if n % b:
        parts.append(reduce_pairs(pcm[:, full * b:]).unsqueeze(1))
    return torch.cat(parts, dim=1)


def same(m, r):
    """a Relations against the recipe's table (64-bit sums, extended by their sign)"""
    return bool(torch.equal(m.records, r))


def case(streams, b):
    decoded_bytes = 0

    def new(c):
        return c.relate_streams(streams, bucket_samples=b)

    def recipe(c):
        idx = c.index_streams(streams)
        got = c.decode_windows([(s, x, 0, None) for s, x in zip(streams, idx)])
        out = [torch_relate(g, b) for g in got]
        for x in idx:
            x.close()
        return out

    forms = {"relate_streams": new, "recipe": recipe}
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
    out = {"streams": len(streams), "bucket_samples": b, "buckets_per_stream": int(answers["relate_streams"][0].records.shape[1])}
    out["answers_equal"] = all(same(m, r) for m, r in zip(answers["relate_streams"], answers["recipe"]))
    out["peak_memory"] = peaks
    ctx = linne_amd.Context(0, use_torch_stream=True)
    idx = ctx.index_streams(streams)
    decoded_bytes = sum(4 * x.header["num_channels"] * x.header["num_samples"] for x in idx)
    out["decoded_pcm_bytes"] = decoded_bytes
    for fn in forms.values():
        fn(ctx)
    ts = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, fn in forms.items():
            ts[name].append(timed(lambda: fn(ctx)))
    for name in forms:
        out[name] = stats(ts[name])
    # kinds 95, 80 and 59 over the same windows, one pass each
    wins = [(s, x, 0, None) for s, x in zip(streams, idx)]
    ctx.enable_timing(True)
    k95, k80, k59, calls = [], [], [], {}
    for _ in range(args.reps + 1):
        ctx.relate_windows(wins, bucket_samples=b)
        assert ctx.last_launches(95) == 1 and ctx.last_launches(59) == 0 and ctx.last_launches(96) == 1 and ctx.last_launches(97) == 1
        k95.append(ctx.last_ms(95)); calls.setdefault("relate_windows_device_ms", []).append(ctx.last_ms(0))
        calls.setdefault("kind_96_preset", []).append(ctx.last_ms(96)); calls.setdefault("kind_97_commit", []).append(ctx.last_ms(97))
        ctx.measure_windows(wins, bucket_samples=b)
        assert ctx.last_launches(80) == 1 and ctx.last_launches(95) == 0
        k80.append(ctx.last_ms(80)); calls.setdefault("measure_windows_device_ms", []).append(ctx.last_ms(0))
        ctx.decode_windows(wins)
        assert ctx.last_launches(59) == 1 and ctx.last_launches(95) == 0
        k59.append(ctx.last_ms(59)); calls.setdefault("decode_windows_device_ms", []).append(ctx.last_ms(0))
    ctx.enable_timing(False)
    out["kind_95_k_wx_relate"], out["kind_80_k_wx_measure"], out["kind_59_k_wx_place"] = stats(k95[1:]), stats(k80[1:]), stats(k59[1:])
    out.update({k: stats(v[1:]) for k, v in calls.items()})
    for x in idx:
        x.close()
    ctx.close()
    slack = max(out["relate_streams"]["spread_ms"], out["recipe"]["spread_ms"])
    slack95 = max(out["kind_95_k_wx_relate"]["spread_ms"], out["kind_80_k_wx_measure"]["spread_ms"])
    out["criteria"] = {
        "faster_than_the_recipe_beyond_the_spread": verdict(out["relate_streams"]["median_ms"] + slack < out["recipe"]["median_ms"],
                                                            f"relate_streams {out['relate_streams']['median_ms']} ms against the recipe's {out['recipe']['median_ms']} ms (spread {slack} ms)"),
        "peak_memory": f"{peaks['relate_streams']['peak_bytes']} bytes against the recipe's {peaks['recipe']['peak_bytes']}; the decoded PCM is {decoded_bytes}",
        "kind_95_not_slower_than_kind_80": verdict(out["kind_95_k_wx_relate"]["median_ms"] <= out["kind_80_k_wx_measure"]["median_ms"] + slack95,
                                                   f"{out['kind_95_k_wx_relate']['median_ms']} ms against {out['kind_80_k_wx_measure']['median_ms']} ms (spread {slack95} ms); k_wx_place {out['kind_59_k_wx_place']['median_ms']} ms"),
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
