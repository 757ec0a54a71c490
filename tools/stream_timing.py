"""What the stream timing tools (tools/stream_measure.py, stream_digest.py, stream_quiet.py, stream_histogram.py, stream_relate.py,
stream_compare.py, stream_mix.py, stream_resample.py) share, so that the figures under profiles/stream_*.json are taken in one way: the arguments, the material (BASELINE
configs[1]'s stream and the clips of that shape, encoded once on the device), the timing of one call, the statistic, the peak-memory
probe of every form on a context of its own, the repetitions in which the forms of a case alternate, the loops that read the HIP
events of single kernel kinds, and the head of the result.  A tool keeps what is its own: its docstring, its torch recipe, its
comparison of the two answers, its forms, its kinds and its criteria.

Every figure is the median of --reps runs after a warm-up, each run ending in a device synchronise, the forms of a case taken in turn
within a repetition; minimum and maximum beside the median, spread = max - min.  Peak device memory of a call = torch's peak
allocation during it plus what the context's scratch grew by (free device memory before and after, on a fresh context, less what
torch's allocator reserved).  A kind's figures leave out the loop's first round."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import linne_amd
from bench import synth_track

nch, bits, rate, block, preset = 2, 16, 44100, 10240, 7
dev = torch.device("cuda", 0)


def arguments(reps=9, label=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--clip-seconds", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=reps)
    if label is not None:
        ap.add_argument("--label", default=label)
    return ap.parse_args()


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


# ---- the material ----
def track(n, seed):
    return synth_track(n, nch, bits, seed, dev, rate=float(rate))


def one_stream(enc, args, prepare=None):
    """(BASELINE configs[1]'s stream, what prepare(pcm) answered after it wrote into the PCM)"""
    x = track(int(args.minutes * 60 * rate), 3)
    made = prepare(x) if prepare else None
    return enc.encode_stream(x, bits, rate, block, preset, True).clone(), made


def clips(enc, args, prepare=None):
    """(the clips' streams, encoded in one call; what prepare(pcm, seed) answered for each)"""
    n = int(args.clip_seconds * rate)
    pcm = [track(n, 100 + t) for t in range(args.clips)]
    made = [prepare(p, 100 + t) for t, p in enumerate(pcm)] if prepare else None
    return [t.clone() for t in enc.encode_streams([(p, bits, rate, block, preset, True) for p in pcm])], made


def one_stream_label(args):
    return f"{args.minutes:g} min (BASELINE configs[1])"


def clips_label(args):
    return f"{args.clips} x {args.clip_seconds:g} s"


def preamble(args, **more):
    return {"config": f"44.1 kHz int16 stereo, -m {preset}, block {block}, MS", "reps": args.reps, **more,
            "statistic": "median (min, max, spread = max - min) ms of the runs, warm-up excluded, each run ends in a device synchronise; the forms of a case alternate within a repetition",
            "recipe_library": "this build: its decode path is the parent commit's, launch for launch"}


def whole(streams, idx):
    return [(s, x, 0, None) for s, x in zip(streams, idx)]


# ---- measuring ----
def peak_memory(forms):
    """every form once on a context of its own -> (its answers, its peak device memory)"""
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
    return answers, peaks


def repetitions(ctx, forms, reps):
    """a warm-up of every form, then reps repetitions in which the forms take turns -> name: stats"""
    for fn in forms.values():
        fn(ctx)
    ts = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ts[name].append(timed(lambda: fn(ctx)))
    return {name: stats(ts[name]) for name in forms}


def kind_timings(ctx, steps, reps):
    """reps + 1 rounds of the steps in turn on a context with timing on.  A step is (call, check, figures): call() makes one library
    call, check(ctx.last_launches) asserts its launch counts, figures is [(kind, name)] -- kind 0 is the whole call's device time, a
    tuple of kinds their sum -> name: stats, the first round left out"""
    out = {name: [] for _, _, figures in steps for _, name in figures}
    for _ in range(reps + 1):
        for call, check, figures in steps:
            call()
            check(ctx.last_launches)
            for kind, name in figures:
                out[name].append(sum(ctx.last_ms(k) for k in kind) if isinstance(kind, tuple) else ctx.last_ms(kind))
    return {name: stats(v[1:]) for name, v in out.items()}


def decode_step(ctx, wins, none_of, figures=((59, "kind_59_k_wx_place"), (0, "decode_windows_device_ms"))):
    def check(n):
        assert n(59) == 1 and n(none_of) == 0
    return (lambda: ctx.decode_windows(wins), check, list(figures))


def compare_step(ctx, wins, pcms):
    def check(n):
        assert n(79) == 1
    held = [w + (p,) for w, p in zip(wins, pcms)]
    return (lambda: ctx.compare_windows(held), check, [(79, "kind_79_k_wx_compare")])


def measure_step(ctx, wins, b, none_of=None, figures=((80, "kind_80_k_wx_measure"),)):
    def check(n):
        assert n(80) == 1 and (none_of is None or n(none_of) == 0)
    return (lambda: ctx.measure_windows(wins, bucket_samples=b), check, list(figures))


def case(streams, forms, head, same, loops, criteria, reps, decoded=("decoded_pcm_bytes", 4), after=None):
    """one case of a tool whose forms are the library's call (the first form) and "recipe".  head(answers of the call) begins the
    case's figures; same(answer, recipe's) compares a stream's two answers; loops(ctx, wins) -> the kind_timings step lists, made
    before timing is switched on; criteria(out, peaks) -> the case's criteria; after(out, idx) adds figures of the tool's own"""
    name = next(iter(forms))
    answers, peaks = peak_memory(forms)
    out = head(answers[name])
    out["answers_equal"] = all(same(a, r) for a, r in zip(answers[name], answers["recipe"]))
    out["peak_memory"] = peaks
    del answers
    ctx = linne_amd.Context(0, use_torch_stream=True)
    idx = ctx.index_streams(streams)
    out[decoded[0]] = sum(decoded[1] * x.header["num_channels"] * x.header["num_samples"] for x in idx)
    out.update(repetitions(ctx, forms, reps))
    todo = loops(ctx, whole(streams, idx), out)
    ctx.enable_timing(True)
    for steps in todo:
        out.update(kind_timings(ctx, steps, reps))
    ctx.enable_timing(False)
    if after:
        after(out, idx)
    del todo, steps
    for x in idx:
        x.close()
    ctx.close()
    out["criteria"] = criteria(out, peaks)
    return out


def recipe_of(streams, table, **decode):
    """the recipe a user wrote before a call existed: index_streams + decode_windows over the whole streams + table(pcm) of each"""
    def recipe(c):
        idx = c.index_streams(streams)
        got = c.decode_windows(whole(streams, idx), **decode)
        out = [table(g) for g in got]
        for x in idx:
            x.close()
        return out
    return recipe


def faster_than(out, name, what="recipe"):
    """the criterion every tool has: the call's median under the recipe's by more than the larger spread"""
    slack = max(out[name]["spread_ms"], out["recipe"]["spread_ms"])
    return verdict(out[name]["median_ms"] + slack < out["recipe"]["median_ms"], f"{name} {out[name]['median_ms']} ms against the {what}'s {out['recipe']['median_ms']} ms (spread {slack} ms)")


def bucketed(args, case):
    """the run of a tool whose cases are bucket_samples 0 (one bucket per stream) and 441 (10 ms), on the one stream and on the clips"""
    result = preamble(args)
    enc = linne_amd.Context(0, use_torch_stream=True)
    s, _ = one_stream(enc, args)
    result["one_stream"] = {"stream": one_stream_label(args), "bucket_0": case([s], 0), "bucket_441": case([s], 441)}
    del s
    streams, _ = clips(enc, args)
    enc.close()
    result["clips"] = {"stream": clips_label(args), "bucket_0": case(streams, 0), "bucket_441": case(streams, 441)}
    print(json.dumps(result))
