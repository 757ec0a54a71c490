"""Timing of the resident stream path on the PCM people hold -- interleaved int16 in, a float32 channels-last batch out -- against
the int32 planar boundary of the commit before the PCM layouts (profiles/pcm_layouts.json holds the MI355X's figures).

  encode  Context.encode_streams of 256 five-second 16-bit stereo clips (44.1 kHz, -m 7, MS, block 10240):
            new  from interleaved int16 tensors (N, 2), as a WAV file's data chunk lies in memory
            (a)  the parent's encode_streams on int32 planar copies made beforehand (the conversion is not timed)
            (b)  what a user of the parent does: x.T.to(torch.int32).contiguous() per track, then (a)
  decode  Context.decode_windows of 256 five-second windows into one float32 (W, n, C) batch:
            new  one call with dtype=torch.float32, channels_last=True
            (p)  the parent's decode_windows into an int32 (W, C, n) batch, then out.transpose(1, 2).to(float32) * 2^-15
  kinds   the kernels that touch the caller's PCM, by the library's own timing: 60 (k_sb_gather) and 59 (k_wx_place) of the calls
          above, and "60s", the gather of one 60-second track through encode_stream (the single call is the one-track case of the
          batch call and reports 60; the parent's own k_se_gather reported 48): new on int16 interleaved, parent on int32 planar

--parent DIR names a directory that holds the parent commit's linne_amd package, built.  Every measurement runs in a process of its
own (a worker: this file with --worker), parent and new in turn, --rounds times over; a worker warms up, then times --reps calls,
each ending in a device synchronise.  The spread is the largest difference between two rounds' medians of the same measurement.
The verdict: new encode not slower than (a) beyond that spread; faster than (b); new decode faster than (p); kinds 60s, 60 and 59 no
slower than the parent's.  Peak memory is torch's (max_memory_allocated over the timed calls: the caller's tensors and temporaries; the
context's own scratch is hipMalloc'ed and the same size on both sides)."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--parent", help="directory holding the parent commit's built linne_amd package")
ap.add_argument("--worker", choices=("new", "parent"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--clips", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm_layouts.json"))
args = ap.parse_args()
assert args.reps >= 5 and args.rounds >= 2


def worker():
    sys.path.insert(0, args.parent if args.worker == "parent" else ROOT)
    sys.path.append(ROOT)
    sys.path.append(os.path.join(ROOT, "tests"))
    import torch
    import linne_amd
    from bench import synth_track
    assert os.path.dirname(os.path.dirname(os.path.abspath(linne_amd.__file__))) == os.path.abspath(args.parent if args.worker == "parent" else ROOT)
    nch, bits, rate, block, preset, ms = 2, 16, 44100, 10240, 7, True
    n5 = 5 * rate
    lengths = [n5 + 13 * i for i in range(args.clips)]
    total = 10 * 60 * rate
    base = synth_track(total, nch, bits, 3, torch.device("cuda", 0), rate=float(rate)).to(torch.int32).contiguous()
    step = (total - max(lengths)) // len(lengths)
    planar32 = [base[:, i * step:i * step + n].contiguous() for i, n in enumerate(lengths)]
    inter16 = [x.T.to(torch.int16).contiguous() for x in planar32]          # (N, 2), as in a WAV file
    ctx = linne_amd.Context(0, use_torch_stream=True)

    def stats(fn):
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            del r
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                "peak_mib_over_held": round((torch.cuda.max_memory_allocated() - held) / 2 ** 20, 1)}

    def kinds(fn, which, name=None):
        ctx.enable_timing(True)
        r = fn()
        out = {name or str(k): {"ms": round(ctx.last_ms(k), 4), "launches": ctx.last_launches(k)} for k in which}
        ctx.enable_timing(False)
        del r
        return out

    def tracks(xs):
        return [(x, bits, rate, block, preset, ms) for x in xs]

    rec = {"worker": args.worker, "clips": args.clips, "reps": args.reps}
    streams = ctx.encode_streams(tracks(planar32))
    rec["stream_bytes"] = int(sum(s.numel() for s in streams))
    indexes = [ctx.index_stream(s) for s in streams]
    wins = [(s, ix, 0, n5) for s, ix in zip(streams, indexes)]
    scale = 2.0 ** -(bits - 1)
    minute = base[:, :60 * rate].contiguous()
    if args.worker == "parent":
        rec["encode_a_int32_planar"] = stats(lambda: ctx.encode_streams(tracks(planar32)))
        rec["encode_b_convert_then_a"] = stats(lambda: ctx.encode_streams(tracks([x.T.to(torch.int32).contiguous() for x in inter16])))
        out32 = torch.empty((args.clips, nch, n5), dtype=torch.int32, device="cuda")
        rec["decode_p_int32_then_convert"] = stats(lambda: ctx.decode_windows(wins, out=out32).transpose(1, 2).to(torch.float32).mul_(scale).contiguous())
        rec["kinds"] = {**kinds(lambda: ctx.encode_streams(tracks(planar32)), (60,)), **kinds(lambda: ctx.decode_windows(wins, out=out32), (59,)),
                        **kinds(lambda: ctx.encode_stream(minute, bits, rate, block, preset, ms), (48,), "60s")}
    else:
        got = ctx.encode_streams(tracks([x.T for x in inter16]))
        rec["streams_equal_the_int32_planar_call's"] = all(bool(torch.equal(g, s)) for g, s in zip(got, streams))
        del got
        rec["encode_new_int16_interleaved"] = stats(lambda: ctx.encode_streams(tracks([x.T for x in inter16])))
        rec["encode_new_int32_planar"] = stats(lambda: ctx.encode_streams(tracks(planar32)))
        batch = torch.empty((args.clips, n5, nch), dtype=torch.float32, device="cuda")
        ref = ctx.decode_windows(wins[:8])
        ctx.decode_windows(wins, out=batch, dtype=torch.float32, channels_last=True)
        rec["batch_equals_the_converted_int32_windows"] = all(bool(torch.equal(batch[i], r.T.to(torch.float32) * scale)) for i, r in enumerate(ref))
        del ref
        rec["decode_new_float32_channels_last"] = stats(lambda: ctx.decode_windows(wins, out=batch, dtype=torch.float32, channels_last=True))
        minute16 = minute.T.to(torch.int16).contiguous()
        rec["kinds"] = {**kinds(lambda: ctx.encode_streams(tracks([x.T for x in inter16])), (60,)),
                        **kinds(lambda: ctx.decode_windows(wins, out=batch, dtype=torch.float32, channels_last=True), (59,)),
                        **kinds(lambda: ctx.encode_stream(minute16.T, bits, rate, block, preset, ms), (60,), "60s")}
    for ix in indexes:
        ix.close()
    ctx.close()
    print("RESULT " + json.dumps(rec))


def main():
    assert args.parent and os.path.exists(os.path.join(args.parent, "linne_amd", "__init__.py")), "--parent DIR: the parent commit's built package"
    runs = {"parent": [], "new": []}
    for rnd in range(args.rounds):
        for who in ("parent", "new"):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", who, "--parent", os.path.abspath(args.parent), "--reps", str(args.reps),
                   "--clips", str(args.clips)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"worker {who} of round {rnd} ended with {r.returncode}")
            runs[who].append(json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:]))
            print(f"round {rnd} {who}: done", flush=True)

    def med(who, key):
        return [r[key]["median_ms"] for r in runs[who]]

    keys = {"parent": ["encode_a_int32_planar", "encode_b_convert_then_a", "decode_p_int32_then_convert"],
            "new": ["encode_new_int16_interleaved", "encode_new_int32_planar", "decode_new_float32_channels_last"]}
    spread = {k: round(max(med(w, k)) - min(med(w, k)), 3) for w in keys for k in keys[w]}
    best = {k: min(med(w, k)) for w in keys for k in keys[w]}
    enc_spread = max(spread["encode_a_int32_planar"], spread["encode_new_int16_interleaved"])

    def kind_ms(who, k):
        return min(r["kinds"][k]["ms"] for r in runs[who])

    def kind_spread(k):
        return max(max(r["kinds"][k]["ms"] for r in runs[w]) - min(r["kinds"][k]["ms"] for r in runs[w]) for w in runs)
    verdict = {
        "encode_not_slower_than_a_beyond_the_spread": bool(best["encode_new_int16_interleaved"] <= best["encode_a_int32_planar"] + enc_spread),
        "encode_faster_than_b": bool(best["encode_new_int16_interleaved"] < best["encode_b_convert_then_a"]),
        "decode_faster_than_parent_plus_conversion": bool(best["decode_new_float32_channels_last"] < best["decode_p_int32_then_convert"]),
        "kinds_no_slower_than_the_parent's": {k: bool(kind_ms("new", k) <= kind_ms("parent", k) + kind_spread(k)) for k in ("60s", "60", "59")},
    }
    peak = {k: max(r[k]["peak_mib_over_held"] for r in runs[w]) for w in keys for k in keys[w]}
    result = {
        "config": "44.1 kHz 16-bit stereo, -m 7, block 10240, MS; %d five-second clips / windows; PCM and streams resident" % args.clips,
        "statistic": "per worker process: median / min / max ms over --reps calls after a warm-up, each ending in a device synchronise; "
                     "compared: the lower of the rounds' medians; spread: the largest difference between two rounds' medians of one measurement",
        "reps": args.reps, "rounds": args.rounds, "runs": runs, "best_median_ms": best, "spread_ms": spread,
        "kind_ms": {k: {"new_int16_interleaved": kind_ms("new", k), "parent_int32_planar": kind_ms("parent", k), "spread": round(kind_spread(k), 4)} for k in ("60s", "60", "59")},
        "peak_mib_over_held": peak,
        "peak_mib_difference": {"encode_new_minus_b": round(peak["encode_new_int16_interleaved"] - peak["encode_b_convert_then_a"], 1),
                                "decode_new_minus_p": round(peak["decode_new_float32_channels_last"] - peak["decode_p_int32_then_convert"], 1)},
        "verdict": verdict,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps({"best_median_ms": best, "spread_ms": spread, "kind_ms": result["kind_ms"], "peak_mib_difference": result["peak_mib_difference"], "verdict": verdict}))


if __name__ == "__main__":
    worker() if args.worker else main()
