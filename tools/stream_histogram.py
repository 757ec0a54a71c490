"""Timing and memory of Context.histogram_streams (the sample levels of resident .lnn streams counted per channel, bucket and bin,
nothing decoded into memory) against the composition a user had before the call existed: index_streams + decode_windows (int32 planar)
over the whole streams + torch (abs, shift, clamp -- or the bit length --, bincount per channel and bucket).  Two workloads, each with
two settings -- 1024 linear bins at shift 5 in one bucket, and 33 log2 bins in buckets of 441 samples:
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS;
  (b) 256 clips of 5 seconds of that shape, in one call.
One-bin material beside them: a 60-minute track of one constant value, and the 60-minute music with two log2 bins; there kind 92 is set
against kind 92 on the music with 1024 linear bins.  The streams are encoded once on the device and stay resident.  Both forms run on
this build -- the decode path is the parent commit's, launch for launch, which the suite holds.  How every figure is taken -- the
statistic, the repetitions, the peak device memory of a call -- is tools/stream_timing.py's.  Kinds 92, 59 and 80 are
HIP events around k_wx_histogram, k_wx_place and k_wx_measure in a histogram_windows, a decode_windows and a measure_windows call over
the same windows (one pass each); kinds 93 and 94 are the histogram call's preset and commit.  The library is measured as it is built:
to see k_wx_histogram without the addition inside a wave, build with -DWXH_SHARE=65 (no wave has 65 lanes) and run this again with
--label.  Prints one JSON line (profiles/stream_histogram.json holds the MI355X's)."""
import json
import stream_timing as st                     # (first: it puts the repository's root on the path)
import torch
import linne_amd
from stream_timing import bits, block, dev, nch, preset, rate, verdict

args = st.arguments(label="as built (WXH_SHARE 8)")
SETTINGS = {"linear_1024_one_bucket": (1024, 5, False, 0), "log2_33_buckets_of_441": (33, 0, True, 441)}


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


def histogram_step(ctx, wins, spec):
    """kind 92 (and 93, 94) of a histogram call over wins, one pass"""
    def check(n):
        assert n(92) == 1 and n(59) == 0 and n(93) == 1 and n(94) == 1
    return (lambda: ctx.histogram_windows(wins, *spec), check,
            [(92, "kind_92_k_wx_histogram"), (93, "kind_93_preset"), (94, "kind_94_commit"), (0, "histogram_windows_device_ms")])


def case(streams, spec):
    bins, shift, log2, b = spec
    forms = {"histogram_streams": lambda c: c.histogram_streams(streams, bins, shift, log2, b), "recipe": st.recipe_of(streams, lambda g: torch_histogram(g, bins, shift, log2, b))}

    def head(answers):
        return {"streams": len(streams), "num_bins": bins, "shift": shift, "log2": log2, "bucket_samples": b}

    def loops(ctx, wins, out):
        return [[histogram_step(ctx, wins, spec)],
                [st.decode_step(ctx, wins, 92, [(59, "kind_59_k_wx_place")]), st.measure_step(ctx, wins, b)]]

    def criteria(out, peaks):
        k92, k59m, k80m = out["kind_92_k_wx_histogram"]["median_ms"], out["kind_59_k_wx_place"]["median_ms"], out["kind_80_k_wx_measure"]["median_ms"]
        return {
            "faster_than_the_composition_beyond_the_spread": st.faster_than(out, "histogram_streams", "composition"),
            "peak_memory_below_the_composition": verdict(peaks["histogram_streams"]["peak_bytes"] < peaks["recipe"]["peak_bytes"],
                                                         f"{peaks['histogram_streams']['peak_bytes']} bytes against {peaks['recipe']['peak_bytes']}; the decoded PCM is {out['decoded_pcm_bytes']}"),
            "kind_92_between_place_and_measure_(a_guess,_not_a_criterion)": f"k_wx_place {k59m} ms, k_wx_histogram {k92} ms, k_wx_measure {k80m} ms",
        }

    return st.case(streams, forms, head, lambda h, r: torch.equal(h.counts, r), loops, criteria, args.reps)


def one_bin(streams, spec, music_k92):
    ctx = linne_amd.Context(0, use_torch_stream=True)
    idx = ctx.index_streams(streams)
    wins = st.whole(streams, idx)
    h = ctx.histogram_windows(wins, *spec)[0].counts
    ctx.enable_timing(True)
    out = st.kind_timings(ctx, [histogram_step(ctx, wins, spec)], args.reps)
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


result = st.preamble(args, library=args.label)
enc = linne_amd.Context(0, use_torch_stream=True)
s, _ = st.one_stream(enc, args)
result["one_stream"] = {"stream": st.one_stream_label(args)}
result["one_stream"].update({name: case([s], spec) for name, spec in SETTINGS.items()})
music_k92 = result["one_stream"]["linear_1024_one_bucket"]["kind_92_k_wx_histogram"]
flat = enc.encode_stream(torch.full((nch, int(args.minutes * 60 * rate)), 1000, dtype=torch.int32, device=dev), bits, rate, block, preset, True).clone()
result["one_bin"] = {"constant_track_linear_1024": one_bin([flat], (1024, 0, False, 0), music_k92),
                     "music_log2_2_bins": one_bin([s], (2, 0, True, 0), music_k92)}
del s, flat
streams, _ = st.clips(enc, args)
enc.close()
result["clips"] = {"stream": st.clips_label(args)}
result["clips"].update({name: case(streams, spec) for name, spec in SETTINGS.items()})
print(json.dumps(result))
