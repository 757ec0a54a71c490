"""Timing and memory of Context.overlay_windows (windows of several resident .lnn streams summed into each output under gains that move
linearly over a source) and of Context.crossfade_streams (streams joined with crossfades into a new stream) against the recipes a user
wrote before the calls existed: index_streams + decode_windows (int32 planar) of every source + torch -- the int64 widening, the ramps
from arange, the multiply, the sum, the rounding shift, the clamp and the conversion -- and decode_stream + that + encode_stream.  The
two answers must be equal.  The cases:
  (a) BASELINE configs[1]'s stream, 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS, overlaid with itself delayed by one
      second, constant gains: int32;
  (b) 256 clips of 5 seconds of that shape, each under the next clip at a gain of its own, in one call: a float32 channels_last batch;
  (c) 16 of the clips joined by crossfades of 100 ms into one stream (crossfade_streams).
The streams are encoded once on the device and stay resident.  How every figure is taken -- the statistic, the repetitions, the peak
device memory of a call -- is tools/stream_timing.py's.  Kinds 101 and 59 are HIP events around k_wx_overlay and k_wx_place in an
overlay_windows call: with one unity source per stream (the floor: k_wx_place of a decode_windows call over the same windows writes the
same bytes, and k_wx_resample at 1/1 with one tap stands beside it) and with two sources.  Prints one JSON line
(profiles/stream_overlay.json holds the MI355X's)."""
import json
import numpy as np
import torch
import stream_timing as st                # (puts the repository's root on the path)
import linne_amd
from stream_timing import verdict

args = st.arguments(reps=9)
LO, HI = -(1 << (st.bits - 1)), (1 << (st.bits - 1)) - 1
ONE = np.array([[1]], dtype=np.int16)
SHIFT = 15
COPY_TBPS = 2.5                           # the copy kernel of profiles/stream_splice.json


def torch_overlay(n_out, parts, shift, float32, channels_last):
    """the recipe's overlay of decoded sources: parts of (pcm (C, n) int32, at, (gain_q32, step_q32))"""
    C = parts[0][0].shape[0]
    acc = torch.zeros((C, n_out), dtype=torch.int64, device=st.dev)
    for g, at, (q, step) in parts:
        n = g.shape[1]
        ramp = (torch.arange(n, dtype=torch.int64, device=st.dev) * step + q) >> 32
        acc[:, at:at + n] += g.to(torch.int64) * ramp
    if shift:
        acc = (acc + (1 << (shift - 1))) >> shift
    acc.clamp_(LO, HI)
    y = acc.to(torch.float32).mul_(2.0 ** -(st.bits - 1)) if float32 else acc.to(torch.int32)
    return y.t().contiguous() if channels_last else y


def overlay_case(streams, jobs, float32, channels_last, batch):
    """jobs: per output (num_samples, [(stream number, at, gain pair)]) over whole streams; batch: the outputs go into one (W, n, C) tensor"""
    kw = {"dtype": torch.float32 if float32 else torch.int32, "channels_last": channels_last}
    pair = lambda g: (int(g) << 32, 0) if isinstance(g, int) else g

    def outputs(idx, js=jobs):
        return [(n, [(streams[k], idx[k], 0, None, at, g) for k, at, g in srcs]) for n, srcs in js]

    def call(c, idx, js=jobs):
        out = torch.empty((len(js), js[0][0], st.nch), dtype=kw["dtype"], device=st.dev) if batch else None
        return c.overlay_windows(outputs(idx, js), shift=SHIFT, clip_bits=st.bits, out=out, **kw)

    def overlaid(c):
        idx = c.index_streams(streams)
        got = call(c, idx)
        for x in idx:
            x.close()
        return got

    def recipe(c):
        idx = c.index_streams(streams)
        flat = [(k, at, g) for _, srcs in jobs for k, at, g in srcs]
        pcm = c.decode_windows([(streams[k], idx[k], 0, None) for k, _, _ in flat])     # every source, as the call takes them
        out, i = [], 0
        for n, srcs in jobs:
            out.append(torch_overlay(n, [(pcm[i + j], at, pair(g)) for j, (_, at, g) in enumerate(srcs)], SHIFT, float32, channels_last))
            i += len(srcs)
        for x in idx:
            x.close()
        return torch.stack(out) if batch else out
    forms = {"overlay_windows": overlaid, "recipe": recipe}
    answers, peaks = st.peak_memory(forms)
    got, want = answers["overlay_windows"], answers["recipe"]
    out = {"streams": len(streams), "outputs": len(jobs), "sources_per_output": len(jobs[0][1]), "output": ("float32" if float32 else "int32") + (", channels_last" if channels_last else ""),
           "output_bytes": int(sum(a.numel() * 4 for a in got)), "answers_equal": bool(all(torch.equal(a, r) for a, r in zip(got, want))), "peak_memory": peaks}
    del answers, got, want
    ctx = linne_amd.Context(0, use_torch_stream=True)
    idx = ctx.index_streams(streams)
    out["decoded_pcm_bytes"] = sum(4 * x.header["num_channels"] * x.header["num_samples"] for x in idx)
    out.update(st.repetitions(ctx, forms, args.reps))
    # the kinds: one unity source per stream (what decode_windows writes), and that stream twice
    wins = st.whole(streams, idx)
    lens = [x.header["num_samples"] for x in idx]
    ones = [(n, [(k, 0, 1)]) for k, n in enumerate(lens)]
    twos = [(n, [(k, 0, 1), (k, 0, -1)]) for k, n in enumerate(lens)]

    def check(n):
        assert n(101) == 1 and n(59) == 1 and n(99) == 0 and n(100) == 0
    def check_resample(n):
        assert n(100) == 1 and n(101) == 0
    steps = [(lambda: ctx.overlay_windows(outputs(idx, ones)), check, [(101, "kind_101_one_unity_source"), (59, "kind_59_k_wx_place_into_the_images"), (0, "overlay_windows_one_source_device_ms")]),
             (lambda: ctx.overlay_windows(outputs(idx, twos)), check, [(101, "kind_101_two_sources")]),
             (lambda: call(ctx, idx), check, [(101, "kind_101_the_case"), (0, "overlay_windows_device_ms")]),
             (lambda: ctx.resample_windows(wins, 1, 1, coef=ONE), check_resample, [(100, "kind_100_identity_1_tap")]),
             st.decode_step(ctx, wins, 101)]
    ctx.enable_timing(True)
    out.update(st.kind_timings(ctx, steps, args.reps))
    ctx.enable_timing(False)
    del steps
    for x in idx:
        x.close()
    ctx.close()
    one, two, k100, k59 = (out[k]["median_ms"] for k in ("kind_101_one_unity_source", "kind_101_two_sources", "kind_100_identity_1_tap", "kind_59_k_wx_place"))
    moved = lambda sources: (sources + 1) * out["decoded_pcm_bytes"]            # 4 C bytes per source and output sample, and the store
    tbps = lambda sources, ms: round(moved(sources) / max(ms, 1e-6) / 1e9, 3)
    out["kind_101_bytes_moved"] = {"one_source": moved(1), "two_sources": moved(2), "one_source_TB_per_s": tbps(1, one), "two_sources_TB_per_s": tbps(2, two), "copy_kernel_TB_per_s": COPY_TBPS}
    out["criteria"] = {
        "faster_than_the_recipe_beyond_the_spread": st.faster_than(out, "overlay_windows"),
        "lower_peak_memory_than_the_recipe": verdict(peaks["overlay_windows"]["peak_bytes"] < peaks["recipe"]["peak_bytes"],
                                                     f"{peaks['overlay_windows']['peak_bytes']} bytes against the recipe's {peaks['recipe']['peak_bytes']}; the decoded PCM is {out['decoded_pcm_bytes']}"),
        "one_source_under_kind_100s_floor": verdict(one < k100, f"k_wx_overlay with one unity source {one} ms, k_wx_resample at 1/1 with one tap {k100} ms, k_wx_place on the same windows {k59} ms"),
        "two_sources_under_twice_one": verdict(two < 2 * one, f"k_wx_overlay with two sources {two} ms, with one {one} ms: {round(two / max(one, 1e-6), 2)} times"),
        "against_the_copy_kernel": f"k_wx_overlay moves {tbps(1, one)} TB/s with one source and {tbps(2, two)} TB/s with two; the copy kernel {COPY_TBPS} TB/s",
    }
    return out


def join_case(streams, overlap):
    """crossfade_streams against decode_stream + torch + encode_stream: the encode dominates both"""
    down, up = linne_amd.crossfade(overlap, 16384)

    def recipe(c):
        pcm = [c.decode_stream(s) for s in streams]
        parts, at = [], 0
        for i, g in enumerate(pcm):
            n = g.shape[1]
            head, tail = overlap if i else 0, overlap if i + 1 < len(pcm) else 0
            parts += ([(g[:, :head], at, up)] if head else []) + [(g[:, head:n - tail], at + head, (16384 << 32, 0))] + ([(g[:, n - tail:], at + n - tail, down)] if tail else [])
            at += n - tail
        y = torch_overlay(at, parts, 14, False, False)
        return [c.encode_stream(y, st.bits, st.rate, st.block, st.preset, True)]
    forms = {"crossfade_streams": lambda c: [c.crossfade_streams(streams, overlap)], "recipe": recipe}
    answers, peaks = st.peak_memory(forms)
    out = {"streams": len(streams), "overlap_samples": overlap, "answers_equal": bool(torch.equal(answers["crossfade_streams"][0], answers["recipe"][0])),
           "stream_bytes": int(answers["recipe"][0].numel()), "peak_memory": peaks}
    del answers
    ctx = linne_amd.Context(0, use_torch_stream=True)
    out.update(st.repetitions(ctx, forms, args.reps))
    ctx.close()
    slack = max(out["crossfade_streams"]["spread_ms"], out["recipe"]["spread_ms"])
    out["criteria"] = {
        "not_slower_than_the_recipe_beyond_the_spread": verdict(out["crossfade_streams"]["median_ms"] <= out["recipe"]["median_ms"] + slack,
                                                                f"crossfade_streams {out['crossfade_streams']['median_ms']} ms against the recipe's {out['recipe']['median_ms']} ms (spread {slack} ms)"),
        "lower_peak_memory_than_the_recipe": verdict(peaks["crossfade_streams"]["peak_bytes"] < peaks["recipe"]["peak_bytes"], f"{peaks['crossfade_streams']['peak_bytes']} bytes against the recipe's {peaks['recipe']['peak_bytes']}"),
    }
    return out


result = st.preamble(args)
enc = linne_amd.Context(0, use_torch_stream=True)
s, _ = st.one_stream(enc, args)
N = int(args.minutes * 60 * st.rate)
delay = min(st.rate, N)
result["one_stream"] = {"stream": st.one_stream_label(args), "with_itself_a_second_later_int32": overlay_case([s], [(N + delay, [(0, 0, 20000), (0, delay, 12000)])], False, False, False)}
del s
streams, _ = st.clips(enc, args)
enc.close()
n = int(args.clip_seconds * st.rate)
jobs = [(n, [(i, 0, 24000), ((i + 1) % len(streams), 0, 1000 + 37 * (i % 200))]) for i in range(len(streams))]
result["clips"] = {"stream": st.clips_label(args), "under_the_next_clip_float32_channels_last": overlay_case(streams, jobs, True, True, True),
                   "join": join_case(streams[:16], max(1, min(st.rate // 10, n // 2)))}
del streams
print(json.dumps(result))
