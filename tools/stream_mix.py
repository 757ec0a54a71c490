"""Timing and memory of Context.mix_windows (an exact integer channel matrix between the samples of resident .lnn streams and the PCM they
are decoded into) and of Context.remix_streams (the same, encoded again into new streams) against the recipes a user wrote before the
calls existed: index_streams + decode_windows (int32 planar) over the whole streams + torch -- the int64 widening, the sum over the
channels, the rounding shift, the clamp and the conversion -- and decode_stream + that + encode_stream.  The cases:
  (a) BASELINE configs[1]'s stream, 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS, to its mono mean: int32, and float32;
  (b) 256 clips of 5 seconds of that shape, in one call, to mono float32 channels_last (the form of a training batch);
  (c) remix_streams on (a)'s stream.
The streams are encoded once on the device and stay resident.  Both forms run on this build -- the decode path is the parent commit's,
launch for launch, which the suite holds.  How every figure is taken -- the statistic, the repetitions, the peak device memory of a
call -- is tools/stream_timing.py's.  Kinds 98 and 59 are HIP events around k_wx_mix and k_wx_place in a mix_windows and a
decode_windows call over the same windows (one pass each), for the identity of the stream's channels, for the mono mean, and -- on a
stream of eight channels a quarter as long -- for the identity of eight.  Prints one JSON line (profiles/stream_mix.json holds the
MI355X's)."""
import json
import torch
import stream_timing as st                # (puts the repository's root on the path)
import linne_amd
from bench import synth_track
from stream_timing import verdict

args = st.arguments(reps=7)
MEAN, SHIFT = linne_amd.downmix_matrix(2)
LO, HI = -(1 << (st.bits - 1)), (1 << (st.bits - 1)) - 1


def torch_mean(g, float32, channels_last):
    """the recipe's mono mean of one decoded stream (2, n) int32: widened, summed, shifted with halves rounded up, clamped, converted"""
    y = ((g.to(torch.int64).sum(0, keepdim=True) + (1 << (SHIFT - 1))) >> SHIFT).clamp_(LO, HI)
    y = y.to(torch.float32).mul_(2.0 ** -(st.bits - 1)) if float32 else y.to(torch.int32)
    return y.t().contiguous() if channels_last else y


def mix_case(streams, float32, channels_last):
    kw = {"dtype": torch.float32 if float32 else torch.int32, "channels_last": channels_last}
    def mixed(c):
        idx = c.index_streams(streams)
        got = c.mix_windows(st.whole(streams, idx), MEAN, shift=SHIFT, clip_bits=st.bits, **kw)
        for x in idx:
            x.close()
        return got
    forms = {"mix_windows": mixed,
             "recipe": st.recipe_of(streams, lambda g: torch_mean(g, float32, channels_last))}

    def head(answers):
        return {"streams": len(streams), "output": ("float32" if float32 else "int32") + (", channels_last" if channels_last else ""), "output_bytes": sum(a.numel() * 4 for a in answers)}

    def loops(ctx, wins, out):
        """kinds 98 and 59 over the same windows, one pass each: the identity of the stream's channels, and the mono mean"""
        def check(n):
            assert n(98) == 1 and n(59) == 0
        C = wins[0][1].header["num_channels"]
        eye = torch.eye(C, dtype=torch.int64).numpy()
        identity = (lambda: ctx.mix_windows(wins, eye), check, [(98, "kind_98_k_wx_mix_identity")])
        mono = (lambda: ctx.mix_windows(wins, MEAN, shift=SHIFT, clip_bits=st.bits, **kw), check, [(98, "kind_98_k_wx_mix_mono"), (0, "mix_windows_device_ms")])
        return [[identity, mono, st.decode_step(ctx, wins, 98)]]

    def criteria(out, peaks):
        k59, ident, mono = out["kind_59_k_wx_place"], out["kind_98_k_wx_mix_identity"], out["kind_98_k_wx_mix_mono"]
        slack = max(k59["spread_ms"], ident["spread_ms"], mono["spread_ms"])
        return {
            "faster_than_the_recipe_beyond_the_spread": st.faster_than(out, "mix_windows"),
            "lower_peak_memory_than_the_recipe": verdict(peaks["mix_windows"]["peak_bytes"] < peaks["recipe"]["peak_bytes"],
                                                         f"{peaks['mix_windows']['peak_bytes']} bytes against the recipe's {peaks['recipe']['peak_bytes']}; the decoded PCM is {out['decoded_pcm_bytes']}"),
            "identity_not_slower_than_kind_59_(a_guess)": verdict(ident["median_ms"] <= k59["median_ms"] + slack, f"k_wx_mix {ident['median_ms']} ms against k_wx_place {k59['median_ms']} ms (spread {slack} ms)"),
            "mono_faster_than_kind_59_(a_guess)": verdict(mono["median_ms"] + slack < k59["median_ms"], f"k_wx_mix {mono['median_ms']} ms against k_wx_place {k59['median_ms']} ms (spread {slack} ms)"),
        }

    return st.case(streams, forms, head, lambda a, r: bool(torch.equal(a, r)), loops, criteria, args.reps)


def eight_channels(enc):
    """kinds 98 and 59 on the identity of eight channels: a stream a quarter as long as (a)'s"""
    n = max(int(args.minutes * 60 * st.rate) // 4, 4 * st.block)
    s = enc.encode_stream(synth_track(n, 8, st.bits, 5, st.dev, rate=float(st.rate)), st.bits, st.rate, st.block, st.preset, False).clone()
    ctx = linne_amd.Context(0, use_torch_stream=True)
    idx = ctx.index_streams([s])
    wins = st.whole([s], idx)
    eye = torch.eye(8, dtype=torch.int64).numpy()
    out = {"stream": f"8 channels, {n} samples", "answers_equal": bool(torch.equal(ctx.mix_windows(wins, eye)[0], ctx.decode_windows(wins)[0]))}

    def check(n):
        assert n(98) == 1 and n(59) == 0
    ctx.enable_timing(True)
    out.update(st.kind_timings(ctx, [(lambda: ctx.mix_windows(wins, eye), check, [(98, "kind_98_k_wx_mix_identity")]), st.decode_step(ctx, wins, 98, [(59, "kind_59_k_wx_place")])], args.reps))
    ctx.enable_timing(False)
    for x in idx:
        x.close()
    ctx.close()
    k59, ident = out["kind_59_k_wx_place"], out["kind_98_k_wx_mix_identity"]
    slack = max(k59["spread_ms"], ident["spread_ms"])
    out["criteria"] = {"identity_not_slower_than_kind_59_(a_guess)": verdict(ident["median_ms"] <= k59["median_ms"] + slack, f"k_wx_mix {ident['median_ms']} ms against k_wx_place {k59['median_ms']} ms (spread {slack} ms)")}
    return out


def remix_case(s):
    """remix_streams against decode_stream + torch + encode_stream: the encode dominates both; the row is about peak memory"""
    def recipe(c):
        y = torch_mean(c.decode_stream(s), False, False)
        return [c.encode_stream(y, st.bits, st.rate, st.block, st.preset, False)]
    forms = {"remix_streams": lambda c: c.remix_streams([s], MEAN, shift=SHIFT), "recipe": recipe}
    answers, peaks = st.peak_memory(forms)
    out = {"answers_equal": bool(torch.equal(answers["remix_streams"][0], answers["recipe"][0])), "stream_bytes": int(answers["recipe"][0].numel()), "peak_memory": peaks}
    del answers
    ctx = linne_amd.Context(0, use_torch_stream=True)
    out.update(st.repetitions(ctx, forms, args.reps))
    ctx.close()
    slack = max(out["remix_streams"]["spread_ms"], out["recipe"]["spread_ms"])
    out["criteria"] = {
        "not_slower_than_the_recipe_beyond_the_spread": verdict(out["remix_streams"]["median_ms"] <= out["recipe"]["median_ms"] + slack,
                                                                f"remix_streams {out['remix_streams']['median_ms']} ms against the recipe's {out['recipe']['median_ms']} ms (spread {slack} ms)"),
        "lower_peak_memory_than_the_recipe": verdict(peaks["remix_streams"]["peak_bytes"] < peaks["recipe"]["peak_bytes"], f"{peaks['remix_streams']['peak_bytes']} bytes against the recipe's {peaks['recipe']['peak_bytes']}"),
    }
    return out


result = st.preamble(args)
enc = linne_amd.Context(0, use_torch_stream=True)
s, _ = st.one_stream(enc, args)
result["one_stream"] = {"stream": st.one_stream_label(args), "mono_int32": mix_case([s], False, False), "mono_float32": mix_case([s], True, False), "remix": remix_case(s)}
del s
streams, _ = st.clips(enc, args)
result["clips"] = {"stream": st.clips_label(args), "mono_float32_channels_last": mix_case(streams, True, True)}
del streams
result["eight_channels"] = eight_channels(enc)
enc.close()
print(json.dumps(result))
