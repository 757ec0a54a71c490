"""Timing and memory of Context.resample_windows (a rational rate change through an exact int16 polyphase FIR between the samples of
resident .lnn streams and the PCM they are decoded into) and of Context.resample_streams (the same, encoded again into new streams)
against the recipes a user wrote before the calls existed: index_streams + decode_windows (int32 planar) over the whole streams + torch
-- the float64 widening, one strided conv1d per phase, the rounding shift, the clamp and the conversion -- and decode_stream + that +
encode_stream.  The recipe is exact for these 16-bit streams (a sum stays far under 2^53), so the two answers must be equal.  The cases:
  (a) BASELINE configs[1]'s stream, 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS, to 16 kHz (160/441) and to 48 kHz
      (160/147): int32;
  (b) 256 clips of 5 seconds of that shape, in one call, to 16 kHz float32 channels_last (the form of a training batch);
  (c) resample_streams on (a)'s stream, to 16 kHz.
The filters are LINNEAmd_ResampleDesign's, 32 taps per phase.  The streams are encoded once on the device and stay resident.  How every
figure is taken -- the statistic, the repetitions, the peak device memory of a call -- is tools/stream_timing.py's.  Kinds 100, 99 and
59 are HIP events around k_wx_resample, k_wx_resample_preset and k_wx_place in a resample_windows call of the case's ratio; kind 100 is
also taken at 1/1 with one tap of 1 (the floor: k_wx_place of a decode_windows call over the same windows writes the same bytes) and
at 1/1 with 32 taps.  Prints one JSON line (profiles/stream_resample.json holds the MI355X's)."""
import json
import math
import numpy as np
import torch
import stream_timing as st                # (puts the repository's root on the path)
import linne_amd
from stream_timing import verdict

args = st.arguments(reps=7)
TAPS = 32
LO, HI = -(1 << (st.bits - 1)), (1 << (st.bits - 1)) - 1
ONE = np.array([[1]], dtype=np.int16)
FLAT, FLAT_SHIFT, FLAT_BEFORE = linne_amd.resample_design(1, 1, TAPS)


def torch_resample(g, coef, up, down, before, shift, float32, channels_last):
    """the recipe's resampling of one decoded stream (C, N) int32: per phase p the outputs m with (m * down) % up == p lie up / gcd
    apart and read the input down / gcd apart -- one float64 conv1d with that stride --, then the shift, the clamp, the conversion"""
    C, N = g.shape
    P = coef.shape[1]
    n_out = -(-N * up // down)
    q = math.gcd(up, down)
    Lp, Mp = up // q, down // q
    last = (n_out - 1) * down // up
    x = torch.zeros((C, 1, before + last + P + Mp), dtype=torch.float64, device=g.device)   # stream sample s at before + s: zeros around it
    x[:, 0, before:before + N] = g
    k = torch.from_numpy(coef.astype(np.float64)).to(g.device)
    y = torch.empty((C, n_out), dtype=torch.int64, device=g.device)
    for m0 in range(min(Lp, n_out)):
        p, n0 = (m0 * down) % up, (m0 * down) // up
        cnt = len(range(m0, n_out, Lp))
        r = torch.nn.functional.conv1d(x[:, :, n0:n0 + (cnt - 1) * Mp + P], k[p].view(1, 1, P), stride=Mp)
        y[:, m0::Lp] = r[:, 0, :].to(torch.int64)
    if shift:
        y = (y + (1 << (shift - 1))) >> shift
    y.clamp_(LO, HI)
    y = y.to(torch.float32).mul_(2.0 ** -(st.bits - 1)) if float32 else y.to(torch.int32)
    return y.t().contiguous() if channels_last else y


def resample_case(streams, up, down, float32, channels_last):
    coef, shift, before = linne_amd.resample_design(up, down, TAPS)
    kw = {"dtype": torch.float32 if float32 else torch.int32, "channels_last": channels_last}

    def call(c, wins):
        return c.resample_windows(wins, up, down, coef=coef, before=before, shift=shift, clip_bits=st.bits, **kw)

    def resampled(c):
        idx = c.index_streams(streams)
        got = call(c, st.whole(streams, idx))
        for x in idx:
            x.close()
        return got
    forms = {"resample_windows": resampled,
             "recipe": st.recipe_of(streams, lambda g: torch_resample(g, coef, up, down, before, shift, float32, channels_last))}

    def head(answers):
        return {"streams": len(streams), "ratio": f"{up}/{down}", "taps": TAPS, "shift": shift,
                "output": ("float32" if float32 else "int32") + (", channels_last" if channels_last else ""), "output_bytes": sum(a.numel() * 4 for a in answers)}

    def loops(ctx, wins, out):
        """kinds 100, 99 and 59 of the case's call; kind 100 at 1/1 with one tap and with 32; kind 59 of the decode call, one pass each"""
        def check(n):
            assert n(100) == 1 and n(99) == 1 and n(59) == 1
        mine = (lambda: call(ctx, wins), check, [(100, "kind_100_k_wx_resample"), (99, "kind_99_k_wx_resample_preset"), (59, "kind_59_k_wx_place_into_the_images"), (0, "resample_windows_device_ms")])
        floor = (lambda: ctx.resample_windows(wins, 1, 1, coef=ONE), check, [(100, "kind_100_identity_1_tap")])
        flat = (lambda: ctx.resample_windows(wins, 1, 1, coef=FLAT, before=FLAT_BEFORE, shift=FLAT_SHIFT, clip_bits=st.bits), check, [(100, "kind_100_identity_32_taps")])
        return [[mine, floor, flat, st.decode_step(ctx, wins, 100)]]

    def criteria(out, peaks):
        k59, one, flat = out["kind_59_k_wx_place"], out["kind_100_identity_1_tap"], out["kind_100_identity_32_taps"]
        return {
            "faster_than_the_recipe_beyond_the_spread": st.faster_than(out, "resample_windows"),
            "lower_peak_memory_than_the_recipe": verdict(peaks["resample_windows"]["peak_bytes"] < peaks["recipe"]["peak_bytes"],
                                                         f"{peaks['resample_windows']['peak_bytes']} bytes against the recipe's {peaks['recipe']['peak_bytes']}; the decoded PCM is {out['decoded_pcm_bytes']}"),
            "above_the_floor": f"k_wx_resample at 1/1 with one tap {one['median_ms']} ms, k_wx_place on the same windows {k59['median_ms']} ms: {round(one['median_ms'] / max(k59['median_ms'], 1e-6), 2)} times the floor",
            "32_taps_against_1": f"k_wx_resample at 1/1 with 32 taps {flat['median_ms']} ms, with one {one['median_ms']} ms: {round(flat['median_ms'] / max(one['median_ms'], 1e-6), 2)} times",
        }

    return st.case(streams, forms, head, lambda a, r: bool(torch.equal(a, r)), loops, criteria, args.reps)


def streams_case(s, rate):
    """resample_streams against decode_stream + torch + encode_stream: the encode dominates both"""
    up, down = linne_amd.resample_ratio(st.rate, rate)
    coef, shift, before = linne_amd.resample_design(up, down, TAPS)

    def recipe(c):
        y = torch_resample(c.decode_stream(s), coef, up, down, before, shift, False, False)
        return [c.encode_stream(y, st.bits, rate, st.block, st.preset, True)]
    forms = {"resample_streams": lambda c: c.resample_streams([s], rate), "recipe": recipe}
    answers, peaks = st.peak_memory(forms)
    out = {"rate": rate, "answers_equal": bool(torch.equal(answers["resample_streams"][0], answers["recipe"][0])), "stream_bytes": int(answers["recipe"][0].numel()), "peak_memory": peaks}
    del answers
    ctx = linne_amd.Context(0, use_torch_stream=True)
    out.update(st.repetitions(ctx, forms, args.reps))
    ctx.close()
    slack = max(out["resample_streams"]["spread_ms"], out["recipe"]["spread_ms"])
    out["criteria"] = {
        "not_slower_than_the_recipe_beyond_the_spread": verdict(out["resample_streams"]["median_ms"] <= out["recipe"]["median_ms"] + slack,
                                                                f"resample_streams {out['resample_streams']['median_ms']} ms against the recipe's {out['recipe']['median_ms']} ms (spread {slack} ms)"),
        "lower_peak_memory_than_the_recipe": verdict(peaks["resample_streams"]["peak_bytes"] < peaks["recipe"]["peak_bytes"], f"{peaks['resample_streams']['peak_bytes']} bytes against the recipe's {peaks['recipe']['peak_bytes']}"),
    }
    return out


result = st.preamble(args)
enc = linne_amd.Context(0, use_torch_stream=True)
s, _ = st.one_stream(enc, args)
result["one_stream"] = {"stream": st.one_stream_label(args), "to_16000_int32": resample_case([s], 160, 441, False, False), "to_48000_int32": resample_case([s], 160, 147, False, False),
                        "streams_to_16000": streams_case(s, 16000)}
del s
streams, _ = st.clips(enc, args)
enc.close()
result["clips"] = {"stream": st.clips_label(args), "to_16000_float32_channels_last": resample_case(streams, 160, 441, True, True)}
del streams
print(json.dumps(result))
