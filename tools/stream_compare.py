"""Timing and memory of Context.verify_streams (resident .lnn streams compared with resident PCM, nothing decoded into memory)
against the recipe a user wrote before the call existed: index_streams + decode_windows over the whole streams + the torch conversion
of their PCM to int32 planar + torch.equal.  Two cases:
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS, against int32 planar PCM;
  (b) 256 clips of 5 seconds of that shape, against interleaved int16 PCM (a WAV file's data chunk).
The streams are encoded once on the device and stay resident.  The recipe comes in two forms: torch.equal per stream (one wait each)
and one torch.equal over everything (the conversions written into one flat buffer beside the one allocation decode_windows returns);
the criterion takes the faster.  Both run on this build -- the decode path of LINNEAmd_CompareWindowsDevice's commit is its parent's,
launch for launch, which the suite holds.  Every figure is the median of --reps runs after a warm-up, each run ending in a device
synchronise, the figures of a case taken in turn within a repetition; minimum and maximum beside the median, spread = max - min.
Peak device memory of a call = torch's peak allocation during it plus what the context's scratch grew by (free device memory before
and after, on a fresh context, less what torch's allocator reserved).  Kinds 79 and 59 are HIP events around k_wx_compare and
k_wx_place in a compare_windows and a decode_windows call over the same windows (one pass each).  Prints one JSON line
(profiles/stream_compare.json holds the MI355X's)."""
import json
import stream_timing as st                     # (first: it puts the repository's root on the path)
import torch
import linne_amd
from stream_timing import bits, block, dev, preset, rate, verdict

args = st.arguments()


def case(streams, pcms):
    """streams: uint8 device tensors; pcms: the PCM each should hold, (C, n) views of any dtype and strides"""
    pairs = list(zip(streams, pcms))
    decoded_bytes = sum(4 * p.shape[0] * p.shape[1] for p in pcms)
    flat = [None]

    def new(c):
        return c.verify_streams(pairs)

    def recipe(c):
        idx = c.index_streams(streams)
        got = c.decode_windows([(s, x, 0, None) for s, x in zip(streams, idx)])
        same = all(torch.equal(g, p if p.dtype == torch.int32 and p.is_contiguous() else p.to(torch.int32).contiguous()) for g, p in zip(got, pcms))
        for x in idx:
            x.close()
        return same

    def recipe_one_equal(c):
        idx = c.index_streams(streams)
        got = c.decode_windows([(s, x, 0, None) for s, x in zip(streams, idx)])
        mine = torch.empty(decoded_bytes // 4, dtype=torch.int32, device=dev)
        at = 0
        for p in pcms:
            k = p.shape[0] * p.shape[1]
            mine[at:at + k].view(p.shape[0], p.shape[1]).copy_(p)
            at += k
        theirs = torch.empty(0, dtype=torch.int32, device=dev).set_(got[0].untyped_storage())[:decoded_bytes // 4]
        same = torch.equal(mine, theirs)
        for x in idx:
            x.close()
        return same

    forms = {"verify_streams": new, "recipe_equal_per_stream": recipe, "recipe_one_equal": recipe_one_equal}
    out = {"streams": len(streams), "decoded_pcm_bytes": decoded_bytes, "pcm": f"{str(pcms[0].dtype).split('.')[-1]}, strides {tuple(pcms[0].stride())}"}
    answers, peaks = st.peak_memory(forms)
    out["answers"] = {"verify_streams_all_identical": all(a == (0, 0, 0, None) for a in answers["verify_streams"]),
                      "recipe_equal_per_stream": bool(answers["recipe_equal_per_stream"]), "recipe_one_equal": bool(answers["recipe_one_equal"])}
    out["peak_memory"] = peaks
    ctx = linne_amd.Context(0, use_torch_stream=True)
    out.update(st.repetitions(ctx, forms, args.reps))
    # kinds 79 and 59 over the same windows, one pass each
    idx = ctx.index_streams(streams)
    wins = st.whole(streams, idx)

    def check(n):
        assert n(79) == 1 and n(59) == 0
    held = [w + (p,) for w, p in zip(wins, pcms)]
    mine = (lambda: ctx.compare_windows(held), check, [(79, "kind_79_k_wx_compare"), (0, "compare_windows_device_ms")])
    ctx.enable_timing(True)
    out.update(st.kind_timings(ctx, [mine, st.decode_step(ctx, wins, 79)], args.reps))
    ctx.enable_timing(False)
    for x in idx:
        x.close()
    ctx.close()
    # the criteria
    best = min(("recipe_equal_per_stream", "recipe_one_equal"), key=lambda n: out[n]["median_ms"])
    slack = max(out["verify_streams"]["spread_ms"], out[best]["spread_ms"])
    saved = peaks[best]["peak_bytes"] - peaks["verify_streams"]["peak_bytes"]
    slack79 = max(out["kind_79_k_wx_compare"]["spread_ms"], out["kind_59_k_wx_place"]["spread_ms"])
    out["criteria"] = {
        "not_slower_than_the_recipe": verdict(out["verify_streams"]["median_ms"] <= out[best]["median_ms"] + slack,
                                              f"verify_streams {out['verify_streams']['median_ms']} ms against {best} {out[best]['median_ms']} ms (spread {slack} ms)"),
        "peak_memory_lower_by_about_the_decoded_pcm": verdict(saved >= 0.9 * decoded_bytes,
                                                              f"{peaks['verify_streams']['peak_bytes']} bytes against {best} {peaks[best]['peak_bytes']}: {saved} fewer, the decoded PCM is {decoded_bytes}"),
        "kind_79_not_slower_than_kind_59": verdict(out["kind_79_k_wx_compare"]["median_ms"] <= out["kind_59_k_wx_place"]["median_ms"] + slack79,
                                                   f"{out['kind_79_k_wx_compare']['median_ms']} ms against {out['kind_59_k_wx_place']['median_ms']} ms (spread {slack79} ms)"),
    }
    return out


result = st.preamble(args)
enc = linne_amd.Context(0, use_torch_stream=True)
x = st.track(int(args.minutes * 60 * rate), 3)
s = enc.encode_stream(x, bits, rate, block, preset, True).clone()
result["one_stream"] = dict(case([s], [x]), stream=st.one_stream_label(args) + ", int32 planar PCM")
del x, s
n = int(args.clip_seconds * rate)
clips = []
for t in range(args.clips):
    y = st.track(n, 100 + t)
    clips.append(y.to(torch.int16).T.contiguous().T)               # interleaved int16: channel stride 1, sample stride 2
streams = [t.clone() for t in enc.encode_streams([(p, bits, rate, block, preset, True) for p in clips])]
enc.close()
result["clips"] = dict(case(streams, clips), stream=st.clips_label(args) + ", interleaved int16 PCM")
print(json.dumps(result))
