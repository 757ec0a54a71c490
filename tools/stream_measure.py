"""Timing and memory of Context.measure_streams (min, max, sum and sum of squares of resident .lnn streams per channel and bucket,
nothing decoded into memory) against the recipe a user wrote before the call existed: index_streams + decode_windows (int32 planar)
over the whole streams + the torch reductions that give the same numbers (amin, amax, the int64 sum, the int64 sum of squares -- enough
for 16-bit material; the library's is 128 bits wide).  Two cases, each with bucket_samples 0 (one bucket per stream) and 441 (10 ms):
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS;
  (b) 256 clips of 5 seconds of that shape, in one call.
The streams are encoded once on the device and stay resident.  Both forms run on this build -- the decode path is the parent
commit's, launch for launch, which the suite holds.  Every figure is the median of --reps runs after a warm-up, each run ending in a
device synchronise, the forms of a case taken in turn within a repetition; minimum and maximum beside the median, spread = max -
min.  Peak device memory of a call = torch's peak allocation during it plus what the context's scratch grew by (free device memory
before and after, on a fresh context, less what torch's allocator reserved).  Kinds 80, 59 and 79 are HIP events around k_wx_measure,
k_wx_place and k_wx_compare in a measure_windows, a decode_windows and a compare_windows call over the same windows (one pass
each).  Prints one JSON line (profiles/stream_measure.json holds the MI355X's)."""
import torch
import stream_timing as st
from stream_timing import verdict

args = st.arguments()


def reduce4(x):
    """(min, max, sum, sum of squares) over the last dimension of an int32 tensor, int64 each"""
    w = x.to(torch.int64)
    return torch.stack([x.amin(-1).to(torch.int64), x.amax(-1).to(torch.int64), w.sum(-1), (w * w).sum(-1)], dim=-1)


def torch_measure(pcm, b):
    """the recipe's table of one stream: (C, nb, 4) int64"""
    n = pcm.shape[1]
    if b == 0 or b >= n:
        return reduce4(pcm).unsqueeze(1)
    full = n // b
    parts = [reduce4(pcm[:, :full * b].view(pcm.shape[0], full, b))]
    if n % b:
        parts.append(reduce4(pcm[:, full * b:]).unsqueeze(1))
    return torch.cat(parts, dim=1)


def same(m, r):
    """a Measurement against the recipe's table (the high word must be 0: the recipe's sum of squares is 64 bits wide)"""
    return bool(torch.equal(m.min.to(torch.int64), r[..., 0]) and torch.equal(m.max.to(torch.int64), r[..., 1]) and torch.equal(m.sum, r[..., 2])
                and torch.equal(m.sumsq_lo, r[..., 3]) and not bool(m.sumsq_hi.any()))


def case(streams, b):
    forms = {"measure_streams": lambda c: c.measure_streams(streams, bucket_samples=b), "recipe": st.recipe_of(streams, lambda g: torch_measure(g, b))}

    def head(answers):
        return {"streams": len(streams), "bucket_samples": b, "buckets_per_stream": int(answers[0].min.shape[1])}

    def loops(ctx, wins, out):
        """kinds 80, 59 and 79 over the same windows, one pass each"""
        def check(n):
            assert n(80) == 1 and n(59) == 0 and n(81) == 1 and n(82) == 1
        mine = (lambda: ctx.measure_windows(wins, bucket_samples=b), check,
                [(80, "kind_80_k_wx_measure"), (0, "measure_windows_device_ms"), (81, "kind_81_preset"), (82, "kind_82_commit")])
        return [[mine, st.decode_step(ctx, wins, 80), st.compare_step(ctx, wins, ctx.decode_windows(wins))]]

    def criteria(out, peaks):
        saved = peaks["recipe"]["peak_bytes"] - peaks["measure_streams"]["peak_bytes"]
        decoded_bytes = out["decoded_pcm_bytes"]
        slack80 = max(out["kind_80_k_wx_measure"]["spread_ms"], out["kind_59_k_wx_place"]["spread_ms"])
        return {
            "faster_than_the_recipe_beyond_the_spread": st.faster_than(out, "measure_streams"),
            "peak_memory_lower_by_about_the_decoded_pcm": verdict(saved >= 0.9 * decoded_bytes,
                                                                  f"{peaks['measure_streams']['peak_bytes']} bytes against {peaks['recipe']['peak_bytes']}: {saved} fewer, the decoded PCM is {decoded_bytes}"),
            "kind_80_not_slower_than_kind_59": verdict(out["kind_80_k_wx_measure"]["median_ms"] <= out["kind_59_k_wx_place"]["median_ms"] + slack80,
                                                       f"{out['kind_80_k_wx_measure']['median_ms']} ms against {out['kind_59_k_wx_place']['median_ms']} ms (spread {slack80} ms); k_wx_compare {out['kind_79_k_wx_compare']['median_ms']} ms"),
        }

    return st.case(streams, forms, head, same, loops, criteria, args.reps)


st.bucketed(args, case)
