"""Timing and memory of Context.relate_streams (per channel pair and bucket the exact sum of a_i * a_j and the counts of equal and of
opposite frames of resident .lnn streams, nothing decoded into memory) against the recipe a user wrote before the call existed:
index_streams + decode_windows (int32 planar) over the whole streams + the torch reductions that give the same numbers (per pair the
int64 sum of the int64 products and the two counts -- exact for 16-bit material; the library's sum is 128 bits wide).  Two cases, each
with bucket_samples 0 (one bucket per stream) and 441 (10 ms):
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS;
  (b) 256 clips of 5 seconds of that shape, in one call.
The streams are encoded once on the device and stay resident.  Both forms run on this build -- the decode path is the parent
commit's, launch for launch, which the suite holds.  How every figure is taken -- the statistic, the repetitions, the peak device
memory of a call -- is tools/stream_timing.py's.  Kinds 95, 80 and 59 are HIP events around k_wx_relate,
k_wx_measure and k_wx_place in a relate_windows, a measure_windows and a decode_windows call over the same windows (one pass each);
k_wx_measure and k_wx_place are the parent commit's kernels, unchanged.  Prints one JSON line (profiles/stream_relate.json holds
the MI355X's; profiles/stream_relate_wide_fold.json the same run on a library built with -DWXR_NARROW=0, where every wave folds the
products as (lo, hi))."""
import torch
import stream_timing as st
from stream_timing import verdict

args = st.arguments()


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
    forms = {"relate_streams": lambda c: c.relate_streams(streams, bucket_samples=b), "recipe": st.recipe_of(streams, lambda g: torch_relate(g, b))}

    def head(answers):
        return {"streams": len(streams), "bucket_samples": b, "buckets_per_stream": int(answers[0].records.shape[1])}

    def loops(ctx, wins, out):
        """kinds 95, 80 and 59 over the same windows, one pass each"""
        def check(n):
            assert n(95) == 1 and n(59) == 0 and n(96) == 1 and n(97) == 1
        mine = (lambda: ctx.relate_windows(wins, bucket_samples=b), check,
                [(95, "kind_95_k_wx_relate"), (0, "relate_windows_device_ms"), (96, "kind_96_preset"), (97, "kind_97_commit")])
        return [[mine, st.measure_step(ctx, wins, b, 95, [(80, "kind_80_k_wx_measure"), (0, "measure_windows_device_ms")]), st.decode_step(ctx, wins, 95)]]

    def criteria(out, peaks):
        slack95 = max(out["kind_95_k_wx_relate"]["spread_ms"], out["kind_80_k_wx_measure"]["spread_ms"])
        return {
            "faster_than_the_recipe_beyond_the_spread": st.faster_than(out, "relate_streams"),
            "peak_memory": f"{peaks['relate_streams']['peak_bytes']} bytes against the recipe's {peaks['recipe']['peak_bytes']}; the decoded PCM is {out['decoded_pcm_bytes']}",
            "kind_95_not_slower_than_kind_80": verdict(out["kind_95_k_wx_relate"]["median_ms"] <= out["kind_80_k_wx_measure"]["median_ms"] + slack95,
                                                       f"{out['kind_95_k_wx_relate']['median_ms']} ms against {out['kind_80_k_wx_measure']['median_ms']} ms (spread {slack95} ms); k_wx_place {out['kind_59_k_wx_place']['median_ms']} ms"),
        }

    return st.case(streams, forms, head, same, loops, criteria, args.reps)


st.bucketed(args, case)
