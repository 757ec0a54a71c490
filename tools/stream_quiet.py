"""Timing and memory of Context.quiet_streams (the quiet runs of resident .lnn streams, nothing decoded into memory) against the
composition a user had before the call existed: index_streams + decode_windows (int32 planar) over the whole streams + torch
(abs() <= threshold, all over the channels, run extraction with diff and nonzero).  Two workloads, each with two settings --
threshold 0 / min_samples 1 (digital silence, every run) and 16 / 4410 (a musical setting: a tenth of a second within +-16):
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS;
  (b) 256 clips of 5 seconds of that shape, in one call.
Stretches of digital silence and of low-level noise (within +-8) are written into the PCM before it is encoded; `planted` records how
many and how long.  The streams are encoded once on the device and stay resident.  Both forms run on this build -- the decode path is
the parent commit's, launch for launch, which the suite holds.  How every figure is taken -- the statistic, the repetitions, the peak
device memory of a call -- is tools/stream_timing.py's.  Kinds 86, 59 and 79 are HIP events around
k_wx_quiet, k_wx_place and k_wx_compare in a quiet_windows, a decode_windows and a compare_windows call over the same windows (one
pass each); kinds 87 to 91 are the quiet call's preset and commit stage, in a call whose tables hold every run.  quiet_streams itself is
timed as a user calls it, without a capacity: the streams of more runs than the default are asked once more.  Prints one JSON line
(profiles/stream_quiet.json holds the MI355X's)."""
import json
import stream_timing as st                     # (first: it puts the repository's root on the path)
import torch
import linne_amd
from stream_timing import rate, verdict

args = st.arguments()
SETTINGS = {"threshold_0_min_1": (0, 1), "threshold_16_min_4410": (16, 4410)}


def plant(x, seed, every, lengths):
    """stretches of digital silence and of noise within +-8, alternately, every `every` samples, of the lengths given in turn ->
    what was planted"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n, done = x.shape[1], {"silence": [], "noise": []}
    for k, at in enumerate(range(every // 2, n, every)):
        m = min(lengths[k % len(lengths)], n - at)
        if k % 2 == 0:
            x[:, at:at + m] = 0
            done["silence"].append(m)
        else:
            x[:, at:at + m] = torch.randint(-8, 9, (x.shape[0], m), generator=g, dtype=torch.int32).to(x.device)
            done["noise"].append(m)
    return {kind: {"stretches": len(v), "samples": int(sum(v)), "shortest": min(v, default=0), "longest": max(v, default=0)} for kind, v in done.items()}


def torch_runs(pcm, thr, mn):
    """the composition's table of one stream: (k, 2) int64 of (first, length)"""
    q = (pcm.abs() <= thr).all(dim=0).to(torch.int8)
    zero = torch.zeros(1, dtype=torch.int8, device=pcm.device)
    edge = torch.diff(q, prepend=zero, append=zero)
    starts, ends = (edge == 1).nonzero().squeeze(1), (edge == -1).nonzero().squeeze(1)
    keep = (ends - starts) >= mn
    return torch.stack([starts[keep], (ends - starts)[keep]], dim=1)


def same(q, r):
    return q.num_runs == r.shape[0] and torch.equal(q.runs, r)


def case(streams, thr, mn):
    # (capacity None: a second call for the streams of more runs than the default)
    forms = {"quiet_streams": lambda c: c.quiet_streams(streams, thr, min_samples=mn), "recipe": st.recipe_of(streams, lambda g: torch_runs(g, thr, mn))}

    def head(answers):
        return {"streams": len(streams), "threshold": thr, "min_samples": mn, "runs": int(sum(q.num_runs for q in answers)),
                "quiet_samples": int(sum(q.quiet_samples for q in answers)), "most_runs_in_a_stream": int(max(q.num_runs for q in answers))}

    def loops(ctx, wins, out):
        """kinds 86, 59 and 79 over the same windows, one pass each; the quiet call's preset and commit stage"""
        def check(n):
            assert n(86) == 1 and n(59) == 0 and all(n(k) == 1 for k in (87, 88, 89, 90, 91))
        cap = max(out["most_runs_in_a_stream"], 1)                   # one call in which every run fits
        mine = (lambda: ctx.quiet_windows(wins, thr, mn, capacity=cap), check,
                [(86, "kind_86_k_wx_quiet"), (0, "quiet_windows_device_ms"), (87, "kind_87_preset"), (88, "kind_88_count"), (89, "kind_89_scan"), (90, "kind_90_starts"),
                 (91, "kind_91_ends"), ((88, 89, 90, 91), "commit_stage_kinds_88_to_91")])
        return [[mine, st.decode_step(ctx, wins, 86), st.compare_step(ctx, wins, ctx.decode_windows(wins))]]

    def criteria(out, peaks):
        return {
            "faster_than_the_composition_beyond_the_spread": st.faster_than(out, "quiet_streams", "composition"),
            "peak_memory_below_the_composition": verdict(peaks["quiet_streams"]["peak_bytes"] < peaks["recipe"]["peak_bytes"],
                                                         f"{peaks['quiet_streams']['peak_bytes']} bytes against {peaks['recipe']['peak_bytes']}; the decoded PCM is {out['decoded_pcm_bytes']}"),
        }

    return st.case(streams, forms, head, same, loops, criteria, args.reps)


result = st.preamble(args)
enc = linne_amd.Context(0, use_torch_stream=True)
s, planted = st.one_stream(enc, args, lambda x: plant(x, 1, 20 * rate, [2 * rate, 300, 5 * rate, 4410, 64, rate // 2]))
result["one_stream"] = {"stream": st.one_stream_label(args), "planted": planted}
result["one_stream"].update({name: case([s], thr, mn) for name, (thr, mn) in SETTINGS.items()})
del s
streams, planted = st.clips(enc, args, lambda p, seed: plant(p, seed, rate, [rate // 4, 4410, 100, rate // 2]))
enc.close()
result["clips"] = {"stream": st.clips_label(args),
                   "planted": {kind: {"stretches": sum(p[kind]["stretches"] for p in planted), "samples": sum(p[kind]["samples"] for p in planted)} for kind in ("silence", "noise")}}
result["clips"].update({name: case(streams, thr, mn) for name, (thr, mn) in SETTINGS.items()})
print(json.dumps(result))
