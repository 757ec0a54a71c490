"""Timing and memory of Context.digest_streams (the CRC-32 of the decoded PCM of resident .lnn streams per bucket, nothing decoded into
memory) against what a user did before the call existed: index_streams + decode_windows into the WAV layout (dtype=int16,
channels_last=True) over the whole streams + a .cpu() copy + zlib.crc32 of every bucket's bytes on the host.  Two cases, each with
bucket_samples 0 (one bucket per stream) and 441 (10 ms):
  (a) BASELINE configs[1]'s stream: 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS;
  (b) 256 clips of 5 seconds of that shape, in one call.
The streams are encoded once on the device and stay resident.  Both forms run on this build -- the decode path is the parent
commit's, launch for launch, which the suite holds.  How every figure is taken -- the statistic, the repetitions, the peak device
memory of a call -- is tools/stream_timing.py's.  Kinds 83, 59, 79 and 80 are HIP events around
k_wx_digest, k_wx_place, k_wx_compare and k_wx_measure in a digest_windows, a decode_windows, a compare_windows and a measure_windows
call over the same windows (one pass each).  Prints one JSON line (profiles/stream_digest.json holds the MI355X's)."""
import zlib
import torch
import stream_timing as st
from stream_timing import verdict

args = st.arguments(reps=7)


def host_digest(pcm, b):
    """the recipe's table of one stream: [(crc32, bytes)] of an (n, C) int16 tensor on the host"""
    raw = memoryview(pcm.numpy()).cast("B")
    step = len(raw) if b == 0 else b * pcm.shape[1] * 2
    return [(zlib.crc32(raw[at:at + step]), len(raw[at:at + step])) for at in range(0, len(raw), step)]


def same(d, r):
    return [(int(x["crc32"]), int(x["num_bytes"])) for x in d.cpu()] == r


def case(streams, b):
    forms = {"digest_streams": lambda c: c.digest_streams(streams, bucket_samples=b),
             "recipe": st.recipe_of(streams, lambda g: host_digest(g.cpu(), b), dtype=torch.int16, channels_last=True)}

    def head(answers):
        return {"streams": len(streams), "bucket_samples": b, "buckets_per_stream": int(answers[0].crc32.shape[0])}

    def loops(ctx, wins, out):
        """kinds 83, 59, 79 and 80 over the same windows, one pass each"""
        def check(n):
            assert n(83) == 1 and n(59) == 0 and n(84) == 1 and n(85) == 1
        mine = (lambda: ctx.digest_windows(wins, bucket_samples=b), check,
                [(83, "kind_83_k_wx_digest"), (0, "digest_windows_device_ms"), (84, "kind_84_preset"), (85, "kind_85_commit")])
        return [[mine, st.decode_step(ctx, wins, 83), st.compare_step(ctx, wins, ctx.decode_windows(wins)), st.measure_step(ctx, wins, b)]]

    def per_sample(out, idx):
        samples = sum(x.header["num_channels"] * x.header["num_samples"] for x in idx)
        out["kind_83_ns_per_sample"] = round(out["kind_83_k_wx_digest"]["median_ms"] * 1e6 / samples, 6)

    def criteria(out, peaks):
        slack83 = max(out["kind_83_k_wx_digest"]["spread_ms"], out["kind_80_k_wx_measure"]["spread_ms"])
        return {
            "faster_than_the_recipe_beyond_the_spread": st.faster_than(out, "digest_streams"),
            "reported_kind_83_under_kind_80": verdict(out["kind_83_k_wx_digest"]["median_ms"] + slack83 < out["kind_80_k_wx_measure"]["median_ms"],
                                                      f"k_wx_digest {out['kind_83_k_wx_digest']['median_ms']} ms against k_wx_measure {out['kind_80_k_wx_measure']['median_ms']} ms (spread {slack83} ms); "
                                                      f"k_wx_place {out['kind_59_k_wx_place']['median_ms']} ms, k_wx_compare {out['kind_79_k_wx_compare']['median_ms']} ms"),
        }

    return st.case(streams, forms, head, same, loops, criteria, args.reps, decoded=("decoded_wav_bytes", 2), after=per_sample)


st.bucketed(args, case)
