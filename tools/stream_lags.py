"""Timing and memory of Context.lag_windows (per channel pair and lag the exact sums of a * b and of b^2 under a needle slid over a
resident .lnn stream, nothing decoded into memory) against the recipe a user wrote before the call existed: index_streams +
decode_windows (int32 planar) of the needle and of the haystack range + torch.  Two exact torch formulations are timed and the faster
is the recipe, named in the result: the int64 product of the needle with an `unfold` view of the haystack, in chunks of --unfold-lags
lags (the whole view at once is lags * n * 8 bytes), and float64 `conv1d`, exact for 16-bit material (a sum of 2^18 products of 2^30
stays under 2^53).  Cases:
  (a) BASELINE configs[1]'s stream, 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS: a 5-second needle from its middle
      against the stream itself at +-4096 lags and at +-32768 lags;
  (b) 256 clips of 5 seconds of that shape, each whole clip against its neighbour at +-4096 lags, in one call.
Both channels (pairs (0, 0) and (1, 1)).  How every figure is taken -- the statistic, the repetitions, the peak device memory of a
call -- is tools/stream_timing.py's.  Kinds 102, 103 and 59 are HIP events around k_wx_lags, k_wx_lags_commit and k_wx_place in one
lag_windows call; the multiply-adds per second of kind 102 are the products the call counts (n * lags * pairs) over its median, beside
the lane rate the clock gives (CUs * 64 lanes * 4 SIMDs * --clock-mhz, 2400 unless given: what one 32-bit multiply-add per lane and cycle would be; the 64-bit
multiply-add's issue rate is NOT measured here, so the figure is no share of a peak).  Prints one JSON line (profiles/stream_lags.json
holds the MI355X's; profiles/stream_lags_plain_loop.json the same run on a library built with -DWXL_BLOCK=1, the plain inner loop;
profiles/stream_lags_all_wide.json with -DWXL_NARROW=0, where every sub-tile sums as (lo, hi))."""
import json
import sys

import torch
import stream_timing as st
import linne_amd


def arguments():
    # stream_timing's parser, with this tool's own options taken out in front of it; --cases first: the one stream at +-lags alone
    own = {"--needle-seconds": 5.0, "--unfold-lags": 256, "--wide-lags": 32768, "--lags": 4096, "--cases": "all", "--clock-mhz": 2400.0}
    vals = {}
    for k, d in own.items():
        if k in sys.argv:
            i = sys.argv.index(k)
            vals[k] = type(d)(sys.argv[i + 1])
            del sys.argv[i:i + 2]
        else:
            vals[k] = d
    a = st.arguments(label="default build")
    a.needle_seconds, a.unfold_lags, a.wide_lags, a.lags, a.cases = vals["--needle-seconds"], vals["--unfold-lags"], vals["--wide-lags"], vals["--lags"], vals["--cases"]
    a.clock_mhz = vals["--clock-mhz"]                          # (the MI355X's peak engine clock, 2400 MHz, unless given: torch does not report one)
    return a


args = arguments()
PAIRS = [(0, 0), (1, 1)]


def torch_unfold(a, h, num_lags):
    """int64: (C, num_lags) dots, in chunks of lags"""
    n, a64, h64 = a.shape[1], a.to(torch.int64), h.to(torch.int64)
    out = torch.empty((a.shape[0], num_lags), dtype=torch.int64, device=a.device)
    for l0 in range(0, num_lags, args.unfold_lags):
        l1 = min(l0 + args.unfold_lags, num_lags)
        view = h64[:, l0:l1 - 1 + n].unfold(1, n, 1)                # (C, lags, n)
        out[:, l0:l1] = (view * a64[:, None, :]).sum(-1)
    return out


def torch_conv(a, h, num_lags):
    """float64 conv1d, a channel per group: exact while the sums stay under 2^53"""
    y = torch.nn.functional.conv1d(h.to(torch.float64)[None], a.to(torch.float64)[:, None, :], groups=a.shape[0])[0]
    assert y.shape[1] == num_lags
    return y.to(torch.int64)


def squares(a, h, num_lags):
    n, h64 = a.shape[1], h.to(torch.int64)
    cs = torch.cat([torch.zeros((h.shape[0], 1), dtype=torch.int64, device=h.device), torch.cumsum(h64 * h64, 1)], 1)
    return cs[:, n:n + num_lags] - cs[:, :num_lags], (a.to(torch.int64) ** 2).sum(1)


def recipe_of(jobs, dots):
    """jobs: (stream_a, first_a, n, stream_b, first_b, lag_first, num_lags) -> per job (dots (C, L), b_sq (C, L), a_sq (C)), int64"""
    def recipe(c):
        streams = [s for j in jobs for s in (j[0], j[3])]
        idx = c.index_streams(streams)
        wins = []
        for k, (sa, fa, n, sb, fb, lf, L) in enumerate(jobs):
            N = idx[2 * k + 1].header["num_samples"]
            lo, hi = max(fb + lf, 0), min(fb + lf + L - 1 + n, N)
            wins += [(sa, idx[2 * k], fa, n), (sb, idx[2 * k + 1], lo, max(hi - lo, 0))]
        got = c.decode_windows(wins)
        out = []
        for k, (sa, fa, n, sb, fb, lf, L) in enumerate(jobs):
            a, part = got[2 * k], got[2 * k + 1]
            lo = max(fb + lf, 0)
            h = torch.zeros((part.shape[0], L - 1 + n), dtype=part.dtype, device=part.device)     # zeros where the stream has no samples
            h[:, lo - (fb + lf):lo - (fb + lf) + part.shape[1]] = part
            b_sq, a_sq = squares(a, h, L)
            out.append((dots(a, h, L), b_sq, a_sq))
        for x in idx:
            x.close()
        return out
    return recipe


def call_of(jobs):
    def call(c):
        streams = [s for j in jobs for s in (j[0], j[3])]
        idx = c.index_streams(streams)
        out = c.lag_windows([(sa, idx[2 * k], fa, n, sb, idx[2 * k + 1], fb, lf, L, PAIRS) for k, (sa, fa, n, sb, fb, lf, L) in enumerate(jobs)])
        for x in idx:
            x.close()
        return out
    return call


def same(t, r):
    """a LagSums against the recipe's int64 sums (sign-extended into the high words; b_sq and a_sq stay under 2^63 for this material)"""
    dots, b_sq, a_sq = r
    rec = t.records
    return bool(torch.equal(rec[..., 0], dots) and torch.equal(rec[..., 1], dots >> 63) and torch.equal(rec[..., 2], b_sq) and not rec[..., 3].any()
                and torch.equal(t.a_sq[:, 0], a_sq) and not t.a_sq[:, 1].any())


def lane_rate():
    p = torch.cuda.get_device_properties(0)
    return p.multi_processor_count * 64 * 4 * args.clock_mhz * 1e6, f"{p.multi_processor_count} CUs * 4 SIMDs * 64 lanes * {args.clock_mhz / 1e3:g} GHz"


def case(jobs):
    products = sum(n * L * len(PAIRS) for _, _, n, _, _, _, L in jobs)
    forms = {"lag_windows": call_of(jobs), "recipe_int64_unfold": recipe_of(jobs, torch_unfold), "recipe_float64_conv1d": recipe_of(jobs, torch_conv)}
    out = {"probes": len(jobs), "needle_samples": jobs[0][2], "lags": jobs[0][6], "pairs": len(PAIRS), "products": products}
    probe_ctx = linne_amd.Context(0, use_torch_stream=True)
    try:
        recipe_of(jobs[:1], torch_conv)(probe_ctx)
    except Exception as e:                                        # (a conv1d this build of torch does not run at this size is left out, and said)
        out["recipe_float64_conv1d_left_out"] = f"{type(e).__name__}: {str(e)[:200]}"
        del forms["recipe_float64_conv1d"]
    probe_ctx.close()
    answers, peaks = st.peak_memory(forms)
    out["answers_equal"] = {name: all(same(t, r) for t, r in zip(answers["lag_windows"], answers[name])) for name in forms if name != "lag_windows"}
    out["peak_memory"] = peaks
    del answers
    ctx = linne_amd.Context(0, use_torch_stream=True)
    out.update(st.repetitions(ctx, forms, args.reps))
    fastest = min((name for name in forms if name != "lag_windows"), key=lambda name: out[name]["median_ms"])
    out["recipe_is"] = fastest
    out["recipe"] = out[fastest]
    streams = [s for j in jobs for s in (j[0], j[3])]
    idx = ctx.index_streams(streams)
    probes = [(sa, idx[2 * k], fa, n, sb, idx[2 * k + 1], fb, lf, L, PAIRS) for k, (sa, fa, n, sb, fb, lf, L) in enumerate(jobs)]

    def check(n):
        assert n(102) == 1 and n(103) == 1 and n(59) >= 1 and n(101) == 0
    ctx.enable_timing(True)
    out.update(st.kind_timings(ctx, [(lambda: ctx.lag_windows(probes), check, [(102, "kind_102_k_wx_lags"), (103, "kind_103_k_wx_lags_commit"), (59, "kind_59_k_wx_place"), (0, "lag_windows_device_ms")])], args.reps))
    ctx.enable_timing(False)
    for x in idx:
        x.close()
    ctx.close()
    rate, how = lane_rate()
    ms = out["kind_102_k_wx_lags"]["median_ms"]
    out["kind_102_multiply_adds_per_second"] = round(products / (ms * 1e-3)) if ms > 0 else None
    out["lane_rate_per_second"] = {"value": round(rate), "is": how + ": one multiply-add per lane and cycle; the 64-bit multiply-add's issue rate is not measured, so this is no peak"}
    out["criteria"] = {
        "faster_than_the_recipe_beyond_the_spread": st.faster_than(out, "lag_windows", f"recipe ({fastest})"),
        "peak_memory": f"{peaks['lag_windows']['peak_bytes']} bytes against the recipe's {peaks[fastest]['peak_bytes']}",
    }
    print(f"case done: {len(jobs)} probes, {jobs[0][6]} lags", file=sys.stderr, flush=True)
    return out


result = st.preamble(args, label=args.label, wxl_build={"note": "WXL_BLOCK and WXL_NARROW are compile-time switches of linne_amd/csrc/lnn_k_lags.h; the label names the build"})
enc = linne_amd.Context(0, use_torch_stream=True)
s, _ = st.one_stream(enc, args)
N = int(args.minutes * 60 * st.rate)
n = min(int(args.needle_seconds * st.rate), max(N // 2, 1))
first = (N - n) // 2
result["one_stream"] = {"stream": st.one_stream_label(args)}
for lags in (args.lags, args.wide_lags) if args.cases == "all" else (args.lags,):
    # (+-32768 would be 65537 lags, one more than a probe takes: -32768 .. 32767)
    result["one_stream"][f"needle_against_the_stream_pm_{lags}"] = case([(s, first, n, s, first, -lags, min(2 * lags + 1, linne_amd.LAG_MAX_LAGS))])
del s
if args.cases == "all":
    streams, _ = st.clips(enc, args)
    nclip = int(args.clip_seconds * st.rate)
    result["clips"] = {"stream": st.clips_label(args),
                       f"each_against_its_neighbour_pm_{args.lags}": case([(streams[k], 0, nclip, streams[(k + 1) % len(streams)], 0, -args.lags, 2 * args.lags + 1) for k in range(len(streams))])}
enc.close()
print(json.dumps(result))
