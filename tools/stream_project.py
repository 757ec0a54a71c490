"""Timing and memory of Context.project_windows (the frames of resident .lnn streams projected on int16 basis rows: the exact integer
STFT) against the recipe a user wrote before the call existed: index_streams + decode_windows (int32 planar) over the whole streams + torch
-- the float64 widening, unfold into frames, one float64 matmul with the same int16 basis, the rounding shift, the clamp and the
conversion.  The recipe is exact for these 16-bit streams (a sum stays under 2^53), so the two answers must be equal.  torch.stft in
float32 is timed beside them, for time only.  The cases:
  (a) BASELINE configs[1]'s stream, 60 minutes of 44.1 kHz int16 stereo, -m 7, block 10240, MS: n_fft 512, hop 128, 257 bins, Hann, int32;
  (b) 256 clips of 5 seconds of that shape into one float32 (W, C, K, frames) batch, the same basis;
  (c) a bank of 64 rows of 400 taps, hop 160, on (a)'s stream at 16 kHz after resample_streams.
How every figure is taken -- the statistic, the repetitions, the peak device memory of a call -- is tools/stream_timing.py's.  Kinds 105,
104 and 59 are HIP events around k_wx_project, k_wx_project_preset and k_wx_place in a project_windows call of the case; kind 59 of a
decode_windows call and kind 100 of a resample_windows call at 1/1 with one tap over the windows' input stand beside them.  --label names
the build (the library is LINNE_AMD_LIB's, or the tree's); --against FILE reads another build's result, the plain form's (-DWXP_MATRIX=0),
and states the third criterion from both.  Prints one JSON line (profiles/stream_project.json holds the MI355X's, and
profiles/stream_project_plain.json the plain form's)."""
import argparse
import json
import numpy as np
import torch
import stream_timing as st                # (puts the repository's root on the path)
import linne_amd
from stream_timing import verdict

ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=60.0)
ap.add_argument("--clips", type=int, default=256)
ap.add_argument("--clip-seconds", type=float, default=5.0)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="as shipped")
ap.add_argument("--plain", action="store_true", help="the library under LINNE_AMD_LIB is the -DWXP_MATRIX=0 build: no digit-plane figures")
ap.add_argument("--against", default=None)
args = ap.parse_args()
ONE = np.array([[1]], dtype=np.int16)


def torch_project(g, basis, hop, before, shift, float32, float_exp, rows_first):
    """the recipe's projection of one decoded stream (C, N) int32 -> (C, frames, K), or (C, K, frames)"""
    C, N = g.shape
    K, n_fft = basis.shape
    F = -(-N // hop)
    x = torch.zeros((C, (F - 1) * hop + n_fft), dtype=torch.float64, device=g.device)      # stream sample s at before + s: zeros around it; frame f begins at f * hop
    x[:, before:before + N] = g[:, :x.shape[1] - before]        # (samples behind the last frame's reach are read by nobody)
    y = torch.matmul(x.unfold(1, n_fft, hop), torch.from_numpy(basis.astype(np.float64)).to(g.device).t()).to(torch.int64)
    if shift:
        y = (y + (1 << (shift - 1))) >> shift
    y.clamp_(-(1 << 31), (1 << 31) - 1)
    y = y.to(torch.float32).mul_(2.0 ** -float_exp) if float32 else y.to(torch.int32)
    return y.transpose(1, 2).contiguous() if rows_first else y


def project_case(streams, basis, hop, before, shift, float32, rows_first, stft=None):
    K, n_fft = basis.shape
    float_exp = 0
    kw = dict(before=before, shift=shift, dtype=torch.float32 if float32 else torch.int32, float_exp=float_exp, rows_first=rows_first)

    def call(c, wins):
        return c.project_windows(wins, basis, hop, **kw)

    def library(c):
        idx = c.index_streams(streams)
        out = call(c, st.whole(streams, idx))
        for x in idx:
            x.close()
        return out

    forms = {"project_windows": library, "recipe": st.recipe_of(streams, lambda g: torch_project(g, basis, hop, before, shift, float32, float_exp, rows_first))}
    if stft:
        win = torch.hann_window(n_fft, periodic=True, device=st.dev)
        forms["torch_stft_float32"] = st.recipe_of(streams, lambda g: torch.stft(g.to(torch.float32), n_fft, hop, window=win, center=True, pad_mode="constant", return_complex=True))

    def head(got):
        return {"windows": int(got.shape[0]), "frames_per_window": int(got.shape[3 if rows_first else 2]), "rows": K, "frame_len": n_fft, "hop": hop,
                "output_bytes": int(got.numel() * 4), "output": ("float32" if float32 else "int32") + (" (W, C, K, frames)" if rows_first else " (W, C, frames, K)")}

    def loops(ctx, wins, out):
        one = [(s, x, 0, x.header["num_samples"]) for s, x, _, _ in wins]

        def check(n):
            assert n(104) == 1 and n(105) == 1 and n(59) >= 1
        steps = [(lambda: call(ctx, wins), check, [(105, "kind_105_k_wx_project"), (104, "kind_104_k_wx_project_preset"), (59, "kind_59_k_wx_place_into_the_images"), (0, "project_windows_device_ms")]),
                 st.decode_step(ctx, one, 105, figures=((59, "kind_59_k_wx_place_of_decode_windows"),))]

        def check_r(n):
            assert n(100) == 1
        steps.append((lambda: ctx.resample_windows(one, 1, 1, coef=ONE, before=0, shift=0), check_r, [(100, "kind_100_k_wx_resample_one_tap")]))
        return [steps]

    def after(out, idx):
        C = idx[0].header["num_channels"]
        frames = sum(-(-x.header["num_samples"] // hop) for x in idx)
        ms = out["kind_105_k_wx_project"]["median_ms"]
        out["products"] = int(C * frames * K * n_fft)
        out["products_per_second"] = round(out["products"] / (ms * 1e-3), 0) if ms > 0 else None
        if args.plain:                  # (the plain form has no digit planes: the figures below would mean nothing)
            return
        # what the kernel issues: per 64-row tile its rows rounded up to 16 and one 16-row group of ones, over the samples rounded up to 64;
        # 2 basis planes x 2 sample planes (16-bit streams); the ones group has one plane on the basis side
        Np, tiles = -(-n_fft // 64) * 64, -(-K // 64)
        rows16 = sum(-(-min(64, K - 64 * t) // 16) * 16 for t in range(tiles))
        out["digit_plane_multiply_adds"] = int(C * frames * Np * 2 * (2 * rows16 + 16 * tiles))
        out["digit_plane_multiply_adds_per_second"] = round(out["digit_plane_multiply_adds"] / (ms * 1e-3), 0) if ms > 0 else None
        out["ragged_share_of_the_instructions"] = round(1.0 - (2 * K * n_fft) / (Np * (2 * rows16 + 16 * tiles)), 4)
        out["ragged_share_is"] = ("computed from the shapes, not measured: the share of the issued digit-plane multiply-adds that is zero padding (rows to 16, samples to 64) "
                                  "or the group of ones each 64-row tile adds; the ragged edges run on the matrix unit too, there is no other path to time")
        out["limits"] = "not separated: the staging of the unfolded frames from L2 (each sample N / H times per 64-row block) and the matrix instructions share one loop without double buffering"

    def criteria(out, peaks):
        return {"faster_than_the_recipe_beyond_the_spread": st.faster_than(out, "project_windows"),
                "peak_memory_below_the_recipe": verdict(peaks["project_windows"]["peak_bytes"] < peaks["recipe"]["peak_bytes"],
                                                        f"{peaks['project_windows']['peak_bytes'] / 1e9:.3f} GB against {peaks['recipe']['peak_bytes'] / 1e9:.3f} GB")}

    def same(a, r):
        return bool(torch.equal(a, r))

    answers, peaks = st.peak_memory(forms)
    got = answers["project_windows"]
    out = head(got)
    out["answers_equal"] = all(same(got[i], r) for i, r in enumerate(answers["recipe"]))
    out["peak_memory"] = peaks
    del answers, got
    torch.cuda.empty_cache()
    ctx = linne_amd.Context(0, use_torch_stream=True)
    idx = ctx.index_streams(streams)
    out.update(st.repetitions(ctx, forms, args.reps))
    todo = loops(ctx, st.whole(streams, idx), out)
    ctx.enable_timing(True)
    for steps in todo:
        out.update(st.kind_timings(ctx, steps, args.reps))
    ctx.enable_timing(False)
    after(out, idx)
    for x in idx:
        x.close()
    ctx.close()
    out["criteria"] = criteria(out, peaks)
    return out


result = st.preamble(args, build=args.label, matrix_unit="v_mfma_i32_16x16x64_i8 over int8 digit planes, or the plain 64-bit multiply-add form of -DWXP_MATRIX=0: --label says which")
enc = linne_amd.Context(0, use_torch_stream=True)
stft_basis = linne_amd.project_design(512)
rng = np.random.default_rng(6)
bank = rng.integers(-32768, 32768, (64, 400)).astype(np.int16)
s, _ = st.one_stream(enc, args)
result["one_stream"] = {"stream": st.one_stream_label(args), "stft_512_hop_128": project_case([s], stft_basis, 128, 256, 15, False, False, stft=True)}
s16 = enc.resample_streams([s], 16000)[0].clone()
del s
result["one_stream"]["bank_64x400_hop_160_at_16_kHz"] = project_case([s16], bank, 160, 0, 15, False, False)
del s16
streams, _ = st.clips(enc, args)
enc.close()
result["clips"] = {"stream": st.clips_label(args), "stft_512_hop_128_float32_rows_first": project_case(streams, stft_basis, 128, 256, 15, True, True, stft=True)}
cases = {"one_stream.stft_512_hop_128": result["one_stream"]["stft_512_hop_128"], "one_stream.bank_64x400_hop_160_at_16_kHz": result["one_stream"]["bank_64x400_hop_160_at_16_kHz"],
         "clips.stft_512_hop_128_float32_rows_first": result["clips"]["stft_512_hop_128_float32_rows_first"]}
if args.against:
    other = json.load(open(args.against))
    verdicts = {}
    for name, c in cases.items():
        a, b = name.split(".")
        mine, theirs = c["kind_105_k_wx_project"], other[a][b]["kind_105_k_wx_project"]
        slack = max(mine["spread_ms"], theirs["spread_ms"])
        verdicts[name] = verdict(mine["median_ms"] + slack < theirs["median_ms"], f"kind 105 {mine['median_ms']} ms ({args.label}) against {theirs['median_ms']} ms ({other['build']}), spread {slack} ms")
    result["matrix_form_faster_than_the_plain_form_beyond_the_spread"] = verdicts
else:
    result["matrix_form_faster_than_the_plain_form_beyond_the_spread"] = {name: "not stated: no --against result" for name in cases}
print(json.dumps(result))
