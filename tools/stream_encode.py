"""Timing of the device-resident stream encoder (Context.encode_stream) on BASELINE configs[1]'s input: 60 minutes of 44.1 kHz int16
stereo, -m 7, block 10240, MS, resident in HBM as planar int32.  Reports the median of --reps runs after a warm-up, each run ending in
a device synchronise: encode_stream with the whole stream in one pass, the resident analysis step alone (EncodeFramesDevice on the
same frames, already in the [F][C][S] layout), and LINNEEncoder_EncodeWhole from host memory.  Checks that the device's stream equals
EncodeWhole's bytes and that decode_stream(encode_stream(x)) == x without leaving the device.  Two options add what a pass and what
a call cost: --group-frames G encodes the same track in passes of G frames, --calls N makes N encode_stream calls on 3-second stereo
tracks at block 4096.  Prints one JSON line (profiles/stream_encode.json holds the MI355X's)."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import linne_amd
from refs import LinneApi, _planar_ptrs
from bench import synth_track

ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=60.0)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--group-frames", type=int, default=0, help="also time the track in passes of this many frames")
ap.add_argument("--calls", type=int, default=0, help="also time this many encode_stream calls on 3-second tracks at block 4096")
args = ap.parse_args()
nch, bits, rate, block, preset, ms = 2, 16, 44100, 10240, 7, True
ns = int(args.minutes * 60 * rate)
d_x = synth_track(ns, nch, bits, 3, torch.device("cuda", 0), rate=float(rate)).to(torch.int32).contiguous()
x = np.ascontiguousarray(d_x.cpu().numpy(), dtype=np.int32)
api = LinneApi(linne_amd.LIB_PATH)
ctx = linne_amd.Context(0, use_torch_stream=True)


def median_ms(fn, reps):
    fn()                                                      # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


stream = ctx.encode_stream(d_x, bits, rate, block, preset, ms)
counts = {k: ctx.last_stream_encode_count(i) for i, k in enumerate(("compress", "silent", "raw", "host_settled_plans"))}
ok_round_trip = bool(torch.equal(ctx.decode_stream(stream), d_x))
t_stream, _ = median_ms(lambda: ctx.encode_stream(d_x, bits, rate, block, preset, ms), args.reps)
extra = {}
if args.group_frames:
    g = args.group_frames
    same = bool(torch.equal(ctx.encode_stream(d_x, bits, rate, block, preset, ms, group_frames=g), stream))
    t_g, _ = median_ms(lambda: ctx.encode_stream(d_x, bits, rate, block, preset, ms, group_frames=g), args.reps)
    extra.update({"group_frames": g, "passes": -(-((ns + block - 1) // block) // g), "encode_stream_passes_ms": round(t_g, 3), "passes_same_bytes": same})
if args.calls:
    n3 = 3 * rate
    clips = [d_x[:, i * n3:(i + 1) * n3] for i in range(min(args.calls, ns // n3))]
    assert clips, "--calls needs a track of 3 seconds or more"

    def many():
        for i in range(args.calls):
            ctx.encode_stream(clips[i % len(clips)], bits, rate, 4096, preset, ms)
    t_c, _ = median_ms(many, args.reps)
    extra.update({"calls": args.calls, "clip": "3 s stereo, block 4096, -m 7", "encode_stream_calls_ms": round(t_c, 3)})
# the resident analysis step alone, on the same frames in the [F][C][S] layout
F = (ns + block - 1) // block
frames = torch.zeros((F * block, nch), dtype=torch.int32, device="cuda")
frames[:ns] = d_x.t()
frames = frames.view(F, block, nch).permute(0, 2, 1).contiguous()
nsm = np.full(F, block, dtype=np.uint32); nsm[-1] = ns - (F - 1) * block
shape = ctx.shape(nch, bits, block, preset, ms)
bufs = (torch.empty_like(frames), torch.zeros((F, nch, linne_amd.PARAM_WORDS), dtype=torch.int32, device="cuda"),
        torch.zeros((F, nch, linne_amd.STAT_WORDS), dtype=torch.float64, device="cuda"))
t_frames, _ = median_ms(lambda: ctx.encode_frames(shape, frames, nsm, out=bufs), args.reps)
del frames, bufs
# the kernels of one encode_stream call (timing on: events around every launch)
ctx.enable_timing(True)
ctx.encode_stream(d_x, bits, rate, block, preset, ms)
kinds = {k: round(ctx.last_ms(k), 3) for k in (60, 17, 49, 61, 51, 62, 63, 64, 65, 66, 67, 68) if ctx.last_launches(k) > 0}
ctx.enable_timing(False)
# EncodeWhole from host memory
enc = api.new_encoder(nch, bits, rate, block, preset, ms)
ptrs, _keep = _planar_ptrs(x)
cap = x.size * 8 + 65536
out = np.zeros(cap, dtype=np.uint8)
osz = C.c_uint32(0)
rets = []
t_whole, _ = median_ms(lambda: rets.append(api.L.LINNEEncoder_EncodeWhole(enc, ptrs, ns, out.ctypes.data, cap, C.byref(osz))), args.reps)
api.L.LINNEEncoder_Destroy(enc)
enc = api.new_encoder(nch, bits, rate, block, preset, ms)              # a fresh encoder: quirk Q2 starts from 0.0 as in encode_stream
assert api.L.LINNEEncoder_EncodeWhole(enc, ptrs, ns, out.ctypes.data, cap, C.byref(osz)) == 0
api.L.LINNEEncoder_Destroy(enc)
ok_bytes = all(r == 0 for r in rets) and bytes(stream.cpu().numpy()) == out[:osz.value].tobytes()
print(json.dumps({
    "config": f"{args.minutes:g} min 44.1 kHz int16 stereo, -m 7, block 10240, MS (BASELINE configs[1])", "stream_bytes": int(stream.numel()),
    "frames": F, "blocks": counts, "reps": args.reps, "statistic": "median ms, warm-up excluded, each run ends in a device synchronise",
    "encode_stream_one_pass_ms": round(t_stream, 3), "encode_frames_device_ms": round(t_frames, 3),
    "encode_whole_host_memory_ms": round(t_whole, 3), **extra,
    "kernel_ms_encode_stream": {str(k): v for k, v in kinds.items()},
    "exact": {"equal_to_encode_whole": ok_bytes, "device_round_trip": ok_round_trip},
}))
ctx.close()
