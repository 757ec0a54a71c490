"""Timing of the device-resident stream decoder (Context.index_stream / Context.decode_stream) on BASELINE configs[1]'s stream:
60 minutes of 44.1 kHz int16 stereo, -m 7, encoded once by the product (LINNEEncoder_EncodeWhole), its bytes resident in HBM.
Reports the median of --reps runs after a warm-up, each run ending in a device synchronise: the index build, a whole-stream
decode with a built index, a 5-second window at a random offset, and LINNEDecoder_DecodeWhole of the same bytes from host memory.
Prints one JSON line (profiles/stream_decode.json holds the MI355X's)."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import linne_amd
from refs import LinneApi, _planar_ptrs, _RefDecoderConfig
from bench import synth_track

ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=60.0)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--window-seconds", type=float, default=5.0)
args = ap.parse_args()
nch, bits, rate = 2, 16, 44100
ns = int(args.minutes * 60 * rate)
x = np.ascontiguousarray(synth_track(ns, nch, bits, 3, torch.device("cuda", 0), rate=float(rate)).cpu().numpy(), dtype=np.int32)
api = LinneApi(linne_amd.LIB_PATH)
stream = api.encode_whole(x, bits, rate, 10240, 7, True)
d_stream = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
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


index = ctx.index_stream(d_stream)
t_index, ts_index = median_ms(lambda: ctx.index_stream(d_stream).close(), args.reps)
out = ctx.decode_stream(d_stream, index=index)
ok_whole = bool(np.array_equal(out.cpu().numpy(), x))
del out
t_whole, _ = median_ms(lambda: ctx.decode_stream(d_stream, index=index), args.reps)
win = int(args.window_seconds * rate)
rng = np.random.default_rng(42)
first = int(rng.integers(0, ns - win))
w = ctx.decode_stream(d_stream, first, win, index=index)
ok_window = bool(np.array_equal(w.cpu().numpy(), x[:, first:first + win]))
t_window, _ = median_ms(lambda: ctx.decode_stream(d_stream, first, win, index=index), args.reps)
# the kernels of one whole decode (timing on: events around every launch)
ctx.enable_timing(True)
ctx.decode_stream(d_stream, index=index)
kinds = {k: round(ctx.last_ms(k), 3) for k in (56, 57, 28, 58, 32, 33, 34, 35, 36, 30, 31, 11, 12, 59) if ctx.last_launches(k) > 0}
ctx.index_stream(d_stream).close()
INDEX_KINDS = tuple(range(37, 45)) + (69, 70)
kinds_index = {k: round(ctx.last_ms(k), 3) for k in INDEX_KINDS if ctx.last_launches(k) > 0}
launches_index = {k: ctx.last_launches(k) for k in INDEX_KINDS if ctx.last_launches(k) > 0}
ctx.enable_timing(False)
# DecodeWhole of the same bytes from host memory
cfg = _RefDecoderConfig(nch, 5, 128, 1)
dec = api.L.LINNEDecoder_Create(C.byref(cfg), None, 0)
buf = np.frombuffer(stream, dtype=np.uint8)
back = np.zeros_like(x)
bp, _keep = _planar_ptrs(back)
rets = []
t_dw, _ = median_ms(lambda: rets.append(api.L.LINNEDecoder_DecodeWhole(dec, buf.ctypes.data, len(stream), bp, nch, ns)), args.reps)
api.L.LINNEDecoder_Destroy(dec)
ok_dw = all(r == 0 for r in rets) and bool(np.array_equal(back, x))
print(json.dumps({
    "config": f"{args.minutes:g} min 44.1 kHz int16 stereo, -m 7, block 10240 (BASELINE configs[1])", "stream_bytes": len(stream),
    "blocks": index.num_blocks, "reps": args.reps, "statistic": "median ms, warm-up excluded, each run ends in a device synchronise",
    "index_stream_ms": round(t_index, 3), "index_stream_min_max_ms": [round(min(ts_index), 3), round(max(ts_index), 3)], "decode_stream_whole_ms": round(t_whole, 3),
    "decode_stream_window_ms": round(t_window, 3), "window": {"first_sample": first, "num_samples": win},
    "decode_whole_host_bytes_ms": round(t_dw, 3),
    "kernel_ms_whole_decode": {str(k): v for k, v in kinds.items()}, "kernel_ms_index": {str(k): v for k, v in kinds_index.items()},
    "kernel_launches_index": {str(k): v for k, v in launches_index.items()},
    "exact": {"whole": ok_whole, "window": ok_window, "decode_whole": ok_dw},
}))
index.close()
ctx.close()
