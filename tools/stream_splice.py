"""Timing of cutting a resident stream (Context.splice_streams) against recompressing the same range, and of its copy kernel
(k_sp_copy, timing kind 71) against hipMemcpyDtoDAsync of as many bytes.  One synthetic 60-minute signal: 44.1 kHz, 16 bit, stereo,
-m 7, MS, block 10240, its stream and index resident.
  splice       the middle 50 minutes, one output: decode + encode of the two edge blocks, one copy run, the header
  recompress   decode_stream of that range followed by encode_stream of its samples: the only way before this call; same process,
               same context
  copy kernel  the whole stream as one run into a buffer of the caller's: source and destination 16-byte aligned, then every source
               residue 1..15 against a 16-byte-aligned destination and every destination residue (multiples of 4: an output is
               4-byte aligned) against an aligned source; HIP events around the launch (the context's timing), and torch events
               around hipMemcpyDtoDAsync on the same stream.  --rounds rounds of --copies copies each after a warm-up; compared: the
               best of the rounds' medians; spread: the largest difference between two rounds' medians of one measurement.
Prints one JSON line (profiles/stream_splice.json holds the MI355X's)."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import linne_amd
from bench import synth_track

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--copies", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--minutes", type=int, default=60)
args = ap.parse_args()
nch, bits, rate, block, preset, ms = 2, 16, 44100, 10240, 7, True
total = args.minutes * 60 * rate
pcm = synth_track(total, nch, bits, 3, torch.device("cuda", 0), rate=float(rate)).to(torch.int32).contiguous()
ctx = linne_amd.Context(0, use_torch_stream=True)
stream = ctx.encode_stream(pcm, bits, rate, block, preset, ms).clone()
index = ctx.index_stream(stream)
lo = total // 12 // block * block + block // 2                # the middle five sixths (50 of 60 minutes), from the middle of a block ...
n = (lo + total * 10 // 12) // block * block + block // 3 - lo   # ... to a third of one: two edge blocks to re-encode


def stats_ms(fn, reps):
    fn()                                                      # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def recompress():
    x = ctx.decode_stream(stream, lo, n, index=index)
    return ctx.encode_stream(x, bits, rate, block, preset, ms)


def splice():
    return ctx.splice_streams([[(stream, index, lo, n)]])[0]


result = {"config": f"44.1 kHz int16 stereo, -m 7, block 10240, MS; a {args.minutes}-minute stream resident, its middle five sixths cut out",
          "statistic": "wall ms: median / min / max over --reps calls after a warm-up, each ending in a device synchronise, in --rounds rounds; copies: "
                       "event ms, median of --copies after a warm-up per round; compared: the best of the rounds' medians; spread: the largest "
                       "difference between two rounds' medians", "reps": args.reps, "copies": args.copies, "rounds": args.rounds,
          "stream_bytes": int(stream.numel())}
a, b = splice(), recompress()
ia, ib = ctx.index_stream(a), ctx.index_stream(b)
want = pcm[:, lo:lo + n]
result["splice_decodes_to_the_range"] = bool(torch.equal(ctx.decode_stream(a, index=ia), want))
result["recompression_decodes_to_the_range"] = bool(torch.equal(ctx.decode_stream(b, index=ib), want))
result["splice_bytes"], result["recompress_bytes"] = int(a.numel()), int(b.numel())
ia.close(); ib.close()
del a, b
splice()
result["splice_blocks_copied_reencoded"] = list(ctx.last_splice_blocks[0])
rounds = {"splice": [], "recompress": []}
for _ in range(args.rounds):
    rounds["splice"].append(stats_ms(splice, args.reps))
    rounds["recompress"].append(stats_ms(recompress, args.reps))
result["wall"] = rounds
best = {k: min(r["median_ms"] for r in v) for k, v in rounds.items()}
spread = {k: round(max(r["median_ms"] for r in v) - min(r["median_ms"] for r in v), 3) for k, v in rounds.items()}
result["best_median_ms"], result["spread_ms"] = best, spread
result["recompress_over_splice"] = round(best["recompress"] / best["splice"], 1)

# ---- the copy kernel against hipMemcpyDtoDAsync ----
hip = linne_amd.lib                                            # (its HIP runtime: dlsym on the library's handle searches its dependencies)
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
nbytes = stream.numel()
srcbuf = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
dstbuf = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
whole = index.header["num_samples"]


def kernel_ms(src_res, dst_res):
    """the stream at residue src_res into a buffer at residue dst_res (the run itself starts 30 bytes in on either side)"""
    sbase, dbase = (-srcbuf.data_ptr()) % 16 + src_res, (-dstbuf.data_ptr()) % 16 + dst_res
    view = srcbuf[sbase:sbase + nbytes]
    view.copy_(stream)
    cut = (linne_amd.Cut * 1)()
    cut[0].index, cut[0].d_stream, cut[0].first_sample, cut[0].num_samples = index.h, view.data_ptr(), 0, whole
    one = (linne_amd.Splice * 1)()
    one[0].cuts, one[0].num_cuts, one[0].d_out, one[0].capacity = cut, 1, dstbuf.data_ptr() + dbase, nbytes
    torch.cuda.synchronize()
    meds = []
    for _ in range(args.rounds):
        ts = []
        for i in range(args.copies + 1):
            ret = linne_amd.lib.LINNEAmd_SpliceStreamsDevice(ctx.h, one, 1, 0)
            assert ret == 0 and one[0].out_bytes == nbytes and one[0].encoded_blocks == 0, (ret, linne_amd.lib.LINNEAmd_GetLastError(ctx.h))
            if i:
                ts.append(ctx.last_ms(71))
        meds.append(statistics.median(ts))
    assert torch.equal(dstbuf[dbase:dbase + nbytes], stream)
    return meds


def memcpy_ms():
    s, d = srcbuf[(-srcbuf.data_ptr()) % 16:], dstbuf[(-dstbuf.data_ptr()) % 16:]
    st = torch.cuda.current_stream()
    meds = []
    for _ in range(args.rounds):
        ts = []
        for i in range(args.copies + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            assert hip.hipMemcpyDtoDAsync(d.data_ptr(), s.data_ptr(), nbytes - 30, C.c_void_p(st.cuda_stream)) == 0
            e1.record(st)
            e1.synchronize()
            if i:
                ts.append(e0.elapsed_time(e1))
        meds.append(statistics.median(ts))
    return meds


ctx.enable_timing(True)
run_bytes = nbytes - 30
gbs = lambda ms_: round(run_bytes / ms_ / 1e6, 1)
mem = memcpy_ms()
ali = kernel_ms(0, 0)
copy = {"run_bytes": int(run_bytes), "memcpy_round_medians_ms": [round(v, 4) for v in mem], "kernel_aligned_round_medians_ms": [round(v, 4) for v in ali],
        "memcpy_gb_per_s": gbs(min(mem)), "kernel_aligned_gb_per_s": gbs(min(ali)),
        "spread_ms": {"memcpy": round(max(mem) - min(mem), 4), "kernel_aligned": round(max(ali) - min(ali), 4)}}
pairs = {}
for r in range(1, 16):
    pairs[f"src{r}_dst0"] = gbs(min(kernel_ms(r, 0)))
for r in (4, 8, 12):
    pairs[f"src0_dst{r}"] = gbs(min(kernel_ms(0, r)))
copy["kernel_gb_per_s_by_residues"] = pairs
worst = min(pairs, key=pairs.get)
copy["worst_pair"], copy["worst_pair_gb_per_s"] = worst, pairs[worst]
ctx.enable_timing(False)
result["copy"] = copy
tol = max(copy["spread_ms"].values())
result["verdict"] = {
    "splice_faster_than_recompression_beyond_the_spread": "yes" if best["splice"] + spread["splice"] + spread["recompress"] < best["recompress"] else f"MISSED: {best['splice']} ms against {best['recompress']} ms",
    "copy_kernel_within_the_spread_of_the_device_copy_when_aligned": "yes" if min(ali) <= min(mem) + tol else f"MISSED: {gbs(min(ali))} GB/s against {gbs(min(mem))} GB/s (spread {tol} ms)",
}
print(json.dumps(result))
index.close()
ctx.close()
