"""The device's Rice stage (k_rice_plan, k_rice_scan / k_rice_emit, k_rice_decode) against the ORACLE's coder (oracle_rice_encode /
oracle_rice_decode, a restatement of linne_coder.c), on residuals the test builds itself rather than ones an encoder made from audio:
blocks of up to 65535 samples (k_rice_plan<false> and k_rice_emit<false> beyond REMIT_LDS_SAMPLES), zero runs of 25 to 2049 bits
and of about 65 k and 1 M bits (the ring re-staging of k_rice_decode), magnitudes up to 2^30, parameter jumps of 20 between
partitions, partition order 10 next to order 0, and codes longer than the emission's cap.

Domain: |residual| < 2^30, so that the zig-zag values stay below 2^31 and k1 = k2 + 1 <= 31 both here and in the reference.
Zig-zag values near 0xFFFFFFFF would need 1 << 32 (undefined in the reference as well) and are not tested.  The encoder's search
puts a lone loud sample's run at about 3 n bits at most; the 1 M-bit run is a code with given parameters
(oracle_rice_encode_given), which any decoder must read."""
import ctypes as C
import math

import numpy as np
import pytest

import linne_amd
from signals import LONG_STREAMS, long_block_input, long_stream_args

pytestmark = pytest.mark.gpu

RUNS = [25, 26, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1535, 2047, 2048, 2049]
OPTX = 0.5127629514437670454896078808815218508243560791015625
NB = linne_amd.RICE_PLAN_NBITS


def unzz(u):
    u = np.asarray(u, dtype=np.int64)
    return ((u >> 1) ^ -(u & 1)).astype(np.int32)


def zz(v):
    v = np.asarray(v, dtype=np.int64)
    return np.where(v < 0, -2 * v - 1, 2 * v)


def k2_of(mean):
    """linne_coder.c's parameter of a partition mean (the test aims with it; the oracle's own code is what is compared)"""
    rho = 1.0 / (1.0 + mean)
    return max(0, math.floor(math.log(math.log(OPTX) / math.log(1.0 - rho)) * 1.4426950408889634))


def lone_loud(rng, n, run):
    """n samples (n odd: partition order 0) of quiet noise and one loud sample whose code under the encoder's own parameter has a
    zero run of exactly `run` bits; None when no background of this length allows it"""
    for b in (0, 1, 3, 10, 30, 100, 300, 1000, 3000, 10000, 30000, 100000):
        x = rng.integers(-b, b + 1, size=n).astype(np.int32) if b else np.zeros(n, dtype=np.int32)
        pos = int(rng.integers(0, n))
        x[pos] = 0
        q = int(zz(x).sum())
        for k2 in range(0, 30):
            u = (1 << (k2 + 1)) + (run - 1) * (1 << k2) + int(rng.integers(0, 1 << k2))
            if u >= 1 << 31:
                break
            if k2_of((q + u) / n) == k2:
                x[pos] = unzz(u)
                return x, k2
    return None


def case(rng, name, n):
    """one channel's residual of n samples (named shapes of the module docstring)"""
    if name == "zero":
        return np.zeros(n, dtype=np.int32)
    if name == "tiny":
        return rng.integers(-1, 2, size=n).astype(np.int32)
    if name == "usual":
        return np.round(rng.laplace(0.0, 200.0, size=n)).astype(np.int32)
    if name == "huge":                                    # zig-zag in [1.5 * 2^30, 2^31): k2 = 30, 32-bit codes, over the cap when n == S
        return (rng.integers(3 << 28, 1 << 30, size=n) * rng.choice([-1, 1], size=n)).astype(np.int32)
    if name == "large":                                   # k2 in the high 20s
        return np.clip(np.round(rng.laplace(0.0, float(1 << 27), size=n)), -(1 << 30) + 1, (1 << 30) - 1).astype(np.int32)
    if name == "back_to_back":                            # several long runs back to back in quiet noise
        x = rng.integers(-2, 3, size=n).astype(np.int32)
        p = int(rng.integers(0, max(1, n - 8)))
        x[p:p + 6] = (rng.integers(1 << 16, 1 << 20, size=len(x[p:p + 6])) * rng.choice([-1, 1], size=len(x[p:p + 6]))).astype(np.int32)
        return x
    if name == "jumps":                                   # finest partitions alternate quiet / loud: parameter steps of about +-20
        parts = 1024 if n % 1024 == 0 else 1
        ns = n // parts
        x = rng.integers(-1, 2, size=n).astype(np.int32)
        for p in range(1, parts, 2):
            x[p * ns:(p + 1) * ns] = (rng.integers(1 << 20, 1 << 21, size=ns) * rng.choice([-1, 1], size=ns)).astype(np.int32)
        return x
    if name.startswith("run"):                            # a lone loud sample: a zero run of the given length
        got = lone_loud(rng, n, int(name[3:]))
        assert got is not None, f"n={n}: no background gives a run of {name[3:]}"
        return got[0]
    raise ValueError(name)


def batch_lengths(S, F, rng):
    """ragged lengths: the block, odd lengths (order 0), multiples of 1024 (order 10) and odd multiples of 2^k"""
    odd = S if S % 2 else S - 1
    m1024 = (S // 1024) * 1024 or S
    pool = [S, odd, m1024, max(1, odd - 2 * int(rng.integers(0, 50))), max(1, S - 1 - 64 * int(rng.integers(0, 8)))]
    return np.array([pool[f % len(pool)] for f in range(F)], dtype=np.uint32)


def make_batch(S, Cn, F, seed):
    """[F][C][S] residual, lengths and the name of every channel-frame's shape"""
    rng = np.random.default_rng(seed)
    ns = batch_lengths(S, F, rng)
    res = np.zeros((F, Cn, S), dtype=np.int32)
    names = []
    plain = ["zero", "tiny", "usual", "huge", "large", "back_to_back", "jumps"]
    runs = ["run%d" % r for r in RUNS if r <= 2 * S] + (["run65000"] if S >= 32768 else [])
    k = 0
    for f in range(F):
        n = int(ns[f])
        row = []
        for ch in range(Cn):
            if f == 0:
                nm = "huge"                                     # (n = S: a code over the cap)
            elif n % 2 == 1 and runs and k % 2 == 0:
                nm = runs[(k // 2) % len(runs)]
            else:
                nm = plain[k % len(plain)]
            k += 1
            try:
                res[f, ch, :n] = case(rng, nm, n)
            except AssertionError:
                nm = "usual"
                res[f, ch, :n] = case(rng, nm, n)
            row.append(nm)
        names.append(row)
    return res, ns, names


def longest_run(code, x):
    """the zero run of the loudest sample in an order-0 code (read from the code's own header: 10-bit order, 5-bit parameter)"""
    head = int.from_bytes(code[:2], "big")
    order, k2 = head >> 6, (head >> 1) & 31
    u = int(zz(x).max())
    return None if order or u < (2 << k2) else 1 + ((u - (2 << k2)) >> k2)


_ORACLE_CODES = {}


def oracle_codes(oracle, key, res, ns):
    """(bytes, bits) of the oracle's code of every channel-frame"""
    if key not in _ORACLE_CODES:
        F, Cn, _ = res.shape
        _ORACLE_CODES[key] = [[oracle.rice_encode(res[f, ch, :int(ns[f])]) for ch in range(Cn)] for f in range(F)]
    return _ORACLE_CODES[key]


BATCHES = [(1021, 8, 64), (4096, 2, 64), (12288, 1, 64), (12289, 2, 64), (16384, 8, 64), (32768, 1, 64), (65535, 2, 64)]


@pytest.mark.parametrize("S,Cn,F", BATCHES)
def test_plan_and_emission_equal_the_oracles_code(ctx, oracle, S, Cn, F):
    """k_rice_plan's order, parameters and code length and k_rice_emit's bits are the oracle's, channel-frame by channel-frame; a code
    longer than the emission's cap (4 S bytes) has offset 0xFFFFFFFF; stitched into blocks, the device's codes, the device's plan and
    the host's own search give the same bytes"""
    import torch
    res, ns, names = make_batch(S, Cn, F, seed=S + Cn)
    codes = oracle_codes(oracle, (S, Cn, F), res, ns)
    shape = ctx.shape(Cn, 24, S, 0, False)
    d_res = torch.from_numpy(res).cuda()
    plan = ctx.rice_plan(shape, d_res, ns)
    packed, offsets = ctx.rice_emit(shape, d_res, plan)
    ctx.synchronize()
    plan, packed, off = plan.cpu().numpy(), packed.cpu().numpy(), offsets.cpu().numpy().view(np.uint32)
    nbits = plan[:, :, NB:NB + 4].copy().view(np.uint32)[:, :, 0]
    flagged, over, seen = 0, 0, set()
    for f in range(F):
        for ch in range(Cn):
            cf, where = f * Cn + ch, f"frame {f} ch {ch} ({names[f][ch]}, n={ns[f]})"
            code, bits = codes[f][ch]
            if plan[f, ch, 1]:
                flagged += 1
                assert nbits[f, ch] == 0xFFFFFFFF and off[cf] == 0xFFFFFFFF, where
                continue
            seen.add(names[f][ch])
            if names[f][ch].startswith("run"):                  # (the test's aim, checked on the oracle's code)
                assert longest_run(code, res[f, ch, :ns[f]]) == int(names[f][ch][3:]), where
            assert int(nbits[f, ch]) == bits, f"{where}: code length"
            assert plan[f, ch, 0] == code[0] * 4 + (code[1] >> 6), f"{where}: partition order"
            if (bits + 63) // 64 * 8 > 4 * S:
                over += 1
                assert off[cf] == 0xFFFFFFFF, f"{where}: a code over the cap must be left to the host"
                continue
            assert off[cf] != 0xFFFFFFFF, where
            got = packed[int(off[cf]):int(off[cf]) + len(code)]
            assert np.array_equal(got, np.frombuffer(code, dtype=np.uint8)), f"{where}: the emitted bits"
    assert {"zero", "tiny", "large", "jumps"} <= seen, seen
    assert over > 0 and any(nm.startswith("run") for nm in seen)
    print(f"S={S} C={Cn}: {flagged} plans flagged to the host, {over} codes over the cap")
    # blocks: pcm of ones (no SILENT block), zero statistics (no RAW block), one unit per layer
    pcm = np.ones_like(res)
    prm = np.zeros((F, Cn, linne_amd.PARAM_WORDS), dtype=np.int32)
    prm[:, :, linne_amd.PRM_UNITS:linne_amd.PRM_UNITS + 2] = 1
    st = np.zeros((F, Cn, linne_amd.STAT_WORDS), dtype=np.float64)
    want, _ = linne_amd.pack_frames(shape, pcm, res, prm, st, ns, 0.0, 4)
    assert all(b[8] == 0 for b in want), "every block is COMPRESS"
    got, _ = linne_amd.pack_frames(shape, pcm, res, prm, st, ns, 0.0, 4, plan=plan)
    assert got == want
    planes = np.ascontiguousarray(pcm.transpose(1, 0, 2).reshape(Cn, F * S))
    got, _, fetched = linne_amd.pack_frames_emitted(shape, planes, 0, prm, st, plan, packed, offsets.cpu().numpy(), ns, 0.0, 4, residual=res)
    assert got == want
    assert sorted(set(fetched)) == sorted({int(cf) // Cn for cf in np.nonzero(off[:-1] == 0xFFFFFFFF)[0]})


def bits_of(code, nbits):
    return np.unpackbits(np.frombuffer(code, dtype=np.uint8))[:nbits]


def decode_on_device(ctx, shape, blob, total_bytes, starts, ns, Cn, S):
    """LINNEAmd_RiceDecodeDevice over `blob` (its length: the contract's bound) -> (residual [F][C][S], end bits [F])"""
    import torch
    F = len(starts)
    buf = torch.from_numpy(blob).cuda()
    bitpos = torch.from_numpy(np.asarray(starts, dtype=np.uint64).view(np.int64)).cuda()
    out = torch.full((F, Cn, S), 123456, dtype=torch.int32, device="cuda")
    endbit = torch.zeros(F, dtype=torch.int64, device="cuda")
    nsk = np.ascontiguousarray(ns, dtype=np.uint32)
    ctx._fence()
    ret = linne_amd.lib.LINNEAmd_RiceDecodeDevice(C.c_void_p(ctx.h), C.byref(shape), C.c_void_p(buf.data_ptr()), C.c_uint64(total_bytes),
                                                  C.c_void_p(bitpos.data_ptr()), nsk.ctypes.data_as(C.c_void_p), C.c_uint32(F),
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(endbit.data_ptr()))
    assert ret == 0
    ctx.synchronize()
    return out.cpu().numpy(), endbit.cpu().numpy().view(np.uint64)


def lay_out(codes, rng):
    """every frame's channel codes back to back (a block holds them so: linne_encoder.c EncodeBlock), the frames one after another
    at bit positions off the 8-, 32- and 64-bit grids with random bits in between; -> (buffer sized to the contract, stream bytes,
    frame starts, frame ends)"""
    pieces, starts, ends, pos = [], [], [], 0
    for f, chans in enumerate(codes):
        gap = 1 + 8 * f + int(rng.integers(0, 64)) | 1                # odd: never on a byte, word or 64-bit boundary
        pieces.append(rng.integers(0, 2, size=gap).astype(np.uint8))
        pos += gap
        starts.append(pos)
        for code, nbits in chans:
            pieces.append(bits_of(code, nbits))
            pos += nbits
        ends.append(pos)
    allbits = np.concatenate(pieces)
    total = (pos + 7) // 8
    blob = np.full((total + 7) & ~7, 0xA5, dtype=np.uint8)             # non-zero bytes up to the bound the contract allows reading
    blob[:total] = np.packbits(allbits)
    if pos % 8:
        blob[total - 1] |= (1 << (8 - pos % 8)) - 1                   # (and non-zero bits behind the last code)
    return blob, total, starts, ends


def check_decode(ctx, oracle, codes, res, ns, Cn, S, rng, what):
    blob, total, starts, ends = lay_out(codes, rng)
    allbits = np.unpackbits(blob)
    for f in range(len(starts)):                                       # the layout itself, through the oracle's decoder
        p = starts[f]
        for ch in range(Cn):
            code, nbits = codes[f][ch]
            piece = np.packbits(allbits[p:p + nbits]) if f < 2 else np.frombuffer(code, dtype=np.uint8)
            x, used = oracle.rice_decode(piece.tobytes(), int(ns[f]))
            assert np.array_equal(x, res[f, ch, :ns[f]]) and used == (nbits + 7) // 8, f"{what}: oracle round trip, frame {f} ch {ch}"
            p += nbits
        assert p == ends[f]
    shape = ctx.shape(Cn, 24, S, 0, False)
    got, eb = decode_on_device(ctx, shape, blob, total, starts, ns, Cn, S)
    for f in range(len(starts)):
        assert int(eb[f]) != 0xFFFFFFFFFFFFFFFF, f"{what}: frame {f} refused"
        assert np.array_equal(got[f, :, :ns[f]], res[f, :, :ns[f]]), f"{what}: frame {f} residual"
        assert int(eb[f]) == ends[f], f"{what}: frame {f} end position"


@pytest.mark.parametrize("S,Cn,F", BATCHES)
def test_decode_of_the_oracles_codes(ctx, oracle, S, Cn, F):
    """the oracle's codes of the same batches, laid out as blocks at bit positions off every grid in a buffer that ends at the contract's
    bound: k_rice_decode gives the residual back and ends every frame where the oracle's code ends"""
    res, ns, _ = make_batch(S, Cn, F, seed=S + Cn)
    codes = oracle_codes(oracle, (S, Cn, F), res, ns)
    check_decode(ctx, oracle, codes, res, ns, Cn, S, np.random.default_rng(S), f"S={S} C={Cn}")


def given_code_batch(oracle, S, F, seed, lone_lane=None):
    """mono frames whose codes have parameters the TEST chose: partition 0 has k2 = 0 and zero runs of exactly 25 .. 2049 bits, about
    65 k bits and about 1 M bits, back to back; the other frames are the oracle's own codes of usual samples.  With lone_lane = i only
    frame i holds the runs (one lane of a wave with very long runs, 63 with usual samples)"""
    rng = np.random.default_rng(seed)
    res = np.zeros((F, 1, S), dtype=np.int32)
    ns = np.full(F, S, dtype=np.uint32)
    codes = []
    for f in range(F):
        if lone_lane is None or f == lone_lane:
            n = (S if S % 2 else S - 1) if (lone_lane is not None or f % 2 == 0) else (S // 1024) * 1024
            ns[f] = n
            parts = 1 if n % 2 else 1024
            k2 = [0] * parts
            x = rng.integers(-1, 2, size=n).astype(np.int32)
            runs = (RUNS + [65536, 1 << 20] if f == lone_lane or f % 4 == 0 else RUNS)[:n // parts]
            p = int(rng.integers(0, n // parts - len(runs) + 1))
            x[p:p + len(runs)] = unzz(np.array(runs) + 1)             # k2 = 0: the zig-zag value u has a run of u - 1 bits
            if parts > 1:                                               # later partitions: parameters up and down by 20
                for q in range(1, parts):
                    k2[q] = 20 if q % 2 else (3 if q % 4 == 2 else 0)
                ns_p = n // parts
                for q in range(1, parts):
                    if k2[q] == 20:
                        x[q * ns_p:(q + 1) * ns_p] = (rng.integers(1 << 20, 1 << 22, size=ns_p) * rng.choice([-1, 1], size=ns_p)).astype(np.int32)
            res[f, 0, :n] = x
            codes.append([oracle.rice_encode(x, k2)])
        else:
            x = np.round(rng.laplace(0.0, 50.0, size=S)).astype(np.int32)
            res[f, 0] = x
            codes.append([oracle.rice_encode(x)])
    return res, ns, codes


@pytest.mark.parametrize("S,F,lone", [(65535, 8, None), (32768, 8, None), (16384, 64, 37), (65535, 64, 0)])
def test_decode_of_given_codes_with_very_long_runs(ctx, oracle, S, F, lone):
    """zero runs past the fast path (more than 24 bits), past the staged ring (more than 2048 bits) and far past it (65 k, 1 M bits),
    back to back and next to parameter jumps of 20, in every lane or in one lane of a full wave"""
    res, ns, codes = given_code_batch(oracle, S, F, seed=S + F, lone_lane=lone)
    assert max(c[0][1] for c in codes) > (1 << 20)
    check_decode(ctx, oracle, codes, res, ns, 1, S, np.random.default_rng(F), f"S={S} F={F} lone={lone}")


# ---- whole streams at long blocks and with clicks: the product against the oracle and the reference's recorded answers ----------------

@pytest.mark.parametrize("nch,bits,block,preset,tail,click", LONG_STREAMS)
def test_long_block_streams(ctx, product, oracle, reference, monkeypatch, nch, bits, block, preset, tail, click):
    """EncodeWhole at blocks of 10240 to 65535 samples (the last one 12 k .. 64 k long: k_rice_plan<false>, k_rice_emit<false>,
    k_se_rice<false>) gives the oracle's bytes and the reference's; block-at-a-time encoding and the device stream encoder give them too;
    DecodeWhole (host and device Rice decoding), the device stream decoder and a range inside the long blocks give the input back"""
    x, bits, rate, block, preset, ms = long_stream_args(nch, bits, block, preset, tail, click)
    mine = product.encode_whole(x, bits, rate, block, preset, ms)
    assert mine == oracle.encode_whole(x, bits, rate, block, preset, ms), "oracle"
    assert mine == reference.encode_whole(x, bits, rate, block, preset, ms)
    assert product.encode_blocks(x, bits, rate, block, preset, ms) == mine
    assert bytes(ctx.encode_stream(x, bits, rate, block, preset, ms).cpu().numpy()) == mine
    for mode in ("0", "1"):
        monkeypatch.setenv("LINNE_AMD_DECODE_STREAM", mode)
        ret, dec = product.decode_whole(mine)
        assert ret == 0 and np.array_equal(dec, x), f"DecodeWhole, LINNE_AMD_DECODE_STREAM={mode}"
    monkeypatch.delenv("LINNE_AMD_DECODE_STREAM")
    assert np.array_equal(ctx.decode_stream(mine).cpu().numpy(), x)
    first, n = block // 2 + 7, block + tail // 2 + 3                     # starts inside block 0, ends inside the tail
    assert np.array_equal(ctx.decode_stream(mine, first, n).cpu().numpy(), x[:, first:first + n])


def oracle_frames(oracle, frames, ns, nch, bits, block, preset, ms):
    """the oracle's residual and parameters of every frame (its hot path) and its synthesis of them"""
    from test_gpu_parity import _params_from_tap
    F = len(frames)
    ores = np.zeros_like(frames)
    oprm = np.zeros((F, nch, linne_amd.PARAM_WORDS), dtype=np.int32)
    want = np.zeros_like(frames)
    for f in range(F):
        n = int(ns[f])
        enc = oracle.encoder(nch, bits, 44100, block, preset, ms)
        tap, r = enc.hotpath(frames[f][:, :n])
        enc.close()
        ores[f, :, :n] = r
        oprm[f] = _params_from_tap(tap, preset, nch)
        want[f, :, :n] = oracle.decode_hotpath([tap.ch[ch] for ch in range(nch)], r, bits, block, preset, ms)
    return ores, oprm, want


LONG_FRAMES = [(2, 16, 65535, 7, 30001), (1, 24, 16384, 4, 16383)]


@pytest.mark.parametrize("kernel", ["default", "wave", "lanes", "pipe", "rows", "rows4", "rows_nf"])
@pytest.mark.parametrize("nch,bits,block,preset,tail", LONG_FRAMES)
def test_decode_forms_at_long_blocks(ctx_env, oracle, monkeypatch, kernel, nch, bits, block, preset, tail):
    """every decode form fed the oracle's residual and parameters of frames of 16384 and 65535 samples (a click in an odd tail) gives
    the oracle's synthesis of them, which is the input; by default a small batch of 65535-sample frames, too long for k_synth_pipe's
    LDS image, runs k_synthesize"""
    from test_gpu_parity import _force_decode_form
    if kernel != "default":
        _force_decode_form(monkeypatch, kernel)
    ms = nch >= 2
    x = long_block_input(nch, bits, block, tail, True, seed=block + 5)
    frames = np.zeros((3, nch, block), dtype=np.int32)
    for f in range(3):
        seg = x[:, f * block:(f + 1) * block]
        frames[f, :, :seg.shape[1]] = seg
    ns = np.array([block, block, tail], dtype=np.uint32)
    ores, oprm, want = oracle_frames(oracle, frames, ns, nch, bits, block, preset, ms)
    for f in range(3):
        assert np.array_equal(want[f, :, :ns[f]], frames[f, :, :ns[f]]), f"frame {f}: the oracle's own round trip"
    with ctx_env({}) as c:
        shape = c.shape(nch, bits, block, preset, ms)
        c.enable_timing(True)
        dec = c.decode_frames_host(shape, ores, oprm, ns)
        synth = c.last_launches(11)
    for f in range(3):
        assert np.array_equal(dec[f, :, :ns[f]], want[f, :, :ns[f]]), f"frame {f}: HIP synthesis of the oracle's residual and parameters"
    if kernel == "default" and block == 65535:
        assert synth == 1, "a small batch of 65535-sample frames decodes with k_synthesize"


@pytest.mark.parametrize("nch,bits,block,preset,ms", [(2, 16, 16384, 2, True), (1, 16, 16384, 7, False), (2, 16, 65535, 7, True), (1, 24, 65535, 2, False)])
def test_hotpath_at_long_blocks(ctx, oracle, nch, bits, block, preset, ms):
    """the encode kernels (k_prep, the lag kernels, the search, k_fir_cascade) at frames of 16384 and 65535 samples: the oracle's taps
    and residual, as test_hotpath_full_frames checks them at 10240"""
    from signals import music_frames
    from test_gpu_parity import _check_taps
    frames = music_frames(2, nch, block, bits, seed=block + preset)
    shape = ctx.shape(nch, bits, block, preset, ms)
    res, prm, st = ctx.encode_frames_host(shape, frames)
    for f in range(2):
        enc = oracle.encoder(nch, bits, 44100, block, preset, ms)
        tap, ores = enc.hotpath(frames[f])
        enc.close()
        _check_taps(tap, prm[f], st[f], preset, nch, f"frame {f}")
        assert np.array_equal(ores, res[f]), f"frame {f}: residual"
    assert np.array_equal(ctx.decode_frames_host(shape, res, prm), frames)
