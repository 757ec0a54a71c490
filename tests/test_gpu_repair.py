"""GPU tests of repairing damaged resident .lnn streams (Context.repair_streams; include/linne_amd.h LINNEAmd_RepairStreamsDevice):
every case of tests/repair_cases.py alone and all of them in one call against the numpy restatement of the contract, the launch and
synchronisation counts, the capacity verdict behind sentinels, the repaired stream through decode_windows and splice_streams, and the
command line tool.  tests/test_repair_cpu.py holds the restatement's streams to the real reference."""
import os
import subprocess

import numpy as np
import pytest

import linne_amd
import repair_cases as rc
import splice_cases as sc

pytestmark = pytest.mark.gpu

OK, INSUFFICIENT_BUFFER = rc.OK, rc.INSUFFICIENT_BUFFER
SENTINEL = 0xA5
DAMAGE = ["a", "b", "c/huge", "c/7", "d", "e", "f", "g/middle", "g/boundary", "h", "i", "j", "k", "n"]
OTHERS = ["trim/m0/a", "trim/m0/l", "trim/m7/a", "trim/m7/l", "mono/m0/m/intact", "mono/m0/m/broken"]


def as_bytes(t):
    return bytes(t.cpu().numpy())


@pytest.fixture(scope="module")
def table(oracle):
    """name -> (damaged bytes, the restatement's answer); computed once"""
    cases = rc.build_cases(oracle)
    assert sorted(cases) == sorted([f"{s}/{d}" for s in rc.SOURCES for d in DAMAGE] + OTHERS)
    return {name: (data, rc.repair(data)) for name, (data, _) in cases.items()}


def check(ctx, oracle, name, data, want, got, code, decode=True):
    stream, report = got
    if want is None:                                            # a header error: the index's code, nothing written
        with pytest.raises(linne_amd.LinneAmdError) as e:
            ctx.index_stream(data)
        assert stream is None and code == e.value.code != OK and report["out_bytes"] == 0 and report["gaps"] == [], name
        return
    out, rep = want
    assert code == OK and as_bytes(stream) == out, name
    assert report == rep, name
    if decode:
        ix = ctx.index_stream(stream)
        assert ix.failure()[0] == -1, name
        assert np.array_equal(ctx.decode_stream(stream, index=ix).cpu().numpy(), rc.expected_pcm(oracle, data, out)), name
        ix.close()


@pytest.mark.parametrize("case", DAMAGE + ["others"])
def test_every_case_alone(ctx, oracle, table, case):
    names = OTHERS if case == "others" else [f"{s}/{case}" for s in rc.SOURCES]
    for name in names:
        data, want = table[name]
        got, codes = ctx.repair_streams([data], return_codes=True)
        check(ctx, oracle, name, data, want, got[0], codes[0])
        if name.endswith("/a"):
            assert as_bytes(got[0][0]) == data and got[0][1]["num_gaps"] == 0 and got[0][1]["exact"] == 1


def candidates(b):
    """the block candidates of a stream (the checks in front of the CRC)"""
    n, p = 0, b.find(b"\xff\xff", 30)
    while p >= 0:
        if p + 11 <= len(b) and 5 <= int.from_bytes(b[p + 2:p + 6], "big") <= len(b) - p - 6:
            n += 1
        p = b.find(b"\xff\xff", p + 1)
    return n


def doubling_depth(table, names):
    most = max(candidates(table[n][0]) for n in names if table[n][1] is not None)
    K = 1
    while (1 << K) <= most:
        K += 1
    return K


def test_batch_in_one_call(oracle, table):
    import torch
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        names = sorted(table)
        flat = torch.from_numpy(np.frombuffer(b"".join(table[n][0] for n in names), dtype=np.uint8).copy()).cuda()
        views, at = {}, 0
        for n in names:                                         # adjacent views of one buffer, at every byte alignment
            views[n] = flat[at:at + len(table[n][0])]
            at += len(table[n][0])
        assert {views[n].data_ptr() % 4 for n in names} == {0, 1, 2, 3}
        got, codes = c.repair_streams([views[n] for n in names], return_codes=True)       # (warm: the scratch has grown)
        census = []
        for which in (names[:3], names):
            got, codes = c.repair_streams([views[n] for n in which], return_codes=True)
            census.append((c.last_repair_count(5), c.last_repair_count(6) - (doubling_depth(table, which) - 1)))
        assert census[0] == census[1] and census[0][0] == 5, census
        for i, n in enumerate(names):
            check(c, oracle, n, table[n][0], table[n][1], got[i], codes[i], decode=False)
        good = [n for n in names if table[n][1] is not None]
        assert c.last_repair_count(0) == len(good) and c.last_repair_count(1) == sum(table[n][1][1]["kept_blocks"] for n in good)
        assert c.last_repair_count(2) == sum(table[n][1][1]["fill_blocks"] for n in good) and c.last_repair_count(3) == sum(table[n][1][1]["num_gaps"] for n in good)
        assert as_bytes(flat) == b"".join(table[n][0] for n in names)      # the sources are as they were
        with pytest.raises(linne_amd.LinneAmdError) as e:      # without return_codes a failing stream raises, with every stream's code
            c.repair_streams([views[n] for n in names])
        assert e.value.codes == codes and e.value.code == next(x for x in codes if x != OK) and "repair " in str(e.value)
    finally:
        c.close()


def test_capacity(ctx, table):
    import torch
    small, whole = table["stereo/m7/ms/k"], table["mono/m0/j"]
    need = len(small[1][0])
    room = 1 << 16
    buf = torch.full((2 * room,), SENTINEL, dtype=torch.uint8, device="cuda")
    src = [ctx._stream_bytes(small[0]), ctx._stream_bytes(whole[0])]
    arr = (linne_amd.Repair * 2)()
    for i in range(2):
        arr[i].d_stream, arr[i].stream_bytes, arr[i].d_out = src[i].data_ptr(), src[i].numel(), buf.data_ptr() + i * room + 3
    arr[0].capacity, arr[1].capacity = need - 1, len(whole[1][0])
    ctx._fence()
    ret = linne_amd.lib.LINNEAmd_RepairStreamsDevice(ctx.h, arr, 2)
    assert ret == INSUFFICIENT_BUFFER and linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode().startswith("repair 0: ")
    assert (arr[0].result, arr[0].out_bytes, arr[0].kept_blocks, arr[0].num_gaps) == (INSUFFICIENT_BUFFER, need, 0, 0)
    assert (arr[1].result, arr[1].out_bytes) == (OK, len(whole[1][0]))
    image = np.full(2 * room, SENTINEL, dtype=np.uint8)
    image[room + 3:room + 3 + len(whole[1][0])] = np.frombuffer(whole[1][0], dtype=np.uint8)
    assert np.array_equal(buf.cpu().numpy(), image)             # the one that does not fit untouched, its neighbour whole
    arr[0].capacity = need                                      # exactly the room it needs
    assert linne_amd.lib.LINNEAmd_RepairStreamsDevice(ctx.h, arr, 2) == OK and arr[0].out_bytes == need
    image[3:3 + need] = np.frombuffer(small[1][0], dtype=np.uint8)
    assert np.array_equal(buf.cpu().numpy(), image)


def test_downstream_windows_and_splice(ctx, oracle, table):
    data, (out, report) = table["stereo/m0/ms/k"]
    S = rc.BLOCK
    g = report["gaps"][0]
    assert g["first_sample"] == 3 * S and g["num_samples"] > 600
    repaired = ctx.repair_streams([data])[0][0]
    restated = ctx._stream_bytes(out)
    want = rc.expected_pcm(oracle, data, out)
    answers = []
    for t in (repaired, restated):
        ix = ctx.index_stream(t)
        lo, n = 2 * S + 100, 2 * S + 300                        # a window from a kept block over the fill into the next kept block
        win = ctx.decode_windows([(t, ix, lo, n)])[0].cpu().numpy()
        assert np.array_equal(win, want[:, lo:lo + n]) and not win[:, 3 * S - lo:3 * S - lo + g["num_samples"]].any()
        cut = as_bytes(ctx.splice_streams([[(t, ix, S, 2 * S + 500)]])[0])      # a cut that ends inside the fill block
        answers.append((win.tobytes(), cut))
        ret, pcm, _ = oracle.decode_whole(cut)
        assert ret == OK and np.array_equal(pcm, want[:, S:3 * S + 500])
        ix.close()
    assert answers[0] == answers[1]


def test_cli_repairs_a_file(table, tmp_path):
    data, (out, report) = table["stereo/m7/ms/b"]
    cli = os.path.join(os.path.dirname(os.path.abspath(linne_amd.__file__)), "linne_amd_cli")
    src, dst = tmp_path / "in.lnn", tmp_path / "out.lnn"
    src.write_bytes(data)
    r = subprocess.run([cli, "-r", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert dst.read_bytes() == out
    assert "kept blocks 11" in r.stderr and "gaps 1" in r.stderr and "exact 1" in r.stderr, r.stderr
