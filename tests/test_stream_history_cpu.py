"""CPU side of tests/test_gpu_stream_history.py: the scenarios of tests/stream_history.py test what they claim, so that a green GPU run
means something.  The list of scenario (a) holds every ordered pair of consumers; where two calls of one consumer follow each other,
what the first leaves in the accumulators would change the second's answer if it were not reset; every accumulator region of
scenarios (a) and (b) begins in bytes that the call before it wrote -- by the host's own plan (linne_amd/csrc/lnn_windows_plan.h),
driven by a small stand-alone program over the block tables of the scenarios' streams, built a second time with the address and
undefined-behaviour sanitizers --; and the damaged streams fail where and why the scenarios say."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import index_cases as ic
import stream_history as sh
from stream_refs import expected_quiet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linne_amd", "csrc")
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lnn_windows_plan.h"
%(digest_defines)s
/* bucketing, an accumulator's bytes and the units in front of the accumulators, per consumer, as lnn_device.hip's WxConsumer table has them */
static const struct { int bucketing; unsigned long long unit, prefix; } CONSUMER[5] = { %(consumers)s };
/* stdin: group_frames consumer nstreams nwindows; per stream: C bits S preset ms nb covered stream_bytes address, then nb x (off first
 * size type nsmp); per window: stream lo n bucket_samples */
struct Stream { WxIndexView x; std::vector<uint64_t> off, first; std::vector<uint32_t> size, type, nsmp; unsigned long long address; };
int main(void)
{
    unsigned gf, consumer, ns, nw;
    if (scanf("%%u %%u %%u %%u", &gf, &consumer, &ns, &nw) != 4 || consumer >= 5) return 2;
    printf("consts %%d %%llu %%llu\n", WX_MAXGROUPS, CONSUMER[consumer].unit, CONSUMER[consumer].prefix);
    std::vector<Stream> st(ns);
    for (Stream &s : st) {
        unsigned long long covered, bytes;
        memset(&s.x, 0, sizeof(s.x));
        if (scanf("%%u %%u %%u %%u %%u %%u %%llu %%llu %%llu", &s.x.shape.num_channels, &s.x.shape.bits_per_sample, &s.x.shape.num_samples_per_block, &s.x.shape.preset,
                    &s.x.shape.ch_process_method, &s.x.nb, &covered, &bytes, &s.address) != 9) return 2;
        s.x.covered = covered; s.x.stream_bytes = bytes;
        for (uint32_t r = 0; r < s.x.nb; r++) {
            unsigned long long off, first; unsigned size, type, nsmp;
            if (scanf("%%llu %%llu %%u %%u %%u", &off, &first, &size, &type, &nsmp) != 5) return 2;
            s.off.push_back(off); s.first.push_back(first); s.size.push_back(size); s.type.push_back(type); s.nsmp.push_back(nsmp);
        }
        s.first.push_back(covered);
        s.x.h_off = s.off.data(); s.x.h_first = s.first.data(); s.x.h_size = s.size.data(); s.x.h_type = s.type.data(); s.x.h_nsmp = s.nsmp.data();
    }
    std::vector<WxRange> rg(nw);
    for (WxRange &r : rg) {
        unsigned k; unsigned long long lo, n, b;
        if (scanf("%%u %%llu %%llu %%llu", &k, &lo, &n, &b) != 4 || k >= ns) return 2;
        memset(&r, 0, sizeof(r));
        r.x = st[k].x; r.stream = (const uint8_t *)(uintptr_t)st[k].address; r.lo = lo; r.n = n; r.live = n != 0; r.bucket_samples = b; r.quiet_min = 1;
        r.fmt = LINNE_AMD_PCM_S32; r.sstride = 1; r.stride = n;
        if (n) r.r1 = (lo + n - 1u < r.x.covered) ? wx_block_of(r.x.h_first, r.x.nb, lo + n - 1u) : r.x.nb;
    }
    WxPlanned p;
    const int why = wx_plan_count(rg.data(), nw, gf, p);
    printf("count %%d %%u\n", why, p.ngroups);
    if (why != WXP_OK) return 0;
    const WxBucketing bucketing = (WxBucketing)CONSUMER[consumer].bucketing;
    std::vector<WxWindow> win(p.nlive); std::vector<WxBucket> side(bucketing ? p.nlive : 0); std::vector<WxBlock> rec(p.total_rec); std::vector<uint32_t> crec(p.total_crec);
    wx_plan_fill(rg.data(), nw, gf, bucketing, p, win.data(), bucketing ? side.data() : NULL, rec.data(), crec.data());
    printf("fill %%llu %%llu %%llu %%llu %%llu\n", (unsigned long long)p.scratch_bytes, (unsigned long long)wx_align(p.scratch_bytes), (unsigned long long)p.nacc,
            (unsigned long long)p.nout, (unsigned long long)p.nmask);
    for (const WxPass &q : p.passes) {
        const struct LINNEAmdShape &shape = rg[p.gwin[q.group]].x.shape;
        const WxScratch sc = wx_scratch(q.nc, shape.num_channels, shape.num_samples_per_block, q.seg_bytes);
        printf("pass %%u %%u %%llu %%llu %%llu\n", q.group, q.nc, (unsigned long long)sc.o_data, (unsigned long long)sc.o_seg, (unsigned long long)sc.bytes);
    }
    return 0;
}
"""


def program_text():
    """the program, with the consumers' accumulator units and the digest tables' size as the product's sources state them"""
    digest = open(os.path.join(CSRC, "lnn_k_digest.h")).read()
    defines = [m.group(0) for m in re.finditer(r"^#define WXD_(?:MAXFRAME|TF_WORDS|TB_WORDS|POW_WORDS)\b[^\n]*", digest, flags=re.M)]
    assert len(defines) == 4
    device = open(os.path.join(CSRC, "lnn_device.hip")).read()
    rows = []
    for name in ("PLACE", "MEASURE", "DIGEST", "QUIET", "COMPARE"):                 # sh.CONSUMERS' order
        m = re.search(r"static const WxConsumer WX_%s = \{([^;]*)\};" % name, device)
        f = [v.strip() for v in m.group(1).split(",")]
        rows.append("{ %s, %s, %s }" % (f[3], f[4], f[5]))                          # bucketing, acc_unit, acc_prefix
    return PROGRAM % {"digest_defines": "\n".join(defines), "consumers": ", ".join(rows)}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_history")
    src = str(d / "layout.cpp")
    with open(src, "w") as f:
        f.write(program_text())
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    exes = []
    for name, extra in (("layout", []), ("layout_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        b = subprocess.run(cmd + ["-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        exes.append(exe)
    return exes


@pytest.fixture(scope="module")
def mat(oracle):
    return sh.material(oracle)


def layout(programs, mat, s):
    """the plan of a step by both builds -> {"consts", "count", "fill", "pass"}; streams at 16-byte aligned addresses of their own"""
    names = list(dict.fromkeys(w[0] for w in s["wins"]))
    text = ["%d %d %d %d" % (s["gf"], sh.CONSUMERS.index(s["call"]), len(names), len(s["wins"]))]
    for j, name in enumerate(names):
        data = mat.data[name]
        h = ic.header_fields(data)
        off, first, size, typ, nsmp = mat.tables(name)
        text.append("%d %d %d %d %d %d %d %d %d" % (h["num_channels"], h["bits_per_sample"], h["num_samples_per_block"], h["preset"], h["ch_process_method"],
                                                    len(off), first[-1], len(data), 0x100000 * (j + 1)))
        text += ["%d %d %d %d %d" % (off[r], first[r], size[r], typ[r], nsmp[r]) for r in range(len(off))]
    buckets = s.get("buckets") or [0] * len(s["wins"])
    text += ["%d %d %d %d" % (names.index(name), lo, n, b) for (name, lo, n), b in zip(s["wins"], buckets)]
    outs = []
    for exe in programs:
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    got = {}
    for line in outs[0].splitlines():
        key, *v = line.split()
        got.setdefault(key, []).append([int(x) for x in v])
    return got


def written(g):
    """(scratch bytes, the accumulator region [start, end)) of a planned step"""
    scratch, o_acc, nacc, nout, nmask = g["fill"][0]
    _, unit, prefix = g["consts"][0]
    return scratch, (o_acc, o_acc + (unit * (prefix + nacc) if unit else 0))


# ---- the pair table and the entry points ----
def test_scenario_a_holds_every_ordered_pair():
    order = sh.order_a()
    assert len(order) >= 26 and [s["call"] for s in sh.scenario_a()] == order
    pairs = set(zip(order, order[1:]))
    assert pairs == {(x, y) for x in sh.CONSUMERS for y in sh.CONSUMERS} and len(pairs) == 25


def test_consecutive_calls_of_scenario_a_use_other_streams_and_parameters():
    for steps in sh.scenario_f():
        for a, b in zip(steps, steps[1:]):
            assert all(x[0] != y[0] for x, y in zip(a["wins"][1:], b["wins"][1:]))          # every window on another stream
            for key in ("buckets", "thr", "mins"):
                if key in a and key in b:
                    assert all(x != y for x, y in zip(a[key], b[key])), key
        assert {b for s in steps for b in s.get("buckets", [])} == {1, 7, 441, 0}
    a, b = sh.scenario_f()
    assert all(x["wins"][1:] != y["wins"][1:] for x, y in zip(a, b))                        # the two contexts: other streams, call for call


def test_scenarios_c_and_d_hold_every_entry_point(mat):
    c = sh.scenario_c(mat)
    assert len(c) == 5
    for fail, good in c:
        assert [s["call"] for s in good] == sh.CONSUMERS
        assert "raises" in fail or any(code != sh.OK for code in fail.get("codes", [])) or fail["call"] == "quiet"
    d = sh.scenario_d(mat)
    assert sh.entry_points(d) == set(sh.CONSUMERS) | set(sh.OTHER_CALLS)
    calls = [s["call"] for s in d]
    refused = next(i for i, s in enumerate(d) if "raises" in s)
    assert d[refused]["call"] == "splice_streams" and all(s.get("count") for s in d[refused + 1:]) and not any(s.get("count") for s in d[:refused])
    assert calls[refused + 1:] == ["splice_streams"] + sh.CONSUMERS + ["index_streams"]
    assert len(d[0]["streams"]) == 16 and d[-1]["streams"] == d[0]["streams"]
    assert [s["on"] for s in d if s["call"] == "set_verify"] == [True, False]
    assert [len(s["streams"]) for s in d if s["call"] == "repair_streams"] == [1, 3]
    # every cut of the splices goes through blocks: fragments are decoded and encoded again
    for s in d:
        if s["call"] == "splice_streams" and "raises" not in s:
            for cuts in s["cuts"]:
                assert sh.expected_splice(mat, cuts)[2] >= 2
    b = sh.scenario_b(mat)
    assert sorted(b) == sorted([f"b/{x}" for x in sh.ACCUMULATING] + [f"b/many/{x}" for x in sh.ACCUMULATING])
    for x in sh.ACCUMULATING:
        s = b[f"b/{x}"]
        assert [t["call"] for t in s] == [x, s[1]["call"], x, s[1]["call"]] and s[1]["call"] != x and [t["gf"] for t in s] == [0, 0, 1, 0]
        assert s[1]["wins"] == s[3]["wins"] and s[1]["wins"][0][2] == 64 and sh.expected(s[1], mat) == sh.expected(s[3], mat)
        assert s[0]["wins"] == s[2]["wins"] == [(s[0]["wins"][0][0], 0, sh.num_samples(s[0]["wins"][0][0]))]
        many = b[f"b/many/{x}"]
        assert len(many[0]["wins"]) == 64 and {w[0] for w in many[0]["wins"]} == set(sh.NAMES) and len(many[1]["wins"]) == 1
    assert [s["call"] for s in sh.scenario_e()] == sh.CONSUMERS


# ---- a stale accumulator would change the answer ----
def mask_words(full, first, n, thr):
    x = np.abs(np.asarray(full)[:, first:first + n].astype(np.int64))
    q = (x <= thr).all(axis=0)
    bits = np.zeros(-(-n // 64) * 64, dtype=bool)
    bits[:n] = q
    return bits.reshape(-1, 64)


def runs_of(bits, first, n, m):
    edge = np.diff(np.concatenate([[0], bits.reshape(-1)[:n].astype(np.int8), [0]]))
    return [(first + int(a), int(b - a)) for a, b in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)) if b - a >= m]


def test_what_the_call_before_leaves_would_change_the_answer(mat):
    """the adjacent calls of one consumer in scenario (a): the second's accumulators are the first's, word for word in the plan's order
    (window after window), folded the way the kernels fold -- or, and, add, min, max -- if nothing resets them"""
    for steps in sh.scenario_f():
        seen = set()
        for prev, s in zip(steps, steps[1:]):
            if prev["call"] != s["call"] or s["call"] == "place":
                continue
            seen.add(s["call"])
            before, want = sh.expected(prev, mat), sh.expected(s, mat)
            assert before != want
            if s["call"] == "measure":
                flat = lambda t: [r for win in t for row in win for r in row]
                old, new = flat(before), flat(want)
                folded = [(min(a[0], b[0]), max(a[1], b[1]), a[2] + b[2], a[3] + b[3]) for a, b in zip(new, old)]
                assert sum(f != n[:4] for f, n in zip(folded, new)) >= len(folded) // 2
            elif s["call"] == "digest":
                flat = lambda t: [r[0] for win in t for r in win]
                old, new = flat(before), flat(want)
                assert sum((a ^ b) != a for a, b in zip(new, old)) >= min(len(new), len(old)) - 2
            elif s["call"] == "compare":
                # the words that come back: a count that is added to, a least key that is lowered
                assert any(b[0] and a[0] + b[0] != a[0] for a, b in zip(want, before))
                assert any(a == (0, 0, 0) and b != (0, 0, 0) for a, b in zip(want, before))
            else:
                old = np.concatenate([mask_words(mat.full[name], a, n, t) for (name, a, n), t in zip(prev["wins"], prev["thr"])])
                at, differ = 0, 0
                for (name, a, n), t, m in zip(s["wins"], s["thr"], s["mins"]):
                    mine = mask_words(mat.full[name], a, n, t)
                    assert runs_of(mine, a, n, max(m, 1)) == expected_quiet(mat.full[name], a, n, t, m)[0]
                    stale = mine | old[at:at + len(mine)] if at + len(mine) <= len(old) else mine
                    differ += runs_of(stale, a, n, max(m, 1)) != runs_of(mine, a, n, max(m, 1))
                    at += len(mine)
                assert differ >= 2
        assert seen == {"measure", "digest", "quiet", "compare"}


# ---- the accumulators land on memory the call before wrote ----
def starts_inside(programs, mat, steps):
    checked = 0
    plans = [layout(programs, mat, s) for s in steps]
    for k in range(1, len(steps)):
        if steps[k]["call"] not in sh.ACCUMULATING:
            continue
        scratch0, (a0, e0) = written(plans[k - 1])
        _, (a1, e1) = written(plans[k])
        assert e1 > a1
        assert a1 < scratch0 or a0 <= a1 < e0, (k, steps[k - 1]["call"], steps[k]["call"], scratch0, (a0, e0), (a1, e1))
        checked += 1
    return checked, plans


def test_accumulators_of_scenario_a_begin_in_bytes_the_call_before_wrote(programs, mat):
    for steps in sh.scenario_f():
        checked, plans = starts_inside(programs, mat, steps)
        assert checked == 15                                     # every pair (X, Y) with Y one of measure, digest, quiet
        for s, g in zip(steps, plans):
            # the anchor's pass is the call's largest: it alone decides where the accumulators begin
            assert max(p[4] for p in g["pass"]) == g["pass"][0][4] == g["fill"][0][0] and g["count"][0] == [0, 5]
            if s["call"] == "quiet":                             # the commit's offsets and counts lie behind the mask words
                scratch, o_acc, nacc, nout, nmask = g["fill"][0]
                assert nacc == nmask + 3 * nout + 1 and nmask == sum(-(-n // 64) for _, _, n in s["wins"])


def test_accumulators_of_scenario_b_begin_in_bytes_the_call_before_wrote(programs, mat):
    in_samples = 0
    for name, steps in sh.scenario_b(mat).items():
        checked, plans = starts_inside(programs, mat, steps)
        assert checked == len(steps) - 1, name
        if "many" in name:
            continue
        # the small call's accumulators: a few hundred bytes (behind the digest's tables of powers) behind a one-block pass, inside
        # the whole-stream call's parameter records or its samples
        whole, small, passes, again = (written(g) for g in plans)
        _, unit, prefix = plans[1]["consts"][0]
        assert small[1][1] - small[1][0] - unit * prefix <= 2048 and 1024 <= small[1][0] < plans[0]["pass"][0][3] < whole[0]
        in_samples += plans[0]["pass"][0][2] <= small[1][0]     # (behind o_data, in front of o_seg)
        assert len(plans[2]["pass"]) > 8 and passes[1][0] == small[1][0] == again[1][0]
    assert in_samples >= 1


# ---- the fixtures are what they claim ----
def test_the_streams(mat):
    assert mat.tables("mixed")[3] == sh.MIXED_TYPES and {sh.COMPRESS, sh.SILENT, sh.RAW} == set(sh.MIXED_TYPES)
    shapes = set()
    for name in sh.NAMES:
        nch, bits, block, preset, ms, nb, tail = sh.SPEC[name]
        off, first, size, typ, nsmp = mat.tables(name)
        assert 12 <= nb <= 24 and 0 < tail < block and nsmp == [block] * nb + [tail] and mat.failure(name) == (-1, sh.OK, 0)
        assert np.array_equal(mat.full[name], sh.pcm_of(name)) and mat.full[name].shape == (nch, nb * block + tail)
        shapes.add((nch, bits, block))
    assert shapes == {(2, 16, 1024), (1, 24, 512), (3, 8, 256)}
    assert {sh.SPEC[n][3] for n in sh.NAMES} == {0, 1, 2, 3, 4, 7} and sh.SPEC["loud"][:4] == (2, 16, 1024, 7)
    assert all(t == sh.COMPRESS for t in mat.tables("loud")[3])
    # loud and near-silent: their tables cannot be taken for each other
    assert np.abs(mat.full["loud"]).max() == 32768 and np.percentile(np.abs(mat.full["hush"]), 99) <= 3 and np.percentile(np.abs(mat.full["faint"]), 99) <= 3
    quiet = {n: expected_quiet(mat.full[n], 0, sh.num_samples(n), 3, 2)[0] for n in sh.NAMES}
    assert all(len(v) >= 5 for v in quiet.values()) and len({tuple(v) for v in quiet.values()}) == 6


def test_the_damaged_streams_fail_where_intended(mat, programs):
    off, first, size, typ, nsmp = mat.tables("loud")
    assert mat.failure("loud/crc") == (mat.crc_block, sh.CORRUPTION, off[mat.crc_block]) and mat.tables("loud/crc") == mat.tables("loud")
    # the Rice damage: every block head and CRC is sound -- the walk finds nothing -- and the whole decode fails
    assert mat.failure("loud/rice") == (-1, sh.OK, 0) and mat.tables("loud/rice") == mat.tables("loud") and mat.rice_code != sh.OK
    a, b = mat.data["loud"], mat.data["loud/rice"]
    differ = [i for i in range(len(a)) if a[i] != b[i]]
    r = mat.rice_block
    assert all(off[r] + 6 <= i < off[r] + size[r] + 6 for i in differ) and any(i >= off[r] + 11 + (size[r] - 5) // 2 for i in differ)
    c = sh.scenario_c(mat)
    rice, crc, beyond, cap, shapes = (f for f, _ in c)
    for s, code, block in ((rice, sh.NG, r), (crc, sh.CORRUPTION, mat.crc_block)):
        for (name, lo, n), want in zip(s["wins"], s["codes"]):
            last = max(k for k in range(len(off)) if first[k] <= lo + n - 1) if "/" in name else -1
            assert want == (code if "/" in name and (last >= block if code == sh.CORRUPTION else first[block] < lo + n and lo < first[block + 1]) else sh.OK)
        assert code in s["codes"] and sh.OK in s["codes"]
    name, lo, n = beyond["wins"][1]
    assert beyond["codes"][1] == sh.INVALID_ARGUMENT and lo + n == sh.num_samples(name) + 1
    (name, lo, n), = cap["wins"][:1]
    runs = expected_quiet(mat.full[name], lo, n, cap["thr"][0], cap["mins"][0])
    assert cap["caps"][0] == runs[1] - 1 >= 2 and len(sh.expected(cap, mat)[0][0]) == runs[1] - 1
    # more shapes than a call takes, the limit read from the header
    few = dict(shapes, wins=shapes["wins"][:64])
    maxgroups = layout(programs, mat, few)["consts"][0][0]
    assert layout(programs, mat, few)["count"][0] == [0, 64] and maxgroups == 64
    assert len({ic.header_fields(mat.data[w[0]])["num_samples_per_block"] for w in shapes["wins"]}) == len(shapes["wins"]) == maxgroups + 1
    assert layout(programs, mat, shapes)["count"][0][0] == 1     # WXP_SHAPES
    # the gapped streams of scenario (d) lose what they are written to lose
    d = sh.scenario_d(mat)
    gaps = [[sh.expected_repair(x)[1]["num_gaps"] for x in s["streams"]] for s in d if s["call"] == "repair_streams"]
    assert gaps == [[1], [2, 2, 2]]
    assert [sh.expected_index(mat, n)[3][0] for n in sh.SIXTEEN] == [-1] * 6 + [mat.crc_block, -1] + [-1] * 8
