"""CPU side of the block-head scan that StreamIndexesCreate and RepairStreamsDevice share: where its lists lie
(linne_amd/csrc/lnn_block_scan.h, driven by a small stand-alone program), and that the streams tests/test_gpu_block_scan.py runs both
calls over are the ones it needs."""
import os
import subprocess

import pytest

import scan_cases as sc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "linne_amd", "csrc")
PARTS = ("o_st", "o_row0", "o_early", "o_crow", "o_hdr", "o_seg", "o_len", "o_late", "bytes")
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lnn_block_scan.h"
int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    const struct IbLists a = ib_lists(strtoull(argv[1], 0, 10), strtoull(argv[2], 0, 10), strtoull(argv[3], 0, 10), strtoull(argv[4], 0, 10), strtoull(argv[5], 0, 10));
    printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)a.o_st, (unsigned long long)a.o_row0, (unsigned long long)a.o_early,
            (unsigned long long)a.o_crow, (unsigned long long)a.o_hdr, (unsigned long long)a.o_seg, (unsigned long long)a.o_len, (unsigned long long)a.o_late,
            (unsigned long long)a.bytes);
    return 0;
}
"""
ST, SLOT, TABLES = 40, 32, 3000                                 # a stream record, a header slot, the tables (any sizes do: the rule is the header's)


@pytest.fixture(scope="module")
def lists(tmp_path_factory):
    d = tmp_path_factory.mktemp("block_scan")
    src, exe = str(d / "lists.c"), str(d / "lists")
    with open(src, "w") as f:
        f.write(PROGRAM)
    b = subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr

    def run(T, early, late):
        r = subprocess.run([exe, str(T), str(ST), str(SLOT), str(early), str(late)], capture_output=True, text=True)
        assert r.returncode == 0
        return dict(zip(PARTS, (int(v) for v in r.stdout.split())))
    return run


def up(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("T", [1, 2, 257])
def test_lists_are_aligned_disjoint_and_in_order(lists, T):
    """the index's lists (nothing early, the tables late) and the repair call's (bounds and tables early, two sets of segment bounds
    late): every part 256-byte aligned, in the documented order, with room for what it holds; the repair call's lists begin as the
    index's do, and its upload [o_st, o_crow) holds exactly the streams, row0 and its early part"""
    index = lists(T, 0, TABLES)
    repair = lists(T, up(8 * T) + TABLES, up(8 * (T + 1)) + 8 * (T + 1))
    for a, early, late in ((index, 0, TABLES), (repair, up(8 * T) + TABLES, up(8 * (T + 1)) + 8 * (T + 1))):
        need = {"o_st": ST * T, "o_row0": 8 * (T + 1), "o_early": early, "o_crow": 8 * (T + 1), "o_hdr": SLOT * T, "o_seg": 8 * (T + 1), "o_len": 8 * T, "o_late": late}
        assert all(a[p] % 256 == 0 for p in PARTS)
        assert a["o_st"] == 0
        for p, q in zip(PARTS, PARTS[1:]):                      # q begins behind all p holds, and no further than the alignment asks
            assert a[q] == up(a[p] + need[p]), (p, q)
    assert (index["o_st"], index["o_row0"], index["o_early"]) == (repair["o_st"], repair["o_row0"], repair["o_early"])
    assert index["o_crow"] == index["o_early"]                  # the index uploads the streams and row0, nothing more
    assert repair["o_crow"] - repair["o_early"] == up(up(8 * T) + TABLES)
    # the same bytes as when every part was laid out by its call: the parts' aligned sizes, whatever their order
    assert index["bytes"] == up(ST * T) + 3 * up(8 * (T + 1)) + up(SLOT * T) + up(8 * T) + up(TABLES)
    assert repair["bytes"] == up(ST * T) + 5 * up(8 * (T + 1)) + up(SLOT * T) + 2 * up(8 * T) + up(TABLES)


def test_the_undamaged_streams_are_enough(oracle, product):
    """what tests/test_gpu_block_scan.py needs of the case builders: at least three undamaged streams, one of SILENT and RAW blocks
    only and one with COMPRESS blocks among them, one of exactly one block, and none of more than a few blocks' worth of bytes"""
    streams = sc.undamaged_streams(oracle, product)
    assert len(streams) >= 3 and len({name for name, _ in streams}) == len(streams)
    kinds = [sc.block_types(data) for _, data in streams]
    assert any(k <= {sc.SILENT, sc.RAW} for k in kinds) and any(sc.COMPRESS in k for k in kinds)
    counts = [len(sc.blocks_of(data)[0]) for _, data in streams]
    assert 1 in counts and max(counts) <= 12 and all(len(data) < 64 * 1024 for _, data in streams)
    assert [len(data) for _, data in sc.stumps(product)] == [sc.HEADER - 1, sc.HEADER]
