"""The table of a live session's host-mapped word blocks (csrc/live_pub.h: sizes, plane offsets, strides, empty values, and
the two clears derived from them) without a GPU: tests/sanitize/live_pub_driver.cpp, a stand-alone program built with
AddressSanitizer and UndefinedBehaviorSanitizer, prints every block's size and planes for B in BATCHES, and the bytes of a
sentinel-filled block after pub_clear_all and after pub_clear_stream of the first, a middle and the last stream.  What it
prints is held against LAYOUT below: the layouts the kernels write (live_compact_kernel, live_gate_kernel, the path-cost
kernel, annot_live_kernel, tempo_tail_kernel, ensemble_fuse_kernel) and the readers of include/rtsync.h document, written
out by hand.  Nothing here is computed from the header."""
import os
import struct

import pytest

from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

BATCHES = (1, 2, 3, 7, 64, 65)
SENTINEL = 0xA5
NAN = struct.pack("<Q", 0x7FF8000000000000)
ZERO, MINUS1 = struct.pack("<i", 0), struct.pack("<i", -1)
STREAM, GROUP = 0, 1

# block -> (bytes per stream, planes); a plane: (element bytes, multiple of B in its offset, bytes on top, stride in
# elements, the empty value's bytes, whose word it is)
LAYOUT = {
    # status: int32 [B][4] = status, live position, ref position, feed number
    0: (16, [(4, 0, 0, 4, ZERO, STREAM), (4, 0, 4, 4, ZERO, STREAM), (4, 0, 8, 4, ZERO, STREAM), (4, 0, 12, 4, ZERO, STREAM)]),
    # gate: float64 level[B], then int32 [B][3] = open, seen, passed
    1: (8 + 12, [(8, 0, 0, 1, NAN, STREAM), (4, 8, 0, 3, ZERO, STREAM), (4, 8, 4, 3, ZERO, STREAM), (4, 8, 8, 3, ZERO, STREAM)]),
    # confidence: float64 mean[B], int32 n[B]
    2: (8 + 4, [(8, 0, 0, 1, NAN, STREAM), (4, 8, 0, 1, ZERO, STREAM)]),
    # beats: float64 beat[B], int32 label[B], ref_frame[B]
    3: (8 + 2 * 4, [(8, 0, 0, 1, NAN, STREAM), (4, 8, 0, 1, MINUS1, STREAM), (4, 12, 0, 1, MINUS1, STREAM)]),
    # tempo: float64 slope[B], pos[B], bpm[B], int32 n[B]
    4: (3 * 8 + 4, [(8, 0, 0, 1, NAN, STREAM), (8, 8, 0, 1, NAN, STREAM), (8, 16, 0, 1, NAN, STREAM), (4, 24, 0, 1, ZERO, STREAM)]),
    # consensus: float64 consensus[B], spread[B], dev[B], int32 n_in[B], n_valid[B], strikes[B], out[B]
    5: (3 * 8 + 4 * 4, [(8, 0, 0, 1, NAN, GROUP), (8, 8, 0, 1, NAN, GROUP), (8, 16, 0, 1, NAN, STREAM), (4, 24, 0, 1, ZERO, GROUP),
                        (4, 28, 0, 1, ZERO, GROUP), (4, 32, 0, 1, ZERO, STREAM), (4, 36, 0, 1, ZERO, STREAM)]),
}


@pytest.fixture(scope="module")
def printed():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "live_pub_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "live_pub_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    rc, out, err = _run([exe] + [str(B) for B in BATCHES], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (out[-1000:], err[-2000:])
    lines = {"block": [], "plane": [], "clear": []}
    for text in out.splitlines():
        kind, *items = text.split()
        lines[kind].append(dict(item.split("=") for item in items if "=" in item))
        if kind == "clear":
            lines[kind][-1]["bytes"] = bytes.fromhex(items[-1])
    return lines


def expected(k, B, streams, groups):
    """The block after a clear of `streams`' words (and the group words iff `groups`) on top of the sentinel."""
    per_stream, planes = LAYOUT[k]
    want = bytearray([SENTINEL]) * (per_stream * B)
    for size, mult, plus, stride, empty, whose in planes:
        assert len(empty) == size
        for b in (range(B) if whose == GROUP and groups else [] if whose == GROUP else streams):
            at = mult * B + plus + b * stride * size
            want[at:at + size] = empty
    return bytes(want)


def test_sizes_offsets_strides_and_alignment(printed):
    blocks = {(int(d["B"]), int(d["k"])): int(d["bytes"]) for d in printed["block"]}
    assert blocks == {(B, k): LAYOUT[k][0] * B for B in BATCHES for k in LAYOUT}
    planes = {(int(d["B"]), int(d["k"]), int(d["i"])): d for d in printed["plane"]}
    assert sorted(planes) == sorted((B, k, i) for B in BATCHES for k in LAYOUT for i in range(len(LAYOUT[k][1])))
    for (B, k, i), d in planes.items():
        size, mult, plus, stride, _, whose = LAYOUT[k][1][i]
        got = (8 if int(d["f64"]) else 4, int(d["offset"]), int(d["stride"]), int(d["group"]))
        assert got == (size, mult * B + plus, stride, whose), (B, k, i, d)
        assert int(d["align"]) >= size and int(d["offset"]) % size == 0, (B, k, i, d)  # float64 words 8-byte aligned for every B
        if i and size == 8:
            assert LAYOUT[k][1][i - 1][0] == 8, (k, i)                                 # float64 planes first


def test_clears_write_the_empty_values_and_nothing_else(printed):
    got = {(int(d["B"]), int(d["k"]), d["b"]): d["bytes"] for d in printed["clear"]}
    for B in BATCHES:
        for k in LAYOUT:
            assert got[(B, k, "all")] == expected(k, B, range(B), True), (B, k)
            assert SENTINEL not in got[(B, k, "all")], (B, k)            # no padding: every byte belongs to a word
            for b in {0, B // 2, B - 1}:
                assert got[(B, k, str(b))] == expected(k, B, [b], False), (B, k, b)
    assert len(got) == sum(1 + len({0, B // 2, B - 1}) for B in BATCHES) * len(LAYOUT)
