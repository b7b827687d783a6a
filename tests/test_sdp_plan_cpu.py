"""The strip DP's workspace layout and launch plan (csrc/sdp_plan.h) without a GPU: tests/sanitize/sdp_plan_driver.cpp, a
stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, prints every section's offset and byte
length, the total, where the carve puts each pointer, and the Plan.  Every number is held against a model written out
here from the array shapes DtwArgs documents (csrc/dtw.hip) and from the rule pick_config's comment states; nothing is
computed from the code under test.  The model of the workspace is the formula the three rts_dtw*_workspace_bytes
functions had before the table existed, so the totals also pin the ABI's byte counts -- and the built library is asked."""
import ctypes
import itertools
import os

import pytest

from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

SECTIONS = ("err", "bnd", "entb", "cross", "lens", "yrec", "codes", "scratch", "ticket")
MS, NS_, BS = (1, 64, 65, 129, 768, 769, 19380), (1, 15, 16, 17, 130, 19380), (1, 2, 63, 64, 65)
WS_CASES = list(itertools.product(MS, NS_, BS)) + [(65, 17, 65535)]


@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "sdp_plan_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "sdp_plan_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


def run_driver(driver, tmp_path, lines, **knobs):
    case = tmp_path / "case.txt"
    case.write_text("".join(" ".join(str(v) for v in l) + "\n" for l in lines))
    env = {k: v for k, v in ENV.items() if not k.startswith("RTS_SDP_")}
    env.update({k: str(v) for k, v in knobs.items()})
    rc, out, err = _run([driver, str(case)], env=env, timeout=120)
    _clean_report(err)
    assert rc == 0, (out[-1000:], err[-2000:])
    got = []
    for text in out.splitlines():
        kind, items = text.split()[0], dict(item.split("=") for item in text.split()[1:])
        got.append((kind, {k: [int(x) for x in v.split(",")] if "," in v else int(v) for k, v in items.items()}))
    assert len(got) == len(lines)
    return got


def up256(v):
    return (v + 255) // 256 * 256


def section_bytes(M, N, B):
    """Bytes in use per section, in the workspace's order: the arrays of DtwArgs, [B] of each."""
    S = -(-M // 64)                                   # strips of 64 rows
    chunks = (N + 63 + 15) // 16                      # 16-step chunks a strip's skewed sweep takes
    codes_words = 64 * S * chunks
    pairs = 64 * S + N
    return [256,                                      # header: the err word
            8 * B * S * N,                            # bnd    [B][n_strips][N] u64
            4 * B * S * N,                            # entb   [B][n_strips][N] i32
            4 * B * S,                                # cross  [B][n_strips] i32
            4 * B * S,                                # lens   [B][n_strips] i32
            8 * B * N * 14,                           # yrec   [B][N][14] f64
            4 * B * codes_words,                      # codes  [B][codes_words] u32
            8 * B * pairs,                            # pscr   [B][scratch_pairs][2] i32
            4 * B]                                    # ticket [B] i32


def test_workspace_sections_size_and_carve(driver, tmp_path):
    got = run_driver(driver, tmp_path, [("ws",) + c for c in WS_CASES])
    from real_time_audio_sync_amd import _build
    lib = ctypes.CDLL(_build.build())                 # loads without a GPU
    assert up256(4 * 64) == 256 and section_bytes(1, 1, 64)[-1] == 256     # B = 64: a ticket section without padding
    for (M, N, B), (kind, g) in zip(WS_CASES, got):
        tag = (M, N, B)
        assert kind == "ws" and (g["M"], g["N"], g["B"]) == tag
        want = section_bytes(M, N, B)
        at = 0
        for name, nbytes in zip(SECTIONS, want):
            off, length = g[name]
            # starts where the previous section's rounded length ends, 256-aligned, increasing
            assert (off, length) == (at, nbytes) and off % 256 == 0, tag + (name, g[name], at, nbytes)
            at += up256(nbytes)
        assert g["total"] == g["bytes"] == at == sum(up256(v) for v in want), tag      # the last section ends at the total
        assert g["carve"] == [g[name][0] for name in SECTIONS], tag                   # the carve is the layout
        assert g["bnd_bytes"] == want[1], tag
        for fn in ("rts_dtw_workspace_bytes", "rts_dtw_paths_workspace_bytes", "rts_dtw_subseq_paths_workspace_bytes"):
            n = ctypes.c_size_t(0)
            assert getattr(lib, fn)(M, N, B, ctypes.byref(n)) == 0 and n.value == at, tag + (fn, n.value, at)


def lds_bytes(ns):
    """Dynamic LDS of a workgroup of ns strips (sdp.h, "Roles" and run_rowgroup's carve): per strip a cost ring of 96
    steps x 64 lanes, three [16][65] output tiles, two chunks of 16 column records of 14 doubles, the DP wave's last two
    code words per lane as [2][64] uint32 (= 64 doubles) and the [2][16] row handed in from the row group above; behind
    them 16 bytes for the workgroup's ticket."""
    return 8 * ns * (96 * 64 + 3 * 16 * 65 + 2 * 16 * 14 + 64 + 2 * 16) + 16


def plan_model(strips, B, res1, res2, pad, config=None, grid_knob=None):
    """pick_config's rule as its comment states it."""
    res1, res2 = max(res1, 1), max(res2, 1)            # an occupancy query that answers 0 counts as one workgroup
    ns = 1 if strips * B <= res1 else 2                # a resident workgroup for every strip of every problem, or two strips each
    if config is not None:
        ns = 1 if config == 1 else 2
    ns = min(ns, strips)
    h = 3 if ns == 1 else 2
    n_rg = -(-strips // ns)
    grid = min(max((res1 if ns == 1 else res2) // B, 1), n_rg)
    if grid_knob is not None and grid_knob > 0:
        grid = grid_knob
    return dict(NS=ns, H=h, grid=grid, n_rg=n_rg, block=64 * ns * (1 + h), smem=lds_bytes(ns) + pad)


# (strips, B, resident1, resident2, pad)
PLAN_CASES = [
    (1, 1, 512, 256, 0),          # one strip: with RTS_SDP_CONFIG=2, NS is capped at 1
    (4, 2, 0, 0, 0),              # resident = 0 is treated as 1
    (8, 64, 512, 256, 0),         # strips * B == resident1: one strip per workgroup
    (27, 19, 512, 256, 0),        # ... and one more (513): two
    (27, 19, 513, 256, 0),
    (20, 1000, 512, 256, 0),      # B larger than the residency: grid 1
    (5, 1, 512, 256, 0),          # residency far above n_rg: grid == n_rg
    (13, 3, 512, 256, 0),         # an odd strip count: the round-up of n_rg with two strips per workgroup
    (303, 1, 256, 128, 0),        # 19380 rows: more row groups than resident workgroups
    (12, 64, 256, 256, 80000),    # the LDS padding of tests/test_sdp_residency_gpu.py
]
PLAN_KNOBS = [{}, dict(RTS_SDP_CONFIG=1), dict(RTS_SDP_CONFIG=2), dict(RTS_SDP_GRID=79), dict(RTS_SDP_GRID=0),
              dict(RTS_SDP_CONFIG=2, RTS_SDP_GRID=1), dict(RTS_SDP_CONFIG=1, RTS_SDP_GRID=3)]


@pytest.mark.parametrize("knobs", PLAN_KNOBS, ids=lambda k: ",".join("%s=%s" % kv for kv in sorted(k.items())) or "default")
def test_launch_plan(driver, tmp_path, knobs):
    got = run_driver(driver, tmp_path, [("plan",) + c for c in PLAN_CASES], **knobs)
    want = [plan_model(*c, config=knobs.get("RTS_SDP_CONFIG"), grid_knob=knobs.get("RTS_SDP_GRID")) for c in PLAN_CASES]
    for c, (kind, g), w in zip(PLAN_CASES, got, want):
        assert kind == "plan" and g == w, (c, knobs, g, w)
        assert g["block"] == 64 * g["NS"] * (1 + g["H"]) and g["smem"] == lds_bytes(g["NS"]) + c[4], (c, knobs, g)
    if not knobs:      # the cases are the ones they claim to be
        by = dict(zip(PLAN_CASES, want))
        assert by[PLAN_CASES[1]]["NS"] == 2 and by[PLAN_CASES[1]]["grid"] == 1
        assert [by[c]["NS"] for c in PLAN_CASES[2:5]] == [1, 2, 1]
        assert by[PLAN_CASES[5]]["grid"] == 1 and by[PLAN_CASES[6]]["grid"] == by[PLAN_CASES[6]]["n_rg"] == 5
        assert by[PLAN_CASES[8]]["n_rg"] == 152 and by[PLAN_CASES[8]]["grid"] == 128
    if knobs == dict(RTS_SDP_CONFIG=2):
        assert want[0]["NS"] == 1 and want[7]["n_rg"] == 7
    if knobs.get("RTS_SDP_GRID") == 79:
        assert all(w["grid"] == 79 for w in want)
