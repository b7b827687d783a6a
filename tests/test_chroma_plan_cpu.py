"""The chroma kernels' LDS layouts, kernel choice and grids (csrc/chroma_plan.h) without a GPU: tests/sanitize/
chroma_plan_driver.cpp, a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, prints every
section's byte offset and the total of every kernel for fft_len 64 .. 8192, the kernel a call gets and its grid.  Every
number is held against a model written out here from the array shapes the kernels' comments document (csrc/chroma.hip):
the sections follow one another without gaps, the total is the end of the last one, and the reduction scratch is what
project_normalize touches, [frames of a pass][12][16] doubles.  Nothing is computed from the code under test."""
import os

import pytest

from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

GENERIC, K4096, BIG, PROJECT = range(4)
FR, BIG_FR = 4, 2        # frames per group: kChromaFR, kBigFR (the values tests/test_chroma_paths_gpu.py restates too)
BATCH_GRID = 64          # gridDim.x cap of the batched launches
PROJECT_GRID = 1024
LENGTHS = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
RED = 12 * 16            # doubles of reduction scratch per frame a team projects in one pass: [12][16] row totals


@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "chroma_plan_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "chroma_plan_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


def run_driver(driver, tmp_path, lines):
    case = tmp_path / "case.txt"
    case.write_text("".join(" ".join(str(v) for v in l) + "\n" for l in lines))
    rc, out, err = _run([driver, str(case)], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (out[-1000:], err[-2000:])
    got = []
    for text in out.splitlines():
        items = dict(item.split("=") for item in text.split()[1:])
        got.append({k: [int(x) for x in v.split(",")] for k, v in items.items()})
    return got


def shapes(kernel, L):
    """(teams, double2 slots of a team's FFT buffer, double2 slots of the twiddle table, frames per group, doubles per
    spectrum, frames a team projects in one pass) as the kernels' comments give them."""
    n2 = L // 2
    return {GENERIC: (2, n2, n2 // 2, FR, n2 + 2, FR // 2),               # two teams, quarter-circle table in LDS
            K4096: (2, 2048 + 2048 // 8, 1024, FR, 2048 + 2, FR // 2),    # buffer padded by one slot per 8
            BIG: (1, n2, 0, BIG_FR, n2 + 2, BIG_FR),                      # one team, twiddles from L2
            PROJECT: (1, 0, 0, FR, n2 + 2, FR)}[kernel]                   # spectra only


def test_lds_sections_and_totals(driver, tmp_path):
    got = run_driver(driver, tmp_path, [("lds", L) for L in LENGTHS])
    assert len(got) == 4 * len(LENGTHS)
    in_z = {}
    for i, g in enumerate(got):
        L, kernel = LENGTHS[i // 4], i % 4
        tag = (L, kernel)
        assert (g["L"], g["kernel"]) == ([L], [kernel]), tag
        teams, z_slots, tw_slots, frames, sstride, proj_max = shapes(kernel, L)
        assert (g["teams"], g["group"], g["sstride"]) == ([teams], [frames], [sstride]), tag
        assert sstride >= (4096 if kernel == K4096 else L) // 2 + 1, tag     # a spectrum holds every rfft bin
        # the sections in order, each where the one before ends: FFT buffers, twiddles, spectra
        at = 0
        for t in range(teams):
            assert g["z"][t] == at and at % 16 == 0, tag          # double2
            at += 16 * z_slots
        assert g["z_bytes"] == [16 * z_slots], tag
        assert g["tw"] == [at] and at % 16 == 0, tag              # double2
        at += 16 * tw_slots
        assert g["spec"] == [at] and at % 16 == 0, tag            # filled as doubles, read as doubles
        at += 8 * frames * sstride
        # the scratch: a team's own FFT buffer when it fits in it (the one aliasing), else behind the spectra
        red = proj_max * RED
        assert g["red_bytes"] == [8 * red], tag
        in_z[tag] = bool(g["red_in_z"][0])
        assert in_z[tag] == (16 * z_slots >= 8 * red), tag
        for t in range(teams):
            if in_z[tag]:
                assert g["red"][t] == g["z"][t], tag
            else:
                assert g["red"][t] == at and at % 8 == 0, tag
                at += 8 * red
        assert g["total"] == [at], tag
        if kernel in (K4096, PROJECT) or (kernel == GENERIC and L <= 4096) or (kernel == BIG and L == 8192):
            assert g["total"][0] <= 160 * 1024, tag               # what a plan of this length launches fits a CU's LDS
    # the cases are the ones they claim to be: two frames' row totals are 384 doubles, a team's buffer holds fft_len
    # doubles, so the generic kernel's scratch moves into it at fft_len 512; the project kernel's is 768 doubles
    assert [in_z[(L, GENERIC)] for L in LENGTHS] == [False] * 3 + [True] * 5
    by = {(LENGTHS[i // 4], i % 4): g for i, g in enumerate(got)}
    assert by[(4096, K4096)]["total"] == [155712] and by[(4096, PROJECT)]["red_bytes"] == [8 * 768]
    assert by[(256, GENERIC)]["red_bytes"] == [8 * 384] and by[(256, GENERIC)]["total"] == [16 * (2 * 128 + 64) + 8 * 4 * 130 + 2 * 8 * 384]
    assert all(in_z[(L, K4096)] for L in LENGTHS) and in_z[(8192, BIG)] and not any(in_z[(L, PROJECT)] for L in LENGTHS)


EDGE = 0x7fffffff       # chroma.hip indexes samples with 32 bits when span + 2 L + n_frames * hop stays below this


def test_flavour_rule(driver, tmp_path):
    hop, nf = 2048, 19379
    below = EDGE - 1 - 2 * 4096 - nf * hop       # the sum is EDGE - 1: the specialised kernel
    cases = [(4096, hop, below, nf, K4096), (4096, hop, below + 1, nf, GENERIC),   # one below the edge, at it
             (4096, hop, 1 << 40, nf, GENERIC), (4096, 1 << 20, (1 << 30) + 4096, 1025, GENERIC),
             (4096, hop, 0, 0, K4096), (4096, 1, EDGE - 1 - 8192 - 7, 7, K4096), (4096, 1, EDGE - 8192 - 7, 7, GENERIC),
             (8192, hop, 1000, 5, BIG), (8192, hop, 1 << 40, 5, BIG)]
    cases += [(L, L // 4, 100000, 50, GENERIC) for L in LENGTHS[:6]]
    assert below + 2 * 4096 + nf * hop == EDGE - 1
    got = run_driver(driver, tmp_path, [("flavour",) + c[:4] for c in cases])
    assert [g["kernel"][0] for g in got] == [c[4] for c in cases]


def test_grids(driver, tmp_path):
    cases = []   # kernel, n_frames, cus, batched -> grid
    for cus in (1, 8, 256, 304):
        for kernel, per in ((GENERIC, FR), (K4096, FR), (BIG, BIG_FR)):
            cap = 4 * cus if kernel == BIG else cus
            for groups in (1, 2, cap - 1, cap, cap + 1, 3 * cap + 1):
                if groups < 1:
                    continue
                for n in (per * (groups - 1) + 1, per * groups):          # a partial and a full last group
                    cases.append((kernel, n, cus, 0, min(groups, cap)))
                    cases.append((kernel, n, cus, 1, min(groups, BATCH_GRID)))
    for groups in (1, PROJECT_GRID - 1, PROJECT_GRID, PROJECT_GRID + 1, PROJECT_GRID + PROJECT_GRID // 3 + 1):
        for n in (FR * (groups - 1) + 1, FR * (groups - 1) + 3, FR * groups):
            cases.append((PROJECT, n, 256, 0, min(groups, PROJECT_GRID)))
    cases.append((K4096, 19379, 256, 0, 256))                            # the benchmark's launch
    assert any(c[3] and c[4] == BATCH_GRID for c in cases) and any(c[0] == BIG and c[4] == 4 * 256 for c in cases)
    got = run_driver(driver, tmp_path, [("grid",) + c[:4] for c in cases])
    for c, g in zip(cases, got):
        assert g["x"] == [c[4]], c
