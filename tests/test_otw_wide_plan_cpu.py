"""How many waves per stream an OTW handle's step kernel runs (otw_plan::threads, csrc/otw_plan.h) without a GPU:
tests/sanitize/otw_wide_plan_driver.cpp, a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer,
prints the kernel-table entry and its threads per workgroup over the whole (window, ring kind, B, cus, RTS_OTW_WAVES) grid.
Every answer is held against the table written out here from DESIGN.md 4.1 ("The kernel table", row "wide forms") and
the comment of otw_plan::threads; nothing is computed from the code under test."""
import itertools
import os

import pytest

from test_otw_plan_cpu import CS, CUS, DOUBLE, FLOAT, LEAN, NONE, TPS, batches, entry_model, window_model
from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

# what a handle takes without RTS_OTW_WAVES where every stream has a CU to itself: the default the measurement of
# profiles/otw_wide_summary.md chose
AUTO_WAVES = 12
OVERRIDES = (0, 8, 12, 16)                     # 0: RTS_OTW_WAVES unset
REFUSED = (-1, 1, 4, 7, 9, 10, 24, 32, 768)    # not a wave count the kernel has: rts_otw_create refuses


def threads_model(W, entry, B, cus, waves):
    """The wide forms exist for the pipelined kernel with a ring at W = 512 alone; auto takes one only at B <= cus."""
    ok, pipelined, ring = entry
    if waves not in OVERRIDES:
        return -1
    if not (ok and pipelined and W == 512 and ring in (FLOAT, DOUBLE)):
        return 512                             # plain, none, none-lean, every other window, no entry at all
    if waves == 0:
        waves = AUTO_WAVES if B <= cus else 8  # cus < B: two workgroups share a CU (float32 below tp_from * cus)
    return 64 * waves


CASES = [(c, spec, tp, cus, B, r, l, waves)
         for c, spec, tp, cus in itertools.product(CS, (0, 1), TPS, CUS)
         for B in batches(tp, cus) for r, l in itertools.product((0, 1), (0, 1)) for waves in OVERRIDES]
BAD_CASES = [(c, 1, 2, 256, B, 0, 0, waves) for c in (100, 245, 500, 501) for B in (64, 256, 257) for waves in REFUSED]


@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "otw_wide_plan_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "otw_wide_plan_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


def run_driver(driver, tmp_path, cases):
    case = tmp_path / "case.txt"
    case.write_text("".join(" ".join(str(v) for v in l) + "\n" for l in cases))
    rc, out, err = _run([driver, str(case)], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (out[-1000:], err[-2000:])
    got = [{k: int(v) for k, v in (item.split("=") for item in text.split())} for text in out.splitlines()]
    assert len(got) == len(cases)
    return got


def test_the_model_is_the_table():
    """The model at hand-written points: an MI355X (256 CUs), default knobs, c = 500."""
    f32, f64 = (1, 1, FLOAT), (1, 1, DOUBLE)
    assert AUTO_WAVES in (8, 12, 16)
    # the last wide batch and the first 512-thread batch, both ring kinds
    assert [threads_model(512, f32, B, 256, 0) for B in (1, 64, 256, 257, 511)] == [64 * AUTO_WAVES] * 3 + [512, 512]
    assert [threads_model(512, f64, B, 256, 0) for B in (256, 257)] == [64 * AUTO_WAVES, 512]
    # the override holds at any batch size, for the kernels that have the form
    assert [threads_model(512, f32, 300, 256, w) for w in (8, 12, 16)] == [512, 768, 1024]
    assert [threads_model(512, f64, 4, 256, w) for w in (8, 12, 16)] == [512, 768, 1024]
    for other in ((1, 1, NONE), (1, 1, LEAN), (1, 0, FLOAT), (1, 0, DOUBLE), (0, 0, NONE)):
        assert {threads_model(512, other, B, 256, w) for B in (1, 256, 600) for w in OVERRIDES} == {512}
    assert {threads_model(W, f32, 4, 256, w) for W in (64, 128, 256, 1024, 2048) for w in OVERRIDES} == {512}
    assert {threads_model(512, f32, 4, 256, w) for w in REFUSED} == {-1}
    # where the rows come from: float32 features between one and two streams per CU keep the float ring and 512 threads
    assert entry_model(512, 1, 2, 256, 300, 0, 0) == f32 and entry_model(512, 1, 2, 256, 256, 1, 1) == f64
    assert entry_model(512, 1, 0, 256, 4, 0, 0) == (1, 1, LEAN)    # tp_from = 0: no wide form at any batch


def test_threads_over_the_whole_grid(driver, tmp_path):
    cases = CASES + BAD_CASES
    got = run_driver(driver, tmp_path, cases)
    reached = set()
    for (c, spec, tp, cus, B, r, l, waves), g in zip(cases, got):
        tag = (c, spec, tp, cus, B, r, l, waves, g)
        W = window_model(c)
        want_entry = entry_model(W, spec, tp, cus, B, r, l)
        assert g["W"] == W and g["ok"] == want_entry[0], tag
        if want_entry[0]:
            assert (g["pipelined"], g["ring"]) == want_entry[1:], tag
        assert g["auto_waves"] == AUTO_WAVES, tag
        assert g["waves_ok"] == int(waves in OVERRIDES), tag
        assert g["threads"] == threads_model(W, want_entry, B, cus, waves), tag
        # the dense mirror and the trace replay: the plain kernel, 512 threads under every valid override
        assert g["mirror_threads"] == (512 if waves in OVERRIDES else -1), tag
        if g["threads"] > 512:
            assert W == 512 and spec and want_entry[2] in (FLOAT, DOUBLE) and (waves or B <= cus), tag
            reached.add((want_entry[2], g["threads"], B <= cus))
    # every wide row is reached: both ring kinds, both widths, at B <= cus and (forced) above it
    want = {(ring, th, low) for ring in (FLOAT, DOUBLE) for th in (768, 1024) for low in (True, False)}
    want -= {(DOUBLE, th, False) for th in (768, 1024)}  # float64 features above one stream per CU have no ring
    assert reached == want, reached ^ want
    assert {g["threads"] for g in got[len(CASES):]} == {-1}
    # B = cus and cus + 1 under auto, tp_from = 2, float32: the boundary itself
    edge = {(k[3], k[4]): g["threads"] for k, g in zip(CASES, got)
            if k[0] == 500 and k[1] == 1 and k[2] == 2 and k[5:] == (0, 0, 0) and k[4] in (k[3], k[3] + 1)}
    assert edge and all(th == (64 * AUTO_WAVES if B <= cus else 512) for (cus, B), th in edge.items()), edge
