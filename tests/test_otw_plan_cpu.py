"""Which step kernel an OTW handle takes (csrc/otw_plan.h) without a GPU: tests/sanitize/otw_plan_driver.cpp, a stand-alone
program built with AddressSanitizer and UndefinedBehaviorSanitizer, prints the band window, the kernel-table entry and the
band-fill gate of every case.  Every answer is held against a table written out here from DESIGN.md 4.1 ("The kernel
table") and the comments of otw_plan.h; nothing is computed from the code under test."""
import itertools
import os

import pytest

from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

FLOAT, DOUBLE, NONE, LEAN = 0, 1, 2, 3          # RTS_OTW_RING_* of include/rtsync.h
# the last band width of each LDS window (W >= c + 12)
LAST_C = ((52, 64), (116, 128), (244, 256), (500, 512), (1012, 1024), (2036, 2048))
CS = (1, 52, 53, 116, 117, 244, 245, 500, 501, 1012, 1013, 2036)
WANT_W = (64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024, 2048, 2048)
TPS, CUS = (0, 1, 2, 3), (1, 8, 256, 304)


def window_model(c):
    return next(w for last, w in LAST_C if c <= last)


def batches(tp, cus):
    return sorted({b for b in (1, cus - 1, cus, cus + 1, tp * cus - 1, tp * cus, tp * cus + 1, 65535) if b >= 1})


def entry_model(W, spec, tp, cus, B, ref64, live64):
    """(ok, pipelined, ring): the rows of DESIGN.md 4.1's kernel table, top to bottom."""
    if W >= 1024:                                # no ring fits beside the bands; the plain kernel has no such entry
        return (1, 1, NONE) if spec else (0, 0, NONE)
    both_f32 = not ref64 and not live64
    if not spec:                                 # RTS_OTW_SPEC=0: the plain kernel keeps its ring at every batch size
        return (1, 0, FLOAT if both_f32 else DOUBLE)
    if B >= tp * cus:                            # RTS_OTW_TP_FROM streams per CU or more
        return (1, 1, LEAN)
    if both_f32:
        return (1, 1, FLOAT)
    return (1, 1, DOUBLE if B <= cus else NONE)  # a CU for every stream: the ring stays


def fill_model(fill, max_new, c, mirror):
    """The band fill runs in front of a launch that can bring a fresh stream c frames: RTS_OTW_FILL on, 2 <= c <= 500, no
    dense mirror or trace (include/rtsync.h, rts_otw_read_fill)."""
    return int(bool(fill) and max_new >= c and 2 <= c <= 500 and not mirror)


ENTRY_CASES = [(c, spec, tp, cus, B, r, l, 1, c, 0)
               for c, spec, tp, cus in itertools.product(CS, (0, 1), TPS, CUS)
               for B in batches(tp, cus) for r, l in itertools.product((0, 1), (0, 1))]
FILL_CASES = [(c, 1, 2, 256, 4, 1, 1, fill, max_new, mirror)
              for c in CS for fill in (0, 1, 7) for mirror in (0, 1)
              for max_new in (0, 1, c - 1, c, c + 1, 4000)]


@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "otw_plan_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "otw_plan_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


def run_driver(driver, tmp_path, cases):
    case = tmp_path / "case.txt"
    case.write_text("".join(" ".join(str(v) for v in l) + "\n" for l in cases))
    rc, out, err = _run([driver, str(case)], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (out[-1000:], err[-2000:])
    got = []
    for text in out.splitlines():
        items = dict(item.split("=") for item in text.split())
        got.append({k: tuple(int(x) for x in v.split(",")) if "," in v else int(v) for k, v in items.items()})
    assert len(got) == len(cases)
    return got


def test_the_model_is_the_table():
    """The models above at hand-written points, so that a slip in them does not pass as the rule."""
    assert [window_model(c) for c in CS] == list(WANT_W)
    # an MI355X, 256 CUs, default knobs, W = 512, float64 features: ring, no ring, lean
    assert [entry_model(512, 1, 2, 256, B, 1, 1) for B in (256, 257, 511, 512)] == \
        [(1, 1, DOUBLE), (1, 1, NONE), (1, 1, NONE), (1, 1, LEAN)]
    # a float32 reference: the float ring for float32 live input, the history (float64) as above
    assert entry_model(256, 1, 2, 256, 300, 0, 0) == (1, 1, FLOAT) and entry_model(256, 1, 2, 256, 300, 0, 1) == (1, 1, NONE)
    assert entry_model(64, 1, 0, 256, 1, 0, 0) == (1, 1, LEAN)          # RTS_OTW_TP_FROM=0 forces the lean flavour
    assert entry_model(64, 1, 1, 8, 7, 1, 0) == (1, 1, DOUBLE) and entry_model(64, 1, 1, 8, 8, 1, 0) == (1, 1, LEAN)
    assert entry_model(1024, 0, 2, 256, 4, 0, 0)[0] == 0 and entry_model(2048, 1, 2, 256, 4000, 0, 0) == (1, 1, NONE)
    assert entry_model(128, 0, 2, 256, 4000, 0, 0) == (1, 0, FLOAT) and entry_model(128, 0, 2, 256, 4000, 0, 1) == (1, 0, DOUBLE)
    assert [fill_model(1, n, 245, 0) for n in (244, 245)] == [0, 1] and fill_model(1, 9, 1, 0) == 0
    assert fill_model(1, 4000, 501, 0) == 0 and fill_model(0, 4000, 100, 0) == 0 and fill_model(1, 4000, 100, 1) == 0


def test_window_entry_and_fill_gate(driver, tmp_path):
    cases = ENTRY_CASES + FILL_CASES
    got = run_driver(driver, tmp_path, cases)
    reached = {}
    for (c, spec, tp, cus, B, r, l, fill, max_new, mirror), g in zip(cases, got):
        tag = (c, spec, tp, cus, B, r, l, fill, max_new, mirror, g)
        W = window_model(c)
        assert g["W"] == W and W >= c + 12 and (W == 64 or W // 2 < c + 12), tag
        want = entry_model(W, spec, tp, cus, B, r, l)
        assert g["ok"] == want[0], tag
        if want[0]:
            assert (g["pipelined"], g["ring"]) == want[1:], tag
        assert g["mirror"] == (1, 0, NONE if W >= 1024 else DOUBLE), tag    # the plain kernel, whatever RTS_OTW_SPEC
        assert g["fill"] == fill_model(fill, max_new, c, mirror), tag
        if want[0] and want[1]:
            reached.setdefault(W, set()).add(want[2])
    # a table from which a row has vanished fails: every ring kind of the pipelined kernel at every window that has four
    for W in (64, 128, 256, 512):
        assert reached[W] == {FLOAT, DOUBLE, NONE, LEAN}, (W, reached[W])
    assert reached[1024] == reached[2048] == {NONE}
    assert {g["fill"] for g in got[len(ENTRY_CASES):]} == {0, 1}
    # the no-ring row exists only strictly between one stream per CU and tp_from streams per CU
    none_rows = [k for k, g in zip(ENTRY_CASES, got) if k[0] <= 500 and g["ok"] and g["pipelined"] and g["ring"] == NONE]
    assert none_rows and all(k[3] < k[4] < k[2] * k[3] and (k[5] or k[6]) for k in none_rows)
