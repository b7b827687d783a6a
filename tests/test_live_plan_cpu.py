"""The host's plan of a live feed (csrc/live_plan.h: which feeds are refused, the launch geometry, the mirror of the device
counts) without a GPU: tests/sanitize/live_plan_driver.cpp, a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer, runs live_plan_feed / live_mirror_commit over whole feed schedules, and every number it
prints is held against a model made of drop() (tests/test_live_model_cpu.py), avail() (tests/resample_model.py) and the
carry rule of live_diff_kernel: a stream hands the tracker max(n - skip, 0) of its n new chroma columns, skip = 1 until
it has completed its first column.  Nothing here is computed from the code under test."""
import functools
import os

import numpy as np
import pytest

from resample_model import avail
from test_live_model_cpu import B, GEOMETRIES, build_schedule, drop, max_pending
from test_resample_cpu import EXPECT, RATES
from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

OK, NEGATIVE, STAGING, PENDING = 0, 1, 2, 3       # LiveRefusal
L_FFT, HOP, CAP = 1024, 512, 6000                 # the live cases of tests/test_resample_gpu.py
RS_B = 4

avail_cached = functools.lru_cache(maxsize=None)(avail)


@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "live_plan_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "live_plan_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


def model(geom, feeds):
    """What every feed plans and leaves behind: one dict per feed, keyed like the driver's line."""
    n_streams, L, hop, cap, diff, rs_L, rs_M, rs_half, in_cap = geom
    pend, carry, tot = [0] * n_streams, [0] * n_streams, [0] * (2 * n_streams)
    lines = []
    for counts in feeds:
        rule, stream, new = OK, -1, []
        for b, c in enumerate(counts):
            n = c
            if c < 0:
                rule = NEGATIVE
            elif rs_L and c > in_cap:
                rule = STAGING
            else:
                if rs_L:
                    n = avail_cached(tot[2 * b] + c, rs_L, rs_M, rs_half) - tot[2 * b + 1]
                if pend[b] + n > cap:
                    rule = PENDING
            if rule != OK:
                stream = b
                break
            new.append(n)
        line = dict(rule=rule, stream=stream, same=1)
        if rule == OK:
            cols = []
            for b in range(n_streams):
                pend[b], n = drop(pend[b] + new[b], L, hop)
                cols.append((n, max(n - (0 if carry[b] else 1), 0)))
                carry[b] = int(carry[b] or n > 0)
                if rs_L:
                    tot[2 * b], tot[2 * b + 1] = tot[2 * b] + counts[b], tot[2 * b + 1] + new[b]
            line.update(total=sum(counts), offs=[sum(counts[:b]) for b in range(n_streams)],
                        n_max=max(n for n, _ in cols), n_max_diff=max(d for _, d in cols) if diff else 0,
                        n_out_max=max(new) if rs_L else 0, nout=list(new) if rs_L else None)
        line.update(pending=list(pend), carry=list(carry) if diff else None, tot=list(tot) if rs_L else None)
        lines.append(line)
    return lines


def run_driver(driver, tmp_path, geom, feeds):
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(int(v)) for v in geom) + " %d\n" % len(feeds)
                    + "".join(" ".join(str(int(c)) for c in f) + "\n" for f in feeds))
    rc, out, err = _run([driver, str(case)], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (out[-1000:], err[-2000:])
    lines = []
    for text in out.splitlines():
        d = {}
        for item in text.split():
            k, v = item.split("=")
            d[k] = None if v == "-" else [int(x) for x in v.split(",")] if k in LISTS else int(v)
        assert d.pop("feed") == len(lines)
        lines.append(d)
    return lines


LISTS = ("offs", "nout", "pending", "carry", "tot")


def check(driver, tmp_path, geom, feeds):
    want = model(geom, feeds)
    got = run_driver(driver, tmp_path, geom, feeds)
    assert len(got) == len(want) == len(feeds)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, feeds[i], g, w)       # every number; refusals: same feed, stream and rule; mirror untouched
    return want


@pytest.mark.parametrize("diff", [0, 1])
@pytest.mark.parametrize("L,hop", GEOMETRIES)
def test_plan_of_the_live_schedules(driver, tmp_path, L, hop, diff):
    sched = build_schedule(L, hop, seed=7 * L + hop)
    feeds = [f["counts"] for f in sched]
    cap = max_pending(L, hop)
    want = check(driver, tmp_path, (B, L, hop, cap, diff, 0, 0, 0, 0), feeds)
    # the schedule's own bookkeeping agrees with the model about which feed is refused, and it is the edge stream's
    assert [w["rule"] != OK for w in want] == [f["refused"] for f in sched] and sum(f["refused"] for f in sched) == 1
    refused = [w for w in want if w["rule"] != OK][0]
    assert (refused["rule"], refused["stream"]) == (PENDING, 1)
    k = [w["rule"] for w in want].index(PENDING)
    assert want[k]["pending"] == want[k - 1]["pending"]
    # the boundaries are in: a feed that fills a buffer to the last sample, one without any column, cols_cap columns
    assert max(w["n_max"] for w in want if w["rule"] == OK) == (cap - L) // hop + 1
    assert any(w["n_max"] == 0 for w in want if w["rule"] == OK)
    if diff:
        # a feed whose longest stream keeps its first column back, so the tracker's n_max is below the chroma kernel's
        assert any(w["n_max"] > 0 and w["n_max_diff"] < w["n_max"] for w in want if w["rule"] == OK)
        assert want[-1]["carry"] == [1] * B


@pytest.mark.parametrize("diff", [0, 1])
@pytest.mark.parametrize("fs_in", RATES)
def test_plan_of_resampling_feeds(driver, tmp_path, fs_in, diff):
    rs_L, rs_M, half = EXPECT[fs_in]
    in_cap = -(-(CAP + 1) * rs_M // rs_L) + -(-2 * half // rs_L) + 2          # include/rtsync.h, rts_live_create_resampled
    rs = np.random.RandomState(fs_in)
    mid = 900 * rs_M // rs_L                                                 # input samples of about 900 at the plan's rate
    feeds = []
    for i in range(36):
        c = [0 if i % 5 else int(rs.randint(1, 4 * mid)), 1, int(rs.randint(0, mid)), int(rs.choice([0, 1, 3, mid, 2 * mid]))]
        if i == 20:
            c[2] = in_cap                 # a running stream: about CAP + 1 samples more than fit
        if i == 24:
            c[3] = in_cap + 1             # more than a staging slot holds for one stream
        if i == 28:
            c[1] = -1
        feeds.append(c)
    want = check(driver, tmp_path, (RS_B, L_FFT, HOP, CAP, diff, rs_L, rs_M, half, in_cap), feeds)
    assert [(w["rule"], w["stream"]) for w in want if w["rule"] != OK] == [(PENDING, 2), (STAGING, 3), (NEGATIVE, 1)]
    assert [i for i, w in enumerate(want) if w["rule"] != OK] == [20, 24, 28]
    ok = [w for w in want if w["rule"] == OK]
    assert any(0 in w["nout"] for w in ok) and any(1 in f for f in feeds) and any(0 in f for f in feeds)
    assert max(w["n_out_max"] for w in ok) > L_FFT + HOP and max(w["n_max"] for w in ok) >= 2
    # the totals are those of the whole input, however it was cut
    fed = [sum(f[b] for f, w in zip(feeds, want) if w["rule"] == OK) for b in range(RS_B)]
    assert want[-1]["tot"] == [v for b in range(RS_B) for v in (fed[b], avail_cached(fed[b], rs_L, rs_M, half))]
