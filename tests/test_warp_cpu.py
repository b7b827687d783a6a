"""The renderer without a GPU: the numpy model of the definition (tests/warp_model.py) on signals whose rendering is known;
the anchors rule on hand-made paths; the host-only entry points of the C ABI and their refusals; csrc/warp_plan.h through a
stand-alone driver built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process."""
import ctypes
import os

import numpy as np
import pytest

import warp_model as wm
from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

FS = 22050


def tone(n):
    t = np.arange(n) / FS
    return (0.4 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 661.3 * t + 1)
            + 0.1 * np.sin(2 * np.pi * 1318.7 * t + 2)).astype(np.float32)


def peak_bin(v):
    return int(np.argmax(np.abs(np.fft.rfft(v[2048:2048 + 16384].astype(np.float64) * np.hanning(16384)))))


# ---- (a) the model -----------------------------------------------------------------------------------------------------------

def test_window_is_the_periodic_hann_and_sums_to_one():
    from real_time_audio_sync_amd import filters
    for N in (64, 256, 1024, 4096):
        w = wm.hann(N)
        assert w.tobytes() == filters.hann_window_periodic(N).tobytes()
        # each value carries the cosine's error (1 ulp) and one rounding, the sum one more: a few units of 2^-53
        assert np.abs(w[:N // 2] + w[N // 2:] - 1.0).max() <= 2.0 ** -50
    assert not np.array_equal(filters.hann_window(64), filters.hann_window_periodic(64))   # the symmetric form stays


def test_identity_map_gives_the_input_back():
    n = FS
    x = tone(n)
    y, state, info = wm.warp(x, [0, n], [0, n], n)
    assert len(y) == n and state[0] == wm.blocks(n, 1024)
    # every delta = 0 while the target lies inside the signal (the last one runs past its end, where a frame with more
    # signal in it can score higher than the target itself)
    assert info["p"][:-1] == [k * 512 for k in range(len(info["p"]) - 1)]
    a, b = x[1024:-1024], y[1024:-1024]
    assert np.all(np.abs(a - b) <= np.spacing(np.abs(a)))                                   # within 1 float32 ulp


@pytest.fixture(scope="module")
def stretched():
    n = 2 * FS
    x = tone(n)
    out = {}
    for rate in (0.8, 1.25):
        n_out = int(n / rate)
        out[rate] = wm.warp(x, [0, n_out], [0, n], n_out)[0]
    n_out = int(n / 1.25)
    out["ola"] = wm.warp(x, [0, n_out], [0, n], n_out, D=0)[0]
    return out


@pytest.mark.parametrize("rate", (0.8, 1.25))
def test_pitch_stays_when_the_tempo_changes(stretched, rate):
    want = 440.0 * 16384 / FS                                                               # 326.9 bins
    assert abs(peak_bin(stretched[rate]) - want) <= 1.0


def test_plain_overlap_add_moves_the_pitch(stretched):
    """delta = 0 at rate 1.25 is more than one bin off: the search is what keeps the pitch."""
    assert abs(peak_bin(stretched["ola"]) - 440.0 * 16384 / FS) > 1.0


def test_split_runs_equal_one_run():
    rng = np.random.default_rng(3)
    x = (tone(9000) + 0.05 * rng.standard_normal(9000)).astype(np.float32)
    op, ip, n_out = [0, 3000, 6000, 10001], [0, 4000, 4000, 9000], 10001
    whole, st, info = wm.warp(x, op, ip, n_out, N=256, D=64)
    assert len(whole) == n_out and len(set(np.subtract(info["p"][1:], [wm.amap(k, 128, op, ip) for k in range(1, len(info["p"]))]))) > 1
    parts, state = [], (0, 0)
    for count in (3, 1, 0, 17, 10 ** 6):
        y, state, _ = wm.warp(x, op, ip, n_out, N=256, D=64, state=state, k_count=count)
        parts.append(y)
    assert state == st and np.concatenate(parts).tobytes() == whole.tobytes()


def test_model_ties_and_nan():
    x = np.zeros(4000, np.float32)
    _, _, info = wm.warp(x, [0, 4000], [0, 3000], 4000, N=64, D=40)
    assert info["p"] == [wm.amap(k, 32, [0, 4000], [0, 3000]) for k in range(len(info["p"]))]   # silence: every delta = 0
    x = tone(4000)
    x[1500] = np.nan
    y, _, _ = wm.warp(x, [0, 4000], [0, 4000], 4000, N=64, D=16)
    assert np.isnan(y).any() and not np.isnan(y[:1000]).any()


# ---- (b) the anchors rule ------------------------------------------------------------------------------------------------------

def test_anchors_rule():
    path = [(0, 0), (0, 1), (1, 2), (2, 2), (3, 2), (3, 3), (4, 4)]
    assert wm.anchors(path, 0, 100, 512, 470, 8) == ([0, 100, 200, 300, 400, 512], [0, 200, 200, 200, 400, 470], 0)
    assert wm.anchors(path, 1, 100, 450, 401, 8) == ([0, 100, 200, 300, 400, 450], [0, 0, 100, 300, 400, 401], 0)
    assert wm.map_ok(*wm.anchors(path, 0, 100, 512, 470, 8)[:2], 512)
    assert wm.anchors(path, 0, 100, 512, 470, 6)[2] == 0
    assert wm.anchors(path, 0, 100, 512, 470, 5) == ([], [], wm.PATH_TOO_MANY)
    assert wm.anchors([], 0, 100, 512, 470, 8) == ([], [], wm.PATH_EMPTY)
    assert wm.anchors(path[1:], 1, 100, 512, 470, 8)[2] == wm.PATH_START
    assert wm.anchors([(0, 0), (1, 1), (0, 2)], 0, 1, 9, 9, 8)[2] == wm.PATH_BACKWARD
    assert wm.anchors([(0, 1), (1, 0)], 0, 1, 9, 9, 8)[2] == wm.PATH_BACKWARD
    assert wm.anchors(path, 0, 100, 400, 470, 8)[2] == wm.PATH_SHORT_OUT
    assert wm.anchors(path, 0, 100, 401, 400, 8)[2] == 0
    assert wm.anchors(path, 0, 100, 401, 399, 8)[2] == wm.PATH_SHORT_IN
    assert wm.anchors(path, 0, 100, 400, 399, 2)[2] == wm.PATH_SHORT_OUT | wm.PATH_SHORT_IN | wm.PATH_TOO_MANY


def test_map_arithmetic_is_exact_at_64_bits():
    seg = 2 ** 31 - 1
    op, ip = [k * seg for k in range(6)], [5 + k * (seg - 1) for k in range(5)] + [5 + 4 * (seg - 1)]   # the last one flat
    assert op[5] > 2 ** 33 and wm.map_ok(op, ip, op[-1]) and wm.map_ok(op, ip, op[-2] + 2 ** 31)
    assert not wm.map_ok(op, ip, op[-2] + 2 ** 31 + 1)
    assert not wm.map_ok([0, 2 ** 31], [0, 1], 2 ** 31) and not wm.map_ok([0, 10], [0, 10], 2 ** 31 + 1)
    assert wm.map_ok([0, 10], [0, 10], 2 ** 31) and not wm.map_ok([1, 10], [0, 10], 10) and not wm.map_ok([0], [0], 0)
    k = (op[4] - 1) // 32                                    # the last block that begins in segment 3
    t = 32 * k
    assert op[3] <= t < op[4] and wm.amap(k, 32, op, ip) == ip[3] + ((t - op[3]) * (seg - 1)) // seg
    assert wm.amap(k + 1, 32, op, ip) == ip[4] and wm.amap(0, 32, op, ip) == 5


# ---- (c) the host-only entry points ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


def test_warp_blocks(nat):
    for n_out, N in ((0, 64), (-5, 64), (1, 64), (32, 64), (33, 64), (10001, 256), (2 ** 40 + 1, 4096), (100, 48), (100, 4112),
                     (100, 72), (100, 0), (2 ** 62, 64)):
        assert nat.lib.rts_warp_blocks(n_out, N) == wm.blocks(n_out, N), (n_out, N)
    assert nat.lib.rts_warp_blocks(33, 64) == 2 and nat.lib.rts_warp_blocks(100, 48) == -1


def test_warp_create_refusals_need_no_gpu(nat):
    h = ctypes.c_void_p()
    w = np.ones(4096 + 32)
    wp = w.ctypes.data_as(ctypes.c_void_p)

    def create(N, delta, window=wp, out=ctypes.byref(h)):
        return nat.lib.rts_warp_create(N, delta, window, out), nat.lib.rts_last_error()

    rc, msg = create(64, 0, out=None)
    assert rc == -1 and b"out" in msg
    for N in (-64, 0, 1, 65):
        rc, msg = create(N, 0)
        assert rc == -1 and b"N" in msg, N
    rc, msg = create(64, -1)
    assert rc == -1 and b"delta" in msg
    rc, msg = create(64, 0, window=None)
    assert rc == -1 and b"window_host" in msg
    for N in (48, 4112, 16, 72, 1000, 8192):
        rc, msg = create(N, 0)
        assert rc == -2 and b"N" in msg, N
    rc, msg = create(1024, 1025)
    assert rc == -2 and b"delta" in msg
    assert not h.value
    assert nat.lib.rts_warp_destroy(None) == 0


def test_warp_call_refusals_need_no_gpu(nat):
    p = ctypes.c_void_p(16)
    a = nat.lib.rts_warp_anchors
    good = [p, 8, p, 0, 2048, p, p, 1, p, 9, p, p, None]
    for pos, bad, word in ((0, None, b"path_dev"), (1, -1, b"P_max"), (2, None, b"path_len_dev"), (3, 2, b"onto"), (4, 0, b"hop_f"),
                           (5, None, b"n_out_dev"), (6, None, b"n_in_dev"), (7, 0, b"B"), (7, 65536, b"B"), (8, None, b"anchors_dev"),
                           (9, 1, b"A_max"), (10, None, b"n_anchor_dev"), (11, None, b"status_dev")):
        args = list(good)
        args[pos] = bad
        assert a(*args) == -1 and word in nat.lib.rts_last_error(), word
    r = nat.lib.rts_warp_run
    good = [p, p, nat.F32, 100, p, p, p, 2, p, p, 1, p, 100, p, 1, None]
    for pos, bad, word in ((0, None, b"plan"), (1, None, b"samples_dev"), (2, nat.F64, b"sample_dtype"), (3, -1, b"sample_stride"),
                           (4, None, b"n_in_dev"), (5, None, b"anchors_dev"), (6, None, b"n_anchor_dev"), (7, 1, b"A_max"),
                           (8, None, b"n_out_dev"), (9, None, b"state_dev"), (10, -1, b"k_count"), (11, None, b"out_dev"),
                           (12, -1, b"out_stride"), (13, None, b"status_dev"), (14, 0, b"B")):
        args = list(good)
        args[pos] = bad
        assert r(*args) == -1 and word in nat.lib.rts_last_error(), word


# ---- (d) csrc/warp_plan.h under the sanitizers ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "warp_plan_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "warp_plan_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


def test_plan_header_under_sanitizers(driver, tmp_path):
    top = wm.SEG_LIMIT
    cases = []
    cases += [("B", n, N) for n in (-1, 0, 1, 31, 32, 33, 10001, 2 ** 62 - 1) for N in (48, 64, 80, 1024, 4096, 4112)]
    cases += [("L", N, d) for N in (48, 64, 72, 1024, 4096, 4112) for d in (-1, 0, 256, 1024, 1025)]
    cases += [("T", n, P) for n, P in ((-1, 10), (0, 10), (1, 10), (256, 300), (257, 300), (5000, 300), (2100, 4000))]
    segs = [(0, 0, 10, 10, 10), (0, 0, 10, 0, 10), (0, 0, 10, 10, 9), (0, 0, 10, 10, top), (0, 0, 10, 10, top + 1),
            (0, -5, top - 1, top - 6, top - 1), (0, 0, top, 1, top), (0, 0, 1, top, 1), (2 ** 33, 7, 2 ** 33 + top - 1, 6 + top, 2 ** 33 + top),
            (5, 0, 5, 0, 5), (9, 0, 5, 0, 9), (0, 3, 4, 2, 4), (-1, 0, 4, 2, 4), (0, 0, 4, 2, -2 ** 63), (0, -2 ** 62, 4, 2, 4),
            (0, 0, 2 ** 62, 2, 2 ** 62), (0, 0, 4, 2 ** 62, 4), (0, 2 ** 63 - 1, 4, -2 ** 63, 4)]
    cases += [("S",) + s for s in segs]
    case = tmp_path / "case.txt"
    case.write_text("".join(" ".join(str(v) for v in c) + "\n" for c in cases))
    rc, out, err = _run([driver, str(case)], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (rc, out[-1000:], err[-2000:])
    lines = [l.split() for l in out.splitlines()]
    assert lines[-1] == ["sweep", "checked"] and len(lines) == len(cases) + 1
    seen_ok = set()
    for c, line in zip(cases, lines):
        got = [int(v) for v in line[1:]]
        assert line[0] == c[0] and got[:len(c) - 1] == list(c[1:])
        rest = got[len(c) - 1:]
        if c[0] == "B":
            assert rest == [wm.blocks(c[1], c[2])], c
        elif c[0] == "L":
            ok = wm.n_ok(c[1]) and 0 <= c[2] <= wm.MAX_DELTA
            assert rest == [int(wm.n_ok(c[1])), int(0 <= c[2] <= wm.MAX_DELTA), 4 * (2 * c[1] + 2 * c[2]) if ok else 0], c
        elif c[0] == "T":
            assert rest == [-(-max(0, min(c[1], c[2])) // 256)], c
        else:
            o0, i0, o1, i1, reach = c[1:]
            ok = wm.seg_ok(o0, i0, o1, i1, reach)
            seen_ok.add(ok)
            if ok:
                assert rest == [1] + [i0 + ((t - o0) * (i1 - i0)) // (o1 - o0) for t in (o0, o0 + (reach - o0) // 2, reach - 1)], c
            else:
                assert rest == [0], c
    assert seen_ok == {True, False}
