"""The time map of a path on the device (csrc/pathmap.hip) against the plain-Python definition (tests/pathmap_model.py, whose
own properties and accuracy tests/test_pathmap_cpu.py holds): rts_path_map over a ragged batch with every refusal in it,
rts_annot_transfer over the chopin pair and a long synthetic table, the wrappers, and the ensemble built from one table.
Floats are compared bit for bit; outputs lie inside guard regions."""
import math
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import annot_model as am  # noqa: E402
import pathmap_model as pm  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from guarded import guarded, holds_fill, same_bytes  # noqa: E402
from real_time_audio_sync_amd import evaluate  # noqa: E402
from test_pathmap_cpu import random_path  # noqa: E402

RUB_CSV = os.path.join(GOLDEN, "chopin_rubinstein_20b.csv")        # column 1 of dtw_chopin/path
RACH_CSV = os.path.join(GOLDEN, "chopin_rachmaninoff_20b.csv")     # column 0
FS = evaluate.FRAME_SECONDS
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32))).to(DEV)


def pad_paths(paths, fill=7):
    """[B][P_max][2] int32 with `fill` behind every path (so that a kernel reading past a length would show)."""
    out = np.full((len(paths), max(len(p) for p in paths), 2), fill, dtype=np.int32)
    for k, p in enumerate(paths):
        if len(p):
            out[k, :len(p)] = np.asarray(p, dtype=np.int32)
    return out


@pytest.fixture(scope="module")
def chopin_path(dtw_golden):
    return [(int(a), int(b)) for a, b in dtw_golden["dtw_chopin/path"]]


# ---- 1. rts_path_map ------------------------------------------------------------------------------------------------------

def ragged_batch():
    rng = random.Random(23)
    back_last = random_path(rng, 200)[:300]
    back_last[-1] = (back_last[-2][0] - 1, back_last[-2][1])
    back_256 = [(t, t) for t in range(400)]
    back_256[256] = (256, 254)                                       # v steps back at point 256, the first of the second turn, only
    runs = [(0, v) for v in range(100)] + [(u, 99) for u in range(1, 101)] + [(100, v) for v in range(100, 160)] + [(101, 400)]
    gaps = random_path(rng, 120, max_run=2, max_gap=9)
    usable = random_path(rng, 90)
    cases = [  # (points, length (None: all), offsets)
        ([(5, 9)], None, (0, 0)),
        ([(0, 0), (3, 7)], None, (2, 1)),
        (random_path(rng, 300)[:255], None, (0, 0)),
        (random_path(rng, 300)[:256], None, (0, 3)),
        (random_path(rng, 300)[:257], None, (0, 0)),
        (random_path(rng, 700)[:1025], None, (11, 0)),
        (runs, None, (0, 0)),
        (gaps, None, (1000, 70)),
        (usable, 0, (0, 0)),                                          # empty
        (usable, -1, (0, 0)),                                         # the fault word of dtw_paths
        (back_last, None, (0, 0)),
        (back_256, None, (0, 0)),
        (usable, None, (-5, 0)),                                      # negative after the offset
        (usable, None, (0, -1)),
        (usable, None, (4, 4)),                                       # a good neighbour behind the refused ones
    ]
    cases.append((cases[5][0], 2000, (0, 0)))                         # a length above P_max is clamped to it
    assert [len(c[0]) for c in cases[:6]] == [1, 2, 255, 256, 257, 1025]
    return cases


def positions_for(rng, path, side, off, length, n_max):
    u, _ = pm.columns(path, side, off, length)
    k = sorted(set(u)) or [0, 50]
    xs = [-0.0, math.nan, 2.0 ** 31, 1e300]
    for a in k:
        xs += [float(a), a - 0.5, a + 0.5]
    xs += [rng.uniform(k[0] - 2, k[-1] + 2) for _ in range(max(0, n_max - len(xs)))]
    return xs[:n_max]


@pytest.mark.parametrize("side", (0, 1))
@pytest.mark.parametrize("with_off", (True, False))
def test_path_map_equals_the_model(side, with_off):
    from real_time_audio_sync_amd import _native as nat
    cases = ragged_batch()
    B = len(cases)
    n_max = 4 + 3 * 1025 + 5
    paths = pad_paths([c[0] for c in cases])
    P_max = paths.shape[1]
    assert P_max == 1025
    lens = [len(c[0]) if c[1] is None else c[1] for c in cases]
    offs = [c[2] if with_off else (0, 0) for c in cases]
    n = [n_max] * B
    n[0], n[1], n[3], n[14] = 1, 0, 257, 700
    rng = random.Random(5 + side)
    x = np.zeros((B, n_max))
    want, want_st = [], []
    for b, c in enumerate(cases):
        xs = positions_for(rng, c[0], side, offs[b], lens[b], n_max)
        if b == 0:
            xs[0] = float(c[0][0][side])                             # its one entry: the only knot
        x[b] = xs
        ys, st = pm.map_positions(c[0], xs[:n[b]], side, offs[b], lens[b])
        want.append(np.array(ys, dtype=np.float64))
        want_st.append(st)
    if with_off:
        assert want_st == [0] * 8 + [pm.EMPTY, pm.EMPTY, pm.BACKWARD, pm.BACKWARD, pm.NEGATIVE, pm.NEGATIVE, 0, 0]
    else:
        assert want_st == [0] * 8 + [pm.EMPTY, pm.EMPTY, pm.BACKWARD, pm.BACKWARD, 0, 0, 0, 0]
    assert want[0][0] == float(cases[0][0][0][1 - side]) + offs[0][1 - side]
    for b in (2, 3, 5, 6, 7, 14):                                     # the usable pairs hold images and NaN both
        assert np.isfinite(want[b]).sum() > 100 and np.isnan(want[b]).sum() >= 3, b
    path_d, len_d, n_d = dev_i32(paths), dev_i32(lens), dev_i32(n)
    off_d = dev_i32(offs) if with_off else None
    x_d = torch.from_numpy(x).to(DEV)
    got = {}
    for fill in (0xFF, 0x55):                                         # no result depends on what the outputs held
        y, check_y = guarded((B, n_max), torch.float64, DEV, fill)
        status, check_status = guarded((B,), torch.int32, DEV, fill)
        nat.check(nat.lib.rts_path_map(path_d.data_ptr(), P_max, len_d.data_ptr(), off_d.data_ptr() if with_off else None, side,
                                       x_d.data_ptr(), n_max, n_d.data_ptr(), B, y.data_ptr(), status.data_ptr(), None))
        torch.cuda.synchronize()
        check_y("y_dev")
        check_status("status_dev")
        y, status = y.cpu().numpy(), status.cpu().numpy()
        assert status.tolist() == want_st, fill
        for b in range(B):
            assert same_bytes(y[b, :n[b]], want[b]), (fill, b, want_st[b])
            assert holds_fill(y[b, n[b]:], fill), (fill, b)           # entries behind n[b] are not written
            if want_st[b]:
                assert np.isnan(y[b, :n[b]]).all(), b
        got[fill] = y
    for b in range(B):
        assert same_bytes(got[0xFF][b, :n[b]], got[0x55][b, :n[b]])
    # without n_dev: every entry of every pair
    y, check_y = guarded((B, n_max), torch.float64, DEV, 0x55)
    status, check_status = guarded((B,), torch.int32, DEV, 0x55)
    nat.check(nat.lib.rts_path_map(path_d.data_ptr(), P_max, len_d.data_ptr(), off_d.data_ptr() if with_off else None, side,
                                   x_d.data_ptr(), n_max, None, B, y.data_ptr(), status.data_ptr(), None))
    torch.cuda.synchronize()
    check_y("y_dev")
    check_status("status_dev")
    for b in (1, 5, 10):
        ys, _ = pm.map_positions(cases[b][0], x[b], side, offs[b], lens[b])
        assert same_bytes(y[b].cpu().numpy(), np.array(ys)), b
    # no entries at all: the status words alone
    status, check_status = guarded((B,), torch.int32, DEV, 0xFF)
    nat.check(nat.lib.rts_path_map(path_d.data_ptr(), P_max, len_d.data_ptr(), None, side, None, 0, None, B, None,
                                   status.data_ptr(), None))
    torch.cuda.synchronize()
    check_status("status_dev")
    assert status.cpu().tolist() == [pm.status(c[0], side, (0, 0), l) for c, l in zip(cases, lens)]


def test_map_frames_list_form():
    from real_time_audio_sync_amd.pathmap import map_frames
    rng = random.Random(9)
    paths = [random_path(rng, 40), [(3, 3)], random_path(rng, 300)]
    xs = [[0.0, 0.5, 7.25, 1e9, math.nan], [], [rng.uniform(-1, 400) for _ in range(600)]]
    for side in (0, 1):
        got = map_frames(paths, xs, side, offsets=[(0, 0), (1, 2), (10, 20)])
        for k, off in enumerate([(0, 0), (1, 2), (10, 20)]):
            assert same_bytes(got[k], np.array(pm.map_positions(paths[k], xs[k], side, off)[0], dtype=np.float64)), (side, k)
    with pytest.raises(ValueError, match=r"pairs 1, 2.*1: no path point.*2: a column steps back, an index below 0"):
        map_frames([paths[0], [], [(0, 0), (-1, 1)]], [[0.0], [0.0], [0.0]])


# ---- 2. rts_annot_transfer -------------------------------------------------------------------------------------------------

def long_table():
    rs = np.random.RandomState(4)
    t = np.cumsum(rs.uniform(0.05, 0.6, 700))                        # ends behind the long path's last frame
    return list(t - t[0] + 3 * FS), list(range(700))                  # row 0 exactly on frame 3


def long_path():
    return random_path(random.Random(31), 1600, max_run=3, max_gap=2)[:3000]


def test_annot_transfer_equals_the_model(chopin_path):
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.annotate import AnnotationTables
    host = [evaluate.read_ground_truth(RACH_CSV), evaluate.read_ground_truth(RUB_CSV), long_table()]
    tab = AnnotationTables([RACH_CSV, RUB_CSV, host[2]], device=DEV)
    flipped = [(b, a) for a, b in chopin_path]
    lp = long_path()
    assert len(lp) == 3000
    backward = [(0, 0), (5, 5), (4, 6)]
    # from = 0: column 0 is the side of the table.  Both directions of the chopin pair in one batch, the second flipped.
    paths = [chopin_path, flipped, chopin_path, lp, backward, lp]
    pieces = [0, 1, 7, 2, 0, -1]
    offs = [(0, 0), (0, 0), (0, 0), (3, 40), (0, 0), (0, 0)]
    B, rows_max = len(paths), 700
    try:
        for side in (0, 1):
            use = paths if side == 0 else [[(b, a) for a, b in p] for p in paths]
            use_off = offs if side == 0 else [(o[1], o[0]) for o in offs]
            want, want_n, want_st = [], [], []
            for k in range(B):
                if not 0 <= pieces[k] < 3:
                    want.append([]), want_n.append(0), want_st.append(pm.EMPTY)
                    continue
                new, st = pm.transfer(use[k], host[pieces[k]][0], FS, side, use_off[k])
                want.append(new), want_n.append(len(new)), want_st.append(st)
            assert want_st == [0, 0, pm.EMPTY, 0, pm.BACKWARD, pm.EMPTY] and want_n == [20, 20, 0, 700, 20, 0]
            assert np.isfinite(want[0]).sum() == 19 and np.isfinite(want[1]).sum() == 19
            assert 300 < np.isfinite(want[3]).sum() < 700
            padded = pad_paths(use)
            path_d, len_d = dev_i32(padded), dev_i32([len(p) for p in use])
            off_d, piece_d = dev_i32(use_off), dev_i32(pieces)
            for fill in (0xFF, 0x55):
                times, check_times = guarded((B, rows_max), torch.float64, DEV, fill)
                n_rows, check_n = guarded((B,), torch.int32, DEV, fill)
                status, check_status = guarded((B,), torch.int32, DEV, fill)
                args = [tab._h, path_d.data_ptr(), padded.shape[1], len_d.data_ptr(), off_d.data_ptr(), side, piece_d.data_ptr(), B,
                        rows_max, times.data_ptr(), n_rows.data_ptr(), status.data_ptr(), None]
                nat.check(nat.lib.rts_annot_transfer(*args))
                torch.cuda.synchronize()
                for chk, what in ((check_times, "times_dev"), (check_n, "n_rows_dev"), (check_status, "status_dev")):
                    chk(what)
                t = times.cpu().numpy()
                assert n_rows.cpu().tolist() == want_n and status.cpu().tolist() == want_st, (side, fill)
                for k in range(B):
                    assert same_bytes(t[k, :want_n[k]], np.array(want[k], dtype=np.float64)), (side, fill, k)
                    assert holds_fill(t[k, want_n[k]:], fill), (side, fill, k)
            # rows_max below the longest table: refused before any launch, nothing is written
            times, check_times = guarded((B, rows_max), torch.float64, DEV, 0x55)
            n_rows, _ = guarded((B,), torch.int32, DEV, 0x55)
            status, _ = guarded((B,), torch.int32, DEV, 0x55)
            args[8:12] = [699, times.data_ptr(), n_rows.data_ptr(), status.data_ptr()]
            assert nat.lib.rts_annot_transfer(*args) == -1 and b"rows_max" in nat.lib.rts_last_error()
            torch.cuda.synchronize()
            assert holds_fill(times, 0x55) and holds_fill(n_rows, 0x55) and holds_fill(status, 0x55)
    finally:
        tab.close()


# ---- 3. AnnotationTables.transfer -> AnnotationTables -> path_errors ---------------------------------------------------------

def test_carried_table_is_accepted_and_scores_like_the_hand_made_pair(chopin_path):
    from real_time_audio_sync_amd.annotate import AnnotationTables
    rub = evaluate.read_annotations(RUB_CSV)
    src = AnnotationTables([RUB_CSV, ([1000.0, 2000.0], [1, 2])], device=DEV)
    try:
        # Rubinstein is column 1 of the path: its table carried onto Rachmaninoff, column 0
        tables, dropped = src.transfer([chopin_path], [0], 1)
        (want, want_dropped) = pm.carried_table(chopin_path, rub, FS, 1)
        assert dropped == [want_dropped] == [[19]]
        assert same_bytes(tables[0][0], np.array(want[0])) and tables[0][1].tolist() == want[1] and tables[0][2] == want[2]
        both = AnnotationTables([tables[0], RUB_CSV], device=DEV)            # rts_annot_create takes the carried table
        try:
            stats = both.path_errors([chopin_path], [0], [1])[0]
            assert stats["count"] > 300 and stats["pct_off_beats"][1] == 0
            err, counts = am.metric(chopin_path, (want[0], want[1]), (rub[0], rub[1]), FS)
            assert stats == am.stats(err, counts)
        finally:
            both.close()
        # the device triple does as well, and offsets travel
        pair = (dev_i32(pad_paths([chopin_path])), dev_i32([len(chopin_path)]))
        again, _ = src.transfer(pair, [0], 1, offsets=[(0, 0)])
        assert same_bytes(again[0][0], tables[0][0])
        with pytest.raises(ValueError, match="pair 0.*a column steps back"):
            src.transfer([[(0, 0), (5, 5), (4, 6)]], [0], 1)
        with pytest.raises(ValueError, match="pair 1: no row"):
            src.transfer([chopin_path, chopin_path], [0, 1], 1)              # table 1 begins long after the last frame
        with pytest.raises(ValueError, match="pair 0: no such piece"):
            src.transfer([chopin_path], [2], 1)
    finally:
        src.close()


# ---- 4. straight from the device ---------------------------------------------------------------------------------------------

def test_map_frames_takes_the_device_triple_of_dtw_paths(otw_golden, chopin_path):
    from real_time_audio_sync_amd.dtw import dtw_paths
    from real_time_audio_sync_amd.otw_batch import frames_tensor
    from real_time_audio_sync_amd.pathmap import map_frames
    a, b = frames_tensor(otw_golden["G/live"], torch.device(DEV)), frames_tensor(otw_golden["G/ref"], torch.device(DEV))
    triple = dtw_paths(a.unsqueeze(0), b.unsqueeze(0))
    xs = np.concatenate([np.arange(401.0), np.arange(400.0) + 0.5, [-1.0, 401.0, np.nan]])
    y, status = map_frames(triple, torch.from_numpy(xs[None]).to(DEV), 0)     # no host round trip in between
    assert y.is_cuda and status.is_cuda and tuple(y.shape) == (1, len(xs))
    n = int(triple[1][0])
    read_back = triple[0][0, :n].cpu().numpy()
    assert read_back.tolist() == [list(p) for p in chopin_path]
    assert status.cpu().tolist() == [0]
    assert same_bytes(y[0].cpu().numpy(), map_frames([read_back], [xs], 0)[0])
    assert same_bytes(y[0].cpu().numpy(), np.array(pm.map_positions(chopin_path, xs, 0)[0]))
    y2, _ = map_frames(triple, torch.from_numpy(xs[None]).to(DEV), 0, n=[5])
    assert same_bytes(y2[0, :5].cpu().numpy(), y[0, :5].cpu().numpy())


# ---- 5. an ensemble from one table ---------------------------------------------------------------------------------------------

def test_an_ensemble_from_one_annotated_recording(otw_golden, chopin_audio, chopin_path):
    from real_time_audio_sync_amd.annotate import AnnotationTables
    from real_time_audio_sync_amd.ensemble import EnsembleSession, annotate_recordings
    rach, rub = otw_golden["G/live"], otw_golden["G/ref"]
    src = AnnotationTables([RACH_CSV], device=DEV)
    tabs = annotate_recordings([rach, rub], RACH_CSV, annotated=0, device=DEV)
    sess = hand = by_hand = None
    try:
        carried, dropped = src.transfer([chopin_path], [0], 0)                # align_pairs gives the golden path
        assert dropped == [[19]] and tabs.P == 2
        assert same_bytes(tabs.times[1], carried[0][0]) and tabs.beat_rows[1].tolist() == carried[0][1].tolist()
        assert tabs.labels[1] == carried[0][2]
        own = evaluate.read_annotations(RACH_CSV)
        assert tabs.times[0].tolist() == list(own[0]) and tabs.beat_rows[0].tolist() == list(own[1])
        kw = dict(max_dev=2.0, patience=4, c=50, max_run_count=3, device=DEV)
        sess = EnsembleSession.from_annotated([rach, rub], RACH_CSV, 1, annotated=0, **kw)
        by_hand = AnnotationTables([RACH_CSV, carried[0]], device=DEV)
        hand = EnsembleSession([rach, rub], by_hand, 1, **kw)
        audio = chopin_audio["live"]
        pos = 0
        for feed, cut in enumerate((21000, 14097, 30000, 18048, 26001)):
            buf = audio[pos:pos + cut]
            pos += cut
            sess.feed([buf])
            hand.feed([buf])
            sess.sync()
            hand.sync()
            got, want = sess.consensus(), hand.consensus()
            assert got["feeds_done"] == want["feeds_done"] == feed + 1
            for key in ("consensus", "spread", "dev"):
                assert same_bytes(np.asarray(got[key], dtype=np.float64), np.asarray(want[key], dtype=np.float64)), (feed, key)
            for key in ("n_in", "n_valid", "strikes", "out"):
                assert np.asarray(got[key]).tolist() == np.asarray(want[key]).tolist(), (feed, key)
        assert np.isfinite(got["consensus"]).all()
    finally:
        for s in (sess, hand):
            if s is not None:
                s.close()
        for t in (tabs, src, by_hand):
            if t is not None:
                t.close()
        if sess is not None:
            sess.tables.close()
