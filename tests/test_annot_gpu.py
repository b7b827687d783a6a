"""Beats and labels on the device (csrc/annot.hip) against the plain-Python model of the definition (tests/annot_model.py,
itself held against evaluate.py and the reference's own numbers in tests/test_annot_cpu.py): the batched lookup, the
batched metric, and the beat words a live session publishes with every feed, for both trackers, across a restart with
an offset, with annotations switched off again, and next to the level gate.  Floats are compared bit for bit."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import annot_model as am  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from guarded import guarded, holds_fill, same_bytes  # noqa: E402
from real_time_audio_sync_amd import evaluate  # noqa: E402

REF_CSV = os.path.join(GOLDEN, "chopin_rubinstein_20b.csv")
LIVE_CSV = os.path.join(GOLDEN, "chopin_rachmaninoff_20b.csv")
FS = evaluate.FRAME_SECONDS
ONE_ROW = ([3.0], [7])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def long_tables():
    """Two tables of 700 rows for the long path.  Live side: beats[0] == 0 and times[0] exactly on frame 4, so that a
    beat of exactly 0.0 occurs; reference side: beats 5 ahead, so that its last beats reach 700, the live table's rows."""
    rs = np.random.RandomState(11)
    live_t = np.cumsum(rs.uniform(0.2, 0.6, 700))
    live_t = list(live_t - live_t[0] + 4 * FS)
    ref_t = 0.9 * np.cumsum(rs.uniform(0.2, 0.6, 700))        # ends while the path is still inside the live table
    return (live_t, list(range(700))), (list(ref_t), list(range(5, 705)))


@pytest.fixture(scope="module")
def tables():
    from real_time_audio_sync_amd.annotate import AnnotationTables
    long_live, long_ref = long_tables()
    tab = AnnotationTables([REF_CSV, LIVE_CSV, ONE_ROW, long_live, long_ref])
    yield tab
    tab.close()


def host_tables():
    long_live, long_ref = long_tables()
    return [evaluate.read_ground_truth(REF_CSV), evaluate.read_ground_truth(LIVE_CSV), ONE_ROW, long_live, long_ref]


def beat_array(values):
    return np.array([np.nan if v is None else v for v in values], dtype=np.float64)


# ---- (a) rts_annot_beats ------------------------------------------------------------------------------------------------

def test_beats_equal_the_model(tables):
    from real_time_audio_sync_amd import _native as nat
    dev = tables.device
    host = host_tables()
    B, n_max = 5, 300                                    # two blocks along a stream
    n = [300, 1, 0, 257, 256]
    pieces = [0, 1, 2, 7, 2]                             # stream 3: no such piece
    frame0 = [0, 40, 0, 0, 13]
    rs = np.random.RandomState(3)
    frames = rs.randint(-2, 520, size=(B, n_max)).astype(np.int32)
    frames[4, :40] = np.arange(40)                       # the one-row table's only segment, and its end (frame0 = 13)
    frames[0, 5:7] = (-1, -2)
    frames[1, 0] = -1                                    # negative before the offset is added: no beat
    want_beat = np.zeros((B, n_max))
    want_seg = np.zeros((B, n_max), dtype=np.int32)
    for b in range(B):
        for k in range(n[b]):
            t = host[pieces[b]] if pieces[b] < len(host) else ([], [])
            beat, seg = am.lookup(int(frames[b, k]), t[0], t[1], FS, frame0[b]) if t[0] else (None, -1)
            want_beat[b, k], want_seg[b, k] = (np.nan if beat is None else beat), seg
    assert np.isfinite(want_beat[4, :n[4]]).sum() > 10 and np.isnan(want_beat[4, :n[4]]).sum() > 10
    assert np.isnan(want_beat[3, :n[3]]).all() and (want_seg[3, :n[3]] == -1).all()
    assert np.isnan(want_beat[0, :n[0]][frames[0] < 0]).all() and (frames[0] < 0).any()
    d = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)  # noqa: E731
    frames_d, n_d, pieces_d, frame0_d = d(frames), d(n), d(pieces), d(frame0)
    for fill in (0xFF, 0x55):                            # the result does not depend on what the outputs held
        beat, check_beat = guarded((B, n_max), torch.float64, dev, fill)
        seg, check_seg = guarded((B, n_max), torch.int32, dev, fill)
        nat.check(nat.lib.rts_annot_beats(tables._h, frames_d.data_ptr(), n_max, n_d.data_ptr(), pieces_d.data_ptr(),
                                          frame0_d.data_ptr(), B, beat.data_ptr(), seg.data_ptr(), None))
        torch.cuda.synchronize()
        check_beat("beat_dev")
        check_seg("seg_dev")
        beat, seg = beat.cpu().numpy(), seg.cpu().numpy()
        for b in range(B):
            assert same_bytes(beat[b, :n[b]], want_beat[b, :n[b]]), (fill, b)
            assert np.array_equal(seg[b, :n[b]], want_seg[b, :n[b]]), (fill, b)
            assert holds_fill(beat[b, n[b]:], fill) and holds_fill(seg[b, n[b]:], fill), (fill, b)   # not written
    # without n_dev, frame0_dev and seg_dev: every entry, no offset
    beat, check_beat = guarded((B, n_max), torch.float64, dev, 0x55)
    nat.check(nat.lib.rts_annot_beats(tables._h, frames_d.data_ptr(), n_max, None, pieces_d.data_ptr(), None, B,
                                      beat.data_ptr(), None, None))
    torch.cuda.synchronize()
    check_beat("beat_dev")
    row = beat.cpu().numpy()[1]
    assert same_bytes(row, beat_array(am.lookup(int(f), host[1][0], host[1][1], FS)[0] for f in frames[1]))
    # the wrapper's list form
    out = tables.beats([frames[b, :n[b]] for b in range(B)], pieces, frame0)
    for b in range(B):
        assert same_bytes(out[b][0], want_beat[b, :n[b]]) and np.array_equal(out[b][1], want_seg[b, :n[b]]), b


# ---- (b) rts_annot_path_error -------------------------------------------------------------------------------------------

def percent_lines(stats):
    return [stats["pct_off_beats"][t] for t in (1, 3, 5, 10)] + [stats["pct_off_seconds"][t] for t in (1, 3, 5, 10)]


def test_path_errors_equal_the_model_and_the_reference(tables, wtw_known_answer, dtw_golden):
    host = host_tables()
    gold = json.load(open(os.path.join(GOLDEN, "eval_golden.json")))
    names = ["wtw_known_answer", "dtw_chopin", "shifted", "drift"]
    paths = [wtw_known_answer, dtw_golden["dtw_chopin/path"], np.array(gold["_paths"]["shifted"]), np.array(gold["_paths"]["drift"])]
    paths = [np.asarray(p, dtype=np.int64) for p in paths]
    k = np.arange(3000)
    long_path = np.stack([k, k + k // 100], axis=1)      # three chunks of 1024, three trips of a lane in each
    paths += [np.zeros((0, 2), dtype=np.int64), np.array([[100, 100]]), long_path]
    p0 = [1, 1, 1, 1, 1, 1, 3]                           # column 0: the live side's table
    p1 = [0, 0, 0, 0, 0, 0, 4]
    model = [am.metric(p.tolist(), host[a], host[b], FS) for p, a, b in zip(paths, p0, p1)]
    assert model[6][1][9] > 0 and model[6][1][0] > 2000 and sum(model[6][1][1:9]) > 0    # index errors and real counts
    l4 = am.lookup(4, host[3][0], host[3][1], FS)[0]
    assert l4 == 0.0 and model[4] == (0.0, [0] * 10) and model[5][1][0] == 1             # the == 0.0 skip is in the long path
    # raw: every count and the sum, bit for bit
    host_paths = np.zeros((7, 3000, 2), dtype=np.int32)
    for i, p in enumerate(paths):
        host_paths[i, :len(p)] = p
    plen = torch.tensor([len(p) for p in paths], dtype=torch.int32, device=tables.device)
    sq, counts = tables.path_error_counts(torch.from_numpy(host_paths).to(tables.device), plen, p0, p1)
    sq, counts = sq.cpu().numpy(), counts.cpu().numpy()
    for i in range(7):
        assert counts[i].tolist() == model[i][1], (i, counts[i].tolist(), model[i][1])
        assert same_bytes(sq[i:i + 1], np.array([model[i][0]])), (i, sq[i], model[i][0])
    # the fault marker of dtw_paths and a length past P_max
    plen2 = torch.tensor([-1, 10 ** 6], dtype=torch.int32, device=tables.device)
    sq2, counts2 = tables.path_error_counts(torch.from_numpy(host_paths[[0, 1]][:, :657].copy()).to(tables.device), plen2, p0[:2], p1[:2])
    assert counts2[0].tolist() == [0] * 10 and float(sq2[0]) == 0.0
    assert counts2[1].tolist() == model[1][1] and float(sq2[1]) == model[1][0]
    # the wrapper: the dicts of AlignmentError.stats(), the reference's printed numbers, None for nothing counted
    got = tables.path_errors(paths[:6], p0[:6], p1[:6])
    for i, name in enumerate(names):
        want = evaluate.AlignmentError(REF_CSV, LIVE_CSV, [(int(l), int(r)) for l, r in paths[i]]).stats()
        assert got[i] == want and got[i]["squared_beat_error"] == want["squared_beat_error"], name
        assert percent_lines(got[i]) == gold[name]["percent_lines"] and got[i]["pct_off_seconds"][3] == gold[name]["returned"], name
    assert got[4] is None and got[5] == am.stats(*model[5])
    with pytest.raises(IndexError, match=r"pair 6:"):
        tables.path_errors(paths, p0, p1)


def test_path_errors_take_the_dtw_paths_triple(tables, dtw_golden):
    from real_time_audio_sync_amd import dtw
    host = host_tables()
    a = torch.from_numpy(np.ascontiguousarray(dtw_golden["dtw_small/a"].T)).to(tables.device)
    b = torch.from_numpy(np.ascontiguousarray(dtw_golden["dtw_small/b"].T)).to(tables.device)
    triple = dtw.dtw_paths(torch.stack([a, a]), b, a_len=[45, 30], b_len=[48, 48])
    got = tables.path_errors(triple, [1, 0], [0, 1])
    path, plen = triple[0].cpu().numpy(), triple[1].cpu().numpy()
    assert (plen > 40).all() and got[0] is not None and got[1] is not None
    for i, (p0, p1) in enumerate([(1, 0), (0, 1)]):
        assert got[i] == am.stats(*am.metric(path[i, :plen[i]].tolist(), host[p0], host[p1], FS)), i


# ---- the live words -------------------------------------------------------------------------------------------------------

class Words(object):
    """The model's sticky words of every stream of a session, driven by the session's own paths."""

    def __init__(self, sess, table_of, frame_seconds):
        self.sess, self.table_of, self.fs = sess, list(table_of), frame_seconds     # table_of[b]: (times, beats, label_ok | None)
        self.sticky = [am.Sticky() for _ in range(sess.B)]
        self.frame0 = [0] * sess.B

    def feed(self):
        for b, s in enumerate(self.sticky):
            p = self.sess.path(b)
            t = self.table_of[b]
            s.feed(int(p[-1][1]) if len(p) else None, t[0], t[1], self.fs, self.frame0[b], t[2])

    def check(self, feeds, where):
        got = self.sess.beats()
        assert got["feeds_done"] == feeds == self.sess.poll()["feeds_done"], where
        assert same_bytes(got["beat"], beat_array(s.beat for s in self.sticky)), (where, got["beat"], [s.beat for s in self.sticky])
        assert got["label"].tolist() == [s.label for s in self.sticky], where
        assert got["ref_frame"].tolist() == [s.ref_frame for s in self.sticky], where
        return got


def cut(audio, pos, sizes):
    bufs = []
    for b, n in enumerate(sizes):
        bufs.append(audio[pos[b]:pos[b] + n])
        pos[b] += n
    return bufs


def test_live_words_otw(chopin_audio, otw_golden, tables):
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.live import LiveSession
    ref = otw_golden["G/ref"]
    live = chopin_audio["live"]
    sess = LiveSession([ref, ref, ref], batch=3, c=20, max_run_count=3)
    times, beats = evaluate.read_ground_truth(REF_CSV)
    words = Words(sess, [(times, beats, [1] * len(times))] * 3, FS)
    pos, feeds = [0, 0, 0], 0
    sizes = [(9000, 5000, 12001), (4097, 0, 7000), (2048, 6143, 1), (10000, 4100, 9999)]
    sess.feed(cut(live, pos, sizes[0]))
    feeds += 1
    sess.sync()
    with pytest.raises(nat.RtsyncError, match="before any rts_live_annotate"):
        sess.beats()
    sess.annotate(tables, piece_of=[(ref, 0)])
    words.check(feeds, "annotate alone publishes nothing")
    for i in range(12):
        sess.feed(cut(live, pos, sizes[(i + 1) % 4]))
        feeds += 1
        sess.sync()
        words.feed()
        got = words.check(feeds, i)
    assert np.isfinite(got["beat"]).all() and (got["label"] >= 0).all() and got["label_text"] == ["0"] * 3
    assert len(set(got["ref_frame"].tolist())) > 1                                   # the streams are at different places
    # "follow from frame 40": stream 1 reads nothing until its next path point, then beats of its piece's own frames
    sess.restart([1], offsets=[40])
    sess.sync()
    words.sticky[1].clear()
    words.frame0[1] = 40
    got = words.check(feeds, "restart")
    assert np.isnan(got["beat"][1]) and got["label"][1] == -1 and got["ref_frame"][1] == -1 and got["label_text"][1] is None
    sess.feed(cut(live, pos, (3000, 100, 3000)))                                     # no column for stream 1 yet
    feeds += 1
    sess.sync()
    words.feed()
    got = words.check(feeds, "after the restart, no column")
    assert got["ref_frame"][1] == -1 and len(sess.path(1)) == 0
    for i in range(6):
        sess.feed(cut(live, pos, sizes[i % 4]))
        feeds += 1
        sess.sync()
        words.feed()
        got = words.check(feeds, ("restarted", i))
    j = int(sess.path(1)[-1][1])
    assert got["ref_frame"][1] == j + 40 and got["beat"][1] == am.lookup(j, times, beats, FS, 40)[0]
    # off: the words stay, later feeds leave them alone
    sess.annotate(None)
    before = sess.beats()
    for i in range(2):
        sess.feed(cut(live, pos, sizes[3]))
        feeds += 1
    sess.sync()
    after = sess.beats()
    assert after["feeds_done"] == feeds and int(sess.path(0)[-1][1]) + 0 != before["ref_frame"][0]
    for key in ("beat", "label", "ref_frame"):
        assert same_bytes(after[key], before[key]), key
    assert after["label_text"] == before["label_text"]
    sess.close()


def test_live_words_wtw(tables, tmp_path):
    from real_time_audio_sync_amd.annotate import AnnotationTables
    from test_live_model_cpu import B, FS as RATE, build_case, wtw_refs
    from test_live_paths_gpu import open_wtw
    case = build_case(512, 128)
    refs = wtw_refs(case, per_stream=True)
    fsec = case.hop / float(RATE)
    # a table with labels (two of them empty) from a three-column CSV, and one without a label column
    rows = [((9 * i + 4) * fsec, i, "" if i in (1, 4) else "bar %d" % i) for i in range(14)]
    csv = tmp_path / "piece.csv"
    csv.write_text("".join("%r,%d,%s\n" % r for r in rows))
    plain = ([(5 * i + 2) * fsec for i in range(40)], list(range(3, 43)))
    tab = AnnotationTables([str(csv), plain], frame_seconds=fsec)
    assert tab.labels[0] == [r[2] for r in rows] and tab.labels[1] is None and list(tab.times[0]) == [r[0] for r in rows]
    sess = open_wtw(case, refs[:B], extra=refs[B:])
    with pytest.raises(ValueError, match="no table"):
        sess.annotate(tab, piece_of=[(refs[0], 0)])
    sess.annotate(tab, piece_of=[(r, b % 2) for b, r in enumerate(refs)])
    host = [([r[0] for r in rows], [r[1] for r in rows], [1 if r[2] else 0 for r in rows]), (plain[0], plain[1], None)]
    words = Words(sess, [host[b % 2] for b in range(B)], fsec)
    pos, feeds = [0] * B, 0
    for f in case.feeds:
        if f["refused"]:
            continue
        sess.feed(cut_streams(case.live, pos, f["counts"]))
        feeds += 1
        sess.sync()
        words.feed()
        got = words.check(feeds, feeds)
    assert np.isfinite(got["beat"]).sum() >= 2 and max(len(sess.path(b)) for b in range(B)) > 8
    for b in range(B):
        lab = got["label"][b]
        want = None if lab < 0 or b % 2 else rows[lab][2]
        assert got["label_text"][b] == want and want != "", b
    assert any(t for t in got["label_text"])
    sess.close()
    tab.close()


def cut_streams(streams, pos, counts):
    bufs = []
    for b, n in enumerate(counts):
        bufs.append(streams[b][pos[b]:pos[b] + n])
        pos[b] += n
    return bufs


def test_live_words_with_the_gate(chopin_audio, otw_golden, tables):
    from real_time_audio_sync_amd.live import LiveSession
    ref = otw_golden["G/ref"]
    live = chopin_audio["live"]
    sess = LiveSession(ref, batch=2, c=20, max_run_count=3)
    sess.gate(-60.0)
    sess.annotate(tables)                                          # a single reference: table 0
    times, beats = evaluate.read_ground_truth(REF_CSV)
    words = Words(sess, [(times, beats, [1] * len(times))] * 2, FS)
    pos = 0
    for i in range(10):
        n = 9000 + 7 * i
        sess.feed([live[pos:pos + n], np.zeros(n, dtype=np.float32)])          # nobody plays into microphone 1
        pos += n
        sess.sync()
        words.feed()
        got = words.check(i + 1, i)
    lv = sess.levels()
    assert lv["passed"][1] == 0 and lv["seen"][1] > 30 and lv["passed"][0] > 20
    assert np.isfinite(got["beat"][0]) and got["ref_frame"][0] >= 0
    assert np.isnan(got["beat"][1]) and got["label"][1] == -1 and got["ref_frame"][1] == -1
    sess.close()
