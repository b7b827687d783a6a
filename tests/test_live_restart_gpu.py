"""rts_live_restart (LiveSession.restart): one microphone of a running session starts its piece again while the others go
on.  Three streams on the committed Chopin recording, fed in irregular buffer sizes; stream 1 is restarted while it holds
pending samples that do not make a column, then receives the recording from its first sample again."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PARAMS = {'fft_len': 4096, 'hop_size': 2048, 'dtw_win_size': 4096 * 10, 'dtw_hop_size': 2048 * 10}  # tests.py:174
SIZES = (1500, 4096, 9000)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _feed_all(sess, src, pos, until=None):
    """Feeds every stream its next buffer (SIZES[b] samples) until all have reached `until[b]` (default: the end)."""
    until = until or [len(src)] * 3
    while any(pos[b] < until[b] for b in range(3)):
        bufs = []
        for b in range(3):
            n = max(0, min(SIZES[b], until[b] - pos[b]))
            bufs.append(src[pos[b]:pos[b] + n] if n else None)
            pos[b] += n
        sess.feed(bufs)


def _run(sess, src, restart, sync_first=True):
    """sync_first=False: the restart is enqueued behind feeds that are still in flight, and the next feeds behind it,
    with no synchronisation in between: only stream order puts the old run's samples before it and the new run's after."""
    third = len(src) // 3
    pos = [0, 0, 0]
    _feed_all(sess, src, pos, until=[third, third + 777, third])
    out = {}
    if restart and sync_first:
        sess.sync()
        before = sess.poll()
        pend = sess.pending()
        assert 0 < pend[1] < 4096 and tuple(before["positions"][1]) != (0, 0)   # samples that do not make a column
        sess.restart([1])
        assert list(sess.pending()) == [pend[0], 0, pend[2]]
        sess.sync()
        after = sess.poll()
        assert after["status"][1] == 0 and tuple(after["positions"][1]) == (0, 0)      # RTS_RUNNING, at the start
        assert after["feeds_done"] >= before["feeds_done"] and after["feeds_submitted"] == before["feeds_submitted"]
        for b in (0, 2):
            assert tuple(after["positions"][b]) == tuple(before["positions"][b]) and after["status"][b] == before["status"][b]
        assert len(sess.path(1)) == 0
        pos[1] = 0
    elif restart:
        pend = sess.pending()                      # the host mirror is exact without a synchronisation
        assert 0 < pend[1] < 4096
        sess.restart([1])
        assert list(sess.pending()) == [pend[0], 0, pend[2]]
        pos[1] = 0
    _feed_all(sess, src, pos)
    sess.sync()
    info = sess.poll()
    assert info["feeds_done"] == info["feeds_submitted"]
    out["info"] = info
    out["paths"] = [sess.path(b) for b in range(3)]
    out["pending"] = list(sess.pending())
    return out


def _check(got, plain, known_path):
    assert np.array_equal(got["paths"][1], known_path)
    for b in (0, 2):
        assert np.array_equal(got["paths"][b], plain["paths"][b]), b
        assert tuple(got["info"]["positions"][b]) == tuple(plain["info"]["positions"][b]), b
        assert got["info"]["status"][b] == plain["info"]["status"][b], b
    # stream 1 ends where a stream that was never restarted ends: same recording, from its first sample
    assert tuple(got["info"]["positions"][1]) == tuple(plain["info"]["positions"][1])
    assert got["pending"] == plain["pending"]


def test_wtw_session_float32(chopin_audio, wtw_known_answer):
    """The restarted stream must give the reference's own known answer (Songs/chopin/tests/wtw_test_20b.txt, 509 pairs)."""
    from real_time_audio_sync_amd import chroma
    from real_time_audio_sync_amd.live import LiveSession
    plan = chroma._plan()
    ref_dev = torch.from_numpy(chopin_audio["ref"]).to(plan.device)
    ref_chroma = plan.frames(ref_dev, pad_left=2048)[0].t().contiguous().cpu().numpy()      # wtw.py:37-41
    live = chopin_audio["live"]
    assert len(wtw_known_answer) == 509
    res = []
    for restart in (True, False):
        sess = LiveSession(ref_chroma, batch=3, wtw_params=PARAMS)
        res.append(_run(sess, live, restart))
        sess.close()
    _check(res[0], res[1], wtw_known_answer)
    assert np.array_equal(res[1]["paths"][1], wtw_known_answer)


def test_otw_session_pcm16(chopin_audio, otw_golden):
    """PCM16 feeds into an OTW session, the restart enqueued behind feeds still in flight; the restarted stream must give
    the oracle's path on the same samples."""
    import oracle
    from oracle import chroma_oracle
    from real_time_audio_sync_amd.live import LiveSession
    ref_chroma = otw_golden["G/ref"]
    pcm = np.round(chopin_audio["live"] * 32768.0).astype(np.int16)
    live = pcm.astype(np.float32) / np.float32(32768.0)
    n = (len(live) - 4096) // 2048 + 1
    cols = np.stack([chroma_oracle.wav_to_chroma_col(live[m * 2048:m * 2048 + 4096]) for m in range(n)], axis=1)
    o = oracle.OtwOracle(ref_chroma, 50, 3)
    o.run(cols)
    res = []
    for restart in (True, False):
        sess = LiveSession(ref_chroma, batch=3, c=50, max_run_count=3)
        res.append(_run(sess, pcm, restart, sync_first=False))
        sess.close()
    _check(res[0], res[1], o.path)
    assert tuple(res[0]["info"]["positions"][1]) == (o.state["t"], o.state["j"])


def test_restart_onto_another_piece(chopin_audio):
    """A session with per-stream references and an extra piece: stream 0 moves on to the extra piece and then equals a
    session of its own on that piece; the staging slot handed out before the restart stays valid."""
    from real_time_audio_sync_amd import chroma
    from real_time_audio_sync_amd.live import LiveSession
    plan = chroma._plan()
    to_chroma = lambda x: plan.frames(torch.from_numpy(np.ascontiguousarray(x)).to(plan.device), pad_left=2048)[0].t().contiguous().cpu().numpy()
    live = chopin_audio["live"][:200000]
    piece_a, piece_b = to_chroma(chopin_audio["ref"][:150000]), to_chroma(chopin_audio["live"][:260000])
    sess = LiveSession([piece_a, piece_a], batch=2, c=30, extra_refs=[piece_b])
    for i in range(0, 60000, 6000):
        sess.feed([live[i:i + 6000]] * 2)
    cv, sv = sess.staging(np.float32)            # handed out, written, not yet submitted
    cv[:] = (5000, 6000)
    sv[:5000] = live[:5000]
    sv[5000:11000] = live[60000:66000]
    sess.restart([0], refs=[piece_b])
    assert list(sess.pending())[0] == 0 and list(sess.otw.ref_lens) == [piece_b.shape[1], piece_a.shape[1]]
    sess.submit(np.float32)
    pos = [5000, 66000]
    while pos[0] < len(live):
        bufs = [live[pos[0]:pos[0] + 7000], live[pos[1]:pos[1] + 6000] if pos[1] < len(live) else None]
        sess.feed(bufs)
        pos = [pos[0] + 7000, pos[1] + 6000]
    sess.sync()
    one_b = LiveSession(piece_b, batch=1, c=30)
    one_a = LiveSession(piece_a, batch=1, c=30)
    for i in range(0, len(live), 8192):
        one_b.feed([live[i:i + 8192]])
    for i in range(0, min(pos[1], len(live)), 8192):
        one_a.feed([live[i:min(i + 8192, pos[1])]])
    one_a.sync()
    one_b.sync()
    assert np.array_equal(sess.path(0), one_b.path(0)) and len(sess.path(0)) > 50
    assert np.array_equal(sess.path(1), one_a.path(0))
    assert np.array_equal(sess.otw.states()[0][:15], one_b.otw.states()[0][:15])   # (slot 15 counts per launch granularity)
    for s in (sess, one_a, one_b):
        s.close()
