"""rts_wtw_export / rts_wtw_import (BatchedWTW.export_streams / import_streams): the scheme of
tests/test_snapshot_otw_gpu.py for the windowed tracker.  Streams of a six-stream handle move into slots of a five-slot
handle with a longer M_max and another slot layout, in the middle of a partly filled window, and go on bit for bit like
the control twin that was never exported, and like the WTW oracle fed the whole sequence push by push.  W / hop = 20 / 10
runs the window kernel with one DP wave, 100 / 50 with two, 130 / 65 the strip DP; one case moves streams from a strip-DP
handle (RTS_WTW_WIN=0 at W = 100) to a window-kernel handle, whose control words do not exist."""
import ctypes

import numpy as np
import pytest

from guarded import guarded
from test_restart_gpu import Feeder, _same_wtw_stream, _wtw_vs_oracle
from test_snapshot_otw_gpu import SLOTS, STREAMS, records

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def owned(eng, b, keep_d):
    frames, lens = eng.recent(256)
    d = eng.last_d(b).tobytes() if keep_d and eng.state(b)["windows"] > 0 else b""
    return (eng.states()[b].tobytes(), eng.path(b).tobytes(), frames[b].cpu().numpy().tobytes(), int(lens[b]), d)


def push_moved(fe, target, own_seq, own_pos, own_log):
    """The last round of ``fe`` for the streams STREAMS, into the slots SLOTS of ``target``; its own stream (slot 4) gets
    up to 17 columns of ``own_seq``."""
    width = fe.log[0][-1][0]
    buf = np.zeros((5, width, 12))
    counts = [0] * 5
    for b, s in zip(STREAMS, SLOTS):
        n = fe.log[b][-1][1]
        buf[s, :n] = fe.seqs[b][:, fe.pos[b] - n:fe.pos[b]].T
        counts[s] = n
    counts[4] = min(17, width, own_seq.shape[1] - own_pos)
    buf[4, :counts[4]] = own_seq[:, own_pos:own_pos + counts[4]].T
    target.push(torch.from_numpy(buf).to("cuda:0"), torch.tensor(counts, dtype=torch.int32, device="cuda:0"))
    own_log.append((width, counts[4]))
    return own_pos + counts[4]


@pytest.mark.parametrize("W,hopf,keep_d,flavour", [(20, 10, False, "default"), (20, 10, True, "default"),
                                                   (100, 50, False, "default"), (100, 50, True, "default"),
                                                   (130, 65, False, "default"), (130, 65, True, "default"),
                                                   (100, 50, True, "win0")])
def test_moved_streams_continue_bit_for_bit(monkeypatch, tmp_path, W, hopf, keep_d, flavour):
    from real_time_audio_sync_amd import _native as nat, synth
    from real_time_audio_sync_amd.snapshot import Snapshot
    from real_time_audio_sync_amd.wtw import BatchedWTW
    dev = torch.device("cuda:0")
    tag = (W, hopf, keep_d, flavour)
    to_dev = lambda r: torch.from_numpy(np.ascontiguousarray(r.T)).to(dev)
    scale = lambda l, s: l * (0.5 + np.random.RandomState(s).rand(1, l.shape[1]))
    M = 300
    ref = synth.synth_ref(M, seed=800)
    short = np.ascontiguousarray(ref[:, :W + W // 4])                     # stream 2: stops right after its first window
    r5 = np.ascontiguousarray(ref[:, :M - 33])                            # stream 5: a range of its own length
    longer = synth.synth_ref(M + 57, seed=801)
    t_ref, t_short, t_r5, t_longer = to_dev(ref), to_dev(short), to_dev(r5), to_dev(longer)
    np_of = {4: ref, 0: ref, 2: short, 5: r5}
    lives = [scale(synth.synth_live(r, seed=810 + b), b) for b, r in enumerate([ref, ref, short, ref, ref, r5])]
    lives[2] = scale(synth.synth_live(ref, seed=812), 2)                  # more columns than its range can take
    own = scale(synth.synth_live(longer, seed=830), 30)
    if flavour == "win0":
        monkeypatch.setenv("RTS_WTW_WIN", "0")
    mk_a = lambda: BatchedWTW.with_references([t_ref, t_ref, t_short, t_ref, t_ref, t_r5], W, hopf, keep_last_d=keep_d)
    eng, ctl = mk_a(), mk_a()
    monkeypatch.delenv("RTS_WTW_WIN", raising=False)
    tgt = BatchedWTW.with_references([t_longer, t_short, t_ref, t_longer, t_longer], W, hopf, keep_last_d=keep_d,
                                     extra_refs=[t_r5])
    assert tgt.M == M + 57 and eng.M == M
    own_pos, own_log = 0, []
    for n in (W + 3, 7):                                                  # C is in use before anything arrives
        buf = np.zeros((5, n, 12))
        buf[4] = own[:, own_pos:own_pos + n].T
        tgt.push(torch.from_numpy(buf).to(dev), torch.tensor([0, 0, 0, 0, n], dtype=torch.int32, device=dev))
        own_log.append((n, n))
        own_pos += n

    # small pushes up to the export, so that at M = 300 the long windows are still running then (W = 130 stops at
    # ref_ptr >= 169, after its third window); pushes of several windows afterwards
    chunks, chunks_after = (hopf // 2 + 3, 5, hopf // 3 + 1, 7), (2 * W + 1, 5, hopf, 3 * hopf + 1, hopf + 3)
    held = lives[4]
    seqs = list(lives)
    seqs[4] = held[:, :0]                                                 # stream 4 hears nothing until it has moved
    fe = Feeder(seqs, torch.float64, chunks)
    while fe.pos[0] < lives[0].shape[1] // 2 or fe.pos[2] < W + 8:       # (streams 2 and 5 lag two columns a round)
        fe.round([eng, ctl])
    st = eng.states()
    assert not st[4].any(), tag
    assert st[2][3] == nat.STOP_REF_END and st[0][3] == nat.RUNNING and st[0][5] > 0 and st[5][5] > 0, tag
    assert 0 < st[0][0] - st[0][1] < W, (tag, "the export falls into a partly filled window", st[0])

    before_a = [owned(eng, b, keep_d) for b in range(6)]
    need = ctypes.c_size_t()
    nat.check(nat.lib.rts_wtw_snapshot_bytes(eng._h, ctypes.byref(need)))
    blob0, chk0 = guarded((4, need.value), torch.uint8, "cuda:0", 0x00)
    blob1, chk1 = guarded((4, need.value), torch.uint8, "cuda:0", 0xFF)
    snap = eng.export_streams(STREAMS, verify=True, blob=blob0)
    eng.export_streams(STREAMS, blob=blob1)
    torch.cuda.synchronize()
    chk0("blob 0x00")
    chk1("blob 0xFF")
    assert torch.equal(blob0, blob1), tag
    recs, zero_tail = records(snap)
    assert zero_tail and [owned(eng, b, keep_d) for b in range(6)] == before_a, tag
    hdr = snap.headers()
    assert list(hdr[:, 4]) == [M, M, short.shape[1], r5.shape[1]] and not hdr[:, 3].any(), tag
    assert hdr[0, 5] == 0 and hdr[0, 8] == 0 and list(hdr[1:, 8]) == [W if keep_d else 0] * 3, tag
    assert snap.desc["window"] == W and snap.desc["hop"] == hopf and snap.desc["keep_last_d"] == int(keep_d), tag
    if keep_d:                                                            # half of the cases go through a file
        snap.save(str(tmp_path / "moved.npz"))
        snap = Snapshot.load(str(tmp_path / "moved.npz"), "cuda:0")

    before_own = owned(tgt, 4, keep_d)
    status, chk_s = guarded((4,), torch.int32, "cuda:0", 0x55)
    got = tgt.import_streams(snap, SLOTS, refs=[t_ref, t_ref, t_short, t_r5], status=status)
    chk_s("status")
    assert not got.any() and owned(tgt, 4, keep_d) == before_own, tag
    assert list(tgt.ref_lens) == [short.shape[1], M, M, r5.shape[1], M + 57], tag
    for b, s in zip(STREAMS, SLOTS):
        assert owned(tgt, s, keep_d) == before_a[b], (tag, "right after the import", b)
    again = tgt.export_streams(SLOTS)
    recs2, zero_tail2 = records(again)
    assert recs2 == recs and zero_tail2, tag

    fe.seqs[4], fe.chunks = held, chunks_after
    while not fe.done():
        fe.round([eng, ctl])
        own_pos = push_moved(fe, tgt, own, own_pos, own_log)
    assert eng.state(4)["windows"] > 0, tag
    for b, s in zip(STREAMS, SLOTS):
        _same_wtw_stream(tgt, s, ctl, b, (tag, "moved", b))
        if keep_d and ctl.state(b)["windows"] > 0:
            assert np.array_equal(tgt.last_d(s), ctl.last_d(b)), (tag, "D", b)
        _wtw_vs_oracle(tgt, s, np_of[b], fe.seqs[b], fe.log[b], W, hopf, (tag, "moved", b))
    for b in range(6):
        _same_wtw_stream(eng, b, ctl, b, (tag, "exporter", b))
    tp_c, tp_a = tgt.tempo(32, 1.0), ctl.tempo(32, 1.0)
    fr_c, ln_c = (t.cpu().numpy() for t in tgt.recent(64))
    fr_a, ln_a = (t.cpu().numpy() for t in ctl.recent(64))
    for b, s in zip(STREAMS, SLOTS):
        assert all(tp_c[m][s].tobytes() == tp_a[m][b].tobytes() for m in range(3)), (tag, "tempo", b)
        assert ln_c[s] == ln_a[b] and fr_c[s].tobytes() == fr_a[b].tobytes(), (tag, "recent", b)
    assert records(tgt.export_streams(SLOTS))[0] == records(ctl.export_streams(STREAMS))[0], tag
    _wtw_vs_oracle(tgt, 4, longer, own, own_log, W, hopf, (tag, "C's own stream"))
    for e in (eng, ctl, tgt):
        e.close()


def test_refusals():
    from real_time_audio_sync_amd import _native as nat, synth
    from real_time_audio_sync_amd.wtw import BatchedWTW
    dev = torch.device("cuda:0")
    to_dev = lambda r: torch.from_numpy(np.ascontiguousarray(r.T)).to(dev)
    ref = synth.synth_ref(120, seed=3)
    t_ref, t_short = to_dev(ref), to_dev(np.ascontiguousarray(ref[:, :100]))
    cols = torch.from_numpy(np.ascontiguousarray(np.stack([synth.synth_live(ref, seed=5 + b)[:, :45].T for b in range(3)]))).to(dev)
    src = BatchedWTW(t_ref, 20, 10, batch=3, keep_last_d=True)
    src.push(cols)
    snap = src.export_streams([2, 0])

    def refused(word, fn, *args, **kw):
        with pytest.raises(nat.RtsyncError) as e:
            fn(*args, **kw)
        assert "rtsync error -1:" in str(e.value) and word in str(e.value), str(e.value)

    for kw, word in ((dict(win_frames=21), "window"), (dict(hop_frames=5), "hop"), (dict(keep_last_d=False), "keep_last_d")):
        args = dict(dict(win_frames=20, hop_frames=10, keep_last_d=True), **kw)
        h = BatchedWTW(t_ref, args["win_frames"], args["hop_frames"], batch=2, keep_last_d=args["keep_last_d"])
        before = h.states().copy()
        refused("field " + word, h.import_streams, snap, [0, 1])
        assert np.array_equal(h.states(), before)
        h.close()
    refused("twice", src.export_streams, [1, 1])
    tgt = BatchedWTW.with_references([t_ref, t_short, t_ref], 20, 10, keep_last_d=True)
    tgt.push(cols[:, :25].contiguous())
    before = [owned(tgt, b, True) for b in range(3)]
    status, chk = guarded((2,), torch.int32, "cuda:0", 0xFF)
    with pytest.raises(nat.RtsyncError) as e:
        tgt.import_streams(snap, [1, 2], status=status)
    assert "stream 1 refused record 0" in str(e.value) and "status 4" in str(e.value), str(e.value)
    chk("status")
    assert status.cpu().tolist() == [4, 0]
    assert [owned(tgt, b, True) for b in (0, 1)] == before[:2] and owned(tgt, 2, True) == owned(src, 0, True)
    # an OTW record is no WTW record: the desc says so before anything runs
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    otw = BatchedOTW(ref, 20, 3, batch=2, dtype=torch.float64)
    refused("field kind", otw.import_streams, snap, [0, 1])
    for e in (src, tgt, otw):
        e.close()
