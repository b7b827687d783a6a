"""Ensemble following on the device (csrc/ensemble.hip, annot_frames_kernel of csrc/annot.hip) against the plain-Python model
of the definitions (tests/ensemble_model.py, itself held to closed forms in tests/test_ensemble_cpu.py): the inverse lookup,
the offline curve on groups of 1, 2, 33 and 64 members, the fusion step on OTW and WTW handles push by push, and the words a
live session publishes with every feed -- the Chopin recordings followed against three references, one of which cannot
follow, and a member put back by heal().  Every word is compared bit for bit."""
import ctypes
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import ensemble_model as em  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from guarded import guarded, holds_fill, same_bytes  # noqa: E402
from real_time_audio_sync_amd import evaluate, synth  # noqa: E402

REF_CSV = os.path.join(GOLDEN, "chopin_rubinstein_20b.csv")
LIVE_CSV = os.path.join(GOLDEN, "chopin_rachmaninoff_20b.csv")
FS = evaluate.FRAME_SECONDS
DEV = "cuda:0"
INF = math.inf
SYNTH = ([0.0, 1.0, 1.0, 2.5, 4.0, 7.0], [0, 1, 2, 3, 7, 8])        # times[0] == 0, a zero-width row, a gap in the beats
FLAT = ([0.5, 1.0, 1.5, 2.0], [1, 2, 2, 3])                         # not invertible


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def d32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32))).to(DEV)


def f64(a):
    return np.array(a, dtype=np.float64)


# ---- 1. rts_annot_frames ---------------------------------------------------------------------------------------------------

def test_annot_frames_equals_the_model():
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.annotate import AnnotationTables
    host = [evaluate.read_ground_truth(REF_CSV), evaluate.read_ground_truth(LIVE_CSV), SYNTH, FLAT]
    tab = AnnotationTables([REF_CSV, LIVE_CSV, SYNTH, FLAT], device=DEV)
    try:
        B, n_max = 5, 300
        n = [300, 257, 40, 120, 5]
        pieces = [0, 1, 2, 3, 9]                                     # stream 3: not invertible; stream 4: no such piece
        rs = np.random.RandomState(12)
        x = np.zeros((B, n_max))
        for b in range(B):
            beats = host[pieces[b]][1] if pieces[b] < len(host) else [0, 10]
            x[b] = rs.uniform(beats[0] - 3.0, beats[-1] + 3.0, size=n_max)       # negative values and beats past the end
            rows = np.array(beats, dtype=np.float64)
            x[b, 10:10 + min(len(rows), 25)] = rows[:25]             # exact row beats
            x[b, 5] = np.nan
            x[b, 6] = -np.inf
            x[b, 7] = np.inf
            x[b, 8] = -0.0
            x[b, 9] = float(beats[-1])                               # the last beat itself
        x[2, :10] = [0.0, -0.5, -1.0, 0.5, 1.5, np.nan, 5.0, 6.0, 6.5, 8.0]
        want = np.full((B, n_max), -7, dtype=np.int32)
        for b in range(B):
            t = host[pieces[b]] if pieces[b] < len(host) else None
            for k in range(n[b]):
                want[b, k] = em.invert(float(x[b, k]), list(t[0]), list(t[1]), FS) if t is not None else -1
        assert (want[0, :n[0]] >= 0).sum() > 150 and (want[0, :n[0]] == -1).sum() > 20
        assert (want[2, :n[2]] >= 0).sum() > 10 and (want[3, :n[3]] == -1).all() and (want[4, :n[4]] == -1).all()
        x_d, n_d, pieces_d = torch.from_numpy(x).to(DEV), d32(n), d32(pieces)
        for fill in (0x55, 0xFF):
            out, check = guarded((B, n_max), torch.int32, DEV, fill)
            nat.check(nat.lib.rts_annot_frames(tab._h, x_d.data_ptr(), n_max, n_d.data_ptr(), pieces_d.data_ptr(), B,
                                               out.data_ptr(), None))
            torch.cuda.synchronize()
            check("frame_dev")
            got = out.cpu().numpy()
            for b in range(B):
                assert np.array_equal(got[b, :n[b]], want[b, :n[b]]), (b, got[b, :n[b]], want[b, :n[b]])
                assert holds_fill(got[b, n[b]:], fill), b            # entries behind n_dev: untouched
        got = tab.frames([x[b, :n[b]] for b in range(B)], pieces)
        for b in range(B):
            assert np.array_equal(got[b], want[b, :n[b]]), b
        # the round trip on the device: frame -> beats() -> frames()
        frames = np.arange(0, 380, dtype=np.int32)
        beat = tab.beats([frames, frames], [0, 1])
        for p in range(2):
            has = ~np.isnan(beat[p][0])
            assert has.sum() > 200
            back = tab.frames([beat[p][0][has]], [p])[0]
            assert np.array_equal(back, frames[has]), p
    finally:
        tab.close()


# ---- 2. rts_path_consensus -------------------------------------------------------------------------------------------------

P_MAX, T = 120, 50
SIZES = (1, 2, 33, 64)


@pytest.fixture(scope="module")
def corpus():
    return build_corpus()


def build_corpus():
    """B = 102 paths: groups of 1, 2, 33 and 64 members interleaved in stream order and two streams in no group; monotone
    random walks, one empty path, one with the -1 length marker, two members with the same path and piece (a tie)."""
    rs = np.random.RandomState(21)
    groups = np.concatenate([np.full(s, g) for g, s in enumerate(SIZES)] + [np.full(2, -1)])
    rs.shuffle(groups)
    B = len(groups)
    assert B == 102
    steps = np.array([(1, 0), (0, 1), (1, 1)])
    host = np.zeros((B, P_MAX, 2), dtype=np.int32)
    lens = rs.randint(30, P_MAX + 1, size=B).astype(np.int32)
    for b in range(B):
        pts = np.cumsum(steps[rs.randint(0, 3, size=P_MAX)], axis=0) + (rs.randint(0, 6), rs.randint(0, 40))
        host[b] = pts
    pieces = rs.choice([0, 0, 0, 1, 1, 1, 2], size=B).astype(np.int32)
    frame0 = rs.randint(0, 60, size=B).astype(np.int32)
    big = [b for b in range(B) if groups[b] == 3]
    lens[big[5]] = 0                                                 # an empty path
    lens[big[50]] = -1                                               # the fault marker of rts_dtw_paths
    lens[big[63]] = 10 ** 6                                          # clamped to P_max
    pieces[big[7]] = 9                                               # a member without a piece
    host[big[20], 3, 1] = -4                                         # a negative reference index on the way
    host[big[61]] = host[big[2]]                                     # the last member ties with an early one
    pieces[big[61]], frame0[big[61]], lens[big[61]] = pieces[big[2]], frame0[big[2]], lens[big[2]]
    mid = [b for b in range(B) if groups[b] == 2]
    host[mid[32]] = host[mid[0]]                                     # and the 33rd lane with lane 0
    pieces[mid[32]], frame0[mid[32]], lens[mid[32]] = pieces[mid[0]], frame0[mid[0]], lens[mid[0]]
    host[np.arange(P_MAX)[None, :] >= np.clip(lens, 0, P_MAX)[:, None]] = (-9, 1 << 30)     # behind len: never read
    tables = [evaluate.read_ground_truth(REF_CSV), evaluate.read_ground_truth(LIVE_CSV), SYNTH]
    paths = [[tuple(p) for p in host[b, :max(0, min(int(lens[b]), P_MAX))].tolist()] for b in range(B)]
    want = {}
    for max_dev, patience in ((INF, 1), (1.5, 3)):
        want[max_dev, patience] = em.curve(paths, groups.tolist(), tables, pieces.tolist(), frame0.tolist(), T, FS, max_dev,
                                           patience)
    return dict(groups=groups.astype(np.int32), host=host, lens=lens, pieces=pieces, frame0=frame0, want=want, B=B)


@pytest.mark.parametrize("max_dev,patience", [(INF, 1), (1.5, 3)])
def test_path_consensus_equals_the_model(corpus, max_dev, patience):
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.annotate import AnnotationTables
    from real_time_audio_sync_amd.ensemble import Ensemble
    cons_w, spread_w, n_in_w, out_w = corpus["want"][max_dev, patience]
    B, G = corpus["B"], len(SIZES)
    flat_out = np.array(out_w)
    if max_dev == INF:
        assert not flat_out.any()
    else:                                                            # members go out and come back, in the upper half too
        assert flat_out[corpus["groups"] == 3].any() and flat_out[corpus["groups"] == 2].any()
        assert (np.diff(flat_out, axis=1) < 0).any()
    assert np.isnan(f64(cons_w)).any() and np.isfinite(f64(cons_w)).sum() > 150
    assert max(max(r) for r in n_in_w) >= 50                         # votes in both halves of the wave
    tab = AnnotationTables([REF_CSV, LIVE_CSV, SYNTH], device=DEV)
    ens = Ensemble(corpus["groups"], max_dev, patience, device=DEV)
    try:
        path_d, len_d = torch.from_numpy(corpus["host"]).to(DEV), d32(corpus["lens"])
        pieces_d, frame0_d = d32(corpus["pieces"]), d32(corpus["frame0"])
        for fill, optional in ((0x55, True), (0xFF, True), (0x55, False)):
            cons, c0 = guarded((G, T), torch.float64, DEV, fill)
            spread, c1 = guarded((G, T), torch.float64, DEV, fill)
            n_in, c2 = guarded((G, T), torch.int32, DEV, fill)
            out, c3 = guarded((B, T), torch.int32, DEV, fill)
            nat.check(nat.lib.rts_path_consensus(ens._h, tab._h, path_d.data_ptr(), P_MAX, len_d.data_ptr(), pieces_d.data_ptr(),
                                                 frame0_d.data_ptr(), T, cons.data_ptr(),
                                                 spread.data_ptr() if optional else None,
                                                 n_in.data_ptr() if optional else None,
                                                 out.data_ptr() if optional else None, None))
            torch.cuda.synchronize()
            for chk, what in ((c0, "consensus_dev"), (c1, "spread_dev"), (c2, "n_in_dev"), (c3, "out_dev")):
                chk(what)
            for g in range(G):
                assert same_bytes(cons.cpu().numpy()[g], f64(cons_w[g])), (fill, g)
            if optional:
                assert same_bytes(spread.cpu().numpy(), f64(spread_w))
                assert np.array_equal(n_in.cpu().numpy(), np.array(n_in_w, dtype=np.int32))
                assert np.array_equal(out.cpu().numpy(), flat_out.astype(np.int32))
            else:
                assert holds_fill(spread, fill) and holds_fill(n_in, fill) and holds_fill(out, fill)
        # T == 0 enqueues nothing; T < 0 is refused and names the argument
        assert nat.lib.rts_path_consensus(ens._h, tab._h, path_d.data_ptr(), P_MAX, len_d.data_ptr(), pieces_d.data_ptr(), None, 0,
                                          None, None, None, None, None) == 0
        assert nat.lib.rts_path_consensus(ens._h, tab._h, path_d.data_ptr(), P_MAX, len_d.data_ptr(), pieces_d.data_ptr(), None, -1,
                                          None, None, None, None, None) == -1
        assert b"T" in nat.lib.rts_last_error()
    finally:
        ens.close()
        tab.close()


def test_path_consensus_wrapper(corpus):
    from real_time_audio_sync_amd import ensemble
    from real_time_audio_sync_amd.annotate import AnnotationTables
    tab = AnnotationTables([REF_CSV, LIVE_CSV, SYNTH], device=DEV)
    try:
        cons_w, spread_w, n_in_w, out_w = corpus["want"][1.5, 3]
        paths = [corpus["host"][b, :max(0, min(int(n), P_MAX))] for b, n in enumerate(corpus["lens"])]
        cons, spread, n_in, out = ensemble.path_consensus(paths, corpus["groups"], tab, corpus["pieces"], T,
                                                          frame0=corpus["frame0"], max_dev=1.5, patience=3)
        assert same_bytes(cons.cpu().numpy(), f64(cons_w)) and same_bytes(spread.cpu().numpy(), f64(spread_w))
        assert np.array_equal(n_in.cpu().numpy(), np.array(n_in_w)) and np.array_equal(out.cpu().numpy(), np.array(out_w))
    finally:
        tab.close()


# ---- 3. the trackers -------------------------------------------------------------------------------------------------------

def frames_of(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).T)).to(torch.float64).to(DEV)


def synth_tables(rs, B, seconds):
    """One table per stream: the same beats at slightly different times, like several performances of one score."""
    base = np.cumsum(rs.uniform(0.25, 0.7, size=int(seconds / 0.25)))
    base = base[base < seconds]
    out = []
    for _ in range(B):
        times = np.sort(base * rs.uniform(0.97, 1.03) + rs.uniform(-0.05, 0.05, size=len(base)))
        out.append(([float(t) for t in times], list(range(3, 3 + len(times)))))
    return out


def model_step(eng, groups, tables, pieces, frame0, strikes, out, max_dev, patience):
    """One fusion step of every group from the tracker's paths as they stand -> the words, `strikes` / `out` advanced."""
    B, G = len(groups), max(groups) + 1
    betas = []
    for b in range(B):
        p = eng.path(b)
        tab = tables[pieces[b]] if 0 <= pieces[b] < len(tables) else (None, None)
        betas.append(em.member_beat(int(p[-1][1]) if len(p) else None, tab[0], tab[1], FS, frame0[b]))
    words = dict(consensus=[], spread=[], n_in=[], n_valid=[], dev=[em.NAN] * B)
    for g in range(G):
        mem = [b for b in range(B) if groups[b] == g]
        s, o = [strikes[b] for b in mem], [out[b] for b in mem]
        c, sp, n_in, n_valid, devs = em.fuse_step([betas[b] for b in mem], s, o, max_dev, patience)
        for k, b in enumerate(mem):
            strikes[b], out[b], words["dev"][b] = s[k], o[k], devs[k]
        for key, v in zip(("consensus", "spread", "n_in", "n_valid"), (c, sp, n_in, n_valid)):
            words[key].append(v)
    words["strikes"] = [strikes[b] if groups[b] >= 0 else 0 for b in range(B)]
    words["out"] = [out[b] if groups[b] >= 0 else 0 for b in range(B)]
    return words


def same_words(got, want, where):
    for key in ("consensus", "spread", "dev"):
        assert same_bytes(np.asarray(got[key], dtype=np.float64), f64(want[key])), (where, key, got[key], want[key])
    for key in ("n_in", "n_valid", "strikes", "out"):
        assert np.asarray(got[key]).tolist() == list(want[key]), (where, key, got[key], want[key])


def run_tracker(eng, lives, groups, per_call):
    from real_time_audio_sync_amd.annotate import AnnotationTables
    from real_time_audio_sync_amd.ensemble import Ensemble
    B = eng.B
    rs = np.random.RandomState(31)
    tables = synth_tables(rs, B, 24.0)
    pieces = list(range(B))
    pieces[2] = B + 3                                                # a member without a piece
    frame0 = [int(v) for v in rs.randint(0, 4, size=B)]
    max_dev, patience = 0.4, 3
    tab = AnnotationTables(tables, device=DEV)
    ens = Ensemble(groups, max_dev, patience, device=DEV)
    strikes, out = [0] * B, [0] * B
    try:
        pos = [0] * B
        seen_out = seen_strike = False
        for call in range(10):
            n = [min(per_call + (b + call) % 5, lives[b].shape[1] - pos[b]) if not (b == 1 and call < 2) else 0 for b in range(B)]
            buf = torch.zeros((B, max(max(n), 1), 12), dtype=torch.float64, device=DEV)
            for b in range(B):
                buf[b, :n[b]] = frames_of(lives[b][:, pos[b]:pos[b] + n[b]])
                pos[b] += n[b]
            eng.push(buf, d32(n))
            want = model_step(eng, groups, tables, pieces, frame0, strikes, out, max_dev, patience)
            got = eng.consensus(ens, tab, pieces, frame0)
            same_words(got, want, call)
            seen_out = seen_out or any(want["out"])
            seen_strike = seen_strike or any(s and not o for s, o in zip(want["strikes"], want["out"]))
        assert seen_out and seen_strike and np.isfinite(got["consensus"]).all()
        assert np.isnan(got["dev"][2]) and np.isnan(got["dev"][groups.index(-1)])
        # rts_ensemble_reset with a mask clears exactly the masked streams; the carried state is the handle's
        struck = [b for b in range(B) if strikes[b] > 0]
        assert len(struck) >= 2
        ens.reset(struck[::2])
        for b in struck[::2]:
            strikes[b] = out[b] = 0
        want = model_step(eng, groups, tables, pieces, frame0, strikes, out, max_dev, patience)
        same_words(eng.consensus(ens, tab, pieces, frame0), want, "after the masked reset")
        ens.reset()
        strikes, out = [0] * B, [0] * B
        want = model_step(eng, groups, tables, pieces, frame0, strikes, out, max_dev, patience)
        same_words(eng.consensus(ens, tab, pieces, frame0), want, "after the full reset")
    finally:
        ens.close()
        tab.close()


def test_otw_consensus_equals_the_model():
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    N = 200
    groups = [1, 2, 1, 0, 2, 2, -1, 1, 2, 2, 1, 2, 2]               # groups of 1, 4 and 7, interleaved; stream 6 in none
    assert [groups.count(g) for g in (0, 1, 2, -1)] == [1, 4, 7, 1]
    refs = [synth.synth_ref(N, seed=70 + b) for b in range(13)]
    lives = [synth.synth_live(r, seed=90 + b) for b, r in enumerate(refs)]
    eng = BatchedOTW.with_references(refs, 20, 3, dtype=torch.float64, device=DEV)
    try:
        run_tracker(eng, lives, groups, 17)
    finally:
        eng.close()


def test_wtw_consensus_equals_the_model():
    from real_time_audio_sync_amd.wtw import BatchedWTW
    groups = [0, 1, 0, 0, -1, 1]
    refs = [synth.synth_ref(120, seed=110 + b) for b in range(6)]
    lives = [synth.synth_live(r, seed=130 + b) for b, r in enumerate(refs)]
    eng = BatchedWTW.with_references([frames_of(r) for r in refs], 8, 4)
    try:
        run_tracker(eng, lives, groups, 9)
    finally:
        eng.close()


def test_consensus_refusals():
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.annotate import AnnotationTables
    from real_time_audio_sync_amd.ensemble import Ensemble
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    eng = BatchedOTW(synth.synth_ref(40, seed=1), 5, 3, batch=3, dtype=torch.float64, device=DEV)
    tab = AnnotationTables([SYNTH], device=DEV)
    ens = Ensemble([0, 0, 0, 0], device=DEV)                         # four streams: not this tracker's three
    try:
        with pytest.raises(nat.RtsyncError, match="B = 4"):
            eng.consensus(ens, tab, [0, 0, 0, 0])
        x = d32([0, 0, 0, 0])
        f = nat.lib.rts_otw_consensus
        assert f(eng._h, None, tab._h, x.data_ptr(), None, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None) == -1
        assert b"e is NULL" in nat.lib.rts_last_error()
        assert f(eng._h, ens._h, None, x.data_ptr(), None, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None) == -1
        assert b"tables" in nat.lib.rts_last_error()
        assert f(eng._h, ens._h, tab._h, x.data_ptr(), None, x.data_ptr(), x.data_ptr(), None, x.data_ptr(), None) == -1
        assert b"dev_dev" in nat.lib.rts_last_error()
    finally:
        ens.close()
        tab.close()
        eng.close()


# ---- 4., 5. live: the Chopin fixture ---------------------------------------------------------------------------------------

C = 50
MAX_DEV, PATIENCE = 2.0, 4
CUTS = ([21000, 14097, 30000, 18048, 26001, 9000], [17000, 0, 33143, 24100, 19999, 25001, 1])   # per microphone, cycled


def live_model(sess, tables, frame0, strikes, out):
    """One fusion step per microphone from the session's paths as they stand."""
    G, mics = sess.G, sess.mics
    words = dict(consensus=[], spread=[], n_in=[], n_valid=[], dev=[], strikes=[], out=[])
    for mic in range(mics):
        betas = []
        for k in range(G):
            b = mic * G + k
            p = sess.live.path(b)
            betas.append(em.member_beat(int(p[-1][1]) if len(p) else None, tables[k][0], tables[k][1], FS, frame0[b]))
        s, o = strikes[mic * G:(mic + 1) * G], out[mic * G:(mic + 1) * G]
        c, sp, n_in, n_valid, devs = em.fuse_step(betas, s, o, MAX_DEV, PATIENCE)
        strikes[mic * G:(mic + 1) * G], out[mic * G:(mic + 1) * G] = s, o
        for key, v in zip(("consensus", "spread", "n_in", "n_valid"), (c, sp, n_in, n_valid)):
            words[key].append(v)
        words["dev"] += devs
        words["strikes"] += s
        words["out"] += o
    return words


def check_live(sess, want, feeds, where):
    got = sess.consensus()
    assert got["feeds_done"] == feeds == sess.live.poll()["feeds_done"], where
    flat = dict(got, dev=got["dev"].reshape(-1), strikes=got["strikes"].reshape(-1), out=got["out"].reshape(-1))
    same_words(flat, want, where)
    return got


def feed_all(sess, audio, tables, frame0, strikes, out, after=None):
    """The whole recording into both microphones, cut differently; after every feed the words equal the model's."""
    pos, k, feeds, log = [0, 0], 0, 0, []
    while min(pos) < len(audio):
        bufs = []
        for mic in range(2):
            n = min(CUTS[mic][k % len(CUTS[mic])], len(audio) - pos[mic])
            bufs.append(audio[pos[mic]:pos[mic] + n])
            pos[mic] += n
        k += 1
        sess.feed(bufs)
        feeds += 1
        early = sess.consensus()["feeds_done"]                       # non-blocking: whatever it shows is a whole feed's
        assert 0 <= early <= feeds
        sess.sync()
        want = live_model(sess, tables, frame0, strikes, out)
        got = check_live(sess, want, feeds, feeds)
        log.append((list(pos), got))
        if after is not None:
            feeds += after(feeds, got) or 0
    return log


def test_live_consensus_flags_the_member_that_cannot_follow(chopin_audio, otw_golden):
    from real_time_audio_sync_amd.annotate import AnnotationTables
    from real_time_audio_sync_amd.ensemble import EnsembleSession
    ref, own = otw_golden["G/ref"], otw_golden["G/live"]
    rev = np.ascontiguousarray(ref[:, ::-1])                        # the same columns backwards: nothing to follow
    host = [evaluate.read_ground_truth(REF_CSV), evaluate.read_ground_truth(LIVE_CSV), evaluate.read_ground_truth(REF_CSV)]
    tab = AnnotationTables([REF_CSV, LIVE_CSV, REF_CSV], device=DEV)
    sess = EnsembleSession([ref, own, rev], tab, 2, max_dev=MAX_DEV, patience=PATIENCE, c=C, max_run_count=3, device=DEV)
    try:
        assert sess.B == 6 and sess.consensus()["feeds_done"] == 0 and np.isnan(sess.consensus()["consensus"]).all()
        log = feed_all(sess, chopin_audio["live"], host, [0] * 6, [0] * 6, [0] * 6)
        assert len(log) > 40
        last = log[-1][1]
        assert same_bytes(last["consensus"][:1], last["consensus"][1:]) and np.isfinite(last["consensus"]).all()
        assert same_bytes(last["dev"][0], last["dev"][1])            # feed cuts do not matter
        # The member that cannot follow is flagged, and no other ever is.  With max_dev = 2.0 and patience = 4 the numpy
        # restatement of the reference tracker (oracle/otw_numpy.py, run on the CPU over these three references with
        # these cuts) has member 2 out from 438 000 samples (feed 22 of microphone 0, feed 25 of microphone 1) to
        # 744 000 / 732 000, and members 0 and 1 never.  It does not stay out to the very end at any max_dev that spares
        # the other two: an online tracker's reference index only moves forward, so in the last bars the reversed
        # member's index reaches the end of its reference like everyone's, its beat coincides with theirs by
        # construction, and after one feed within max_dev it is heard again (oracle: from feed 40 of 42).  So the flag
        # is asserted where the oracle has it, between 450 000 and 720 000 samples of each microphone.
        for mic in range(2):
            window = [got["out"][mic].tolist() for pos, got in log if 450000 <= pos[mic] <= 720000]
            assert len(window) >= 8 and all(o == [0, 0, 1] for o in window), (mic, window)
            assert not any(got["out"][mic][:2].any() for _, got in log), mic
            assert all(got["n_in"][mic] == 2 for pos, got in log if 520000 <= pos[mic] <= 720000)
    finally:
        sess.close()
        tab.close()


def test_heal_puts_a_lost_member_back(chopin_audio, otw_golden):
    """G = 3 with the `ref` chroma twice.  After feed 20 member 2 of microphone 0 is restarted at frame 0 of its recording,
    some 190 frames behind the music; `patience` feeds later it is out, heal(back=10) restarts it 10 frames before the
    consensus, and it follows to the end.  Offset and `back` were chosen with oracle/otw_numpy.py on the CPU: there the
    member is out at feed 24, heal gives frame 202, and its |dev| stays below 0.3 beats from three feeds after the heal to
    the end (0.0 at the end), well inside max_dev = 2.0."""
    from real_time_audio_sync_amd import ensemble
    from real_time_audio_sync_amd.annotate import AnnotationTables
    ref, own = otw_golden["G/ref"], otw_golden["G/live"]
    host = [evaluate.read_ground_truth(REF_CSV), evaluate.read_ground_truth(LIVE_CSV), evaluate.read_ground_truth(REF_CSV)]
    tab = AnnotationTables([REF_CSV, LIVE_CSV, REF_CSV], device=DEV)
    ref_again = ref.copy()                                           # a recording of its own to the session
    sess = ensemble.EnsembleSession([ref, own, ref_again], tab, 2, max_dev=MAX_DEV, patience=PATIENCE, c=C, max_run_count=3,
                                    device=DEV)
    WRONG, BACK, LOST = 0, 10, 2
    frame0, strikes, out = [0] * 6, [0] * 6, [0] * 6
    story = {}

    def after(feeds, got):
        if feeds == 20:
            sess.live.restart([LOST], offsets=[WRONG])
            frame0[LOST], strikes[LOST], out[LOST] = WRONG, 0, 0
            sess.sync()
            now = sess.consensus()
            assert now["strikes"][0].tolist() == [0, 0, 0] and np.isnan(now["dev"][0][LOST])   # republished NaN / 0 / 0
            assert same_bytes(now["dev"][1], got["dev"][1]) and same_bytes(now["consensus"], got["consensus"])
        if 20 < feeds < 20 + PATIENCE:
            assert got["out"][0][LOST] == 0 and got["strikes"][0][LOST] == feeds - 20
        if feeds == 20 + PATIENCE:
            assert got["out"].reshape(-1).tolist() == [0, 0, 1, 0, 0, 0]
            c = got["consensus"][0]
            want = min(max(ensemble.frames_of_beat(host[2], c, FS) - BACK, 0), ref.shape[1] - 1)
            assert want == min(max(em.invert(float(c), host[2][0], host[2][1], FS) - BACK, 0), ref.shape[1] - 1)
            moved = sess.heal(back=BACK)
            assert moved == {LOST: want} and 150 < want < 260
            frame0[LOST], strikes[LOST], out[LOST] = want, 0, 0
            story["healed"] = want
        if feeds == 21 + PATIENCE:
            assert got["strikes"][0][LOST] == 0 and got["out"][0][LOST] == 0
        return 0

    try:
        log = feed_all(sess, chopin_audio["live"], host, frame0, strikes, out, after)
        assert "healed" in story
        last = log[-1][1]
        assert abs(last["dev"][0][LOST]) <= MAX_DEV and last["out"].reshape(-1).tolist() == [0] * 6
        assert sess.heal(back=BACK) == {}                            # nobody is out: nothing moves
        beats = sess.live.beats()                                    # the inner session is the ordinary one
        assert beats["ref_frame"][LOST] == story["healed"] + int(sess.live.path(LOST)[-1][1])
    finally:
        sess.close()
        tab.close()


# ---- 6. a session without the feature --------------------------------------------------------------------------------------

L, HOP, RATE = 512, 128, 22050


def small_session(kind):
    from real_time_audio_sync_amd.live import LiveSession
    ref = synth.synth_ref(120, seed=60)
    wtw = {'dtw_win_size': 8 * HOP, 'dtw_hop_size': 4 * HOP} if kind == "wtw" else None
    return LiveSession(ref, batch=3, c=10, max_run_count=3, fft_len=L, hop_size=HOP, fs=RATE, max_pending=1 << 14,
                       wtw_params=wtw, device=DEV)


@pytest.mark.parametrize("kind", ["otw", "wtw"])
def test_a_session_that_never_follows_consensus_is_unaffected(kind):
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.annotate import AnnotationTables
    rs = np.random.RandomState(9)
    t = np.arange(int(1.2 * RATE)) / float(RATE)
    audio = []
    for b in range(3):
        x = 0.05 * rs.randn(len(t))
        for k in range(4):
            x += 0.2 * np.sin(2 * np.pi * (220.0 * 2 ** ((3 * k + b + 2 * t) / 12.0)) * t)
        audio.append(x.astype(np.float32))
    sizes = [(1500, 900, 2100), (513, 0, 1300), (128, 1407, 1), (2000, 700, 1999)]
    table = evaluate.read_ground_truth(REF_CSV)
    tab = AnnotationTables([REF_CSV], device=DEV)
    sess, plain = small_session(kind), small_session(kind)
    try:
        with pytest.raises(nat.RtsyncError, match="before any rts_live_annotate"):
            sess.follow_consensus([0, 0, 0])
        sess.annotate(tab)
        plain.annotate(tab)
        with pytest.raises(nat.RtsyncError, match="before any rts_live_follow_consensus"):
            plain.consensus()
        assert nat.lib.rts_live_consensus(plain._h, None, None, None, None, None, None, None, None) == -1
        with pytest.raises(nat.RtsyncError, match="B = 2"):
            sess.follow_consensus([0, 0])
        sess.follow_consensus([0, -1, 0], max_dev=0.05, patience=2)
        groups, strikes, out = [0, -1, 0], [0] * 3, [0] * 3
        pos, ppos, feeds = [0] * 3, [0] * 3, 0

        def feed(s, p, i):
            s.feed([audio[b][p[b]:p[b] + n] for b, n in enumerate(sizes[i % 4])])
            for b, n in enumerate(sizes[i % 4]):
                p[b] += n

        for i in range(8):
            feed(sess, pos, i)
            feed(plain, ppos, i)
            feeds += 1
            sess.sync()
            want = model_step(sess.otw or sess.wtw, groups, [table], [0] * 3, [0] * 3, strikes, out, 0.05, 2)
            got = sess.consensus()
            assert got["feeds_done"] == feeds
            same_words(got, want, i)
        assert np.isfinite(got["consensus"]).all() and np.isnan(got["dev"][1])
        plain.sync()
        for b in range(3):
            assert np.array_equal(sess.path(b), plain.path(b)), b
        assert np.array_equal((sess.otw or sess.wtw).states(), (plain.otw or plain.wtw).states())
        mine, theirs = sess.beats(), plain.beats()
        for key in ("beat", "label", "ref_frame"):
            assert same_bytes(mine[key], theirs[key]), key
        # annotations off: the launch is skipped and the words stay
        sess.annotate(None)
        kept = sess.consensus()
        feed(sess, pos, 0)
        feeds += 1
        sess.sync()
        later = sess.consensus()
        assert later["feeds_done"] == feeds
        for key in ("consensus", "spread", "dev", "n_in", "n_valid", "strikes", "out"):
            assert same_bytes(later[key], kept[key]), key
        # reset: NaN / NaN / 0 / 0 per group, NaN / 0 / 0 per stream, and the carried state is zero again
        sess.annotate(tab)
        sess.reset()
        sess.sync()
        cleared = sess.consensus()
        assert np.isnan(cleared["consensus"]).all() and np.isnan(cleared["spread"]).all() and np.isnan(cleared["dev"]).all()
        assert not cleared["n_in"].any() and not cleared["n_valid"].any() and not cleared["strikes"].any() and not cleared["out"].any()
        strikes, out = [0] * 3, [0] * 3
        sess.feed([a[:1500] for a in audio])
        sess.sync()
        want = model_step(sess.otw or sess.wtw, groups, [table], [0] * 3, [0] * 3, strikes, out, 0.05, 2)
        same_words(sess.consensus(), want, "after the reset")
        # consensus off: the words stay
        sess.follow_consensus(None)
        kept = sess.consensus()
        sess.feed([a[1500:3000] for a in audio])
        sess.sync()
        for key in ("consensus", "dev", "strikes"):
            assert same_bytes(sess.consensus()[key], kept[key]), key
    finally:
        sess.close()
        plain.close()
        tab.close()
