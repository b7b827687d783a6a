"""The tuning estimator on the device (csrc/tuning.hip) against its numpy model (tests/tuning_model.py), `==` on every
histogram bin and bit for bit on every pick; the tuned chroma chain through ChromaPlan, the file entry points, LiveSession and
WTW.  Caller-owned outputs of the new entry points lie in guarded buffers (tests/guarded.py)."""
import ctypes
import struct
import wave

import numpy as np
import pytest

import tuning_model as tm
from guarded import guarded, same_bytes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FS = tm.FS
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def mods():
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd import chroma, filters
    return chroma, filters, nat


# ---- crafted STFTs ------------------------------------------------------------------------------------------------------

class Handle(object):
    """rts_tuning_* with a table of the test's own making."""

    def __init__(self, nat, fft_len, k_lo, k_hi, R, E, bin_hz, thr_pow):
        self.nat, self.R, self.E = nat, R, np.ascontiguousarray(E, dtype=np.float64)
        self.args = (k_lo, k_hi, self.E, R, bin_hz, thr_pow)
        self.h = ctypes.c_void_p()
        nat.check(nat.lib.rts_tuning_create(fft_len, k_lo, k_hi, R, len(self.E), self.E.ctypes.data, bin_hz, thr_pow,
                                            ctypes.byref(self.h)))

    def accumulate(self, stft, seg, S, hist):
        st = torch.view_as_real(stft).contiguous() if stft.is_complex() else stft
        self.nat.check(self.nat.lib.rts_tuning_accumulate(self.h, st.data_ptr() if st.shape[0] else None, st.shape[0],
                                                          seg.data_ptr() if seg is not None else None, S, hist.data_ptr(), None))
        torch.cuda.synchronize()

    def model(self, stft, seg=None, S=1):
        k_lo, k_hi, E, R, bin_hz, thr_pow = self.args
        return tm.histogram(stft, k_lo, k_hi, E, R, bin_hz, thr_pow, seg=seg, S=S)

    def close(self):
        self.nat.lib.rts_tuning_destroy(self.h)


def crafted(fft_len, M, k_lo, k_hi, bin_hz, seed):
    """[M][n_bins] complex128 made to hit the rules: components quantised to seven levels (so equal neighbours, plateaus
    and P[k] == P[k-1] non-peaks abound, beside plenty of peaks), frame 1 all zero, frame 2 one bin at k_lo and one at
    k_hi, frame 3 a symmetric peak -- a == c, so d == 0 and f == k * bin_hz exactly, an edge of the custom table."""
    n_bins = fft_len // 2 + 1
    rs = np.random.RandomState(seed)
    x = (rs.randint(-3, 4, (M, n_bins)) + 1j * rs.randint(-3, 4, (M, n_bins))).astype(np.complex128)
    x *= rs.choice([1.0, 0.25, 1e-3], (M, 1))                       # the threshold is relative to the frame's own maximum
    x[::5, rs.randint(0, n_bins, 3)] *= 4.0                         # a few bins far above the rest: most others fall below lim
    x[1] = 0.0
    x[2] = 0.0
    x[2, k_lo] = 3.0 - 1.0j
    x[2, k_hi] = 0.5j
    k_edge = (k_lo + k_hi) // 2
    x[3] = 0.0
    x[3, k_edge - 1:k_edge + 2] = [1.0 + 1.0j, 3.0, -1.0 - 1.0j]
    return x, k_edge


PARAMS = [(64, 37), (1024, 37), (4096, 37), (8192, 5)]


@pytest.fixture(scope="module", params=PARAMS, ids=["fft%d-M%d" % p for p in PARAMS])
def crafted_case(request, mods):
    chroma, filters, nat = mods
    fft_len, M = request.param
    kw = dict(f_min=0.0, f_max=1e9) if fft_len == 64 else {}
    k_lo, k_hi, E = filters.tuning_edges(FS, fft_len, **kw)
    if fft_len == 64:
        assert (k_lo, k_hi) == (1, 31)
    bin_hz = float(FS) / fft_len
    x, k_edge = crafted(fft_len, M, k_lo, k_hi, bin_hz, seed=fft_len)
    E = np.unique(np.concatenate([E, [k_edge * bin_hz]]))           # the symmetric peak of frame 3 lies exactly on an edge
    n_edge = int(np.searchsorted(E, k_edge * bin_hz, "left"))
    assert E[n_edge] == k_edge * bin_hz
    h = Handle(nat, fft_len, k_lo, k_hi, 100, E, bin_hz, 0.01)
    dev = torch.from_numpy(x).to(DEV)
    yield h, x, dev, n_edge
    h.close()


def test_histogram_equals_the_model_on_crafted_frames(crafted_case):
    h, x, dev, n_edge = crafted_case
    want = h.model(x)
    hist, check = guarded((1, h.R), torch.int64, DEV, 0x00)
    h.accumulate(dev, None, 1, hist)
    check("hist_dev")
    got = hist.cpu().numpy().view(np.uint64)
    print("peaks counted: %d in %d frames" % (want.sum(), x.shape[0]))
    assert want.sum() > x.shape[0]
    assert (got == want).all()
    # the special frames one by one, so each rule is seen to act: nothing, two peaks, one peak in the bin its edge opens
    for m, n_peaks in ((1, 0), (2, 2), (3, 1)):
        one, chk = guarded((1, h.R), torch.int64, DEV, 0x00)
        h.accumulate(dev[m:m + 1], None, 1, one)
        chk("hist_dev")
        one = one.cpu().numpy().view(np.uint64)
        assert (one == h.model(x[m:m + 1])).all() and one.sum() == n_peaks, m
        if m == 3:
            assert one[0, n_edge % h.R] == 1


def test_histogram_by_segments(crafted_case):
    h, x, dev, _ = crafted_case
    M = x.shape[0]
    lengths = [0, 1, 19, 17] if M == 37 else [0, 1, 2, 2]           # segment 0 stays empty; workgroups own 3-4 frames each,
    seg = np.repeat(np.arange(4), lengths).astype(np.int32)         # so their ranges cross the boundaries at 1 and 20
    assert len(seg) == M
    want = h.model(x, seg=seg, S=4)
    hist, check = guarded((4, h.R), torch.int64, DEV, 0x00)
    h.accumulate(dev, torch.from_numpy(seg).to(DEV), 4, hist)
    check("hist_dev")
    got = hist.cpu().numpy().view(np.uint64)
    assert (got == want).all() and got[0].sum() == 0 and (got[2:].sum(axis=1) > 0).all()
    # values outside [0, S) count nowhere; the rows of the others are unchanged
    bad = seg.copy()
    bad[seg == 2] = np.where(np.arange(lengths[2]) % 2 == 0, -1, 4)
    bad[-1] = np.iinfo(np.int32).max
    bad[-2] = np.iinfo(np.int32).min
    want = h.model(x, seg=bad, S=4)
    hist, check = guarded((4, h.R), torch.int64, DEV, 0x00)
    h.accumulate(dev, torch.from_numpy(bad).to(DEV), 4, hist)
    check("hist_dev")
    got = hist.cpu().numpy().view(np.uint64)
    assert (got == want).all() and got[2].sum() == 0 and got[3].sum() < h.model(x, seg=seg, S=4)[3].sum()


def test_histogram_accumulates(crafted_case):
    h, x, dev, _ = crafted_case
    M = x.shape[0]
    cuts = [0, 1, 21, 37] if M == 37 else [0, 1, 3, 5]
    whole, c0 = guarded((1, h.R), torch.int64, DEV, 0x00)
    parts, c1 = guarded((1, h.R), torch.int64, DEV, 0x00)
    h.accumulate(dev, None, 1, whole)
    for a, b in zip(cuts[:-1], cuts[1:]):
        h.accumulate(dev[a:b].contiguous(), None, 1, parts)
    h.accumulate(dev[:0], None, 1, parts)                           # n_frames == 0: a no-op
    c0("hist_dev")
    c1("hist_dev")
    assert same_bytes(whole.cpu().numpy(), parts.cpu().numpy()) and whole.sum() > 0
    pre = np.random.RandomState(1).randint(0, 1 << 40, (1, h.R)).astype(np.int64)
    filled, c2 = guarded((1, h.R), torch.int64, DEV, 0x55)
    filled.copy_(torch.from_numpy(pre))
    h.accumulate(dev, None, 1, filled)
    c2("hist_dev")
    assert (filled.cpu().numpy() == pre + whole.cpu().numpy()).all()


# ---- the pick -----------------------------------------------------------------------------------------------------------

def test_pick_equals_the_model(mods):
    chroma, filters, nat = mods
    cases = tm.pick_cases()
    for R in sorted(set(len(h) for _, h, _ in cases)):
        plan = chroma.TuningPlan(R=R)
        for W in sorted(set(W for _, h, W in cases if len(h) == R)):
            rows = [(name, h) for name, h, w in cases if len(h) == R and w == W]
            S = len(rows)
            hist = torch.from_numpy(np.array([[v for v in h] for _, h in rows], dtype=np.uint64).view(np.int64)).to(DEV)
            cents, c0 = guarded((S,), torch.float64, DEV, 0xFF)
            n, c1 = guarded((S,), torch.int64, DEV, 0x55)
            nat.check(nat.lib.rts_tuning_pick(plan._h, hist.data_ptr(), S, W, cents.data_ptr(), n.data_ptr(), None))
            torch.cuda.synchronize()
            c0("cents_dev")
            c1("n_dev")
            for s, (name, h) in enumerate(rows):
                want_c, want_n = tm.pick(h, W)
                assert struct.pack("<d", float(cents[s])) == struct.pack("<d", want_c), (name, float(cents[s]), want_c)
                assert int(n[s]) == want_n, name
            # and through the wrapper
            c2, n2 = plan.pick(hist, W)
            assert same_bytes(c2.cpu().numpy(), cents.cpu().numpy()) and same_bytes(n2.cpu().numpy(), n.cpu().numpy())
        for W in (-1, (R - 1) // 2 + 1):
            with pytest.raises(nat.RtsyncError, match="W must be"):
                plan.pick(torch.zeros((1, R), dtype=torch.int64, device=DEV), W)
        plan.close()


# ---- end to end on the device's own STFT --------------------------------------------------------------------------------

OFFSETS = (-50.0, -37.0, 0.0, 25.0, 49.5)


def test_batch_estimate_on_the_devices_own_stft(mods):
    chroma, filters, nat = mods
    xs = [tm.source(c, seconds=2.0) for c in OFFSETS]
    cents, n = chroma.estimate_tuning_batch(xs)
    assert cents.shape == n.shape == (len(OFFSETS),) and cents.dtype == np.float64 and n.dtype == np.int64
    plan, tuner = chroma._plan(), chroma._tuner()
    for b, (x, truth) in enumerate(zip(xs, OFFSETS)):
        _, stft = plan.frames(torch.from_numpy(x).to(plan.device), pad_left=chroma.fft_len // 2, want_stft=True, want_chroma=False)
        assert stft.shape == (21, 2049)
        hist = tuner.histogram(tuner.accumulate(stft))
        want = tm.histogram(stft.cpu().numpy(), tuner.k_lo, tuner.k_hi, tuner.edges, tuner.R, tuner.bin_hz, tuner.thr_pow)
        assert (hist.view(np.uint64) == want).all(), truth
        want_c, want_n = tm.pick(want[0])
        print("truth %+.1f: estimate %+.1f from %d peaks" % (truth, cents[b], n[b]))
        assert (cents[b], n[b]) == (want_c, want_n) and want_n > 200
        assert tm.circular_error(cents[b], truth) <= 1.0            # one histogram bin
        assert chroma.estimate_tuning(x) == (want_c, want_n)


def test_chunked_estimate_equals_the_whole(mods):
    chroma, filters, nat = mods
    x = tm.source(-37.0)                                            # 6 s: 65 frames, 9 chunks of 8
    whole = chroma.estimate_tuning(x, chunk_frames=2048)
    assert chroma.estimate_tuning(x, chunk_frames=8) == whole
    assert chroma.estimate_tuning(x, chunk_frames=1) == whole
    assert whole[1] > 800 and tm.circular_error(whole[0], -37.0) <= 1.0
    # at another rate: resampled on the device first, like the file entry points
    assert tm.circular_error(chroma.estimate_tuning(tm.source(25.0, seconds=2.0, fs=44100), fs_in=44100)[0], 25.0) <= 1.0
    # PCM16 and other dtypes, arrays and tensors: converted like the resampler converts them, never read as float32
    pcm = np.round(x.astype(np.float64) * 32767.0).astype(np.int16)
    as_float = pcm.astype(np.float32) / np.float32(32768.0)
    want = chroma.estimate_tuning(as_float)
    assert tm.circular_error(want[0], -37.0) <= 1.0
    for given in (pcm, torch.from_numpy(pcm), torch.from_numpy(pcm).to(DEV), as_float.astype(np.float64),
                  torch.from_numpy(as_float).to(DEV)):
        assert chroma.estimate_tuning(given) == want
    with pytest.raises(ValueError):
        chroma.estimate_tuning(x, chunk_frames=0)
    with pytest.raises(ValueError):
        chroma.ChromaPlan(tuning=float("nan"))
    assert chroma.estimate_tuning(np.zeros(3 * 4096, dtype=np.float32)) == (0.0, 0)
    assert chroma.estimate_tuning(np.zeros(100, dtype=np.float32)) == (0.0, 0)      # no frame at all


def test_handle_belongs_to_its_device(mods):
    chroma, filters, nat = mods
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    tuner = chroma._tuner()
    hist = torch.zeros((1, tuner.R), dtype=torch.int64, device="cuda:1")
    x = torch.zeros((1, tuner.n_bins, 2), dtype=torch.float64, device="cuda:1")
    with torch.cuda.device(1):
        rc = nat.lib.rts_tuning_accumulate(tuner._h, x.data_ptr(), 1, None, 1, hist.data_ptr(), None)
        assert rc == -1 and b"device" in nat.lib.rts_last_error()
        rc = nat.lib.rts_tuning_pick(tuner._h, hist.data_ptr(), 1, 5, x.data_ptr(), hist.data_ptr(), None)
        assert rc == -1 and b"device" in nat.lib.rts_last_error()


# ---- tuned chroma -------------------------------------------------------------------------------------------------------

def test_tuned_plan_against_the_oracle(mods):
    from oracle import chroma_oracle as co
    from test_chroma_gpu import CHROMA_ATOL
    chroma, filters, nat = mods
    x = tm.source(-40.0, seconds=2.0)
    fb = co.chroma_filterbank(a440=filters.tuning_a440(-40.0))
    want = co.l2_normalize_columns(np.dot(fb, np.abs(co.create_stft(x)) ** 2))
    plan = chroma.ChromaPlan(tuning=-40.0)
    assert plan.tuning == -40.0 and same_bytes(plan.chromafb, filters.chroma_filterbank(FS, 4096, a440=filters.tuning_a440(-40.0)))
    dev = torch.from_numpy(x).to(plan.device)
    got, _ = plan.frames(dev, pad_left=2048)
    assert np.abs(got.t().cpu().numpy() - want).max() <= CHROMA_ATOL
    plain_plan = chroma.ChromaPlan()
    plain, _ = plain_plan.frames(dev, pad_left=2048)
    assert np.abs(plain.t().cpu().numpy() - want).max() > 1e-3      # the table did change
    # frames_batch, un-padded framing, two buffers of different lengths
    lens = [len(x), len(x) - 5000]
    buf = torch.zeros((2, len(x)), dtype=torch.float32, device=plan.device)
    buf[0], buf[1, :lens[1]] = dev, dev[5000:]
    nf = [(n - 4096) // 2048 + 1 for n in lens]
    out = plan.frames_batch(buf, torch.tensor(lens, dtype=torch.int32, device=plan.device),
                            torch.tensor(nf, dtype=torch.int32, device=plan.device), max(nf))
    for b, start in enumerate((0, 5000)):
        cols = co.l2_normalize_columns(np.dot(fb, np.abs(np.stack(
            [np.fft.rfft(x[start + m * 2048:start + m * 2048 + 4096].astype(np.float64) * np.hanning(4096)) for m in range(nf[b])]).T) ** 2))
        assert np.abs(out[b, :nf[b]].t().cpu().numpy() - cols).max() <= CHROMA_ATOL, b
    # tuning=None is the plan of before, byte for byte
    none_plan = chroma.ChromaPlan(tuning=None)
    assert none_plan.tuning is None and plain_plan.tuning is None
    assert same_bytes(none_plan.chromafb, plain_plan.chromafb) and same_bytes(none_plan.chromafb, filters.chroma_filterbank(FS, 4096))
    assert same_bytes(none_plan.frames(dev, pad_left=2048)[0].cpu().numpy(), plain.cpu().numpy())
    assert chroma._plan(tuning=None) is chroma._plan() and chroma._plan(tuning=-40.0) is not chroma._plan()
    assert chroma._plan(tuning=-40.0) is chroma._plan(tuning=-40)
    col = chroma.wav_to_chroma_col(x[:4096], tuning=-40.0)
    spec = np.abs(np.fft.rfft(x[:4096].astype(np.float64) * np.hanning(4096))) ** 2
    assert np.abs(col - co.l2_normalize_columns(np.dot(fb, spec)[:, None])[:, 0]).max() <= CHROMA_ATOL
    assert same_bytes(chroma.wav_to_chroma_col(x[:4096], tuning=None), chroma.wav_to_chroma_col(x[:4096]))
    for p in (plan, plain_plan, none_plan):
        p.close()


def write_wav(path, x, fs=FS):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.round(np.asarray(x, dtype=np.float64) * 32767.0).astype("<i2").tobytes())


def test_what_tuning_buys(mods, tmp_path):
    """The same notes in tune and 40 cents flat, as files: mean cosine per frame between their chroma, with the filterbank
    for 440 Hz and with tuning="auto".  tests/test_tuning_cpu.py clears both bounds through the numpy chain first."""
    chroma, filters, nat = mods
    in_tune, flat = tmp_path / "in_tune.wav", tmp_path / "flat.wav"
    write_wav(in_tune, tm.source(0.0))
    write_wav(flat, tm.source(-40.0))

    def mean_cos(a, b):
        assert a.shape == b.shape and a.shape[0] == 12
        return float((a * b).sum(axis=0).mean())

    plain = mean_cos(chroma.wav_to_chroma(str(in_tune)), chroma.wav_to_chroma(str(flat)))
    auto = mean_cos(chroma.wav_to_chroma(str(in_tune), tuning="auto"), chroma.wav_to_chroma(str(flat), tuning="auto"))
    print("mean cosine: untuned %.4f, tuning='auto' %.4f" % (plain, auto))
    assert auto >= 0.99
    assert plain <= 0.96
    assert same_bytes(chroma.wav_to_chroma(str(flat), tuning=None), chroma.wav_to_chroma(str(flat)))
    est = chroma.estimate_tuning(str(flat))[0]
    assert tm.circular_error(est, -40.0) <= 1.0
    assert same_bytes(chroma.wav_to_chroma(str(flat), tuning="auto"), chroma.wav_to_chroma(str(flat), tuning=est))
    d = chroma.wav_to_chroma_diff(str(flat), tuning="auto")
    assert same_bytes(d, np.clip(np.diff(chroma.wav_to_chroma(str(flat), tuning=est)), 0, np.inf))
    assert same_bytes(chroma.wav_to_chroma_diff(str(flat), tuning=None), chroma.wav_to_chroma_diff(str(flat)))
    with pytest.raises(ValueError):
        chroma.wav_to_chroma(str(flat), tuning="automatic")


# ---- live and WTW -------------------------------------------------------------------------------------------------------

def test_live_session_with_tuning(mods):
    from real_time_audio_sync_amd.live import LiveSession
    chroma, filters, nat = mods
    L, H, B = 4096, 2048, 3
    x = tm.source(25.0)
    plan = chroma.ChromaPlan(tuning=25.0)
    ref = plan.frames(torch.from_numpy(x).to(plan.device), pad_left=L // 2)[0].t().contiguous().cpu().numpy()
    live = [x[1000 * b:1000 * b + 60000 + 777 * b] for b in range(B)]
    sess = LiveSession(ref, batch=B, c=20, tuning=25.0)
    plain = LiveSession(ref, batch=B, c=20)
    try:
        assert sess.tuning == 25.0 and plain.tuning is None and sess.plan.tuning == 25.0
        assert same_bytes(sess.plan.chromafb, plan.chromafb)
        rs = np.random.RandomState(2)
        pos, got, got_plain = [0] * B, [[] for _ in range(B)], [[] for _ in range(B)]
        while any(pos[b] < len(live[b]) for b in range(B)):
            bufs = []
            for b in range(B):
                n = min(int(rs.choice([0, 1, 700, 2048, 4096, 5001, 9000])), len(live[b]) - pos[b])
                bufs.append(live[b][pos[b]:pos[b] + n])
                pos[b] += n
            for s, acc in ((sess, got), (plain, got_plain)):
                s.feed(bufs, wait=True)
                cols, n_cols = s.last_columns()
                for b in range(B):
                    acc[b].append(cols[b, :int(n_cols[b])].cpu().numpy())
        lens = [len(v) for v in live]
        nf = [(n - L) // H + 1 for n in lens]
        buf = torch.zeros((B, max(lens)), dtype=torch.float32, device=plan.device)
        for b in range(B):
            buf[b, :lens[b]] = torch.from_numpy(live[b])
        want = plan.frames_batch(buf, torch.tensor(lens, dtype=torch.int32, device=plan.device),
                                 torch.tensor(nf, dtype=torch.int32, device=plan.device), max(nf)).cpu().numpy()
        untuned = chroma._plan().frames_batch(buf, torch.tensor(lens, dtype=torch.int32, device=plan.device),
                                              torch.tensor(nf, dtype=torch.int32, device=plan.device), max(nf)).cpu().numpy()
        for b in range(B):
            mine = np.concatenate(got[b])
            assert mine.shape == (nf[b], 12) and nf[b] >= 28
            assert same_bytes(mine, np.ascontiguousarray(want[b, :nf[b]])), b
            assert same_bytes(np.concatenate(got_plain[b]), np.ascontiguousarray(untuned[b, :nf[b]])), b
            assert not same_bytes(mine, np.concatenate(got_plain[b]))
    finally:
        sess.close()
        plain.close()
        plan.close()


def test_wtw_with_tuning(mods):
    from real_time_audio_sync_amd.wtw import WTW
    chroma, filters, nat = mods
    x = tm.source(25.0, seconds=3.0)
    params = dict(fft_len=4096, hop_size=2048, dtw_win_size=2048 * 8, dtw_hop_size=2048 * 4)
    w = WTW.from_samples(x, params, tuning=25.0)
    plan = chroma.ChromaPlan(tuning=25.0)
    want = plan.frames(torch.from_numpy(x).to(plan.device), pad_left=2048)[0].t().contiguous().cpu().numpy()
    assert w.tuning == 25.0 and same_bytes(w.chromafb, plan.chromafb) and same_bytes(w.chroma_ref, want)
    w0 = WTW.from_samples(x, params)
    assert w0.tuning is None and same_bytes(w0.chromafb, filters.chroma_filterbank(FS, 4096))
    assert not same_bytes(w0.chroma_ref, want)
    assert w.insert(list(x[:3 * 4096].astype(np.float64))) is None and w.chroma_ptr >= 1   # the inserted buffers take the same plan
    plan.close()
