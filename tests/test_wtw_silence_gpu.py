"""NaN costs on the WTW kernels: digital silence (tests/silence_inputs.py::wtw_silence_case).

wtw.py:169 divides by the column norms, so an all-zero live frame makes a NaN row of costs and an all-zero reference
frame a NaN column; wtw.py:201-215 then keeps a NaN that sits in (i-1, j) and ignores one in (i, j-1) or (i-1, j-1).
The kernels restate that with a minimum that ignores NaN plus one select (``WtwPolicy::cell``, csrc/sdp.h).  Here NaN
reaches every kernel that runs it: the one- and two-wave window kernel with its prefetch across the windows of one push,
the strip DP in its one-, two-, three- and many-strip forms with the hand-off between strips through HBM (whose "not yet
written" sentinel is itself a NaN pattern), and the separate backtrack kernels from 13 strips on -- with silent rows and
columns at 0, at the last index, on both sides of the 64-row wave and 128-row strip boundaries, as runs longer than a
window, partly and wholly NaN windows (tests/test_silence_cpu.py pins how many of each).

Each case must equal ``WtwOracle``: path, live_ptr / ref_ptr / status / windows of every stream, and the last window's D
(NaN positions included; an x86 0/0 is a negative NaN and the GPU's a positive one, so NaN bytes are never compared)."""
import numpy as np
import pytest

import silence_inputs as si

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = si.wtw_cases()
SMALL = sorted(n for n, kw in CASES.items() if kw["W"] <= 128)
STRIPS = sorted(n for n, kw in CASES.items() if kw["W"] > 128)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(params=["win", "win_two_waves", "strip_65_128"])
def wtw_path(request, monkeypatch):
    """The three settings of tests/test_wtw_gpu.py: windows of at most 128 frames on wtw_win_kernel; of at most 65 on
    its two-wave form as well (RTS_WIN_FORCE_R2); of 65 to 128 on the strip DP's one- and two-strip forms
    (RTS_WTW_WIN=0)."""
    if request.param == "strip_65_128":
        monkeypatch.setenv("RTS_WTW_WIN", "0")
    if request.param == "win_two_waves":
        monkeypatch.setenv("RTS_WIN_FORCE_R2", "1")
    return request.param


_inputs = {}


def _case(name):
    """(ref, lives, per-stream oracle records) of one case, computed once and shared by every test that uses it."""
    if name not in _inputs:
        _inputs[name] = si.wtw_silence_case(**CASES[name])
    return _inputs[name]


def _heard_at_a_partly_nan_d(name):
    """The number of live frames after which the last window stream 0 has run left a D that is NaN in part (the last
    such window of the stream): an all-NaN D and a NaN-free one say little about where the NaNs belong."""
    ref, lives, recs = _case(name)
    W = CASES[name]["W"]
    for lp, rp, share in reversed(recs[0]["windows"]):
        if share > 0:
            D = _last_d(ref, lives[0], dict(windows=[(lp, rp, share)]), W)
            if np.isnan(D).any() and not np.isnan(D).all():
                return lp + W
    raise AssertionError("no partly NaN D in " + name)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda:0")


def _push(eng, lives, chunk=None, start=0, stop=None):
    """Frames start..stop of every stream in one push (many windows in one launch), or in chunks of ``chunk`` frames."""
    tmax = max(l.shape[1] for l in lives)
    cols = np.zeros((len(lives), tmax, 12))
    for b, l in enumerate(lives):
        cols[b, : l.shape[1]] = l.T
    n = torch.tensor([l.shape[1] for l in lives], dtype=torch.int32, device="cuda:0")
    stop = tmax if stop is None else min(stop, tmax)
    n = torch.clamp(n, max=stop)
    step = chunk or max(stop - start, 1)
    for a in range(start, stop, step):
        # precheck=False: wtw.py:76's per-call check belongs to the drop-in, the oracle here pushes column by column
        k = min(step, stop - a)
        eng.push(torch.from_numpy(cols[:, a: a + k].copy()).to("cuda:0"), torch.clamp(n - a, min=0, max=k), precheck=False)


def _same(eng, recs, tag):
    for b, r in enumerate(recs):
        st = eng.state(b)
        assert np.array_equal(eng.path(b), r["path"]), (tag, b)
        assert (st["live_ptr"], st["ref_ptr"], st["status"], st["windows"]) == (
            r["live_ptr"], r["ref_ptr"], r["status"], len(r["windows"])), (tag, b)


def _last_d(ref, live, rec, W, heard=None):
    """D of the last window the oracle ran (of those it ran on the first ``heard`` frames), from the (live_ptr, ref_ptr)
    its record holds (tests/silence_inputs.py::wtw_last_d, which tests/sdp_soak.py uses too)."""
    D, known = si.wtw_last_d(ref, live, [w for w in rec["windows"] if heard is None or w[0] + W <= heard][-1:], W)
    assert known.all()      # every window of these cases is W x W
    return D


def _run_case(name, tag, chunk=None, keep_d=True):
    from real_time_audio_sync_amd.wtw import BatchedWTW
    kw = CASES[name]
    W, hop = kw["W"], kw["hop"]
    ref, lives, recs = _case(name)
    eng = BatchedWTW(_dev(ref), W, hop, len(lives), keep_last_d=keep_d)
    if keep_d:
        # two pushes: the first ends where stream 0's last D is NaN in part
        heard = _heard_at_a_partly_nan_d(name)
        _push(eng, lives, stop=heard)
        for b in range(len(lives)):
            D = _last_d(ref, lives[b], recs[b], W, heard)
            assert np.array_equal(eng.last_d(b), D, equal_nan=True), (name, tag, b, "first push")
        _push(eng, lives, start=heard)
    else:
        _push(eng, lives, chunk)
    _same(eng, recs, (name, tag))
    if keep_d:
        for b in range(len(lives)):
            assert np.array_equal(eng.last_d(b), _last_d(ref, lives[b], recs[b], W), equal_nan=True), (name, tag, b)
    # the stream without silent frames equals its own single-stream handle
    one = BatchedWTW(_dev(ref), W, hop, 1)
    _push(one, lives[-1:], chunk)
    assert np.array_equal(eng.path(len(lives) - 1), one.path(0)), (name, tag)
    assert eng.state(len(lives) - 1) == one.state(0), (name, tag)
    one.close()
    eng.close()


@pytest.mark.parametrize("name", SMALL)
def test_silence_on_the_window_kernels(wtw_path, name):
    """W in {16, 33, 64, 65, 100, 128}: silent rows, silent columns and both, the whole live stream in one push."""
    _run_case(name, wtw_path)


@pytest.mark.parametrize("name", SMALL)
def test_silence_in_chunks_of_seven(name):
    """The same streams in pushes of 7 frames: at most one window per launch, nothing prefetched."""
    _run_case(name, "chunks", chunk=7, keep_d=False)


@pytest.mark.parametrize("name", STRIPS)
def test_silence_on_the_strip_dp(name):
    """W in {129, 130, 200}: three and four strips.  W in {768, 800}: 12 strips (backtrack and control step in the DP
    launch) and 13 (separate backtrack kernels), one silent row and one silent column each plus the run."""
    _run_case(name, "strips")
    if CASES[name]["W"] <= 200:
        _run_case(name, "strips, chunks", chunk=7, keep_d=False)


def test_silence_with_per_stream_references():
    """One create_refs handle: streams 0 and 2 follow a piece with silent frames, stream 1 a clean piece; streams 0 and
    1 hear silence, stream 2 does not."""
    from real_time_audio_sync_amd.wtw import BatchedWTW
    W, hop = 100, 37
    ref_a = _case("w100_cols")[0]
    ref_b, lives_b, _ = _case("w100_rows")
    assert not ref_a.all() and ref_b.all()
    ta, tb = _dev(ref_a), _dev(ref_b)
    lives = [lives_b[0], lives_b[0], lives_b[2]]
    recs = [si.wtw_window_record(r, l, W, hop) for r, l in zip((ref_a, ref_b, ref_a), lives)]
    eng = BatchedWTW.with_references([ta, tb, ta], W, hop, keep_last_d=True)
    _push(eng, lives)
    _same(eng, recs, "refs")
    for b in range(3):
        assert np.array_equal(eng.last_d(b), _last_d((ref_a, ref_b, ref_a)[b], lives[b], recs[b], W), equal_nan=True), b
    eng.close()


def test_restart_of_a_stream_whose_history_holds_silence():
    """Stream 1 hears the silent stream up to the end of its run, is restarted and hears it again from the start:
    nothing of the NaN-ridden history may survive.  The other streams have ended and stay as they are."""
    from real_time_audio_sync_amd.wtw import BatchedWTW
    name = "w65_rows"
    kw = CASES[name]
    W, hop = kw["W"], kw["hop"]
    ref, lives, recs = _case(name)
    eng = BatchedWTW(_dev(ref), W, hop, 3, keep_last_d=True)
    _push(eng, lives)
    _same(eng, recs, "before")
    assert np.isnan(eng.last_d(1)).any()
    eng.restart([1])
    empty = np.zeros((12, 0))
    _push(eng, [empty, lives[0], empty], chunk=50)
    _same(eng, [recs[0], recs[0], recs[2]], "restart")
    assert np.array_equal(eng.last_d(1), eng.last_d(0), equal_nan=True)
    eng.close()
