"""Chroma-difference live features (RTS_FEATURE_CHROMA_DIFF) without a GPU: the reference-made golden of the headline
configuration (tests.py:145-163 from microphone-style columns, tests/golden/make_livenote_diff_golden.py), the
condition under which the GPU test may demand its path exactly, and the carry model the GPU test counts columns with."""
import hashlib
import os

import numpy as np
import pytest

from test_chroma_gpu import CHROMA_ATOL  # noqa: E402  (the project's gate, not restated)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "livenote_diff_golden.npz")
C, MRC = 50, 3                  # tests.py:140
FFT_LEN, HOP = 4096, 2048

# Samples of the chopin live recording the GPU test feeds: the whole recording.  test_path_is_robust_to_the_chroma_gate
# holds for all of it (20 seeds, reference and live chroma both perturbed), so no prefix had to be cut.
LIVE_PREFIX_SAMPLES = None
# The golden holds the recording twice: as librosa.load returns it, (L + R) / 65536, and as a mono PCM16 microphone
# delivers it, round((L + R) / 2) / 32768 (suffix _pcm16).  The rounding moves path points, so a PCM16 stream is held to
# the second one.
VARIANTS = ["", "_pcm16"]


def live_samples(chopin_audio, suffix):
    """(float32 samples of the golden variant, the same as int16 or None)."""
    live = chopin_audio["live"][:LIVE_PREFIX_SAMPLES]
    if suffix == "":
        return live, None
    pcm = np.round(live * 32768.0).astype(np.int16)
    return pcm.astype(np.float32) / np.float32(32768.0), pcm


def clip_diff(cols):
    """np.clip(np.diff(chroma), 0, inf) (chroma.py:89-90) for frame-major columns [K][12] -> [max(K - 1, 0)][12]."""
    cols = np.asarray(cols, dtype=np.float64).reshape(-1, 12)
    return np.clip(np.diff(cols, axis=0), 0, np.inf)


def carry_model(events):
    """One stream of a chroma_diff session.  ``events``: per feed the number of chroma columns it completes, with
    "restart" in between where the stream is restarted (or the session reset).  Returns (n_cols per feed, emitted):
    ``emitted`` lists (run, i) for every column handed to the tracker, meaning chroma[i] - chroma[i - 1] of that run's
    chroma columns -- column i - 1 of np.diff over the run's concatenation."""
    has_carry, k, run = False, 0, 0
    n_cols, emitted = [], []
    for ev in events:
        if ev == "restart":
            has_carry, k, run = False, 0, run + 1
            continue
        skip = 0 if has_carry else 1
        n_cols.append(max(ev - skip, 0))
        emitted += [(run, i) for i in range(k + skip, k + ev)]
        k += ev
        has_carry = has_carry or ev > 0
    return n_cols, emitted


def live_chroma_columns(live):
    """oracle wav_to_chroma_col over un-padded hops (livenote_live.py:185-208) -> [K][12]."""
    from oracle import chroma_oracle as co
    n = (len(live) - FFT_LEN) // HOP + 1
    return np.stack([co.wav_to_chroma_col(live[m * HOP:m * HOP + FFT_LEN]) for m in range(n)])


def run_oracle(ref_diff, live_diff):
    """ref_diff (12, M), live_diff [K][12] -> (path, (live_ptr, ref_ptr), stopped)."""
    import oracle
    o = oracle.OtwOracle(ref_diff, C, MRC, variant=oracle.LIVENOTE_V2, cost=oracle.COST_EUCLID)
    o.run(np.ascontiguousarray(live_diff.T))
    return o.path, (o.state["t"], o.state["j"]), int(o.state["status"] == oracle.STOP_REF_END)


@pytest.fixture(scope="module", params=VARIANTS)
def chain(request, chopin_audio):
    from oracle import chroma_oracle as co
    ref_chroma = co.wav_to_chroma(chopin_audio["ref"])          # (12, M), what wav_to_chroma_diff differences
    return ref_chroma, live_chroma_columns(live_samples(chopin_audio, request.param)[0]), request.param


def test_pcm16_rounding_moves_the_path():
    g = np.load(GOLDEN)
    assert g["path"].shape == g["path_pcm16"].shape and not np.array_equal(g["path"], g["path_pcm16"])


def test_oracle_chain_reproduces_the_reference_golden(chain):
    ref_chroma, live_cols, suffix = chain
    z = np.load(GOLDEN)
    g = {k: z[k + suffix] if k + suffix in z.files else z[k] for k in z.files if not k.endswith("_pcm16")}
    ref_diff, live_diff = np.clip(np.diff(ref_chroma), 0, np.inf), clip_diff(live_cols)
    assert ref_diff.shape == (12, int(g["n_ref_cols"]))
    if LIVE_PREFIX_SAMPLES is None:
        assert live_cols.shape[0] == int(g["n_live_chroma_cols"]) and live_diff.shape[0] == int(g["n_live_cols"])
        # the very arrays the reference's code made (same numpy primitives in the same order)
        sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
        assert sha(ref_diff) == str(g["ref_seq_sha"])
        assert sha(np.ascontiguousarray(live_diff.T)) == str(g["live_cols_sha"])
    path, end, stopped = run_oracle(ref_diff, live_diff)
    k = len(live_diff)
    want = g["path"][g["path"][:, 0] < k] if LIVE_PREFIX_SAMPLES is not None else g["path"]
    assert np.array_equal(path, want) and len(path) > 200
    if LIVE_PREFIX_SAMPLES is None:
        assert end == (int(g["live_ptr"]), int(g["ref_ptr"])) and stopped == int(g["stopped"])
        assert int(g["consumed"]) == k


def test_path_is_robust_to_the_chroma_gate(chain):
    """What lets the GPU test demand the golden path exactly although the device's FFT is not numpy's: chroma columns
    anywhere within CHROMA_ATOL of the oracle's (live and reference) give the same path and end state."""
    ref_chroma, live_cols, _ = chain
    base = run_oracle(np.clip(np.diff(ref_chroma), 0, np.inf), clip_diff(live_cols))
    for seed in range(20):
        rs = np.random.RandomState(seed)
        lv = live_cols + rs.uniform(-CHROMA_ATOL, CHROMA_ATOL, size=live_cols.shape)
        rf = ref_chroma + rs.uniform(-CHROMA_ATOL, CHROMA_ATOL, size=ref_chroma.shape)
        got = run_oracle(np.clip(np.diff(rf), 0, np.inf), clip_diff(lv))
        assert np.array_equal(got[0], base[0]) and got[1:] == base[1:], seed


SCHEDULES = [
    [0, 0, 1, 0, 1, 3, 0, 2],                         # feeds without a column; the first column alone in its feed
    [1, "restart", 1, 1, 0, 4],                       # a restart between two single-column feeds
    [5, 0, 2, "restart", 0, 0, 3, "restart", 1, 0, 1, 1],
    [0, "restart", 0, 2, 1],                          # a restart before anything was carried
    [4, 1, 1, "restart", "restart", 1, 2],
]


@pytest.mark.parametrize("events", SCHEDULES)
def test_carry_model_is_np_diff_over_the_concatenation(events):
    n_cols, emitted = carry_model(events)
    runs, feeds = [[]], [e for e in events if e != "restart"]
    for e in events:
        if e == "restart":
            runs.append([])
        else:
            runs[-1].append(e)
    assert len(n_cols) == len(feeds) and sum(n_cols) == len(emitted)
    rs = np.random.RandomState(len(events))
    got, want = [], []
    for r, counts in enumerate(runs):
        chroma = rs.rand(sum(counts), 12)
        want.append(clip_diff(chroma))
        got.append(np.array([np.clip(chroma[i] - chroma[i - 1], 0, np.inf) for run, i in emitted if run == r]).reshape(-1, 12))
        assert [i for run, i in emitted if run == r] == list(range(1, sum(counts)))
    assert np.array_equal(np.concatenate(got), np.concatenate(want))
    # a feed hands over one column fewer than it completes exactly when it completes the first column of a run
    k = 0
    for r, counts in enumerate(runs):
        seen = 0
        for c in counts:
            assert n_cols[k] == (c if seen else max(c - 1, 0))
            seen += c
            k += 1


def test_carry_model_cases_the_gpu_test_relies_on():
    assert carry_model([0, 1, 1]) == ([0, 0, 1], [(0, 1)])
    assert carry_model([1, "restart", 1, 1]) == ([0, 0, 1], [(1, 1)])
    assert carry_model([3, "restart", 3]) == ([2, 2], [(0, 1), (0, 2), (1, 1), (1, 2)])
