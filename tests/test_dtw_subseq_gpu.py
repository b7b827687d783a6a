"""rts_dtw_subseq_paths / dtw_subseq_paths / align_excerpts (csrc/dtw.hip, sdp::DtwSubseqPolicy) on the GPU: subsequence
DTW with paths.  Bar: every pair's path, total, start, end and last row bit for bit what the serial restatement of the
contract gives (tests/dtw_subseq_model.py, pinned on the CPU by tests/test_dtw_subseq_cpu.py), path rows behind path_len
and row cells behind a pair's own N untouched; the same doubles as rts_locate and as rts_dtw_paths on the reported range.

The padding behind a pair's own frames is NaN in these tests: a kernel that read a frame beyond a pair's length could
not produce the model's result.  Every model result is computed once (module fixtures)."""
import ctypes

import numpy as np
import pytest

from scoped_env import Env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from dtw_subseq_model import planted, subseq  # noqa: E402

FILL = -7        # what the path buffer holds before a call
MARK = -12345.5  # and the row buffer
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _padded(seqs, n_max, tdt):
    """(12, n_k) arrays -> device [B][n_max][12], NaN behind every sequence's own frames."""
    out = np.full((len(seqs), n_max, 12), np.nan)
    for k, x in enumerate(seqs):
        out[k, :x.shape[1]] = x.T
    return torch.from_numpy(out).to(tdt).to(DEV)


def _frames(x, tdt):
    return torch.from_numpy(np.ascontiguousarray(x.T)).to(tdt).to(DEV)


def _call(a, b, a_len, b_len, B, want_row=True):
    """rts_dtw_subseq_paths through ctypes on pre-filled outputs.  a / b: device [B][n_max][12] or [n_max][12] (shared);
    a_len / b_len: lists or None (NULL).  -> dict of numpy arrays: path, plen, total, start, end, row (None without)."""
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.otw_batch import _np_dtype_code
    M, N = a.shape[-2], b.shape[-2]
    al = None if a_len is None else torch.tensor(a_len, dtype=torch.int32, device=DEV)
    bl = None if b_len is None else torch.tensor(b_len, dtype=torch.int32, device=DEV)
    path = torch.full((B, M + N, 2), FILL, dtype=torch.int32, device=DEV)
    plen = torch.full((B,), -5, dtype=torch.int32, device=DEV)
    total = torch.full((B,), -5.0, dtype=torch.float64, device=DEV)
    start = torch.full((B,), -5, dtype=torch.int32, device=DEV)
    end = torch.full((B,), -5, dtype=torch.int32, device=DEV)
    row = torch.full((B, N), MARK, dtype=torch.float64, device=DEV) if want_row else None
    nbytes = ctypes.c_size_t(0)
    nat.check(nat.lib.rts_dtw_subseq_paths_workspace_bytes(M, N, B, ctypes.byref(nbytes)))
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=DEV)
    nat.check(nat.lib.rts_dtw_subseq_paths(
        a.data_ptr(), _np_dtype_code(a.dtype), 0 if a.dim() == 2 else M, None if al is None else al.data_ptr(),
        b.data_ptr(), _np_dtype_code(b.dtype), 0 if b.dim() == 2 else N, None if bl is None else bl.data_ptr(),
        12, M, N, B, path.data_ptr(), plen.data_ptr(), total.data_ptr(), start.data_ptr(), end.data_ptr(),
        None if row is None else row.data_ptr(), ws.data_ptr(), nbytes.value,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return dict(path=path.cpu().numpy(), plen=plen.cpu().numpy(), total=total.cpu().numpy(), start=start.cpu().numpy(),
                end=end.cpu().numpy(), row=None if row is None else row.cpu().numpy())


def _check_pair(out, k, want):
    """Pair k against want = the model's (path, total, start, end, last row)."""
    mpath, mtotal, mstart, mend, mrow = want
    n = int(out["plen"][k])
    assert n == len(mpath), (k, n, len(mpath))
    assert np.array_equal(out["path"][k, :n], mpath), k
    assert (out["path"][k, n:] == FILL).all(), "pair %d: rows behind path_len were written" % k
    assert out["total"][k:k + 1].view(np.int64)[0] == np.float64(mtotal).view(np.int64), (k, out["total"][k], mtotal)
    assert (int(out["start"][k]), int(out["end"][k])) == (mstart, mend), (k, out["start"][k], out["end"][k], mstart, mend)
    if out["row"] is not None:
        nk = len(mrow)
        assert np.array_equal(out["row"][k, :nk].view(np.int64), mrow.view(np.int64)), k
        assert (out["row"][k, nk:] == MARK).all(), "pair %d: row cells behind N_k were written" % k


def _check_empty(out, k):
    assert out["plen"][k] == 0 and out["total"][k] == np.inf and out["start"][k] == -1 and out["end"][k] == -1, k
    assert (out["path"][k] == FILL).all() and (out["row"] is None or (out["row"][k] == MARK).all()), k


def _same_bits(x, y):
    for key in ("path", "plen", "start", "end"):
        assert np.array_equal(x[key], y[key]), key
    assert np.array_equal(x["total"].view(np.int64), y["total"].view(np.int64))


RAGGED_13 = [(1, 1), (1, 7), (9, 1), (2, 2), (64, 700), (65, 130), (513, 40), (769, 130), (700, 333)]  # 13 strips
RAGGED_12 = [(1, 40), (63, 300), (64, 77), (129, 150), (768, 130)]                                      # 12 strips


def _batch(a_list, b_list):
    return dict(shapes=[(x.shape[1], y.shape[1]) for x, y in zip(a_list, b_list)], a=a_list, b=b_list,
                want=[subseq(x, y) for x, y in zip(a_list, b_list)])


def _ragged(shapes, seed):
    from real_time_audio_sync_amd import synth
    return _batch([synth.synth_ref(m, seed=seed + k) for k, (m, _) in enumerate(shapes)],
                  [synth.synth_ref(n, seed=seed + 50 + k) for k, (_, n) in enumerate(shapes)])


def _sharp(n, seed):
    """A piece without held chords -- every frame its own random unit vector (float32 values) -- so that an exact copy of
    some of its frames matches exactly there and nowhere else."""
    x = np.random.RandomState(seed).rand(12, n) ** 3 + 0.02
    return (x / np.sqrt((x * x).sum(axis=0, keepdims=True))).astype(np.float32).astype(np.float64)


# (M, N, end): exact copies of frames [end - M + 1, end] of a sharp piece.  The last row sits on lane (M - 1) & 63 of the
# last strip and finishes column j at strip-step j + lane; a chunk is 16 steps.  With M = 1 and M = 65 (lane 0) ends 15
# and 16 / 79 and 80 are the last step of one chunk and the first of the next; with M = 8 (lane 7) ends 15 and 16 are that
# in columns; 37 of 40 and 98 of 100 lie in the last, partial chunk of columns.
EDGES = [(1, 40, 15), (1, 40, 16), (8, 40, 15), (8, 40, 16), (8, 40, 37), (65, 100, 79), (65, 100, 80), (65, 100, 98)]


def _planted(shapes, seed):
    """The shapes of a ragged batch with, wherever the piece is longer than the excerpt, the excerpt planted in it
    (noisy frames [A, A + M) of the piece, A about a third of the slack from the end), plus the EDGES pairs."""
    from real_time_audio_sync_amd import synth
    a_list, b_list = [], []
    for k, (m, n) in enumerate(shapes):
        if m < n:
            q, piece = planted(n, (2 * (n - m)) // 3, m, seed=seed + 2 * k)
        else:
            q, piece = synth.synth_ref(m, seed=seed + 2 * k), synth.synth_ref(n, seed=seed + 2 * k + 1)
        a_list.append(q)
        b_list.append(piece)
    for k, (m, n, e) in enumerate(EDGES):
        piece = _sharp(n, seed + 100 + k)
        a_list.append(piece[:, e - m + 1:e + 1].copy())
        b_list.append(piece)
    r = _batch(a_list, b_list)
    for (m, n, e), want in zip(EDGES, r["want"][len(shapes):]):
        assert want[3] == e and want[2] == e - m + 1, "the input is not the edge case it is meant to be"
    return r


@pytest.fixture(scope="module")
def ragged13():
    return _ragged(RAGGED_13, 100)


def _run(r, tdt=torch.float64, want_row=True):
    m_max, n_max = max(m for m, _ in r["shapes"]), max(n for _, n in r["shapes"])
    a, b = _padded(r["a"], m_max, tdt), _padded(r["b"], n_max, tdt)
    return _call(a, b, [m for m, _ in r["shapes"]], [n for _, n in r["shapes"]], len(r["shapes"]), want_row)


def _check_batch(out, r):
    for k in range(len(r["shapes"])):
        _check_pair(out, k, r["want"][k])


def test_ragged_batch_segment_backtrack(ragged13):
    """M_max = 769: 13 strips, so the backtrack is the hops / segment form with a workgroup per strip of the longest pair;
    pairs of 1 to 13 strips and 1 to 700 columns side by side."""
    _check_batch(_run(ragged13), ragged13)


def test_ragged_batch_tail_backtrack():
    """M_max = 768: 12 strips, the whole backtrack in one launch of 12 waves per pair."""
    r = _ragged(RAGGED_12, 300)
    _check_batch(_run(r), r)


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_zero_frames(tdt):
    """Digital silence (tests/silence_inputs.py): a 130 x 200 and a 200 x 70 pair in one call, zero frames on rows 0, 63, 64
    and the last of the excerpt, a run of zero columns and both ends of the piece: rows and columns of cost exactly 1.0,
    so whole stretches of the last row are equal and ``end`` is the first of them."""
    import silence_inputs as si
    pairs = [si.dtw_silent_pair(m, n, m + n) for m, n in si.DTW_SHAPES]
    r = _batch([x for x, _ in pairs], [y for _, y in pairs])
    _check_batch(_run(r, tdt), r)


@pytest.mark.parametrize("shapes,seed", [(RAGGED_13, 500), (RAGGED_12, 600)], ids=["segment", "tail"])
def test_planted_excerpts_in_ragged_batches(shapes, seed):
    """Both backtrack forms with ends and starts inside the piece, the chunk edges of EDGES among them."""
    r = _planted(shapes, seed)
    # every planted pair of the ragged shapes (M < N) and every EDGES pair begins and ends inside its piece; the other
    # ragged pairs (M >= N: nothing to plant) are random and end where they end
    inside = [k for k, ((m, n), w) in enumerate(zip(r["shapes"], r["want"])) if w[2] != 0 and w[3] != n - 1]
    planted_k = [k for k, (m, n) in enumerate(shapes) if m < n] + list(range(len(shapes), len(r["shapes"])))
    assert set(planted_k) <= set(inside), (planted_k, inside)
    assert 2 * len(inside) > len(r["shapes"]), "most pairs of the batch are meant to begin and end inside their piece"
    _check_batch(_run(r), r)


@pytest.mark.parametrize("config,grid", [(1, 3), (2, 1), (1, 13)])
def test_ragged_batch_forced_configurations(ragged13, config, grid):
    """Fewer workgroups than the longest pair's row groups, one workgroup for all of them, and one per strip of the
    longest pair: the last row is parked in the pair's own last row group's slot whatever the configuration."""
    base = _run(ragged13)
    with Env(RTS_SDP_CONFIG=config, RTS_SDP_GRID=grid):
        out = _run(ragged13)
    assert (out["plen"] > 0).all(), out["plen"]
    _same_bits(out, base)
    assert np.array_equal(out["row"].view(np.int64), base["row"].view(np.int64))
    _check_batch(out, ragged13)


@pytest.fixture(scope="module")
def shared_piece():
    """Eight excerpts of different lengths (1 to 5 strips) against one piece of 300 frames, and the model's results."""
    from real_time_audio_sync_amd import synth
    piece = synth.synth_ref(300, seed=400)
    lens = [1, 20, 63, 64, 65, 129, 200, 290]
    exc = [planted(300, min(7 + k, 300 - m), m, seed=400)[0] if k % 2 else synth.synth_ref(m, seed=410 + k)
           for k, m in enumerate(lens)]
    for q in exc:
        assert np.array_equal(q, q.astype(np.float32).astype(np.float64))
    return dict(piece=piece, lens=lens, exc=exc, want=[subseq(q, piece) for q in exc])


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_dtypes_sharing_clamping_and_empty_pairs(shared_piece, tdt):
    """All inputs hold float32 values, so both dtypes must give the model's float64 results."""
    from real_time_audio_sync_amd.dtw import dtw_subseq_paths
    s = shared_piece
    piece_d, exc_d = _frames(s["piece"], tdt), _padded(s["exc"], 290, tdt)
    # b shared (stride 0), b_len NULL, ragged a_len
    out = _call(exc_d, piece_d, s["lens"], None, 8)
    for k in range(8):
        _check_pair(out, k, s["want"][k])
    # both length tables NULL: two full-length excerpts, each against its own piece
    two = [s["exc"][7], s["exc"][7][:, ::-1].copy()]
    pieces = [s["piece"][:, :290], s["piece"][:, 10:]]
    out = _call(_padded(two, 290, tdt), _padded(pieces, 290, tdt), None, None, 2)
    for k in range(2):
        _check_pair(out, k, subseq(two[k], pieces[k]))
    # lengths above the maximum are clamped to it; the Python entry point takes plain lists and infers B
    res = dtw_subseq_paths(exc_d[6:8], piece_d, a_len=[200, 2 ** 31 - 1], b_len=[301, 300], want_row=True, check=True)
    path, plen, total, start, end, row = (t.cpu().numpy() for t in res)
    for k in range(2):
        mpath, mtotal, mstart, mend, mrow = s["want"][6 + k]
        n = int(plen[k])
        assert n == len(mpath) and np.array_equal(path[k, :n], mpath), k
        assert (total[k], int(start[k]), int(end[k])) == (mtotal, mstart, mend) and np.array_equal(row[k], mrow), k
    assert len(dtw_subseq_paths(exc_d[6:8], piece_d)) == 5
    # pairs without cells (length 0, negative) between ordinary ones
    out = _call(exc_d[:4], piece_d, [1, 0, 63, 64], [300, 300, -3, 300], 4)
    _check_empty(out, 1)
    _check_empty(out, 2)
    _check_pair(out, 0, s["want"][0])
    _check_pair(out, 3, s["want"][3])


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_same_doubles_as_rts_locate(tdt):
    """(total, end, start) == rts_locate's (cost, end, start) with RTS_COST_DOT on the same query and piece."""
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.locate import locate_batch
    piece = synth.synth_ref(500, seed=41)
    q = synth.synth_live(synth.synth_ref(300, seed=42), seed=43)[:, :256]
    pool = _frames(piece, tdt)
    first = torch.zeros(1, dtype=torch.int64, device=DEV)
    lens = torch.tensor([500], dtype=torch.int32, device=DEV)
    ms = [1, 64, 65, 256]
    out = _call(_padded([q[:, :m] for m in ms], 256, tdt), pool, ms, None, len(ms), want_row=False)
    for k, m in enumerate(ms):
        cost, end, start = (t.cpu().numpy() for t in locate_batch(_frames(q[:, :m], tdt), None, pool, first, lens))
        assert out["total"][k:k + 1].view(np.int64)[0] == cost[0].view(np.int64)[0], (m, out["total"][k], cost)
        assert (int(out["end"][k]), int(out["start"][k])) == (int(end[0, 0]), int(start[0, 0])), m
        assert int(out["plen"][k]) >= m


def test_total_is_rts_dtw_paths_on_the_reported_range(shared_piece):
    """Paths may differ under ties and are not compared."""
    from real_time_audio_sync_amd.dtw import dtw_paths
    s = shared_piece
    piece_d = _frames(s["piece"], torch.float64)
    out = _call(_padded(s["exc"], 290, torch.float64), piece_d, s["lens"], None, 8, want_row=False)
    for k in (0, 3, 4, 7):
        st, en = int(out["start"][k]), int(out["end"][k])
        assert 0 <= st <= en < 300
        _, plen, total = dtw_paths(_frames(s["exc"][k], torch.float64), piece_d[st:en + 1].contiguous(), check=True)
        assert total.cpu().numpy().view(np.int64)[0] == out["total"][k:k + 1].view(np.int64)[0], k


def test_longer_than_rts_locate_can_take():
    """M = 700 (11 strips) against N = 1500: frames [400, 925) of the piece with every third frame repeated.  Found where
    planted -- within the 8 frames tests/test_dtw_subseq_cpu.py states for its planted case: the same generator, the same
    noise, ends that may slide along a held chord -- and equal to the model."""
    A, L = 400, 525
    q, piece = planted(1500, A, L, seed=900, stretch=True)
    assert q.shape[1] == 700
    want = subseq(q, piece)
    out = _call(_frames(q, torch.float32), _frames(piece, torch.float32), None, None, 1)
    _check_pair(out, 0, want)
    print("start - A = %d, end - (A + L - 1) = %d" % (out["start"][0] - A, out["end"][0] - (A + L - 1)))
    assert abs(int(out["start"][0]) - A) <= 8 and abs(int(out["end"][0]) - (A + L - 1)) <= 8


def test_row_given_and_null_give_the_same_other_outputs(ragged13):
    _same_bits(_run(ragged13, want_row=True), _run(ragged13, want_row=False))


def test_no_dense_memory():
    """8 excerpts of 1 500 frames against their own pieces of 3 000: the call allocates less than ONE dense float64
    matrix of one pair (36 MB; workspace: about 0.45 bytes per cell, i.e. some 17 MB, plus outputs)."""
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.dtw import dtw_subseq_paths
    B, m, n = 8, 1500, 3000
    b = torch.stack([_frames(synth.synth_ref(n, seed=600 + k), torch.float32) for k in range(B)])
    a = (b[:, 700:700 + m] + 0.01).contiguous()
    a = (a / a.norm(dim=-1, keepdim=True)).contiguous()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    path, plen, total, start, end = dtw_subseq_paths(a, b, check=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - before
    print("peak bytes during dtw_subseq_paths: %d (cap %d)" % (peak, m * n * 8))
    assert peak < m * n * 8, peak
    plen, start, end = plen.cpu().numpy(), start.cpu().numpy(), end.cpu().numpy()
    for k in range(B):
        assert tuple(path[k, 0].tolist()) == (0, int(start[k])) and tuple(path[k, int(plen[k]) - 1].tolist()) == (m - 1, int(end[k]))
        assert 0 <= int(start[k]) <= int(end[k]) < n, (k, start[k], end[k])
    assert torch.isfinite(total).all()


def test_align_excerpts_against_the_model(shared_piece):
    """The list form end to end: four excerpts, one shared piece, the one-buffer read-back; an odd number of pairs with
    a piece of its own each and an excerpt without frames."""
    from real_time_audio_sync_amd.dtw import align_excerpts
    s = shared_piece

    def check(res, wants):
        assert len(res) == len(wants)
        for k, ((p, t, st, en), (mpath, mtotal, mstart, mend, _)) in enumerate(zip(res, wants)):
            assert p.dtype == np.int64 and p.shape == mpath.shape and np.array_equal(p, mpath), k
            assert isinstance(t, float) and t == mtotal and (st, en) == (mstart, mend), k
    pick = [1, 4, 5, 7]
    check(align_excerpts([s["exc"][k] for k in pick], s["piece"]), [s["want"][k] for k in pick])
    check(align_excerpts([s["exc"][k] for k in pick], s["piece"], dtype=torch.float32), [s["want"][k] for k in pick])
    res = align_excerpts([s["exc"][2], np.zeros((12, 0)), s["exc"][3]], [s["piece"]] * 3)
    assert res[1][0].shape == (0, 2) and res[1][1] == np.inf and res[1][2:] == (-1, -1)
    check([res[0], res[2]], [s["want"][2], s["want"][3]])
    check(align_excerpts(s["exc"][6], s["piece"]), [s["want"][6]])
    with pytest.raises(ValueError):
        align_excerpts([s["exc"][0], s["exc"][1]], [s["piece"]] * 3)
