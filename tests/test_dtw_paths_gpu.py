"""rts_dtw_paths / dtw_paths / align_pairs (csrc/dtw.hip): offline DTW that writes paths and total costs only, over
pairs of different lengths in one call.  Bar: every pair's path and acc_cost[-1][-1] bit-exact against the CPU oracle
(or against rts_dtw where the oracle would take too long), path rows behind path_len untouched.

The padding behind a pair's own frames is NaN in these tests: a kernel that read a frame beyond a pair's length could
not produce the oracle's result."""
import ctypes

import numpy as np
import pytest

from scoped_env import Env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = -7   # what the path buffer holds before a call


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _widen(x, tdt):
    return x.astype(np.float32).astype(np.float64) if tdt == torch.float32 else x


def _padded(seqs, n_max, tdt):
    """(12, n_k) arrays -> device [B][n_max][12], NaN behind every sequence's own frames."""
    out = np.full((len(seqs), n_max, 12), np.nan)
    for k, x in enumerate(seqs):
        out[k, :x.shape[1]] = x.T
    return torch.from_numpy(out).to(tdt).to("cuda:0")


def _call(a, b, a_len, b_len, B):
    """rts_dtw_paths through ctypes on a path buffer pre-filled with FILL.  a / b: device [B][n_max][12] or [n_max][12]
    (shared); a_len / b_len: lists or None (NULL).  Returns numpy (path [B][M+N][2], path_len [B], total [B])."""
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.otw_batch import _np_dtype_code
    dev = a.device
    M, N = a.shape[-2], b.shape[-2]
    al = None if a_len is None else torch.tensor(a_len, dtype=torch.int32, device=dev)
    bl = None if b_len is None else torch.tensor(b_len, dtype=torch.int32, device=dev)
    path = torch.full((B, M + N, 2), FILL, dtype=torch.int32, device=dev)
    plen = torch.full((B,), -5, dtype=torch.int32, device=dev)
    total = torch.full((B,), -5.0, dtype=torch.float64, device=dev)
    nbytes = ctypes.c_size_t(0)
    nat.check(nat.lib.rts_dtw_paths_workspace_bytes(M, N, B, ctypes.byref(nbytes)))
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    nat.check(nat.lib.rts_dtw_paths(a.data_ptr(), _np_dtype_code(a.dtype), 0 if a.dim() == 2 else M,
                                    None if al is None else al.data_ptr(),
                                    b.data_ptr(), _np_dtype_code(b.dtype), 0 if b.dim() == 2 else N,
                                    None if bl is None else bl.data_ptr(), 12, M, N, B, path.data_ptr(),
                                    plen.data_ptr(), total.data_ptr(), ws.data_ptr(), nbytes.value,
                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize()
    return path.cpu().numpy(), plen.cpu().numpy(), total.cpu().numpy()


def _check_pair(path, plen, total, k, want):
    """Pair k against want = (oracle path, oracle acc[-1, -1])."""
    opath, ototal = want
    n = int(plen[k])
    assert n == len(opath), (k, n, len(opath))
    assert np.array_equal(path[k, :n], opath), k
    assert total[k] == ototal, (k, total[k], ototal)
    assert (path[k, n:] == FILL).all(), "pair %d: rows behind path_len were written" % k


def _oracle(a, b):
    import oracle
    _, oacc, opath, _ = oracle.dtw(a, b)
    return opath, oacc[-1, -1]


RAGGED_13 = [(1, 1), (1, 7), (9, 1), (2, 2), (64, 700), (65, 130), (513, 40), (769, 130), (700, 333)]  # 13 strips
RAGGED_12 = [(1, 40), (63, 300), (64, 77), (129, 150), (768, 130)]                                      # 12 strips


def _ragged(shapes, seed):
    from real_time_audio_sync_amd import synth
    a_list = [synth.synth_ref(m, seed=seed + k) for k, (m, _) in enumerate(shapes)]
    b_list = [synth.synth_ref(n, seed=seed + 50 + k) for k, (_, n) in enumerate(shapes)]
    return dict(shapes=shapes, a=a_list, b=b_list, want=[_oracle(x, y) for x, y in zip(a_list, b_list)])


@pytest.fixture(scope="module")
def ragged13():
    return _ragged(RAGGED_13, 100)


def _run_ragged(r, tdt=torch.float64):
    m_max, n_max = max(m for m, _ in r["shapes"]), max(n for _, n in r["shapes"])
    a, b = _padded(r["a"], m_max, tdt), _padded(r["b"], n_max, tdt)
    return _call(a, b, [m for m, _ in r["shapes"]], [n for _, n in r["shapes"]], len(r["shapes"]))


def test_ragged_batch_segment_backtrack(ragged13):
    """M_max = 769: 13 strips, so the backtrack is the hops / segment form with a workgroup per strip of the longest pair;
    pairs of 1 to 13 strips and 1 to 700 columns side by side."""
    path, plen, total = _run_ragged(ragged13)
    for k in range(len(RAGGED_13)):
        _check_pair(path, plen, total, k, ragged13["want"][k])


def test_ragged_batch_tail_backtrack():
    """M_max = 768: 12 strips, the whole backtrack in one launch of 12 waves per pair.  The waves a shorter pair has no
    strip for must pass the barriers and write nothing."""
    r = _ragged(RAGGED_12, 300)
    path, plen, total = _run_ragged(r)
    for k in range(len(RAGGED_12)):
        _check_pair(path, plen, total, k, r["want"][k])


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_zero_frames(tdt):
    """Digital silence (tests/silence_inputs.py): a 130 x 200 and a 200 x 70 pair in one call, zero frames on rows 0, 63, 64
    and the last, a run of zero columns and both ends of the other sequence: rows and columns of cost exactly 1.0."""
    import silence_inputs as si
    pairs = [si.dtw_silent_pair(m, n, m + n) for m, n in si.DTW_SHAPES]
    r = dict(shapes=list(si.DTW_SHAPES), a=[x for x, _ in pairs], b=[y for _, y in pairs],
             want=[_oracle(x, y) for x, y in pairs])
    path, plen, total = _run_ragged(r, tdt)
    for k in range(len(pairs)):
        _check_pair(path, plen, total, k, r["want"][k])


@pytest.mark.parametrize("config,grid", [(1, 3), (2, 1), (1, 13)])
def test_ragged_batch_forced_configurations(ragged13, config, grid):
    """Row groups are per pair: fewer workgroups than the longest pair's row groups, one workgroup for all of them, and
    one per strip of the longest pair (most of which find no row group in a short pair).  Same bits as the default."""
    base = _run_ragged(ragged13)
    with Env(RTS_SDP_CONFIG=config, RTS_SDP_GRID=grid):
        path, plen, total = _run_ragged(ragged13)
    assert (plen > 0).all(), plen
    assert np.array_equal(plen, base[1]) and np.array_equal(path, base[0])
    assert np.array_equal(total.view(np.int64), base[2].view(np.int64))
    for k in range(len(RAGGED_13)):
        _check_pair(path, plen, total, k, ragged13["want"][k])


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_dtypes_sharing_clamping_and_empty_pairs(tdt):
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.dtw import dtw_paths
    from real_time_audio_sync_amd.otw_batch import frames_tensor
    dev = torch.device("cuda:0")
    one = synth.synth_ref(150, seed=400)                                    # 3 strips when it is `a`
    many = [synth.synth_ref(n, seed=410 + k) for k, n in enumerate((300, 77, 1, 129))]
    one_d, many_d = frames_tensor(one, dev, tdt), _padded(many, 300, tdt)
    lens = [300, 77, 1, 129]
    # a shared, a_len NULL, ragged b_len
    path, plen, total = _call(one_d, many_d, None, lens, 4)
    for k, y in enumerate(many):
        _check_pair(path, plen, total, k, _oracle(_widen(one, tdt), _widen(y, tdt)))
    # the reverse: b shared, b_len NULL, ragged a_len (5 strips at most)
    path, plen, total = _call(many_d, one_d, lens, None, 4)
    for k, x in enumerate(many):
        _check_pair(path, plen, total, k, _oracle(_widen(x, tdt), _widen(one, tdt)))
    # lengths above the maximum are clamped to it; the Python entry point takes plain lists
    full = [synth.synth_ref(300, seed=420 + k) for k in range(2)]
    full_d = _padded(full, 300, tdt)
    p, n, t = dtw_paths(full_d, one_d, a_len=[1000, 2 ** 31 - 1], b_len=[151, 150], check=True)
    p, n, t = p.cpu().numpy(), n.cpu().numpy(), t.cpu().numpy()
    for k, x in enumerate(full):
        opath, ototal = _oracle(_widen(x, tdt), _widen(one, tdt))
        assert int(n[k]) == len(opath) and np.array_equal(p[k, :int(n[k])], opath) and t[k] == ototal, k
    # pairs without cells (length 0, negative) between ordinary ones
    path, plen, total = _call(many_d, one_d, [300, 0, 77, 129], [150, 150, -3, 149], 4)
    for k in (1, 2):
        assert plen[k] == 0 and total[k] == np.inf and (path[k] == FILL).all(), k
    _check_pair(path, plen, total, 0, _oracle(_widen(many[0], tdt), _widen(one, tdt)))
    _check_pair(path, plen, total, 3, _oracle(_widen(many[3][:, :129], tdt), _widen(one[:, :149], tdt)))


def test_agrees_with_the_dense_call():
    """Six 700 x 333 pairs (11 strips each, b shared), as in test_dtw_batched_pipelines_side_by_side."""
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.dtw import dtw_batch, dtw_paths
    from real_time_audio_sync_amd.otw_batch import frames_tensor
    dev = torch.device("cuda:0")
    ref = synth.synth_ref(333, seed=901)
    lives = [synth.synth_live(synth.synth_ref(900, seed=910 + k), seed=920 + k, max_frames=700)[:, :700] for k in range(6)]
    a = torch.stack([frames_tensor(l, dev, torch.float64) for l in lives])
    b = frames_tensor(ref, dev, torch.float64)
    _, acc, _, dpath, dlen = dtw_batch(a, b, want_back=False, check=True)
    path, plen, total = dtw_paths(a, b, check=True)
    assert torch.equal(plen, dlen)
    for k in range(6):
        n = int(plen[k])
        assert torch.equal(path[k, :n], dpath[k, :n]), k
    assert np.array_equal(total.cpu().numpy(), acc[:, -1, -1].cpu().numpy())
    assert (total == acc[:, -1, -1]).all()


def test_long_pair_beside_thin_ones():
    """A 30-minute-sized pair (303 strips, hundreds of workgroups in one pipeline) in one call with a 5-strip pair of
    19 000 columns and a 297-strip pair of 300 columns."""
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.dtw import align_pairs, dtw_batch, dtw_paths
    from real_time_audio_sync_amd.otw_batch import frames_tensor
    dev = torch.device("cuda:0")
    n = 19380
    ref = synth.synth_ref(n, seed=80)
    live = synth.synth_live(ref, seed=81)
    wide_a, wide_b = synth.synth_ref(300, seed=82), synth.synth_ref(19000, seed=83)
    tall_a, tall_b = synth.synth_ref(19000, seed=84), synth.synth_ref(300, seed=85)
    a_list, b_list = [live, wide_a, tall_a], [ref, wide_b, tall_b]
    shapes = [(x.shape[1], y.shape[1]) for x, y in zip(a_list, b_list)]
    m_max, n_max = max(m for m, _ in shapes), max(k for _, k in shapes)
    a, b = _padded(a_list, m_max, torch.float32), _padded(b_list, n_max, torch.float32)
    path, plen, total = dtw_paths(a, b, a_len=[m for m, _ in shapes], b_len=[k for _, k in shapes], check=True)
    path, plen, total = path.cpu().numpy(), plen.cpu().numpy(), total.cpu().numpy()
    _, acc, _, dpath, dlen = dtw_batch(frames_tensor(live, dev, torch.float32), frames_tensor(ref, dev, torch.float32),
                                       want_back=False, check=True)
    assert int(plen[0]) == int(dlen[0])
    assert np.array_equal(path[0, :int(plen[0])], dpath[0, :int(dlen[0])].cpu().numpy())
    assert total[0] == float(acc[0, -1, -1])
    del acc, dpath
    for k in (1, 2):
        p = path[k, :int(plen[k])]
        assert tuple(p[0]) == (0, 0) and tuple(p[-1]) == (shapes[k][0] - 1, shapes[k][1] - 1), k
        step = np.diff(p, axis=0)
        assert (step >= 0).all() and (step <= 1).all() and (step.sum(axis=1) >= 1).all(), k
        assert np.isfinite(total[k]) and total[k] > 0
    # the list form a corpus harness calls: same paths and totals for the two thin pairs
    res = align_pairs([wide_a, tall_a], [wide_b, tall_b], dtype=torch.float32)
    for (p, t), k in zip(res, (1, 2)):
        assert p.dtype == np.int64 and np.array_equal(p, path[k, :int(plen[k])]) and t == total[k], k


def test_align_pairs_against_the_oracle():
    """The list form end to end: padding on the host, the one-buffer read-back (odd and even numbers of pairs move
    the path's place in it), a shared array on either side, a sequence without frames."""
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.dtw import align_pairs
    a_list = [synth.synth_ref(m, seed=700 + k) for k, m in enumerate((130, 64, 201))]
    b_list = [synth.synth_ref(n, seed=710 + k) for k, n in enumerate((90, 300, 65))]
    one = synth.synth_ref(77, seed=720)

    def check(res, pairs):
        assert len(res) == len(pairs)
        for k, ((p, t), (x, y)) in enumerate(zip(res, pairs)):
            opath, ototal = _oracle(x, y)
            assert p.dtype == np.int64 and p.shape == opath.shape and np.array_equal(p, opath), k
            assert isinstance(t, float) and t == ototal, k
    check(align_pairs(a_list, b_list), list(zip(a_list, b_list)))                              # 3 pairs, ragged
    check(align_pairs(a_list[:2], one), [(x, one) for x in a_list[:2]])                        # 2 pairs, b shared
    check(align_pairs(one, b_list, dtype=torch.float32), [(one, y) for y in b_list])          # a shared, float32
    check(align_pairs(one, one), [(one, one)])
    res = align_pairs([a_list[0], np.zeros((12, 0)), a_list[2]], b_list)                       # a sequence without frames
    assert res[1][0].shape == (0, 2) and res[1][1] == np.inf
    check([res[0], res[2]], [(a_list[0], b_list[0]), (a_list[2], b_list[2])])
    with pytest.raises(ValueError):
        align_pairs(a_list, b_list[:2])


def test_no_dense_memory():
    """8 pairs of 3 000 x 3 000: the call allocates less than one eighth of ONE dense float64 matrix of the batch
    (workspace: about 0.45 bytes per cell, i.e. some 33 MB, plus 0.4 MB of outputs, against the cap of 72 MB)."""
    from real_time_audio_sync_amd import _native as nat, synth
    from real_time_audio_sync_amd.dtw import dtw_paths
    from real_time_audio_sync_amd.otw_batch import frames_tensor
    dev = torch.device("cuda:0")
    B, n = 8, 3000
    b = frames_tensor(synth.synth_ref(n, seed=600), dev, torch.float32)
    a = torch.stack([frames_tensor(synth.synth_ref(n, seed=601 + k), dev, torch.float32) for k in range(B)])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    path, plen, total = dtw_paths(a, b, check=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    print("peak bytes during dtw_paths: %d (cap %d)" % (peak, n * n * 8))
    assert peak < n * n * 8, peak
    plen = plen.cpu().numpy()
    for k in range(B):
        assert tuple(path[k, int(plen[k]) - 1].tolist()) == (n - 1, n - 1) and tuple(path[k, 0].tolist()) == (0, 0)
    assert torch.isfinite(total).all()
    nbytes = ctypes.c_size_t(0)
    nat.check(nat.lib.rts_dtw_paths_workspace_bytes(19380, 19380, 1, ctypes.byref(nbytes)))
    print("workspace for one 19380 x 19380 pair: %d bytes" % nbytes.value)
    assert nbytes.value < 256 * 1000 * 1000


def test_argument_errors():
    """Every documented argument error, with the argument named; nothing is enqueued (the pointers are never used)."""
    from real_time_audio_sync_amd import _native as nat
    INVALID, UNSUPPORTED = -1, -2
    nbytes = ctypes.c_size_t(0)
    nat.check(nat.lib.rts_dtw_paths_workspace_bytes(100, 90, 2, ctypes.byref(nbytes)))
    P = ctypes.c_void_p
    ok = dict(a=P(4096), a_len=None, b=P(8192), b_len=None, F=12, M=100, N=90, B=2, path=P(12288), plen=P(16384),
              total=P(20480), ws=P(1 << 20), ws_bytes=nbytes.value)

    def call(**kw):
        v = dict(ok, **kw)
        rc = nat.lib.rts_dtw_paths(v["a"], nat.F32, v["M"], v["a_len"], v["b"], nat.F32, v["N"], v["b_len"], v["F"],
                                   v["M"], v["N"], v["B"], v["path"], v["plen"], v["total"], v["ws"], v["ws_bytes"], None)
        return rc, nat.lib.rts_last_error()

    for arg, name in (("path", b"path_dev"), ("plen", b"path_len_dev"), ("total", b"total_dev"), ("ws", b"ws_dev"),
                      ("a", b"a_dev"), ("b", b"b_dev")):
        rc, msg = call(**{arg: None})
        assert rc == INVALID and name in msg, (arg, rc, msg)
    rc, msg = call(F=13)
    assert rc == UNSUPPORTED and b"F" in msg and b"12" in msg, msg
    rc, msg = call(M=0)
    assert rc == INVALID and b"M_max" in msg, msg
    rc, msg = call(N=-1)
    assert rc == INVALID and b"N_max" in msg, msg
    rc, msg = call(ws_bytes=nbytes.value - 1)
    assert rc == INVALID and b"workspace" in msg and b"rts_dtw_paths_workspace_bytes" in msg, msg
    rc, msg = call(ws=P((1 << 20) + 8))
    assert rc == INVALID and b"16-byte aligned" in msg, msg
    rc, msg = call(B=65536)
    assert rc == INVALID and b"65535" in msg, msg
    size = ctypes.c_size_t(0)
    assert nat.lib.rts_dtw_paths_workspace_bytes(0, 90, 2, ctypes.byref(size)) == INVALID
    assert b"M_max" in nat.lib.rts_last_error()
    assert nat.lib.rts_dtw_paths_workspace_bytes(100, 90, 2, None) == INVALID and b"bytes" in nat.lib.rts_last_error()
