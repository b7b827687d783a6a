"""Where the offline entry points write: only into the device memory the caller handed them.

rts_dtw, rts_dtw_paths, rts_dtw_subseq_paths, rts_chroma_frames, rts_chroma_project, rts_chroma_diff, rts_resample_run,
rts_otw_path_cost and the dense mirrors of rts_otw_set_dense / rts_otw_replay_dense are called through ``_native.lib``
with every output -- and, for the three DTW calls, a workspace of exactly the bytes their size function returned -- placed
by tests/guarded.py between two guards.  Three properties per entry point, next to the comparison with its plain reference:

  (a) confinement   no guard byte in front of or behind any output or the workspace has changed after the call;
  (b) independence  the call is repeated with outputs and workspace pre-filled with 0x00, 0xFF and 0x55: what the header
                    documents as written is bit-identical every time and equals the reference, what it calls "left
                    untouched" (path rows behind path_len, samples behind n_out_dev[b], row_dev cells behind a pair's N)
                    still holds the fill;
  (c) offsets       the workspace at base + 16 and base + 240 (the header promises nothing beyond 16 bytes), every
                    output at the smallest alignment the header allows: int8 at an odd address, double at 8 mod 16,
                    int32 at 4 mod 16, path_dev at 8 mod 16, stft_out_dev at 16 mod 512.  The two outputs that need
                    more than their element type's alignment (path_dev: 8 bytes, stft_out_dev: 16) are refused below
                    it, and the refusals are tested here instead of the stores.

What a green run does NOT show: the workspace is one allocation of eight sections behind a header, and a section that
spills into the next one hits no guard.  That the carve agrees with the size function is checked elsewhere: both walk
one table (csrc/sdp_plan.h), and tests/test_sdp_plan_cpu.py holds every section's offset and length, and the total,
against a model of the arrays' shapes.  A kernel that writes past the end of a section it was handed correctly is
still seen only through (b) and the reference comparison -- as a result that is wrong or that changes with the fill --
never as a guard that tripped."""
import ctypes
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from dtw_subseq_model import subseq  # noqa: E402
from guarded import FILLS, guarded, holds_fill, same_bytes  # noqa: E402
from resample_model import out_len, resample_model  # noqa: E402
from scoped_env import Env  # noqa: E402
from test_chroma_gpu import CHROMA_ATOL, STFT_RTOL  # noqa: E402
from test_reacquire_cpu import path_cost_ref  # noqa: E402

DEV = "cuda:0"
INVALID = -1
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "real_time_audio_sync_amd", "csrc")
I8, I32, F32, F64, U8 = torch.int8, torch.int32, torch.float32, torch.float64, torch.uint8
# (c): the smallest alignment each element type may arrive at, as an offset from a 512-byte boundary
NATURAL = {I8: 1, I32: 4, F32: 4, F64: 8}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _const(source, name):
    """``constexpr int <name> = <value>;`` as the kernels' source states it."""
    with open(os.path.join(CSRC, source)) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


K_CHUNK = _const("sdp.h", "kChunk")            # columns per step-code word
K_TAIL_STRIPS = _const("sdp.h", "kTailStrips")  # most strips the one-launch backtrack takes
K_CHROMA_FR = _const("chroma.hip", "kChromaFR")  # frames per workgroup pass, fft_len <= 4096
K_BIG_FR = _const("chroma.hip", "kBigFR")        # the same for fft_len 8192


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nat():
    from real_time_audio_sync_amd import _native
    return _native


class _Bufs(object):
    """The guarded buffers of one call: ``new`` makes one, ``done`` synchronises, checks every guard and returns the
    contents as numpy arrays."""

    def __init__(self, fill, offsets=False, ws_offset=0):
        self.fill, self.offsets, self.ws_offset = fill, offsets, ws_offset
        self.t, self.checks = {}, {}

    def new(self, name, shape, dtype, offset=None):
        if offset is None:
            offset = NATURAL[dtype] if self.offsets else 0
        self.t[name], self.checks[name] = guarded(shape, dtype, DEV, self.fill, offset_bytes=offset)
        return self.t[name].data_ptr()

    def workspace(self, nbytes):
        return self.new("workspace", (nbytes,), U8, self.ws_offset)

    def done(self):
        torch.cuda.synchronize()
        for name, check in self.checks.items():
            check(name)
        return {name: t.cpu().numpy() for name, t in self.t.items() if name != "workspace"}


def _frames(x, tdt):
    return torch.from_numpy(np.ascontiguousarray(x.T)).to(tdt).to(DEV)


def _widen(x, tdt):
    return x.astype(np.float32).astype(np.float64) if tdt == F32 else x


def _code(tdt):
    return _nat().F32 if tdt == F32 else _nat().F64


# ---- rts_dtw ----------------------------------------------------------------------------------------------------------
# (M, N): one cell; one strip and one chunk of columns; a second strip of one row with N one past a chunk; three strips;
# 12 strips (the whole backtrack in one launch) and 13 (separate kernels); N at the step-code chunk width and one either
# side of it.  B = 64 makes the workspace's trailing ticket section exactly 256 bytes: nothing past it hides in padding.
DTW_SHAPES = [(1, 1), (64, 16), (65, 17), (129, 33), (768, 130), (769, 130),
              (64, K_CHUNK - 1), (65, K_CHUNK), (64, K_CHUNK + 1)]
# (M, N, B, dtype, b shared, back_dev given)
DTW_CASES = [(1, 1, 1, F32, True, True), (1, 1, 64, F64, False, False), (64, 16, 3, F64, False, True),
             (65, 17, 64, F32, False, True), (129, 33, 3, F64, True, False), (129, 33, 1, F32, False, True),
             (768, 130, 3, F32, False, True), (768, 130, 1, F64, True, False), (769, 130, 64, F64, True, True),
             (769, 130, 1, F32, False, False), (64, K_CHUNK - 1, 3, F32, True, True), (65, K_CHUNK, 1, F64, False, True),
             (64, K_CHUNK + 1, 64, F64, False, False)]
assert {(c[0], c[1]) for c in DTW_CASES} == set(DTW_SHAPES) and {c[2] for c in DTW_CASES} == {1, 3, 64}
assert 768 // 64 == K_TAIL_STRIPS, "768 and 769 rows are meant to lie on both sides of the one-launch backtrack"

_dtw_refs = {}


def _dtw_case(M, N, B, tdt, shared_b):
    """Inputs and the oracle's (cost, acc, path, back) of every pair, computed once per case."""
    key = (M, N, B, tdt, shared_b)
    if key not in _dtw_refs:
        import oracle
        from real_time_audio_sync_amd import synth
        a = [_widen(synth.synth_ref(M, seed=7000 + 31 * M + k), tdt) for k in range(B)]
        b = [_widen(synth.synth_ref(N, seed=9000 + 17 * N + k), tdt) for k in range(1 if shared_b else B)]
        want = [oracle.dtw(a[k], b[0 if shared_b else k]) for k in range(B)]
        _dtw_refs[key] = (a, b, want)
    return _dtw_refs[key]


def _run_dtw(M, N, B, tdt, shared_b, want_back, fill, offsets=False, ws_offset=0):
    nat = _nat()
    a_np, b_np, _ = _dtw_case(M, N, B, tdt, shared_b)
    a = torch.stack([_frames(x, tdt) for x in a_np])
    b = _frames(b_np[0], tdt) if shared_b else torch.stack([_frames(x, tdt) for x in b_np])
    nbytes = ctypes.c_size_t(0)
    nat.check(nat.lib.rts_dtw_workspace_bytes(M, N, B, ctypes.byref(nbytes)))
    bufs = _Bufs(fill, offsets, ws_offset)
    cost, acc = bufs.new("cost", (B, M, N), F64), bufs.new("acc", (B, M, N), F64)
    back = bufs.new("back", (B, M, N), I8) if want_back else None
    # path_dev: 8 bytes is the least the header allows (its refusal below that: test_misaligned_outputs_are_refused)
    path = bufs.new("path", (B, M + N, 2), I32, 8 if offsets else 0)
    plen = bufs.new("plen", (B,), I32)
    ws = bufs.workspace(nbytes.value)
    nat.check(nat.lib.rts_dtw(a.data_ptr(), _code(tdt), M, b.data_ptr(), _code(tdt), 0 if shared_b else N, 12, M, N, B,
                              cost, acc, back, path, plen, ws, nbytes.value, _stream()))
    return bufs.done()


def _check_dtw(out, M, N, B, tdt, shared_b, want_back, fill, tag):
    _, _, want = _dtw_case(M, N, B, tdt, shared_b)
    for k, (ocost, oacc, opath, oback) in enumerate(want):
        n = int(out["plen"][k])
        assert n == len(opath), (tag, k, n, len(opath))
        assert np.array_equal(out["path"][k, :n], opath), (tag, k)
        assert holds_fill(out["path"][k, n:], fill), (tag, k, "path rows behind path_len were written")
        assert same_bytes(out["cost"][k], ocost), (tag, k, "cost")
        assert same_bytes(out["acc"][k], oacc), (tag, k, "acc")
        if want_back:
            assert np.array_equal(out["back"][k], oback), (tag, k, "back")


@pytest.mark.parametrize("M,N,B,tdt,shared_b,want_back", DTW_CASES,
                         ids=["%dx%d-B%d-%s-%s-%s" % (c[0], c[1], c[2], "f32" if c[3] == F32 else "f64",
                                                      "bshared" if c[4] else "bperpair", "back" if c[5] else "noback")
                              for c in DTW_CASES])
def test_dtw_confined_and_independent_of_stale_contents(M, N, B, tdt, shared_b, want_back):
    """(a) and (b) for rts_dtw.  bnd is refilled with the "not yet written" pattern only when a pair has more than one
    row group, codes and entb never: a word read before it was written would change the result with the fill."""
    for fill in FILLS:
        out = _run_dtw(M, N, B, tdt, shared_b, want_back, fill)
        _check_dtw(out, M, N, B, tdt, shared_b, want_back, fill, "fill 0x%02X" % fill)


@pytest.mark.parametrize("ws_offset", [16, 240])
@pytest.mark.parametrize("M,N,B", [(65, 17, 3), (129, 33, 64), (768, 130, 3), (769, 130, 3)])
def test_dtw_at_the_alignments_the_header_states(M, N, B, ws_offset):
    """(c) for rts_dtw.  What the kernels store where, read before this ran: every workspace section starts at
    ws_dev + a multiple of 256, so ws_dev's own 16 bytes are what the 16-byte accesses to the column records
    (sdp::prep_column, fetch_records) and the 8-byte ones to bnd and pscr get; cost, back, path_len: scalar stores;
    acc: 16-byte stores at 8-byte aligned addresses whatever acc_dev is (run_rowgroup: a row's segment starts at column
    16 m - r), so acc_dev at 8 mod 16 is nothing new to them; path: 8-byte stores (path_segment), hence path_dev at 8."""
    fill = FILLS[1] if ws_offset == 16 else FILLS[2]
    out = _run_dtw(M, N, B, F64, False, True, fill, offsets=True, ws_offset=ws_offset)
    _check_dtw(out, M, N, B, F64, False, True, fill, "ws + %d" % ws_offset)


# ---- rts_dtw_paths / rts_dtw_subseq_paths -------------------------------------------------------------------------------
def _ragged_lens(M, N, B, seed):
    """Per-pair lengths as the call gets them, and as the pair has them after clamping.  Pair 0 is clamped from above the
    maxima (so it is the full M x N), pair 1 has no frames on one side, the next five are drawn from the whole range,
    the rest are short (the subsequence model is a Python loop over cells)."""
    rs = np.random.RandomState(seed)
    given = [(M + 5, N + 1000)]
    if B > 1:
        given.append((0, N))
    while len(given) < B:
        big = len(given) < 7
        m_top, n_top = (M, N) if big else (min(M, 70), min(N, 40))
        given.append((int(rs.randint(1, m_top + 1)), int(rs.randint(1, n_top + 1))))
    return given, [(max(0, min(m, M)), max(0, min(n, N))) for m, n in given]


PATHS_CASES = [(1, 1, 1, F64), (64, 16, 3, F32), (65, 17, 64, F64), (129, 33, 3, F32), (768, 130, 3, F64),
               (769, 130, 64, F32), (769, 130, 1, F64), (64, K_CHUNK - 1, 3, F64), (65, K_CHUNK, 3, F32),
               (64, K_CHUNK + 1, 1, F32)]
assert {(c[0], c[1]) for c in PATHS_CASES} == set(DTW_SHAPES) and {c[2] for c in PATHS_CASES} == {1, 3, 64}
_paths_refs = {}


def _paths_case(M, N, B, tdt):
    """Padded inputs (NaN behind a pair's own frames), the lengths, and both references of every pair: the oracle's
    (path, acc[-1, -1]) and the subsequence model's (path, total, start, end, last row); None for a pair without cells."""
    key = (M, N, B, tdt)
    if key not in _paths_refs:
        import oracle
        from real_time_audio_sync_amd import synth
        given, own = _ragged_lens(M, N, B, 100 * M + N + B)
        a = np.full((B, M, 12), np.nan)
        b = np.full((B, N, 12), np.nan)
        full, sub = [], []
        for k, (m, n) in enumerate(own):
            x = _widen(synth.synth_ref(max(m, 1), seed=5000 + k), tdt)
            y = _widen(synth.synth_ref(max(n, 1), seed=6000 + k), tdt)
            a[k, :m], b[k, :n] = x.T[:m], y.T[:n]
            if m < 1 or n < 1:
                full.append(None)
                sub.append(None)
                continue
            _, oacc, opath, _ = oracle.dtw(x, y)
            full.append((opath, oacc[-1, -1]))
            sub.append(subseq(x, y))
        _paths_refs[key] = (a, b, given, own, full, sub)
    return _paths_refs[key]


def _run_paths(M, N, B, tdt, fill, subseq_form, want_row=True, offsets=False, ws_offset=0):
    nat = _nat()
    a_np, b_np, given, _, _, _ = _paths_case(M, N, B, tdt)
    a, b = torch.from_numpy(a_np).to(tdt).to(DEV), torch.from_numpy(b_np).to(tdt).to(DEV)
    al = torch.tensor([m for m, _ in given], dtype=I32, device=DEV)
    bl = torch.tensor([n for _, n in given], dtype=I32, device=DEV)
    nbytes = ctypes.c_size_t(0)
    size_fn = nat.lib.rts_dtw_subseq_paths_workspace_bytes if subseq_form else nat.lib.rts_dtw_paths_workspace_bytes
    nat.check(size_fn(M, N, B, ctypes.byref(nbytes)))
    bufs = _Bufs(fill, offsets, ws_offset)
    path = bufs.new("path", (B, M + N, 2), I32, 8 if offsets else 0)
    plen, total = bufs.new("plen", (B,), I32), bufs.new("total", (B,), F64)
    if subseq_form:
        start, end = bufs.new("start", (B,), I32), bufs.new("end", (B,), I32)
        row = bufs.new("row", (B, N), F64) if want_row else None
    ws = bufs.workspace(nbytes.value)
    if subseq_form:
        nat.check(nat.lib.rts_dtw_subseq_paths(a.data_ptr(), _code(tdt), M, al.data_ptr(), b.data_ptr(), _code(tdt), N,
                                               bl.data_ptr(), 12, M, N, B, path, plen, total, start, end, row, ws,
                                               nbytes.value, _stream()))
    else:
        nat.check(nat.lib.rts_dtw_paths(a.data_ptr(), _code(tdt), M, al.data_ptr(), b.data_ptr(), _code(tdt), N,
                                        bl.data_ptr(), 12, M, N, B, path, plen, total, ws, nbytes.value, _stream()))
    return bufs.done()


def _check_paths(out, M, N, B, tdt, fill, subseq_form, tag):
    _, _, _, own, full, sub = _paths_case(M, N, B, tdt)
    for k in range(B):
        want = (sub if subseq_form else full)[k]
        tagk = (tag, k, own[k])
        if want is None:
            assert out["plen"][k] == 0 and out["total"][k] == np.inf and holds_fill(out["path"][k], fill), tagk
            if subseq_form:
                assert out["start"][k] == -1 and out["end"][k] == -1, tagk
                assert "row" not in out or holds_fill(out["row"][k], fill), tagk
            continue
        n = int(out["plen"][k])
        assert n == len(want[0]), tagk + (n, len(want[0]))
        assert np.array_equal(out["path"][k, :n], want[0]), tagk
        assert holds_fill(out["path"][k, n:], fill), tagk + ("path rows behind path_len were written",)
        assert same_bytes(out["total"][k:k + 1], np.array([want[1]], dtype=np.float64)), tagk + (out["total"][k], want[1])
        if subseq_form:
            assert (int(out["start"][k]), int(out["end"][k])) == (want[2], want[3]), tagk
            if "row" in out:
                nk = own[k][1]
                assert same_bytes(out["row"][k, :nk], want[4]), tagk + ("row",)
                assert holds_fill(out["row"][k, nk:], fill), tagk + ("row cells behind the pair's N were written",)


def _same_documented(x, y, own, tag):
    """Two runs of a path-only call agree bit for bit in everything the header documents as written."""
    for key in ("plen", "total", "start", "end"):
        if key in x:
            assert same_bytes(x[key], y[key]), (tag, key)
    for k, (m, n) in enumerate(own):
        p = max(int(x["plen"][k]), 0)
        assert same_bytes(x["path"][k, :p], y["path"][k, :p]), (tag, k, "path")
        if "row" in x and "row" in y and m >= 1:
            assert same_bytes(x["row"][k, :n], y["row"][k, :n]), (tag, k, "row")


@pytest.mark.parametrize("subseq_form", [False, True], ids=["rts_dtw_paths", "rts_dtw_subseq_paths"])
@pytest.mark.parametrize("M,N,B,tdt", PATHS_CASES,
                         ids=["%dx%d-B%d-%s" % (c[0], c[1], c[2], "f32" if c[3] == F32 else "f64") for c in PATHS_CASES])
def test_paths_confined_and_independent_of_stale_contents(M, N, B, tdt, subseq_form):
    """(a) and (b) for the two path-only calls on ragged batches, once per fill, then with one and with two strips per
    workgroup (RTS_SDP_CONFIG): both row-group sizes carve the same workspace.  row_dev is given in every run but the
    last, which passes NULL."""
    own = _paths_case(M, N, B, tdt)[3]
    runs = [(fill, {}, True) for fill in FILLS]
    runs += [(FILLS[1], dict(RTS_SDP_CONFIG=1), True), (FILLS[2], dict(RTS_SDP_CONFIG=2), not subseq_form)]
    first = None
    for fill, env, want_row in runs:
        tag = "fill 0x%02X %s" % (fill, env or "")
        with Env(**env):
            out = _run_paths(M, N, B, tdt, fill, subseq_form, want_row=want_row)
        _check_paths(out, M, N, B, tdt, fill, subseq_form, tag)
        first = first or out
        _same_documented(first, out, own, tag)


@pytest.mark.parametrize("subseq_form", [False, True], ids=["rts_dtw_paths", "rts_dtw_subseq_paths"])
@pytest.mark.parametrize("ws_offset", [16, 240])
@pytest.mark.parametrize("M,N,B,tdt", [(65, 17, 64, F64), (129, 33, 3, F32), (769, 130, 64, F32)])
def test_paths_at_the_alignments_the_header_states(M, N, B, tdt, ws_offset, subseq_form):
    """(c) for the path-only calls: the stores are rts_dtw's (see there) plus scalar ones to total, start and end and
    8-byte ones to row_dev (sdp::last_row_min)."""
    fill = FILLS[2] if ws_offset == 16 else FILLS[1]
    out = _run_paths(M, N, B, tdt, fill, subseq_form, offsets=True, ws_offset=ws_offset)
    _check_paths(out, M, N, B, tdt, fill, subseq_form, "ws + %d" % ws_offset)


def test_misaligned_outputs_are_refused():
    """The two outputs whose stores are wider than their element type, and a workspace below 16 bytes: RTS_ERR_INVALID
    naming the argument, before anything is enqueued (the pointers are never used)."""
    nat = _nat()
    P = ctypes.c_void_p
    nbytes = ctypes.c_size_t(0)
    nat.check(nat.lib.rts_dtw_workspace_bytes(100, 90, 2, ctypes.byref(nbytes)))
    a, b, out, ws = P(4096), P(8192), P(1 << 20), P(1 << 24)
    for path, what in ((P((1 << 22) + 4), b"path_dev must be 8-byte aligned"), (P((1 << 22) + 12), b"path_dev")):
        rc = nat.lib.rts_dtw(a, nat.F32, 100, b, nat.F32, 90, 12, 100, 90, 2, out, out, None, path, out, ws, nbytes.value, None)
        assert rc == INVALID and what in nat.lib.rts_last_error(), nat.lib.rts_last_error()
        rc = nat.lib.rts_dtw_paths(a, nat.F32, 100, None, b, nat.F32, 90, None, 12, 100, 90, 2, path, out, out, ws,
                                   nbytes.value, None)
        assert rc == INVALID and what in nat.lib.rts_last_error(), nat.lib.rts_last_error()
        rc = nat.lib.rts_dtw_subseq_paths(a, nat.F32, 100, None, b, nat.F32, 90, None, 12, 100, 90, 2, path, out, out, out,
                                          out, None, ws, nbytes.value, None)
        assert rc == INVALID and what in nat.lib.rts_last_error(), nat.lib.rts_last_error()
    for bad_ws in (P((1 << 24) + 8), P((1 << 24) + 4), P((1 << 24) + 1)):
        rc = nat.lib.rts_dtw(a, nat.F32, 100, b, nat.F32, 90, 12, 100, 90, 2, out, out, None, P(1 << 22), out, bad_ws,
                             nbytes.value, None)
        assert rc == INVALID and b"16-byte aligned" in nat.lib.rts_last_error(), nat.lib.rts_last_error()
    from real_time_audio_sync_amd.chroma import ChromaPlan
    plan = ChromaPlan(64, 32, 22050)
    try:
        x = torch.zeros(64, dtype=F32, device=DEV)
        stft = torch.zeros((2, 33, 2), dtype=F64, device=DEV)
        rc = nat.lib.rts_chroma_frames(plan._h, x.data_ptr(), nat.F32, 64, 0, 1, 1, None, nat.F64, stft.data_ptr() + 8, _stream())
        assert rc == INVALID and b"stft_out_dev must be 16-byte aligned" in nat.lib.rts_last_error()
        torch.cuda.synchronize()
        assert not stft.any()
    finally:
        plan.close()


# ---- chroma -------------------------------------------------------------------------------------------------------------
def _chroma_case(L, nf):
    """nf centred frames of hop L / 2 over seeded noise, and the numpy oracle's STFT and chroma of them."""
    from oracle import chroma_oracle as co
    H = L // 2
    x = (np.random.RandomState(L + nf).rand((nf - 1) * H + L - L // 2) - 0.5).astype(np.float32)
    ost = co.create_stft(x, L, H)
    assert ost.shape == (L // 2 + 1, nf)
    och = co.l2_normalize_columns(np.dot(co.chroma_filterbank(22050, L), np.abs(ost) ** 2))
    return x, ost, och


@pytest.mark.parametrize("L", [64, 4096, 8192])
def test_chroma_frames_confined_and_independent_of_stale_contents(L):
    """rts_chroma_frames: one frame and one more than a workgroup takes per pass (kChromaFR, kBigFR for fft_len 8192), so
    the last pass is a partial one; chroma as float64 and float32, with and without the STFT output.  (a) and (b) at
    offset 0, then (c): chroma at 8 / 4 mod 16 (scalar stores, project_normalize), the STFT 16 bytes past a 512-byte
    boundary (one 16-byte store per bin: below 16 bytes it is refused, test_misaligned_outputs_are_refused)."""
    from real_time_audio_sync_amd.chroma import ChromaPlan
    nat = _nat()
    per_pass = K_BIG_FR if L > 4096 else K_CHROMA_FR
    plan = ChromaPlan(L, L // 2, 22050)
    try:
        for nf in (1, per_pass + 1):
            x, ost, och = _chroma_case(L, nf)
            xd = torch.from_numpy(x).to(DEV)
            scale = np.abs(ost).max(axis=0, keepdims=True)
            first = {}
            for fill, offsets in [(f, False) for f in FILLS] + [(FILLS[1], True)]:
                for out_dt, want_stft in ((F64, True), (F32, False), (F64, False), (F32, True)):
                    bufs = _Bufs(fill, offsets)
                    ch = bufs.new("chroma", (nf, 12), out_dt)
                    st = bufs.new("stft", (nf, L // 2 + 1, 2), F64, 16 if offsets else 0) if want_stft else None
                    nat.check(nat.lib.rts_chroma_frames(plan._h, xd.data_ptr(), nat.F32, len(x), L // 2, nf, 1, ch,
                                                        _code(out_dt), st, _stream()))
                    out = bufs.done()
                    tag = (L, nf, "fill 0x%02X" % fill, offsets, str(out_dt), want_stft)
                    for name, arr in out.items():   # (b): bit-identical whatever the buffers held and wherever they lie
                        ref = first.setdefault((name, out_dt), arr)
                        assert same_bytes(ref, arr), tag + (name,)
                    if out_dt == F64:
                        assert np.abs(out["chroma"].T - och).max() <= CHROMA_ATOL, tag
                    else:   # the float32 form is the float64 value rounded once
                        assert same_bytes(out["chroma"], first[("chroma", F64)].astype(np.float32)), tag
                    if want_stft:
                        got = out["stft"][..., 0] + 1j * out["stft"][..., 1]
                        assert (np.abs(got.T - ost) <= STFT_RTOL * scale).all(), tag
    finally:
        plan.close()


def test_chroma_project_and_diff_confined():
    """rts_chroma_project with a partial last group of frames; rts_chroma_diff with 1 frame (nothing to write), 2 and
    10 007 (a last workgroup with 52 of its 256 threads in range), float64 and float32."""
    from oracle import chroma_oracle as co
    from real_time_audio_sync_amd.chroma import ChromaPlan
    nat = _nat()
    plan = ChromaPlan(4096, 2048, 22050)
    try:
        nf = K_CHROMA_FR + 2
        spec = np.random.RandomState(3).rand(nf, 2049) ** 4
        sd = torch.from_numpy(spec).to(DEV)
        want = co.l2_normalize_columns(np.dot(co.chroma_filterbank(22050, 4096), spec.T))
        first = {}
        for fill, offsets in [(f, False) for f in FILLS] + [(FILLS[2], True)]:
            for out_dt in (F64, F32):
                bufs = _Bufs(fill, offsets)
                ch = bufs.new("chroma", (nf, 12), out_dt)
                nat.check(nat.lib.rts_chroma_project(plan._h, sd.data_ptr(), nf, 1, ch, _code(out_dt), _stream()))
                got = bufs.done()["chroma"]
                assert same_bytes(first.setdefault(out_dt, got), got), (fill, offsets, str(out_dt))
                if out_dt == F64:
                    assert np.abs(got.T - want).max() <= CHROMA_ATOL, (fill, offsets)
                else:
                    assert same_bytes(got, first[F64].astype(np.float32)), (fill, offsets)
        for n in (1, 2, 10007):
            for dt in (F64, F32):
                c = np.random.RandomState(n).rand(n, 12).astype(np.float64 if dt == F64 else np.float32)
                cd = torch.from_numpy(c).to(DEV)
                want = np.clip(np.diff(c, axis=0), 0, np.inf)
                for fill, offsets in [(f, False) for f in FILLS] + [(FILLS[0], True)]:
                    bufs = _Bufs(fill, offsets)
                    out = bufs.new("diff", (max(n - 1, 1), 12), dt)
                    nat.check(nat.lib.rts_chroma_diff(cd.data_ptr(), _code(dt), n, out, _stream()))
                    got = bufs.done()["diff"]
                    if n == 1:
                        assert holds_fill(got, fill), (n, fill)
                    else:
                        assert same_bytes(got, want), (n, str(dt), fill, offsets)
    finally:
        plan.close()


# ---- rts_resample_run ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs_in", [24000, 48000, 11025], ids=["147/160", "147/320", "2/1"])
def test_resample_run_confined_and_independent_of_stale_contents(fs_in):
    """24 kHz, 48 kHz and 11.025 kHz to 22.05 kHz.  B = 3 ragged streams, one of them empty, into an output shorter and one longer than rts_resample_out_len: the
    counts are clamped, samples behind n_out_dev[b] keep the fill.  (c): float32 / int32 outputs at 4 mod 16 (scalar
    stores, resample_tile)."""
    from real_time_audio_sync_amd.chroma import ResamplePlan
    nat = _nat()
    p = ResamplePlan(fs_in)
    try:
        assert (p.L, p.M) == {24000: (147, 160), 48000: (147, 320), 11025: (2, 1)}[fs_in]
        lens = [700, 0, 257]
        xs = [(np.random.RandomState(40 + i).rand(n) - 0.5).astype(np.float32) for i, n in enumerate(lens)]
        buf = np.full((3, 700), np.float32(3.0))    # what lies behind a stream's samples is not signal
        for i, x in enumerate(xs):
            buf[i, :len(x)] = x
        want = [resample_model(x, p.L, p.M, p.taps) for x in xs]
        assert [len(w) for w in want] == [out_len(n, p.L, p.M) for n in lens]
        sd = torch.from_numpy(buf).to(DEV)
        nd = torch.tensor(lens, dtype=I32, device=DEV)
        for n_out_max in (100, len(want[0]) + 8):
            for fill, offsets in [(f, False) for f in FILLS] + [(FILLS[1], True)]:
                bufs = _Bufs(fill, offsets)
                out, n_out = bufs.new("out", (3, n_out_max), F32), bufs.new("n_out", (3,), I32)
                nat.check(nat.lib.rts_resample_run(p._h, sd.data_ptr(), nat.F32, 700, nd.data_ptr(), 3, n_out_max, out,
                                                   n_out, _stream()))
                got = bufs.done()
                for i, w in enumerate(want):
                    n = min(len(w), n_out_max)
                    tag = (fs_in, n_out_max, "fill 0x%02X" % fill, offsets, i)
                    assert got["n_out"][i] == n, tag
                    assert same_bytes(got["out"][i, :n], w[:n]), tag
                    assert holds_fill(got["out"][i, n:], fill), tag + ("samples behind n_out were written",)
    finally:
        p.close()


# ---- rts_otw_path_cost --------------------------------------------------------------------------------------------------
def test_path_cost_confined_and_independent_of_stale_contents():
    """Four streams on their own references, one of which has heard nothing (no path point: n = 0, mean NaN, all of
    costs NaN); K on both sides of a wave and at its bounds; costs_dev given and NULL.  The header defines every cell of
    all three outputs, so nothing keeps the fill.  (c): mean and costs at 8 mod 16, n at 4 mod 16 (scalar stores)."""
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    nat = _nat()
    ns, counts = (8, 20, 70, 130), (20, 0, 64, 250)
    refs = [synth.synth_ref(n, seed=900 + b) for b, n in enumerate(ns)]
    heard = [synth.synth_live(np.concatenate([refs[b]] * 4, axis=1), seed=950 + b, lo=0.45, hi=0.55)[:, :counts[b]]
             for b in range(4)]
    eng = BatchedOTW.with_references(refs, 10, 3, dtype=F32, device=DEV)
    try:
        frames = torch.zeros((4, max(counts), 12), dtype=F32)
        for b, h in enumerate(heard):
            frames[b, :h.shape[1]] = torch.from_numpy(np.ascontiguousarray(h.T)).to(F32)
        eng.push(frames.to(DEV), torch.tensor(counts, dtype=I32, device=DEV))
        paths = [eng.path(b) for b in range(4)]
        assert len(paths[1]) == 0 and min(len(paths[b]) for b in (0, 2, 3)) > 0
        stored = [r.T.astype(np.float32) for r in refs]
        for K in (1, 64, 65, 256):
            want = [path_cost_ref(paths[b], heard[b].T, stored[b], K) for b in range(4)]
            for fill, offsets in [(f, False) for f in FILLS] + [(FILLS[2], True)]:
                for want_costs in (True, False):
                    bufs = _Bufs(fill, offsets)
                    mean, n = bufs.new("mean", (4,), F64), bufs.new("n", (4,), I32)
                    costs = bufs.new("costs", (4, K), F64) if want_costs else None
                    nat.check(nat.lib.rts_otw_path_cost(eng._h, K, mean, n, costs, _stream()))
                    got = bufs.done()
                    for b, (em, en, ec) in enumerate(want):
                        tag = (K, "fill 0x%02X" % fill, offsets, want_costs, b)
                        assert got["n"][b] == en, tag
                        assert (np.isnan(em) and np.isnan(got["mean"][b])) or got["mean"][b] == em, tag
                        if want_costs:
                            assert np.array_equal(got["costs"][b], ec, equal_nan=True), tag
                            assert np.isnan(got["costs"][b, en:]).all(), tag
    finally:
        eng.close()


# ---- the dense mirrors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [10, 45])
def test_dense_mirrors_confined_and_independent_of_stale_contents(c):
    """N = 40, B = 2, caller-owned acc / cost [B][2N][N], as the live mirror (rts_otw_set_dense, then pushes) and as the
    replay (rts_otw_replay_dense).  c = 10: stream 0 hears the piece at a third of its speed and runs out of live rows
    (RTS_LIVE_OVERFLOW: row 2N - 1, the last of its slice, is written), stream 1 hears the piece itself and stops at the
    reference end (column N - 1 is written).  c = 45 is wider than the reference: the tracker expands rows and columns
    together until the reference ends, so stream 0 stops there too, and stream 1, cut short, is still running.  Every
    cell is defined (never-evaluated ones hold the sentinel / -1), so the whole of both matrices is compared."""
    import oracle
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    nat = _nat()
    N = 40
    ref = synth.synth_ref(N, seed=3)
    slow = synth.synth_live(np.concatenate([ref] * 4, axis=1), seed=5, lo=0.3, hi=0.4)[:, :120]
    lives = [slow, np.concatenate([ref, ref], axis=1) if c == 10 else ref[:, :25].copy()]
    want = []
    for lv in lives:
        o = oracle.OtwOracle(ref, c, 3, oracle.OTW, keep_cost=True)
        o.run(lv)
        want.append((o.acc_cost(), o.cost(), o.state["status"], o.path))
    if c == 10:
        assert [w[2] for w in want] == [oracle.LIVE_OVERFLOW, oracle.STOP_REF_END]
        assert (want[0][1][2 * N - 1] != -1).any() and (want[1][1][:, N - 1] != -1).any()
    else:
        assert [w[2] for w in want] == [oracle.STOP_REF_END, oracle.RUNNING] and (want[0][1][:, N - 1] != -1).any()
    eng = BatchedOTW(ref, c, 3, batch=2, dtype=F64, device=DEV)
    try:
        frames, lens = eng.pack(lives, dtype=F64)
        for fill, offsets in [(f, False) for f in FILLS] + [(FILLS[1], True)]:
            tag = (c, "fill 0x%02X" % fill, offsets)
            live = _Bufs(fill, offsets)
            acc, cost = live.new("acc", (2, 2 * N, N), F64), live.new("cost", (2, 2 * N, N), F64)
            nat.check(nat.lib.rts_otw_set_dense(eng._h, acc, cost, _stream()))
            half = frames.shape[1] // 2
            eng.push(frames[:, :half].contiguous(), torch.clamp(lens, max=half))
            eng.push(frames[:, half:].contiguous(), torch.clamp(lens - half, min=0))
            got = live.done()
            replay = _Bufs(fill, offsets)
            racc, rcost = replay.new("acc", (2, 2 * N, N), F64), replay.new("cost", (2, 2 * N, N), F64)
            nat.check(nat.lib.rts_otw_replay_dense(eng._h, None, nat.F64, 0, None, racc, rcost, _stream()))
            again = replay.done()
            for b, (oacc, ocost, status, opath) in enumerate(want):
                assert np.array_equal(eng.path(b), opath) and eng.state(b)["status"] == status, tag + (b,)
                for name, o in (("acc", oacc), ("cost", ocost)):
                    assert same_bytes(got[name][b], o), tag + (b, name, "mirror")
                    assert same_bytes(again[name][b], o), tag + (b, name, "replay")
            nat.check(nat.lib.rts_otw_set_dense(eng._h, None, None, _stream()))   # detach before the buffers go
            torch.cuda.synchronize()
    finally:
        eng.close()
