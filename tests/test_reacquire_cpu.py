"""Re-acquiring lost streams (rts_otw_recent / rts_wtw_recent, rts_otw_path_cost, rts_live_watch / rts_live_confidence,
``recent`` / ``path_cost`` / ``locate_recent`` / ``reacquire``) without a GPU: the entry points exist with the header's
signatures, their argument checks answer before the first HIP call, and the SERIAL RESTATEMENTS of their contracts --
``recent_ref`` and ``path_cost_ref`` below, which tests/test_reacquire_gpu.py compares the kernels with bit for bit --
show on the oracle tracker alone what the GPU file's end-to-end case relies on: a stream fed another piece's frames has
the higher mean path cost, and locating its excerpt finds the piece and the bar it really plays."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_locate_cpu import dot_cost, excerpt_case, locate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def recent_ref(frames, M_max, cap, masked=False):
    """The contract of rts_*_recent for one stream.  ``frames`` [n_pushed][12] float64: everything the stream consumed
    since create / reset / its last restart; ``cap``: the history capacity of its own range (2 N_b, 2 M_b).
    -> (out [M_max][12] float64, len)."""
    n = min(len(frames), cap)
    ln = 0 if masked else min(M_max, n)
    out = np.zeros((M_max, 12))
    out[:ln] = np.asarray(frames, dtype=np.float64)[n - ln:n]
    return out, ln


def path_cost_ref(path, frames, ref, K, euclid=False):
    """The contract of rts_otw_path_cost for one stream.  ``path``: the stored (t, j) pairs in recording order;
    ``frames`` [n][12] float64: the stream's history; ``ref`` [N][12]: its current reference range, float32 or float64
    (widened exactly).  Every cost through the oracle's own cell cost (orc_dot_strided / orc_euclid, live first as in the
    oracle tracker), the mean as the sequential float64 sum, oldest first, over (double)n.  A tracker that was fed NaN
    columns may record points outside its history or range; such a point costs NaN.
    -> (mean, n, costs [K] with NaN behind the n-th)."""
    import oracle.binding as ob
    L = ob.lib()
    frames = np.ascontiguousarray(frames, dtype=np.float64)
    ref = np.ascontiguousarray(np.asarray(ref).astype(np.float64))
    n = min(K, len(path))
    costs = np.full(K, np.nan)
    total = 0.0
    for k, (t, j) in enumerate(path[len(path) - n:]):
        if 0 <= t < len(frames) and 0 <= j < len(ref):      # (a point outside the history or the range costs NaN)
            a, b = frames.ctypes.data + 96 * int(t), ref.ctypes.data + 96 * int(j)
            costs[k] = L.orc_euclid(a, b, 12) if euclid else 1.0 - L.orc_dot_strided(a, b, 12)
        total = total + float(costs[k])
    return (total / float(n) if n else float("nan")), n, costs


def lost_case():
    """The end-to-end case of the GPU file: the pieces and the excerpt of test_locate_cpu.excerpt_case(); stream "good"
    follows piece 0 and hears synth_live(piece 0), stream "lost" is assigned piece 0 and hears the 64 excerpt frames cut
    from piece 1.  -> (pieces, {"good": (12, T) frames, "lost": (12, 64) frames}, A)."""
    from real_time_audio_sync_amd import synth
    pieces, q, A = excerpt_case()
    return pieces, {"good": synth.synth_live(pieces[0], seed=5), "lost": q}, A


def oracle_path(ref, live, c=50, max_run_count=3):
    import oracle.binding as ob
    o = ob.OtwOracle(ref, c, max_run_count, variant=ob.OTW, cost=ob.COST_DOT)
    o.run(live)
    return o.path, o


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


RECENT = ["int M_max", "double *out_dev", "int32_t *len_dev", "const uint8_t *mask_dev", "void *stream"]
DECLS = {
    "rts_otw_recent": ["rts_otw *h"] + RECENT,
    "rts_wtw_recent": ["rts_wtw *h"] + RECENT,
    "rts_otw_path_cost": ["rts_otw *h", "int K", "double *mean_dev", "int32_t *n_dev", "double *costs_dev", "void *stream"],
    "rts_live_watch": ["rts_live *h", "int K"],
    "rts_live_confidence": ["rts_live *h", "double *mean_cost", "int32_t *n_points", "int *feeds_done"],
}


def test_header_declares_exports_binding_and_methods(nat):
    txt = open(os.path.join(ROOT, "include", "rtsync.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    so = ctypes.CDLL(nat.SO_PATH)
    for name, args in DECLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, "include/rtsync.h does not declare %s" % name
        assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == args, name
        assert hasattr(so, name), name
        fn = nat.EXPORTS[name]
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(args), name
    from real_time_audio_sync_amd import _handle, live, otw_batch, wtw
    for cls in (otw_batch.BatchedOTW, wtw.BatchedWTW):
        for meth in ("recent", "locate_recent", "reacquire"):
            assert callable(getattr(cls, meth)) and getattr(cls, meth) is getattr(_handle._BatchedHandle, meth)
    assert callable(otw_batch.BatchedOTW.path_cost) and not hasattr(wtw.BatchedWTW, "path_cost")
    for meth in ("watch", "confidence", "locate_recent", "reacquire"):
        assert callable(getattr(live.LiveSession, meth)), meth


def test_argument_errors_come_before_any_hip_call(nat):
    p = ctypes.c_void_p(4096)              # never dereferenced: every call below is refused on the host
    hbuf = ctypes.create_string_buffer(4096)   # stands in for a handle: the checks below come before anything reads it
    h = ctypes.cast(hbuf, ctypes.c_void_p)

    def call(fn, *args):
        nat.lib.rts_otw_set_waves(None, 4)    # leaves another message behind
        rc = getattr(nat.lib, fn)(*args)
        return rc, nat.lib.rts_last_error()

    for fn in ("rts_otw_recent", "rts_wtw_recent"):
        rc, msg = call(fn, None, 64, p, p, None, None)
        assert rc == -1 and b"handle" in msg, (fn, rc, msg)
        rc, msg = call(fn, h, 64, None, p, None, None)
        assert rc == -1 and b"out_dev" in msg, (fn, rc, msg)
        rc, msg = call(fn, h, 64, p, None, None, None)
        assert rc == -1 and b"len_dev" in msg, (fn, rc, msg)
        rc, msg = call(fn, h, 0, p, p, None, None)
        assert rc == -1 and b"M_max" in msg, (fn, rc, msg)
        rc, msg = call(fn, h, 257, p, p, None, None)
        assert rc == -2 and b"M_max" in msg, (fn, rc, msg)
    rc, msg = call("rts_otw_path_cost", None, 64, p, p, None, None)
    assert rc == -1 and b"handle" in msg, (rc, msg)
    rc, msg = call("rts_otw_path_cost", h, 64, None, p, None, None)
    assert rc == -1 and b"mean_dev" in msg, (rc, msg)
    rc, msg = call("rts_otw_path_cost", h, 64, p, None, None, None)
    assert rc == -1 and b"n_dev" in msg, (rc, msg)
    for K in (0, 257):
        rc, msg = call("rts_otw_path_cost", h, K, p, p, None, None)
        assert rc == -1 and b"K " in msg, (K, rc, msg)
    for K in (0, 16, 300):
        rc, msg = call("rts_live_watch", None, K)
        assert rc == -1 and b"handle" in msg, (K, rc, msg)
    rc, msg = call("rts_live_confidence", None, None, None, None)
    assert rc == -1 and b"handle" in msg, (rc, msg)


def test_product_does_not_import_the_oracle():
    for fn in ("_handle.py", "otw_batch.py", "wtw.py", "live.py", "locate.py", "_native.py", "csrc/otw.hip", "csrc/wtw.hip",
               "csrc/live.hip", "csrc/cost.h", "csrc/otw_device.h", "csrc/otw_stamps.h", "csrc/otw_fill.h", "csrc/otw_host.h",
               "csrc/otw_backward.h"):
        src = open(os.path.join(ROOT, "real_time_audio_sync_amd", fn)).read()
        assert "import oracle" not in src and "from oracle" not in src and "liboracle" not in src, fn
    tool = open(os.path.join(ROOT, "tools", "bench_live.py")).read()
    assert "import oracle" not in tool and "from oracle" not in tool


def test_restatement_of_recent():
    fr = np.arange(20 * 12, dtype=np.float64).reshape(20, 12)
    out, ln = recent_ref(fr, 8, 40)
    assert ln == 8 and np.array_equal(out, fr[12:20])
    out, ln = recent_ref(fr, 64, 16)                    # pushed past the capacity: frames 0 .. 15 are the history
    assert ln == 16 and np.array_equal(out[:16], fr[:16]) and not out[16:].any()
    out, ln = recent_ref(fr[:0], 4, 16)
    assert ln == 0 and not out.any()
    out, ln = recent_ref(fr, 4, 40, masked=True)
    assert ln == 0 and not out.any()


def test_lost_stream_has_the_higher_mean_path_cost():
    """Case A.  Oracle tracker, c = 50, max_run_count = 3, variant otw, dot cost, K = 32."""
    pieces, heard, _ = lost_case()
    means = {}
    for name, live in heard.items():
        path, _ = oracle_path(pieces[0], live)
        mean, n, costs = path_cost_ref(path, live.T, pieces[0].T, 32)
        assert n == 32 and np.isfinite(costs).all(), (name, n)
        s = 0.0
        for v in costs:
            s += float(v)
        assert mean == s / 32.0
        means[name] = mean
    print("mean path cost at K = 32: good %.6f, lost %.6f" % (means["good"], means["lost"]))
    assert means["lost"] > means["good"], means


def test_reacquiring_the_lost_stream_by_the_restatement():
    """Case B.  The excerpt the lost stream heard is located on piece 1 within 8 frames of where it was cut out; the
    tracker restarted there and fed the same 64 frames follows with a lower mean path cost than it had when lost."""
    pieces, heard, A = lost_case()
    out, ln = recent_ref(heard["lost"].T, 64, 2 * pieces[0].shape[1])
    assert ln == 64 and np.array_equal(out, heard["lost"].T)
    res = [locate_ref(dot_cost(out[:ln].T, p))[:3] for p in pieces]
    k = min(range(3), key=lambda i: (res[i][0], i))
    cost, end, start = res[k]
    assert k == 1 and abs(start - A) <= 8, (k, start)
    path, _ = oracle_path(pieces[1][:, start:], heard["lost"])
    mean_after = path_cost_ref(path, heard["lost"].T, pieces[1][:, start:].T, 32)[0]
    lost_path, _ = oracle_path(pieces[0], heard["lost"])
    mean_lost = path_cost_ref(lost_path, heard["lost"].T, pieces[0].T, 32)[0]
    assert mean_after < mean_lost, (mean_after, mean_lost)


def test_restatement_edge_cases():
    rs = np.random.RandomState(3)
    fr = rs.rand(10, 12)
    ref32 = rs.rand(7, 12).astype(np.float32)
    path = np.array([[0, 0], [1, 0], [2, 1], [3, 3]], dtype=np.int32)
    mean, n, costs = path_cost_ref(path, fr, ref32, 3)
    assert n == 3 and mean == ((float(costs[0]) + float(costs[1])) + float(costs[2])) / 3.0
    mean, n, costs = path_cost_ref(path, fr, ref32, 6, euclid=True)
    assert n == 4 and np.isnan(costs[4:]).all() and np.isfinite(costs[:4]).all()
    assert abs(costs[3] - np.sqrt(((fr[3] - ref32[3].astype(np.float64)) ** 2).sum())) < 1e-12
    mean, n, costs = path_cost_ref(path[:0], fr, ref32, 4)
    assert n == 0 and np.isnan(mean) and np.isnan(costs).all()
    fr[2, 5] = np.nan
    mean, n, costs = path_cost_ref(path, fr, ref32, 4)
    assert np.isnan(mean) and np.isnan(costs[2]) and np.isfinite(costs[[0, 1, 3]]).all()
