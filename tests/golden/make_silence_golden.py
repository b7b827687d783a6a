#!/usr/bin/env python3
"""Generate tests/golden/silence_golden.npz by executing the REFERENCE's own code (build container only) on inputs with
digital silence -- all-zero chroma columns (tests/silence_inputs.py).  The other .npz files are not rewritten.

What runs, all of it the reference's text (tests/golden/make_golden.py::load_reference_module, ::run_otw_like):
  * otw_eran.py / livenote.py / livenote_v2.py on silent_pair(2 c + 100, c, ...) for c in {20, 70}: every variant,
    insert loop and set_live, with the dot cost (a zero frame costs exactly 1.0 against everything), and LiveNoteV2 with
    chroma_diff=True (Euclidean cost: zero against zero costs exactly 0, the band minima tie) at both widths;
  * wtw.py's get_cost_matrix / run_dtw / find_path, called unbound, on windows of 70, 130 and 200 frames with silent
    rows / columns at 0, at the last index, at 63/64 and as a run (a zero column makes 0/0 = NaN costs, wtw.py:169).

Only data is written: inputs, paths, end state, the two live accumulated-cost bands, and C / D / B / sub-path of the
windows (C and D whole for the 70-frame windows, as ``digest`` below for the larger ones).  An x86 0/0 is a negative NaN
and the GPU's is a positive one, so users of this file compare with equal_nan=True and never compare NaN bytes.

Usage:  python tests/golden/make_silence_golden.py      (about a minute; the reference is pure Python)
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import load_reference_module, run_otw_like, sha  # noqa: E402
from real_time_audio_sync_amd import synth  # noqa: E402
import silence_inputs  # noqa: E402

# name -> (W, silent rows, silent columns)
WINDOWS = {
    "win70_rows63_64_last": (70, (63, 64, 69), ()),
    "win70_col0_row_last": (70, (69,), (0,)),
    "win70_all_rows": (70, tuple(range(70)), ()),
    "win130_cols63_64_last": (130, (), (63, 64, 129)),
    "win130_row0": (130, (0,), ()),
    "win130_row_run": (130, tuple(range(100, 120)), (129,)),
    "win200_col_run_row_last": (200, (199,), tuple(range(150, 181))),
    "win200_rows63_64_cols127_128": (200, (63, 64), (127, 128)),
}


def digest(A):
    """What is kept of a large float64 matrix: where its NaNs are, the sha256 of its bytes with every NaN replaced by
    0.0 (so no NaN byte is ever compared), its last row and column and a coarse grid of samples."""
    Z = np.where(np.isnan(A), 0.0, A)
    return dict(nan=np.packbits(np.isnan(A)), sha=np.asarray(sha(Z)), last_row=A[-1].copy(), last_col=A[:, -1].copy(),
                grid=A[::7, ::5].copy())


def main():
    np.int = int
    mods = {n: load_reference_module(n) for n in ("otw_eran", "livenote", "livenote_v2")}
    wtw = load_reference_module("wtw", drop_imports=("matplotlib", "IPython", "librosa", "pyaudio", "plt.rcParams")).WTW
    out, meta = {}, []
    for c in (20, 70):
        for euclid in (False, True):
            grp = "c%d_%s" % (c, "euclid" if euclid else "dot")
            ref, lives = silence_inputs.silent_pair(2 * c + 100, c, silence_inputs.otw_seed(c), euclid)
            live = lives[0]
            out[grp + "/ref"], out[grp + "/live"] = ref.astype(np.float32), live.astype(np.float32)
            for variant in ("otw", "livenote", "livenote_v2") if not euclid else ("livenote_v2",):
                for mode in ("insert", "set_live"):
                    cid = "%s_%s_%s" % (grp, variant, mode)
                    r = run_otw_like(mods, variant, ref, live, c, 3, mode, euclid)
                    meta.append("|".join([cid, variant, str(c), "3", mode, str(int(euclid))]))
                    for k in ("path", "t", "j", "direction", "previous", "run_count", "consumed", "stopped", "row_band",
                              "col_band"):
                        out[cid + "/" + k] = np.asarray(r[k])
                    print("%-36s path %5d  t=%d j=%d stop=%d" % (cid, len(r["path"]), r["t"], r["j"], r["stopped"]))
    out["cases"] = np.array(meta)
    wmeta = []
    for cid, (W, rows, cols) in WINDOWS.items():
        r = synth.synth_ref(W + 5, seed=900 + W + len(rows))
        x = synth.synth_live(r, seed=901 + W + len(cols), lo=0.9, hi=1.0)[:, :W].copy()
        y = r[:, :W].copy()
        assert x.shape[1] == W
        x[:, list(rows)] = 0.0
        y[:, list(cols)] = 0.0
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            C = wtw.get_cost_matrix(None, x, y)
            D, B = wtw.run_dtw(None, C)
            sub = np.array(wtw.find_path(None, B), dtype=np.int32)
        # the inputs are float32 values, C and D are kept as float64
        out[cid + "/x"], out[cid + "/y"] = x.astype(np.float32), y.astype(np.float32)
        out[cid + "/B"], out[cid + "/sub"] = B.astype(np.int8), sub
        for k, A in (("C", C), ("D", D)):
            if W <= 70:
                out[cid + "/" + k] = A
            else:   # float64 matrices of 130 and 200 frames would not fit the size limit of a committed file
                out.update({cid + "/" + k + "_" + n: v for n, v in digest(A).items()})
        wmeta.append(cid)
        print("%-36s sub-path %d  NaN share C %.3f D %.3f" % (cid, len(sub), np.isnan(C).mean(), np.isnan(D).mean()))
    out["windows"] = np.array(wmeta)
    fn = os.path.join(HERE, "silence_golden.npz")
    np.savez_compressed(fn, **out)
    print("wrote %s, %d bytes" % (fn, os.path.getsize(fn)))
    assert os.path.getsize(fn) < 1 << 20


if __name__ == "__main__":
    main()
