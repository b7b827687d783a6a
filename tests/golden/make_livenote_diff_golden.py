#!/usr/bin/env python3
"""Generate tests/golden/livenote_diff_golden.npz by executing the REFERENCE's own code (build container only): its
headline configuration, tests.py:145-163 -- LiveNoteV2(..., chroma_diff=True) on wav_to_chroma_diff features -- with the
live side made the way a microphone makes it (livenote_live.py:185-208).

What runs, all of it the reference's text (tests/golden/make_golden.py::load_reference_module):
  * chroma.py  wav_to_chroma_diff(rubinstein)                       -> ref_seq
               wav_to_chroma_col(data[:4096]); data = data[2048:]   -> the live chroma columns of the rachmaninoff samples
  * numpy      np.clip(np.diff(columns), 0, inf)                    -> the live difference columns (chroma.py:89-90)
  * livenote_v2.py  LiveNoteV2(ref_seq, {'search_band_width': 50, 'max_run_count': 3}, debug_params, chroma_diff=True)
               and the insert loop of tests.py:160-163, stopped at "stop"

chroma.py is Python 2 and imports matplotlib, IPython, librosa and pyaudio at module level, none of which this image has.
The imports are dropped (as make_golden.py does for wtw.py), create_stft's three integer `/` become `//` (as
make_golden.py::make_stft_golden does), and the three librosa functions chroma.py calls -- librosa.load,
librosa.filters.chroma, librosa.util.normalize -- are the restatements of oracle/chroma_oracle.py, whose docstring says
what they are restated from.  The chroma values in this golden therefore rest on those restatements exactly as
otw_golden.npz's chopin group does; everything downstream of them is the reference's own arithmetic.

The live side is run twice: on the samples librosa.load returns for the stereo file, (L + R) / 65536, and on what a
mono PCM16 microphone delivers of them, round((L + R) / 2) / 32768 (keys with the suffix _pcm16) -- half of the samples
are half-integers in PCM16 units, and the rounding moves a few path points, so a PCM16 stream has a golden of its own.

Only data is written: the paths, the end states, column counts and sha256 digests of the float64 feature arrays.

Usage:  python tests/golden/make_livenote_diff_golden.py      (a few seconds)
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, load_reference_module, sha  # noqa: E402
from oracle import chroma_oracle  # noqa: E402

PARAMS = {'search_band_width': 50, 'max_run_count': 3}      # tests.py:140
DEBUG_PARAMS = {'seq': False, 'all': False}                 # tests.py:141


def load_reference_chroma():
    mod = load_reference_module("chroma", drop_imports=("matplotlib", "IPython", "librosa", "pyaudio", "plt.rcParams"))
    src = open(os.path.join(REF, "chroma.py")).read()
    a = src.index("def create_stft(wav):")
    fn_src = src[a:src.index("def create_chroma(", a)]
    assert fn_src.count("/") == 3, "chroma.py:49,53,54 are the only divisions expected"
    exec(compile(fn_src.replace("/", "//"), os.path.join(REF, "chroma.py"), "exec"), mod.__dict__)
    mod.librosa = types.SimpleNamespace(
        load=chroma_oracle.load_wav_mono,
        filters=types.SimpleNamespace(chroma=chroma_oracle.chroma_filterbank),
        util=types.SimpleNamespace(normalize=lambda S, norm, axis: _normalize(S, norm, axis)))
    return mod


def _normalize(S, norm, axis):
    assert norm == 2 and axis == 0
    S = np.asarray(S)
    if S.ndim == 1:                       # wav_to_chroma_col hands create_chroma one column
        return chroma_oracle.l2_normalize_columns(S[:, None])[:, 0]
    return chroma_oracle.l2_normalize_columns(S)


def main():
    chroma = load_reference_chroma()
    lnv2 = load_reference_module("livenote_v2")
    ref_wav = os.path.join(REF, "Songs/chopin/chopin_rubinstein_20b.wav")
    live_wav = os.path.join(REF, "Songs/chopin/chopin_rachmaninoff_20b.wav")
    ref_seq = chroma.wav_to_chroma_diff(ref_wav)
    wav, fs = chroma_oracle.load_wav_mono(live_wav)
    assert fs == 22050
    pcm = np.round(wav * 32768.0).astype(np.int16)
    out = dict(n_ref_cols=np.int32(ref_seq.shape[1]), ref_seq_sha=np.asarray(sha(ref_seq)))
    for suffix, data in (("", wav), ("_pcm16", pcm.astype(np.float32) / np.float32(32768.0))):
        out.update(run_live(chroma, lnv2, ref_seq, data, suffix))
    np.savez_compressed(os.path.join(HERE, "livenote_diff_golden.npz"), **out)


def run_live(chroma, lnv2, ref_seq, data, suffix):
    cols = []
    while len(data) >= chroma.fft_len:                      # livenote_live.py:185-208
        cols.append(chroma.wav_to_chroma_col(data[:chroma.fft_len]))
        data = data[chroma.hop_size:]
    live_chroma = np.stack(cols, axis=1)
    live_seq = np.clip(np.diff(live_chroma), 0, float('inf'))
    with contextlib.redirect_stdout(io.StringIO()):
        ln = lnv2.LiveNoteV2(ref_seq, PARAMS, DEBUG_PARAMS, chroma_diff=True)
        consumed, stopped = 0, 0
        for i in range(live_seq.shape[1]):                  # tests.py:160-163
            cont = ln.insert(live_seq[:, i])
            consumed += 1
            if cont == "stop":
                stopped = 1
                break
    path = np.array(ln.path, dtype=np.int32).reshape(-1, 2)
    out = dict(path=path, live_ptr=np.int32(ln.live_ptr), ref_ptr=np.int32(ln.ref_ptr), stopped=np.int32(stopped),
               consumed=np.int32(consumed), n_live_chroma_cols=np.int32(live_chroma.shape[1]),
               n_live_cols=np.int32(live_seq.shape[1]), live_cols_sha=np.asarray(sha(live_seq)),
               live_chroma_sha=np.asarray(sha(live_chroma)))
    print("%-6s path %d  live_ptr=%d ref_ptr=%d  stop=%d  consumed %d of %d live columns, ref %d columns"
          % (suffix, len(path), ln.live_ptr, ln.ref_ptr, stopped, consumed, live_seq.shape[1], ref_seq.shape[1]))
    return {k + suffix: v for k, v in out.items()}


if __name__ == "__main__":
    main()
