"""Drop-in for the reference's chroma.py (module-level API and constants kept):
``wav_to_chroma(path)``, ``wav_to_chroma_col(buf)``, ``create_stft(wav)``,
``create_chroma(ft, normalize=True)``, ``wav_to_chroma_diff(path)``; arrays are feature-major
(12, M) / (2049, M) like the reference's.  Computation: csrc/chroma.hip.

``resample(samples, fs_in)`` and the ``resample=True`` keyword of the file entry points stand where librosa.load's
silent resampling to 22 050 Hz stands in the reference (chroma.py:27): csrc/resample.hip."""
import ctypes

import numpy as np
import torch

from . import _native as nat
from . import filters

# globals (chroma.py:20-22)
fft_len = 4096
hop_size = 2048
fs = 22050


class ChromaPlan(object):
    """Device-resident window / twiddles / filterbank for one (fft_len, hop, fs).  ``tuning``: None uploads the table
    for A4 = 440 Hz; a float c the one for a source c cents from it, ``filters.chroma_filterbank(fs, fft_len,
    a440=filters.tuning_a440(c))``.  ``self.tuning`` and ``self.chromafb`` say which."""

    def __init__(self, fft_len=fft_len, hop=hop_size, fs=fs, device="cuda:0", tuning=None):
        if not torch.cuda.is_available():
            raise RuntimeError("the chroma kernels need a ROCm GPU (no CPU fallback)")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.fft_len, self.hop, self.fs = int(fft_len), int(hop), int(fs)
        self.n_bins = self.fft_len // 2 + 1
        self.tuning = None if tuning is None else float(tuning)
        if self.tuning is not None and not np.isfinite(self.tuning):
            raise ValueError("tuning must be None or a finite number of cents (got %r)" % (tuning,))
        if self.tuning is None:
            self.chromafb = filters.chroma_filterbank(fs, self.fft_len)
        else:
            self.chromafb = filters.chroma_filterbank(fs, self.fft_len, a440=filters.tuning_a440(self.tuning))
        win = filters.hann_window(self.fft_len)
        h = ctypes.c_void_p()
        nat.check(nat.lib.rts_chroma_create(self.fft_len, self.hop, win.ctypes.data, self.chromafb.ctypes.data,
                                            ctypes.byref(h)))
        self._h = h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            nat.destroy_on(self.device, nat.lib.rts_chroma_destroy, h)

    __del__ = close

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def num_frames(self, n_samples, pad_left):
        return int(nat.lib.rts_chroma_num_frames(int(n_samples), self.fft_len, self.hop, int(pad_left)))

    @nat.on_device
    def frames(self, samples_dev, pad_left, normalize=True, out_dtype=torch.float64, want_stft=False,
               want_chroma=True, n_frames=None):
        """samples_dev: 1-D float32/float64 device tensor.  Returns (chroma [M][12] or None,
        stft [M][n_bins] complex128 or None), asynchronous on the current stream."""
        assert samples_dev.dim() == 1 and samples_dev.is_contiguous()
        n = samples_dev.numel()
        m = self.num_frames(n, pad_left) if n_frames is None else int(n_frames)
        chroma = torch.empty((m, 12), dtype=out_dtype, device=self.device) if want_chroma else None
        stft = torch.empty((m, self.n_bins, 2), dtype=torch.float64, device=self.device) if want_stft else None
        if m > 0:
            nat.check(nat.lib.rts_chroma_frames(
                self._h, samples_dev.data_ptr(), nat.F64 if samples_dev.dtype == torch.float64 else nat.F32, n,
                int(pad_left), m, int(bool(normalize)), chroma.data_ptr() if want_chroma else None,
                nat.F64 if out_dtype == torch.float64 else nat.F32, stft.data_ptr() if want_stft else None,
                self._stream()))
        return chroma, (torch.view_as_complex(stft) if want_stft else None)

    @nat.on_device
    def frames_batch(self, samples_dev, n_samples_dev, n_frames_dev, n_frames_max, pad_left=0, normalize=True,
                     out_dtype=torch.float64):
        """B sample buffers at once: samples_dev [B][stride] float32/64, n_samples_dev / n_frames_dev int32 [B].
        Returns chroma [B][n_frames_max][12] (rows beyond n_frames_dev[b] are left untouched)."""
        assert samples_dev.dim() == 2 and samples_dev.is_contiguous()
        B, stride = samples_dev.shape
        out = torch.zeros((B, int(n_frames_max), 12), dtype=out_dtype, device=self.device)
        if n_frames_max > 0:
            nat.check(nat.lib.rts_chroma_frames_batch(
                self._h, samples_dev.data_ptr(), nat.F64 if samples_dev.dtype == torch.float64 else nat.F32, stride,
                n_samples_dev.data_ptr(), int(pad_left), B, int(n_frames_max), n_frames_dev.data_ptr(),
                int(bool(normalize)), out.data_ptr(), nat.F64 if out_dtype == torch.float64 else nat.F32,
                self._stream()))
        return out

    @nat.on_device
    def project(self, spec_dev, normalize=True, out_dtype=torch.float64):
        """spec_dev: [M][n_bins] float64 power spectrum on the device -> chroma [M][12]."""
        assert spec_dev.dtype == torch.float64 and spec_dev.is_contiguous() and spec_dev.shape[1] == self.n_bins
        m = spec_dev.shape[0]
        out = torch.empty((m, 12), dtype=out_dtype, device=self.device)
        if m > 0:
            nat.check(nat.lib.rts_chroma_project(self._h, spec_dev.data_ptr(), m, int(bool(normalize)),
                                                 out.data_ptr(), nat.F64 if out_dtype == torch.float64 else nat.F32,
                                                 self._stream()))
        return out

    @nat.on_device
    def diff(self, chroma_dev):
        m = chroma_dev.shape[0]
        out = torch.empty((max(m - 1, 0), 12), dtype=chroma_dev.dtype, device=self.device)
        if m >= 2:
            nat.check(nat.lib.rts_chroma_diff(chroma_dev.data_ptr(),
                                              nat.F64 if chroma_dev.dtype == torch.float64 else nat.F32, m,
                                              out.data_ptr(), self._stream()))
        return out


class ResamplePlan(object):
    """Device-resident filter table for one (fs_in, fs_out): the resampler DESIGN.md defines, taps from
    ``filters.resample_taps``.  Equal rates build no resampler (ValueError)."""

    def __init__(self, fs_in, fs_out=fs, device="cuda:0", **taps_kw):
        if not torch.cuda.is_available():
            raise RuntimeError("the resampling kernels need a ROCm GPU (no CPU fallback)")
        self.L, self.M = filters.resample_ratio(fs_in, fs_out)
        if self.L == self.M:
            raise ValueError("fs_in == fs_out = %d: nothing to resample" % int(fs_out))
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.taps = filters.resample_taps(fs_in, fs_out, **taps_kw)
        self.half = (len(self.taps) - 1) // 2
        h = ctypes.c_void_p()
        nat.check(nat.lib.rts_resample_create(self.L, self.M, self.taps.ctypes.data, self.half, ctypes.byref(h)))
        self._h = h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            nat.destroy_on(self.device, nat.lib.rts_resample_destroy, h)

    __del__ = close

    def out_len(self, n_in):
        """Samples a one-shot run makes of ``n_in``: ceil(n_in * L / M)."""
        return int(nat.lib.rts_resample_out_len(int(n_in), self.L, self.M))

    def avail(self, in_total):
        """Samples a live stream has handed on once it has been fed ``in_total``: max(0, ceil((in_total * L - half) / M))."""
        return int(nat.lib.rts_resample_avail(int(in_total), self.L, self.M, self.half))

    @nat.on_device
    def run(self, samples_dev, n_in_dev=None, out=None):
        """samples_dev: [B][stride] (or 1-D) float32 / int16 device tensor, n_in_dev int32 [B] valid samples per stream
        (None: the whole row).  Returns (out float32 [B][n_out_max], n_out int32 [B]), asynchronous on the current
        stream; ``out`` (optional, [B][n_out_max] float32) is written only up to each stream's n_out."""
        if samples_dev.dim() == 1:
            samples_dev = samples_dev.unsqueeze(0)
        assert samples_dev.dim() == 2 and samples_dev.is_contiguous() and samples_dev.dtype in (torch.float32, torch.int16)
        B, stride = samples_dev.shape
        if n_in_dev is None:
            n_in_dev = torch.full((B,), stride, dtype=torch.int32, device=self.device)
        if out is None:
            out = torch.empty((B, self.out_len(stride)), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == B
        n_out = torch.empty((B,), dtype=torch.int32, device=self.device)
        # a row of zero samples has no address to hand over: the kernel reads nothing of it
        src = samples_dev.data_ptr() if samples_dev.numel() else n_out.data_ptr()
        nat.check(nat.lib.rts_resample_run(
            self._h, src, nat.F32 if samples_dev.dtype == torch.float32 else nat.I16, stride, n_in_dev.data_ptr(), B,
            int(out.shape[1]), out.data_ptr() if out.numel() else None, n_out.data_ptr(), self._stream()))
        return out, n_out

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class TuningPlan(object):
    """The tuning estimator of include/rtsync.h (rts_tuning_*) for one (fft_len, fs): spectral peaks with centres in
    [f_min, f_max] and at least ``thr`` of the frame's largest magnitude are counted by their distance from the nearest
    equal-tempered pitch at A4 = 440 Hz, ``R`` histogram bins to the semitone (``filters.tuning_edges``)."""

    def __init__(self, fft_len=fft_len, fs=fs, f_min=150.0, f_max=4000.0, R=100, thr=0.1, device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("the tuning kernels need a ROCm GPU (no CPU fallback)")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.fft_len, self.fs, self.R = int(fft_len), int(fs), int(R)
        self.n_bins = self.fft_len // 2 + 1
        self.k_lo, self.k_hi, self.edges = filters.tuning_edges(fs, self.fft_len, f_min, f_max, self.R)
        self.bin_hz = float(fs) / self.fft_len
        self.thr_pow = float(thr) * float(thr)
        h = ctypes.c_void_p()
        nat.check(nat.lib.rts_tuning_create(self.fft_len, self.k_lo, self.k_hi, self.R, len(self.edges),
                                            self.edges.ctypes.data, self.bin_hz, self.thr_pow, ctypes.byref(h)))
        self._h = h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            nat.destroy_on(self.device, nat.lib.rts_tuning_destroy, h)

    __del__ = close

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @nat.on_device
    def accumulate(self, stft_dev, seg_dev=None, hist=None, S=1):
        """Adds the peaks of ``stft_dev`` ([M][n_bins] complex128 as ``ChromaPlan.frames(want_stft=True)`` returns it) to
        ``hist`` ([S][R] int64 on the device; None makes a zeroed one): frame m to row ``seg_dev[m]`` (int32 [M], a value
        outside [0, S) drops the frame), every frame to row 0 without ``seg_dev``.  Returns ``hist``; asynchronous."""
        if stft_dev.is_complex():
            stft_dev = torch.view_as_real(stft_dev)
        assert stft_dev.dtype == torch.float64 and stft_dev.is_contiguous() and tuple(stft_dev.shape[1:]) == (self.n_bins, 2)
        m = int(stft_dev.shape[0])
        if hist is None:
            hist = torch.zeros((int(S), self.R), dtype=torch.int64, device=self.device)
        assert hist.dtype == torch.int64 and hist.is_contiguous() and hist.dim() == 2 and hist.shape[1] == self.R
        if seg_dev is not None:
            assert seg_dev.dtype == torch.int32 and seg_dev.is_contiguous() and seg_dev.numel() == m
        nat.check(nat.lib.rts_tuning_accumulate(self._h, stft_dev.data_ptr() if m else None, m,
                                                seg_dev.data_ptr() if seg_dev is not None and m else None,
                                                int(hist.shape[0]), hist.data_ptr(), self._stream()))
        return hist

    @nat.on_device
    def pick(self, hist, W=5):
        """(cents float64 [S], n int64 [S]) device tensors from ``hist`` [S][R]: the centre of the bin where the circular
        triangular sum of half-width ``W`` bins is largest, and the peaks counted; (0.0, 0) for an empty row."""
        assert hist.dtype == torch.int64 and hist.is_contiguous() and hist.dim() == 2 and hist.shape[1] == self.R
        S = int(hist.shape[0])
        cents = torch.empty((S,), dtype=torch.float64, device=self.device)
        n = torch.empty((S,), dtype=torch.int64, device=self.device)
        nat.check(nat.lib.rts_tuning_pick(self._h, hist.data_ptr(), S, int(W), cents.data_ptr(), n.data_ptr(),
                                          self._stream()))
        return cents, n

    def histogram(self, hist):
        """``hist`` on the host: numpy int64 [S][R]; bin i holds the offsets [-50 + 100 i/R, -50 + 100 (i+1)/R) cents."""
        return hist.cpu().numpy()


_PLANS = {}
_RESAMPLERS = {}
_TUNERS = {}


def _plan(device="cuda:0", tuning=None):
    """The module's plan for ``device`` and ``tuning``, made on first use and kept for the life of the process: one
    filterbank (200 KB on the device) per distinct offset.  ``tuning="auto"`` gives bin centres, so at most R = 100 of
    them; a caller that passes arbitrary per-file floats and must not grow should hold ``ChromaPlan`` objects of its own
    and ``close()`` them.  A tuning that is not finite is refused by ``ChromaPlan`` and never cached."""
    tuning = None if tuning is None else float(tuning)
    key = (fft_len, hop_size, fs, str(device), tuning)
    if key not in _PLANS:
        _PLANS[key] = ChromaPlan(fft_len, hop_size, fs, device, tuning=tuning)
    return _PLANS[key]


def _tuner(device="cuda:0"):
    key = (fft_len, fs, str(device))
    if key not in _TUNERS:
        _TUNERS[key] = TuningPlan(fft_len, fs, device=device)
    return _TUNERS[key]


def resample(samples, fs_in, fs_out=fs, device="cuda:0"):
    """One-shot resampling on the device of mono ``samples`` (float32, or int16 PCM scaled by 1/32768) from ``fs_in`` to
    ``fs_out``: a numpy array gives a numpy array, a tensor a float32 tensor on ``device``.  Equal rates return the
    samples as float32, unchanged."""
    is_tensor = torch.is_tensor(samples)
    x = samples if is_tensor else torch.from_numpy(np.ascontiguousarray(np.asarray(samples)))
    if x.dtype not in (torch.float32, torch.int16):
        x = x.to(torch.float32)
    x = x.reshape(-1).contiguous().to(torch.device(device))
    if int(fs_in) == int(fs_out):
        y = x if x.dtype == torch.float32 else x.to(torch.float32) / 32768.0
    else:
        key = (int(fs_in), int(fs_out), str(device))
        if key not in _RESAMPLERS:
            _RESAMPLERS[key] = ResamplePlan(fs_in, fs_out, device)
        y = _RESAMPLERS[key].run(x)[0][0]
    return y if is_tensor else y.cpu().numpy()


_resample = resample  # the file entry points below have a keyword of that name


def _to_dev(x, plan):
    x = np.ascontiguousarray(np.asarray(x))
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    return torch.from_numpy(x).to(plan.device)


def _load(path_to_wav):
    wav, wav_fs = filters.load_wav(path_to_wav)
    assert (wav_fs == 22050)
    return wav


def _load_dev(path_to_wav, resample_file, plan):
    """The file's samples at 22 050 Hz on the plan's device.  ``resample_file``: a file at another rate is resampled
    there and goes on from there, instead of failing the reference's assertion."""
    if not resample_file:
        return _to_dev(_load(path_to_wav), plan)
    wav, wav_fs = filters.load_wav_native(path_to_wav)
    return _to_dev(wav, plan) if wav_fs == fs else _resample(torch.from_numpy(wav), wav_fs, fs, plan.device)


def _tuning_chunks(plan, tuner, samples_dev, hist, chunk_frames):
    """The STFT of ``samples_dev`` (padded framing, like wav_to_chroma) in chunks of ``chunk_frames`` frames, each chunk's
    peaks added to row 0 of ``hist``.  Frame m starts at sample m * hop - pad, so a chunk that begins at frame m0 > 0 is
    the un-padded framing of the samples from m0 * hop - pad on: the whole STFT never exists at once."""
    if chunk_frames < 1:
        raise ValueError("chunk_frames must be >= 1 (got %d)" % chunk_frames)
    L, H, pad = plan.fft_len, plan.hop, plan.fft_len // 2
    total = plan.num_frames(samples_dev.numel(), pad)
    for m0 in range(0, total, chunk_frames):
        c = min(chunk_frames, total - m0)
        if m0 == 0:
            piece, pad_left = samples_dev[:(c - 1) * H + L - pad], pad
        else:
            piece, pad_left = samples_dev[m0 * H - pad:m0 * H - pad + (c - 1) * H + L], 0
        _, stft = plan.frames(piece, pad_left=pad_left, want_stft=True, want_chroma=False, n_frames=c)
        tuner.accumulate(stft, None, hist)


def _tuning_samples(samples_or_path, fs_in, plan):
    """Mono samples at ``fs`` on the plan's device, from a WAV path (at its own rate) or an array at ``fs_in``."""
    if isinstance(samples_or_path, str):
        x, rate = filters.load_wav_native(samples_or_path)
    else:
        x, rate = samples_or_path, (fs if fs_in is None else int(fs_in))
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if x.dtype == torch.int16:          # PCM16, scaled like the resampler and the live chain scale it
        x = x.to(torch.float32) / 32768.0
    elif x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float32)
    x = x.reshape(-1).contiguous().to(plan.device)
    return x if rate == fs else _resample(x.to(torch.float32), rate, fs, plan.device)


def estimate_tuning(samples_or_path, fs_in=None, chunk_frames=2048, W=5, device="cuda:0"):
    """(cents, n_peaks) of one recording -- a WAV path, or mono samples at ``fs_in`` (None: 22 050 Hz): its offset from
    A4 = 440 Hz, as the centre of a histogram bin one cent wide, and the spectral peaks that voted (0.0 and 0 for
    silence).  Loaded and resampled like ``wav_to_chroma(resample=True)``; the STFT is made and searched on the device
    ``chunk_frames`` frames at a time, and only the result is read back."""
    plan, tuner = _plan(device), _tuner(device)
    x = _tuning_samples(samples_or_path, fs_in, plan)
    hist = torch.zeros((1, tuner.R), dtype=torch.int64, device=plan.device)
    _tuning_chunks(plan, tuner, x, hist, int(chunk_frames))
    cents, n = tuner.pick(hist, W)
    return float(cents.cpu()[0]), int(n.cpu()[0])


def estimate_tuning_batch(list_of_sample_arrays, fs_in=None, chunk_frames=2048, W=5, device="cuda:0"):
    """(cents float64 [B], n_peaks int64 [B]) of B recordings at once, e.g. the sound check of B microphones: the frames
    of all of them one behind the other with a table that says whose each frame is, one ``accumulate`` per
    ``chunk_frames`` of them into a [B][R] histogram, one ``pick``."""
    plan, tuner = _plan(device), _tuner(device)
    B = len(list_of_sample_arrays)
    if B == 0:
        return np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.int64)
    pad, chunk_frames = plan.fft_len // 2, int(chunk_frames)
    if chunk_frames < 1:
        raise ValueError("chunk_frames must be >= 1 (got %d)" % chunk_frames)
    stfts, segs = [], []
    for b, samples in enumerate(list_of_sample_arrays):
        _, stft = plan.frames(_tuning_samples(samples, fs_in, plan), pad_left=pad, want_stft=True, want_chroma=False)
        stfts.append(stft)
        segs.append(torch.full((stft.shape[0],), b, dtype=torch.int32, device=plan.device))
    stft, seg = torch.cat(stfts).contiguous(), torch.cat(segs).contiguous()
    hist = torch.zeros((B, tuner.R), dtype=torch.int64, device=plan.device)
    for m0 in range(0, stft.shape[0], chunk_frames):
        tuner.accumulate(stft[m0:m0 + chunk_frames], seg[m0:m0 + chunk_frames], hist)
    cents, n = tuner.pick(hist, W)
    return cents.cpu().numpy(), n.cpu().numpy()


def _file_tuning(tuning, path_to_wav):
    """The ``tuning`` keyword of the file entry points: None, a float, or "auto" (estimate_tuning of the file)."""
    if isinstance(tuning, str):
        if tuning != "auto":
            raise ValueError("tuning must be None, a number of cents or 'auto', not %r" % (tuning,))
        return estimate_tuning(path_to_wav)[0]
    return tuning


def wav_to_chroma(path_to_wav, resample=False, tuning=None):
    """``tuning``: None is the filterbank for A4 = 440 Hz; a float that many cents from it; "auto" estimates the file's
    offset first (``estimate_tuning``; a file at another rate then needs ``resample=True`` like the chroma itself)."""
    plan = _plan(tuning=_file_tuning(tuning, path_to_wav))
    chroma, _ = plan.frames(_load_dev(path_to_wav, resample, plan), pad_left=fft_len // 2)
    return chroma.t().contiguous().cpu().numpy()


def wav_to_chroma_col(wav_buf, resample=False, fs_in=None, tuning=None):
    """``resample=True``: ``wav_buf`` holds samples at ``fs_in``, as many as resample to exactly ``fft_len``.
    ``tuning``: None or the offset in cents the filterbank is built for."""
    if resample:
        if fs_in is None:
            raise ValueError("resample=True needs fs_in, the rate of wav_buf")
        wav_buf = _resample(np.asarray(wav_buf, dtype=np.float32), fs_in, fs)
    assert (len(wav_buf) == fft_len)
    plan = _plan(tuning=tuning)
    chroma, _ = plan.frames(_to_dev(np.array(wav_buf), plan), pad_left=0)
    return chroma[0].cpu().numpy()


def create_stft(wav):
    plan = _plan()
    _, stft = plan.frames(_to_dev(wav, plan), pad_left=fft_len // 2, want_stft=True, want_chroma=False)
    return stft.t().contiguous().cpu().numpy()


def create_chroma(ft, normalize=True):
    plan = _plan()
    ft = np.asarray(ft)
    one_col = ft.ndim == 1
    if one_col:
        ft = ft[:, None]
    spec = torch.from_numpy(np.ascontiguousarray((np.abs(ft) ** 2).T.astype(np.float64))).to(plan.device)
    out = plan.project(spec, normalize=normalize).t().contiguous().cpu().numpy()
    return out[:, 0] if one_col else out


def wav_to_chroma_diff(path_to_wav, resample=False, tuning=None):
    """``tuning``: as in ``wav_to_chroma``."""
    plan = _plan(tuning=_file_tuning(tuning, path_to_wav))
    chroma, _ = plan.frames(_load_dev(path_to_wav, resample, plan), pad_left=fft_len // 2)
    return plan.diff(chroma).t().contiguous().cpu().numpy()
