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
    """Device-resident window / twiddles / filterbank for one (fft_len, hop, fs)."""

    def __init__(self, fft_len=fft_len, hop=hop_size, fs=fs, device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("the chroma kernels need a ROCm GPU (no CPU fallback)")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.fft_len, self.hop, self.fs = int(fft_len), int(hop), int(fs)
        self.n_bins = self.fft_len // 2 + 1
        self.chromafb = filters.chroma_filterbank(fs, self.fft_len)
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


_PLANS = {}
_RESAMPLERS = {}


def _plan(device="cuda:0"):
    key = (fft_len, hop_size, fs, str(device))
    if key not in _PLANS:
        _PLANS[key] = ChromaPlan(fft_len, hop_size, fs, device)
    return _PLANS[key]


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


def wav_to_chroma(path_to_wav, resample=False):
    plan = _plan()
    chroma, _ = plan.frames(_load_dev(path_to_wav, resample, plan), pad_left=fft_len // 2)
    return chroma.t().contiguous().cpu().numpy()


def wav_to_chroma_col(wav_buf, resample=False, fs_in=None):
    """``resample=True``: ``wav_buf`` holds samples at ``fs_in``, as many as resample to exactly ``fft_len``."""
    if resample:
        if fs_in is None:
            raise ValueError("resample=True needs fs_in, the rate of wav_buf")
        wav_buf = _resample(np.asarray(wav_buf, dtype=np.float32), fs_in, fs)
    assert (len(wav_buf) == fft_len)
    plan = _plan()
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


def wav_to_chroma_diff(path_to_wav, resample=False):
    plan = _plan()
    chroma, _ = plan.frames(_load_dev(path_to_wav, resample, plan), pad_left=fft_len // 2)
    return plan.diff(chroma).t().contiguous().cpu().numpy()
