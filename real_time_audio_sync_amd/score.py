"""Following a score instead of a recording: note lists to reference chroma and beat tables.

``Score`` holds what a standard MIDI file (or a caller's own note list) says: ticks, tempo map, time signatures, notes.
``ScorePlan`` turns the notes of many scores into reference chroma on the device (csrc/score.hip; include/rtsync.h,
rts_score_create, has the definition to the bit), modelling what the chroma chain makes of sounding notes: the Gaussian
filterbank and its octave weighting, the overtones, the 4096-sample Hann window and, optionally, the decay of a struck
string.  ``Score.beat_table`` gives the score's own metre as a ground-truth table, so a piece needs neither a recording nor
a hand-made beat CSV.  ``references(scores, plan)`` is both at once.

The reference project follows recordings only; nothing here has a counterpart in it."""
import ctypes
import struct
from fractions import Fraction

import numpy as np

from . import filters

MICRO = 10 ** 6
PERCUSSION_CHANNEL = 9   # "channel 10", counted from 0
SUSTAIN = 64             # the controller number of the right pedal


# ---- standard MIDI files ------------------------------------------------------------------------------------------------
def _vlq(b, i):
    v = 0
    while True:
        c = b[i]
        i += 1
        v = (v << 7) | (c & 0x7F)
        if not c & 0x80:
            return v, i


def _track_events(b, i, end, track):
    """Events of one MTrk chunk: (tick, track, seq, kind, ...) with kind 'meta' (type, data) or 'ch' (status high nibble,
    channel, data1, data2)."""
    tick, status, seq, out = 0, None, 0, []
    while i < end:
        d, i = _vlq(b, i)
        tick += d
        c = b[i]
        if c == 0xFF:
            typ = b[i + 1]
            n, i = _vlq(b, i + 2)
            out.append((tick, track, seq, "meta", typ, bytes(b[i:i + n])))
            i += n
            status = None
            if typ == 0x2F:
                break
        elif c in (0xF0, 0xF7):
            n, i = _vlq(b, i + 1)
            i += n
            status = None
        else:
            if c & 0x80:
                status = c
                i += 1
            elif status is None:
                raise ValueError("MIDI track %d: a data byte without a status byte before it" % track)
            kind = status & 0xF0
            n = 1 if kind in (0xC0, 0xD0) else 2
            d1 = b[i]
            d2 = b[i + 1] if n == 2 else 0
            i += n
            out.append((tick, track, seq, "ch", kind, status & 0x0F, d1, d2))
        seq += 1
    return out


def _midi_events(data):
    b = memoryview(bytes(data))
    if len(b) < 14 or bytes(b[:4]) != b"MThd":
        raise ValueError("not a standard MIDI file (no MThd header)")
    hlen, fmt, ntrks, division = struct.unpack(">IHHH", b[4:14])
    if fmt not in (0, 1):
        raise ValueError("MIDI format %d is not supported (formats 0 and 1 are)" % fmt)
    if division & 0x8000:
        raise ValueError("SMPTE time division is not supported: the file must count ticks per quarter note")
    if division < 1:
        raise ValueError("MIDI header: ticks per quarter note must be >= 1")
    i, events, track = 8 + hlen, [], 0
    try:
        while i + 8 <= len(b) and track < ntrks:
            tag, n = bytes(b[i:i + 4]), struct.unpack(">I", b[i + 4:i + 8])[0]
            i += 8
            if tag == b"MTrk":
                if i + n > len(b):
                    raise IndexError
                events += _track_events(b, i, i + n, track)
                track += 1
            i += n
    except IndexError:
        raise ValueError("MIDI file is truncated (track %d)" % track)
    events.sort(key=lambda e: e[:3])   # by tick, then track, then order inside the track
    return division, events


class Score(object):
    """Ticks, tempo map, time signatures and notes of one piece.

    ``division``: ticks per quarter note.  ``tempos``: [(tick, microseconds per quarter)], the first at tick 0.
    ``timesigs``: [(tick, numerator, denominator)], the first at tick 0.  ``on_tick`` / ``end_tick`` (int64), ``pitch``
    (int32), ``velocity`` (float64): the notes in ascending onset order, ties in the order of the source."""

    def __init__(self, division, tempos, timesigs, on_tick, end_tick, pitch, velocity, beat_times=None, last_tick=None):
        self.division = int(division)
        self.tempos = [(int(t), int(u)) for t, u in tempos] or [(0, 500000)]
        if self.tempos[0][0] != 0:
            self.tempos.insert(0, (0, 500000))
        self.timesigs = [(int(t), int(n), int(d)) for t, n, d in timesigs] or [(0, 4, 4)]
        if self.timesigs[0][0] != 0:
            self.timesigs.insert(0, (0, 4, 4))
        on = np.asarray(on_tick, dtype=np.int64).reshape(-1)
        order = np.argsort(on, kind="stable")
        self.on_tick = on[order]
        self.end_tick = np.asarray(end_tick, dtype=np.int64).reshape(-1)[order]
        self.pitch = np.asarray(pitch, dtype=np.int32).reshape(-1)[order]
        self.velocity = np.asarray(velocity, dtype=np.float64).reshape(-1)[order]
        if not (len(self.on_tick) == len(self.end_tick) == len(self.pitch) == len(self.velocity)):
            raise ValueError("onsets, ends, pitches and velocities must have one length")
        self.beat_times = None if beat_times is None else [float(t) for t in beat_times]
        ends = [int(self.end_tick.max())] if len(self.end_tick) else [0]
        self.last_tick = max(ends + [int(last_tick or 0)])
        # microseconds x division up to the start of every tempo segment
        self._cum = [0]
        for (t0, u0), (t1, _) in zip(self.tempos, self.tempos[1:]):
            self._cum.append(self._cum[-1] + (t1 - t0) * u0)

    # ---- construction -------------------------------------------------------------------------------------------
    @classmethod
    def from_midi(cls, path_or_bytes, pedal=True):
        """Reads a standard MIDI file (a path, or its bytes): formats 0 and 1, running status, note-on with velocity 0
        as note-off, tempo and time-signature meta events.  ``pedal``: controller 64 holds the ends of released notes
        until the pedal comes up or the same pitch is struck again.  A pitch struck while it sounds ends the earlier
        note there.  Channel 10 (percussion) is left out.  SMPTE time division and format 2 raise ValueError."""
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            data = bytes(path_or_bytes)
        else:
            with open(path_or_bytes, "rb") as fh:
                data = fh.read()
        division, events = _midi_events(data)
        tempos, timesigs, notes = [], [], []            # notes: [onset, end, pitch, velocity]
        sounding, held, down = {}, {}, set()             # (channel, pitch) -> index in notes; channels with the pedal down
        last = 0
        for ev in events:
            tick = ev[0]
            last = max(last, tick)
            if ev[3] == "meta":
                typ, d = ev[4], ev[5]
                if typ == 0x51 and len(d) >= 3:
                    tempos.append((tick, (d[0] << 16) | (d[1] << 8) | d[2]))
                elif typ == 0x58 and len(d) >= 2:
                    timesigs.append((tick, d[0], 1 << d[1]))
                continue
            kind, ch, d1, d2 = ev[4:8]
            if kind == 0xB0 and d1 == SUSTAIN and pedal:
                if d2 >= 64:
                    down.add(ch)
                else:
                    down.discard(ch)
                    for key in [k for k in held if k[0] == ch]:
                        notes[held.pop(key)][1] = tick
                continue
            if kind not in (0x80, 0x90) or ch == PERCUSSION_CHANNEL:
                continue
            key = (ch, d1)
            if kind == 0x90 and d2 > 0:
                for table in (sounding, held):
                    if key in table:
                        notes[table.pop(key)][1] = tick
                sounding[key] = len(notes)
                notes.append([tick, None, d1, d2])
            elif key in sounding:
                if ch in down:
                    held[key] = sounding.pop(key)
                else:
                    notes[sounding.pop(key)][1] = tick
        for n in notes:
            if n[1] is None:                             # never released: to the end of the file
                n[1] = last
        # the last of several events on one tick is the one in force
        tempos = list({t: u for t, u in tempos}.items())
        timesigs = [(t,) + nd for t, nd in {t: (n, d) for t, n, d in timesigs}.items()]
        return cls(division, sorted(tempos), sorted(timesigs), [n[0] for n in notes], [n[1] for n in notes],
                   [n[2] for n in notes], [n[3] for n in notes], last_tick=last)

    @classmethod
    def from_notes(cls, onsets_s, ends_s, pitches, velocities, beat_times=None):
        """For callers with their own parser: onsets and ends in seconds (rounded once to whole microseconds, the tick
        of such a score), MIDI pitches, velocities 0..127.  ``beat_times``: the seconds of beats 0, 1, 2, ... for
        ``beat_table``; without them the score has no beats."""
        on = np.rint(np.asarray(onsets_s, dtype=np.float64) * MICRO).astype(np.int64)
        end = np.rint(np.asarray(ends_s, dtype=np.float64) * MICRO).astype(np.int64)
        return cls(MICRO, [(0, MICRO)], [(0, 4, 4)], on, end, pitches, velocities,
                   beat_times=[] if beat_times is None else beat_times)

    # ---- time ---------------------------------------------------------------------------------------------------------
    def _scaled_us(self, tick):
        """Microseconds x division at ``tick`` (an int or a Fraction), through the tempo map."""
        j = 0
        for k, (t, _) in enumerate(self.tempos):
            if t <= tick:
                j = k
        return self._cum[j] + (tick - self.tempos[j][0]) * self.tempos[j][1]

    def seconds(self, tick):
        """The time of ``tick`` as an exact Fraction of a second."""
        return Fraction(self._scaled_us(tick), self.division * MICRO)

    def sample_of(self, tick, fs):
        """floor(seconds(tick) * fs + 1/2) in exact integers."""
        d = self.division * MICRO
        return (2 * self._scaled_us(int(tick)) * int(fs) + d) // (2 * d)

    def samples(self, fs):
        """(onsets, ends) of the notes in samples at ``fs``, int64: ticks x microseconds per quarter through the tempo
        map in exact integer arithmetic, rounded half up.  No float is involved."""
        fs = int(fs)
        on = np.array([self.sample_of(t, fs) for t in self.on_tick.tolist()], dtype=np.int64).reshape(-1)
        end = np.array([self.sample_of(t, fs) for t in self.end_tick.tolist()], dtype=np.int64).reshape(-1)
        return on, end

    def energies(self):
        """(velocity / 127)^2 of every note, float64."""
        return (self.velocity / 127.0) ** 2

    # ---- beats --------------------------------------------------------------------------------------------------------
    def beat_table(self):
        """``(times, beats, labels)`` as ``AnnotationTables`` and ``evaluate.get_beat`` take them: one row per beat of
        the score's own metre from tick 0 to the first beat at or behind the last note's end.  A beat is the note value
        of the time signature's denominator; a change of signature starts a new bar.  Times come through the tempo map
        (exact, then rounded once to float64); beats count from 0; the label is ``"bar N"`` (N from 1) on the first beat
        of a bar and ``""`` elsewhere.  A ``from_notes`` score returns the beat times it was given."""
        if self.beat_times is not None:
            if not self.beat_times:
                raise ValueError("this score was made by from_notes without beat_times: it has no beats")
            return list(self.beat_times), list(range(len(self.beat_times))), [""] * len(self.beat_times)
        times, beats, labels, bar = [], [], [], 0
        for j, (start, num, den) in enumerate(self.timesigs):
            final = j + 1 == len(self.timesigs)
            stop = self.last_tick if final else self.timesigs[j + 1][0]
            if not final and stop <= start:
                continue
            step, tick, i = Fraction(4 * self.division, den), Fraction(start), 0
            while True:
                if i % num == 0:
                    bar += 1
                times.append(float(self.seconds(tick)))
                beats.append(len(beats))
                labels.append("bar %d" % bar if i % num == 0 else "")
                if tick >= stop if final else tick + step >= stop:
                    break
                tick, i = tick + step, i + 1
        return times, beats, labels


# ---- the three host tables ----------------------------------------------------------------------------------------------
DEFAULT_HARMONICS = (1.0, 1.0 / 2, 1.0 / 3, 1.0 / 4, 1.0 / 5)


def tables(fft_len, hop, fs, harmonics=DEFAULT_HARMONICS, half_life_s=None, K=64, tuning=None):
    """(T [128][12], CW [fft_len + 1], DK [K + 1]) float64 for rts_score_create.

    T[p]: the filterbank (``filters.chroma_filterbank``, built for ``filters.tuning_a440(tuning)`` as ``ChromaPlan`` does)
    applied to the power spectrum of the Hann-windowed sum of unit cosines at the harmonics of MIDI pitch p below Nyquist,
    harmonic h at amplitude ``harmonics[h - 1]`` -- what the chroma chain makes of a steady tone -- divided by the
    window's energy.  CW: the cumulative energy of the window, summed in order.  DK[k] = 2^(-k hop / fs / half_life_s),
    all ones for None."""
    L, K = int(fft_len), int(K)
    a440 = 440.0 if tuning is None else filters.tuning_a440(tuning)
    fb = filters.chroma_filterbank(fs, L, a440=a440)
    win = filters.hann_window(L)
    CW = np.zeros(L + 1, dtype=np.float64)
    for n in range(L):
        CW[n + 1] = CW[n] + win[n] * win[n]
    T = np.zeros((128, 12), dtype=np.float64)
    t = np.arange(L, dtype=np.float64) / float(fs)
    for p in range(128):
        f0 = a440 * 2.0 ** ((p - 69) / 12.0)
        x = np.zeros(L, dtype=np.float64)
        for h, amp in enumerate(harmonics, 1):
            if f0 * h < fs / 2.0:
                x += float(amp) * np.cos(2.0 * np.pi * (f0 * h) * t)
        spec = np.abs(np.fft.rfft(x * win)) ** 2
        T[p] = np.dot(fb, spec) / CW[L]
    if half_life_s is None:
        DK = np.ones(K + 1, dtype=np.float64)
    else:
        if not (float(half_life_s) > 0.0):
            raise ValueError("half_life_s must be None or > 0")
        DK = np.exp2(-(np.arange(K + 1, dtype=np.float64) * hop / float(fs)) / float(half_life_s))
    return T, CW, DK


class ScorePlan(object):
    """Device-resident tables for one (fft_len, hop, fs): ``tables(...)`` uploaded once.

    ``harmonics``: amplitudes of the partials 1, 2, ...  ``half_life_s``: the time in which a struck note's energy falls
    to a half -- None for sustained instruments (organ, strings), about 0.12 s suits a piano.  ``K``: frames after the
    onset the decay is followed for (it stays at DK[K] from there).  ``tuning``: cents from A4 = 440 Hz, like
    ``ChromaPlan``.  ``pad_left``: None is fft_len / 2, the centred framing of ``wav_to_chroma``; 0 is the framing of a
    live feed."""

    def __init__(self, fft_len=4096, hop=2048, fs=22050, harmonics=DEFAULT_HARMONICS, half_life_s=None, K=64, tuning=None,
                 device="cuda:0", pad_left=None, host_tables=None):
        import torch

        from . import _native as nat
        if not torch.cuda.is_available():
            raise RuntimeError("the score kernels need a ROCm GPU (no CPU fallback)")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device(self.device.type, torch.cuda.current_device())
        self.fft_len, self.hop, self.fs, self.K = int(fft_len), int(hop), int(fs), int(K)
        self.pad_left = self.fft_len // 2 if pad_left is None else int(pad_left)
        if host_tables is None:
            host_tables = tables(self.fft_len, self.hop, self.fs, harmonics, half_life_s, self.K, tuning)
        self.T, self.CW, self.DK = (np.ascontiguousarray(a, dtype=np.float64) for a in host_tables)
        if self.T.shape != (128, 12) or self.CW.shape != (self.fft_len + 1,) or self.DK.shape != (self.K + 1,):
            raise ValueError("host tables must be T [128][12], CW [fft_len + 1], DK [K + 1]")
        # close() may run while the interpreter shuts down, when nothing can be imported and module globals are gone
        self._destroy_on, self._destroy = nat.destroy_on, nat.lib.rts_score_destroy
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib.rts_score_create(self.fft_len, self.hop, self.pad_left, self.K, self.T.ctypes.data,
                                               self.CW.ctypes.data, self.DK.ctypes.data, ctypes.byref(h)))
        self._h = h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._destroy_on(self.device, self._destroy, h)

    __del__ = close

    def num_frames(self, n_samples):
        """Frames the chroma chain makes of ``n_samples`` samples with this plan's framing."""
        n = int(n_samples) + self.pad_left
        return 0 if n < self.fft_len else (n - self.fft_len) // self.hop + 1

    @staticmethod
    def workspace_bytes(n_notes):
        from . import _native as nat
        b = ctypes.c_size_t()
        nat.check(nat.lib.rts_score_workspace_bytes(int(n_notes), ctypes.byref(b)))
        return int(b.value)

    def run(self, onset, end, pitch, energy, note_first, note_len, frame_first, n_frames, out, normalize=True,
            skipped=None, status=None, workspace=None):
        """The raw call (rts_score_chroma) on device tensors: notes ``onset`` / ``end`` int64, ``pitch`` int32,
        ``energy`` float64; piece tables ``note_first`` / ``frame_first`` int64 [P], ``note_len`` / ``n_frames`` int32
        [P]; ``out`` [n_pool_frames][12] float32 or float64; ``skipped`` / ``status`` int32 [P] or None; ``workspace``
        a uint8 tensor of ``workspace_bytes(n_notes)`` (None allocates one).  Asynchronous on the current stream."""
        import torch

        from . import _native as nat
        n_notes, P = int(onset.numel()), int(note_first.numel())
        for t, dt, what in ((onset, torch.int64, "onset"), (end, torch.int64, "end"), (pitch, torch.int32, "pitch"),
                            (energy, torch.float64, "energy"), (note_first, torch.int64, "note_first"),
                            (note_len, torch.int32, "note_len"), (frame_first, torch.int64, "frame_first"),
                            (n_frames, torch.int32, "n_frames")):
            if t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise TypeError("%s must be a contiguous %s tensor on %s" % (what, dt, self.device))
        if not (end.numel() == pitch.numel() == energy.numel() == n_notes):
            raise ValueError("onset, end, pitch and energy must have one length")
        if not (note_len.numel() == frame_first.numel() == n_frames.numel() == P):
            raise ValueError("the four piece tables must have one length")
        if out.dim() != 2 or out.shape[1] != 12 or not out.is_contiguous() or out.dtype not in (torch.float32, torch.float64):
            raise TypeError("out must be a contiguous [n_pool_frames][12] float32 / float64 tensor")
        if workspace is None:
            workspace = torch.empty((self.workspace_bytes(n_notes),), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(nat.lib.rts_score_chroma(
                self._h, onset.data_ptr() if n_notes else None, end.data_ptr() if n_notes else None,
                pitch.data_ptr() if n_notes else None, energy.data_ptr() if n_notes else None, n_notes,
                note_first.data_ptr(), note_len.data_ptr(), frame_first.data_ptr(), n_frames.data_ptr(), P,
                int(bool(normalize)), out.data_ptr(), nat.F64 if out.dtype == torch.float64 else nat.F32, int(out.shape[0]),
                skipped.data_ptr() if skipped is not None else None, status.data_ptr() if status is not None else None,
                workspace.data_ptr() if workspace.numel() else None, int(workspace.numel()),
                ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

    def chroma(self, scores, dtype=None, normalize=True, n_samples=None):
        """Reference chroma of a list of ``Score`` objects in one call.  ``n_samples``: None frames every score up to its
        last note's end, as ``wav_to_chroma`` would frame a recording that ends there; else one sample count per score.

        Returns ``(pool, first, lens, views)``: the device tensor [n_pool_frames][12] (``dtype``, default float64), the
        device tables int64 [P] / int32 [P] that ``locate`` and ``rts_otw_create_refs`` take, and one feature-major
        ``(12, N_k)`` view of the pool per score.  Raises ValueError when a score holds a note the kernel had to leave
        out (a pitch outside 0..127, a negative onset, an end before its onset).  Synchronises."""
        import torch
        dtype = torch.float64 if dtype is None else dtype
        scores = list(scores)
        if not scores:
            raise ValueError("chroma: no score given")
        parts = [s.samples(self.fs) for s in scores]
        if n_samples is None:
            n_samples = [int(p[1].max()) if len(p[1]) else 0 for p in parts]
        lens = np.array([self.num_frames(n) for n in n_samples], dtype=np.int32)
        first = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
        note_len = np.array([len(p[0]) for p in parts], dtype=np.int32)
        note_first = np.concatenate([[0], np.cumsum(note_len[:-1], dtype=np.int64)]).astype(np.int64)

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

        n_pool = max(int(lens.sum()), 1)
        pool = torch.zeros((n_pool, 12), dtype=dtype, device=self.device)
        skipped = torch.zeros((len(scores),), dtype=torch.int32, device=self.device)
        status = torch.zeros((len(scores),), dtype=torch.int32, device=self.device)
        first_dev, lens_dev = dev(first), dev(lens)
        self.run(dev(np.concatenate([p[0] for p in parts])), dev(np.concatenate([p[1] for p in parts])),
                 dev(np.concatenate([s.pitch for s in scores])), dev(np.concatenate([s.energies() for s in scores])),
                 dev(note_first), dev(note_len), first_dev, lens_dev, pool, normalize, skipped, status)
        skipped, status = skipped.cpu().numpy(), status.cpu().numpy()
        if status.any():
            raise RuntimeError("rts_score_chroma flagged pieces %s" % np.flatnonzero(status).tolist())
        if skipped.any():
            raise ValueError("scores %s hold notes that cannot sound (pitch outside 0..127, a negative onset, an end before "
                             "its onset or a bad velocity): %s of them" % (np.flatnonzero(skipped).tolist(),
                                                                           skipped[skipped > 0].tolist()))
        views = [pool[int(f):int(f) + int(n)].t() for f, n in zip(first, lens)]
        return pool, first_dev, lens_dev, views


def references(scores, plan, dtype=None):
    """``(chroma, beat_tables)`` of a list of scores: ``chroma[k]`` a feature-major (12, N_k) numpy array like
    ``wav_to_chroma`` returns for a recording -- ready for ``BatchedOTW`` / ``BatchedOTW.with_references``,
    ``LiveSession``, ``locate`` and ``dtw.align_pairs``, beside recordings or instead of them -- and ``beat_tables[k]``
    the score's ``beat_table()``, ready for ``AnnotationTables`` and ``EnsembleSession``."""
    _, _, _, views = plan.chroma(scores, dtype)
    return [v.contiguous().cpu().numpy() for v in views], [s.beat_table() for s in scores]
