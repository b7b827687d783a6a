"""The beats-and-labels definition of include/rtsync.h restated in plain Python, for tests/test_annot_cpu.py (which holds
it against evaluate.py and the reference's own numbers) and tests/test_annot_gpu.py (which holds the kernels against it).
Python floats are float64 and every expression below is written in the operation order of the definition, so `==` on
its results is a bit-for-bit comparison.  Nothing here imports the package."""
import bisect
import math

THRESHOLDS = (1, 3, 5, 10)


def lookup(frame, times, beats, frame_seconds, frame0=0):
    """-> (beat | None, seg): the first row i with time <= times[i], by bisection."""
    if frame < 0:
        return None, -1
    time = float(frame + frame0) * frame_seconds
    i = bisect.bisect_left(times, time)          # first i with times[i] >= time
    if i >= len(times):
        return None, -1
    seg = 0 if i == 0 else i - 1
    if i == 0 and times[0] == 0:
        return float(beats[0]), seg
    start = 0.0 if i == 0 else times[i - 1]
    return float(beats[i]) - (times[i] - time) / (times[i] - start), seg


class Sticky(object):
    """The three words of one stream (livenote_live.py:199-202): `if beat: self.beat = beat`, `if mus_label: ...`."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.beat, self.label, self.ref_frame = None, -1, -1

    def feed(self, last_ref_index, times, beats, frame_seconds, frame0=0, label_ok=None):
        """One feed: `last_ref_index` is path[-1][1] of the stream's tracker, None while it has no path point."""
        if last_ref_index is None:
            self.ref_frame = -1
            return
        beat, seg = lookup(last_ref_index, times, beats, frame_seconds, frame0)
        if beat is not None and beat != 0.0:
            self.beat = beat
        if seg >= 0 and (label_ok is None or label_ok[seg]):
            self.label = seg
        self.ref_frame = last_ref_index + frame0

    def words(self):
        return (self.beat, self.label, self.ref_frame)


def pymod1(b):
    r = math.fmod(b, 1.0)
    if r != 0 and r < 0:
        r += 1.0
    return r


def time_of(b, times):
    """get_time on the live table -> seconds, or None where int(b) is no row of it."""
    whole = int(b)                               # toward zero
    if whole < 0 or whole >= len(times):
        return None
    sec = times[whole]
    if whole + 1 < len(times):
        sec += pymod1(b) * (times[whole + 1] - times[whole])
    return sec


def metric(path, live, ref, frame_seconds):
    """`live` / `ref`: (times, beats) of the path's column 0 / column 1.  -> (squared_beat_error, counts[10])."""
    counts = [0] * 10
    err = 0.0
    for l, r in path:
        l_beat = lookup(int(l), live[0], live[1], frame_seconds)[0]
        r_beat = lookup(int(r), ref[0], ref[1], frame_seconds)[0]
        if l_beat is None or r_beat is None or l_beat == 0.0 or r_beat == 0.0:
            continue
        t_r, t_l = time_of(r_beat, live[0]), time_of(l_beat, live[0])
        if t_r is None or t_l is None:
            counts[9] += 1
            continue
        diff = abs(l_beat - r_beat)
        err += diff * diff
        secs = abs(t_r - t_l)
        for q, thr in enumerate(THRESHOLDS):
            if diff > thr:
                counts[1 + q] += 1
            if secs > thr:
                counts[5 + q] += 1
        counts[0] += 1
    return err, counts


def stats(err, counts):
    """The dict of AlignmentError.stats() from the integer counts, or None with count == 0."""
    count = counts[0]
    if count == 0:
        return None
    return dict(count=count, squared_beat_error=err,
                pct_off_beats={t: float(v) / count * 100 for t, v in zip(THRESHOLDS, counts[1:5])},
                pct_off_seconds={t: float(v) / count * 100 for t, v in zip(THRESHOLDS, counts[5:9])})
