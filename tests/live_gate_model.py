"""The level gate of the live chain (rts_live_gate) restated per stream in plain Python: what the GPU is
held to.  Builds on oracle.chroma_oracle.LiveLoopModel, which is only read: the frames are the model's own ``slices``,
a frame's level is ``math.fsum`` of the exact float64 squares of its float32 samples divided by fft_len (fsum is exact, so
the level is the correctly rounded mean square), and the decision is the recurrence of the definition:

    loud = level >= min_level            (a NaN level compares false: quiet)
    loud:  q = 0, the column passes
    else:  q = min(q + 1, hold + 1), the column passes iff q <= hold

with q = hold + 1 on a fresh or restarted stream.  ``diff``: the chroma-difference rule -- the stream's first chroma
column since create / restart only becomes the carry; the difference column of chroma columns (m - 1, m) is handed on iff
both passed.  Ordinals count the stream's chroma columns since create / restart; a handed column carries the ordinal of
its (later) chroma column."""
import math

import numpy as np


def frame_level(frame):
    a = np.asarray(frame, dtype=np.float64)      # float32 -> float64 is exact, and so is each square
    return math.fsum((a * a).tolist()) / len(a)


def decide(levels, min_level, hold, q):
    """The recurrence over ``levels`` from run length ``q`` -> (pass flags, q afterwards)."""
    passes = []
    for lv in levels:
        if lv >= min_level:
            q = 0
            passes.append(True)
        else:
            q = min(q + 1, hold + 1)
            passes.append(q <= hold)
    return passes, q


class GateStreamModel(object):
    def __init__(self, fft_len, hop_size, min_level, hold, diff=False):
        from oracle.chroma_oracle import LiveLoopModel
        self.min_level, self.hold, self.diff = float(min_level), int(hold), bool(diff)
        self.loop = LiveLoopModel(fft_len, hop_size)
        self.restart()

    def restart(self):
        self.loop.restart()
        self.q = self.hold + 1
        self.prev = False            # the previous chroma column passed (False whenever there is no carry)
        self.has_carry = False
        self.levels = []             # of every chroma column of the run
        self.passes = []
        self.ordinals = []           # of every column handed to the tracker
        self.per_feed = []           # (chroma columns completed, ordinals handed on) of every feed of the run

    def feed(self, samples):
        k0 = len(self.loop.slices)
        self.loop.feed(samples)
        new = [frame_level(s) for s in self.loop.slices[k0:]]
        passes, self.q = decide(new, self.min_level, self.hold, self.q)
        handed = []
        for i, p in enumerate(passes):
            if not self.diff:
                hand = p
            else:
                hand = p and self.prev and self.has_carry
                self.has_carry = True
            self.prev = p
            if hand:
                handed.append(k0 + i)
        self.levels += new
        self.passes += passes
        self.ordinals += handed
        self.per_feed.append((len(new), handed))
        return handed

    # what rts_live_levels publishes
    @property
    def seen(self):
        return len(self.levels)

    @property
    def passed(self):
        return len(self.ordinals)

    @property
    def open(self):
        return bool(self.passes and self.passes[-1])

    @property
    def level(self):
        return self.levels[-1] if self.levels else float("nan")
