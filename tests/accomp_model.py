"""The steering law of the live accompaniment (include/rtsync.h, rts_live_accompany) restated in plain
Python and composed from the models the suite already trusts: the regression is tempo_model.tail, the audio
warp_model.warp on the anchors the law makes.  Python integers carry every position (exact at any size; the model asserts
the bounds under which the library promises the same integers), Python floats are float64 and every expression is written
in the operation order of the definition, so tests/test_accomp_gpu.py compares bytes.  Nothing here imports the package."""
import math

import numpy as np

import tempo_model as tm
import warp_model as wm

ON, WAIT, FREE, LO, HI, END, FULL, LATE = (1 << i for i in range(8))
MAX_HOP_TRACK, MIN_K, MAX_K, MAX_RATE_PM = 65536, 2, 1024, 4000
LIMIT31, TARGET_LIMIT, POS_LIMIT = 1 << 31, 1 << 52, 1 << 61
SLOTS = 4
NAN = tm.NAN
(OK, BAD_HOP_TRACK, BAD_K, BAD_GLIDE, BAD_LEAD, BAD_RATES, BAD_CHUNK, BAD_ANCHORS, OVERFLOW) = range(9)   # AccompRefusal


class Params(object):
    def __init__(self, H, hop, hop_track, K=16, glide=0, lead=0, rate_min_pm=500, rate_max_pm=2000, chunk_blocks=3, A_max=64):
        self.H, self.hop, self.hop_track, self.K, self.glide, self.lead = H, hop, hop_track, K, glide, lead
        self.rate_min_pm, self.rate_max_pm, self.chunk_blocks, self.A_max = rate_min_pm, rate_max_pm, chunk_blocks, A_max


def chunk_overflows(chunk_blocks, H, hop_track, hop, rate_max_pm):
    Ls = chunk_blocks * H
    return Ls >= LIMIT31 or (Ls * hop_track * rate_max_pm) // (hop * 1000) >= LIMIT31


def params_check(p):
    """csrc/accomp_plan.h, accomp_params_check: the first limit broken, in the order of the table."""
    if not 1 <= p.hop_track <= MAX_HOP_TRACK:
        return BAD_HOP_TRACK
    if not MIN_K <= p.K <= MAX_K:
        return BAD_K
    if not 0 <= p.glide < LIMIT31:
        return BAD_GLIDE
    if not -LIMIT31 < p.lead < LIMIT31:
        return BAD_LEAD
    if p.rate_min_pm < 0 or p.rate_min_pm > p.rate_max_pm or p.rate_max_pm > MAX_RATE_PM or p.rate_max_pm < 1:
        return BAD_RATES
    if p.chunk_blocks < 1:
        return BAD_CHUNK
    if p.A_max < 2:
        return BAD_ANCHORS
    if chunk_overflows(p.chunk_blocks, p.H, p.hop_track, p.hop, p.rate_max_pm):
        return OVERFLOW
    return OK


def track_ok(first, length, origin):
    if first < 0 or length < 0 or first >= POS_LIMIT or length >= POS_LIMIT or first + length >= POS_LIMIT:
        return False
    return -POS_LIMIT < origin < POS_LIMIT and -POS_LIMIT < first + origin < POS_LIMIT


# ---- the law's integers (steps 3, 5, 7 tail, 8) ---------------------------------------------------------------------

def due(fed, base, H, k, chunk_blocks):
    q, cap = (fed - base) // H, k + chunk_blocks
    return min(q, cap), q > cap


def rate_step(Ls, hop_track, hop, rate_pm):
    return (Ls * hop_track * rate_pm) // (hop * 1000)


def nominal(Ls, hop_track, hop):
    return (Ls * hop_track) // hop


def step_raw(tgt, origin, i0, Ls, G):
    d = min(max(tgt + origin - i0, 0), LIMIT31 - 1)
    return (d * Ls) // (Ls + G)


def advance(i0, raw, lo, hi, track_end):
    status, step = 0, raw
    if step < lo:
        step, status = lo, status | LO
    if step > hi:
        step, status = hi, status | HI
    i1 = i0 + step
    stop = max(i0, track_end)
    if i1 > stop:
        i1, status = stop, status | END
    return i1, status


# ---- one stream ------------------------------------------------------------------------------------------------------

class Stream(object):
    """The device state of one stream and the words it publishes.  ``origin`` and ``track_end`` are pool samples
    (first + origin, first + len)."""

    def __init__(self, params):
        self.p = params
        self.armed = False
        self.words = dict(out_total=0, in_pos=0, rate=NAN, blocks=0, status=0)

    def arm(self, origin, track_end):
        self.armed = True
        self.origin, self.track_end = int(origin), int(track_end)
        self.fed, self.base, self.k = 0, -1, 0
        self.out_pos, self.in_pos = [0], [self.origin]
        self.n_out = 0
        self.rate = NAN

    def disarm(self):
        self.armed = False

    def _publish(self, blocks, status):
        self.words = dict(out_total=self.out_pos[-1], in_pos=self.in_pos[-1], rate=self.rate, blocks=blocks, status=status)
        return blocks

    def steer(self, n_b, points, x_limit, y_limit):
        """One feed: ``n_b`` samples appended, ``points`` the tracker's stored path after its push.  -> blocks made due.
        The caller renders them (``render``) or moves ``k`` on itself."""
        p = self.p
        if not self.armed:
            self.words = dict(out_total=0, in_pos=0, rate=NAN, blocks=0, status=0)
            return 0
        fed_prev = self.fed
        self.fed += n_b
        status = ON
        if self.base < 0:
            if not len(points):
                return self._publish(0, status | WAIT)
            self.base = fed_prev
        k_due, late = due(self.fed, self.base, p.H, self.k, p.chunk_blocks)
        if late:
            status |= LATE
        if k_due == self.k:
            return self._publish(0, status)
        if len(self.out_pos) >= p.A_max:
            return self._publish(0, status | FULL)
        o0, i0 = self.out_pos[-1], self.in_pos[-1]
        assert o0 == self.k * p.H, "the invariant of step 4"
        o1 = k_due * p.H
        Ls, G = o1 - o0, p.glide
        lo, hi = rate_step(Ls, p.hop_track, p.hop, p.rate_min_pm), rate_step(Ls, p.hop_track, p.hop, p.rate_max_pm)
        assert Ls * p.hop_track * MAX_RATE_PM < 2 ** 63 and hi < LIMIT31
        slope, at, n = tm.tail(points, p.K, 0.0, x_limit, y_limit)
        raw = None
        if slope == slope and slope > 0.0:
            x_i = int(points[-1][0])
            x1 = float(self.base + o1 + G + p.lead) / float(p.hop)
            y1 = at + slope * (x1 - float(x_i))
            y = y1 * float(p.hop_track)
            if math.isfinite(y) and abs(math.floor(y)) < TARGET_LIMIT:
                raw = step_raw(math.floor(y), self.origin, i0, Ls, G)
        if raw is None:
            raw, status = nominal(Ls, p.hop_track, p.hop), status | FREE
        i1, st = advance(i0, raw, lo, hi, self.track_end)
        status |= st
        self.out_pos.append(o1)
        self.in_pos.append(i1)
        self.n_out = o1
        self.rate = float(i1 - i0) / float(Ls)
        return self._publish(k_due - self.k, status)

    def map_ok(self):
        return wm.map_ok(self.out_pos, self.in_pos, self.n_out)

    def render(self, x, N, D, state, w=None):
        """rts_warp_run with k_count = chunk_blocks on the stream's anchors: -> (audio of the blocks rendered, new state,
        warp status).  ``state``: the renderer's (k, p_prev); the model's k moves with it."""
        if not self.armed or len(self.out_pos) < 2:
            return np.zeros(0, np.float32), state, wm.NO_MAP
        y, state, _ = wm.warp(x, self.out_pos, self.in_pos, self.n_out, N=N, D=D, w=w, state=state, k_count=self.p.chunk_blocks)
        self.k = state[0]
        return y, state, 0
