"""The chroma kernels (csrc/chroma.hip) on the paths tests/test_chroma_gpu.py never reaches: every persistent loop
taking more than one trip with a partial last group, the batched entry point called directly, fft_len 4096 on the
generic kernel (64-bit sample indices), a caller-supplied window, odd / long hops and pads, extreme input scales,
and rts_chroma_diff pinned exactly.

Inputs are seeded synthetic audio (``synth``): sinusoids at musical pitches whose amplitudes swing with periods of
5 to 23 hops, low noise, float32-exact values, and a stretch of exact zeros longer than two frames that starts in
the middle of a frame group.  Adjacent frames differ visibly (asserted), so a frame read from the wrong offset or
written to the wrong row cannot pass.

Reference: oracle/chroma_oracle.py; where it offers no such framing (arbitrary pad_left, custom window) ``ref_frames``
restates it with the same primitives (np.concatenate((zeros(pad), x)), slice, * win, np.fft.rfft, np.dot(fb, |X|^2),
l2_normalize_columns).  np.fft.rfft itself is pinned against a longdouble DFT in tests/test_chroma_oracle_cpu.py, and
the loop and 64-bit cases compare the HIP STFT with that DFT directly as well.  Value gates are those of
tests/test_chroma_gpu.py, imported from there.  The bit-exact checks say in their docstrings why no tolerance is needed.

Largest errors against the oracle observed in these runs on an MI355X (256 CUs), over all frames of all cases
(gates: 1e-11; the tests print each figure on an OBSERVED line before they assert, run with -s):
    kernel                                        STFT |delta| / max|X|    normalised chroma |delta|
    chroma_frames4096_kernel (single and batch)   5.1e-16                  1.3e-15
    chroma_frames_kernel, fft_len 64 .. 2048      4.4e-16                  1.2e-15
    chroma_frames_kernel, fft_len 4096 (64-bit)   4.1e-16                  1.1e-15
    chroma_frames_big_kernel (single and batch)   4.2e-16                  1.2e-15
    chroma_project_kernel                         2.4e-15 (raw, per frame) 1.1e-15
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_chroma_gpu import CHROMA_ATOL, STFT_RTOL  # noqa: E402  (the project's gates, not restated)
from test_chroma_oracle_cpu import dft_bins, longdouble_dft  # noqa: E402

RAW_RTOL = 1e-11    # un-normalised chroma, relative to its max (tests/test_chroma_gpu.py)
F32_ATOL = 1e-6     # float32 output (tests/test_chroma_gpu.py)
FS = 22050
FR, BIG_FR = 4, 2   # frames per group: kChromaFR, kBigFR
BATCH_GRID = 64     # gridDim.x cap of the batched launches
PROJECT_GRID = 1024


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def mods():
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd import chroma
    from oracle import chroma_oracle
    return chroma, chroma_oracle, nat


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- inputs and references --------------------------------------------------------------------------------------------

_MIDI = (60, 64, 67, 72, 76, 81, 57)


def synth(n, hop, seed, zeros=()):
    """float32 samples: seven pitches, each with its own amplitude swing (period 5..23 hops), noise at 1e-3, and exact
    zeros on every [a, b) of ``zeros``."""
    rs = np.random.RandomState(seed)
    i = np.arange(n, dtype=np.float64)
    x = 1e-3 * rs.standard_normal(n)
    for j, m in enumerate(_MIDI):
        f = 440.0 * 2.0 ** ((m - 69) / 12.0)
        period = hop * (5 + 3 * j) + 0.37
        env = 0.5 + 0.45 * np.sin(2 * np.pi * i / period + rs.uniform(0, 2 * np.pi))
        x += 0.12 * env * np.sin(2 * np.pi * f / FS * i + rs.uniform(0, 2 * np.pi))
    for a, b in zeros:
        x[max(a, 0):max(b, 0)] = 0.0
    return x.astype(np.float32)


def zero_stretch(m0, L, hop, pad):
    """Sample range that makes frames m0 .. m0 + nz - 1 exactly zero, nz = 2L/hop + 3: 3L + 2 hop samples."""
    nz = 2 * L // hop + 3
    return (m0 * hop - pad, (m0 + nz - 1) * hop - pad + L), nz


def ref_frames(co, x, L, hop, pad, win, fb, n_frames=None):
    """The reference's framing restated for any pad and window -> (stft [M][nb], raw chroma [M][12], normalised)."""
    xp = np.concatenate((np.zeros(pad), np.asarray(x, dtype=np.float64)))
    fit = (len(xp) - L) // hop + 1 if len(xp) >= L else 0
    m = fit if n_frames is None else n_frames
    assert m <= fit
    st = np.empty((m, L // 2 + 1), dtype=complex)
    for k in range(m):
        st[k] = np.fft.rfft(xp[k * hop:k * hop + L] * win)
    raw = np.dot(fb, (np.abs(st) ** 2).T)
    return st, np.ascontiguousarray(raw.T), np.ascontiguousarray(co.l2_normalize_columns(raw).T)


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex128:
        a = a.view(np.float64)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def bit_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def stft_err(got, want):
    """Per-frame max |delta| over the frame's max |X|; frames whose reference is all zero must be exactly zero."""
    scale = np.abs(want).max(axis=1)
    d = np.abs(got - want).max(axis=1)
    assert (d[scale == 0] == 0).all()
    live = scale > 0
    return float((d[live] / scale[live]).max()) if live.any() else 0.0


def adjacent_frames_differ(ch):
    """Every pair of adjacent chroma rows differs by more than 1e-4 somewhere, unless both are zero rows."""
    d = np.abs(np.diff(ch, axis=0)).max(axis=1)
    both_zero = (np.abs(ch[1:]).max(axis=1) == 0) & (np.abs(ch[:-1]).max(axis=1) == 0)
    return bool((d[~both_zero] > 1e-4).all())


def kernel_name(L, generic=False):
    return "chroma_frames_big_kernel" if L > 4096 else (
        "chroma_frames4096_kernel" if L == 4096 and not generic else "chroma_frames_kernel")


def report(kernel, case, stft=None, chroma=None):
    print("OBSERVED %-26s %-34s stft=%s chroma=%s" % (kernel, case, "-" if stft is None else "%.3g" % stft,
                                                     "-" if chroma is None else "%.3g" % chroma))


def dev(x, plan, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(plan.device)


def run_frames(plan, xdev, pad, **kw):
    ch, st = plan.frames(xdev, pad_left=pad, **kw)
    torch.cuda.synchronize()
    return (None if ch is None else ch.cpu().numpy()), (None if st is None else st.cpu().numpy())


# ---- 1 + 2: every loop more than once ----------------------------------------------------------------------------------

LOOP_CASES = [  # L, hop, float64 samples, frames in the last group
    (4096, 2048, False, 1),
    (4096, 2048, True, 2),
    (4096, 512, False, 3),
    (2048, 1024, False, 2),
    (1024, 256, False, 1),
    (64, 16, False, 3),
    (8192, 1024, False, 1),
    (512, 128, False, 2),    # the shortest length whose reduction scratch lives in the team's FFT buffer ...
    (256, 64, True, 3),      # ... and the longest that keeps it behind the spectra (chroma_plan.h, Lds::red_in_z)
]


def loop_geometry(L, cus, nf_last):
    """(grid, groups, frames per group, n_frames) such that workgroups 0 .. grid/3 take three trips, the others two,
    and the last group holds nf_last frames."""
    per = BIG_FR if L > 4096 else FR
    grid = 4 * cus if L > 4096 else cus
    groups = 2 * grid + grid // 3 + 1
    assert 1 <= nf_last < per
    n_frames = per * (groups - 1) + nf_last
    assert groups > grid and 2 * grid < groups < 3 * grid and (n_frames + per - 1) // per == groups
    return grid, groups, per, n_frames


def loop_input(L, hop, cus, nf_last, seed):
    grid, groups, per, n_frames = loop_geometry(L, cus, nf_last)
    pad = L // 2
    n = (n_frames - 1) * hop + L - pad + hop // 2     # the tail is too short for another frame
    # zero frames from the middle of a group of the second trip on, across group boundaries, and again in the third trip
    (z1, nz) = zero_stretch(per * (grid + 3) + 1, L, hop, pad)
    (z2, _) = zero_stretch(per * (2 * grid + 1) + per - 1, L, hop, pad)
    return synth(n, hop, seed, zeros=(z1, z2)), pad, n_frames, grid, per, (per * (grid + 3) + 1, nz)


@pytest.mark.parametrize("L,hop,f64,nf_last", LOOP_CASES)
def test_loops_take_several_trips_every_frame_checked(mods, cus, L, hop, f64, nf_last):
    """Some workgroups take three trips through the persistent loop, the rest two, the last group is partial; every
    frame of the STFT and of the chroma is compared with the oracle, and three frames with the longdouble DFT."""
    chroma, co, _ = mods
    x, pad, n_frames, grid, per, (m0, nz) = loop_input(L, hop, cus, nf_last, seed=L + hop)
    plan = chroma.ChromaPlan(L, hop, FS)
    try:
        assert plan.num_frames(len(x), pad) == n_frames
        ch, st = run_frames(plan, dev(x, plan, torch.float64 if f64 else None), pad, want_stft=True)
    finally:
        plan.close()
    ost = co.create_stft(x, L, hop).T
    assert st.shape == ost.shape == (n_frames, L // 2 + 1)
    e_st = stft_err(st, ost)
    fb = co.chroma_filterbank(FS, L)
    och = co.l2_normalize_columns(np.dot(fb, np.abs(ost.T) ** 2)).T
    assert adjacent_frames_differ(och)
    assert (och[m0:m0 + nz] == 0).all() and och[m0 - 1].any() and och[m0 + nz].any() and m0 % per != 0
    e_ch = float(np.abs(ch - och).max())
    report(kernel_name(L), "L=%d hop=%d %s M=%d" % (L, hop, "f64" if f64 else "f32", n_frames), e_st, e_ch)
    assert e_st <= STFT_RTOL
    assert e_ch <= CHROMA_ATOL
    assert (ch[m0:m0 + nz] == 0).all() and (st[m0:m0 + nz] == 0).all()
    # the same bins against the direct longdouble DFT: first frame, one of a third trip, last frame
    xp = np.concatenate((np.zeros(pad), x.astype(np.float64)))
    kb = dft_bins(L)
    for m in (0, per * 2 * grid + 1, n_frames - 1):
        D = longdouble_dft(xp[m * hop:m * hop + L] * np.hanning(L), kb)
        assert float(np.abs(st[m, kb] - D).max()) <= STFT_RTOL * float(np.abs(ost[m]).max()), m


@pytest.mark.parametrize("L,hop,f64,nf_last", LOOP_CASES)
def test_frame_values_do_not_depend_on_position(mods, cus, L, hop, f64, nf_last):
    """Bit-exact.  A frame's FFT is a function of its L windowed samples alone, and project_normalize reduces the 256
    partial sums of a (frame, pitch class) in a fixed order "independent of how many frames share the pass".  So frame m
    of a long run -- whichever workgroup, trip, team and round computed it, after whatever the prefetch and the reused
    scratch held before -- equals a one-frame call on its own slice bit for bit, STFT and chroma.  The float32 output
    is the kernel's (float) of the same double, which is torch's .to(float32) (round to nearest even)."""
    chroma, _, _ = mods
    x, pad, n_frames, grid, per, _ = loop_input(L, hop, cus, nf_last, seed=L + hop)
    plan = chroma.ChromaPlan(L, hop, FS)
    try:
        xd = dev(x, plan, torch.float64 if f64 else None)
        ch, st = run_frames(plan, xd, pad, want_stft=True)
        ch32, _ = plan.frames(xd, pad_left=pad, out_dtype=torch.float32)
        ch64, _ = plan.frames(xd, pad_left=pad)
        assert torch.equal(ch32.view(torch.int32), ch64.to(torch.float32).view(torch.int32))
        raw, _ = run_frames(plan, xd, pad, normalize=False)
        # first and last frame; for two workgroups, both sides of each of their group boundaries in every trip, which
        # includes both sides of the trip boundaries (last frame of one trip, first frame of the next)
        ms = {0, n_frames - 1}
        for w in (1, grid // 3, grid - 1):
            for trip in range(3):
                f0 = per * (w + trip * grid)
                ms.update((f0 - 1, f0, f0 + 1, f0 + per - 1, f0 + per))
        ms = sorted(m for m in ms if 0 <= m < n_frames)
        assert any(m >= per * 2 * grid for m in ms)
        xp = np.concatenate((np.zeros(pad, dtype=x.dtype), x))   # explicit zeros where the slice starts before sample 0
        for m in ms:
            one = dev(xp[m * hop:m * hop + L], plan, torch.float64 if f64 else None)
            c1, s1 = run_frames(plan, one, 0, want_stft=True)
            r1, _ = run_frames(plan, one, 0, normalize=False)
            assert c1.shape == (1, 12)
            assert bit_equal(s1[0], st[m]), "stft of frame %d" % m
            assert bit_equal(c1[0], ch[m]), "chroma of frame %d" % m
            assert bit_equal(r1[0], raw[m]), "un-normalised chroma of frame %d" % m
    finally:
        plan.close()


@pytest.mark.parametrize("L", [4096, 64])
def test_project_loops_and_partial_group(mods, L):
    """rts_chroma_project with more groups than its grid cap of 1024 and a partial last group, against np.dot (+ the
    oracle's normalisation), normalised and not, float64 and float32 output.  Spectra span 12 decades and some are 0."""
    chroma, co, _ = mods
    groups = PROJECT_GRID + PROJECT_GRID // 3 + 1
    m = FR * (groups - 1) + 3
    assert groups > PROJECT_GRID and m > 4 * PROJECT_GRID and m % FR == 3
    nb = L // 2 + 1
    rs = np.random.RandomState(L)
    spec = np.exp(4.5 * rs.standard_normal((m, nb))) * rs.rand(m, 1)
    spec[[5, FR * PROJECT_GRID + 2, m - 2]] = 0.0
    plan = chroma.ChromaPlan(L, L // 2, FS)
    try:
        sd = dev(spec, plan)
        got = plan.project(sd).cpu().numpy()
        graw = plan.project(sd, normalize=False).cpu().numpy()
        g32 = plan.project(sd, out_dtype=torch.float32)
        assert torch.equal(g32.view(torch.int32), plan.project(sd).to(torch.float32).view(torch.int32))
    finally:
        plan.close()
    oraw = np.dot(co.chroma_filterbank(FS, L), spec.T)
    e_raw = float((np.abs(graw - oraw.T).max(axis=1) / np.maximum(np.abs(oraw).max(axis=0), 1e-300)).max())
    e_ch = float(np.abs(got - co.l2_normalize_columns(oraw).T).max())
    report("chroma_project_kernel", "L=%d M=%d (raw: per-frame relative)" % (L, m), e_raw, e_ch)
    assert (np.abs(graw - oraw.T).max(axis=1) <= RAW_RTOL * np.abs(oraw).max(axis=0)).all()
    assert e_ch <= CHROMA_ATOL
    assert (got[[5, FR * PROJECT_GRID + 2, m - 2]] == 0).all()


# ---- 3: the batched entry point ---------------------------------------------------------------------------------------

BATCH_FRAMES = [0, 1, 257, 2 * 256 + 4 * 5 + 3, 255]
BATCH_ROWS = 540    # out_frames_stride: more rows than any stream fills
GUARD_ROWS = 16


def batch_streams(L, hop, pad):
    extra = [17, 5, hop // 2, 1, hop - 1]
    xs = []
    for b, nf in enumerate(BATCH_FRAMES):
        if nf == 0:
            xs.append(synth(extra[b], hop, 900 + b))    # too short for one frame even with the pad
            assert len(xs[-1]) + pad < L
            continue
        n = (nf - 1) * hop + L - pad + extra[b]
        zs = (zero_stretch(min(5, nf), L, hop, pad)[0], zero_stretch(4 * BATCH_GRID + 6, L, hop, pad)[0])
        xs.append(synth(n, hop, 900 + b + L, zeros=[z for z in zs if z[1] <= n]))
    return xs


def call_batch(nat, plan, xs, pad, sdtype, odtype, normalize=1):
    B = len(xs)
    stride = max(len(x) for x in xs) + 1001
    assert all(len(x) < stride for x in xs) and len(set(len(x) for x in xs)) == B
    buf = torch.full((B, stride), float("nan"), dtype=sdtype, device=plan.device)
    for b, x in enumerate(xs):
        buf[b, :len(x)] = torch.from_numpy(x).to(sdtype).to(plan.device)
    n_s = torch.tensor([len(x) for x in xs], dtype=torch.int32, device=plan.device)
    n_f = torch.tensor(BATCH_FRAMES, dtype=torch.int32, device=plan.device)
    out = torch.full((B * BATCH_ROWS + GUARD_ROWS, 12), float("nan"), dtype=odtype, device=plan.device)
    with torch.cuda.device(plan.device):
        nat.check(nat.lib.rts_chroma_frames_batch(
            plan._h, buf.data_ptr(), nat.F64 if sdtype == torch.float64 else nat.F32, stride, n_s.data_ptr(), pad, B,
            BATCH_ROWS, n_f.data_ptr(), normalize, out.data_ptr(), nat.F64 if odtype == torch.float64 else nat.F32,
            ctypes.c_void_p(torch.cuda.current_stream(plan.device).cuda_stream)))
        torch.cuda.synchronize()
    out = out.cpu().numpy()
    return out[:B * BATCH_ROWS].reshape(B, BATCH_ROWS, 12), out[B * BATCH_ROWS:]


@pytest.mark.parametrize("L,hop", [(4096, 2048), (512, 128), (8192, 2048)])
def test_frames_batch_ragged_streams(mods, L, hop):
    """rts_chroma_frames_batch on five ragged streams (0, 1, 257, 535 and 255 frames; 535 frames are 134 groups on
    a grid of 64, so workgroups take two and three trips and the last group is partial), pad_left 0 and L/2, float32
    and float64 samples, float64 and float32 output, into a NaN-filled buffer with a guard behind the last stream.
    Rows below n_frames[b] equal ChromaPlan.frames on that stream alone bit for bit: the batched launch runs the same
    kernel on the same values, only the grid and the per-stream offsets differ (and float32 samples convert to the
    very doubles the float64 copy holds).  Rows from n_frames[b] on and the guard stay NaN."""
    chroma, co, nat = mods
    per = BIG_FR if L > 4096 else FR
    assert (BATCH_ROWS + per - 1) // per > BATCH_GRID and (max(BATCH_FRAMES) + per - 1) // per > 2 * BATCH_GRID
    assert max(BATCH_FRAMES) % 4 == 3 and max(BATCH_FRAMES) > 2 * 256
    plan = chroma.ChromaPlan(L, hop, FS)
    fb, win = co.chroma_filterbank(FS, L), np.hanning(L)
    try:
        for pad in (0, L // 2):
            xs = batch_streams(L, hop, pad)
            refs = [ref_frames(co, x, L, hop, pad, win, fb, n_frames=nf) for x, nf in zip(xs, BATCH_FRAMES)]
            assert adjacent_frames_differ(refs[3][2])
            worst = 0.0
            for odtype in (torch.float64, torch.float32):
                alone = [run_frames(plan, dev(x, plan), pad, n_frames=nf, out_dtype=odtype)[0]
                         for x, nf in zip(xs, BATCH_FRAMES)]
                for sdtype in (torch.float32, torch.float64):
                    got, guard = call_batch(nat, plan, xs, pad, sdtype, odtype)
                    assert np.isnan(guard).all()
                    for b, nf in enumerate(BATCH_FRAMES):
                        assert np.isnan(got[b, nf:]).all(), (pad, b)
                        assert bit_equal(got[b, :nf], alone[b]), (pad, sdtype, odtype, b)
                        if nf:
                            err = float(np.abs(got[b, :nf] - refs[b][2]).max())
                            assert err <= (CHROMA_ATOL if odtype == torch.float64 else F32_ATOL), (pad, b)
                            if odtype == torch.float64:
                                worst = max(worst, err)
            report(kernel_name(L) + " (batch)", "L=%d hop=%d pad=%d" % (L, hop, pad), None, worst)
        # once un-normalised
        pad = L // 2
        got, guard = call_batch(nat, plan, xs, pad, torch.float32, torch.float64, normalize=0)
        assert np.isnan(guard).all()
        for b, nf in enumerate(BATCH_FRAMES):
            assert np.isnan(got[b, nf:]).all()
            assert bit_equal(got[b, :nf], run_frames(plan, dev(xs[b], plan), pad, n_frames=nf, normalize=False)[0])
            if nf:
                assert np.abs(got[b, :nf] - refs[b][1]).max() <= RAW_RTOL * np.abs(refs[b][1]).max()
    finally:
        plan.close()


# ---- 4: framing edges -------------------------------------------------------------------------------------------------

def check_framing(mods, plan, x, pad, n_frames=None, f64=False):
    chroma, co, _ = mods
    L, hop = plan.fft_len, plan.hop
    st_ref, raw_ref, ch_ref = ref_frames(co, x, L, hop, pad, np.hanning(L), co.chroma_filterbank(FS, L), n_frames)
    xd = dev(x, plan, torch.float64 if f64 else None)
    ch, st = run_frames(plan, xd, pad, want_stft=True, n_frames=n_frames)
    raw, _ = run_frames(plan, xd, pad, normalize=False, n_frames=n_frames)
    assert st.shape == st_ref.shape and ch.shape == ch_ref.shape, (L, hop, pad, len(x))
    assert stft_err(st, st_ref) <= STFT_RTOL, (L, hop, pad, len(x))
    assert np.abs(ch - ch_ref).max() <= CHROMA_ATOL, (L, hop, pad, len(x))
    assert np.abs(raw - raw_ref).max() <= RAW_RTOL * np.abs(raw_ref).max(), (L, hop, pad, len(x))
    return ch, st


@pytest.mark.parametrize("L,hop,n", [(4096, 441, 60000), (64, 1, 3000), (256, 1000, 150000)])
def test_odd_and_long_hops(mods, L, hop, n):
    """An odd hop, hop 1 and hop > fft_len, every frame against the restated framing, pad_left 0 and L/2."""
    chroma = mods[0]
    plan = chroma.ChromaPlan(L, hop, FS)
    try:
        x = synth(n, max(hop, 16), 3 * L + hop, zeros=(zero_stretch(9, L, hop, 0)[0],))
        for pad in (0, L // 2):
            ch, _ = check_framing(mods, plan, x, pad)
            assert ch.shape[0] == (n + pad - L) // hop + 1 > 4
    finally:
        plan.close()


@pytest.mark.parametrize("L,hop", [(4096, 2048), (512, 128), (8192, 2048)])
def test_pads_and_frame_count_edges(mods, L, hop):
    chroma, _, nat = mods
    plan = chroma.ChromaPlan(L, hop, FS)
    try:
        x = synth(11 * hop + L + 77, hop, 5 * L, zeros=(zero_stretch(4, L, hop, 0)[0],))
        for pad in (1, 333):                               # odd pads
            check_framing(mods, plan, x, pad)
            check_framing(mods, plan, x, pad, f64=True)
        ch, st = check_framing(mods, plan, x, L + 7)        # frame 0 is all padding: exactly zero
        assert (ch[0] == 0).all() and (st[0] == 0).all() and ch[1].any()
        for pad in (0, 1, L // 2):                          # n_samples + pad_left == L: exactly one frame
            ch, _ = check_framing(mods, plan, x[:L - pad], pad)
            assert ch.shape[0] == 1
            assert plan.num_frames(L - pad - 1, pad) == 0
        for pad in (0, L // 2):
            n_end = 7 * hop + L - pad                       # the last frame ends on the last sample
            assert plan.num_frames(n_end, pad) == 8 and plan.num_frames(n_end - 1, pad) == 7
            ch, _ = check_framing(mods, plan, x[:n_end], pad)
            assert ch.shape[0] == 8
            ch, _ = check_framing(mods, plan, x[:n_end - 1], pad)
            assert ch.shape[0] == 7
            full = check_framing(mods, plan, x[:n_end], pad)[0]
            for fewer in (1, 5, 7):                         # n_frames= smaller than what fits
                ch, _ = check_framing(mods, plan, x[:n_end], pad, n_frames=fewer)
                assert ch.shape[0] == fewer and bit_equal(ch, full[:fewer])
            with pytest.raises(nat.RtsyncError):            # one too many
                plan.frames(dev(x[:n_end], plan), pad_left=pad, n_frames=9)
    finally:
        plan.close()


# ---- 5: dynamic range -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,hop", [(4096, 2048), (512, 128), (8192, 2048)])
def test_power_of_two_scaling_is_exact(mods, L, hop):
    """Bit-exact.  Multiplying the samples by 2^k multiplies every float64 intermediate of a linear chain (window
    product, FFT butterflies, untangling) by 2^k exactly, the power spectrum and the filterbank sums by 4^k exactly, and
    leaves the quotient chroma / norm unchanged, as long as nothing under- or overflows: scaling by a power of two only
    changes exponents, so every rounding falls the same way.  A float32 intermediate, or a reordering that depends on
    magnitude, would break it.  With k = -600 every power underflows to 0, and the tiny-norm rule of
    librosa.util.normalize must leave exact zeros, not 0/0."""
    chroma = mods[0]
    plan = chroma.ChromaPlan(L, hop, FS)
    pad = L // 2
    try:
        x = synth(40 * hop, hop, 7 * L, zeros=(zero_stretch(13, L, hop, pad)[0],))
        ch0, st0 = run_frames(plan, dev(x, plan), pad, want_stft=True)
        raw0, _ = run_frames(plan, dev(x, plan), pad, normalize=False)
        assert np.isfinite(ch0).all() and (ch0[13] == 0).all() and ch0[12].any()
        cases = [(k, np.float64) for k in (40, -40)] + [(k, np.float32) for k in (20, -20)]
        for k, dt in cases:
            xs = x.astype(dt) * dt(2.0) ** k
            assert np.array_equal(xs.astype(np.float64), x.astype(np.float64) * 2.0 ** k)     # the scaling is exact
            ch, st = run_frames(plan, dev(xs, plan), pad, want_stft=True)
            raw, _ = run_frames(plan, dev(xs, plan), pad, normalize=False)
            assert bit_equal(st.view(np.float64), st0.view(np.float64) * 2.0 ** k), (k, dt)
            assert bit_equal(raw, raw0 * 4.0 ** k), (k, dt)
            assert bit_equal(ch, ch0), (k, dt)
        tiny = x.astype(np.float64) * 2.0 ** -600
        assert (tiny[x != 0] != 0).all()
        ch, st = run_frames(plan, dev(tiny, plan), pad, want_stft=True)
        # the spectrum itself is still there (its smallest non-zero parts stay far above the subnormals)
        assert bit_equal(st.view(np.float64), st0.view(np.float64) * 2.0 ** -600) and np.abs(st).max() > 0
        assert (ch == 0).all()                                               # no NaN, no Inf
    finally:
        plan.close()


# ---- 6: caller-supplied window ----------------------------------------------------------------------------------------

def plan_with_window(chroma, nat, L, hop, win):
    """A ChromaPlan whose handle comes from rts_chroma_create with window_host set."""
    plan = chroma.ChromaPlan(L, hop, FS)
    plan.close()
    win = np.ascontiguousarray(win, dtype=np.float64)
    h = ctypes.c_void_p()
    with torch.cuda.device(plan.device):
        nat.check(nat.lib.rts_chroma_create(L, hop, win.ctypes.data, plan.chromafb.ctypes.data, ctypes.byref(h)))
    plan._h = h
    return plan


@pytest.mark.parametrize("L,hop", [(4096, 2048), (256, 64)])
@pytest.mark.parametrize("window", ["ones", "periodic_hann"])
def test_caller_supplied_window(mods, L, hop, window):
    """window_host != NULL: the 4096 kernel holds the window in registers, the generic one reads the table."""
    chroma, co, nat = mods
    win = np.ones(L) if window == "ones" else 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(L) / L)
    assert not np.array_equal(win, np.hanning(L))
    plan = plan_with_window(chroma, nat, L, hop, win)
    try:
        x = synth(45 * hop + 123, hop, 11 * L, zeros=(zero_stretch(17, L, hop, 333)[0],))
        for pad in (0, 333, L // 2):
            st_ref, raw_ref, ch_ref = ref_frames(co, x, L, hop, pad, win, plan.chromafb)
            ch, st = run_frames(plan, dev(x, plan), pad, want_stft=True)
            raw, _ = run_frames(plan, dev(x, plan), pad, normalize=False)
            assert st.shape == st_ref.shape and st.shape[0] > 40
            assert stft_err(st, st_ref) <= STFT_RTOL
            assert np.abs(ch - ch_ref).max() <= CHROMA_ATOL
            assert np.abs(raw - raw_ref).max() <= RAW_RTOL * np.abs(raw_ref).max()
            # and the default window would not have passed
            wrong = ref_frames(co, x, L, hop, pad, np.hanning(L), plan.chromafb)[0]
            assert stft_err(st, wrong) > 1e-6
    finally:
        plan.close()


# ---- 7: fft_len 4096 on the generic kernel ----------------------------------------------------------------------------

def test_fft4096_beyond_32bit_indices_runs_the_generic_kernel(mods):
    """hop 2^20, pad_left 2048, 2^30 + 4096 float32 samples (4.3 GB, generated on the device): the host's routing
    inequality sends this 4096 plan to chroma_frames_kernel<float> with 64-bit sample indices and all eight sample
    pairs per thread.  All 1025 frames are compared with the oracle on the frame slices copied back."""
    chroma, co, _ = mods
    L, hop, pad = 4096, 1 << 20, 2048
    n = (1 << 30) + 4096
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * 4 * n:
        pytest.skip("needs %.1f GB of free device memory (three times the 4.3 GB sample buffer), %.1f GB are free"
                    % (3 * 4 * n / 1e9, free / 1e9))
    plan = chroma.ChromaPlan(L, hop, FS)
    try:
        n_frames = plan.num_frames(n, pad)
        assert n_frames == 1025
        assert n + 2 * L + n_frames * hop >= 0x7fffffff          # chroma_plan.h, flavour(): not the 4096 kernel
        assert (n_frames + FR - 1) // FR == 257                  # more groups than CUs on a 256-CU part
        x = torch.empty(n, dtype=torch.float32, device=plan.device)
        gen = torch.Generator(device=plan.device)
        gen.manual_seed(4096)
        rs = np.random.RandomState(4096)
        tones = [(440.0 * 2.0 ** ((m - 69) / 12.0), hop * (5 + 3 * j) + 0.37, rs.uniform(0, 2 * np.pi),
                  rs.uniform(0, 2 * np.pi)) for j, m in enumerate(_MIDI)]
        chunk = 1 << 24
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            i = torch.arange(s, e, dtype=torch.float64, device=plan.device)
            v = 1e-3 * torch.randn(e - s, dtype=torch.float64, device=plan.device, generator=gen)
            for f, period, p0, p1 in tones:
                v += 0.12 * (0.5 + 0.45 * torch.sin(2 * np.pi / period * i + p0)) * torch.sin(2 * np.pi * f / FS * i + p1)
            x[s:e] = v.to(torch.float32)
            del i, v
        (za, zb), nz = zero_stretch(601, L, hop, pad)
        x[za:zb] = 0.0
        ch, st = plan.frames(x, pad_left=pad, want_stft=True)
        torch.cuda.synchronize()
        ch, st = ch.cpu().numpy(), st.cpu().numpy()
        # the 1025 frame slices, zero where they start before sample 0
        idx = (torch.arange(n_frames, device=plan.device, dtype=torch.int64)[:, None] * hop - pad
               + torch.arange(L, device=plan.device, dtype=torch.int64)[None, :])
        assert int(idx.max()) < n
        sl = torch.where(idx >= 0, x[idx.clamp(min=0)], torch.zeros((), dtype=x.dtype, device=x.device)).cpu().numpy()
        del x, idx
    finally:
        plan.close()
    ost = np.fft.rfft(sl.astype(np.float64) * np.hanning(L), axis=1)
    och = co.l2_normalize_columns(np.dot(co.chroma_filterbank(FS, L), np.abs(ost.T) ** 2)).T
    assert adjacent_frames_differ(och) and (och[601:601 + nz] == 0).all() and (sl[0, :pad] == 0).all()
    e_st, e_ch = stft_err(st, ost), float(np.abs(ch - och).max())
    report(kernel_name(L, generic=True), "L=4096 hop=2^20 M=1025 (64-bit)", e_st, e_ch)
    assert e_st <= STFT_RTOL
    assert e_ch <= CHROMA_ATOL
    assert (ch[601:601 + nz] == 0).all()
    kb = dft_bins(L)
    for m in (0, 1023, 1024):
        D = longdouble_dft(sl[m].astype(np.float64) * np.hanning(L), kb)
        assert float(np.abs(st[m, kb] - D).max()) <= STFT_RTOL * float(np.abs(ost[m]).max()), m


# ---- 8: rts_chroma_diff -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [2, 10007])
def test_chroma_diff_is_exact(mods, dtype, m):
    """Bit-exact: one IEEE subtraction and a comparison per element, in the input's own type.  10007 frames are 470
    workgroups of 256 threads with a partial last one."""
    chroma = mods[0]
    plan = chroma._plan()
    rs = np.random.RandomState(m)
    c = (rs.rand(m, 12) * np.exp(3 * rs.standard_normal((m, 1)))).astype(dtype)
    c[m // 2] = c[m // 2 - 1]      # zero differences
    assert ((m - 1) * 12 + 255) // 256 >= (1 if m == 2 else 300)
    out = plan.diff(dev(c, plan))
    assert out.shape == (m - 1, 12) and out.dtype == (torch.float32 if dtype == np.float32 else torch.float64)
    want = np.clip(np.diff(c, axis=0), 0, np.inf)
    assert want.dtype == dtype and np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chroma_diff_propagates_nan_like_numpy(mods, dtype):
    """np.clip(np.diff(c), 0, inf) keeps a NaN difference; so does the kernel (the two rows next to a NaN frame)."""
    chroma = mods[0]
    plan = chroma._plan()
    rs = np.random.RandomState(9)
    c = rs.rand(300, 12).astype(dtype)
    c[100] = np.nan
    c[200, 3] = np.inf
    c[201, 3] = np.inf             # inf - inf
    with np.errstate(invalid="ignore"):
        want = np.clip(np.diff(c, axis=0), 0, np.inf)
    assert np.isnan(want[99]).all() and np.isnan(want[100]).all() and np.isnan(want[200, 3])
    got = plan.diff(dev(c, plan)).cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True)
