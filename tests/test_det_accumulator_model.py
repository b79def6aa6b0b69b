"""Host model of the long accumulators of the deterministic mode (csrc/common.h: det_add_pieces / det_value).

The device code cannot run here; this restates its arithmetic in Python integers with the same constants (six signed 64-bit
windows, window j weighing 2^(BASE + 32 j), BASE = -110) and checks the three properties the mode rests on: the pieces of a value
reconstruct it exactly, the windows are independent of the order of the additions, and the read-out equals the exactly rounded
sum.  The GPU tests (test_long_accumulator_finalize_matches_fp64, test_deterministic_*) pin the device code itself.

Non-finite and out-of-range addends: the device code MARKS the accumulator -- an atomic MAX of the signed top window with 2^62
(idempotent) -- and det_value reads a top window outside +-2^61 as NaN.  ``det_add_f32`` / ``det_read`` below restate that branch
with 64-bit wrap-around; tests/test_gpu_det_nonfinite.py feeds NaN / Inf to the device accumulators themselves."""
import math
import random
import struct

K, BASE = 6, -110
MASK64 = (1 << 64) - 1


def pieces_f32(v):
    """-> list of (window, signed piece) exactly as det_add_f32 adds them"""
    b = struct.unpack("<I", struct.pack("<f", v))[0]
    ex = (b >> 23) & 0xff
    assert ex != 0xff
    m = (b & 0x7fffff) | 0x800000 if ex else (b & 0x7fffff)
    if not m:
        return []
    shift = (ex if ex else 1) - 150 - BASE
    neg = bool(b >> 31)
    if shift < 0:
        m = m >> (-shift) if shift > -64 else 0
        shift = 0
    j, r = shift >> 5, shift & 31
    lo64 = (m << r) & MASK64
    hi = (m >> (64 - r)) if r else 0
    ps = [lo64 & 0xffffffff, lo64 >> 32, hi]
    assert not (j >= K or (ps[1] and j + 1 >= K) or (ps[2] and j + 2 >= K))
    return [(j + i, -p if neg else p) for i, p in enumerate(ps) if p]


def value(windows):
    s = 0.0
    for j in range(K - 1, -1, -1):
        s += math.ldexp(float(windows[j]), BASE + 32 * j)
    return s


def test_pieces_reconstruct_the_value_exactly():
    rng = random.Random(1)
    for _ in range(2000):
        v = struct.unpack("<f", struct.pack("<f", rng.uniform(-1, 1) * 10.0 ** rng.uniform(-20, 20)))[0]
        exact = sum(p * 2 ** (BASE + 32 * j) if BASE + 32 * j >= 0 else p / 2 ** (-(BASE + 32 * j)) for j, p in pieces_f32(v))
        assert exact == v, (v, exact)          # (every term a dyadic rational: exact in Python's arithmetic here)
        assert all(abs(p) < 2 ** 32 for _, p in pieces_f32(v))


def test_windows_do_not_depend_on_the_order_and_give_the_exact_sum():
    rng = random.Random(2)
    vals = [struct.unpack("<f", struct.pack("<f", rng.gauss(0, 1) * 10.0 ** rng.uniform(-6, 6)))[0] for _ in range(20000)]

    def accumulate(seq):
        w = [0] * K
        for v in seq:
            for j, p in pieces_f32(v):
                w[j] += p
        assert all(-2 ** 63 <= x < 2 ** 63 for x in w)        # (a window takes 2^31 pieces before it can overflow)
        return w

    a = accumulate(vals)
    for seed in (3, 4, 5):
        sh = vals[:]
        random.Random(seed).shuffle(sh)
        assert accumulate(sh) == a
    exact = math.fsum(vals)
    got = value(a)
    assert abs(got - exact) <= 4 * 2.0 ** -53 * sum(abs(v) for v in vals) / len(vals) * 1e3 and abs(got - exact) <= 1e-9 * abs(exact) + 1e-12
    # a plain float32 running sum of the same values depends on the order (what the mode removes)
    import numpy as np
    f1 = float(np.cumsum(np.array(vals, dtype=np.float32))[-1])
    sh = vals[:]
    random.Random(9).shuffle(sh)
    f2 = float(np.cumsum(np.array(sh, dtype=np.float32))[-1])
    assert f1 != f2


def test_tiny_values_are_truncated_the_same_way_every_time():
    tiny = struct.unpack("<f", struct.pack("<f", 1e-38))[0]
    assert pieces_f32(tiny) == pieces_f32(tiny)
    assert sum(abs(p) for _, p in pieces_f32(tiny)) == 0 or pieces_f32(tiny)[0][0] == 0     # below 2^-110: dropped / lowest window


# ---- non-finite / out-of-range addends: the mark and the read-out as the device code has them -------------------------------------
MARK = 1 << 62


def _wrap(x):
    """a Python integer as the signed 64-bit value the device holds"""
    x &= MASK64
    return x - (1 << 64) if x >> 63 else x


def det_add_f32(w, v, mark=lambda top: max(top, MARK)):
    """det_add_f32 + det_add_pieces on the window list w; ``mark`` = what a non-finite / too large addend does to the top window
    (device code: atomicMax with 2^62).  Returns True if the addend took the mark branch."""
    b = struct.unpack("<I", struct.pack("<f", v))[0]
    ex = (b >> 23) & 0xff
    if ex == 0xff:
        w[K - 1] = _wrap(mark(w[K - 1]))
        return True
    m = (b & 0x7fffff) | 0x800000 if ex else (b & 0x7fffff)
    if not m:
        return False
    shift = (ex if ex else 1) - 150 - BASE
    if shift < 0:
        m = m >> (-shift) if shift > -64 else 0
        shift = 0
    j, r = shift >> 5, shift & 31
    lo64 = (m << r) & MASK64
    hi = (m >> (64 - r)) if r else 0
    ps = [lo64 & 0xffffffff, lo64 >> 32, hi]
    if j >= K or (ps[1] and j + 1 >= K) or (ps[2] and j + 2 >= K):
        w[K - 1] = _wrap(mark(w[K - 1]))
        return True
    for i, p in enumerate(ps):
        if p:
            w[j + i] = _wrap(w[j + i] + (-p if b >> 31 else p))
    return False


def det_read(w):
    """det_value: a top window at or beyond +-2^61 reads as NaN"""
    if w[K - 1] >= (1 << 61) or w[K - 1] <= -(1 << 61):
        return math.nan
    return value(w)


def _f32(v):
    return struct.unpack("<f", struct.pack("<f", v))[0]


def _finite_addends(rng, n=10000):
    """both signs, from below the lowest window (2^-110 = 8e-34) to the top one (2^50 ... 2^81 = 2.4e24)"""
    return [_f32(rng.choice((-1, 1)) * rng.uniform(1, 10) * 10.0 ** rng.uniform(-36, 23)) for _ in range(n)]


def test_marked_accumulator_reads_nan_for_any_number_of_marks_in_any_order():
    rng = random.Random(6)
    fin = _finite_addends(rng)
    assert max(abs(v) for v in fin) > 2.0 ** 70 and min(abs(v) for v in fin) < 2.0 ** -100
    for k in (1, 2, 3, 4, 8, 1024):
        bad = [rng.choice((math.nan, math.inf, -math.inf)) for _ in range(k)]
        for seed in (0, 1, 2):
            seq = fin + bad
            random.Random(100 * k + seed).shuffle(seq)
            w = [0] * K
            assert sum(det_add_f32(w, v) for v in seq) == k
            assert math.isnan(det_read(w)), (k, seed, w[K - 1])
        # the two extreme orders: every mark first, every mark last
        for seq in (bad + fin, fin + bad):
            w = [0] * K
            for v in seq:
                det_add_f32(w, v)
            assert math.isnan(det_read(w)), (k, w[K - 1])


def test_addend_too_large_for_the_windows_marks_the_accumulator():
    """det_add_pieces' overflow branch: the top window weighs 2^50 and takes pieces below 2^32, so a float of 2^82 or more has no
    place; everything below is summed exactly."""
    for big in (2.0 ** 82, -2.0 ** 82, 1e30, -3.0e38, _f32(3.4028234e38)):
        for k in (1, 4, 1024):
            w = [0] * K
            det_add_f32(w, 1.5)
            assert all(det_add_f32(w, big) for _ in range(k))
            det_add_f32(w, -2.5)
            assert math.isnan(det_read(w)), (big, k)
    for ok in (2.0 ** 70, -2.0 ** 81, _f32(2.0 ** 82 * (1 - 2.0 ** -24))):
        w = [0] * K
        assert not det_add_f32(w, ok) and not det_add_f32(w, ok)
        assert det_read(w) == 2 * ok


def test_without_marks_the_model_is_the_plain_sum_of_pieces():
    rng = random.Random(7)
    vals = _finite_addends(rng, 5000)
    w = [0] * K
    assert not any(det_add_f32(w, v) for v in vals)
    plain = [0] * K
    for v in vals:
        for j, p in pieces_f32(v):
            plain[j] += p
    assert w == plain and abs(w[K - 1]) < 1 << 61
    assert det_read(w) == value(plain) and math.isfinite(det_read(w))


def test_why_the_mark_is_a_max_and_not_a_sum():
    """The earlier scheme ADDED 2^62 to the top window per non-finite addend.  One, two or three marks are outside +-2^61 (2^62,
    -2^63, -2^62 as signed 64-bit values); four are 2^64 = 0: the accumulator read back finite.  A persistent grid adds one
    partial per workgroup -- 256, 512, 768 or 1024 of them -- so "every partial is NaN" always gave a multiple of four."""
    assert (4 << 62) % 2 ** 64 == 0
    assert [_wrap(k << 62) for k in (1, 2, 3, 4)] == [1 << 62, -(1 << 63), -(1 << 62), 0]

    def additive(top):
        return top + MARK

    for k, reads_nan in ((1, True), (2, True), (3, True), (4, False), (8, False), (1024, False)):
        w = [0] * K
        det_add_f32(w, 0.25)
        for _ in range(k):
            det_add_f32(w, math.nan, mark=additive)
        assert math.isnan(det_read(w)) == reads_nan
        if not reads_nan:
            assert det_read(w) == 0.25
        w = [0] * K
        det_add_f32(w, 0.25)
        for _ in range(k):
            det_add_f32(w, math.nan)
        assert math.isnan(det_read(w))
