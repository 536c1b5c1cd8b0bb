"""TEST INFRASTRUCTURE - the numpy twin of sx_stats_* (include/scythe_hip.h): a sequence of samples (q, time, weight).

q is formed by tests/distribution.py::program_values64, which reproduces an output of a field program bit for bit.  MAX, MIN and
their times follow the header's order in plain float64 and are held bitwise.  SUM and DURATION are computed in longdouble.

The bound of a SUM, derived (u = 2^-53, n samples, S_abs = sum |w q| at the point):
  - the device forms w q as the pair (ph, pl) with ph + pl = w q exactly (fma), and adds ph to hi with a two-sum, whose error term e
    is exact: hi + ph = s + e.  Nothing is lost there.  What is rounded is lo: two additions per sample, lo += e and lo += pl.
  - |e| <= u |s| <= u S_abs (1 + u)^n and |pl| <= u |ph|, so after k samples |lo| <= (k + 1) u S_abs to first order, and each of its
    2 n additions commits at most u |lo|: together at most 2 n (n + 1) u^2 S_abs; the factor 4 below covers the (1 + u)^n growth
    that "to first order" leaves out (for any n below 2^20).
  - the copy-out folds hi + lo once: at most u |hi + lo| <= u S_abs (1 + u).
  - the twin itself: a longdouble product of two doubles is rounded (106 bits do not fit 64), 2^-64 |w q| each, and so is each of
    its n additions: at most (2 n + 2) 2^-64 S_abs.
  bound = S_abs (u + 4 n (n + 1) u^2 + (2 n + 2) 2^-64).  Nothing here was fitted to the kernel.
A DURATION is a sum of the weights themselves; the twin forms it in longdouble and rounds once.  The device's double-double sum is
off by at most 2 n (n + 1) u^2 of the sum, the twin by n 2^-64: both round to the same double unless the exact sum lies that close
to the midpoint of two doubles, which tests/test_stats.py rules out for the weights the GPU tests use (against math.fsum)."""
import math

import numpy as np

from tests import distribution as DI

XP = np.longdouble
U = 2.0 ** -53
OPS = ("sum", "max", "min", "duration")


def sum_bound(S_abs, n):
    return np.asarray(S_abs, dtype=XP) * XP(U + 4.0 * n * (n + 1) * U * U + (2 * n + 2) * 2.0 ** -64)


class Twin:
    """One output at N points: feed it samples (q [N] float64, time, weight) in order"""

    def __init__(self, op, n_points, threshold=None):
        assert op in OPS
        self.op, self.thr = op, threshold
        self.samples = 0
        self.value = np.full(n_points, np.nan)       # max / min
        self.time = np.full(n_points, np.nan)
        self.sum = np.zeros(n_points, dtype=XP)      # sum / duration
        self.S_abs = np.zeros(n_points, dtype=XP)
        self.counted = []                            # duration: per sample with w != 0, (w, mask [N])

    def add(self, q, time, w):
        q = np.asarray(q, dtype=np.float64)
        if self.op == "sum":
            if w != 0.0:
                with np.errstate(all="ignore"):
                    p = XP(w) * q.astype(XP)
                self.sum = self.sum + p
                self.S_abs = self.S_abs + np.abs(p)
        elif self.op == "duration":
            if w != 0.0:
                with np.errstate(invalid="ignore"):
                    m = q >= self.thr                # a NaN compares false
                self.sum = self.sum + np.where(m, XP(w), XP(0))
                self.counted.append((float(w), m))
        else:
            if self.samples == 0:
                take = np.ones(len(q), dtype=bool)
            else:
                with np.errstate(invalid="ignore"):
                    better = q > self.value if self.op == "max" else q < self.value
                # a NaN that is there stays; a NaN that comes wins; a tie (-0.0 == +0.0 included) keeps the earlier sample
                take = ~np.isnan(self.value) & (np.isnan(q) | better)
            self.value = np.where(take, q, self.value)
            self.time = np.where(take, float(time), self.time)
        self.samples += 1

    def result(self):
        """float64 value [N] as sx_stats_get returns slot 0 (sum-like: the longdouble sum rounded once)"""
        return self.sum.astype(np.float64) if self.op in ("sum", "duration") else self.value

    def duration_exact(self):
        """the correctly rounded exact sum of the counted weights (math.fsum), per point"""
        out = np.zeros(len(self.sum))
        if not self.counted:
            return out
        key = np.zeros(len(self.sum), dtype=np.int64)
        for j, (_, m) in enumerate(self.counted):
            key |= m.astype(np.int64) << j
        for k in np.unique(key):
            out[key == k] = math.fsum(w for j, (w, _) in enumerate(self.counted) if (int(k) >> j) & 1)
        return out


def run(program, ops, thresholds, samples, radii):
    """samples: a list of (data [N, V] or [N, V, D], time, weight); program = (coef, packed, n_out) as pack_reduce_program gives it.
    Returns the list of Twins, one per output."""
    n = len(np.asarray(radii))
    twins = [Twin(op, n, thr) for op, thr in zip(ops, thresholds)]
    for data, time, w in samples:
        for o, tw in enumerate(twins):
            tw.add(DI.program_values64(data, radii, program, out=o), time, w)
    return twins


def elapsed(weights):
    """(hi, lo) of the double-double sum of the weights as the handle keeps it (Knuth's two-sum in float64)"""
    hi = lo = 0.0
    for w in weights:
        s = hi + w
        b = s - hi
        lo += (hi - (s - b)) + (w - b)
        hi = s
    return hi, lo


def check_bitwise(got, want, what=""):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    same = (got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d points differ, first at %d: %r vs %r" % (
        what, (~same).sum(), same.size, int(np.argmin(same)), got.reshape(-1)[int(np.argmin(same))], want.reshape(-1)[int(np.argmin(same))])


def check_sum(got, twin, what=""):
    """|got - longdouble sum| <= sum_bound at every point; a NaN sum where the twin's is NaN.  Returns the largest ratio to the bound."""
    got = np.asarray(got, dtype=np.float64)
    nan = np.isnan(twin.sum.astype(np.float64))
    assert (np.isnan(got) == nan).all(), "%s: NaN sums at other points than the twin's" % what
    err = np.abs(np.where(nan, XP(0), got.astype(XP) - twin.sum))
    bound = np.where(nan, XP(1), sum_bound(twin.S_abs, twin.samples))
    zero = bound == 0
    assert (err[zero] == 0).all(), "%s: a non-zero sum where every product is zero" % what
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    assert ratio <= 1.0, "%s: |sum - twin| is %.3f of the derived bound" % (what, ratio)
    return ratio
