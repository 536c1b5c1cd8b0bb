"""CPU-only: the twin of sx_crossings (tests/crossings.py) against closed forms, the host helper sx_bracket_step against the twin's
step operation for operation, the pure-measure program, and the refusals that need no device.

test_twin_converges_to_closed_form prints both errors; DESIGN.md 15, "Figures", holds them."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import crossings as X

XP = X.XP
A_LEN, EPS2 = 4.0, 0.1


def _rl_grid(nc):
    return O.Grid("RL", 0.0, 10.0, nc, {"h": 1}, ring_L=16)


def _closed_form_error(nc, levels, lam):
    g = _rl_grid(nc)
    pts = g.gridpoints()
    h = np.exp(-(pts[:, 0] / A_LEN) ** 2) * (1.0 + EPS2 * np.cos(2.0 * pts[:, 1]))
    A = X.project(g, h[:, None])
    prog = (np.array([1.0]), np.array([[0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32), 1)
    res = X.crossings(g, A, prog, levels, lam[:, None], max_cross=2, xp=True)
    assert (res.count == 1).all() and (res.dir[0] == -1).all() and (res.status == 0).all()
    exact = A_LEN * np.sqrt(np.log((1.0 + EPS2 * np.cos(2.0 * lam))[None, :] / np.asarray(levels)[:, None]))
    return float(np.abs(res.radius[0] - exact).max())


def test_twin_converges_to_closed_form():
    """h = exp(-r^2 / a^2) (1 + eps cos 2 lambda) projected onto RL grids of 10 and 20 cells: the crossings of c lie at
    a sqrt(ln((1 + eps cos 2 lambda) / c)).  Cubic-spline projection is fourth order (16 per halving); more than 8 is asserted."""
    levels, lam = [0.6, 0.3], np.linspace(0.0, 2.0 * np.pi, 12, endpoint=False) + 0.1
    e10, e20 = _closed_form_error(10, levels, lam), _closed_form_error(20, levels, lam)
    print("closed form: |r - exact| max %.3e (10 cells), %.3e (20 cells), ratio %.1f" % (e10, e20, e10 / e20))
    assert e10 / e20 > 8.0


def _lib_step(B, fx, wtol, first=False):
    import scythe_jl_amd as S
    s, f = B.state()
    return S.bracket_step(s, f, fx, wtol, first)


def test_bracket_step_is_the_twin_bitwise():
    """random brackets driven to the end through the host helper and through the twin, on a cubic with a root inside: every state
    after every step agrees bitwise; d == 0 at an end finishes at once; a step that does not halve the bracket is followed by a
    bisection"""
    rng = np.random.default_rng(7)
    n_bis = 0
    for trial in range(200):
        root, k = rng.uniform(-3.0, 3.0), rng.uniform(0.0, 4.0)
        fn = lambda x: np.float64((x - root) * (1.0 + k * (x - root) ** 2) * (1.0 if trial % 2 else -1.0))
        a, b = root - rng.uniform(0.01, 2.0), root + rng.uniform(0.01, 2.0)
        wtol = 10.0 ** rng.uniform(-14, -6)
        T = X.Bracket(a, fn(a), b, fn(b))
        s, f = T.state()
        s, f, st = _lib_step(T, 0.0, wtol, first=True)
        st_t = T.start(wtol)
        for it in range(80):
            ts, tf = T.state()
            assert st == st_t and s.tobytes() == ts.tobytes() and f.tobytes() == tf.tobytes(), (trial, it)
            if st != -1:
                break
            n_bis += int(f[1])
            fx = fn(s[6])
            import scythe_jl_amd as S
            s, f, st = S.bracket_step(s, f, fx, wtol)
            st_t = T.step(fx, wtol)
        assert st == 0 and T.b - T.a <= wtol or T.fa == 0 or T.fb == 0
        assert (T.fa < 0) != (T.fb < 0) or T.a == T.b                # the bracket still holds the sign change
        assert abs(T.root() - root) <= wtol + 4e-16 * abs(root)
    assert n_bis > 0                                                 # the bisection fallback was taken somewhere
    # d == 0 exactly at an end: finished before any trial, the root is that end (inner end: fa = 0 counts as non-negative)
    for a, fa, b, fb, want in ((1.0, 0.0, 2.0, -3.0, 1.0), (1.0, -3.0, 2.0, 0.0, 2.0)):
        T = X.Bracket(a, fa, b, fb)
        s, f, st = _lib_step(T, 0.0, 1e-9, first=True)
        assert st == 0 and T.start(1e-9) == 0 and s.tobytes() == T.state()[0].tobytes() and T.root() == want
    # d == 0 at a trial point: both ends collapse onto it
    T = X.Bracket(0.0, -1.0, 2.0, 1.0)
    s, f, st = _lib_step(T, 0.0, 1e-9, first=True)
    assert st == -1 and s[6] == 1.0
    import scythe_jl_amd as S
    s, f, st = S.bracket_step(s, f, 0.0, 1e-9)
    assert st == 0 and s[0] == s[2] == 1.0 and s[1] == s[3] == 0.0
    # a NaN at the trial point leaves the bracket as it is
    T = X.Bracket(0.0, -1.0, 2.0, 1.0)
    s0, f0, _ = _lib_step(T, 0.0, 1e-9, first=True)
    s, f, st = S.bracket_step(s0, f0, np.nan, 1e-9)
    assert st == 2 and s.tobytes() == s0.tobytes()


def test_bisection_fallback():
    """a function flat on one side: false position creeps, so every second step is a bisection and the bracket halves at least
    every two steps, in the helper as in the twin"""
    import scythe_jl_amd as S
    fn = lambda x: np.float64(np.expm1(12.0 * (x - 1.0)))            # root at 1, flat to the left
    T = X.Bracket(-4.0, fn(-4.0), 1.5, fn(1.5))
    s, f, st = _lib_step(T, 0.0, 1e-12, first=True)
    T.start(1e-12)
    widths, bis = [T.b - T.a], 0
    while st == -1:
        fx = fn(s[6])
        s, f, st = S.bracket_step(s, f, fx, 1e-12)
        assert T.step(fx, 1e-12) == st and s.tobytes() == T.state()[0].tobytes() and f.tobytes() == T.state()[1].tobytes()
        widths.append(T.b - T.a)
        bis += int(f[1])
    assert bis > 0 and len(widths) <= 60
    assert all(widths[i + 2] <= 0.5 * widths[i] for i in range(len(widths) - 2))
    assert abs(T.root() - 1.0) <= 1e-12


def test_pure_measure_program():
    """the program r^2 (one term, no factor, p = 2) needs no A: roots of r^2 = c, and a level equal to a station's r^2 exactly is
    counted once, at the station"""
    g = O.Grid("R", 0.0, 12.0, 7, {"u": 1})
    prog = (np.array([1.0]), np.array([[0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32), 1)
    A = np.zeros((g.S_patch(), 1))
    st = X.stations(g)
    assert len(st) == 3 * 7 + 2 and st[0] == 0.0 and st[-1] == 12.0 and (np.diff(st) > 0).all()
    on = float(st[11])
    levels = [2.0, 30.25, on * on, 200.0, 0.0]
    for xp in (False, True):
        res = X.crossings(g, A, prog, levels, None, max_cross=3, xp=xp)
        assert res.radius.shape == (3, 5, 1)
        assert list(res.count[:, 0]) == [1, 1, 1, 0, 0] and res.status[0] == 0      # 200 > 144 is never reached; 0 = g(0) is non-negative: no change
        assert (res.dir[0, :3, 0] == 1).all() and (res.dir[1:] == 0).all() and np.isnan(res.radius[1:]).all() and np.isnan(res.radius[0, 3:]).all()
        assert abs(res.radius[0, 0, 0] - np.sqrt(2.0)) <= 1e-9 * g.DX and abs(res.radius[0, 1, 0] - 5.5) <= 1e-9 * g.DX
        assert res.radius[0, 2, 0] == on                              # bitwise the station
    sel = X.select(X.crossings(g, A, prog, [2.0], None, xp=False), 0, "outermost", falling=True)
    assert np.isnan(sel[0])                                           # r^2 rises through 2: no falling crossing


def test_selection_rules():
    rad = np.full((4, 1, 3), np.nan)
    dr = np.zeros((4, 1, 3), dtype=np.int32)
    rad[:3, 0, 0], dr[:3, 0, 0] = [1.0, 2.0, 3.0], [-1, 1, -1]
    rad[:2, 0, 1], dr[:2, 0, 1] = [4.0, 5.0], [-1, 1]
    res = X.Result(rad, dr, np.array([[3, 2, 0]]), np.zeros(3, dtype=np.int32))
    assert np.array_equal(X.select(res, 0, "outermost"), [3.0, 5.0, np.nan], equal_nan=True)
    assert np.array_equal(X.select(res, 0, "innermost"), [1.0, 4.0, np.nan], equal_nan=True)
    assert np.array_equal(X.select(res, 0, "outermost", falling=True), [3.0, 4.0, np.nan], equal_nan=True)
    lam = np.array([0.1, 2.0, 3.5, 5.0, 0.5])
    q = X.quadrant_max(lam, np.array([1.0, np.nan, 3.0, 4.0, 2.0]))
    assert np.array_equal(q, [2.0, 4.0, 3.0, np.nan], equal_nan=True)       # NE, SE, SW, NW


def test_refusals_without_a_device():
    """the program rules are sx_reduce_planes' own, with one output: a term whose out is 1 is refused; sx_bracket_step refuses a
    bracket without a sign change, a = b excepted, and a null pointer"""
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    gp = S.GridParameters(geometry="RL", xmin=0.0, xmax=10.0, num_cells=6, vars={"h": 1, "u": 2})
    from scythe_jl_amd.model import grid_desc
    d, keep = grid_desc(gp)

    def planes(rows):
        t = np.array(rows, dtype=np.int32)
        return lib.sx_reduce_planes(C.byref(d), 0, len(t), t.ctypes.data_as(L.P_I32), 1, None, None)
    assert planes([[0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]]) == 0
    assert planes([[0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0]]) != 0 and b"out = 1" in lib.sx_last_error()
    assert planes([[0, 0, 1, 1, 0, 0, 0, 5, 0, 0, 0]]) != 0               # an RL grid has no z slot
    assert planes([[0, 0, 1, 3, 0, 0, 0, 0, 0, 0, 0]]) != 0               # var out of range
    with pytest.raises(S.ScytheHipError, match="change sign"):
        S.bracket_step([0.0, 1.0, 1.0, 2.0], [0, 0], first=True)
    with pytest.raises(S.ScytheHipError, match="finite a <= b"):
        S.bracket_step([2.0, -1.0, 1.0, 2.0], [0, 0], first=True)
    with pytest.raises(S.ScytheHipError, match="outside the bracket"):
        S.bracket_step([0.0, -1.0, 1.0, 2.0, -1.0, 2.0, 3.0], [0, 0], 0.5, 1e-9)
    st = C.c_int32(0)
    assert lib.sx_bracket_step(None, None, 1, 0.0, 1e-9, C.byref(st)) != 0
