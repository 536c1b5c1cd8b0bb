"""CPU-only: the host statements of sx_project (sx_project_point, sx_project_check), the numpy twin's two pins (tests/project.py), the
companion descriptors and the field programs."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import distribution as D
from tests import project as PJ

XP = O.XP


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def limit_program(seed, V, D_slots, n_out=16, n_terms=64, n_planes=16, source="physical"):
    """A seeded random program at the limits: n_terms terms over n_out outputs (every output has one), exactly n_planes distinct
    planes, up to 4 factors, every p in -2 .. 2; returns (coef, packed int32 [n_terms, 11], n_out) and the planes in first-use order"""
    rng = np.random.default_rng(seed)
    allp = [(v, s) for v in range(1, V + 1) for s in (range(D_slots) if source == "physical" else (0,))]
    planes = [allp[i] for i in rng.permutation(len(allp))[:min(n_planes, len(allp))]]
    coef = rng.uniform(-2.0, 2.0, n_terms)
    packed = np.zeros((n_terms, 11), dtype=np.int32)
    for t in range(n_terms):
        nf = 4 if t < 4 else int(rng.integers(0, 5))
        packed[t, :3] = t % n_out, (t % 5) - 2, nf
        for f in range(nf):
            v, s = planes[(4 * t + f) % len(planes)] if t < 4 else planes[int(rng.integers(len(planes)))]
            packed[t, 3 + f], packed[t, 7 + f] = v, s
    return (coef, packed, n_out), planes


def test_project_point_is_program_values64_bitwise():
    import scythe_jl_amd as S
    V, Dn = 5, 7
    for seed in range(6):
        prog, _ = limit_program(100 + seed, V, Dn)
        planes = [(v, s) for v in range(1, V + 1) for s in range(Dn)]
        used = sorted({(int(prog[1][t, 3 + f]), int(prog[1][t, 7 + f])) for t in range(64) for f in range(prog[1][t, 2])})
        assert len(used) == 16 and {int(p) for p in prog[1][:, 1]} == {-2, -1, 0, 1, 2} and prog[1][:, 2].max() == 4
        rng = np.random.default_rng(seed)
        n = 40
        data = rng.standard_normal((n, V, Dn)) * 10.0 ** rng.integers(-3, 4, (n, V, Dn))
        special = [0.0, -0.0, np.inf, -np.inf, np.nan]
        for i in range(n // 2):
            data[i, rng.integers(V), rng.integers(Dn)] = special[i % 5]
            v, s = used[i % 16]
            data[i, v - 1, s] = special[(i // 2) % 5]
        r = np.abs(rng.standard_normal(n)) * 100.0 + 0.5
        want = np.stack([D.program_values64(data, r, prog, o) for o in range(16)], axis=1)
        assert np.isnan(want).any() and np.isinf(want).any()
        got = np.stack([S.project_point(prog, used, [data[i, v - 1, s] for v, s in used], r[i]) for i in range(n)])
        assert _bits(got) == _bits(want), seed
    # terms given as tuples by index: the packer project shares with reduce
    out = S.project_point([(0, 2.0, 2, []), (1, -1.0, -1, [(1, 0), (2, 1)]), (0, 0.5, 0, [(1, 0)])], [(1, 0), (2, 1)], [3.0, -4.0], 2.0)
    assert list(out) == [0.0 + 2.0 * 4.0 + 0.5 * 3.0, -1.0 * 0.5 * 3.0 * -4.0]
    with pytest.raises(S.ScytheHipError, match="does not list"):
        S.project_point([(0, 1.0, 0, [(3, 0)])], [(1, 0)], [1.0], 1.0)


def _gp(**kw):
    import scythe_jl_amd as S
    base = dict(geometry="RLZ", xmin=0.0, xmax=10.0, num_cells=4, zmin=0.0, zmax=3.0, zDim=9, vars={"u": 1, "v": 2})
    base.update(kw)
    return S.GridParameters(**base)


def test_project_check_refusals():
    import scythe_jl_amd as S
    src = _gp()
    terms = [(0, 1.0, 0, [("v", "r")]), (0, 1.0, -1, [("v", "")]), (1, 0.5, 0, [("u", ""), ("u", "")])]
    dst = S.companion_params(src, "R0", "R0", "R0", "R0", "R0", names=["zeta", "ke"])
    S.project_check(src, dst, terms)
    S.project_check(src, dst, terms, var_dst=("ke", "zeta"))
    # a destination that truncates more: accepted
    small = S.companion_params(src, "R0", "R0", "R0", "R0", "R0", names=["zeta", "ke"])
    small.b_zDim = 4
    S.project_check(src, small, terms)

    def refused(match, s=src, d=dst, t=terms, **kw):
        with pytest.raises(S.ScytheHipError, match=match):
            S.project_check(s, d, t, **kw)

    def other(**kw):
        d = S.companion_params(_gp(**kw), "R0", "R0", "R0", "R0", "R0", names=["zeta", "ke"])
        return d
    refused("differs from the source's in geometry", d=S.companion_params(_gp(geometry="RL", zDim=0), "R0", "R0", "R0", names=["zeta", "ke"]))
    refused("in xmin", d=other(xmin=1.0))
    refused("in xmax", d=other(xmax=11.0))
    refused("in num_cells", d=other(num_cells=5))
    refused("in ring table", d=other(ring_uniform_L=16))
    refused("in zDim", d=other(zDim=10))
    refused("in zmin", d=other(zmin=-1.0))
    refused("in zmax", d=other(zmax=4.0))
    refused("not the destination's number of variables", d=S.companion_params(src, names=["a", "b", "c"]))
    refused("not a permutation", var_dst=(2, 2))
    refused("not a permutation", var_dst=(0, 1))
    refused("not a permutation", var_dst=(1, 3))
    refused("output 1 has no term", t=[terms[0], (2, 1.0, 0, [("u", "")])], d=S.companion_params(src, names=["a", "b", "c"]))
    # everything sx_reduce_planes refuses
    refused("SX_REDUCE_STATE holds the values only", source="state")
    refused("r_power", t=terms[:2] + [(1, 1.0, 3, [("u", "")])])
    refused("not a derivative slot", t=terms[:2] + [(1, 1.0, 0, [("u", 7)])])
    refused("1-based and at most nvars", t=terms[:2] + [(1, 1.0, 0, [(3, 0)])])
    many = [(o, 1.0, 0, [("u", "")]) for o in range(17)]
    refused("n_out must be 0 .. 16", t=many, d=S.companion_params(src, names=["v%d" % i for i in range(17)]))
    # one-tile patches only, and null pointers with a non-zero count: through the descriptors themselves
    lib = S.load()
    from scythe_jl_amd import model as M, _lib as L
    ds, k1 = M.grid_desc(src, 0, 2)
    dd, k2 = M.grid_desc(dst)
    coef, packed, n_out = S.pack_reduce_program(src, terms)
    vd = np.array([1, 2], dtype=np.int32)
    args = lambda a, b, t, v: lib.sx_project_check(C.byref(a), C.byref(b), 0, len(coef), t, n_out, v)
    assert args(ds, dd, packed.ctypes.data_as(L.P_I32), vd.ctypes.data_as(L.P_I32)) == 1 and b"one-tile" in lib.sx_last_error()
    ds, k1 = M.grid_desc(src)
    assert args(ds, dd, None, vd.ctypes.data_as(L.P_I32)) == 1 and b"null terms" in lib.sx_last_error()
    assert args(ds, dd, packed.ctypes.data_as(L.P_I32), None) == 1 and b"null var_dst" in lib.sx_last_error()
    assert args(ds, dd, packed.ctypes.data_as(L.P_I32), vd.ctypes.data_as(L.P_I32)) == 0


def _case_values(g, seed):
    pts = g.gridpoints()
    pts = pts.reshape(len(pts), -1)
    rng = np.random.default_rng(seed)
    return pts, rng.standard_normal((len(pts), g.V))


@pytest.mark.parametrize("geometry", ["R", "RLZ"])
def test_twin_identity_program_is_the_forward_transform(geometry):
    """1 . field(v, 0) projected is oracle_np's forward + spline transform of that variable, exactly"""
    import scythe_jl_amd as S
    kw = dict(zmin=0.0, zmax=3.0, zDim=9) if geometry == "RLZ" else {}
    g = O.Grid(geometry, 0.0, 10.0, 5, {"a": 1, "b": 2}, BCL={"b": "R1T0"}, BCR={"b": "R1T1"}, **kw)
    pts, vals = _case_values(g, 3)
    gp = S.GridParameters(geometry=geometry, xmin=0.0, xmax=10.0, num_cells=5, vars={"a": 1, "b": 2}, **kw)
    prog = S.pack_reduce_program(gp, [(0, 1.0, 0, [("b", "")])])
    dst = PJ.companion(g, ["f"], BCL={"f": "R1T0"}, BCR={"f": "R1T1"})
    A = PJ.project64(dst, PJ.values(vals, pts[:, 0], prog))
    want = g.spline_transform(g.forward(np.asfortranarray(vals)))[:, 1]
    assert _bits(A[:, 0]) == _bits(want)


def test_twin_reproduces_r_squared():
    """the program r^2 (no factors, p = 2) into an R0 / R0 variable evaluates back to r^2 between the gridpoints, to longdouble
    rounding: the l_q penalty acts on the third derivative, which r^2 has none of (default l_q = 2)"""
    import scythe_jl_amd as S
    g = O.Grid("R", 1.0, 9.0, 8, {"a": 1})
    assert g.l_q == 2.0
    pts, vals = _case_values(g, 5)
    gp = S.GridParameters(geometry="R", xmin=1.0, xmax=9.0, num_cells=8, vars={"a": 1})
    prog = S.pack_reduce_program(gp, [(0, 1.0, 2, [])])
    dst = PJ.companion(g, ["f"])
    v = PJ.values(vals, pts[:, 0], prog)
    assert _bits(v[:, 0]) == _bits(pts[:, 0] * pts[:, 0])
    radii = np.linspace(1.0, 9.0, 41) + 0.0371
    radii = radii[radii < 9.0]
    got = PJ.radial_values(dst, PJ.project_xp(dst, v), 0, radii)
    want = radii.astype(XP) ** 2
    # the gridpoint values are r^2 rounded to float64 (2^-53 relative): the spline of those roundings is that far from r^2, and the
    # longdouble solve adds its own few hundred ulp_xp x the condition of the 11 x 11 system
    assert float(np.max(np.abs(got - want) / want)) < 64 * 2.0 ** -53
    got64 = PJ.radial_values(dst, PJ.project64(dst, v), 0, radii)
    assert float(np.max(np.abs(got64 - want) / want)) < 1e-10


def test_companion_params_default_is_the_one_variable_psi_companion():
    """names=None: the descriptor companion_grid has always made, byte for byte"""
    import scythe_jl_amd as S
    from scythe_jl_amd import model as M
    gp = _gp(ring_uniform_L=16, BCB={"u": "R1T1"})
    for kw in (dict(), dict(bcb="R1T1", bct="R1T0"), dict(bcl="R0", bcl_k0="R0", bcr="R0", name="F")):
        name = kw.get("name", "psi")
        args = dict(bcl="R1T0", bcl_k0="R1T1", bcr="R1T0", bcb="R0", bct="R0")
        args.update({k: v for k, v in kw.items() if k != "name"})
        old = S.GridParameters(geometry=gp.geometry, xmin=gp.xmin, xmax=gp.xmax, num_cells=gp.num_cells, l_q=gp.l_q, BCL={name: args["bcl"]},
                               BCR={name: args["bcr"]}, BCL_k0={name: args["bcl_k0"]}, zmin=gp.zmin, zmax=gp.zmax, zDim=gp.zDim, b_zDim=gp.b_zDim,
                               BCB={name: args["bcb"]}, BCT={name: args["bct"]}, vars={name: 1}, ring_uniform_L=gp.ring_uniform_L)
        new = S.companion_params(gp, **kw)
        assert new == old
        (d0, k0), (d1, k1) = M.grid_desc(old), M.grid_desc(new)
        skip = {"bcl", "bcl_k0", "bcr", "bcb", "bct"}                       # pointers: compared by what they point to
        for f, _ in d0._fields_:
            if f not in skip:
                assert getattr(d0, f) == getattr(d1, f), f
        for k in k0:
            assert list(k0[k]) == list(k1[k]), k
    many = S.companion_params(gp, bcr={"zeta": "R1T0"}, bcb="R1T1", names=["zeta", "ke"])
    assert many.vars == {"zeta": 1, "ke": 2} and many.BCR == {"zeta": "R1T0", "ke": "R0"} and many.BCB == {"zeta": "R1T1", "ke": "R1T1"}
    with pytest.raises(ValueError):
        S.companion_params(gp, names=["a", "a"])


def test_field_programs_and_invariants_share_their_terms():
    import scythe_jl_amd as S
    gp = S.GridParameters(geometry="RL", xmin=0.0, xmax=10.0, num_cells=4, vars={"h": 1, "u": 2, "v": 3})
    mp = S.ModelParameters(equation_set="LinearShallowWaterRL", grid_params=gp, physical_params={"g": 9.81, "H": 100.0})
    fp = S.field_programs(mp)
    assert fp["vorticity"] == [(1.0, 0, [("v", "r")]), (1.0, -1, [("v", "")]), (-1.0, -1, [("u", "l")])]
    assert fp["divergence"] == [(1.0, 0, [("u", "r")]), (1.0, -1, [("u", "")]), (1.0, -1, [("v", "l")])]
    assert fp["kinetic_energy"] == [(0.5, 0, [("u", ""), ("u", "")]), (0.5, 0, [("v", ""), ("v", "")])]
    assert fp["speed2"] == [(1.0, 0, [("u", ""), ("u", "")]), (1.0, 0, [("v", ""), ("v", "")])]
    inv = S.invariants(mp)
    assert list(inv) == [(0, 1.0, 0, [("h", "")]), (1, 0.5 * 9.81, 0, [("h", ""), ("h", "")]), (1, 50.0, 0, [("u", ""), ("u", "")]),
                         (1, 50.0, 0, [("v", ""), ("v", "")])] and inv.names == ["mass", "energy"]
    rz = S.ModelParameters(grid_params=S.GridParameters(geometry="RZ", xmin=0.0, xmax=1.0, num_cells=4, zDim=8, zmax=1.0, vars={"u": 1, "v": 2}))
    assert S.field_programs(rz)["vorticity"] == [(1.0, 0, [("v", "r")])] and S.field_programs(rz)["divergence"] == [(1.0, 0, [("u", "r")])]
    one = S.ModelParameters(grid_params=S.GridParameters(geometry="R", xmin=0.0, xmax=1.0, num_cells=4, vars={"h": 1, "u": 2}))
    assert "vorticity" not in S.field_programs(one) and S.field_programs(one)["kinetic_energy"] == [(0.5, 0, [("u", ""), ("u", "")])]
    assert S.program_of_outputs([fp["speed2"], fp["vorticity"][:1]]) == [(0, 1.0, 0, [("u", ""), ("u", "")]), (0, 1.0, 0, [("v", ""), ("v", "")]),
                                                                         (1, 1.0, 0, [("v", "r")])]
