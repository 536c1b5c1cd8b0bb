"""CPU-only: the host statements of sx_derive (sx_derive_point, sx_derive_check) against the numpy twin of tests/derive.py, the packer
of function programs, and the named thermodynamic programs against scythe_jl_amd/thermodynamics.py on the reference state."""
import numpy as np
import pytest

from tests import cases
from tests import derive as DV


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def var(n):
    return [(1.0, 0, [(n, "")])]


def exact_programs(gp, names=("h", "u", "v")):
    """the programs of exactly rounded operations only, by name: speed, a potential vorticity and a Rossby number of the wind (u, v)
    with depth 2 + h and f = 0.7 (state source: the parts of the vorticity that need no derivative), and a SELECT on u - 0.3"""
    import scythe_jl_amd as S
    h, u, v = names
    zeta = [(1.0, -1, [(v, "")])] if "L" in gp.geometry else var(v)
    return {"speed": ("sqrt", S.field_programs(S.ModelParameters(grid_params=gp), u, v)["speed2"]),
            "pv": ("div", zeta + [(0.7, 0, [])], [(2.0, 0, []), (1.0, 0, [(h, "")])]),
            "rossby": ("div", zeta, 0.7),
            "sel": ("select", ("sub", var(u), 0.3), ("neg", var(h)), ("abs", var(v)))}


def every_operation(names, has_z, thermo=None):
    """a program that uses every operation once on the planes A, B, C = names; Z where the grid has a vertical; REF and the composites
    from the thermodynamic programs `thermo` (a source with a reference state).  SELECT's argument is a mid offset by a constant."""
    A, B, C = (var(n) for n in names)
    Dm = [(1.0, 0, [(names[1], ""), (names[1], "")]), (1.0, 0, [(names[2], ""), (names[2], "")]), (0.5, 0, [])]      # positive
    out = {"add": ("add", A, B), "sub": ("sub", A, C), "mul": ("mul", A, B), "div": ("div", A, Dm), "neg": ("neg", A), "abs": ("abs", B),
           "min": ("min", A, B), "max": ("max", A, B), "sqrt": ("sqrt", Dm), "select": ("select", ("sub", A, 0.3), A, B), "exp": ("exp", A),
           "log": ("log", Dm), "pow": ("pow", Dm, 0.3), "atan2": ("atan2", A, B), "r": "r"}
    if has_z:
        out["z"] = "z"
    if thermo is not None:
        T, p, q_v = thermo["T"], thermo["p"], thermo["q_v"]
        out.update(T=T, p=p, e=("vapor_pressure", p, q_v), es=("esat_buck", T, p), lv=("l_v", T))
    return out


def euler_state(case, seed=3):
    """(points, values [N, V], ref [3, 3, zDim]): the case's own initial state plus seeded perturbations (s 2, xi 0.01, mu 1e-4, the
    wind 1) - small enough that T stays within 180 .. 330 K and p positive, which every test that uses them asserts"""
    g = cases.oracle_grid(case)
    pts = g.gridpoints()
    rng = np.random.default_rng(seed)
    vals = case["ic"](pts) + rng.standard_normal((len(pts), 5)) * np.array([2.0, 0.01, 1.0e-4, 1.0, 1.0])
    rs = case["par"]["ref_state"]
    return pts, vals, np.stack([rs[k].T for k in ("sbar", "xibar", "mubar")])


def assert_physical(T, p):
    assert np.all((T > 180.0) & (T < 330.0)) and np.all(p > 0.0), (T.min(), T.max(), p.min())


def point_regs(fp, gp, data, r, z=None, ref=None):
    """sx_derive_point at every point: [n_regs, N]"""
    import scythe_jl_amd as S
    data = data[:, :, None] if data.ndim == 2 else data
    planes = sorted({(int(q[3 + f]), int(q[7 + f])) for q in fp.terms for f in range(int(q[2]))})
    nz = 1 if z is None else len(z)
    return np.stack([S.derive_point(fp, planes, [data[i, v - 1, s] for v, s in planes], r[i], 0.0 if z is None else z[i % nz],
                                    None if ref is None else ref[:, :, i % nz]) for i in range(data.shape[0])], axis=1)


def _generic(geometry="RL", n=60, seed=5):
    import scythe_jl_amd as S
    gp = S.GridParameters(geometry=geometry, xmin=0.0, xmax=10.0, num_cells=4, vars={"h": 1, "u": 2, "v": 3},
                          **(dict(zmin=0.0, zmax=3.0, zDim=6) if "Z" in geometry else {}))
    rng = np.random.default_rng(seed)
    return gp, rng.standard_normal((n, 3)), np.abs(rng.standard_normal(n)) * 3.0 + 0.1


def test_point_exact_operations_bitwise():
    import scythe_jl_amd as S
    gp, data, r = _generic()
    data[:6, 1] = data[:6, 2] = 0.0                 # a zero radicand
    data[6:9, 0] = -2.0                             # a zero denominator of the potential vorticity
    fp = S.pack_function_program(gp, exact_programs(gp))
    want = DV.values64(fp, data, r)
    assert np.isinf(want).any() or np.isnan(want).any()
    assert _bits(point_regs(fp, gp, data, r)) == _bits(want)


def test_point_every_operation_and_thermo_within_bound():
    import scythe_jl_amd as S
    case = cases.rz_euler(num_cells=3, zDim=9)
    gp, mp = cases.hip_params(case)
    pts, vals, ref = euler_state(case)
    r, z = pts[:, 0], pts[:9, 1]
    tp = S.thermo_programs(mp)
    groups = [every_operation(("s", "xi", "mu"), True, tp), {k: tp[k] for k in tp if k != "theta_e"}, {"theta_e": tp["theta_e"]}]
    for outs in groups:
        fp = S.pack_function_program(gp, outs)
        truth, bnd = DV.bound(fp, vals, r, z, ref)
        if "T" in outs:
            assert_physical(truth[fp.reg_dst[list(outs).index("T")]], truth[fp.reg_dst[list(outs).index("p")]])
        keep = ~DV.mask(fp, truth, bnd)
        assert keep.mean() >= 0.99
        got = point_regs(fp, gp, vals, r, z, ref)
        err = np.abs(got - truth).astype(np.float64)
        worst = np.max(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))[:, keep], axis=1)
        print("registers of %s: worst |got - xp| / bound = %.3g" % (list(outs)[:3], worst.max()))
        assert np.all(err[:, keep] <= bnd[:, keep]), (list(outs), worst)


def test_nan_and_inf_placement():
    import scythe_jl_amd as S
    gp, data, r = _generic(n=8)
    data[:, 0] = [-1.0, 0.0, 1.0, -0.0, 4.0, np.nan, np.inf, -np.inf]
    fp = S.pack_function_program(gp, {"root": ("sqrt", var("h")), "log": ("log", var("h")), "inv": ("div", 1.0, var("h")),
                                      "min": ("min", var("h"), 2.0), "sel": ("select", var("h"), 1.0, -1.0)})
    got = point_regs(fp, gp, data, r)[fp.reg_dst]
    assert _bits(got) == _bits(DV.values64(fp, data, r)[fp.reg_dst])
    with np.errstate(all="ignore"):
        assert _bits(got[0]) == _bits(np.sqrt(0.0 + data[:, 0])) and np.isnan(got[0][[0, 5, 7]]).all() and got[0][4] == 2.0
        assert got[1][1] == -np.inf and got[1][3] == -np.inf and np.isnan(got[1][0])
        assert got[2][1] == np.inf and got[2][3] == np.inf and got[2][6] == 0.0      # a mid starts from +0.0: -0.0 arrives as +0.0
    assert np.isnan(got[3][5]) and got[3][6] == 2.0 and got[3][7] == -np.inf
    assert list(got[4]) == [-1.0, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, -1.0]          # a NaN takes c


def test_check_refusals():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    gp, _, _ = _generic("RL")
    gz, _, _ = _generic("RLZ")
    one = S.companion_params(gp, names=["a"])
    FP = S.FunctionProgram
    ok = S.pack_function_program(gp, [("sqrt", var("u"))])
    S.derive_check(gp, one, ok)
    S.derive_check(gz, S.companion_params(gz, names=["a"]), S.pack_function_program(gz, ["z"]))
    S.derive_check(gp, one, S.pack_function_program(gp, [("ref", "xibar", "z")]), has_ref_state=True)

    def refused(match, fp=ok, src=gp, dst=one, **kw):
        with pytest.raises(S.ScytheHipError, match=match):
            S.derive_check(src, dst, fp, **kw)
    ops = lambda *rows: np.array(rows, dtype=np.int32)
    refused("SX_REDUCE_STATE holds the values only", S.pack_function_program(gp, [("sqrt", [(1.0, 0, [("u", "r")])])]), source="state")
    refused("n_out must be 0 .. 16", FP(ok.coef, ok.terms, 17, ok.ops, [], [0], ["a"]))
    refused("mid 1 has no term", FP(ok.coef, ok.terms, 2, ok.ops, [], [0], ["a"]))
    refused("names its own or a later register", FP(ok.coef, ok.terms, 1, ops([L.FN["sqrt"], 1, 0, 0]), [], [1], ["a"]))
    refused("names its own or a later register", FP(ok.coef, ok.terms, 1, ops([L.FN["add"], 0, 2, 0], [L.FN["neg"], 0, 0, 0]), [], [1], ["a"]))
    refused("names constant 1 of 1", FP(ok.coef, ok.terms, 1, ops([L.FN["add"], 0, -2, 0]), [1.0], [1], ["a"]))
    refused("unknown fn 24", FP(ok.coef, ok.terms, 1, ops([24, 0, 0, 0]), [], [1], ["a"]))
    refused("unknown fn -1", FP(ok.coef, ok.terms, 1, ops([-1, 0, 0, 0]), [], [1], ["a"]))
    refused("Z on a grid without a vertical", S.pack_function_program(gp, ["z"]))
    refused("the source has no reference state", S.pack_function_program(gp, [("ref", "sbar", "")]))
    refused("REF of profile 3", FP(ok.coef, ok.terms, 1, ops([L.FN["ref"], 3, 0, 0]), [], [1], ["a"]), has_ref_state=True)
    refused("n_ops = 33 is outside", FP(ok.coef, ok.terms, 1, ops(*[[L.FN["neg"], 0, 0, 0]] * 33), [], [1], ["a"]))
    refused("n_consts = 17 is outside", FP(ok.coef, ok.terms, 1, ok.ops, np.zeros(17), [1], ["a"]))
    refused(r"reg_dst\[0\] = 2 is outside the registers 0 .. 1", FP(ok.coef, ok.terms, 1, ok.ops, [], [2], ["a"]))
    refused(r"reg_dst\[0\] = -1 is outside", FP(ok.coef, ok.terms, 1, ok.ops, [], [-1], ["a"]))
    refused("2 entries of reg_dst for the destination's 1 variables", FP(ok.coef, ok.terms, 1, ok.ops, [], [0, 1], ["a", "b"]))
    gp5 = S.GridParameters(geometry="RL", xmin=0.0, xmax=10.0, num_cells=5, vars={"h": 1, "u": 2, "v": 3})
    refused("differs from the source's in num_cells", dst=S.companion_params(gp5, names=["a"]))
    # null pointers with a non-zero count, through the C ABI itself
    import ctypes as C
    lib = S.load()
    ds, k1 = S.model.grid_desc(gp)
    dd, k2 = S.model.grid_desc(one)
    P = lambda a: a.ctypes.data_as(L.P_I32)
    call = lambda terms, ops_, reg: lib.sx_derive_check(C.byref(ds), 0, C.byref(dd), 0, 1, terms, 1, 1, ops_, 0, 1, reg)
    assert call(P(ok.terms), P(ok.ops), P(ok.reg_dst)) == 0
    assert call(None, P(ok.ops), P(ok.reg_dst)) == 1 and b"null terms" in lib.sx_last_error()
    assert call(P(ok.terms), None, P(ok.reg_dst)) == 1 and b"null ops" in lib.sx_last_error()
    assert call(P(ok.terms), P(ok.ops), None) == 1 and b"null reg_dst" in lib.sx_last_error()
    regs = np.zeros(2)
    assert lib.sx_derive_point(1, None, P(ok.terms), 1, 1, P(ok.ops), 0, None, 0, None, None, 1.0, 0.0, None, regs.ctypes.data_as(L.P_D)) == 1


def test_pack_function_program():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    gp, _, _ = _generic()
    u2 = [(1.0, 0, [("u", ""), ("u", "")])]
    fp = S.pack_function_program(gp, {"a": ("sqrt", u2), "b": ("add", ("sqrt", list(u2)), 2.0), "c": ("mul", "a", ("add", "a", 2.0)), "d": u2})
    # sharing: one mid, one root, one sum, one constant; an output that is a term list is its mid
    assert fp.n_mid == 1 and len(fp.consts) == 1 and [int(q[0]) for q in fp.ops] == [L.FN["sqrt"], L.FN["add"], L.FN["mul"]]
    assert list(fp.reg_dst) == [1, 2, 3, 0] and fp.names == ["a", "b", "c", "d"]
    # evaluation order: every register operand is lower than the operation's own register
    tp = S.thermo_programs(cases.hip_params(cases.rz_euler())[1])
    big = S.pack_function_program(cases.hip_params(cases.rz_euler())[0], {k: tp[k] for k in tp if k != "theta_e"})
    for i, (fn, a, b, c) in enumerate(big.ops):
        name = DV.NAME[int(fn)]
        assert all(x < big.n_mid + i for x in (a, b, c)[:L.FN_ARITY.get(name, 2)])
    # -0.0 and 0.0 are two constants
    assert len(S.pack_function_program(gp, [("add", ("mul", u2, 0.0), -0.0)]).consts) == 2
    # the limits
    chain = u2
    for _ in range(32):
        chain = ("neg", chain)
    assert len(S.pack_function_program(gp, [chain]).ops) == 32
    with pytest.raises(ValueError, match="33 operations"):
        S.pack_function_program(gp, [("neg", chain)])
    mids = [[(float(k + 1), 0, [("u", "")])] for k in range(17)]
    assert S.pack_function_program(gp, mids[:16]).n_mid == 16
    with pytest.raises(ValueError, match="17 mids"):
        S.pack_function_program(gp, mids)
    consts = u2
    for k in range(17):
        if k == 16:
            with pytest.raises(ValueError, match="17 constants"):
                S.pack_function_program(gp, [("add", consts, 16.5)])
        else:
            consts = ("add", consts, float(k) + 0.5)
    with pytest.raises(ValueError, match="cycle"):
        S.pack_function_program(gp, {"a": ("neg", "b"), "b": ("sqrt", "a")})
    with pytest.raises(ValueError, match="cycle"):
        S.pack_function_program(gp, {"a": ("neg", "a")})
    with pytest.raises(ValueError, match="neither an output"):
        S.pack_function_program(gp, {"a": ("neg", "q")})
    with pytest.raises(ValueError, match="unknown operation"):
        S.pack_function_program(gp, [("cbrt", u2)])
    with pytest.raises(ValueError, match="bare number"):
        S.pack_function_program(gp, [1.0])


def test_function_programs_by_equation_set():
    import scythe_jl_amd as S
    gp, mp = cases.hip_params(cases.rl_slab(num_cells=6))
    fp = S.function_programs(mp)
    assert set(fp) == {"speed", "inflow_angle", "potential_vorticity", "rossby_number"}
    assert fp["potential_vorticity"][2][0] == (2000.0, 0, []) and fp["rossby_number"][2] == 5.0e-5          # Hfree and f of the set
    S.pack_function_program(gp, fp)


def test_thermo_programs_reproduce_the_reference_state():
    """level by level on the reference state itself (zero perturbation): thermo_programs against thermodynamics.py's host functions"""
    import scythe_jl_amd as S
    from scythe_jl_amd import thermodynamics as TH
    case = cases.rz_euler(num_cells=3, zDim=9)
    gp, mp = cases.hip_params(case)
    rs = case["par"]["ref_state"]
    ref = np.stack([rs[k].T for k in ("sbar", "xibar", "mubar")])
    nz = 9
    zero = np.zeros((nz, 5))
    r, z = np.ones(nz), cases.oracle_grid(case).gridpoints()[:nz, 1]
    sb, xb, mb = ref[0, 0], ref[1, 0], ref[2, 0]
    q_v, rho_d, Tk, p = TH.thermodynamic_tuple(sb, xb, mb)
    es = TH.sat_pressure_liquid_buck(Tk, p)
    host = dict(q_v=q_v, rho_d=rho_d, T=Tk, p=p, rho=rho_d * (1.0 + q_v), theta=TH.potential_temperature(sb, xb, mb),
                theta_e=TH.reversible_theta_e(sb, xb, mb), theta_rho=TH.theta_rho(sb, xb, mb), rh=TH.vapor_pressure(p, q_v) / es,
                q_sat=TH.q_sat_liquid(Tk, p))
    tp = S.thermo_programs(mp)
    assert set(tp) == set(host)
    assert_physical(Tk, p)
    for outs in ({k: tp[k] for k in tp if k != "theta_e"}, {"theta_e": tp["theta_e"]}):
        fp = S.pack_function_program(gp, outs)
        truth, bnd = DV.bound(fp, zero, r, z, ref)
        got = point_regs(fp, gp, zero, r, z, ref)
        for name, k in zip(outs, fp.reg_dst):
            assert np.all(np.abs(got[k] - host[name]) <= 2.0 * bnd[k]), name        # two float64 evaluations, each within bound of the truth
            assert np.all(np.abs(got[k] - truth[k]) <= bnd[k]), name


def test_thermo_programs_of_rainfall_test():
    """the rainfall_test branch: q_l = ahyp(mu_c) + ahyp(mu_r) and rho = rho_d (1 + q_t).  The nine outputs without theta_e pack; theta_e
    with the set's own q_l needs 34 operations and is refused by the packer; with one liquid variable it fits (32) and is, like
    theta_rho, thermodynamics.py's function of mu_l.  Evaluated by sx_derive_point on the case's initial state."""
    import scythe_jl_amd as S
    from scythe_jl_amd import thermodynamics as TH
    from tests import rainfall
    case = rainfall.rz_rain(num_cells=3, zDim=9)
    gp, mp = cases.hip_params(case)
    pts = cases.oracle_grid(case).gridpoints()
    vals = case["ic"](pts)
    rs = case["par"]["ref_state"]
    ref = np.stack([rs[k].T for k in ("sbar", "xibar", "mubar")])
    r, z, lev = pts[:, 0], pts[:9, 1], np.arange(len(pts)) % 9
    tp = S.thermo_programs(mp)
    with pytest.raises(ValueError, match="34 operations"):
        S.pack_function_program(gp, {"theta_e": tp["theta_e"]})
    nine = {k: tp[k] for k in tp if k != "theta_e"}
    fp = S.pack_function_program(gp, nine)
    assert len(fp.ops) <= 32 and fp.n_mid == 5
    Sx, XI, MU = (vals[:, j] + ref[j, 0][lev] for j in range(3))
    q_v, rho_d, Tk, p = TH.thermodynamic_tuple(Sx, XI, MU)
    q_l = TH.ahyp(vals[:, 5]) + TH.ahyp(vals[:, 6])
    assert_physical(Tk, p)
    assert q_l.min() > 0.0
    theta = TH.potential_temperature(Sx, XI, MU)
    host = dict(q_v=q_v, rho_d=rho_d, T=Tk, p=p, rho=rho_d * (1.0 + (q_v + q_l)), theta=theta,
                theta_rho=theta * (1.0 + (q_v / TH.Eps)) / (1.0 + (q_v + q_l)), rh=TH.vapor_pressure(p, q_v) / TH.sat_pressure_liquid_buck(Tk, p),
                q_sat=TH.q_sat_liquid(Tk, p))

    def held(fp, host):
        truth, bnd = DV.bound(fp, vals, r, z, ref)
        got = point_regs(fp, gp, vals, r, z, ref)
        for name, k in zip(fp.names, fp.reg_dst):
            assert np.all(np.abs(got[k] - truth[k]) <= bnd[k]), name
            assert np.all(np.abs(got[k] - host[name]) <= 2.0 * bnd[k]), name      # two float64 evaluations, each within bound of the truth
    held(fp, host)
    cloud = S.thermo_programs(mp, liquid=("ahyp", var("mu_c")))
    fe = S.pack_function_program(gp, {"theta_e": cloud["theta_e"]})
    assert len(fe.ops) == 32
    held(fe, dict(theta_e=TH.reversible_theta_e(Sx, XI, MU, vals[:, 5])))
    held(S.pack_function_program(gp, {"theta_rho": cloud["theta_rho"]}), dict(theta_rho=TH.theta_rho(Sx, XI, MU, vals[:, 5])))
