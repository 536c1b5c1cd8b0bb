"""The Float64 results of oracle_np's equation sets, as bytes, before tendency() learned to follow its input's precision:
expdot, impdot and the A coefficients after one Model.step of one small case per equation set (tests/physics.py PER_SET), from the
case's initial condition.  tests/test_physics.py::test_float64_oracle_is_pinned holds every later oracle_np to these bytes.

How the committed .npz was made: this script and tests/physics.py (for PER_SET / case_of, which the parent commit does not have)
were copied into a checkout of the commit before that change and run there, so oracle/oracle_np.py - the only module whose
arithmetic is pinned - was the parent's.  To reproduce: put the parent's oracle/oracle_np.py in place of this tree's and run

    python tests/golden/make_physics_pin_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "physics_f64_pin.npz")


def pin_arrays():
    from oracle import oracle_np as O
    from tests import cases, physics
    out = {}
    for cid in physics.PER_SET:
        case = physics.case_of(cid)[0]
        g = cases.oracle_grid(case)
        m = O.Model(g, case["eq"], case["ts"], case["par"], semiimplicit=case.get("semiimplicit", False),
                    pxi_bar=case["par"].get("Pxi_bar", 0.0))
        pts = g.gridpoints()
        pts = pts.reshape(len(pts), -1)
        m.set_initial(case["ic"](pts))
        E, I, _ = O.tendency(g, case["eq"], case["par"], g.inverse(m.A), pts)
        m.step()
        out[cid + ".expdot"] = E
        if I is not None:
            out[cid + ".impdot"] = I
        out[cid + ".step"] = m.A
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **pin_arrays())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
