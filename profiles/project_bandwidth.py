"""k_project against k_stats on the bench grid (RLZ 513 x 256 x 64, six variables): the figures of DESIGN.md 22.

A 2-output, 4-plane program (vorticity and kinetic energy of (u, v): planes v_r, v, u_l, u) is projected into a two-variable
companion REPS times with the handle's timers on; k_stats accumulates a MAX / SUM set of the same program in the same session.
Prints, per kernel, the median and the spread of the per-launch time, sx_kernel_bytes, the bandwidth that gives and its fraction of
the HBM peak, and the time of the companion's own forward chain (k_fl_forward ... k_solve of the companion handle)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import scythe_jl_amd as S          # noqa: E402
from tests import cases            # noqa: E402

HBM_PEAK = 8.0e12                  # bytes / s, MI355X
REPS = 20


def per_launch(tile, name, launch):
    """per-launch milliseconds of kernel `name` over REPS launches, each timed on its own"""
    ms = []
    for _ in range(REPS):
        tile.reset_timers()
        launch()
        tile.synchronize()
        ms.append(tile.timers()[name][0])
    return np.array(ms)


def main():
    case = cases.rlz_hrbl(num_cells=171, zDim=64, ring_L=256)
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp)
    pts = S.getGridpoints(tile)
    tile.set_physical_values(case["ic"](pts))
    tile.spectralTransform_()
    tile.splineTransform_()
    tile.tileTransform_()
    fp = S.field_programs(mp)
    outs = [fp["vorticity"], fp["kinetic_energy"]]
    terms = S.program_of_outputs(outs)
    comp = tile.project_companion(["zeta", "ke"])
    tile.enable_timers(True)
    comp.enable_timers(True)
    for _ in range(3):                                   # warm-up: first launches, the companion's plans
        tile.project(terms, comp)
    res = {"N": tile.N, "planes": len(S.reduce_planes(gp, terms)), "reps": REPS}
    ms = per_launch(tile, "k_project", lambda: tile.project(terms, comp))
    b = tile.kernel_bytes("k_project")
    res["k_project"] = dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()), bytes=b,
                            GBps=b / np.median(ms) / 1e6, of_hbm_peak=b / (np.median(ms) * 1e-3) / HBM_PEAK)
    comp.reset_timers()
    for _ in range(REPS):
        tile.project(terms, comp)
    chain = {k: v[0] / v[1] for k, v in comp.timers().items() if v[1]}
    res["companion_transform"] = dict(ms_per_call=float(sum(chain.values())), kernels=chain)
    tile.set_statistics([("max", outs[0]), ("sum", outs[1])], "physical")
    for _ in range(3):
        tile.accumulate_statistics(0.0, 1.0)
    t = [0.0]

    def sample():
        t[0] += 1.0
        tile.accumulate_statistics(t[0], 1.0)
    ms = per_launch(tile, "k_stats", sample)
    b = tile.kernel_bytes("k_stats")
    res["k_stats"] = dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()), bytes=b,
                          GBps=b / np.median(ms) / 1e6, of_hbm_peak=b / (np.median(ms) * 1e-3) / HBM_PEAK)
    print(json.dumps(res))
    tile.close()


if __name__ == "__main__":
    main()
