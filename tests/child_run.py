"""One GPU job in a fresh child process started with SX_* switches set, as a user sets them: before the process starts.  (The
library reads every switch once per handle, at sx_create, so a monkeypatch.setenv before a handle is created reaches that handle
too; tests/test_gpu_static_switches.py holds that with two handles in one process.)

run_in_child(tmp_path, job, overrides): the child is `python -m tests.child_run <job json> <out.npz>` with os.environ | overrides
(every queue and device variable inherited as it is), one child at a time, under a time limit.  The child writes the job's arrays
to the .npz; the parent compares them with run_job(job) in its own process and with the oracle.  A child that dies on a signal or
hangs ends the whole session (pytest.exit): after a crashed or hung GPU process nothing more may start on the GPU.

A job is JSON: {"kind": "spline" | "rz_transforms" | "model" | "forward" | "physics" (tests/physics.py: {"kind", "id"}), "cases": [[maker, kwargs, grid overrides(, storage)],
...], "steps": n} with `maker` a function of tests/cases.py and `storage` a GridParameters.storage (default "f64")."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_case(spec):
    from tests import cases
    maker, kw, grid = spec[:3]
    case = getattr(cases, maker)(**kw)
    case["grid"].update(grid)
    return case


def forward_inputs(N, V, s_patch, seed=11):
    """The random inputs of a "forward" job: physical values [N, V] and A coefficients [s_patch, V]."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, V)), rng.standard_normal((s_patch, V))


def run_job(job):
    """The job's arrays, in this process: {name: ndarray}."""
    import scythe_jl_amd as S
    from tests import cases
    out = {}
    if job["kind"] == "physics":             # sx_physics at t = 1..4 on the case tests/physics.py names (test_gpu_physics.py)
        from tests import physics
        return physics.device_run(job["id"])
    for i, spec in enumerate(job["cases"]):
        case = make_case(spec)
        if job["kind"] == "spline":          # splineTransform! on random B (tests/test_gpu_solve.py)
            gp, mp = cases.hip_params(case)
            g = S.Grid(gp, mp)
            g.set_patch_spectral_b(np.random.default_rng(5).standard_normal((int(g.dims.s_patch), g.V)))
            g.splineTransform_()
            out["a%d" % i] = g.patchSpectral
            g.close()
        elif job["kind"] == "rz_transforms":     # tileTransform! and spectralTransform! on random data (test_gpu_parity.py)
            gp, mp = cases.hip_params(case)
            g = S.Grid(gp, mp)
            rng = np.random.default_rng(9)
            a = rng.standard_normal((int(g.dims.s_patch), g.V))
            vals = rng.standard_normal((g.N, g.V))
            g.set_patch_spectral_a(a)
            g.tileTransform_()
            out["phys%d" % i] = g.physical
            g.set_physical_values(vals)
            g.spectralTransform_()
            out["spec%d" % i] = g.spectral
            g.close()
        elif job["kind"] == "forward":           # spectralTransform! + splineTransform!, tileTransform! (test_gpu_forward.py)
            gp, mp = cases.hip_params(case, spec[3] if len(spec) > 3 else "f64")
            g = S.Grid(gp, mp)
            vals, a = forward_inputs(g.N, g.V, int(g.dims.s_patch))
            g.set_physical_values(vals)
            g.spectralTransform_()
            out["b%d" % i] = g.spectral
            g.splineTransform_()
            out["a%d" % i] = g.patchSpectral
            g.set_patch_spectral_a(a)
            g.tileTransform_()
            out["phys%d" % i] = g.physical
            g.close()
        elif job["kind"] == "model":             # job["steps"] model steps from the case's initial condition
            hip = cases.HipModel(case)
            for _ in range(job["steps"]):
                hip.step()
            out["var%d" % i] = hip.run.tiles[0].var_np1
            out["phys%d" % i] = hip.physical()
            hip.run.close()
        else:
            raise ValueError("unknown job kind %r" % job["kind"])
    return out


def _tail(text, n=40):
    if isinstance(text, bytes):
        text = text.decode(errors="replace")
    return "\n".join((text or "").splitlines()[-n:])


def run_in_child(tmp_path, job, overrides, timeout=300):
    """run_job(job) in a fresh `python` with os.environ | overrides; returns its arrays."""
    import pytest
    tag = "_".join("%s%s" % kv for kv in sorted(overrides.items()))
    out = os.path.join(str(tmp_path), "child_%s.npz" % tag)
    cmd = [sys.executable, "-m", "tests.child_run", json.dumps(job), out]
    env = os.environ | {k: str(v) for k, v in overrides.items()}
    try:
        p = subprocess.run(cmd, cwd=ROOT, env=env, timeout=timeout, capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        pytest.exit("child GPU process with %s hung (no exit within %d s); nothing more starts on the GPU in this session\n%s"
                    % (overrides, timeout, _tail(e.stderr)), returncode=3)
    if p.returncode < 0:
        pytest.exit("child GPU process with %s died on signal %d; nothing more starts on the GPU in this session\n%s"
                    % (overrides, -p.returncode, _tail(p.stderr)), returncode=3)
    assert p.returncode == 0, "child with %s failed (exit %d):\n%s" % (overrides, p.returncode, _tail(p.stderr))
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    arrays = run_job(json.loads(sys.argv[1]))
    np.savez(sys.argv[2], **arrays)
