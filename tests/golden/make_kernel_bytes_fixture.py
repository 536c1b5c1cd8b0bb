"""Generates tests/golden/kernel_bytes_parent.json: what sx_kernel_bytes answered on the commit BEFORE the byte counts moved from
sx_kernel_bytes' own chain of formulas to the launchers (each TimedLaunch scope now states its launch's bytes).  Per case of
tests/kernel_bytes.py CASES: the SX_* switches, the storage mode, and per stage - after two steps, then after tileTransform! - and
per tile the names sx_get_timers lists, in its order, and a {name: repr(bytes)} map of them plus k_solve, k_zinv, k_node_fft and the
alloc.* keys.
tests/test_gpu_kernel_bytes.py replays the cases on the current build and demands == on every entry (but for the
two differences of the change, which its docstring names).

How the committed file was made: this script and tests/kernel_bytes.py were put into a checkout of the parent commit, the library
built there, and on an MI355X

    python tests/golden/make_kernel_bytes_fixture.py <parent commit>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernel_bytes_parent.json")


def main(commit, out=OUT):
    from tests import kernel_bytes as KB
    doc = {"commit": commit, "cases": {}}
    for cid, (_, env, storage, tiles, _) in KB.CASES.items():
        doc["cases"][cid] = dict(env=env, storage=storage, tiles=tiles, stages=KB.record(cid))
        print(cid, "done", flush=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], *sys.argv[2:3])
