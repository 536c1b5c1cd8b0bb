"""Phase stamps of k_fl_forward_cells (diagnostic build, `make -C scythe.jl_amd/csrc phases`; see profiles/phases.py):
   SX_CELLS_PHASES_OUT=... ; per workgroup, as seen by wave 0 and summed over the rings it walks: 0 wait for the ring's tile + LDS
   write, 1 workgroup barrier, 2 transform, 3 untangling + node sums, 4 node stores issued, 5 entry to the first ring, 6 rings, 7 total."""
import sys
import numpy as np

a = np.fromfile(sys.argv[1], dtype=np.int64).reshape(-1, 8)
a = a[a[:, 6] > 0]
names = ["tile landed + written to LDS (wait for HBM)", "workgroup barrier (LDS only)", "transform (4 radix-4 passes)",
         "untangle + accumulate into the node sums", "node stores issued (per cell + 3 edge nodes)", "entry -> first ring (twiddles, first tile request)"]
tot, rings = a[:, 7], a[:, 6]
full = rings == rings.max()
print("workgroups %d (%d with %d rings)   total cycles per workgroup: median %.0f  mean %.0f  p10 %.0f  p90 %.0f" % (len(a), full.sum(), rings.max(), np.median(tot), tot.mean(), np.percentile(tot, 10), np.percentile(tot, 90)))
print("cycles per ring (total / rings), full workgroups: median %.0f" % np.median(tot[full] / rings[full]))
for i, n in enumerate(names):
    per = a[full, i] / (rings[full] if i < 5 else 1)
    print("  %-52s per %s: median %7.0f  mean %7.0f   (%4.1f %% of the workgroup)" % (n, "ring" if i < 5 else "wg  ", np.median(per), per.mean(), 100 * a[:, i].mean() / tot.mean()))
