/* Stand-alone host program for the sanitizer build of the regrid helpers (scythe.jl_amd/csrc/Makefile, target regrid_asan): calls
 * sx_regrid_check and sx_regrid_columns - pure host code, no device - on the shapes of tests/test_gpu_regrid.py, with buffers of
 * exactly the documented sizes so that an overrun is an AddressSanitizer report.  Exit status 0: every call behaved as documented. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "scythe_hip.h"

static sx_grid_desc desc(int geometry, double xmin, double xmax, int cells, double zmin, double zmax, int zDim) {
    sx_grid_desc d;
    memset(&d, 0, sizeof(d));
    d.abi_version = SX_ABI_VERSION; d.geometry = geometry; d.xmin = xmin; d.xmax = xmax; d.num_cells = cells; d.l_q = 2.0; d.nvars = 3;
    d.zmin = zmin; d.zmax = zmax; d.zDim = zDim; d.tile_num_cells = cells;
    return d;
}

static int fails = 0;
static void expect(int ok, const char *what) {
    if (!ok) { fprintf(stderr, "FAILED: %s (%s)\n", what, sx_last_error()); fails++; }
}

static void columns(const sx_grid_desc *s, const sx_grid_desc *d, const double *centre, int nh, int64_t want_out) {
    int64_t n = 0, out = 0;
    expect(sx_regrid_columns(s, d, centre, NULL, NULL, &n) == 0 && n > 0, "sx_regrid_columns: the count");
    double *cols = (double *)malloc(sizeof(double) * (size_t)(n * nh));
    int32_t *inside = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
    expect(sx_regrid_columns(s, d, centre, cols, inside, &n) == 0, "sx_regrid_columns");
    for (int64_t c = 0; c < n; c++) {
        out += !inside[c];
        expect(isfinite(cols[c]) && (nh == 1 || isfinite(cols[n + c])), "a finite coordinate");
    }
    expect(want_out < 0 ? out > 0 : out == want_out, "the number of columns outside");
    expect(sx_regrid_columns(s, d, centre, cols, NULL, NULL) == 0 && sx_regrid_columns(s, d, centre, NULL, inside, NULL) == 0, "NULL outputs");
    free(cols);
    free(inside);
}

int main(void) {
    const int32_t vs[3] = {3, 1, 3}, bad[3] = {1, 4, 1};
    const double off[2] = {0.3, -0.2}, far[2] = {2.5, 0.0}, nanc[2] = {NAN, 0.0};
    sx_grid_desc s, d;
    s = desc(SX_GEOM_RLZ, 0.0, 6.0, 6, 0.0, 3.0, 10); d = desc(SX_GEOM_RLZ, 0.0, 4.5, 9, 0.5, 2.5, 12);
    expect(sx_regrid_check(&s, &d, NULL, vs, SX_REGRID_REFUSE) == 0, "RLZ, the same axis");
    expect(sx_regrid_check(&s, &d, off, vs, SX_REGRID_REFUSE) == 0, "RLZ, an offset axis");
    expect(sx_regrid_check(&s, &d, far, vs, SX_REGRID_REFUSE) == 1 && sx_regrid_check(&s, &d, far, vs, SX_REGRID_FILL) == 0, "RLZ, columns outside");
    expect(sx_regrid_check(&s, &d, nanc, vs, 0) == 1 && sx_regrid_check(&s, &d, NULL, bad, 0) == 1 && sx_regrid_check(&s, &d, NULL, vs, 2) == 1 &&
               sx_regrid_check(&s, &d, NULL, NULL, 0) == 1 && sx_regrid_check(NULL, &d, NULL, vs, 0) == 1,
           "RLZ, the refusals");
    columns(&s, &d, NULL, 2, 0); columns(&s, &d, off, 2, 0); columns(&s, &d, far, 2, -1);
    s = desc(SX_GEOM_RL, 0.0, 6.0, 6, 0, 0, 0); d = desc(SX_GEOM_RL, 0.0, 3.0, 4, 0, 0, 0);
    expect(sx_regrid_check(&s, &d, off, vs, SX_REGRID_REFUSE) == 0, "RL");
    columns(&s, &d, NULL, 2, 0); columns(&s, &d, off, 2, 0);
    s = desc(SX_GEOM_RZ, 0.0, 5.0, 5, 0.0, 3.0, 10); d = desc(SX_GEOM_RZ, 0.5, 4.5, 8, 0.5, 2.5, 12);
    expect(sx_regrid_check(&s, &d, NULL, vs, SX_REGRID_REFUSE) == 0 && sx_regrid_check(&s, &d, off, vs, 0) == 1, "RZ");
    columns(&s, &d, NULL, 1, 0);
    d.xmax = 5.5;
    columns(&s, &d, NULL, 1, -1);
    s = desc(SX_GEOM_R, 0.0, 5.0, 5, 0, 0, 0); d = desc(SX_GEOM_R, 0.5, 4.5, 8, 0, 0, 0);
    expect(sx_regrid_check(&s, &d, NULL, vs, SX_REGRID_REFUSE) == 0, "R");
    columns(&s, &d, NULL, 1, 0);
    printf(fails ? "regrid_host: %d failure(s)\n" : "regrid_host: ok\n", fails);
    return fails != 0;
}
