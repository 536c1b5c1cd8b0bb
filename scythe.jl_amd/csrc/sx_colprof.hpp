// The column profiles as their two users see them: sx_isosurface (sx_isosurface.hip, which holds the kernels k_column_profiles and
// k_column_profiles_rz and states what they compute) and sx_regrid (sx_regrid.hip).  Both sort the columns by radial cell with
// colprof_batches and launch through launch_column_profiles: one statement of the kernels, of their argument record and of the batching.
#pragma once
#include "sx_internal.hpp"
#include "sx_redprog.hpp"

namespace sx {

constexpr int ISO_KINDS = 5;              // profile kinds of a variable, (sr, sl) = (0, 0) (1, 0) (2, 0) (0, 1) (0, 2)
constexpr int ISO_BATCH = 16;             // columns of one radial cell per matrix product
constexpr int ISO_KC = 32;                // blocks of A per staged tile: 32 K steps
constexpr int ISO_AS = 36;                // row stride of the staged tile in doubles
constexpr size_t ISO_LDS_MAX = 64 * 1024;

struct IsoVar {
    int var;                              // 0-based variable
    int prof[ISO_KINDS];                  // profile number of each kind, -1 = not named
};
struct IsoBatch { int first, n, cell, pad; };     // sorted positions [first, first + n) share the radial cell `cell`
struct ColProfArgs {
    const double *A;                      // [b_rDim][C]
    const double *cols;                   // [n_coord - 1][n_cols]: r[, lambda]; |lambda| <= 2 pi
    const int *order;                     // sorted position -> the caller's column
    const IsoBatch *batch;
    double *P;                            // [n_cols][nprof][Zb], the caller's order
    int64_t C;
    int n_cols, nprof, Zb, K2, kDim, cell_lo, cell_hi;
    double xmin, DX;
    IsoVar v[RED_PLANES];
    uint8_t pvar[RED_PLANES], psr[RED_PLANES];     // profile -> 0-based variable, radial order (k_column_profiles_rz)
};

// doubles of LDS: cs [kDim + 1][16] double2 | sA [64][ISO_AS]
inline size_t colprof_lds(int kDim) { return sizeof(double) * (32 * (size_t)(kDim + 1) + 64 * ISO_AS); }

// the columns (radii r [n]) by radial cell - within a cell the caller's order - in idx, and on a grid with an azimuth each cell's in
// batches of at most ISO_BATCH (without one the batches stay empty: k_column_profiles_rz finds the cell itself)
void colprof_batches(const sx_handle *h, const double *r, int64_t n, std::vector<int> &idx, std::vector<IsoBatch> &batches);
// the grid's fields of the record (A, C, Zb, K2, kDim, the cells, xmin, DX); the caller fills the columns, the profiles and the plan
void colprof_grid_args(const sx_handle *h, ColProfArgs &pa);
// k_column_profiles over n_batches batches and nv variables (grids with an azimuth) or k_column_profiles_rz over pa.n_cols x pa.nprof
// x pa.Zb outputs, on the handle's stream and under the timer "k_column_profiles" with the launch's algorithmic bytes (0: no model)
void launch_column_profiles(sx_handle *h, const ColProfArgs &pa, int n_batches, int nv, double bytes);

}  // namespace sx
