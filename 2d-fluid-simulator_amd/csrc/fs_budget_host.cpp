// fs_budget_host.cpp - the per-cell function of fs_budget.h (with limit_cell and vortex_grad of fs_cell.h behind it) and the header's
// constants, the text the kernel runs, compiled by the host compiler for the CPU tests (tests/test_budget_cpu.py).  Test infrastructure:
// libfs_hip.so does not link it.
#include "fs_budget.h"

namespace {

// in [cells][BUDGET_INPUTS]: u, w, p, ul, wl, ur, wr, um, wm, un, wn -> out [cells][BUDGET_PLANES]
template <typename T>
void cells_of(const T *in, long long cells, double limit, double two_dx, double *out)
{
    for (long long e = 0; e < cells; ++e) {
        const T *x = in + e * fs::BUDGET_INPUTS;
        double o[fs::BUDGET_PLANES];
        fs::budget_cell<T>(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9], x[10], (T)limit, two_dx, o);
        for (int k = 0; k < fs::BUDGET_PLANES; ++k) out[e * fs::BUDGET_PLANES + k] = o[k];
    }
}

}  // namespace

extern "C" {

void fs_budget_host_limits(int *planes, int *state, int *inputs, int *cells, int *rows0, int *rows, int *pad, int *lds_bytes)
{
    *planes = fs::BUDGET_PLANES; *state = fs::BUDGET_STATE; *inputs = fs::BUDGET_INPUTS; *cells = fs::BUDGET_CELLS; *rows0 = fs::BUDGET_ROWS0;
    *rows = fs::BUDGET_ROWS; *pad = fs::BUDGET_PAD; *lds_bytes = 0;
}

void fs_budget_host_cell_f32(const float *in, long long cells, double limit, double two_dx, double *out) { cells_of(in, cells, limit, two_dx, out); }
void fs_budget_host_cell_f64(const double *in, long long cells, double limit, double two_dx, double *out) { cells_of(in, cells, limit, two_dx, out); }

}  // extern "C"
