// fs_mg.h - kernels of the multigrid pressure updater (include/fs_hip.h fs_mg_*; fs/pressure_updater.py MultigridPressureUpdater).
//
// A W-cycle corrects the pressure on the FLUID cells by an error E1 that lives on a hierarchy of coarse levels.  A level holds five arrays
// of nx * ny cells, x contiguous and unpadded: the iterate E, the right-hand side R and the coefficients cx (coupling to the cell at I + 1),
// cy (to J + 1) and diag (0: the cell is inactive and its E stays 0).  The coefficients come from the host (fs/multigrid.py) and are dyadic
// rationals.  Every operation below is one IEEE operation in the field type, in the order the restatement tests/multigrid_ref.py writes
// (-ffp-contract=off), so all forms - one launch per half sweep, or a whole tail of levels in one workgroup - give the same bits:
//     off(E)[I, J] = ((cx[I-1, J] E[I-1, J] + cx[I, J] E[I+1, J]) + cy[I, J-1] E[I, J-1]) + cy[I, J] E[I, J+1]     (outside the level: 0.0 * 0.0)
//     half sweep   E = (off(E) + R) / diag                       active cells with (I + J) % 2 == parity; a sweep is parity 1, then parity 0
//     residual     R - (diag E - off(E))                         active cells, 0 elsewhere
//     restriction  (r[2I, 2J] + r[2I+1, 2J]) + (r[2I, 2J+1] + r[2I+1, 2J+1]);  prolongation copies E[i >> 1, j >> 1]
// Cross-workgroup ordering comes from launch boundaries alone: no kernel waits for another workgroup, nothing is atomic.
#pragma once
#include "fs_device.h"
#include "fs_kernels.h"

namespace fs {

constexpr int MG_MAX_LEVELS = 24;
constexpr int MG_TAIL_THREADS = 64;      // ONE wave: the tail's smallest levels are chains of barriers, and a one-wave workgroup's barrier costs nothing

// a level's five arrays (global memory or LDS)
template <typename T>
struct MgLevel {
    T *E, *R;
    const T *cx, *cy, *diag;
    int nx, ny;
};

template <typename T>
__device__ __forceinline__ T mg_off(const T *E, const T *cx, const T *cy, int nx, int ny, int I, int J)
{
    const int c = J * nx + I;
    const bool w = I > 0, e = I < nx - 1, s = J > 0, n = J < ny - 1;
    const T cw = w ? cx[c - 1] : (T)0, ew = w ? E[c - 1] : (T)0;
    const T ee = e ? E[c + 1] : (T)0;
    const T cs = s ? cy[c - nx] : (T)0, es = s ? E[c - nx] : (T)0;
    const T en = n ? E[c + nx] : (T)0;
    return ((cw * ew + cx[c] * ee) + cs * es) + cy[c] * en;
}

// the new value of an active cell / the residual of a cell (0 on inactive cells)
template <typename T>
__device__ __forceinline__ void mg_relax(T *E, const T *R, const T *cx, const T *cy, const T *diag, int nx, int ny, int I, int J)
{
    const int c = J * nx + I;
    const T d = diag[c];
    if (d > (T)0) E[c] = (mg_off(E, cx, cy, nx, ny, I, J) + R[c]) / d;
}
template <typename T>
__device__ __forceinline__ T mg_res(const T *E, const T *R, const T *cx, const T *cy, const T *diag, int nx, int ny, int I, int J)
{
    const int c = J * nx + I;
    const T d = diag[c];
    return d > (T)0 ? R[c] - (d * E[c] - mg_off(E, cx, cy, nx, ny, I, J)) : (T)0;
}

// ---- the fine grid -----------------------------------------------------------------------------------------------------------------------
// r = 4 (predict_p(p, v) - p) on fluid cells of a p the pressure boundary kernel has been applied to (predict_p: fs/pressure_updater.py:23-38 in
// the reference's order, fs_kernels.h), restricted to level 1 in the same pass; E1 is zeroed for the cycle that follows.  One lane per level-1
// cell = 2 x 2 fine cells; the only full-resolution read of v the cycle adds.
template <typename T>
__device__ __forceinline__ T mg_fine_r(const Grid &g, const Konst<T> &k, const T *p, const T *v, int i, int j)
{
    if (mask_at(g, i, j) != 0) return (T)0;
    T s2, s3;
    poisson_source(v, g, k, i, j, s2, s3);
    return (T)4 * (((p_avg(p, g, i, j) + s2) - s3) - at<1>(p, g, 0, i, j));
}
template <typename T>
__global__ __launch_bounds__(256) void k_mg_fine_residual(Grid g, Konst<T> k, const T *p, const T *v, T *R1, T *E1, int nx, int ny)
{
    const int I = blockIdx.x * blockDim.x + threadIdx.x, J = blockIdx.y;
    if (I >= nx || J >= ny) return;
    const int i = 2 * I, j = 2 * J;      // (the host checked X == 2 nx, rows == 2 ny: all four cells exist)
    const T r00 = mg_fine_r(g, k, p, v, i, j), r10 = mg_fine_r(g, k, p, v, i + 1, j);
    const T r01 = mg_fine_r(g, k, p, v, i, j + 1), r11 = mg_fine_r(g, k, p, v, i + 1, j + 1);
    R1[J * nx + I] = (r00 + r10) + (r01 + r11);
    E1[J * nx + I] = (T)0;
}

// pc[fluid] += E1[i >> 1, j >> 1] and pn[fluid] += the same, in place (fluid cells only: the cells no kernel writes stay equal in every pressure
// buffer).  Both buffers of the red-black pair are iterates of the same equation - its even half sweep blends with what p.next held - so both
// take the correction.
template <typename T>
__global__ __launch_bounds__(256) void k_mg_fine_correct(Grid g, T *pc, T *pn, const T *E1, int nx)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= g.X || j >= g.rows) return;
    if (mask_at(g, i, j) != 0) return;
    const size_t c = idx<1, T>(g, 0, i, j);
    const T e = E1[(j >> 1) * nx + (i >> 1)];
    pc[c] = pc[c] + e;
    pn[c] = pn[c] + e;
}

// ---- a level in global memory ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_mg_halfsweep(MgLevel<T> l, int parity)
{
    const int J = blockIdx.y;
    const int I = 2 * (blockIdx.x * blockDim.x + threadIdx.x) + ((J + parity) & 1);
    if (I >= l.nx || J >= l.ny) return;
    mg_relax(l.E, l.R, l.cx, l.cy, l.diag, l.nx, l.ny, I, J);
}

// coarse R <- restriction of the level's residual; the coarse E <- 0 (the cycle on the coarse level starts from it).  One lane per coarse cell.
template <typename T>
__global__ __launch_bounds__(256) void k_mg_restrict(MgLevel<T> f, T *Rc, T *Ec, int nxc, int nyc)
{
    const int I = blockIdx.x * blockDim.x + threadIdx.x, J = blockIdx.y;
    if (I >= nxc || J >= nyc) return;
    const int i = 2 * I, j = 2 * J;      // (f.nx == 2 nxc, f.ny == 2 nyc)
    const T r00 = mg_res(f.E, f.R, f.cx, f.cy, f.diag, f.nx, f.ny, i, j), r10 = mg_res(f.E, f.R, f.cx, f.cy, f.diag, f.nx, f.ny, i + 1, j);
    const T r01 = mg_res(f.E, f.R, f.cx, f.cy, f.diag, f.nx, f.ny, i, j + 1), r11 = mg_res(f.E, f.R, f.cx, f.cy, f.diag, f.nx, f.ny, i + 1, j + 1);
    Rc[J * nxc + I] = (r00 + r10) + (r01 + r11);
    Ec[J * nxc + I] = (T)0;
}

// E[active] += Ec[i >> 1, j >> 1]
template <typename T>
__global__ __launch_bounds__(256) void k_mg_prolong(MgLevel<T> f, const T *Ec, int nxc)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= f.nx || j >= f.ny) return;
    const int c = j * f.nx + i;
    if (f.diag[c] > (T)0) f.E[c] = f.E[c] + Ec[(j >> 1) * nxc + (i >> 1)];
}

// ---- the last level solved exactly (fs_mg_set_direct) ---------------------------------------------------------------------------------------
// E[active] = M R[active] with the dense inverse M of the level's operator on its n active cells (fs/multigrid.py direct_solve; rows padded with
// zeros to `stride` = 64 ceil(n / 64) elements).  One wave per row, MG_DIRECT_ROWS rows per workgroup; every workgroup stages the compact
// right-hand side r in LDS once (at most 4096 elements: 32 KB in f64).  Lane l walks the columns 64 k + l - coalesced rows of M, conflict-free
// reads of r - and the 64 partial sums meet in a halving tree.  The order is the specification (tests/multigrid_direct_ref.py):
//     r[j] = R[cells[j]] for j < n, 0 for n <= j < stride                          (the padded columns take part: 0 * 0)
//     a_l = 0;  for k = 0 .. stride / 64 - 1:  a_l = a_l + M[i][64 k + l] * r[64 k + l]
//     for s = 32, 16, 8, 4, 2, 1:  a_l = a_l + a_{l + s} for l < s;    E[cells[i]] = a_0
// Inactive cells keep the 0 the kernel that wrote R stored in E.
constexpr int MG_DIRECT_MAX = 4096;      // active cells of a level with an exact solve
constexpr int MG_DIRECT_ROWS = 4;        // rows (waves) per workgroup

template <typename T>
__global__ __launch_bounds__(64 * MG_DIRECT_ROWS) void k_mg_direct(const T *M, const int *cells, const T *R, T *E, int n, int stride)
{
    __shared__ T r[MG_DIRECT_MAX];
    for (int j = threadIdx.x; j < stride; j += 64 * MG_DIRECT_ROWS) r[j] = j < n ? R[cells[j]] : (T)0;
    __syncthreads();
    const int lane = threadIdx.x & 63, i = blockIdx.x * MG_DIRECT_ROWS + (threadIdx.x >> 6);
    if (i >= n) return;                  // (whole waves leave: the shuffles below see all 64 lanes)
    const T *row = M + (size_t)i * stride;
    T a = (T)0;
    for (int c = lane; c < stride; c += 64) a = a + row[c] * r[c];
    for (int s = 32; s >= 1; s >>= 1) a = a + __shfl_down(a, s);      // (lanes >= s add what nothing reads)
    if (lane == 0) E[cells[i]] = a;
}

// ---- the tail: every level from `first` down in the LDS of one workgroup ----------------------------------------------------------------------
// The levels of a W-cycle below a few thousand cells are chains of tiny dependent launches (level k is visited 2^(k-1) times per cycle).  One
// workgroup loads their coefficients and the first level's R into LDS, runs W(first, R) with an explicit visit stack - `done` holds, per level,
// whether its first coarse visit has returned - and stores the first level's E.  Same operations as the launches above, same order.
struct MgTail {
    int n;                           // levels in the tail
    int nx[MG_MAX_LEVELS], ny[MG_MAX_LEVELS];
    int off[MG_MAX_LEVELS];          // first cell of the level in the concatenated global arrays, from the tail's first level
    int coarse_sweeps, coarsest_sweeps;
};

// level k of the tail in LDS: E, R, cx, cy, diag one after the other, 5 * off[k] elements in (the levels keep their global order)
template <typename T>
__device__ __forceinline__ MgLevel<T> mg_tail_level(const MgTail &tl, T *lds, int k)
{
    const int n = tl.nx[k] * tl.ny[k];
    T *q = lds + 5 * tl.off[k];
    MgLevel<T> l;
    l.E = q; l.R = q + n; l.cx = q + 2 * n; l.cy = q + 3 * n; l.diag = q + 4 * n; l.nx = tl.nx[k]; l.ny = tl.ny[k];
    return l;
}

template <typename T>
__device__ __forceinline__ void mg_tail_sweeps(const MgLevel<T> &l, int sweeps)
{
    const int half = (l.nx + 1) / 2;
    for (int s = 0; s < 2 * sweeps; ++s) {
        const int parity = (s & 1) ^ 1;
        for (int t = threadIdx.x; t < half * l.ny; t += MG_TAIL_THREADS) {
            const int J = t / half, I = 2 * (t - J * half) + ((J + parity) & 1);
            if (I < l.nx) mg_relax(l.E, l.R, l.cx, l.cy, l.diag, l.nx, l.ny, I, J);
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(MG_TAIL_THREADS) void k_mg_tail(MgTail tl, const T *gcx, const T *gcy, const T *gdiag, const T *gR, T *gE)
{
    extern __shared__ double mg_lds_raw[];
    T *lds = reinterpret_cast<T *>(mg_lds_raw);
    for (int k = 0; k < tl.n; ++k) {
        const int n = tl.nx[k] * tl.ny[k];
        T *q = lds + 5 * tl.off[k];
        for (int c = threadIdx.x; c < n; c += MG_TAIL_THREADS) {
            q[c] = (T)0;
            q[n + c] = k == 0 ? gR[c] : (T)0;
            q[2 * n + c] = gcx[tl.off[k] + c]; q[3 * n + c] = gcy[tl.off[k] + c]; q[4 * n + c] = gdiag[tl.off[k] + c];
        }
    }
    __syncthreads();
    int k = 0;
    unsigned done = 0;               // bit k: the first of level k's two coarse visits has returned
    bool enter = true;
    for (;;) {
        const MgLevel<T> l = mg_tail_level(tl, lds, k);
        if (enter) {                 // (E of the level is 0: set by the load above or by the restriction that produced its R)
            if (k == tl.n - 1) {
                mg_tail_sweeps(l, tl.coarsest_sweeps);
                enter = false;       // return to the level above
                if (k == 0) break;
                --k;
                continue;
            }
            mg_tail_sweeps(l, tl.coarse_sweeps);
            done &= ~(1u << k);
        } else {
            // level k + 1 has returned: E += prolongation on active cells, sweeps, then the second visit or the return
            const MgLevel<T> c = mg_tail_level(tl, lds, k + 1);
            for (int t = threadIdx.x; t < l.nx * l.ny; t += MG_TAIL_THREADS) {
                const int j = t / l.nx, i = t - j * l.nx;
                if (l.diag[t] > (T)0) l.E[t] = l.E[t] + c.E[(j >> 1) * c.nx + (i >> 1)];
            }
            __syncthreads();
            mg_tail_sweeps(l, tl.coarse_sweeps);
            if (done & (1u << k)) {
                if (k == 0) break;
                --k;
                continue;
            }
            done |= 1u << k;
        }
        // descend: the next level's R <- restriction of this level's residual, its E <- 0
        const MgLevel<T> c = mg_tail_level(tl, lds, k + 1);
        for (int t = threadIdx.x; t < c.nx * c.ny; t += MG_TAIL_THREADS) {
            const int J = t / c.nx, I = t - J * c.nx, i = 2 * I, j = 2 * J;
            const T r00 = mg_res(l.E, l.R, l.cx, l.cy, l.diag, l.nx, l.ny, i, j), r10 = mg_res(l.E, l.R, l.cx, l.cy, l.diag, l.nx, l.ny, i + 1, j);
            const T r01 = mg_res(l.E, l.R, l.cx, l.cy, l.diag, l.nx, l.ny, i, j + 1), r11 = mg_res(l.E, l.R, l.cx, l.cy, l.diag, l.nx, l.ny, i + 1, j + 1);
            c.R[t] = (r00 + r10) + (r01 + r11);
            c.E[t] = (T)0;
        }
        __syncthreads();
        ++k;
        enter = true;
    }
    const int n0 = tl.nx[0] * tl.ny[0];
    for (int c = threadIdx.x; c < n0; c += MG_TAIL_THREADS) gE[c] = lds[c];
}

}  // namespace fs
