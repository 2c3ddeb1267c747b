// fs_cell.h - the two per-cell functions that a rider applies to the values it reads, as host-and-device text: limit_cell (limit_field's
// function, from fs_kernels.h) and vortex_grad (the velocity gradient of a cell from its four neighbours, from fs_vortex.h).  They moved here
// with the same operations in the same order - two things changed: they are __host__ __device__ (still forced inline on the device), and
// limit_cell takes its square root through cell_sqrt below, sqrtf / sqrt as fs_device.h's tsqrt, which no host compiler can read - so that a
// host library for the CPU tests (fs_budget_host.cpp) compiles the text the kernels run; fs_kernels.h and fs_vortex.h include this header,
// and every kernel calls the functions under their old names.  No HIP header is needed to read it.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define FS_CELL_HD __host__ __device__ __forceinline__
#else
#define FS_CELL_HD inline
#endif

namespace fs {

FS_CELL_HD float cell_sqrt(float a) { return sqrtf(a); }
FS_CELL_HD double cell_sqrt(double a) { return sqrt(a); }

// the per-cell function of limit_field: (x, y) scaled onto the circle of radius lim when it lies outside -> whether it did (also what
// fs_history.h applies to a probe while v still owes a deferred pass, so that a record equals the download after the pass, bit for bit)
template <typename T>
FS_CELL_HD bool limit_cell(T &x, T &y, T lim)
{
    const T nrm = cell_sqrt(x * x + y * y);
    if (!(nrm > lim)) return false;
    x = lim * (x / nrm);
    y = lim * (y / nrm);
    return true;
}

// the gradient terms of a cell from its four neighbours' (u, w), in the order of fs_vortex.h's header
struct VxGrad { double ux, uy, wx, wy, om; };
template <typename T>
FS_CELL_HD VxGrad vortex_grad(T ul, T wl, T ur, T wr, T um, T wm, T un, T wn, T limit, double two_dx)
{
    if (limit > (T)0) { limit_cell(ul, wl, limit); limit_cell(ur, wr, limit); limit_cell(um, wm, limit); limit_cell(un, wn, limit); }
    VxGrad d;
    d.ux = ((double)ur - (double)ul) / two_dx;
    d.uy = ((double)un - (double)um) / two_dx;
    d.wx = ((double)wr - (double)wl) / two_dx;
    d.wy = ((double)wn - (double)wm) / two_dx;
    d.om = (((double)wr - (double)wl) - ((double)un - (double)um)) / two_dx;
    return d;
}

}  // namespace fs
