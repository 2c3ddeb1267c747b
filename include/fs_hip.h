/*
 * fs_hip.h - C-ABI of libfs_hip.so: the MI355X (gfx950) implementation of the
 * FluidSimulator.step() hot path of takah29/2d-fluid-simulator.
 *
 * The reference has no FFI: its hot path is a set of Taichi kernels behind plain Python classes
 * (SURVEY.md 8b).  This header is the boundary a maintainer would bind instead of Taichi: one entry
 * point per reference kernel, taking opaque device-field handles, so that the Python classes keep
 * the reference's own orchestration (and its DoubleBuffer swap semantics).  Each declaration cites
 * the reference code it replaces (paths relative to the reference repo).
 *
 * Conventions
 *   - every function returns 0 on success, a negative fs_status on failure; fs_last_error() gives text.
 *   - all launches are asynchronous on the context's HIP stream; fs_sync()/downloads synchronise.
 *   - host arrays use the reference layout: shape (X, rows[, C]), y contiguous, channels innermost
 *     (what Taichi's to_numpy()/from_numpy() exchange: fs/fluid_simulator.py:34-36,
 *     fs/boundary_condition.py:78-85).  Device layout is private (row-major in x).
 *   - dtype: 0 = f32 (the reference's only precision, fs/double_buffer.py:7-11), 1 = f64.
 *   - a context owns one slab of the grid: global rows [y0, y0 + ny_local) plus `halo` ghost rows on
 *     each side (single GPU: y0 = 0, ny_local = ny).  "local row" r maps to global y = y0 - halo + r.
 *   - kernels take a local row range [row_begin, row_end) to compute on; reads reach up to 2 rows
 *     outside it (clamped at the global domain edge like fs/differentiation.py:4-9 sample()).
 */
#ifndef FS_HIP_H
#define FS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ABI_VERSION 28

typedef struct fs_ctx fs_ctx;
typedef struct fs_field fs_field;

enum fs_status {
    FS_OK = 0,
    FS_ERR_ARG = -1,      /* bad argument / shape / dtype mismatch        */
    FS_ERR_HIP = -2,      /* HIP runtime error (text in fs_last_error)    */
    FS_ERR_STATE = -3,    /* call order (e.g. kernel before mask upload)  */
    FS_ERR_COMM = -4,     /* RCCL error / communicator not initialised    */
    FS_ERR_UNSUPPORTED = -5
};

enum fs_scheme { FS_UPWIND = 0, FS_KK = 1 };   /* fs/advection.py:12-24 / :27-60 */

int fs_abi_version(void);
const char *fs_last_error(void);
int fs_device_count(int *count);
/* Compact launch lists of this context: how many exist (one hipMalloc + stream synchronisation each, at the first launch of a geometry / slab row
 * range), and how many launches wanted one they could not build (inside a hipGraph capture / tape recording, or beyond 512 lists) and ran dense. */
int fs_tile_list_stats(const fs_ctx *ctx, int *built, int *misses);

/* ---- context -------------------------------------------------------------------------------- */
/* replaces ti.init(...) + Taichi's field allocator (main.py:65-69). */
int fs_create(fs_ctx **out, int device, int nx, int ny, int dtype, int y0, int ny_local, int halo);
int fs_destroy(fs_ctx *ctx);
int fs_sync(fs_ctx *ctx);
int fs_ctx_info(const fs_ctx *ctx, int *nx, int *ny, int *dtype, int *y0, int *ny_local, int *halo, int *pitch);

/* ---- scene (BoundaryCondition.to_field, fs/boundary_condition.py:78-85, :101-112) ----------- */
/* Arrays are GLOBAL: mask (X, Y) u8; bc_const (X, Y, 2); bc_dye (X, Y, 3) of the ctx dtype.      */
int fs_upload_mask(fs_ctx *ctx, const uint8_t *mask_xy);
int fs_upload_bc_const(fs_ctx *ctx, const void *bc_xy2);
int fs_upload_bc_dye(fs_ctx *ctx, const void *bc_xy3);
/* Stencil radius in rows of the velocity / pressure boundary kernels on this mask: how far (chains of the
 * reference's in-kernel read-after-write hazards included) a rewritten cell depends on pre-kernel data.
 * 2 and 1 for regular scenes; slab runs need halo >= these.                                            */
int fs_bc_radius(const fs_ctx *ctx, int *velocity_rows, int *pressure_rows);

/* ---- fields (ti.field / ti.Vector.field + DoubleBuffer members, fs/double_buffer.py:4-18) ---- */
int fs_field_alloc(fs_ctx *ctx, int nchan, fs_field **out);           /* zero-initialised */
int fs_field_free(fs_field *f);
int fs_field_fill(fs_field *f, double value);                          /* field.fill()     */
int fs_field_nchan(const fs_field *f);
/* from_numpy / to_numpy on a window of local rows: host shape (X, nrows, C). */
int fs_field_upload(fs_field *f, const void *host_xrc, int row_begin, int nrows);
int fs_field_download(const fs_field *f, void *host_xrc, int row_begin, int nrows);
int fs_field_copy(fs_field *dst, const fs_field *src);
/* raw device pointer + geometry, for zero-copy interop (hipMemcpy peers, profilers). */
/* Is the velocity buffer's "may hold a speed above 9.95" flag up?  (Synchronises; lets the host take limit_field as its own launch again in a run that has gone hot.) */
int fs_field_hot(const fs_field *f, int *hot);
int fs_field_devptr(const fs_field *f, void **ptr, size_t *bytes);

/* ---- boundary-condition kernels -------------------------------------------------------------- */
/* BoundaryCondition.set_velocity_boundary_condition   fs/boundary_condition.py:16-39  (in place) */
int fs_velocity_bc(fs_ctx *ctx, fs_field *v, int row_begin, int row_end);
/* limit_field of step n + set_velocity_boundary_condition of step n+1 in ONE launch (new: fs/solver.py:38-43 then fs/boundary_condition.py:16-39;
 * the reference issues them as the last kernel of one step and the first of the next).  Behind the velocity buffer's flag the limit pass
 * does nothing in a healthy run, yet its launch is a fifth of a small-grid step; the Python shell defers it (the field carries a pending
 * limit until anything else looks at it) and this entry point runs gate + limit (rare) + boundary op list.  Same bits as fs_limit_field
 * over [limit_begin, limit_end) followed by fs_velocity_bc over [row_begin, row_end).  fs_velocity_bc_limit_ok: available for this context.
 * `parity` (0 / 1): consecutive calls on ONE field alternate it - a launch's op list raises the flag word of its parity and its gate reads
 * the other one, so that every workgroup of a launch takes the same decision (a call that repeats its predecessor's parity would see what
 * that predecessor's op list raised one call late).  fs_field_copy / fs_field_fill / fs_limit_field read all words: any order there. */
int fs_velocity_bc_limit_ok(const fs_ctx *ctx, int *ok);
int fs_velocity_bc_limit(fs_ctx *ctx, double limit, fs_field *v, int parity, int limit_begin, int limit_end, int row_begin, int row_end);
/* BoundaryCondition.set_pressure_boundary_condition   fs/boundary_condition.py:41-65  (in place) */
int fs_pressure_bc(fs_ctx *ctx, fs_field *p, int row_begin, int row_end);
/* DyeBoundaryCondition.set_dye_boundary_condition     fs/boundary_condition.py:94-99  (in place) */
int fs_dye_bc(fs_ctx *ctx, fs_field *dye, int row_begin, int row_end);
/* limit_field(v) at the end of the flow step + set_dye_boundary_condition in ONE launch (the dye solvers: fs/solver.py:148-155, 385-392 call
 * them back to back).  Same bits as fs_limit_field(v) over [limit_begin, limit_end) followed by fs_dye_bc(dye) over [row_begin, row_end). */
int fs_dye_bc_limit_ok(const fs_ctx *ctx, int *ok);
int fs_dye_bc_limit(fs_ctx *ctx, double limit, fs_field *v, fs_field *dye, int limit_begin, int limit_end, int row_begin, int row_end);

/* ---- velocity / dye transport ----------------------------------------------------------------- */
/* MacSolver._update_velocities        fs/solver.py:94-107   (fluid cells; scheme = fs_scheme)   */
int fs_mac_update(fs_ctx *ctx, int scheme, double dt, double dx, double re,
                  fs_field *vn, const fs_field *vc, const fs_field *pc, int row_begin, int row_end);
/* DyeMacSolver._update_dye            fs/solver.py:157-161                                      */
int fs_mac_dye(fs_ctx *ctx, int scheme, double dt, double dx,
               fs_field *dn, const fs_field *dc, const fs_field *vc, int row_begin, int row_end);
/* CipMacSolver._set_grad              fs/solver.py:207-211  (all cells)                         */
int fs_cip_set_grad(fs_ctx *ctx, double dx, fs_field *fx, fs_field *fy, const fs_field *f,
                    int row_begin, int row_end);
/* CipMacSolver._non_advection_phase   fs/solver.py:229-240  (not-wall cells)                    */
int fs_cip_nonadv(fs_ctx *ctx, double dt, double dx, double re,
                  fs_field *fn, const fs_field *fc, const fs_field *pc, int row_begin, int row_end);
/* DyeCipMacSolver._non_advection_phase_dye  fs/solver.py:378-383                                */
int fs_cip_nonadv_dye(fs_ctx *ctx, double dt, double dx, double re,
                      fs_field *dn, const fs_field *dc, int row_begin, int row_end);
/* CipMacSolver._non_advection_phase_grad    fs/solver.py:242-261  (C = 2 or 3 channels)         */
int fs_cip_nonadv_grad(fs_ctx *ctx, double dx, fs_field *fxn, fs_field *fyn,
                       const fs_field *fxc, const fs_field *fyc, const fs_field *fc, const fs_field *fn,
                       int row_begin, int row_end);
/* CipMacSolver._advection_phase / _cip_advect  fs/solver.py:267-332  (v = advecting velocity)   */
int fs_cip_advect(fs_ctx *ctx, double dt, double dx, fs_field *fn, fs_field *fxn, fs_field *fyn,
                  const fs_field *fc, const fs_field *fxc, const fs_field *fyc, const fs_field *v,
                  int row_begin, int row_end);

/* _non_advection_phase_grad + _advection_phase of the VELOCITY field fused into one pass (build-side optimisation, same
 * bits for everything observable): the intermediate gradients never go through HBM.  fn = velocity after
 * _non_advection_phase, fc = velocity before it, gxc/gyc = gradients before; outputs: v_out (advected value on fluid cells, fc
 * carried elsewhere - what the reference's in-place update of fc's buffer leaves), gx_out / gy_out (not-wall cells).  v_out must
 * be a third buffer distinct from fn and fc; the caller rotates buffers (see fs/solver.py).  Tiles without a fluid cell carry only
 * the cells some kernel writes (not-wall cells and the targets of the velocity boundary kernel): every other cell is equal in fc and
 * v_out unless somebody uploaded into one of them - then ONE call with full != 0 carries every cell.                           */
int fs_cip_grad_advect(fs_ctx *ctx, double dt, double dx, fs_field *v_out, fs_field *gx_out, fs_field *gy_out,
                       const fs_field *fn, const fs_field *fc, const fs_field *gxc, const fs_field *gyc,
                       int full, int row_begin, int row_end);
/* CipMacSolver._update_velocities (fs/solver.py:213-227) as ONE call: _non_advection_phase (:229-240; fn <- fc, pc on the not-wall cells)
 * followed by the fused pass above.  Same results in v_out / gx_out / gy_out and in every cell of fn that anything reads before it is
 * rewritten.  On f32 grids of even width (wherever the compact launch lists exist) the post-K2 velocity is evaluated in registers on the way (csrc/fs_k234.h: one launch over every
 * tile - FS_FUSE_K2=1: one over the tiles that see nothing but fluid, one over the others) and stored only on the not-wall cells that are not
 * fluid (inflow / outflow): the fluid cells of fn keep their old content - which the reference's own sequence overwrites (K2 of the next step,
 * or this step's vorticity confinement) before reading it.  fs_cip_step_ok: whether calls take that form (f32, FS_FUSE_K2 != 0, the size; one GPU:
 * calls over the whole grid; a slab context: any row range - K2 is then evaluated for the rows within 2 of the range from rows within 3 of it,
 * which the caller keeps valid, where the two calls would read what an earlier K2 launch left in fn); otherwise the call is exactly
 * fs_cip_nonadv + fs_cip_grad_advect (on a slab: fs_cip_nonadv over the range widened by 2 rows).                                    */
int fs_cip_step_ok(const fs_ctx *ctx, int *ok);
/* The same for the dye: DyeCipMacSolver._update_dye (fs/solver.py:385-401) as ONE call = fs_cip_nonadv_dye(fn <- fc) + fs_cip_grad_advect_dye, with
 * K12 evaluated in registers under the conditions of fs_cip_step_ok (csrc/fs_k234.h k_cip_dye). */
int fs_cip_step_dye(fs_ctx *ctx, double dt, double dx, double re, fs_field *d_out, fs_field *gx_out, fs_field *gy_out, fs_field *fn,
                    const fs_field *fc, const fs_field *gxc, const fs_field *gyc, const fs_field *v, int clamp01, int full, int row_begin, int row_end);
/* diagnostic: the tiles (tile_rows x tile_cells cells each) of the two classes of a whole-grid fs_cip_step launch - all-fluid tiles, the others
 * (`band`: always 0 since ABI 8's three-part form is gone); 0 0 0 where the call takes the two-call form. */
int fs_cip_step_tiles(fs_ctx *ctx, int *plain, int *boundary, int *band, int *tile_rows, int *tile_cells);
int fs_cip_step(fs_ctx *ctx, double dt, double dx, double re, fs_field *v_out, fs_field *gx_out, fs_field *gy_out, fs_field *fn,
                const fs_field *fc, const fs_field *pc, const fs_field *gxc, const fs_field *gyc, int full, int row_begin, int row_end);
/* The same for the dye (C = 3, advected by the velocity field v of the finished flow step; fs/solver.py:378-401 _update_dye without its
 * first kernel): K3 (_non_advection_phase_grad, :242-261) + K4 (_cip_advect, :267-332), d_out = a third dye buffer the caller rotates.
 * clamp01 != 0 folds clamp_field(dye, 0, 1) (:46-49) into the store of the advected cells; full as above.  f32 only.                   */
int fs_cip_grad_advect_dye(fs_ctx *ctx, double dt, double dx, fs_field *d_out, fs_field *gx_out, fs_field *gy_out,
                           const fs_field *fn, const fs_field *fc, const fs_field *gxc, const fs_field *gyc, const fs_field *v,
                           int clamp01, int full, int row_begin, int row_end);

/* ---- vorticity confinement -------------------------------------------------------------------- */
/* VorticityConfinement._calc_vorticity    fs/vorticity_confinement.py:27-32                     */
int fs_vort_calc(fs_ctx *ctx, double dx, fs_field *vort, fs_field *vort_abs, const fs_field *vc,
                 int row_begin, int row_end);
/* VorticityConfinement._add_vorticity     fs/vorticity_confinement.py:34-55                     */
int fs_vort_add(fs_ctx *ctx, double dt, double dx, double weight, fs_field *vn, const fs_field *vc,
                const fs_field *vort, const fs_field *vort_abs, int row_begin, int row_end);

/* _calc_vorticity + _add_vorticity fused into one pass (build-side optimisation, same bits): the vorticity never
 * goes through HBM.  vort / vort_abs may be NULL; when given they are also written (fluid cells), like K5 does. */
int fs_vort_confine(fs_ctx *ctx, double dt, double dx, double weight, fs_field *vn, const fs_field *vc,
                    fs_field *vort, fs_field *vort_abs, int row_begin, int row_end);

/* ---- pressure Poisson relaxation (predict_p, fs/pressure_updater.py:23-38) -------------------- */
/* JacobiPressureUpdater._update           fs/pressure_updater.py:62-66   (not-wall cells)       */
int fs_jacobi_sweep(fs_ctx *ctx, double dt, double dx, fs_field *pn, const fs_field *pc,
                    const fs_field *vc, int row_begin, int row_end);
/* RedBlackSorPressureUpdater._update_pressures_odd/_even  fs/pressure_updater.py:98-114.
 * parity 1 = odd cells ((i + j) % 2 == 1), 0 = even; pn may be the same field as pc (even pass).  */
int fs_rbsor_halfsweep(fs_ctx *ctx, double dt, double dx, double omega, int parity,
                       fs_field *pn, const fs_field *pc, const fs_field *vc, int row_begin, int row_end);
/* One whole red-black iteration (odd pass pc -> pn, then even pass in place on pn; fs/pressure_updater.py:92-96)
 * as a single fused kernel (build-side optimisation, same bits, 21 instead of 34 B/cell).  pn != pc.   */
int fs_rbsor_iteration(fs_ctx *ctx, double dt, double dx, double omega, fs_field *pn, const fs_field *pc,
                       const fs_field *vc, int row_begin, int row_end);
/* Source-term precompute (build-side optimisation; the source of predict_p depends only on v and is
 * constant over the sweeps of one step).  src has 2 channels: (s2, s3) with predict_p = (0.25*sum + s2) - s3,
 * i.e. the reference's operation order is kept and results stay bit-identical to the v-reading kernels.  src is defined on every
 * cell a sweep reads it at (not-wall cells and everything within a few cells of one); regions of nothing but wall may be left untouched. */
int fs_poisson_source(fs_ctx *ctx, double dt, double dx, fs_field *src, const fs_field *vc,
                      int row_begin, int row_end);
int fs_jacobi_sweep_src(fs_ctx *ctx, fs_field *pn, const fs_field *pc, const fs_field *src,
                        int row_begin, int row_end);
/* Jacobi sweep on the source pair with the pressure boundary condition evaluated on the fly from the RAW output of the previous
 * sweep (build-side optimisation for long Jacobi runs, same bits): replaces fs_pressure_bc + fs_jacobi_sweep_src for all but the
 * last two sweeps of a JacobiPressureUpdater.update (fs/pressure_updater.py:56-66).  fs_lazy_bc_ok: does this mask admit it
 * (every K7 source a not-wall cell, no computed cell in the first / last row)?                                                */
int fs_lazy_bc_ok(const fs_ctx *ctx, int *ok);
int fs_jacobi_sweep_lazy(fs_ctx *ctx, fs_field *pn, const fs_field *pc, const fs_field *src, int row_begin, int row_end);
/* Diagnostic: the classification the two kernels above and below work from, one byte per (wave column of 248 cells, local row),
 * [wave column][row]; bit 0: a computed cell of the row has a K7 target among its 4 neighbours, 1: a wall / target within 2 columns,
 * 3: a target that reads another row within 4 columns, 2: such a target in a wall one cell thick, or a wall cell whose content is
 * history, 4 / 5: the row goes through the general path of fs_jacobi_pair_lazy with mode bit 1 = 0 / 1 (general_rows[0 / 1] = how many
 * such rows hold computed cells; an int[2]).  out may be NULL to query the sizes.                                                    */
int fs_lazy_flags(fs_ctx *ctx, uint8_t *out, int capacity, int *wave_columns, int *rows, int *general_rows);
/* TWO such sweeps in one pass: pn <- sweep(sweep(pc)), the first sweep's rows staying in registers.  mode bit 0 ("swapped"): the two
 * buffers of the reference's rotation differ in the wall cells nothing ever writes, and not-wall cells beside them read them - 0 when pc
 * is the physical buffer the reference holds this pass's input iterate in (the 1st, 3rd ... pass of a pc -> pn -> pc sequence; the
 * intermediate iterate's wall cells are then pn's), 1 when it is the other way round (2nd, 4th ... pass).  mode bit 1: the tile path also
 * applies the recipes that read the row below / above (pays on masks with staircase outlines, costs a few percent elsewhere; same bits).
 * Both buffers are read 4 rows beyond the written range, src 2 rows.                                                                  */
int fs_jacobi_pair_lazy(fs_ctx *ctx, fs_field *pn, const fs_field *pc, const fs_field *src, int mode, int row_begin, int row_end);
/* Diagnostic.  f32 runs divide by their loop-invariant divisors (dx, 2 dx, dx^2, dx^3, 6 dx, 8 dt, Re - the divisions of
 * fs/differentiation.py:41-60, fs/solver.py:257-260, 304-313, fs/advection.py:46-58, fs/pressure_updater.py:37) as
 * (float)((double)x * (1.0 / d)), which equals the IEEE quotient x / d for every f32 x (csrc/fs_device.h f64div).  This checks the
 * identity on the device for one divisor: ~2^28 dividends (all significands of nine binades incl. the denormals, both signs, and
 * arbitrary bit patterns); *mismatches must come back 0.                                                                        */
int fs_selftest_f64div(fs_ctx *ctx, double divisor, int *mismatches);
/* TWO red-black iterations - RedBlackSorPressureUpdater.update with n_iter = 2, fs/pressure_updater.py:86-96, which is what
 * fs/fluid_simulator.py:76-78 wires into every create() - and the two set_pressure_boundary_condition passes between them
 * (fs/boundary_condition.py:41-65) in ONE pass over HBM (build-side optimisation, same bits): (pc_out, pn_out) receive what the
 * reference leaves in (p.current, p.next) after two iterations that start from (pc, pn).  Out of place: four distinct fields; the caller
 * rotates the pairs.  Only fluid cells and boundary-condition targets are stored (every other cell holds the same value in all four
 * buffers as long as nobody uploads into them); full != 0 stores every cell of the row range - the carry pass after an upload.  pc and
 * vc are read 4 rows beyond the written range, pn 3.  fs_rbsor_pair_ok: f32, X % 4 == 0, and a mask without one-cell-thin walls between
 * fluid regions and without fluid in the first / last row (csrc/fs_rbpair.h); otherwise FS_ERR_UNSUPPORTED - use fs_rbsor_iteration. */
int fs_rbsor_pair_ok(const fs_ctx *ctx, int *ok);
int fs_rbsor_pair(fs_ctx *ctx, double dt, double dx, double omega, fs_field *pc_out, fs_field *pn_out, const fs_field *pc,
                  const fs_field *pn, const fs_field *vc, int full, int row_begin, int row_end);
/* FOUR such sweeps in one pass (csrc/fs_jquad.h): pn[not wall] <- sweep(sweep(sweep(sweep(pc)))), the boundary condition evaluated in
 * front of each; for long Jacobi runs whose data stay cache resident and whose cost is launches and latency.  Writes the not-wall cells
 * of pn only: the caller guarantees that the wall cells no kernel writes are equal in pn and pc (nobody uploaded into one of them).
 * pc is read 4 rows beyond the written range, src 3.  fs_jacobi_quad_ok: f32, fs_lazy_bc_ok, and no recipe that reads the far side of
 * its target as seen from a cell whose value is used; otherwise FS_ERR_UNSUPPORTED - use fs_jacobi_pair_lazy / fs_jacobi_sweep_lazy.  */
int fs_jacobi_quad_ok(const fs_ctx *ctx, int *ok);
int fs_jacobi_quad_lazy(fs_ctx *ctx, fs_field *pn, const fs_field *pc, const fs_field *src, int row_begin, int row_end);
/* The LAST two rounds (K7, sweep, swap; K7, sweep, swap - fs/pressure_updater.py:56-66) of such a run in one pass: pc holds the raw iterate
 * n-2; pc_out (a third buffer) receives what the reference leaves in p.current (iterate n on the not-wall cells, K7(iterate n-2) on the wall
 * cells with a recipe), pn what it leaves in p.next (iterate n-1 with K7 applied).  Cells no kernel writes are not stored: they must be
 * equal in the three buffers.  Same conditions as fs_jacobi_quad_lazy; pc is read 2 rows beyond the written range, src 1. */
int fs_jacobi_finish(fs_ctx *ctx, fs_field *pc_out, fs_field *pn, const fs_field *pc, const fs_field *src, int row_begin, int row_end);
int fs_rbsor_halfsweep_src(fs_ctx *ctx, double omega, int parity, fs_field *pn, const fs_field *pc,
                           const fs_field *src, int row_begin, int row_end);
/* Residual diagnostic (new; the reference never measures convergence): sum over owned not-wall cells of
 * (predict_p(p) - p)^2 and the cell count, accumulated in double.  Does not alter any field.       */
int fs_poisson_residual(fs_ctx *ctx, double dt, double dx, const fs_field *p, const fs_field *vc,
                        double *sum_sq, double *count);

/* Flow diagnostics (new; the reference only draws the flow): ONE pass over the owned rows of v, p and the mask -> this rank's
 * FS_FLOW_NSTAT partials in `out` (cross-rank combination is the caller's: sums add, maxima take the maximum and propagate NaN).
 * Arithmetic in double on the stored values; F = fluid cells (mask 0), N = not-wall cells (mask != 1); u = v[..., 0], w = v[..., 1];
 * u(i, j) etc. are clamped samples (fs/differentiation.py:4-9 sample()), stored wall-cell values enter the stencils as they are:
 *   s2 = u*u + w*w    om = ((w(i+1,j) - w(i-1,j)) - (u(i,j+1) - u(i,j-1))) / (2.0*dx)
 *   a = fabs(u) + fabs(w)    dv = ((u(i+1,j) - u(i-1,j)) + (w(i,j+1) - w(i,j-1))) / (2.0*dx)
 *   slot 0 fluid_cells   sum   count of F          slot 5 max_a       max   max_F a
 *   slot 1 sum_s2        sum   sum_F s2            slot 6 max_abs_dv  max   max_F |dv|
 *   slot 2 sum_om2       sum   sum_F om^2          slot 7 nonfinite   sum   cells of N whose u, w or p is NaN or +-Inf
 *   slot 3 sum_dv2       sum   sum_F dv^2          slot 8 force_x     sum   pressure force per unit depth on the wall cells of the box
 *   slot 4 max_s2        max   max_F s2            slot 9 force_y     sum   (0 without a box)
 * Force: for each wall cell inside the half-open box [x0, x1) x [y0, y1) (`box` = x0, y0, x1, y1 in global cells, or NULL) and each of
 * its 4 neighbours that is fluid (neighbours beyond the domain edge do not exist): fluid at (i+1, j): force_x -= p(i+1,j)*dx;
 * (i-1, j): force_x += p(i-1,j)*dx; (i, j+1): force_y -= p(i,j+1)*dx; (i, j-1): force_y += p(i,j-1)*dx.  Viscous stress is omitted here: fs_loads_* below adds it.
 * Maxima start at 0 and propagate NaN.  On a slab, v and p must be valid one ghost row deep.  Deterministic (no atomics: two-stage
 * reduction in a fixed order); refused with FS_ERR_STATE during graph capture / tape recording.  Does not alter any field.          */
#define FS_FLOW_NSTAT 10
int fs_flow_stats(fs_ctx *ctx, double dx, const fs_field *v, const fs_field *p, const int *box, double *out);

/* Per-step history (new): a ring of `capacity` records on the device, appended to by ONE small launch per step that can be captured in
 * a hipGraph and recorded in a tape (csrc/fs_history.h).  Record layout, doubles: [force_x, force_y, u0, w0, p0, u1, w1, p1, ...].
 *   points: npoints (x, y) GLOBAL cells - the probes, in record order;
 *   faces:  nfaces (x, y, dir): the FLUID cell of a face of a body and the direction wall -> fluid; dir 0 +x: force_x -= p*dx,
 *           1 -x: force_x += p*dx, 2 +y: force_y -= p*dx, 3 -y: force_y += p*dx (the terms of fs_flow_stats, per face).
 * Every point and face must lie in this context's OWNED rows (FS_ERR_ARG otherwise): on slabs each rank takes its own share, and the
 * ranks' records combine by adding the forces and taking each probe from the rank that owns it.  Pass the faces sorted by (y, x, dir):
 * the force is summed in a fixed order from that list.
 * fs_history_record: launch n (counted from 0) appends a record when (n + 1) % every == 0 - if the ring is full the record is counted as
 *   dropped instead.  limit > 0: v still owes limit_field(limit) (a deferred pass): the probes' (u, w) are limited as that pass would
 *   store them.  Reads the owned rows of v and p only (no ghost row); changes no field.
 * fs_history_read: synchronises, copies the records in the ring (oldest first) to `out` (max_records >= the count, or `out` NULL: counts
 *   only, nothing is reset), then empties the ring: *n_records, *dropped and the launch count (never reset) describe the ring before.
 *   FS_ERR_STATE during graph capture / tape recording.
 * fs_history_free: a graph or tape that holds the launch must not be replayed afterwards; during a capture the release is deferred to
 *   its end (as fs_field_free).                                                                                                        */
typedef struct fs_history fs_history;
int fs_history_create(fs_ctx *ctx, int npoints, const int *points, int nfaces, const int *faces, int capacity, int every, fs_history **out);
int fs_history_record(fs_ctx *ctx, fs_history *h, double dx, double limit, const fs_field *v, const fs_field *p);
int fs_history_read(fs_ctx *ctx, fs_history *h, double *out, int max_records, int *n_records, long long *launches, int *dropped);
int fs_history_free(fs_ctx *ctx, fs_history *h);

/* Body surface loads (new): pressure force, viscous force and their moments on a body per sampling step, and running first and second
 * moments of the per-face pressure and wall shear, by launches that can be captured in a hipGraph and recorded in a tape (csrc/fs_loads.h).
 *   faces:     nfaces >= 1 (x, y, dir) as fs_history_create: the FLUID cell and the direction wall -> fluid (0 +x, 1 -x, 2 +y, 3 -y), in this
 *              context's OWNED rows (FS_ERR_ARG otherwise; on slabs each rank takes its share and the ranks' records add).
 *   centre_xy: (cx, cy) in cell units, finite: the moments' reference point.  Face midpoint (xm, ym): dir 0 (x, y + 0.5), 1 (x + 1, y + 0.5),
 *              2 (x + 0.5, y), 3 (x + 0.5, y + 1); lever arms ax = (xm - cx) * dx, ay = (ym - cy) * dx.
 * Per face on a sampling launch, each line one IEEE double operation per operator, in this order, no FMA:
 *   pk = (double)p[cell];  (u, w) = v[cell], through limit_field's per-cell function in the field's precision when limit > 0 (a deferred pass);
 *   ut = (double)w for dir 0, 1 and (double)u for dir 2, 3;  tv = inv_re * ut;  tk = tv / dx  (wall shear: the no-slip point is the wall
 *   cell's centre, one dx from the fluid value - the distance of the solver's Laplacian);
 *   S_p += pk; S_pp += pk * pk; S_t += tk; S_tt += tk * tk  (the face's four sums);
 *   tp = pk * dx; (fpx, fpy) = (-tp, 0), (+tp, 0), (0, -tp), (0, +tp) for dir 0..3 (the terms of fs_flow_stats);
 *   (fvx, fvy) = (0, tv) for dir 0, 1 and (tv, 0) for dir 2, 3;  mp = ax * fpy - ay * fpx;  mv = ax * fvy - ay * fvx.
 * A record is FS_LOADS_NREC doubles [Fpx, Fpy, Fvx, Fvy, Mp, Mv], each the sum of its face terms in a fixed order (no atomics).
 * record:     launch n (counted from 0) samples when n + 1 > start and (n + 1 - start) % every == 0.  A sampling launch adds to the per-face
 *             sums and appends its record to the ring - or counts it as dropped when the ring holds `capacity` records.  Reads the owned
 *             rows of v and p only, changes no field; a launch that does not sample reads the counters.  The counters advance on the device.
 * read:       synchronises, copies the ring (oldest first) to ring_out (max_records >= the count; NULL: counters only, nothing is reset),
 *             then empties it: *n_records and *dropped describe the ring before; launches and samples run on.
 * sums_read:  sums_out receives [FS_LOADS_NSUM][nfaces] doubles: S_p, S_pp, S_t, S_tt in the order of `faces`.
 * sums_write: the inverse, with both counters (resume): 0 <= samples <= launches.
 * reset:      sums and sample count to zero; the launch count (the phase of `every` / `start`) runs on.
 * free:       a graph or tape that holds the launch must not be replayed afterwards; during a capture the release is deferred to its end.
 * create, read, sums_read, sums_write and reset return FS_ERR_STATE during graph capture / tape recording; a non-finite centre, every < 1,
 * start < 0, capacity < 1 and nfaces < 1 return FS_ERR_ARG.                                                                             */
#define FS_LOADS_NREC 6
#define FS_LOADS_NSUM 4
typedef struct fs_loads fs_loads;
int fs_loads_create(fs_ctx *ctx, int nfaces, const int *faces, const double *centre_xy, int capacity, long long every, long long start,
                    fs_loads **out);
int fs_loads_record(fs_ctx *ctx, fs_loads *l, double dx, double inv_re, double limit, const fs_field *v, const fs_field *p);
int fs_loads_read(fs_ctx *ctx, fs_loads *l, double *ring_out, int max_records, int *n_records, long long *launches, long long *samples,
                  int *dropped);
int fs_loads_sums_read(fs_ctx *ctx, fs_loads *l, double *sums_out);
int fs_loads_sums_write(fs_ctx *ctx, fs_loads *l, const double *sums_in, long long launches, long long samples);
int fs_loads_reset(fs_ctx *ctx, fs_loads *l);
int fs_loads_free(fs_ctx *ctx, fs_loads *l);

/* Time averages (new): first and second moments of u, w and p summed on the device by a launch that can be captured in a hipGraph and
 * recorded in a tape (csrc/fs_mean.h).  State: FS_MEAN_NPLANE planes of double over this context's OWNED rows, in the order S_u, S_w, S_p,
 * S_uu, S_ww, S_uw, S_pp (56 bytes per cell), and two device counters: launches since creation and samples accumulated.
 * create:     every >= 1, start >= 0; sums and counters zero.  An allocation that does not fit returns FS_ERR_HIP.
 * accumulate: launch n (counted from 0) samples when n + 1 > start and (n + 1 - start) % every == 0; it then adds, on every not-wall cell
 *             (mask != 1) of the owned rows, (double)u, (double)w, (double)p and the products (double)u * (double)u, w * w, u * w, p * p, each
 *             formed and added in double - one lane per cell, samples in stream order: the sums are deterministic and an IEEE double loop
 *             over the sampled fields reproduces them bit for bit.  limit > 0: v still owes limit_field(limit) (a deferred pass): u, w are
 *             limited as that pass would store them.  Wall cells keep their sums.  Reads no ghost row, changes no field; a launch that
 *             does not sample reads one counter per workgroup.  The counters advance on the device behind the launch.
 * finalize:   (T)(S_u / n), (T)(S_w / n) into the 2-channel v_out and (T)(S_p / n) into the 1-channel p_out on the not-wall cells of the
 *             owned rows, 0 on wall cells; n = samples (FS_ERR_STATE when 0).  Ghost rows of the targets are not written.
 * read:       synchronises; sums_out (NULL: counters only) receives [FS_MEAN_NPLANE][ny_local][X] doubles, x contiguous.
 * write:      the inverse of read (resume): sums_in in the same layout, 0 <= samples <= launches.
 * reset:      sums and the sample count to zero; the launch count (and with it the phase of `every` / `start`) runs on.
 * free:       a graph or tape that holds the launch must not be replayed afterwards; during a capture the release is deferred to its end
 *             (as fs_history_free).
 * create, finalize, read, write and reset return FS_ERR_STATE during graph capture / tape recording.                                   */
#define FS_MEAN_NPLANE 7
typedef struct fs_mean fs_mean;
int fs_mean_create(fs_ctx *ctx, long long every, long long start, fs_mean **out);
int fs_mean_accumulate(fs_ctx *ctx, fs_mean *m, double limit, const fs_field *v, const fs_field *p);
int fs_mean_finalize(fs_ctx *ctx, fs_mean *m, fs_field *v_out, fs_field *p_out);
int fs_mean_read(fs_ctx *ctx, fs_mean *m, double *sums_out, long long *launches, long long *samples);
int fs_mean_write(fs_ctx *ctx, fs_mean *m, const double *sums_in, long long launches, long long samples);
int fs_mean_reset(fs_ctx *ctx, fs_mean *m);
int fs_mean_free(fs_ctx *ctx, fs_mean *m);
/* diagnostic: the rows per workgroup that the next fs_flow_stats, fs_mean_accumulate and fs_mean_finalize launches of this context take
 * (4 - 32, 4 - 8 and 1 - 8: more on larger grids; env FS_DIAG_WGS, read by fs_create, moves the grid size at which they grow).  Launches
 * nothing: allowed during graph capture / tape recording. */
int fs_diag_rows(fs_ctx *ctx, int *flow_stats_rows, int *mean_accumulate_rows, int *mean_finalize_rows);

/* Harmonic flow modes (new, ABI 18): per-cell Fourier sums of u, w and p at nfreq frequencies, accumulated on the device by a launch that can
 * be captured in a hipGraph and recorded in a tape (csrc/fs_modes.h).  With B = 1 + 2 nfreq and the basis b = [1, c_1, s_1, ..., c_K, s_K]:
 * 3 B planes of double over this context's OWNED rows - plane a * B + j holds the sum over the samples of x_a * b_j, a in (u, w, p) - which
 * is 24 B bytes per cell; two device counters (launches, samples); and FS_MODES_NSCALAR(nfreq) scalars of double: the phasors c_1, s_1, ...,
 * c_K, s_K, then the upper triangle (i <= j, row major) of the Gram matrix G[i][j] = sum over the samples of b_i * b_j.
 * create:     1 <= nfreq <= FS_MODES_MAX_FREQ; cos_sin holds cd_1, sd_1, ..., cd_K, sd_K, the cosine and sine of the phase step per sample
 *             2 pi f_k every dt, computed by the caller (the device evaluates no sin / cos); every >= 1, start >= 0.  Planes, Gram matrix and
 *             counters zero, every phasor (1, 0).  An allocation that does not fit returns FS_ERR_HIP.
 * accumulate: launch n (from 0) samples by the rule of fs_mean_accumulate.  A sampling launch adds, on every not-wall cell of the owned rows,
 *             x to plane a B and x * b_j to plane a B + j (j > 0), x the stored value promoted to double, the product rounded before the sum;
 *             limit > 0: u, w are limited as a deferred limit_field(limit) would store them.  Behind it on the stream, a sampling launch
 *             adds b_i * b_j to the Gram matrix, adds 1 to samples and rotates the phasors, c' = c cd - s sd, s' = s cd + c sd, in this order;
 *             every launch adds 1 to launches.  Deterministic: an IEEE double loop over the sampled fields reproduces every number bit for bit.
 *             Wall cells keep their sums.  Reads no ghost row, changes no field.
 * combine:    v_out[a] = (T) sum_j weights[a B + j] * plane[a B + j] (j = 0 .. B - 1 in this order from 0.0, in double, product then sum) for
 *             a = u, w into the 2-channel v_out and a = p into the 1-channel p_out on the not-wall cells of the owned rows, 0 on wall cells;
 *             weights: 3 B doubles.  Ghost rows of the targets are not written.
 * read:       synchronises; sums_out (NULL: skipped) receives [3 B][ny_local][X] doubles, x contiguous; scalars_out (NULL: skipped) the
 *             FS_MODES_NSCALAR(nfreq) scalars.  write: the inverse (resume), 0 <= samples <= launches.
 * reset:      planes, Gram matrix and the sample count to zero, the phasors to (1, 0); the launch count runs on.
 * free:       as fs_mean_free (during a capture the release is deferred to its end).
 * rows:       diagnostic - the rows per workgroup the accumulate (nfreq frequencies) and combine launches of this context take (fs_diag_rows).
 * create, combine, read, write and reset return FS_ERR_STATE during graph capture / tape recording.                                     */
#define FS_MODES_MAX_FREQ 4
#define FS_MODES_NSCALAR(nfreq) (2 * (nfreq) + (1 + 2 * (nfreq)) * (2 + 2 * (nfreq)) / 2)
typedef struct fs_modes fs_modes;
int fs_modes_create(fs_ctx *ctx, int nfreq, const double *cos_sin, long long every, long long start, fs_modes **out);
int fs_modes_accumulate(fs_ctx *ctx, fs_modes *m, double limit, const fs_field *v, const fs_field *p);
int fs_modes_combine(fs_ctx *ctx, fs_modes *m, const double *weights, fs_field *v_out, fs_field *p_out);
int fs_modes_read(fs_ctx *ctx, fs_modes *m, double *sums_out, double *scalars_out, long long *launches, long long *samples);
int fs_modes_write(fs_ctx *ctx, fs_modes *m, const double *sums_in, const double *scalars_in, long long launches, long long samples);
int fs_modes_reset(fs_ctx *ctx, fs_modes *m);
int fs_modes_free(fs_ctx *ctx, fs_modes *m);
int fs_modes_rows(fs_ctx *ctx, int nfreq, int *accumulate_rows, int *combine_rows);

/* Snapshot POD (new, ABI 21): the last M sampled flow fields kept resident on the device by a launch that can be captured in a hipGraph, their
 * M x M Gram matrix reduced on the device, and linear combinations of them as fields (csrc/fs_pod.h).  State: M slots of three planes (u, w, p)
 * of the context's dtype over the owned rows - 12 bytes per cell and slot in f32, 24 in f64 - and two device counters (launches, samples).
 * Single-GPU contexts: create returns FS_ERR_UNSUPPORTED on a slab context (the Gram matrix would need a rank-ordered reduction).
 * create:  2 <= M <= FS_POD_MAX, every >= 1, start >= 0; slots and counters zero.  An allocation that does not fit returns FS_ERR_HIP and
 *          leaves nothing behind.
 * launch:  launch n (from 0) samples by the rule of fs_mean_accumulate, into slot samples % M (a ring: the object holds the last
 *          min(samples, M) samples): u, w, p as stored on the not-wall cells (limit > 0: u, w limited as a deferred limit_field(limit) would
 *          store them), +0 on the wall cells.  The counters advance on the device behind the launch.  Reads no ghost row, changes no field.
 * gram:    synchronises.  n = min(samples, M) goes to *n_out; with out != NULL (max_n >= n) out receives the dense n x n matrix in SLOT order,
 *          G[a][b] = sum over the cells of (double)u_a * (double)u_b + (double)w_a * (double)w_b, every product and sum rounded on its own, in
 *          the fixed order csrc/fs_pod.h states (two deterministic stages, no atomics): two calls return the same bits, and G is exactly
 *          symmetric.  n == 0: nothing is launched.
 * combine: v_out, p_out = (T) sum_m weights[m] * slot_m, m = 0 .. M - 1 in this order from 0.0, in double, product then sum, for u, w into the
 *          2-channel v_out and p into the 1-channel p_out; 0 on wall cells; weights: M doubles.  Ghost rows of the targets are not written.
 * read:    synchronises; the counters.
 * get:     synchronises; slots_out receives [M][3][Y][X] values of the context's dtype, x contiguous.  set: the inverse (resume),
 *          0 <= samples <= launches.
 * reset:   slots and the sample count to zero; the launch count (and with it the phase of `every` / `start`) runs on.
 * free:    as fs_mean_free (during a capture the release is deferred to its end).
 * create, gram, combine, read, get, set and reset return FS_ERR_STATE during graph capture / tape recording.                            */
#define FS_POD_MAX 64
typedef struct fs_pod fs_pod;
int fs_pod_create(fs_ctx *ctx, int M, long long every, long long start, fs_pod **out);
int fs_pod_launch(fs_ctx *ctx, fs_pod *pod, double limit, const fs_field *v, const fs_field *p);
int fs_pod_gram(fs_ctx *ctx, fs_pod *pod, double *out, int max_n, int *n_out, long long *launches, long long *samples);
int fs_pod_combine(fs_ctx *ctx, fs_pod *pod, const double *weights, fs_field *v_out, fs_field *p_out);
int fs_pod_read(fs_ctx *ctx, fs_pod *pod, long long *launches, long long *samples);
int fs_pod_get(fs_ctx *ctx, fs_pod *pod, void *slots_out);
int fs_pod_set(fs_ctx *ctx, fs_pod *pod, const void *slots_in, long long launches, long long samples);
int fs_pod_reset(fs_ctx *ctx, fs_pod *pod);
int fs_pod_free(fs_ctx *ctx, fs_pod *pod);

/* Flow maps through the resident snapshots (new, ABI 22): a lattice of particles carried through the ring of a snapshot POD, forwards or
 * backwards in time, and the largest eigenvalue lam of the Cauchy-Green tensor of the map - FTLE = log(lam) / (2 |T|) is the host's (fs/lcs.py).
 * Kernels, operation order and the bit-for-bit specification: csrc/fs_lcs.h.  Only reads the ring and the mask; never part of a captured step.
 * Single-GPU contexts: create returns FS_ERR_UNSUPPORTED on a slab context, as fs_pod_create.
 * create:  box = {x0, y0, x1, y1} in cells, 0 <= x0 < x1 <= X, 0 <= y0 < y1 <= Y; refine r in {1, 2, 4, 8}: nx = r (x1 - x0) by ny = r (y1 - y0)
 *          nodes, at most 2^30; node (a, b) starts at (x0 + (a + 0.5) / r, y0 + (b + 0.5) / r), status 0 (alive) or FS_FLOWMAP_UNSEEDED where the
 *          start cell is a wall cell; lam NaN.  28 bytes per node.  Needs the mask.
 * advance: every alive node across one interval of the ring, from slot_from to slot_to (0 .. M - 1, different), in `substeps` (1 ..
 *          FS_FLOWMAP_MAX_SUBSTEPS) midpoint steps of signed size h (finite, not 0; cell units: +- every dt / (dx substeps)) in the velocity
 *          interpolated bilinearly in space and linearly in time between the two slots.  A node that leaves the domain, or enters an outflow cell
 *          (h > 0) or an inflow cell (h < 0), gets status FS_TRACER_LEFT, one that enters a wall cell FS_TRACER_WALL; it keeps its last valid
 *          position and is never moved again.  One launch; no synchronisation.
 * cauchy_green: lam of every node from the positions of its lattice neighbours (central differences, one-sided beside the lattice's edge and
 *          beside UNSEEDED nodes; NaN where a direction has neither neighbour, and on UNSEEDED nodes).  One launch; no synchronisation.
 * get:     synchronises; x, y, lam receive [ny][nx] doubles and status [ny][nx] ints (a contiguous); each may be NULL.
 * reset:   seeds again (the state after create).
 * free:    as fs_mean_free.
 * Every call returns FS_ERR_STATE during graph capture / tape recording, and FS_ERR_ARG - without touching anything - for a null argument
 * (get's outputs apart), a box outside the grid or empty, another refine, too many nodes, a slot outside 0 .. M - 1, equal slots, substeps
 * outside 1 .. FS_FLOWMAP_MAX_SUBSTEPS, a non-finite or zero h.                                                                          */
#define FS_FLOWMAP_UNSEEDED 4
#define FS_FLOWMAP_MAX_SUBSTEPS 16
typedef struct fs_flowmap fs_flowmap;
int fs_flowmap_create(fs_ctx *ctx, const int *box, int refine, fs_flowmap **out);
int fs_flowmap_advance(fs_ctx *ctx, fs_flowmap *fm, const fs_pod *pod, int slot_from, int slot_to, double h, int substeps);
int fs_flowmap_cauchy_green(fs_ctx *ctx, fs_flowmap *fm);
int fs_flowmap_get(fs_ctx *ctx, fs_flowmap *fm, double *x, double *y, int *status, double *lam);
int fs_flowmap_reset(fs_ctx *ctx, fs_flowmap *fm);
int fs_flowmap_free(fs_ctx *ctx, fs_flowmap *fm);

/* Vortex identification (new, ABI 23): a criterion field of the velocity gradient, its 4-connected components of equal rotation sense labelled
 * on the device in a fixed number of launches, and one record of INTEGER sums per component appended to a ring of samples (kernels, operation
 * order, accumulator layout and bounds: csrc/fs_vortex.h).  Planes are [Y][X] with x contiguous; a label is the smallest j * X + i of the
 * component, -1 on a cell without a flag.  Single-GPU contexts: create, label and criterion return FS_ERR_UNSUPPORTED on a slab context.
 * create:  criterion 0 "q", 1 "swirl", 2 "vorticity"; threshold finite, in 1 / time^2; scale = 2^(30 - e) > 0 with e = ceil(log2(omega_max)):
 *          q = llrint(om * scale) clamped to +-2^30; every >= 1, start >= 0 (the sampling rule of fs_mean_create); min_area >= 1;
 *          1 <= max_vortices <= FS_VORTEX_MAX_VORTICES; max_components >= 1; capacity >= 1 samples of FS_VORTEX_NHEAD + FS_VORTEX_NREC *
 *          max_vortices long long words.  9 bytes per cell, 8 FS_VORTEX_NACC max_components for the table, and the ring.
 * launch:  nine launches behind the step, nothing else (no allocation, copy or synchronisation: capturable); all of them return at once
 *          unless this launch samples and the ring has room.  limit > 0: v still owes limit_field(limit).  A sampling launch that finds the
 *          ring full counts as lost.
 * read:    synchronises; copies the n samples of the ring (at most max_samples, else FS_ERR_ARG) to `out`, empties the ring, and returns the
 *          launch count and the samples lost since the last read.  Sample: {launch index (from 0), components, passed, count, clipped,
 *          dropped cells, 0, 0}, then `count` records {label, area, sum q, sum |q|, sum (2i+1), sum (2j+1), sum |q|(2i+1) low 32 bits / the
 *          rest, the same for |q|(2j+1), min i, max i, min j, max j, peak, flag of the root}; the words behind them are undefined.
 * get_labels: the flag and label planes of the last sampling launch (zeros / undefined before the first); either may be NULL.
 * set:     the launch count (resume; the ring is empty).
 * label:   the labels of a caller's flag plane (host memory, any non-zero byte is a flag; cells join when their bytes are equal).
 * criterion: the criterion field as doubles, 0 on cells that are not fluid.  Needs the mask.
 * free:    as fs_mean_free (during a capture the release is deferred to its end).
 * Everything but launch and free returns FS_ERR_STATE during graph capture / tape recording.                                             */
#define FS_VORTEX_NACC 15
#define FS_VORTEX_NREC 16
#define FS_VORTEX_NHEAD 8
#define FS_VORTEX_MAX_VORTICES 1024
typedef struct fs_vortex fs_vortex;
int fs_vortex_create(fs_ctx *ctx, int criterion, double threshold, double scale, long long every, long long start, int min_area, int max_vortices,
                     int max_components, int capacity, fs_vortex **out);
int fs_vortex_launch(fs_ctx *ctx, fs_vortex *vx, double limit, double dx, const fs_field *v);
int fs_vortex_read(fs_ctx *ctx, fs_vortex *vx, long long *out, int max_samples, int *n_out, long long *launches, long long *lost);
int fs_vortex_get_labels(fs_ctx *ctx, fs_vortex *vx, unsigned char *flags, int *labels);
int fs_vortex_set(fs_ctx *ctx, fs_vortex *vx, long long launches);
int fs_vortex_label(fs_ctx *ctx, const unsigned char *flags, int *labels);
int fs_vortex_criterion(fs_ctx *ctx, int which, double limit, double dx, const fs_field *v, double *out);
int fs_vortex_free(fs_ctx *ctx, fs_vortex *vx);

/* Field distributions (new, ABI 24): histograms and joint histograms of a quantity over the fluid cells, accumulated over a run by launches that
 * can be captured in a hipGraph, and exact order statistics of the current fields (kernels, the value of a cell, the bin rule and the radix
 * select: csrc/fs_dist.h).  Counts are 64-bit integers and an order statistic is one stored value: both are exact and do not depend on the
 * order of any atomic.  Quantities: 0 "u", 1 "w", 2 "p", 3 "speed", 4 "vorticity", 5 "q", 6 "swirl", as doubles; the selection is the fluid
 * cells (mask 0) of a half-open box x0, y0, x1, y1 of global cells (0 <= x0 < x1 <= X, 0 <= y0 < y1 <= Y, else FS_ERR_ARG).  NaN values are
 * counted apart; +-Inf are values.  Single-GPU contexts: create and select return FS_ERR_UNSUPPORTED on a slab context.
 * create:  1 <= nchan <= FS_DIST_MAX_CHANNELS tables.  spec: quantity over [lo, hi) in `bins` bins, 1 <= bins <= FS_DIST_MAX_BINS, lo < hi
 *          finite with a finite positive bins / (hi - lo); quantity_b >= 0 makes the table joint with quantity_b over [lo_b, hi_b) in bins_b
 *          bins, bins * bins_b <= FS_DIST_MAX_BINS, bin bb * bins + ba (quantity_b < 0: 1-D, the _b members are not read).  every >= 1,
 *          start >= 0 (the sampling rule of fs_mean_create).  Tables and counters start at zero.
 * launch:  one pass per channel and a one-lane tick, nothing else (no allocation, copy or synchronisation: capturable); the passes return
 *          at once unless this launch samples.  limit > 0: v still owes limit_field(limit).  Needs the mask.
 * read:    synchronises; counts: the bins (bins, or bins * bins_b) words of channel `chan`; tails: FS_DIST_NTAIL words {below, above, nan, 0}
 *          - joint: {outside, 0, nan, 0}; either may be NULL.  Resets nothing.
 * get / set: all tables, channel after channel, each its bins then its FS_DIST_NTAIL tail words, for checkpoints;
 *          set also takes the counters, 0 <= samples <= launches.
 * reset:   tables and sample count to zero; the launch count runs on.
 * select:  the ranks[k]-th smallest (0-based; 0 <= nranks <= FS_DIST_MAX_RANKS, ascending, equal ones allowed) of the values of `quantity`
 *          on the selection that are not NaN, by a radix select over their order-preserving keys -> values_out[k], exactly the double a full
 *          sort would put there; *n: how many such values, *nan: selected cells whose value is NaN (both written before the ranks are
 *          looked at).  n == 0 with nranks > 0, or a rank >= n: FS_ERR_ARG.  Extra device memory of 8 bytes per cell of the box for the
 *          duration of the call (nranks == 0: none); synchronises.
 * free:    as fs_mean_free (during a capture the release is deferred to its end).
 * Everything but launch and free returns FS_ERR_STATE during graph capture / tape recording.                                             */
#define FS_DIST_MAX_BINS 4096
#define FS_DIST_MAX_CHANNELS 4
#define FS_DIST_MAX_RANKS 8
#define FS_DIST_NTAIL 4
typedef struct fs_dist fs_dist;
typedef struct fs_dist_spec {
    int quantity, bins, quantity_b, bins_b;
    int box[4];
    double lo, hi, lo_b, hi_b;
} fs_dist_spec;
int fs_dist_create(fs_ctx *ctx, int nchan, const fs_dist_spec *specs, long long every, long long start, fs_dist **out);
int fs_dist_launch(fs_ctx *ctx, fs_dist *d, double limit, double dx, const fs_field *v, const fs_field *p);
int fs_dist_read(fs_ctx *ctx, fs_dist *d, int chan, long long *counts, long long *tails, long long *launches, long long *samples);
int fs_dist_get(fs_ctx *ctx, fs_dist *d, long long *words_out);
int fs_dist_set(fs_ctx *ctx, fs_dist *d, const long long *words_in, long long launches, long long samples);
int fs_dist_reset(fs_ctx *ctx, fs_dist *d);
int fs_dist_free(fs_ctx *ctx, fs_dist *d);
int fs_dist_select(fs_ctx *ctx, int quantity, const int *box, double limit, double dx, const fs_field *v, const fs_field *p,
                   const long long *ranks, int nranks, double *values_out, long long *n, long long *nan);

/* Energy spectra (new, ABI 25): the windowed 2-D FFT of the velocity over a box of cells and the accumulated power of every bin, by launches
 * that can be captured in a hipGraph (the transform, the operation order and the kernels: csrc/fs_spec.h).  All doubles; a plane is a pure
 * function of the field, the tables and the order of the samples - no atomics.  The box is half-open, x0, y0, x1, y1 of global cells inside the
 * grid, its sides Nx = x1 - x0 and Ny = y1 - y0 powers of two in FS_SPEC_MIN_N .. FS_SPEC_MAX_N (else FS_ERR_ARG).  Planes are (Nx, Ny) in C
 * order, bin (a, b) at a * Ny + b, indexed like a DFT: a and b are the wavenumber indices modulo N.  Single-GPU contexts: create returns
 * FS_ERR_UNSUPPORTED on a slab context.
 * create:  wx[Nx], wy[Ny]: the window of each axis; twx, twy: per axis N / 2 pairs (cos, -sin) of 2 pi k / N, N doubles - all four are copied;
 *          the library calls no sin or cos.  detrend != 0: Z'[a, b] = Z[a, b] - (Z[0, 0] c[a]) c[b] with c[0] = 1, c[1] = c[N - 1] = c1x / c1y
 *          and 0 elsewhere (nine bins).  every >= 1, start >= 0 (the sampling rule of fs_mean_create).  Power and counters start at zero.
 *          Device memory: 40 bytes per cell of the box.
 * launch:  five kernel launches, nothing else (no allocation, copy or synchronisation: capturable); all but the last return at once unless
 *          this launch samples: Z = FFT2((u + i w) wx wy), wall cells as zeros, and power += |Z'|^2.  limit > 0: v still owes
 *          limit_field(limit).  Needs the mask.
 * read:    synchronises; power: Nx * Ny doubles, the sums over the samples, or NULL; launches, samples: may be NULL.  Resets nothing.
 * plane:   the Z' of the last sampling launch, 2 * Nx * Ny doubles (re, im interleaved); zeros before the first.
 * get / set: the power plane and the counters, for checkpoints; set: 0 <= samples <= launches.
 * reset:   power and sample count to zero; the launch count runs on.
 * free:    as fs_mean_free (during a capture the release is deferred to its end).
 * Everything but launch and free returns FS_ERR_STATE during graph capture / tape recording.                                             */
#define FS_SPEC_MIN_N 8
#define FS_SPEC_MAX_N 4096
typedef struct fs_spec fs_spec;
int fs_spec_create(fs_ctx *ctx, const int *box, const double *wx, const double *wy, const double *twx, const double *twy, double c1x, double c1y,
                   int detrend, long long every, long long start, fs_spec **out);
int fs_spec_launch(fs_ctx *ctx, fs_spec *s, double limit, const fs_field *v);
int fs_spec_read(fs_ctx *ctx, fs_spec *s, double *power, long long *launches, long long *samples);
int fs_spec_plane(fs_ctx *ctx, fs_spec *s, double *plane);
int fs_spec_get(fs_ctx *ctx, fs_spec *s, double *power, long long *launches, long long *samples);
int fs_spec_set(fs_ctx *ctx, fs_spec *s, const double *power, long long launches, long long samples);
int fs_spec_reset(fs_ctx *ctx, fs_spec *s);
int fs_spec_free(fs_ctx *ctx, fs_spec *s);

/* Cross-spectra of two flow quantities (new, ABI 26): the windowed 2-D FFT of the packed plane a + i b over a box of cells - a, b two of the
 * seven quantities of fs_dist_spec (0 "u", 1 "w", 2 "p", 3 "speed", 4 "vorticity", 5 "q", 6 "swirl") -, split on the device into the transforms A
 * and B of the two real fields, and the accumulated |A|^2, |B|^2 and A conj(B) of every bin, by launches that can be captured in a hipGraph
 * (operation order and kernels: csrc/fs_xspec.h).  Box, tables, detrend, sampling rule, plane layout and refusals are those of fs_spec_*; all
 * doubles, no atomics.  Single-GPU contexts: create returns FS_ERR_UNSUPPORTED on a slab context.
 * create:  as fs_spec_create, and 0 <= qa <= 6, -1 <= qb <= 6 (-1: one scalar, the imaginary part of the packed plane is +0), dx finite and > 0
 *          (the gradients).  u, w, p, speed contribute where mask != 1, vorticity, q, swirl where mask == 0; every other cell takes +0.
 *          Device memory: 64 bytes per cell of the box (two work planes, FS_XSPEC_NPLANE accumulators); 40 with qb = -1 (one accumulator).
 * launch:  five kernel launches, nothing else (capturable); all but the last return at once unless this launch samples.  limit > 0: v still
 *          owes limit_field(limit).  Needs the mask.
 * read:    synchronises; sums: the accumulator planes Paa, Pbb, Cre, Cim (C = A conj B), FS_XSPEC_NPLANE * Nx * Ny doubles - with qb = -1
 *          Paa alone, Nx * Ny -, or NULL; launches, samples: may be NULL.  Resets nothing.
 * plane:   the detrended packed plane Z' of the last sampling launch, 2 * Nx * Ny doubles (re, im interleaved); zeros before the first.
 * get / set: the accumulators and the counters, for checkpoints; set: 0 <= samples <= launches.
 * reset:   accumulators and sample count to zero; the launch count runs on.
 * free:    as fs_mean_free.
 * Everything but launch and free returns FS_ERR_STATE during graph capture / tape recording.                                             */
#define FS_XSPEC_NPLANE 4
typedef struct fs_xspec fs_xspec;
int fs_xspec_create(fs_ctx *ctx, const int *box, int qa, int qb, double dx, const double *wx, const double *wy, const double *twx, const double *twy,
                    double c1x, double c1y, int detrend, long long every, long long start, fs_xspec **out);
int fs_xspec_launch(fs_ctx *ctx, fs_xspec *s, double limit, const fs_field *v, const fs_field *p);
int fs_xspec_read(fs_ctx *ctx, fs_xspec *s, double *sums, long long *launches, long long *samples);
int fs_xspec_plane(fs_ctx *ctx, fs_xspec *s, double *plane);
int fs_xspec_get(fs_ctx *ctx, fs_xspec *s, double *sums, long long *launches, long long *samples);
int fs_xspec_set(fs_ctx *ctx, fs_xspec *s, const double *sums, long long launches, long long samples);
int fs_xspec_reset(fs_ctx *ctx, fs_xspec *s);
int fs_xspec_free(fs_ctx *ctx, fs_xspec *s);

/* Scale-to-scale fluxes by filtering (new, ABI 27): the velocity and the vorticity box-filtered at up to FS_FLUX_MAX_WIDTHS half-widths r (a
 * square of (2 r + 1)^2 cells, direct ordered sums), the sub-filter stresses tau = filt(u_i u_j) - filt(u_i) filt(u_j), and per cell of a box the
 * accumulated energy flux PI = -tau_ij S_ij, enstrophy flux ZF and sub-filter energy K, by launches that can be captured in a hipGraph (the
 * quantities, the operation order and the kernels: csrc/fs_flux.h).  All doubles, no atomics; a plane is a pure function of the field and the
 * order of the samples.  The box is half-open, x0, y0, x1, y1 of global cells inside the grid, any sides; the filter reads outside the box, never
 * outside the grid; solid cells count as fluid at rest.  Planes are (Ny, Nx) in C order, cell (a, b) of the box at b * Nx + a.  Single-GPU
 * contexts: create returns FS_ERR_UNSUPPORTED on a slab context.
 * create:  nr half-widths, 1 .. FS_FLUX_MAX_WIDTHS of them, each 1 .. FS_FLUX_MAX_R, strictly increasing; a cell (i, j) is valid for r when
 *          r + 1 <= i <= X - 2 - r and r + 1 <= j <= Y - 2 - r, and a half-width without a valid cell in the box is FS_ERR_ARG.  dx finite and > 0.
 *          every >= 1, start >= 0 (the sampling rule of fs_mean_create).  Device memory: 192 bytes per cell of the box dilated by r_max + 1
 *          (clipped to the grid) and 24 bytes per cell of the box and half-width.
 * launch:  2 + 3 nr kernel launches, nothing else (capturable); all but the last return at once unless this launch samples.  limit > 0: v still
 *          owes limit_field(limit).  Needs the mask.
 * read:    synchronises; sums: nr * FS_FLUX_NSUM planes - per half-width PI, ZF, K, the sums over the samples; a cell that is not valid for
 *          the half-width holds +0 -, or NULL; launches, samples: may be NULL.  Resets nothing.
 * filtered: the FS_FLUX_NQ filtered planes (of U, W, OM, U U, U W, W W, U OM, W OM) of half-width number `width` over the box, from the
 *          fields of the last sampling launch (zeros before the first): two kernel launches and a download.  +0 where the window leaves the grid.
 * get / set: the sums and the counters, for checkpoints; set: 0 <= samples <= launches.
 * reset:   sums and sample count to zero; the launch count runs on.
 * free:    as fs_mean_free.
 * Everything but launch and free returns FS_ERR_STATE during graph capture / tape recording.                                             */
#define FS_FLUX_NQ 8
#define FS_FLUX_NSUM 3
#define FS_FLUX_MAX_WIDTHS 8
#define FS_FLUX_MAX_R 64
typedef struct fs_flux fs_flux;
int fs_flux_create(fs_ctx *ctx, const int *box, int nr, const int *half_widths, double dx, long long every, long long start, fs_flux **out);
int fs_flux_launch(fs_ctx *ctx, fs_flux *s, double limit, const fs_field *v);
int fs_flux_read(fs_ctx *ctx, fs_flux *s, double *sums, long long *launches, long long *samples);
int fs_flux_filtered(fs_ctx *ctx, fs_flux *s, int width, double *planes);
int fs_flux_get(fs_ctx *ctx, fs_flux *s, double *sums, long long *launches, long long *samples);
int fs_flux_set(fs_ctx *ctx, fs_flux *s, const double *sums, long long launches, long long samples);
int fs_flux_reset(fs_ctx *ctx, fs_flux *s);
int fs_flux_free(fs_ctx *ctx, fs_flux *s);

/* Kinetic-energy budget (new, ABI 28): the raw moments behind the budget of k = (<u'u'> + <w'w'>) / 2 - production, dissipation, turbulent and
 * pressure transport, pressure dilatation -, accumulated per FLUID cell (mask == 0) of a box by a launch that can be captured in a hipGraph
 * (the values, their order and the kernel: csrc/fs_budget.h; the algebra: fs/budgets.py).  FS_BUDGET_NPLANE planes of double:
 *   0-2 S_u S_w S_p | 3-5 S_uu S_ww S_uw | 6-7 S_pu S_pw | 8-11 S_uuu S_uuw S_wwu S_www | 12-15 S_ux S_uy S_wx S_wy |
 *   16-19 S_uxux S_uyuy S_wxwx S_wywy | 20 S_pd (p times ux + wy)
 * with the gradient by central differences over 2 dx, neighbour indices clamped at the grid's edge, neighbours taken as stored.  All doubles, no
 * atomics; one lane owns a cell, so a plane is a pure function of the fields and the order of the samples; planes 0 - 5 equal fs_mean's on the
 * fluid cells bit for bit.  A cell of the box that is not fluid holds +0.  Planes are (Ny, Nx) in C order, cell (a, b) of the box at b * Nx + a.
 * Single-GPU contexts: create returns FS_ERR_UNSUPPORTED on a slab context.
 * create:  the half-open box x0, y0, x1, y1 of global cells, anything inside the grid with at least one cell; a box without a fluid cell is
 *          FS_ERR_ARG (needs the mask).  dx finite and > 0; every >= 1, start >= 0 (the sampling rule of fs_mean_create).  Device memory: 168
 *          bytes per cell of the box.
 * launch:  two kernel launches, nothing else (capturable); the first returns at once unless this launch samples.  limit > 0: v still owes
 *          limit_field(limit), and the kernel limits every value it reads, the neighbours' too.  Needs the mask.
 * read:    synchronises; sums: the planes, or NULL; launches, samples: may be NULL.  Resets nothing.
 * get / set: the planes and the counters, for checkpoints; set: 0 <= samples <= launches.
 * reset:   planes and sample count to zero; the launch count runs on.
 * free:    as fs_mean_free.
 * Everything but launch and free returns FS_ERR_STATE during graph capture / tape recording.                                             */
#define FS_BUDGET_NPLANE 21
typedef struct fs_budget fs_budget;
int fs_budget_create(fs_ctx *ctx, int x0, int y0, int x1, int y1, double dx, long long every, long long start, fs_budget **out);
int fs_budget_launch(fs_ctx *ctx, fs_budget *s, double limit, const fs_field *v, const fs_field *p);
int fs_budget_read(fs_ctx *ctx, fs_budget *s, double *sums, long long *launches, long long *samples);
int fs_budget_get(fs_ctx *ctx, fs_budget *s, double *sums, long long *launches, long long *samples);
int fs_budget_set(fs_ctx *ctx, fs_budget *s, const double *sums, long long launches, long long samples);
int fs_budget_reset(fs_ctx *ctx, fs_budget *s);
int fs_budget_free(fs_ctx *ctx, fs_budget *s);

/* Multigrid pressure correction (new, ABI 19): one W-cycle (two coarse visits per level) on a mask-aware hierarchy of coarse levels, for the
 * third pressure updater (fs/pressure_updater.py MultigridPressureUpdater; kernels and operation order: csrc/fs_mg.h).  Single-GPU contexts.
 * create:  levels 1 .. nlevels with dims = nx_1, ny_1, nx_2, ny_2, ... - level 1 half the grid, every level half the one above; cx, cy, diag:
 *          the levels' coefficients in the context's dtype, level after level, each [ny][nx] with x contiguous (host memory; built by
 *          fs/multigrid.py - diag 0 marks an inactive cell).  tail_cells: the levels from the first one of at most that many cells down run
 *          in ONE workgroup that holds them in LDS (< 0: from the first level that fits the LDS of a workgroup; 0: no such kernel) - the
 *          bits are the same for every value.  coarse_sweeps / coarsest_sweeps: red-black sweeps around every coarse visit / on the last level.
 * cycle:   pc must hold a pressure the boundary kernel has been applied to.  R1 <- restriction of 4 (predict_p(pc, vc) - pc) over fluid
 *          cells; E1 <- W(1, R1); pc[fluid] += E1[i >> 1, j >> 1] and pn[fluid] += the same (both buffers of the red-black pair are iterates
 *          of the same equation).  Every launch goes on the context's stream: capturable, no synchronisation, no allocation, no atomics,
 *          and no kernel waits for another workgroup.
 * info:    levels; the first level the one-workgroup kernel holds (0: none); the kernel launches of the last cycle.
 * free:    as fs_mean_free (during a capture the release is deferred to its end).  create returns FS_ERR_STATE during graph capture.
 * set_direct (ABI 20): attaches an exact solve to the hierarchy's LAST level: from then on a cycle computes that level's E = M R on its n
 *          active cells with ONE launch (k_mg_direct, csrc/fs_mg.h: the operation order is written there; none when n == 0) instead of
 *          coarsest_sweeps sweeps.  cells: the n active cells' indices J * nx + I in the level, strictly ascending; M: the inverse of the
 *          level's operator on them (fs/multigrid.py direct_solve), [n][row_stride] in the context's dtype, row-major, every row padded with
 *          zeros to row_stride = 64 * ceil(n / 64) elements.  Both arrays are copied to the device; fs_mg_free releases them.  FS_ERR_ARG
 *          for a null argument, n < 0 or n > 4096, another stride, cells that are not strictly ascending or lie outside the level;
 *          FS_ERR_STATE for a hierarchy with a one-workgroup tail (create it with tail_cells = 0), for a second call on the same handle and
 *          during graph capture / tape recording.  A refused call changes nothing.
 * direct_info: the level with an exact solve (nlevels; 0: none) and its active cells.                                                        */
typedef struct fs_mg fs_mg;
int fs_mg_create(fs_ctx *ctx, int nlevels, const int *dims, const void *cx, const void *cy, const void *diag, long long tail_cells,
                 int coarse_sweeps, int coarsest_sweeps, fs_mg **out);
int fs_mg_cycle(fs_ctx *ctx, fs_mg *m, double dt, double dx, fs_field *pc, fs_field *pn, const fs_field *vc);
int fs_mg_info(fs_ctx *ctx, fs_mg *m, int *levels, int *tail_level, int *launches);
int fs_mg_set_direct(fs_ctx *ctx, fs_mg *m, int n, const int *cells, const void *M, long long row_stride);
int fs_mg_direct_info(fs_ctx *ctx, fs_mg *m, int *direct_level, int *direct_cells);
int fs_mg_free(fs_ctx *ctx, fs_mg *m);

/* Tracer particles (new): n passive particles advanced on the device by one launch per step that can be captured in a hipGraph
 * (csrc/fs_tracer.h).  Positions are doubles in CELL units: cell (i, j) covers [i, i + 1) x [j, j + 1), its stored value sits at
 * (i + 0.5, j + 0.5).  State per particle: x, y, age (steps), status (FS_TRACER_ALIVE / _LEFT / _WALL / _EXPIRED), respawns, and the
 * constant seed; plus one device counter of launches.  Single-context grids only: on a slab context (or with a communicator) create
 * returns FS_ERR_UNSUPPORTED - particles that cross slab boundaries would have to migrate.
 * create:   n >= 1 seeds as [n][2] doubles (x, y), each inside [0, X) x [0, Y) (FS_ERR_ARG otherwise; whether the cell is fluid is the
 *           caller's business); respawn != 0: a particle that meets a fate starts again at its seed; max_age > 0: fate EXPIRED at that age.
 * advance:  every particle with status 0 takes one midpoint step h = dt / dx in the 2-channel field v:
 *             V(x, y): bilinear in the four stored values around (x - 0.5, y - 0.5), i0 = clamp(floor(x - 0.5), 0, X - 2), tx = min(max(
 *             x - 0.5 - i0, 0), 1), likewise in y; V = (1 - ty) ((1 - tx) a00 + tx a10) + ty ((1 - tx) a01 + tx a11) on values promoted to
 *             double; wall cells take part with what they store.  limit > 0: v still owes limit_field(limit) (a deferred pass): every
 *             corner's (u, w) is limited first, in the field's precision, as that pass would store it.
 *             k1 = V(x, y); (xm, ym) = (x, y) + (0.5 h) k1; not inside -> LEFT.  k2 = V(xm, ym); (xn, yn) = (x, y) + h k2; not inside ->
 *             LEFT.  Mask of cell (floor xn, floor yn): 1 -> WALL, 3 -> LEFT, else the particle moves there.  age += 1; max_age > 0 and
 *             age >= max_age and no other fate -> EXPIRED.
 *           With respawn a fate puts the particle back on its seed (age 0, respawns + 1, status 0); without, status takes the fate's code,
 *           LEFT / WALL keep the last valid position, EXPIRED keeps (xn, yn), and the particle is never touched again.  Every operation is
 *           one IEEE double operation in the order written (no FMA): an IEEE double loop reproduces the state bit for bit.  No atomics;
 *           changes no field; the counter advances on the device.
 * read:     synchronises; pos (may be NULL) receives [4][n] doubles: x, y, x_seed, y_seed; ints (may be NULL) [3][n]: age, status, respawns.
 *           Always in SEED order (entry k belongs to seed k), whatever fs_tracer_sort has done to the device arrays.
 * write:    the inverse of read (checkpoints): status in 0 .. 3, age and respawns >= 0, launches >= 0.  Seed order; the slot order on the
 *           device is the seed order again afterwards.
 * sort:     reorders the particle SLOTS on the device by key = floor(y) * NB + floor(x) / FS_TRACER_SORT_BIN_CELLS, NB = ceil(X /
 *           FS_TRACER_SORT_BIN_CELLS); a particle that is not alive, or not inside the domain (NaN included), has key = Y * NB.  Afterwards
 *           the keys are non-decreasing along the slots; the order inside a bin is unspecified.  A counting sort in a handful of launches
 *           (integer atomics; profiled as tracer_sort_count / _scan / _scatter / _copy); its scratch (36 bytes per particle + 4 bytes per
 *           bin) is allocated at the first sort and freed with the set.  Changes nothing any other entry point shows except order, and no
 *           device address: a graph that holds the advance launch stays valid.
 * order:    synchronises; ids receives [n] ints: the seed index of the particle in slot k (the identity until the first sort).
 * fields:   one launch: every alive particle inside the domain adds 1 to the count and its age to the age sum of cell (floor x, floor y).
 *           count receives [Y][X] ints, age_sum [Y][X] 64-bit sums (x contiguous, the library's layout).  Integer atomics: exact and
 *           repeatable.  12 bytes per cell of device memory for the duration of the call.
 * draw:     stores (r, g, b) into pixel (floor x, floor y) of the 3-channel field rgb for every particle with status 0.
 * free:     a graph that holds the launch must not be replayed afterwards; during a capture the release is deferred to its end (as
 *           fs_history_free).
 * create, read, write, sort, order and fields return FS_ERR_STATE during graph capture / tape recording.                               */
#define FS_TRACER_SORT_BIN_CELLS 32
#define FS_TRACER_ALIVE 0
#define FS_TRACER_LEFT 1
#define FS_TRACER_WALL 2
#define FS_TRACER_EXPIRED 3
typedef struct fs_tracer fs_tracer;
int fs_tracer_create(fs_ctx *ctx, int n, const double *seeds_xy, int respawn, int max_age, fs_tracer **out);
int fs_tracer_advance(fs_ctx *ctx, fs_tracer *t, double h, double limit, const fs_field *v);
int fs_tracer_read(fs_ctx *ctx, fs_tracer *t, double *pos, int *ints, long long *launches);
int fs_tracer_write(fs_ctx *ctx, fs_tracer *t, const double *pos, const int *ints, long long launches);
int fs_tracer_draw(fs_ctx *ctx, fs_tracer *t, double r, double g, double b, fs_field *rgb);
int fs_tracer_sort(fs_ctx *ctx, fs_tracer *t);
int fs_tracer_order(fs_ctx *ctx, fs_tracer *t, int *ids);
int fs_tracer_fields(fs_ctx *ctx, fs_tracer *t, int *count, long long *age_sum);
int fs_tracer_free(fs_ctx *ctx, fs_tracer *t);

/* Inertial tracer sets, wall deposition and accumulated occupancy (new; csrc/fs_tracer.h).  An inertial set is a tracer set whose particles
 * also carry a velocity pu, pw (double, the field's velocity units), a response alpha in (0, 1] and a response time tau >= 0; the set
 * carries gravity (gx, gy) in velocity per time.  Every fs_tracer_* call above works on it; fs_tracer_advance dispatches on the set's kind.
 * create_inertial: as create, plus alpha [n] and tau [n] (seed order; FS_ERR_ARG unless 0 < alpha <= 1, tau finite and >= 0, gravity
 *           finite).  The caller computes alpha = -expm1(-dt / tau), 1 for tau == 0: the device evaluates no transcendental function.
 *           deposits != 0: the set owns an int plane [Y][X], zeroed.  Slab contexts: FS_ERR_UNSUPPORTED.
 * advance (inertial set): every particle with status 0, each line ONE IEEE double operation in the order written, no FMA:
 *             (U, W) = V(x, y) exactly as above (same bilinear form, clamps and handling of a deferred limit_field)
 *             age == 0: pu = U; pw = W            (released with the fluid's velocity: creation and every respawn)
 *             su = tau gx; sw = tau gy; pu = pu + alpha ((U + su) - pu); pw = pw + alpha ((W + sw) - pw)
 *             xn = x + h pu; yn = y + h pw; not inside [0, X) x [0, Y) (NaN included) -> LEFT before any index is formed
 *             mask of cell (floor xn, floor yn): 1 -> WALL, 3 -> LEFT, else the particle moves there; age and max_age as above.
 *           Fates as above; a respawn also stores pu = pw = 0 (never read), without respawn the updated pu, pw are stored in every case.
 *           With deposits a particle whose fate is WALL adds 1 to cell (floor xn, floor yn) of the plane (one integer atomic), respawn or
 *           not.  One gather stage: as tau -> 0 this is the forward-Euler tracer, not the midpoint rule of a passive set; a particle may
 *           cross more than one cell per step.  Profiled as tracer_advance_inertial.
 * read_vel / write_vel: synchronise; vel is [2][n] doubles pu, pw in SEED order.
 * write (inertial set): pu, pw follow their particles back into seed order; alpha and tau are those of create_inertial.
 * sort (inertial set): carries pu, pw, alpha, tau with the slots (32 more bytes of scratch per particle).
 * deposits / deposits_write: synchronise; [Y][X] ints (x contiguous); FS_ERR_ARG for a set without the plane, or counts < 0.
 * accum_create: attaches to the set (passive or inertial) two resident 64-bit planes [Y][X], occupancy and age_sum, zeroed, and a sample
 *           counter; every >= 1, start >= 0.  One accumulator per set: FS_ERR_STATE while one is attached.
 * accum_add: one launch, to be issued behind fs_tracer_advance; can be captured.  Gated on the device from the set's launch counter by the
 *           rule of fs_mean_accumulate: with n launches of the advance before this step's since accum_create, the launch samples when
 *           n + 1 > start and (n + 1 - start) % every == 0.  A sampling launch adds, for every alive particle inside the domain, 1 to
 *           occupancy and its age to age_sum of cell (floor x, floor y) (integer atomics: exact, the sum of the fs_tracer_fields snapshots
 *           at the sampled steps) and counts the sample.  Profiled as tracer_accumulate.
 * accum_read: synchronises; occupancy, age_sum (each may be NULL) [Y][X] 64-bit; launches: advances since accum_create; samples.
 * accum_write: the inverse (checkpoints; after fs_tracer_write): 0 <= samples <= launches <= the set's launch count.
 * accum_reset: planes and samples to zero; the phase of every / start runs on.
 * accum_free: a graph that holds the launch must not be replayed afterwards; during a capture the release is deferred to its end.
 *           fs_tracer_free releases the accumulator with the set.
 * create_inertial, read_vel, write_vel, deposits, deposits_write, accum_create, accum_read, accum_write and accum_reset return FS_ERR_STATE
 * during graph capture / tape recording.                                                                                              */
int fs_tracer_create_inertial(fs_ctx *ctx, int n, const double *seeds_xy, const double *alpha, const double *tau, double gx, double gy, int respawn,
                              int max_age, int deposits, fs_tracer **out);
int fs_tracer_read_vel(fs_ctx *ctx, fs_tracer *t, double *vel);
int fs_tracer_write_vel(fs_ctx *ctx, fs_tracer *t, const double *vel);
int fs_tracer_deposits(fs_ctx *ctx, fs_tracer *t, int *out);
int fs_tracer_deposits_write(fs_ctx *ctx, fs_tracer *t, const int *in);
int fs_tracer_accum_create(fs_ctx *ctx, fs_tracer *t, long long every, long long start);
int fs_tracer_accum_add(fs_ctx *ctx, fs_tracer *t);
int fs_tracer_accum_read(fs_ctx *ctx, fs_tracer *t, long long *occupancy, long long *age_sum, long long *launches, long long *samples);
int fs_tracer_accum_write(fs_ctx *ctx, fs_tracer *t, const long long *occupancy, const long long *age_sum, long long launches, long long samples);
int fs_tracer_accum_reset(fs_ctx *ctx, fs_tracer *t);
int fs_tracer_accum_free(fs_ctx *ctx, fs_tracer *t);

/* ---- pointwise -------------------------------------------------------------------------------- */
/* limit_field   fs/solver.py:38-43 ;  clamp_field   fs/solver.py:46-49                           */
int fs_limit_field(fs_ctx *ctx, double limit, fs_field *v, int row_begin, int row_end);
int fs_clamp_field(fs_ctx *ctx, double low, double high, fs_field *f, int row_begin, int row_end);

/* Dye transport with the final clamp_field(dye, 0, 1) folded in (build-side optimisation, same bits): CIP advection of the
 * 3-channel dye that stores clamp(value, 0, 1) on fluid cells, and the clamp of the inflow cells (the only other cells the
 * step leaves outside [0, 1]).  Together they replace fs_cip_advect + fs_clamp_field over the whole grid.                    */
int fs_cip_advect_dye_clamped(fs_ctx *ctx, double dt, double dx, fs_field *fn, fs_field *fxn, fs_field *fyn,
                              const fs_field *fc, const fs_field *fxc, const fs_field *fyc, const fs_field *v,
                              int row_begin, int row_end);
int fs_clamp_inflow(fs_ctx *ctx, double low, double high, fs_field *dye, int row_begin, int row_end);

/* ---- visualisation (the image buffers main.py:93-107 shows; all cells, wall cells take the wall colour) ---------------- */
/* FluidSimulator._to_norm        fs/fluid_simulator.py:38-44   0.2 * visualize_norm(v) + 0.002 * visualize_pressure(p)    */
int fs_vis_norm(fs_ctx *ctx, fs_field *rgb, const fs_field *v, const fs_field *p, int row_begin, int row_end);
/* FluidSimulator._to_pressure    fs/fluid_simulator.py:46-51   0.04 * visualize_pressure(p)   (fs/visualization.py:14-16) */
int fs_vis_pressure(fs_ctx *ctx, fs_field *rgb, const fs_field *p, int row_begin, int row_end);
/* FluidSimulator._to_vorticity   fs/fluid_simulator.py:53-58   0.005 * visualize_vorticity(v) (fs/visualization.py:19-22) */
int fs_vis_vorticity(fs_ctx *ctx, double dx, fs_field *rgb, const fs_field *v, int row_begin, int row_end);
/* DyeFluidSimulator._to_dye      fs/fluid_simulator.py:121-126                                                            */
int fs_vis_dye(fs_ctx *ctx, fs_field *rgb, const fs_field *dye, int row_begin, int row_end);

/* ---- multi-GPU: y-slab halo exchange over RCCL (new; the reference is single-device) ---------- */
#define FS_UNIQUE_ID_BYTES 128
/* librccl loads and exports what the exchange needs (*ok; no GPU call): the pre-flight check of an N > 1 job, before any rank can block in
 * ncclCommInitRank.  *ok = 0: the reason is in fs_last_error(). */
int fs_comm_available(int *ok);
int fs_comm_unique_id(void *out_128_bytes);
int fs_comm_init(fs_ctx *ctx, int rank, int nranks, const void *unique_id_128_bytes);
int fs_comm_destroy(fs_ctx *ctx);
/* Fill `depth` ghost rows on each side from the slab neighbours (ncclSend/ncclRecv pairs).  All RCCL calls of a context
 * run on its own communication stream; these two are begin + wait (see below).                                          */
int fs_halo_exchange(fs_ctx *ctx, fs_field *f, int depth);
/* Same for several fields in ONE grouped RCCL call: their ghost-row blocks travel as one packed message per neighbour.   */
int fs_halo_exchange_multi(fs_ctx *ctx, fs_field *const *fields, int nfields, int depth);
/* Split form for overlap: begin() queues the exchange on the communication stream after everything already queued on the
 * compute stream; until wait() the caller may launch kernels that neither read ghost rows nor write the `depth` outermost
 * owned rows of these fields (the interior rows of the kernel that needed the exchange).  wait() orders the compute
 * stream after the exchange.  One exchange in flight per context.                                                        */
int fs_halo_exchange_begin(fs_ctx *ctx, fs_field *const *fields, int nfields, int depth);
/* As begin(), but field k's ghost rows are known to be correct to depth valid_rows[k] already: only depth offsets
 * [valid_rows[k], depth) travel (same numbers on both sides of a slab boundary; the host tracker has them).          */
int fs_halo_exchange_begin_partial(fs_ctx *ctx, fs_field *const *fields, const int *valid_rows, int nfields, int depth);
int fs_halo_exchange_wait(fs_ctx *ctx);
/* Optional, before begin(): the exchange will depend on the compute stream as of NOW - kernels launched between mark() and
 * begin() (same restrictions as above) are already running while the host still issues the exchange.                     */
int fs_halo_exchange_mark(fs_ctx *ctx);
/* Exchanges in line on the compute stream (0, default) or on the communication stream (1: overlappable; FS_OVERLAP=1 at fs_comm_init).  Same
 * bits either way; a tape recorded under one setting is replayed under it. */
int fs_comm_set_overlap(fs_ctx *ctx, int on);
/* Loop-back self-test on a 1-rank communicator: the rank is its own lower and upper neighbour, so afterwards
 * lower ghost rows == first owned rows and upper ghost rows == last owned rows (single-GPU check of the RCCL leg).
 * fs_comm_loopback(ctx, 1) makes every later exchange of a 1-rank communicator behave that way.                          */
int fs_halo_exchange_self(fs_ctx *ctx, fs_field *const *fields, int nfields, int depth);
int fs_comm_loopback(fs_ctx *ctx, int on);
int fs_allreduce_sum(fs_ctx *ctx, double *values, int n);

/* ---- launch-overhead removal: capture the launches issued between begin/end into a hipGraph ---- */
int fs_graph_begin(fs_ctx *ctx);
int fs_graph_end(fs_ctx *ctx, int *graph_id);
int fs_graph_launch(fs_ctx *ctx, int graph_id, int times);
int fs_graph_free(fs_ctx *ctx, int graph_id);

/* ---- command tapes: replay of a recorded launch sequence INCLUDING the RCCL ghost-row exchanges (slab runs) ---------------
 * Between begin and end every kernel entry point and fs_halo_exchange_begin* / _mark / _wait appends a closure holding its
 * arguments (execute = 1: and runs as usual; execute = 0: records only).  fs_tape_replay re-issues the closures `times` times
 * from a C++ loop - the fused driver of SURVEY.md 8b for N > 1, where a hipGraph cannot carry the exchange.  The caller
 * guarantees that the recorded sequence is valid to repeat (fs/runtime.py records a whole period of the buffer rotation and
 * of its ghost-row bookkeeping).                                                                                          */
int fs_tape_begin(fs_ctx *ctx, int execute);
int fs_tape_end(fs_ctx *ctx, int *tape_id);
int fs_tape_length(fs_ctx *ctx, int tape_id, int *nops);
int fs_tape_replay(fs_ctx *ctx, int tape_id, int times);
int fs_tape_free(fs_ctx *ctx, int tape_id);

/* Measurement hygiene (new; no reference counterpart): what THIS GPU streams at - float4 read of one buffer and float4 copy between two
 * buffers of `bytes` each, about budget_ms of GPU time per leg, HIP events on the context's stream.  bench.py prints the two rates and
 * `frac_of_box_copy` next to every roofline fraction, so that a slow box is not mistaken for a regression. */
int fs_box_rates(fs_ctx *ctx, size_t bytes, double budget_ms, double *read_GBps, double *copy_GBps);
/* ... and the rate at which one SIMD issues independent f32 multiplies / adds at 4 waves per SIMD, in 1e9 wave-instructions per second
 * (no memory traffic): what the issue-bound K3+K4 pass is priced against (bench.py roofline.valu_issue). */
int fs_box_valu_rate(fs_ctx *ctx, double budget_ms, double *ginstr_per_simd);
/* The same chains on packed operands (v_pk_mul_f32 / v_pk_add_f32: two f32 operations per lane and instruction) - what the packed bodies of
 * the transport kernels (csrc/fs_k34n.h, fs_k234.h) issue.  Wave-instructions per second and SIMD. */
int fs_box_valu_pk_rate(fs_ctx *ctx, double budget_ms, double *ginstr_per_simd);
/* ... and a float4 copy with 176 f32 multiplies / adds per 16 bytes on the way (5.5 lane-operations per byte moved: the instruction density of the K3+K4 pass): memory system and SIMDs loaded
 * together, in GB/s of read + written bytes. */
int fs_box_mixed_rate(fs_ctx *ctx, size_t bytes, double budget_ms, double *GBps);

/* ---- per-kernel timing with HIP events on the ctx stream (bench.py roofline leg) --------------- */
int fs_prof_enable(fs_ctx *ctx, int on);          /* record an event pair around every launch      */
/* One HIP-event pair on the context's stream around whatever is queued between the two calls (launch boundaries included); fs_span_end waits
 * for it and returns the milliseconds.  Independent of the per-launch profile. */
int fs_span_begin(fs_ctx *ctx);
int fs_span_end(fs_ctx *ctx, double *ms);
int fs_prof_reset(fs_ctx *ctx);
int fs_prof_count(fs_ctx *ctx, int *n);           /* number of distinct kernels seen (syncs)       */
int fs_prof_get(fs_ctx *ctx, int idx, char *name, int name_cap, int *launches, double *total_ms);
/* The __global__ functions launched under profile name `name` since fs_prof_enable, demangled ("fs::k_jacobi_ov2<4, 4>"), one per line in
 * `out` (may be null), their number in *n: what a rocprofv3 --kernel-trace of the same run lists.  bench.py names the kernels it prices
 * from here instead of from string literals. */
int fs_prof_kernels(fs_ctx *ctx, const char *name, char *out, int capacity, int *n);

#ifdef __cplusplus
}
#endif
#endif /* FS_HIP_H */
