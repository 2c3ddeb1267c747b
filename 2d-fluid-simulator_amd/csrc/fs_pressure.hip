// fs_pressure.hip - C-ABI entry points of the pressure kernels: Jacobi sweeps (single, lazily bounded pairs / quads / finishing pass), red-black
// SOR (half sweeps, one fused iteration, two iterations per pass), the Poisson source pair, the residual, the flow diagnostics and the
// per-step history ring, the body surface loads and the time averages.
#include "fs_launch.h"
#include "fs_stats.h"
#include "fs_mean.h"
#include "fs_loads.h"

static_assert(fs::STATS_N == FS_FLOW_NSTAT, "fs_stats.h and include/fs_hip.h disagree on the slots");
static_assert(fs::LOADS_REC == FS_LOADS_NREC && fs::LOADS_SUMS == FS_LOADS_NSUM, "fs_loads.h and include/fs_hip.h disagree on the record / the sums");
static_assert(fs::MEAN_PLANES == FS_MEAN_NPLANE, "fs_mean.h and include/fs_hip.h disagree on the planes");

namespace fs {
void history_release(fs_history *h)
{
    if (h->d_probes) hipFree(h->d_probes);
    if (h->d_faces) hipFree(h->d_faces);
    if (h->d_ring) hipFree(h->d_ring);
    if (h->d_state) hipFree(h->d_state);
    if (h->d_partial) hipFree(h->d_partial);
    delete h;
}
void loads_release(fs_loads *l)
{
    if (l->d_faces) hipFree(l->d_faces);
    if (l->d_sums) hipFree(l->d_sums);
    if (l->d_ring) hipFree(l->d_ring);
    if (l->d_state) hipFree(l->d_state);
    if (l->d_partial) hipFree(l->d_partial);
    delete l;
}
void mean_release(fs_mean *m)
{
    if (m->d_sums) hipFree(m->d_sums);
    if (m->d_state) hipFree(m->d_state);
    delete m;
}
}  // namespace fs

using namespace fs;

#define FS_PAIR(RT) FS_KLAUNCH((k_jacobi_pair<RT, SW, HV, T>), grid, dim3(256), 0, ctx->stream, og.g, og.nbx, og.nby, row_begin, row_end, \
                               (const uint8_t *)ctx->d_bcmap, (const uint8_t *)ctx->d_lazyflags, list, nlist, zoff, (T *)pn->d, (const T *)pc->d, (const T *)src->d)
template <bool SW, bool HV, typename T>
static void launch_pair(fs_ctx *ctx, const OvGrid &og, int rt, int row_begin, int row_end, fs_field *pn, const fs_field *pc, const fs_field *src)
{
    // the general rows ride in front: `zoff` leading z slices of the same launch, one wave per listed row
    const uint32_t *list = ctx->d_pairlist + (HV ? (size_t)ctx->nwx * ctx->rows : 0);
    const int nlist = ctx->n_pairlist[HV ? 1 : 0];
    const int per_slice = (int)(og.grid.x * og.grid.y), blocks = nlist, zoff = (blocks + per_slice - 1) / per_slice;      // one listed row per workgroup
    const dim3 grid(og.grid.x, og.grid.y, og.grid.z + zoff);
    if (rt == 2) FS_PAIR(2); else FS_PAIR(3);
}

template <bool SRC, typename T>
static int launch_jacobi(fs_ctx *ctx, const char *name, const Konst<T> &k, int jb, int je, T *pn, const T *pc, const T *vs)
{
    if constexpr (!SRC && std::is_same<T, float>::value) {
        // the literal f32 sweep on packed lanes of 2 cells, 4-row tiles, per-wave plain hints in the launch list (fs_jquad.h k_jacobi_ov2; round 5:
        // 74.5-75.6 against 81.6 us for the quad form below - 8-row tiles 86, 2-row tiles 84, without the hints 79-80)
        if (ctx->use_pairs) {
            const OvGrid og = ov_grid_lanes(ctx, jb, je, 4, 1, XCD_JACOBI, 3, true, 0, 1);      // (reach 1: the hints)
            const int dm = dm_const(ctx, k);
#define FS_JAC2(DM) FS_KLAUNCH((k_jacobi_ov2<4, DM>), og.grid, dim3(og.threads), 0, ctx->stream, og.g, k, og.nbx, og.nby, jb, je, pn, pc, vs)
            return launch(ctx, name, [=] { FS_DMC(dm, FS_JAC2); });
        }
    }
    // overlapped-wave register tiles of quads: the source-pair form streams best with 1-row tiles at 8 waves/SIMD (76 vs 79 us), the v-reading form (f64)
    // with 4-row tiles (round 4: 84.7 against 85.9-86.4 us; the tile heights 2 and 3 of rounds 2 - 4 went with their switch in round 6)
    constexpr int RT = SRC ? 1 : 4;
    const OvGrid og = ov_grid(ctx, jb, je, RT, 1, XCD_JACOBI);
    const int dm = SRC ? 0 : dm_const(ctx, k);           // the source-pair form divides nothing
#define FS_JAC(DM) FS_KLAUNCH((k_jacobi_ov<SRC, RT, DM, T>), og.grid, dim3(256), 0, ctx->stream, og.g, k, og.nbx, og.nby, jb, je, pn, pc, vs)
    return launch(ctx, name, [=] { FS_DMC(dm, FS_JAC); });
}

extern "C" {

int fs_jacobi_sweep(fs_ctx *ctx, double dt, double dx, fs_field *pn, const fs_field *pc, const fs_field *vc, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(vc, 2);
    FS_REQUIRE(pn != pc, "Jacobi needs two distinct pressure fields");
    FS_ROWS();
    FS_DISPATCH(ctx, {
        auto k = make_konst<T>(ctx, dt, dx, 1.0);
        // (odd res - X = 2 res not a multiple of 4: the f32 sweep on packed lanes of 2 cells needs an even width only, fs_jquad.h k_jacobi_ov2)
        if (ctx->use_march || (ctx->use_pairs && std::is_same<T, float>::value))
            return launch_jacobi<false, T>(ctx, "jacobi_sweep", k, row_begin, row_end, (T *)pn->d, (const T *)pc->d, (const T *)vc->d);
        FS_LAUNCH_CELLS("jacobi_sweep", (k_jacobi<false, T>), ctx->grid(), k, row_begin, (T *)pn->d, (const T *)pc->d, (const T *)vc->d)
    })
}

int fs_jacobi_sweep_src(fs_ctx *ctx, fs_field *pn, const fs_field *pc, const fs_field *src, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(src, 2);
    FS_REQUIRE(pn != pc, "Jacobi needs two distinct pressure fields");
    FS_ROWS();
    FS_DISPATCH(ctx, {
        auto k = make_konst<T>(ctx, 1.0, 1.0, 1.0);
        if (ctx->use_march) return launch_jacobi<true, T>(ctx, "jacobi_sweep_src", k, row_begin, row_end, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
        FS_LAUNCH_CELLS("jacobi_sweep_src", (k_jacobi<true, T>), ctx->grid(), k, row_begin, (T *)pn->d, (const T *)pc->d, (const T *)src->d)
    })
}

int fs_lazy_bc_ok(const fs_ctx *ctx, int *ok)
{
    FS_REQUIRE(ctx && ok, "null argument");
    *ok = ctx->mask_set && ctx->lazy_ok && ctx->use_march ? 1 : 0;
    return FS_OK;
}

// diagnostic: the per wave-tile-row flags of the lazy / two-sweep kernels (fs_march.h k_lazy_flags, k_pair_list), [wave column][local row]
int fs_lazy_flags(fs_ctx *ctx, uint8_t *out, int capacity, int *wave_columns, int *rows, int *general_rows)
{
    FS_REQUIRE(ctx && wave_columns && rows && general_rows, "null argument");
    FS_REQUIRE(ctx->mask_set && ctx->d_lazyflags, "no mask uploaded");
    *wave_columns = ctx->nwx; *rows = ctx->rows; general_rows[0] = ctx->n_pairlist[0]; general_rows[1] = ctx->n_pairlist[1];
    if (out) {
        FS_REQUIRE(capacity >= ctx->nwx * ctx->rows, "buffer too small");
        FS_HIP(hipMemcpyAsync(out, ctx->d_lazyflags, (size_t)ctx->nwx * ctx->rows, hipMemcpyDeviceToHost, ctx->stream));
        FS_HIP(hipStreamSynchronize(ctx->stream));
    }
    return FS_OK;
}

int fs_jacobi_sweep_lazy(fs_ctx *ctx, fs_field *pn, const fs_field *pc, const fs_field *src, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(src, 2);
    FS_REQUIRE(pn != pc, "Jacobi needs two distinct pressure fields");
    FS_ROWS();
    if (!(ctx->lazy_ok && ctx->use_march)) { set_error("this mask does not admit the lazy pressure boundary condition (fs_lazy_bc_ok)"); return FS_ERR_UNSUPPORTED; }
    const OvGrid og = ov_grid(ctx, row_begin, row_end, 1, 1, XCD_JACOBI);
    FS_DISPATCH(ctx, {
        return launch(ctx, "jacobi_sweep_lazy", [=] {
            FS_KLAUNCH((k_jacobi_lazy<T>), og.grid, dim3(256), 0, ctx->stream, og.g, og.nbx, og.nby, row_begin, row_end,
                               (const uint8_t *)ctx->d_bcmap, (const uint8_t *)ctx->d_lazyflags, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
        });
    })
}

// two lazily-bounded sweeps in one pass (fs_march.h k_jacobi_pair): pn <- sweep(sweep(pc)); pn's wall cells are read (the intermediate
// buffer of the two-buffer rotation is pn itself)
int fs_jacobi_pair_lazy(fs_ctx *ctx, fs_field *pn, const fs_field *pc, const fs_field *src, int mode, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(src, 2);
    FS_REQUIRE(pn != pc, "Jacobi needs two distinct pressure fields");
    FS_REQUIRE(mode >= 0 && mode <= 3, "mode: bit 0 = swapped buffers, bit 1 = vertical recipes in the tile path");
    FS_ROWS();
    if (!(ctx->lazy_ok && ctx->use_march)) { set_error("this mask does not admit the lazy pressure boundary condition (fs_lazy_bc_ok)"); return FS_ERR_UNSUPPORTED; }
    const int rt = (mode & 2) ? 2 : 3;      // rows per tile: 3 is within 2 % of the best of 2 / 3 / 4 from res 1024 to 4096 (the third tile path at 3 rows: 97 VGPRs, one wave per SIMD less)
    const OvGrid og = ov_grid(ctx, row_begin, row_end, rt, 1, XCD_JACOBI, false);      // (dense: its general rows ride in leading z slices)
    FS_DISPATCH(ctx, {
        return launch(ctx, "jacobi_pair_lazy", [=] {
            switch (mode) {
            case 0: launch_pair<false, false, T>(ctx, og, rt, row_begin, row_end, pn, pc, src); break;
            case 1: launch_pair<true, false, T>(ctx, og, rt, row_begin, row_end, pn, pc, src); break;
            case 2: launch_pair<false, true, T>(ctx, og, rt, row_begin, row_end, pn, pc, src); break;
            default: launch_pair<true, true, T>(ctx, og, rt, row_begin, row_end, pn, pc, src); break;
            }
        });
    })
}

static inline dim3 rb_grid(const fs_ctx *c, int jb, int je) { return dim3(((c->X + 1) / 2 + 255) / 256, je - jb, 1); }

int fs_rbsor_halfsweep(fs_ctx *ctx, double dt, double dx, double omega, int parity, fs_field *pn, const fs_field *pc,
                       const fs_field *vc, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_REQUIRE(parity == 0 || parity == 1, "parity must be 0 or 1");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(vc, 2);
    FS_ROWS();
    FS_DISPATCH(ctx, {
        auto k = make_konst<T>(ctx, dt, dx, 1.0, 0.0, omega);
        return launch(ctx, parity ? "rbsor_odd" : "rbsor_even", [=] {
            FS_KLAUNCH((k_rbsor<false, T>), rb_grid(ctx, row_begin, row_end), dim3(256), 0, ctx->stream, ctx->grid(), k,
                               row_begin, parity, (T *)pn->d, (const T *)pc->d, (const T *)vc->d);
        });
    })
}

int fs_rbsor_iteration(fs_ctx *ctx, double dt, double dx, double omega, fs_field *pn, const fs_field *pc, const fs_field *vc,
                       int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(vc, 2);
    FS_REQUIRE(pn != pc, "the fused iteration needs distinct p.next / p.current");
    FS_ROWS();
    if (!ctx->use_pairs) {
        int rc = fs_rbsor_halfsweep(ctx, dt, dx, omega, 1, pn, pc, vc, std::max(row_begin - 1, 0), std::min(row_end + 1, ctx->rows));
        if (rc) return rc;
        return fs_rbsor_halfsweep(ctx, dt, dx, omega, 0, pn, pn, vc, row_begin, row_end);
    }
    // lanes of 2 cells, 4-row tiles (fs_k34n.h k_rbsor_iter_n): 119 -> 115 us at bc5 res 4096 against the 3-row quad tiles it replaces, f64 (bc3 res
    // 4096) 318 -> 289; 2 / 6 rows: 129 / 115
    const OvGrid og = ov_grid_lanes(ctx, row_begin, row_end, 4, 1, XCD_RBSOR, 3, false);
    FS_DISPATCH(ctx, {
        auto k = make_konst<T>(ctx, dt, dx, 1.0, 0.0, omega);
#define FS_RBN4(DM) FS_KLAUNCH((k_rbsor_iter_n<2, 4, DM, T>), og.grid, dim3(256), 0, ctx->stream, og.g, k, og.nbx, og.nby, row_begin, row_end, \
                               (T *)pn->d, (const T *)pc->d, (const T *)vc->d)
        return launch(ctx, "rbsor_iteration", [=] { FS_DMC(dm_const(ctx, k), FS_RBN4); });
    })
}

// four lazily-bounded Jacobi sweeps in one pass (fs_jquad.h): pn[not wall] <- sweep^4(pc); both buffers hold raw sweep output
int fs_jacobi_quad_ok(const fs_ctx *ctx, int *ok)
{
    FS_REQUIRE(ctx && ok, "null argument");
    *ok = ctx->mask_set && ctx->jq_ok && ctx->use_march && ctx->dtype == 0 ? 1 : 0;
    return FS_OK;
}

int fs_jacobi_quad_lazy(fs_ctx *ctx, fs_field *pn, const fs_field *pc, const fs_field *src, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(src, 2);
    FS_REQUIRE(pn != pc, "Jacobi needs two distinct pressure fields");
    FS_ROWS();
    if (!(ctx->jq_ok && ctx->use_march && ctx->dtype == 0)) { set_error("this mask / precision does not admit the four-sweep Jacobi pass (fs_jacobi_quad_ok)"); return FS_ERR_UNSUPPORTED; }
    using T = float;
    // lanes of 2 cells (116 VGPRs = 4 waves per SIMD at 4 rows; quads: 182 = 2 waves, 44.9 against 34.3 us per pass at bc2 res 1600)
    constexpr int rt = 4;
#define FS_JQ(RT, PATH) FS_KLAUNCH((k_jacobi_quad<2, RT, PATH, T>), og.grid, dim3(og.threads), 0, ctx->stream, og.g, og.nbx, og.nby, row_begin, row_end, \
                               (const uint8_t *)ctx->d_bcmap, (T *)pn->d, (const T *)pc->d, (const T *)src->d)
    // ONE launch of one-wave workgroups whose list entry says which body the tile takes, masked tiles first (round 6; fs_launch.h ov_grid_lanes: the hinted
    // launches of the pressure families) - bc5 res 4096 122.5 -> 108.7 us per pass against rounds 4 - 5's two compact launches over the all-fluid and the other
    // workgroups (81.4 + 49.8; 137.5 dense), bc2 res 1600 30.2 -> 23.9 against the 4-wave workgroups with per-wave hints
    const OvGrid og = ov_grid_lanes(ctx, row_begin, row_end, rt, 1, XCD_RBSOR, 2, true, 0, 4);      // (reach 4: the hints)
    return launch(ctx, "jacobi_quad_lazy", [=] {
        FS_JQ(4, 2);
    });
}

// the last two rounds of a lazily-bounded Jacobi run in one pass (fs_jquad.h k_jacobi_finish): from pc = raw iterate n-2,
//   pc_out <- iterate n (not-wall cells) + K7(iterate n-2) (wall cells with a recipe);  pn <- iterate n-1 as K7 leaves it
int fs_jacobi_finish(fs_ctx *ctx, fs_field *pc_out, fs_field *pn, const fs_field *pc, const fs_field *src, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(pc_out, 1); FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(src, 2);
    FS_REQUIRE(pc_out != pc && pc_out != pn && pn != pc, "the finishing pass needs three distinct pressure fields");
    FS_ROWS();
    if (!(ctx->jq_ok && ctx->use_march && ctx->dtype == 0)) { set_error("this mask / precision does not admit the multi-sweep Jacobi passes (fs_jacobi_quad_ok)"); return FS_ERR_UNSUPPORTED; }
    using T = float;
    const OvGrid og = ov_grid_lanes(ctx, row_begin, row_end, 4, 1, XCD_RBSOR, 2, true, 0, 2);      // (per-wave plain hints: two sweeps reach 2 rows)
    return launch(ctx, "jacobi_finish", [=] {
        FS_KLAUNCH((k_jacobi_finish<2, 4, T>), og.grid, dim3(og.threads), 0, ctx->stream, og.g, og.nbx, og.nby, row_begin, row_end,
                           (const uint8_t *)ctx->d_bcmap, (T *)pc_out->d, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
    });
}

int fs_rbsor_pair_ok(const fs_ctx *ctx, int *ok)
{
    FS_REQUIRE(ctx && ok, "null argument");
    *ok = ctx->mask_set && ctx->rb_pair_ok && ctx->use_pairs ? 1 : 0;      // (f32 and, since round 4, f64)
    return FS_OK;
}

// two red-black iterations + both pressure boundary passes in one pass (fs_rbpair.h): (pc_out, pn_out) <- the state two iterations of
// fs/pressure_updater.py:86-96 leave in (p.current, p.next) when they start from (pc, pn)
int fs_rbsor_pair(fs_ctx *ctx, double dt, double dx, double omega, fs_field *pc_out, fs_field *pn_out, const fs_field *pc, const fs_field *pn,
                  const fs_field *vc, int full, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(pc_out, 1); FS_FIELD(pn_out, 1); FS_FIELD(pc, 1); FS_FIELD(pn, 1); FS_FIELD(vc, 2);
    FS_REQUIRE(pc_out != pn_out && pc_out != pc && pc_out != pn && pn_out != pc && pn_out != pn && pc != pn, "the two-iteration pass needs four distinct pressure fields");
    FS_ROWS();
    if (!(ctx->rb_pair_ok && ctx->use_pairs)) {
        set_error("this mask does not admit the two-iteration red-black pass (fs_rbsor_pair_ok)");
        return FS_ERR_UNSUPPORTED;
    }
    const Grid gg = ctx->grid();
    const int par0 = (gg.ybase + row_begin) & 1;
    if (ctx->dtype == 1) {
        // f64 (round 4; BASELINE configs[4]'s truth leg): the same body on double2 lanes.  A lane's window costs twice the registers, so the
        // tiles are 2 rows high (230 VGPRs with both paths = 2 waves per SIMD; the plain part on 4-row tiles: 220) - against 2 x (K7 + single
        // iteration) at 137 VGPRs that is still one pass over p and v instead of two.
        using T = double;
        auto k = make_konst<T>(ctx, dt, dx, 1.0, 0.0, omega);
#define FS_RBPD_K(RT, PAR, PATH, FULL) FS_KLAUNCH((k_rbsor_pair<2, RT, PAR, 0, PATH, FULL, T>), og.grid, dim3(og.threads), 0, ctx->stream, og.g, k, og.nbx, og.nby, row_begin, row_end, \
                               (const uint8_t *)ctx->d_bcmap, (T *)pc_out->d, (T *)pn_out->d, (const T *)pc->d, (const T *)pn->d, (const T *)vc->d)
#define FS_RBPD(RT, PATH, FULL) do { if (par0) FS_RBPD_K(RT, 1, PATH, FULL); else FS_RBPD_K(RT, 0, PATH, FULL); } while (0)
        if (!full && (ctx->rbpair_split == 2 || (ctx->rbpair_split == 1 && (size_t)ctx->X * ctx->Y >= ((size_t)1 << 23)))) {
            // (round 6: ONE launch of one-wave workgroups over both kinds of tile, as the f32 pass has it, loses here - 514-527 against 424 us at bc3 res 4096:
            //  the double2 bodies hold 220-256 VGPRs, and the masked one then sets the occupancy of the all-fluid tiles too)
            const OvGrid og = ov_grid_lanes(ctx, row_begin, row_end, 4, 1, XCD_RBSOR, 2, true, 1, 4, 1);
            const OvGrid ogb = ov_grid_lanes(ctx, row_begin, row_end, 2, 1, XCD_RBSOR, 2, true, 2, 4, 1, 4);
            if (og.g.tiles && ogb.g.tiles) {
                int rc = launch(ctx, "rbsor_pair", [=] { FS_RBPD(4, 3, false); });
                if (rc) return rc;
                { const OvGrid og = ogb; return launch(ctx, "rbsor_pair_bnd", [=] { FS_RBPD(2, 2, false); }); }
            }
        }
        const OvGrid og = ov_grid_lanes(ctx, row_begin, row_end, 2, 1, XCD_RBSOR, 2, !full, 0, 4);
        return launch(ctx, "rbsor_pair", [=] { if (full) FS_RBPD(2, 2, true); else FS_RBPD(2, 2, false); });
    }
    using T = float;
    auto k = make_konst<T>(ctx, dt, dx, 1.0, 0.0, omega);
    const int dm = dm_const(ctx, k);
    // lanes of 2 cells (8-byte loads: 126 - 156 VGPRs where quads need 223 - 248), RT = 4 rows per tile (6: 210-254 us, window registers).  The carrying
    // pass after an upload (full) is rare: one configuration.
    // (grids below 1 M cells: 2-row tiles - fewer waves than SIMDs there, the pass takes as long as ONE wave's chain of loads and stages:
    //  res 200 12.1 -> 9.2 us per launch, BASELINE configs[0] 53.3 -> 62.8 k steps/s; res 1600: 4 rows, 5602 against 5435 steps/s)
    const int rt = full || !small_tiles(ctx) ? 4 : 2;
#define FS_RBP_K(RT, PAR, DM, PATH, FULL) FS_KLAUNCH((k_rbsor_pair<2, RT, PAR, DM, PATH, FULL, T>), og.grid, dim3(og.threads), 0, ctx->stream, og.g, k, og.nbx, og.nby, row_begin, row_end, \
                               (const uint8_t *)ctx->d_bcmap, (T *)pc_out->d, (T *)pn_out->d, (const T *)pc->d, (const T *)pn->d, (const T *)vc->d)
#define FS_RBP_PAR(RT, DM, PATH, FULL) do { if (par0) FS_RBP_K(RT, 1, DM, PATH, FULL); else FS_RBP_K(RT, 0, DM, PATH, FULL); } while (0)
#define FS_RBP_DM(RT, PATH) do { if (dm & DM_F64) FS_RBP_PAR(RT, 4, PATH, false); else FS_RBP_PAR(RT, 0, PATH, false); } while (0)
    // Compact launch in two parts where the lists exist (single GPU, whole grid): the workgroups that see nothing but fluid within reach run
    // the plain path as its own kernel (PATH 3: no mask loads, 126 VGPRs = 4 waves per SIMD), the others the kernel with both paths.
    // Round 6: ONE launch over both kinds of tile (fs_rbpair.h k_rbsor_pair_all: all-fluid 16-row tiles as two stacked waves, the others as two 4-row
    // tiles with masks, boundary entries first) from 1 M cells - bc5 res 4096: 161 -> 139.5 us; bc2 res 1600 45.8 -> 36.4, res 1200 26.2 -> 20.2, res 1024
    // 23.0 -> 19.0, res 800 20.0 -> 16.7; res 512 14.5 -> 14.9 and res 400 12.6 -> 14.0 (the 2-row tiles of small grids stay there).  Round 5's two
    // launches over the two kinds of tile (k_rbsor_pair_stack, then the masked kernel: from 8 M cells) went with it.
    if (!full && (ctx->rbpair_split == 2 || (ctx->rbpair_split == 1 && (size_t)ctx->X * ctx->Y >= ((size_t)1 << 20)))) {
        const OvGrid og = ov_grid_lanes(ctx, row_begin, row_end, 8, 1, XCD_RBSOR, 2, true, 3, 4, 1, 16, ctx->halo != 0);
        if (og.g.tiles) {
#define FS_RBA_K(PAR, DM) FS_KLAUNCH((k_rbsor_pair_all<2, PAR, DM, T>), og.grid, dim3(128), 0, ctx->stream, og.g, k, og.nbx, og.nby, row_begin, row_end, \
                               (const uint8_t *)ctx->d_bcmap, (T *)pc_out->d, (T *)pn_out->d, (const T *)pc->d, (const T *)pn->d, (const T *)vc->d)
#define FS_RBA_PAR(DM) do { if (par0) FS_RBA_K(1, DM); else FS_RBA_K(0, DM); } while (0)
            return launch(ctx, "rbsor_pair", [=] { if (dm & DM_F64) FS_RBA_PAR(4); else FS_RBA_PAR(0); });
        }
    }
    // (one launch: the list's entries carry a per-wave "plain" hint - a wave that sees nothing but fluid within 4 rows skips its mask loads)
    const OvGrid og = ov_grid_lanes(ctx, row_begin, row_end, rt, 1, XCD_RBSOR, 2, !full, 0, 4);
    return launch(ctx, "rbsor_pair", [=] {
        if (full) FS_RBP_PAR(4, 0, 2, true);
        else if (rt == 2) FS_RBP_DM(2, 2);
        else FS_RBP_DM(4, 2);
    });
}

int fs_rbsor_halfsweep_src(fs_ctx *ctx, double omega, int parity, fs_field *pn, const fs_field *pc, const fs_field *src,
                           int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_REQUIRE(parity == 0 || parity == 1, "parity must be 0 or 1");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(src, 2);
    FS_ROWS();
    FS_DISPATCH(ctx, {
        auto k = make_konst<T>(ctx, 1.0, 1.0, 1.0, 0.0, omega);
        return launch(ctx, parity ? "rbsor_odd_src" : "rbsor_even_src", [=] {
            FS_KLAUNCH((k_rbsor<true, T>), rb_grid(ctx, row_begin, row_end), dim3(256), 0, ctx->stream, ctx->grid(), k,
                               row_begin, parity, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
        });
    })
}

int fs_poisson_source(fs_ctx *ctx, double dt, double dx, fs_field *src, const fs_field *vc, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(src, 2); FS_FIELD(vc, 2);
    FS_REQUIRE(src != vc, "src must not alias vc");
    FS_ROWS();
    FS_DISPATCH(ctx, {
        auto k = make_konst<T>(ctx, dt, dx, 1.0);
        if (ctx->use_pairs) {
            const OvGrid og = ov_grid_lanes(ctx, row_begin, row_end, 4, 1, XCD_JACOBI, 3);      // (deep-wall workgroups skipped: nobody reads the source there)
#define FS_PSN(DM) FS_KLAUNCH((k_poisson_source_n<2, 4, DM, T>), og.grid, dim3(og.threads), 0, ctx->stream, og.g, k, og.nbx, og.nby, row_begin, row_end, (T *)src->d, (const T *)vc->d)
            return launch(ctx, "poisson_source", [=] { FS_DMC(dm_const(ctx, k), FS_PSN); });
        }
        FS_LAUNCH_CELLS("poisson_source", (k_poisson_source<T>), ctx->grid(), k, row_begin, (T *)src->d, (const T *)vc->d)
    })
}

int fs_poisson_residual(fs_ctx *ctx, double dt, double dx, const fs_field *p, const fs_field *vc, double *sum_sq, double *count)
{
    FS_REQUIRE(ctx && sum_sq && count, "null argument");
    FS_FIELD(p, 1); FS_FIELD(vc, 2);
    FS_REQUIRE(!ctx->capturing && !ctx->tape_rec, "residual during graph capture / tape recording");
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    const int row_begin = ctx->halo, row_end = ctx->halo + ctx->nyl;
    const dim3 grid((ctx->X + 255) / 256, (row_end - row_begin + RES_ROWS - 1) / RES_ROWS);
    const size_t nblocks = (size_t)grid.x * grid.y;
    if (nblocks > ctx->partial_cap) {
        if (ctx->d_partial) { FS_HIP(hipStreamSynchronize(ctx->stream)); FS_HIP(hipFree(ctx->d_partial)); ctx->d_partial = nullptr; ctx->partial_cap = 0; }
        FS_HIP(hipMalloc(&ctx->d_partial, nblocks * 2 * sizeof(double)));
        ctx->partial_cap = nblocks;
    }
    int rc;
    FS_DISPATCH(ctx, {
        auto k = make_konst<T>(ctx, dt, dx, 1.0);
        rc = launch(ctx, "poisson_residual", [=] {
            FS_KLAUNCH((k_residual<T>), grid, dim3(256), 0, ctx->stream, ctx->grid(), k, row_begin, row_end,
                               (const T *)p->d, (const T *)vc->d, ctx->d_partial);
            FS_KLAUNCH((k_residual_final<double>), dim3(1), dim3(1024), 0, ctx->stream, (const double *)ctx->d_partial, (int)nblocks, ctx->d_acc);
        });
    })
    if (rc) return rc;
    double h[2];
    FS_HIP(hipMemcpyAsync(h, ctx->d_acc, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    *sum_sq = h[0];
    *count = h[1];
    return FS_OK;
}

// rows per workgroup of k_flow_stats: STATS_G on small grids, up to STATS_ROWS (fs_launch.h diag_rows)
static int stats_rows(const fs_ctx *ctx) { return diag_rows(ctx, (ctx->X + 255) / 256, ctx->nyl, STATS_G, STATS_ROWS); }

int fs_flow_stats(fs_ctx *ctx, double dx, const fs_field *v, const fs_field *p, const int *box, double *out)
{
    FS_REQUIRE(ctx && out, "null argument");
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    if (ctx->capturing || ctx->tape_rec) { set_error("flow stats during graph capture / tape recording"); return FS_ERR_STATE; }
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    int b[4] = {0, 0, 0, 0};      // empty box: no force
    if (box) {
        FS_REQUIRE(0 <= box[0] && box[0] <= box[2] && box[2] <= ctx->X && 0 <= box[1] && box[1] <= box[3] && box[3] <= ctx->Y,
                   "body box must satisfy 0 <= x0 <= x1 <= X and 0 <= y0 <= y1 <= Y");
        for (int k = 0; k < 4; ++k) b[k] = box[k];
    }
    const int row_begin = ctx->halo, row_end = ctx->halo + ctx->nyl;
    const int nx = (ctx->X + 255) / 256, ny = row_end - row_begin;
    const int rpw = stats_rows(ctx);
    const dim3 grid(nx, (ny + rpw - 1) / rpw);
    const size_t nblocks = (size_t)grid.x * grid.y;
    if (nblocks + 1 > ctx->stats_cap) {
        if (ctx->d_stats) { FS_HIP(hipStreamSynchronize(ctx->stream)); FS_HIP(hipFree(ctx->d_stats)); ctx->d_stats = nullptr; ctx->stats_cap = 0; }
        FS_HIP(hipMalloc(&ctx->d_stats, (nblocks + 1) * STATS_N * sizeof(double)));
        ctx->stats_cap = nblocks + 1;
    }
    double *partial = ctx->d_stats, *total = ctx->d_stats + nblocks * STATS_N;
    int rc;
    FS_DISPATCH(ctx, {
        rc = launch(ctx, "flow_stats", [=] {
            FS_KLAUNCH((k_flow_stats<T>), grid, dim3(256), 0, ctx->stream, ctx->grid(), row_begin, row_end, rpw, dx, b[0], b[1], b[2], b[3],
                       (const T *)v->d, (const T *)p->d, partial);
            FS_KLAUNCH((k_flow_stats_final), dim3(1), dim3(256), 0, ctx->stream, (const double *)partial, (int)nblocks, total);
        });
    })
    if (rc) return rc;
    FS_HIP(hipMemcpyAsync(out, total, STATS_N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_history_create(fs_ctx *ctx, int npoints, const int *points, int nfaces, const int *faces, int capacity, int every, fs_history **out)
{
    FS_REQUIRE(ctx && out, "null argument");
    FS_REQUIRE(npoints >= 0 && nfaces >= 0 && (points || npoints == 0) && (faces || nfaces == 0), "bad point / face list");
    FS_REQUIRE(capacity >= 1 && every >= 1, "capacity and every must be >= 1");
    FS_REQUIRE((2 + 3 * (long long)npoints) * capacity < (1LL << 40), "ring too large");
    if (ctx->capturing || ctx->tape_rec) { set_error("history create during graph capture / tape recording"); return FS_ERR_STATE; }
    // a probe / face outside the owned rows would read a ghost row (stale between exchanges) or count a face twice across slabs
    const int jo = ctx->y0, je = ctx->y0 + ctx->nyl;
    auto local = [&](int x, int y) -> long long { return (long long)(y - ctx->y0 + ctx->halo) * ctx->P + x; };      // row-major element of (x, y)
    std::vector<HistProbe> hp(npoints);
    for (int k = 0; k < npoints; ++k) {
        const int x = points[2 * k], y = points[2 * k + 1];
        FS_REQUIRE(0 <= x && x < ctx->X && jo <= y && y < je, "probe outside this context's owned rows");
        const int j = y - ctx->y0 + ctx->halo;
        hp[k].u = (unsigned)(((long long)j * 2 + 0) * ctx->P + x);      // fs_device.h idx<2>
        hp[k].w = (unsigned)(((long long)j * 2 + 1) * ctx->P + x);
        hp[k].p = (unsigned)local(x, y);
    }
    std::vector<HistFace> hf(nfaces);
    for (int k = 0; k < nfaces; ++k) {
        const int x = faces[3 * k], y = faces[3 * k + 1], d = faces[3 * k + 2];
        FS_REQUIRE(0 <= x && x < ctx->X && jo <= y && y < je, "face outside this context's owned rows");
        FS_REQUIRE(0 <= d && d <= 3, "face direction must be 0 (+x), 1 (-x), 2 (+y) or 3 (-y)");
        hf[k].p = (unsigned)local(x, y);
        hf[k].dir = d;
    }
    FS_HIP(hipSetDevice(ctx->device));
    fs_history *h = new fs_history();
    h->ctx = ctx; h->np = npoints; h->nf = nfaces; h->cap = capacity; h->every = every;
    h->nparts = nfaces > HIST_SPLIT ? (nfaces + HIST_FACES_PER_WG - 1) / HIST_FACES_PER_WG : 0;
    const size_t ring = (size_t)capacity * (2 + 3 * (size_t)npoints) * sizeof(double);
    hipError_t e = hipMalloc(&h->d_state, HIST_STATE * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(&h->d_ring, ring);
    if (e == hipSuccess && h->nparts) e = hipMalloc(&h->d_partial, 2 * (size_t)h->nparts * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&h->d_probes, std::max<size_t>(1, hp.size()) * sizeof(HistProbe));
    if (e == hipSuccess) e = hipMalloc(&h->d_faces, std::max<size_t>(1, hf.size()) * sizeof(HistFace));
    if (e == hipSuccess) e = hipMemsetAsync(h->d_state, 0, HIST_STATE * sizeof(long long), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_ring, 0, ring, ctx->stream);
    if (e == hipSuccess && npoints) e = hipMemcpyAsync(h->d_probes, hp.data(), hp.size() * sizeof(HistProbe), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && nfaces) e = hipMemcpyAsync(h->d_faces, hf.data(), hf.size() * sizeof(HistFace), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { history_release(h); return hip_fail(e, "fs_history_create", __FILE__, __LINE__); }
    ctx->histories.insert(h);
    *out = h;
    return FS_OK;
}

int fs_history_record(fs_ctx *ctx, fs_history *h, double dx, double limit, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && h, "null argument");
    FS_REQUIRE(h->ctx == ctx && ctx->histories.count(h), "history from another context or freed");
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    // everything the launch needs is in `h` and the fields: no allocation, copy or synchronisation here (the closure is captured / taped)
    const HistProbe *pr = h->d_probes;
    const HistFace *fc = h->d_faces;
    const int np = h->np, nf = h->nf, every = h->every, cap = h->cap, threads = h->threads, nparts = h->nparts;
    double *ring = h->d_ring, *partial = h->d_partial;
    long long *state = h->d_state;
    FS_DISPATCH(ctx, {
        return launch(ctx, "history_record", [=] {
            if (nparts)
                FS_KLAUNCH((k_history_faces<T>), dim3(nparts), dim3(HIST_FACES_PER_WG), 0, ctx->stream, (const T *)p->d, fc, nf, dx, every, cap,
                           (const long long *)state, partial);
            FS_KLAUNCH((k_history_record<T>), dim3(1), dim3(threads), 0, ctx->stream, (const T *)v->d, (const T *)p->d, pr, np, fc, nf,
                       (const double *)partial, nparts, dx, limit, every, cap, ring, state);
        });
    })
}

int fs_history_read(fs_ctx *ctx, fs_history *h, double *out, int max_records, int *n_records, long long *launches, int *dropped)
{
    FS_REQUIRE(ctx && h && n_records, "null argument");
    FS_REQUIRE(h->ctx == ctx && ctx->histories.count(h), "history from another context or freed");
    if (ctx->capturing || ctx->tape_rec) { set_error("history read during graph capture / tape recording"); return FS_ERR_STATE; }
    FS_HIP(hipSetDevice(ctx->device));
    long long st[HIST_STATE];
    FS_HIP(hipMemcpyAsync(st, h->d_state, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    *n_records = (int)st[1];
    if (launches) *launches = st[0];
    if (dropped) *dropped = (int)st[2];
    if (!out) return FS_OK;
    FS_REQUIRE(max_records >= st[1], "out holds fewer records than the ring");
    if (st[1] > 0)
        FS_HIP(hipMemcpyAsync(out, h->d_ring, (size_t)st[1] * (2 + 3 * (size_t)h->np) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipMemsetAsync(h->d_state + 1, 0, 2 * sizeof(long long), ctx->stream));       // written, dropped; the launch count runs on
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_history_free(fs_ctx *ctx, fs_history *h)
{
    if (!h) return FS_OK;
    FS_REQUIRE(ctx && h->ctx == ctx && ctx->histories.count(h), "history from another context or freed");
    ctx->histories.erase(h);
    if (ctx->capturing) { ctx->deferred_hist.push_back(h); return FS_OK; }      // (no synchronisation / hipFree inside a capture)
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    history_release(h);
    return FS_OK;
}

// ---- body surface loads (fs_loads.h) -----------------------------------------------------------------------------------------------------
#define FS_LOADS_HANDLE(l) FS_REQUIRE((l)->ctx == ctx && ctx->loads.count(l), "loads from another context or freed")
#define FS_LOADS_NO_CAPTURE(what) \
    if (ctx->capturing || ctx->tape_rec) { set_error("loads " what " during graph capture / tape recording"); return FS_ERR_STATE; }

int fs_loads_create(fs_ctx *ctx, int nfaces, const int *faces, const double *centre_xy, int capacity, long long every, long long start,
                    fs_loads **out)
{
    FS_REQUIRE(ctx && out && faces && centre_xy, "null argument");
    FS_REQUIRE(nfaces >= 1, "nfaces must be >= 1");
    FS_REQUIRE(capacity >= 1 && every >= 1 && start >= 0, "capacity and every must be >= 1 and start >= 0");
    FS_REQUIRE(std::isfinite(centre_xy[0]) && std::isfinite(centre_xy[1]), "the centre must be finite");
    FS_LOADS_NO_CAPTURE("create")
    // a face outside the owned rows would read a ghost row (stale between exchanges) or be counted twice across slabs
    const int jo = ctx->y0, je = ctx->y0 + ctx->nyl;
    const double cx = centre_xy[0], cy = centre_xy[1];
    std::vector<LoadFace> lf(nfaces);
    for (int k = 0; k < nfaces; ++k) {
        const int x = faces[3 * k], y = faces[3 * k + 1], d = faces[3 * k + 2];
        FS_REQUIRE(0 <= x && x < ctx->X && jo <= y && y < je, "face outside this context's owned rows");
        FS_REQUIRE(0 <= d && d <= 3, "face direction must be 0 (+x), 1 (-x), 2 (+y) or 3 (-y)");
        const long long j = y - ctx->y0 + ctx->halo;
        lf[k].u = (unsigned)((j * 2 + 0) * ctx->P + x);      // fs_device.h idx<2>
        lf[k].w = (unsigned)((j * 2 + 1) * ctx->P + x);
        lf[k].p = (unsigned)(j * ctx->P + x);
        lf[k].dir = d;
        const double xm = d == 0 ? (double)x : d == 1 ? (double)x + 1.0 : (double)x + 0.5;      // the face midpoint, cell units
        const double ym = d == 2 ? (double)y : d == 3 ? (double)y + 1.0 : (double)y + 0.5;
        lf[k].rx = xm - cx;
        lf[k].ry = ym - cy;
    }
    FS_HIP(hipSetDevice(ctx->device));
    fs_loads *l = new fs_loads();
    l->ctx = ctx; l->nf = nfaces; l->cap = capacity; l->every = every; l->start = start;
    l->nparts = nfaces > LOADS_SPLIT ? (nfaces + LOADS_WG - 1) / LOADS_WG : 0;
    const size_t ring = (size_t)capacity * LOADS_REC * sizeof(double), sums = (size_t)LOADS_SUMS * nfaces * sizeof(double);
    hipError_t e = hipMalloc(&l->d_state, LOADS_STATE * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(&l->d_ring, ring);
    if (e == hipSuccess) e = hipMalloc(&l->d_sums, sums);
    if (e == hipSuccess && l->nparts) e = hipMalloc(&l->d_partial, (size_t)LOADS_REC * l->nparts * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&l->d_faces, lf.size() * sizeof(LoadFace));
    if (e == hipSuccess) e = hipMemsetAsync(l->d_state, 0, LOADS_STATE * sizeof(long long), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(l->d_ring, 0, ring, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(l->d_sums, 0, sums, ctx->stream);
    if (e == hipSuccess && l->nparts) e = hipMemsetAsync(l->d_partial, 0, (size_t)LOADS_REC * l->nparts * sizeof(double), ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(l->d_faces, lf.data(), lf.size() * sizeof(LoadFace), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { loads_release(l); return hip_fail(e, "fs_loads_create", __FILE__, __LINE__); }
    ctx->loads.insert(l);
    *out = l;
    return FS_OK;
}

int fs_loads_record(fs_ctx *ctx, fs_loads *l, double dx, double inv_re, double limit, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && l, "null argument");
    FS_LOADS_HANDLE(l);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    // everything the launches need is in `l` and the fields: no allocation, copy or synchronisation here (the closure is captured / taped)
    const LoadFace *fc = l->d_faces;
    const int nf = l->nf, cap = l->cap, nparts = l->nparts;
    const size_t stride = (size_t)l->nf;
    const long long every = l->every, start = l->start;
    double *sums = l->d_sums, *ring = l->d_ring, *partial = l->d_partial;
    long long *state = l->d_state;
    FS_DISPATCH(ctx, {
        return launch(ctx, "loads_record", [=] {
            if (nparts) {
                FS_KLAUNCH((k_loads_faces<T>), dim3(nparts), dim3(LOADS_WG), 0, ctx->stream, (const T *)v->d, (const T *)p->d, fc, nf, stride, dx,
                           inv_re, limit, start, every, (const long long *)state, sums, partial);
                FS_KLAUNCH((k_loads_record), dim3(1), dim3(LOADS_WG), 0, ctx->stream, (const double *)partial, nparts, start, every, cap, ring, state);
            } else {
                FS_KLAUNCH((k_loads_one<T>), dim3(1), dim3(LOADS_WG), 0, ctx->stream, (const T *)v->d, (const T *)p->d, fc, nf, stride, dx, inv_re,
                           limit, start, every, cap, sums, ring, state);
            }
        });
    })
}

int fs_loads_read(fs_ctx *ctx, fs_loads *l, double *ring_out, int max_records, int *n_records, long long *launches, long long *samples,
                  int *dropped)
{
    FS_REQUIRE(ctx && l && n_records, "null argument");
    FS_LOADS_HANDLE(l);
    FS_LOADS_NO_CAPTURE("read")
    FS_HIP(hipSetDevice(ctx->device));
    long long st[LOADS_STATE];
    FS_HIP(hipMemcpyAsync(st, l->d_state, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    *n_records = (int)st[2];
    if (launches) *launches = st[0];
    if (samples) *samples = st[1];
    if (dropped) *dropped = (int)st[3];
    if (!ring_out) return FS_OK;
    FS_REQUIRE(max_records >= st[2], "ring_out holds fewer records than the ring");
    if (st[2] > 0)
        FS_HIP(hipMemcpyAsync(ring_out, l->d_ring, (size_t)st[2] * LOADS_REC * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipMemsetAsync(l->d_state + 2, 0, 2 * sizeof(long long), ctx->stream));       // written, dropped; launches and samples run on
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_loads_sums_read(fs_ctx *ctx, fs_loads *l, double *sums_out)
{
    FS_REQUIRE(ctx && l && sums_out, "null argument");
    FS_LOADS_HANDLE(l);
    FS_LOADS_NO_CAPTURE("sums_read")
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemcpyAsync(sums_out, l->d_sums, (size_t)LOADS_SUMS * l->nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_loads_sums_write(fs_ctx *ctx, fs_loads *l, const double *sums_in, long long launches, long long samples)
{
    FS_REQUIRE(ctx && l && sums_in, "null argument");
    FS_LOADS_HANDLE(l);
    FS_REQUIRE(launches >= 0 && samples >= 0 && samples <= launches, "counters must satisfy 0 <= samples <= launches");
    FS_LOADS_NO_CAPTURE("sums_write")
    FS_HIP(hipSetDevice(ctx->device));
    const long long st[2] = {launches, samples};
    FS_HIP(hipMemcpyAsync(l->d_sums, sums_in, (size_t)LOADS_SUMS * l->nf * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipMemcpyAsync(l->d_state, st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));      // (both sources are the caller's / this frame's memory)
    return FS_OK;
}

int fs_loads_reset(fs_ctx *ctx, fs_loads *l)
{
    FS_REQUIRE(ctx && l, "null argument");
    FS_LOADS_HANDLE(l);
    FS_LOADS_NO_CAPTURE("reset")
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemsetAsync(l->d_sums, 0, (size_t)LOADS_SUMS * l->nf * sizeof(double), ctx->stream));
    FS_HIP(hipMemsetAsync(l->d_state + 1, 0, sizeof(long long), ctx->stream));      // samples; the launch count runs on
    return FS_OK;
}

int fs_loads_free(fs_ctx *ctx, fs_loads *l)
{
    if (!l) return FS_OK;
    FS_REQUIRE(ctx && l->ctx == ctx && ctx->loads.count(l), "loads from another context or freed");
    ctx->loads.erase(l);
    if (ctx->capturing) { ctx->deferred_loads.push_back(l); return FS_OK; }      // (no synchronisation / hipFree inside a capture)
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    loads_release(l);
    return FS_OK;
}

// ---- time averages (fs_mean.h) ---------------------------------------------------------------------------------------------------------
#define FS_MEAN_HANDLE(m) FS_REQUIRE((m)->ctx == ctx && ctx->means.count(m), "mean from another context or freed")
#define FS_MEAN_NO_CAPTURE(what) \
    if (ctx->capturing || ctx->tape_rec) { set_error("mean " what " during graph capture / tape recording"); return FS_ERR_STATE; }

// workgroups of 256 lanes x `w` columns and `rpw` rows over the owned rows: rows per workgroup from `g0` up to MEAN_ROWS (fs_launch.h
// diag_rows) - a non-sampling launch is a counter read per workgroup, so the grid stays in the thousands
static int mean_width(const fs_ctx *ctx) { return ctx->X % 2 == 0 ? 2 : 1; }      // columns per lane: W of k_mean_accumulate / k_mean_finalize
static dim3 mean_grid(const fs_ctx *ctx, int w, int g0, int *rpw)
{
    const int nx = (ctx->X + 256 * w - 1) / (256 * w), ny = ctx->nyl;
    const int r = diag_rows(ctx, nx, ny, g0, MEAN_ROWS);
    *rpw = r;
    return dim3(nx, (ny + r - 1) / r);
}

// diagnostic: the rows per workgroup the next fs_flow_stats / fs_mean_accumulate / fs_mean_finalize launches of this context take
int fs_diag_rows(fs_ctx *ctx, int *flow_stats_rows, int *mean_accumulate_rows, int *mean_finalize_rows)
{
    FS_REQUIRE(ctx && flow_stats_rows && mean_accumulate_rows && mean_finalize_rows, "null argument");
    *flow_stats_rows = stats_rows(ctx);
    mean_grid(ctx, mean_width(ctx), MEAN_G, mean_accumulate_rows);
    mean_grid(ctx, mean_width(ctx), 1, mean_finalize_rows);
    return FS_OK;
}

int fs_mean_create(fs_ctx *ctx, long long every, long long start, fs_mean **out)
{
    FS_REQUIRE(ctx && out, "null argument");
    FS_REQUIRE(every >= 1 && start >= 0, "every must be >= 1 and start >= 0");
    FS_MEAN_NO_CAPTURE("create")
    FS_HIP(hipSetDevice(ctx->device));
    fs_mean *m = new fs_mean();
    m->ctx = ctx; m->every = every; m->start = start;
    m->plane = (size_t)ctx->nyl * ctx->P + MEAN_PAD;
    const size_t bytes = MEAN_PLANES * m->plane * sizeof(double);
    hipError_t e = hipMalloc(&m->d_state, MEAN_STATE * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc(&m->d_sums, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(m->d_state, 0, MEAN_STATE * sizeof(long long), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->d_sums, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { mean_release(m); return hip_fail(e, "fs_mean_create", __FILE__, __LINE__); }
    ctx->means.insert(m);
    *out = m;
    return FS_OK;
}

int fs_mean_accumulate(fs_ctx *ctx, fs_mean *m, double limit, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_MEAN_HANDLE(m);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launches need is in `m` and the fields: no allocation, copy or synchronisation here (the closure is captured / taped)
    const int jb = ctx->halo, je = ctx->halo + ctx->nyl, w = mean_width(ctx);
    int rpw;
    const dim3 grid = mean_grid(ctx, w, MEAN_G, &rpw);
    const long long every = m->every, start = m->start;
    long long *state = m->d_state;
    double *sums = m->d_sums;
    const size_t plane = m->plane;
    FS_DISPATCH(ctx, {
        return launch(ctx, "mean_accumulate", [=] {
            if (w == 2)
                FS_KLAUNCH((k_mean_accumulate<T, 2>), grid, dim3(256), 0, ctx->stream, ctx->grid(), jb, je, rpw, limit, start, every,
                           (const long long *)state, (const T *)v->d, (const T *)p->d, sums, plane);
            else
                FS_KLAUNCH((k_mean_accumulate<T, 1>), grid, dim3(256), 0, ctx->stream, ctx->grid(), jb, je, rpw, limit, start, every,
                           (const long long *)state, (const T *)v->d, (const T *)p->d, sums, plane);
            FS_KLAUNCH((k_mean_tick), dim3(1), dim3(64), 0, ctx->stream, start, every, state);
        });
    })
}

static int mean_counters(fs_ctx *ctx, fs_mean *m, long long *st)
{
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemcpyAsync(st, m->d_state, MEAN_STATE * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_mean_finalize(fs_ctx *ctx, fs_mean *m, fs_field *v_out, fs_field *p_out)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_MEAN_HANDLE(m);
    FS_FIELD(v_out, 2); FS_FIELD(p_out, 1);
    FS_MEAN_NO_CAPTURE("finalize")
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    long long st[MEAN_STATE];
    if (int rc = mean_counters(ctx, m, st)) return rc;
    if (st[1] < 1) { set_error("mean finalize: no sample accumulated yet"); return FS_ERR_STATE; }
    const int jb = ctx->halo, je = ctx->halo + ctx->nyl, w = mean_width(ctx);
    int rpw;
    const dim3 grid = mean_grid(ctx, w, 1, &rpw);
    const long long *state = m->d_state;
    const double *sums = m->d_sums;
    const size_t plane = m->plane;
    FS_DISPATCH(ctx, {
        return launch(ctx, "mean_finalize", [=] {
            if (w == 2)
                FS_KLAUNCH((k_mean_finalize<T, 2>), grid, dim3(256), 0, ctx->stream, ctx->grid(), jb, je, rpw, state, sums, plane, (T *)v_out->d,
                           (T *)p_out->d, v_out->hot);
            else
                FS_KLAUNCH((k_mean_finalize<T, 1>), grid, dim3(256), 0, ctx->stream, ctx->grid(), jb, je, rpw, state, sums, plane, (T *)v_out->d,
                           (T *)p_out->d, v_out->hot);
        });
    })
}

int fs_mean_read(fs_ctx *ctx, fs_mean *m, double *sums_out, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_MEAN_HANDLE(m);
    FS_MEAN_NO_CAPTURE("read")
    long long st[MEAN_STATE];
    if (int rc = mean_counters(ctx, m, st)) return rc;
    if (launches) *launches = st[0];
    if (samples) *samples = st[1];
    if (!sums_out) return FS_OK;
    // per plane: nyl device rows of pitch P -> dense rows of X
    for (int k = 0; k < MEAN_PLANES; ++k)
        FS_HIP(hipMemcpy2DAsync(sums_out + (size_t)k * ctx->nyl * ctx->X, (size_t)ctx->X * sizeof(double), m->d_sums + k * m->plane,
                                (size_t)ctx->P * sizeof(double), (size_t)ctx->X * sizeof(double), (size_t)ctx->nyl, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_mean_write(fs_ctx *ctx, fs_mean *m, const double *sums_in, long long launches, long long samples)
{
    FS_REQUIRE(ctx && m && sums_in, "null argument");
    FS_MEAN_HANDLE(m);
    FS_REQUIRE(launches >= 0 && samples >= 0 && samples <= launches, "counters must satisfy 0 <= samples <= launches");
    FS_MEAN_NO_CAPTURE("write")
    FS_HIP(hipSetDevice(ctx->device));
    const long long st[MEAN_STATE] = {launches, samples};
    for (int k = 0; k < MEAN_PLANES; ++k)
        FS_HIP(hipMemcpy2DAsync(m->d_sums + k * m->plane, (size_t)ctx->P * sizeof(double), sums_in + (size_t)k * ctx->nyl * ctx->X,
                                (size_t)ctx->X * sizeof(double), (size_t)ctx->X * sizeof(double), (size_t)ctx->nyl, hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipMemcpyAsync(m->d_state, st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));      // (both sources are the caller's / this frame's memory)
    return FS_OK;
}

int fs_mean_reset(fs_ctx *ctx, fs_mean *m)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_MEAN_HANDLE(m);
    FS_MEAN_NO_CAPTURE("reset")
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemsetAsync(m->d_sums, 0, MEAN_PLANES * m->plane * sizeof(double), ctx->stream));
    FS_HIP(hipMemsetAsync(m->d_state + 1, 0, sizeof(long long), ctx->stream));      // samples; the launch count runs on
    return FS_OK;
}

int fs_mean_free(fs_ctx *ctx, fs_mean *m)
{
    if (!m) return FS_OK;
    FS_REQUIRE(ctx && m->ctx == ctx && ctx->means.count(m), "mean from another context or freed");
    ctx->means.erase(m);
    if (ctx->capturing) { ctx->deferred_mean.push_back(m); return FS_OK; }      // (no synchronisation / hipFree inside a capture)
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    mean_release(m);
    return FS_OK;
}

}  // extern "C"
