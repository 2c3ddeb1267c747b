// fs_pressure.hip - C-ABI entry points of the pressure kernels: Jacobi sweeps (single, lazily bounded pairs / quads / finishing pass), red-black
// SOR (half sweeps, one fused iteration, two iterations per pass), the Poisson source pair and the residual.
#include "fs_launch.h"

using namespace fs;

template <bool SW, bool HV, typename T>
static bool launch_pair(fs_ctx *ctx, const OvGrid &og, int rt, int row_begin, int row_end, fs_field *pn, const fs_field *pc, const fs_field *src)
{
    // the general rows ride in front: `zoff` leading z slices of the same launch, one wave per listed row
    const uint32_t *list = ctx->d_pairlist + (HV ? (size_t)ctx->nwx * ctx->rows : 0);
    const int nlist = ctx->n_pairlist[HV ? 1 : 0];
    const int per_slice = (int)(og.grid.x * og.grid.y), blocks = nlist, zoff = (blocks + per_slice - 1) / per_slice;      // one listed row per workgroup
    const dim3 grid(og.grid.x, og.grid.y, og.grid.z + zoff);
    return pick<2, 3>(rt, [&](auto RT) {
        klaunch(k_jacobi_pair<RT, SW, HV, T>, grid, dim3(256), ctx->stream, og.g, og.nbx, og.nby, row_begin, row_end, (const uint8_t *)ctx->d_bcmap,
                (const uint8_t *)ctx->d_lazyflags, list, nlist, zoff, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
    });
}

template <bool SRC, typename T>
static int launch_jacobi(fs_ctx *ctx, const char *name, const Konst<T> &k, int jb, int je, T *pn, const T *pc, const T *vs)
{
    if constexpr (!SRC && std::is_same<T, float>::value) {
        // the literal f32 sweep on packed lanes of 2 cells, 4-row tiles, per-wave plain hints in the launch list (fs_jquad.h k_jacobi_ov2; round 5:
        // 74.5-75.6 against 81.6 us for the quad form below - 8-row tiles 86, 2-row tiles 84, without the hints 79-80)
        if (ctx->use_pairs) {
            const OvGrid og = ov_grid(ctx, jb, je, tiles(XCD_JACOBI, LANES_PAIR_WIDE).rows(4).hints_within(1));
            const int dm = dm_const(ctx, k);
            return launch(ctx, name, [=] { return with_dm_const<T>(dm, [&](auto DM) { klaunch(k_jacobi_ov2<4, DM>, og, ctx->stream, k, jb, je, pn, pc, vs); }); });
        }
    }
    // overlapped-wave register tiles of quads: the source-pair form streams best with 1-row tiles at 8 waves/SIMD (76 vs 79 us), the v-reading form (f64)
    // with 4-row tiles (round 4: 84.7 against 85.9-86.4 us; the tile heights 2 and 3 of rounds 2 - 4 went with their switch in round 6)
    constexpr int RT = SRC ? 1 : 4;
    const OvGrid og = ov_grid(ctx, jb, je, tiles(XCD_JACOBI, LANES_QUAD).rows(RT));
    const int dm = SRC ? 0 : dm_const(ctx, k);           // the source-pair form divides nothing
    return launch(ctx, name, [=] { return with_dm_const<T>(dm, [&](auto DM) { klaunch(k_jacobi_ov<SRC, RT, DM, T>, og, ctx->stream, k, jb, je, pn, pc, vs); }); });
}

extern "C" {

int fs_jacobi_sweep(fs_ctx *ctx, double dt, double dx, fs_field *pn, const fs_field *pc, const fs_field *vc, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(vc, 2);
    FS_REQUIRE(pn != pc, "Jacobi needs two distinct pressure fields");
    FS_ROWS();
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        auto k = make_konst<T>(ctx, dt, dx, 1.0);
        // (odd res - X = 2 res not a multiple of 4: the f32 sweep on packed lanes of 2 cells needs an even width only, fs_jquad.h k_jacobi_ov2)
        if (ctx->use_march || (ctx->use_pairs && std::is_same<T, float>::value))
            return launch_jacobi<false, T>(ctx, "jacobi_sweep", k, row_begin, row_end, (T *)pn->d, (const T *)pc->d, (const T *)vc->d);
        return launch_cells(ctx, "jacobi_sweep", k_jacobi<false, T>, row_begin, row_end, k, (T *)pn->d, (const T *)pc->d, (const T *)vc->d);
    });
}

int fs_jacobi_sweep_src(fs_ctx *ctx, fs_field *pn, const fs_field *pc, const fs_field *src, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(src, 2);
    FS_REQUIRE(pn != pc, "Jacobi needs two distinct pressure fields");
    FS_ROWS();
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        auto k = make_konst<T>(ctx, 1.0, 1.0, 1.0);
        if (ctx->use_march) return launch_jacobi<true, T>(ctx, "jacobi_sweep_src", k, row_begin, row_end, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
        return launch_cells(ctx, "jacobi_sweep_src", k_jacobi<true, T>, row_begin, row_end, k, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
    });
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
    const OvGrid og = ov_grid(ctx, row_begin, row_end, tiles(XCD_JACOBI, LANES_QUAD).rows(1));
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "jacobi_sweep_lazy", [=] {
            klaunch(k_jacobi_lazy<T>, og, ctx->stream, row_begin, row_end, (const uint8_t *)ctx->d_bcmap, (const uint8_t *)ctx->d_lazyflags, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
        });
    });
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
    const OvGrid og = ov_grid(ctx, row_begin, row_end, tiles(XCD_JACOBI, LANES_QUAD).rows(rt).dense_if(true));      // (dense: its general rows ride in leading z slices)
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "jacobi_pair_lazy", [=] {
            return pick_bool((mode & 1) != 0, [&](auto SW) { return pick_bool((mode & 2) != 0, [&](auto HV) {
                return launch_pair<SW, HV, T>(ctx, og, rt, row_begin, row_end, pn, pc, src);
            }); });
        });
    });
}

static inline dim3 rb_grid(const fs_ctx *c, int jb, int je) { return dim3(((c->X + 1) / 2 + 255) / 256, je - jb, 1); }

int fs_rbsor_halfsweep(fs_ctx *ctx, double dt, double dx, double omega, int parity, fs_field *pn, const fs_field *pc,
                       const fs_field *vc, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_REQUIRE(parity == 0 || parity == 1, "parity must be 0 or 1");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(vc, 2);
    FS_ROWS();
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        auto k = make_konst<T>(ctx, dt, dx, 1.0, 0.0, omega);
        return launch(ctx, parity ? "rbsor_odd" : "rbsor_even", [=] {
            klaunch(k_rbsor<false, T>, rb_grid(ctx, row_begin, row_end), dim3(256), ctx->stream, ctx->grid(), k,
                               row_begin, parity, (T *)pn->d, (const T *)pc->d, (const T *)vc->d);
        });
    });
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
    const OvGrid og = ov_grid(ctx, row_begin, row_end, tiles(XCD_RBSOR, LANES_PAIR_WIDE).rows(4).dense_if(true));
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        auto k = make_konst<T>(ctx, dt, dx, 1.0, 0.0, omega);
        const int dm = dm_const(ctx, k);
        return launch(ctx, "rbsor_iteration", [=] {
            return with_dm_const<T>(dm, [&](auto DM) { klaunch(k_rbsor_iter_n<2, 4, DM, T>, og, ctx->stream, k, row_begin, row_end, (T *)pn->d, (const T *)pc->d, (const T *)vc->d); });
        });
    });
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
    // ONE launch of one-wave workgroups whose list entry says which body the tile takes, masked tiles first (round 6; fs_launch.h one_wave_where_hinted: the hinted
    // launches of the pressure families) - bc5 res 4096 122.5 -> 108.7 us per pass against rounds 4 - 5's two compact launches over the all-fluid and the other
    // workgroups (81.4 + 49.8; 137.5 dense), bc2 res 1600 30.2 -> 23.9 against the 4-wave workgroups with per-wave hints
    const OvGrid og = ov_grid(ctx, row_begin, row_end, tiles(XCD_RBSOR, LANES_PAIR).rows(rt).hints_within(4));
    return launch(ctx, "jacobi_quad_lazy", [=] {
        klaunch(k_jacobi_quad<2, rt, 2, T>, og, ctx->stream, row_begin, row_end, (const uint8_t *)ctx->d_bcmap, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
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
    const OvGrid og = ov_grid(ctx, row_begin, row_end, tiles(XCD_RBSOR, LANES_PAIR).rows(4).hints_within(2));      // (two sweeps reach 2 rows)
    return launch(ctx, "jacobi_finish", [=] {
        klaunch(k_jacobi_finish<2, 4, T>, og, ctx->stream, row_begin, row_end, (const uint8_t *)ctx->d_bcmap, (T *)pc_out->d, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
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
        // k_rbsor_pair<2, RT, parity of the first row, 0, PATH, FULL, double> over the tiles of `og`
        auto run = [=](const OvGrid &og, auto RT, auto PATH, auto FULL) {
            constexpr int rt = decltype(RT)::value, path = decltype(PATH)::value;
            constexpr bool carry = decltype(FULL)::value;
            return pick<0, 1>(par0, [&](auto PAR) {
                klaunch(k_rbsor_pair<2, rt, PAR, 0, path, carry, T>, og, ctx->stream, k, row_begin, row_end, (const uint8_t *)ctx->d_bcmap, (T *)pc_out->d, (T *)pn_out->d,
                        (const T *)pc->d, (const T *)pn->d, (const T *)vc->d);
            });
        };
        if (!full && split_launch(ctx, (size_t)ctx->X * ctx->Y, (size_t)1 << 23)) {
            // (round 6: ONE launch of one-wave workgroups over both kinds of tile, as the f32 pass has it, loses here - 514-527 against 424 us at bc3 res 4096:
            //  the double2 bodies hold 220-256 VGPRs, and the masked one then sets the occupancy of the all-fluid tiles too)
            const OvGrid ogp = ov_grid(ctx, row_begin, row_end, tiles(XCD_RBSOR, LANES_PAIR).rows(4).waves(1).plain_within(4));
            const OvGrid ogb = ov_grid(ctx, row_begin, row_end, tiles(XCD_RBSOR, LANES_PAIR).rows(2).waves(1).boundary_within(4).parent_rows(4));
            if (ogp.g.tiles && ogb.g.tiles) {
                int rc = launch(ctx, "rbsor_pair", [=] { return run(ogp, Int<4>{}, Int<3>{}, Bool<false>{}); });
                if (rc) return rc;
                return launch(ctx, "rbsor_pair_bnd", [=] { return run(ogb, Int<2>{}, Int<2>{}, Bool<false>{}); });
            }
        }
        const OvGrid og = ov_grid(ctx, row_begin, row_end, tiles(XCD_RBSOR, LANES_PAIR).rows(2).dense_if(full).hints_within(4));
        return launch(ctx, "rbsor_pair", [=] { return pick_bool(full != 0, [&](auto FULL) { return run(og, Int<2>{}, Int<2>{}, FULL); }); });
    }
    using T = float;
    auto k = make_konst<T>(ctx, dt, dx, 1.0, 0.0, omega);
    const int dm = dm_const(ctx, k);
    // lanes of 2 cells (8-byte loads: 126 - 156 VGPRs where quads need 223 - 248), RT = 4 rows per tile (6: 210-254 us, window registers).  The carrying
    // pass after an upload (full) is rare: one configuration.
    // (grids below 1 M cells: 2-row tiles - fewer waves than SIMDs there, the pass takes as long as ONE wave's chain of loads and stages:
    //  res 200 12.1 -> 9.2 us per launch, BASELINE configs[0] 53.3 -> 62.8 k steps/s; res 1600: 4 rows, 5602 against 5435 steps/s)
    const int rt = full || !small_tiles(ctx) ? 4 : 2;
    // Compact launch in two parts where the lists exist (single GPU, whole grid): the workgroups that see nothing but fluid within reach run
    // the plain path as its own kernel (PATH 3: no mask loads, 126 VGPRs = 4 waves per SIMD), the others the kernel with both paths.
    // Round 6: ONE launch over both kinds of tile (fs_rbpair.h k_rbsor_pair_all: all-fluid 16-row tiles as two stacked waves, the others as two 4-row
    // tiles with masks, boundary entries first) from 1 M cells - bc5 res 4096: 161 -> 139.5 us; bc2 res 1600 45.8 -> 36.4, res 1200 26.2 -> 20.2, res 1024
    // 23.0 -> 19.0, res 800 20.0 -> 16.7; res 512 14.5 -> 14.9 and res 400 12.6 -> 14.0 (the 2-row tiles of small grids stay there).  Round 5's two
    // launches over the two kinds of tile (k_rbsor_pair_stack, then the masked kernel: from 8 M cells) went with it.
    if (!full && split_launch(ctx, (size_t)ctx->X * ctx->Y, (size_t)1 << 20)) {
        const OvGrid og = ov_grid(ctx, row_begin, row_end, tiles(XCD_RBSOR, LANES_PAIR).rows(8).waves(1).mixed_within(4).parent_rows(16).classes_on_slabs(ctx->halo != 0));
        if (og.g.tiles) {
            return launch(ctx, "rbsor_pair", [=] {      // (a list entry: a tile of two component waves, 128 threads)
                return pick<0, 1>(par0, [&](auto PAR) { return with_dm_const<T>(dm, [&](auto DM) {
                    klaunch(k_rbsor_pair_all<2, PAR, DM, T>, og.with_threads(128), ctx->stream, k, row_begin, row_end, (const uint8_t *)ctx->d_bcmap, (T *)pc_out->d, (T *)pn_out->d,
                            (const T *)pc->d, (const T *)pn->d, (const T *)vc->d);
                }); });
            });
        }
    }
    // (one launch: the list's entries carry a per-wave "plain" hint - a wave that sees nothing but fluid within 4 rows skips its mask loads)
    const OvGrid og = ov_grid(ctx, row_begin, row_end, tiles(XCD_RBSOR, LANES_PAIR).rows(rt).dense_if(full).hints_within(4));
    // k_rbsor_pair<2, RT, parity of the first row, DM, 2, FULL, float>: the carrying pass exists on 4-row tiles with the IEEE division alone
    auto run = [=](auto RT, auto DM, auto FULL) {
        constexpr int tile = decltype(RT)::value, mode = decltype(DM)::value;
        constexpr bool carry = decltype(FULL)::value;
        return pick<0, 1>(par0, [&](auto PAR) {
            klaunch(k_rbsor_pair<2, tile, PAR, mode, 2, carry, T>, og, ctx->stream, k, row_begin, row_end, (const uint8_t *)ctx->d_bcmap, (T *)pc_out->d, (T *)pn_out->d,
                    (const T *)pc->d, (const T *)pn->d, (const T *)vc->d);
        });
    };
    return launch(ctx, "rbsor_pair", [=] {
        if (full) return run(Int<4>{}, Int<0>{}, Bool<true>{});
        return pick<2, 4>(rt, [&](auto RT) { return with_dm_const<T>(dm, [&](auto DM) { return run(RT, DM, Bool<false>{}); }); });
    });
}

int fs_rbsor_halfsweep_src(fs_ctx *ctx, double omega, int parity, fs_field *pn, const fs_field *pc, const fs_field *src,
                           int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_REQUIRE(parity == 0 || parity == 1, "parity must be 0 or 1");
    FS_FIELD(pn, 1); FS_FIELD(pc, 1); FS_FIELD(src, 2);
    FS_ROWS();
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        auto k = make_konst<T>(ctx, 1.0, 1.0, 1.0, 0.0, omega);
        return launch(ctx, parity ? "rbsor_odd_src" : "rbsor_even_src", [=] {
            klaunch(k_rbsor<true, T>, rb_grid(ctx, row_begin, row_end), dim3(256), ctx->stream, ctx->grid(), k,
                               row_begin, parity, (T *)pn->d, (const T *)pc->d, (const T *)src->d);
        });
    });
}

int fs_poisson_source(fs_ctx *ctx, double dt, double dx, fs_field *src, const fs_field *vc, int row_begin, int row_end)
{
    FS_REQUIRE(ctx, "ctx is null");
    FS_FIELD(src, 2); FS_FIELD(vc, 2);
    FS_REQUIRE(src != vc, "src must not alias vc");
    FS_ROWS();
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        auto k = make_konst<T>(ctx, dt, dx, 1.0);
        if (ctx->use_pairs) {
            const OvGrid og = ov_grid(ctx, row_begin, row_end, tiles(XCD_JACOBI, LANES_PAIR_WIDE).rows(4));      // (deep-wall workgroups skipped: nobody reads the source there)
            const int dm = dm_const(ctx, k);
            return launch(ctx, "poisson_source", [=] {
                return with_dm_const<T>(dm, [&](auto DM) { klaunch(k_poisson_source_n<2, 4, DM, T>, og, ctx->stream, k, row_begin, row_end, (T *)src->d, (const T *)vc->d); });
            });
        }
        return launch_cells(ctx, "poisson_source", k_poisson_source<T>, row_begin, row_end, k, (T *)src->d, (const T *)vc->d);
    });
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
    const int rc = by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        auto k = make_konst<T>(ctx, dt, dx, 1.0);
        return launch(ctx, "poisson_residual", [=] {
            klaunch(k_residual<T>, grid, dim3(256), ctx->stream, ctx->grid(), k, row_begin, row_end, (const T *)p->d, (const T *)vc->d, ctx->d_partial);
            klaunch(k_residual_final<double>, dim3(1), dim3(1024), ctx->stream, (const double *)ctx->d_partial, (int)nblocks, ctx->d_acc);
        });
    });
    if (rc) return rc;
    double h[2];
    FS_HIP(hipMemcpyAsync(h, ctx->d_acc, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    *sum_sq = h[0];
    *count = h[1];
    return FS_OK;
}

}  // extern "C"
