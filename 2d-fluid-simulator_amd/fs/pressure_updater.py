"""Pressure-Poisson relaxation (reference: fs/pressure_updater.py).

predict_p (fs/pressure_updater.py:23-38) is evaluated inside the HIP sweep kernels.  Two equivalent
kernel forms exist: reading v like the reference, or reading a per-step precomputed source pair (the
source term depends only on v, which is constant over the sweeps of one step).  Both keep the
reference's operation order and give bit-identical pressures; `precompute_source` only trades one
extra pass per step for cheaper sweeps.
"""
import os
from abc import ABCMeta, abstractmethod


class PressureUpdater(metaclass=ABCMeta):
    def __init__(self, boundary_condition, dt, dx):
        self._bc = boundary_condition
        self._dev = boundary_condition.device
        self.dt = dt
        self.dx = dx

    @abstractmethod
    def update(self, p, v_current):
        pass


class JacobiPressureUpdater(PressureUpdater):
    """Jacobi method: n_iter x { pressure BC on p.current; p.next <- predict_p(p.current) on not-wall cells; swap }
    (fs/pressure_updater.py:41-66)."""

    def __init__(self, boundary_condition, dt, dx, n_iter, precompute_source=None, lazy_bc=None):
        super().__init__(boundary_condition, dt, dx)
        self._n_iter = n_iter
        # one extra pass per step (~110 us at res 4096) buys cheaper sweeps (76 vs 87 us): worth it from 9 sweeps on - from 6 on where
        # two-sweep passes are in use (decided below): 110 + 2 x 98 + 2 x 82 against 6 x 93 us
        tentative = precompute_source is None and 6 <= n_iter < 9 and self._dev.lazy_bc_ok
        self._precompute = (n_iter >= 9 or tentative) if precompute_source is None else bool(precompute_source)
        self._src = self._dev.alloc(2) if self._precompute else None
        # Long runs: all but the last two sweeps evaluate the pressure boundary condition on the fly from the raw output of the
        # previous sweep instead of launching the boundary kernel in between (same bits; the last two sweeps run the real kernel,
        # which leaves both p buffers exactly as the reference's n x (BC, sweep, swap) does).  Needs the source-pair form, a mask
        # that admits it (fs_lazy_bc_ok) and a p that no user upload has put into an arbitrary state.
        self._lazy = (self._precompute and n_iter >= 6 and self._dev.lazy_bc_ok) if lazy_bc is None else \
            (bool(lazy_bc) and self._precompute and n_iter >= 3 and self._dev.lazy_bc_ok)
        # Two sweeps per launch (fs_jacobi_pair_lazy): bc2 res 1600 +50 %, res 4096 +51 %, bc5 res 4096 +30 %, bc1 res 2048 +27 %; a mask
        # full of small obstacles sends too many rows down its general path (bc3 res 1000: 31 % of the rows, -6 %).  Same bits either
        # way, so a single-GPU run times the three forms on this mask once (FS_JACOBI_PAIRS=0 / 1 / 2 decides instead; 2 = vertical recipes in the tiles too).
        want = os.environ.get("FS_JACOBI_PAIRS", "auto")
        self._pairs = (self._lazy and want != "0" and n_iter >= 6
                       and (self._dev.nranks == 1 or 2 * max(2, 1 + self._dev.bc_radius_p) <= self._dev.halo))   # a pass reaches 4 rows
        # The tiles of the two-sweep pass hand rows with floors / ceilings / corners nearby to a general path (one row per workgroup); the
        # variant whose tiles also apply the vertical recipes keeps only thin walls there but costs 6 % where it is not needed.  Decided from
        # the mask, not from a timing run (round 2 timed three forms inside this constructor: the launch sequence then differed from run to
        # run): vertical when more than 5 % of the wave-tile rows would take the general path otherwise (bc3's cylinders: 31 %; bc2 / bc5: < 1 %).
        self._vertical = want == "2"
        self.form = "single sweeps"
        if self._pairs:
            if want == "auto" and hasattr(self._dev, "lazy_flags"):
                flags, (general, general_v) = self._dev.lazy_flags()
                self._vertical = general > 0.05 * max(flags.size, 1) and general_v < general
            self.form = "two sweeps per pass" + (", vertical recipes in the tiles" if self._vertical else "")
        elif self._lazy:
            self.form = "single sweeps, boundary condition in the sweep"
        # Four sweeps per pass (fs_jacobi_quad_lazy) where the mask admits it: the passes of a long run are launch- and latency-bound
        # (BASELINE configs[1]: 24 two-sweep passes of 21.6 us = 78 % of the step)
        self._quads = (self._pairs and n_iter >= 10 and os.environ.get("FS_JACOBI_QUADS", "1") == "1" and getattr(self._dev, "jacobi_quad_ok", False))
        if self._quads:
            self.form = "four sweeps per pass"
        if tentative and not self._pairs:
            self._precompute, self._src, self._lazy = False, None, False
        # The last two rounds - 2 x (boundary kernel + sweep), which leave both buffers as the reference does - in ONE pass into a third
        # buffer (fs_jacobi_finish; bc2 res 1600: 47 -> 25 us of a 585 us step).  Single GPU, masks that admit the four-sweep pass.
        self._finish = self._quads and self._dev.nranks == 1
        self._spare = (self._dev.alloc(1),) if self._finish else None      # (a tuple, like RedBlackSorPressureUpdater's: FluidSimulator._signature)

    def update(self, p, v_current):
        if self._precompute:
            self._dev.poisson_source(self.dt, self.dx, self._src, v_current)
        n_lazy = self._n_iter - 2 if self._lazy else 0
        n_real = self._n_iter - n_lazy
        if self._quads and p.current.static_id == p.next.static_id:
            # four sweeps per pass (the pass writes not-wall cells only: the wall cells nothing writes must be equal in the two buffers,
            # Field.static_id); what does not fill a pass runs as single lazily-bounded sweeps
            for _ in range(n_lazy // 4):
                self._dev.jacobi_quad_lazy(p.next, p.current, self._src)
                p.swap()
            n_lazy %= 4
            n_pairs = n_lazy // 2        # (equal wall histories: a single two-sweep pass is as good as an even number of them)
        else:
            # two sweeps per pass where possible; an even number of passes, so that every iterate lands in the physical buffer the
            # reference's rotation puts it in (the buffers differ in the wall cells nothing ever writes)
            n_pairs = (n_lazy // 4) * 2 if self._pairs else 0
        for k in range(n_pairs):
            self._dev.jacobi_pair_lazy(p.next, p.current, self._src, swapped=bool(k & 1), vertical=self._vertical)
            p.swap()
        for _ in range(n_lazy - 2 * n_pairs):
            self._dev.jacobi_sweep_lazy(p.next, p.current, self._src)
            p.swap()
        if (self._finish and n_real == 2 and self._n_iter - 2 >= 4
                and p.current.static_id == p.next.static_id == self._spare[0].static_id and not (p.current.user_data or p.next.user_data)):
            # (the pass stores the cells some kernel writes; the rest must agree in the three buffers: no uploads / fills in between)
            self._dev.jacobi_finish(self._spare[0], p.next, p.current, self._src)
            p.current, self._spare = self._spare[0], (p.current,)
            return
        for _ in range(n_real):
            self._bc.set_pressure_boundary_condition(p.current)
            self._update(p.next, p.current, v_current)
            p.swap()

    def _update(self, p_next, p_current, v_current):
        if self._precompute:
            self._dev.jacobi_sweep_src(p_next, p_current, self._src)
        else:
            self._dev.jacobi_sweep(self.dt, self.dx, p_next, p_current, v_current)


class RedBlackSorPressureUpdater(PressureUpdater):
    """Red-black SOR (fs/pressure_updater.py:69-114): per iteration the odd cells are relaxed from p.current
    into p.next, then the even cells are relaxed IN PLACE on p.next (blending with that buffer's stale
    value), then the buffers swap.  Not a textbook single-buffer SOR - reproduced literally."""

    def __init__(self, boundary_condition, dt, dx, relaxation_factor, n_iter, precompute_source=False, fused=True, pair=None):
        super().__init__(boundary_condition, dt, dx)
        self._n_iter = n_iter
        self._relaxation_factor = relaxation_factor
        # fused: odd + even pass of one iteration in a single kernel (same bits, fewer bytes)
        fast = fused and not precompute_source and os.environ.get("FS_MARCH", "1") != "0"
        self._fused = fast and boundary_condition.get_resolution()[0] % 2 == 0          # (lanes of 2 cells: any even width, like the pair pass below)
        self._precompute = bool(precompute_source)
        self._src = self._dev.alloc(2) if self._precompute else None
        # pair: TWO iterations and the two boundary passes between them in one pass over HBM (csrc/fs_rbpair.h; same bits, 25 instead of
        # 2 x 21 B per fluid cell and two launches less).  Out of place: the pressure rotates through a second pair of buffers.  Needs a
        # mask that admits it (Device.rb_pair_ok: no one-cell-thin walls between fluid regions), f32, and on slabs a halo of 4 rows.
        # Slab runs: the pass wants v and p.current 4 rows deep at the END of the step, where the ghost rows are at their shallowest.  At halo 16
        # the tracker then exchanges 0.6 times per step in a 5-step pattern that, times the 6-step buffer rotation, no tape can hold; at halo 20
        # (the default for slabs of 160 rows and more since round 4) the pattern is one exchange every 2 steps with and without the pass
        # (tools/slab_period.py) and the pass is on - loop-back, middle slab of the 8-way cut of bc5 res 4096: 131-132 us per step against
        # 133-134 at halo 16 without it (profiles/r3_loopback_slab_step.txt).  Shallower halos keep the single iterations.
        if pair is None:
            pair = os.environ.get("FS_RBSOR_PAIR", "1" if (self._dev.nranks == 1 or self._dev.halo >= 20) else "0") == "1"
        self._pair = (bool(pair) and fast and n_iter >= 2 and getattr(self._dev, "rb_pair_ok", False)
                      and (self._dev.nranks == 1 or self._dev.halo >= 4))
        self._spare = (self._dev.alloc(1), self._dev.alloc(1)) if self._pair else None

    def update(self, p, v_current):
        if self._precompute:
            self._dev.poisson_source(self.dt, self.dx, self._src, v_current)
        n = self._n_iter
        while self._pair and n >= 2:
            c_out, n_out = self._spare
            # the pass stores fluid cells and boundary targets only: every other cell must already be equal in the buffer it reads and
            # the one it writes (Field.static_id).  After an upload / fill into one of them the pass carries every cell once.
            full = c_out.static_id != p.current.static_id or n_out.static_id != p.next.static_id
            self._dev.rbsor_pair(self.dt, self.dx, self._relaxation_factor, c_out, n_out, p.current, p.next, v_current, full=full)
            c_out.static_id, n_out.static_id = p.current.static_id, p.next.static_id
            self._spare = (p.current, p.next)
            p.current, p.next = c_out, n_out
            n -= 2
        for _ in range(n):
            self._bc.set_pressure_boundary_condition(p.current)
            self._update(p.next, p.current, v_current)
            p.swap()

    def _update(self, p_next, p_current, v_current):
        if self._fused:
            self._dev.rbsor_iteration(self.dt, self.dx, self._relaxation_factor, p_next, p_current, v_current)
            return
        self._update_pressures_odd(p_next, p_current, v_current)
        self._update_pressures_even(p_next, p_next, v_current)

    def _half(self, parity, pn, pc, vc):
        if self._precompute:
            self._dev.rbsor_halfsweep_src(self._relaxation_factor, parity, pn, pc, self._src)
        else:
            self._dev.rbsor_halfsweep(self.dt, self.dx, self._relaxation_factor, parity, pn, pc, vc)

    def _update_pressures_odd(self, pn, pc, vc):
        self._half(1, pn, pc, vc)

    def _update_pressures_even(self, pn, pc, vc):
        self._half(0, pn, pc, vc)


class MultigridPressureUpdater(PressureUpdater):
    """W-cycle multigrid around the reference's red-black SOR (new; the reference has no converging pressure solve).  Per cycle:
    `pre` red-black iterations (the class above, unchanged - pair pass and buffer rotation included), the pressure boundary kernel on
    p.current, then one call that restricts the fluid-cell residual 4 (predict_p - p) to the mask-aware coarse hierarchy of
    fs/multigrid.py, runs W(1, R1) there (two coarse visits per level: V-cycles diverge with these piecewise-constant transfers) and adds
    the prolonged correction to the fluid cells of p.current AND p.next (csrc/fs_mg.h; include/fs_hip.h fs_mg_cycle), the boundary kernel
    on p.next, and `post` red-black iterations.  Both buffers take the correction because the reference's iteration is a two-buffer method:
    its even half sweep blends with the value p.next held, so a correction p.next lacks comes back as (1 - omega) x itself.
    FS_MG_TAIL=<cells>: the levels from the first one of at most that many cells down run in one workgroup (default: whatever fits its
    LDS; 0: one launch per half sweep everywhere) - the same bits for every value.  Single GPU; nothing to checkpoint.
    coarsest="sweeps" (the default) relaxes the last level - where an extent turns odd - with `coarsest_sweeps` sweeps, which does not solve a
    last level of more than a few dozen cells (res 100, 200, 400 end on 50 x 25).  coarsest="direct" cuts the hierarchy at the first level
    of at most `direct_cells` cells (the last level if none is that small; ValueError beyond 4096 active cells) and solves it exactly: the
    inverse of its operator is built once on the host (fs/multigrid.py direct_solve, float64, rounded to the field dtype) and applied with
    one launch per visit.  Then FS_MG_TAIL is not read (no one-workgroup kernel) and `coarsest_sweeps` is ignored."""

    def __init__(self, boundary_condition, dt, dx, relaxation_factor=1.3, n_cycles=1, pre=2, post=2, coarse_sweeps=2, coarsest_sweeps=64,
                 coarsest="sweeps", direct_cells=2048):
        super().__init__(boundary_condition, dt, dx)
        if self._dev.nranks > 1:
            raise NotImplementedError("the multigrid pressure updater runs on a single GPU (no slabs)")
        from .multigrid import build_hierarchy, direct_level, direct_solve
        self._n_cycles, self._pre, self._post = int(n_cycles), int(pre), int(post)
        if min(self._n_cycles, self._pre, self._post, int(coarse_sweeps), int(coarsest_sweeps)) < 0:
            raise ValueError("cycle, iteration and sweep counts must be >= 0")
        if coarsest not in ("sweeps", "direct"):
            raise ValueError(f"coarsest must be 'sweeps' or 'direct', got {coarsest!r}")
        if int(direct_cells) < 1:
            raise ValueError("direct_cells must be >= 1")
        self._relaxation_factor = relaxation_factor
        levels = build_hierarchy(boundary_condition.mask, self._dev.dtype)      # (ValueError: odd extents, no coarse level)
        self._direct = None
        if coarsest == "direct":
            k = direct_level([lv[0].shape for lv in levels], int(direct_cells), [int((lv[2] > 0).sum()) for lv in levels])
            levels = levels[:k]
            self._mg = self._dev.mg_create(levels, 0, int(coarse_sweeps), int(coarsest_sweeps))
            self._direct = self._dev.mg_set_direct(self._mg, *direct_solve(*levels[-1]))
        else:
            tail = int(os.environ.get("FS_MG_TAIL", "-1"))
            self._mg = self._dev.mg_create(levels, tail, int(coarse_sweeps), int(coarsest_sweeps))
        self.levels = [lv[0].shape for lv in levels]
        # one inner updater serves both smoothing legs (its iteration count is set per leg): one pair of rotating spare buffers
        self._inner = RedBlackSorPressureUpdater(boundary_condition, dt, dx, relaxation_factor, max(self._pre, self._post, 1))

    @property
    def _spare(self):
        """The inner updater's rotating buffers (FluidSimulator._signature)."""
        return self._inner._spare

    def info(self):
        """{"levels", "tail_level" (0: no one-workgroup kernel), "launches" of the last correction, "direct_level" (0: the last level is
        relaxed), "direct_cells" (the active cells of the level that is solved exactly)}."""
        return self._dev.mg_info(self._mg)

    def direct_matrix(self):
        """(cells, M) of coarsest="direct" exactly as uploaded: the active cells' indices J * nx + I in the last level (int32, ascending) and
        the inverse in the field dtype, padding stripped."""
        if self._direct is None:
            raise ValueError("direct_matrix() needs coarsest='direct'")
        return self._direct

    def _smooth(self, n, p, v_current):
        self._inner._n_iter = n
        self._inner.update(p, v_current)

    def update(self, p, v_current):
        for _ in range(self._n_cycles):
            self._smooth(self._pre, p, v_current)
            self._bc.set_pressure_boundary_condition(p.current)
            self._dev.mg_cycle(self._mg, self.dt, self.dx, p.current, p.next, v_current)
            self._bc.set_pressure_boundary_condition(p.next)
            self._smooth(self._post, p, v_current)

    def __del__(self):
        try:
            self._dev.mg_free(self._mg)
        except Exception:
            pass
