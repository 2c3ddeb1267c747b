"""Worker for tests/test_flow_stats_cpu.py: one rank of a gloo job whose device is the CPU stand-in of tests/oracle_device.py with the
flow diagnostics added (tests/flow_stats_ref.py on the rank's own window, NaN-poisoned ghost rows included).  The product's
DeviceBase.flow_stats (exchange to depth 1, sums over ranks, NaN-safe maxima) combines the ranks."""
import os
import sys

import numpy as np


def _device_cls():
    import torch
    import torch.distributed as dist
    from flow_stats_ref import SLOTS, flow_stats_ref
    from oracle_device import OracleSlabDevice

    class StatsSlabDevice(OracleSlabDevice):
        def _p_upload_scene(self, bc_mask, bc_const, bc_dye):
            self.win_mask = np.asarray(bc_mask)[:, self.g_lo:self.g_hi]
            return super()._p_upload_scene(bc_mask, bc_const, bc_dye)

        def _p_flow_stats(self, dx, vh, ph, box):
            lo = self.halo - self.r_off              # window row of the first owned row
            d = flow_stats_ref(vh.a, ph.a, self.win_mask, dx, box, rows=(lo, lo + self.nyl), y0=self.g_lo)
            return [d[k] for k in SLOTS]

        def _p_allreduce(self, values):
            t = torch.tensor([float(v) for v in values], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return tuple(t.tolist())

    return StatsSlabDevice


def run(rank, world, port, fname, halo, steps, out_dir, poison_rank=-1):
    """`steps` steps of the golden trajectory's scene on `world` slabs, then flow_stats; rank 0 compares with the single-domain reference
    on the gathered fields.  poison_rank >= 0: that rank plants NaN in one owned fluid cell of p first (the count and the NaN must reach
    every rank)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    for p in (repo, os.path.join(repo, "2d-fluid-simulator_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import fs
    from flow_stats_ref import compare, flow_stats_ref
    from fs.boundary_condition import default_body_box
    from helpers import make_product, traj_config

    def allgather(obj):
        out = [None] * world
        dist.all_gather_object(out, obj)
        return out

    g = np.load(os.path.join(here, "golden", fname))
    cfg = traj_config(g)
    fs.runtime.init(dtype="f64" if cfg["fp64"] else "f32", rank=rank, nranks=world, halo=halo, allgather=allgather,
                    device_cls=_device_cls())
    sim = make_product(g, cfg)
    dev, s = sim._solver._bc.device, sim._solver
    for _ in range(steps):
        sim.step()
    v, p = s.get_fields()[:2]
    if poison_rank >= 0:
        # one fluid cell in the middle owned row of poison_rank, planted in the rank's own window (an upload would refresh every row)
        if rank == poison_rank:
            r = dev.halo - dev.r_off + dev.nyl // 2
            i = int(np.nonzero(dev.win_mask[:, r] == 0)[0][0])
            p._h.a[i, r] = np.nan
    box = default_body_box(cfg["bc"], cfg["res"]) if cfg["bc"] in (1, 3, 5, 6) else None
    # every ghost row of v and p stale: NaN in the window outside the owned rows, validity 0 - as a kernel that wrote them leaves them here
    lo = dev.halo - dev.r_off
    for f in (v, p):
        f._h.a[:, :lo] = np.nan
        f._h.a[:, lo + dev.nyl:] = np.nan
        f.valid = 0
    local = dev._p_flow_stats(s.dx, v._h, p._h, box)          # without the exchange the owned edge rows read NaN
    nan_without = bool(np.isnan(local[2]) or np.isnan(local[3]))
    n0 = dev.n_exchanges
    got = dev.flow_stats(s.dx, v, p, box)
    exchanged = dev.n_exchanges > n0
    vg, pg = v.to_numpy(), p.to_numpy()
    seen = allgather((nan_without, exchanged))
    if rank == 0:
        exp = flow_stats_ref(vg, pg, g["bc_mask"], s.dx, box)
        bad = compare(got, exp)
        if poison_rank >= 0 and got["nonfinite"] != 1:
            bad.append(f"planted NaN counted {got['nonfinite']} times")
        if not all(x for x, _ in seen):
            bad.append(f"stale ghost rows did not reach the local sums on every rank: {seen}")
        if not all(e for _, e in seen):
            bad.append(f"flow_stats did not exchange the stale ghost rows on every rank: {seen}")
        with open(os.path.join(out_dir, "result.txt"), "w") as f:
            f.write(f"{len(bad)} {' | '.join(bad)}\n")
    dist.barrier()
    dist.destroy_process_group()
