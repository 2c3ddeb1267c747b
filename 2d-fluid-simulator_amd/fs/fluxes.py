"""Host side of the scale-to-scale fluxes (new; the reference has none): where the energy and the enstrophy of the flow are going.  The
device (csrc/fs_flux.h, include/fs_hip.h fs_flux_*) filters the velocity and the vorticity with boxes of (2 r + 1)^2 cells (coarse-graining:
Germano 1992, Eyink 2005, Aluie et al. 2018), forms the sub-filter stress tau_ij = filt(u_i u_j) - filt(u_i) filt(u_j) and accumulates, per
cell of a box and per half-width r, PI = -tau_ij S_ij - the rate at which the scales larger than the filter feed the smaller ones -, the
enstrophy flux ZF and the sub-filter energy K, by launches that ride the step.  It holds on any domain, with walls inside it: solid cells
count as fluid at rest.  This module holds the rider and the result dict.  Driven by FluidSimulator.start_scale_fluxes / scale_fluxes /
reset_scale_fluxes / stop_scale_fluxes / scale_flux / filtered_fields."""
import numpy as np

from .riders import Rider, samples_after

PLANES = ("pi", "zf", "k")
FILTERED = ("u", "w", "om", "uu", "uw", "ww", "uom", "wom")


def valid_rect(box, r, shape):
    """The valid cells of half-width r inside the box, (x0, y0, x1, y1) half-open in global cells: r + 1 <= i <= X - 2 - r and
    r + 1 <= j <= Y - 2 - r on a grid of shape (X, Y)."""
    return (max(box[0], r + 1), max(box[1], r + 1), min(box[2], shape[0] - 1 - r), min(box[3], shape[1] - 1 - r))


def _mean_over(planes, box, rect):
    """The mean of every plane (..., Nx, Ny) over the global rectangle `rect` inside the box."""
    sub = planes[..., rect[0] - box[0]:rect[2] - box[0], rect[1] - box[1]:rect[3] - box[1]]
    return sub.mean(axis=(-2, -1))


def flux_result(sums, samples, sample_steps, box, half_widths, dx, shape):
    """The dict scale_fluxes() / scale_flux() return from the accumulated planes `sums` (n_r, 3, Nx, Ny) of `samples` samples on a grid of
    `shape` = (X, Y) cells."""
    sums = np.asarray(sums, np.float64)
    half_widths = tuple(int(r) for r in half_widths)
    with np.errstate(all="ignore"):
        mean = sums / samples if samples else np.zeros_like(sums)
    valid = [valid_rect(box, r, shape) for r in half_widths]
    common = valid[-1]              # the largest half-width's: inside every other
    out = {"half_widths": half_widths, "widths": np.array([(2 * r + 1) * dx for r in half_widths], np.float64), "samples": int(samples),
           "sample_steps": sample_steps, "box": tuple(box), "valid": valid, "sums": sums}
    own = {}
    for n, name in enumerate(PLANES):
        out[name] = mean[:, n]
        out["mean_" + name] = np.array([_mean_over(mean[k, n], box, common) for k in range(len(half_widths))], np.float64)
        own[name] = np.array([_mean_over(mean[k, n], box, valid[k]) for k in range(len(half_widths))], np.float64)
    out["mean_own"] = own
    return out


class ScaleFluxes(Rider):
    """The accumulated scale-to-scale fluxes of a FluidSimulator (start_scale_fluxes): the device planes and their parameters.  No ring:
    room() is None and run() is not cut by it."""

    def __init__(self, dev, flux, shape):
        self.dev, self.flux, self.shape = dev, flux, tuple(shape)
        self.every, self.start_step = int(flux.every), int(flux.start)
        self.base = 0              # samples taken before the last reset (sample_steps)

    @property
    def token(self):
        return ("flux", self.flux.serial)

    def launch(self, sim):
        self.dev.flux_launch(self.flux, sim._solver.get_fields()[0])

    def free(self):
        self.dev.flux_free(self.flux)

    def sample_steps(self, samples):
        """The step (counted from start_scale_fluxes, from 1) of every sample in the planes, int64 (samples,)."""
        k = self.base + np.arange(int(samples), dtype=np.int64)
        return self.start_step + (k + 1) * self.every

    def data(self):
        sums, _, samples = self.dev.flux_read(self.flux)
        return flux_result(sums, samples, self.sample_steps(samples), self.flux.box, self.flux.half_widths, self.flux.dx, self.shape)

    def reset(self):
        _, launches, _ = self.dev.flux_read(self.flux, sums=False)
        self.dev.flux_reset(self.flux)
        self.base = samples_after(launches, self.every, self.start_step)

    def checkpoint(self):
        sums, launches, samples = self.dev.flux_get(self.flux)
        return {"flux.sums": sums, "flux.launches": np.array(launches), "flux.samples": np.array(samples), "flux.base": np.array(self.base),
                "flux.box": np.array(self.flux.box, np.int64), "flux.half_widths": np.array(self.flux.half_widths, np.int64),
                "flux.every": np.array(self.every), "flux.start": np.array(self.start_step)}

    @staticmethod
    def held(z):
        """-> (box, half_widths, every, start), or None."""
        if "flux.sums" not in z:
            return None
        return (tuple(int(b) for b in np.asarray(z["flux.box"])), tuple(int(r) for r in np.asarray(z["flux.half_widths"])),
                int(z["flux.every"]), int(z["flux.start"]))

    def restore(self, z):
        """Refused (ValueError) before any device work when the checkpoint's box, half-widths, every or start_step are not the attached
        ones."""
        held = self.held(z)
        if held is None:
            raise ValueError("the checkpoint holds no scale fluxes")
        box, half_widths, every, start = held
        if box != tuple(self.flux.box):
            raise ValueError(f"the checkpoint's scale fluxes were accumulated over the box {box}, the attached ones over {tuple(self.flux.box)}")
        if half_widths != tuple(self.flux.half_widths):
            raise ValueError(f"the checkpoint's scale fluxes were accumulated with the half_widths {half_widths}, the attached ones with "
                             f"{tuple(self.flux.half_widths)}")
        if (every, start) != (self.every, self.start_step):
            raise ValueError(f"the checkpoint's scale fluxes sample every {every} from {start}, the attached ones every {self.every} from "
                             f"{self.start_step}")
        self.dev.flux_set(self.flux, z["flux.sums"], int(z["flux.launches"]), int(z["flux.samples"]))
        self.base = int(z["flux.base"])
        return int(z["flux.samples"])
