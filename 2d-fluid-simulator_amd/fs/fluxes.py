"""Host side of the scale-to-scale fluxes (new; the reference has none): where the energy and the enstrophy of the flow are going.  The
device (csrc/fs_flux.h, include/fs_hip.h fs_flux_*) filters the velocity and the vorticity with boxes of (2 r + 1)^2 cells (coarse-graining:
Germano 1992, Eyink 2005, Aluie et al. 2018), forms the sub-filter stress tau_ij = filt(u_i u_j) - filt(u_i) filt(u_j) and accumulates, per
cell of a box and per half-width r, PI = -tau_ij S_ij - the rate at which the scales larger than the filter feed the smaller ones -, the
enstrophy flux ZF and the sub-filter energy K, by launches that ride the step.  It holds on any domain, with walls inside it: solid cells
count as fluid at rest.  This module holds the rider and the result dict.  Driven by FluidSimulator.start_scale_fluxes / scale_fluxes /
reset_scale_fluxes / stop_scale_fluxes / scale_flux / filtered_fields."""
import numpy as np

from .riders import BOX, CountedRider, Param

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


class ScaleFluxes(CountedRider):
    """The accumulated scale-to-scale fluxes of a FluidSimulator (start_scale_fluxes): the device planes and their parameters.
    held(z) -> (box, half_widths, every, start), or None."""
    kind, payload, noun, plural = "flux", "sums", "scale fluxes", True
    params = (BOX, Param("half_widths", BOX.write, BOX.read, "{theirs} accumulated with the half_widths {0}, {ours} with {1}"))

    def __init__(self, dev, flux, shape):
        super().__init__(dev, flux, flux.every, flux.start)
        self.flux, self.shape = flux, tuple(shape)

    def attached(self):
        return tuple(self.flux.box), tuple(self.flux.half_widths)

    def launch(self, sim):
        self.dev.flux_launch(self.flux, sim._solver.get_fields()[0])

    def data(self):
        sums, _, samples = self.dev.flux_read(self.flux)
        return flux_result(sums, samples, self.sample_steps(samples), self.flux.box, self.flux.half_widths, self.flux.dx, self.shape)
