"""Host side of the kinetic-energy budget (new; the reference has none): where the fluctuation energy k = (<u'u'> + <w'w'>) / 2 of a flow is
made, where it is destroyed, and by what.  The device (csrc/fs_budget.h, include/fs_hip.h fs_budget_*) accumulates 21 raw moments per fluid
cell of a box - first, second and third moments of u, w, the pressure correlations, the velocity gradient and its squares - by launches that
ride the step; this module turns them into the terms of the budget (derive_budget), the terms of the mean momentum equation
(momentum_balance), and holds the rider.  Driven by FluidSimulator.start_budget / budget / reset_budget / stop_budget / budget_sample.

Raw moments are differenced here (<ab> - <a><b>, and the third-moment expansions), as in fs.averages: the accumulators are doubles of
f32-sized values for that reason, and a central moment far below the product of the means carries the rounding of that difference."""
import numpy as np

from .riders import BOX, CountedRider

PLANES = ("u", "w", "p", "uu", "ww", "uw", "pu", "pw", "uuu", "uuw", "wwu", "www", "ux", "uy", "wx", "wy", "uxux", "uyuy", "wxwx", "wywy", "pd")
NPLANE = len(PLANES)                 # FS_BUDGET_NPLANE
BYTES_PER_CELL = 8 * NPLANE          # device memory per cell of the box
DERIVED = ("U", "W", "P", "uu", "ww", "uw", "k", "pu", "pw", "uuu", "uuw", "wwu", "www", "Ux", "Uy", "Wx", "Wy")      # besides TERMS
TERMS = ("convection", "production", "dissipation", "turbulent_transport", "pressure_diffusion", "pressure_dilatation", "viscous_diffusion",
         "residual")


def valid_cells(fluid):
    """The cells of the box whose four neighbours are fluid cells of the box, and which are fluid themselves."""
    fluid = np.asarray(fluid, bool)
    v = np.zeros_like(fluid)
    v[1:-1, 1:-1] = fluid[1:-1, 1:-1] & fluid[:-2, 1:-1] & fluid[2:, 1:-1] & fluid[1:-1, :-2] & fluid[1:-1, 2:]
    return v


def _ddx(f, two_dx):
    out = np.zeros_like(f)
    out[1:-1, :] = (f[2:, :] - f[:-2, :]) / two_dx
    return out


def _ddy(f, two_dx):
    out = np.zeros_like(f)
    out[:, 1:-1] = (f[:, 2:] - f[:, :-2]) / two_dx
    return out


def _laplacian(f, dx):
    out = np.zeros_like(f)
    out[1:-1, 1:-1] = (f[2:, 1:-1] + f[:-2, 1:-1] + f[1:-1, 2:] + f[1:-1, :-2] - 4.0 * f[1:-1, 1:-1]) / (dx * dx)
    return out


def derive_budget(sums, samples, fluid, dx, re):
    """The budget of k from the accumulated planes `sums` (21, Nx, Ny) of `samples` samples over a box whose fluid cells (mask == 0) are
    `fluid` (Nx, Ny) -> dict of float64 (Nx, Ny) arrays.  With m(X) = S_X / n:
      U, W, P; uu = m(uu) - U U, ww, uw (the order of fs.averages.derive_averages); k = (uu + ww) / 2; pu = m(pu) - P U, pw;
      uuu = m(uuu) - 3 U m(uu) + 2 U^3, uuw = m(uuw) - W m(uu) - 2 U m(uw) + 2 U^2 W, wwu, www (third central moments);
      Ux, Uy, Wx, Wy = m(ux) .. (the accumulated gradients, not differences of U).
    On every fluid cell: production = -(uu Ux + uw (Uy + Wx) + ww Wy); dissipation = (1 / re) sum over the four gradients of
    (m(g^2) - G^2), reported positive; pressure_dilatation = m(pd) - P (Ux + Wy).  On the `valid` cells - fluid, with four fluid neighbours
    inside the box -, with d the central difference over 2 dx: convection = -(U dx k + W dy k); turbulent_transport = -(dx Tx + dy Ty),
    Tx = (uuu + wwu) / 2, Ty = (uuw + www) / 2; pressure_diffusion = -(dx pu + dy pw); viscous_diffusion = (1 / re) (5-point Laplacian of
    k) / dx^2; and residual = convection + production - dissipation + turbulent_transport + pressure_diffusion + pressure_dilatation +
    viscous_diffusion.  In a statistically steady flow -residual is the rate at which the advection scheme, the confinement, the velocity
    limit and the splitting change k.  Everything is 0 where it is not defined.  "totals": each term summed over `valid` times dx^2.
    samples == 0 raises ValueError."""
    n = int(samples)
    if n <= 0:
        raise ValueError("no samples accumulated yet")
    sums = np.asarray(sums, np.float64)
    fluid = np.asarray(fluid, bool)
    if sums.shape != (NPLANE,) + fluid.shape:
        raise ValueError(f"expected sums of shape {(NPLANE,) + fluid.shape}, got {sums.shape}")
    dx, re = float(dx), float(re)
    m = dict(zip(PLANES, sums / np.float64(n)))
    U, W, P = m["u"], m["w"], m["p"]
    uu = m["uu"] - U * U
    ww = m["ww"] - W * W
    uw = m["uw"] - U * W
    k = 0.5 * (uu + ww)
    pu = m["pu"] - P * U
    pw = m["pw"] - P * W
    uuu = m["uuu"] - 3.0 * U * m["uu"] + 2.0 * U * U * U
    uuw = m["uuw"] - W * m["uu"] - 2.0 * U * m["uw"] + 2.0 * U * U * W
    wwu = m["wwu"] - U * m["ww"] - 2.0 * W * m["uw"] + 2.0 * U * W * W
    www = m["www"] - 3.0 * W * m["ww"] + 2.0 * W * W * W
    Ux, Uy, Wx, Wy = m["ux"], m["uy"], m["wx"], m["wy"]
    out = {"U": U, "W": W, "P": P, "uu": uu, "ww": ww, "uw": uw, "k": k, "pu": pu, "pw": pw, "uuu": uuu, "uuw": uuw, "wwu": wwu, "www": www,
           "Ux": Ux, "Uy": Uy, "Wx": Wx, "Wy": Wy}
    out["production"] = -(uu * Ux + uw * (Uy + Wx) + ww * Wy)
    out["dissipation"] = ((m["uxux"] - Ux * Ux) + (m["uyuy"] - Uy * Uy) + (m["wxwx"] - Wx * Wx) + (m["wywy"] - Wy * Wy)) / re
    out["pressure_dilatation"] = m["pd"] - P * (Ux + Wy)
    valid = valid_cells(fluid)
    two_dx = 2.0 * dx
    out["convection"] = -(U * _ddx(k, two_dx) + W * _ddy(k, two_dx))
    out["turbulent_transport"] = -(_ddx(0.5 * (uuu + wwu), two_dx) + _ddy(0.5 * (uuw + www), two_dx))
    out["pressure_diffusion"] = -(_ddx(pu, two_dx) + _ddy(pw, two_dx))
    out["viscous_diffusion"] = _laplacian(k, dx) / re
    for name in ("convection", "turbulent_transport", "pressure_diffusion", "viscous_diffusion"):
        out[name] = np.where(valid, out[name], 0.0)
    for name, a in out.items():
        if name not in ("convection", "turbulent_transport", "pressure_diffusion", "viscous_diffusion"):
            out[name] = np.where(fluid, a, 0.0)
    out["residual"] = np.where(valid, out["convection"] + out["production"] - out["dissipation"] + out["turbulent_transport"]
                               + out["pressure_diffusion"] + out["pressure_dilatation"] + out["viscous_diffusion"], 0.0)
    out["totals"] = {name: float(out[name][valid].sum() * dx * dx) for name in TERMS}
    out["fluid"], out["valid"] = fluid, valid
    return out


def momentum_balance(out, dx, re):
    """The terms of the mean momentum equation from what derive_budget returned -> {"u": {...}, "w": {...}}, per component float64 (Nx, Ny)
    arrays on `valid` (0 elsewhere): "convection" -(U dx U_i + W dy U_i) with the accumulated mean gradients, "pressure_gradient" -d_i P,
    "viscous" (1 / re) (5-point Laplacian of U_i) / dx^2, "reynolds_stress" -(dx <u_i'u'> + dy <u_i'w'>), and "residual", their sum: what
    the scheme, the confinement, the limit and the unconverged pressure add to the mean momentum of a statistically steady flow."""
    dx, re = float(dx), float(re)
    two_dx = 2.0 * dx
    valid = out["valid"]
    U, W, P = out["U"], out["W"], out["P"]
    res = {}
    for name, Ui, gx, gy, sx, sy, dp in (("u", U, out["Ux"], out["Uy"], out["uu"], out["uw"], _ddx), ("w", W, out["Wx"], out["Wy"], out["uw"], out["ww"], _ddy)):
        t = {"convection": -(U * gx + W * gy), "pressure_gradient": -dp(P, two_dx), "viscous": _laplacian(Ui, dx) / re,
             "reynolds_stress": -(_ddx(sx, two_dx) + _ddy(sy, two_dx))}
        t = {k: np.where(valid, a, 0.0) for k, a in t.items()}
        t["residual"] = t["convection"] + t["pressure_gradient"] + t["viscous"] + t["reynolds_stress"]
        res[name] = t
    return res


def budget_result(sums, samples, sample_steps, box, fluid, dx, re):
    """The dict budget() / budget_sample() return: derive_budget's arrays - every one of DERIVED and TERMS, zeros while samples == 0 - and
    "samples", "sample_steps", "box", "dx", "re" and the raw "sums"."""
    sums = np.asarray(sums, np.float64)
    fluid = np.asarray(fluid, bool)
    if int(samples) > 0:
        out = derive_budget(sums, samples, fluid, dx, re)
    else:
        out = {"fluid": fluid, "valid": valid_cells(fluid), "totals": {name: 0.0 for name in TERMS}}
        out.update({name: np.zeros(fluid.shape, np.float64) for name in DERIVED + TERMS})
    out.update(samples=int(samples), sample_steps=sample_steps, box=tuple(box), dx=float(dx), re=float(re), sums=sums)
    return out


class Budget(CountedRider):
    """The accumulated kinetic-energy budget of a FluidSimulator (start_budget): the device planes and their parameters.
    held(z) -> (box, every, start), or None."""
    kind, payload, noun = "budget", "sums", "budget"
    params = (BOX,)

    def __init__(self, dev, budget, fluid, re):
        super().__init__(dev, budget, budget.every, budget.start)
        self.budget, self.fluid, self.re = budget, np.asarray(fluid, bool), float(re)

    def attached(self):
        return (tuple(self.budget.box),)

    def launch(self, sim):
        v, p = sim._solver.get_fields()[:2]
        self.dev.budget_launch(self.budget, v, p)

    def data(self):
        sums, _, samples = self.dev.budget_read(self.budget)
        return budget_result(sums, samples, self.sample_steps(samples), self.budget.box, self.fluid, self.budget.dx, self.re)
