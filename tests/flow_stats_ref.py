"""NumPy f64 restatement of fs_flow_stats (include/fs_hip.h): the 10 slots over the owned rows of a window of the grid.

Every per-cell term is evaluated in double on the stored values, in the order the header states, so it matches the kernel's terms bit
for bit; only the order of the sums differs (the kernel reduces in a tree)."""
import numpy as np

SLOTS = ("fluid_cells", "sum_s2", "sum_om2", "sum_dv2", "max_s2", "max_a", "max_abs_dv", "nonfinite", "force_x", "force_y")
MAX_SLOTS = ("max_s2", "max_a", "max_abs_dv")


def flow_stats_ref(v, p, mask, dx, box=None, rows=None, y0=0):
    """v (X, R, 2), p (X, R), mask (X, R): a window of R rows whose first row is global row y0.  rows = (r0, r1): the owned rows of the
    window (default: all).  Neighbours are clamped at the window's edge - the domain edge, or a ghost row one row beyond the owned ones.
    box = (x0, y0, x1, y1) in global cells or None.  -> {slot: float}."""
    v = np.asarray(v, np.float64)
    p = np.asarray(p, np.float64)
    mask = np.asarray(mask)
    X, R = mask.shape
    r0, r1 = rows if rows is not None else (0, R)
    u, w = v[..., 0], v[..., 1]
    ii, jj = np.arange(X), np.arange(r0, r1)
    il, ir = np.clip(ii - 1, 0, X - 1), np.clip(ii + 1, 0, X - 1)
    jm, jp = np.clip(jj - 1, 0, R - 1), np.clip(jj + 1, 0, R - 1)
    uc, wc, pc, m = u[:, r0:r1], w[:, r0:r1], p[:, r0:r1], mask[:, r0:r1]
    two_dx = 2.0 * dx
    out = dict.fromkeys(SLOTS, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        om = ((w[ir][:, jj] - w[il][:, jj]) - (u[:, jp] - u[:, jm])) / two_dx
        dv = ((u[ir][:, jj] - u[il][:, jj]) + (w[:, jp] - w[:, jm])) / two_dx
        s2 = uc * uc + wc * wc
        a = np.abs(uc) + np.abs(wc)
        F = m == 0
        out["fluid_cells"] = float(F.sum())
        out["sum_s2"] = float(s2[F].sum())
        out["sum_om2"] = float((om[F] * om[F]).sum())
        out["sum_dv2"] = float((dv[F] * dv[F]).sum())
        out["max_s2"] = float(np.max(s2[F], initial=0.0))          # (np.max propagates NaN, like the kernel)
        out["max_a"] = float(np.max(a[F], initial=0.0))
        out["max_abs_dv"] = float(np.max(np.abs(dv[F]), initial=0.0))
        bad = ~np.isfinite(uc) | ~np.isfinite(wc) | ~np.isfinite(pc)
        out["nonfinite"] = float((bad & (m != 1)).sum())
        if box is not None:
            x0, by0, x1, by1 = box
            gy = y0 + jj
            inbox = (m == 1) & ((ii >= x0) & (ii < x1))[:, None] & ((gy >= by0) & (gy < by1))[None, :]
            fx = fy = scale = 0.0
            for di, dj, sign, comp in ((1, 0, -1.0, "x"), (-1, 0, 1.0, "x"), (0, 1, -1.0, "y"), (0, -1, 1.0, "y")):
                ni, nj = ii + di, jj + dj
                okx, oky = (ni >= 0) & (ni < X), (nj >= 0) & (nj < R)       # neighbours beyond the edge do not exist (no clamping)
                ni_c, nj_c = np.clip(ni, 0, X - 1), np.clip(nj, 0, R - 1)
                fluid = (mask[ni_c][:, nj_c] == 0) & okx[:, None] & oky[None, :]
                terms = p[ni_c][:, nj_c][inbox & fluid] * dx
                term = float(terms.sum())
                scale += float(np.abs(terms).sum())
                if comp == "x":
                    fx += sign * term
                else:
                    fy += sign * term
            out["force_x"], out["force_y"] = fx, fy
            out["_force_scale"] = scale        # (not a slot: the size of the terms, for comparing sums that cancel)
    return out


def compare(got, exp, rel=1e-12):
    """Differences between two slot dicts: sums to relative `rel`, maxima and counts exactly (NaN == NaN) -> list of messages."""
    bad = []
    for k in SLOTS:
        g, e = float(got[k]), float(exp[k])
        if k in MAX_SLOTS or k in ("fluid_cells", "nonfinite"):
            ok = (g == e) or (g != g and e != e)
        else:
            scale = max(abs(e), float(exp.get("_force_scale", 0.0)) if k.startswith("force") else 0.0, 1e-300)
            ok = (g != g and e != e) or g == e or abs(g - e) <= rel * scale
        if not ok:
            bad.append(f"{k}: {g!r} != {e!r}")
    return bad
