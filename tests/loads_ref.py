"""NumPy float64 restatement of the body surface loads (include/fs_hip.h fs_loads_*, csrc/fs_loads.h): one sample as a plain loop over the
faces, every operation one IEEE double operation in the order the header states, the sampling rule, and the worst-case rounding bound of
a record.  Shared by tests/test_loads_cpu.py, tests/loads_standin.py, tests/test_gpu_loads.py and tests/test_cli_loads.py."""
import numpy as np

MID = ((0.0, 0.5), (1.0, 0.5), (0.5, 0.0), (0.5, 1.0))        # face midpoint - (x, y) per dir
NREC, NSUM = 6, 4


def samples(n, start, every):
    """Launch n (from 0) samples."""
    return n + 1 > start and (n + 1 - start) % every == 0


def limit_pair(u, w, limit, t):
    """limit_field's per-cell function in the field's precision t (csrc/fs_kernels.h limit_cell)."""
    lim = t(limit)
    nrm = np.sqrt(u * u + w * w)
    if nrm > lim:
        return lim * (u / nrm), lim * (w / nrm)
    return u, w


def sample_ref(sums, v, p, faces, centre, dx, inv_re, limit=None, y_off=0):
    """Add one sample to sums (4, F) in place -> (record (6,), scale (6,): the sum of |face terms| of each entry).  v (X, Y, 2), p (X, Y)
    in the fields' precision; y_off: row of v / p that holds global row 0 (slab arrays)."""
    cx, cy = float(centre[0]), float(centre[1])
    dx, inv_re = float(dx), float(inv_re)
    t = v.dtype.type
    rec, scale = np.zeros(NREC), np.zeros(NREC)
    for k, (x, y, d) in enumerate(np.asarray(faces).tolist()):
        ax = ((x + MID[d][0]) - cx) * dx
        ay = ((y + MID[d][1]) - cy) * dx
        pk = float(p[x, y - y_off])
        u, w = v[x, y - y_off, 0], v[x, y - y_off, 1]
        if limit is not None and limit > 0.0:
            u, w = limit_pair(u, w, limit, t)
        ut = float(w) if d < 2 else float(u)
        tv = inv_re * ut
        tk = tv / dx
        sums[0, k] += pk
        sums[1, k] += pk * pk
        sums[2, k] += tk
        sums[3, k] += tk * tk
        tp = pk * dx
        fpx, fpy = ((-tp, 0.0), (tp, 0.0), (0.0, -tp), (0.0, tp))[d]
        fvx, fvy = (0.0, tv) if d < 2 else (tv, 0.0)
        mp = ax * fpy - ay * fpx
        mv = ax * fvy - ay * fvx
        terms = (fpx, fpy, fvx, fvy, mp, mv)
        for c in range(NREC):
            rec[c] += terms[c]
            scale[c] += abs(terms[c])
    return rec, scale


def record_bound(nfaces, scale):
    """|computed - exact| of a sum of F terms in ANY order is at most (F - 1) u sum|t| (1 + O(F u)), u = 2^-53; a term is at most three
    rounded operations (a product, a product, a difference; the arms one more each).  Two summations can therefore differ by
    (F + 4) 2^-52 sum|t| at the most."""
    return (nfaces + 4) * 2.0 ** -52 * np.asarray(scale, np.float64)


# ---- manufactured fields for the sign conventions; every value is exact in float32 (powers of two and small multiples) -----------------------
DX, RE, G, U, OMEGA = 2.0 ** -6, 128.0, 4.0, 0.5, 0.25


def manufactured(mask, box, dtype=np.float32):
    """[(name, v, p, check(record dict, bound dict))] for a mask with ONE rectangular body in `box`; shared by the CPU and the GPU test."""
    from fs.history import body_faces
    X, Y = mask.shape
    x0, y0, x1, y1 = box
    w, h = x1 - x0, y1 - y0
    faces = body_faces(mask, box)
    n23 = int(np.sum(faces[:, 2] >= 2))
    cx, cy = x0 + 0.5 * w, y0 + 0.5 * h
    i, j = np.meshgrid(np.arange(X) + 0.5, np.arange(Y) + 0.5, indexing="ij")
    zero_v, zero_p = np.zeros((X, Y, 2), dtype), np.zeros((X, Y), dtype)
    cases = []

    def near(r, b, key, exp):
        assert abs(r[key] - exp) <= b[key], (key, r[key], exp, b[key])

    def gradient(r, b):
        near(r, b, "pressure_x", -G * DX * DX * (w + 1) * h)
        near(r, b, "pressure_y", 0.0)
        near(r, b, "viscous_x", 0.0)
        near(r, b, "viscous_y", 0.0)
    cases.append(("gradient", zero_v, (G * i * DX).astype(dtype), gradient))

    def uniform_p(r, b):
        for key in ("pressure_x", "pressure_y", "moment_pressure"):
            near(r, b, key, 0.0)
    cases.append(("uniform_p", zero_v, np.full((X, Y), 3.0, dtype), uniform_p))

    def uniform_u(r, b):
        near(r, b, "viscous_x", n23 * U / RE)
        near(r, b, "viscous_y", 0.0)
        near(r, b, "pressure_x", 0.0)
        near(r, b, "moment_viscous", 0.0)       # (top and bottom friction pull the same way: their moments about the centroid cancel)
    vu = zero_v.copy()
    vu[..., 0] = U
    cases.append(("uniform_u", vu, zero_p, uniform_u))

    def rotation(r, b):
        assert r["moment_viscous"] > b["moment_viscous"] >= 0.0, r["moment_viscous"]
        near(r, b, "viscous_x", 0.0)
        near(r, b, "viscous_y", 0.0)
    vr = np.stack([-OMEGA * (j - cy), OMEGA * (i - cx)], axis=2).astype(dtype)
    cases.append(("rotation", vr, zero_p, rotation))
    return faces, (cx, cy), cases
