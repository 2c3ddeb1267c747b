"""NumPy restatement of the field distributions (csrc/fs_dist.h, include/fs_hip.h fs_dist_*): the value of a cell through the restatement
of the vortex identification (tests/vortex_ref.py gradient / criterion / limited), the bin rule, the tables and the order statistics (np.sort
of the selected values that are not NaN).  Arrays are (X, Y) like every host array of the product: cell (i, j) at [i, j]."""
import numpy as np
import vortex_ref as R

QUANTITIES = ("u", "w", "p", "speed", "vorticity", "q", "swirl")
BELOW, ABOVE, NAN = -1, -2, -3
MAX_BINS, MAX_CHANNELS, MAX_RANKS = 4096, 4, 8


def values(quantity, v, p, mask, dx, limit=None):
    """float64 (X, Y): the value of every cell (meaningful on the fluid cells), every operation rounded on its own."""
    with np.errstate(all="ignore"):
        if quantity in ("u", "w", "speed"):
            lv = R.limited(v, limit)
            u, w = lv[..., 0].astype(np.float64), lv[..., 1].astype(np.float64)
            if quantity == "u":
                return u
            if quantity == "w":
                return w
            t = u * u
            t = t + w * w
            return np.sqrt(t)
        if quantity == "p":
            return np.asarray(p).astype(np.float64)
        if quantity == "vorticity":
            return R.gradient(v, dx, limit)[4]
        if quantity in ("q", "swirl"):
            return R.criterion(quantity, v, mask, dx, limit)[0]      # (0 on the cells that are not fluid: never selected)
    raise ValueError(quantity)


def selection(mask, box=None):
    """bool (X, Y): the fluid cells inside the half-open box."""
    mask = np.asarray(mask)
    sel = mask == 0
    if box is not None:
        inside = np.zeros(mask.shape, bool)
        inside[box[0]:box[2], box[1]:box[3]] = True
        sel &= inside
    return sel


def bins_of(x, lo, hi, B):
    """int64 array: the bin of every value - BELOW, ABOVE or NAN for a value without one.  inv = B / (hi - lo) in double; x itself is
    compared with lo and hi, floor((x - lo) * inv) is clamped to B - 1."""
    x = np.asarray(x, np.float64)
    inv = np.float64(B) / (np.float64(hi) - np.float64(lo))
    with np.errstate(all="ignore"):
        s = np.floor((x - np.float64(lo)) * inv)
    inr = ~np.isnan(x) & (x >= lo) & (x < hi)
    b = np.where(inr, np.minimum(np.where(inr, s, 0.0), B - 1), 0.0).astype(np.int64)
    return np.where(np.isnan(x), NAN, np.where(x < lo, BELOW, np.where(x >= hi, ABOVE, b)))


def histogram(x, lo, hi, B):
    """The table of the values x (any shape; the selected ones) -> {"counts": int64 (B,), "below", "above", "nan"}."""
    b = bins_of(np.ravel(x), lo, hi, B)
    return {"counts": np.bincount(b[b >= 0], minlength=B).astype(np.int64), "below": int((b == BELOW).sum()), "above": int((b == ABOVE).sum()),
            "nan": int((b == NAN).sum())}


def joint(xa, xb, ra, rb):
    """The joint table of the value pairs; ra, rb = (lo, hi, B) -> {"counts": int64 (Ba, Bb), "outside", "nan"}."""
    ba, bb = bins_of(np.ravel(xa), *ra), bins_of(np.ravel(xb), *rb)
    nan = (ba == NAN) | (bb == NAN)
    out = ~nan & ((ba < 0) | (bb < 0))
    ok = ~nan & ~out
    counts = np.zeros((ra[2], rb[2]), np.int64)
    np.add.at(counts, (ba[ok], bb[ok]), 1)
    return {"counts": counts, "outside": int(out.sum()), "nan": int(nan.sum())}


def field_histogram(quantity, v, p, mask, dx, B, rng, box=None, limit=None):
    return histogram(values(quantity, v, p, mask, dx, limit)[selection(mask, box)], rng[0], rng[1], B)


def field_joint(qa, qb, v, p, mask, dx, ra, rb, box=None, limit=None):
    sel = selection(mask, box)
    return joint(values(qa, v, p, mask, dx, limit)[sel], values(qb, v, p, mask, dx, limit)[sel], ra, rb)


def sorted_values(quantity, v, p, mask, dx, box=None, limit=None):
    """-> (np.sort of the selected values that are not NaN, the number of selected NaN)."""
    x = values(quantity, v, p, mask, dx, limit)[selection(mask, box)]
    nan = np.isnan(x)
    return np.sort(x[~nan]), int(nan.sum())


# ---- the order-preserving key and a radix select in NumPy, driven through a digit pick ----------------------------------------------------------
def keys(x):
    b = np.asarray(x, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b ^ np.uint64(1 << 63))


def unkeys(k):
    k = np.asarray(k, np.uint64)
    return np.where(k >> np.uint64(63), k ^ np.uint64(1 << 63), ~k).view(np.float64)


def digit_geometry(p):
    """(shift, width) of digit p of 6: 11 bits from the top, the last of 9."""
    return (53 - 11 * p, 11) if p < 5 else (0, 9)


def radix_select(x, k, pick):
    """The k-th smallest of x (no NaN) by six passes over the keys; pick(table int64, rank) -> (digit, rank within it)."""
    ks = keys(x)
    prefix, rest = np.uint64(0), int(k)
    for p in range(6):
        shift, width = digit_geometry(p)
        hb = shift + width
        match = np.ones(len(ks), bool) if hb >= 64 else (ks >> np.uint64(hb)) == (prefix >> np.uint64(hb))
        digits = ((ks[match] >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64)
        table = np.bincount(digits, minlength=1 << width).astype(np.int64)
        d, rest = pick(table, rest)
        prefix = prefix | (np.uint64(d) << np.uint64(shift))
    return float(unkeys(np.array([prefix], np.uint64))[0])
