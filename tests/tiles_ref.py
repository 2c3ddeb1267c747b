"""NumPy / Python restatement of the launch-list layer (csrc/fs_tiles.h), written from the text of tile_list() and of fs_upload_mask's activity
loop as they stood before the builder became a header of its own: the scene's activity maps, the launch geometry of ov_grid, and the whole list
builder - which workgroups are listed with which hint bits, masked-first ordering, balancing over the 8 XCDs, interleaving.

Everything is indexed as the library does: mask and bcmap in host layout (X, Y), activity maps [wave column][local row], lists as uint32 words
[k * 8 + xcd] padded with 0xffffffff.  Plain loops over tiles on purpose - this file is the thing the C++ is compared with, not a fast path."""
import numpy as np

PAD = 0xFFFFFFFF
PAIR, PAIR_WIDE, QUAD = 2, 3, 4                      # `lanes`: 60 owner lanes x 2 cells, 62 x 2, 62 x 4
ALL, PLAIN, BOUNDARY, MIXED = 0, 1, 2, 3             # `cls`
WORK, NONFLUID, FLUID = 1, 2, 4                      # activity bits


def cells(lanes):
    return 4 if lanes == QUAD else 2


def owners(lanes):
    return 60 if lanes == PAIR else 62


WIDTH = {QUAD: 248, PAIR: 120, PAIR_WIDE: 124}       # cells per wave column
HALO = {QUAD: 4, PAIR: 4, PAIR_WIDE: 2}              # cells per side that the halo lanes re-read from the neighbouring wave column


def waves(X, lanes):
    return (X // cells(lanes) + owners(lanes) - 1) // owners(lanes)


def activity(mask, bcmap, lanes, rows=None, g0=0):
    """[wave column][local row]: bit 0 - an own cell that is not deep wall (mask != 1 or a bcmap byte); bit 1 - a cell that is not fluid, or a
    row outside the domain; bit 2 - a fluid cell; bits 1 and 2 over the own cells AND the cells the halo lanes cover."""
    X, Y = mask.shape
    rows = Y if rows is None else rows
    w, halo = WIDTH[lanes], HALO[lanes]
    n = (X + w - 1) // w
    j = g0 + np.arange(rows)
    inside = (j >= 0) & (j < Y)
    jc = np.clip(j, 0, Y - 1)
    m, b = mask[:, jc], bcmap[:, jc]
    nf = np.where(inside[None, :], np.where(m != 0, NONFLUID, FLUID), NONFLUID).astype(np.uint8)
    own = np.where(inside[None, :], (m != 1) | (b != 0), False).astype(np.uint8) | nf
    act = np.zeros((n, rows), np.uint8)
    for i in range(X):
        c, r = divmod(i, w)
        act[c] |= own[i]
        if r < halo and c > 0:
            act[c - 1] |= nf[i]
        elif r >= w - halo and c + 1 < n:
            act[c + 1] |= nf[i]
    return act


def launch_geometry(X, lanes, rt, wgw, stacked, jb, je):
    """(nbx, nby, group) of the dense grid (fs_launch.h ov_grid): blocks across, block rows, block rows per XCD group."""
    nw, tiles = waves(X, lanes), (je - jb + rt - 1) // rt
    stacked = stacked and wgw > 1
    nbx = nw if stacked else (nw + wgw - 1) // wgw
    nby = (tiles + wgw - 1) // wgw if stacked else tiles
    group = max(1, 8 // wgw) if stacked else 8
    return nbx, nby, group


def spec_ok(rows, lanes, rt, wgw, cls, parent_rt, nbx, nby):
    if parent_rt == rt:
        parent_rt = 0
    if nbx > 0xFFF or nby > 0xFFFF or lanes > 4 or rows > 0xFFFF:
        return False
    if parent_rt and (wgw != 1 or parent_rt % rt != 0 or parent_rt > 64):
        return False
    if cls == MIXED and not (rt == 8 and parent_rt == 16 and wgw == 1 and lanes == PAIR):
        return False
    return True


def build(act, X, lanes, rt, wgw, stacked, group, cls, reach, parent_rt, jb, je, nbx, nby):
    """-> (words uint32 [per_xcd * 8], per_xcd, count, needed); words is empty when the dense grid needs no list."""
    if parent_rt == rt:
        parent_rt = 0
    nw, Y = waves(X, lanes), act.shape[1]
    per = [[] for _ in range(8)]
    any_hint = False

    def plain_box(wx0, wx1, p0, p1):
        if wx0 <= 0 or wx1 >= nw or p0 - reach < 0 or p1 + reach > Y:
            return False
        return not (act[wx0:wx1, p0 - reach:p1 + reach] & NONFLUID).any()

    groups = (nby + group - 1) // group
    for xcd in range(8):
        lg = 0
        while lg * 8 + xcd < groups:
            for o in range(group * nbx):
                ly, bx = o % group, o // group
                by = (lg * 8 + xcd) * group + ly
                if by >= nby:
                    continue
                wx0 = bx if stacked else bx * wgw
                wx1 = min(nw, bx + 1 if stacked else bx * wgw + wgw)
                j0 = jb + (by * wgw if stacked else by) * rt
                j1 = min(je, jb + ((by * wgw + wgw) if stacked else by + 1) * rt)
                work = bool((act[wx0:wx1, j0:j1] & WORK).any())
                if cls == MIXED:
                    p0 = jb + (j0 - jb) // parent_rt * parent_rt
                    p1 = min(je, p0 + parent_rt)
                    if p1 - p0 == parent_rt and plain_box(wx0, wx1, p0, p1):
                        if j0 == p0:
                            per[xcd].append((1 << 28) | (by << 12) | bx)
                    elif work:
                        h = 0
                        for s in range(2):
                            if (act[bx, j0 + 4 * s:min(j1, j0 + 4 * s + 4)] & FLUID).any():
                                h |= 2 << s
                        per[xcd].append((h << 28) | (by << 12) | bx)
                    any_hint = True
                    continue
                if work and cls:
                    p0, p1, full = j0, j1, (wgw if stacked else 1) * rt
                    if parent_rt:
                        p0 = jb + (j0 - jb) // parent_rt * parent_rt
                        p1 = min(je, p0 + parent_rt)
                        full = parent_rt
                    work = (p1 - p0 == full and plain_box(wx0, wx1, p0, p1)) == (cls == PLAIN)
                hints = 0
                if work and not cls and reach > 0 and wgw <= 4:
                    for w in range(wgw):
                        wx = bx if stacked else bx * wgw + w
                        t0 = jb + ((by * wgw + w) if stacked else by) * rt
                        t1 = min(je, t0 + rt)
                        if wx >= nw or t0 >= je:
                            continue
                        if plain_box(wx, wx + 1, t0, t1):
                            hints |= 1 << w
                    any_hint = any_hint or hints != 0
                if work and cls == BOUNDARY and wgw == 1:
                    if (act[bx, j0:j1] & FLUID).any():
                        hints |= 2
                if work:
                    per[xcd].append((hints << 28) | (by << 12) | bx)
            lg += 1
    if (not cls or cls == MIXED) and any_hint and wgw == 1:      # masked first
        per = [[e for e in v if (e >> 28) & 1 == 0] + [e for e in v if (e >> 28) & 1] for v in per]
    total = sum(len(v) for v in per)
    if total >= 64:                                               # balance over the XCDs
        target = (total + 7) // 8
        for d in range(8):
            while len(per[d]) > target:
                r = min(range(8), key=lambda x: (len(per[x]), x))
                if len(per[r]) >= target:
                    break
                n = min(len(per[d]) - target, target - len(per[r]))
                per[r] += per[d][len(per[d]) - n:]
                per[d] = per[d][:len(per[d]) - n]
    K = max(len(v) for v in per)
    needed = K > 0 and bool(cls or any_hint or total < nbx * nby)
    if not needed:
        return np.zeros(0, np.uint32), 0, 0, False
    words = np.full(K * 8, PAD, np.uint32)
    for xcd in range(8):
        words[xcd:len(per[xcd]) * 8:8] = per[xcd]
    return words, K, total, True
