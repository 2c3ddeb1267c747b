"""Error behaviour of the C-ABI through the Python shell: every misuse is a negative status + message (FsError), never a
crash or a silent no-op.  (The reference raises plain Python exceptions only for unknown scheme / scene.)"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dev(hip_lib):
    import fs
    from fs.boundary_condition import BoundaryCondition
    fs.runtime.init(gpu=0, dtype="f32")
    mask = np.zeros((32, 16), np.uint8); mask[:, :2] = 1; mask[:, -2:] = 1
    bc = BoundaryCondition(np.zeros((32, 16, 2), np.float32), mask)
    yield bc.device
    bc.device.close()


def test_wrong_channel_count_and_aliasing(dev):
    from fs._lib import FsError
    v, p, d = dev.alloc(2), dev.alloc(1), dev.alloc(3)
    with pytest.raises(FsError, match="channel count"):
        dev.jacobi_sweep(0.01, 0.1, v, p, v)                # pn must be 1-channel
    with pytest.raises(FsError, match="alias"):
        dev.cip_nonadv(0.01, 0.1, 100.0, v, v, p)           # fn == fc
    with pytest.raises(FsError, match="distinct"):
        dev.jacobi_sweep(0.01, 0.1, p, p, v)
    with pytest.raises(FsError):
        dev.mac_update(7, 0.01, 0.1, 100.0, dev.alloc(2), v, p)   # unknown scheme code
    with pytest.raises(FsError, match="bc_dye"):
        dev.dye_bc(d)                                        # no dye scene uploaded


def test_row_range_and_foreign_field(dev, hip_lib):
    import fs
    from fs import _lib
    from fs.boundary_condition import BoundaryCondition
    v = dev.alloc(2)
    assert hip_lib.fs_limit_field(dev._ctx, 10.0, v._h, 0, 17) < 0           # 17 > rows
    assert b"row range" in hip_lib.fs_last_error()
    other = BoundaryCondition(np.zeros((32, 16, 2), np.float32), np.ones((32, 16), np.uint8)).device
    try:
        assert hip_lib.fs_limit_field(dev._ctx, 10.0, other.alloc(2)._h, 0, 16) < 0
        assert b"another context" in hip_lib.fs_last_error()
    finally:
        other.close()
    with pytest.raises(ValueError, match="expected array of shape"):
        v.from_numpy(np.zeros((16, 32, 2), np.float32))


def test_kernel_before_mask_upload(hip_lib):
    from fs import _lib
    ctx = ctypes.c_void_p()
    _lib.call("fs_create", ctypes.byref(ctx), 0, 32, 16, 0, 0, 16, 0)
    f = ctypes.c_void_p()
    _lib.call("fs_field_alloc", ctx, 2, ctypes.byref(f))
    assert hip_lib.fs_limit_field(ctx, 10.0, f, 0, 16) == -3                 # FS_ERR_STATE
    assert b"mask not uploaded" in hip_lib.fs_last_error()
    assert hip_lib.fs_create(ctypes.byref(ctypes.c_void_p()), 0, 2, 2, 0, 0, 2, 0) == -1     # grid too small
    assert hip_lib.fs_create(ctypes.byref(ctypes.c_void_p()), 0, 32, 16, 5, 0, 16, 0) == -1    # bad dtype
    hip_lib.fs_destroy(ctx)


def test_exchange_misuse(dev, hip_lib):
    """Ghost-row exchange entry points without a communicator, and the begin / wait protocol on a 1-rank communicator."""
    import os
    from fs import _lib
    from fs._lib import FsError
    v = dev.alloc(2)
    arr = (ctypes.c_void_p * 1)(v._h)
    for name, args in (("fs_halo_exchange_multi", (arr, 1, 0)), ("fs_halo_exchange_begin", (arr, 1, 0)),
                       ("fs_halo_exchange_self", (arr, 1, 0))):
        with pytest.raises(FsError, match="fs_comm_init"):
            _lib.call(name, dev._ctx, *args)
    with pytest.raises(FsError, match="fs_comm_init"):
        _lib.call("fs_halo_exchange_mark", dev._ctx)
    _lib.call("fs_halo_exchange_wait", dev._ctx)                      # nothing in flight: a no-op, not an error
    with pytest.raises(FsError, match="communicator"):
        _lib.call("fs_comm_loopback", dev._ctx, 1)
    # 1-rank communicator: protocol errors
    uid = ctypes.create_string_buffer(128)
    _lib.call("fs_comm_unique_id", uid)
    saved = os.dup(1); os.dup2(2, 1)
    try:
        _lib.call("fs_comm_init", dev._ctx, 0, 1, ctypes.c_char_p(uid.raw))
    finally:
        ctypes.CDLL(None).fflush(None); os.dup2(saved, 1); os.close(saved)
    with pytest.raises(FsError, match="already initialised"):
        _lib.call("fs_comm_init", dev._ctx, 0, 1, ctypes.c_char_p(uid.raw))
    with pytest.raises(FsError, match="depth"):
        _lib.call("fs_halo_exchange_begin", dev._ctx, arr, 1, 1)      # this context has no ghost rows (halo 0)
    _lib.call("fs_halo_exchange_begin", dev._ctx, arr, 1, 0)
    with pytest.raises(FsError, match="in flight"):
        _lib.call("fs_halo_exchange_begin", dev._ctx, arr, 1, 0)
    with pytest.raises(FsError, match="in flight"):
        _lib.call("fs_halo_exchange_mark", dev._ctx)
    _lib.call("fs_halo_exchange_wait", dev._ctx)
    neg = (ctypes.c_int * 1)(-1)
    with pytest.raises(FsError, match="negative"):
        _lib.call("fs_halo_exchange_begin_partial", dev._ctx, arr, neg, 1, 0)
    _lib.load().fs_comm_destroy(dev._ctx)


def test_box_probes_give_plausible_rates_and_refuse_nonsense(dev):
    """The three probes bench.py runs before its timed region (include/fs_hip.h fs_box_rates, fs_box_valu_rate, fs_box_mixed_rate): on an
    MI355X a float4 stream moves TB/s, a SIMD issues tenths of a G wave-instruction per second; a zero budget / a buffer below 1 MiB is an error."""
    from fs._lib import FsError
    rd, cp = dev.box_rates(64 << 20, 5.0)
    assert 500.0 < rd < 20000.0 and 500.0 < cp < 20000.0
    assert 0.05 < dev.box_valu_rate(5.0) < 5.0
    assert 500.0 < dev.box_mixed_rate(64 << 20, 5.0) < 20000.0
    with pytest.raises(FsError):
        dev.box_rates(1024, 5.0)
    with pytest.raises(FsError):
        dev.box_valu_rate(0.0)
    with pytest.raises(FsError):
        dev.box_mixed_rate(64 << 20, -1.0)


# ---- the multigrid entry points (include/fs_hip.h fs_mg_*) ---------------------------------------------------------------------------------
MG_DT, MG_DX = 0.05 / 32, 1.0 / 32


@pytest.fixture()
def mg(hip_lib):
    """A 32 x 16 context with a random mask -> (bc, a function that runs one valid multigrid update on it and compares it with the restatement)."""
    import fs
    import multigrid_ref as M
    from fs.boundary_condition import BoundaryCondition
    from fs.double_buffer import DoubleBuffer
    from oracle import oracle as O
    from test_gpu_random_masks import _random_scene
    fs.runtime.init(gpu=0, dtype="f32")
    rng = np.random.default_rng(3216)
    const, mask, _ = _random_scene(rng, 32, 16, 0.15, 0.03)
    pc, pn = (rng.uniform(-1, 1, (32, 16)).astype(np.float32) for _ in range(2))
    v = rng.uniform(-1, 1, (32, 16, 2)).astype(np.float32)
    exp = O.Buf2(pc.shape, 1, pc.dtype)
    exp.current[...], exp.next[...] = pc, pn
    M.MultigridRef(O.OracleBC(const, mask, None, np.float32), MG_DT, MG_DX).update(exp, v.copy())
    assert np.isfinite(exp.current).all() and not np.array_equal(exp.current, pc)
    bc = BoundaryCondition(const, mask)
    p, vf = DoubleBuffer((32, 16), 1, bc.device), bc.device.alloc(2)

    def still_usable():
        pu = fs.MultigridPressureUpdater(bc, MG_DT, MG_DX)
        p.current.from_numpy(pc); p.next.from_numpy(pn); vf.from_numpy(v)
        pu.update(p, vf)
        assert np.array_equal(p.current.to_numpy(), exp.current) and np.array_equal(p.next.to_numpy(), exp.next), "the context no longer computes the restatement's update"
        bc.device.mg_free(pu._mg)
        pu._mg = None

    yield bc, still_usable
    bc.device.close()


def test_mg_cycle_misuse(mg, hip_lib):
    """One pressure buffer given twice, a hierarchy used on another context, a hierarchy used after fs_mg_free (a stale handle is only ever
    looked up in the context's set of live hierarchies, never read)."""
    import fs
    from fs._lib import FsError
    from fs.boundary_condition import BoundaryCondition
    bc, still_usable = mg
    dev = bc.device
    pu = fs.MultigridPressureUpdater(bc, MG_DT, MG_DX)
    p, q, v = dev.alloc(1), dev.alloc(1), dev.alloc(2)
    with pytest.raises(FsError, match="distinct pressure buffers"):
        dev.mg_cycle(pu._mg, MG_DT, MG_DX, p, p, v)
    still_usable()
    with pytest.raises(FsError, match="channel count"):
        dev.mg_cycle(pu._mg, MG_DT, MG_DX, p, v, v)
    still_usable()
    other = BoundaryCondition(np.zeros((32, 16, 2), np.float32), np.zeros((32, 16), np.uint8)).device
    try:
        with pytest.raises(FsError, match="another context or freed"):
            other.mg_cycle(pu._mg, MG_DT, MG_DX, other.alloc(1), other.alloc(1), other.alloc(2))
        with pytest.raises(FsError, match="another context or freed"):
            other.mg_info(pu._mg)
        assert hip_lib.fs_mg_free(other._ctx, pu._mg) == -1 and b"another context or freed" in hip_lib.fs_last_error()
    finally:
        other.close()
    assert dev.mg_info(pu._mg)["levels"] == 4              # the refused free on the other context left it alive here
    still_usable()
    stale, pu._mg = pu._mg, None                           # (the updater's finaliser must not free it a second time)
    dev.mg_free(stale)
    with pytest.raises(FsError, match="another context or freed"):
        dev.mg_cycle(stale, MG_DT, MG_DX, p, q, v)
    with pytest.raises(FsError, match="another context or freed"):
        dev.mg_info(stale)
    assert hip_lib.fs_mg_free(dev._ctx, stale) == -1 and b"another context or freed" in hip_lib.fs_last_error()
    assert hip_lib.fs_mg_free(dev._ctx, None) == 0         # a null handle: nothing to free
    still_usable()


def test_mg_create_refuses_bad_hierarchies(mg, hip_lib):
    from fs import _lib
    from fs._lib import FsError
    from fs.multigrid import build_hierarchy
    bc, still_usable = mg
    dev = bc.device
    good = build_hierarchy(bc.mask, np.float32)
    assert [lv[0].shape for lv in good] == [(16, 8), (8, 4), (4, 2), (2, 1)]

    def level(nx, ny):
        return tuple(np.ones((nx, ny), np.float32) for _ in range(3))

    one = np.ones(1, np.float32).ctypes.data_as(ctypes.c_void_p)
    with pytest.raises(FsError, match="nlevels"):          # (Device.mg_create cannot flatten an empty list: the entry point itself)
        _lib.call("fs_mg_create", dev._ctx, 0, (ctypes.c_int * 2)(16, 8), one, one, one, -1, 2, 64, ctypes.byref(ctypes.c_void_p()))
    still_usable()
    for levels, tail, sweeps, msg in (([level(1, 1)] * 25, -1, (2, 64), "nlevels"),
                                      (good, -1, (-1, 64), "sweep counts"),
                                      (good, -1, (2, -1), "sweep counts"),
                                      (good[1:], -1, (2, 64), "level 1 must be half the grid"),
                                      ([good[0], level(4, 4)], -1, (2, 64), "half the level above"),
                                      ([good[0], good[1], level(4, 1)], 0, (2, 64), "half the level above")):
        with pytest.raises(FsError, match=msg):
            dev.mg_create(levels, tail, *sweeps)
        still_usable()


def test_mg_create_inside_a_capture_is_a_state_error(mg):
    from fs._lib import FsError
    from fs.multigrid import build_hierarchy
    bc, still_usable = mg
    dev = bc.device
    good = build_hierarchy(bc.mask, np.float32)
    p = dev.alloc(1)
    seen = []

    def body():
        dev.pressure_bc(p)
        with pytest.raises(FsError, match="status -3: multigrid create during graph capture") as e:
            dev.mg_create(good, -1, 2, 64)
        seen.append(e)
        dev.pressure_bc(p)

    gid = dev.capture(body)                                # the refusal left the capture intact
    assert seen
    dev.replay(gid)
    dev.free_graph(gid)
    still_usable()


def test_mg_constructor_refuses_an_odd_grid(hip_lib):
    import fs
    from fs.boundary_condition import BoundaryCondition
    from fs.double_buffer import DoubleBuffer
    from oracle import oracle as O
    fs.runtime.init(gpu=0, dtype="f32")
    rng = np.random.default_rng(3316)
    mask = (rng.random((33, 16)) < 0.15).astype(np.uint8)
    const = np.zeros((33, 16, 2), np.float32)
    bc = BoundaryCondition(const, mask)
    try:
        with pytest.raises(ValueError, match="even grid extents"):
            fs.MultigridPressureUpdater(bc, MG_DT, MG_DX)
        with pytest.raises(ValueError, match=">= 0"):
            fs.MultigridPressureUpdater(bc, MG_DT, MG_DX, coarse_sweeps=-1)
        # no multigrid on this grid; the context still runs the red-black updater as the oracle does
        pc = rng.uniform(-1, 1, (33, 16)).astype(np.float32)
        v = rng.uniform(-1, 1, (33, 16, 2)).astype(np.float32)
        exp = O.Buf2(pc.shape, 1, pc.dtype)
        exp.current[...] = pc
        O.OracleRedBlackSor(O.OracleBC(const, mask, None, np.float32), MG_DT, MG_DX, 1.3, 2).update(exp, v.copy())
        p, vf = DoubleBuffer((33, 16), 1, bc.device), bc.device.alloc(2)
        p.current.from_numpy(pc); vf.from_numpy(v)
        fs.RedBlackSorPressureUpdater(bc, MG_DT, MG_DX, 1.3, 2).update(p, vf)
        assert np.array_equal(p.current.to_numpy(), exp.current)
    finally:
        bc.device.close()


# ---- the nine kinds of device object behind one registry, one handle check and one free (csrc/fs_objects.h, fs_host.h) -------------------------
# Straight through the C-ABI: the Python layer nulls a handle it has released (RideOps._release), so a stale one never gets past it.
_LL = ctypes.c_longlong


def _handle(L, name, ctx, *args):
    h = ctypes.c_void_p()
    assert getattr(L, name)(ctx, *args, ctypes.byref(h)) == 0, L.fs_last_error()
    return h


def _mg_create(L, ctx):
    ones = np.ones(16 * 8, np.float32).ctypes.data_as(ctypes.c_void_p)      # one level, half of 32 x 16
    return _handle(L, "fs_mg_create", ctx, 1, (ctypes.c_int * 2)(16, 8), ones, ones, ones, 0, 2, 4)


# kind -> (create(L, ctx) -> handle, the cheapest use(L, ctx, handle) -> status, the free's name, the text of a refused handle)
KINDS = {
    "history": (lambda L, c: _handle(L, "fs_history_create", c, 1, (ctypes.c_int * 2)(5, 5), 0, None, 4, 1),
                lambda L, c, h: L.fs_history_read(c, h, None, 0, ctypes.byref(ctypes.c_int()), None, None),
                "fs_history_free", b"history from another context or freed"),
    "loads": (lambda L, c: _handle(L, "fs_loads_create", c, 1, (ctypes.c_int * 3)(5, 5, 0), (ctypes.c_double * 2)(4.0, 4.0), 4, 1, 0),
              lambda L, c, h: L.fs_loads_reset(c, h), "fs_loads_free", b"loads from another context or freed"),
    "mean": (lambda L, c: _handle(L, "fs_mean_create", c, 1, 0),
             lambda L, c, h: L.fs_mean_reset(c, h), "fs_mean_free", b"mean from another context or freed"),
    "modes": (lambda L, c: _handle(L, "fs_modes_create", c, 1, (ctypes.c_double * 2)(1.0, 0.0), 1, 0),
              lambda L, c, h: L.fs_modes_reset(c, h), "fs_modes_free", b"modes from another context or freed"),
    "pod": (lambda L, c: _handle(L, "fs_pod_create", c, 2, 1, 0),
            lambda L, c, h: L.fs_pod_reset(c, h), "fs_pod_free", b"pod from another context or freed"),
    "vortex": (lambda L, c: _handle(L, "fs_vortex_create", c, 0, 0.0, 1.0, 1, 0, 1, 4, 16, 2),
               lambda L, c, h: L.fs_vortex_read(c, h, None, 0, ctypes.byref(ctypes.c_int()), None, None),
               "fs_vortex_free", b"vortex tracker from another context or freed"),
    "flowmap": (lambda L, c: _handle(L, "fs_flowmap_create", c, (ctypes.c_int * 4)(4, 4, 12, 12), 1),
                lambda L, c, h: L.fs_flowmap_reset(c, h), "fs_flowmap_free", b"flow map from another context or freed"),
    "tracer": (lambda L, c: _handle(L, "fs_tracer_create", c, 1, (ctypes.c_double * 2)(8.0, 8.0), 1, 0),
               lambda L, c, h: L.fs_tracer_order(c, h, (ctypes.c_int * 1)()), "fs_tracer_free", b"tracer set from another context or freed"),
    "mg": (_mg_create, lambda L, c, h: L.fs_mg_info(c, h, *(ctypes.byref(ctypes.c_int()) for _ in range(3))),
           "fs_mg_free", b"multigrid hierarchy from another context or freed"),
}


def _refused(L, status, text):
    return status == -1 and L.fs_last_error() == text


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_object_handle_of_another_context_or_freed(dev, hip_lib, kind):
    """Per kind: a handle of context A used or freed through context B, and used or freed again after its free, is refused with the kind's text
    (FS_ERR_ARG) - by a lookup that never reads through the handle; the refusals leave the object usable on A; a null free is fine."""
    from fs import _lib
    L, a = hip_lib, dev._ctx
    create, use, free_name, text = KINDS[kind]
    free = getattr(L, free_name)
    b = ctypes.c_void_p()
    _lib.call("fs_create", ctypes.byref(b), 0, 32, 16, 0, 0, 16, 0)
    try:
        h = create(L, a)
        assert use(L, a, h) == 0
        assert _refused(L, use(L, b, h), text)
        assert _refused(L, free(b, h), text)
        assert use(L, a, h) == 0                                # the refused free on B left it alive on A
        assert free(a, h) == 0
        assert _refused(L, use(L, a, h), text)                  # stale from here on
        assert _refused(L, free(a, h), text)
        assert _refused(L, use(L, b, h), text)
        assert free(a, None) == 0 and free(b, None) == 0        # a null handle: nothing to free
    finally:
        assert L.fs_destroy(b) == 0


@pytest.mark.parametrize("given, expected", [("mean", "modes"), ("pod", "mean"), ("tracer", "vortex"), ("modes", "pod"), ("mg", "history")])
def test_object_handle_of_another_kind(dev, hip_lib, given, expected):
    """A LIVE handle of one kind where another is expected: refused with the expected kind's text, and still what it was afterwards."""
    L, a = hip_lib, dev._ctx
    create, use, free_name, _ = KINDS[given]
    _, use_as, free_as, text = KINDS[expected]
    h = create(L, a)
    assert _refused(L, use_as(L, a, h), text)
    assert _refused(L, getattr(L, free_as)(a, h), text)
    assert use(L, a, h) == 0
    assert getattr(L, free_name)(a, h) == 0


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_object_free_inside_a_capture(dev, hip_lib, kind):
    """Per kind: *_free inside a hipGraph capture returns 0 and defers the release to the capture's end - the capture stays valid and the graph
    replays - and the handle is stale from the call on.  fs_flowmap_free is the one free that refuses a capture instead (FS_ERR_STATE, as
    tests/test_gpu_lcs.py asserts since the flow maps exist): there the capture stays valid too and the flow map stays live."""
    L, a = hip_lib, dev._ctx
    create, use, free_name, text = KINDS[kind]
    free = getattr(L, free_name)
    h, p = create(L, a), dev.alloc(1)
    seen = []

    def body():
        dev.pressure_bc(p)
        seen.append(free(a, h))
        seen.append(L.fs_last_error())
        dev.pressure_bc(p)

    gid = dev.capture(body)                                     # (fs_graph_end fails on an invalidated capture)
    dev.replay(gid)
    dev.free_graph(gid)
    if kind == "flowmap":
        assert seen == [-3, b"flow map free during graph capture / tape recording"]
        assert use(L, a, h) == 0 and free(a, h) == 0
    else:
        assert seen[0] == 0
    assert _refused(L, use(L, a, h), text)
    assert _refused(L, free(a, h), text)
    dev.pressure_bc(p)
    assert np.isfinite(p.to_numpy()).all()


def test_destroy_with_a_live_object_of_every_kind(hip_lib):
    """fs_destroy releases whatever the registry still holds - one live object of each kind here, and one freed before - and returns 0; a context
    created afterwards runs a launch."""
    import fs
    from fs.boundary_condition import BoundaryCondition
    fs.runtime.init(gpu=0, dtype="f32")
    L = hip_lib
    mask = np.zeros((32, 16), np.uint8); mask[:, :2] = 1; mask[:, -2:] = 1
    victim = BoundaryCondition(np.zeros((32, 16, 2), np.float32), mask).device
    ctx, victim._ctx = victim._ctx, None                        # (its close() and finaliser must not destroy the context a second time)
    handles = {kind: KINDS[kind][0](L, ctx) for kind in sorted(KINDS)}
    extra = KINDS["mean"][0](L, ctx)
    assert L.fs_mean_free(ctx, extra) == 0
    for kind, h in handles.items():
        assert KINDS[kind][1](L, ctx, h) == 0, kind
    assert L.fs_destroy(ctx) == 0
    fresh = BoundaryCondition(np.zeros((32, 16, 2), np.float32), mask).device
    try:
        p = fresh.alloc(1)
        p.from_numpy(np.ones((32, 16), np.float32))
        fresh.pressure_bc(p)
        assert np.isfinite(p.to_numpy()).all()
    finally:
        fresh.close()
