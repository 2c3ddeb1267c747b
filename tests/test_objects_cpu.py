"""The registry of a context's device objects and the one handle check (csrc/fs_objects.h) without a GPU: libfs_objects_host.so hands the header
to ctypes (csrc/fs_objects_host.cpp).  Its objects log their destruction, so the tests see WHEN a deleter ran and in which order.  A stale handle is
only ever looked up by its pointer value; the same cases run as a stand-alone program under the host sanitizers (-DFS_OBJECTS_HOST_MAIN)."""
import ctypes
import os

import pytest
from conftest import REPO

_lib = None
A, B = 0, 1      # two kinds


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(REPO, "2d-fluid-simulator_amd", "csrc", "libfs_objects_host.so"))
        vp, i = ctypes.c_void_p, ctypes.c_int
        for name, res, args in (("new", vp, []), ("destroy", None, [vp]), ("create", vp, [vp, i, i]), ("holds", i, [vp, vp, i]),
                                ("free", i, [vp, vp, i, i]), ("run_deferred", None, [vp]), ("log", i, [ctypes.POINTER(i), i]), ("log_clear", None, [])):
            f = getattr(_lib, "fs_objects_host_" + name)
            f.restype, f.argtypes = res, args
    return _lib


def log():
    buf = (ctypes.c_int * 64)()
    n = lib().fs_objects_host_log(buf, 64)
    return list(buf[:n])


@pytest.fixture()
def regs():
    """Two registries; whatever a test leaves in them is destroyed afterwards."""
    L = lib()
    L.fs_objects_host_log_clear()
    made = [L.fs_objects_host_new(), L.fs_objects_host_new()]
    yield made
    for r in made:
        if r is not None:
            L.fs_objects_host_destroy(r)


def test_live_handle_kind_and_registry(regs):
    L = lib()
    r, other = regs
    ha, hb, ho = L.fs_objects_host_create(r, A, 1), L.fs_objects_host_create(r, B, 2), L.fs_objects_host_create(other, A, 3)
    assert L.fs_objects_host_holds(r, ha, A) == 1 and L.fs_objects_host_holds(r, hb, B) == 1
    assert L.fs_objects_host_holds(r, ha, B) == 0 and L.fs_objects_host_holds(r, hb, A) == 0           # a live handle of the other kind
    assert L.fs_objects_host_holds(other, ha, A) == 0 and L.fs_objects_host_holds(r, ho, A) == 0       # a handle from another registry
    assert L.fs_objects_host_holds(r, None, A) == 0
    # a refused free leaves the object alive
    assert L.fs_objects_host_free(other, ha, A, 0) == -1 and L.fs_objects_host_free(r, ha, B, 0) == -1
    assert L.fs_objects_host_holds(r, ha, A) == 1 and log() == []


def test_freed_handle_is_refused_and_null_is_fine(regs):
    L = lib()
    r, _ = regs
    h, keep = L.fs_objects_host_create(r, A, 1), L.fs_objects_host_create(r, B, 2)
    assert L.fs_objects_host_free(r, None, A, 0) == 0 and log() == []
    assert L.fs_objects_host_free(r, h, A, 0) == 0 and log() == [1]
    assert L.fs_objects_host_holds(r, h, A) == 0 and L.fs_objects_host_holds(r, h, B) == 0             # stale: looked up, never read
    assert L.fs_objects_host_free(r, h, A, 0) == -1 and L.fs_objects_host_free(r, h, A, 1) == -1 and log() == [1]
    assert L.fs_objects_host_holds(r, keep, B) == 1


def test_free_inside_a_capture_is_deferred_in_call_order(regs):
    L = lib()
    r, _ = regs
    h = [L.fs_objects_host_create(r, k % 2, 10 + k) for k in range(4)]
    assert L.fs_objects_host_free(r, h[2], A, 1) == 0 and L.fs_objects_host_free(r, h[0], A, 1) == 0 and L.fs_objects_host_free(r, h[3], B, 1) == 0
    assert log() == []                                                     # no deleter ran yet
    for k in (2, 0, 3):                                                    # ... but the handles are stale at once
        assert L.fs_objects_host_holds(r, h[k], k % 2) == 0 and L.fs_objects_host_free(r, h[k], k % 2, 1) == -1
    assert L.fs_objects_host_free(r, h[1], B, 0) == 0 and log() == [11]    # (a free outside the capture does not wait for the list)
    L.fs_objects_host_run_deferred(r)
    assert log() == [11, 12, 10, 13]
    L.fs_objects_host_run_deferred(r)                                      # the list is empty: nothing runs twice
    assert log() == [11, 12, 10, 13]


def test_destroy_releases_every_live_object_exactly_once(regs):
    L = lib()
    r, other = regs
    h = [L.fs_objects_host_create(r, k % 2, 20 + k) for k in range(5)]
    assert L.fs_objects_host_free(r, h[0], A, 0) == 0                      # freed
    assert L.fs_objects_host_free(r, h[1], B, 1) == 0                      # deferred and run
    L.fs_objects_host_run_deferred(r)
    assert L.fs_objects_host_free(r, h[2], A, 1) == 0                      # deferred, never run: the capture did not end
    assert log() == [20, 21]
    L.fs_objects_host_destroy(r)
    regs[0] = None
    assert sorted(log()[2:]) == [22, 23, 24] and log()[-1] == 22           # the live ones, then what the open capture left; none twice
    L.fs_objects_host_destroy(other)                                       # an empty registry
    regs[1] = None
    assert len(log()) == 5
