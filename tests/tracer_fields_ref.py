"""NumPy restatements for the device sort and the per-cell fields of the tracer particles (csrc/fs_tracer.h k_tracer_sort_* /
k_tracer_fields, include/fs_hip.h fs_tracer_sort / fs_tracer_fields): the fields by np.add.at into int32 / int64, alive and inside
particles only, and the checks of the order contract.  Shared by tests/test_tracer_sort_cpu.py and tests/test_gpu_tracer_sort.py."""
import numpy as np

ALIVE = 0


def fields_ref(state, X, Y):
    """-> (count int32 (X, Y), age_sum int64 (X, Y)) of a tracer state ({"x", "y", "age", "status"}, any order)."""
    x, y = np.asarray(state["x"], np.float64), np.asarray(state["y"], np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.asarray(state["status"]) == ALIVE) & (x >= 0) & (x < X) & (y >= 0) & (y < Y)
    i, j = np.floor(x[ok]).astype(np.int64), np.floor(y[ok]).astype(np.int64)
    count, age_sum = np.zeros((X, Y), np.int32), np.zeros((X, Y), np.int64)
    np.add.at(count, (i, j), 1)
    np.add.at(age_sum, (i, j), np.asarray(state["age"])[ok].astype(np.int64))
    return count, age_sum


def assert_order_contract(raw, X, Y):
    """`raw`: DeviceBase.tracer_read(tr, raw=True) after a sort: id is a permutation, the keys do not decrease along the slots, the dead
    (and outside) particles stand last."""
    from fs.tracers import sort_key
    n = len(raw["x"])
    assert raw["id"].dtype == np.int32 and np.array_equal(np.sort(raw["id"]), np.arange(n)), "id is no permutation of arange(N)"
    key = sort_key(raw["x"], raw["y"], raw["status"], X, Y)
    assert np.all(np.diff(key) >= 0), "the sort keys decrease somewhere along the slots"
    with np.errstate(invalid="ignore"):
        last = (raw["status"] != ALIVE) | ~((raw["x"] >= 0) & (raw["x"] < X) & (raw["y"] >= 0) & (raw["y"] < Y))
    nlast = int(last.sum())
    assert not last[:n - nlast].any() and last[n - nlast:].all(), "dead / outside particles do not stand last"
    return key
