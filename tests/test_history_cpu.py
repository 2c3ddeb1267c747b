"""Per-step history without a GPU: the face list of a body against the force of the flow-stats restatement (tests/flow_stats_ref.py), the
slab partition of faces and probes, probe checks, dominant_frequency, and the host logic of FluidSimulator.record_history / history on the
NumPy stand-in device (tests/history_standin.py): numbering, draining a tiny ring, and a gloo job of 2 - 4 slabs against one domain."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp
from flow_stats_ref import flow_stats_ref


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _face_force(faces, p, dx):
    from fs.history import SIGNS
    f = np.zeros(2)
    scale = 0.0
    for x, y, d in faces:
        t = float(p[x, y]) * dx
        f[d // 2] += SIGNS[d] * t
        scale += abs(t)
    return f, scale


def _check_faces(mask, box, rng, dx=0.01):
    from fs.history import body_faces
    faces = body_faces(mask, box)
    keys = [tuple(r) for r in faces[:, [1, 0, 2]].tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys), "faces not sorted by (y, x, dir) or duplicated"
    assert (mask[faces[:, 0], faces[:, 1]] == 0).all() if len(faces) else True
    p = rng.standard_normal(mask.shape)
    exp = flow_stats_ref(np.zeros(mask.shape + (2,)), p, mask, dx, box)
    got, scale = _face_force(faces, p, dx)
    tol = max(len(faces), 1) * 2.0 ** -52 * scale
    assert abs(got[0] - exp["force_x"]) <= tol and abs(got[1] - exp["force_y"]) <= tol, (got, exp["force_x"], exp["force_y"])
    return len(faces)


@pytest.mark.parametrize("res", [32, 41, 64, 97])
def test_face_list_matches_flow_stats_force_on_scenes(res):
    from fs.boundary_condition import create_scene_arrays, default_body_box
    rng = np.random.default_rng(res)
    for bc in (1, 3, 5):
        mask = create_scene_arrays(bc, res)[1]
        assert _check_faces(mask, default_body_box(bc, res), rng) > 0
    for bc in (2, 4) if res % 2 == 0 else (2,):        # (scene 4's builder needs an even resolution)
        mask = create_scene_arrays(bc, res)[1]
        X, Y = mask.shape
        for _ in range(3):
            x0, x1 = sorted(rng.integers(0, X + 1, 2))
            y0, y1 = sorted(rng.integers(0, Y + 1, 2))
            _check_faces(mask, (int(x0), int(y0), int(x1), int(y1)), rng)
        _check_faces(mask, (0, 0, X, Y), rng)


def test_face_list_on_random_masks():
    rng = np.random.default_rng(7)
    for X, Y in ((16, 8), (33, 17), (64, 31)):
        for _ in range(6):
            mask = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), size=(X, Y))
            x0, x1 = sorted(rng.integers(0, X + 1, 2))
            y0, y1 = sorted(rng.integers(0, Y + 1, 2))
            _check_faces(mask, (int(x0), int(y0), int(x1), int(y1)), rng)


def test_face_list_rejects_bad_box():
    from fs.history import body_faces
    with pytest.raises(ValueError):
        body_faces(np.zeros((8, 4), np.uint8), (0, 0, 9, 4))
    with pytest.raises(ValueError):
        body_faces(np.zeros((8, 4), np.uint8), (3, 0, 2, 4))


@pytest.mark.parametrize("world", range(1, 9))
def test_slab_partition_is_disjoint_and_complete(world):
    from fs.boundary_condition import create_scene_arrays, default_body_box
    from fs.history import body_faces, owned
    from fs.runtime import slab_rows
    res = 43                                    # Y = 43: uneven slab heights for every world size > 1
    mask = create_scene_arrays(3, res)[1]
    X, Y = mask.shape
    faces = body_faces(mask, default_body_box(3, res))
    fluid = np.argwhere(mask == 0)
    probes = fluid[np.random.default_rng(world).choice(len(fluid), 25, replace=False)]
    for items in (faces, probes):
        seen = []
        for r in range(world):
            y0, n = slab_rows(Y, r, world)
            idx = owned(items, y0, n)
            assert ((items[idx, 1] >= y0) & (items[idx, 1] < y0 + n)).all()
            seen.extend(idx.tolist())
        assert sorted(seen) == list(range(len(items))), "per-rank sets are not a partition of the list"


def test_check_probes():
    from fs.history import check_probes
    mask = np.zeros((8, 4), np.uint8)
    mask[3, 2] = 1
    mask[0, 0] = 2
    assert check_probes(mask, [(1, 1), (5, 3)]).tolist() == [[1, 1], [5, 3]]
    assert check_probes(mask, []).shape == (0, 2)
    for bad in ([(8, 0)], [(-1, 0)], [(0, 4)], [(3, 2)], [(0, 0)], [(1, 1), (1, 1)]):
        with pytest.raises(ValueError):
            check_probes(mask, bad)


def test_dominant_frequency():
    from fs.history import dominant_frequency
    n, dt = 1024, 0.002
    t = np.arange(n) * dt
    for k in (3, 17, 100, 511):
        f = k / (n * dt)
        assert dominant_frequency(np.sin(2 * np.pi * f * t), dt) == f
        noisy = 5.0 + np.sin(2 * np.pi * f * t + 0.3) + 0.2 * np.random.default_rng(k).standard_normal(n)
        assert dominant_frequency(noisy, dt) == f


# ---- host logic on the NumPy stand-in ------------------------------------------------------------------------------------------
FNAME = "traj_bc1_upwind_vc0.npz"


def _probes(fname=FNAME, n=6):
    from conftest import GOLDEN
    mask = np.load(os.path.join(GOLDEN, fname))["bc_mask"]
    fluid = np.argwhere(mask == 0)
    return [tuple(int(c) for c in fluid[k]) for k in np.linspace(0, len(fluid) - 1, n).astype(int)]


@pytest.fixture
def standin():
    import fs
    from history_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def _fields_at(sim, probes):
    d = sim.field_to_numpy()
    return np.array([[d["v"][x, y, 0], d["v"][x, y, 1], d["p"][x, y]] for x, y in probes], np.float64)


def test_numbering_every_and_start_step(standin):
    from history_standin import run_scene
    probes = _probes()
    sim, h = run_scene(FNAME, 20, probes, every=3, start_step=100)
    assert h["step"].tolist() == [100 + 3 * k for k in range(1, 7)]
    assert np.array_equal(h["time"], h["step"] * sim._solver.dt)
    assert h["u"].shape == (6, len(probes)) and h["probes"].tolist() == [list(p) for p in probes]
    assert "force_x" in h and h["force_x"].shape == (6,)
    sim.run(1)                      # step 121: the last row is the current state
    h = sim.history()
    assert h["step"][-1] == 121
    assert np.array_equal(np.stack([h["u"][-1], h["w"][-1], h["p"][-1]], axis=1), _fields_at(sim, probes))
    sim.stop_history()
    sim.run(3)
    assert sim.history()["step"][-1] == 121       # (kept after stop_history, nothing more recorded)


def test_tiny_ring_drains_without_loss(standin):
    from history_standin import run_scene
    probes = _probes()
    sim, h = run_scene(FNAME, 47, probes, capacity=5)
    assert h["step"].tolist() == list(range(1, 48))
    sim2, h2 = run_scene(FNAME, 47, probes, chunks=[10, 30, 7])       # one ring large enough for all
    for k in ("u", "w", "p", "force_x", "force_y"):
        assert np.array_equal(h[k], h2[k]), k
    for _ in range(12):                                            # eager steps past the ring: drained on the way
        sim.step()
    h = sim.history()
    assert h["step"].tolist() == list(range(1, 60))


def test_probes_only_and_body_only(standin):
    from history_standin import run_scene
    probes = _probes()
    sim, h = run_scene(FNAME, 5, probes)
    sim.record_history(probes)                   # no body box: no force keys
    sim.run(4)
    h = sim.history()
    assert "force_x" not in h and h["step"].tolist() == [1, 2, 3, 4]
    sim.record_history([], (0, 0) + sim._solver._bc.mask.shape)
    sim.run(2)
    h = sim.history()
    assert h["u"].shape == (2, 0) and h["force_x"].shape == (2,)


def test_record_history_refusals(standin):
    from history_standin import run_scene
    sim, _ = run_scene(FNAME, 1, _probes())
    mask = sim._solver._bc.mask
    wall = tuple(int(c) for c in np.argwhere(mask == 1)[0])
    for kw in (dict(probes=[wall]), dict(probes=[(0, 10 ** 6)]), dict(), dict(probes=_probes(), every=0)):
        with pytest.raises(ValueError):
            sim.record_history(**kw)


@pytest.mark.parametrize("world,halo", [(2, 2), (3, 2), (4, 2)])
def test_slab_history_matches_single_domain(world, halo, tmp_path, standin):
    from history_standin import run, run_scene
    probes = _probes()
    steps = 60
    mp.spawn(run, args=(world, _free_port(), FNAME, halo, steps, probes, str(tmp_path)), nprocs=world, join=True)
    got = dict(np.load(os.path.join(tmp_path, "slabs.npz")))
    sim, exp = run_scene(FNAME, steps, probes, capacity=40, chunks=[steps - 5, 5])
    assert int(got["tapes"]) > 0, "the slab run never replayed a tape"
    assert got["step"].tolist() == exp["step"].tolist() == list(range(1, steps + 1))
    for k in ("u", "w", "p"):
        assert np.array_equal(got[k], exp[k]), f"probe {k} differs from the single domain"
    ring = sim._recorder.hist._h
    tol = len(ring.faces) * 2.0 ** -52 * np.array(ring.scales)           # n 2^-52 sum |term| per record
    assert np.abs(exp["force_x"]).max() > 0.0
    for k in ("force_x", "force_y"):
        assert np.all(np.abs(got[k] - exp[k]) <= tol), k
