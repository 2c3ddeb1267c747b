"""Body surface loads without a GPU: face geometry and centroid on a hand-made rectangle, the sign conventions of the definitions
(tests/loads_ref.py) on manufactured fields, the helper functions, and the host logic of FluidSimulator.track_body / body_loads /
body_surface / body_snapshot on the NumPy stand-in device (tests/loads_standin.py): numbering, a tiny ring, a recorder and a tracker side by
side, refusals, and a gloo job of 2 - 4 slabs against one domain."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp
from loads_ref import DX, RE, manufactured, record_bound, sample_ref


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def _rect(X=12, Y=9, x0=4, y0=3, w=3, h=2):
    mask = np.zeros((X, Y), np.uint8)
    mask[x0:x0 + w, y0:y0 + h] = 1
    return mask, (x0, y0, x0 + w, y0 + h)


def test_geometry_on_a_3x2_rectangle():
    from fs.history import body_faces
    from fs.loads import body_centroid, face_geometry
    mask, box = _rect()
    assert body_centroid(mask, box) == (5.5, 4.0)
    assert body_centroid(mask, (0, 0, 12, 9)) == (5.5, 4.0)
    with pytest.raises(ValueError):
        body_centroid(mask, (0, 0, 2, 2))
    faces = body_faces(mask, box)
    assert len(faces) == 2 * (3 + 2)
    g = face_geometry(faces, (5.5, 4.0))
    exp = {  # (x, y, dir) -> midpoint, normal
        (7, 3, 0): (7.0, 3.5, 1, 0), (7, 4, 0): (7.0, 4.5, 1, 0), (3, 3, 1): (4.0, 3.5, -1, 0), (3, 4, 1): (4.0, 4.5, -1, 0),
        (4, 5, 2): (4.5, 5.0, 0, 1), (5, 5, 2): (5.5, 5.0, 0, 1), (6, 5, 2): (6.5, 5.0, 0, 1),
        (4, 2, 3): (4.5, 3.0, 0, -1), (5, 2, 3): (5.5, 3.0, 0, -1), (6, 2, 3): (6.5, 3.0, 0, -1)}
    assert sorted(exp) == sorted(tuple(f) for f in faces.tolist())
    for k, f in enumerate(faces.tolist()):
        xm, ym, nx, ny = exp[tuple(f)]
        assert (g["x"][k], g["y"][k], g["nx"][k], g["ny"][k]) == (xm, ym, nx, ny)
        assert g["theta"][k] == np.arctan2(ym - 4.0, xm - 5.5)
    # the midpoint lies on the face: half a cell from the fluid cell's centre against the normal
    assert np.array_equal(g["x"], faces[:, 0] + 0.5 - 0.5 * g["nx"]) and np.array_equal(g["y"], faces[:, 1] + 0.5 - 0.5 * g["ny"])


# ---- sign conventions on manufactured fields (tests/loads_ref.py manufactured: values exact in float32) ------------------------------------
def test_sign_conventions_on_manufactured_fields():
    from fs.loads import RECORD, body_centroid
    for dims in (dict(), dict(X=16, Y=14, x0=5, y0=4, w=4, h=5)):
        mask, box = _rect(**dims)
        faces, centre, cases = manufactured(mask, box)
        assert centre == body_centroid(mask, box)
        for name, v, p, check in cases:
            sums = np.zeros((4, len(faces)))
            rec, scale = sample_ref(sums, v, p, faces, centre, DX, 1.0 / RE)
            b = record_bound(len(faces), scale)
            check(dict(zip(RECORD, rec)), dict(zip(RECORD, b)))
            assert np.array_equal(sums[0], p[faces[:, 0], faces[:, 1]].astype(np.float64)), name
            assert np.array_equal(sums[1], sums[0] ** 2) and np.array_equal(sums[3], sums[2] ** 2), name
            ut = np.where(faces[:, 2] < 2, v[faces[:, 0], faces[:, 1], 1], v[faces[:, 0], faces[:, 1], 0]).astype(np.float64)
            assert np.array_equal(sums[2], ut / RE / DX), name            # (tau = u_t / (re dx); exact here: powers of two)


def test_helper_functions():
    from fs.loads import coefficients, pressure_coefficient, skin_friction, surface_statistics
    assert np.array_equal(coefficients([1.0, -3.0], 2.0, 0.5), [1.0, -3.0])
    assert coefficients(0.75, 1.0, 0.25) == 6.0
    assert np.array_equal(pressure_coefficient([1.5, 0.5], 2.0, p_ref=0.5), [0.5, 0.0])
    assert pressure_coefficient(0.5, 1.0) == 1.0
    assert np.array_equal(skin_friction([0.25, -1.0], 1.0), [0.5, -2.0])
    sums = np.array([[4.0, 5.0, 7.0], [10.0, 13.0, 25.0], [2.0, 2.0, 2.0], [2.0, 2.0, 1.0]])       # S_p, S_pp, S_t, S_tt of 3 faces, 2 samples
    pm, pr, tm, tr = surface_statistics(sums, 2)
    assert np.array_equal(pm, [2.0, 2.5, 3.5]) and np.array_equal(pr, [1.0, 0.5, 0.5])
    assert np.array_equal(tm, [1.0, 1.0, 1.0]) and np.array_equal(tr, [0.0, 0.0, 0.0])        # (the last: -0.5 clipped at 0)
    assert np.isnan(surface_statistics(sums, 0)[0]).all()


# ---- host logic on the NumPy stand-in ------------------------------------------------------------------------------------------------
FNAME = "traj_bc1_upwind_vc0.npz"
SERIES = ("pressure_x", "pressure_y", "viscous_x", "viscous_y", "moment_pressure", "moment_viscous")


@pytest.fixture
def standin():
    import fs
    from loads_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def test_numbering_every_and_start_step(standin):
    from loads_standin import run_scene
    sim = run_scene(FNAME, [20], every=3, start_step=4)
    h = sim.body_loads()
    assert h["step"].tolist() == [7, 10, 13, 16, 19]
    assert np.array_equal(h["time"], h["step"] * sim._solver.dt)
    for k in SERIES + ("force_x", "force_y", "moment"):
        assert h[k].shape == (5,) and h[k].dtype == np.float64
    assert np.array_equal(h["force_x"], h["pressure_x"] + h["viscous_x"]) and np.array_equal(h["moment"], h["moment_pressure"] + h["moment_viscous"])
    s = sim.body_surface()
    assert s["samples"] == 5 and s["sums"].shape == (4, len(s["faces"])) and s["p_mean"].shape == (len(s["faces"]),)
    sim.run(2)                      # step 22: a sample, the current state
    h = sim.body_loads()
    assert h["step"][-1] == 22
    box = sim._tracker.box
    snap = sim.body_snapshot(box)
    for k in SERIES:
        assert snap[k] == h[k][-1], k
    assert np.abs(h["pressure_x"]).max() > 0.0
    st = sim.flow_stats(box)
    b = record_bound(len(s["faces"]), sim._tracker.loads._h.scales[-1])
    assert abs(h["pressure_x"][-1] - st["force_x"]) <= b[0] and abs(h["pressure_y"][-1] - st["force_y"]) <= b[1]
    sim.stop_body()
    sim.run(3)
    assert sim.body_loads()["step"][-1] == 22 and sim.body_surface()["samples"] == 6       # (kept after stop_body, nothing more sampled)


def test_tiny_ring_drains_without_loss(standin):
    from loads_standin import run_scene
    a = run_scene(FNAME, [47], capacity=3)
    b = run_scene(FNAME, [10, 30, 7])
    ha, hb = a.body_loads(), b.body_loads()
    assert ha["step"].tolist() == list(range(1, 48))
    for k in SERIES:
        assert np.array_equal(ha[k], hb[k]), k
    assert np.array_equal(a.body_surface()["sums"], b.body_surface()["sums"])
    for _ in range(8):                                             # eager steps past the ring: drained on the way
        a.step()
    assert a.body_loads()["step"].tolist() == list(range(1, 56))


def test_recorder_and_tracker_with_different_capacities(standin):
    from loads_standin import make_sim
    from fs.boundary_condition import default_body_box
    sim, cfg = make_sim(FNAME)
    box = default_body_box(cfg["bc"], cfg["res"])
    sim.record_history([], box, capacity=5)
    sim.track_body(box, capacity=3, every=2)
    sim.run(41)
    h, b = sim.history(), sim.body_loads()
    assert h["step"].tolist() == list(range(1, 42)) and b["step"].tolist() == list(range(2, 42, 2))
    nf = len(sim.body_surface()["faces"])
    scales = sim._tracker.loads._h.scales
    for k, n in enumerate(b["step"].tolist()):                      # the tracker's pressure force is the recorder's
        tol = record_bound(nf, scales[k])
        assert abs(b["pressure_x"][k] - h["force_x"][n - 1]) <= tol[0] and abs(b["pressure_y"][k] - h["force_y"][n - 1]) <= tol[1]
    sim.reset_body_surface()
    assert sim.body_surface()["samples"] == 0 and not sim.body_surface()["sums"].any()
    sim.run(3)                                                      # steps 42 - 44: the phase of `every` runs on
    assert sim.body_loads()["step"].tolist()[-2:] == [42, 44] and sim.body_surface()["samples"] == 2


def test_refusals(standin):
    from loads_standin import make_sim
    from fs.boundary_condition import default_body_box
    sim, cfg = make_sim(FNAME)
    box = default_body_box(cfg["bc"], cfg["res"])
    with pytest.raises(RuntimeError):
        sim.body_loads()
    for kw in (dict(every=0), dict(start_step=-1), dict(capacity=0), dict(center=(np.nan, 1.0)), dict(center=(1.0,))):
        with pytest.raises(ValueError):
            sim.track_body(box, **kw)
    with pytest.raises(ValueError):
        sim.track_body((0, 0, 2, 2))                # no wall cell: no centroid, no face
    with pytest.raises(ValueError):
        sim.track_body((0, 0, 2, 2), center=(1.0, 1.0))
    sim.track_body(box)
    with pytest.raises(RuntimeError):
        sim.track_body(box)
    sim.stop_body()
    sim.track_body(box)
    sim.run(2)
    assert sim.body_loads()["step"].tolist() == [1, 2]


@pytest.mark.parametrize("world,halo", [(2, 2), (3, 2), (4, 2)])
def test_slab_loads_match_single_domain(world, halo, tmp_path, standin):
    from loads_standin import run, run_scene
    chunks = [55, 5]
    mp.spawn(run, args=(world, _free_port(), FNAME, halo, chunks, 2, 3, str(tmp_path)), nprocs=world, join=True)
    got = dict(np.load(os.path.join(tmp_path, "slabs.npz")))
    sim = run_scene(FNAME, chunks, every=2, start_step=3, capacity=40)
    exp, surf = sim.body_loads(), sim.body_surface()
    assert int(got["tapes"]) > 0, "the slab run never replayed a tape"
    assert got["step"].tolist() == exp["step"].tolist() == list(range(5, 61, 2))
    assert int(got["samples"]) == surf["samples"] == len(exp["step"])
    assert np.array_equal(got["sums"], surf["sums"]), "per-face sums differ from the single domain"
    assert np.signbit(got["sums"]).tolist() == np.signbit(surf["sums"]).tolist()
    body = sim._tracker.loads._h
    tol = record_bound(len(body.faces), np.array(body.scales))           # (n, 6)
    assert np.abs(exp["pressure_x"]).max() > 0.0
    for c, k in enumerate(SERIES):
        assert np.all(np.abs(got[k] - exp[k]) <= tol[:, c]), k
