"""Child process of tests/test_gpu_multigrid.py: one MultigridPressureUpdater.update() on the developed state of a scene, in float32, with
whatever FS_MG_TAIL the parent put into the environment.  Prints the first level of the one-workgroup kernel (0: none) and the SHA-256 of
(p.current, p.next).  usage: multigrid_worker.py SCENE RES"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, "2d-fluid-simulator_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    num, res = int(sys.argv[1]), int(sys.argv[2])
    import test_gpu_multigrid as T
    pc, pn, v = T.developed(num, res, "float32")
    sim = T.make_sim(num, res, "float32")
    s = sim._solver
    s.v.current.from_numpy(v)
    s.p.current.from_numpy(pc)
    s.p.next.from_numpy(pn)
    s.pressure_updater.update(s.p, s.v.current)
    digest = hashlib.sha256(s.p.current.to_numpy().tobytes() + s.p.next.to_numpy().tobytes()).hexdigest()
    info = s.pressure_updater.info()
    s._bc.device.close()
    print(info["tail_level"], digest)


if __name__ == "__main__":
    main()
