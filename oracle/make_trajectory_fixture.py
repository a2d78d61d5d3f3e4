"""Generate the trajectory round-trip fixture: write the two small
trajectories of tests/test_trajectory.py (two fibers, two frames; one
spherical body, one frame) with this engine's TrajectoryWriter, load them
through the REFERENCE'S OWN TrajectoryReader (src/skelly_sim/reader.py) and
record both the msgpack streams it accepted and what it decoded:

  tests/golden/trajectory_fibers.out    the fiber stream, as written
  tests/golden/trajectory_body.out      the body stream, as written
  tests/golden/trajectory_reader.npz    the reference reader's view of both

Needs a checkout of the reference tree:
  python oracle/make_trajectory_fixture.py <reference-root>"""

import os
import shutil
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_periphery_fixture import install_shims  # noqa: E402


def install_reader_shims():
    """Stand-ins for the reference python package's optional deps."""
    install_shims()
    for name, attrs in {
        "toml": dict(load=lambda f: {}, dump=lambda *a, **k: None),
        "dataclass_utils": dict(check_type=lambda *a, **k: None),
    }.items():
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules.setdefault(name, m)
    if "nptyping" not in sys.modules:
        m = types.ModuleType("nptyping")

        class _Sub:
            def __class_getitem__(cls, item):
                return np.ndarray

        m.NDArray = _Sub
        m.Shape = _Sub
        m.Float64 = float
        sys.modules["nptyping"] = m


def main(reference_root):
    install_reader_shims()
    sys.path.insert(0, os.path.join(reference_root, "src"))
    from skelly_sim.reader import TrajectoryReader
    import test_trajectory as tt
    import skellysim_amd.trajectory as trajectory
    from skellysim_amd.trajectory import TrajectoryWriter
    # keep the generating host's name out of the recorded headers
    trajectory.socket = types.SimpleNamespace(gethostname=lambda: "fixture")

    golden = os.path.join(REPO, "tests", "golden")
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        toml_file = os.path.join(tmp, "skelly_config.toml")
        open(toml_file, "w").write("")
        out = os.path.join(tmp, "skelly_sim.out")

        tt._write_traj(tmp)
        traj = TrajectoryReader(toml_file)
        rec["fibers_trajectory_version"] = traj.trajectory_version
        rec["fibers_times"] = np.asarray(list(traj.times), float)
        last = len(traj.times) - 1
        traj.load_frame(last)
        fibs = traj["fibers"]
        rec["fibers_count"] = len(fibs)
        rec["fibers_x"] = np.stack([np.asarray(f["x_"], float) for f in fibs])
        rec["fibers_time"] = float(traj["time"])
        shutil.copyfile(out, os.path.join(golden, "trajectory_fibers.out"))
        os.remove(out)
        # the reader caches its frame index next to the trajectory
        for name in os.listdir(tmp):
            if name not in ("skelly_config.toml",):
                os.remove(os.path.join(tmp, name))

        sys_b, _ = tt._body_system()
        with TrajectoryWriter(out) as tw:
            assert sys_b.step(tol=1e-11, maxiter=100)["converged"]
            tw.write_frame(sys_b, 0.1, 0.1)
        traj2 = TrajectoryReader(toml_file)
        traj2.load_frame(0)
        bodies = traj2["bodies"]
        rec["body_count"] = len(bodies)
        bm = bodies[0]
        rec["body_radius"] = float(bm["radius_"])
        rec["body_position"] = np.asarray(bm["position_"], float)
        rec["body_orientation"] = np.asarray(bm["orientation_"], float)
        rec["body_solution_vec"] = np.asarray(bm["solution_vec_"], float)
        shutil.copyfile(out, os.path.join(golden, "trajectory_body.out"))

    path = os.path.join(golden, "trajectory_reader.npz")
    np.savez_compressed(path, **rec)
    for k, v in rec.items():
        print(k, np.shape(v))
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
