"""GPU test of the flow_sources evaluation on device tensors: flows'
*_at_targets are, bit for bit, the sum in the documented order (fibers, shell,
body nodes, body centre stokeslets, body centre rotlets; point forces and
point torques before them) of the direct evaluator.*_device calls. 37 sources
of each kind and 16 targets: a sum goes wrong in which terms it has and in
which order, and that shows at any size."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ETA = 1.3


@pytest.fixture(scope="module")
def case(hip_lib_path):
    import torch
    rng = np.random.default_rng(37)
    dev = torch.device("cuda:0")
    a = lambda n=37: torch.from_numpy(rng.uniform(-1, 1, (n, 3))).to(dev)
    fiber = dict(r_src=a(), forces=a(), weights=torch.from_numpy(rng.uniform(0.1, 0.2, 37)).to(dev))
    shell = dict(node_pos=a(), node_normal=a(), density=a())
    bodies = dict(node_pos=a(), node_normals=a(), densities=a(), centers=a(), forces=a(),
                  torques=a())
    points = dict(force_pos=a(), forces=a(), torque_pos=a(), torques=a())
    return dict(fiber=fiber, shell=shell, bodies=bodies), points, 2.5 + a(16)


def direct_sum(suffix, shape, kw, points, trg, eta_args):
    """zeros + each term's evaluator.<kernel><suffix>_device, in order."""
    import torch
    from skellysim_amd import evaluator
    from skellysim_amd.flows import double_layer_strength
    fn = lambda kernel: getattr(evaluator, kernel + suffix + "_device")
    fiber, shell, bodies = kw["fiber"], kw["shell"], kw["bodies"]
    out = torch.zeros((16,) + shape, dtype=torch.float64, device=trg.device)
    if points is not None:
        out = out + fn("oseen_contract")(points["force_pos"], trg, points["forces"], *eta_args)
        if suffix != "_pressure":
            out = out + fn("rotlet")(points["torque_pos"], trg, points["torques"], ETA)
    out = out + fn("stokeslet")(fiber["r_src"], fiber["forces"] * fiber["weights"][:, None], trg,
                                *eta_args)
    out = out + fn("stresslet")(shell["node_pos"], double_layer_strength(
        shell["node_normal"], shell["density"], ETA), trg, *eta_args)
    out = out + fn("stresslet")(bodies["node_pos"], double_layer_strength(
        bodies["node_normals"], bodies["densities"], ETA), trg, *eta_args)
    out = out + fn("stokeslet")(bodies["centers"], bodies["forces"], trg, *eta_args)
    if suffix != "_pressure":
        out = out + fn("rotlet")(bodies["centers"], trg, bodies["torques"], ETA)
    return out


@pytest.mark.parametrize("quantity, suffix, shape, eta_args", [
    ("velocity", "", (3,), (ETA,)), ("gradient", "_grad", (3, 3), (ETA,)),
    ("pressure", "_pressure", (), ())])
def test_at_targets_are_the_ordered_sum_of_the_device_calls(case, quantity, suffix, shape,
                                                            eta_args):
    import torch
    from skellysim_amd import flows
    from skellysim_amd.flow_sources import evaluate, flow_sources
    kw, points, trg = case
    at_targets = {"velocity": flows.velocity_at_targets,
                  "gradient": flows.velocity_gradient_at_targets,
                  "pressure": flows.pressure_at_targets}[quantity]
    got = at_targets(trg, ETA, **kw)
    want = direct_sum(suffix, shape, kw, None, trg, eta_args)
    assert got.is_cuda and got.shape == (16,) + shape
    assert torch.equal(got, want)
    assert bool(torch.all(want != 0))
    # with the point sources in front, through evaluate
    got = evaluate(flow_sources(sources=points, **kw), quantity, trg, ETA)
    assert torch.equal(got, direct_sum(suffix, shape, kw, points, trg, eta_args))
    assert not torch.equal(got, want)
