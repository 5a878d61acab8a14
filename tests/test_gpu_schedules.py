"""Every step schedule (config.STEP_SCHEDULES) computes the same bits.

The schedules only move the Cholesky-independent work of a step (K1, the tril(q_sqrt)
images, the KL) between K3's step launches, the side stream and the main stream ("serial":
everything on the main stream, so a cross-stream race shows as a difference from it).
So, for a fixed Philox key, the ELBO of
_build_likelihood (models.py:69-79) and the ELBO and every gradient block of
elbo_and_grad (utils/training_utils.py:10) must be bit-identical to the default
schedule's.  Shapes: one problem with equal M for both layers (the batched K3 / K4 /
K5 path) and one whose layers differ (M = 130 against 64, one of them ARD), where every
schedule falls back as conditionals decides (no batched K3, so no k1_in_k3; K4 / K5 per
layer); ragged N in both."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as R
from tests.helpers import UNEQUAL_CASES, build_model, unequal_problem

pytestmark = pytest.mark.gpu


def _problem(which):
    if which == "equal":
        return R.synthetic_problem(3001, 128, 4, 3, 0.8, state="perturbed", S=6)
    return unequal_problem(*UNEQUAL_CASES["b"])


def _run(device, sched, train, which):
    from modulatedgps_amd import config
    old = config.step_schedule()
    config.set_step_schedule(sched)
    try:
        X, Y, p = _problem(which)
        model = build_model(p, device)
        Xd = torch.as_tensor(X, dtype=torch.float32, device=device)
        if train:
            e, g = model.elbo_and_grad(Xd, Y, seed=1234)
            return e.clone(), {k: v.clone() for k, v in g.items()}
        return model._build_likelihood(Xd, Y, seed=1234), None
    finally:
        config.set_step_schedule(old)


@pytest.mark.parametrize("train", [False, True], ids=["forward", "training"])
def test_step_schedules_bit_identical(device, train):
    _check_schedules(device, train, "equal")


@pytest.mark.parametrize("train", [False, True], ids=["forward", "training"])
def test_step_schedules_bit_identical_unequal_layers(device, train):
    _check_schedules(device, train, "unequal")


def _check_schedules(device, train, which):
    from modulatedgps_amd import config
    ref_e, ref_g = _run(device, config.STEP_SCHEDULES[0], train, which)
    assert np.isfinite(float(ref_e.cpu()))
    for sched in config.STEP_SCHEDULES[1:]:
        e, g = _run(device, sched, train, which)
        assert torch.equal(e, ref_e), (sched, float(e), float(ref_e))
        if train:
            assert sorted(g) == sorted(ref_g)
            for k in ref_g:
                assert torch.equal(g[k], ref_g[k]), (sched, k)
