"""Which libmgp_hip entries an ELBO step launches, in which order and on which stream.

The value-comparing tests cannot see a step that falls from the two-layer launches to the
per-layer ones (the batch entries are bit-identical to the per-layer ones), nor work that
moves between the main and the side stream, so the launch sequence of the second call of
each case is pinned here: `_lib.call` and `_lib.call_raw` are wrapped, and every entry whose
last argument is a stream is recorded by name, with "@side" appended when that stream is the
model's side stream (every other launch must be on torch's current stream).

Case 1 (equal SquaredExponential layers, default config, _build_likelihood) is the chain of
the modulatedgps_amd/models.py module docstring.  The other lists were recorded with this
recorder on the commit before SMGP.conditionals was split along its launch plan; they are
the project's own entry names (include/mgp_hip.h).  Shapes: the smallest that take every
branch (M = 130: two row tiles; ragged N)."""
import pytest
import torch

from oracle import cpu_ref as R
from tests import matern_ref as MR
from tests.helpers import UNEQUAL_CASES, build_model, unequal_problem

pytestmark = pytest.mark.gpu

_PAIRED_BACKWARD = ["mgp_elbo_terms", "mgp_elbo_terms_backward", "mgp_conditional_backward_f16c_prepped",
                    "mgp_conditional_backward_f16c_prepped", "mgp_chol_backward_batch", "mgp_rbf_backward_batch",
                    "mgp_kl_grad", "mgp_kl_grad", "mgp_elbo_combine"]
_PAIRED_K4_K5 = ["mgp_trsm_stats_f16_batch", "mgp_expert_conditional_f16_batch"]

# case -> (layers_per_launch, [entry, or entry@side on the side stream, ...])
EXPECTED = {
    "equal_forward": (2, [
        "mgp_kuu_potrf_trtri_kuf", "mgp_split_upper_f16_bounded_batch", "mgp_qsqrt_images_kl_f16_batch@side",
        *_PAIRED_K4_K5, "mgp_elbo_terms", "mgp_elbo_combine"]),
    "equal_training": (2, [
        "mgp_kuu_potrf_trtri_kuf", "mgp_split_upper_f16_bounded_batch", "mgp_colnorm_max@side",
        "mgp_colnorm_max@side", "mgp_qsqrt_images_kl_f16_batch@side", "mgp_conditional_backward_prep_f16c@side",
        "mgp_conditional_backward_prep_f16c@side", *_PAIRED_K4_K5, *_PAIRED_BACKWARD]),
    "unequal_forward": (1, [
        "mgp_kuu_potrf_trtri", "mgp_kuu_potrf_trtri", "mgp_split_upper_f16", "mgp_split_upper_f16",
        "mgp_rbf_kuf_f16@side", "mgp_split_lower_f16@side", "mgp_rbf_kuf_f16@side", "mgp_split_lower_f16@side",
        "mgp_gauss_kl_white@side", "mgp_gauss_kl_white@side", "mgp_trsm_stats_f16", "mgp_trsm_stats_f16",
        "mgp_expert_conditional_f16", "mgp_expert_conditional_f16", "mgp_elbo_terms", "mgp_elbo_combine"]),
    "unequal_training": (1, [
        "mgp_kuu_potrf_trtri", "mgp_kuu_potrf_trtri", "mgp_split_upper_f16", "mgp_split_upper_f16",
        "mgp_rbf_kuf_f16@side", "mgp_split_lower_f16@side", "mgp_colnorm_max@side",
        "mgp_rbf_kuf_f16@side", "mgp_split_lower_f16@side", "mgp_colnorm_max@side",
        "mgp_gauss_kl_white@side", "mgp_gauss_kl_white@side", "mgp_conditional_backward_prep_f16c@side",
        "mgp_conditional_backward_prep_f16c@side", "mgp_trsm_stats_f16", "mgp_trsm_stats_f16",
        "mgp_expert_conditional_f16c", "mgp_expert_conditional_f16c", "mgp_elbo_terms", "mgp_elbo_terms_backward",
        "mgp_conditional_backward_f16c_prepped", "mgp_chol_backward", "mgp_rbf_backward", "mgp_rbf_backward",
        "mgp_conditional_backward_f16c_prepped", "mgp_chol_backward", "mgp_rbf_backward", "mgp_rbf_backward",
        "mgp_kl_grad", "mgp_kl_grad", "mgp_elbo_combine"]),
    "matern_forward": (2, [
        "mgp_matern_kuu_potrf_trtri", "mgp_kuu_potrf_trtri", "mgp_split_upper_f16", "mgp_split_upper_f16",
        "mgp_matern_kuf_image@side", "mgp_rbf_kuf_f16@side", "mgp_qsqrt_images_kl_f16_batch@side",
        *_PAIRED_K4_K5, "mgp_elbo_terms", "mgp_elbo_combine"]),
    "equal_forward_overlap": (2, [
        "mgp_kuu_potrf_trtri_ex", "mgp_split_upper_f16_bounded_batch", "mgp_rbf_kuf_f16@side",
        "mgp_rbf_kuf_f16@side", "mgp_qsqrt_images_kl_f16_batch@side", *_PAIRED_K4_K5, "mgp_elbo_terms",
        "mgp_elbo_combine"]),
    "equal_training_overlap": (2, [
        "mgp_kuu_potrf_trtri_ex", "mgp_split_upper_f16_bounded_batch", "mgp_rbf_kuf_f16@side",
        "mgp_colnorm_max@side", "mgp_rbf_kuf_f16@side", "mgp_colnorm_max@side",
        "mgp_qsqrt_images_kl_f16_batch@side", "mgp_conditional_backward_prep_f16c@side",
        "mgp_conditional_backward_prep_f16c@side", *_PAIRED_K4_K5, *_PAIRED_BACKWARD]),
    "equal_forward_serial": (2, [
        "mgp_kuu_potrf_trtri_ex", "mgp_split_upper_f16_bounded_batch", "mgp_qsqrt_images_kl_f16_batch",
        "mgp_rbf_kuf_f16", "mgp_rbf_kuf_f16", *_PAIRED_K4_K5, "mgp_elbo_terms", "mgp_elbo_combine"]),
    "equal_training_serial": (2, [
        "mgp_kuu_potrf_trtri_ex", "mgp_split_upper_f16_bounded_batch", "mgp_colnorm_max", "mgp_colnorm_max",
        "mgp_qsqrt_images_kl_f16_batch", "mgp_conditional_backward_prep_f16c", "mgp_conditional_backward_prep_f16c",
        "mgp_rbf_kuf_f16", "mgp_rbf_kuf_f16", *_PAIRED_K4_K5, *_PAIRED_BACKWARD]),
}


def _model(device, which):
    """(model, X, Y): equal SquaredExponential layers, the unequal case b, or a Matern32 pred layer."""
    if which == "unequal":
        X, Y, p = unequal_problem(*UNEQUAL_CASES["b"])
    else:
        X, Y, p = R.synthetic_problem(301, 130, 3, 2, 0.8, state="perturbed", S=2)
    model = MR.build_model(p, device, ("matern32", "se")) if which == "matern" else build_model(p, device)
    return model, torch.as_tensor(X, dtype=torch.float32, device=device), Y


def record(monkeypatch, model, step):
    """The launches of the second step() call: entry names, "@side" on the model's side stream."""
    from modulatedgps_amd import _lib
    step()
    main = torch.cuda.current_stream(model.device).cuda_stream
    side = model._side_stream().cuda_stream
    assert side != main
    log = []
    with monkeypatch.context() as mp:
        for fn in ("call", "call_raw"):
            inner = getattr(_lib, fn)

            def wrapped(name, *args, _inner=inner):
                stream = args[-1]
                assert stream in (main, side), (name, stream)
                log.append(name + ("@side" if stream == side else ""))
                return _inner(name, *args)
            mp.setattr(_lib, fn, wrapped)
        step()
    torch.cuda.synchronize()
    return log


def run_case(monkeypatch, device, case):
    """(layers_per_launch, launches) of a case "<model>_<forward|training>[_<schedule>]"."""
    from modulatedgps_amd import config
    which, mode, *sched = case.split("_", 2)
    model, X, Y = _model(device, which)
    old = config.step_schedule()
    config.set_step_schedule(sched[0] if sched else old)
    try:
        if mode == "training":
            log = record(monkeypatch, model, lambda: model.elbo_and_grad(X, Y, seed=3))
        else:
            log = record(monkeypatch, model, lambda: model._build_likelihood(X, Y, seed=3))
    finally:
        config.set_step_schedule(old)
    return model.layers_per_launch, log


CASES = ["equal_forward", "equal_training", "unequal_forward", "unequal_training", "matern_forward",
         "equal_forward_overlap", "equal_training_overlap", "equal_forward_serial", "equal_training_serial"]


@pytest.mark.parametrize("case", CASES)
def test_step_launches(monkeypatch, device, case):
    lpl, log = run_case(monkeypatch, device, case)
    want_lpl, want = EXPECTED[case]
    print(case, lpl, log, flush=True)
    assert lpl == want_lpl
    assert log == want
    if case.endswith("_serial"):
        assert not any(name.endswith("@side") for name in log)

