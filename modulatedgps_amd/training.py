"""Optimiser of the training step: TF 2.10 Keras-legacy Adam on the unconstrained
variables (utils/training_utils.py:6,10), one HIP kernel
launch for all parameter blocks (mgp_adam_step_set, csrc/train.hip; one launch per
block when there are more than 16).

Positive parameters (GPflow positive() = softplus) keep an unconstrained shadow
u = softplus^-1(theta) on the device; Adam updates u and the kernel refreshes
theta = softplus(u) in the same launch.  Free parameters are updated in place.
q_sqrt is updated as a dense [K*M, M] block: its gradient is zero above the
diagonal, so the upper triangle stays zero (the same trajectory as Adam on the
packed FillTriangular vector, since Adam is elementwise)."""
import torch

from . import ops

_ADAM_SET = True   # False: one mgp_adam_step launch per block (A/B probes only)


def _as2d(t):
    if t.dim() == 1:
        return t.view(1, -1)
    if t.dim() == 3:
        return t.flatten(0, 1)
    return t


NATGRAD_BLOCKS = ("pred.q_mu", "pred.q_sqrt", "assign.q_mu", "assign.q_sqrt")


class NaturalGradient:
    """gpflow.optimizers.NaturalGradient(gamma) on (q_mu, q_sqrt) of both SVGP layers
    (XiSqrtMeanVar; ops.natgrad_step, csrc/natgrad.hip), used beside AdamTF on the other
    blocks.  The model's loss is the per-datum ELBO (data mean - KL / num_data), so the
    kernel's step is gamma * scale with scale = model.num_data by default: gamma then has
    the meaning it has for GPflow's total-ELBO loss, and gamma = 1 solves a conjugate model
    in one step.  An expert whose step does not exist (info != 0) is left as it is and
    counted on the device; skipped() reads the count (a host sync: readback points only)."""

    def __init__(self, gamma, scale=None):
        self.gamma = float(gamma)
        self.scale = None if scale is None else float(scale)
        self._skipped = None
        self._ws = {}

    def step(self, model, grads):
        """Apply one step to both layers from the ELBO gradients (dict name -> tensor)."""
        scale = self.scale if self.scale is not None else model.num_data
        if scale is None:
            raise ValueError("NaturalGradient needs scale= or a model with num_data set")
        infos = []
        for name, layer in (("pred", model.pred_layer), ("assign", model.assign_layer)):
            M, K = layer.q_mu.shape
            key = (M, K, layer.q_mu.device)
            if key not in self._ws:
                self._ws[key] = ops.natgrad_workspace(M, K, layer.q_mu.device)
            infos.append(ops.natgrad_step(layer.q_mu, layer.q_sqrt, grads[name + ".q_mu"], grads[name + ".q_sqrt"],
                                          self.gamma * float(scale), grad_sign=-1.0, workspace=self._ws[key]))
        n = sum((i != 0).sum() for i in infos)
        self._skipped = n if self._skipped is None else self._skipped + n
        return infos

    def skipped(self):
        """Expert steps skipped so far (synchronises with the device)."""
        return 0 if self._skipped is None else int(self._skipped.cpu())


class AdamTF:
    """tf.optimizers.Adam(lr) (beta1 0.9, beta2 0.999, epsilon 1e-7) over
    model.trainable_parameters()."""

    def __init__(self, params, lr, beta1=0.9, beta2=0.999, epsilon=1e-7):
        self.params = list(params)
        self.lr, self.beta1, self.beta2, self.eps = float(lr), float(beta1), float(beta2), float(epsilon)
        self.t = 0
        self.state = {}
        for name, theta, kind in self.params:
            v = _as2d(theta)
            st = {"m1": torch.zeros(v.shape, dtype=torch.float32, device=theta.device),
                  "m2": torch.zeros(v.shape, dtype=torch.float32, device=theta.device), "u": None}
            if kind == "positive":   # u = softplus^-1(theta) (parameter transform, set once)
                th = theta.detach().double()
                st["u"] = torch.where(th > 20, th, torch.log(torch.expm1(th))).float().reshape(v.shape).contiguous()
            self.state[name] = st

    def step(self, grads):
        """Apply one step from the ELBO gradients (dict name -> tensor)."""
        self.t += 1
        if _ADAM_SET and len(self.params) <= 16:
            if getattr(self, "_set", None) is None:
                self._set = ops.AdamSet([(_as2d(theta), self.state[name]["m1"], self.state[name]["m2"],
                                          self.state[name]["u"]) for name, theta, _ in self.params])
            self._set.step([_as2d(grads[name]) for name, _, _ in self.params], self.t, self.lr, beta1=self.beta1,
                           beta2=self.beta2, eps=self.eps, grad_sign=-1.0)
            return
        for name, theta, kind in self.params:
            st = self.state[name]
            ops.adam_step(_as2d(theta), _as2d(grads[name]), st["m1"], st["m2"], self.t, self.lr, u=st["u"],
                          beta1=self.beta1, beta2=self.beta2, eps=self.eps, grad_sign=-1.0)
