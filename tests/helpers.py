"""Shared test helpers: build device models from oracle parameter sets."""
import os

import numpy as np
import torch

from oracle import cpu_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name)))


def params_from_golden(d):
    layers = {}
    for name in ("pred", "assign"):
        layers[name] = {k: d[f"{name}_{k}"] for k in ("Z", "variance", "lengthscales", "q_mu", "q_sqrt")}
    return R.SMGPParams(layers["pred"], layers["assign"], d["lik_variance"], int(d["num_data"]),
                        int(d["S"]))


def build_model(p, device, seed=0):
    """SMGP on the device from an oracle SMGPParams (float64 -> float32)."""
    from modulatedgps_amd.kernels import SquaredExponential
    from modulatedgps_amd.likelihoods import GaussianModified
    from modulatedgps_amd.models import SMGP, SVGPModified

    K = p.lik_variance.shape[1]
    lik = GaussianModified(variance=p.lik_variance, device=device)
    layers = []
    for L in (p.pred, p.assign):
        kern = SquaredExponential(variance=L["variance"], lengthscales=L["lengthscales"], device=device)
        layer = SVGPModified(kern, lik, L["Z"], num_latent_gps=K, whiten=True, device=device)
        layer.set_variational(L["q_mu"], L["q_sqrt"])
        layers.append(layer)
    return SMGP(lik, layers[0], layers[1], K=K, num_samples=p.S, num_data=p.num_data, seed=seed)


def unequal_problem(N, Mf, Ma, K, D, ls_f, ls_a, S, seed=0):
    """The synthetic problem with layers that differ: pred_layer keeps Mf inducing points
    and lengthscales ls_f, assign_layer Ma and ls_a (a scalar: isotropic; D values: ARD).
    Drawn at max(Mf, Ma) and cut per layer (a leading block of tril(q_sqrt) is lower
    triangular with the same positive diagonal).  Returns (X, Y, SMGPParams)."""
    X, Y, p = R.synthetic_problem(N, max(Mf, Ma), K, D, 1.0, state="perturbed", S=S, seed=seed)
    for L, M, ls in ((p.pred, Mf, ls_f), (p.assign, Ma, ls_a)):
        L["Z"] = L["Z"][:M].copy()
        L["q_mu"] = L["q_mu"][:M].copy()
        L["q_sqrt"] = L["q_sqrt"][:, :M, :M].copy()
        L["lengthscales"] = float(ls) if np.ndim(ls) == 0 else np.asarray(ls, np.float64).reshape(D).copy()
    return X, Y, p


# (N, Mf, Ma, K, D, ls_f, ls_a, S): models whose two layers differ in M and / or in the
# kind of lengthscale (tests/test_gpu_unequal_layers.py, tests/test_oracle.py)
UNEQUAL_CASES = {
    "a": (301, 40, 25, 3, 2, [0.3, 0.5], 0.4, 5),                      # both M <= 64; pred ARD
    "b": (777, 130, 64, 4, 3, 0.6, [0.5, 0.6, 0.9], 3),                # two row tiles / one; assign ARD
    "c": (777, 64, 130, 4, 3, [0.5, 0.6, 0.9], 0.6, 3),                # b with the larger layer second
    "d": (513, 33, 160, 5, 8, np.linspace(1.5, 2.5, 8), 2.0, 2),       # K no multiple of 4
    "e": (515, 129, 128, 8, 8, 2.0, np.linspace(1.5, 2.5, 8), 2),      # stats tile counts differ by one
    "f": (130, 1, 17, 2, 2, 0.8, 0.8, 2),                              # degenerate M = 1 layer
    "g": (301, 40, 40, 3, 2, [0.3, 0.5], 0.4, 5),                      # equal M, mixed lengthscale counts
}


def round4(n):
    return (n + 3) // 4 * 4


def poison_like(poison, shape, device):
    """A float32 tensor of the padding pattern: "nan", or "big" = 3e38 with alternating sign."""
    if poison == "nan":
        return torch.full(shape, float("nan"), dtype=torch.float32, device=device)
    n = int(np.prod(shape))
    sign = 1.0 - 2.0 * (torch.arange(n, device=device) % 2).float()
    return (3e38 * sign).reshape(shape)


def wide(values, ld, poison, device, batch_stride=None):
    """A float32 device view of values' shape over storage of row length ld (floats).  Every
    element outside the view holds the poison pattern: the padding columns and, for 3-D
    values, the gap between batch entries (batch_stride > rows * ld).  A 1-D values is one
    row.  An output buffer is wide(zeros, ld, "nan", ...) filled with a sentinel by the caller."""
    v = torch.as_tensor(np.asarray(values), dtype=torch.float32)
    if v.dim() == 1:
        v = v[None]
    rows, cols = v.shape[-2:]
    assert ld >= cols
    if v.dim() == 2:
        store = poison_like(poison, (rows * ld,), device)
        view = store.as_strided((rows, cols), (ld, 1))
    else:
        bs = rows * ld if batch_stride is None else batch_stride
        assert bs >= rows * ld
        store = poison_like(poison, (v.shape[0] * bs,), device)
        view = store.as_strided((v.shape[0], rows, cols), (bs, ld, 1))
    view.copy_(v.to(device))
    return view


def _storage_bits(view):
    n = view.untyped_storage().nbytes() // 4
    return view.as_strided((n,), (1,), 0).view(torch.int32)


def padding_intact(view, poison):
    """Every storage element outside the view still holds the poison pattern, compared as
    bit patterns (a NaN sentinel compares equal to itself)."""
    bits = _storage_bits(view).clone()
    want = poison_like(poison, (bits.numel(),), view.device).view(torch.int32).clone()
    inside = torch.zeros(bits.numel(), dtype=torch.bool, device=view.device)
    inside.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
    return bool(torch.equal(bits[~inside], want[~inside]))


def normwise(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def to_np(t):
    if isinstance(t, np.ndarray):  # the public predict_* return host arrays
        return np.asarray(t, np.float64)
    return t.detach().double().cpu().numpy()


def dev_noise(z, u, device):
    return (torch.as_tensor(z, dtype=torch.float32, device=device),
            torch.as_tensor(u, dtype=torch.float32, device=device))


def decode_cols_image(img, M, N):
    """Split-bf16 column image (modulatedgps_amd/csrc/frag_image.hpp layout
    [nb][mk][plane][lane][8]) -> float64 [M, N] = hi + mid + lo."""
    Mp, Np = -(-M // 128) * 128, -(-N // 256) * 256
    nb, nmk = Np // 32, Mp // 16
    u16 = img.detach().cpu().numpy().view(np.uint16)[: nb * nmk * 3 * 64 * 8].reshape(nb, nmk, 3, 64, 8)
    f = (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64).sum(axis=2)  # [nb][mk][64][8]
    lane, j = np.arange(64), np.arange(8)
    kp = (j[None, :] & 3) + 8 * (j[None, :] >> 2) + 4 * (lane[:, None] >> 5)          # [64][8]
    rows = 16 * np.arange(nmk)[None, :, None, None] + kp[None, None]
    cols = 32 * np.arange(nb)[:, None, None, None] + (lane & 31)[None, None, :, None]
    out = np.zeros((Mp, Np))
    out[np.broadcast_to(rows, f.shape), np.broadcast_to(cols, f.shape)] = f
    return out[:M, :N]


def decode_cols_f16(img, M, N, bound):
    """Split-f16 column image (planes 0 / 1 = fp16 hi / lo of x 2^e, e = 13 - ilogb(bound);
    modulatedgps_amd/csrc/mgp_common.hpp) -> float64 [M, N] = (hi + lo) 2^-e."""
    Mp, Np = -(-M // 128) * 128, -(-N // 256) * 256
    nb, nmk = Np // 32, Mp // 16
    u = img.detach().cpu().numpy().view(np.float16)[: nb * nmk * 3 * 64 * 8].reshape(nb, nmk, 3, 64, 8)
    e = 13 - int(np.floor(np.log2(bound)))
    f = (u[:, :, 0].astype(np.float64) + u[:, :, 1].astype(np.float64)) * 2.0 ** -e
    lane, j = np.arange(64), np.arange(8)
    kp = (j[None, :] & 3) + 8 * (j[None, :] >> 2) + 4 * (lane[:, None] >> 5)
    rows = 16 * np.arange(nmk)[None, :, None, None] + kp[None, None]
    cols = 32 * np.arange(nb)[:, None, None, None] + (lane & 31)[None, None, :, None]
    out = np.zeros((Mp, Np))
    out[np.broadcast_to(rows, f.shape), np.broadcast_to(cols, f.shape)] = f
    return out[:M, :N]
