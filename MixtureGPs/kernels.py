"""Stand-in for gpflow.kernels.SquaredExponential as used by the demos (demo_tf2.py:37-38), and
for the Matern32 / Matern52 kernels of the original ModulatedGPs."""
from modulatedgps_amd.kernels import Matern32, Matern52, SquaredExponential  # noqa: F401
