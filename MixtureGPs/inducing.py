"""Inducing-point initialisation by greedy conditional variance, on the device."""
from modulatedgps_amd.inducing import (ConditionalVariance, GreedyVarianceResult, greedy_variance,  # noqa: F401
                                       greedy_variance_device)
