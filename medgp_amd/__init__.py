"""medgp_amd -- MI355X-native hot path of bee-hive/MedGP (per-patient nlml + gradient).

The product is libmedgp_hip.so (hand-written HIP for gfx950 behind the C ABI in
include/medgp_hip.h).  This package is the thin Python host layer used by the tests and
bench.py: a ctypes binding (`capi`), the synthetic cohort generator (`synth`) and the
cohort sharding helper (`shard`); `trend` reads the slope posterior of `Context.trend`
(`prob_rising`, `rate_interval`, `grid`), `components` the per-component posterior of `Context.components`
(`table`, `select`, `band`), `functionals` builds the linear functionals of `Context.functionals` (`point`, `change`, `contrast`,
`window_mean`, `pack`, `prob_above`), `design` reads the joint covariance of `Context.functionals_joint` (`variance_reduction`,
`condition`, `greedy`: which measurement to take next), `censoring` is the numpy side of detection-limit (censored) lab values (`from_limits`,
`ep_dense`, `impute`, `exact_single`, `naive_bias`; no device call yet).  There is no CPU fallback: importing works anywhere,
but every compute call needs the built library and a HIP device.
"""
from . import capi, synth, shard, trend, components, functionals, design, censoring  # noqa: F401
from .capi import Context, MedgpError, lib_path, load  # noqa: F401
from .trend import grid, prob_rising, rate_interval  # noqa: F401

__all__ = ["capi", "synth", "shard", "trend", "components", "functionals", "design", "censoring", "Context", "MedgpError", "lib_path", "load", "grid", "prob_rising", "rate_interval"]
