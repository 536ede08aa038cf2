"""The core feature functions; `adx_core` is exported here as well as from `.trend`, and the window statistics of `.shape` and
`.entropy`, and the bar-clock, run-length and opening-range features of `.clock`, and the causal FIR filter and the fractional
differentiation of `.fracdiff` with the search for its smallest stationary order, and the encoding and the entropies of an encoded
series of `.lz`."""
from .clock import bar_duration, bar_duration_ewma, bar_rate, dir_run_len, orb_break
from .entropy import approximate_entropy
from .fracdiff import fir, frac_diff_ffd, frac_diff_weights, min_ffd_d
from .lz import binary_edges, encode, kontoyiannis_entropy, match_lengths, plugin_entropy, quantile_edges, sigma_edges
from .shape import bipower_variation, hurst_exponent, rolling_kurtosis, trend_slope
from .trend import adx_core

__all__ = ["adx_core", "approximate_entropy", "bar_duration", "bar_duration_ewma", "bar_rate", "binary_edges", "bipower_variation",
           "dir_run_len", "encode", "fir", "frac_diff_ffd", "frac_diff_weights", "hurst_exponent", "kontoyiannis_entropy",
           "match_lengths", "min_ffd_d", "orb_break", "plugin_entropy", "quantile_edges", "rolling_kurtosis", "sigma_edges",
           "trend_slope"]
