"""The core feature functions; `adx_core` is exported here as well as from `.trend`, and the window statistics of `.shape` and
`.entropy`, and the bar-clock, run-length and opening-range features of `.clock`, and the causal FIR filter and the fractional
differentiation of `.fracdiff` with the search for its smallest stationary order."""
from .clock import bar_duration, bar_duration_ewma, bar_rate, dir_run_len, orb_break
from .entropy import approximate_entropy
from .fracdiff import fir, frac_diff_ffd, frac_diff_weights, min_ffd_d
from .shape import bipower_variation, hurst_exponent, rolling_kurtosis, trend_slope
from .trend import adx_core

__all__ = ["adx_core", "approximate_entropy", "bar_duration", "bar_duration_ewma", "bar_rate", "bipower_variation", "dir_run_len",
           "fir", "frac_diff_ffd", "frac_diff_weights", "hurst_exponent", "min_ffd_d", "orb_break", "rolling_kurtosis", "trend_slope"]
