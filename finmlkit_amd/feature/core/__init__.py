"""The core feature functions; `adx_core` is exported here as well as from `.trend`, and the window statistics of `.shape` and
`.entropy`."""
from .entropy import approximate_entropy
from .shape import bipower_variation, hurst_exponent, rolling_kurtosis, trend_slope
from .trend import adx_core

__all__ = ["adx_core", "approximate_entropy", "bipower_variation", "hurst_exponent", "rolling_kurtosis", "trend_slope"]
