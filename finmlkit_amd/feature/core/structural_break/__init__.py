"""Structural-break tests on the MI355X (drop-in for finmlkit/feature/core/structural_break, and the ADF / SADF explosiveness test the
reference does not have)."""
from .adf import adf_rolling, adf_stat, sadf
from .cusum import cusum_test_developing, cusum_test_last, cusum_test_rolling

__all__ = ["adf_rolling", "adf_stat", "cusum_test_developing", "cusum_test_last", "cusum_test_rolling", "sadf"]
