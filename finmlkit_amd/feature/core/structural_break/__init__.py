"""Structural-break tests on the MI355X (drop-in for finmlkit/feature/core/structural_break)."""
from .cusum import cusum_test_developing, cusum_test_last, cusum_test_rolling

__all__ = ["cusum_test_developing", "cusum_test_last", "cusum_test_rolling"]
