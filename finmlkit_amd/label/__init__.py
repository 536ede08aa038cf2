"""Labels and sample weights on the raw tick tape, computed on the MI355X (drop-in for finmlkit/label)."""
from .betsize import (avg_active_signals, bet_size_at, bet_size_budget, bet_size_path, bet_size_sigmoid, calibrate_w, discretise,
                      inv_price, limit_price, signal_from_probability, target_position)
from .bootstrap import bootstrap_uniqueness, sequential_bootstrap
from .kit import BetSizing, SampleWeights, TBMLabel
from .otr import OTRMesh, optimal_trading_rule, ou_fit
from .tbm import triple_barrier
from .trend_scanning import trend_scanning
from .weights import average_uniqueness, class_balance_weights, return_attribution, time_decay

__all__ = ["triple_barrier", "trend_scanning", "average_uniqueness", "return_attribution", "time_decay", "class_balance_weights",
           "sequential_bootstrap", "bootstrap_uniqueness", "optimal_trading_rule", "ou_fit", "OTRMesh", "TBMLabel", "SampleWeights",
           "bet_size_path", "bet_size_at", "avg_active_signals", "bet_size_budget", "discretise", "signal_from_probability",
           "bet_size_sigmoid", "calibrate_w", "target_position", "inv_price", "limit_price", "BetSizing"]
