"""Labels and sample weights on the raw tick tape, computed on the MI355X (drop-in for finmlkit/label)."""
from .bootstrap import bootstrap_uniqueness, sequential_bootstrap
from .kit import SampleWeights, TBMLabel
from .otr import OTRMesh, optimal_trading_rule, ou_fit
from .tbm import triple_barrier
from .trend_scanning import trend_scanning
from .weights import average_uniqueness, class_balance_weights, return_attribution, time_decay

__all__ = ["triple_barrier", "trend_scanning", "average_uniqueness", "return_attribution", "time_decay", "class_balance_weights",
           "sequential_bootstrap", "bootstrap_uniqueness", "optimal_trading_rule", "ou_fit", "OTRMesh", "TBMLabel", "SampleWeights"]
