"""`TBMLabel` and `SampleWeights` with the constructor arguments, properties, DataFrame columns and error messages of
finmlkit/label/kit.py.  The tape is uploaded once: `compute_labels` keeps the resident columns for `compute_weights` when that is
handed the same `TradesData`."""
from __future__ import annotations

import warnings
from typing import Optional, Tuple

import numpy as np
import pandas as pd

from .. import _ffi
from ..bar.data_model import TradesData
from .betsize import bet_size_at, signal_from_probability
from .bootstrap import sequential_bootstrap
from .tbm import check_arguments
from .weights import (average_uniqueness, class_balance_weights, normalize_attribution, return_attribution, time_decay)


def _resident_tape(trades: TradesData):
    """timestamp + price of the frame in HBM.  The label kernels read nothing else, so the amount column of this DeviceTrades is
    EMPTY: it serves triple_barrier / label_concurrency / label_weights only and never leaves this module."""
    from ..engine import DeviceTrades
    ctx = _ffi.default_context()
    ts, px = _ffi.upload_columns(ctx, [np.ascontiguousarray(trades.data.timestamp.values, dtype=np.int64),
                                       np.ascontiguousarray(trades.data.price.values, dtype=np.float64)])
    return DeviceTrades(ctx, ts, px, _ffi.DeviceArray(ctx, 0, np.float32), None)


class TBMLabel:
    """Triple-barrier labels (Lopez de Prado, AFML chapter 3) for a frame of events: +1 / -1 by the sign of the return at the first
    barrier touch, or 0 / 1 meta labels when `is_meta` and the frame has an integer `side` column.  See finmlkit/label/kit.py:12-100
    for the arguments."""

    def __init__(self, features: pd.DataFrame, target_ret_col: str, min_ret: float, horizontal_barriers: Tuple[float, float],
                 vertical_barrier: pd.Timedelta, min_close_time: pd.Timedelta = pd.Timedelta(seconds=1), is_meta: bool = False):
        self._check(features, target_ret_col, min_ret, horizontal_barriers, is_meta)
        # the labelling rule
        self.target_ret_col, self.min_ret, self.is_meta = target_ret_col, min_ret, is_meta
        self.horizontal_barriers = horizontal_barriers
        self.vertical_barrier = vertical_barrier.total_seconds()
        self.min_close_time_sec = min_close_time.total_seconds()
        # the events: all that qualify, and those of the last compute_labels call (a full window inside its tape)
        self._events_all = self._select_events(features, target_ret_col, min_ret, horizontal_barriers)
        self._events = self._events_all
        self._result = None
        # the tape of the last compute_labels call in HBM (timestamp + price, 16 B/tick) and the TradesData it was made from:
        # kept only until compute_weights has used it, see there
        self._tape = self._tape_of = None

    @staticmethod
    def _check(features, target_ret_col, min_ret, horizontal_barriers, is_meta):
        if target_ret_col not in features.columns:
            raise ValueError(f"Target column '{target_ret_col}' not found in features DataFrame.")
        if not isinstance(features.index, pd.DatetimeIndex):
            raise ValueError("Features index must be a DatetimeIndex.")
        if not (isinstance(horizontal_barriers, tuple) and len(horizontal_barriers) == 2):
            raise ValueError("Horizontal barriers must be a tuple of two floats (bottom, top).")
        if min_ret < 0.:
            raise ValueError("Minimum return must be non-negative.")
        if not is_meta:
            return
        if "side" not in features.columns:
            raise ValueError("For meta labeling, 'side' column must be present in features DataFrame.")
        if not pd.api.types.is_integer_dtype(features["side"]):
            raise ValueError("The 'side' column must be of integer type (e.g., -1, 0, 1).")

    @staticmethod
    def _select_events(x: pd.DataFrame, target_ret_col: str, min_ret: float,
                             horizontal_barriers: Tuple[float, float]) -> pd.DataFrame:
        # rows from the point on where every column has started, then the events whose widest barrier reaches min_ret
        starts = [s for s in (x[col].first_valid_index() for col in x.columns) if s is not None]
        if not starts:
            raise ValueError("All columns contain only NaN values.")
        x = x.loc[max(starts):]
        x = x[x[target_ret_col].abs() * np.max(horizontal_barriers) >= min_ret]
        if x.empty:
            raise ValueError("No valid events found after filtering by minimum return and removing leading NaNs.")
        if x[target_ret_col].isna().any():
            raise ValueError(f"Target return column '{target_ret_col}' contains NaN values. Please ensure it is fully populated.")
        return x

    # ------------------------------------------------------------------ properties
    @property
    def event_count(self) -> int:
        return len(self._events)

    @property
    def first_event_timestamp(self) -> Optional[pd.Timestamp]:
        return None if self._events.empty else self._events.index[0]

    @property
    def last_event_timestamp(self) -> Optional[pd.Timestamp]:
        return None if self._events.empty else self._events.index[-1]

    @property
    def event_range(self) -> str:
        return f"From {self.first_event_timestamp} to {self.last_event_timestamp} ({self.event_count} events)"

    @property
    def features(self) -> pd.DataFrame:
        """The events the labels belong to (trailing events without a full window are dropped by compute_labels)."""
        return self._events

    @property
    def target_returns(self) -> pd.Series:
        if self.target_ret_col not in self._events.columns:
            raise ValueError(f"Target return column '{self.target_ret_col}' not found in features DataFrame.")
        return self._events[self.target_ret_col]

    @property
    def labels(self) -> pd.Series:
        if self._result is None:
            raise ValueError("Labels have not been computed yet. Call `compute_labels()` first.")
        return self._result["labels"]

    @property
    def event_returns(self) -> pd.Series:
        if self._result is None or "returns" not in self._result.columns:
            raise ValueError("Log returns have not been computed yet. Call `compute_labels()` first.")
        return self._result["returns"]

    @property
    def full_output(self) -> pd.DataFrame:
        if self._result is None:
            raise ValueError("Labels have not been computed yet. Call `compute_labels()` and `compute_weights` first.")
        return self._result

    # ------------------------------------------------------------------ the two tape walks
    def _with_full_window(self, trades: TradesData) -> pd.DataFrame:
        last = pd.Timestamp(trades.data.timestamp.values[-1], unit="ns")
        f = self._events_all
        return f[f.index + pd.Timedelta(self.vertical_barrier, unit="s") <= last]

    def compute_labels(self, trades: TradesData) -> Tuple[pd.DataFrame, pd.DataFrame]:
        """-> (features, frame of touch_time, event_idx, touch_idx, labels, returns, vertical_touch_weights)."""
        if not isinstance(trades, TradesData):
            raise ValueError("Trades must be an instance of TradesData.")
        self._events = self._with_full_window(trades)
        ts_host = trades.data.timestamp.values
        if "event_idx" in self._events.columns:
            event_idx = self._events.event_idx.values
        else:
            event_idx = np.searchsorted(ts_host, self._events.index.values.astype(np.int64))
        targets = self.target_returns.values
        side = self.features["side"].values.astype(np.int8) if self.is_meta else None
        check_arguments(len(ts_host), len(trades.data.price.values), len(event_idx), len(targets),
                        None if side is None else len(side), self.vertical_barrier, self.min_ret)
        if self._tape_of is not trades:
            self._tape, self._tape_of = _resident_tape(trades), trades
        dev, A = self._tape, _ffi.DeviceArray
        d_ev = A.from_host(dev.ctx, np.ascontiguousarray(event_idx, dtype=np.int64))
        d_tg = A.from_host(dev.ctx, np.ascontiguousarray(targets, dtype=np.float64))
        d_sd = None if side is None else A.from_host(dev.ctx, side)
        out = dev.triple_barrier(d_ev, d_tg, self.horizontal_barriers, self.vertical_barrier, self.min_close_time_sec, d_sd,
                                 self.min_ret)
        labels, touch_idx, rets, ratios = (o.to_host() for o in out[:4])
        n_skipped = int(out[4].to_host()[0])
        if n_skipped:
            warnings.warn(f"compute_labels: {n_skipped} of {len(event_idx)} events have no later tick inside their vertical barrier "
                          "and were skipped (label 0, NaN return, touch index = event index)", RuntimeWarning, stacklevel=2)
        self._result = pd.DataFrame({"touch_time": pd.to_datetime(ts_host[touch_idx]), "event_idx": event_idx, "touch_idx": touch_idx,
                                  "labels": labels, "returns": rets, "vertical_touch_weights": ratios},
                                 index=self.features.index)
        return self.features, self.full_output

    def compute_weights(self, trades: TradesData, normalized: bool = False) -> pd.DataFrame:
        """Average uniqueness and return attribution of the labelled events.  Handed the very TradesData object of compute_labels,
        the call works on the copy of its tape that compute_labels left in HBM -- the frame must not have been modified in place
        in between -- and then RELEASES that copy; any other TradesData is uploaded afresh."""
        tape = self._tape if trades is self._tape_of else None
        try:
            return SampleWeights.compute_info_weights(trades, self._result, normalized, _resident=tape)
        finally:
            self._tape = self._tape_of = None


class SampleWeights:
    """Information weights on the tape, then time decay and class balance on the events (run on the training window)."""

    @staticmethod
    def compute_info_weights(trades: TradesData, labels: pd.DataFrame, normalize: bool = False, _resident=None) -> pd.DataFrame:
        if not isinstance(trades, TradesData):
            raise ValueError("Trades must be an instance of TradesData.")
        if not isinstance(labels, pd.DataFrame):
            raise ValueError("Events must be a pandas DataFrame.")
        if "event_idx" not in labels.columns or "touch_idx" not in labels.columns:
            raise ValueError("Events DataFrame must contain 'event_idx' and 'touch_idxs' columns.")
        ev, tc = labels.event_idx.values, labels.touch_idx.values
        if _resident is not None and len(ev):
            dev, A = _resident, _ffi.DeviceArray
            d_ev = A.from_host(dev.ctx, np.ascontiguousarray(ev, dtype=np.int64))
            d_tc = A.from_host(dev.ctx, np.ascontiguousarray(tc, dtype=np.int64))
            avg, att = dev.label_weights(d_ev, d_tc, dev.label_concurrency(d_ev, d_tc))
            avg_u, info_w = avg.to_host(), att.to_host()
            if normalize:
                info_w = normalize_attribution(info_w)
        else:
            avg_u, concurrency = average_uniqueness(trades.data.timestamp.values, ev, tc)
            info_w = return_attribution(ev, tc, trades.data.price.values, concurrency, normalize)
        out = pd.DataFrame({"avg_uniqueness": avg_u}, index=labels.index)
        out["return_attribution"] = info_w
        return out

    @staticmethod
    def sequential_bootstrap(labels: pd.DataFrame, n_draws: Optional[int] = None, n_runs: int = 1, seed: int = 0) -> np.ndarray:
        """Sequential-bootstrap samples (label/bootstrap.py) of the rows of a frame with `event_idx` / `touch_idx` columns, the one
        `compute_labels` returns -> int64 row positions of shape (n_runs, n_draws), for `labels.iloc[...]`; n_draws defaults to the
        number of rows."""
        if not isinstance(labels, pd.DataFrame):
            raise ValueError("Events must be a pandas DataFrame.")
        if "event_idx" not in labels.columns or "touch_idx" not in labels.columns:
            raise ValueError("Events DataFrame must contain 'event_idx' and 'touch_idxs' columns.")
        return sequential_bootstrap(labels.event_idx.values, labels.touch_idx.values, n_draws, n_runs, seed)

    @staticmethod
    def compute_final_weights(avg_uniqueness: pd.Series, time_decay_intercept: float = 1., return_attribution: pd.Series = None,
                              vertical_touch_weights: pd.Series = None, labels: pd.Series = None) -> pd.DataFrame:
        """Time decay x information weight (x vertical touch weight), scaled to mean 1, then class balance when labels are given
        -> frame of the parts and the combined `weights`."""
        if not isinstance(avg_uniqueness, pd.Series):
            raise ValueError("avg_uniqueness must be a pandas Series.")
        if not isinstance(time_decay_intercept, (int, float)):
            raise ValueError("time_decay_intercept must be a numeric value.")
        if not -1.0 <= time_decay_intercept <= 1.0:
            raise ValueError("time_decay_intercept must lie in [-1, 1]")
        for name, s in (("return_attribution", return_attribution), ("vertical_touch_weights", vertical_touch_weights),
                        ("labels", labels)):
            if s is not None and not isinstance(s, pd.Series):
                raise ValueError(f"{name} must be a pandas Series.")
        for name, s in (("return_attribution", return_attribution), ("vertical_touch_weights", vertical_touch_weights),
                        ("labels", labels)):
            if s is not None and not avg_uniqueness.index.equals(s.index):
                raise ValueError(f"avg_uniqueness and {name} must have the same index.")
        n_events = len(avg_uniqueness)
        decay = time_decay(avg_uniqueness=avg_uniqueness.values, last_weight=time_decay_intercept)
        out = pd.DataFrame({"time_decay_weights": decay}, index=avg_uniqueness.index)
        if return_attribution is not None:
            if return_attribution.sum() <= 0:
                raise ValueError("Return attribution sum is zero or negative, cannot normalize.")
            scaled = return_attribution.values * n_events / return_attribution.sum()
            out["return_attribution"] = scaled
            combined = decay * scaled
        else:
            combined = decay * avg_uniqueness.values
        if vertical_touch_weights is not None:
            out["vertical_touch_weights"] = vertical_touch_weights.values
            combined = combined * vertical_touch_weights.values
        mean = combined.mean()
        if mean <= 0:
            raise ValueError("Mean of combined weights is zero or negative, cannot normalize.")
        base = combined / mean
        out["weights"] = class_balance_weights(labels=labels.values, base_w=base)[3] if labels is not None else base
        return out


class BetSizing:
    """From a classifier's probabilities to bet sizes (AFML chapter 10; label/betsize.py)."""

    @staticmethod
    def from_probabilities(labels: pd.DataFrame, prob, pred=None, n_classes: int = 2, step: float = 0.0) -> pd.DataFrame:
        """`labels`: a frame with `event_idx` / `touch_idx` columns, the one `compute_labels` returns; prob: the probability of the
        predicted class per row, pred: the predicted class (-1 / 1; default 1, as for meta labels).  -> a frame on the same index:
        `signal` (`signal_from_probability`, times the frame's `side` column when it has one) and `bet_size`, the average of the
        signals of the bets open at each event's own tick (`bet_size_at`), discretised when step > 0."""
        if not isinstance(labels, pd.DataFrame):
            raise ValueError("Events must be a pandas DataFrame.")
        if "event_idx" not in labels.columns or "touch_idx" not in labels.columns:
            raise ValueError("Events DataFrame must contain 'event_idx' and 'touch_idx' columns.")
        prob = np.asarray(prob, dtype=np.float64)
        if prob.ndim != 1 or len(prob) != len(labels):
            raise ValueError("from_probabilities: prob must have one value per row of the frame.")
        side = labels["side"].values if "side" in labels.columns else None
        signal = signal_from_probability(prob, None if pred is None else np.asarray(pred), side, n_classes)
        bet = bet_size_at(labels.event_idx.values, labels.touch_idx.values, signal, step=step)
        return pd.DataFrame({"signal": signal, "bet_size": bet}, index=labels.index)
