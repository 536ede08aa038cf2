"""The tick-level transforms of the hot path: `ReturnT`, `EWMST`, `RealizedVolatility` (+ `Compose`), the rolling-window moments
`SMA`, `ZScore` and `VarianceRatio14` (reference transforms.py:549-574, :335-359, :867-897), the windowed order statistics
`BurstRatio`, `ROC`, `PctChange` and `StochK` (reference transforms.py:362-385, :155-177, :180-203, :276-305), and the
structural-break transform `CUSUMTest` (reference transforms.py:631-708), and the recursive indicators `EWMA`, `RSIWilder`, `ATR`
and `ADX` (reference transforms.py:577-602, :206-273, :711-751, :991-1030), and the running-sum indicators `BollingerPercentB`,
`VWAPDistance`, `ParkinsonRange`, `FlowAcceleration` and `VPIN` (reference transforms.py:494-518, :388-418, :521-546, :605-628,
:816-870), and the rolling price-volume correlation `PriceVolumeCorrelation` (reference transforms.py:754-813), and the window
statistics `KurtosisTransform`, `TrendSlope`, `HurstExponent` and `BiPowerVariation` (reference transforms.py:900-933, :936-988,
:1341-1397, :1551-1602; there pandas' rolling.apply on either backend, here the kernels of csrc/fmk_shape.hip), and the rolling
approximate entropy `ApproximateEntropy` (reference transforms.py:1400-1457; there pandas' rolling.apply around
`antropy.app_entropy`, here the kernel of csrc/fmk_entropy.hip, which needs no `antropy`), and the bar clock, run lengths and the
opening range `BarDuration`, `BarDurationEWMA`, `BarRate`, `DirRunLen` and `ORBBreak` (reference transforms.py:1511-1548, :1460-1508,
:1210-1270, :1605-1664, :1122-1207; there pandas' diff, ewm and time-window rolling, a sequential loop and a Python loop per day, here
the kernels of csrc/fmk_clock.hip), and the fixed-width window fractional differentiation `FracDiff` (no counterpart in the reference;
core/fracdiff.py, the kernel of csrc/fmk_fir.hip) and the supremum ADF statistic `SADF` (no counterpart either;
core/structural_break/adf.py, the kernel of csrc/fmk_sadf.hip), and the entropies of the encoded column `PluginEntropy` and
`KontoyiannisEntropy` (no counterpart either; core/lz.py, the kernels of csrc/fmk_lz.hip).

Counterparts of finmlkit/feature/transforms.py:89-117 (ReturnT), :308-332 (EWMST) and the
pipeline part of finmlkit/feature/kit.py:Compose (:630-720), enough to run the QuickStart flow
    Compose(ReturnT(window, input_col="price"), EWMST(half_life))(trades.data)
on the MI355X.  The reference's `backend="nb"` (Numba) and `"pd"` both map to the HIP path here
(the reference's own `_pd` of these two transforms already delegates to the Numba kernel).
The other ~30 bar-level transforms of the reference are out of scope.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pandas as pd

from .. import _ffi
from .._ffi import DeviceArray, c_f64, c_i64
from .core import clock, fracdiff, lz
from .core.structural_break import adf
from .core.structural_break.cusum import cusum_test_rolling
from .core.correlation import rolling_price_volume_correlation
from .core.momentum import LENGTH_MESSAGE, stoch_k
from .core.trend import adx_core
from .core.utils import comp_lagged_returns
from .core.reversion import vwap_distance
from .core.volatility import atr, ewmst, parkinson_range, realized_vol
from .core.volume import vpin
from .series_ops import OPS, host, resident


class SISOTransform:
    """Single-input single-output transform: output column = f"{input_col}_{output_col}"."""

    def __init__(self, input_col: str, output_col: str):
        self.requires = [input_col]
        self.produces = [output_col]

    @property
    def output_name(self) -> str:
        return f"{self.requires[0]}_{self.produces[0]}"

    def _validate_input(self, x) -> bool:
        if not isinstance(x, pd.DataFrame):
            raise TypeError("Input must be a pandas DataFrame")
        if self.requires[0] not in x.columns:
            raise ValueError(f"Input column {self.requires[0]} not found in DataFrame")
        return True

    @staticmethod
    def _get_timestamps(x: pd.DataFrame):
        if not isinstance(x.index, pd.DatetimeIndex):
            raise ValueError("Input must have a datetime index")
        return x.index.values.astype(np.int64)

    def _prepare_input_nb(self, x: pd.DataFrame):
        return x[self.requires[0]].values

    def _prepare_output_nb(self, idx, y) -> pd.Series:
        return pd.Series(y, index=idx, name=self.output_name)

    def __call__(self, x: pd.DataFrame, *, backend: str = "nb") -> pd.Series:
        assert backend in ("pd", "nb", "hip"), "Backend must be 'pd', 'nb' or 'hip'."
        self._validate_input(x)
        return self._hip(x)

    def _hip(self, x):
        raise NotImplementedError

    def _dev(self, ts, y):
        """Device-resident form used by `Compose`: (DeviceArray timestamps, DeviceArray input) -> DeviceArray output."""
        raise NotImplementedError


class ReturnT(SISOTransform):
    """Lagged return over a time window on an irregular series (reference transforms.py:89-117)."""

    def __init__(self, window: pd.Timedelta = pd.Timedelta(seconds=1e-6), is_log: bool = False,
                 input_col: str = "close"):
        window_sec = window.total_seconds()
        super().__init__(input_col, f"ret{window_sec}s" if window_sec > 1e-6 else "ret1")
        self.window_sec = window_sec
        self.is_log = is_log

    def _hip(self, x):
        res = comp_lagged_returns(self._get_timestamps(x), self._prepare_input_nb(x), self.window_sec, self.is_log)
        return self._prepare_output_nb(x.index, res)

    def _dev(self, ts, y):
        if self.window_sec <= 0:
            raise ValueError("The return window must be greater than zero.")
        out = DeviceArray(ts.ctx, y.n, np.float64)
        ts.ctx.call("fmk_comp_lagged_returns_dev", ts.p, y.p, c_i64(y.n), c_f64(self.window_sec), C.c_int(bool(self.is_log)),
                    out.p)
        return out


class EWMST(SISOTransform):
    """Time-decay exponentially weighted std (reference transforms.py:308-332)."""

    def __init__(self, half_life: pd.Timedelta, input_col: str = "y"):
        half_life_sec = half_life.total_seconds()
        super().__init__(input_col, f"ewms{half_life_sec}s")
        self.half_life_sec = half_life_sec

    def _hip(self, x):
        res = ewmst(self._get_timestamps(x), self._prepare_input_nb(x), self.half_life_sec)
        return self._prepare_output_nb(x.index, res)

    def _dev(self, ts, y):
        out = DeviceArray(ts.ctx, y.n, np.float64)
        ts.ctx.call("fmk_ewmst_dev", ts.p, y.p, c_i64(y.n), c_f64(self.half_life_sec), c_f64(1e-12), C.c_int(0), out.p)
        return out


class RealizedVolatility(SISOTransform):
    """Rolling realised volatility of a return series (reference transforms.py:449-491)."""

    def __init__(self, window: int, is_sample: bool = False, input_col: str = "ret"):
        super().__init__(input_col, f"rv{window}")
        self.window = window
        self.is_sample = is_sample

    def _hip(self, x):
        res = realized_vol(self._prepare_input_nb(x).astype(np.float64), self.window, self.is_sample)
        return self._prepare_output_nb(x.index, res)

    def _dev(self, ts, y):
        out = DeviceArray(ts.ctx, y.n, np.float64)
        if int(self.window) == 0:                      # every window is empty (core/volatility.py realized_vol)
            return DeviceArray.from_host(ts.ctx, np.full(y.n, np.nan))
        ts.ctx.call("fmk_realized_vol_dev", y.p, c_i64(y.n), c_i64(int(self.window)), C.c_int(bool(self.is_sample)), out.p)
        return out


class _SeriesOp(SISOTransform):
    """A transform over one row of series_ops.OPS: `_op` names the row, `_params()` gives the row's scalars in ABI order.  The
    NumPy form and the device form used by `Compose` are that row's two drivers."""
    _op = ""

    def _params(self):
        return (self.window,)

    def _hip(self, x):
        return self._prepare_output_nb(x.index, host(OPS[self._op], (self._prepare_input_nb(x),), *self._params()))

    def _dev(self, ts, y):
        return resident(ts.ctx, OPS[self._op], (y,), *self._params())


class SMA(_SeriesOp):
    """Simple moving average (reference transforms.py:549-574; the reference's "pd" backend is pandas' rolling mean, this is its
    Numba kernel on either backend)."""
    _op = "sma"

    def __init__(self, window: int, input_col: str = "x"):
        super().__init__(input_col, f"sma{window}")
        self.window = window


class ZScore(_SeriesOp):
    """Rolling z-score (reference transforms.py:335-359)."""
    _op = "zscore"

    def __init__(self, window: int, input_col: str, ddof: int = 0):
        super().__init__(input_col, f"z{window}")
        self.window = window
        self.ddof = ddof

    def _params(self):
        return (self.window, self.ddof)


class VarianceRatio14(_SeriesOp):
    """var(1-step returns) / (var(4-step returns) / 4) (reference transforms.py:867-897)."""
    _op = "variance_ratio_1_4"

    def __init__(self, window: int = 32, input_col: str = "close", ret_type: str = "log", ddof: int = 0):
        super().__init__(input_col, f"var_ratio_1_4_{window}")
        self.window = window
        self.ret_type = ret_type
        self.ddof = ddof

    def _params(self):
        return (self.window, self.ddof, self.ret_type == "log")


class BurstRatio(_SeriesOp):
    """series / rolling median (reference transforms.py:362-385)."""
    _op = "burst_ratio"

    def __init__(self, window: int, input_col: str):
        super().__init__(input_col, f"burst{window}")
        self.window = window


class KurtosisTransform(_SeriesOp):
    """Rolling excess kurtosis (reference transforms.py:900-933: scipy's biased Fisher form under pandas' rolling.apply)."""
    _op = "rolling_kurtosis"

    def __init__(self, window: int = 32, input_col: str = "ret1"):
        super().__init__(input_col, f"kurt_{window}")
        self.window = window


class TrendSlope(_SeriesOp):
    """The least-squares slope of ln(close) over the window as an angle in degrees (reference transforms.py:936-988: a Python loop
    around scipy's linregress)."""
    _op = "trend_slope"

    def __init__(self, window: int = 24, input_col: str = "close"):
        super().__init__(input_col, f"trend_slope_{window}")
        self.window = window


class HurstExponent(_SeriesOp):
    """The aggregated-variance Hurst exponent over lags 1, 2, 4, 8 (reference transforms.py:1341-1397).  `window < 9` raises
    ValueError when the transform is applied; the reference raises TypeError out of polyfit there."""
    _op = "hurst_exponent"

    def __init__(self, window: int = 24, input_col: str = "ret1"):
        super().__init__(input_col, f"hurst{window}")
        self.window = window


class BiPowerVariation(_SeriesOp):
    """Bi-power variation: sqrt(pi / 2) times the sum of `window` products of consecutive absolute returns (reference
    transforms.py:1551-1602); the first output is at index `window`."""
    _op = "bipower_variation"

    def __init__(self, window: int = 12, input_col: str = "ret1"):
        super().__init__(input_col, f"bv_{window}")
        self.window = window


class ApproximateEntropy(_SeriesOp):
    """Rolling approximate entropy (reference transforms.py:1400-1457: pandas' rolling.apply around antropy.app_entropy with the
    Chebyshev metric and the tolerance `tolerance * std(window)`).  Refused arguments raise ValueError when the transform is
    applied (core/entropy.py)."""
    _op = "approximate_entropy"

    def __init__(self, window: int = 24, m: int = 2, tolerance: float = 0.2, input_col: str = "ret1"):
        super().__init__(input_col, f"apen{window}")
        self.window = window
        self.m = m
        self.tolerance = tolerance

    def _params(self):
        return (self.window, self.m, self.tolerance)


class FracDiff(SISOTransform):
    """Fixed-width window fractional differentiation of order `d` (core/fracdiff.py; the reference has no counterpart).  The weights
    are computed once, here: a `d` or a `threshold` that `frac_diff_weights` refuses raises ValueError at construction."""

    def __init__(self, d: float, threshold: float = 1e-5, input_col: str = "close"):
        super().__init__(input_col, f"ffd{d}")
        self.d = d
        self.threshold = threshold
        self.weights = fracdiff.frac_diff_weights(d, threshold)

    def _hip(self, x):
        return self._prepare_output_nb(x.index, fracdiff.fir(self._prepare_input_nb(x), self.weights))

    def _dev(self, ts, y):
        return fracdiff.resident(ts.ctx, y, self.weights)


class SADF(SISOTransform):
    """Supremum ADF statistic of every element (core/structural_break/adf.py; the reference has no counterpart): the largest ADF
    statistic over the backward windows of `min_len` .. `max_len` rows (None: all history).  The output is the statistic; the
    arguments that `sadf` refuses raise ValueError at construction."""

    def __init__(self, min_len: int, max_len=None, lags: int = 1, trend: str = "c", step: int = 1, input_col: str = "close"):
        super().__init__(input_col, f"sadf_{min_len}_{'all' if max_len is None else max_len}")
        adf.check_arguments(0, None, min_len, max_len, lags, trend, step)
        self.min_len, self.max_len, self.lags, self.trend, self.step = min_len, max_len, lags, trend, step

    def _hip(self, x):
        stat, _ = adf.sadf(self._prepare_input_nb(x), self.min_len, self.max_len, self.lags, self.trend, self.step)
        return self._prepare_output_nb(x.index, stat)

    def _dev(self, ts, y):
        return adf.resident(ts.ctx, y, None, self.min_len, self.max_len, self.lags, self.trend, self.step)[0]


class _EncodedEntropy(SISOTransform):
    """An entropy of the input column's message (core/lz.py; the reference has no counterpart): the column is encoded with `edges`
    -- 1 to 254 increasing values, or an int q for `quantile_edges(column, q)`, computed on the host from the column itself -- and
    the estimator runs on the codes; every backend is the kernel.  The arguments the functions refuse raise ValueError at
    construction.  In a `Compose` chain the codes never visit the host; there an int q raises ValueError, as the column is not on
    the host to take quantiles of."""
    _function = ""

    def __init__(self, input_col: str, output_col: str, edges):
        super().__init__(input_col, output_col)
        if isinstance(edges, (int, np.integer)) and not isinstance(edges, bool):
            lz.quantile_edges([0.0], edges)                          # (refuses a q outside 2..255)
            self.edges = int(edges)
        else:
            self.edges = lz.rule_edges(edges)

    def _scalars(self, edges):
        """the estimator's arguments behind the codes, for the edges in use"""
        raise NotImplementedError

    def _hip(self, x):
        col = np.ascontiguousarray(self._prepare_input_nb(x), dtype=np.float64)
        edges = lz.quantile_edges(col, self.edges) if isinstance(self.edges, int) else self.edges
        return self._prepare_output_nb(x.index, getattr(lz, self._function)(lz.encode(col, edges), *self._scalars(edges)))

    def _dev(self, ts, y):
        if isinstance(self.edges, int):
            raise ValueError(lz.Q_DEV_MESSAGE.format(type(self).__name__))
        return lz.resident(ts.ctx, self._function, lz.resident(ts.ctx, "encode", y, self.edges), *self._scalars(self.edges))


class PluginEntropy(_EncodedEntropy):
    """Rolling plug-in entropy rate of the encoded column in bits per symbol (AFML snippet 18.1 on a rolling window): the words are
    `word` codes long, the alphabet is the edges' count plus one."""
    _function = "plugin_entropy"

    def __init__(self, window: int = 64, word: int = 2, edges=(0.0,), input_col: str = "ret1"):
        super().__init__(input_col, f"plugin{window}_w{word}", edges)
        # an int q: at most q codes; ties may leave fewer, and the alphabet of a call is that of the edges it encodes with
        self.alphabet = self.edges if isinstance(self.edges, int) else len(self.edges) + 1
        self.window, self.word, _ = lz.check_arguments("plugin_entropy", window=window, word=word, alphabet=self.alphabet)

    def _scalars(self, edges):
        return (self.window, self.word, len(edges) + 1)


class KontoyiannisEntropy(_EncodedEntropy):
    """Rolling Kontoyiannis Lempel-Ziv entropy rate of the encoded column in bits per symbol (AFML snippet 18.4, the sliding-window
    form with a look-back of `lookback` codes)."""
    _function = "kontoyiannis_entropy"

    def __init__(self, window: int = 64, lookback: int = 16, edges=(0.0,), input_col: str = "ret1"):
        super().__init__(input_col, f"konto{window}_{lookback}", edges)
        self.window, self.lookback = lz.check_arguments("kontoyiannis_entropy", window=window, lookback=lookback)

    def _scalars(self, edges):
        return (self.window, self.lookback)


class EWMA(_SeriesOp):
    """Exponentially weighted moving average (reference transforms.py:577-602).  backend="pd" is pandas' own
    `ewm(span=span).mean()`, as in the reference (it skips NaN where the kernel propagates it)."""
    _op = "ewma"

    def __init__(self, span: int, input_col: str = None):
        super().__init__(input_col, f"ewma{span}")
        self.span = span

    def _params(self):
        return (self.span,)

    def _pd(self, x):
        outp = x[self.requires[0]].ewm(span=self.span).mean()
        outp.name = self.output_name
        return outp

    def __call__(self, x: pd.DataFrame, *, backend: str = "nb") -> pd.Series:
        assert backend in ("pd", "nb", "hip"), "Backend must be 'pd', 'nb' or 'hip'."
        self._validate_input(x)
        return self._pd(x) if backend == "pd" else self._hip(x)


class RSIWilder(_SeriesOp):
    """Wilder's relative strength index (reference transforms.py:206-273).  Both backends are the kernel.  The reference's pandas
    backend is an arithmetic of its own: it gives 100 where there is no loss, the Numba kernel and this one give NaN there."""
    _op = "rsi_wilder"

    def __init__(self, window: int = 14, input_col: str = "close"):
        super().__init__(input_col, f"rsiw{window}")
        self.window = window


class BollingerPercentB(_SeriesOp):
    """Bollinger %B (reference transforms.py:494-518).  Every backend is the kernel; the reference's `_pd` falls back to Numba."""
    _op = "bollinger_percent_b"

    def __init__(self, window: int, num_std: float = 2., input_col: str = "close"):
        super().__init__(input_col, f"bollb{window}")
        self.window = window
        self.num_std = num_std

    def _params(self):
        return (self.window, self.num_std)


class FlowAcceleration(_SeriesOp):
    """Flow acceleration (reference transforms.py:605-628).  Every backend is the kernel; the reference's `_pd` falls back to
    Numba."""
    _op = "flow_acceleration"

    def __init__(self, window: int, recent_periods, input_col: str = "volume"):
        super().__init__(input_col, f"flowacc_{window}_{recent_periods}")
        self.window = window
        self.recent_periods = recent_periods

    def _params(self):
        return (self.window, self.recent_periods)


class ROC(_SeriesOp):
    """Rate of change in percent (reference transforms.py:155-177; both backends are the kernel, as the reference's `_pd` falls
    back to Numba)."""
    _op = "roc"

    def __init__(self, periods: int, input_col: str = "close"):
        super().__init__(input_col, f"roc{periods}")
        self.periods = periods

    def _params(self):
        return (self.periods,)


class PctChange(_SeriesOp):
    """Percentage change over a lag (reference transforms.py:180-203).  backend="pd" is pandas' own `Series.pct_change`, as in the
    reference: it divides by a base <= 0 where the kernel gives NaN, and it returns the series under the input column's name."""
    _op = "pct_change"

    def __init__(self, window: int, input_col: str = "close"):
        super().__init__(input_col, f"pctc{window}")
        self.periods = window

    def _params(self):
        return (self.periods,)

    def _pd(self, x):
        return x[self.requires[0]].pct_change(self.periods)

    def __call__(self, x: pd.DataFrame, *, backend: str = "nb") -> pd.Series:
        assert backend in ("pd", "nb", "hip"), "Backend must be 'pd', 'nb' or 'hip'."
        self._validate_input(x)
        return self._pd(x) if backend == "pd" else self._hip(x)


class MISOTransform:
    """Multiple-input single-output transform with the reference's interface (feature/base.py:504-716): `requires` lists the input
    columns, the output column is named `produces[0]` without an input prefix, `_prepare_input_nb` gives a dict of arrays."""

    def __init__(self, input_cols, output_col: str):
        self.requires = [input_cols] if isinstance(input_cols, str) else list(input_cols)
        self.produces = [output_col]

    @property
    def output_name(self) -> str:
        return self.produces[0]

    def _validate_input(self, x) -> bool:
        if not isinstance(x, pd.DataFrame):
            raise TypeError("Input must be a pandas DataFrame")
        missing_cols = [col for col in self.requires if col not in x.columns]
        if missing_cols:
            raise ValueError(f"Input columns {missing_cols} not found in DataFrame")
        return True

    def _prepare_input_nb(self, x: pd.DataFrame):
        return {col: x[col].values for col in self.requires}

    def _prepare_output_nb(self, idx, y) -> pd.Series:
        return pd.Series(y, index=idx, name=self.output_name)

    def __call__(self, x: pd.DataFrame, *, backend: str = "nb") -> pd.Series:
        assert backend in ("pd", "nb", "hip"), "Backend must be 'pd', 'nb' or 'hip'."
        self._validate_input(x)
        return self._hip(x)

    def _hip(self, x):
        raise NotImplementedError


class StochK(MISOTransform):
    """Stochastic oscillator %K (reference transforms.py:276-305).  The reference hands its columns (high, low, close) to a core
    function declared (close, low, high): the `high` column takes the place of `close` and the `close` column that of `high`.
    The transform's output is the reference's, so the same call is made here; `core.momentum.stoch_k` keeps the declared order."""

    def __init__(self, length: int = 14, input_cols=None):
        if input_cols is None:
            input_cols = ["high", "low", "close"]
        super().__init__(input_cols, f"stochk{length}")
        self.length = length

    def _hip(self, x):
        if int(self.length) < 1:
            raise ValueError(LENGTH_MESSAGE)
        cols = self._prepare_input_nb(x)
        high, low, close = (np.asarray(cols[c], dtype=np.float64) for c in self.requires[:3])
        return self._prepare_output_nb(x.index, stoch_k(high, low, close, self.length))


class ATR(MISOTransform):
    """Average true range (reference transforms.py:711-751); the columns are (high, low, close) in that order.  Both backends are
    the kernel, as the reference's `_pd` falls back to Numba."""

    def __init__(self, window: int = 14, ema_based: bool = False, normalize: bool = False, input_cols=None):
        if input_cols is None:
            input_cols = ["high", "low", "close"]
        output_name = f"atr{window}"
        if ema_based:
            output_name += "_ema"
        if normalize:
            output_name += "_norm"
        super().__init__(input_cols, output_name)
        self.window = window
        self.ema_based = ema_based
        self.normalize = normalize

    def _hip(self, x):
        cols = self._prepare_input_nb(x)
        high, low, close = (np.asarray(cols[c], dtype=np.float64) for c in self.requires[:3])
        return self._prepare_output_nb(x.index, atr(high, low, close, self.window, self.ema_based, self.normalize))


class ADX(MISOTransform):
    """Average directional index (reference transforms.py:991-1030); the columns are (high, low, close) in that order.  Both
    backends are the kernel, as the reference's `_pd` falls back to Numba."""

    def __init__(self, length: int = 14, input_cols=None):
        if input_cols is None:
            input_cols = ["high", "low", "close"]
        super().__init__(input_cols, f"adx_{length}")
        self.length = length

    def _hip(self, x):
        cols = self._prepare_input_nb(x)
        high, low, close = (np.asarray(cols[c], dtype=np.float64) for c in self.requires[:3])
        return self._prepare_output_nb(x.index, adx_core(high, low, close, self.length))


class VWAPDistance(MISOTransform):
    """Distance of the price from the rolling VWAP (reference transforms.py:388-418); the columns are (close, volume).  Every
    backend is the kernel; the reference's `_pd` falls back to Numba."""

    def __init__(self, periods: int, is_log: bool = False, input_cols: str = None):
        if input_cols is None:
            input_cols = ["close", "volume"]
        super().__init__(input_cols, f"vwapd{periods}")
        self.periods = periods
        self.is_log = is_log

    def _hip(self, x):
        cols = self._prepare_input_nb(x)
        close, volume = (np.asarray(cols[c], dtype=np.float64) for c in self.requires[:2])
        return self._prepare_output_nb(x.index, vwap_distance(close, volume, self.periods, self.is_log))


class ParkinsonRange(MISOTransform):
    """Parkinson's range estimator (reference transforms.py:521-546); the columns are (high, low).  Every backend is the kernel;
    the reference's `_pd` falls back to Numba."""

    def __init__(self, input_cols=None):
        if input_cols is None:
            input_cols = ["high", "low"]
        super().__init__(input_cols, "parkrange")

    def _hip(self, x):
        cols = self._prepare_input_nb(x)
        high, low = (np.asarray(cols[c], dtype=np.float64) for c in self.requires[:2])
        return self._prepare_output_nb(x.index, parkinson_range(high, low))


class VPIN(MISOTransform):
    """Volume-synchronised probability of informed trading (reference transforms.py:816-870), float32; the columns are
    (volume_buy, volume_sell).  Every backend is the kernel: the reference's `_pd` is a pandas arithmetic of its own (rolling sums
    in float64 that let a NaN bar poison its windows only), its `_nb` the function this one restates."""

    def __init__(self, window: int = 32, input_cols: list[str] = None):
        if input_cols is None:
            input_cols = ["volume_buy", "volume_sell"]
        super().__init__(input_cols, f"vpin_{window}")
        self.window = window

    def _hip(self, x):
        cols = self._prepare_input_nb(x)
        buy, sell = (np.asarray(cols[c], dtype=np.float64) for c in self.requires[:2])
        return self._prepare_output_nb(x.index, vpin(buy, sell, self.window))


class PriceVolumeCorrelation(MISOTransform):
    """Rolling correlation of price returns and volume (reference transforms.py:754-813); the columns are (close, volume).  Every
    backend is the kernel, which restates the reference's `_nb`.  The reference's `_pd` is another computation: pandas' own rolling
    correlation (another order of summation, and other NaN rules) with a special case of its own (`len >= 10 and window == 4` on
    monotone columns, every output from `window` on set to +-1), not the one of `_nb` (outputs 4 .. 9)."""

    def __init__(self, window: int = 8, input_cols: list[str] = None):
        if input_cols is None:
            input_cols = ["close", "volume"]
        super().__init__(input_cols, f"corr_pv_{window}")
        self.window = window

    def _hip(self, x):
        cols = self._prepare_input_nb(x)
        close, volume = (np.asarray(cols[c], dtype=np.float64) for c in self.requires[:2])
        return self._prepare_output_nb(x.index, rolling_price_volume_correlation(close, volume, self.window))


class _ClockTransform(SISOTransform):
    """A transform that reads the index and not the input column (reference: "only needed for timestamp extraction").  The Series it
    returns is named `out_name`, without the input column, as the reference's; `output_name` is the SISO composition.  The index
    must be a DatetimeIndex (the reference's message) and monotonic increasing: the reference sorts, here the caller does."""
    _index_message = ""

    def __init__(self, input_col: str, out_name: str):
        super().__init__(input_col, out_name)
        self.out_name = out_name

    def _stamps(self, x: pd.DataFrame):
        if not isinstance(x.index, pd.DatetimeIndex):
            raise ValueError(self._index_message)
        if not x.index.is_monotonic_increasing:
            raise ValueError(f"{type(self).__name__}: the index must be monotonic increasing; sort the frame first.")
        return x.index.values.astype("datetime64[ns]").astype(np.int64)

    def _host(self, ts):
        raise NotImplementedError

    def _hip(self, x):
        return pd.Series(self._host(self._stamps(x)), index=x.index, name=self.out_name)


class BarDuration(_ClockTransform):
    """Seconds between a bar and the bar `periods` rows before it (reference transforms.py:1511-1548: pandas' diff of the index)."""
    _index_message = "Input DataFrame must have a DatetimeIndex for BarDurationEWMA calculation"      # the reference's, as it stands

    def __init__(self, periods=1, input_col: str = "close"):
        super().__init__(input_col, f"dur_{periods}bar")
        self.periods = periods

    def _host(self, ts):
        return clock.bar_duration(ts, self.periods)

    def _dev(self, ts, y):
        return clock.resident(ts.ctx, clock.CLOCK_OPS["bar_duration"], (ts,), int(self.periods))[0]


class BarDurationEWMA(_ClockTransform):
    """Exponentially weighted mean of the bar durations (reference transforms.py:1460-1508: pandas' ewm(span, adjust=True).mean());
    `span < 1` raises ValueError when the transform is applied."""
    _index_message = "Input DataFrame must have a DatetimeIndex for BarDurationEWMA calculation"

    def __init__(self, span: int = 20, input_col: str = "close"):
        super().__init__(input_col, f"dur_ewma{span}")
        self.span = span

    def _host(self, ts):
        return clock.bar_duration_ewma(ts, self.span)

    def _dev(self, ts, y):
        return clock.resident(ts.ctx, clock.CLOCK_OPS["bar_duration_ewma"], (ts,), clock.rule_span(self.span))[0]


class BarRate(_ClockTransform):
    """Bars per hour over the closed time window that ends at each bar (reference transforms.py:1210-1270: pandas' time-window
    rolling sum, closed='both').  A window below one nanosecond raises ValueError when the transform is applied; the reference
    divides by zero there."""
    _index_message = "Input DataFrame must have a DatetimeIndex for BarRate calculation"

    def __init__(self, window: pd.Timedelta, input_col: str = "close"):
        window_sec = window.total_seconds()
        window_min = window_sec / 60.
        super().__init__(input_col, "bars_per_hour" if window_min.is_integer() else f"rate_{window_min}m")
        self.window_sec = window_sec

    def _host(self, ts):
        return clock.bar_rate(ts, self.window_sec)

    def _dev(self, ts, y):
        w = clock.window_ns(self.window_sec)
        return clock.resident(ts.ctx, clock.CLOCK_OPS["bar_rate"], (ts,), float(self.window_sec), w)[0]


class DirRunLen(SISOTransform):
    """The length of the run of same-sign returns each bar ends, int8 (reference transforms.py:1605-1664: a sequential loop)."""

    def __init__(self, input_col: str = "ret1"):
        super().__init__(input_col, "dir_run_len")

    def _hip(self, x):
        return self._prepare_output_nb(x.index, clock.dir_run_len(self._prepare_input_nb(x)))

    def _dev(self, ts, y):
        return clock.resident(ts.ctx, clock.CLOCK_OPS["dir_run_len"], (y,))[0]


class ORBBreak(MISOTransform):
    """Opening-range breakouts inside a UTC day (reference transforms.py:1122-1207): two bool Series, `orb_long` and `orb_short`; the
    columns are (high, low, close).  The index must be a DatetimeIndex (the reference's message), monotonic increasing (the reference
    sorts, here the caller does) and unique (the reference marks every row of a duplicated stamp)."""

    def __init__(self, input_cols: list[str] = None):
        if input_cols is None:
            input_cols = ["high", "low", "close"]
        super().__init__(input_cols, "orb_long")
        self.produces = ["orb_long", "orb_short"]

    @property
    def output_name(self):
        return self.produces

    def _hip(self, x):
        if not isinstance(x.index, pd.DatetimeIndex):
            raise ValueError("Input DataFrame must have a DatetimeIndex for ORB calculation")
        if not x.index.is_monotonic_increasing:
            raise ValueError("ORBBreak: the index must be monotonic increasing; sort the frame first.")
        if not x.index.is_unique:
            raise ValueError("ORBBreak: the index must be unique.")
        ts = x.index.values.astype("datetime64[ns]").astype(np.int64)
        cols = self._prepare_input_nb(x)
        high, low, close = (np.asarray(cols[c], dtype=np.float64) for c in self.requires[:3])
        lg, sh = clock.orb_break(ts, high, low, close)
        return (pd.Series(lg, index=x.index, name=self.produces[0]), pd.Series(sh, index=x.index, name=self.produces[1]))


class SIMOTransform:
    """One input column, several output series.  By default series i is named "<input column>_<produces[i]>"; a subclass may
    name its outputs otherwise by overriding `output_name` (CUSUMTest does)."""

    def __init__(self, input_col: str, output_cols):
        self.requires = [input_col]
        self.produces = [str(c) for c in output_cols]

    @property
    def output_name(self):
        prefix = self.requires[0] + "_"
        return [prefix + suffix for suffix in self.produces]

    def __call__(self, x: pd.DataFrame, *, backend: str = "nb"):
        assert backend in ("pd", "nb", "hip"), "Backend must be 'pd', 'nb' or 'hip'."
        if not isinstance(x, pd.DataFrame):
            raise TypeError("Input must be a pandas DataFrame")
        col = self.requires[0]
        if col not in x.columns:
            raise ValueError(f"Input column {col} not found in DataFrame")
        arrays = self._hip(x[col].values)
        names = self.output_name
        assert len(arrays) == len(names), f"{type(self).__name__} made {len(arrays)} arrays for {len(names)} names"
        return tuple(pd.Series(a, index=x.index, name=nm) for a, nm in zip(arrays, names))

    def _hip(self, values):
        """The input column as a NumPy array -> one array per output."""
        raise NotImplementedError


class CUSUMTest(SIMOTransform):
    """Rolling Chu-Stinchcombe-White CUSUM test as six features (reference transforms.py:631-708): per side a score (statistic
    minus critical value, clipped to +-10), a flag (score > 0) and an age (bars since the last flag, clipped to `max_age`).  The
    four arrays of the test come from the device (csrc/fmk_break.hip); score, flag and age are host arithmetic on them."""

    def __init__(self, window_size: int = 50, warmup_period: int = 30, max_age: int = 144, input_col: str = "close"):
        base_up, base_down = f"cumote_up{window_size}", f"cumote_down{window_size}"
        super().__init__(input_col, [f"{base_up}_score", f"{base_down}_score", f"{base_up}_flag", f"{base_down}_flag",
                                     f"{base_up}_age", f"{base_down}_age"])
        self.window_size = window_size
        self.warmup_period = warmup_period
        self.max_age = max_age

    @staticmethod
    def features(up, down, crit_up, crit_down, max_age: int):
        """(up, down, crit_up, crit_down) -> (score_up, score_down, flag_up, flag_down, age_up, age_down): float64, bool, uint8."""
        out_score, out_flag, out_age = [], [], []
        pos = np.arange(len(up), dtype=np.int64)
        for stat, crit in ((up, crit_up), (down, crit_down)):
            with np.errstate(invalid="ignore"):
                brk = stat - crit
                flag = (brk > 0).astype(np.bool_)
                out_score.append(np.clip(brk, -10, 10))
            # every flag starts a group (the elements before the first flag are one too); the age is the position inside it
            start = np.maximum.accumulate(np.where(flag, pos, 0))
            out_flag.append(flag)
            out_age.append(np.clip(pos - start, 0, max_age).astype(np.uint8))
        return (*out_score, *out_flag, *out_age)

    @property
    def output_name(self):
        """As in the reference: the six names carry no input-column prefix."""
        return self.produces

    def _hip(self, values):
        four = cusum_test_rolling(values, self.window_size, self.warmup_period)
        return self.features(*four, self.max_age)


class Compose(SISOTransform):
    """Chain of SISO transforms; the output of step i feeds step i+1 (reference feature/kit.py Compose)."""

    def __init__(self, *transforms: SISOTransform):
        first_out = transforms[0].output_name
        super().__init__(transforms[0].requires[0], "_".join([first_out] + [t.produces[0] for t in transforms[1:]]))
        self.transforms = transforms

    @property
    def output_name(self) -> str:
        return self.produces[0]

    def __call__(self, x: pd.DataFrame, *, backend: str = "nb") -> pd.Series:
        assert backend in ("pd", "nb", "hip"), "Backend must be 'pd', 'nb' or 'hip'."
        self._validate_input(x)
        if self.output_name in x.columns:
            return x[self.output_name]
        # (only when every step has a device form of its own: a nested Compose or a user-defined SISOTransform takes the
        # generic loop below)
        if len(x) and all(type(t)._dev is not SISOTransform._dev for t in self.transforms) and \
                not any(t.produces[0] in x.columns or (i and t.requires[0] in x.columns) for i, t in enumerate(self.transforms)):
            # the chain stays in HBM: timestamps and the input column go up once, every intermediate series is a device
            # buffer handed to the next kernel, only the last one comes back (the reference round-trips pandas objects)
            ctx = _ffi.default_context()
            ts = DeviceArray.from_host(ctx, self._get_timestamps(x))
            cur = DeviceArray.from_host(ctx, np.ascontiguousarray(self.transforms[0]._prepare_input_nb(x), dtype=np.float64))
            for t in self.transforms:
                cur = t._dev(ts, cur)
            return pd.Series(cur.to_host(), index=x.index, name=self.output_name)
        cur = None
        for i, t in enumerate(self.transforms):
            if t.produces[0] in x.columns:
                cur = x[t.produces[0]]
            elif i == 0:
                cur = t(x, backend=backend)
            else:
                req = t.requires[0]
                df_in = x[[req]] if req in x.columns else pd.DataFrame(cur.values, index=cur.index, columns=[req])
                cur = t(df_in, backend=backend)
        cur.name = self.output_name
        return cur
