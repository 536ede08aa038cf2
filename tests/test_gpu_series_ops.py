"""The three routes to a series feature on the MI355X -- the NumPy drop-in of feature/core, the `DeviceTrades` method and, where the
feature has a SISO transform, a one-step `Compose` -- give the same bits for every row of feature/series_ops.py: they end in the same
kernel, so there is no tolerance.  One random series of 300 elements (longer than a wave, shorter than any tile) with a NaN in the
middle, and its first element alone."""
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from finmlkit_amd.feature.series_ops import OPS

pytestmark = pytest.mark.gpu

N, NAN_AT, W = 300, 150, 24


def routes():
    """row -> (drop-in on the host columns h, DeviceTrades method on the resident columns d, transform on column "x" or None)"""
    from finmlkit_amd.feature import transforms as T
    from finmlkit_amd.feature.core import correlation, entropy, ma, momentum, reversion, shape, trend, utils, volatility, volume
    return {
        "sma": (lambda h: ma.sma(h.x, W), lambda t, d: t.sma(d.x, W), T.SMA(W, "x")),
        "zscore": (lambda h: utils.comp_zscore(h.x, W, 1), lambda t, d: t.zscore(d.x, W, 1), T.ZScore(W, "x", 1)),
        "rolling_variance": (lambda h: volatility.rolling_variance_nb(h.x, W, 1, 2), lambda t, d: t.rolling_variance(d.x, W, 1, 2), None),
        "variance_ratio_1_4": (lambda h: volatility.variance_ratio_1_4_core(h.x, W, 0, "log"),
                               lambda t, d: t.variance_ratio_1_4(W, 0, "log", series=d.x), T.VarianceRatio14(W, "x")),
        "burst_ratio": (lambda h: utils.comp_burst_ratio(h.x, W), lambda t, d: t.burst_ratio(d.x, W), T.BurstRatio(W, "x")),
        "roc": (lambda h: momentum.roc(h.x, W), lambda t, d: t.roc(d.x, W), T.ROC(W, "x")),
        "pct_change": (lambda h: utils.pct_change(h.x, W), lambda t, d: t.pct_change(d.x, W), T.PctChange(W, "x")),
        "stoch_k": (lambda h: momentum.stoch_k(h.x, h.low, h.high, W), lambda t, d: t.stoch_k(d.x, d.low, d.high, W), None),
        "ewma": (lambda h: ma.ewma(h.x, 10), lambda t, d: t.ewma(d.x, 10), T.EWMA(10, "x")),
        "rsi_wilder": (lambda h: momentum.rsi_wilder(h.x, W), lambda t, d: t.rsi_wilder(d.x, W), T.RSIWilder(W, "x")),
        "true_range": (lambda h: volatility.true_range(h.high, h.low, h.x), lambda t, d: t.true_range(d.high, d.low, d.x), None),
        "atr": (lambda h: volatility.atr(h.high, h.low, h.x, W, True, True), lambda t, d: t.atr(d.high, d.low, d.x, W, True, True), None),
        "adx": (lambda h: trend.adx_core(h.high, h.low, h.x, W), lambda t, d: t.adx(d.high, d.low, d.x, W), None),
        "bollinger_percent_b": (lambda h: volatility.bollinger_percent_b(h.x, W, 2.0), lambda t, d: t.bollinger_percent_b(d.x, W, 2.0),
                                T.BollingerPercentB(W, 2.0, "x")),
        "vwap_distance": (lambda h: reversion.vwap_distance(h.x, h.rev, W, True), lambda t, d: t.vwap_distance(d.x, d.rev, W, True), None),
        "flow_acceleration": (lambda h: volume.comp_flow_acceleration(h.x, W, 6), lambda t, d: t.flow_acceleration(d.x, W, 6),
                              T.FlowAcceleration(W, 6, "x")),
        "vpin": (lambda h: volume.vpin(h.x, h.rev, W), lambda t, d: t.vpin(d.x, d.rev, W), None),
        "parkinson_range": (lambda h: volatility.parkinson_range(h.high, h.low), lambda t, d: t.parkinson_range(d.high, d.low), None),
        "price_volume_corr": (lambda h: correlation.rolling_price_volume_correlation(h.x, h.rev, W),
                              lambda t, d: t.price_volume_corr(d.x, d.rev, W), None),
        "rolling_kurtosis": (lambda h: shape.rolling_kurtosis(h.x, W), lambda t, d: t.kurtosis(d.x, W), T.KurtosisTransform(W, "x")),
        "trend_slope": (lambda h: shape.trend_slope(h.x, W), lambda t, d: t.trend_slope(d.x, W), T.TrendSlope(W, "x")),
        "hurst_exponent": (lambda h: shape.hurst_exponent(h.x, W), lambda t, d: t.hurst_exponent(d.x, W), T.HurstExponent(W, "x")),
        "bipower_variation": (lambda h: shape.bipower_variation(h.x, W), lambda t, d: t.bipower_variation(d.x, W), T.BiPowerVariation(W, "x")),
        "approximate_entropy": (lambda h: entropy.approximate_entropy(h.x, W, 2, 0.2), lambda t, d: t.approximate_entropy(d.x, W, 2, 0.2),
                                T.ApproximateEntropy(W, 2, 0.2, "x")),
    }


@pytest.fixture(scope="module")
def columns():
    """n -> (host columns, trade set, resident columns, frame): the one series x and, for the features of two and three series,
    x * 1.01 and x * 0.99 as high and low and x reversed as the second series.  Never written to."""
    from finmlkit_amd import _ffi
    from finmlkit_amd.engine import DeviceTrades
    x = np.random.default_rng(2024).uniform(50.0, 150.0, N)
    x[NAN_AT] = np.nan
    made = {}
    for n in (N, 1):
        h = SimpleNamespace(x=x[:n].copy(), high=x[:n] * 1.01, low=x[:n] * 0.99, rev=x[:n][::-1].copy())
        for a in vars(h).values():
            a.setflags(write=False)
        ctx = _ffi.default_context()
        t = DeviceTrades.from_numpy(np.arange(n, dtype=np.int64), h.x, np.ones(n, np.float32), ctx=ctx)
        d = SimpleNamespace(**{k: _ffi.DeviceArray.from_host(ctx, a) for k, a in vars(h).items()})
        frame = pd.DataFrame({"x": h.x}, index=pd.to_datetime(np.arange(n, dtype=np.int64) * 1_000_000_000))
        made[n] = (h, t, d, frame)
    return made


def test_every_row_has_its_routes():
    assert list(routes()) == list(OPS)


@pytest.mark.parametrize("n", [N, 1])
@pytest.mark.parametrize("name", list(OPS))
def test_host_resident_and_compose_give_the_same_bits(columns, name, n):
    from finmlkit_amd.feature.transforms import Compose, SISOTransform
    h, t, d, frame = columns[n]
    drop_in, method, transform = routes()[name]
    want = drop_in(h)
    assert want.shape == (n,) and want.dtype == OPS[name].out
    got = method(t, d).to_host()
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), name
    if n == N:
        assert np.isfinite(want).any(), name                                   # an output of NaN alone would compare nothing
    if transform is not None:
        assert isinstance(transform, SISOTransform) and type(transform)._dev is not SISOTransform._dev
        series = Compose(transform)(frame)
        assert series.name == transform.output_name and series.index.equals(frame.index)
        assert series.values.dtype == want.dtype and np.array_equal(series.values, want, equal_nan=True), name
        assert np.array_equal(transform(frame).values, want, equal_nan=True), name
