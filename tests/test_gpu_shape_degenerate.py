"""rolling_kurtosis and hurst_exponent on the MI355X (csrc/fmk_shape.hip) where a window has no statistic or the statistic is badly
conditioned: every case of tests/golden/shape_degenerate.npz through the host-pointer entry and the `_dev` entry -- NaN on exactly the
head plus the windows of class `none`, the exact rational value elsewhere within the tolerance recorded per statistic and input family
(measured on the CPU against the exact value, never from a kernel), host and `_dev` equal in every bit -- and the resident chain on an
SMA of held prices, a constant non-dyadic series made on the device."""
import numpy as np
import pytest

from tests import _counts
from tests import _rolling_ref as R
from tests import _shape_ref as H
from tests import test_shape_host as S
from tests.test_gpu_shape import _resident, dev_call
from tests.test_shape_degenerate_host import CASES, MANIFEST, case_input, check, exact, tolerance

pytestmark = pytest.mark.gpu

WORST = {}                                                          # (statistic, family) -> the worst deviation from the exact value


@pytest.mark.parametrize("name", CASES)
def test_fixture_replay(name):
    c, x = MANIFEST[name], case_input(name)
    fn, w = c["fn"], c["window"]
    host, dev = S.product(fn)(x, w), dev_call(fn, x, w)
    assert host.tobytes() == dev.tobytes(), name
    worst = check(name, host, name + " (python)")
    check(name, dev, name + " (_dev)")
    if exact(name) is None:                                        # the long window: the class mask is exact, the values the restatement's
        worst = S.close(fn, host, H.call(fn, x, w), name + " against the restatement")
        print(name, "deviation from the restatement", worst)
    else:
        print(name, "deviation from the exact value", worst, "tolerance", tolerance(name))
    key = (fn, c["family"])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    _counts.record(f"shape_degenerate/max_deviation/{fn}/{c['family']}", value=repr(WORST[key]),
                   bound=repr(S.tolerance(fn) if exact(name) is None else tolerance(name)))
    _counts.record(f"shape_degenerate/fixture/{name}", outputs_compared=2 * c["n"], none=c["none"], value=c["value"])


@pytest.fixture(scope="module")
def held():
    """Held prices, and their SMA over 5 as the CPU restatement gives it (shared, never written to)."""
    x = H.held_series(2200, 1795, 100.0, 100)
    smooth = R.sma(x, 5)
    for a in (x, smooth):
        a.setflags(write=False)
    return x, smooth


CHAIN = (("kurtosis", "kurtosis", 12), ("hurst", "hurst_exponent", 24))


def _both_classes(want, w):
    body = want[w + 3:]                                             # the SMA has no value before index 4
    assert np.isnan(want[:w + 3]).all() and np.isnan(body).sum() >= 300 and np.isfinite(body).sum() >= 300


def test_resident_chain_on_an_sma_of_held_prices(held):
    x, smooth = held
    t, d_x = _resident(np.array(x))
    d_smooth = t.sma(d_x, 5)
    assert d_smooth.to_host().tobytes() == smooth.tobytes()          # the device's SMA of a held price is the held price's own constant
    for fn, method, w in CHAIN:
        want = H.call(fn, smooth, w)
        _both_classes(want, w)
        got = getattr(t, method)(d_smooth, w).to_host()
        dev = S.close(fn, got, want, f"resident chain {fn} on held prices")
        assert got.tobytes() == S.product(fn)(smooth, w).tobytes()
        _counts.record(f"shape_degenerate/resident/{fn}", outputs_compared=len(x), nan=int(np.isnan(want).sum()), value=repr(dev))


def test_compose_chain_on_an_sma_of_held_prices(held):
    import pandas as pd
    from finmlkit_amd.feature import transforms as T
    x, smooth = held
    frame = pd.DataFrame({"close": np.array(x)}, index=pd.date_range("2024-01-01", periods=len(x), freq="1s"))
    for fn, tr in (("kurtosis", T.KurtosisTransform(12, "sma5")), ("hurst", T.HurstExponent(24, "sma5"))):
        got = T.Compose(T.SMA(5, "close"), tr)(frame)
        want = H.call(fn, smooth, tr.window)
        _both_classes(want, tr.window)
        S.close(fn, got.values, want, f"Compose(SMA, {type(tr).__name__}) on held prices")
    _counts.record("shape_degenerate/compose", outputs_compared=2 * len(x))
