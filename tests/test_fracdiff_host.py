"""CPU-only: the weights of the fractional differentiation, what `frac_diff_weights` and `fir` refuse (in Python and, with a null
context and null pointers, in the library), the calls that need no device, and the oracle of tests/_fracdiff_ref.py checked against
its own definition."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from finmlkit_amd import _ffi
from finmlkit_amd.feature import transforms as T
from finmlkit_amd.feature.core import fracdiff as P
from tests import _fracdiff_ref as F

NAN, INF = math.nan, math.inf
WIDTHS = {0.4: (11, 55, 282, 1458), 0.5: (10, 44, 200, 927), 0.1: (8, 62, 503, 4076)}      # at thresholds 1e-2 .. 1e-5
THRESHOLDS = (1e-2, 1e-3, 1e-4, 1e-5)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------- the oracle against its definition
def test_libm_fma_is_the_correctly_rounded_one():
    triples = F.fma_triples(5001)
    assert len(triples) >= 10_000
    got = np.array([F.fma_libm(*t) for t in triples])
    want = np.array([F.fma_fraction(*t) for t in triples])
    assert np.array_equal(bits(got), bits(want))
    tiny = np.abs(want) < 2.0 ** -1022
    assert int((tiny & (want != 0.0)).sum()) >= 1000, "subnormal results"
    ties = [t for t in triples[-2500:] if (Fraction(t[0]) * Fraction(t[1]) + Fraction(t[2])).denominator == 1 << 53]
    assert len(ties) == 2500, "1 + an odd multiple of 2^-53 lies halfway between two float64"
    fused = sum(1 for a, b, c in triples[2500:5000] if F.fma_libm(a, b, c) != a * b + c)
    assert fused >= 2000, "the cancelling triples tell a fused multiply-add from a rounded product"


def test_fir_ref_is_a_difference_and_the_two_forms_agree():
    x = F.log_price_walk(300, 11)
    y = F.fir_ref(x, [1.0, -1.0])
    assert math.isnan(y[0]) and np.array_equal(bits(y[1:]), bits(x[1:] - x[:-1]))
    line = 7.0 + 3.0 * np.arange(200.0)
    y = F.fir_ref(line, [1.0, -2.0, 1.0])
    assert np.isnan(y[:2]).all() and np.array_equal(bits(y[2:]), bits(np.zeros(198)))                 # exactly +0.0
    x = F.mantissa_returns(120, 12)
    x[[5, 40, 41, 90]] = [NAN, INF, -INF, NAN]
    w = F.random_weights(7, 13)
    a, b = F.fir_ref(x, w), F.fir_ref(x, w, fma=F.fma_fraction)
    assert F.bits_equal(a, b)
    want_nan = np.zeros(120, bool)
    want_nan[:6] = True
    for i in (5, 40, 41, 90):
        want_nan[i:i + 7] = True
    assert np.array_equal(np.isnan(a), want_nan)
    assert F.fir_ref(x[:6], w).shape == (6,) and np.isnan(F.fir_ref(x[:6], w)).all()                  # n < W


# ---------------------------------------------------------------------------------------------- weights
def test_integer_orders_are_the_binomial_rows():
    for d, want in ((0, [1.0]), (1, [1.0, -1.0]), (2, [1.0, -2.0, 1.0]), (3, [1.0, -3.0, 3.0, -1.0])):
        for w in (P.frac_diff_weights(d), np.array(F.weights_ref(float(d)))):
            assert w.dtype == np.float64 and np.array_equal(bits(w), bits(want)), d


@pytest.mark.parametrize("d", sorted(WIDTHS))
def test_widths_at_the_usual_thresholds(d):
    assert tuple(len(P.frac_diff_weights(d, thr)) for thr in THRESHOLDS) == WIDTHS[d]
    assert tuple(len(F.weights_ref(d, thr)) for thr in THRESHOLDS) == WIDTHS[d]
    assert len(P.frac_diff_weights(d)) == WIDTHS[d][3]                                             # the default threshold is 1e-5


def test_product_weights_are_the_restatement_bit_for_bit():
    for d in np.random.default_rng(77).uniform(0.0, 2.0, 50):
        for thr in (1e-3, 1e-5):
            w = P.frac_diff_weights(d, thr)
            assert np.array_equal(bits(w), bits(F.weights_ref(float(d), thr))), (d, thr)
            assert w[0] == 1.0 and np.abs(w).min() >= thr


def test_no_order_up_to_two_needs_more_than_4093_weights():
    widths = [len(P.frac_diff_weights(i / 100.0, 1e-5)) for i in range(201)]
    assert max(widths) == 4093 and min(widths) == 1


# ---------------------------------------------------------------------------------------------- refusals
REFUSED_WEIGHTS = [((NAN, 1e-5), P.D_MESSAGE), ((INF, 1e-5), P.D_MESSAGE), ((-INF, 1e-5), P.D_MESSAGE), ((-0.3, 1e-4), P.D_MESSAGE),
                   ((-1e-300, 1e-5), P.D_MESSAGE),
                   ((0.4, 0.0), P.THRESHOLD_MESSAGE), ((0.4, 1.0), P.THRESHOLD_MESSAGE), ((0.4, -1e-5), P.THRESHOLD_MESSAGE),
                   ((0.4, NAN), P.THRESHOLD_MESSAGE), ((0.4, INF), P.THRESHOLD_MESSAGE),
                   ((0.1, 1e-6), P.WIDTH_MESSAGE), ((0.2, 1e-7), P.WIDTH_MESSAGE),
                   # two checks fail: the earlier message
                   ((NAN, NAN), P.D_MESSAGE), ((-1.0, 2.0), P.D_MESSAGE), ((-0.1, 1e-6), P.D_MESSAGE)]


@pytest.mark.parametrize("args,message", REFUSED_WEIGHTS)
def test_what_frac_diff_weights_refuses(args, message):
    with pytest.raises(ValueError) as e:
        P.frac_diff_weights(*args)
    assert str(e.value) == message
    with pytest.raises(ValueError) as e:
        T.FracDiff(*args)
    assert str(e.value) == message


def test_the_messages_are_the_issues_texts():
    assert P.FIR_MAX_WIDTH == 8192
    assert P.D_MESSAGE == "frac_diff: d must be finite and not negative."
    assert P.THRESHOLD_MESSAGE == "frac_diff: threshold must be greater than 0 and less than 1."
    assert P.WIDTH_MESSAGE == "frac_diff: more than 8192 weights reach the threshold; raise the threshold."
    assert P.FIR_EMPTY_MESSAGE == "fir: at least one weight is needed."
    assert P.FIR_MAX_WIDTH_MESSAGE == "fir: at most 8192 weights."
    assert P.FIR_FINITE_MESSAGE == "fir: the weights must be finite."
    assert P.FIR_ALIAS_MESSAGE == "fir: the output must not be the input."


def test_a_threshold_just_within_the_limit_is_served():
    """8192 weights are allowed: the refusal is for the 8193rd."""
    thr = abs(F.weights_ref(0.1, 1e-7, limit=8194)[8192])                # |w[8192]| itself: strictly below is what ends the list
    with pytest.raises(ValueError) as e:
        P.frac_diff_weights(0.1, thr)
    assert str(e.value) == P.WIDTH_MESSAGE
    w = P.frac_diff_weights(0.1, math.nextafter(thr, 1.0))
    assert len(w) == 8192 == P.FIR_MAX_WIDTH


REFUSED_FIR = [(np.empty(0), P.FIR_EMPTY_MESSAGE), (np.ones(8193), P.FIR_MAX_WIDTH_MESSAGE),
               (np.array([1.0, NAN]), P.FIR_FINITE_MESSAGE), (np.array([INF]), P.FIR_FINITE_MESSAGE),
               (np.array([1.0, -INF, 2.0]), P.FIR_FINITE_MESSAGE),
               (np.full(8193, NAN), P.FIR_MAX_WIDTH_MESSAGE)]                  # two checks fail: the earlier message


@pytest.mark.parametrize("case", range(len(REFUSED_FIR)))
def test_what_fir_refuses_in_python(case, monkeypatch):
    weights, message = REFUSED_FIR[case]

    def no_context():
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(_ffi, "default_context", no_context)
    f32 = SimpleNamespace(dtype=np.dtype(np.float32), n=10)
    for call in (lambda: P.fir(np.zeros(10), weights), lambda: P.fir(np.empty(0), weights), lambda: P.resident(None, f32, weights)):
        with pytest.raises(ValueError) as e:                                  # the rule before the dtype, before the empty answer
            call()
        assert str(e.value) == message


def test_the_library_refuses_a_bad_width_before_it_looks_at_anything():
    for fn in P.entries():
        for width in (0, -1, 8193, 1 << 40):
            assert fn(None, None, 10, None, width, None) == _ffi.E_ARG, (fn.__name__, width)
    assert _ffi.lib().fmk_last_error(None).decode() == P.FIR_MAX_WIDTH_MESSAGE
    assert P.entries()[0](None, None, 10, None, 0, None) == _ffi.E_ARG
    assert _ffi.lib().fmk_last_error(None).decode() == P.FIR_EMPTY_MESSAGE
    # the weights are a host array in both flavours: both can refuse them, and an output that is the input, without a device
    w = np.array([1.0, NAN, 2.0])
    x = np.zeros(10)
    for fn in P.entries():
        assert fn(None, _ffi.ptr(x), 10, _ffi.ptr(w), 3, _ffi.ptr(np.zeros(10))) == _ffi.E_ARG
        assert _ffi.lib().fmk_last_error(None).decode() == P.FIR_FINITE_MESSAGE
        assert fn(None, _ffi.ptr(x), 10, _ffi.ptr(np.ones(3)), 3, _ffi.ptr(x)) == _ffi.E_ARG
        assert _ffi.lib().fmk_last_error(None).decode() == P.FIR_ALIAS_MESSAGE
        assert fn(None, _ffi.ptr(x), 1 << 31, _ffi.ptr(np.ones(3)), 3, _ffi.ptr(np.zeros(10))) == _ffi.E_ARG
        assert fn(None, _ffi.ptr(x), 0, _ffi.ptr(np.ones(3)), 3, _ffi.ptr(np.zeros(1))) == _ffi.OK    # n == 0 touches nothing


def test_the_geometry_needs_no_device():
    tile, taps = P.geometry()
    assert tile >= 64 and taps >= 8 and tile % 64 == 0


# ---------------------------------------------------------------------------------------------- no device needed
def test_an_empty_series_needs_no_context(monkeypatch):
    def no_context():
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(_ffi, "default_context", no_context)
    w = P.frac_diff_weights(0.4, 1e-3)
    for out in (P.fir(np.empty(0), w), P.frac_diff_ffd(np.empty(0), 0.4, 1e-3), P.frac_diff_ffd([], 1)):
        assert out.shape == (0,) and out.dtype == np.float64
    out = P.resident(None, SimpleNamespace(dtype=np.dtype(np.float64), n=0), w)
    assert out.n == 0 and out.dtype == np.float64 and out.ptr == 0
    with pytest.raises(TypeError) as e:
        P.resident(None, SimpleNamespace(dtype=np.dtype(np.float32), n=10), w)
    assert str(e.value) == "fmk_fir_dev: the series must be float64, not float32"


def test_the_transform_is_built_without_a_device():
    t = T.FracDiff(0.4)
    assert (t.requires, t.produces, t.output_name) == (["close"], ["ffd0.4"], "close_ffd0.4")
    assert (t.d, t.threshold) == (0.4, 1e-5) and len(t.weights) == 1458
    t = T.FracDiff(0.5, 1e-3, input_col="price")
    assert (t.requires, t.produces, t.output_name) == (["price"], ["ffd0.5"], "price_ffd0.5")
    assert np.array_equal(bits(t.weights), bits(F.weights_ref(0.5, 1e-3))) and len(t.weights) == 44
    assert isinstance(t, T.SISOTransform) and type(t)._dev is not T.SISOTransform._dev               # Compose keeps it on the device
    c = T.Compose(T.FracDiff(0.4, 1e-3, input_col="price"), T.SMA(24))
    assert c.output_name == "price_ffd0.4_sma24"
    from finmlkit_amd.feature import core
    assert core.fir is P.fir and core.frac_diff_ffd is P.frac_diff_ffd and core.frac_diff_weights is P.frac_diff_weights
