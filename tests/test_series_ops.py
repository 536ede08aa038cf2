"""CPU-only: the table of series features (finmlkit_amd/feature/series_ops.py) against the header and the library.  Every row's
prototype is the one include/fmk.h declares, type for type, and no series feature of the header lacks a row; what a row's rule
refuses, both C flavours refuse too (FMK_E_ARG from a null context and null pointers: nothing is dereferenced first); and both
drivers check in the documented order and answer an empty series without a context."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from finmlkit_amd import _ffi
from finmlkit_amd.feature import series_ops as S
from finmlkit_amd.feature.series_ops import OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPE = {C.c_int64: "int64_t", C.c_double: "double", C.c_int: "int"}
OUT_TYPE = {np.float64: "double *", np.float32: "float *"}
NAN, INF = math.nan, math.inf

# scalars every row accepts, in ABI order
VALID = {"sma": (24,), "zscore": (24, 0), "rolling_variance": (24, 1, 1), "variance_ratio_1_4": (24, 0, True), "burst_ratio": (24,),
         "roc": (24,), "pct_change": (24,), "stoch_k": (24,), "ewma": (10.0,), "rsi_wilder": (24,), "true_range": (),
         "atr": (24, False, False), "adx": (24,), "bollinger_percent_b": (24, 2.0), "vwap_distance": (24, False),
         "flow_acceleration": (24, 6), "vpin": (24,), "parkinson_range": (), "price_volume_corr": (24,), "rolling_kurtosis": (24,),
         "trend_slope": (24,), "hurst_exponent": (24,), "bipower_variation": (24,), "approximate_entropy": (24, 2, 0.2)}

# refused scalars per row with the message of the first check that fires: every message of a row at least once, and where a row
# has more than one check, a tuple that fails several of them (the earlier check's message wins)
REFUSED = {
    "sma": [((0,), S.WINDOW_MESSAGE)],
    "zscore": [((0, 0), S.WINDOW_MESSAGE), ((0, 5), S.WINDOW_MESSAGE), ((5, 5), S.ZSCORE_MESSAGE), ((3, 7), S.ZSCORE_MESSAGE)],
    "rolling_variance": [((0, 1, 1), S.WINDOW_MESSAGE)],
    "variance_ratio_1_4": [((0, 0, True), S.WINDOW_MESSAGE)],
    "burst_ratio": [((0,), S.WINDOW_MESSAGE)],
    "roc": [((-1,), S.ROC_PERIOD_MESSAGE)],
    "pct_change": [((-1,), S.PCT_PERIODS_MESSAGE)],
    "stoch_k": [((0,), S.STOCH_LENGTH_MESSAGE)],
    "ewma": [((0.5,), S.SPAN_MESSAGE), ((NAN,), S.SPAN_MESSAGE)],
    "rsi_wilder": [((0,), S.RSI_WINDOW_MESSAGE)],
    "true_range": [],
    "atr": [((-1, False, False), S.ATR_WINDOW_MESSAGE)],
    "adx": [((0,), S.ADX_LENGTH_MESSAGE)],
    "bollinger_percent_b": [((0, 2.0), S.BOLLINGER_WINDOW_MESSAGE)],
    "vwap_distance": [((0, False), S.VWAP_PERIODS_MESSAGE)],
    "flow_acceleration": [((5, -1), S.RECENT_MESSAGE)],
    "vpin": [((-1,), S.VPIN_WINDOW_MESSAGE)],
    "parkinson_range": [],
    "price_volume_corr": [((0,), S.WINDOW_MESSAGE)],
    "rolling_kurtosis": [((0,), S.WINDOW_MESSAGE)],
    "trend_slope": [((0,), S.WINDOW_MESSAGE)],
    "hurst_exponent": [((0,), S.WINDOW_MESSAGE), ((8,), S.HURST_WINDOW_MESSAGE)],
    "bipower_variation": [((0,), S.WINDOW_MESSAGE)],
    "approximate_entropy": [((24, 0, 0.2), S.APEN_M_MESSAGE), ((2, 0, -1.0), S.APEN_M_MESSAGE), ((24, 5, 0.2), S.APEN_MAX_M_MESSAGE),
                            ((2, 5, 0.2), S.APEN_MAX_M_MESSAGE), ((2, 2, 0.2), S.APEN_WINDOW_MESSAGE),
                            ((2, 2, -1.0), S.APEN_WINDOW_MESSAGE), ((1025, 2, 0.2), S.APEN_MAX_WINDOW_MESSAGE),
                            ((1025, 2, NAN), S.APEN_MAX_WINDOW_MESSAGE), ((24, 2, -0.1), S.APEN_TOLERANCE_MESSAGE),
                            ((24, 2, NAN), S.APEN_TOLERANCE_MESSAGE), ((24, 2, INF), S.APEN_TOLERANCE_MESSAGE)],
}


def header_prototypes():
    """{entry: [parameter types]} of the header's series sections (from the rolling-window moments up to the labels)."""
    text = open(os.path.join(ROOT, "include", "fmk.h")).read()
    first, last = text.index("/* ---- rolling-window moments"), text.index("/* ---- labels and sample weights")
    assert 0 < first < last
    code = re.sub(r"/\*.*?\*/", "", text[first:last], flags=re.S)
    found = {}
    for name, params in re.findall(r"\bint\s+(fmk_\w+)\s*\(([^)]*)\)\s*;", code):
        # a parameter is its type and then its name: "const double *d_x" -> "const double *"
        found[name] = [re.sub(r"\s+", " ", re.fullmatch(r"\s*(.*?)\w+\s*", p, flags=re.S).group(1)).strip() for p in params.split(",")]
    return found


def is_series_feature(types):
    """context, 1..3 float64 series, n, 0..3 scalars, one output pointer"""
    text = " , ".join(types)
    return re.fullmatch(r"fmk_ctx \*( , const double \*){1,3} , int64_t( , (int64_t|double|int)){0,3} , (double|float) \*", text) is not None


def test_the_table_has_the_24_rows_and_one_entry_each():
    assert list(OPS) == list(VALID) == list(REFUSED) and len(OPS) == 24
    assert len({op.entry for op in OPS.values()}) == 24
    for name, op in OPS.items():
        assert op.entry == "fmk_" + name and op.inputs in (1, 2, 3) and len(op.params) <= 3 and set(op.params) <= set(C_TYPE), name
        assert (op.unequal != "") == (op.inputs > 1), name
        assert op.out is (np.float32 if name == "vpin" else np.float64), name
    corr = OPS["price_volume_corr"]
    assert corr.unequal_resident and corr.unequal_resident != corr.unequal
    assert all(not op.unequal_resident for name, op in OPS.items() if name != "price_volume_corr")


def test_every_row_is_the_headers_prototype_and_every_series_feature_has_a_row():
    header = header_prototypes()
    for name, op in OPS.items():
        want = ["fmk_ctx *"] + ["const double *"] * op.inputs + ["int64_t"] + [C_TYPE[t] for t in op.params] + [OUT_TYPE[op.out]]
        assert header.get(op.entry) == want, (name, header.get(op.entry), want)
        assert header.get(op.entry + "_dev") == want, (name, header.get(op.entry + "_dev"), want)
        assert len(S.prototype(op)) == len(want)
    declared = {n for n, types in header.items() if is_series_feature(types)}
    assert declared == {e for op in OPS.values() for e in (op.entry, op.entry + "_dev")}, "a series feature of the header has no row"
    # the drivers' prototypes are on the loaded library
    lib = _ffi.lib()
    for op in OPS.values():
        for fn, name in zip(S.entries(op), (op.entry, op.entry + "_dev")):
            assert fn is getattr(lib, name) and fn.restype is C.c_int and list(fn.argtypes) == S.prototype(op)


def test_a_forgotten_row_shows():
    header = header_prototypes()
    declared = {n for n, types in header.items() if is_series_feature(types)}
    assert len(declared) == 48 and "fmk_sma_dev" in declared and "fmk_vpin" in declared
    assert not is_series_feature(["fmk_ctx *", "const double *", "int64_t", "double *", "double *"])       # two outputs
    assert not is_series_feature(["fmk_ctx *", "const int64_t *", "const double *", "int64_t", "double", "double *"])   # timestamps


@pytest.mark.parametrize("name", list(OPS))
def test_what_the_rule_refuses_the_library_refuses(name):
    op = OPS[name]
    op.rule(*VALID[name])
    host_entry, dev_entry = S.entries(op)
    for params, message in REFUSED[name]:
        with pytest.raises(ValueError) as e:
            op.rule(*params)
        assert str(e.value) == message, (name, params)
        # only now C: a null context, null pointers, n = 10 -- the status comes before anything is dereferenced
        for fn in (host_entry, dev_entry):
            assert fn(None, *[None] * op.inputs, 10, *params, None) == _ffi.E_ARG, (name, params, fn.__name__)


@pytest.mark.parametrize("name", list(OPS))
def test_the_drivers_check_in_order_and_need_no_context_for_an_empty_series(name, monkeypatch):
    op = OPS[name]

    def no_context():
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(_ffi, "default_context", no_context)
    out = S.host(op, [np.empty(0)] * op.inputs, *VALID[name])
    assert out.shape == (0,) and out.dtype == op.out
    f64 = lambda n: SimpleNamespace(dtype=np.dtype(np.float64), n=n)          # noqa: E731 -- a stand-in: no pointer, no context
    f32 = lambda n: SimpleNamespace(dtype=np.dtype(np.float32), n=n)          # noqa: E731
    out = S.resident(None, op, [f64(0)] * op.inputs, *VALID[name])
    assert out.n == 0 and out.dtype == op.out and out.ptr == 0
    # the rule's error before the dtype error, the dtype error before the length error
    wrong = [f32(10)] + [f64(9)] * (op.inputs - 1)
    for params, message in REFUSED[name]:
        with pytest.raises(ValueError) as e:
            S.resident(None, op, wrong, *params)
        assert str(e.value) == message
        with pytest.raises(ValueError) as e:
            S.host(op, [np.zeros(10)] + [np.zeros(9)] * (op.inputs - 1), *params)
        assert str(e.value) == message
    with pytest.raises(TypeError) as e:
        S.resident(None, op, wrong, *VALID[name])
    assert str(e.value) == f"{op.entry}_dev: the series must be float64, not float32"
    if op.inputs > 1:
        with pytest.raises(ValueError) as e:
            S.resident(None, op, [f64(10)] + [f64(9)] * (op.inputs - 1), *VALID[name])
        assert str(e.value) == (op.unequal_resident or op.unequal)
        for arrays in ([np.zeros(10)] + [np.zeros(9)] * (op.inputs - 1), [np.zeros((2, 5))] * op.inputs):
            with pytest.raises(ValueError) as e:
                S.host(op, arrays, *VALID[name])
            assert str(e.value) == op.unequal
