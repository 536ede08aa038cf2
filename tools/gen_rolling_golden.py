#!/usr/bin/env python3
"""Writes tests/golden/rolling_stats.npz + rolling_stats.json: outputs of the REFERENCE's rolling-window moments -- sma
(feature/core/ma.py), comp_zscore (feature/core/utils.py), rolling_variance_nb and variance_ratio_1_4_core
(feature/core/volatility.py) -- on seeded walks that the tests regenerate (tests/_rolling_ref.py: grid_walk, integer arithmetic) and
their log returns, on a held walk with long equal runs, on series with NaN runs, +inf, zero and negative prices, on the edge
lengths, on the calls of the reference's own tests, and the refused arguments.  Build container only: imports the reference in
pure-Python mode through oracle/shim, like tools/gen_break_golden.py; no GPU, nothing of the product.

The reference's functions are Numba kernels.  Compiled, their np.sum / np.mean are plain left-to-right loops and their np.log is
the host's log(); interpreted, NumPy sums pairwise from 8 elements up and has a log of its own.  The recorded outputs are the
reference's code with `sum`, `mean` and `log` as it has them when compiled (substituted in the reference modules' `np`, as the
break generator substitutes `log`).  A case is refused unless the reference so run and both forms of tests/_rolling_ref.py agree
exactly, NaN positions included; a case with window < 8 also unless the UNMODIFIED reference agrees exactly.  For larger windows the
number of elements the unmodified reference rounds differently is recorded ("np_pairwise_differs": information, not a gate).
The log-return ratio is the exception: the untouched reference calls NumPy's own log, which rounds some arguments differently from
the host's, so its gate substitutes the host's log and nothing else, and the elements NumPy's log changes are counted
("np_log_differs").
    python tools/gen_rolling_golden.py [reference checkout]
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402

import finmlkit.feature.core.ma as RMA  # noqa: E402
import finmlkit.feature.core.utils as RUT  # noqa: E402
import finmlkit.feature.core.volatility as RVO  # noqa: E402

from tests import _rolling_ref as H  # noqa: E402

MODULES = (RMA, RUT, RVO)


class CompiledNumpy:
    """numpy with `sum`, `mean` and `log` as Numba compiles them: a left-to-right loop from 0.0, that sum over the size, libm."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def sum(a, dtype=None):
        c = 0.0
        for v in np.asarray(a, np.float64).tolist():
            c = c + v
        return np.float64(c)

    @staticmethod
    def mean(a):
        return CompiledNumpy.sum(a) / np.asarray(a).size

    @staticmethod
    def log(a):
        return H.host_log(a) if isinstance(a, np.ndarray) else np.float64(H._log1(float(a)))


class HostLogNumpy(CompiledNumpy):
    """numpy with `log` from libm alone: NumPy's own sum and mean."""
    sum = staticmethod(np.sum)
    mean = staticmethod(np.mean)


class compiled_order_in_reference:
    def __init__(self, numpy=CompiledNumpy):
        self.numpy = numpy

    def __enter__(self):
        for m in MODULES:
            m.np = self.numpy()

    def __exit__(self, *a):
        for m in MODULES:
            m.np = np


class Reference:
    """The reference's four functions under the names tests/_rolling_ref.call expects."""
    sma = staticmethod(lambda x, w: RMA.sma(x, w))
    comp_zscore = staticmethod(lambda x, w, d: RUT.comp_zscore(x, w, d))
    rolling_variance_nb = staticmethod(lambda x, w, d, mp: RVO.rolling_variance_nb(x, w, d, mp))
    variance_ratio_1_4_core = staticmethod(lambda x, w, d, rt: RVO.variance_ratio_1_4_core(x, w, d, rt))


def case(fn, x, window, ddof=None, min_periods=None, ret_type=None, **source):
    """`source`: how the tests regenerate x ({"walk": [n, seed, step, hold], "returns": bool}); without it x is stored."""
    return dict(fn=fn, x=np.asarray(x, np.float64), window=window, ddof=ddof, min_periods=min_periods, ret_type=ret_type,
                source=source or None)


def four(prefix, x, window, source, out, ddofs=(0, 1), ratio=True):
    """sma, z-score, variance (default arguments) and, on prices, the ratio in both return types."""
    out[f"{prefix}.sma"] = case("sma", x, window, **source)
    for d in ddofs:
        if window - d > 0:
            out[f"{prefix}.zscore_ddof{d}"] = case("zscore", x, window, ddof=d, **source)
    out[f"{prefix}.variance"] = case("variance", x, window, ddof=1, min_periods=1, **source)
    if ratio:
        for rt in ("log", "simple"):
            out[f"{prefix}.ratio_{rt}"] = case("ratio", x, window, ddof=0, ret_type=rt, **source)


def walk_cases():
    out = {}
    for k, window in enumerate((1, 2, 7, 8, 50, 200, 1000)):
        spec = [1500, 400 + k, 35, 0.0]
        four(f"walk.w{window}", H.grid_walk(*spec), window, {"walk": spec}, out, ddofs=(0,) if window != 50 else (0, 1))
        r = H.walk_returns(*spec)
        src = {"walk": spec, "returns": True}
        out[f"returns.w{window}.sma"] = case("sma", r, window, **src)
        out[f"returns.w{window}.zscore"] = case("zscore", r, window, ddof=1 if window > 1 else 0, **src)
        out[f"returns.w{window}.variance"] = case("variance", r, window, ddof=0, min_periods=1, **src)
    # long equal runs: windows whose std is exactly 0, variances clamped to 0, a zero 4-step variance
    for window, hold in ((5, 0.9), (50, 0.985)):
        spec = [700, 420 + window, 1, hold]
        four(f"held.w{window}", H.grid_walk(*spec), window, {"walk": spec}, out)
    return out


def odd_cases():
    """NaN runs shorter and longer than the window, +inf, zero and negative prices: what IEEE arithmetic makes of the code."""
    out = {}
    window = 20
    x = H.grid_walk(600, 431)
    x[50:53] = np.nan                      # shorter than the window
    x[150:190] = np.nan                    # longer
    x[300] = np.inf
    x[400], x[450], x[451] = 0.0, -3.0, -0.0
    four("odd.prices", x, window, {}, out)
    for d in (0, 1):
        for mp in (1, window, window + 1):
            out[f"odd.variance_ddof{d}_mp{mp}"] = case("variance", x, window, ddof=d, min_periods=mp)
        for rt in ("log", "simple"):
            out[f"odd.ratio_{rt}_ddof{d}"] = case("ratio", x, window, ddof=d, ret_type=rt)
    r = H.walk_returns(600, 432)
    r[[10, 11, 300]] = [np.nan, np.nan, -np.inf]
    r[100:140] = np.nan
    four("odd.returns", r, window, {}, out, ratio=False)
    return out


def length_cases():
    out = {}
    window = 10
    for n in (0, window - 1, window, window + 3, window + 4, window + 5):
        x = H.grid_walk(max(n, 1), 440 + n)[:n]
        four(f"length.n{n}", x, window, {}, out, ddofs=(0,))
    return out


def reference_test_calls():
    """The calls of tests/features/test_variance_ratio.py and test_core_utils.py, inputs as those files build them (the transform
    test's frame columns go through variance_ratio_1_4_core)."""
    out = {}
    series = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0])
    with_nans = np.array([1.0, np.nan, 3.0, 4.0, np.nan, 6.0, 7.0, 8.0, np.nan, 10.0])
    out["refcall.variance"] = case("variance", series, 3, ddof=1, min_periods=1)
    out["refcall.variance_nans"] = case("variance", with_nans, 3, ddof=1, min_periods=1)
    out["refcall.variance_ddof0"] = case("variance", series, 3, ddof=0, min_periods=1)
    out["refcall.variance_min2"] = case("variance", with_nans, 3, ddof=1, min_periods=2)
    np.random.seed(42)
    n = 100
    price = np.insert(np.cumprod(1 + np.random.normal(0, 0.01, n)), 0, 1.0)
    out["refcall.ratio_simple"] = case("ratio", price, 20, ddof=0, ret_type="simple")
    out["refcall.ratio_log"] = case("ratio", price, 20, ddof=0, ret_type="log")
    nans = price.copy()
    nans[30:35] = np.nan
    out["refcall.ratio_nans"] = case("ratio", nans, 20, ddof=0, ret_type="simple")
    zeros = price.copy()
    zeros[40:45] = 0.0
    out["refcall.ratio_zeros"] = case("ratio", zeros, 20, ddof=0, ret_type="simple")
    trend = 100.0 + np.linspace(0, 1, n + 1) * 10.0 + np.random.normal(0, 0.5, n + 1)
    out["refcall.ratio_trend"] = case("ratio", trend, 20, ddof=0, ret_type="simple")
    rev = np.zeros(n + 1)
    rev[0] = 100.0
    for i in range(1, n + 1):
        rev[i] = rev[i - 1] + (100 - rev[i - 1]) * 0.7 + np.random.normal(0, 0.5, 1)[0]
    out["refcall.ratio_mean_reverting"] = case("ratio", rev, 20, ddof=0, ret_type="simple")
    np.random.seed(42)
    price = np.insert(np.cumprod(1 + np.random.normal(0, 0.01, n)), 0, 1.0)
    out["refcall.transform_close"] = case("ratio", price, 20, ddof=0, ret_type="log")
    out["refcall.transform_high"] = case("ratio", price * 1.01, 20, ddof=0, ret_type="log")
    out["refcall.zscore"] = case("zscore", np.array([1.0, 2.0, 3.0, 4.0, 5.0]), 3, ddof=0)
    return out


def refused_calls():
    """Arguments this project refuses with ValueError; what the interpreted reference does with them is recorded beside."""
    x = H.grid_walk(40, 450)
    out = {}
    for fn, kw in (("sma", {}), ("zscore", {"ddof": 0}), ("variance", {"ddof": 1, "min_periods": 1}),
                   ("ratio", {"ddof": 0, "ret_type": "log"})):
        for window in (0, -2):
            out[f"refused.{fn}_w{window}"] = case(fn, x, window, **kw)
    out["refused.zscore_w5_ddof5"] = case("zscore", x, 5, ddof=5)
    out["refused.zscore_w5_ddof7"] = case("zscore", x, 5, ddof=7)
    return out


def run(mod, c, **kw):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            r = H.call(c["fn"], c["x"].copy(), c["window"], c["ddof"], c["min_periods"], c["ret_type"], mod=mod, **kw)
        return ("ok", np.asarray(r, np.float64))
    except Exception as e:                                        # noqa: BLE001 -- recorded as data
        return ("raises", type(e).__name__, str(e))


def differs(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum()) if a.shape == b.shape else -1


def main():
    out, manifest = {}, {}
    cases = {}
    for group in (walk_cases, odd_cases, length_cases, reference_test_calls, refused_calls):
        cases.update(group())
    for name, c in cases.items():
        entry = {k: c[k] for k in ("fn", "window", "ddof", "min_periods", "ret_type") if c[k] is not None}
        entry["n"] = int(len(c["x"]))
        if c["source"]:
            entry["source"] = c["source"]
            spec = c["source"]["walk"]
            entry["walk_sha256"] = H.sha256(H.grid_walk(*spec))
        else:
            out[name + ".x"] = c["x"]
        own = [run(None, c, form=form) for form in ("scalar", "vector")]
        plain = run(Reference, c)
        if name.startswith("refused."):
            if not all(o[0] == "raises" and o[1] == "ValueError" and o[1:] == own[0][1:] for o in own):
                raise SystemExit(f"{name}: the helper does not refuse this call")
            entry.update(raises=own[0][1], message=own[0][2],
                         reference=f"raises {plain[1]}" if plain[0] == "raises" else
                         f"returns ({int(np.isnan(plain[1]).sum())} NaN, {int(np.isinf(plain[1]).sum())} inf of {len(plain[1])})")
            manifest[name] = entry
            continue
        with compiled_order_in_reference():
            ref = run(Reference, c)
        if ref[0] != "ok":
            raise SystemExit(f"{name}: the reference raises {ref[1:]} -- case refused")
        for form, o in zip(("scalar", "vector"), own):
            if o[0] != "ok" or differs(ref[1], o[1]) != 0:
                raise SystemExit(f"{name}: reference and helper ({form}) disagree -- case refused")
        d = differs(ref[1], plain[1]) if plain[0] == "ok" else -1
        if c["ret_type"] == "log":
            # the one case where the untouched reference cannot agree at any window: interpreted, its np.log is NumPy's own
            # routine, not the host's (the contract, as in the break test).  The gate runs it with the host's log and nothing
            # else substituted (the ratio calls neither np.sum nor np.mean); what NumPy's log changes is recorded
            entry["np_log_differs"] = d
            with compiled_order_in_reference(HostLogNumpy):
                host = run(Reference, c)
            d = differs(ref[1], host[1]) if host[0] == "ok" else -1
        if c["window"] < 8 and d != 0:
            raise SystemExit(f"{name}: window < 8 and the unmodified reference differs in {d} elements -- case refused")
        out[name + ".out"] = ref[1]
        entry.update(finite=int(np.isfinite(ref[1]).sum()), zeros=int((ref[1] == 0).sum()), np_pairwise_differs=d)
        manifest[name] = entry
    for k in sorted(manifest):
        print(k, {a: b for a, b in manifest[k].items() if a != "walk_sha256"})
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "rolling_stats.npz"), **out)
    with open(os.path.join(gold, "rolling_stats.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    print(len(manifest), "cases,", os.path.getsize(os.path.join(gold, "rolling_stats.npz")), "bytes")


if __name__ == "__main__":
    main()
