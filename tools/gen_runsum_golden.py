#!/usr/bin/env python3
"""Writes tests/golden/runsum.npz + runsum.json: outputs of the REFERENCE's running-sum indicators -- bollinger_percent_b and
parkinson_range (feature/core/volatility.py), vwap_distance (feature/core/reversion.py), comp_flow_acceleration and vpin
(feature/core/volume.py) -- on seeded series that the tests regenerate (tests/_runsum_ref.py: walks and volumes in integer
arithmetic), on series with NaN in and after the first window, with zero-volume runs, with zero-volume bars among volumes that are
not exactly summable, on the edge lengths, on vpin's window 0, and the refused arguments.  Build container only: imports the
reference in pure-Python mode through oracle/shim, like tools/gen_recur_golden.py; no GPU, nothing of the product.

The truth is the UNTOUCHED reference's code with two things as the compiled reference has them.  `log` in the reference modules'
`np` is the host's (tools/gen_rolling_golden.py does the same); NumPy's own log rounds some arguments differently, and the elements
it changes are counted per case ("np_log_differs").  And `x ** 2` is the product x * x, as Numba compiles a constant integer power:
interpreted, it is libm's pow(x, 2.0), which is not correctly rounded (it differs from the product on about 5 squares in 10 000).
The code is not edited for that: bollinger_percent_b is handed a series whose elements are floats with a `**` of their own (class F
below), and `log` returns such a float to parkinson_range; what pow changes is counted too ("py_pow_differs").  A case is refused
unless the reference and tests/_runsum_ref.py agree in every element, NaN positions and the sign of every zero included.  Cases
of more than 2100 elements record `output_sha256` (over the output's bytes, every NaN made the canonical quiet NaN) instead of the
output.
    python tools/gen_runsum_golden.py <reference checkout>
"""
import json
import operator
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_runsum_golden.py <reference checkout>   (or FINMLKIT_REFERENCE in the environment)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402

import finmlkit.feature.core.reversion as RRE  # noqa: E402
import finmlkit.feature.core.volatility as RVO  # noqa: E402
import finmlkit.feature.core.volume as RVL  # noqa: E402

from tests import _runsum_ref as H  # noqa: E402

MODULES = (RRE, RVO, RVL)


class F(float):
    """A float as the compiled reference has it: `** 2` is a product, a division by zero is IEEE's; every operation gives an F."""

    def __pow__(self, e):
        return F(float(self) * float(self)) if e == 2 else F(float(self) ** e)

    def __neg__(self):
        return F(-float(self))


def _binary(name, op):
    setattr(F, f"__{name}__", lambda a, b: F(op(float(a), float(b))))
    setattr(F, f"__r{name}__", lambda a, b: F(op(float(b), float(a))))


for _name, _op in (("add", operator.add), ("sub", operator.sub), ("mul", operator.mul), ("truediv", H._div)):
    _binary(_name, _op)


class Compiled:
    """A series whose elements are F."""

    def __init__(self, a):
        self.a, self.size = a, a.size

    def __len__(self):
        return self.size

    def __getitem__(self, i):
        return F(self.a[i])


class HostLogNumpy:
    """numpy with `log` from libm."""
    product_square = True

    def __getattr__(self, name):
        return getattr(np, name)

    def log(self, a):
        v = H._log(float(a))
        return F(v) if self.product_square else np.float64(v)


class HostLogPowNumpy(HostLogNumpy):
    product_square = False


class Reference:
    """The reference's five functions under the names tests/_runsum_ref.call expects."""
    bollinger_percent_b = staticmethod(RVO.bollinger_percent_b)
    parkinson_range = staticmethod(RVO.parkinson_range)
    vwap_distance = staticmethod(RRE.vwap_distance)
    comp_flow_acceleration = staticmethod(RVL.comp_flow_acceleration)
    vpin = staticmethod(RVL.vpin)


GENERATORS = H.GENERATORS
STORED_MAX = 2100                      # longer cases record the hash of their output, not the output
WINDOWS = (1, 2, 3, 20, 100)
N = 600
LONG = 6444


def case(fn, inputs, args, source=None):
    """`source`: how the tests regenerate the inputs, one [generator name, arguments] per input; without it they are stored."""
    return dict(fn=fn, inputs=tuple(np.asarray(a, np.float64) for a in inputs), args=list(args), source=source)


def seeded(fn, args, *gens):
    source = [[g, list(a)] for g, *a in gens]
    return case(fn, tuple(H.generate(source)), args, source)


def series_cases():
    out = {}
    for k, w in enumerate(WINDOWS):
        # (twice the length: a move of 0 cents has 1 chance in 71, and the flat windows of 2 must stay under 2 % of a case)
        out[f"walk.boll_cent_w{w}"] = seeded("boll", [w, 2.0], ("grid_walk", 2 * N, 800 + k))
        out[f"walk.boll_g64_w{w}"] = seeded("boll", [w, 2.0], ("grid64_walk", 2 * N, 805 + k))
        out[f"walk.boll_hlc_w{w}"] = seeded("boll", [w, 1.5], ("hlc_close", 2 * N, 810 + k))
        for lg in (False, True):
            tag = "log" if lg else "simple"
            out[f"walk.vwap_lot_{tag}_w{w}"] = seeded("vwap", [w, lg], ("grid_walk", N, 815 + k), ("lot_volumes", N, 820 + k))
            out[f"walk.vwap_exact_{tag}_w{w}"] = seeded("vwap", [w, lg], ("grid64_walk", N, 825 + k), ("int_volumes", N, 830 + k))
        for r in sorted({0, 5, w - 1}):
            if r < w:
                out[f"walk.flow_lot_w{w}_r{r}"] = seeded("flow", [w, r], ("lot_volumes", N, 835 + k))
                out[f"walk.flow_int_w{w}_r{r}"] = seeded("flow", [w, r], ("int_volumes", N, 840 + k))
        out[f"walk.vpin_lot_w{w}"] = seeded("vpin", [w], ("lot_volumes", N, 845 + k), ("lot_volumes", N, 850 + k))
        out[f"walk.vpin_int_w{w}"] = seeded("vpin", [w], ("int_volumes", N, 855 + k), ("int_volumes", N, 860 + k))
    out["walk.boll_std0_w20"] = seeded("boll", [20, 0.0], ("grid_walk", N, 865))
    out["walk.boll_held_w3"] = seeded("boll", [3, 2.0], ("grid64_walk", N, 866, 35, 0.7))          # flat windows, exactly summable
    out["walk.flow_recent_is_window"] = seeded("flow", [20, 20], ("lot_volumes", N, 867))
    out["walk.flow_window0"] = seeded("flow", [0, 0], ("lot_volumes", N, 867))
    out["walk.park"] = seeded("park", [], ("hlc_high", N, 868), ("hlc_low", N, 868))
    out["walk.park_held"] = seeded("park", [], ("hlc_high", N, 869, 2, 1, 0.9), ("hlc_low", N, 869, 2, 1, 0.9))
    # long: three tiles; zero-volume runs that are shorter (5) and longer (100, 30) than the window of 20
    runs = [[40, 5], [700, 100], [2040, 30]]
    out["long.boll_cent_w20"] = seeded("boll", [20, 2.0], ("grid_walk", LONG, 870))
    out["long.boll_g64_w100"] = seeded("boll", [100, 2.0], ("grid64_walk", LONG, 871))
    for lg in (False, True):
        tag = "log" if lg else "simple"
        out[f"long.vwap_exact_{tag}_w20"] = seeded("vwap", [20, lg], ("grid64_walk", LONG, 872), ("int_volumes", LONG, 873, runs))
        out[f"long.vwap_lot_{tag}_w20"] = seeded("vwap", [20, lg], ("grid_walk", LONG, 874), ("lot_volumes", LONG, 875))
    out["long.flow_lot_w20_r5"] = seeded("flow", [20, 5], ("lot_volumes", LONG, 876))
    out["long.vpin_lot_w32"] = seeded("vpin", [32], ("lot_volumes", LONG, 877), ("lot_volumes", LONG, 878))
    out["long.park"] = seeded("park", [], ("hlc_high", LONG, 879), ("hlc_low", LONG, 879))
    return out


def zero_run_cases():
    """Exactly summable inputs: a zero run shorter than the window holds nothing, a longer one holds, one over the first window
    leaves NaN until the first window with volume."""
    out = {}
    c = ("grid64_walk", N, 880)
    out["zeros.vwap_short_w20"] = seeded("vwap", [20, False], c, ("int_volumes", N, 881, [[100, 19]]))
    out["zeros.vwap_exact_w20"] = seeded("vwap", [20, False], c, ("int_volumes", N, 881, [[100, 20]]))
    out["zeros.vwap_long_w20"] = seeded("vwap", [20, True], c, ("int_volumes", N, 881, [[100, 75], [300, 21]]))
    out["zeros.vwap_first_w20"] = seeded("vwap", [20, True], c, ("int_volumes", N, 881, [[0, 33]]))
    out["zeros.vwap_first_exact_w20"] = seeded("vwap", [20, False], c, ("int_volumes", N, 881, [[0, 20]]))
    out["zeros.vwap_all_w3"] = seeded("vwap", [3, False], c, ("int_volumes", N, 881, [[0, N]]))
    out["zeros.vwap_w1"] = seeded("vwap", [1, True], c, ("int_volumes", N, 881, [[0, 2], [50, 7]]))
    out["zeros.vpin_w20"] = seeded("vpin", [20], ("int_volumes", N, 882, [[100, 40]]), ("int_volumes", N, 883, [[100, 40]]))
    out["zeros.flow_w20_r5"] = seeded("flow", [20, 5], ("int_volumes", N, 884, [[100, 40]]))
    return out


def zero_lot_cases():
    """Zero-volume bars among volumes that are not exactly summable (30 % of the bars and a run of 60 over the tile edge), one tile
    and 52 elements so that every output is stored: a zero recent or past part of a flow window and a vpin window of zero bars are
    exactly 0.0 in the reference, whatever the total in front of them; vwap's all-zero windows are its own sliding-sum residue.
    With a NaN in element 5 every prefix sum of flow behind it is NaN, and so is every output, on windows of zero bars too."""
    out = {}
    n, runs = 2048 + 52, [[2048 - 30, 60]]
    out["zerolot.flow_w20_r1"] = seeded("flow", [20, 1], ("zero_lot_volumes", n, 960, runs))
    out["zerolot.flow_w20_r5"] = seeded("flow", [20, 5], ("zero_lot_volumes", n, 960, runs))
    for w, r in ((1, 0), (20, 1), (20, 5)):
        out[f"zerolot.flow_nan_w{w}_r{r}"] = seeded("flow", [w, r], ("zero_lot_nan", n, 960, runs, 5))
    out["zerolot.vpin_kilo_w20"] = seeded("vpin", [20], ("zero_lot_kilo", n, 961, runs), ("zero_lot_kilo", n, 962, runs))
    out["zerolot.vwap_log_w20"] = seeded("vwap", [20, True], ("grid_walk", n, 963), ("zero_lot_volumes", n, 964, runs))
    return out


def nan_cases():
    out = {}
    for where, at in (("first", 5), ("after", 300)):
        c = H.grid_walk(N, 890)
        c[at] = np.nan
        out[f"nan.boll_{where}_w20"] = case("boll", (c,), [20, 2.0])
        c, v = H.grid_walk(N, 891), H.lot_volumes(N, 892)
        c[at] = np.nan                     # NaN while the bar is in the window, and in wsum for good
        out[f"nan.vwap_close_{where}_w20"] = case("vwap", (c, v), [20, True])
        c, v = H.grid64_walk(N, 893), H.int_volumes(N, 894)
        v[at] = np.nan                     # vsum is NaN from there on: held for good
        out[f"nan.vwap_volume_{where}_w20"] = case("vwap", (c, v), [20, False])
        v = H.lot_volumes(N, 895)
        v[at] = np.nan
        out[f"nan.flow_{where}_w20_r5"] = case("flow", (v,), [20, 5])
        b, s = H.lot_volumes(N, 896), H.lot_volumes(N, 897)
        b[at] = np.nan
        out[f"nan.vpin_buy_{where}_w20"] = case("vpin", (b, s), [20])
        b, s = H.int_volumes(N, 898), H.int_volumes(N, 899)
        s[at] = np.nan
        s[at + 100:at + 103] = np.nan
        out[f"nan.vpin_sell_{where}_w20"] = case("vpin", (b, s), [20])
        h, lo, _ = (a.copy() for a in H.hlc_walk(N, 900))
        h[at] = np.nan
        lo[at + 1] = np.nan
        out[f"nan.park_{where}"] = case("park", (h, lo), [])
    h, lo, _ = (a.copy() for a in H.hlc_walk(60, 901))
    lo[3] = 0.0                            # inf
    lo[4] = -lo[4]                         # a negative ratio: NaN
    h[5] = 0.0                             # log(0) ** 2: inf
    h[6] = lo[6] = 0.0                     # 0 / 0
    out["edge.park"] = case("park", (h, lo), [])
    return out


def length_cases():
    out = {}
    w = 10
    for n in (0, 1, w - 1, w, w + 1):
        c = H.grid_walk(max(n, 2), 910 + n)[:n]
        v, u = H.lot_volumes(max(n, 2), 920 + n)[:n], H.lot_volumes(max(n, 2), 930 + n)[:n]
        out[f"length.n{n}.boll"] = case("boll", (c,), [w, 2.0])
        out[f"length.n{n}.vwap"] = case("vwap", (c, v), [w, True])
        out[f"length.n{n}.flow"] = case("flow", (v,), [w, 3])
        out[f"length.n{n}.vpin"] = case("vpin", (v, u), [w])
        out[f"length.n{n}.park"] = case("park", (c + 1.0, c), [])
    out["window0.vpin"] = case("vpin", (H.lot_volumes(40, 940), H.lot_volumes(40, 941)), [0])
    return out


def refused_calls():
    """Arguments this project refuses with ValueError; what the interpreted reference does with them is recorded beside."""
    c, v = H.grid_walk(40, 950), H.lot_volumes(40, 951)
    out = {}
    out["refused.boll_w0"] = case("boll", (c,), [0, 2.0])
    out["refused.vwap_w0"] = case("vwap", (c, v), [0, False])
    out["refused.flow_r-1"] = case("flow", (v,), [10, -1])
    out["refused.vpin_w-1"] = case("vpin", (v, v), [-1])
    out["refused.vwap_unequal"] = case("vwap", (c, v[:-1]), [5, False])
    out["refused.vpin_unequal"] = case("vpin", (v, v[:-1]), [5])
    out["refused.park_unequal"] = case("park", (c, c[:-1]), [])
    return out


def run(mod, c, host_log=True, product_square=True):
    """`mod` None: the helper.  Reference: as compiled, or with NumPy's own log, or with the interpreter's pow for `** 2`."""
    ins = tuple(a.copy() for a in c["inputs"])
    if mod is Reference:
        for m in MODULES:
            m.np = (HostLogNumpy() if product_square else HostLogPowNumpy()) if host_log else np
        if c["fn"] == "boll" and product_square:
            ins = tuple(Compiled(a) for a in ins)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            r = H.call(c["fn"], ins, c["args"], mod=mod)
        return ("ok", np.asarray(r))
    except Exception as e:                                        # noqa: BLE001 -- recorded as data
        return ("raises", type(e).__name__, str(e))
    finally:
        for m in MODULES:
            m.np = np


def differs(a, b):
    """The elements in which a and b differ: NaN equals NaN, a zero of the other sign differs."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return -1
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    bad |= (a == b) & (np.signbit(a) != np.signbit(b))
    return int(bad.sum())


def main():
    out, manifest = {}, {}
    cases = {}
    for group in (series_cases, zero_run_cases, zero_lot_cases, nan_cases, length_cases, refused_calls):
        cases.update(group())
    for name, c in cases.items():
        ins = c["inputs"]
        entry = {"fn": c["fn"], "args": c["args"], "n": int(len(ins[0]))}
        if c["source"]:
            entry["source"] = c["source"]
            entry["input_sha256"] = [H.sha256(a) for a in ins]
        else:
            for k, a in enumerate(ins):
                out[f"{name}.in{k}"] = a
        own, ref = run(None, c), run(Reference, c)
        if name.startswith("refused."):
            if not (own[0] == "raises" and own[1] == "ValueError"):
                raise SystemExit(f"{name}: the helper does not refuse this call")
            entry.update(raises=own[1], message=own[2],
                         reference=f"raises {ref[1]}" if ref[0] == "raises" else
                         f"returns ({int(np.isnan(ref[1]).sum())} NaN, {int(np.isinf(ref[1]).sum())} inf of {len(ref[1])})")
            manifest[name] = entry
            continue
        if ref[0] != "ok":
            raise SystemExit(f"{name}: the reference raises {ref[1:]} -- case refused")
        if own[0] != "ok" or differs(ref[1], own[1]) != 0:
            raise SystemExit(f"{name}: reference and helper disagree ({own[0]}, {differs(ref[1], own[1]) if own[0] == 'ok' else own[1:]})"
                             " -- case refused")
        if any(np.isinf(a).any() for a in ins):
            raise SystemExit(f"{name}: an infinite input -- outside the contract")
        if c["fn"] in ("vwap", "flow", "park"):
            plain = run(Reference, c, host_log=False)
            entry["np_log_differs"] = differs(plain[1], ref[1]) if plain[0] == "ok" else -1
        if c["fn"] in ("boll", "park"):
            plain = run(Reference, c, product_square=False)
            entry["py_pow_differs"] = differs(plain[1], ref[1]) if plain[0] == "ok" else -1
        if len(ref[1]) <= STORED_MAX:
            out[name + ".out"] = ref[1]
        else:
            entry["output_sha256"] = H.sha256(H.nan_canonical(ref[1].astype(np.float64)))
        entry.update(dtype=str(ref[1].dtype), finite=int(np.isfinite(ref[1]).sum()), nan=int(np.isnan(ref[1]).sum()),
                     inf=int(np.isinf(ref[1]).sum()))
        if c["fn"] == "vwap":
            entry["held"] = int(H.vwap_distance(*ins, *c["args"], sums=True)[1].sum())
            entry["zero_windows"] = int(H.zero_windows(ins[1], c["args"][0]).sum())
        if c["fn"] == "boll":
            entry["flat"] = int(H.flat_windows(ins[0], c["args"][0]).sum())
        manifest[name] = entry
    for k in sorted(manifest):
        print(k, {a: b for a, b in manifest[k].items() if not a.endswith("_sha256") and a != "source"})
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "runsum.npz"), **out)
    with open(os.path.join(gold, "runsum.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    print(len(manifest), "cases,", os.path.getsize(os.path.join(gold, "runsum.npz")), "+",
          os.path.getsize(os.path.join(gold, "runsum.json")), "bytes")


if __name__ == "__main__":
    main()
