#!/usr/bin/env python3
"""Record every call the REFERENCE'S OWN tests/labels make to triple_barrier, average_uniqueness, return_attribution, time_decay,
class_balance_weights and to TBMLabel / SampleWeights as data: tests/golden/label_refcalls.npz (arrays) + label_refcalls.json
(function, encoded arguments, result or exception type and message, citing test).  Build container only; the machinery (encoder,
wrappers, pytest plugin) is oracle/record_reference_tests.py's, the reference runs in pure-Python mode through oracle/shim.

A recorded call whose indices lie outside 0 <= event_idx <= touch_idx < n (the reference slices silently into something else there;
this project returns FMK_E_ARG), or whose prices break the label contract (finite, > 0), stays in the fixture with a `skip_reason`.
    python tools/record_label_tests.py
"""
import copy
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

from oracle import record_reference_tests as R  # noqa: E402  (puts the reference and the shim on sys.path)

import numpy as np  # noqa: E402
import pytest  # noqa: E402

TARGETS = {"finmlkit.label.tbm": ["triple_barrier"],
           "finmlkit.label.weights": ["average_uniqueness", "return_attribution", "time_decay", "class_balance_weights"]}
TEST_FILES = ["tests/labels/test_triple_barrier.py", "tests/labels/test_label_concurrency.py",
              "tests/labels/test_average_uniqueness.py", "tests/labels/test_return_attribution.py",
              "tests/labels/test_time_decay.py", "tests/labels/test_class_balace_weights.py", "tests/labels/test_label_kit.py"]


def enc(v):
    """R.enc, with a TradesData stored as the two columns the label code reads"""
    from finmlkit.bar.data_model import TradesData
    if isinstance(v, TradesData):
        return {"t": "dict", "v": {"__trades__": R.enc(True), "timestamp": R.enc(v.data.timestamp.values.copy()),
                                   "price": R.enc(v.data.price.values.copy()), "amount": R.enc(v.data.amount.values.copy())}}
    return R.enc(copy.deepcopy(v))


def record(rec, fn, *args, **kwargs):
    R.STATE["depth"] += 1                  # the functions called inside are not recorded a second time
    try:
        out = fn(*args, **kwargs)
    except Exception as e:                 # noqa: BLE001 -- the exception IS the recorded behaviour
        rec["raises"] = {"type": type(e).__name__, "msg": str(e)}
        R.CALLS.append(rec)
        raise
    finally:
        R.STATE["depth"] -= 1
    rec["result"] = enc(out)
    R.CALLS.append(rec)
    return out


def wrap_kit():
    """TBMLabel(...) with compute_labels / compute_weights, and the two static methods of SampleWeights"""
    import finmlkit.label.kit as K
    init, labels, weights = K.TBMLabel.__init__, K.TBMLabel.compute_labels, K.TBMLabel.compute_weights

    def k_init(self, *args, **kwargs):
        self._rec_ctor = {"args": [enc(a) for a in args], "kwargs": {k: enc(v) for k, v in kwargs.items()}}
        rec = {"fn": "TBMLabel", "module": K.__name__, "test": R.STATE["test"], "kind": "tbm_init", "args": self._rec_ctor["args"],
               "kwargs": self._rec_ctor["kwargs"]}
        try:
            init(self, *args, **kwargs)
        except Exception as e:             # noqa: BLE001
            rec["raises"] = {"type": type(e).__name__, "msg": str(e)}
            R.CALLS.append(rec)
            raise

    def k_labels(self, trades):
        rec = {"fn": "TBMLabel.compute_labels", "module": K.__name__, "test": R.STATE["test"], "kind": "tbm", "ctor": self._rec_ctor,
               "args": [enc(trades)], "kwargs": {}}
        return record(rec, labels, self, trades)

    def k_weights(self, trades, *a, **kw):
        rec = {"fn": "TBMLabel.compute_weights", "module": K.__name__, "test": R.STATE["test"], "kind": "tbm",
               "ctor": self._rec_ctor, "args": [enc(trades)] + [enc(x) for x in a], "kwargs": {k: enc(v) for k, v in kw.items()}}
        return record(rec, weights, self, trades, *a, **kw)

    K.TBMLabel.__init__, K.TBMLabel.compute_labels, K.TBMLabel.compute_weights = k_init, k_labels, k_weights
    for name in ("compute_info_weights", "compute_final_weights"):
        orig = getattr(K.SampleWeights, name)

        def make(name=name, orig=orig):
            def call(*args, **kwargs):
                rec = {"fn": "SampleWeights." + name, "module": K.__name__, "test": R.STATE["test"], "kind": "static",
                       "args": [enc(a) for a in args], "kwargs": {k: enc(v) for k, v in kwargs.items()}}
                if R.STATE["depth"] > 0:
                    return orig(*args, **kwargs)
                return record(rec, orig, *args, **kwargs)
            return staticmethod(call)
        setattr(K.SampleWeights, name, make())


def comparable(c, arrays):
    """None, or why this project does not define the call the way the reference happens to behave"""
    if "raises" in c or c.get("kind"):
        return None
    a = [arrays[e["k"]] if e.get("t") == "nd" else None for e in c["args"]]
    kw = {k: arrays[e["k"]] if e.get("t") == "nd" else None for k, e in c["kwargs"].items()}

    def arg(i, name):
        return a[i] if i < len(a) else kw.get(name)
    if c["fn"] == "triple_barrier":
        close, ev, ts = arg(1, "close"), arg(2, "event_idxs"), arg(0, "timestamps")
        if not (np.all(np.isfinite(close)) and np.all(close > 0)):
            return "prices outside the label contract (finite, > 0)"
        if np.any(ev < 0) or np.any(ev >= len(close)):
            return "event index outside [0, n): Python's negative indexing in the reference, FMK_E_ARG here"
        if np.any(np.diff(ts) < 0):
            return "unsorted timestamps: searchsorted's answer is undefined"
        return None
    if c["fn"] in ("average_uniqueness", "return_attribution"):
        first = c["fn"] == "average_uniqueness"
        ev, tc = arg(1 if first else 0, "event_idxs"), arg(2 if first else 1, "touch_idxs")
        n = len(arg(0, "timestamps") if first else arg(2, "close"))
        if len(ev) and (np.any(ev < 0) or np.any(tc < ev) or np.any(tc >= n)):
            return "indices outside 0 <= event_idx <= touch_idx < n: the reference slices into something else, FMK_E_ARG here"
    return None


def main():
    for modname, names in TARGETS.items():
        mod = importlib.import_module(modname)
        for n in names:
            orig = getattr(mod, n)
            w = R.wrap(modname, n, orig)
            setattr(mod, n, w)
            for m in list(sys.modules.values()):
                if m is None or not getattr(m, "__name__", "").startswith("finmlkit"):
                    continue
                for attr, val in list(vars(m).items()):
                    if val is orig:
                        setattr(m, attr, w)
    wrap_kit()
    plug = R.Plugin()
    os.chdir(R.REF)
    rc = pytest.main(["-q", "-p", "no:cacheprovider", "--no-header", "--rootdir", R.REF, "-o", "addopts=", *TEST_FILES],
                     plugins=[plug])
    os.chdir(ROOT)
    for c in R.CALLS:
        c["test_outcome"] = plug.outcome.get(c["test"], "unknown")
        if c["test"]:
            c["test"] = c["test"].replace(R.REF + "/", "")
        why = comparable(c, R.ARRAYS)
        if why:
            c["skip_reason"] = why
    manifest = {"generator": "tools/record_label_tests.py", "reference_test_files": TEST_FILES, "pytest_exit_code": int(rc),
                "n_tests": len(plug.outcome), "n_tests_passed": sum(1 for v in plug.outcome.values() if v == "passed"),
                "tests_not_passed": {k.replace(R.REF + "/", ""): plug.reason.get(k, "?")
                                     for k, v in sorted(plug.outcome.items()) if v != "passed"},
                "calls": R.CALLS}
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "label_refcalls.npz"), **R.ARRAYS)
    with open(os.path.join(gold, "label_refcalls.json"), "w") as fh:
        json.dump(manifest, fh, indent=0)
    by = {}
    for c in R.CALLS:
        by[c["fn"]] = by.get(c["fn"], 0) + 1
    print("tests run %d, passed %d; calls %d, arrays %d" % (manifest["n_tests"], manifest["n_tests_passed"], len(R.CALLS),
                                                            len(R.ARRAYS)))
    print(by)
    print("raise:", sum(1 for c in R.CALLS if "raises" in c), "not comparable:", sum(1 for c in R.CALLS if "skip_reason" in c))
    print("not passed:", manifest["tests_not_passed"])
    print("opaque:", [c["fn"] for c in R.CALLS if '"opaque"' in json.dumps(c)])


if __name__ == "__main__":
    main()
