"""Replay of tests/golden/label_refcalls.{npz,json} (tools/record_label_tests.py): every call the reference's own tests/labels make
to the five label functions and to TBMLabel / SampleWeights, through finmlkit_amd.label.  Values within the label contract
(DESIGN.md "labels"), exceptions by type and message."""
import builtins
import json
import os

import numpy as np

from tests import _label_ref as H
from tests._refcalls import _cmp_array, dec, to_pandas

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOST_ONLY = ("time_decay", "class_balance_weights", "SampleWeights.compute_final_weights")


def load():
    man = json.load(open(os.path.join(GOLD, "label_refcalls.json")))
    return man, np.load(os.path.join(GOLD, "label_refcalls.npz"), allow_pickle=False)


def _bind(names, args, kwargs):
    out = dict(zip(names, args))
    out.update(kwargs)
    return out


def _pandas(v):
    if isinstance(v, dict) and (v.get("__df__") or v.get("__series__")):
        return to_pandas(v)
    return v


def _trades(v):
    from finmlkit_amd.bar.data_model import TradesData
    n = len(v["timestamp"])
    return TradesData(v["timestamp"], v["price"], v["amount"], np.arange(n), timestamp_unit="ns")


def _frame(got, want, what, rtol, atol=None):
    want = to_pandas(want)
    assert list(got.columns) == list(want.columns), f"{what}: columns {list(got.columns)}"
    assert got.index.equals(want.index), f"{what}: index"
    for c in want.columns:
        assert got[c].dtype == want[c].dtype, f"{what}.{c}: dtype {got[c].dtype} vs {want[c].dtype}"
        g, w = got[c].to_numpy(), want[c].to_numpy()
        if w.dtype.kind in "iubM":
            np.testing.assert_array_equal(g, w, err_msg=f"{what}.{c}")
        elif atol is not None and c in atol:
            assert np.all(np.abs(g - w) <= atol[c]), f"{what}.{c}"
        else:
            _cmp_array(g, w, ("rtol", rtol), f"{what}.{c}")


def run_call(c, d, label, state):
    """-> a function that makes the recorded call through the package and compares its answer"""
    fn = c["fn"]
    args = [dec(a, d) for a in c["args"]]
    kwargs = {k: dec(v, d) for k, v in c["kwargs"].items()}
    what = f"{fn} <- {c['test']}"
    want = dec(c["result"], d) if "result" in c else None
    if fn == "triple_barrier":
        def go():
            got = label.triple_barrier(*args, **kwargs)
            if want is None:
                return
            b = _bind(("timestamps", "close", "event_idxs", "targets", "horizontal_barriers", "vertical_barrier",
                       "min_close_time_sec", "side", "min_ret"), args, kwargs)
            skipped = H.triple_barrier(**b)[4]
            ok = ~skipped
            assert skipped.sum() * 100 < len(skipped) or c.get("mostly_skipped"), f"{what}: {skipped.sum()} events skipped"
            state["events"] += int(ok.sum())
            state["skipped"] += int(skipped.sum())
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape, what
            np.testing.assert_array_equal(got[0][ok], want[0][ok], err_msg=what)
            np.testing.assert_array_equal(got[1][ok], want[1][ok], err_msg=what)
            tol = 4 * 2.0 ** -52 * np.abs(np.log(np.asarray(b["close"], np.float64))).max()
            assert np.array_equal(np.isnan(got[2][ok]), np.isnan(want[2][ok])), what
            assert np.all(np.nan_to_num(np.abs(got[2][ok] - want[2][ok])) <= tol), what
            _cmp_array(got[3][ok], want[3][ok], ("rtol", 1e-12), what)
    elif fn == "average_uniqueness":
        def go():
            got = label.average_uniqueness(*args, **kwargs)
            if want is None:
                return
            assert got[1].dtype == np.int16
            np.testing.assert_array_equal(got[1], want[1], err_msg=what)
            _cmp_array(got[0], want[0], ("rtol", 1e-9), what)
            state["events"] += len(want[0])
    elif fn == "return_attribution":
        def go():
            got = label.return_attribution(*args, **kwargs)
            if want is None:
                return
            b = _bind(("event_idxs", "touch_idxs", "close", "concurrency", "normalize"), args, kwargs)
            _, bound = H.return_attribution(b["event_idxs"], b["touch_idxs"], b["close"], b["concurrency"], False)
            raw = label.return_attribution(b["event_idxs"], b["touch_idxs"], b["close"], b["concurrency"], False)
            scale = len(raw) / raw.sum() if b["normalize"] else 1.0
            assert got.shape == want.shape and got.dtype == want.dtype, what
            assert np.all(np.abs(got - want) <= bound * scale + (1e-12 * np.abs(want) if b["normalize"] else 0)), what
            state["events"] += len(want)
    elif fn in ("time_decay", "class_balance_weights"):
        def go():
            got = getattr(label, fn)(*args, **kwargs)
            if want is None:
                return
            if fn == "time_decay":
                _cmp_array(got, want, ("rtol", 1e-12), what)
            else:
                assert len(got) == 4 and got[0].dtype == want[0].dtype, what
                for g, w in zip(got, want):
                    _cmp_array(g, w, ("rtol", 1e-12), what)
    elif fn == "TBMLabel":
        def go():
            label.TBMLabel(*[_pandas(a) for a in args], **{k: _pandas(v) for k, v in kwargs.items()})
    elif c.get("kind") == "tbm":
        def go():
            ctor = c["ctor"]
            key = json.dumps(ctor, sort_keys=True)
            if key not in state["tbm"]:
                state["tbm"][key] = (label.TBMLabel(*[_pandas(dec(a, d)) for a in ctor["args"]],
                                                    **{k: _pandas(dec(v, d)) for k, v in ctor["kwargs"].items()}),
                                     _trades(args[0]))
            tbm, trades = state["tbm"][key]
            if fn.endswith("compute_labels"):
                f, out = tbm.compute_labels(trades)
                _frame(f, want[0], what + "[0]", 1e-12)
                _frame(out, want[1], what + "[1]", 1e-12)
                state["events"] += len(out)
            else:
                got = tbm.compute_weights(trades, *args[1:], **kwargs)
                out = tbm.full_output
                px = trades.data.price.values
                conc = H.concurrency(len(px), out.event_idx.values, out.touch_idx.values)
                _, bound = H.return_attribution(out.event_idx.values, out.touch_idx.values, px, conc, False)
                _frame(got, want, what, 1e-9, atol={"return_attribution": bound})
    elif fn == "SampleWeights.compute_final_weights":
        def go():
            got = label.SampleWeights.compute_final_weights(*[_pandas(a) for a in args],
                                                            **{k: _pandas(v) for k, v in kwargs.items()})
            if want is not None:
                _frame(got, want, what, 1e-12)
    else:
        raise AssertionError(f"recorded function {fn} has no replay")
    return go, what


def replay(label, only_host):
    """only_host: the calls that need no device (time_decay, class_balance_weights, compute_final_weights and every call the
    reference answers with an exception: the argument checks).  -> counts"""
    man, d = load()
    assert not man["tests_not_passed"], man["tests_not_passed"]
    state = {"events": 0, "skipped": 0, "tbm": {}}
    done, left, not_comparable, raised = 0, 0, 0, 0
    for c in man["calls"]:
        if "skip_reason" in c:
            not_comparable += 1
            continue
        # "cannot normalize" is a computed condition, not an argument check: that record needs the device
        if only_host and not (c["fn"] in HOST_ONLY or ("raises" in c and c["fn"] != "return_attribution")):
            left += 1
            continue
        go, what = run_call(c, d, label, state)
        if "raises" in c:
            exc = getattr(builtins, c["raises"]["type"])
            try:
                go()
            except exc as e:
                assert str(e) == c["raises"]["msg"], f"{what}: message {str(e)!r} vs {c['raises']['msg']!r}"
            else:
                raise AssertionError(f"{what}: expected {c['raises']['type']}({c['raises']['msg']!r})")
            raised += 1
        else:
            go()
        done += 1
    return {"calls_replayed": done, "calls_raising": raised, "calls_left_to_the_gpu": left, "not_comparable": not_comparable,
            "events_compared": state["events"], "events_skipped": state["skipped"], "calls_total": len(man["calls"])}
