"""CPU: the oracle against the REFERENCE on a fixed-seed slice of tools/fuzz_reference.py's random campaign (600 cases, seed 20260929,
sizes up to 36 000).  The reference's answers to every call of that slice are stored data (tests/golden/fuzz_reference_slice.npz,
recorded by oracle/gen_fuzz_reference.py where the reference is at hand): the cases are regenerated from the seed, the oracle computes
its side, and the recorded answers stand in the reference's place under the campaign's own comparison policy (tools/fuzz_parity.py).
An answer the oracle matched bit for bit when the slice was recorded is stored as its digest and must be matched bit for bit again."""
import builtins
import os

import numpy as np

from tests import _refcalls as R
from tools import fuzz_parity as FP

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_reference_slice.npz")


def _exception(rec):
    """the recorded exception as an instance with the same class name and its nearest built-in base"""
    names = rec["exc"]
    base = next(c for c in (getattr(builtins, n, None) for n in names) if isinstance(c, type) and issubclass(c, BaseException))
    cls = base if base.__name__ == names[0] else type(names[0], (base,), {})
    return cls(rec["msg"])


class _Replay:
    """one entry of fuzz_reference's `pkg`: each call returns (or raises) the next recorded answer of the case"""
    def __init__(self, name, calls, arrays):
        self._name, self._calls, self._arrays = name, calls, arrays

    def __getattr__(self, attr):
        key = f"{self._name}.{attr}"

        def call(*a, **kw):
            rec = next(self._calls)
            assert rec["fn"] == key, f"the case calls {key} where the recording has {rec['fn']}"
            if "exc" in rec:
                raise _exception(rec)
            v = R.dec(rec["result"], self._arrays)
            return R.to_pandas(v) if isinstance(v, dict) and v.get("__df__") else v
        return call


def _resolve(got, want, name):
    """the reference's answer with every digest replaced by the oracle's output it stands for; a mismatch is a failure"""
    if isinstance(got, R.Digest):
        assert got.matches(want), f"{name}: not the reference's answer (recorded as the digest of the oracle's bit-identical output)"
        return want
    if isinstance(got, (tuple, list)) and isinstance(want, (tuple, list)) and len(got) == len(want):
        return type(got)(_resolve(g, w, name) for g, w in zip(got, want))
    return got


def _outcome(thunk):
    try:
        return thunk(), None
    except Exception as e:      # noqa: BLE001 -- judged by the campaign's both()
        return None, e


def _give(value, exc):
    if exc is not None:
        raise exc
    return value


_campaign_both = FP.both


def _both(fn, got_thunk, want_thunk, name):
    """tools/fuzz_parity.both with the recorded digests resolved against the oracle's output first"""
    want, we = _outcome(want_thunk)
    got, ge = _outcome(got_thunk)
    if ge is None and we is None:
        got = _resolve(got, want, name)
    _campaign_both(fn, lambda: _give(got, ge), lambda: _give(want, we), name)


def test_oracle_against_the_reference_on_random_cases(orc, monkeypatch):
    monkeypatch.setattr(FP, "both", _both)
    manifest, arrays = R.load(PATH)
    assert len(manifest["records"]) == manifest["cases"] == 600
    fails, skipped = [], 0
    for it, case in enumerate(manifest["records"]):
        calls = iter(case["calls"])
        pkg = {k: _Replay(k, calls, arrays) for k in ("base", "logic", "utils", "futils", "vol", "volume", "io")}
        rng = np.random.default_rng([manifest["seed"], it])
        with np.errstate(all="ignore"):
            msg = FP.one_case(rng, orc, pkg, False, manifest["hi"])
        assert next(calls, None) is None, f"case {it}: recorded calls left over"
        if msg and "NotImplementedError" in msg:        # no namesake / ill-conditioned ewmst: skipped by the campaign as well
            skipped += 1
        elif msg:
            fails.append(f"[seed {manifest['seed']} case {it}] {msg}")
    assert not fails, "\n".join(f[:600] for f in fails[:10])
    assert skipped == sum(bool(c["outcome"]) for c in manifest["records"]) < 60, skipped
