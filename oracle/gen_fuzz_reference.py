#!/usr/bin/env python3
"""Record the fixed-seed slice of tools/fuzz_reference.py's campaign that tests/test_reference_live.py checks the oracle on (600
cases, seed 20260929, sizes up to 36 000) as data: every call the case generator makes to the reference's functions -- through
fuzz_reference's typed-mode adapters -- with its result or its exception, in the order made.  An answer the oracle reproduces
bit for bit (as np.testing.assert_array_equal sees it) is kept as its digest (tests/_refcalls.py: digest), every other answer as its
values; the replay compares the oracle's output with the digest, or with the values under the campaign's policy.

Runs only where the reference checkout is at hand (it goes through tools/fuzz_reference.py, which imports the reference in its
pure-Python mode through oracle/shim).  Nothing of the reference's source is stored: tests/golden/fuzz_reference_slice.npz holds
arrays + a JSON manifest in the encoding of oracle/record_reference_tests.py; tests/test_reference_live.py replays the cases with the
recorded answers in the reference's place.

    python oracle/gen_fuzz_reference.py
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

from oracle import record_reference_tests as RR  # noqa: E402
from tools import fuzz_parity as FP  # noqa: E402
from tools import fuzz_reference as FR  # noqa: E402
from tests import _refcalls as R  # noqa: E402

CASES, SEED, HI = 600, 20260929, 3000
OUT = os.path.join(ROOT, "tests", "golden", "fuzz_reference_slice.npz")
EXACT = {}             # id() -> the recorded answers the oracle matched exactly (kept alive: an id is not reused)


def _numeric(v):
    """an ndarray, or a list of numbers (the pure-Python indexers' return value), that np.asarray turns into a numeric array"""
    if not isinstance(v, (np.ndarray, list)) or (isinstance(v, list) and any(isinstance(x, (list, tuple, np.ndarray)) for x in v)):
        return None
    a = np.asarray(v)
    return a if a.dtype.kind in "biuf" else None


def mark(got, want):
    """the leaves of the reference's answer `got` that equal the oracle's `want` exactly -> EXACT"""
    if isinstance(got, (tuple, list)) and isinstance(want, (tuple, list)) and len(got) == len(want):
        for g, w in zip(got, want):
            mark(g, w)
        return
    a = _numeric(got)
    if a is not None and isinstance(want, np.ndarray) and want.dtype != object and R.digest(a) == R.digest(want):
        EXACT[id(got)] = got


_both = FP.both


def both(fn, got_thunk, want_thunk, name):
    """tools/fuzz_parity.both, noting which answers the oracle matched exactly"""
    seen = {}

    def got():
        seen["got"] = got_thunk()
        return seen["got"]

    def want():
        seen["want"] = want_thunk()
        return seen["want"]
    _both(fn, got, want, name)
    mark(seen["got"], seen["want"])


FP.both = both


def enc(v):
    if id(v) in EXACT:
        return {"t": "digest", "h": R.digest(np.asarray(v))}
    if isinstance(v, tuple):
        return {"t": "list", "kind": "tuple", "v": [enc(x) for x in v]}
    if isinstance(v, list) and any(id(x) in EXACT for x in v):
        return {"t": "list", "kind": "list", "v": [enc(x) for x in v]}
    return RR.enc(v)


class Recorder:
    """stands in for one entry of fuzz_reference's `pkg`: calls go through, results and exceptions are appended to `log`"""
    def __init__(self, name, target, log):
        self._name, self._target, self._log = name, target, log

    def __getattr__(self, attr):
        fn = getattr(self._target, attr)
        key = f"{self._name}.{attr}"

        def call(*a, **kw):
            try:
                r = fn(*a, **kw)
            except Exception as e:      # noqa: BLE001 -- the answer is the exception
                self._log.append({"fn": key, "exc": [c.__name__ for c in type(e).__mro__], "msg": str(e)[:300]})
                raise
            self._log.append({"fn": key, "result": r})          # encoded when the case is done (enc)
            return r
        return call


def main():
    from oracle import oracle as orc
    orc.build()
    FR._Base.orc = orc
    pkg = {"base": FR._Base, "logic": FR._Logic, "utils": FR.RU, "futils": FR.RFU, "vol": FR._Vol, "volume": FR._Volume, "io": FR._Io}
    cases, fails = [], 0
    warnings.simplefilter("ignore")
    for it in range(CASES):
        log = []
        rec = {k: Recorder(k, v, log) for k, v in pkg.items()}
        rng = np.random.default_rng([SEED, it])
        with np.errstate(all="ignore"):
            msg = FP.one_case(rng, orc, rec, False, HI)
        for rec_ in log:
            if "result" in rec_:
                rec_["result"] = enc(rec_["result"])
        EXACT.clear()
        cases.append({"calls": log, "outcome": msg})
        fails += bool(msg) and "NotImplementedError" not in msg
    manifest = {"cases": CASES, "seed": SEED, "hi": HI, "records": cases}
    np.savez_compressed(OUT, __manifest__=np.frombuffer(json.dumps(manifest).encode(), dtype=np.uint8), **RR.ARRAYS)
    print(f"{OUT}: {CASES} cases, {sum(len(c['calls']) for c in cases)} calls, {len(RR.ARRAYS)} arrays, "
          f"{os.path.getsize(OUT) / 1e6:.2f} MB; oracle vs reference: {fails} failures")


if __name__ == "__main__":
    main()
