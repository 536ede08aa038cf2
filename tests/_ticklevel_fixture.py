"""The recorded cases of the tick-level features (tests/golden/ticklevel_edges.npz + .json, written by
tools/gen_ticklevel_edges_golden.py) for the tests that replay them: the manifest, the regenerated inputs and the restatement's
outputs, each computed once and never written to."""
import json
import os

import numpy as np

from tests import _ticklevel_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "ticklevel_edges.json")))
NOTES = MANIFEST.pop("_notes")
_NPZ = np.load(os.path.join(GOLD, "ticklevel_edges.npz"))

OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v)
REFUSED = sorted(k for k, v in MANIFEST.items() if "raises" in v)
GATED_CASES = [k for k in OK_CASES if MANIFEST[k]["fn"] in H.GATED]
RV_CASES = [k for k in OK_CASES if MANIFEST[k]["fn"] == "rv"]
_INPUTS, _RESTATED = {}, {}


def case_input(name):
    """The inputs of a fixture case, regenerated from its recipe (kept, never written to)."""
    if name not in _INPUTS:
        ins = H.build(MANIFEST[name]["source"])
        for a in ins:
            a.setflags(write=False)
        _INPUTS[name] = ins
    return _INPUTS[name]


def restated(name):
    """The restatement's output of a fixture case, computed once (kept, never written to)."""
    if name not in _RESTATED:
        c = MANIFEST[name]
        out = H.call(c["fn"], case_input(name), c["args"])
        out.setflags(write=False)
        _RESTATED[name] = out
    return _RESTATED[name]


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True) and \
        np.array_equal(np.signbit(got) | np.isnan(got), np.signbit(want) | np.isnan(want))


def relative_deviation(got, want):
    ok = np.isfinite(want) & (want != 0)
    return float((np.abs(got[ok] - want[ok]) / np.abs(want[ok])).max()) if ok.any() else 0.0


def holds_reference(name, out):
    """`out` is the reference's recorded output in every bit: the stored array, or its hash."""
    if name + ".out" in _NPZ.files:
        return same_bits(out, _NPZ[name + ".out"])
    return H.sha256(H.nan_canonical(out)) == MANIFEST[name]["output_sha256"]
