#!/usr/bin/env python3
"""Writes tests/golden/ticklevel_edges.npz + ticklevel_edges.json: outputs of the REFERENCE's tick-level features --
comp_lagged_returns (feature/core/utils.py), ewms, ewmst_mean0, ewmst and realized_vol (feature/core/volatility.py) -- on the seeded
tapes of tests/_ticklevel_ref.py (fixture_cases: lengths and windows cut at the kernels' tile sizes, runs of equal timestamps, 3-day
gaps, a timestamp that steps back, zero and NaN prices, the odd half lives, three sigma floors) and the refused arguments.  Build
container only: imports the reference in pure-Python mode through oracle/shim, like tools/gen_recur_golden.py; no GPU, nothing of
the product.

exp and log.  The reference's functions are Numba kernels: compiled, their np.exp and np.log are the host's exp() and log(), which
is the project's contract (csrc/fmk_exp.h, csrc/fmk_log.h).  Interpreted, NumPy's own scalar routines differ from libm in the last
bit on some arguments, so the reference's modules see a numpy whose `exp` and `log` are libm's (LibmNumpy: the HostLogNumpy of
tools/gen_break_golden.py, extended by exp).  How many elements of a case the unredirected run rounds differently is recorded
("np_exp_log_differs").

The gate.  A case of comp_lagged_returns, ewmst, ewmst_mean0 or ewms is refused unless the reference and the restatement agree in
every bit, NaN positions and the sign of every zero included (ewms: with the restatement's squares taken as the interpreted run takes
them, pow(x, 2.0); "pow_differs" and "pow_deviation" say how far the contract's x * x is from that).  realized_vol is not gated exactly: its restatement is the correctly
rounded value, the interpreted reference sums pairwise; NaN and inf positions must agree, and the largest relative deviation of the
reference from the correctly rounded value is recorded per case ("reference_deviation") -- the figure the GPU's bound is set
against.  Cases of more than 2100 elements record `output_sha256` (every NaN made the canonical quiet NaN) instead of the output.
    python tools/gen_ticklevel_edges_golden.py <reference checkout>
"""
import json
import math
import os
import sys
import warnings
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_ticklevel_edges_golden.py <reference checkout>   (or FINMLKIT_REFERENCE in the environment)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402

import finmlkit.feature.core.utils as RUT  # noqa: E402
import finmlkit.feature.core.volatility as RVO  # noqa: E402

from tests import _ticklevel_ref as H  # noqa: E402

STORED_MAX = 2100                      # longer cases record the hash of their output, not the output


class LibmNumpy:
    """numpy with the scalar `exp` and `log` taken from libm."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def exp(a):
        return np.exp(a) if isinstance(a, np.ndarray) else np.float64(H.host_exp(float(a)))

    @staticmethod
    def log(a):
        return np.log(a) if isinstance(a, np.ndarray) else np.float64(H.host_log(float(a)))


class libm_in_reference:
    def __enter__(self):
        RUT.np = RVO.np = LibmNumpy()

    def __exit__(self, *a):
        RUT.np = RVO.np = np


class Reference:
    """The reference's five functions under the names tests/_ticklevel_ref.call expects."""
    comp_lagged_returns = staticmethod(RUT.comp_lagged_returns)
    ewmst = staticmethod(RVO.ewmst)
    ewmst_mean0 = staticmethod(RVO.ewmst_mean0)
    ewms = staticmethod(RVO.ewms)
    realized_vol = staticmethod(RVO.realized_vol)


def run(mod, c, ins, libm=True):
    devnull = open(os.devnull, "w")
    stdout, sys.stdout = sys.stdout, devnull                       # the reference prints a warning per zero price
    try:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)
            if mod is not None and libm:
                with libm_in_reference():
                    r = H.call(c["fn"], tuple(a.copy() for a in ins), c["args"], mod=mod)
            else:
                r = H.call(c["fn"], tuple(a.copy() for a in ins), c["args"], mod=mod)
        return ("ok", np.asarray(r, np.float64))
    except Exception as e:                                        # noqa: BLE001 -- recorded as data
        return ("raises", type(e).__name__, str(e))
    finally:
        sys.stdout = stdout
        devnull.close()


def differs(a, b):
    """The elements in which a and b differ: NaN equals NaN, a zero of the other sign differs."""
    if a.shape != b.shape:
        return -1
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    bad |= (a == b) & (np.signbit(a) != np.signbit(b))
    return int(bad.sum())


def relative_deviation(got, want):
    """The largest |got - want| / want over the finite non-zero elements of want (0.0 when there is none)."""
    ok = np.isfinite(want) & (want != 0)
    return float((np.abs(got[ok] - want[ok]) / np.abs(want[ok])).max()) if ok.any() else 0.0


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: two runs write the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.ascontiguousarray(arrays[key]), allow_pickle=False)


def main():
    out, manifest, left_out = {}, {}, []
    cases = H.fixture_cases()
    for name, c in {**cases, **H.refused_cases()}.items():
        ins = H.build(c["source"])
        entry = {"fn": c["fn"], "args": c["args"], "n": int(len(ins[-1])), "source": c["source"],
                 "input_sha256": [H.input_hash(a) for a in ins]}
        own, ref = run(None, c, ins), run(Reference, c, ins)
        if name.startswith("refused."):
            if not (own[0] == "raises" and own[1] == "ValueError"):
                raise SystemExit(f"{name}: the restatement does not refuse this call")
            entry.update(raises=own[1], message=own[2],
                         reference=f"raises {ref[1]}" if ref[0] == "raises" else
                         f"returns ({int(np.isnan(ref[1]).sum())} NaN, {int(np.isinf(ref[1]).sum())} inf of {len(ref[1])})")
            manifest[name] = entry
            continue
        if ref[0] != "ok":
            if ".half_life." in name and c["args"][0] in H.ODD_HALF_LIVES:
                left_out.append(f"{name}: the reference raises {ref[1]}")
                continue
            raise SystemExit(f"{name}: the reference raises {ref[1:]} -- case refused")
        if own[0] != "ok":
            raise SystemExit(f"{name}: the restatement raises {own[1:]} -- case refused")
        if c["fn"] != "rv":                                # (realized_vol calls neither)
            plain = run(Reference, c, ins, libm=False)
            entry["np_exp_log_differs"] = differs(plain[1], ref[1]) if plain[0] == "ok" else -1
        if c["fn"] == "ewms":
            # interpreted, the reference's `x ** 2` is libm's pow(x, 2.0); compiled it is x * x (Numba multiplies for a constant
            # integer exponent), which the restatement takes by default.  The gate runs the restatement with the interpreted power;
            # how far the contract's output is from the recorded one is recorded beside it.
            as_run = H.ewms(*ins, *c["args"], square=H.libm_square)
            if differs(ref[1], as_run) != 0:
                raise SystemExit(f"{name}: reference and restatement disagree in {differs(ref[1], as_run)} elements -- case refused")
            if not np.array_equal(np.isnan(ref[1]), np.isnan(own[1])):
                raise SystemExit(f"{name}: the two powers disagree in NaN positions -- case refused")
            entry.update(pow_differs=differs(ref[1], own[1]), pow_deviation=relative_deviation(own[1], ref[1]),
                         restatement_sha256=H.sha256(H.nan_canonical(own[1])))
        elif c["fn"] in H.GATED:
            if differs(ref[1], own[1]) != 0:
                raise SystemExit(f"{name}: reference and restatement disagree in {differs(ref[1], own[1])} elements -- case refused")
        else:
            if not (np.array_equal(np.isnan(ref[1]), np.isnan(own[1])) and np.array_equal(np.isinf(ref[1]), np.isinf(own[1]))):
                raise SystemExit(f"{name}: reference and restatement disagree in NaN or inf positions -- case refused")
            entry.update(reference_deviation=relative_deviation(ref[1], own[1]), restatement_sha256=H.sha256(H.nan_canonical(own[1])))
        if len(ref[1]) <= STORED_MAX:
            out[name + ".out"] = ref[1]
        else:
            entry["output_sha256"] = H.sha256(H.nan_canonical(ref[1]))
        entry.update(finite=int(np.isfinite(ref[1]).sum()), nan=int(np.isnan(ref[1]).sum()), inf=int(np.isinf(ref[1]).sum()),
                     zeros=int((ref[1] == 0).sum()))
        manifest[name] = entry
        print(name, {a: b for a, b in entry.items() if a in ("n", "finite", "nan", "inf", "np_exp_log_differs", "reference_deviation")},
              flush=True)
    manifest["_notes"] = {"left_out": left_out, "left_out_names": [k.split(":")[0] for k in left_out],
                          "pow_deviation_max": max(v.get("pow_deviation", 0.0) for v in manifest.values()),
                          "reference_deviation_max": max(v.get("reference_deviation", 0.0) for v in manifest.values()),
                          "math_nextafter_2_0": repr(math.nextafter(2.0, 0.0))}
    gold = os.path.join(ROOT, "tests", "golden")
    save_npz(os.path.join(gold, "ticklevel_edges.npz"), out)
    with open(os.path.join(gold, "ticklevel_edges.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    print(len(manifest) - 1, "cases,", os.path.getsize(os.path.join(gold, "ticklevel_edges.npz")), "+",
          os.path.getsize(os.path.join(gold, "ticklevel_edges.json")), "bytes; left out:", left_out)


if __name__ == "__main__":
    main()
