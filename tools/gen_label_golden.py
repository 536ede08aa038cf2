#!/usr/bin/env python3
"""Writes tests/golden/labels.npz + labels.json: outputs of the REFERENCE's triple_barrier / average_uniqueness /
return_attribution on synthetic tapes that the tests regenerate from their seed (oracle.synth).  Build container only: imports the
reference in pure-Python mode through oracle/shim, like tools/fuzz_reference.py; no GPU, nothing of the product.

A case is refused unless the reference and tests/_label_ref.py agree exactly on every label and touch index, so that no fixture
rests on a decision inside rounding noise.
    python tools/gen_label_golden.py [reference checkout]
"""
import contextlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402

import finmlkit.label.tbm as RT  # noqa: E402
import finmlkit.label.weights as RW  # noqa: E402

from oracle import oracle as orc  # noqa: E402
from tests import _label_ref as H  # noqa: E402

INF = float("inf")
# name: (seed, ticks, events, (bottom, top), vertical barrier s, min close time s, meta, target scale, unsorted)
CASES = {
    "symmetric":      (101, 200_000, 1000, (1.0, 1.0), 60.0, 1.0, False, 1.0, False),
    "meta":           (102, 200_000, 1000, (1.0, 2.0), 60.0, 0.0, True, 1.0, False),
    "upper_disabled": (103, 200_000, 1000, (1.0, INF), 60.0, 1.0, False, 1.0, False),
    "vertical_inf":   (104, 200_000, 1000, (1.0, 1.0), INF, 1.0, False, 3.0, False),
    "tight":          (105, 200_000, 1000, (1.0, 1.0), 60.0, 0.0, False, 1e-6, False),
    "wide":           (106, 200_000, 1000, (1.0, 1.0), 60.0, 1.0, False, 30.0, False),
    "unsorted":       (107, 200_000, 1000, (0.5, 1.5), 120.0, 1.0, False, 1.0, True),
    "concurrent":     (108, 200_000, 1200, (1.0, 1.0), 600.0, 1.0, False, 30.0, False),
}


def make_inputs(name):
    """Events, targets and sides of a case (stored in the fixture; the tape itself is regenerated from the seed)."""
    seed, n, ne, _, vb, _, meta, scale, unsorted = CASES[name]
    ts, px, _, _ = orc.synth(seed, 0, n)
    rng = np.random.default_rng(seed)
    lc = np.log(px)
    w = 1200 if vb != INF else 4000
    sigma = float(np.std(lc[w:] - lc[:-w]))                       # the move of one window, as a volatility estimate would give
    last = n - 2 if vb == INF else int(np.searchsorted(ts, ts[-1] - int(vb * 1e9))) - 1
    if name == "tight":                                           # three events in four sit in front of a tick whose price differs:
        moves = np.flatnonzero(px[1:last + 1] != px[:last])       # with a barrier this tight they touch at their first tick
        first = rng.choice(moves, 3 * ne // 4, replace=False)
        rest = rng.choice(np.setdiff1d(np.arange(last), first), ne - len(first), replace=False)
        ev = np.sort(np.concatenate([first, rest])).astype(np.int64)
    else:
        ev = np.sort(rng.choice(last, ne, replace=False)).astype(np.int64)
    if unsorted:
        rng.shuffle(ev)
    tg = sigma * scale * (0.5 + rng.random(ne))
    sd = rng.integers(-1, 2, ne).astype(np.int8) if meta else None
    return ts, px, ev, tg, sd


def main():
    out, manifest = {}, {}
    for name, (seed, n, ne, hb, vb, mc, meta, scale, unsorted) in CASES.items():
        ts, px, ev, tg, sd = make_inputs(name)
        min_ret = 1e-5 if meta else 0.0
        with contextlib.redirect_stdout(io.StringIO()):           # the reference prints a warning per skipped event
            lab, tch, ret, rat = RT.triple_barrier(ts, px, ev, tg, hb, vb, mc, sd, min_ret)
        hl, ht, hr, hq, skipped = H.triple_barrier(ts, px, ev, tg, hb, vb, mc, sd, min_ret)
        ok = ~skipped
        if skipped.sum() * 100 >= ne:
            raise SystemExit(f"{name}: the reference skips {int(skipped.sum())} of {ne} events")
        if not (np.array_equal(lab[ok], hl[ok]) and np.array_equal(tch[ok], ht[ok])):
            raise SystemExit(f"{name}: reference and helper disagree on a label or a touch index -- case refused")
        tch = np.where(skipped, ev, tch)                          # uninitialised in the reference
        avg, conc = RW.average_uniqueness(ts, ev, tch)
        att = RW.return_attribution(ev, tch, px, conc, False)
        attn = RW.return_attribution(ev, tch, px, conc, True)
        for k, v in (("event_idx", ev), ("targets", tg), ("side", sd), ("labels", lab), ("touch_idx", tch), ("returns", ret),
                     ("ratios", rat), ("skipped", skipped), ("avg_uniqueness", avg), ("concurrency", conc),
                     ("return_attribution", att), ("return_attribution_norm", attn)):
            if v is not None:
                out[f"{name}.{k}"] = np.asarray(v)
        manifest[name] = {"seed": seed, "n": n, "events": ne, "horizontal_barriers": [str(hb[0]), str(hb[1])],
                          "vertical_barrier": str(vb), "min_close_time_sec": mc, "meta": meta, "min_ret": min_ret,
                          "skipped": int(skipped.sum()), "touch_first_tick": int((tch == ev + 1).sum()),
                          "vertical_touches": int((np.asarray(rat) != 1.0).sum()), "max_concurrency": int(conc.max()),
                          "mean_concurrency": float(conc[conc > 0].mean())}
        print(name, manifest[name])
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "labels.npz"), **out)
    with open(os.path.join(gold, "labels.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
