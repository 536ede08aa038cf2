#!/usr/bin/env python3
"""Writes tests/golden/labels_odd.npz + labels_odd.json: outputs of the REFERENCE's triple_barrier / average_uniqueness /
return_attribution on small PLANTED tapes (stored in the fixture) with zero, negative zero, negative, NaN, infinite and subnormal
prices at block boundaries and inside blocks, odd targets, all three sides and odd barrier multipliers.  Build container only:
imports the reference in pure-Python mode through oracle/shim, like tools/gen_label_golden.py; no GPU, nothing of the product.

Meta cases record every event.  With side=None the reference raises on a NaN final return, so those events are left out of the
reference's call (at most 10 % of a case) and the tests compare them with tests/_label_ref.py alone.  A case is refused unless the
reference, the scalar restatement and the vectorised helper agree bit for bit (NaN == NaN, the sign of an infinity counts) on all
four outputs of every recorded event, and unless the counts of MINIMA below hold over the fixture.
    python tools/gen_label_odd_golden.py [reference checkout]
"""
import contextlib
import io
import json
import math
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

from tests import _label_ref as H  # noqa: E402

INF = float("inf")
NAN = float("nan")
BLOCK = 1024
N = 6 * BLOCK + 37
MINIMA = {"base_minus_inf": 8, "base_plus_inf": 8, "base_nan": 8, "nan_inside_path": 50, "touch_at_infinite_return": 20,
          "side_zero": 20, "target_nan": 10, "target_zero": 10, "target_negative": 10, "target_infinite": 10,
          "two_whole_blocks_in_window": 100}
# name: (tape, (bottom, top), vertical barrier s, min close time s, meta, made for skipping)
CASES = {
    "nan_sym":     ("nan", (1.0, 1.0), INF, 0.0, False, False),
    "nan_meta":    ("nan", (1.0, 1.0), INF, 0.05, True, False),
    "nan_lowoff":  ("nan", (INF, 1.0), 3.0, 0.05, False, False),
    "nan_negtop":  ("nan", (1.0, -0.5), INF, 0.0, True, False),
    "zero_sym":    ("zero", (1.0, 1.0), INF, 0.0, False, False),
    "zero_meta":   ("zero", (1.0, 1.0), 3.0, 0.05, True, False),
    "zero_hb00":   ("zero", (0.0, 0.0), INF, 0.0, True, False),
    "zero_upoff":  ("zero", (1.0, INF), INF, 0.05, True, False),
    "nan_skip":    ("nan", (1.0, 1.0), 1e-7, 0.0, True, True),
}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize)


def same(a, b):
    """bit for bit, except that every NaN equals every NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def make_tape(kind):
    """Epoch-scale timestamps with equal neighbours and sub-ulp gaps (float64 rounds to 256 ns there); cent prices with the odd
    values planted at k*1024 - 1, k*1024, k*1024 + 1 and inside blocks."""
    rng = np.random.default_rng({"nan": 31, "zero": 32}[kind])
    gap = np.where(rng.random(N) < 0.3, rng.integers(0, 500, N), rng.exponential(1.4e6, N).astype(np.int64))
    gap[rng.random(N) < 0.05] = 0
    ts = 1_700_000_000_000_000_000 + np.cumsum(gap).astype(np.int64)
    px = np.round(100.0 * np.exp(np.cumsum(rng.normal(0, 2e-4, N))), 2)
    # the fixture is compared bit for bit: keep prices at which the reference's log (NumPy's) is the host's
    with np.errstate(all="ignore"):
        off = np.flatnonzero(np.log(px) != H.log_column(px))
    for j in off:
        while np.log(px[j]) != H.host_log(px[j]):
            px[j] = np.round(px[j] + 0.01, 2)
    planted = {}
    if kind == "nan":            # paths run on over NaN and negative prices; a few stoppers late in the tape
        odd = [NAN, -5.0, NAN, -0.01]
        for k in range(1, 7):
            for off_, v in zip((-1, 0, 1), (odd[k % 4], odd[(k + 1) % 4], odd[(k + 2) % 4])):
                planted[k * BLOCK + off_] = v
        for j in rng.choice(np.arange(5, N - 5), 60, replace=False):
            planted.setdefault(int(j), odd[int(j) % 4])
        for j in range(3 * BLOCK + 200, 3 * BLOCK + 230):        # a run of NaN inside a block
            planted[j] = NAN
        planted[5 * BLOCK + 500] = 0.0
        planted[5 * BLOCK + 700] = INF
    else:                        # zero, -0.0, +inf, a subnormal, with some NaN: every one of them ends or starts a path
        odd = [0.0, INF, -0.0, 5e-324, NAN, -3.0]
        for k in range(1, 7):
            for off_, v in zip((-1, 0, 1), (odd[k % 6], odd[(k + 1) % 6], odd[(k + 3) % 6])):
                planted[k * BLOCK + off_] = v
        planted[2 * BLOCK - 1] = 0.0                              # event tick at the end of a block, one more zero in the next
        planted[2 * BLOCK] = 0.0
        planted[2 * BLOCK + 1] = px[2 * BLOCK + 1]
        planted[4 * BLOCK - 1] = INF
        planted[4 * BLOCK] = INF
        planted[4 * BLOCK + 1] = px[4 * BLOCK + 1]
        for j in rng.choice(np.arange(5, N - 5), 24, replace=False):
            planted.setdefault(int(j), odd[int(j) % 6])
    for j, v in planted.items():
        px[j] = v
    px[-1] = 101.0
    return ts, px, np.array(sorted(planted), np.int64)


def make_events(case, ts, px, planted, rng):
    tape, hb, vb, mc, meta, skipping = CASES[case]
    odd_ticks = planted[planted < N - 2]
    if not meta:                 # a NaN base has a NaN final return, which the reference cannot label with side=None
        with np.errstate(all="ignore"):
            odd_ticks = odd_ticks[~np.isnan(H.log_column(px[odd_ticks]))]
    at_bounds = np.array([k * BLOCK + o for k in range(1, 6) for o in (-2, -1, 0, 1)], np.int64)
    near_bounds = np.array([k * BLOCK - o for k in range(1, 5) for o in (10, 30, 45)], np.int64)
    rnd = rng.choice(N - 2, 170, replace=False)
    early = rng.choice(2 * BLOCK, 50, replace=False)                # windows that hold whole blocks
    ev = np.unique(np.concatenate([[0, 1], odd_ticks, at_bounds, near_bounds, rnd, early])).astype(np.int64)
    rng.shuffle(ev)
    ne = len(ev)
    sigma = 2e-4 * math.sqrt(500)
    tg = sigma * rng.choice([0.3, 1.0, 3.0, 40.0], ne) * (0.5 + rng.random(ne))
    for v in (NAN, 0.0, -sigma, INF):
        tg[rng.choice(ne, 5, replace=False)] = v
    sd = rng.integers(-1, 2, ne).astype(np.int8) if meta else None
    return ev, tg, sd


def count(case, ts, px, ev, tg, sd, out, recorded):
    """what the recorded events of a case exercise (from the inputs and the agreed outputs)"""
    _, hb, vb, mc, meta, _ = CASES[case]
    lab, tch, ret, rat, skipped = out
    with np.errstate(all="ignore"):
        lc = H.log_column(px)
    tsf = ts.astype(np.float64)
    c = dict.fromkeys(MINIMA, 0)
    for i in np.flatnonzero(recorded & ~skipped):
        i0 = int(ev[i])
        base = lc[i0]
        c["base_minus_inf"] += base == -INF
        c["base_plus_inf"] += base == INF
        c["base_nan"] += bool(np.isnan(base))
        t1 = int(np.searchsorted(tsf, float(ts[i0]) + vb * 1e9, side="right")) - 1
        js = H.first_open(ts, i0, t1, mc * 1e9)
        c["nan_inside_path"] += bool(np.isnan(lc[js:int(tch[i])]).any())
        with np.errstate(all="ignore"):
            up, lo = tg[i] * hb[1], -tg[i] * hb[0]
        c["touch_at_infinite_return"] += bool(np.isinf(ret[i]) and (ret[i] >= up or ret[i] <= lo))
        c["side_zero"] += bool(meta and sd[i] == 0)
        c["target_nan"] += bool(np.isnan(tg[i]))
        c["target_zero"] += tg[i] == 0.0
        c["target_negative"] += tg[i] < 0.0
        c["target_infinite"] += bool(np.isinf(tg[i]))
        c["two_whole_blocks_in_window"] += (t1 + 1) // BLOCK - (js + BLOCK - 1) // BLOCK >= 2
    return {k: int(v) for k, v in c.items()}


def weights_cases(tapes, out, manifest):
    """events spanning 0 to 5 whole blocks on both tapes: average_uniqueness and return_attribution of the reference; once more
    return_attribution under a hand-made concurrency column with runs of 0 and of negative values across block boundaries"""
    for tape, (ts, px, _) in tapes.items():
        rng = np.random.default_rng(77 + len(tape))
        ne = 240
        whole = rng.integers(0, 6, ne)
        ev = np.empty(ne, np.int64)
        tch = np.empty(ne, np.int64)
        for i in range(ne):
            b0 = int(rng.integers(0, 6 - whole[i] + 1)) if whole[i] else int(rng.integers(0, 6))
            if whole[i]:
                ev[i] = max(0, b0 * BLOCK - int(rng.integers(0, 300)))
                tch[i] = min(N - 1, (b0 + whole[i]) * BLOCK - 1 + int(rng.integers(0, 300)))
            else:
                ev[i] = b0 * BLOCK + int(rng.integers(1, 500))
                tch[i] = ev[i] + int(rng.integers(0, 500))
        ev[:4], tch[:4] = [0, BLOCK, BLOCK - 1, N - 1], [N - 1, 2 * BLOCK - 1, BLOCK, N - 1]
        with np.errstate(all="ignore"):
            avg, conc = RW.average_uniqueness(ts, ev, tch)
            att = RW.return_attribution(ev, tch, px, conc, False)
        hand = conc.copy()
        for k in range(1, 6):
            hand[k * BLOCK - 40:k * BLOCK + 25] = 0 if k % 2 else -(k * 7)
        hand[3 * BLOCK + 100:5 * BLOCK - 100] = -32768                    # whole blocks of a wrapped-around count
        hand[10:20] = 0
        with np.errstate(all="ignore"):
            att_hand = RW.return_attribution(ev, tch, px, hand, False)
        havg, hconc = H.average_uniqueness(ts, ev, tch)
        if not (same(hconc, conc) and same(havg, avg)):
            raise SystemExit(f"weights/{tape}: reference and helper disagree on concurrency or average uniqueness")
        for c_, a_ in ((conc, att), (hand, att_hand)):
            hatt, bound = H.return_attribution(ev, tch, px, c_, False)
            fin = np.isfinite(a_)
            if not (np.all(np.abs(hatt[fin] - a_[fin]) <= bound[fin]) and same(hatt[~fin], a_[~fin])):
                raise SystemExit(f"weights/{tape}: reference and helper disagree on return attribution")
        name = f"weights_{tape}"
        for k, v in (("event_idx", ev), ("touch_idx", tch), ("avg_uniqueness", avg), ("concurrency", conc),
                     ("return_attribution", att), ("hand_concurrency", hand), ("return_attribution_hand", att_hand)):
            out[f"{name}.{k}"] = v
        whole_blocks = (tch + 1) // BLOCK - (ev + BLOCK - 1) // BLOCK
        manifest[name] = {"tape": tape, "events": ne, "weights": True,
                          "whole_blocks": {str(k): int((np.maximum(whole_blocks, 0) == k).sum()) for k in range(7)},
                          "attribution_not_finite": int((~np.isfinite(att)).sum()),
                          "attribution_hand_not_finite": int((~np.isfinite(att_hand)).sum())}
        print(name, manifest[name])


def main():
    out, manifest = {}, {}
    tapes = {kind: make_tape(kind) for kind in ("nan", "zero")}
    for kind, (ts, px, planted) in tapes.items():
        out[f"tape_{kind}.ts"], out[f"tape_{kind}.close"], out[f"tape_{kind}.planted"] = ts, px, planted
    totals = dict.fromkeys(MINIMA, 0)
    for case, (tape, hb, vb, mc, meta, skipping) in CASES.items():
        ts, px, planted = tapes[tape]
        rng = np.random.default_rng(sum(map(ord, case)))
        ev, tg, sd = make_events(case, ts, px, planted, rng)
        ne = len(ev)
        min_ret = 1e-5 if meta else 0.0
        args = (hb, vb, mc)
        scalar = H.triple_barrier_scalar(ts, px, ev, tg, *args, sd, min_ret)
        with np.errstate(all="ignore"):
            vector = H.triple_barrier(ts, px, ev, tg, *args, sd, min_ret)
        names = ("labels", "touch_idx", "returns", "ratios", "skipped")
        for a, b, what in zip(scalar, vector, names):
            if not same(a, b):
                raise SystemExit(f"{case}: scalar restatement and vectorised helper disagree on {what} -- case refused")
        skipped = scalar[4]
        recorded = np.ones(ne, bool) if meta else ~(np.isnan(scalar[2]) & ~skipped)
        if (~recorded).sum() * 10 > ne:
            raise SystemExit(f"{case}: {int((~recorded).sum())} of {ne} events have a NaN final return with side=None")
        if not skipping and skipped.sum() * 100 > ne:
            raise SystemExit(f"{case}: the reference skips {int(skipped.sum())} of {ne} events")
        rec = np.flatnonzero(recorded)
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):      # a warning per skipped event
            ref = RT.triple_barrier(ts, px, ev[rec], tg[rec], hb, vb, mc, None if sd is None else sd[rec], min_ret)
        ok = ~skipped[rec]
        for r, h, what in zip(ref, scalar, names):
            if not same(np.asarray(r)[ok], h[rec][ok]):
                bad = np.flatnonzero(ok & (bits(np.asarray(r)) != bits(h[rec])))
                raise SystemExit(f"{case}: reference and restatement disagree on {what} at events {rec[bad][:5]} -- case refused")
        full = [h.copy() for h in scalar[:4]]                    # left-out and skipped events: the yardstick's values
        for f, r in zip(full, ref):
            f[rec[ok]] = np.asarray(r)[ok]
        for k, v in (("event_idx", ev), ("targets", tg), ("side", sd), ("labels", full[0]), ("touch_idx", full[1]),
                     ("returns", full[2]), ("ratios", full[3]), ("skipped", skipped), ("recorded", recorded)):
            if v is not None:
                out[f"{case}.{k}"] = np.asarray(v)
        counts = count(case, ts, px, ev, tg, sd, scalar, recorded)
        for k, v in counts.items():
            totals[k] += v
        manifest[case] = {"tape": tape, "events": ne, "horizontal_barriers": [str(hb[0]), str(hb[1])], "vertical_barrier": str(vb),
                          "min_close_time_sec": mc, "meta": meta, "min_ret": min_ret, "made_for_skipping": skipping,
                          "skipped": int(skipped.sum()), "left_out_nan_return": int((~recorded).sum()), "counts": counts}
        print(case, manifest[case])
    short = {k: (totals[k], m) for k, m in MINIMA.items() if totals[k] < m}
    if short:
        raise SystemExit(f"the fixture misses its minima: {short}")
    manifest["_totals"] = totals
    manifest["_minima"] = MINIMA
    weights_cases(tapes, out, manifest)
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "labels_odd.npz"), **out)
    with open(os.path.join(gold, "labels_odd.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    size = sum(os.path.getsize(os.path.join(gold, f)) for f in ("labels_odd.npz", "labels_odd.json"))
    print("totals", totals, "bytes", size)
    if size >= 300_000:
        raise SystemExit("the fixture is larger than 300 KB")


if __name__ == "__main__":
    main()
