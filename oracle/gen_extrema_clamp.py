#!/usr/bin/env python3
"""Reference-made vectors for the order-flow extrema at the reference's start values.

comp_bar_directional_features (base.py:409-546) starts cum_volumes_min / max and cum_dollars_min / max at 1e9 / -1e9 (base.py:459-464),
so a bar whose running signed volume or dollar sum stays above 1e9 (below -1e9) from its first tick reports exactly 1e9 (-1e9).
Trades of whale size reach that: meme-token quantities of 1e9 .. 4e9, or one trade worth more than 1e9 in dollars.  The tape here
has twelve bars of a few dozen ticks:

  all buys / all sells with amounts in [1e9, 4e9), as whole multiples of 2^20 (they certify integer units) and with full mantissas;
  mixed sides on such amounts, so that the running sums cross +-1e9 both ways;
  a bar that starts small and then buys whale amounts (its minimum is the small start, not the clamp);
  bars where only the dollar sum passes 1e9 (price ~100, amounts ~2e7: the volume sums stay far below 1e9);
  an ordinary bar of amounts near 1.

The amounts are float32 and go to the reference as float64 carriers of the float32 values (oracle/gen_f32amounts.py says why): its
accumulators are then float64, as under Numba's typing.  The tape itself is stored with the result.

    python oracle/gen_extrema_clamp.py        # seconds; rewrites tests/golden/extrema_clamp.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "shim"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402

import finmlkit.bar.base as RB  # noqa: E402

SEED = 1009
DIR_KEYS = ["ticks_buy", "ticks_sell", "volume_buy", "volume_sell", "dollars_buy", "dollars_sell", "mean_spread", "max_spread",
            "cum_ticks_min", "cum_ticks_max", "cum_volumes_min", "cum_volumes_max", "cum_dollars_min", "cum_dollars_max"]


def tape(seed=SEED):
    """-> (prices float64, amounts float32, sides int8, close indices int64)"""
    rng = np.random.default_rng(seed)

    def whale_units(k):                  # whole multiples of 2^20 in [1e9, 4e9)
        return rng.integers(954, 3815, k) * 2.0 ** 20

    def whale_full(k):                   # full 24-bit mantissas
        return rng.uniform(1e9, 4e9, k)

    def dollar_only(k):                  # ~2e7: at a price of ~100, 2e9 per trade; 20 of them stay below 1e9 in volume
        return rng.integers(300_000, 340_000, k) * 64.0

    def ones(k):
        return rng.integers(1, 4097, k) / 1024.0

    buy = lambda k: np.ones(k, np.int8)                                     # noqa: E731
    sell = lambda k: -np.ones(k, np.int8)                                   # noqa: E731
    mixed = lambda k: rng.choice(np.array([-1, 1], np.int8), k)             # noqa: E731
    bars = [
        (whale_units(40), buy(40)), (whale_units(40), sell(40)),
        (whale_full(40), buy(40)), (whale_full(40), sell(40)),
        (whale_units(60), mixed(60)), (whale_full(60), mixed(60)),
        (np.concatenate([ones(5), whale_units(30)]), buy(35)),
        (dollar_only(20), buy(20)), (dollar_only(20), sell(20)),
        (dollar_only(24) + rng.uniform(0, 64, 24), mixed(24)),             # full mantissas
        (ones(40), mixed(40)),
        (np.concatenate([whale_units(10), ones(10)]), sell(20)),
    ]
    am = np.concatenate([a for a, _ in bars]).astype(np.float32)
    sd = np.concatenate([s for _, s in bars])
    lens = np.array([len(s) for _, s in bars], np.int64)
    ci = np.concatenate([[-1], np.cumsum(lens) - 1]).astype(np.int64)
    px = np.round(100.0 + np.cumsum(rng.integers(-1, 2, len(am))) * 0.01, 2)
    return px, am, sd, ci


def main():
    px, am, sd, ci = tape()
    got = RB.comp_bar_directional_features(px.copy(), am.astype(np.float64), ci.copy(), sd.copy())
    d = {"price": px, "amount": am, "side": sd, "close_idx": ci, "seed": np.int64(SEED)}
    for k, v in zip(DIR_KEYS, got):
        d["dir_" + k] = np.asarray(v)
    for k, v in (("cum_volumes_min", 1e9), ("cum_volumes_max", -1e9), ("cum_dollars_min", 1e9), ("cum_dollars_max", -1e9)):
        print(f"{k}: {int((d['dir_' + k] == np.float32(v)).sum())} of {len(ci) - 1} bars at {v:g}")
    path = os.path.join(ROOT, "tests", "golden", "extrema_clamp.npz")
    np.savez_compressed(path, **d)
    print(f"{path}: {len(px)} ticks, {len(ci) - 1} bars, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
