#!/usr/bin/env python3
"""Writes tests/golden/lz.json: the closed forms of the encoded-series entropies as cases with their values,
from the formulas alone -- no library, no device, no reference implementation.

    constant, or period P <= lookback     every match length is lookback + 1:  H = log2(lookback + 1) / (lookback + 1)
    codes[k] = k mod A, A > lookback      no lag matches, every match length is 1:  H = log2(lookback + 1)
    plug-in, a constant window            one word:  exactly 0.0
    plug-in, k mod A, word 1, A | window  A codes of equal count:  log2 A

usage: gen_lz_golden.py [OUT.json]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lz.json")


def main():
    konto = []
    for lookback, window in ((1, 2), (3, 6), (3, 7), (16, 64), (63, 126), (64, 129), (65, 200), (200, 400), (200, 600)):
        value = math.log2(lookback + 1) / (lookback + 1)
        konto.append({"message": "constant", "code": 1, "lookback": lookback, "window": window, "match_length": lookback + 1, "value": value})
        for period in sorted({2, 3, lookback} - {1}):
            if period <= lookback:
                konto.append({"message": "period", "period": period, "lookback": lookback, "window": window,
                              "match_length": lookback + 1, "value": value})
        for modulus in (lookback + 1, 255):
            if lookback < modulus <= 255:
                konto.append({"message": "ramp", "modulus": modulus, "lookback": lookback, "window": window, "match_length": 1,
                              "value": math.log2(lookback + 1)})
    plugin = []
    for window, word in ((1, 1), (2, 2), (64, 1), (64, 2), (100, 3), (600, 12), (4096, 1)):
        plugin.append({"message": "constant", "code": 1, "window": window, "word": word, "alphabet": 2, "value": 0.0})
    for modulus, window in ((2, 64), (3, 66), (16, 64), (16, 256), (64, 576), (255, 510)):
        plugin.append({"message": "ramp", "modulus": modulus, "window": window, "word": 1, "alphabet": max(2, modulus),
                       "value": math.log2(modulus)})
    with open(OUT, "w") as fh:
        json.dump({"note": "closed forms; see tools/gen_lz_golden.py", "kontoyiannis": konto, "plugin": plugin}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {OUT}: {len(konto)} + {len(plugin)} cases")


if __name__ == "__main__":
    main()
