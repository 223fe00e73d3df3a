"""Writes tests/golden/structured_primes.json: the primes nearest to the ends
of the H-bit range, as offsets.

    python tests/golden/gen_structured_primes.py

For every prime width H in WIDTHS:
  below   the first four primes below 2^H, as k with p = 2^H - k
  above   the first four primes above 2^(H-1), as k with p = 2^(H-1) + k
and for H = 1024 two pattern primes, each the first prime at or above a
repeated bit pattern (unit * reps + tail, read as a binary number), as the
offset from that number.

The search uses GMP (xfl_amd.paillier._gmp: mpz_nextprime upwards,
mpz_probab_prime_p with 25 rounds downwards) when libgmp is present and the
package's Miller-Rabin otherwise. tests/structured_keys.py turns the file into
keys; tests/test_structured_keys.py re-checks every entry.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from xfl_amd.paillier import _gmp  # noqa: E402
from xfl_amd.paillier.utils import _SMALL_PRIMES, is_probable_prime  # noqa: E402

WIDTHS = (1024, 1536, 2048, 4096)
COUNT = 4
PATTERNS = {1024: [("10000", 204, "1000"), ("10101", 204, "1011")]}
OUT = os.path.join(HERE, "structured_primes.json")


def is_prime(x):
    if x < 2000:
        return x == 2 or x in _SMALL_PRIMES
    if x % 2 == 0 or any(x % s == 0 for s in _SMALL_PRIMES):
        return False
    if _gmp.available():
        return _gmp.probab_prime(x, 25)
    return is_probable_prime(x, rounds=12, rng=random.Random(x & 0xFFFFFFFF))


def first_primes(start, step, count):
    """the first `count` primes among start, start + step, start + 2 step, ..."""
    out, x = [], start
    while len(out) < count:
        if is_prime(x):
            out.append(x)
        x += step
    return out


def pattern_value(unit, reps, tail):
    return int(unit * reps + tail, 2)


def main():
    widths = {}
    for H in WIDTHS:
        top, bot = 1 << H, 1 << (H - 1)
        entry = {"below": [top - p for p in first_primes(top - 1, -2, COUNT)],
                 "above": [p - bot for p in first_primes(bot + 1, 2, COUNT)]}
        if H in PATTERNS:
            entry["pattern"] = []
            for unit, reps, tail in PATTERNS[H]:
                v = pattern_value(unit, reps, tail)
                assert v.bit_length() == H
                p = first_primes(v | 1, 2, 1)[0] if v > 2 else 2
                entry["pattern"].append({"unit": unit, "reps": reps, "tail": tail, "offset": p - v})
        widths[str(H)] = entry
        print(H, entry, flush=True)
    doc = {"about": "offsets of the primes nearest 2^H (below: 2^H - k) and 2^(H-1) (above: 2^(H-1) + k), and of the "
                    "first prime at or above a repeated bit pattern; written by gen_structured_primes.py",
           "widths": widths}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
