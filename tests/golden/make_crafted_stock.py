#!/usr/bin/env python3
"""Generates tests/golden/crafted_stock.npz from the REFERENCE ITSELF (oracle/_ref/libsz3ref.so, built by `make -C oracle ref`): the
stock ALGO_NOPRED container the reference writes for every case of tests/crafted_stock.py but fib35, one entry per case, keyed by the
case's name. The arrays are not stored: crafted_stock.crafted(name) makes them again from the counts and the seed, and
tests/test_crafted_stock_cpu.py holds every stored container to a fresh ref_compress of that array.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import crafted_stock as cs  # noqa: E402
from oracle_binding import ref_compress  # noqa: E402

OUT = os.path.join(HERE, "crafted_stock.npz")


def main():
    out = {}
    for name in cs.FIXTURE_CASES:
        x, _ = cs.crafted(name)
        out[name] = ref_compress(x, cs.nopred_config(x.size))
        print(name, x.size, "elements ->", out[name].size, "bytes")
    np.savez(OUT, **out)  # (not compressed again: the containers are zstd's output)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
