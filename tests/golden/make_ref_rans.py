#!/usr/bin/env python3
"""Generates ref_rans.json in this directory: what the reference's own rANS coder (its rans_byte.h, compiled in place into
oracle/_ref/librefrans.so by oracle/Makefile) computes on the cases of tests/test_oracle.py, kept as lengths and sha256.
With it those tests pin the oracle's rANS and the product's rANS algebra to the reference on a machine that has no
reference tree; where oracle/_ref is built they compare with it directly as well.
Re-run (where oracle/_ref/librefrans.so exists):  python tests/golden/make_ref_rans.py
"""
import ctypes as C
import hashlib
import json
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "librefrans.so")
OUT = os.path.join(HERE, "ref_rans.json")

BLOCK_NS = (1, 2, 17, 1000, 131072)


def random_entries(rng, n, raw_frac=0.1):
    """valid coder entries: (freq, cum) with cum+freq <= 4096, some raw bytes"""
    freq = rng.integers(1, 4097, n)
    # skew towards small and large frequencies
    freq = np.where(rng.random(n) < 0.3, rng.integers(1, 8, n), freq)
    cum = (rng.random(n) * (4096 - freq + 1)).astype(np.int64)
    e = np.stack([freq, cum], axis=1).astype(np.uint16)
    raw = rng.random(n) < raw_frac
    e[raw, 0] = 0
    e[raw, 1] = rng.integers(0, 256, raw.sum())
    return e


def block_entries(n):
    return random_entries(np.random.default_rng(n), n)


def algebra_cases():
    """(freq, start, states) for every freq 1..4096: the starts 0, 4096 - freq and one drawn, each with edge and drawn states"""
    rng = np.random.default_rng(7)
    edge_states = [1 << 23, (1 << 23) + 1, (1 << 31) - 1, (1 << 31) - 256, 1 << 30, (1 << 27) - 1, 1 << 27]
    for freq in range(1, 4097):
        for start in {0, 4096 - freq, int(rng.integers(0, 4096 - freq + 1))}:
            states = edge_states + [(freq << 19) - 1, freq << 19, min((freq << 27) - 1, (1 << 31) - 1), min(freq << 27, (1 << 31) - 1)] + rng.integers(1 << 23, 1 << 31, 6).tolist()
            yield freq, start, [int(max(1 << 23, min(x, (1 << 31) - 1))) for x in states]


def algebra_records(params, step):
    """the records of algebra_cases in order: params(freq, start) -> (x_max, rcp, shift, bias - start, 4096 - freq) once per
    (freq, start), then step(x, start, freq) -> (new state, byte count, bytes...) per state; each keyed by its case"""
    for freq, start, states in algebra_cases():
        yield (freq, start, None), tuple(params(freq, start))
        for x in states:
            yield (freq, start, x), tuple(step(x, start, freq))


def digest(records):
    h = hashlib.sha256()
    for _, r in records:
        h.update(struct.pack(f"<{len(r)}I", *r))
    return h.hexdigest()


def sha256(a) -> str:
    return hashlib.sha256(bytes(a)).hexdigest()


class Ref:
    """the reference's coder through oracle/_ref/librefrans.so (oracle/ref_rans.c)"""

    def __init__(self, so=REF_SO):
        self.lib = C.CDLL(so)
        self.lib.ref_enc_put_symbol.restype = C.c_uint32

    def block(self, e):
        n = len(e)
        out = np.zeros(2 * n + 16, dtype=np.uint8)
        scratch = np.zeros(2 * n + 16, dtype=np.uint8)
        sz = self.lib.ref_rans_block(e.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p),
                                     scratch.ctypes.data_as(C.c_void_p), scratch.size)
        return bytes(out[:sz])

    def decode_values(self, data, e):
        """the reference decoder's walk over `data`: (bytes used, the 12-bit value or raw byte taken per entry)"""
        vals = np.zeros(len(e), dtype=np.uint16)
        buf = np.frombuffer(data + b"\0" * 8, dtype=np.uint8)
        used = self.lib.ref_rans_decode_values(buf.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), len(e),
                                               vals.ctypes.data_as(C.c_void_p))
        return used, vals

    def params(self, freq, start):
        r5 = (C.c_uint32 * 5)()
        self.lib.ref_enc_symbol_init(start, freq, r5)
        x_max, rcp, bias, cmpl, shift = list(r5)
        return x_max, rcp, shift, (bias - start) & 0xFFFFFFFF, cmpl

    def step(self, x, start, freq):
        b, n = (C.c_uint8 * 8)(), C.c_int()
        s = self.lib.ref_enc_put_symbol(x, start, freq, b, C.byref(n))
        return (s, n.value) + tuple(b[:n.value])


def main():
    ref = Ref()
    blocks = {}
    for n in BLOCK_NS:
        e = block_entries(n)
        data = ref.block(e)
        used, vals = ref.decode_values(data, e)
        blocks[str(n)] = {"bytes": len(data), "sha256": sha256(data), "used": int(used), "values_sha256": sha256(vals.astype("<u2").tobytes())}
    recs = list(algebra_records(ref.params, ref.step))
    res = {"source": "the reference's rans_byte.h through oracle/ref_rans.c (oracle/_ref/librefrans.so)",
           "blocks": blocks, "algebra": {"records": len(recs), "sha256": digest(recs)}}
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
