"""Scalar operations for protocols: what a signature or a proof needs around the point calls and the reference does not
have -- the reduction of arbitrary 64 / 32 bytes mod L (hash-to-scalar), s = a*b + c in one pass, and a^-1 mod L.

A base class of `Engine` (engine.py): the methods use its `_rows` / `_checked` helpers, take numpy arrays or torch tensors
like every other method and return outputs of the kind of the first input.  Values are read as sum (w_i mod 2^52) 2^(52 i);
every result is the canonical five limbs of the residue.
"""
from __future__ import annotations

import numpy as np

U64, U8 = np.dtype(np.uint64), np.dtype(np.uint8)


class ScalarExtMixin:
    def sc_from_bytes_wide(self, b):
        """(n, 64) uint8 little-endian 512-bit integers -> (n, 5) limbs of v mod L; every input is accepted."""
        return self._rows("zc_sc_from_bytes_wide", [(b, 64, U8)], [(5, U64)])

    def sc_from_bytes_mod_order(self, b):
        """(n, 32) uint8 -> (n, 5) limbs of v mod L: the companion of sc_from_bytes that refuses nothing."""
        return self._rows("zc_sc_from_bytes_mod_order", [(b, 32, U8)], [(5, U64)])

    def sc_muladd(self, a, b, c, out=None):
        """a*b + c mod L per row; `out` may be any of the inputs (or a fresh (n, 5) array of the same kind)."""
        return self._rows("zc_sc_muladd", [(a, 5, U64), (b, 5, U64), (c, 5, U64)], [(5, U64)], out=out)

    def sc_invert(self, a):
        """(a^-1 mod L, ok): a row that is 0 mod L by value gives zero limbs and ok = 0, and changes no other row."""
        return self._checked("zc_sc_invert", a, 5, 5)
