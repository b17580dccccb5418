"""Point sums (include/zerocaf_hip_ext_sum_rows.h, a part of zerocaf_hip_ext.h): the plain group operation over rows of any length,
out[i] = P_i0 + P_i1 + ..., on points and between the Ristretto codecs -- an ElGamal tally, an aggregate of keys or commitments,
the fold of partial results.

A base class of `Engine` (engine.py), like GeneratorsMixin: `ed_sum_rows` / `ris_sum_rows` take (n, terms, 20) points or
(n, terms, 32) encodings, numpy arrays or torch tensors like every other method, and return outputs of the kind of the input.
"""
from __future__ import annotations

import numpy as np

U64, U8 = np.dtype(np.uint64), np.dtype(np.uint8)


class PointSumsMixin:
    def ed_sum_rows(self, points):
        """(n, terms, 20) points, terms >= 0 -> (n, 20): the sum of every row under the unified addition, associated in the order
        the header fixes for `terms` (a left fold up to 32 terms, strided slices and a pairwise tree above).  The limbs depend on
        the row and on terms only.  terms = 0 gives identity rows."""
        with self._launch_lock:                     # bind + launch are one step (engine.py: _one_call)
            points, pp, (n, terms) = self._prep(points, 20, U64, lead=2)
            out, po = self._alloc(points, n, 20, U64)
            self._call("zc_ed_sum_rows", pp if terms else po, terms, po, n)      # terms = 0: nothing of `points` is read
            return out

    def ris_sum_rows(self, enc):
        """(n, terms, 32) uint8 encodings -> ((n, 32) uint8, (n,) uint8 accept mask): compress(sum_j decompress(enc[i, j])) with
        the bytes of the reference's composition; a row with an undecodable term is 32 zero bytes with ok = 0, an identity sum
        (terms = 0 included) 32 zero bytes with ok = 1."""
        with self._launch_lock:
            enc, pe, (n, terms) = self._prep(enc, 32, U8, lead=2)
            out, po = self._alloc(enc, n, 32, U8)
            ok, pko = self._alloc(enc, n, 0, U8)
            self._call("zc_ris_sum_rows", pe if terms else po, terms, po, pko, n)
            return out, ok
