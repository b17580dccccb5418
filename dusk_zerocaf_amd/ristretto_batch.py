"""Batched Ristretto calls whose rows share work (include/zerocaf_hip_ext.h and zerocaf_hip_ext_sum.h, which it includes):
the encodings of doubled points, and the weighted sum of all rows of a wire-format batch as one MSM.

A base class of `Engine` (engine.py), like ScalarExtMixin: the methods use its helpers (`_rows`, `_inputs`, `_alloc`), take
numpy arrays or torch tensors like every other method and return outputs of the kind of the input.
"""
from __future__ import annotations

import numpy as np

U64, U8 = np.dtype(np.uint64), np.dtype(np.uint8)


class RistrettoBatchMixin:
    def ris_double_and_compress(self, p):
        """(n, 20) points -> (n, 32) uint8: the Ristretto encodings of 2 * P_i, without a square root -- the rows of a batch
        share inversions.  compress(k * P) for a point of order L is this call on (k * 2^-1 mod L) * P.  A row whose shared
        factor is 0 mod p by value (the points of E[8]) gives 32 zero bytes and changes no other row."""
        return self._rows("zc_ris_double_and_compress", [(p, 20, U64)], [(32, U8)])

    def ris_lincomb_sum(self, enc, scalars, base_scalars=None, weights=None):
        """The weighted sum of all rows as one MSM (zc_ris_lincomb_sum): (n, t, 32) uint8 encodings, (n, t, 5) scalars and,
        optionally, (n, 5) base scalars and (n, 5) weights -- numpy arrays, or contiguous torch tensors on one device -> (the
        32 bytes of compress(b * B + sum_i sum_j w_ij * decompress(enc[i, j])), always `bytes`: the library writes them to host
        memory and the call is synchronous; the (n,) uint8 accept mask, of the kind of the inputs).  w_ij = weights[i] *
        scalars[i, j] mod L and b = sum_i weights[i] * base_scalars[i] mod L, every operand read by value; a row with an
        undecodable term has ok = 0 and is left out of both.  A batch verifies when every ok is 1 and the bytes are zero."""
        given = [x for x in (base_scalars, weights) if x is not None]
        self._same_kind("ris_lincomb_sum", enc, scalars, *given)
        with self._launch_lock:                 # bind, allocate and launch as one step (engine._one_call)
            return self._ris_lincomb_sum_locked(enc, scalars, base_scalars, weights)

    def _ris_lincomb_sum_locked(self, enc, scalars, base_scalars, weights):
        (enc, _), (pe, pk), (n, t) = self._inputs([(enc, 32, U8), (scalars, 5, U64)], lead=2)
        per_row = []
        for x in (base_scalars, weights):
            p = None
            if x is not None:
                _, p, nx = self._prep(x, 5, U64)
                assert tuple(nx) == (n,), "row counts differ: %s" % ((n, tuple(nx)),)
            per_row.append(p)
        out = np.zeros(32, dtype=U8)
        ok, pko = self._alloc(enc, n, 0, U8)
        self._call("zc_ris_lincomb_sum", pe, pk, t, per_row[0], per_row[1], out.ctypes.data, pko, n)
        return out.tobytes(), ok
