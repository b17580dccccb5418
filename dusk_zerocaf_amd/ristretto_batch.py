"""Batched Ristretto encoders whose rows share work (include/zerocaf_hip_ext.h).

A base class of `Engine` (engine.py), like ScalarExtMixin: the methods use its `_rows` helper, take numpy arrays or torch
tensors like every other method and return outputs of the kind of the input.
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
