"""Scalar vector ops mod L (include/zerocaf_hip_scvec.h, a header of its own): row sums, inner products and power rows -- the
<a, b>, <a, y^n> and y^0 .. y^(n-1) of an inner-product argument, the weighted sum of a batch verifier, a Shamir evaluation as a
dot product with a power row.

A base class of `Engine` (engine.py), like PointSumsMixin: the methods take numpy arrays or torch tensors like every other method
and return outputs of the kind of the first input.  Values are read as sum (w_i mod 2^52) 2^(52 i); every result is the
canonical five limbs of the residue.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

U64 = np.dtype(np.uint64)
DOT_SHARED_B = 1


class ScalarVecMixin:
    def sc_sum_rows(self, a):
        """(n, terms, 5) scalars, terms >= 0 -> (n, 5): the sum of every row mod L.  terms = 0 gives zero rows."""
        with self._launch_lock:                     # bind + launch are one step (engine.py: _one_call)
            a, pa, (n, terms) = self._prep(a, 5, U64, lead=2)
            out, po = self._alloc(a, n, 5, U64)
            self._call("zc_sc_sum_rows", pa if terms else po, terms, po, n)      # terms = 0: nothing of `a` is read
            return out

    def sc_dot_rows(self, a, b, shared_b=False):
        """(n, terms, 5) x (n, terms, 5) -> (n, 5): sum_j a[i, j] * b[i, j] mod L.  shared_b: b is one row (terms, 5) that every
        row uses -- weights, Lagrange coefficients, a challenge vector, y^n."""
        with self._launch_lock:
            a, pa, (n, terms) = self._prep(a, 5, U64, lead=2)
            if shared_b:
                b, pb, (tb, ) = self._prep(b, 5, U64)
                assert tb == terms, "b has %d records, the rows of a have %d" % (tb, terms)
            else:
                b, pb, shape = self._prep(b, 5, U64, lead=2)
                assert tuple(shape) == (n, terms), "shapes differ: %s, %s" % ((n, terms), tuple(shape))
            out, po = self._alloc(a, n, 5, U64)
            self._call("zc_sc_dot_rows", pa if terms else po, pb if terms else po, terms, C.c_uint(DOT_SHARED_B if shared_b else 0), po, n)
            return out

    def sc_powers(self, x, terms):
        """(n, 5) scalars -> (n, terms, 5): out[i, j] = x_i^j mod L; out[i, 0] = 1 also for x = 0 mod L."""
        with self._launch_lock:
            x, px, (n, ) = self._prep(x, 5, U64)
            terms = int(terms)
            assert terms >= 0
            out, po = self._alloc(x, n * terms, 5, U64)
            self._call("zc_sc_powers", px, terms, po if terms else px, n)        # terms = 0: nothing is written
            return out.reshape(n, terms, 5)
