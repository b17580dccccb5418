"""One scalar applied to a whole batch (include/zerocaf_hip_ext_shared.h, a part of zerocaf_hip_ext.h): a view-key scan, an
OPRF or PSI server, ElGamal under one key.

A base class of `Engine` (engine.py), like ScalarExtMixin: the methods use its helper `_rows`, take numpy arrays or torch
tensors for the rows like every other method and return outputs of the kind of the input.  The scalar `k` is ONE scalar -- five
words (radix 2^52) or a Python int below 2^260 -- and always host memory: the library reads and recodes it before the call
returns, also when the rows are on the device and the work is still in flight.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

U64, U8 = np.dtype(np.uint64), np.dtype(np.uint8)
M52 = (1 << 52) - 1


def scalar_words(k) -> np.ndarray:
    """`k` as the five host words the library reads: a Python int below 2^260, or five words as they are."""
    if isinstance(k, (int, np.integer)):
        k = int(k)
        assert 0 <= k < 1 << 260, "a scalar is below 2^260"
        return np.array([(k >> (52 * i)) & M52 for i in range(5)], dtype=U64)
    if hasattr(k, "data_ptr"):                      # a tensor: the scalar is read by the host
        k = k.detach().cpu().numpy()
    a = np.ascontiguousarray(k).view(U64) if getattr(k, "dtype", None) == np.int64 else np.ascontiguousarray(k, dtype=U64)
    assert a.shape == (5,), "one scalar: five words, got shape %s" % (a.shape,)
    return a


def scalar_vector_words(k, t) -> np.ndarray:
    """`k` as the t * 5 host words the library reads: a sequence of t Python ints below 2^260, or (t, 5) words as they are."""
    if hasattr(k, "data_ptr"):
        k = k.detach().cpu().numpy()
    if not hasattr(k, "dtype") and len(k) and all(isinstance(x, (int, np.integer)) for x in k):
        a = np.stack([scalar_words(x) for x in k])
    else:
        a = np.ascontiguousarray(k).view(U64) if getattr(k, "dtype", None) == np.int64 else np.ascontiguousarray(k, dtype=U64)
    assert a.shape == (t, 5), "one scalar per term: (%d, 5) words, got shape %s" % (t, a.shape)
    return a


class SharedScalarMixin:
    def ed_scalar_mul_shared(self, p, k):
        """(n, 20) points, one scalar -> (n, 20) points: k * P_i for every row, the same group elements as ed_scalar_mul with
        k in every row (the FAST contract: equal under ==, identical encodings, deterministic limbs)."""
        kw = scalar_words(k)
        return self._rows("zc_ed_scalar_mul_shared", [(p, 20, U64)], [(20, U64)], mid=(C.c_void_p(kw.ctypes.data),))

    def ris_mul_shared(self, enc, k):
        """(n, 32) uint8 encodings, one scalar -> ((n, 32) uint8, (n,) uint8 ok): compress(k * decompress(enc[i])), the bytes of
        ris_roundtrip_mul with k in every row; an undecodable row gives 32 zero bytes and ok = 0."""
        kw = scalar_words(k)
        return self._rows("zc_ris_mul_shared", [(enc, 32, U8)], [(32, U8), (0, U8)], mid=(C.c_void_p(kw.ctypes.data),))

    # one scalar VECTOR for the batch (include/zerocaf_hip_ext_shared_lincomb.h): out[i] = sum_j k[j] * P[i, j]
    def ed_lincomb_shared(self, p, k):
        """(n, t, 20) points, t scalars -> (n, 20) points: sum_j k[j] * p[i, j] for every row, the same group elements as
        ed_lincomb with the t scalars in every row (the FAST contract).  `k`: (t, 5) words or a list of t Python ints, host
        memory; t = 1..8."""
        with self._launch_lock:                     # bind + allocate + launch are one step (engine.py: _one_call)
            (p, ), (pp, ), (n, t) = self._inputs([(p, 20, U64)], lead=2)
            kw = scalar_vector_words(k, t)
            out, po = self._alloc(p, n, 20, U64)
            self._call("zc_ed_lincomb_shared", pp, C.c_void_p(kw.ctypes.data), t, po, n)
            return out

    def ris_lincomb_shared(self, enc, k):
        """(n, t, 32) uint8 encodings, t scalars -> ((n, 32) uint8, (n,) uint8 ok): compress(sum_j k[j] * decompress(enc[i, j])),
        the bytes of ris_lincomb without a base term and with the t scalars in every row; a row with an undecodable term gives
        32 zero bytes and ok = 0.  There is no basepoint term: pass the encoding of B as a term."""
        with self._launch_lock:
            (enc, ), (pe, ), (n, t) = self._inputs([(enc, 32, U8)], lead=2)
            kw = scalar_vector_words(k, t)
            out, po = self._alloc(enc, n, 32, U8)
            ok, pko = self._alloc(enc, n, 0, U8)
            self._call("zc_ris_lincomb_shared", pe, C.c_void_p(kw.ctypes.data), t, po, pko, n)
            return out, ok
