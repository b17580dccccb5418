"""Bounded discrete logs (include/zerocaf_hip_dlog.h): recover m from m * G, 0 <= m < bound -- the last step of exponential
ElGamal, of a tally, of a Pedersen opening with a known blinding.

A base class of `Engine` (engine.py), like GeneratorsMixin: `dlog_table(point, bits, coset4=False)` builds the baby-step table of
2^bits multiples once (synchronous, on every device of the context) and returns a `DlogTable`; its `ed(points, bound)` and
`ris(enc, bound)` take numpy arrays or torch tensors like every other method and return (m, found, ok) of the kind of the input.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

U64, U8 = np.dtype(np.uint64), np.dtype(np.uint8)
MIN_BITS, MAX_BITS, MAX_STEPS, COSET4 = 4, 22, 65536, 1


class DlogTable:
    """A baby-step table owned by an Engine's context (Engine.dlog_table).  `.id`: the library's id (0 once closed), `.bits`,
    `.coset4`.  `.close()` frees the table; also usable as a context manager."""

    def __init__(self, engine, point, bits, coset4=False):
        self.engine = engine
        self.id = 0
        with engine._launch_lock:                   # bind + launch are one step (engine.py: _one_call)
            point = point.reshape(1, 20) if hasattr(point, "reshape") else np.asarray(point, dtype=U64).reshape(1, 20)
            point, pp, _ = engine._prep(point, 20, U64)
            out = C.c_uint64(0)
            engine._call("zc_dlog_create", pp, C.c_uint(bits), C.c_uint(COSET4 if coset4 else 0), C.byref(out))
        self.bits, self.coset4 = bits, bool(coset4)
        self.id = out.value

    def _search(self, name, rows, width, dtype, bound):
        if self.id == 0:
            raise _lib.ZerocafHipError("DlogTable: the table was closed")
        eng = self.engine
        with eng._launch_lock:
            (rows, ), (pr, ), (n, ) = eng._inputs([(rows, width, dtype)])
            m, pm = eng._alloc(rows, n, 0, U64)
            found, pf = eng._alloc(rows, n, 0, U8)
            ok, po = eng._alloc(rows, n, 0, U8)
            eng._call(name, C.c_uint64(self.id), pr, C.c_uint64(bound), pm, pf, po, n)
            return m, found, ok

    def ed(self, points, bound):
        """(n, 20) points -> (m (n,), found (n,) uint8, ok (n,) uint8): found[i] = 1 and m[i] = m iff 0 <= m < bound and
        P_i == m * G (with coset4: P_i - m * G in E[4]); ok[i] = 0 for a row that is no point of the curve."""
        return self._search("zc_ed_dlog", points, 20, U64, bound)

    def ris(self, enc, bound):
        """(n, 32) Ristretto encodings -> (m, found, ok), ok[i] = 0 for a row that does not decode.  Needs a coset4 table."""
        return self._search("zc_ris_dlog", enc, 32, U8, bound)

    def close(self):
        if self.id and self.engine.ctx:
            self.engine._call("zc_dlog_destroy", C.c_uint64(self.id))
        self.id = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DlogMixin:
    def dlog_table(self, point, bits, coset4=False):
        """One point of 20 limbs (numpy, or a torch tensor on a device of the context; X, Y, Z are read) and the table size
        2^bits, bits = 4..22 -> DlogTable.  coset4: the table of 4 G, for equality modulo E[4] -- what `ris` needs."""
        return DlogTable(self, point, bits, coset4)
