"""Generator sets (include/zerocaf_hip_ext_gens.h, a part of zerocaf_hip_ext.h): a few fixed points of the caller's -- the second
Pedersen generator, a recipient key, the bases of a DLEQ proof -- with a comb table each, and per row one scalar per point.

A base class of `Engine` (engine.py), like SharedScalarMixin: `generators(points)` builds the tables once (synchronous, on every
device of the context) and returns a `Generators` handle; `ed_mul_gens` / `ris_mul_gens_compress` take the handle and (n, count, 5)
scalars, numpy arrays or torch tensors like every other method, and return outputs of the kind of the input.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

U64, U8 = np.dtype(np.uint64), np.dtype(np.uint8)


class Generators:
    """A generator set owned by an Engine's context (Engine.generators).  `.id`: the library's id (0 once closed), `.count`: the
    number of generators.  `.close()` frees the tables; also usable as a context manager."""

    def __init__(self, engine, points):
        self.engine = engine
        self.id = 0
        with engine._launch_lock:                   # bind + launch are one step (engine.py: _one_call)
            points, pp, (count,) = engine._prep(points, 20, U64)
            out = C.c_uint64(0)
            engine._call("zc_gens_create", pp, count, C.byref(out))
        self.count = count
        self.id = out.value

    def close(self):
        if self.id and self.engine.ctx:
            self.engine._call("zc_gens_destroy", C.c_uint64(self.id))
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


class GeneratorsMixin:
    def generators(self, points):
        """(count, 20) points, count = 1..8, numpy or a torch tensor on a device of the context -> Generators.  Only X, Y, Z are
        read; a point that is not on the curve (or has Z = 0 mod p) is refused by the library."""
        return Generators(self, points)

    def _mul_gens(self, name, gens, scalars, width, dtype):
        if gens.id == 0:
            raise _lib.ZerocafHipError("Generators: the set was closed")
        with self._launch_lock:
            (scalars, ), (pk, ), (n, count) = self._inputs([(scalars, 5, U64)], lead=2)
            assert count == gens.count, "one scalar per generator: (n, %d, 5), got %d per row" % (gens.count, count)
            out, po = self._alloc(scalars, n, width, dtype)
            self._call(name, C.c_uint64(gens.id), pk, po, n)
            return out

    def ed_mul_gens(self, gens, scalars):
        """(n, count, 5) scalars -> (n, 20) points: sum_j scalars[i, j] * G_j, the same group elements as the composition of
        ed_scalar_mul and ed_add (the FAST contract: ed_eq / encodings, not the same limbs)."""
        return self._mul_gens("zc_ed_mul_gens", gens, scalars, 20, U64)

    def ris_mul_gens_compress(self, gens, scalars):
        """(n, count, 5) scalars -> (n, 32) uint8: the Ristretto encoding of that sum; an identity sum is 32 zero bytes."""
        return self._mul_gens("zc_ris_mul_gens_compress", gens, scalars, 32, U8)
