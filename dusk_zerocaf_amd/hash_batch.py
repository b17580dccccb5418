"""SHA-512 over batched rows (include/zerocaf_hip_ext_hash.h, a part of zerocaf_hip_ext.h): the digests, and hash-to-scalar and
hash-to-group with the digest kept in registers.

A base class of `Engine` (engine.py), like ScalarExtMixin: the methods use its helpers (`_prep`, `_alloc`, `_call`).  The message
of row i is prefix || parts[0][i] || parts[1][i] || ...: `parts` is a list of 1..4 (n, len_j) uint8 numpy arrays, or contiguous
uint8 torch tensors on one device (the call then runs on torch's current stream and the result stays on the device); `prefix`
is `bytes` (at most 256), the same for every row.  Outputs are of the kind of the parts.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

U64, U8 = np.dtype(np.uint64), np.dtype(np.uint8)
MAX_PARTS, MAX_PREFIX, MAX_ROW_BYTES = 4, 256, 65535


class HashMixin:
    def _hash_rows(self, name, parts, prefix, width, dtype):
        parts = list(parts)
        prefix = bytes(prefix)
        assert 1 <= len(parts) <= MAX_PARTS, "%s: 1..%d parts, got %d" % (name, MAX_PARTS, len(parts))
        assert len(prefix) <= MAX_PREFIX, "%s: a prefix of at most %d bytes" % (name, MAX_PREFIX)
        self._same_kind(name, *parts)
        with self._launch_lock:                 # bind, allocate and launch as one step (engine._one_call)
            return self._hash_rows_locked(name, parts, prefix, width, dtype)

    def _hash_rows_locked(self, name, parts, prefix, width, dtype):
        arrs, ptrs, lens, n = [], [], [], None
        for x in parts:
            assert len(x.shape) == 2 and x.shape[1] >= 1, "%s: every part is (n, len) with len >= 1, got %s" % (name, tuple(x.shape))
            a, p, (rows,) = self._prep(x, int(x.shape[1]), U8)
            assert n is None or rows == n, "row counts differ: %s, %s" % (n, rows)
            n = rows
            arrs.append(a)
            ptrs.append(p)
            lens.append(int(x.shape[1]))
        assert len(prefix) + sum(lens) <= MAX_ROW_BYTES, "%s: a row of at most %d bytes" % (name, MAX_ROW_BYTES)
        out, po = self._alloc(arrs[0], n, width, dtype)
        self._call(name, prefix if prefix else None, len(prefix), (C.c_void_p * len(ptrs))(*ptrs), (C.c_size_t * len(lens))(*lens), len(ptrs), po, n)
        return out

    def sha512_rows(self, parts, prefix=b""):
        """(n, 64) uint8: SHA-512(prefix || parts[0][i] || ...) per row, the bytes hashlib.sha512(...).digest() returns."""
        return self._hash_rows("zc_sha512_rows", parts, prefix, 64, U8)

    def sc_from_sha512(self, parts, prefix=b""):
        """(n, 5) limbs: sc_from_bytes_wide(sha512_rows(parts, prefix)) -- the digest as a little-endian integer mod L -- in one
        kernel; no digest is written."""
        return self._hash_rows("zc_sc_from_sha512", parts, prefix, 5, U64)

    def ris_from_sha512(self, parts, prefix=b""):
        """(n, 20) limbs: ris_from_uniform_bytes(sha512_rows(parts, prefix)), the same limbs, in one kernel."""
        return self._hash_rows("zc_ris_from_sha512", parts, prefix, 20, U64)
