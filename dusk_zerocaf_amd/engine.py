"""Batch engine: the host-side mirror of zerocaf's field / scalar / edwards / ristretto
operator surface over the C ABI (include/zerocaf_hip.h).

Arrays use the reference's in-memory layout: FieldElement / Scalar = (n, 5) uint64 limbs
(radix 2^52), EdwardsPoint = (n, 20) uint64 (X|Y|Z|T), encodings = (n, 32) uint8.
Inputs may be numpy arrays (host memory: staged over PCIe by the library) or torch CUDA
tensors (device memory: used in place on the engine's stream, asynchronous).  Outputs are
of the same kind as the first input.  All arithmetic runs in the HIP library.
"""
from __future__ import annotations

import ctypes as C
import functools
import threading

import numpy as np

from . import _lib
from .dlog import DlogMixin
from .generators import GeneratorsMixin
from .hash_batch import HashMixin
from .point_sums import PointSumsMixin
from .ristretto_batch import RistrettoBatchMixin
from .scalar_vec import ScalarVecMixin
from .scalar_ext import ScalarExtMixin
from .shared_scalar import SharedScalarMixin

STRICT = 0          # double_and_add (Mul<Scalar>)
LTR_BIN = 1         # ltr_bin_mul
BINARY_NAF = 2      # binary_naf_mul
FAST = 16           # same group element, not limb-exact (windowed, dedicated doubling)

U64, U8 = np.dtype(np.uint64), np.dtype(np.uint8)


def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "device")


def _one_call(method):
    """The stream binding (_follow_torch_stream), the allocation of the outputs and the launch of one call are one step under
    the engine's lock: torch's current stream is thread-local and ctypes drops the GIL, so without it another thread could
    rebind the slot between this thread's bind and its launch, and the kernel would run on that thread's stream.  The lock is
    re-entrant (MsmBases goes through the engine's helpers); `self` is the Engine, or an object with one in `.engine`."""
    @functools.wraps(method)
    def locked(self, *args, **kwargs):
        with getattr(self, "engine", self)._launch_lock:
            return method(self, *args, **kwargs)
    return locked


class Engine(ScalarExtMixin, RistrettoBatchMixin, HashMixin, SharedScalarMixin, GeneratorsMixin, PointSumsMixin, DlogMixin, ScalarVecMixin):
    """One zc_ctx.  `devices=None` = one slot on torch's current device when torch is loaded and sees a GPU; otherwise
    zc_ctx_create(NULL, 0): the calling thread's current HIP device (whatever hipSetDevice chose), read back from the
    context.  The context reads the library's tuning knobs (ZC_* environment variables)
    once, here.  `lib`: another build of the same ABI (tests: the ZC_TEST_HOOKS build)."""

    _launch_lock = threading.RLock()    # the fallback of an object made without __init__; every engine gets its own below

    def __init__(self, devices=None, lib=None):
        self.lib = lib if lib is not None else _lib.load()
        self.ctx = C.c_void_p()
        self._launch_lock = threading.RLock()   # bind + allocate + launch of one call: see _one_call
        self._pinned_stream = False      # set_stream() was called: keep that stream
        self._last_torch_stream = {}     # device slot -> handle of the torch stream last bound to it
        if not devices:
            import sys
            torch = sys.modules.get("torch")
            devices = [torch.cuda.current_device()] if torch is not None and torch.cuda.is_available() else []
        arr = (C.c_int * len(devices))(*devices) if devices else None
        rc = self.lib.zc_ctx_create(arr, len(devices), C.byref(self.ctx))
        _lib.check(rc, "zc_ctx_create", self.lib)
        # slot i of the context = HIP device _devices[i], as the context itself reports it: always known, so the
        # ownership check of _follow_torch_stream always runs
        self._devices = [self.lib.zc_ctx_device(self.ctx, i) for i in range(self.lib.zc_ctx_device_count(self.ctx))]
        if any(d < 0 for d in self._devices) or (devices and self._devices != list(devices)):
            got = self._devices
            self.close()
            raise _lib.ZerocafHipError("zc_ctx_create: the context reports devices %s, asked for %s" % (got, list(devices)))

    def close(self):
        if self.ctx:
            self.lib.zc_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @_one_call
    def set_stream(self, stream_handle):
        """Launch on the caller's HIP stream (handle 0 = the HIP null stream, which is what
        torch.cuda.current_stream().cuda_stream is by default)."""
        _lib.check(self.lib.zc_ctx_set_stream(self.ctx, C.c_void_p(stream_handle), 1), "zc_ctx_set_stream", self.lib)
        self._pinned_stream = True

    @_one_call
    def use_own_stream(self):
        """Back to the default: host batches run on the context's own stream; calls on torch CUDA
        tensors follow torch's current stream of that device (see _follow_torch_stream)."""
        for slot in range(len(self._devices)):
            _lib.check(self.lib.zc_ctx_set_stream_dev(self.ctx, slot, None, 0), "zc_ctx_set_stream_dev", self.lib)
        self._pinned_stream = False
        self._last_torch_stream = {}

    def _follow_torch_stream(self, t):
        """Device tensors are produced and consumed on torch's streams and their memory belongs to
        torch's caching allocator, so unless the caller pinned a stream with set_stream() every
        call on torch tensors is enqueued on torch.cuda.current_stream(device): ordered after the
        work that produced the inputs, and outputs allocated with torch.empty are safe to use from
        that stream.  (The library orders a stream switch with an event, no host sync.)
        The stream is bound to the context slot that OWNS the tensor's device (a multi-device engine keeps
        one stream per slot); a tensor on a device outside the context is refused here, before any launch."""
        if self._pinned_stream:
            return
        import torch
        dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
        if dev not in self._devices:
            raise _lib.ZerocafHipError("tensor on cuda:%d, but this engine's context owns devices %s" % (dev, self._devices))
        slot = self._devices.index(dev)
        h = torch.cuda.current_stream(t.device).cuda_stream
        if self._last_torch_stream.get(slot) != h:
            _lib.check(self.lib.zc_ctx_set_stream_dev(self.ctx, slot, C.c_void_p(h), 1), "zc_ctx_set_stream_dev", self.lib)
            self._last_torch_stream[slot] = h

    def synchronize(self):
        _lib.check(self.lib.zc_ctx_synchronize(self.ctx), "zc_ctx_synchronize", self.lib)

    # ------------------------------------------------------------------ helpers
    def _prep(self, x, width, dtype, lead=1):
        """Rows of shape (n, [t,] width) -- `lead` leading dimensions -- as the library reads them: a contiguous numpy array
        of `dtype` (converted when it is not), or a contiguous torch tensor with elements of that size, used in place on
        torch's current stream.  Returns (array, pointer, leading shape)."""
        if _is_torch(x):
            shape = x.shape
            assert x.is_contiguous() and len(shape) == lead + 1 and shape[-1] == width, (shape, lead, width)
            assert x.element_size() == dtype.itemsize
            self._follow_torch_stream(x)
            return x, x.data_ptr(), shape[:lead]
        a = np.ascontiguousarray(x, dtype=dtype)
        assert a.ndim == lead + 1 and a.shape[-1] == width, (a.shape, lead, width)
        return a, a.ctypes.data, a.shape[:lead]

    def _inputs(self, ins, lead=1):
        """_prep for every (array, width, dtype) of `ins`, which must agree in their leading shape:
        (arrays, pointers, that shape)."""
        arrs, ptrs, shape = [], [], None
        for x, w, dt in ins:
            a, p, s = self._prep(x, w, dt, lead)
            assert shape is None or s == shape, "row counts differ: %s, %s" % (shape, s)
            shape = s
            arrs.append(a)
            ptrs.append(p)
        return arrs, ptrs, shape

    @staticmethod
    def _alloc(like, n, width, dtype):
        """An output of n rows (width 0: a flat array) of the kind of `like`.  Tensors: uint8 for bytes, else the input's own
        8-byte dtype, or int64 when it has none."""
        shape = (n, width) if width else (n,)
        if _is_torch(like):
            import torch
            tdt = torch.uint8 if dtype == U8 else like.dtype if like.element_size() == 8 else torch.int64
            t = torch.empty(shape, dtype=tdt, device=like.device)
            return t, t.data_ptr()
        a = np.empty(shape, dtype=dtype)
        return a, a.ctypes.data

    def _call(self, name, *args):
        _lib.check(getattr(self.lib, name)(self.ctx, *args), name, self.lib)

    @_one_call
    def _rows(self, name, ins, outs, mid=(), tail=(), out=None):
        """One batched entry point, name(ctx, inputs..., mid..., outputs..., n, tail...): `ins` = (array, width, dtype) per
        input, `outs` = (width, dtype) per output, allocated like the first input -- except the first when the caller
        brings it (`out`).  Returns the output, or the tuple of them."""
        if out is not None:
            ins = ins + [(out, outs[0][0], outs[0][1])]
        arrs, ptrs, shape = self._inputs(ins)
        n = shape[0]
        res = [self._alloc(arrs[0], n, w, dt) for w, dt in outs]
        if out is not None:
            res[0] = (arrs.pop(), ptrs.pop())
        self._call(name, *ptrs, *mid, *[p for _, p in res], n, *tail)
        return res[0][0] if len(res) == 1 else tuple(a for a, _ in res)

    def _bin(self, name, a, b, w): return self._rows(name, [(a, w, U64), (b, w, U64)], [(w, U64)])
    def _un(self, name, a, w): return self._rows(name, [(a, w, U64)], [(w, U64)])
    def _flag(self, name, a, w): return self._rows(name, [(a, w, U64)], [(0, U8)])
    def _checked(self, name, a, w, wout, dt=U64): return self._rows(name, [(a, w, U64)], [(wout, dt), (0, U8)])
    def _decode(self, name, b, wout): return self._rows(name, [(b, 32, U8)], [(wout, U64), (0, U8)])

    # ------------------------------------------------------------------ FieldElement (field.rs)
    def fe_add(self, a, b): return self._bin("zc_fe_add", a, b, 5)
    def fe_sub(self, a, b): return self._bin("zc_fe_sub", a, b, 5)
    def fe_mul(self, a, b): return self._bin("zc_fe_mul", a, b, 5)
    def fe_neg(self, a): return self._un("zc_fe_neg", a, 5)
    def fe_square(self, a): return self._un("zc_fe_square", a, 5)
    def fe_invert(self, a): return self._checked("zc_fe_invert", a, 5, 5)
    def fe_div(self, a, b): return self._rows("zc_fe_div", [(a, 5, U64), (b, 5, U64)], [(5, U64), (0, U8)])
    def fe_half(self, a): return self._un("zc_fe_half", a, 5)
    def fe_pow(self, a, e): return self._bin("zc_fe_pow", a, e, 5)
    def fe_legendre_symbol(self, a): return self._flag("zc_fe_legendre_symbol", a, 5)
    def fe_is_positive(self, a): return self._flag("zc_fe_is_positive", a, 5)
    def fe_mod_sqrt(self, a, sign): return self._rows("zc_fe_mod_sqrt", [(a, 5, U64)], [(5, U64), (0, U8)], mid=(C.c_int(int(sign)),))
    def fe_from_bytes(self, b): return self._rows("zc_fe_from_bytes", [(b, 32, U8)], [(5, U64)])
    def fe_to_bytes(self, a): return self._rows("zc_fe_to_bytes", [(a, 5, U64)], [(32, U8)])
    def fe_sqrt_ratio_i(self, u, v): return self._rows("zc_fe_sqrt_ratio_i", [(u, 5, U64), (v, 5, U64)], [(5, U64), (0, U8)])

    def fe_inv_sqrt(self, a):
        """InvSqrt (field.rs:443-460): (1/sqrt(a) or sqrt(i/a), was_square)."""
        return self._checked("zc_fe_inv_sqrt", a, 5, 5)

    # ------------------------------------------------------------------ Scalar (scalar.rs)
    def sc_add(self, a, b): return self._bin("zc_sc_add", a, b, 5)
    def sc_sub(self, a, b): return self._bin("zc_sc_sub", a, b, 5)
    def sc_mul(self, a, b): return self._bin("zc_sc_mul", a, b, 5)
    def sc_neg(self, a): return self._un("zc_sc_neg", a, 5)
    def sc_square(self, a): return self._un("zc_sc_square", a, 5)

    # the Scalar operations beside the default scalar-mul path (scalar.rs:165-182, 285-322, 352-415)
    def sc_half(self, a): return self._un("zc_sc_half", a, 5)
    def sc_pow(self, a, e): return self._bin("zc_sc_pow", a, e, 5)
    def sc_shr(self, a, shift): return self._rows("zc_sc_shr", [(a, 5, U64)], [(5, U64)], mid=(C.c_uint(int(shift)),))

    def sc_into_bits(self, a):
        """into_bits: (n, 256) uint8, the bits of to_bytes(), least significant first."""
        return self._rows("zc_sc_into_bits", [(a, 5, U64)], [(256, U8)])

    def sc_compute_naf(self, a, width=0):
        """compute_NAF (width 0) / compute_window_NAF(width 2..7): (n, 256) int8 digits."""
        out = self._rows("zc_sc_compute_naf", [(a, 5, U64)], [(256, U8)], mid=(C.c_uint(int(width)),))
        if _is_torch(out):
            import torch
            return out.view(torch.int8)
        return out.view(np.int8)

    def sc_from_bytes(self, b): return self._decode("zc_sc_from_bytes", b, 5)
    def sc_to_bytes(self, a): return self._rows("zc_sc_to_bytes", [(a, 5, U64)], [(32, U8)])

    # ------------------------------------------------------------------ EdwardsPoint (edwards.rs)
    def ed_add(self, p, q): return self._bin("zc_ed_add", p, q, 20)
    def ed_sub(self, p, q): return self._bin("zc_ed_sub", p, q, 20)
    def ed_double(self, p): return self._un("zc_ed_double", p, 20)
    def ed_neg(self, p): return self._un("zc_ed_neg", p, 20)

    def ed_scalar_mul(self, p, k, out=None, flags=STRICT):
        return self._rows("zc_ed_scalar_mul", [(p, 20, U64), (k, 5, U64)], [(20, U64)], tail=(flags,), out=out)

    def _same_kind(self, who, *arrays):
        assert all(_is_torch(x) == _is_torch(arrays[0]) for x in arrays), who + ": the arrays must all be numpy arrays or all torch tensors"

    @_one_call
    def ed_lincomb(self, points, scalars):
        """out[i] = sum_j scalars[i, j] * points[i, j] (zc_ed_lincomb): (n, t, 20) points and (n, t, 5) scalars, t = 1..8 --
        numpy arrays, or contiguous torch tensors on one device (the call then runs on torch's current stream and the result
        stays on the device) -> (n, 20) of the same kind.  One doubling chain per row is shared by its terms; the result is
        the same group element as the composition of ed_scalar_mul and ed_add (ed_eq / encodings), not the same limbs."""
        self._same_kind("ed_lincomb", points, scalars)
        (points, _), (pp, pk), (n, t) = self._inputs([(points, 20, U64), (scalars, 5, U64)], lead=2)
        out, po = self._alloc(points, n, 20, U64)
        self._call("zc_ed_lincomb", pp, pk, t, po, n)
        return out

    def ed_mul_by_pow_2(self, p, kexp): return self._rows("zc_ed_mul_by_pow_2", [(p, 20, U64)], [(20, U64)], mid=(C.c_uint64(kexp),))
    def ed_mul_by_cofactor(self, p): return self._un("zc_ed_mul_by_cofactor", p, 20)
    def ed_to_affine(self, p): return self._checked("zc_ed_to_affine", p, 20, 10)
    def ed_eq(self, p, q): return self._rows("zc_ed_eq", [(p, 20, U64), (q, 20, U64)], [(0, U8)])
    def ed_compress(self, p): return self._checked("zc_ed_compress", p, 20, 32, U8)
    def ed_decompress(self, b): return self._decode("zc_ed_decompress", b, 20)

    # ------------------------------------------------------------------ Ristretto (ristretto.rs)
    def ris_compress(self, p): return self._rows("zc_ris_compress", [(p, 20, U64)], [(32, U8)])
    def ris_decompress(self, b): return self._decode("zc_ris_decompress", b, 20)
    def ris_eq(self, p, q): return self._rows("zc_ris_eq", [(p, 20, U64), (q, 20, U64)], [(0, U8)])

    def ris_roundtrip_mul(self, b, k, out=None):
        return self._rows("zc_ris_roundtrip_mul", [(b, 32, U8), (k, 5, U64)], [(32, U8), (0, U8)], out=out)

    @_one_call
    def ris_lincomb(self, enc, scalars, base_scalars=None):
        """out32[i] = compress(base_scalars[i] * B + sum_j scalars[i, j] * decompress(enc[i, j])) (zc_ris_lincomb): (n, t, 32)
        uint8 encodings, (n, t, 5) scalars and, for the basepoint term, (n, 5) base scalars, t + (base term) <= 8 -- numpy
        arrays, or contiguous torch tensors on one device (the call then runs on torch's current stream and the results stay
        on the device) -> ((n, 32) uint8, (n,) uint8 accept mask) of the same kind.  The bytes are those of the reference's
        decompress / Mul<Scalar> / + / compress; a row with an undecodable term is 32 zero bytes with ok = 0."""
        self._same_kind("ris_lincomb", enc, scalars, *([] if base_scalars is None else [base_scalars]))
        (enc, _), (pe, pk), (n, t) = self._inputs([(enc, 32, U8), (scalars, 5, U64)], lead=2)
        pb = None
        if base_scalars is not None:
            _, pb, nb = self._prep(base_scalars, 5, U64)
            assert nb == (n,), "row counts differ: %s" % ((n, nb),)
        out, po = self._alloc(enc, n, 32, U8)
        ok, pko = self._alloc(enc, n, 0, U8)
        self._call("zc_ris_lincomb", pe, pk, t, pb, po, pko, n)
        return out, ok

    # ------------------------------------------------------------------ next rows (N3, N4)
    def ed_is_valid(self, p): return self._flag("zc_ed_is_valid", p, 20)
    def ris_is_valid(self, p): return self._flag("zc_ris_is_valid", p, 20)
    def ris_elligator(self, r0): return self._rows("zc_ris_elligator", [(r0, 5, U64)], [(20, U64)])
    def ris_from_uniform_bytes(self, b): return self._rows("zc_ris_from_uniform_bytes", [(b, 64, U8)], [(20, U64)])
    def proj_add(self, p, q): return self._bin("zc_proj_add", p, q, 15)
    def proj_double(self, p): return self._un("zc_proj_double", p, 15)
    def proj_to_extended(self, p): return self._rows("zc_proj_to_extended", [(p, 15, U64)], [(20, U64)])

    # ProjectivePoint beside add / double (edwards.rs:701-748, 787-912) and EdwardsPoint::coset4 (:603-610)
    def proj_neg(self, p): return self._un("zc_proj_neg", p, 15)
    def proj_sub(self, p, q): return self._bin("zc_proj_sub", p, q, 15)
    def proj_eq(self, p, q): return self._rows("zc_proj_eq", [(p, 15, U64), (q, 15, U64)], [(0, U8)])
    def proj_is_valid(self, p): return self._flag("zc_proj_is_valid", p, 15)
    def proj_scalar_mul(self, p, k): return self._rows("zc_proj_scalar_mul", [(p, 15, U64), (k, 5, U64)], [(15, U64)])

    def ed_coset4(self, p):
        """coset4: (n, 80) uint64 = four points per input point."""
        return self._rows("zc_ed_coset4", [(p, 20, U64)], [(80, U64)])

    # ------------------------------------------------------------------ fixed-base (key generation)
    def ed_mul_base(self, k): return self._rows("zc_ed_mul_base", [(k, 5, U64)], [(20, U64)])

    def ed_mul_base_wnaf(self, k, width):
        """window_naf_mul (edwards.rs:155-171) with the table indexed correctly, one launch; width 2..7."""
        return self._rows("zc_ed_mul_base_wnaf", [(k, 5, U64)], [(20, U64)], mid=(int(width),))

    def msm_plan(self, n, points_aligned16=True):
        """What the bucket method would do for a shard of n pairs on this context (a query, no device work)."""
        v = (C.c_int32 * 17)()
        self._call("zc_msm_plan", int(n), 1 if points_aligned16 else 0, v, 17)
        g = v[7]
        return {"window_bits": v[0], "windows": v[1], "affine": bool(v[2]), "record_bytes": v[3], "record_stride": v[8], "run": v[4],
                "segment_buckets": v[5], "sort_passes": v[6], "window_groups": g,
                "group_windows": [v[9 + i] for i in range(g)], "group_runs": [v[13 + i] for i in range(g)]}

    def ris_mul_base_compress(self, k): return self._rows("zc_ris_mul_base_compress", [(k, 5, U64)], [(32, U8)])

    # ------------------------------------------------------------------ MSM (not in the reference)
    @_one_call
    def _msm(self, name, points, scalars, out_ptr):
        _, (pp, pk), (n,) = self._inputs([(points, 20, U64), (scalars, 5, U64)])
        self._call(name, pp, pk, n, out_ptr)

    def msm(self, points, scalars):
        out = np.empty((1, 20), dtype=np.uint64)
        self._msm("zc_msm", points, scalars, out.ctypes.data)
        return out

    def msm_bases(self, points, window_bits=0):
        """A fixed-base table of the (n, 20) points (zc_msm_bases_create): `MsmBases.msm(scalars)` then runs the MSM of one
        or many scalar vectors against them without re-normalising the points.  window_bits 0 = the library's choice."""
        return MsmBases(self, points, window_bits)

    def msm_fixed_plan(self, n, window_bits=0):
        """What a table of n bases would be (a query, no device work)."""
        v = (C.c_int32 * 8)()
        self._call("zc_msm_fixed_plan", int(n), int(window_bits), v, 8)
        return {"window_bits": v[0], "windows": v[1], "record_stride": v[2], "run": v[3], "segment_buckets": v[4],
                "sort_passes": v[5], "table_mib": v[6], "window_groups": v[7]}

    @_one_call
    def msm_batch(self, points, scalars):
        """`batch` independent MSMs (zc_msm_batch): (batch, n, 20) points and (batch, n, 5) scalars -- numpy, or torch tensors
        on one device of this context -- give a (batch, 20) numpy array, row b = sum_i scalars[b, i] * points[b, i]."""
        _, (pp, pk), (batch, n) = self._inputs([(points, 20, U64), (scalars, 5, U64)], lead=2)
        out = np.empty((batch, 20), dtype=np.uint64)
        self._call("zc_msm_batch", pp, pk, n, batch, out.ctypes.data)
        return out

    def msm_batch_plan(self, n, batch, points_aligned16=True):
        """What zc_msm_batch would do for `batch` instances of n pairs (a query, no device work)."""
        v = (C.c_int32 * 8)()
        self._call("zc_msm_batch_plan", int(n), int(batch), 1 if points_aligned16 else 0, v, 8)
        return {"regime": "buckets" if v[0] else "scalar_mul", "window_bits": v[1], "windows": v[2], "affine": bool(v[3]),
                "run": v[4], "segment_buckets": v[5], "sort_passes": v[6], "record_stride": v[7]}

    # ---- the exchange step of a sharded MSM (BASELINE configs[4])
    @_one_call
    def msm_partial(self, points, scalars, out=None):
        """This device's sum left in device memory: a (1, 20) int64 torch CUDA tensor (asynchronous)."""
        import torch
        if out is None:
            dev = points.device if _is_torch(points) else torch.device("cuda", torch.cuda.current_device())
            out = torch.empty((1, 20), dtype=torch.int64, device=dev)
            self._follow_torch_stream(out)
        self._msm("zc_msm_partial", points, scalars, out.data_ptr())
        return out

    @_one_call
    def ed_fold_ordered(self, parts):
        """((p_0 + p_1) + p_2) + ... in index order, one kernel launch; (count, 20) -> (1, 20)."""
        parts, pp, (n,) = self._prep(parts, 20, U64)
        out, po = self._alloc(parts, 1, 20, U64)
        self._call("zc_ed_fold_ordered", pp, n, po)
        return out

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _lib.check(_lib.load().zc_comm_unique_id(buf), "zc_comm_unique_id")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == 128
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._call("zc_comm_init", buf, rank, world)

    def comm_destroy(self):
        self._call("zc_comm_destroy")

    def comm_size(self) -> int:
        """Ranks of the context's RCCL communicator as RCCL reports them (ncclCommCount); 0 without one."""
        r = C.c_int(0)
        self._call("zc_comm_size", C.byref(r))
        return r.value

    def msm_sharded(self, points, scalars):
        """This rank's shard of a global MSM through the library's own RCCL communicator
        (comm_init first): local bucket method, ncclAllGather of the 160-byte partial sums,
        ordered fold on the device.  Returns the global sum as a (1, 20) numpy array."""
        out = np.empty((1, 20), dtype=np.uint64)
        self._msm("zc_msm_sharded", points, scalars, out.ctypes.data)
        return out

    @_one_call
    def set_stream_dev(self, slot, stream_handle):
        self._call("zc_ctx_set_stream_dev", slot, C.c_void_p(stream_handle), 1)
        self._pinned_stream = True

    @staticmethod
    def host_register(arr: np.ndarray):
        _lib.check(_lib.load().zc_host_register(arr.ctypes.data, arr.nbytes), "zc_host_register")

    @staticmethod
    def host_unregister(arr: np.ndarray):
        _lib.check(_lib.load().zc_host_unregister(arr.ctypes.data), "zc_host_unregister")


class MsmBases:
    """A fixed-base MSM table owned by an Engine's context (Engine.msm_bases).  `.msm(scalars)`: (n, 5) scalars give a (1, 20)
    numpy array, (batch, n, 5) give (batch, 20); numpy or device-resident torch scalars.  `.plan`: what the table was built
    with (zc_msm_fixed_plan).  `.close()` frees the table; also usable as a context manager."""

    def __init__(self, engine, points, window_bits=0):
        self.engine = engine
        self.id = 0
        self._create(points, window_bits)

    @_one_call
    def _create(self, points, window_bits):
        engine = self.engine
        points, pp, (n,) = engine._prep(points, 20, U64)
        self.n = n
        self.plan = engine.msm_fixed_plan(n, window_bits)
        out = C.c_uint64(0)
        engine._call("zc_msm_bases_create", pp, n, int(window_bits), C.byref(out))
        self.id = out.value

    @_one_call
    def msm(self, scalars):
        if self.id == 0:
            raise _lib.ZerocafHipError("MsmBases: the table was closed")
        scalars, pk, lead = self.engine._prep(scalars, 5, U64, lead=len(scalars.shape) - 1)
        assert len(lead) in (1, 2) and lead[-1] == self.n, (lead, self.n)
        batch = 1 if len(lead) == 1 else lead[0]
        out = np.empty((batch, 20), dtype=np.uint64)
        self.engine._call("zc_msm_fixed", C.c_uint64(self.id), pk, batch, out.ctypes.data)
        return out

    def close(self):
        if self.id and self.engine.ctx:
            self.engine._call("zc_msm_bases_destroy", C.c_uint64(self.id))
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
