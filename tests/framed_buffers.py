"""Framed buffers: rows handed to the library as a pointer into the MIDDLE of one allocation (this module holds no test).

A framed buffer is one allocation laid out as [front frame | n rows | back frame].  The library gets a raw pointer to the rows,
as a caller does who passes a sub-range of a larger array (a Rust slice, a torch view).  After the call the frames are read
back and compared byte for byte: a write before row 0 or after row n - 1 has then LANDED in memory this module owns, and shows.
Nothing here turns an overrun into a fault: no guard pages, no protection changes, no memory advice, no small neighbouring
allocations.  A frame is at least 64 KiB and at least 256 rows, so that an overrun of a whole workgroup stays inside it.

Two backends, one interface: numpy (host pointers; also what the CPU self-test of these checks runs on) and torch on the GPU
(device pointers).

Inputs are framed as well and compared whole, frames and rows: no entry point writes to an input.  Their frames hold either
zeros or HOSTILE rows of the buffer's own type (hostile_frame_rows: all-ones words, the limbs of p / L, a point with
Z = 0 mod p, an undecodable encoding, scalars at or above 2^256).  A call whose outputs differ between the two fills has read
a neighbour into a result (same_outputs)."""
import ctypes as C

import numpy as np

from oracle import pymodel as pm
from tests import hostile_rows as HR
from tests import point_classes as PC
from tests import scalar_ext_rows as SX

FRAME_MIN_BYTES = 64 << 10
FRAME_MIN_ROWS = 256
OUT_ROW_FILL = 0xEE                     # what output rows hold before the call
OUT_FRAME_FILL = 0xA5                   # what output frames hold
ZERO, HOSTILE = "zero", "hostile"


def frame_bytes(row_bytes):
    """Bytes of one frame of a buffer with rows of row_bytes: >= 64 KiB, >= 256 rows, a multiple of 16."""
    return -(-max(FRAME_MIN_BYTES, FRAME_MIN_ROWS * row_bytes) // 16) * 16


class FrameError(AssertionError):
    """A frame or an input changed.  buffer: its name; side: 'front', 'back' or 'rows'; first / last: the changed byte offsets,
    relative to the first row for 'front' (negative) and 'rows', to the end of the last row for 'back' (0 = the byte after
    the last row); found: the bytes there now."""

    def __init__(self, buffer, side, first, last, found, count):
        self.buffer, self.side, self.first, self.last, self.found, self.count = buffer, side, first, last, found, count
        where = {"front": "before the first row", "back": "after the last row", "rows": "inside the (input) rows"}[side]
        AssertionError.__init__(self, "%s: %d byte(s) changed %s, offsets %+d .. %+d; found %s" % (
            buffer, count, where, first, last, " ".join("%02x" % b for b in found)))


def _tile_rows(frame_rows, row_bytes, nbytes, end_on_row):
    """nbytes of frame: the bytes of frame_rows repeated on the row grid -- ending on a row boundary (front frame) or starting
    on one (back frame)."""
    pat = np.ascontiguousarray(frame_rows).view(np.uint8).reshape(-1)
    assert len(pat) % row_bytes == 0 and len(pat) > 0
    reps = -(-(nbytes + row_bytes) // len(pat)) + 1
    long = np.tile(pat, reps)
    if end_on_row:
        return long[len(long) - nbytes:].copy()
    return long[:nbytes].copy()


class FramedBuffer:
    """[front frame | rows | back frame] in one allocation of `backend` ('numpy' or 'torch').

    rows: (n, width) array (a flat (n,) array is n rows of one element) -- the bytes the row range starts with.
    frame: a byte value, or an array of rows of the same width and dtype that is repeated through both frames on the row grid.
    shift: the rows start `shift` bytes past a 16-byte boundary (0 <= shift < 16); .ptr is their address."""

    def __init__(self, name, rows, backend="numpy", frame=0, shift=0):
        rows = np.ascontiguousarray(rows)
        self.name, self.backend, self.shift = name, backend, int(shift)
        self.shape, self.dtype = rows.shape, rows.dtype
        self.row_bytes = rows.dtype.itemsize * (rows.shape[1] if rows.ndim == 2 else 1)
        self.nbytes = rows.nbytes
        assert 0 <= self.shift < 16 and rows.ndim in (1, 2)
        F = frame_bytes(self.row_bytes)
        self.front = F + self.shift                      # the shift bytes belong to the front frame
        self.back = F
        total = self.front + self.nbytes + self.back
        img = np.empty(total, dtype=np.uint8)
        if isinstance(frame, (int, np.integer)):
            img[:self.front] = frame
            img[self.front + self.nbytes:] = frame
        else:
            frame = np.ascontiguousarray(frame, dtype=rows.dtype)
            assert frame.ndim == 2 and frame.shape[1] * frame.dtype.itemsize == self.row_bytes, (name, frame.shape, self.row_bytes)
            img[:self.front] = _tile_rows(frame, self.row_bytes, self.front, True)
            img[self.front + self.nbytes:] = _tile_rows(frame, self.row_bytes, self.back, False)
        img[self.front:self.front + self.nbytes] = rows.view(np.uint8).reshape(-1)
        self.before = img
        if backend == "numpy":
            self._store = np.empty(total + 16, dtype=np.uint8)
            base = self._store.ctypes.data
            off = -base % 16
            self._view = self._store[off:off + total]
            self._view[:] = img
        else:
            import torch
            self._store = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
            base = self._store.data_ptr()
            off = -base % 16
            self._view = self._store[off:off + total]
            self._view.copy_(torch.from_numpy(img))
        self.ptr = base + off + self.front
        assert self.ptr % 16 == self.shift
        self._after = None

    @property
    def tensor(self):
        """torch backend: the allocation (for Engine._follow_torch_stream)."""
        return self._store

    def read(self):
        """The whole allocation as bytes, read back once (call after the device has finished)."""
        if self._after is None:
            self._after = self._view.copy() if self.backend == "numpy" else self._view.cpu().numpy()
        return self._after

    def forget(self):
        self._after = None

    def rows(self):
        now = self.read()[self.front:self.front + self.nbytes]
        return now.view(self.dtype).reshape(self.shape).copy()

    def _check(self, side, lo, hi, origin):
        now, was = self.read()[lo:hi], self.before[lo:hi]
        bad = np.flatnonzero(now != was)
        if len(bad):
            first, last = int(bad[0]), int(bad[-1])
            raise FrameError(self.name, side, lo + first - origin, lo + last - origin, now[first:first + 16].tolist(), len(bad))

    def assert_frames_intact(self):
        self._check("front", 0, self.front, self.front)
        self._check("back", self.front + self.nbytes, len(self.before), self.front + self.nbytes)

    def assert_unchanged(self):
        """An input: frames and rows."""
        self.assert_frames_intact()
        self._check("rows", self.front, self.front + self.nbytes, self.front)


def hostile_frame_rows(kind, oracle=None):
    """Hostile rows for the frames of an input of `kind`, from the catalogues of tests/hostile_rows.py, tests/point_classes.py
    and tests/scalar_ext_rows.py.  kind: 'fe' / 'sc' (5 u64), 'pt' (20 u64), 'proj' (15 u64), 'enc32' / 'scbytes' (32 bytes),
    'bytes64'; 'pt*t', 'sc*t', 'enc32*t': t records per row."""
    if "*" in kind:
        base, t = kind.split("*")
        one = hostile_frame_rows(base, oracle)
        t = int(t)
        reps = -(-t // len(one)) + 1
        long = np.concatenate([one] * (reps + 1))
        return np.stack([long[i:i + t].reshape(-1) for i in range(len(one))])
    if kind == "fe":
        return np.array([w for _, w in HR.fe_patterns() if max(w) > 0], dtype=np.uint64)
    if kind == "sc":
        rows = [[HR.ALL_ONES] * 5, pm.limbs(pm.L), pm.limbs(2 * pm.L), [HR.M52] * 5] + [w for _, w in SX.zero_patterns()[1:]]
        return np.concatenate([np.array(rows, dtype=np.uint64), PC.scalars_for_torsion()])      # with the raw patterns at or above 2^256
    if kind in ("pt", "proj"):
        valid = sum(pm.pt_limbs(pm.BASEPOINT), [])
        rows = np.array([w for _, w in HR.point_patterns(valid)[1:]], dtype=np.uint64)
        assert any(HR.zero_by_value(r[10:15]) and r[:10].any() for r in rows)          # a point with Z = 0 mod p
        return np.ascontiguousarray(rows[:, :15]) if kind == "proj" else rows
    if kind in ("enc32", "scbytes"):
        rows = [np.full(32, 0xFF, dtype=np.uint8)]
        if oracle is not None:
            rows += [b for dec in (oracle.ris_decompress, oracle.ed_decompress) for _, b in HR.undecodable(dec)]
        rows.append(np.frombuffer((pm.L).to_bytes(32, "little"), dtype=np.uint8))     # a scalar encoding at L: refused
        return np.stack(rows)
    if kind == "bytes64":
        return np.stack([np.full(64, 0xFF, dtype=np.uint8), np.frombuffer((pm.L << 250).to_bytes(64, "little"), dtype=np.uint8)])
    raise KeyError(kind)


def run_framed(call, inputs, outputs, backend="numpy", fill=ZERO, in_shifts=None, out_shifts=None, alias=None, out_backend=None):
    """One call on framed buffers, checked.

    inputs:  [(name, rows array, frame rows for the HOSTILE fill)]
    outputs: [(name, rows, width (0: flat), dtype)]
    call(input pointers, output pointers) makes the call and returns once the results are in memory.
    out_backend: where the outputs live when not where the inputs do (host results of device inputs).
    alias: {output index: input index} -- that output IS that input's buffer (an in-place call); the input then may change,
    its frames may not.
    Asserts that every output frame is intact and every input unchanged (FrameError), returns the output rows."""
    in_shifts = in_shifts or [0] * len(inputs)
    out_shifts = out_shifts or [0] * len(outputs)
    alias = alias or {}
    ins = [FramedBuffer("input '%s'" % nm, rows, backend, 0 if fill == ZERO else hostile, sh)
           for (nm, rows, hostile), sh in zip(inputs, in_shifts)]
    outs = []
    for j, ((nm, n, w, dt), sh) in enumerate(zip(outputs, out_shifts)):
        if j in alias:
            outs.append(ins[alias[j]])
            continue
        shape = (n, w) if w else (n,)
        blank = np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, OUT_ROW_FILL, dtype=np.uint8).view(dt).reshape(shape)
        outs.append(FramedBuffer("output '%s'" % nm, blank, out_backend or backend, OUT_FRAME_FILL, sh))
    call([b.ptr for b in ins], [b.ptr for b in outs])
    for b in outs:
        b.assert_frames_intact()
    for i, b in enumerate(ins):
        if i in alias.values():
            b.assert_frames_intact()
        else:
            b.assert_unchanged()
    return [b.rows() for b in outs]


class NeighbourLeak(AssertionError):
    """An output depends on what lies around the input rows.  buffer: the output's name; row: the first differing row."""

    def __init__(self, buffer, row, count, what):
        self.buffer, self.row, self.count = buffer, row, count
        AssertionError.__init__(self, "%s: output '%s' differs in %d row(s), first row %d, between %s" % (what, buffer, count, row, "two runs that differ only outside the rows"))


def same_outputs(names, a, b, what=""):
    """Byte-identical outputs of two runs (lists of arrays), else NeighbourLeak with the buffer and the first row."""
    assert len(a) == len(b) == len(names)
    for nm, x, y in zip(names, a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (nm, x.shape, y.shape)
        diff = (x.reshape(len(x), -1) != y.reshape(len(y), -1)).any(axis=1)
        if diff.any():
            raise NeighbourLeak(nm, int(np.flatnonzero(diff)[0]), int(diff.sum()), what)


def host_bytes(ptr, nbytes):
    """The nbytes at host address ptr as a writable uint8 array (what the Python stand-in for the library uses)."""
    return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(ptr))
