"""What the kernel harnesses' helper modules (tests/helpers/*_cases.py) share: the element types, poison and guard of tools/kbench_dev.h, the
ulp helpers, and the typed-array file format of tools/kbench_io.h --

  launch record        int64 { op, B, n_ipar, n_dpar, n_arrays }; int64 ipar[]; double dpar[]; n_arrays x { int64 type, int64 count; data }
  single-launch case   magic, one record                                  (adapt, dense, mfma)
  multi-launch case    magic, int64 n_launches, the records               (rollout, loop)
  result               magic, header words of the tool's own, then arrays { int64 type, int64 count; data }

The three raw-header formats (select, sample, dynamics) stay in their own modules.  Nothing here touches the engine."""
import struct
import numpy as np

F64, I32, U64 = 0, 1, 2
DT = {F64: np.float64, I32: np.int32, U64: np.uint64}
GUARD = 64
LD = np.longdouble
U = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def is_poison(a):
    """elementwise: every byte of the entry is still the harness's fill byte 0xA5 (any element type)"""
    a = np.ascontiguousarray(a)
    return (a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)) == 0xA5).all(axis=-1)


def poisoned(shape, t=F64):
    return np.frombuffer(b"\xa5" * (int(np.prod(shape)) * np.dtype(DT[t]).itemsize), dtype=DT[t]).copy().reshape(shape)


def split_guard(a, shape):
    """-> (body reshaped, guard)"""
    n = int(np.prod(shape))
    assert a.size == n + GUARD, (a.size, n)
    return a[:n].reshape(shape), a[n:]


def ulp_of(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return np.maximum(np.spacing(a), 2.0 ** -1074)


def ulp_err(got, ref_ld):
    """|got - ref| in ulps of the float64 nearest the long-double reference"""
    r64 = np.asarray(ref_ld, dtype=LD).astype(np.float64)
    return (np.abs(np.asarray(got, dtype=np.float64).astype(LD) - np.asarray(ref_ld, dtype=LD)) / ulp_of(r64).astype(LD)).astype(np.float64)


# ---- typed arrays ------------------------------------------------------------------------------------------------------------------------------
def pack_array(t, a):
    """{ type, count; data }; None = not given (count 0)"""
    if a is None:
        return struct.pack("<2q", t, 0)
    a = np.ascontiguousarray(a, dtype=DT[t]).reshape(-1)
    return struct.pack("<2q", t, a.size) + a.tobytes()


def unpack_array(buf, off):
    """-> (type, array, offset behind it)"""
    t, n = struct.unpack_from("<2q", buf, off)
    a = np.frombuffer(buf, dtype=DT[t], count=n, offset=off + 16).copy()
    return t, a, off + 16 + a.nbytes


def pack_arrays(magic, words, arrays):
    """magic, the header words, then every (type, array or None)"""
    return b"".join([magic, struct.pack("<%dq" % len(words), *[int(v) for v in words])] + [pack_array(t, a) for t, a in arrays])


def unpack_arrays(magic, nwords, buf):
    """-> (header words; the last one is the number of arrays, [(type, array)]); the file must end behind the last array"""
    assert buf[:8] == magic, buf[:8]
    words = struct.unpack_from("<%dq" % nwords, buf, 8)
    off, arrays = 8 + 8 * nwords, []
    for _ in range(words[-1]):
        t, a, off = unpack_array(buf, off)
        arrays.append((t, a))
    assert off == len(buf), (off, len(buf))
    return words, arrays


# ---- launch records --------------------------------------------------------------------------------------------------------------------------
def pack_launch(op, B, ipar, dpar, arrays):
    """arrays: list of (type, array or None) in the op's fixed order (None = not given)"""
    return b"".join([struct.pack("<5q", op, B, len(ipar), len(dpar), len(arrays)), struct.pack("<%dq" % len(ipar), *[int(v) for v in ipar]),
                     struct.pack("<%dd" % len(dpar), *[float(v) for v in dpar])] + [pack_array(t, a) for t, a in arrays])


def unpack_launch(buf, off):
    """-> ((op, B, ipar, dpar, [(type, array)]), offset behind the record)"""
    op, B, nI, nD, nA = struct.unpack_from("<5q", buf, off)
    off += 40
    ipar = list(struct.unpack_from("<%dq" % nI, buf, off)); off += 8 * nI
    dpar = list(struct.unpack_from("<%dd" % nD, buf, off)); off += 8 * nD
    arrays = []
    for _ in range(nA):
        t, a, off = unpack_array(buf, off)
        arrays.append((t, a))
    return (op, B, ipar, dpar, arrays), off


def pack_case(magic, op, B, ipar, dpar, arrays):
    return magic + pack_launch(op, B, ipar, dpar, arrays)


def unpack_case(magic, buf):
    assert buf[:8] == magic
    rec, off = unpack_launch(buf, 8)
    assert off == len(buf)
    return rec


def pack_launches(magic, records):
    """a multi-launch case file from pack_launch records"""
    return b"".join([magic, struct.pack("<q", len(records))] + list(records))


def pack_result(magic, form, arrays):
    """a single-launch tool's result: { magic, form, guard, n_arrays } and the arrays with their guard entries"""
    return pack_arrays(magic, (form, GUARD, len(arrays)), arrays)


def unpack_result(magic, buf):
    """-> (form, [arrays as written, guard entries included])"""
    (form, guard, _), arrays = unpack_arrays(magic, 3, buf)
    assert guard == GUARD
    return form, [a for _, a in arrays]
