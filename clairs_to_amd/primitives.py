"""The shared device primitives alone, for the tests (csrc/primitives.hip): the prefix sums of csrc/scan.h, the tile scan among them, and the
line starts of csrc/lines.h, each on the device or as the plain host loop that states the operation.  numpy arrays in, new arrays out."""
import ctypes as C

import numpy as np


def _where(where):
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    from ._lib import current_stream_ptr
    return (0, C.c_void_p(current_stream_ptr())) if where == "device" else (1, None)


def constants():
    """SCAN_TILE, SORT_TILE, LINE_TILE and SORT_MAX_N as the library was compiled (cto_prim_constants)"""
    from ._lib import check, lib
    out = np.zeros(4, dtype=np.int64)
    check(lib.cto_prim_constants(out.ctypes.data))
    return dict(zip(("SCAN_TILE", "SORT_TILE", "LINE_TILE", "SORT_MAX_N"), (int(v) for v in out)))


def scan(values, dtype=np.int32, form=0, where="device", second=None, with_total=True):
    """cto_prim_scan: (out [n + 1], total or None) of an int32 vector, or ((out, total), (out2, total2)) with `second`.  dtype: np.int32 or
    np.int64, the type of the sums; form 0 scan_exclusive, form 1 k_scan_small in place; with_total: hand the kernels a `total` pointer."""
    from ._lib import check, lib
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise ValueError("dtype is int32 or int64")
    a = np.ascontiguousarray(values, dtype=np.int32)
    b = None if second is None else np.ascontiguousarray(second, dtype=np.int32)
    if a.ndim != 1 or (b is not None and b.shape != a.shape):
        raise ValueError("one vector, or two of one length")
    n = len(a)
    out, out2 = np.empty(n + 1, dtype=dt), (None if b is None else np.empty(n + 1, dtype=dt))
    total = np.zeros(2, dtype=dt) if with_total else None
    w, stream = _where(where)
    check(lib.cto_prim_scan(a.ctypes.data, None if b is None else b.ctypes.data, n, dt.itemsize * 8, int(form), w, stream, out.ctypes.data,
                            None if b is None else out2.ctypes.data, None if total is None else total.ctypes.data))
    first = (out, int(total[0]) if with_total else None)
    return first if b is None else (first, (out2, int(total[1]) if with_total else None))


def scan_tiles(values, where="device"):
    """cto_prim_scan_tiles: (exclusive prefix sums down every column, the column sums) of an int64 [n, stride] array, stride 1 .. 3"""
    from ._lib import check, lib
    a = np.array(values, dtype=np.int64, order="C", copy=True)
    if a.ndim != 2:
        raise ValueError("an [n, stride] array")
    totals = np.zeros(a.shape[1], dtype=np.int64)
    w, stream = _where(where)
    check(lib.cto_prim_scan_tiles(a.ctypes.data, a.shape[0], a.shape[1], w, stream, totals.ctypes.data))
    return a, totals


def line_starts(text, cr=False, where="device"):
    """cto_prim_line_starts: the uint32 offsets at which the lines of `text` (bytes or a uint8 vector) start"""
    from ._lib import check, lib
    t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    w, stream = _where(where)
    starts = np.empty(len(t), dtype=np.uint32)       # a text has at most as many lines as bytes
    n = check(lib.cto_prim_line_starts(t.ctypes.data if len(t) else None, len(t), int(bool(cr)), w, stream, starts.ctypes.data if len(t) else None, len(t)))
    return starts[:n].copy()


def release():
    """cto_prim_release: the device buffers of the calls above are freed and grow again from nothing"""
    from ._lib import check, lib
    check(lib.cto_prim_release())
