"""Shared by the float16 payload tests (test_payload_cpu.py, test_gpu_payload.py); imported by their driver scripts too, which run in
the interpreter that has h5py."""
import struct

import numpy as np


def _mtime_offsets(raw, addr):
    """File offsets of the 4-byte modification-time fields of the object header at `addr` (HDF5 file format, IV.A.1 / IV.A.2.r):
    version 1 headers carry a Modification Time message (type 0x12: version, 3 reserved bytes, seconds), found by walking the header's
    messages through its continuation blocks; version 2 headers ("OHDR") carry four times in their prefix when flag bit 5 is set."""
    if raw[addr:addr + 4] == b"OHDR":
        return [addr + 6 + 4 * k for k in range(4)] if raw[addr + 5] & 0x20 else []
    version, _, nmsgs, _, size = struct.unpack_from("<BBHII", raw, addr)
    assert version == 1, f"object header version {version} at {addr}"
    chunks, found, seen = [(addr + 16, size)], [], 0
    while chunks and seen < nmsgs:
        pos, left = chunks.pop(0)
        end = pos + left
        while pos + 8 <= end and seen < nmsgs:
            mtype, msize = struct.unpack_from("<HH", raw, pos)
            data = pos + 8
            if mtype == 0x12:
                assert raw[data] == 1, "modification time message version"
                found.append(data + 4)
            elif mtype == 0x10:                         # continuation: offset, length (8-byte offsets and lengths, h5py's default)
                chunks.append(struct.unpack_from("<QQ", raw, data))
            pos, seen = data + msize, seen + 1
    return found


def same_file(a, b):
    """Two HDF5 files, byte for byte.  HDF5 stamps every dataset's object header with its modification time in seconds (h5py's default,
    which the writer keeps as the reference does), so files written in different seconds differ in those 4-byte fields.  Exactly those
    fields are set aside: their offsets are read from the object headers of every object of both files, must be the same in both, and
    every dataset must have exactly one; every other byte must be equal."""
    import h5py
    A, B = open(a, "rb").read(), open(b, "rb").read()
    if len(A) != len(B):
        return False
    stamps = []
    for path, raw in ((a, A), (b, B)):
        offs = {}
        with h5py.File(path, "r") as f:
            def visit(name, obj):
                o = _mtime_offsets(raw, h5py.h5o.get_info(obj.id).addr)
                if isinstance(obj, h5py.Dataset) and len(o) != 1:
                    raise AssertionError(f"{path}: dataset {name} has {len(o)} modification times")
                offs[name] = o
            f.visititems(visit)
        stamps.append(offs)
    if stamps[0] != stamps[1] or not any(stamps[0].values()):
        return False
    x, y = np.frombuffer(A, np.uint8).copy(), np.frombuffer(B, np.uint8).copy()
    for offs in stamps[0].values():
        for o in offs:
            x[o:o + 4] = 0
            y[o:o + 4] = 0
    return bool(np.array_equal(x, y))
