"""Minimal GGUF (version 3) writer for tools and tests: synthetic checkpoints for tools/bench_gguf.py and the quantised twins of the tiny
models in tests/test_gpu_gguf.py.  Not part of the package (the package only reads GGUF), written from the public format description.

    write_gguf(path, [(name, qtype, shape, raw_bytes), ...], {"general.architecture": "flux", ...})

`shape` is row-major (the fastest axis LAST, as torch has it); the file stores it reversed.  `raw_bytes` is a uint8 array holding the packed
blocks.  Metadata values: str, bool, int (stored as uint32, or int64 when negative / large), float (float32), or a list of one of those.
"""
import struct

import numpy as np

ALIGNMENT = 32
_U32, _F32, _BOOL, _STR, _ARR, _I64 = 4, 6, 7, 8, 9, 11


def _string(s):
    b = s.encode("utf-8")
    return struct.pack("<Q", len(b)) + b


def _scalar_type(v):
    if isinstance(v, bool):
        return _BOOL
    if isinstance(v, int):
        return _U32 if 0 <= v < 2 ** 32 else _I64
    if isinstance(v, float):
        return _F32
    if isinstance(v, str):
        return _STR
    raise TypeError(f"metadata value {v!r}")


def _scalar(v, t):
    return {_BOOL: lambda: struct.pack("<?", v), _U32: lambda: struct.pack("<I", v), _I64: lambda: struct.pack("<q", v),
            _F32: lambda: struct.pack("<f", v), _STR: lambda: _string(v)}[t]()


def _value(v):
    if isinstance(v, (list, tuple)):
        t = _scalar_type(v[0]) if v else _U32
        return struct.pack("<I", _ARR) + struct.pack("<IQ", t, len(v)) + b"".join(_scalar(x, t) for x in v)
    t = _scalar_type(v)
    return struct.pack("<I", t) + _scalar(v, t)


def write_gguf(path, tensors, metadata=None, chunk=1 << 26):
    metadata = dict(metadata or {})
    head = b"GGUF" + struct.pack("<IQQ", 3, len(tensors), len(metadata))
    for k, v in metadata.items():
        head += _string(k) + _value(v)
    offset = 0
    for name, qtype, shape, raw in tensors:
        head += _string(name) + struct.pack("<I", len(shape)) + b"".join(struct.pack("<Q", int(d)) for d in reversed(shape))
        head += struct.pack("<IQ", int(qtype), offset)
        offset += (int(raw.nbytes) + ALIGNMENT - 1) // ALIGNMENT * ALIGNMENT
    with open(path, "wb") as f:
        f.write(head)
        f.write(b"\0" * (-len(head) % ALIGNMENT))
        for _, _, _, raw in tensors:
            flat = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
            for i in range(0, flat.size, chunk):
                f.write(flat[i:i + chunk].tobytes())
            f.write(b"\0" * (-flat.size % ALIGNMENT))
    return path
