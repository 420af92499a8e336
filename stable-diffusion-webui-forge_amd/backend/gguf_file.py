"""Reader for GGUF checkpoint files (host only, no third-party package), written from the public format description
(ggml `docs/gguf.md`): counterpart of the `gguf.GGUFReader` the reference vendors under packages_3rdparty/gguf and uses in
backend/utils.py:27-31.

Layout (little endian): magic "GGUF", uint32 version (2 or 3), uint64 tensor count, uint64 key-value count, the typed key-value
section, the tensor infos (name, n_dims, dims -- fastest axis first --, GGML type, offset into the data section), padding to
`general.alignment` (default 32), the data section.  The file is memory-mapped; a tensor is a `GGUFTensor(name, qtype, shape,
data)` whose `shape` is the REVERSED dims (row-major, what `ParameterGGUF.real_shape` of the reference gives) and whose `data`
is a zero-copy uint8 view of its packed bytes.  Every extent is checked against the size of the mapping before a view is made:
malformed input raises ValueError, it never indexes out of the file.
"""
import mmap
import struct
from collections import namedtuple

import numpy as np

GGUF_MAGIC = b"GGUF"
VERSIONS = (2, 3)
DEFAULT_ALIGNMENT = 32

# GGML type number -> (name, weights per block, bytes per block): facts of the format.  Types the device kernels expand (hipops.gguf_dequant)
# are in DEQUANT_TYPES; the others are listed so that a file holding them is still readable and the error names the type.
GGML_TYPES = {
    0: ("F32", 1, 4), 1: ("F16", 1, 2), 2: ("Q4_0", 32, 18), 3: ("Q4_1", 32, 20), 6: ("Q5_0", 32, 22), 7: ("Q5_1", 32, 24),
    8: ("Q8_0", 32, 34), 9: ("Q8_1", 32, 36), 10: ("Q2_K", 256, 84), 11: ("Q3_K", 256, 110), 12: ("Q4_K", 256, 144),
    13: ("Q5_K", 256, 176), 14: ("Q6_K", 256, 210), 15: ("Q8_K", 256, 292), 16: ("IQ2_XXS", 256, 66), 17: ("IQ2_XS", 256, 74),
    18: ("IQ3_XXS", 256, 98), 19: ("IQ1_S", 256, 50), 20: ("IQ4_NL", 32, 18), 21: ("IQ3_S", 256, 110), 22: ("IQ2_S", 256, 82),
    23: ("IQ4_XS", 256, 136), 24: ("I8", 1, 1), 25: ("I16", 1, 2), 26: ("I32", 1, 4), 27: ("I64", 1, 8), 28: ("F64", 1, 8),
    29: ("IQ1_M", 256, 56), 30: ("BF16", 1, 2),
}
DEQUANT_TYPES = (0, 1, 2, 3, 6, 7, 8, 10, 11, 12, 13, 14, 30)
QTYPE = {name: num for num, (name, _, _) in GGML_TYPES.items()}

# metadata value types: number -> struct format of a scalar; 8 = string, 9 = array
_SCALARS = {0: "<B", 1: "<b", 2: "<H", 3: "<h", 4: "<I", 5: "<i", 6: "<f", 7: "<?", 10: "<Q", 11: "<q", 12: "<d"}
_STRING, _ARRAY = 8, 9
MAX_DIMS = 4


class GGUFTensor(namedtuple("GGUFTensor", "name qtype shape data")):
    """One tensor of a GGUF file: `qtype` the GGML type number, `shape` row-major (reversed `ne`), `data` the packed bytes (uint8, zero copy)."""
    __slots__ = ()

    @property
    def type_name(self):
        return GGML_TYPES[self.qtype][0]

    @property
    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def dim(self):
        return len(self.shape)

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]


class _Cursor:
    """bounds-checked sequential reader over the mapping"""

    def __init__(self, buf, what):
        self.buf, self.pos, self.end, self.what = buf, 0, len(buf), what

    def take(self, n, ctx):
        if n < 0 or self.pos + n > self.end:
            raise ValueError(f"{self.what}: truncated while reading {ctx} (need {n} bytes at offset {self.pos}, file has {self.end})")
        p = self.pos
        self.pos += n
        return p

    def scalar(self, fmt, ctx):
        p = self.take(struct.calcsize(fmt), ctx)
        return struct.unpack_from(fmt, self.buf, p)[0]

    def string(self, ctx):
        n = self.scalar("<Q", ctx + " length")
        p = self.take(n, ctx)
        return bytes(self.buf[p:p + n]).decode("utf-8", errors="replace")

    def value(self, vtype, ctx, depth=0):
        if vtype in _SCALARS:
            return self.scalar(_SCALARS[vtype], ctx)
        if vtype == _STRING:
            return self.string(ctx)
        if vtype == _ARRAY:
            if depth > 4:
                raise ValueError(f"{self.what}: {ctx}: arrays nested too deeply")
            etype = self.scalar("<I", ctx + " element type")
            n = self.scalar("<Q", ctx + " length")
            if etype in _SCALARS:   # one bounds check and one unpack for the whole array (token tables hold 10^5 entries)
                fmt = _SCALARS[etype]
                size = struct.calcsize(fmt)
                if n > (self.end - self.pos) // size:
                    raise ValueError(f"{self.what}: {ctx}: array of {n} elements runs past the end of the file")
                p = self.take(n * size, ctx)
                return list(struct.unpack_from("<%d%s" % (n, fmt[1]), self.buf, p))
            if n > self.end - self.pos:
                raise ValueError(f"{self.what}: {ctx}: array of {n} elements runs past the end of the file")
            return [self.value(etype, ctx, depth + 1) for _ in range(n)]
        raise ValueError(f"{self.what}: {ctx}: unknown metadata value type {vtype}")


class GGUFFile:
    """`metadata`: {key: value}; `tensors`: {name: GGUFTensor} in file order; `architecture`: metadata['general.architecture'] or None."""

    def __init__(self, path):
        self.path = str(path)
        with open(self.path, "rb") as f:
            size = f.seek(0, 2)
            if size < 24:
                raise ValueError(f"{self.path}: truncated GGUF header ({size} bytes)")
            self._map = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        buf = memoryview(self._map)
        cur = _Cursor(buf, self.path)
        magic = bytes(buf[cur.take(4, "magic"):4])
        if magic != GGUF_MAGIC:
            raise ValueError(f"{self.path}: not a GGUF file (magic {magic!r})")
        self.version = cur.scalar("<I", "version")
        if self.version not in VERSIONS:
            raise ValueError(f"{self.path}: GGUF version {self.version} is not supported (known: {VERSIONS})")
        n_tensors = cur.scalar("<Q", "tensor count")
        n_kv = cur.scalar("<Q", "key-value count")
        self.metadata = {}
        for _ in range(n_kv):
            key = cur.string("metadata key")
            vtype = cur.scalar("<I", f"type of metadata key {key!r}")
            self.metadata[key] = cur.value(vtype, f"metadata key {key!r}")
        self.alignment = self.metadata.get("general.alignment", DEFAULT_ALIGNMENT)
        if not isinstance(self.alignment, int) or self.alignment <= 0 or self.alignment & (self.alignment - 1):
            raise ValueError(f"{self.path}: general.alignment {self.alignment!r} is not a power of two")
        infos = []
        for i in range(n_tensors):
            name = cur.string(f"name of tensor #{i}")
            n_dims = cur.scalar("<I", f"n_dims of tensor {name!r}")
            if n_dims > MAX_DIMS:
                raise ValueError(f"{self.path}: tensor {name!r} has {n_dims} dimensions (at most {MAX_DIMS})")
            ne = [cur.scalar("<Q", f"dims of tensor {name!r}") for _ in range(n_dims)]
            qtype = cur.scalar("<I", f"type of tensor {name!r}")
            offset = cur.scalar("<Q", f"offset of tensor {name!r}")
            infos.append((name, ne, qtype, offset))
        self.data_offset = (cur.pos + self.alignment - 1) // self.alignment * self.alignment
        whole = np.frombuffer(buf, dtype=np.uint8)
        self.tensors = {}
        self.offsets = {}
        for name, ne, qtype, offset in infos:
            if qtype not in GGML_TYPES:
                raise ValueError(f"{self.path}: tensor {name!r} has unknown GGML type {qtype}")
            tname, bw, bb = GGML_TYPES[qtype]
            row = ne[0] if ne else 1
            if row % bw:
                raise ValueError(f"{self.path}: tensor {name!r}: row length {row} is not a multiple of the {tname} block size {bw}")
            numel = 1
            for d in ne:
                numel *= d
            nbytes = numel // bw * bb
            start = self.data_offset + offset
            if offset % self.alignment:
                raise ValueError(f"{self.path}: tensor {name!r}: offset {offset} is not aligned to {self.alignment}")
            if start > size or nbytes > size - start:
                raise ValueError(f"{self.path}: tensor {name!r} ({nbytes} bytes at offset {start}) runs past the end of the file ({size} bytes)")
            if name in self.tensors:
                raise ValueError(f"{self.path}: tensor {name!r} appears twice")
            self.tensors[name] = GGUFTensor(name, qtype, tuple(int(d) for d in reversed(ne)), whole[start:start + nbytes])
            self.offsets[name] = offset

    @property
    def architecture(self):
        return self.metadata.get("general.architecture")


def load_gguf(path):
    """-> {name: GGUFTensor} (what loader.load_torch_file returns for a .gguf path); the mapping stays alive as long as any view does."""
    return dict(GGUFFile(path).tensors)
