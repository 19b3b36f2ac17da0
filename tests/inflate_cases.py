"""The inflate corpus that the CPU program (tests/csrc/verify_inflate.cpp) and the device kernel (DenseFlow.inflate) are both held to:
zlib streams made with the standard library's zlib alone, from seeded data, and malformed ones.  What is expected of a stream is what
zlib.decompressobj().decompress does with it here, never an assumption: see verdict().

cases() -> [Case(name, stream, out_bytes)], built once; among the good ones zlib's level-9 streams of the deflate corpus' cases whose
trees pass their depth limit (tests/deflate_cases.deep), the only ones with codes of 14 and 15 bits.  verdict(case) -> (kind, out):
  GOOD   zlib decodes the stream to its end and gives out_bytes bytes: the status must be 0 and the output those bytes
  BAD    zlib raises: the status must not be 0; `out` is what zlib had decoded before it raised (the stream fed byte by byte), and
         what the decoder wrote into its slot must be a prefix of that
  SHORT  zlib raises nothing, but the stream ends before its trailer does or its output is not out_bytes long: the status must not
         be 0 (the stream is not a whole one of that size), and where zlib's partial output is out_bytes long the output is those bytes
"""
import functools
import itertools
import os
import struct
import zlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name stream out_bytes")
GOOD, BAD, SHORT = 0, 1, 2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY_H5 = "/opt/conda/bin/python3.9"       # the interpreter that has h5py (tests/test_study_driver_cpu.py)

SIZES = [0, 1, 2, 257, 258, 259, 32767, 32768, 32769, 65536 + 3, 73728]
LEVELS = [0, 1, 6, 9]
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE, "fixed": zlib.Z_FIXED}
MEMLEVELS = [1, 8]
WBITS = [9, 15]


def _smooth_f16(rng, n):
    v = np.convolve(rng.standard_normal(n // 2 + 16), np.ones(9) / 9.0, mode="same") * 3.0
    return v.astype(np.float16).tobytes()[:n]


def _mask(rng, n):
    side = int(np.ceil(np.sqrt(max(n, 1))))
    f = rng.standard_normal((side + 8, side + 8))
    k = np.ones(9) / 9.0
    f = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 0, f)
    f = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, f)
    return (f[:side, :side] > 0).astype(np.uint8).tobytes()[:n]


def _period(rng, n, p):
    unit = rng.integers(0, 256, p, dtype=np.uint8)
    return np.tile(unit, n // p + 1)[:n].tobytes()


FAMILIES = {
    "zeros": lambda rng, n: bytes(n),
    "byte": lambda rng, n: bytes([0xA7]) * n,
    "period2": lambda rng, n: _period(rng, n, 2),               # distance 1 and 2
    "period32768": lambda rng, n: _period(rng, n, 32768),       # the largest distance
    "random": lambda rng, n: rng.integers(0, 256, n, dtype=np.uint8).tobytes(),      # stored or near-stored
    "f16noise": _smooth_f16,                                    # what a study's flow looks like
    "mask": _mask,
}


def data(family, n):
    """the seeded bytes of a family at a size"""
    return FAMILIES[family](np.random.default_rng([sorted(FAMILIES).index(family), n]), n)


def deflate(raw, level=6, strategy="default", mem=8, wbits=15, flushes=()):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, STRATEGIES[strategy])
    out, at = [], 0
    for pos, mode in flushes:
        out.append(c.compress(raw[at:pos]))
        out.append(c.flush(mode))
        at = pos
    out.append(c.compress(raw[at:]))
    out.append(c.flush())
    return b"".join(out)


class _BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        """n bits of v, the lowest first"""
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        """a Huffman code of n bits, the highest first"""
        for i in range(n - 1, -1, -1):
            self.bits((v >> i) & 1, 1)

    def done(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


def _header(cmf=0x78, fdict=False):
    flg = 0x20 if fdict else 0
    flg += 31 - (cmf * 256 + flg) % 31
    return bytes([cmf, flg])


def _malformed():
    out = []
    small = [(deflate(b"the quick brown fox", 6, "fixed"), 19, "fixed"),
             (deflate(bytes(np.random.default_rng(77).integers(97, 105, 400, dtype=np.uint8)), 9), 400, "dynamic")]
    for stream, n, kind in small:
        for k in range(len(stream)):
            out.append(Case(f"prefix-{kind}-{k}", stream[:k], n))
    good = deflate(data("f16noise", 259), 9)
    for bit in range(16):
        s = bytearray(good)
        s[bit // 8] ^= 1 << (bit % 8)
        out.append(Case(f"header-bit-{bit}", bytes(s), 259))
    for k in range(1, 5):
        for delta in (1, 0x80):
            s = bytearray(good)
            s[-k] = (s[-k] + delta) & 255
            out.append(Case(f"trailer-byte-{k}-{delta}", bytes(s), 259))
    w = _BitWriter()
    w.bits(1, 1); w.bits(3, 2)
    out.append(Case("block-type-3", _header() + w.done() + bytes(8), 4))
    out.append(Case("stored-len-nlen", _header() + bytes([1, 5, 0, 0xFA, 0xFE]) + b"hello" + struct.pack(">I", zlib.adler32(b"hello")), 5))
    w = _BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    w.code(1, 7)          # length symbol 257: 3 bytes
    w.code(0, 5)          # distance symbol 0: 1 back, before anything was written
    w.code(0, 7)          # end of block
    out.append(Case("match-before-start", _header() + w.done() + struct.pack(">I", 1), 3))
    w = _BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    w.code(0x30 + ord("a"), 8)
    w.code(1, 7); w.code(1, 5)     # 3 bytes, 2 back: one byte before the start
    w.code(0, 7)
    out.append(Case("match-one-before-start", _header() + w.done() + struct.pack(">I", 1), 4))
    out.append(Case("fdict", _header(fdict=True) + good[2:], 259))
    out.append(Case("cm-not-8", _header(cmf=0x77) + good[2:], 259))
    body = data("f16noise", 1001)
    out.append(Case("one-byte-longer", deflate(body, 9), 1000))
    out.append(Case("one-byte-shorter", deflate(body[:999], 9), 1000))
    out.append(Case("stored-one-byte-longer", deflate(data("random", 1001), 0), 1000))
    out.append(Case("bytes-after-trailer", good + b"\x00\x01trailing", 259))
    victim = deflate(data("f16noise", 4099), 9)
    rng = np.random.default_rng(4099)
    for k in range(40):
        pos = int(rng.integers(2, len(victim) - 4))
        s = bytearray(victim)
        s[pos] ^= int(rng.integers(1, 256))
        out.append(Case(f"corrupt-{k}-at-{pos}", bytes(s), 4099))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for fam in FAMILIES:
        for n in SIZES:
            raw = data(fam, n)
            for level in (6, 9):
                out.append(Case(f"{fam}-{n}-L{level}", deflate(raw, level), n))
    for fam, n in (("f16noise", 73728), ("mask", 32769)):
        raw = data(fam, n)
        for level in LEVELS:
            for strat in STRATEGIES:
                for mem in MEMLEVELS:
                    for wb in WBITS:
                        out.append(Case(f"{fam}-{n}-L{level}-{strat}-m{mem}-w{wb}", deflate(raw, level, strat, mem, wb), n))
    for fam in ("period2", "period32768", "zeros", "random"):
        raw = data(fam, 65536 + 3)
        for strat, level, mem in (("rle", 6, 8), ("huffman", 6, 8), ("fixed", 9, 1), ("default", 0, 8), ("filtered", 1, 1)):
            out.append(Case(f"{fam}-65539-L{level}-{strat}-m{mem}", deflate(raw, level, strat, mem), len(raw)))
    raw = data("f16noise", 32769)
    out.append(Case("flushes", deflate(raw, 6, flushes=((1000, zlib.Z_SYNC_FLUSH), (1000, zlib.Z_SYNC_FLUSH), (20000, zlib.Z_FULL_FLUSH))), len(raw)))
    out.append(Case("flushes-at-start", deflate(raw[:300], 9, flushes=((0, zlib.Z_SYNC_FLUSH), (0, zlib.Z_FULL_FLUSH))), 300))
    from tests import deflate_cases as DC                 # (it imports this module: hence here)
    for name, raw in DC.deep():                           # codes of 15 bits, literal/length and distance: behind the one-step tables
        out.append(Case(f"{name}-L9", deflate(raw, 9), len(raw)))
    out += _malformed()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def _partial(stream):
    """what zlib decodes of a stream it raises on, before it raises"""
    d, got = zlib.decompressobj(), bytearray()
    try:
        for k in range(len(stream)):
            got += d.decompress(stream[k:k + 1])
    except zlib.error:
        pass
    return bytes(got)


@functools.lru_cache(maxsize=None)
def verdicts():
    """(kind, zlib's output) of every case, in cases()' order"""
    out = []
    for c in cases():
        d = zlib.decompressobj()
        try:
            got = d.decompress(c.stream)
        except zlib.error:
            out.append((BAD, _partial(c.stream)))
            continue
        out.append((GOOD, got) if d.eof and len(got) == c.out_bytes else (SHORT, got))
    return tuple(out)


def verdict(case):
    return verdicts()[cases().index(case)]


def check(case, kind, want, status, got):
    """what a decoder's (status, output bytes of the case's slot) must satisfy; returns the complaint or None"""
    if kind == GOOD:
        if status != 0:
            return f"{case.name}: zlib decodes it, status {status}"
        if bytes(got) != want:
            return f"{case.name}: output differs from zlib's"
    elif status == 0:
        return f"{case.name}: zlib {'raises' if kind == BAD else 'stops short of a whole stream of that size'}, status 0"
    elif kind == SHORT and len(want) == case.out_bytes and bytes(got) != want:
        return f"{case.name}: zlib's partial output has the expected length and differs"
    return None


def written(got, pattern):
    """how far a slot that was pre-filled with `pattern` has been written: everything behind is the pattern still"""
    for p in range(len(got), 0, -1):
        if got[p - 1] != pattern[p - 1]:
            return p
    return 0


def check_prefix(case, kind, want, got, produced):
    """a stream that is not GOOD leaves in its slot a prefix of what zlib decoded of it, `produced` bytes long; the complaint or None"""
    if kind != GOOD and (produced > len(want) or bytes(got[:produced]) != want[:produced]):
        return f"{case.name}: the slot's first {produced} bytes are not what zlib decoded of the stream ({len(want)} bytes)"
    return None


def chunked(arr, chunks, level=9, unfiltered=(), missing=()):
    """(record, expected array): the chunks of arr as a file would hold them (edge chunks whole, zero-padded), as an
    analysis.chunks_record; chunk numbers in `unfiltered` are stored as they are, those in `missing` are not stored: the array is
    expected to be 0 there"""
    from tee_optical_flow_amd import analysis as A
    stored, want = [], arr.copy()
    for i, at in enumerate(itertools.product(*[range(0, s, c) for s, c in zip(arr.shape, chunks)])):
        sl = tuple(slice(o, min(o + c, s)) for o, c, s in zip(at, chunks, arr.shape))
        if i in missing:
            want[sl] = 0
            continue
        full = np.zeros(chunks, arr.dtype)
        full[tuple(slice(0, s.stop - s.start) for s in sl)] = arr[sl]
        raw = full.tobytes()
        stored.append((at, 1, raw) if i in unfiltered else (at, 0, zlib.compress(raw, level)))
    return A.chunks_record(arr.shape, arr.dtype, chunks, stored), want
