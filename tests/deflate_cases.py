"""The deflate corpus that the CPU program (tests/csrc/verify_deflate.cpp) and the device (DenseFlow.deflate) are both held to: seeded
inputs, the smallest at which each part of the compressor can go wrong.  The yardstick is zlib.compress(raw, 9), byte for byte; its
length and SHA-256 per case are recorded in tests/golden/deflate_digests.json (made with zlib 1.2.11 by
tests/golden/make_deflate_digests.py), so that a machine whose zlib writes other bytes fails the digest test and not the kernel's.

cases() -> [Case(name, raw)], built once.  The families of tests/inflate_cases.py at every size of SIZES, and further ones:
  random (of inflate_cases)   stored blocks, before and after a window slide
  tiny                        inputs under 100 B: fixed blocks
  seven                       seven byte values: hash chains thousands long
  counter                     16-bit counters, next to no three bytes repeat, so nearly every byte is a literal: 16,396 (16,382 symbols),
                              16,397 (one block of exactly 16,383), 16,398 and 16,399 (a full block and a last one of one and two
                              symbols), 40,000 (two full blocks and a third)
  far3-D                      a three-byte match D = 4,096 and 4,097 back in such data (beyond 4,096 zlib drops it)
  chain-K-short / -long       one prefix 4,300 times; the one long match is chain candidate K (counted from 0) of the probe, K around
                              the two chain limits: 1022..1025 and 4094..4097; the probe follows a literal (short: 4,096 candidates
                              are tried) or a match of 35 bytes (long: 1,024)
  dist-D                      a 24-byte match D = 32,505, 32,506 and 32,507 back (the head of a chain is admitted up to 32,506)
  slide0-N-P                  a 24-byte match from P = 32,768 k + 32,506 back to 32,768 k, the chain's head at exactly 32,506, in an input
                              of N bytes.  Where N ends within 262 bytes behind P, zlib slides its window at P itself, although no
                              input is left: the head becomes position 0 of the window, which is "none", and the match is not found
                              (65,400, 65,300, 98,200, 130,900); where the input goes on, it slides later and finds it (65,540, 98,400)
  fibdist, fibdist-bl         six-byte matches at chosen distances, so that one block's distance codes have frequencies in Fibonacci
                              proportion: in `fibdist` (17 codes, ratio 1.65) the distance tree's unbounded depth is 16, past its
                              limit of 15, and is repaired; in `fibdist-bl` (16 codes) the code-length tree's passes 7 (the corpus'
                              test computes both depths from the decoded frequencies).
  lloverflow-16, -17          the same for the literal/length tree, so that the repair, one routine, is run for all three trees.
                              32,766 random bytes (two full blocks of literals end where they end), then a last block of matches
                              alone: pieces copied from 300 to 30,000 back whose lengths are the first of length codes 258, 259, ..
                              (4, 5, .. 51; not 3, which zlib drops when it lies more than 4,096 back), code i of 17 or 18 taken
                              round(1.65 ** (codes - 1 - i)) times, shuffled.  A source is drawn again while the piece before it,
                              with the source's first byte, occurs in the window: that match would grow by a byte and leave a rest
                              of literals, which flatten the tree.  The block's unbounded depth is 16 and 17, its deepest code 15.
  collide-N                   bytes (r << 5) | s, r uniform in 0..7 and s one of 2 (N = 4,099) or 3 (73,728) values: hash3 drops the
                              first byte's top three bits, so every three-byte string shares its hash with seven others, matches
                              abound, and the 64 positions that the device links in one step hold different strings of one hash
  prefix-slide-N              16,000 random bytes, then a mask to N bytes: the second block begins below 32,768 and is flushed behind
                              the window's slide, when zlib holds no pointer to its first byte any more and cannot store it.  (Its
                              stored form cannot also be the shortest: a block of at most 16,383 symbols over more than 32,507 bytes
                              has matches for more than half of them.  The stored blocks of `random` begin behind the slide.)

sweep(size) -> 1,500 seeded chunks of one size, drawn in turn from seven families (SWEEP_FAMILIES): the randomized comparison with
zlib, at 61, 512 and 4,000 bytes (SWEEP_SIZES).  Their yardstick is one SHA-256 per size over zlib's streams end to end, under
"sweeps" in the digests' file; first_difference() names the chunk where a compressor leaves zlib.
"""
import functools
import hashlib
import json
import os
import zlib
from collections import namedtuple

import numpy as np

from tests.inflate_cases import FAMILIES, data

Case = namedtuple("Case", "name raw")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGESTS = os.path.join(ROOT, "tests", "golden", "deflate_digests.json")

SIZES = [0, 1, 2, 3, 4, 257, 258, 259, 32505, 32506, 32507, 32767, 32768, 32769, 65273, 65274, 65275, 65400, 65539, 73728, 75000, 81600,
         98041, 98042, 98043, 98200, 140000]           # (65,400 and 98,200: the input ends within 262 bytes behind a slide's position)
SLIDE0 = [(65400, 65274), (65300, 65274), (98200, 98042), (130900, 130810), (65540, 65274), (98400, 98042)]
SLIDE_SIZES = [65273, 65274, 65275, 73728, 98042, 140000]
CHAIN_AT = [1022, 1023, 1024, 1025, 4094, 4095, 4096, 4097]


def _rng(*key):
    return np.random.default_rng([9, *key])


def _random(n, *key):
    return _rng(*key).integers(0, 256, n, dtype=np.uint8).tobytes()


def _counter(n):
    return np.arange(n // 2 + 1, dtype="<u2").tobytes()[:n]


def _far3(d):
    raw = bytearray(_counter(12000))
    raw[100:103] = b"\xF0\xF1\xF2"
    raw[100 + d:103 + d] = b"\xF0\xF1\xF2"
    raw[103], raw[103 + d] = 1, 2
    return bytes(raw)


def _chain(k, long_prev):
    """... Z? + ABC + L as the probe at the end; before it 4,300 records ABC + a counter, and the one ABC + L among them with k records
    between it and the probe"""
    L = _random(60, 5)
    rec = [b"ABC" + bytes([0x80 | (i & 0x3F), 0xC0 | (i >> 6)]) for i in range(4300)]
    rec.insert(4300 - k, b"ABC" + L + b"\x7F")
    head = b"ZABC" + L[:31] + b"\x7E" if long_prev else b""
    return head + b"".join(rec) + (b"Z" if long_prev else b"\x7D") + b"ABC" + L + b"\x7C\x7B"


def _dist(d):
    raw = bytearray(_counter(40000))
    token = bytes(range(200, 224))
    raw[100:124] = token
    raw[100 + d:124 + d] = token
    return bytes(raw)


def _slide0(n, p):
    """random bytes below 31, whose hash of three is the three bytes themselves, and a token that begins 31 31 30 at P - 32,506 and at
    P: no other position has the token's hash, so the earlier token is the head of the later one's chain"""
    rng = _rng(17, n)
    raw = bytearray(rng.integers(0, 31, n, dtype=np.uint8).tobytes())
    token = bytes([31, 31, 30]) + rng.integers(0, 31, 21, dtype=np.uint8).tobytes()
    raw[p - 32506:p - 32506 + 24] = token
    raw[p:p + 24] = token
    return bytes(raw)


@functools.lru_cache(maxsize=None)
def _fibdist(n_codes, first, ratio):
    """32 KiB of random bytes, then pieces of six bytes copied from P back and one byte that differs from the one P back; P is the
    second distance of distance code first + i, taken round(ratio ** i) times (ratio None: the Fibonacci numbers), in shuffled order"""
    rng = _rng(11)
    out = bytearray(rng.integers(0, 256, 32768, dtype=np.uint8).tobytes())
    a, b, counts = 1, 1, []
    for i in range(n_codes):
        counts.append(a if ratio is None else int(round(ratio ** i)))
        a, b = b, a + b
    pieces = np.repeat(np.arange(first, first + n_codes), counts)
    pieces = pieces[rng.permutation(len(pieces))]
    for c, v in zip(pieces, rng.integers(0, 256, len(pieces))):
        c, v = int(c), int(v)
        p = 2 + ((2 + (c & 1)) << ((c >> 1) - 1))
        for _ in range(6):
            out.append(out[-p])
        out.append((v + 1) & 255 if v == out[-p] else v)
    return bytes(out)


LENGTH_FIRST = [4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51]      # the first length of length codes 258, 259, ..


@functools.lru_cache(maxsize=None)
def _lloverflow(n_codes, ratio):
    """32,766 random bytes, then pieces of LENGTH_FIRST[i] bytes, i < n_codes, copied from 300 + the length to 30,000 back; length i
    is taken round(ratio ** (n_codes - 1 - i)) times, in shuffled order.  No piece lets the match before it grow: a source whose first
    byte, behind the piece before, makes a string the window holds is drawn again."""
    rng = _rng(19, n_codes)
    out = bytearray(rng.integers(0, 256, 32766, dtype=np.uint8).tobytes())
    counts = [int(round(ratio ** (n_codes - 1 - i))) for i in range(n_codes)]
    pieces = np.repeat(np.array(LENGTH_FIRST[:n_codes]), counts)
    pieces = pieces[rng.permutation(len(pieces))]
    prev = None
    for n in pieces.tolist():
        while True:
            src = len(out) - int(rng.integers(n + 300, 30000))
            if prev is None or out.find(prev + out[src:src + 1], len(out) - 32768) < 0:
                break
        prev = bytes(out[src:src + n])
        out += prev
    return bytes(out)


COLLIDE = {4099: 2, 73728: 3}                           # size: how many values the low five bits take


def _collide(rng, n, k):
    low = rng.choice(32, k, replace=False)
    return ((rng.integers(0, 8, n) << 5) | low[rng.integers(0, k, n)]).astype(np.uint8).tobytes()


def hash3(b, p=0):
    """zlib's hash of the three bytes at p, as csrc/teeflow_deflate_core.h has it"""
    return ((b[p] << 10) ^ (b[p + 1] << 5) ^ b[p + 2]) & 32767


def colliding_steps(raw):
    """how many of the 64-position steps of k_deflate_links hold two different three-byte strings of one hash"""
    found = 0
    for base in range(0, len(raw) - 2, 64):
        seen, hit = {}, False
        for p in range(base, min(base + 64, len(raw) - 2)):
            hit = hit or seen.setdefault(hash3(raw, p), raw[p:p + 3]) != raw[p:p + 3]
        found += hit
    return found


def _prefix_slide(n):
    return _random(16000, 13) + FAMILIES["mask"](_rng(13, n), n - 16000)


# ---- the sweep: many small seeded inputs, where a byte can differ silently (the run-length corners of the trees' own coding, ties
# between a stored, a fixed and a dynamic block, the lazy parse on short inputs)
SWEEP_SIZES, SWEEP_COUNT = [61, 512, 4000], 1500


def _sw_geometric(rng, n):
    k = int(rng.integers(2, 41))
    return rng.permutation(256)[np.minimum(rng.geometric(rng.uniform(0.05, 0.7), n) - 1, k - 1)]


def _sw_runs(rng, n):
    values = rng.integers(0, 256, int(rng.integers(1, 9)))
    runs = rng.geometric(1.0 / rng.uniform(1.5, 150.0), n)
    return np.repeat(values[rng.integers(0, len(values), n)], runs)[:n]


def _sw_uniform(rng, n):
    return rng.permutation(256)[rng.integers(0, int(rng.integers(1, 257)), n)]


def _sw_f16(rng, n):
    v = (rng.standard_normal(n // 2 + 1) * 10.0 ** rng.uniform(-3, 3)).astype(np.float16)
    return np.frombuffer(v.tobytes(), np.uint8)[:n]


def _sw_mask(rng, n):
    runs = rng.geometric(1.0 / rng.uniform(2.0, 400.0), n)
    return np.repeat((np.arange(n) + int(rng.integers(0, 2))) & 1, runs)[:n]


def _sw_collide(rng, n):
    return np.frombuffer(_collide(rng, n, int(rng.integers(2, 4))), np.uint8)


def _sw_phrases(rng, n):
    words = [rng.integers(0, 256, int(rng.integers(3, 21))) for _ in range(int(rng.integers(2, 17)))]
    return np.concatenate([words[i] for i in rng.integers(0, len(words), n // 3 + 1)])[:n]


SWEEP_FAMILIES = [_sw_geometric, _sw_runs, _sw_uniform, _sw_f16, _sw_mask, _sw_collide, _sw_phrases]


@functools.lru_cache(maxsize=None)
def sweep(size, count=SWEEP_COUNT):
    """`count` chunks of `size` bytes: chunk i is of family i % 7, seeded by the size and i alone"""
    out = []
    for i in range(count):
        raw = np.asarray(SWEEP_FAMILIES[i % len(SWEEP_FAMILIES)](_rng(31, size, i), size)).astype(np.uint8).tobytes()
        assert len(raw) == size
        out.append(raw)
    return tuple(out)


def sweep_digest(streams):
    """[length, sha256] of a sweep's streams end to end"""
    return digest(b"".join(streams))


def first_difference(chunks, streams):
    """of the first chunk whose stream is not the running zlib's: (index, its family, the stream's length, zlib's length), or None"""
    for i, (c, s) in enumerate(zip(chunks, streams)):
        z = zlib.compress(c, 9)
        if bytes(s) != z:
            return i, SWEEP_FAMILIES[i % len(SWEEP_FAMILIES)].__name__, len(s), len(z)
    return None


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for fam in FAMILIES:
        for n in SIZES:
            out.append(Case(f"{fam}-{n}", data(fam, n)))
    text = b"the quick brown fox jumps over the lazy dog; the quick brown fox jumps over the lazy dog again and again, lazily"
    for n in (5, 19, 64, 99):
        out.append(Case(f"tiny-{n}", text[:n]))
    for n in (73728, 140000):
        out.append(Case(f"seven-{n}", _rng(1, n).integers(0, 7, n, dtype=np.uint8).tobytes()))
    for n in (16396, 16397, 16398, 16399, 40000):
        out.append(Case(f"counter-{n}", _counter(n)))
    for n in SLIDE_SIZES:
        out.append(Case(f"prefix-slide-{n}", _prefix_slide(n)))
    for d in (4096, 4097):
        out.append(Case(f"far3-{d}", _far3(d)))
    for k in CHAIN_AT:
        out.append(Case(f"chain-{k}-short", _chain(k, False)))
        out.append(Case(f"chain-{k}-long", _chain(k, True)))
    for d in (32505, 32506, 32507):
        out.append(Case(f"dist-{d}", _dist(d)))
    for n, p in SLIDE0:
        out.append(Case(f"slide0-{n}-{p}", _slide0(n, p)))
    out += deep()
    for n, k in COLLIDE.items():
        out.append(Case(f"collide-{n}", _collide(_rng(23, n), n, k)))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def deep():
    """the cases whose trees pass their depth limit: zlib's streams of them hold codes of 15 bits, the inflate corpus takes them too"""
    return [Case("fibdist", _fibdist(17, 13, 1.65)), Case("fibdist-bl", _fibdist(16, 14, None)),
            Case("lloverflow-16", _lloverflow(17, 1.65)), Case("lloverflow-17", _lloverflow(18, 1.65))]


def digest(stream):
    return [len(stream), hashlib.sha256(stream).hexdigest()]


@functools.lru_cache(maxsize=None)
def digests():
    """{name: [length, sha256]} of zlib 1.2.11's level-9 stream of every case, as recorded"""
    with open(DIGESTS) as f:
        return json.load(f)["cases"]


@functools.lru_cache(maxsize=None)
def sweep_digests():
    """{size: [length, sha256]} of zlib 1.2.11's level-9 streams of sweep(size), end to end, as recorded"""
    with open(DIGESTS) as f:
        return {int(k): v for k, v in json.load(f)["sweeps"].items()}


def huffman_depth(freqs):
    """the depth of the Huffman tree of the non-zero frequencies, not limited to any code length; of two nodes of one weight the
    shallower is merged first, as zlib does it"""
    import heapq
    h = [(f, 0) for f in freqs if f]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1] if h else 0


def blocks(stream):
    """[(type, symbols, bytes, lf, df, cf, depths)] of a zlib stream's blocks: 0 stored (symbols: its bytes), 1 fixed, 2 dynamic (symbols
    without the end-of-block; bytes: what they decode to; lf, df, cf: how often each literal/length, distance and code-length symbol
    occurs; None for a stored block, cf None for a fixed one; depths: the block's longest literal/length and distance code, None for
    a stored block), and the deepest literal/length, code-length and distance code of its dynamic blocks.  A plain decoder after
    RFC 1951, for the corpus' own test."""
    bits, at, out, deep = int.from_bytes(stream, "little") >> 16, 0, [], [0, 0, 0]

    def take(n):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += n
        return v

    def table(lens):
        code, t, count = 0, {}, [0] * 17
        for l in lens:
            count[l] += 1
        count[0], nxt = 0, [0] * 17
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        for s, l in enumerate(lens):
            if l:
                t[(l, nxt[l])] = s
                nxt[l] += 1
        return t

    def sym(t):
        code = 0
        for l in range(1, 16):
            code = code << 1 | take(1)
            if (l, code) in t:
                return t[(l, code)]
        raise ValueError("no such code")

    fixed = (table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 30))
    while True:
        last, kind = take(1), take(2)
        if kind == 0:
            at = (at + 7) & ~7
            n = take(16)
            take(16)
            at += 8 * n
            out.append((0, n, n, None, None, None, None))
        else:
            cf, depths = None, (9, 5)
            if kind == 1:
                lt, dt = fixed
            else:
                nl, nd, nc = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for i in range(nc):
                    cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = take(3)
                ct, lens, cf = table(cl), [], [0] * 19
                while len(lens) < nl + nd:
                    s = sym(ct)
                    cf[s] += 1
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + take(2))
                    else:
                        lens += [0] * (3 + take(3) if s == 17 else 11 + take(7))
                lt, dt = table(lens[:nl]), table(lens[nl:])
                depths = (max(lens[:nl]), max(lens[nl:]))
                deep = [max(deep[0], depths[0]), max(deep[1], max(cl)), max(deep[2], depths[1])]
            n = made = 0
            lf, df = [0] * 286, [0] * 30
            lf[256] = 1
            while True:
                s = sym(lt)
                if s == 256:
                    break
                lf[s] += 1
                n += 1
                made += 1
                if s > 256:
                    s -= 257
                    x = 0 if s < 8 or s == 28 else (s - 4) >> 2
                    made += (2 + s if s < 8 else 257 if s == 28 else 2 + ((4 + (s & 3)) << x)) + take(x)
                    d = sym(dt)
                    df[d] += 1
                    take(0 if d < 4 else (d >> 1) - 1)
            out.append((kind, n, made, lf, df, cf, depths))
        if last:
            return out, deep
