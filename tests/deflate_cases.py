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
                              test computes both depths from the decoded frequencies).  The repair is one routine for all three
                              trees; the literal/length tree's own overflow is NOT in the corpus.  A block has at most 16,383
                              symbols; literals that skewed repeat their three-byte strings and turn into matches, and length codes
                              in exact Fibonacci proportion (built like fibdist) share the tree with the literals that separate the
                              matches, which flatten it: every input tried ended at depth 14 or less.
  prefix-slide-N              16,000 random bytes, then a mask to N bytes: the second block begins below 32,768 and is flushed behind
                              the window's slide, when zlib holds no pointer to its first byte any more and cannot store it.  (Its
                              stored form cannot also be the shortest: a block of at most 16,383 symbols over more than 32,507 bytes
                              has matches for more than half of them.  The stored blocks of `random` begin behind the slide.)
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


def _prefix_slide(n):
    return _random(16000, 13) + FAMILIES["mask"](_rng(13, n), n - 16000)


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
    out.append(Case("fibdist", _fibdist(17, 13, 1.65)))
    out.append(Case("fibdist-bl", _fibdist(16, 14, None)))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def digest(stream):
    return [len(stream), hashlib.sha256(stream).hexdigest()]


@functools.lru_cache(maxsize=None)
def digests():
    """{name: [length, sha256]} of zlib 1.2.11's level-9 stream of every case, as recorded"""
    with open(DIGESTS) as f:
        return json.load(f)["cases"]


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
    """[(type, symbols, bytes, lf, df, cf)] of a zlib stream's blocks: 0 stored (symbols: its bytes), 1 fixed, 2 dynamic (symbols without the
    end-of-block; bytes: what they decode to; lf, df, cf: how often each literal/length, distance and code-length symbol occurs;
    None for a stored block, cf None for a fixed one), and the deepest literal/length and code-length code of its dynamic blocks.  A plain decoder after RFC 1951, for the corpus' own test."""
    bits, at, out, deep = int.from_bytes(stream, "little") >> 16, 0, [], [0, 0]

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
            out.append((0, n, n, None, None, None))
        else:
            cf = None
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
                deep = [max(deep[0], max(lens[:nl])), max(deep[1], max(cl))]
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
            out.append((kind, n, made, lf, df, cf))
        if last:
            return out, deep
