"""Streams for the split entropy decode of JPEG Lossless (csrc/teeflow_jpegll_sync_core.h), shared by tests/test_jpegll_sync_cpu.py and
tests/test_gpu_jpegll_sync.py.  Every stream is aimed at one place where cutting a restart interval into pieces of S bytes can go
wrong; tests/test_jpegll_sync_cpu.py asserts that each one hits its target, so that the GPU tests cannot quietly miss it.  The
builder and the independent reference decoder are tests/jpegll_cases.py's.  No case provokes a fault: a malformed stream is an input
the bounds-checked decoder answers with a status."""
import functools

import numpy as np

from tee_optical_flow_amd import frames as F

from tests import jpegll_cases as LC
from tests.jpegll_cases import Case

S = 32                                                                     # bytes a piece (tf_jpegll_segment_bytes)
R = 8                                                                      # the library's default of "jpegll_sync_rounds" (_lib.JPEGLL_SYNC_ROUNDS)


def scan_offset(buf):
    """the first byte of a stream's entropy data"""
    i = buf.index(b"\xff\xda")
    return i + 2 + int.from_bytes(buf[i + 2:i + 4], "big")


def entropy_bytes(buf):
    """the length of the entropy data of a stream without DRI that ends with EOI"""
    assert buf[-2:] == b"\xff\xd9"
    return len(buf) - 2 - scan_offset(buf)


def pieces(buf):
    return max(1, -(-entropy_bytes(buf) // S))


def _grey(name, img, **kw):
    H, W = img.shape
    return Case(name, LC.build(H, W, 1, LC.diffs_of(img), **kw), H, W, 1)


# ---- the bit-offset walk: k one-bit symbols in front of noise, so that the noise's symbol boundaries stand k bits further on ---------------
def walk_image(k, rng):
    a = np.full(k + 150, 128, np.uint8)                                    # one row; 128 is the first prediction: k zero differences
    a[k:] = rng.integers(0, 256, 150)
    if k:
        a[k] = 77                                                          # (the first difference behind the zeros is none)
    return a.reshape(1, -1)


@functools.lru_cache(maxsize=None)
def bit_offset_walk():
    """k = 0 .. 8 * S: under LONG a zero difference is the one-bit code, so symbol k starts at bit k of the entropy data"""
    rng = np.random.default_rng(3100)
    return tuple(_grey(f"walk_{k}", walk_image(k, rng), tables=(LC.LONG,)) for k in range(8 * S + 1))


# ---- stuffing at a cut: a seeded search -------------------------------------------------------------------------------------------------------
def stuffing_at_cuts(buf):
    """-> (cuts with FF the last byte of a piece and its 00 the first of the next, cuts right behind a pair FF 00)"""
    o, n = scan_offset(buf), entropy_bytes(buf)
    data = buf[o:o + n]
    straddle = [c for c in range(S, n, S) if data[c - 1] == 0xFF and data[c] == 0x00]
    behind = [c for c in range(S, n, S) if c >= 2 and data[c - 2] == 0xFF and data[c - 1] == 0x00]
    return straddle, behind


@functools.lru_cache(maxsize=None)
def stuffing_cases():
    """the first three seeds of each kind: differences of +-255 under FLAT5 give all-ones magnitude bits, so stuffed FF bytes are dense"""
    found = {"straddle": [], "behind": []}
    for seed in range(400):
        rng = np.random.default_rng(5000 + seed)
        a = rng.integers(0, 256, (6, 40), dtype=np.uint8)
        a[:, ::3] = 255
        a[:, 1::3] = 0
        c = _grey(f"stuff_{seed}", a, tables=(LC.FLAT5,))
        straddle, behind = stuffing_at_cuts(c.buf)
        for kind, hit in (("straddle", straddle), ("behind", behind)):
            if hit and len(found[kind]) < 3:
                found[kind].append(c._replace(name=f"stuff_{kind}_{seed}"))
        if all(len(v) == 3 for v in found.values()):
            break
    return tuple(found["straddle"]), tuple(found["behind"])


# ---- tables and phase -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_cases():
    rng = np.random.default_rng(3200)
    a = LC.image("noise", 12, 40, 3, rng)
    d = LC.diffs_of(a)
    return (Case("tables_0_1_2", LC.build(12, 40, 3, d, tables=(LC.K3, LC.NINE, LC.LONG)), 12, 40, 3),
            Case("tables_0_1_1", LC.build(12, 40, 3, d, tables=(LC.K3, LC.NINE), sel=[0, 1, 1]), 12, 40, 3),
            Case("tables_same_code_two_ids", LC.build(12, 40, 3, d, tables=(LC.K3, LC.K3), sel=[0, 1, 0]), 12, 40, 3))


@functools.lru_cache(maxsize=None)
def big_table_cases():
    """three and two codes on three components over several blocks of pieces: the phase is part of the compared state and guessed 0, so
    the truth travels a block of pieces a round and the default rounds do not suffice"""
    rng = np.random.default_rng(3250)
    a = LC.image("noise", 80, 200, 3, rng)
    return (Case("tables_big_0_1_2", F.jpegll_encode_frame(a, tables=[LC.K3, LC.NINE, LC.LONG]), 80, 200, 3),
            Case("tables_big_0_1_1", F.jpegll_encode_frame(a, tables=[LC.K3, LC.NINE]), 80, 200, 3))


# ---- streams that do not synchronise, and one that is slow to --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stubborn_cases():
    y, x = np.mgrid[0:40, 0:96]
    checker = (((x + y) % 2) * 255).astype(np.uint8)
    ramp = (np.arange(40 * 96) % 200).astype(np.uint8).reshape(40, 96)
    yy, xx = np.mgrid[0:80, 0:200]
    big = np.ascontiguousarray(np.stack([((xx + yy) % 2) * 255] * 3, -1).astype(np.uint8))
    return (Case("checkerboard", F.jpegll_encode_frame(checker), 40, 96, 1), Case("ramp", F.jpegll_encode_frame(ramp), 40, 96, 1),
            Case("checkerboard_big", F.jpegll_encode_frame(big, tables=LC.LONG), 80, 200, 3))   # (LONG: 24 bits a symbol, a stream of 20 blocks of pieces)


# ---- noise and speckle, 1 and 3 samples: what the default R is for -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_cases():
    rng = np.random.default_rng(3300)
    out = []
    for kind in ("noise", "speckle"):
        for C in (1, 3):
            a = LC.image(kind, 80, 200, C, rng)
            out.append(Case(f"plain_{kind}_{C}", F.jpegll_encode_frame(a[..., 0] if C == 1 else a), 80, 200, C))
    return tuple(out)


# ---- the smallest shapes ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_cases():
    """1 x 1, and streams whose entropy data is exactly one piece, one piece and a byte, two pieces and a byte"""
    rng = np.random.default_rng(3400)
    out = [_grey("small_1x1", np.array([[200]], np.uint8))]
    want = {S: "one_piece", S + 1: "one_piece_and_a_byte", 2 * S + 1: "last_piece_of_one_byte"}
    for _ in range(4000):
        W = int(rng.integers(20, 70))
        c = _grey("small", rng.integers(0, 256, (1, W), dtype=np.uint8))
        n = entropy_bytes(c.buf)
        if n in want and b"\xff" not in c.buf[scan_offset(c.buf):-2]:       # (no stuffing: the length is the data bytes)
            out.append(c._replace(name="small_" + want.pop(n)))
        if not want:
            break
    return tuple(out)


# ---- the data's end -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def end_cases():
    rng = np.random.default_rng(3500)
    a = rng.integers(0, 256, (4, 60), dtype=np.uint8)
    a[-1, -2:] = (0, 255)                                                  # the last difference is +255: eight extra bits
    good = _grey("end_good", a)
    o, n = scan_offset(good.buf), entropy_bytes(good.buf)
    early = good.buf[:o + n - 1] + b"\xff\xd9"                              # the last data byte is gone: the extra bits of the last sample run out
    short = LC.build(4, 60, 1, LC.diffs_of(a), tables=(LC.SHORT,), extra=b"\xff\x00" * 40)   # all-ones bits behind the last sample: no code of SHORT
    return (good, Case("end_early", early, 4, 60, 1), Case("end_garbage_tail", short, 4, 60, 1))


# ---- restart intervals of several rows -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restart_cases():
    rng = np.random.default_rng(3600)
    a = LC.image("noise", 60, 90, 3, rng)
    b = rng.integers(0, 256, (40, 70, 3), dtype=np.uint8)
    return (Case("restart_12_rows", LC.build(60, 90, 3, LC.diffs_of(a, 12), rows=12), 60, 90, 3),
            Case("restart_7_rows_grey", LC.build(60, 90, 1, LC.diffs_of(a[..., 0], 7), rows=7, fill=1), 60, 90, 1),
            Case("restart_40_intervals", LC.build(40, 70, 3, LC.diffs_of(b, 1), rows=1, fill=2), 40, 70, 3),
            Case("restart_none_of_the_40", LC.build(40, 70, 3, LC.diffs_of(b)), 40, 70, 3))


def groups():
    straddle, behind = stuffing_cases()
    return {"walk": bit_offset_walk(), "stuff_straddle": straddle, "stuff_behind": behind, "tables": table_cases(), "tables_big": big_table_cases(), "stubborn": stubborn_cases(),
            "plain": plain_cases(), "small": small_cases(), "end": end_cases(), "restart": restart_cases()}


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(c for g in groups().values() for c in g)


@functools.lru_cache(maxsize=None)
def expected():
    """{name: (array, status)} by the reference decoder of tests/jpegll_cases.py"""
    return {c.name: LC.reference_decode(c.buf, c.H, c.W, c.samples) for c in cases()}
