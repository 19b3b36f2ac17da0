"""JPEG Baseline test material shared by tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py: an independent reference decoder (straight
scalar loops, a sequential reader; it shares no code with frames.jpeg_decode_frame or the C++ core), a small baseline ENCODER for
hand-made streams (quantised coefficients and chosen tables -> bytes), and the corpus: the encoder-made streams of
tests/golden/jpeg_corpus.npz (with the SHA-256 of Pillow's two decodes), hand-made streams, and malformed ones for every status.
No case provokes a fault: a malformed stream is an input the bounds-checked decoder refuses."""
import functools
import hashlib
import os
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_corpus.npz")
T = 1024                                                                   # the kernels' stage (tf_jpeg_stage_bytes)
Case = namedtuple("Case", "name buf H W samples")

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


# ---- the reference decoder ---------------------------------------------------------------------------------------------------------------
class _Fail(Exception):
    def __init__(self, status):
        self.status = status


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def _idct8(x):
    z1 = (x[2] + x[6]) * 4433
    t2 = z1 - x[6] * 15137
    t3 = z1 + x[2] * 6270
    t0 = (x[0] + x[4]) << 13
    t1 = (x[0] - x[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0 *= 2446
    a1 *= 16819
    a2 *= 25172
    a3 *= 12299
    z1 *= -7373
    z2 *= -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    a0 += z1 + z3
    a1 += z2 + z4
    a2 += z2 + z3
    a3 += z1 + z4
    return [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]


def _idct_block(coef_zz, q_zz):
    """64 quantised coefficients and the table, both in zig-zag order -> 8 rows of 8 samples.  Exact integers, cut to signed 32 bits
    where a descale shifts them (a ring: the same as 32-bit registers throughout)."""
    ws = [0] * 64
    for k in range(64):
        ws[ZZ[k]] = coef_zz[k] * q_zz[k]
    for c in range(8):
        col = _idct8([ws[8 * i + c] for i in range(8)])
        for i in range(8):
            ws[8 * i + c] = _i32(col[i] + 1024) >> 11
    out = []
    for r in range(8):
        row = _idct8(ws[8 * r:8 * r + 8])
        out.append([min(255, max(0, (_i32(v + 131072) >> 18) + 128)) for v in row])
    return out


class _Scan:
    """the entropy data read in sequence, bit by bit: FF 00 is the byte FF, an FF before an FF is fill, any other FF xx is a marker
    and ends the data; a bit that is not there fails"""
    def __init__(self, b, pos):
        self.b, self.pos, self.cur, self.left = b, pos, 0, 0

    def bit(self):
        if self.left == 0:
            b, n = self.b, len(self.b)
            while True:
                if self.pos >= n:
                    raise _Fail(3)
                c = b[self.pos]
                if c != 0xFF:
                    self.pos += 1
                    break
                if self.pos + 1 >= n:
                    raise _Fail(3)
                if b[self.pos + 1] == 0x00:
                    self.pos += 2
                    break
                if b[self.pos + 1] == 0xFF:
                    self.pos += 1
                    continue
                raise _Fail(3)                                             # a marker inside an interval
            self.cur, self.left = c, 8
        self.left -= 1
        return (self.cur >> self.left) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise _Fail(3)

    def next_marker(self):
        """drops what is left of the interval -> the next marker's code and moves behind it, or None at the frame's end"""
        self.left = 0
        b, n = self.b, len(self.b)
        while self.pos + 1 < n:
            if b[self.pos] == 0xFF and b[self.pos + 1] not in (0x00, 0xFF):
                self.pos += 2
                return b[self.pos - 1]
            self.pos += 1
        self.pos = n
        return None


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def _table(bits, vals):
    t, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            t[(length, code)] = vals[k]
            k += 1
            code += 1
        code <<= 1
    return t


def _u16(b, p):
    return b[p] << 8 | b[p + 1]


def _reference(b, H, W, samples):
    n = len(b)
    if n < 2 or b[0] != 0xFF or b[1] != 0xD8:
        raise _Fail(1)
    qt, ht, ri, frame, p = {}, {}, 0, None, 2
    while True:                                                            # the marker segments, in the order the core documents
        if p >= n or b[p] != 0xFF:
            raise _Fail(1)
        while p < n and b[p] == 0xFF:
            p += 1
        if p >= n:
            raise _Fail(1)
        marker = b[p]
        p += 1
        if marker == 0 or marker == 0xD9:
            raise _Fail(1)
        if marker == 1 or 0xD0 <= marker <= 0xD8:
            continue
        if p + 2 > n:
            raise _Fail(1)
        length = _u16(b, p)
        if length < 2 or p + length > n:
            raise _Fail(1)
        seg, p = b[p + 2:p + length], p + length
        if marker in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF, 0xDC, 0xDE, 0xDF):
            raise _Fail(2)
        if marker == 0xC0:
            if frame is not None or len(seg) < 6:
                raise _Fail(1)
            if seg[0] != 8:
                raise _Fail(2)
            nf = seg[5]
            if len(seg) != 6 + 3 * nf:
                raise _Fail(1)
            if _u16(seg, 1) == 0:
                raise _Fail(2)
            if _u16(seg, 1) != H or _u16(seg, 3) != W or nf != samples:
                raise _Fail(1)
            frame = [{"id": seg[6 + 3 * c], "h": seg[7 + 3 * c] >> 4, "v": seg[7 + 3 * c] & 15, "tq": seg[8 + 3 * c]} for c in range(nf)]
            for comp in frame:
                if comp["tq"] > 3:
                    raise _Fail(1)
            if nf == 1:
                frame[0]["h"] = frame[0]["v"] = 1
            else:
                hv = [(c["h"], c["v"]) for c in frame]
                if hv not in ([(1, 1)] * 3, [(2, 1), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1)]):
                    raise _Fail(2)
        elif marker == 0xDB:
            at = 0
            while at < len(seg):
                if (seg[at] & 15) > 3 or (seg[at] >> 4) > 1:
                    raise _Fail(1)
                if seg[at] >> 4:
                    raise _Fail(2)
                if len(seg) - at < 65:
                    raise _Fail(1)
                qt[seg[at] & 15] = list(seg[at + 1:at + 65])
                at += 65
        elif marker == 0xC4:
            at = 0
            while at < len(seg):
                tc, th = seg[at] >> 4, seg[at] & 15
                if tc > 1 or th > 3:
                    raise _Fail(1)
                if th > 1:
                    raise _Fail(2)
                if len(seg) - at < 17:
                    raise _Fail(1)
                bits = list(seg[at + 1:at + 17])
                space = 1
                for length in range(16):                                   # Kraft: the codes of each length must fit what the shorter ones left
                    space = space * 2 - bits[length]
                    if space < 0:
                        raise _Fail(1)
                if sum(bits) > 256 or len(seg) - at - 17 < sum(bits):
                    raise _Fail(1)
                ht[(tc, th)] = _table(bits, seg[at + 17:at + 17 + sum(bits)])
                at += 17 + sum(bits)
        elif marker == 0xDD:
            if len(seg) != 2:
                raise _Fail(1)
            ri = _u16(seg, 0)
        elif marker == 0xDA:
            if frame is None or len(seg) < 1:
                raise _Fail(1)
            ns = seg[0]
            if len(seg) != 4 + 2 * ns:
                raise _Fail(1)
            if ns != len(frame):
                raise _Fail(2)
            for c in range(ns):
                if seg[1 + 2 * c] != frame[c]["id"]:
                    raise _Fail(2)
                td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
                if td > 3 or ta > 3:
                    raise _Fail(1)
                if td > 1 or ta > 1:
                    raise _Fail(2)
                frame[c]["td"], frame[c]["ta"] = td, ta
            if list(seg[1 + 2 * ns:4 + 2 * ns]) != [0, 63, 0]:
                raise _Fail(2)
            for comp in frame:
                if comp["tq"] not in qt or (0, comp["td"]) not in ht or (1, comp["ta"]) not in ht:
                    raise _Fail(1)
            break
    hmax, vmax = frame[0]["h"], frame[0]["v"]
    mcux, mcuy = (W + 8 * hmax - 1) // (8 * hmax), (H + 8 * vmax - 1) // (8 * vmax)
    planes = [[[0] * (mcux * c["h"] * 8) for _ in range(mcuy * c["v"] * 8)] for c in frame]
    scan, pred, done, interval = _Scan(b, p), [0] * len(frame), 0, 0
    for my in range(mcuy):
        for mx in range(mcux):
            if ri and done and done % ri == 0:                             # a restart: RSTm, m = the interval's number mod 8
                if scan.next_marker() != 0xD0 + interval % 8:
                    raise _Fail(3)
                interval += 1
                pred = [0] * len(frame)
            for ci, comp in enumerate(frame):
                for by in range(comp["v"]):
                    for bx in range(comp["h"]):
                        coef = [0] * 64
                        s = scan.symbol(ht[(0, comp["td"])])
                        if s > 15:
                            raise _Fail(3)
                        pred[ci] += _extend(scan.bits(s), s) if s else 0
                        if not -32768 <= pred[ci] <= 32767:
                            raise _Fail(3)
                        coef[0] = pred[ci]
                        k = 1
                        while k < 64:
                            rs = scan.symbol(ht[(1, comp["ta"])])
                            run, size = rs >> 4, rs & 15
                            if size == 0:
                                if run == 0:
                                    break
                                if run != 15 or k + 16 > 64:
                                    raise _Fail(3)
                                k += 16
                                continue
                            k += run
                            if k > 63:
                                raise _Fail(3)
                            coef[k] = _extend(scan.bits(size), size)
                            k += 1
                        px = _idct_block(coef, qt[comp["tq"]])
                        y0, x0 = (my * comp["v"] + by) * 8, (mx * comp["h"] + bx) * 8
                        for r in range(8):
                            planes[ci][y0 + r][x0:x0 + 8] = px[r]
            done += 1
    while True:                                                            # behind the last MCU: an RSTn more is one too many
        m = scan.next_marker()
        if m is None or not 0xD0 <= m <= 0xD7:
            break
        raise _Fail(3)
    out = np.zeros((H, W, len(frame)), np.uint8)
    for ci, comp in enumerate(frame):
        s = planes[ci]
        if (comp["h"], comp["v"]) == (hmax, vmax):
            for y in range(H):
                out[y, :, ci] = s[y][:W]
        elif vmax == 1:                                                    # h2v1 fancy
            wd = (W + 1) // 2
            for y in range(H):
                row = [0] * (2 * wd)
                for i in range(wd):
                    row[2 * i] = s[y][i] if i == 0 else (3 * s[y][i] + s[y][i - 1] + 1) >> 2
                    row[2 * i + 1] = s[y][i] if i == wd - 1 else (3 * s[y][i] + s[y][i + 1] + 2) >> 2
                out[y, :, ci] = row[:W]
        else:                                                              # h2v2 fancy
            wd, hd = (W + 1) // 2, (H + 1) // 2
            for y in range(H):
                near = min(hd - 1, y // 2 + 1) if y % 2 else max(0, y // 2 - 1)
                t = [3 * s[y // 2][i] + s[near][i] for i in range(wd)]
                row = [0] * (2 * wd)
                for i in range(wd):
                    row[2 * i] = (4 * t[i] + 8) >> 4 if i == 0 else (3 * t[i] + t[i - 1] + 8) >> 4
                    row[2 * i + 1] = ((4 * t[i] + (8 if wd == 1 else 7)) >> 4) if i == wd - 1 else (3 * t[i] + t[i + 1] + 7) >> 4
                out[y, :, ci] = row[:W]
    return out


def reference_decode(buf, H, W, samples):
    """-> (uint8 [H,W,samples] or [H,W]; status): the stream's own components, upsampled; zeros for a frame that fails"""
    shape = (H, W) if samples == 1 else (H, W, samples)
    try:
        return np.ascontiguousarray(_reference(bytes(buf), H, W, samples).reshape(shape)), 0
    except _Fail as f:
        return np.zeros(shape, np.uint8), f.status


def reference_rgb(ycc):
    """libjpeg's colour tables on uint8 [...,3], one pixel at a time"""
    a = np.asarray(ycc).reshape(-1, 3)
    out = np.zeros(a.shape, np.uint8)
    for i, (y, cb, cr) in enumerate(a.tolist()):
        cb, cr = cb - 128, cr - 128
        out[i] = [min(255, max(0, y + ((91881 * cr + 32768) >> 16))), min(255, max(0, y + ((-22554 * cb + 32768 - 46802 * cr) >> 16))),
                  min(255, max(0, y + ((116130 * cb + 32768) >> 16)))]
    return out.reshape(np.asarray(ycc).shape)


# ---- the encoder for hand-made streams -----------------------------------------------------------------------------------------------------
def code_table(lengths):
    """[(symbol, code length)] in code order -> (bits[16], vals): the canonical table that gives each symbol that length"""
    lengths = sorted(lengths, key=lambda sl: sl[1])
    return [sum(1 for _, l in lengths if l == n) for n in range(1, 17)], [s for s, _ in lengths]


def flat_table(symbols, length):
    return code_table([(s, length) for s in symbols])


AC_SYMBOLS = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)]
DC_FLAT = flat_table(range(12), 4)
AC_FLAT = flat_table(AC_SYMBOLS, 8)                                        # every code in the 8-bit look-ahead
AC_NINE = flat_table(AC_SYMBOLS, 9)                                        # every code behind it
DC_LONG = code_table([(s, s + 1) for s in range(12)])                      # category 11 has a 12-bit code
DC_WIDE = code_table([(s, 5) for s in range(17)])                          # categories up to 16: for DC values outside int16


def _codes(table):
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            k += 1
            code += 1
        code <<= 1
    return out


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


class _BitsOut:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc, self.n = self.acc << n | (v & ((1 << n) - 1)), self.n + n
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)                  # pad with ones, as encoders do


def _size(v):
    return abs(v).bit_length()


def encode(H, W, blocks, sampling=((1, 1),), q=None, dc=DC_FLAT, ac=AC_FLAT, ri=0, fill=0, com=None, dht_in_one=False, extra=b""):
    """A baseline stream of H x W.  blocks: the quantised coefficients in zig-zag order, a list of 64 per block, in the order the scan
    holds them (MCU by MCU; a component's h x v blocks row by row).  sampling: (h, v) per component.  q: the quantisation table (64,
    zig-zag order; one table for all).  dc / ac: (bits, vals), or a list of two of them -- table 0 for the first component, table 1
    for the others.  ri: the restart interval.  fill: FF bytes in front of every RSTn.  com: a COM segment's payload, in front.  extra:
    bytes behind the entropy data, in front of EOI."""
    q = [1] * 64 if q is None else list(q)
    dcs, acs = (dc if isinstance(dc, list) else [dc]), (ac if isinstance(ac, list) else [ac])
    out = bytearray(b"\xff\xd8")
    if com is not None:
        out += _seg(0xFE, com)
    out += _seg(0xDB, [0] + q)
    tables = [(0x00 + i, t) for i, t in enumerate(dcs)] + [(0x10 + i, t) for i, t in enumerate(acs)]
    if dht_in_one:
        out += _seg(0xC4, b"".join(bytes([tcth]) + bytes(t[0]) + bytes(t[1]) for tcth, t in tables))
    else:
        for tcth, t in tables:
            out += _seg(0xC4, bytes([tcth]) + bytes(t[0]) + bytes(t[1]))
    nc = len(sampling)
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc]) + b"".join(bytes([c + 1, h << 4 | v, 0]) for c, (h, v) in enumerate(sampling)))
    if ri:
        out += _seg(0xDD, ri.to_bytes(2, "big"))
    sel = lambda c, ts: min(1 if c else 0, len(ts) - 1)
    out += _seg(0xDA, bytes([nc]) + b"".join(bytes([c + 1, sel(c, dcs) << 4 | sel(c, acs)]) for c in range(nc)) + bytes([0, 63, 0]))
    per_mcu = [c for c, (h, v) in enumerate(sampling) for _ in range(h * v)] if nc > 1 else [0]
    dcc, acc = [_codes(t) for t in dcs], [_codes(t) for t in acs]
    bits, pred, rst = _BitsOut(), [0] * nc, 0
    for i, blk in enumerate(blocks):
        if ri and i and i % (ri * len(per_mcu)) == 0:
            bits.flush()
            out += bits.out + b"\xff" * fill + bytes([0xFF, 0xD0 + rst % 8])
            bits, pred, rst = _BitsOut(), [0] * nc, rst + 1
        c = per_mcu[i % len(per_mcu)]
        d, a = dcc[sel(c, dcs)], acc[sel(c, acs)]
        diff = blk[0] - pred[c]
        pred[c] = blk[0]
        s = _size(diff)
        bits.put(*d[s])
        if s:
            bits.put(diff if diff > 0 else diff + (1 << s) - 1, s)
        run = 0
        last = max([k for k in range(1, 64) if blk[k]], default=0)
        for k in range(1, last + 1):
            if blk[k] == 0:
                run += 1
                continue
            while run > 15:
                bits.put(*a[0xF0])
                run -= 16
            s = _size(blk[k])
            bits.put(*a[run << 4 | s])
            bits.put(blk[k] if blk[k] > 0 else blk[k] + (1 << s) - 1, s)
            run = 0
        if last < 63:
            bits.put(*a[0x00])
    bits.flush()
    return bytes(out + bits.out + extra + b"\xff\xd9")


def _blocks(rng, n, amp=40, density=0.3):
    out = []
    for _ in range(n):
        b = [0] * 64
        b[0] = int(rng.integers(-200, 200))
        for k in range(1, 64):
            if rng.random() < density / (1 + k / 8):
                b[k] = int(rng.integers(-amp, amp + 1))
        out.append(b)
    return out


# ---- the corpus --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    """the encoder-made streams: (cases, {name: (sha of the stream's own components, sha of the RGB)})"""
    z = np.load(GOLDEN)
    blob, sha = z["blob"].tobytes(), {}
    cases = []
    for i, name in enumerate(z["names"].tolist()):
        o, n = int(z["off"][i]), int(z["len"][i])
        H, W, samples = (int(v) for v in z["shape"][i])
        cases.append(Case(name, blob[o:o + n], H, W, samples))
        sha[name] = (str(z["sha_own"][i]), str(z["sha_rgb"][i]))
    return tuple(cases), sha


def stage_stream(pad):
    """one 16 x 16 grey stream behind a COM segment of `pad` bytes: Ri = 1, stuffed FF runs, 16-bit codes -- as pad goes 0 ... T + 16
    every one of them sits on every offset of the stage boundary.  The pixels do not depend on pad."""
    rng = np.random.default_rng(77)
    blocks = []
    for i in range(4):
        b = [0] * 64
        b[0] = [255, -255, 1023, 0][i]                                      # (all-ones magnitude bits: stuffed FF bytes)
        for k in (1, 2, 3):
            b[k] = [1023, -1, 255, 511][(i + k) % 4]
        b[5], b[8], b[40] = (-1) ** i, 3, 10                                # runs of 1, 2 and -- behind a ZRL -- 15
        b[63] = 1023 if i % 2 else int(rng.integers(1, 4))                  # behind another ZRL; 0x6A has a 16-bit code
        blocks.append(b)
    return encode(16, 16, blocks, dc=DC_LONG, ac=AC_LONG_FULL, ri=1, fill=pad % 3, com=bytes(pad))


AC_LONG_FULL = code_table([(s, l) for s, l in zip([0x01, 0x00, 0x02, 0x0A, 0x09, 0x08, 0x03, 0xF0] + [r << 4 | s for r in range(1, 16) for s in (1, 2, 4)] + [0x1A, 0x2A, 0x3A, 0x4A, 0x5A, 0x6A, 0x7A],
                                                  [2, 2, 3, 4, 5, 6, 7, 8] + [10] * 45 + [11, 12, 13, 14, 15, 16, 16])])


def _patch(buf, marker, at, value):
    """byte `at` of the first segment `marker`'s payload set to value (at < 0: the marker's own code)"""
    i = buf.index(bytes([0xFF, marker]))
    b = bytearray(buf)
    if at < 0:
        b[i + 1] = value
    else:
        b[i + 4 + at] = value
    return bytes(b)


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(4150)
    cases = list(golden()[0])
    add = lambda name, buf, H, W, samples: cases.append(Case(name, bytes(buf), H, W, samples))
    # hand-made, valid
    one = [0] * 64
    add("hand_flat_tables", encode(16, 24, _blocks(rng, 6)), 16, 24, 1)
    add("hand_nine_bit_codes", encode(16, 24, _blocks(rng, 6), ac=AC_NINE), 16, 24, 1)
    add("hand_sixteen_bit_codes", stage_stream(0), 16, 16, 1)
    zrl = list(one); zrl[0] = 5; zrl[20] = 3; zrl[60] = -2
    add("hand_zrl_before_eob", encode(8, 8, [zrl]), 8, 8, 1)
    zrl_end = list(one); zrl_end[63] = 1
    add("hand_three_zrl_then_last", encode(8, 8, [zrl_end]), 8, 8, 1)
    full = [int(v) for v in rng.integers(1, 30, 64)]
    add("hand_all_63_ac", encode(8, 8, [full]), 8, 8, 1)
    add("hand_dc_plus_2047_q255", encode(8, 16, [[2047] + [0] * 63, [-2047] + [0] * 63], q=[255] * 64, ri=1), 8, 16, 1)
    add("hand_dc_steps_q255", encode(8, 32, [[v] + [0] * 63 for v in (1023, -1024, 1023, 0)], q=[255] + [1] * 63, ri=2), 8, 32, 1)
    add("hand_ac_extremes_q255", encode(8, 8, [[0, 1023, -1023] + [0] * 61], q=[255] * 64), 8, 8, 1)
    add("hand_fill_before_rst", encode(16, 16, _blocks(rng, 4), ri=1, fill=3), 16, 16, 1)
    add("hand_stuffed_runs", encode(8, 16, [[255] + [255, -1, 1023, 511, 255] * 4 + [0] * 43] * 2), 8, 16, 1)
    add("hand_420_two_tables", encode(17, 23, _blocks(rng, 2 * 2 * 6), sampling=((2, 2), (1, 1), (1, 1)), dc=[DC_FLAT, DC_LONG], ac=[AC_FLAT, AC_NINE], ri=3), 17, 23, 3)
    add("hand_422_one_dht", encode(9, 33, _blocks(rng, 2 * 3 * 4), sampling=((2, 1), (1, 1), (1, 1)), dht_in_one=True, ri=2), 9, 33, 3)
    add("hand_444_restart_9_intervals", encode(8, 72, _blocks(rng, 27), sampling=((1, 1),) * 3, ri=1, fill=1), 8, 72, 3)
    add("hand_bytes_after_last_mcu", encode(8, 8, [zrl], extra=b"\x12\x34\x00\x56"), 8, 8, 1)
    add("hand_no_eoi", encode(8, 8, [zrl])[:-2], 8, 8, 1)
    add("hand_com_and_app", b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes(9)) + _seg(0xEC, b"x") + b"\xff\xff" + encode(8, 8, [zrl], com=b"hello")[2:], 8, 8, 1)
    # tables redefined between the frames of one batch: the same shape, other tables and other quantisation
    for i, (dcq, acq, qv) in enumerate([(DC_FLAT, AC_FLAT, 1), (DC_LONG, AC_NINE, 7), (DC_FLAT, AC_NINE, 255), (DC_LONG, AC_FLAT, 16)]):
        add(f"hand_redefined_{i}", encode(16, 16, _blocks(rng, 4, amp=8), dc=dcq, ac=acq, q=[qv] * 64), 16, 16, 1)
    # malformed: every status
    good = encode(8, 16, _blocks(rng, 2), ri=1)
    good3 = encode(8, 8, _blocks(rng, 3), sampling=((1, 1),) * 3)
    add("bad_no_soi", b"\x00" + good[1:], 8, 16, 1)
    add("bad_empty", b"", 8, 16, 1)
    add("bad_segment_past_frame", good[:good.index(b"\xff\xc4") + 2] + b"\xff\xff" + good[good.index(b"\xff\xc4") + 4:], 8, 16, 1)
    add("bad_no_huffman_table", good.replace(_seg(0xC4, bytes([0x10]) + bytes(AC_FLAT[0]) + bytes(AC_FLAT[1])), b""), 8, 16, 1)
    add("bad_no_quant_table", good.replace(_seg(0xDB, [0] + [1] * 64), b""), 8, 16, 1)
    add("bad_size", good, 8, 17, 1)
    add("bad_components", good, 8, 16, 3)
    add("bad_no_sos", good[:good.index(b"\xff\xda")] + b"\xff\xd9", 8, 16, 1)
    add("bad_garbage_between_segments", good[:2] + b"\x55" + good[2:], 8, 16, 1)
    add("bad_oversubscribed_dht", _patch(good, 0xC4, 1, 3), 8, 16, 1)
    for m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
        add(f"refused_sof_{m:02x}", _patch(good, 0xC0, -1, m), 8, 16, 1)
    add("refused_dac", good[:2] + _seg(0xCC, b"\x00\x10") + good[2:], 8, 16, 1)
    add("refused_dnl", good[:2] + _seg(0xDC, b"\x00\x08") + good[2:], 8, 16, 1)
    add("refused_zero_lines", _patch(_patch(good, 0xC0, 1, 0), 0xC0, 2, 0), 8, 16, 1)
    add("refused_precision_12", _patch(good, 0xC0, 0, 12), 8, 16, 1)
    add("refused_16_bit_dqt", _patch(good, 0xDB, 0, 0x10), 8, 16, 1)
    add("refused_sampling_1x2", _patch(good3, 0xC0, 7, 0x12), 8, 8, 3)
    add("refused_sampling_4x1", _patch(good3, 0xC0, 7, 0x41), 8, 8, 3)
    add("refused_sampling_chroma_2x1", _patch(good3, 0xC0, 10, 0x21), 8, 8, 3)
    add("bad_scan_length", _patch(good3, 0xDA, 0, 1), 8, 8, 3)
    sos = good3.index(b"\xff\xda")
    add("refused_scan_of_two", good3[:sos] + _seg(0xDA, bytes([2, 1, 0, 2, 0, 0, 63, 0])) + good3[sos + 14:], 8, 8, 3)
    add("refused_scan_order", _patch(good3, 0xDA, 1, 2), 8, 8, 3)
    add("refused_spectral", _patch(good, 0xDA, 4, 62), 8, 16, 1)
    add("refused_approximation", _patch(good, 0xDA, 5, 0x10), 8, 16, 1)
    add("refused_huffman_table_2", _patch(good, 0xDA, 2, 0x20), 8, 16, 1)
    data = good.index(b"\xff\xda") + 10
    add("data_no_code", good[:data] + b"\xff\x00" * 6 + good[data + 12:], 8, 16, 1)
    add("data_missing_rst", good.replace(b"\xff\xd0", b"\x00\x00"), 8, 16, 1)
    add("data_wrong_rst_number", good.replace(b"\xff\xd0", b"\xff\xd1"), 8, 16, 1)
    add("data_extra_rst", good[:-2] + b"\xff\xd1\xff\xd9", 8, 16, 1)
    add("data_rst_without_dri", encode(8, 16, _blocks(rng, 2))[:-2] + b"\xff\xd0\xff\xd9", 8, 16, 1)
    add("data_interval_ends_early", good[:good.index(b"\xff\xd0") - 2] + good[good.index(b"\xff\xd0"):], 8, 16, 1)
    add("data_marker_inside", good[:data + 1] + b"\xff\xd9" + good[data + 3:], 8, 16, 1)
    add("data_dc_outside_int16", encode(8, 24, [[0x7FFF] + [0] * 63, [0x7FFF * 2] + [0] * 63, one], dc=DC_WIDE), 8, 24, 1)
    add("data_dc_category_16", encode(8, 8, [[0x8000] + [0] * 63], dc=DC_WIDE), 8, 8, 1)
    add("data_zrl_past_63", _raw_ac(8, 8, [0xF0, 0xF0, 0xF0, 0xF0]), 8, 8, 1)
    add("data_run_past_63", _raw_ac(8, 8, [0xF0, 0xF0, 0xF0, 0xF1, 1]), 8, 8, 1)
    add("data_eob_run", _raw_ac(8, 8, [0x50]), 8, 8, 1)
    small = encode(8, 8, [zrl], ri=0)
    for cut in range(len(small)):
        add(f"cut_after_{cut}", small[:cut], 8, 8, 1)
    return tuple(cases)


def _raw_ac(H, W, symbols):
    """one grey block: DC 0, then the AC symbols as given (a symbol with a size is followed by its magnitude bits' value)"""
    table = flat_table(sorted(set(AC_SYMBOLS) | {0x50, 0xF1}), 8)
    head = encode(H, W, [[0] * 64], ac=table)
    head = head[:head.index(b"\xff\xda") + 10]
    codes, bits = _codes(table), _BitsOut()
    bits.put(*_codes(DC_FLAT)[0])
    i = 0
    while i < len(symbols):
        bits.put(*codes[symbols[i]])
        if symbols[i] & 15:
            bits.put(symbols[i + 1], symbols[i] & 15)
            i += 1
        i += 1
    bits.flush()
    return head + bytes(bits.out) + b"\xff\xd9"


@functools.lru_cache(maxsize=None)
def expected():
    """{name: (array, status)} by the reference decoder"""
    return {c.name: reference_decode(c.buf, c.H, c.W, c.samples) for c in corpus()}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def write_corpus(path, cases=None, want=None):
    """corpus.bin for tests/csrc/verify_jpeg.cpp: uint32 count, then per case uint32 H, W, samples, len, status, the stream's bytes and
    -- status 0 -- the H * W * samples bytes it decodes to"""
    want = expected() if want is None else want
    cases = corpus() if cases is None else cases
    with open(path, "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for c in cases:
            arr, status = want[c.name]
            f.write(np.array([c.H, c.W, c.samples, len(c.buf), status], np.uint32).tobytes())
            f.write(c.buf)
            if status == 0:
                f.write(arr.tobytes())
