"""JPEG Lossless (SOF3, predictor 1) test material shared by tests/test_jpegll_cpu.py and tests/test_gpu_jpegll.py: an independent
reference decoder (one plain loop over the samples, predicting each from its decoded neighbours as T.81 Annex H words it; a sequential
bit reader; it shares no code with frames.jpegll_decode_frame or the C++ core), a hand-written stream BUILDER (differences and chosen
tables -> bytes), and the corpus: the encoder-made streams of tests/golden/jpegll_corpus.npz (with the SHA-256 of the encoded array and
of Pillow's decode), hand-made streams, and malformed ones for every status.  No case provokes a fault: a malformed stream is an input
the bounds-checked decoder refuses."""
import functools
import hashlib
import os
from collections import namedtuple

import numpy as np

from tests.jpeg_cases import _BitsOut, _Fail, _Scan, _codes, _seg, _table, _u16, code_table, flat_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpegll_corpus.npz")
T = 1024                                                                   # the kernels' stage (tf_jpeg_stage_bytes)
Case = namedtuple("Case", "name buf H W samples")
FRAME_MARKERS = (0xC0, 0xC1, 0xC2, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF)


# ---- the reference decoder ---------------------------------------------------------------------------------------------------------------
def _reference(b, H, W, samples):
    n = len(b)
    if n < 2 or b[0] != 0xFF or b[1] != 0xD8:
        raise _Fail(1)
    ht, ri, frame, p = {}, 0, None, 2
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
        if marker in FRAME_MARKERS or marker in (0xCC, 0xDC, 0xDE, 0xDF):
            raise _Fail(2)
        if marker == 0xC3:
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
            frame = [{"id": seg[6 + 3 * c], "hv": seg[7 + 3 * c]} for c in range(nf)]
            if nf > 1 and any(c["hv"] != 0x11 for c in frame):
                raise _Fail(2)
        elif marker == 0xC4:
            at = 0
            while at < len(seg):
                tc, th = seg[at] >> 4, seg[at] & 15
                if tc != 0 or th > 3:
                    raise _Fail(1)
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
                ht[th] = _table(bits, seg[at + 17:at + 17 + sum(bits)])
                at += 17 + sum(bits)
        elif marker == 0xDD:
            if len(seg) != 2:
                raise _Fail(1)
            ri = _u16(seg, 0)
            if ri % W:
                raise _Fail(1)
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
                if seg[2 + 2 * c] >> 4 > 3:
                    raise _Fail(1)
                frame[c]["td"] = seg[2 + 2 * c] >> 4
            if list(seg[1 + 2 * ns:4 + 2 * ns]) != [1, 0, 0]:              # predictor 1, Se 0, no point transform
                raise _Fail(2)
            if any(comp["td"] not in ht for comp in frame):
                raise _Fail(1)
            break
    out = [[[0] * len(frame) for _ in range(W)] for _ in range(H)]
    scan, done, interval, first_line = _Scan(b, p), 0, 0, 0
    for y in range(H):
        for x in range(W):
            if ri and done and done % ri == 0:                             # a restart: RSTm, m = the interval's number mod 8
                if scan.next_marker() != 0xD0 + interval % 8:
                    raise _Fail(3)
                interval += 1
                first_line = y
            for ci, comp in enumerate(frame):
                s = scan.symbol(ht[comp["td"]])
                if s > 16:
                    raise _Fail(3)
                if s == 0:
                    d = 0
                elif s == 16:
                    d = 32768
                else:
                    v = scan.bits(s)
                    d = v - (1 << s) + 1 if v < (1 << (s - 1)) else v
                if y == first_line:
                    px = 128 if x == 0 else out[y][x - 1][ci]              # the first line of the scan or of an interval: 2^(P-1), then Ra
                else:
                    px = out[y - 1][0][ci] if x == 0 else out[y][x - 1][ci]    # Rb at a line's start, else Ra
                out[y][x][ci] = (px + d) % 65536
            done += 1
    while True:                                                            # behind the last sample: an RSTn more is one too many
        m = scan.next_marker()
        if m is None or not 0xD0 <= m <= 0xD7:
            break
        raise _Fail(3)
    a = np.array(out, np.int64)
    if (a > 255).any():                                                    # a sample outside the precision: judged when all are there
        raise _Fail(3)
    return a.astype(np.uint8)


def reference_decode(buf, H, W, samples):
    """-> (uint8 [H,W,samples] or [H,W]; status): the encoded array; zeros for a frame that fails"""
    shape = (H, W) if samples == 1 else (H, W, samples)
    try:
        return np.ascontiguousarray(_reference(bytes(buf), H, W, samples).reshape(shape)), 0
    except _Fail as f:
        return np.zeros(shape, np.uint8), f.status


# ---- the builder for hand-made streams -------------------------------------------------------------------------------------------------------
K3 = code_table([(s, l) for s, l in zip(range(17), [2, 3, 3, 3, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14])])
FLAT5 = flat_table(range(17), 5)                                           # every category, 16 included, in the 8-bit look-ahead
NINE = flat_table(range(9), 9)                                             # every code behind the look-ahead
LONG = code_table([(s, l) for s, l in zip([0, 1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7, 16, 16])])    # categories 7 and 8: 16-bit codes
SHORT = flat_table(range(9), 4)                                            # 1001 ... 1111 are no codes
WITH_17 = flat_table(range(18), 5)                                         # holds a category above 16


def diffs_of(arr, rows=0):
    """uint8 [H,W] or [H,W,C] -> the differences in scan order, a flat list, with a restart interval of `rows` rows (0: none)"""
    a = np.asarray(arr)
    a = a.reshape(a.shape[0], a.shape[1], -1).astype(int).tolist()
    H, W, C = len(a), len(a[0]), len(a[0][0])
    out = []
    for y in range(H):
        top = y % rows == 0 if rows else y == 0
        for x in range(W):
            for c in range(C):
                pred = (128 if top else a[y - 1][0][c]) if x == 0 else a[y][x - 1][c]
                out.append(a[y][x][c] - pred)
    return out


def build(H, W, C, diffs, tables=(K3,), sel=None, ids=None, rows=0, ri=None, fill=0, com=None, extra=b"", scan=(1, 0, 0), precision=8, sampling=0x11,
          eoi=True):
    """A lossless stream of H x W x C.  diffs: the differences in scan order (sample by sample, the components of a sample in turn), each
    in -32767 .. 32768.  tables: {id: (bits, vals)} or a list (ids 0, 1, ...); sel: the table id per component (default min(c, last)).
    rows: the restart interval in rows (ri: in samples, where it is to differ).  fill: FF bytes in front of every RSTn.  com: a COM
    segment's payload, in front.  extra: bytes behind the entropy data, in front of EOI.  scan: (Ss, Se, Ah << 4 | Al)."""
    tables = dict(enumerate(tables)) if not isinstance(tables, dict) else tables
    ids = sorted(tables) if ids is None else ids
    sel = [ids[min(c, len(ids) - 1)] for c in range(C)] if sel is None else sel
    ri = rows * W if ri is None else ri
    out = bytearray(b"\xff\xd8")
    if com is not None:
        out += _seg(0xFE, com)
    out += _seg(0xC3, bytes([precision]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([C]) + b"".join(bytes([c + 1, sampling, 0]) for c in range(C)))
    for t in ids:
        out += _seg(0xC4, bytes([t]) + bytes(tables[t][0]) + bytes(tables[t][1]))
    if ri:
        out += _seg(0xDD, ri.to_bytes(2, "big"))
    out += _seg(0xDA, bytes([C]) + b"".join(bytes([c + 1, sel[c] << 4]) for c in range(C)) + bytes(scan))
    codes = {t: _codes(tables[t]) for t in ids}
    bits, rst = _BitsOut(), 0
    for i, d in enumerate(diffs):
        if ri and i and i % (ri * C) == 0:
            bits.flush()
            out += bits.out + b"\xff" * fill + bytes([0xFF, 0xD0 + rst % 8])
            bits, rst = _BitsOut(), rst + 1
        s = 16 if d == 32768 else abs(d).bit_length()
        bits.put(*codes[sel[i % C]][s])
        if 0 < s < 16:
            bits.put(d if d > 0 else d + (1 << s) - 1, s)
    bits.flush()
    return bytes(out + bits.out + extra + (b"\xff\xd9" if eoi else b""))


def image(kind, H, W, C, rng):
    """the corpus's contents -> uint8 [H,W,C]"""
    y, x = np.mgrid[0:H, 0:W]
    if kind == "noise":
        a = rng.integers(0, 256, (H, W, C))
    elif kind == "const":
        a = np.zeros((H, W, C), int) + np.array([128, 0, 255])[:C]       # (128: every difference of the first component is zero)
    elif kind == "ramp":
        a = np.stack([(x * (c + 1) + y * 3) % 256 for c in range(C)], -1)
    elif kind == "checker":
        a = np.stack([((x + y + c) % 2) * 255 for c in range(C)], -1)      # differences of +-255
    else:                                                                  # speckle inside a sector, black outside it
        r, th = np.hypot(x - W / 2, y + 1.0), np.arctan2(x - W / 2, y + 1.0)
        inside = (np.abs(th) < 0.7) & (r < 0.95 * max(H, 2))
        g = np.clip(rng.gamma(2.0, 30.0, (H, W)), 0, 255)
        a = np.stack([np.where(inside, g, 0)] * C, -1)
    return np.ascontiguousarray(a.astype(np.uint8))


# ---- the corpus --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    """the encoder-made streams: (cases, {name: (sha of the encoded array, sha of Pillow's decode)})"""
    z = np.load(GOLDEN)
    blob, sha = z["blob"].tobytes(), {}
    cases = []
    for i, name in enumerate(z["names"].tolist()):
        o, n = int(z["off"][i]), int(z["len"][i])
        H, W, samples = (int(v) for v in z["shape"][i])
        cases.append(Case(name, blob[o:o + n], H, W, samples))
        sha[name] = (str(z["sha_array"][i]), str(z["sha_pillow"][i]))
    return tuple(cases), sha


def _stage_image():
    rng = np.random.default_rng(77)
    a = rng.integers(0, 256, (4, 24), dtype=np.uint8)
    a[:, ::3] = 255                                                        # (differences of +255 and -255: all-ones magnitude bits, stuffed FF bytes)
    a[:, 1::3] = 0
    return a


def stage_stream(pad):
    """one 4 x 24 grey stream behind a COM segment of `pad` bytes: one row an interval, stuffed FF bytes, 16-bit codes -- as pad goes
    0 ... T + 16 every one of them sits on every offset of the stage boundary.  The pixels do not depend on pad."""
    a = _stage_image()
    return build(4, 24, 1, diffs_of(a, 1), tables=(LONG,), rows=1, fill=pad % 3, com=bytes(pad))


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
    rng = np.random.default_rng(4157)
    cases = list(golden()[0])
    add = lambda name, buf, H, W, samples: cases.append(Case(name, bytes(buf), H, W, samples))
    # hand-made, valid
    a1, a3 = image("noise", 6, 10, 1, rng), image("noise", 5, 7, 3, rng)
    add("hand_flat_table", build(6, 10, 1, diffs_of(a1), tables=(FLAT5,)), 6, 10, 1)
    add("hand_nine_bit_codes", build(6, 10, 1, diffs_of(a1), tables=(NINE,)), 6, 10, 1)
    add("hand_sixteen_bit_codes", stage_stream(0), 4, 24, 1)
    add("hand_three_tables_0_1_2", build(5, 7, 3, diffs_of(a3, 2), tables=(K3, NINE, LONG), rows=2), 5, 7, 3)
    add("hand_three_tables_3_1_0", build(5, 7, 3, diffs_of(a3), tables={0: FLAT5, 1: K3, 3: NINE}, sel=[3, 1, 0]), 5, 7, 3)
    add("hand_grey_on_table_3", build(6, 10, 1, diffs_of(a1, 4), tables={3: K3}, rows=4), 6, 10, 1)
    add("hand_fill_before_rst", build(6, 10, 1, diffs_of(a1, 1), rows=1, fill=3), 6, 10, 1)
    ones = np.zeros((3, 40, 3), np.uint8)
    ones[:, ::2] = 255
    add("hand_stuffed_runs", build(3, 40, 3, diffs_of(ones), tables=(FLAT5,)), 3, 40, 3)
    add("hand_eleven_intervals", build(11, 3, 3, diffs_of(image("noise", 11, 3, 3, rng), 1), rows=1, fill=1), 11, 3, 3)
    add("hand_bytes_after_last_sample", build(6, 10, 1, diffs_of(a1), extra=b"\x12\x34\x00\x56"), 6, 10, 1)
    add("hand_no_eoi", build(6, 10, 1, diffs_of(a1, 2), rows=2, eoi=False), 6, 10, 1)
    add("hand_grey_sampling_ignored", build(6, 10, 1, diffs_of(a1), sampling=0x22), 6, 10, 1)
    add("hand_interval_above_h", build(6, 10, 1, diffs_of(a1), ri=70), 6, 10, 1)
    plain = build(6, 10, 1, diffs_of(a1))
    add("hand_com_app_dqt", b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes(9)) + _seg(0xDB, bytes(65)) + _seg(0xEC, b"x") + b"\xff\xff" + plain[2:], 6, 10, 1)
    add("hand_dri_zero", plain[:2] + _seg(0xDD, b"\x00\x00") + plain[2:], 6, 10, 1)
    for i, t in enumerate([K3, FLAT5, NINE, LONG]):                        # tables redefined between the frames of one batch
        add(f"hand_redefined_{i}", build(4, 6, 1, diffs_of(image("noise", 4, 6, 1, rng)), tables=(t,)), 4, 6, 1)
    # malformed: every status.  `good`: 4 x 6 grey, two rows an interval; `good3`: 4 x 6 x 3
    g1, g3 = image("noise", 4, 6, 1, rng), image("noise", 4, 6, 3, rng)
    good, good3 = build(4, 6, 1, diffs_of(g1, 2), rows=2), build(4, 6, 3, diffs_of(g3))
    add("hand_good", good, 4, 6, 1)
    add("hand_good3", good3, 4, 6, 3)
    dht = good.index(b"\xff\xc4")
    add("bad_no_soi", b"\x00" + good[1:], 4, 6, 1)
    add("bad_empty", b"", 4, 6, 1)
    add("bad_segment_past_frame", good[:dht + 2] + b"\xff\xff" + good[dht + 4:], 4, 6, 1)
    add("bad_segment_length_1", good[:dht + 2] + b"\x00\x01" + good[dht + 4:], 4, 6, 1)
    add("bad_sof3_twice", good[:dht] + good[2:dht] + good[dht:], 4, 6, 1)
    add("bad_sof3_short", _patch(good, 0xC3, 5, 2), 4, 6, 1)
    add("bad_size", good, 4, 7, 1)
    add("bad_rows", good, 5, 6, 1)
    add("bad_components", good, 4, 6, 3)
    add("bad_dht_class_1", _patch(good, 0xC4, 0, 0x10), 4, 6, 1)
    add("bad_dht_id_4", _patch(good, 0xC4, 0, 0x04), 4, 6, 1)
    add("bad_oversubscribed_dht", _patch(good, 0xC4, 1, 3), 4, 6, 1)
    add("bad_dht_cut_short", good.replace(_seg(0xC4, bytes([0]) + bytes(K3[0]) + bytes(K3[1])), _seg(0xC4, bytes([0]) + bytes(K3[0]) + bytes(K3[1][:5]))), 4, 6, 1)
    add("bad_dri_not_a_multiple_of_w", _patch(good, 0xDD, 1, 13), 4, 6, 1)
    add("bad_dri_length", good.replace(_seg(0xDD, b"\x00\x0c"), _seg(0xDD, b"\x00\x0c\x00")), 4, 6, 1)
    add("bad_undefined_table", _patch(good, 0xDA, 2, 0x10), 4, 6, 1)
    add("bad_table_id_4", _patch(good, 0xDA, 2, 0x40), 4, 6, 1)
    add("bad_no_huffman_table", good[:dht] + good[good.index(b"\xff\xdd"):], 4, 6, 1)
    add("bad_no_sos", good[:good.index(b"\xff\xda")] + b"\xff\xd9", 4, 6, 1)
    add("bad_sos_before_sof3", good[:2] + good[good.index(b"\xff\xda"):], 4, 6, 1)
    add("bad_scan_length", _patch(good3, 0xDA, 0, 1), 4, 6, 3)
    add("bad_garbage_between_segments", good[:2] + b"\x55" + good[2:], 4, 6, 1)
    for m in FRAME_MARKERS:
        add(f"refused_sof_{m:02x}", _patch(good, 0xC3, -1, m), 4, 6, 1)
    add("refused_dac", good[:2] + _seg(0xCC, b"\x00\x10") + good[2:], 4, 6, 1)
    add("refused_dnl", good[:2] + _seg(0xDC, b"\x00\x08") + good[2:], 4, 6, 1)
    add("refused_zero_lines", _patch(_patch(good, 0xC3, 1, 0), 0xC3, 2, 0), 4, 6, 1)
    add("refused_precision_12", build(4, 6, 1, diffs_of(g1), precision=12), 4, 6, 1)
    add("refused_precision_16", build(4, 6, 1, diffs_of(g1), precision=16), 4, 6, 1)
    add("refused_sampling_2x1", _patch(good3, 0xC3, 7, 0x21), 4, 6, 3)
    add("refused_sampling_chroma_1x2", _patch(good3, 0xC3, 10, 0x12), 4, 6, 3)
    for ss in (0, 2, 3, 4, 5, 6, 7, 8):
        add(f"refused_predictor_{ss}", build(4, 6, 1, diffs_of(g1), scan=(ss, 0, 0)), 4, 6, 1)
    add("refused_point_transform", build(4, 6, 1, diffs_of(g1), scan=(1, 0, 1)), 4, 6, 1)
    add("refused_se", build(4, 6, 1, diffs_of(g1), scan=(1, 63, 0)), 4, 6, 1)
    add("refused_ah", build(4, 6, 1, diffs_of(g1), scan=(1, 0, 0x10)), 4, 6, 1)
    sos = good3.index(b"\xff\xda")
    add("refused_scan_of_two", good3[:sos] + _seg(0xDA, bytes([2, 1, 0, 2, 0, 1, 0, 0])) + good3[sos + 14:], 4, 6, 3)
    add("refused_scan_order", _patch(good3, 0xDA, 1, 2), 4, 6, 3)
    head = lambda buf: buf[:buf.index(b"\xff\xda") + 10]                     # a grey stream up to its entropy data
    data = len(head(good))
    add("data_no_code", head(build(4, 6, 1, diffs_of(g1), tables=(SHORT,))) + b"\xff\x00" * 3 + b"\x00" * 40 + b"\xff\xd9", 4, 6, 1)
    add("data_category_17", head(build(4, 6, 1, [0] * 24, tables=(WITH_17,))) + bytes([17 << 3, 0, 0, 0]) + bytes(40) + b"\xff\xd9", 4, 6, 1)
    add("data_category_16", build(4, 6, 1, [0, 32768] + [0] * 22, tables=(FLAT5,)), 4, 6, 1)
    add("data_category_16_twice_is_still_outside", build(4, 6, 1, [0, 32768, 32768] + [0] * 21, tables=(FLAT5,)), 4, 6, 1)
    add("data_category_9", build(4, 6, 1, [-128, 256] + [0] * 22), 4, 6, 1)
    add("data_category_15", build(4, 6, 1, [0, -32767] + [0] * 22), 4, 6, 1)
    add("data_sample_256", build(4, 6, 1, [127, 1] + [0] * 22), 4, 6, 1)                  # (what a decoder that masks to 8 bits calls 0)
    add("data_sample_minus_1", build(4, 6, 1, [-128, 0, 0, -1] + [0] * 20), 4, 6, 1)      # (... and 255)
    add("data_first_column_outside", build(4, 6, 1, [0] * 6 + [100] + [0] * 5 + [100] + [0] * 11), 4, 6, 1)
    add("data_last_sample_outside", build(4, 6, 3, [0] * 71 + [200]), 4, 6, 3)
    add("data_missing_rst", good.replace(b"\xff\xd0", b"\x00\x00"), 4, 6, 1)
    add("data_wrong_rst_number", good.replace(b"\xff\xd0", b"\xff\xd1"), 4, 6, 1)
    add("data_extra_rst", good[:-2] + b"\xff\xd1\xff\xd9", 4, 6, 1)
    add("data_rst_without_dri", plain[:-2] + b"\xff\xd0\xff\xd9", 6, 10, 1)
    add("data_interval_ends_early", good[:good.index(b"\xff\xd0") - 4] + good[good.index(b"\xff\xd0"):], 4, 6, 1)
    add("data_marker_inside", good[:data + 1] + b"\xff\xd9" + good[data + 3:], 4, 6, 1)
    small = build(3, 4, 1, diffs_of(image("noise", 3, 4, 1, rng), 2), rows=2)
    for cut in range(len(small)):
        add(f"cut_after_{cut}", small[:cut], 3, 4, 1)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def expected():
    """{name: (array, status)} by the reference decoder"""
    return {c.name: reference_decode(c.buf, c.H, c.W, c.samples) for c in corpus()}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def categories(case):
    """the categories a valid stream of the corpus codes: the bit lengths of its array's differences (the restart rows from its DRI)"""
    arr, status = expected()[case.name]
    assert status == 0
    i = case.buf.find(b"\xff\xdd")
    rows = _u16(case.buf, i + 4) // case.W if 0 <= i < case.buf.index(b"\xff\xda") else 0
    return {abs(d).bit_length() for d in diffs_of(arr, rows)}


def write_corpus(path, cases=None, want=None):
    """corpus.bin for tests/csrc/verify_jpegll.cpp: uint32 count, then per case uint32 H, W, samples, len, status, the stream's bytes and
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
