"""DICOM RLE Lossless (tf_rle_decode, tf_hold_frames_rle, frames.rle_decode_frame, csrc/teeflow_rle_core.h): the corpus the CPU and the
GPU tests share, deterministic and seeded, and an independent decoder that says what each of its frames decodes to.  A helper module of
tests/test_rle_cpu.py and tests/test_gpu_rle.py: nothing here is collected.

The independent decoder (reference_decode) is written from PS3.5 Annex G, a byte at a time, as a decode-then-trim reader: it decodes a
whole segment, whatever follows the plane included, and keeps the first H * W bytes.  It is not the twin (frames.rle_decode_frame stops
at H * W bytes and clips); the two must agree on the whole corpus."""
import struct
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import frames as F

T = _lib.RLE_STAGE_BYTES             # the bytes of a segment k_rle_decode stages at a time (the library's tf_rle_stage_bytes())

# PackBits by hand: (segment bytes, what they decode to)
KNOWN = [
    (bytes([0xFE, 0x41]), b"AAA"),
    (bytes([0x02, 0x41, 0x42, 0x43]), b"ABC"),
    (bytes([0x80]), b""),
    (bytes([0x81, 0x58]), b"X" * 128),
    (bytes([0xFF, 0x59]), b"YY"),
    (bytes([0x7F]) + bytes(range(100, 228)), bytes(range(100, 228))),
]

# widths around 64 and 128 / 129 are where a lane round or the largest count can slip
SIZES = [(1, 1), (1, 2), (1, 129), (3, 5), (37, 53), (64, 64), (128, 130), (130, 257)]
FAMILIES = ("speckle", "sector", "constant", "alternating", "ramps")

Case = namedtuple("Case", "name buf H W samples")


# ---- the independent decoder --------------------------------------------------------------------------------------------------------
def reference_segment(seg):
    """every byte a PackBits segment decodes to, to its last byte"""
    out, i, n = bytearray(), 0, len(seg)
    while i < n:
        c = seg[i]
        i += 1
        if c <= 127:                                          # copy the next c + 1 bytes: those that are there
            for _ in range(c + 1):
                if i == n:
                    break
                out.append(seg[i])
                i += 1
        elif c >= 129:                                        # the next byte 257 - c times; nothing without it
            if i == n:
                break
            for _ in range(257 - c):
                out.append(seg[i])
            i += 1
    return bytes(out)


def reference_decode(buf, H, W, samples):
    """(uint8 [H,W,samples] -- [H,W] for one sample -- or None, status) of one frame"""
    n = len(buf)
    if n < 64 or struct.unpack_from("<I", buf, 0)[0] != samples:
        return None, 1
    offs = list(struct.unpack_from(f"<{samples}I", buf, 4))
    for k, o in enumerate(offs):
        if o < 64 or o >= n or (k and o <= offs[k - 1]):
            return None, 2
    planes = []
    for k, o in enumerate(offs):
        full = reference_segment(buf[o:offs[k + 1] if k + 1 < samples else n])
        if len(full) < H * W:
            return None, 3
        planes.append(np.frombuffer(full[:H * W], np.uint8).reshape(H, W))
    return (planes[0].copy() if samples == 1 else np.stack(planes, -1)), 0


# ---- frames to encode ---------------------------------------------------------------------------------------------------------------
def family_frame(family, H, W, samples, seed=0):
    rng = np.random.default_rng([FAMILIES.index(family), H, W, samples, seed])
    shape = (H, W, samples)
    if family == "speckle":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
    elif family == "sector":                                  # an ultrasound fan: speckle inside, black outside
        y, x = np.mgrid[0:H, 0:W]
        inside = (np.abs(x - (W - 1) / 2) <= 0.8 * (y + 1)) & ((x - (W - 1) / 2) ** 2 + y ** 2 <= (0.95 * H) ** 2 + 1)
        a = rng.integers(1, 256, shape, dtype=np.uint8) * inside[..., None].astype(np.uint8)
    elif family == "constant":
        a = np.full(shape, 200 + seed % 50, np.uint8)
    elif family == "alternating":                             # runs of two bytes: the densest stream of controls
        a = np.broadcast_to(((np.arange(H * W) // 2 % 2) * 90 + 10 + seed % 7).astype(np.uint8).reshape(H, W, 1), shape)
    else:                                                     # ramps: along the rows, down the columns, and slowly (runs of 3)
        y, x = np.mgrid[0:H, 0:W]
        a = np.stack([(x + seed) % 256, (y * 3) % 256, ((x + y) // 3) % 256][:samples], -1).astype(np.uint8)
    a = np.ascontiguousarray(a)
    return a[..., 0] if samples == 1 else a


def make_frame(segments, count=None, offsets=None, gaps=None, fill=0xA5):
    """header + segments by hand: `gaps[k]` bytes of `fill` in front of segment k (the first offset is then not 64); `count` and
    `offsets` overrule what the header would say"""
    gaps = gaps or [0] * len(segments)
    body, offs = b"", []
    for g, s in zip(gaps, segments):
        body += bytes([fill]) * g
        offs.append(64 + len(body))
        body += bytes(s)
    offs = list(offs if offsets is None else offsets)
    head = struct.pack("<16I", *([len(segments) if count is None else count] + offs + [0] * (15 - len(offs))))
    return head + body


def _lit(data):
    return bytes([len(data) - 1]) + bytes(data)


def _run(v, n):
    return bytes([257 - n, v])


def _hand_built():
    cases, rng = [], np.random.default_rng(25)
    px = bytes(rng.integers(0, 256, 15, dtype=np.uint8))      # a 3 x 5 plane
    streams = {                                               # (the short ones stand between good ones: a call meets them mid-way)
        "run_crosses_rows": _run(7, 15),
        "literal_cut_short": bytes([14]) + px[:10],           # asks for 15, 10 exist: short
        "literal_crosses_rows": _lit(px),
        "run_then_literal_cross": _run(9, 7) + _lit(px[:8]),
        "noops_between": b"\x80" + _run(9, 7) + b"\x80\x80" + _lit(px[:4]) + b"\x80" + _run(1, 4),
        "run_without_value": _run(2, 5) + b"\xf7",            # 5 bytes, then a run control and the segment's end: short
        "odd_then_pad": _run(3, 2) + _lit(px[:13]) + b"\x00",
        "garbage_after": _lit(px) + bytes(rng.integers(0, 256, 37, dtype=np.uint8)),
        "only_noops": b"\x80" * 9,
        "garbage_is_a_cut_literal": _run(4, 15) + b"\x7f\x01\x02",
        "garbage_is_a_lone_run": _lit(px) + b"\xf0",
        "overlong_run_is_clipped": _run(5, 128),
        "one_byte_short": _lit(px[:14]),
        "overlong_literal_is_clipped": _lit(bytes(range(40))),
        "literal_cut_but_enough": bytes([19]) + px,          # asks for 20 bytes, 15 exist: the plane is full
    }
    for name, s in streams.items():
        cases.append(Case("hand_" + name, make_frame([s]), 3, 5, 1))
    three = [streams["run_then_literal_cross"], streams["noops_between"], streams["odd_then_pad"]]
    cases.append(Case("hand_three_planes", make_frame(three), 3, 5, 3))
    cases.append(Case("hand_middle_plane_short", make_frame([three[0], streams["one_byte_short"], three[2]]), 3, 5, 3))
    for g in range(16):                                       # segment starts at every offset mod 16; a first offset that is not 64
        cases.append(Case(f"hand_gaps_{g}", make_frame(three, gaps=[g, (g * 7 + 3) % 16, 15 - g]), 3, 5, 3))
        if g == 0:
            cases.append(Case("hand_last_plane_short", make_frame([three[0], three[1], streams["run_without_value"]]), 3, 5, 3))
        cases.append(Case(f"hand_first_offset_{64 + g}", make_frame([streams["literal_crosses_rows"]], gaps=[g]), 3, 5, 1))
    return cases


def _malformed():
    cases = []
    good1, good3 = _run(7, 15), [_run(1, 15), _run(2, 15), _run(3, 15)]
    f1, f3 = make_frame([good1]), make_frame(good3)
    for n in (0, 1, 4, 63):                                   # status 1: shorter than a header
        cases.append(Case(f"bad_short_frame_{n}", f1[:n], 3, 5, 1))
    for count in (0, 2, 3, 16, 0xFFFFFFFF):                   # ... or a segment count that is not the sample count
        cases.append(Case(f"bad_count_{count}_for_1", make_frame([good1], count=count), 3, 5, 1))
    for count in (0, 1, 2, 4):
        cases.append(Case(f"bad_count_{count}_for_3", make_frame(good3, count=count), 3, 5, 3))
    n1, n3 = len(f1), len(f3)
    for o in (0, 4, 63, n1, n1 + 1, 0x80000000, 0xFFFFFFFF):  # status 2: an offset before the header's end or not inside the frame
        cases.append(Case(f"bad_offset_{o}_of_1", make_frame([good1], offsets=[o]), 3, 5, 1))
    for name, offs in (("first_low", [63, 66, 68]), ("second_low", [64, 10, 68]), ("third_low", [64, 66, 0]), ("equal", [64, 66, 66]),
                       ("all_equal", [64, 64, 64]), ("descending", [68, 66, 64]), ("swapped", [64, 68, 66]), ("last_at_end", [64, 66, n3]),
                       ("last_past_end", [64, 66, n3 + 5]), ("middle_huge", [64, 0xFFFFFFF0, 68])):
        cases.append(Case(f"bad_offsets_{name}", make_frame(good3, offsets=offs), 3, 5, 3))
    cases.append(Case("odd_offsets_still_ascending", make_frame(good3, offsets=[64, 65, n3 - 1]), 3, 5, 3))   # (valid offsets, short planes)
    # a short stream cut after each of its bytes: status 2 (no byte of the segment left), 3, or -- the pad alone missing -- still a plane
    px = bytes(range(50, 65))
    whole = make_frame([_run(9, 4) + b"\x80" + _lit(px[:6]) + _run(0, 5) + b"\x00"])
    for n in range(64, len(whole)):
        cases.append(Case(f"cut_after_{n}", whole[:n], 3, 5, 1))
    whole3 = make_frame([_run(9, 15), _lit(px), _run(8, 10) + _lit(px[:5])])
    for n in range(64, len(whole3)):
        cases.append(Case(f"cut3_after_{n}", whole3[:n], 3, 5, 3))
    return cases


def _stage_walk():
    """One stream behind k no-op bytes, k = 0 .. T + 1: a control byte last in a stage, a run's value byte first in the next, a literal
    across a refill, at every alignment"""
    rng = np.random.default_rng(7)
    lit = bytes(rng.integers(0, 256, 128, dtype=np.uint8))
    stream = _run(0xC3, 3) + _lit(lit) + _run(0x11, 69)      # 3 + 128 + 69 = the 200 bytes of a 2 x 100 plane
    return [Case(f"stage_noops_{k}", make_frame([b"\x80" * k + stream]), 2, 100, 1) for k in range(T + 2)]


@lru_cache(maxsize=None)
def encoded():
    """rle_encode_frame of every family at every size, 1 and 3 samples: [(Case, the frame that was encoded)]"""
    out = []
    for H, W in SIZES:
        for samples in (1, 3):
            for fam in FAMILIES:
                a = family_frame(fam, H, W, samples)
                out.append((Case(f"enc_{fam}_{H}x{W}x{samples}", F.rle_encode_frame(a), H, W, samples), a))
    return out


@lru_cache(maxsize=None)
def corpus():
    """every case, in one fixed order"""
    cases = [Case(f"known_{i}", make_frame([seg]), 1, max(len(want), 1), 1) for i, (seg, want) in enumerate(KNOWN)]
    return cases + [c for c, _ in encoded()] + _hand_built() + _malformed() + _stage_walk()


@lru_cache(maxsize=None)
def expected():
    """{case name: (array or None, status)} by the independent decoder, computed once"""
    return {c.name: reference_decode(c.buf, c.H, c.W, c.samples) for c in corpus()}


def by_shape():
    """the corpus grouped into calls: {(H, W, samples): [Case]}, a bad frame wherever it falls among the good ones"""
    groups = {}
    for c in corpus():
        groups.setdefault((c.H, c.W, c.samples), []).append(c)
    return groups


def study(family, N, H, W, samples, seed=0):
    """N frames of a family (the seed moves from frame to frame) and their RLE record: (uint8 [N,H,W] or [N,H,W,3], (blob, off, len))"""
    frames = np.stack([family_frame(family, H, W, samples, seed + i) for i in range(N)])
    return frames, F.rle_record([F.rle_encode_frame(f) for f in frames])


def write_corpus(path):
    """the corpus for tests/csrc/verify_rle.cpp: uint32 count, then per case uint32 H, W, samples, len, status, the frame's bytes and --
    status 0 -- the H * W * samples bytes it decodes to"""
    want = expected()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(corpus())))
        for c in corpus():
            arr, status = want[c.name]
            f.write(struct.pack("<5I", c.H, c.W, c.samples, len(c.buf), status) + c.buf)
            if status == 0:
                f.write(arr.tobytes())


# ---- the GPU cases (tests/test_gpu_rle.py runs `python -m tests.rle_cases` once, under a time limit; here every case has its own: a
# watchdog ends the process when a case is not done in CASE_SECONDS, whatever the main thread waits for) ----------------------------------
GPU_CASES = ["decode_corpus", "hold_equals_ingest", "study_call_and_otsu", "failed_hold_keeps_frames", "refusals", "junk_in_front"]
CASE_SECONDS = 60


def _record(cases):
    return F.rle_record([c.buf for c in cases])


def _case_decode_corpus(pkg, e):
    """rle_decode over the whole corpus, one call a shape: every array and status is the independent decoder's, a bad frame is zeros
    and leaves its neighbours valid"""
    want, middle = expected(), 0
    for (H, W, samples), cases in by_shape().items():
        got, status = e.rle_decode(_record(cases), H, W, samples)
        assert got.shape == (len(cases), H, W) + ((samples,) if samples > 1 else ()) and got.dtype == np.uint8 and status.dtype == np.int32
        for i, c in enumerate(cases):
            arr, st = want[c.name]
            assert status[i] == st, (c.name, int(status[i]), st)
            assert np.array_equal(got[i], arr) if st == 0 else not got[i].any(), c.name
        bad = np.flatnonzero(status)
        middle += sum(1 for i in bad if 0 < i < len(cases) - 1 and status[i - 1] == 0 and status[i + 1] == 0)
        blob = _record(cases)[0]
        assert e.counter("rle_bytes") == blob.size + got.size
    assert middle >= 3                                        # bad frames between good ones


def _case_hold_equals_ingest(pkg, e):
    """hold_frames_rle + download_frames == ingest_host(decoded, form, flip); the compressed bytes alone cross the bus"""
    sizes = [(1, 1), (1, 2), (1, 129), (3, 5), (37, 53), (64, 64), (128, 130)]
    for k, (H, W) in enumerate(sizes):
        N = 1 + k % 4
        for form in ("RGB", "GRAY", "YBR_FULL"):
            samples = 1 if form == "GRAY" else 3
            frames, rec = study(FAMILIES[k % 2], N, H, W, samples, seed=k)
            for flip in (False, True):
                up = e.counter("frames_upload_bytes")
                tok = e.hold_frames_rle(rec, H, W, samples, form, flip)
                assert tok.shape == (N, H, W, 3) and e.counter("frames_upload_bytes") - up == rec[0].size, (H, W, form, flip)
                assert np.array_equal(e.download_frames(), F.ingest_host(frames, form, flip)), (H, W, form, flip)
                assert e.counter("rle_bytes") == rec[0].size + frames.nbytes and e.counter("ingest_bytes") == frames.nbytes + 3 * N * H * W


def _case_study_call_and_otsu(pkg, e):
    """a study call and otsu_masks on the RLE token == the same calls on a hold_frames token of the decoded array, bit for bit"""
    from tests.frames_cases import speckle_source
    src = speckle_source("YBR_FULL", 6, 37, 53)
    rec = F.rle_record([F.rle_encode_frame(f) for f in src])
    tok = e.hold_frames(src, "YBR_FULL", True)
    want = e.calc_study_payload(tok, 2.0), e.otsu_masks(tok, 20), e.echo_frames(tok[1:4])
    rle_tok = e.hold_frames_rle(rec, 37, 53, 3, "YBR_FULL", True)
    assert rle_tok.generation > tok.generation
    up = e.counter("frames_upload_bytes")
    got = e.calc_study_payload(rle_tok, 2.0), e.otsu_masks(rle_tok, 20), e.echo_frames(rle_tok[1:4])
    assert e.counter("frames_upload_bytes") == up
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[0][1], want[0][1]) and np.abs(got[0][0].astype(np.float32)).max() > 0
    assert np.array_equal(got[1], want[1]) and got[1].any() and np.array_equal(got[2], want[2])


def _case_failed_hold_keeps_frames(pkg, e):
    """a hold_frames_rle that fails leaves the frames held before, their generation and a token of them working"""
    from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError
    frames, rec = study("sector", 3, 37, 53, 3)
    tok = e.hold_frames(frames, "RGB", True)
    held, echo = e.download_frames(), e.echo_frames(tok)
    good = [F.rle_encode_frame(f) for f in family_frame("speckle", 64, 64, 3)[None].repeat(3, 0)]
    bad = F.rle_record([good[0], good[1][:-100], good[2][:70]])           # the last plane short; the second offset behind the frame's end
    try:
        e.hold_frames_rle(bad, 64, 64, 3, "RGB")
        raise AssertionError("a record with two short frames was held")
    except OpticalFlowCalculationError as err:
        assert "frame 1 did not decode: status 3" in str(err) and "2 of 3 failed" in str(err), str(err)
    assert e._held_frames_shape() == (3, 37, 53, tok.generation)
    assert np.array_equal(e.download_frames(), held) and np.array_equal(e.echo_frames(tok), echo) and np.array_equal(e.echo_frames(tok[1:2]), echo[1:2])
    e.release_frames()                                        # ... and with nothing held before, nothing is held after
    try:
        e.hold_frames_rle(bad, 64, 64, 3, "RGB")
        raise AssertionError("a record with two short frames was held")
    except OpticalFlowCalculationError:
        assert e._held_frames_shape()[:3] == (0, 0, 0)


def _case_refusals(pkg, e):
    """what is refused is refused before any GPU work: nothing is uploaded, the held frames stay"""
    from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError
    frames, (blob, off, ln) = study("sector", 2, 3, 5, 3)
    tok = e.hold_frames_rle((blob, off, ln), 3, 5, 3, "RGB")
    up, L, h = e.counter("frames_upload_bytes"), e._L, e._h
    out, status = np.zeros(frames.size, np.uint8), np.zeros(2, np.int32)
    b, o, n = blob.ctypes.data, off.ctypes.data, ln.ctypes.data
    far = np.array([2 ** 63, 0], np.uint64)
    decode = lambda b=b, o=o, n=n, N=2, H=3, W=5, s=3, out=out.ctypes.data, st=status.ctypes.data: L.tf_rle_decode(h, b, o, n, N, H, W, s, out, st)
    hold = lambda b=b, o=o, n=n, N=2, H=3, W=5, s=3, form=0: L.tf_hold_frames_rle(h, b, o, n, N, H, W, s, form, 0, None)
    for rc in (decode(b=None), decode(o=None), decode(n=None), decode(out=None), decode(st=None), decode(N=0), decode(H=0), decode(W=-1), decode(s=2),
               decode(s=0), decode(s=4), decode(o=far.ctypes.data), decode(H=1 << 16, W=1 << 15),
               hold(b=None), hold(N=0), hold(s=1), hold(s=3, form=1), hold(s=1, form=2), hold(form=3), hold(form=-1), hold(o=far.ctypes.data)):
        assert rc == _lib.TF_ERR_INVALID_ARG
    assert b"overflows" in L.tf_last_error(h)
    assert e.counter("frames_upload_bytes") == up and not out.any() and not status.any()
    assert e._held_frames_shape() == (2, 3, 5, tok.generation) and np.array_equal(e.download_frames(), frames)
    for call in (lambda: e.hold_frames_rle((blob, off, ln), 3, 5, 3, "GRAY"), lambda: e.hold_frames_rle((blob, off, ln), 3, 5, 1, "RGB"),
                 lambda: e.hold_frames_rle((blob, off, ln), 3, 5, 3, "YBR"), lambda: e.rle_decode((blob[:10], off, ln), 3, 5, 3),
                 lambda: e.rle_decode((blob, off[:1], ln), 3, 5, 3), lambda: e.rle_decode((blob, off, ln), 0, 5, 3), lambda: e.rle_decode(blob, 3, 5, 3)):
        try:
            call()
            raise AssertionError("accepted")
        except OpticalFlowCalculationError:
            pass
    assert L.tf_abi_version() == 2


def _case_junk_in_front(pkg, e):
    """Three frames of the stage walk (k = T - 1, T, T + 1 no-ops: a refill is crossed) behind g junk bytes, g = 0 .. 15, as a file's
    pixel data has its frames at an unaligned offset: the span's first byte sits at every offset mod 16 of the blob, and the call
    gives the bits and statuses of g = 0 and uploads the frames' span, not the junk"""
    walk, want = _stage_walk(), expected()
    cases = [walk[k] for k in (T - 1, T, T + 1)]
    blob, off, ln = _record(cases)
    first = None
    for g in range(16):
        rec = (np.concatenate([np.full(g, 0x3C, np.uint8), blob]), off + np.uint64(g), ln)
        up = e.counter("frames_upload_bytes")
        got, status = e.rle_decode(rec, 2, 100, 1)
        assert e.counter("frames_upload_bytes") - up == blob.size, g
        if first is None:
            first = got, status
            assert not status.any() and all(np.array_equal(got[i], want[c.name][0]) for i, c in enumerate(cases))
        assert np.array_equal(got, first[0]) and np.array_equal(status, first[1]), g
    g = 11
    rec = (np.concatenate([np.full(g, 0x3C, np.uint8), blob]), off + np.uint64(g), ln)
    up = e.counter("frames_upload_bytes")
    tok = e.hold_frames_rle(rec, 2, 100, 1, "GRAY", True)
    assert tok.shape == (3, 2, 100, 3) and e.counter("frames_upload_bytes") - up == blob.size
    assert np.array_equal(e.download_frames(), F.ingest_host(first[0], "GRAY", True))


if __name__ == "__main__":
    import faulthandler
    import json
    import sys
    import time
    import tee_optical_flow_amd as pkg                                   # (T is the stage size)
    results = {}
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    e = pkg.DenseFlow(device_id=0, max_batch=3)
    for name in GPU_CASES:
        faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)          # this case's own time limit
        t0 = time.time()
        try:
            globals()["_case_" + name](pkg, e)
            outcome = "ok"
        except Exception:                                                # the parent test shows it
            import traceback
            outcome = traceback.format_exc()[-2500:]
        results[name] = (round(time.time() - t0, 2), outcome)
        print(json.dumps({name: results[name]}), flush=True)
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    e.close()
    faulthandler.cancel_dump_traceback_later()
    print(json.dumps(results))
