"""The cases of tests/test_gpu_segmentor_glue.py, run in ONE child process that imports torch before the engine's library is loaded:
torch and the library then share one HIP runtime, which passing device pointers between them needs (in the pytest process the library
has usually initialised HIP first, and the copy of the runtime torch brings along then sees no device).
    python -m tests.segmentor_glue_cases  ->  one JSON line {case id: [seconds, "ok" | traceback]}
A case that ends in anything but an AssertionError stops the run: the cases behind it are reported as not run."""
import json
import sys
import time
import traceback

import numpy as np

from tee_optical_flow_amd import masks
from tests.test_segmentor_glue_cpu import FakeSam, glue_fixture, twin_classmap

FX = glue_fixture()
CASES = []                                  # (id, function, arguments behind the engine)


def case(*params, ids=None):
    """register fn once, or once per parameter tuple"""
    def reg(fn):
        name = fn.__name__
        if not params:
            CASES.append((name, fn, ()))
        for p in params:
            p = p if isinstance(p, tuple) else (p,)
            tag = "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in p)
            CASES.append((f"{name}[{tag}]", fn, p))
        return fn
    return reg


class Patch:
    """with Patch(cls, name, wrapper): cls.name replaced for the block"""

    def __init__(self, cls, name, new):
        self.cls, self.name, self.new = cls, name, new

    def __enter__(self):
        self.old = getattr(self.cls, self.name)
        setattr(self.cls, self.name, self.new)

    def __exit__(self, *exc):
        setattr(self.cls, self.name, self.old)


def raises(exc, fn):
    try:
        fn()
    except exc as e:
        return e
    raise AssertionError(f"{exc.__name__} was not raised")


def _contents(seed, N, H, W):
    """frames cycling through random bytes, all 255, all 0 and a 1-pixel checkerboard"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    kinds = [lambda: rng.integers(0, 256, (H, W, 3), dtype=np.uint8), lambda: np.full((H, W, 3), 255, np.uint8),
             lambda: np.zeros((H, W, 3), np.uint8), lambda: np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)]
    return np.stack([kinds[i % 4]() for i in range(N)])


def _want_input(frames, size):
    lut = masks.segmentor_lut()
    r = np.stack([masks.pil_resize_bilinear(f, size) for f in frames])
    return np.stack([lut[c][r[..., c]] for c in range(3)], axis=1)


def _check_input(x, frames, size, dev=0):
    import torch
    assert isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.device == torch.device("cuda", dev) and x.is_contiguous()
    assert tuple(x.shape) == (frames.shape[0], 3) + tuple(size)
    assert np.array_equal(x.cpu().numpy(), _want_input(frames, size))


@case(*sorted(FX["in"]))
def input_equals_fixture(engine, name):
    frames, resized = FX["in"][name]
    lut = masks.segmentor_lut()
    x = engine.segmentor_input(frames, resized.shape[1:3])
    want = np.stack([lut[c][resized[..., c]] for c in range(3)], axis=1)       # PIL's bytes through the table
    assert np.array_equal(x.cpu().numpy(), want)
    _check_input(x, frames, resized.shape[1:3])


@case(
    (4, (37, 53), (64, 64)),                # upscale, odd sizes
    (4, (96, 80), (64, 64)),                # downscale, ksize 5
    (4, (50, 64), (64, 64)),                # the horizontal pass keeps its length
    (4, (1, 7), (16, 16)),                  # a one-row frame
    (4, (33, 31), (30, 30)),                # out_w % 4 != 0: element stores
    (4, (64, 48), (61, 70)),                # ... with one axis up and one down
    (2, (512, 512), (1024, 1024)),
    (1, (600, 800), (1024, 1024)),
    (1, (1080, 1920), (1024, 1024)),
)
def input_equals_twin(engine, N, src, dst):
    frames = _contents(src[0] + src[1] + N, N, *src)
    _check_input(engine.segmentor_input(frames, dst), frames, dst)


@case()
def input_checkerboard_and_random_at_the_real_target(engine):
    frames = _contents(5, 4, 128, 160)[[3, 0]]
    _check_input(engine.segmentor_input(frames, (1024, 1024)), frames, (1024, 1024))


@case()
def input_reuses_out_across_calls(engine):
    import torch
    a, b = _contents(1, 5, 37, 53), _contents(2, 5, 37, 53)[::-1].copy()
    out = torch.full((5, 3, 64, 64), float("nan"), device="cuda:0")
    xa = engine.segmentor_input(a, (64, 64), out=out)
    assert xa.data_ptr() == out.data_ptr()
    got_a = xa.cpu().numpy()
    xb = engine.segmentor_input(b, (64, 64), out=out)
    assert xb.data_ptr() == out.data_ptr()
    assert np.array_equal(got_a, _want_input(a, (64, 64))) and np.array_equal(xb.cpu().numpy(), _want_input(b, (64, 64)))
    big = torch.full((8, 3, 64, 64), -7.0, device="cuda:0")                     # room to spare: the first N frames are written
    xs = engine.segmentor_input(a[:3], (64, 64), out=big)
    assert xs.data_ptr() == big.data_ptr() and tuple(xs.shape) == (3, 3, 64, 64)
    assert np.array_equal(xs.cpu().numpy(), _want_input(a[:3], (64, 64))) and bool((big[3:] == -7.0).all())
    other = engine.segmentor_input(a, (32, 32), out=out)                        # an `out` of another shape is not used
    assert other.data_ptr() != out.data_ptr()
    _check_input(other, a, (32, 32))


@case()
def input_is_ordered_on_torchs_current_stream(engine):
    """work queued on the caller's stream after the call reads the finished tensor, on a side stream and on the default one"""
    import torch
    frames = _contents(9, 3, 96, 80)
    want = _want_input(frames, (128, 128))
    s = torch.cuda.Stream(0)
    with torch.cuda.stream(s):
        y = engine.segmentor_input(frames, (128, 128)) * 2.0
    s.synchronize()
    assert np.array_equal(y.cpu().numpy(), want * np.float32(2.0))
    z = engine.segmentor_input(frames, (128, 128)) + 1.0
    assert np.array_equal(z.cpu().numpy(), want + np.float32(1.0))


@case()
def glue_on_a_deepflow_handle(engine):
    import torch
    import tee_optical_flow_amd as T
    frames = _contents(4, 3, 96, 80)
    logits, cmap = FX["cm"]["odd"]
    deep = T.DenseFlow(device_id=0, algo="deepflow")
    try:
        _check_input(deep.segmentor_input(frames, (64, 64)), frames, (64, 64))
        assert np.array_equal(deep.segmentor_classmap(torch.from_numpy(logits).cuda(), cmap.shape[1:]), cmap)
    finally:
        deep.close()


@case(*sorted(FX["cm"]))
def classmap_equals_fixture(engine, name):
    import torch
    logits, cmap = FX["cm"][name]
    got = engine.segmentor_classmap(torch.from_numpy(logits).cuda(), cmap.shape[1:])
    assert got.dtype == np.uint8 and got.shape == cmap.shape and np.array_equal(got, cmap)
    assert np.array_equal(got, twin_classmap(logits, cmap.shape[1:]))


def _logits(seed, n, C, h, w):
    """few distinct values (exact ties at most pixels), with +-inf and NaN at chosen classes"""
    rng = np.random.default_rng(seed)
    a = (rng.integers(-3, 4, (n, C, h, w)) / 4.0).astype(np.float32)
    a[0, 0, ::5, ::3] = np.inf
    a[0, C - 1, 1::5, ::3] = np.inf
    a[0, C // 2, 2::5, ::3] = -np.inf
    a[-1, C - 1, ::4, 1::4] = np.nan
    a[-1, 0, ::8, 1::4] = np.nan                                                # two NaNs at one pixel: the first wins
    return a


@case(*[(C, src, dst) for C in (1, 3, 9, 256) for src, dst in (((256, 256), (512, 512)), ((256, 256), (600, 800)), ((256, 256), (37, 53)),
                                                               ((4, 4), (1, 1)), ((64, 64), (25, 100)))])
def classmap_equals_twin(engine, C, src, dst):
    import torch
    n = 1 if C == 256 else 2
    logits = _logits(C + src[0] + dst[1], n, C, *src)
    got = engine.segmentor_classmap(torch.from_numpy(logits).cuda(), dst)
    want = twin_classmap(logits, dst)
    assert got.dtype == np.uint8 and got.shape == (n,) + dst and np.array_equal(got, want)
    if C > 1 and src[0] > 4:
        assert len(np.unique(want)) > 1


@case()
def classmap_of_equal_logits_is_all_zero(engine):
    import torch
    for v in (0.0, -2.5, float("inf"), float("-inf"), float("nan")):
        got = engine.segmentor_classmap(torch.full((2, 9, 64, 64), v, device="cuda:0"), (37, 53))
        assert got.shape == (2, 37, 53) and not got.any(), v


@case()
def classmap_equals_torch_argmax_on_the_cpu(engine):
    """the argmax rule itself, against torch's on the CPU (what the reference runs after .cpu()): ties, infinities, NaN"""
    import torch
    logits = _logits(77, 3, 9, 64, 64)
    want = torch.from_numpy(logits).argmax(dim=1).numpy().astype(np.uint8)
    assert np.array_equal(engine.segmentor_classmap(torch.from_numpy(logits).cuda(), (64, 64)), want)     # same size: every index is its own


@case()
def classmap_takes_float16_and_strided_logits(engine):
    import torch
    logits = _logits(5, 2, 9, 64, 64)
    half = torch.from_numpy(logits).cuda().half()
    assert np.array_equal(engine.segmentor_classmap(half, (25, 100)), twin_classmap(half.float().cpu().numpy(), (25, 100)))
    strided = torch.from_numpy(np.ascontiguousarray(logits.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)      # channels last
    assert not strided.is_contiguous()
    assert np.array_equal(engine.segmentor_classmap(strided, (25, 100)), twin_classmap(logits, (25, 100)))
    from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError
    raises(OpticalFlowCalculationError, lambda: engine.segmentor_classmap(torch.from_numpy(logits), (25, 100)))    # CPU logits


@case()
def error_paths_leave_the_engine_working(engine):
    import torch
    from tee_optical_flow_amd import _lib
    from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError
    from tee_optical_flow_amd.synth import speckle_pair
    I0, I1, _ = speckle_pair(3, 64, 64)
    before = engine.calc(I0, I1, None).copy()
    bad = [
        (lambda: engine.segmentor_classmap(torch.zeros((1, 257, 4, 4), device="cuda:0"), (4, 4)), _lib.TF_ERR_UNSUPPORTED),
        (lambda: engine.segmentor_classmap(torch.zeros((1, 3, 4, 4), device="cuda:0"), (0, 4)), _lib.TF_ERR_INVALID_ARG),
        (lambda: engine.segmentor_classmap(torch.zeros((0, 3, 4, 4), device="cuda:0"), (4, 4)), _lib.TF_ERR_INVALID_ARG),
        (lambda: engine.segmentor_input(np.zeros((0, 8, 8, 3), np.uint8), (16, 16)), _lib.TF_ERR_INVALID_ARG),
        (lambda: engine.segmentor_input(np.zeros((2, 8, 8, 3), np.uint8), (16, 0)), _lib.TF_ERR_INVALID_ARG),
        (lambda: engine.segmentor_input(np.zeros((2, 8, 0, 3), np.uint8), (16, 16)), _lib.TF_ERR_INVALID_ARG),
    ]
    for call, code in bad:
        assert raises(OpticalFlowCalculationError, call).code == code
        assert np.array_equal(engine.calc(I0, I1, None), before)
    frames = _contents(8, 2, 20, 24)
    _check_input(engine.segmentor_input(frames, (32, 32)), frames, (32, 32))


def _study(seed, N, H, W):
    from tee_optical_flow_amd.synth import speckle_sequence
    rng = np.random.default_rng(seed)
    g = speckle_sequence(seed, N, H, W).astype(np.int16)
    return np.stack([np.clip(g + rng.integers(-12, 13, g.shape, dtype=np.int16), 0, 255).astype(np.uint8) for _ in range(3)], axis=-1)


def _same_masks(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@case((5, 64, 64), (3, 96, 128))
def predict_movie_on_the_device_equals_the_host(engine, N, H, W):
    """chunk=2: a chunk boundary and a short last chunk"""
    import tee_optical_flow_amd as T
    nparr = _study(N + H, N, H, W)
    want = masks.predict_movie(nparr, FakeSam(), mode="RVIO_2class")
    calls = []
    real = T.DenseFlow.segmentor_input
    with Patch(T.DenseFlow, "segmentor_input", lambda self, fr, *a, **k: (calls.append(fr.shape[0]), real(self, fr, *a, **k))[1]):
        got = masks.predict_movie(nparr, FakeSam("cuda:0"), mode="RVIO_2class", engine=engine, chunk=2)
    assert calls == [2] * (N // 2) + [1]
    _same_masks(got, want)
    assert want["rv"].any() and want["av"].any() and want["bkgd"].any()
    _same_masks(masks.predict_movie(nparr, FakeSam("cuda:0"), mode="RVIO_2class", engine=engine), want)        # the default chunk: one call


@case()
def predict_movie_beside_a_submitted_study(engine):
    """a study submitted (tf_submit_seq_rgb) and still in flight on the engine's lanes, the segmentor masks made on the same engine
    before the wait: masks and flows equal their separate runs"""
    import tee_optical_flow_amd as T
    nparr = _study(21, 5, 64, 64)
    study = _study(22, 24, 256, 256)
    want = masks.predict_movie(nparr, FakeSam(), mode="RVIO_2class")
    eng = T.DenseFlow(device_id=0)
    try:
        alone = eng.calc_study(study).copy()
        t = eng.submit_study(study)
        got = masks.predict_movie(nparr, FakeSam("cuda:0"), mode="RVIO_2class", engine=eng, chunk=2)
        flows = np.array(eng.wait(t))
    finally:
        eng.close()
    _same_masks(got, want)
    assert np.array_equal(flows, alone)


@case()
def a_cpu_model_stays_on_the_host_path(engine):
    import tee_optical_flow_amd as T
    nparr = _study(31, 4, 64, 64)
    calls = []
    real = T.DenseFlow.segmentor_input
    want = masks.predict_movie(nparr, FakeSam(), mode="RVIO_2class")
    with Patch(T.DenseFlow, "segmentor_input", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1]):
        _same_masks(masks.predict_movie(nparr, FakeSam(), mode="RVIO_2class", engine=engine), want)
    assert calls == []


def main():
    import torch                                                                # before the engine's library: one HIP runtime for both
    assert torch.cuda.is_available(), "torch sees no GPU"
    torch.zeros(1, device="cuda:0")
    import tee_optical_flow_amd as T
    engine = T.DenseFlow(device_id=0)
    out, stopped = {}, None
    for name, fn, args in CASES:
        if stopped:
            out[name] = [0.0, f"not run: {stopped} ended in an error that is no assertion"]
            continue
        t = time.perf_counter()
        try:
            fn(engine, *args)
            res = "ok"
        except AssertionError:
            res = traceback.format_exc()
        except BaseException:                                                   # a HIP error, a crash of the layer: nothing more on the GPU
            res = traceback.format_exc()
            stopped = name
        out[name] = [round(time.perf_counter() - t, 3), res]
    if not stopped:
        engine.close()
    print(json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
