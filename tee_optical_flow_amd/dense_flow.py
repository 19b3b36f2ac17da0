"""`DenseFlow`: the object that takes the place of cv2's DenseOpticalFlow on the reference's hot path.

Reference call sites it is a drop-in for (/root/reference/optical_flow/calculate_optical_flow.py):
  :577  OF_model = cv2.optflow.createOptFlow_DualTVL1()        -> createOptFlow_DualTVL1()
  :575  OF_model = cv2.cuda.OpticalFlowDual_TVL1.create()      -> createOptFlow_DualTVL1()
  :578  OF_model.setLambda(config.lambda_value)                -> DenseFlow.setLambda
  :631/:638/:642  flow = OF_model.calc(I0, I1, None)           -> DenseFlow.calc

Same protocol: `calc(I0: uint8[H,W], I1: uint8[H,W], None) -> float32[H,W,2]`, the 12 cv2 getters/setters,
not re-entrant, result owned by the caller.  Everything is computed by hand-written HIP kernels through the
C ABI in include/teeflow.h; there is no CPU path.
"""
import ctypes as C
import weakref
from collections import namedtuple
from functools import partial

import numpy as np

from . import _lib
from .exceptions import OpticalFlowCalculationError


def _u8_image_stack(a, name, ndim, allow_f32=False):
    a = np.asarray(a)
    if a.dtype != np.uint8 and not (allow_f32 and a.dtype == np.float32):
        raise OpticalFlowCalculationError(f"{name} must be uint8 (CV_8UC1){' or float32 (CV_32FC1)' if allow_f32 else ''}, got {a.dtype}")
    if a.ndim != ndim:
        raise OpticalFlowCalculationError(f"{name} must have {ndim} dimensions, got shape {a.shape}")
    return np.ascontiguousarray(a)


def _chain_stacks(stacks, name, ndim):
    """The arrays of a lock-step call (calc_chains & co.): a non-empty list of uint8 arrays of `ndim` dimensions -- [N,H,W] frames, or
    [N,H,W,3] RGB studies -- each of N >= 2 frames, all of one frame size -> (C-contiguous arrays, H, W)"""
    if isinstance(stacks, np.ndarray) or not isinstance(stacks, (list, tuple)) or len(stacks) < 1:
        raise OpticalFlowCalculationError(f"{name} must be a non-empty list of arrays, one per chain")
    out = [_u8_image_stack(a, f"{name}[{i}]", ndim) for i, a in enumerate(stacks)]
    for i, a in enumerate(out):
        if a.shape[0] < 2:
            raise OpticalFlowCalculationError(f"{name}[{i}] has {a.shape[0]} frame(s): a chain needs at least 2 frames")
        if ndim == 4 and a.shape[3] != 3:
            raise OpticalFlowCalculationError(f"{name}[{i}] must be [N,H,W,3], got {a.shape}")
        if a.shape[1:] != out[0].shape[1:] or min(a.shape) < 1:
            raise OpticalFlowCalculationError(f"chains in lock-step need one frame size: {name}[{i}] is {a.shape[1:3]}, {name}[0] is "
                                              f"{out[0].shape[1:3]}")
    return out, out[0].shape[1], out[0].shape[2]


def _mask_stack(a, name):
    """bool or uint8 [N,H,W,C], C = 1 or 2, as C-contiguous uint8 (a bool array is viewed, not copied)"""
    a = np.asarray(a)
    if a.dtype not in (np.bool_, np.uint8):
        raise OpticalFlowCalculationError(f"{name} must be bool or uint8, got {a.dtype}")
    if a.ndim != 4 or a.shape[3] not in (1, 2) or min(a.shape) < 1:
        raise OpticalFlowCalculationError(f"{name} must be [N,H,W,C] with C = 1 or 2 and no empty side, got shape {a.shape}")
    return np.ascontiguousarray(a).view(np.uint8)


# What a call leaves to be collected (at once, or by wait()): the result array, the frame count whose last flow is repeated (0: no
# repeat), what the caller gets after the flows (a study's echo -- an array or None -- and / or its backgrounds), and the input arrays
# the library reads until then
_Job = namedtuple("_Job", "out pad_n extra inputs", defaults=(0, (), ()))


# What DenseFlow.held reports of the study held on the device: the flow's frames and size, the echo's frames (0: none), the generation
# (it grows with every replacement and release) and {label: (n_frames, C)} of the held masks
HeldShape = namedtuple("HeldShape", "N H W n_echo generation masks")


class HeldFrames:
    """What DenseFlow.hold_frames returns: the token of the RGB frames held on the engine's device -- their count and size, and the
    generation they were held under.  Every method that takes `nparr` or `frames` takes the token in their place and reads the held
    frames where they are; `token[a:b]` is the token of frames [a, b).  Once the engine holds other frames, or none (hold_frames again,
    release_frames, close), the token is stale and a call that gets it raises OpticalFlowCalculationError."""
    dtype, ndim = np.dtype(np.uint8), 4

    def __init__(self, engine, N, H, W, generation, first=0, count=None):
        self._engine = weakref.ref(engine)
        self.N, self.H, self.W, self.generation, self.first = int(N), int(H), int(W), int(generation), int(first)
        self.count = self.N if count is None else int(count)

    @property
    def shape(self):
        return (self.count, self.H, self.W, 3)

    def __len__(self):
        return self.count

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise OpticalFlowCalculationError(f"held frames take a frame range token[a:b], got {key!r}")
        a, b, step = key.indices(self.count)
        if step != 1 or b <= a:
            raise OpticalFlowCalculationError(f"held frames take a non-empty contiguous frame range, got {key!r} of {self.count} frames")
        return HeldFrames(self._engine(), self.N, self.H, self.W, self.generation, self.first + a, b - a)

    def checked(self, engine, held, min_frames=1):
        """This token, for a call of `engine`, which now holds `held` = (N, H, W, generation) (N == 0: nothing): raises where the token
        is another engine's, stale, or shorter than the call's `min_frames`.  No device call."""
        N, H, W, gen = held
        if self._engine() is not engine:
            raise OpticalFlowCalculationError(f"{self!r} belongs to another engine")
        if gen != self.generation or N < 1:
            raise OpticalFlowCalculationError(f"{self!r} is stale: the engine now holds " +
                                              (f"{N} x {H} x {W} frames of generation {gen}" if N else "no frames"))
        if self.count < min_frames:
            raise OpticalFlowCalculationError(f"the call needs at least {min_frames} frames, got {self!r}")
        return self

    def __repr__(self):
        return f"HeldFrames(frames [{self.first}, {self.first + self.count}) of {self.N} x {self.H} x {self.W} x 3, generation {self.generation})"


class _HeldLabels:
    """The mask labels of one held study and the library's mask slots they sit in, in the order they came; they belong to one
    generation of the held study and are forgotten with it."""

    def __init__(self, n_slots=_lib.HELD_SLOTS):
        self.n_slots, self.generation, self.slots = n_slots, None, {}

    def sync(self, generation):
        """forget the labels of a study that has been replaced or released since"""
        if generation != self.generation:
            self.generation, self.slots = generation, {}

    def slot_for(self, label):
        """the slot a mask under `label` goes to: the label's own, or the next free one; one label more than there are slots raises"""
        if label not in self.slots:
            if len(self.slots) >= self.n_slots:
                raise OpticalFlowCalculationError(f"a held study takes {self.n_slots} masks; no slot left for label {label!r} "
                                                  f"(held: {list(self.slots)})")
            self.slots[label] = len(self.slots)
        return self.slots[label]

    def slot_of(self, label):
        if label not in self.slots:
            raise OpticalFlowCalculationError(f"no mask is held under label {label!r} (held: {list(self.slots)})")
        return self.slots[label]


class _PinnedPool:
    """Result arrays backed by pinned host memory (tf_host_alloc): the library then copies flows out at PCIe speed while
    the next sub-batch is still being solved.  A buffer returns to the pool when the numpy array that owns it is garbage
    collected (the caller still gets a fresh array per call, like cv2), so a steady stream of equally sized calls
    allocates nothing."""

    def __init__(self, L, keep_bytes=2 << 30):
        self._L, self._free, self._kept, self._keep = L, {}, 0, keep_bytes
        self.closed = False

    def empty(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if n == 0:
            return np.empty(shape, dtype)
        lst = self._free.get(n)
        if lst:
            ptr = lst.pop()
            self._kept -= n
        else:
            ptr = self._L.tf_host_alloc(n)
            if not ptr:
                return np.empty(shape, dtype)            # pinning refused (limits): pageable memory still works
        raw = (C.c_char * n).from_address(ptr)
        weakref.finalize(raw, self._give_back, ptr, n).atexit = False    # at interpreter exit the process frees it
        return np.frombuffer(raw, dtype=dtype).reshape(shape)

    def _give_back(self, ptr, n):
        if self.closed or self._kept + n > self._keep:
            self._L.tf_host_free(ptr)
        else:
            self._free.setdefault(n, []).append(ptr)
            self._kept += n

    def close(self):
        self.closed = True
        for lst in self._free.values():
            for ptr in lst:
                self._L.tf_host_free(ptr)
        self._free, self._kept = {}, 0


class DenseFlow:
    """MI355X DualTVL1 solver with the cv2.DenseOpticalFlow calling convention."""

    device_unit_scale = True        # calc_study(scale=, pad_last=) applies the unit scale in the output kernel (pipeline.flow_for_study)
    device_payload = True           # calc_study_payload & co. hand over the study file's float16 `flow` and `echo` (process_folder(payload="device"))
    device_chain = True             # calc_batch, calc_seq_device, submit_batch, submit_seq_device and every study form take chain=True (after setUseInitialFlow(True))
    device_chains = True            # calc_chains, calc_chains_device and calc_study_chains{,_payload} solve several chains of one frame size in lock-step
    device_study_chunks = True      # study_chunks solves an RGB study into its `flow` and `echo` gzip-9 chunks, no float16 array downloaded (process_folder(deflate="device"))
    device_wase = True              # calc_study_wase & co. solve and compensate a bkgd_comp="WASE" study in one call, float32 or float16

    _SETTERS = {"Tau": "tau", "Lambda": "lambda", "Theta": "theta", "ScalesNumber": "nscales",
                "WarpingsNumber": "warps", "Epsilon": "epsilon", "InnerIterations": "inner_iterations",
                "OuterIterations": "outer_iterations", "ScaleStep": "scale_step", "Gamma": "gamma",
                "MedianFiltering": "median_filtering", "UseInitialFlow": "use_initial_flow"}

    def __init__(self, device_id=0, max_batch=128, algo="TVL1", **params):
        self._L = _lib.load()
        self._pool = _PinnedPool(self._L)
        self._jobs = {}                                    # ticket -> what a submitted job reads and writes (kept alive until wait)
        self._held_labels = _HeldLabels()                  # mask label -> slot of the study held on the device
        self.algo = algo
        if algo == "deepflow":
            p, create = _lib.TfDeepflowParams(), "tf_create_deepflow"
            _lib.check(self._L.tf_default_deepflow_params(C.byref(p)), None, "tf_default_deepflow_params")
            p.max_batch = int(max_batch)
            for k, v in params.items():
                if not hasattr(p, k):
                    raise OpticalFlowCalculationError(f"unknown DeepFlow parameter {k!r}")
                setattr(p, k, v)
        elif algo == "TVL1":
            p, create = _lib.TfParams(), "tf_create"
            _lib.check(self._L.tf_default_params(C.byref(p)), None, "tf_default_params")
            p.max_batch = int(max_batch)
            variant = params.pop("variant", "cpu")
            if variant not in ("cpu", "cuda", 0, 1):
                raise OpticalFlowCalculationError(f"variant must be 'cpu' or 'cuda', got {variant!r}")
            p.variant = 1 if variant in ("cuda", 1) else 0          # TF_VARIANT_CUDA: cv2.cuda.OpticalFlowDual_TVL1 semantics (row a5)
            for k, v in params.items():
                key = "lambda_" if k in ("lambda", "lambda_") else k
                if not hasattr(p, key):
                    raise OpticalFlowCalculationError(f"unknown DualTVL1 parameter {k!r}")
                setattr(p, key, v)
        else:
            raise OpticalFlowCalculationError("OF_algo only supports deepflow or TVL1")
        h = C.c_void_p()
        _lib.check(getattr(self._L, create)(C.byref(p), int(device_id), C.byref(h)), None, create)
        self._h = h
        self.device_id = int(device_id)
        self.last_stats = None

    # ---- lifetime ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_pool", None):
            self._pool.close()
        if getattr(self, "_h", None):
            self._L.tf_destroy(self._h)                    # jobs still queued are finished first
            self._h = None
        self._jobs = {}

    def _out(self, shape):
        """A fresh float32 result array (pinned host memory from the pool)."""
        return self._pool.empty(shape, np.float32)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the 12 cv2 setters/getters (setLambda is the one the reference calls, :578) -------------
    def _set(self, key, value):
        _lib.check(self._L.tf_set_param(self._h, _lib.PARAM_KEYS[key], float(value)), self._h, f"set {key}")

    def _get(self, key):
        v = C.c_double()
        _lib.check(self._L.tf_get_param(self._h, _lib.PARAM_KEYS[key], C.byref(v)), self._h, f"get {key}")
        return v.value

    def __getattr__(self, name):
        if name.startswith(("set", "get")) and name[3:] in DenseFlow._SETTERS:
            key = DenseFlow._SETTERS[name[3:]]
            is_int = key in ("nscales", "warps", "inner_iterations", "outer_iterations", "median_filtering")
            if name.startswith("set"):
                return lambda v: self._set(key, v)
            if key == "use_initial_flow":
                return lambda: bool(self._get(key))
            return (lambda: int(self._get(key))) if is_int else (lambda: self._get(key))
        raise AttributeError(name)

    # ---- engine controls -----------------------------------------------------------------------
    def set_stream(self, hip_stream_ptr, external=True):
        """Run on a caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream, 0 = legacy default stream);
        external=False returns to the handle's own non-blocking stream."""
        _lib.check(self._L.tf_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0), 1 if external else 0), self._h, "tf_set_stream")

    def set_profile(self, level):
        _lib.check(self._L.tf_set_profile(self._h, int(level)), self._h, "tf_set_profile")

    def set_tuning(self, name, value):
        """Implementation knobs (never change results), e.g. iter_variant, min_rows_work, warp_margin, lanes, sor_coop; the full list is
        tf_set_tuning's in include/teeflow.h.  An unknown name raises."""
        _lib.check(self._L.tf_set_tuning(self._h, name.encode(), int(value)), self._h, "tf_set_tuning")

    def counter(self, name):
        """Debug counters of the engine (tf_dbg_counter): coop_launches, coop_aborts, coop_disabled, coop_rearms, coop_cooldown, coop_occ16, coop_occ8,
        queue_jobs, queue_units_done, queue_units_skipped, queue_outstanding, queue_lanes, stream_retries, streams_serialised, chain_steps,
        saliency_kernel_us, wase_study_kernel_us (device time of the last WASE study call's reduction and output kernels),
        inflate_kernel_us, unchunk_kernel_us (device time of k_inflate / k_unchunk since the engine was made),
        deflate_match_us, deflate_emit_us, chunk_kernel_us (device time of deflate's links and match search, of its parse, trees, bits and
        compaction, and of k_chunk, since the engine was made), deflate_batches (the batches of chunks deflate has worked through),
        study_download_bytes (bytes of flow and echo the study calls have
        copied to the host; calc_study_held and study_chunks add nothing), tail_upload_bytes."""
        return int(self._L.tf_dbg_counter(self._h, name.encode()))

    def _raise_unless_verdict(self, rc, status, fn):
        """inflate's and rle_decode's rule: a code other than TF_OK beside all-zero statuses is no verdict on a stream or a frame -- the
        call itself failed, and raises; with a status set, the statuses are the answer."""
        if rc != _lib.TF_OK and not status.any():
            _lib.check(rc, self._h, fn)

    def _finish(self, st, chain_pairs=None):
        self.last_stats = st.as_dict()
        self._last_chain_pairs = chain_pairs               # a lock-step call: the pairs of each chain, in the caller's order

    def last_iters(self):
        """Executed (inner, outer) iteration counts of the last call: int32 [pairs, levels, warps, 2]; after a lock-step call
        (calc_chains & co.) a list of such arrays, one per chain in the order the chains were passed."""
        s = self.last_stats
        n = s["n_pairs"] * s["nscales_used"] * s["warps"] * 2
        out = np.zeros(n, np.int32)
        w = C.c_size_t()
        _lib.check(self._L.tf_get_iters(self._h, out.ctypes.data_as(C.c_void_p), n, C.byref(w)), self._h, "tf_get_iters")
        out = out.reshape(s["n_pairs"], s["nscales_used"], s["warps"], 2)
        if getattr(self, "_last_chain_pairs", None):
            return np.split(out, np.cumsum(self._last_chain_pairs)[:-1])
        return out

    # ---- cv2 protocol --------------------------------------------------------------------------
    def _initial_flows(self, init, shape, name):
        """The initial flows of a pairs call as the library reads them, or None where it reads none.  getUseInitialFlow() decides, as
        in cv2: off, whatever was passed is ignored; on, `init` must be a float32-convertible array of `shape` = the frames' + (2,),
        x then y displacement in pixels per frame."""
        if self.algo != "TVL1" or not self.getUseInitialFlow():
            return None
        if init is None:
            raise OpticalFlowCalculationError(f"useInitialFlow is set: {name} must be the initial flow, got None")
        try:
            init = np.ascontiguousarray(init, dtype=np.float32)
        except (TypeError, ValueError) as e:
            raise OpticalFlowCalculationError(f"{name} must be convertible to float32: {e}") from None
        if init.shape != tuple(shape):
            raise OpticalFlowCalculationError(f"{name} must be float32 {list(shape)} (the frames' size, x and y), got shape {init.shape}")
        return init

    def calc(self, I0, I1, flow=None):
        """flow = OF_model.calc(I0, I1, None): uint8 [H,W] x2 -> float32 [H,W,2] (x, y displacement).  float32 frames
        (CV_32FC1) are accepted like cv2 does: DualTVL1 scales values in [0,1] by 255, DeepFlow takes them as they are.
        `flow` is read only after setUseInitialFlow(True), as in cv2: the solve then starts from it (float32 [H,W,2], pixels per frame)
        and None raises.  It is never written: the result is a fresh array."""
        I0 = _u8_image_stack(I0, "I0", 2, allow_f32=True)
        I1 = _u8_image_stack(I1, "I1", 2, allow_f32=True)
        if I0.shape != I1.shape or I0.dtype != I1.dtype:
            raise OpticalFlowCalculationError(f"I0 and I1 differ: {I0.shape} {I0.dtype} vs {I1.shape} {I1.dtype}")
        H, W = I0.shape
        init = self._initial_flows(flow, (H, W, 2), "flow")
        out = self._out((H, W, 2))
        st = _lib.TfStats()
        if init is not None:
            _lib.check(self._L.tf_calc_pairs_init(self._h, I0.ctypes.data, I1.ctypes.data, int(I0.dtype == np.float32), init.ctypes.data, 1, H, W,
                                                  out.ctypes.data, C.byref(st)), self._h, "tf_calc_pairs_init")
        else:
            fn = self._L.tf_calc_pair_f32 if I0.dtype == np.float32 else self._L.tf_calc_pair
            _lib.check(fn(self._h, I0.ctypes.data, I1.ctypes.data, H, W, out.ctypes.data, C.byref(st)), self._h, "tf_calc_pair")
        self._finish(st)
        return out

    # ---- batched forms (the data-parallel path the reference lacks) ------------------------------
    def chain_next(self, on=True):
        """Arm (or disarm) the next solve call, a sequence or study call, to be solved as a chain: what chain=True does.  Needs
        setUseInitialFlow(True) on a DualTVL1 model of the CPU form; the library spends the flag on the next solve call, whatever becomes
        of it, and refuses an armed pairs call."""
        _lib.check(self._L.tf_chain_next(self._h, 1 if on else 0), self._h, "tf_chain_next")

    def calc_batch(self, frames, scale=1.0, chain=False):
        """frames uint8 [N,H,W] -> float32 [N-1,H,W,2]: flow(frame i -> i+1) * scale (reference loop :584-597).
        `chain` (after setUseInitialFlow(True)): the video idiom `flow = calc(frames[k], frames[k+1], flow)` in one call -- pair 0 starts
        from zero, pair k from pair k-1's unscaled float32 flow -- with the bits and iteration counts of that loop.  The pairs are solved
        one after the other on the device: expect about N-1 single-pair solves, several times the batched call."""
        frames = _u8_image_stack(frames, "frames", 3)
        N, H, W = frames.shape
        if N < 2:
            raise OpticalFlowCalculationError("need at least 2 frames")
        out = self._out((N - 1, H, W, 2))
        st = _lib.TfStats()
        if chain:
            self.chain_next()
        _lib.check(self._L.tf_calc_seq(self._h, frames.ctypes.data, N, H, W, float(scale), out.ctypes.data, C.byref(st)),
                   self._h, "tf_calc_seq")
        self._finish(st)
        return out

    # ---- several chains of one frame size in lock-step (include/teeflow.h, tf_calc_chains): step k solves pair k of every chain still
    # running as one batch.  After setUseInitialFlow(True), like chain=True; last_iters() then returns one array per chain ---------------
    def _chains_call(self, fn, srcs, n_frames, H, W, own, dsts):
        """one lock-step call: the per-chain pointer arrays, the C function `fn`, its own arguments between the sizes and the outputs"""
        S = len(srcs)
        st = _lib.TfStats()
        ptrs = lambda ps: (C.c_void_p * S)(*ps)
        _lib.check(getattr(self._L, fn)(self._h, ptrs(srcs), (C.c_int * S)(*n_frames), S, int(H), int(W), *own, *(ptrs(d) if d is not None else None for d in dsts),
                                        C.byref(st)), self._h, fn)
        self._finish(st, [int(n) - 1 for n in n_frames])

    def calc_chains(self, list_of_frames, scale=1.0):
        """A list of uint8 [N_s,H,W] frame stacks of one H x W (the N_s may differ) -> a list of float32 [N_s-1,H,W,2]: each what
        calc_batch(frames, scale, chain=True) gives for it, bits and iteration counts, but solved together -- step k solves pair k of
        every chain that still has one as a single batch, so the launches that one pair cannot fill carry one pair per chain.  At most
        max_batch chains per call."""
        frs, H, W = _chain_stacks(list_of_frames, "list_of_frames", 3)
        outs = [self._out((len(f) - 1, H, W, 2)) for f in frs]
        self._chains_call("tf_calc_chains", [f.ctypes.data for f in frs], [len(f) for f in frs], H, W, (float(scale),), ([o.ctypes.data for o in outs],))
        return outs

    def calc_chains_device(self, dframes_ptrs, n_frames, H, W, dflow_ptrs, scale=1.0):
        """tf_calc_chains_device: calc_chains on raw device pointers, one per chain -- frames uint8 [n_frames[s],H,W], flows float32
        [n_frames[s]-1,H,W,2] * scale, written where dflow_ptrs[s] points."""
        if len(dframes_ptrs) < 1 or not len(dframes_ptrs) == len(n_frames) == len(dflow_ptrs):
            raise OpticalFlowCalculationError("calc_chains_device needs one frame pointer, frame count and flow pointer per chain, at least one chain")
        if min(int(n) for n in n_frames) < 2:
            raise OpticalFlowCalculationError("a chain needs at least 2 frames")
        self._chains_call("tf_calc_chains_device", list(dframes_ptrs), list(n_frames), H, W, (float(scale),), (list(dflow_ptrs),))
        return self.last_stats

    def _study_chains(self, list_of_rgb, scale, pad_last, f16, echo):
        studies, H, W = _chain_stacks(list_of_rgb, "list_of_rgb", 4)
        ns = [len(s) for s in studies]
        outs = [self._pool.empty((n if pad_last else n - 1, H, W, 2), np.float16 if f16 else np.float32) for n in ns]
        echos = [self._pool.empty((n, H, W), np.float16) for n in ns] if echo else None
        self._chains_call("tf_calc_chains_rgb", [s.ctypes.data for s in studies], ns, H, W, (float(scale), int(f16)),
                          ([o.ctypes.data for o in outs], [e.ctypes.data for e in echos] if echo else None))
        jobs = [_Job(o, n if pad_last else 0, ((echos[i] if echo else None,) if f16 else ())) for i, (o, n) in enumerate(zip(outs, ns))]
        return [self._collect(j) for j in jobs]

    def calc_study_chains(self, list_of_rgb, scale=1.0, pad_last=False):
        """A list of RGB studies uint8 [N_s,H,W,3] of one H x W -> a list of float32 arrays, each what calc_study(study, scale, pad_last,
        chain=True) gives for it: the studies' chains are solved in lock-step (calc_chains)."""
        return self._study_chains(list_of_rgb, scale, pad_last, False, False)

    def calc_study_chains_payload(self, list_of_rgb, scale=1.0, pad_last=True, echo=True):
        """calc_study_chains with the study file's float16 payload: -> a list of (flow16, echo16 | None), each what
        calc_study_payload(study, scale, pad_last, echo, chain=True) gives for it.  Holds nothing on the device."""
        return self._study_chains(list_of_rgb, scale, pad_last, True, echo)

    # ---- frames held on the device (tf_hold_frames): ingested once in the form the file stores, read in place by every call below that
    # takes `nparr` or `frames` ------------------------------------------------------------------------------------------------------------
    def _held_frames_shape(self):
        out = (C.c_longlong * 4)()
        _lib.check(self._L.tf_held_frames_shape(self._h, C.byref(out)), self._h, "tf_held_frames_shape")
        return tuple(int(v) for v in out)

    def hold_frames(self, arr, form="RGB", flip=False):
        """Puts a study's frames on the device once, as the file stores them: uint8 "RGB" [N,H,W,3], "GRAY" [N,H,W] (gray2rgb on the
        device) or "YBR_FULL" [N,H,W,3] of Y, Cb, Cr (pydicom's pixel_array for YBR_FULL and YBR_FULL_422; converted on the device, bit
        for bit frames.ybr_full_to_rgb); `flip`: columns mirrored (np.flip(axis=2), the reference's flipLR).  What is held is
        frames.ingest_host(arr, form, flip).  -> the HeldFrames token that stands for these frames in calc_study*, submit_study*,
        calc_study_held, study_chunks, otsu_masks, segmentor_input, saliency_frames, echo_frames and condition_frames.  Replaces the
        frames held before (their tokens go stale); a held study is untouched."""
        if form not in _lib.FRAMES_FORMS:
            raise OpticalFlowCalculationError(f"form must be one of {tuple(_lib.FRAMES_FORMS)}, got {form!r}")
        a = _u8_image_stack(arr, "arr", 3 if form == "GRAY" else 4)
        if (form != "GRAY" and a.shape[3] != 3) or min(a.shape) < 1:
            raise OpticalFlowCalculationError(f"{form} frames must be {'[N,H,W]' if form == 'GRAY' else '[N,H,W,3]'} with no empty side, got {a.shape}")
        N, H, W = a.shape[:3]
        _lib.check(self._L.tf_hold_frames(self._h, a.ctypes.data, _lib.FRAMES_FORMS[form], 1 if flip else 0, N, H, W), self._h, "tf_hold_frames")
        return HeldFrames(self, N, H, W, self._held_frames_shape()[3])

    def download_frames(self):
        """The held frames as uint8 RGB [N,H,W,3] on the host (for a host segmentor or host Otsu: the conversion has still left the host)."""
        N, H, W, _ = self._held_frames_shape()
        if N < 1:
            raise OpticalFlowCalculationError("no frames are held (hold_frames)")
        out = np.empty((N, H, W, 3), np.uint8)
        _lib.check(self._L.tf_download_frames(self._h, out.ctypes.data), self._h, "tf_download_frames")
        return out

    def release_frames(self):
        """Frees the held frames; their tokens go stale."""
        _lib.check(self._L.tf_release_frames(self._h), self._h, "tf_release_frames")

    # ---- DICOM RLE Lossless pixel data (tf_rle_decode, tf_hold_frames_rle): the PackBits segments are decoded on the device, one wave per
    # (frame, segment); frames.rle_decode_frame is the twin, frames.rle_record makes the record ------------------------------------------
    @staticmethod
    def _rle_record(record, H, W, samples):
        """(blob, off, len) of frames.rle_record, checked -> the three C-contiguous arrays and the sizes as ints"""
        try:
            blob, off, ln = record
        except (TypeError, ValueError):
            raise OpticalFlowCalculationError("an RLE record is (blob, off, len), as frames.rle_record makes it") from None
        blob = np.ascontiguousarray(blob, np.uint8).reshape(-1)
        off, ln = np.ascontiguousarray(off, np.uint64).reshape(-1), np.ascontiguousarray(ln, np.uint32).reshape(-1)
        H, W, samples = int(H), int(W), int(samples)
        if off.shape != ln.shape or off.size < 1 or off.size > 2 ** 31 - 1:
            raise OpticalFlowCalculationError(f"an RLE record needs one off and one len per frame and at least one frame, got {off.size} and {ln.size}")
        if H < 1 or W < 1 or H * W > 2 ** 30 or samples not in (1, 3):
            raise OpticalFlowCalculationError(f"RLE frames are H x W x samples with H, W >= 1, H * W <= 2^30 and samples 1 or 3, got {H} x {W} x {samples}")
        if max(int(o) + int(n) for o, n in zip(off, ln)) > blob.size:
            raise OpticalFlowCalculationError(f"RLE record: a frame ends behind the blob's {blob.size} bytes")
        if blob.size == 0:
            blob = np.zeros(1, np.uint8)
        return blob, off, ln, H, W, samples

    def rle_decode(self, record, H, W, samples):
        """RLE Lossless frames -- record = (blob, off, len), frame i the len[i] bytes at blob[off[i]:] (frames.rle_record) -- of H x W
        pixels of `samples` (1 or 3) 8-bit samples -> (uint8 [N,H,W,samples], or [N,H,W] for samples == 1; status int32 [N]).  A status
        is 0, 1 bad header, 2 bad offsets or 3 a segment decoded short (frames.rle_decode_frame has the rules); the call does not raise
        for a frame that does not decode: its status says so and its frame is zeros.  A call that fails as a whole -- refused
        arguments, a HIP error -- raises."""
        blob, off, ln, H, W, samples = self._rle_record(record, H, W, samples)
        N = off.size
        out = np.zeros((N, H, W) if samples == 1 else (N, H, W, samples), np.uint8)
        status = np.zeros(N, np.int32)
        rc = self._L.tf_rle_decode(self._h, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, N, H, W, samples, out.ctypes.data, status.ctypes.data)
        self._raise_unless_verdict(rc, status, "tf_rle_decode")
        return out, status

    def hold_frames_rle(self, record, H, W, samples, form="RGB", flip=False):
        """hold_frames from RLE Lossless pixel data as the file stores it: record = (blob, off, len) (frames.rle_record, or
        pipeline.dicom_rle_frames' fields), H x W pixels of `samples` 8-bit samples -- 1 for form "GRAY", 3 for "RGB" and "YBR_FULL".
        Only the compressed bytes are uploaded; the device decodes them and ingests the planes as hold_frames ingests `form` and `flip`.
        -> the HeldFrames token; what is held is frames.ingest_host(decoded, form, flip).  If a frame does not decode the call raises
        with the first bad frame and its status, and the frames held before, their generation and their tokens stay as they were."""
        if form not in _lib.FRAMES_FORMS:
            raise OpticalFlowCalculationError(f"form must be one of {tuple(_lib.FRAMES_FORMS)}, got {form!r}")
        blob, off, ln, H, W, samples = self._rle_record(record, H, W, samples)
        if samples != (1 if form == "GRAY" else 3):
            raise OpticalFlowCalculationError(f"{form} frames have {1 if form == 'GRAY' else 3} samples a pixel, got samples = {samples}")
        N = off.size
        status = np.zeros(N, np.int32)
        _lib.check(self._L.tf_hold_frames_rle(self._h, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, N, H, W, samples, _lib.FRAMES_FORMS[form],
                                              1 if flip else 0, status.ctypes.data), self._h, "tf_hold_frames_rle")
        return HeldFrames(self, N, H, W, self._held_frames_shape()[3])

    # ---- DICOM JPEG Baseline pixel data (tf_jpeg_decode, tf_hold_frames_jpeg): Huffman decode, dequantisation, IDCT and chroma upsampling
    # on the device; frames.jpeg_decode_frame is the twin, frames.jpeg_record makes the record --------------------------------------------
    @staticmethod
    def _jpeg_record(record, H, W, samples):
        """(blob, off, len) of frames.jpeg_record, checked -> the three C-contiguous arrays and the sizes as ints"""
        H, W = int(H), int(W)
        if H > 65535 or W > 65535:
            raise OpticalFlowCalculationError(f"a JPEG frame has at most 65535 rows and columns, got {H} x {W}")
        return DenseFlow._rle_record(record, H, W, samples)

    def jpeg_decode(self, record, H, W, samples):
        """JPEG Baseline frames -- record = (blob, off, len), frame i the len[i] bytes at blob[off[i]:] (frames.jpeg_record), each a full
        interchange stream -- of H x W pixels of `samples` (1 or 3) components -> (uint8 [N,H,W,samples], or [N,H,W] for samples == 1;
        status int32 [N]): the stream's own components, upsampled, no colour transform; on a valid stream what libjpeg-turbo gives.  A
        status is 0, 1 bad header, 2 a process that is not decoded or 3 entropy data that does not decode (frames.jpeg_decode_frame has
        the rules); the call does not raise for a frame that does not decode: its status says so and its frame is zeros.  A call that
        fails as a whole -- refused arguments, a HIP error -- raises."""
        blob, off, ln, H, W, samples = self._jpeg_record(record, H, W, samples)
        N = off.size
        out = np.zeros((N, H, W) if samples == 1 else (N, H, W, samples), np.uint8)
        status = np.zeros(N, np.int32)
        rc = self._L.tf_jpeg_decode(self._h, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, N, H, W, samples, out.ctypes.data, status.ctypes.data)
        self._raise_unless_verdict(rc, status, "tf_jpeg_decode")
        return out, status

    def hold_frames_jpeg(self, record, H, W, samples, form="RGB", color="none", flip=False):
        """hold_frames from JPEG Baseline pixel data as the file stores it: record = (blob, off, len) (frames.jpeg_record, or
        pipeline.dicom_jpeg_frames' fields), H x W pixels of `samples` components -- 1 for form "GRAY", 3 for "RGB" and "YBR_FULL".  Only
        the compressed bytes are uploaded.  color "none": the decoded samples are ingested as hold_frames ingests `form` and `flip`, and
        what is held is frames.ingest_host(decoded, form, flip).  color "libjpeg" (form "YBR_FULL"): Y, Cb, Cr go through libjpeg's
        colour tables, and what is held is frames.ingest_host(frames.ycc_to_rgb_libjpeg(decoded), "RGB", flip): the RGB a Pillow-backed
        reader returns.  -> the HeldFrames token.  If a frame does not decode the call raises with the first bad frame and its status, and
        the frames held before, their generation and their tokens stay as they were."""
        if form not in _lib.FRAMES_FORMS:
            raise OpticalFlowCalculationError(f"form must be one of {tuple(_lib.FRAMES_FORMS)}, got {form!r}")
        if color not in _lib.JPEG_COLORS:
            raise OpticalFlowCalculationError(f"color must be one of {tuple(_lib.JPEG_COLORS)}, got {color!r}")
        if color == "libjpeg" and form != "YBR_FULL":
            raise OpticalFlowCalculationError(f"color 'libjpeg' converts Y, Cb, Cr: it needs form 'YBR_FULL', got {form!r}")
        blob, off, ln, H, W, samples = self._jpeg_record(record, H, W, samples)
        if samples != (1 if form == "GRAY" else 3):
            raise OpticalFlowCalculationError(f"{form} frames have {1 if form == 'GRAY' else 3} samples a pixel, got samples = {samples}")
        N = off.size
        status = np.zeros(N, np.int32)
        _lib.check(self._L.tf_hold_frames_jpeg(self._h, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, N, H, W, samples, _lib.FRAMES_FORMS[form],
                                               _lib.JPEG_COLORS[color], 1 if flip else 0, status.ctypes.data), self._h, "tf_hold_frames_jpeg")
        return HeldFrames(self, N, H, W, self._held_frames_shape()[3])

    # ---- DICOM JPEG Lossless pixel data (SOF3, predictor 1; tf_jpegll_decode, tf_hold_frames_jpegll): the Huffman decode emits
    # prediction differences, the reconstruction is prefix sums on the device; frames.jpegll_decode_frame is the twin ------------------------
    def jpeg_lossless_decode(self, record, H, W, samples):
        """JPEG Lossless frames -- record = (blob, off, len), frame i the len[i] bytes at blob[off[i]:] (frames.jpegll_record), each a
        full interchange stream with an SOF3 frame header and predictor 1 -- of H x W pixels of `samples` (1 or 3) components -> (uint8
        [N,H,W,samples], or [N,H,W] for samples == 1; status int32 [N]): the encoded array, no colour transform.  A status is 0, 1 bad
        header, 2 a process that is not decoded or 3 data that does not decode, a sample outside 0..255 included
        (frames.jpegll_decode_frame has the rules); the call does not raise for a frame that does not decode: its status says so and
        its frame is zeros.  A call that fails as a whole -- refused arguments, a HIP error -- raises."""
        blob, off, ln, H, W, samples = self._jpeg_record(record, H, W, samples)
        N = off.size
        out = np.zeros((N, H, W) if samples == 1 else (N, H, W, samples), np.uint8)
        status = np.zeros(N, np.int32)
        rc = self._L.tf_jpegll_decode(self._h, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, N, H, W, samples, out.ctypes.data, status.ctypes.data)
        self._raise_unless_verdict(rc, status, "tf_jpegll_decode")
        return out, status

    def hold_frames_jpeg_lossless(self, record, H, W, samples, form="RGB", flip=False):
        """hold_frames from JPEG Lossless pixel data as the file stores it: record = (blob, off, len) (frames.jpegll_record, or
        pipeline.dicom_jpegll_frames' fields), H x W pixels of `samples` components -- 1 for form "GRAY", 3 for "RGB" and "YBR_FULL".
        Only the compressed bytes are uploaded; the codec applies no colour transform, and what is held is
        frames.ingest_host(decoded, form, flip).  -> the HeldFrames token.  If a frame does not decode the call raises with the first bad
        frame and its status, and the frames held before, their generation and their tokens stay as they were."""
        if form not in _lib.FRAMES_FORMS:
            raise OpticalFlowCalculationError(f"form must be one of {tuple(_lib.FRAMES_FORMS)}, got {form!r}")
        blob, off, ln, H, W, samples = self._jpeg_record(record, H, W, samples)
        if samples != (1 if form == "GRAY" else 3):
            raise OpticalFlowCalculationError(f"{form} frames have {1 if form == 'GRAY' else 3} samples a pixel, got samples = {samples}")
        N = off.size
        status = np.zeros(N, np.int32)
        _lib.check(self._L.tf_hold_frames_jpegll(self._h, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, N, H, W, samples, _lib.FRAMES_FORMS[form],
                                                 1 if flip else 0, status.ctypes.data), self._h, "tf_hold_frames_jpegll")
        return HeldFrames(self, N, H, W, self._held_frames_shape()[3])

    def _frames_in(self, frames, check, min_frames=1):
        """A method's `nparr` / `frames` argument: an array goes through `check`; a HeldFrames token is checked for being this engine's
        current frames and comes back as it is (it has the array's .shape).  Nothing is armed yet: _frames_ptr does that."""
        if not isinstance(frames, HeldFrames):
            return check(frames)
        return frames.checked(self, self._held_frames_shape(), min_frames)

    def _frames_ptr(self, frames):
        """The frame pointer of the C call that follows at once: an array's data, or None behind tf_frames_next for a token."""
        if not isinstance(frames, HeldFrames):
            return frames.ctypes.data
        _lib.check(self._L.tf_frames_next(self._h, frames.first, frames.count), self._h, "tf_frames_next")
        return None

    @staticmethod
    def _rgb_frames(nparr):
        nparr = _u8_image_stack(nparr, "nparr", 4)
        if nparr.shape[3] != 3:
            raise OpticalFlowCalculationError(f"nparr must be [N,H,W,3], got {nparr.shape}")
        return nparr

    def condition_frames(self, nparr):
        """Device version of frames.condition_frames: uint8 [N,H,W,3] (or a HeldFrames token) -> uint8 [N,H,W] =
        img2uint8(rgb2gray(frame)) per frame."""
        nparr = self._frames_in(nparr, self._rgb_frames)
        N, H, W, _ = nparr.shape
        out = np.empty((N, H, W), np.uint8)
        _lib.check(self._L.tf_condition_frames(self._h, self._frames_ptr(nparr), N, H, W, out.ctypes.data), self._h, "tf_condition_frames")
        return out

    # ---- a study: RGB frames in, the study file's `flow` array out.  The ten public forms below are cells of one grid -- the solver's
    # frames (conditioned gray | saliency maps) x the output (float32 | the file's float16 payload, with its echo) x the compensation
    # (none | WASE) x the collection (waited for | submitted) -- and _study is the one path through it -----------------------------------
    @staticmethod
    def _rgb_study(nparr, min_frames=2, channels=(3,)):
        nparr = _u8_image_stack(nparr, "nparr", 4)
        if nparr.shape[3] not in channels or nparr.shape[0] < min_frames:
            raise OpticalFlowCalculationError(f"nparr must be [N>={min_frames},H,W,3], got {nparr.shape}")
        return nparr

    def _study(self, nparr, scale, pad_last, *, saliency=False, map_dtype="f32", f16=False, echo=False, bkgd_mask=None, submit=False,
               hold=False, chain=False):
        """One study call: the frame check, the pinned outputs, the C function of the cell and its arguments.  -> what _collect makes of
        the job, or (`submit`) the ticket wait() collects it by.  Only the float32 saliency form takes one-channel frames.  `hold` (the
        float16 forms that are waited for): the call also leaves its payload held on the device (hold_study's doc).  `chain` (every
        cell, after setUseInitialFlow(True)): the study's pairs are solved as a chain (calc_batch's doc)."""
        wase = bkgd_mask is not None
        if hold and (submit or not f16):
            raise OpticalFlowCalculationError("only a float16 study call that is waited for can leave its payload held")
        nparr = self._frames_in(nparr, partial(self._rgb_study, channels=(1, 3) if saliency and not (f16 or wase) else (3,)), 2)
        N, H, W, ch = nparr.shape
        if wase:
            mask = np.ascontiguousarray(bkgd_mask)
            if mask.dtype != np.bool_ or mask.ndim != 4 or mask.shape[0] < 1 or mask.shape[1:] != (H, W, 2):
                raise OpticalFlowCalculationError(f"bkgd mask must be bool [n>=1,{H},{W},2], got {mask.dtype} {mask.shape}")
        if submit and (saliency or wase):
            raise OpticalFlowCalculationError("only a study without saliency and background compensation can be submitted")
        out = self._pool.empty((N if pad_last else N - 1, H, W, 2), np.float16 if f16 else np.float32)
        e16 = self._pool.empty((N, H, W), np.float16) if echo else None
        bg = np.empty(N - 1, np.float32) if wase else None
        st, t = _lib.TfStats(), C.c_int(-1)
        map_f32 = saliency and self._map_is_f32(map_dtype)
        e, last = e16.ctypes.data if echo else None, C.byref(t) if submit else C.byref(st)
        # tf_{calc,submit}_seq_{rgb,saliency}{,_f32,_f16,_wase}(h, frames, N, H, W[, channels[, map_f32]], <the form's own>)
        if wase:
            form, own = "_wase", (mask.view(np.uint8).ctypes.data, mask.shape[0], float(scale), int(f16), out.ctypes.data, e, bg.ctypes.data, last)
        elif f16:
            form, own = "_f16", (float(scale), out.ctypes.data, e, last)
        else:
            form, own = "_f32" if map_f32 else "", (float(scale), out.ctypes.data, last)
        name = ("tf_submit_seq_" if submit else "tf_calc_seq_") + ("saliency" if saliency else "rgb") + form
        sizes = (N, H, W)
        if saliency:
            sizes += (ch, int(map_f32)) if f16 or wase else (ch,)
        if chain:
            self.chain_next()                              # (first: a refusal here leaves nothing else armed)
        if hold:
            self.hold_next()
        _lib.check(getattr(self._L, name)(self._h, self._frames_ptr(nparr), *sizes, *own), self._h, name)
        job = _Job(out, N if pad_last else 0, ((e16,) if f16 else ()) + ((bg,) if wase else ()))
        if submit:
            self._jobs[t.value] = job
            return t.value
        self._finish(st)
        return self._collect(job)

    @staticmethod
    def _collect(job):
        """What a finished job returns: its result array, the last flow repeated (reference :599) inside the pinned buffer where that was
        asked for -- alone, or a study's (out, echo), (out, bg) or (out, echo, bg)."""
        if job.pad_n:
            job.out[job.pad_n - 1] = job.out[job.pad_n - 2]
        return (job.out,) + job.extra if job.extra else job.out

    def calc_study(self, nparr, scale=1.0, pad_last=False, chain=False):
        """RGB study uint8 [N,H,W,3] -> float32 [N-1,H,W,2]: conditioning and all pair solves stay on the device.
        `pad_last`: the result is [N,H,W,2] with the last flow repeated (reference :599) -- written into one pinned buffer, no
        concatenate on the host; with `scale` = pixel_spacing * frame_rate this is the study's whole flow array (:600).
        `chain` (this and every other study form, after setUseInitialFlow(True)): each pair starts from the flow before it, as in
        calc_batch."""
        return self._study(nparr, scale, pad_last, chain=chain)

    # ---- the study file's float16 payload, made on the device (reference :400-404 casts on the host at write time) -------------
    def echo_frames(self, nparr):
        """The study file's `echo` dataset on the device: RGB frames uint8 [N,H,W,3] -> float16 [N,H,W] =
        frames.rgb2gray(nparr).astype(np.float16), bit for bit (the float64 luma rounded once to half)."""
        nparr = self._frames_in(nparr, partial(self._rgb_study, min_frames=1))
        N, H, W, _ = nparr.shape
        out = self._pool.empty((N, H, W), np.float16)
        _lib.check(self._L.tf_echo_frames(self._h, self._frames_ptr(nparr), N, H, W, out.ctypes.data), self._h, "tf_echo_frames")
        return out

    def calc_study_payload(self, nparr, scale=1.0, pad_last=True, echo=True, hold=False, chain=False):
        """calc_study with the flows rounded to float16 by the output kernel: RGB study uint8 [N,H,W,3] -> (flow16, echo16).  flow16 has
        the bits of calc_study(nparr, scale, pad_last).astype(np.float16) -- the study file's `flow` dataset with `scale` = pixel_spacing
        * frame_rate and `pad_last` -- at half the download; echo16 is echo_frames(nparr), made from the same upload, or None.
        `hold`: the payload (all N flow frames, the last one repeated whatever `pad_last`; the echo if made) also stays held on the
        device, as after hold_study of the returned arrays, without being uploaded again; the returned arrays are the same."""
        return self._study(nparr, scale, pad_last, f16=True, echo=echo, hold=hold, chain=chain)

    def calc_study_saliency_payload(self, nparr, scale=1.0, pad_last=True, echo=True, map_dtype="f32", hold=False, chain=False):
        """calc_study_saliency with float16 flows, and the `echo` of the RGB frames: -> (flow16, echo16 | None), as calc_study_payload."""
        return self._study(nparr, scale, pad_last, saliency=True, map_dtype=map_dtype, f16=True, echo=echo, hold=hold, chain=chain)

    def submit_study_payload(self, nparr, scale=1.0, pad_last=True, echo=True, chain=False):
        """calc_study_payload without waiting: -> ticket; `wait(ticket)` returns the (flow16, echo16 | None) pair.  The frames are
        conditioned and the echo is complete before this returns (nparr may be reused at once)."""
        return self._study(nparr, scale, pad_last, f16=True, echo=echo, submit=True, chain=chain)

    def calc_study_held(self, nparr, scale=1.0, echo=True, chain=False):
        """calc_study_payload(hold=True) without its arrays: the RGB study uint8 [N,H,W,3] is solved into the held payload (N float16
        flow frames, the last one repeated; the echo if asked for) and nothing is downloaded.  Returns nothing; `last_stats` and
        last_iters() are the float16 call's, and `held` describes the study afterwards.  For a consumer that wants the payload's
        compressed chunks (study_chunks) or its statistics (the held_* calls), not the arrays."""
        nparr = self._frames_in(nparr, self._rgb_study, 2)
        N, H, W, _ = nparr.shape
        st = _lib.TfStats()
        if chain:
            self.chain_next()
        _lib.check(self._L.tf_calc_seq_rgb_held(self._h, self._frames_ptr(nparr), N, H, W, float(scale), 1 if echo else 0, C.byref(st)), self._h,
                   "tf_calc_seq_rgb_held")
        self._finish(st)

    def study_chunks(self, nparr, scale, flow_chunks, echo_chunks=None, chain=False):
        """The study file's `flow` and `echo` datasets as gzip-9 chunks, with no float16 array on the host: calc_study_held, then
        held_deflate("flow", flow_chunks) and, where echo_chunks is given, held_deflate("echo", echo_chunks).  -> {"flow": record,
        "echo": record or None}, the records in analysis.chunks_record's layout.  The study stays held."""
        self.calc_study_held(nparr, scale, echo=echo_chunks is not None, chain=chain)
        return {"flow": self.held_deflate("flow", flow_chunks), "echo": None if echo_chunks is None else self.held_deflate("echo", echo_chunks)}

    def saliency_frames(self, nparr, dtype=np.float32):
        """cv2.saliency.StaticSaliencyFineGrained_create().computeSaliency(frame)[1] for every frame, on the device (reference
        calculate_optical_flow.py:559-560, :586): uint8 [N,H,W,3] or [N,H,W] -> [N,H,W].  dtype float32 (default): the CV_32F map in
        [0,1] that opencv-contrib 4.x returns; uint8: the algorithm's 8-bit map (opencv-contrib 3.x).  Three-channel frames meet
        OpenCV's BGR2GRAY in the order given, as the reference's RGB frames do."""
        def check(nparr):
            nparr = np.ascontiguousarray(nparr)
            if nparr.ndim == 3:
                return _u8_image_stack(nparr, "nparr", 3)
            nparr = _u8_image_stack(nparr, "nparr", 4)
            if nparr.shape[3] not in (1, 3):
                raise OpticalFlowCalculationError(f"nparr must be [N,H,W], [N,H,W,1] or [N,H,W,3], got {nparr.shape}")
            return nparr
        nparr = self._frames_in(nparr, check)
        ch = 1 if len(nparr.shape) == 3 else nparr.shape[3]
        N, H, W = nparr.shape[:3]
        f32 = self._map_is_f32(dtype)
        out = np.empty((N, H, W), np.float32 if f32 else np.uint8)
        fn = self._L.tf_saliency_frames_f32 if f32 else self._L.tf_saliency_frames
        _lib.check(fn(self._h, self._frames_ptr(nparr), N, H, W, ch, out.ctypes.data), self._h, "tf_saliency_frames")
        return out

    @staticmethod
    def _map_is_f32(dtype):
        if dtype in ("f32", "float32") or (not isinstance(dtype, str) and np.dtype(dtype) == np.float32):
            return True
        if dtype in ("u8", "uint8") or (not isinstance(dtype, str) and np.dtype(dtype) == np.uint8):
            return False
        raise OpticalFlowCalculationError(f"saliency map dtype must be float32 ('f32') or uint8 ('u8'), got {dtype!r}")

    def calc_study_saliency(self, nparr, scale=1.0, pad_last=False, map_dtype="f32", chain=False):
        """RGB study uint8 [N,H,W,3] -> float32 [N-1,H,W,2] with the saliency maps as the solver's frames (no_saliency=False).
        map_dtype "f32" (default): the solver receives computeSaliency()'s CV_32F maps in [0,1], as under opencv-contrib >= 4.5 -- DualTVL1
        multiplies them by 255 in float, DeepFlow takes them as they are; "u8": the 8-bit maps.  `scale` / `pad_last` as in calc_study."""
        return self._study(nparr, scale, pad_last, saliency=True, map_dtype=map_dtype, chain=chain)

    def clean_masks(self, class_map, class_ids, min_size):
        """The reference's clean_mask (calculate_optical_flow.py:90-111, :113-182) on the device, exact: class map uint8 [N,H,W] ->
        bool [len(class_ids) + 1, N, H, W, 2], one plane per class id in the order given (moving average of `== id` with the
        reference's defaults, fill holes, remove_small_objects(min_size), all 4-connected) and 'bkgd' last.  Each plane is a
        C-contiguous view in pinned host memory.  May be called while submitted studies are in flight on this engine."""
        class_map = _u8_image_stack(class_map, "class_map", 3)
        ids = np.ascontiguousarray(class_ids, dtype=np.uint8)
        if ids.ndim != 1 or ids.size < 1:
            raise OpticalFlowCalculationError(f"class_ids must be a non-empty list of class ids, got {class_ids!r}")
        N, H, W = class_map.shape
        out = self._pool.empty((ids.size + 1, N, H, W, 2), np.uint8)
        _lib.check(self._L.tf_clean_masks(self._h, class_map.ctypes.data, N, H, W, ids.ctypes.data, int(ids.size), int(min_size),
                                          out.ctypes.data), self._h, "tf_clean_masks")
        return out.view(np.bool_)

    def otsu_masks(self, nparr, min_size, return_thresholds=False):
        """The reference's predict_movie_thres (calculate_optical_flow.py:184-213) on the device, exact: RGB frames uint8 [N,H,W,3]
        (N, H, W >= 2) -> bool [N,H,W,2]: per frame rgb2gray, skimage's threshold_otsu, fill holes, remove_small_objects(min_size), then
        the moving average with the reference's defaults over the cleaned planes.  A C-contiguous array in pinned host memory.  With
        `return_thresholds` also the per-frame Otsu thresholds, float64 [N].  May be called while submitted studies are in flight on
        this engine."""
        nparr = self._frames_in(nparr, partial(_u8_image_stack, name="nparr", ndim=4))
        if nparr.shape[3] != 3 or min(nparr.shape[:3]) < 2:
            raise OpticalFlowCalculationError(f"nparr must be [N>=2,H>=2,W>=2,3], got {nparr.shape}")
        N, H, W = nparr.shape[:3]
        out = self._pool.empty((N, H, W, 2), np.uint8)
        thr = np.empty(N, np.float64) if return_thresholds else None
        _lib.check(self._L.tf_otsu_masks(self._h, self._frames_ptr(nparr), N, H, W, int(min_size), out.ctypes.data,
                                         thr.ctypes.data if return_thresholds else None), self._h, "tf_otsu_masks")
        return (out.view(np.bool_), thr) if return_thresholds else out.view(np.bool_)

    def _torch_stream(self, torch):
        """(stream to hand the library, stream torch is on): torch's current stream of this engine's device -- or, where that is the
        legacy default stream (handle 0, which the C ABI reads as "the handle's own"), a side stream ordered behind it."""
        cur = torch.cuda.current_stream(self.device_id)
        if cur.cuda_stream:
            return cur, cur
        side = getattr(self, "_seg_side_stream", None)
        if side is None:
            side = self._seg_side_stream = torch.cuda.Stream(self.device_id)
        side.wait_stream(cur)
        return side, cur

    def segmentor_input(self, frames, out_size=(1024, 1024), out=None):
        """evaluate_1_slice's model input (reference calculate_optical_flow.py:47-70) for a stack of frames, on the device and exact: RGB
        frames uint8 [N,H,W,3] -> float32 torch tensor [N,3,out_h,out_w] on cuda:<device_id> = PIL's BILINEAR resize to out_size =
        (out_h, out_w), ToTensor, ImageNet normalisation (masks.segmentor_lut).  `out`: a float32 contiguous tensor on that device with
        room for the result is reused (its first N frames are returned).  Runs on torch's current stream and does not wait for it.
        torch and the library must share one HIP runtime, i.e. torch was imported before the first engine of the process was made
        (a process that made the engine first finds no GPU in torch; a model that sits on the GPU is proof of the right order)."""
        import torch
        from .masks import segmentor_lut
        frames = self._frames_in(frames, partial(_u8_image_stack, name="frames", ndim=4))
        if frames.shape[3] != 3:
            raise OpticalFlowCalculationError(f"frames must be [N,H,W,3], got {frames.shape}")
        N, H, W, _ = frames.shape
        oh, ow = int(out_size[0]), int(out_size[1])
        dev = torch.device("cuda", self.device_id)
        if (out is not None and out.dtype == torch.float32 and out.device == dev and out.is_contiguous() and out.dim() == 4
                and tuple(out.shape[1:]) == (3, oh, ow) and out.shape[0] >= N):
            x = out[:N]
        else:
            x = torch.empty((max(N, 0), 3, max(oh, 0), max(ow, 0)), dtype=torch.float32, device=dev)
        lut = segmentor_lut()
        s, cur = self._torch_stream(torch)
        _lib.check(self._L.tf_segmentor_input(self._h, self._frames_ptr(frames), N, H, W, oh, ow, lut.ctypes.data, x.data_ptr(),
                                              C.c_void_p(s.cuda_stream)), self._h, "tf_segmentor_input")
        if s is not cur:
            x.record_stream(s)
            cur.wait_stream(s)
        return x

    def segmentor_classmap(self, logits, size):
        """evaluate_1_slice's way back (reference :84-88) for a stack of frames, on the device and exact: logits torch tensor [n,C,h,w] on
        cuda:<device_id> (made float32 and contiguous with torch if they are not) -> class map uint8 [n,H,W], size = (H, W): torch's CPU
        argmax over C (lowest index of equal maxima, NaN is the maximum), then PIL's NEAREST resize.  Waits for the result."""
        import torch
        if not isinstance(logits, torch.Tensor) or logits.dim() != 4 or logits.device != torch.device("cuda", self.device_id):
            raise OpticalFlowCalculationError(f"logits must be a torch tensor [n,C,h,w] on cuda:{self.device_id}")
        if logits.dtype != torch.float32 or not logits.is_contiguous():
            logits = logits.float().contiguous()
        n, Cn, h, w = logits.shape
        H, W = int(size[0]), int(size[1])
        out = np.empty((max(n, 0), max(H, 0), max(W, 0)), np.uint8)
        s, _ = self._torch_stream(torch)
        _lib.check(self._L.tf_segmentor_classmap(self._h, logits.data_ptr(), n, Cn, h, w, H, W, out.ctypes.data, C.c_void_p(s.cuda_stream)),
                   self._h, "tf_segmentor_classmap")
        return out

    # ---- the consumer's tail.  Six calls have a host-pointer form and a held form (held_*, further down) over one private body; the two
    # forms differ in the C function they name and in its leading arguments: host pointers and sizes, or the frame count and the slot ----
    def _centroids(self, fn, lead, n):
        cent = np.zeros((max(n, 0), 2), np.float64)
        area = np.zeros(max(n, 0), np.int64)
        _lib.check(getattr(self._L, fn)(self._h, *lead, cent.ctypes.data, area.ctypes.data), self._h, fn)
        return cent, area

    def _region_areas(self, fn, lead, n):
        area = np.zeros(max(n, 0), np.int64)
        _lib.check(getattr(self._L, fn)(self._h, *lead, area.ctypes.data), self._h, fn)
        return area

    def _project(self, fn, lead, shape, return_arrays, polar=False):
        """The outputs of a projection of shape = (n, H, W) and its call: -> (minmax, nonzero, plane, plane) in float64, or (`polar`) in
        float32 with the angle mode after nonzero; the planes are None without return_arrays."""
        n, H, W = shape
        dt = np.float32 if polar else np.float64
        planes = [np.empty((n, H, W), dt) if return_arrays else None for _ in range(2)]
        mm = np.zeros(4, dt)
        nz = np.zeros((n, 2), np.int64)
        mode = (np.zeros(n, np.float32),) if polar else ()
        _lib.check(getattr(self._L, fn)(self._h, *lead, *(a.ctypes.data if return_arrays else None for a in planes), mm.ctypes.data,
                                        nz.ctypes.data, *(a.ctypes.data for a in mode)), self._h, fn)
        return (mm, nz, *mode, *planes)

    def _overlay(self, fn, lut_rad, lut_long, echo=None):
        """`echo` (the host form): checked against the planes' shape and passed first"""
        luts = []
        for name, lut in (("lut_rad", lut_rad), ("lut_long", lut_long)):
            lut = np.ascontiguousarray(lut, dtype=np.float64)
            if lut.shape != (256, 3):
                raise OpticalFlowCalculationError(f"{name} must be [256,3], got shape {lut.shape}")
            luts.append(lut)
        # the library knows the planes' shape; an echo's must be checked against it before the library reads n * H * W values of it
        shape = (C.c_int * 3)()
        _lib.check(self._L.tf_radlong_shape(self._h, C.byref(shape)), self._h, "tf_radlong_shape")
        n, H, W = shape
        lead = ()
        if echo is not None:
            if n >= 1 and (echo.shape[0] < n or echo.shape[1:] != (H, W)):
                raise OpticalFlowCalculationError(f"echo must be [>= {n},{H},{W}] (the projection's frames), got shape {echo.shape}")
            echo = np.ascontiguousarray(echo[:max(n, 1)])
            lead = (echo.ctypes.data, _lib.ECHO_F16 if echo.dtype == np.float16 else _lib.ECHO_U8)
        # (without rad/long planes the library refuses, and says why, before it reads the echo or writes out)
        out = self._pool.empty((n, H, 2 * W, 3), np.uint8) if n >= 1 else np.empty(1, np.uint8)
        info = np.zeros(3, np.float64)
        _lib.check(getattr(self._L, fn)(self._h, *lead, luts[0].ctypes.data, luts[1].ctypes.data, out.ctypes.data, info.ctypes.data), self._h, fn)
        return out, info

    def av_centroids(self, masks):
        """calc_AV_centroid's per-frame step (analyze_optical_flow.py:202-232) on the device, exact: masks bool or uint8 [N,H,W,C]
        (C = 1 or 2; the set is channel 0 != 0, 8-connected) -> (centroids float64 [N,2] (row, col) of the largest component, areas
        int64 [N], 0 for an empty frame).  May be called while submitted studies are in flight on this engine."""
        m = _mask_stack(masks, "masks")
        return self._centroids("tf_av_centroids", (m.ctypes.data, *m.shape), m.shape[0])

    def first_region_areas(self, masks):
        """AreaDetector.detect's per-frame step (cardiac_cycle_detection.py:159-172: skimage label, regionprops, props[0].area) on the
        device, exact: masks bool or uint8 [N,H,W,C] (C = 1 or 2; only channel 0 is read) -> int64 [N], the pixel count of the
        8-connected region of equal value that holds the frame's first non-zero pixel in raster order, 0 for an empty frame.  May be
        called while submitted studies are in flight on this engine."""
        m = _mask_stack(masks, "masks")
        return self._region_areas("tf_first_region_areas", (m.ctypes.data, *m.shape), m.shape[0])

    def _project_param(self, fn, flow, mask, param, spacing, grad_f64, n_used, centroids, return_arrays, polar=False):
        """the host-pointer form of a param projection (the polar one takes no centroids): what both check and lay out -- flow [N,H,W,2]
        float16 / float32, mask [n_used,H,W,C] uint8 -- and the call"""
        flow = np.asarray(flow)
        if flow.dtype not in (np.float16, np.float32):
            flow = flow.astype(np.float32)
        flow = np.ascontiguousarray(flow)
        if flow.ndim != 4 or flow.shape[3] != 2 or min(flow.shape) < 1:
            raise OpticalFlowCalculationError(f"flow must be [N,H,W,2], got {flow.shape}")
        N, H, W, _ = flow.shape
        n_used = int(n_used)
        if not 1 <= n_used <= N:
            raise OpticalFlowCalculationError(f"n_used must be in [1, {N}], got {n_used}")
        if param not in (0, 1, 2):
            raise OpticalFlowCalculationError(f"param must be 0 (velocity), 1 (acceleration) or 2 (PWR), got {param!r}")
        if param != 0 and N < 2:
            raise OpticalFlowCalculationError("the gradient needs at least 2 flow frames")
        if param != 0 and not (np.isfinite(spacing) and spacing != 0):
            raise OpticalFlowCalculationError(f"spacing must be finite and non-zero for the gradient, got {spacing!r}")
        m = _mask_stack(np.asarray(mask)[:n_used], "mask")
        if m.shape[:3] != (n_used, H, W):
            raise OpticalFlowCalculationError(f"mask must be [>= {n_used},{H},{W},C], got {np.shape(mask)}")
        cent = () if centroids is None else (np.ascontiguousarray(centroids, dtype=np.float64).reshape(n_used, 2),)
        lead = (flow.ctypes.data, 1 if flow.dtype == np.float16 else 0, N, n_used, H, W, m.ctypes.data, m.shape[3], int(param), float(spacing),
                1 if grad_f64 else 0, *(c.ctypes.data for c in cent))
        return self._project(fn, lead, (n_used, H, W), return_arrays, polar)

    def radlong_project_param(self, flow, mask, param, spacing, grad_f64, n_used, centroids, return_arrays=False):
        """tf_radlong_project_param: the rad/long projection of OpticalFlowDataset's param field (param 0 velocity, 1 acceleration,
        2 PWR) for frames [0, n_used), resident on the device for tf_radlong_hist / _select.  flow float16 or float32 [N,H,W,2],
        mask bool or uint8 [>= n_used,H,W,C].  Returns (minmax float64 [4], nonzero int64 [n_used, 2], rad, long): rad / long are
        float64 [n_used,H,W] with return_arrays, else None."""
        return self._project_param("tf_radlong_project_param", flow, mask, param, spacing, grad_f64, n_used, centroids, return_arrays)

    def polar_project_param(self, flow, mask, param, spacing, grad_f64, n_used, return_arrays=False):
        """tf_polar_project_param: cv2.cartToPolar (analysis.cart_to_polar's arithmetic) of OpticalFlowDataset's param field (param 0
        velocity, 1 acceleration, 2 PWR) for frames [0, n_used); magnitude and angle stay resident on the device for tf_radlong_hist /
        _select (which 0 / 1).  flow float16 or float32 [N,H,W,2], mask bool or uint8 [>= n_used,H,W,C].  Returns (minmax float32 [4]
        (mag min, max, ang min, max), nonzero int64 [n_used, 2] (non-zero mag, ang per frame), ang_mode float32 [n_used] (the angle
        detector's per-frame mode, NaN if none), mag, ang): mag / ang are float32 [n_used,H,W] with return_arrays, else None.  May
        be called while submitted studies are in flight on this engine."""
        return self._project_param("tf_polar_project_param", flow, mask, param, spacing, grad_f64, n_used, None, return_arrays, polar=True)

    def radlong_overlay(self, echo, lut_rad, lut_long):
        """tf_radlong_overlay: the radial / longitudinal overlay frames of visualize_radlong (analyze_optical_flow.py:488-560) from the
        planes the last radlong_project_param (or tf_radlong_project) call left on the device; n, H and W are that call's.  echo float16
        (the study file's) or uint8 [>= n,H,W]; lut_rad / lut_long float64 [256,3] (analysis.colormap_lut).  Returns (out uint8
        [n,H,2W,3] in pinned host memory, info float64 [3] = (half, echo max, m2)).  May be called while submitted studies are in
        flight on this engine."""
        echo = np.asarray(echo)
        if echo.dtype not in (np.float16, np.uint8):
            raise OpticalFlowCalculationError(f"echo must be float16 or uint8, got {echo.dtype}")
        if echo.ndim != 3 or min(echo.shape) < 1:
            raise OpticalFlowCalculationError(f"echo must be [N,H,W] with no empty side, got shape {echo.shape}")
        return self._overlay("tf_radlong_overlay", lut_rad, lut_long, echo)

    def _magnitude_overlay(self, fn, lead, shape, lut):
        """The outputs of a magnitude overlay of shape = (n, H, W) and its call: -> (out uint8 [n,H,W,3] in pinned host memory, info
        float64 [2] = (vmin, vmax), frame_info float64 [n,2] = each frame's (echo max, colour max))."""
        lut = np.ascontiguousarray(lut, dtype=np.float64)
        if lut.shape != (256, 3):
            raise OpticalFlowCalculationError(f"lut must be [256,3], got shape {lut.shape}")
        n, H, W = shape
        out = self._pool.empty((n, H, W, 3), np.uint8)
        info = np.zeros(2, np.float64)
        frame_info = np.zeros((n, 2), np.float64)
        _lib.check(getattr(self._L, fn)(self._h, *lead, lut.ctypes.data, out.ctypes.data, info.ctypes.data, frame_info.ctypes.data), self._h, fn)
        return out, info, frame_info

    def magnitude_overlay(self, flow, mask, param, spacing, grad_f64, norm_f64, n_used, echo, lut):
        """tf_magnitude_overlay: the frames of the reference's single-component video (example_peak_plots.py:459-513): the float32
        magnitude of OpticalFlowDataset's param field (param 0 velocity, 1 acceleration, 2 PWR) through the table `lut`, one norm over
        all N frames, frames [0, n_used) rendered and blended half and half with the echo, each frame normalised by its own maxima.
        flow float16 or float32 [N,H,W,2], mask bool or uint8 [>= N,H,W,C], echo float16 (the study file's) or uint8 [>= n_used,H,W],
        lut float64 [256,3]; norm_f64 as analysis.norm_is_f64.  Returns (out uint8 [n_used,H,W,3], info, frame_info) as
        _magnitude_overlay.  Leaves the resident planes of the last projection alone.  May be called while submitted studies are in
        flight on this engine."""
        flow = np.asarray(flow)
        if flow.dtype not in (np.float16, np.float32):
            flow = flow.astype(np.float32)
        flow = np.ascontiguousarray(flow)
        if flow.ndim != 4 or flow.shape[3] != 2 or min(flow.shape) < 1:
            raise OpticalFlowCalculationError(f"flow must be [N,H,W,2], got {flow.shape}")
        N, H, W, _ = flow.shape
        n_used = int(n_used)
        if not 1 <= n_used <= N:
            raise OpticalFlowCalculationError(f"n_used must be in [1, {N}], got {n_used}")
        if param not in (0, 1, 2):
            raise OpticalFlowCalculationError(f"param must be 0 (velocity), 1 (acceleration) or 2 (PWR), got {param!r}")
        if param != 0 and N < 2:
            raise OpticalFlowCalculationError("the gradient needs at least 2 flow frames")
        if param != 0 and not (np.isfinite(spacing) and spacing != 0):
            raise OpticalFlowCalculationError(f"spacing must be finite and non-zero for the gradient, got {spacing!r}")
        m = _mask_stack(np.asarray(mask)[:N], "mask")
        if m.shape[:3] != (N, H, W):
            raise OpticalFlowCalculationError(f"mask must be [>= {N},{H},{W},C] (the norm's range is over every frame), got {np.shape(mask)}")
        echo = np.asarray(echo)
        if echo.dtype not in (np.float16, np.uint8):
            raise OpticalFlowCalculationError(f"echo must be float16 or uint8, got {echo.dtype}")
        if echo.ndim != 3 or echo.shape[0] < n_used or echo.shape[1:] != (H, W):
            raise OpticalFlowCalculationError(f"echo must be [>= {n_used},{H},{W}], got shape {echo.shape}")
        echo = np.ascontiguousarray(echo[:n_used])
        lead = (flow.ctypes.data, 1 if flow.dtype == np.float16 else 0, N, n_used, H, W, m.ctypes.data, m.shape[3], int(param), float(spacing),
                1 if grad_f64 else 0, 1 if norm_f64 else 0, echo.ctypes.data, _lib.ECHO_F16 if echo.dtype == np.float16 else _lib.ECHO_U8)
        return self._magnitude_overlay("tf_magnitude_overlay", lead, (n_used, H, W), lut)

    # ---- the statistics of the planes a projection left resident: what analysis.py's glue calls ------------------------------------
    def radlong_project(self, flow, centroids, return_arrays=False):
        """tf_radlong_project: the rad/long projection of a field given whole, flow [>= n,H,W,2] (made float32) and n centroids (row, col),
        resident on the device for radlong_hist / radlong_select.  Returns (minmax, nonzero, rad, long) as radlong_project_param."""
        n = len(centroids)
        flow = np.ascontiguousarray(np.asarray(flow)[:n], dtype=np.float32)
        N, H, W, _ = flow.shape
        cent = np.ascontiguousarray(centroids, dtype=np.float64).reshape(N, 2)
        return self._project("tf_radlong_project", (flow.ctypes.data, cent.ctypes.data, N, H, W), (N, H, W), return_arrays)

    def radlong_hist(self, which, edges, n_frames):
        """tf_radlong_hist: per frame, the histogram of the non-zero values of resident plane `which` (0 rad / mag, 1 long / ang) over
        `edges` (passed as float64, exactly): int64 [n_frames, len(edges) - 1].  n_frames is the last projection's frame count."""
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        freq = np.zeros((int(n_frames), len(edges) - 1), np.int64)
        _lib.check(self._L.tf_radlong_hist(self._h, int(which), edges.ctypes.data, len(edges) - 1, freq.ctypes.data), self._h, "tf_radlong_hist")
        return freq

    def radlong_select(self, which, ranks):
        """tf_radlong_select: the order statistics of the non-zero values of resident plane `which`: ranks int64 [n, 4] per frame of the
        last projection (a negative rank is skipped) -> float64 [n, 4], sorted(frame's non-zero values)[rank]."""
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        vals = np.zeros(ranks.shape, np.float64)
        _lib.check(self._L.tf_radlong_select(self._h, int(which), ranks.ctypes.data, vals.ctypes.data), self._h, "tf_radlong_select")
        return vals

    # ---- a study held on the device (include/teeflow.h, tf_hold_study): the file's payload uploaded once -- or left there by the solve
    # that made it -- and the consumer's tail reading it there.  The held_* methods are av_centroids, first_region_areas,
    # radlong_project_param, polar_project_param, radlong_overlay and magnitude_overlay with a mask label in the place of the mask array and no flow or
    # echo array; results are the same bits --------------------------------------------------------------------------------------------
    def _held_shape(self):
        shape = (C.c_longlong * _lib.HELD_SHAPE_LEN)()
        _lib.check(self._L.tf_held_shape(self._h, C.byref(shape)), self._h, "tf_held_shape")
        self._held_labels.sync(shape[4])
        return shape

    @property
    def held(self):
        """The study held on the device, a HeldShape(N, H, W, n_echo, generation, masks = {label: (n_frames, C)}), or None."""
        s = self._held_shape()
        if s[0] < 1:
            return None
        masks = {label: (int(s[5 + 2 * k]), int(s[6 + 2 * k])) for label, k in self._held_labels.slots.items()}
        return HeldShape(int(s[0]), int(s[1]), int(s[2]), int(s[3]), int(s[4]), masks)

    def hold_study(self, flow16, echo16=None):
        """Put a study file's payload on the device, where the held_* calls read it: flow16 float16 [N,H,W,2] (the file's `flow`),
        echo16 float16 [n,H,W] (its `echo`) or None.  Replaces the study held before and forgets its masks.  Device memory: 4 bytes per
        flow pixel, 2 per echo pixel, until the next hold_study, a study call with hold=True, release_study or close."""
        flow = np.ascontiguousarray(flow16)
        if flow.dtype != np.float16 or flow.ndim != 4 or flow.shape[3] != 2 or min(flow.shape) < 1:
            raise OpticalFlowCalculationError(f"flow16 must be float16 [N,H,W,2] with no empty side, got {flow.dtype} {flow.shape}")
        N, H, W, _ = flow.shape
        echo = None if echo16 is None else np.ascontiguousarray(echo16)
        if echo is not None and (echo.dtype != np.float16 or echo.ndim != 3 or echo.shape[0] < 1 or echo.shape[1:] != (H, W)):
            raise OpticalFlowCalculationError(f"echo16 must be float16 [n>=1,{H},{W}], got {echo.dtype} {echo.shape}")
        _lib.check(self._L.tf_hold_study(self._h, flow.ctypes.data, N, H, W, None if echo is None else echo.ctypes.data,
                                         0 if echo is None else echo.shape[0]), self._h, "tf_hold_study")
        return self.held

    def _held_or_raise(self):
        shape = self._held_shape()
        if shape[0] < 1:
            raise OpticalFlowCalculationError("no study is held (hold_study, or a study call with hold=True)")
        return shape

    def _hold_mask(self, fn, label, frame_shape, channels, what, call):
        """what hold_mask and hold_mask_chunks share, for the library's call `fn`: the mask's frames are the held study's, the label
        gets its slot, and a label that is new goes again if the library refuses the mask.  call(slot) -> the library's return code."""
        shape = self._held_or_raise()
        if tuple(frame_shape) != (shape[1], shape[2]) or channels not in (1, 2):
            raise OpticalFlowCalculationError(f"mask must be [n,{shape[1]},{shape[2]},C] (the held study's frames), C = 1 or 2, got {what}")
        known = label in self._held_labels.slots
        slot = self._held_labels.slot_for(label)
        try:
            _lib.check(call(slot), self._h, fn)
        except OpticalFlowCalculationError:
            if not known:
                del self._held_labels.slots[label]
            raise

    def hold_mask(self, label, mask):
        """Put a mask of the held study on the device under `label`: bool or uint8 [n,H,W,C], C = 1 or 2, H and W the held study's.  A
        label held already is replaced; a held study takes 12 labels, a 13th raises."""
        self._held_or_raise()
        m = _mask_stack(mask, "mask")
        self._hold_mask("tf_hold_mask", label, m.shape[1:3], m.shape[3], m.shape, lambda slot: self._L.tf_hold_mask(self._h, slot, m.ctypes.data, m.shape[0], m.shape[3]))

    # ---- inflate on the device (include/teeflow.h, tf_inflate): the gzip chunks of a study file are independent zlib streams; the
    # device decodes them, one wave per stream, and a study is held from the compressed bytes of its file -------------------------------
    def inflate(self, streams, out_bytes, out=None):
        """zlib streams (bytes-like objects), each to out_bytes bytes -> (uint8 [n,out_bytes], status int32 [n]).  A status is 0 or the
        library's code for what is wrong with the stream (teeflow.h); the call does not raise for a stream that does not decode: its
        status says so, and its row holds what was decoded before the fault and is otherwise untouched (zeros, or what `out` held:
        out, a C-contiguous uint8 [n,out_bytes] array of the caller's, is written in place of a fresh one).  A call that fails as a
        whole -- refused arguments, a HIP error -- raises."""
        streams = [bytes(s) if not isinstance(s, (bytes, bytearray)) else s for s in streams]
        n, out_bytes = len(streams), int(out_bytes)
        if out_bytes < 0:
            raise OpticalFlowCalculationError(f"out_bytes must be >= 0, got {out_bytes}")
        if out is None:
            out = np.zeros((n, out_bytes), np.uint8)
        elif not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.shape != (n, out_bytes) or not out.flags.c_contiguous:
            raise OpticalFlowCalculationError(f"out must be a C-contiguous uint8 [{n},{out_bytes}] array")
        status = np.zeros(n, np.int32)                       # the library's alone: a call that fails as a whole leaves it clear
        lens = np.array([len(s) for s in streams], np.uint32)
        offs = np.zeros(n, np.uint64)
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        blob = np.frombuffer(b"".join(streams) or b"\0", np.uint8)
        rc = self._L.tf_inflate(self._h, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data, None, n, out_bytes, out.ctypes.data, status.ctypes.data)
        self._raise_unless_verdict(rc, status, "tf_inflate")
        return out, status

    @staticmethod
    def _chunked(rec, what, ndim, dtypes):
        """a dataset record of analysis.study_chunks -> (tf_chunked, the arrays it points into)"""
        shape, chunk = tuple(int(v) for v in rec["shape"]), tuple(int(v) for v in rec["chunks"])
        dt = np.dtype(str(rec["dtype"]))
        if dt not in dtypes or len(shape) != ndim or len(chunk) != ndim or min(shape + chunk) < 1:
            raise OpticalFlowCalculationError(f"{what} chunks must describe a {ndim}-D {' or '.join(str(np.dtype(d)) for d in dtypes)} dataset with no "
                                              f"empty side, got {dt} {shape} in chunks of {chunk}")
        coord = np.ascontiguousarray(rec["coord"], np.int64).reshape(-1, ndim)
        n = coord.shape[0]
        off, ln = np.ascontiguousarray(rec["off"], np.uint64), np.ascontiguousarray(rec["len"], np.uint32)
        raw = np.ascontiguousarray((np.asarray(rec["filter_mask"], np.uint32) & 1).astype(np.uint8))
        blob = np.ascontiguousarray(rec["blob"], np.uint8)
        if not (off.shape == ln.shape == raw.shape == (n,)):
            raise OpticalFlowCalculationError(f"{what} chunks: coord, off, len and filter_mask disagree about the number of chunks")
        if n and int((off + ln.astype(np.uint64)).max()) > blob.size:
            raise OpticalFlowCalculationError(f"{what} chunks: a chunk ends behind the blob's {blob.size} bytes")
        if blob.size == 0:
            blob = np.zeros(1, np.uint8)
        c = _lib.TfChunked(blob.ctypes.data, off.ctypes.data, ln.ctypes.data, raw.ctypes.data, coord.ctypes.data, n, ndim)
        for d in range(ndim):
            c.shape[d], c.chunk[d] = shape[d], chunk[d]
        c.elem_bytes, c.chunk_bytes = dt.itemsize, int(np.prod(chunk, dtype=np.int64)) * dt.itemsize
        return c, (blob, off, ln, raw, coord)

    def hold_study_chunks(self, flow_chunks, echo_chunks=None):
        """hold_study from the file's own chunks: flow_chunks / echo_chunks are the `flow` and `echo` dataset records of
        analysis.study_chunks (float16 [N,H,W,2] and [n,H,W], gzip chunks as the file holds them).  The compressed bytes are uploaded
        and inflated on the device; the held study is what hold_study of the arrays leaves.  If a chunk does not decode the call
        raises and the study held before, with its masks, stays."""
        f, keep_f = self._chunked(flow_chunks, "flow", 4, (np.float16,))
        if f.shape[3] != 2:
            raise OpticalFlowCalculationError(f"flow chunks must describe [N,H,W,2], got {tuple(f.shape)}")
        e, keep_e = (None, None) if echo_chunks is None else self._chunked(echo_chunks, "echo", 3, (np.float16,))
        _lib.check(self._L.tf_hold_study_chunks(self._h, C.byref(f), None if e is None else C.byref(e)), self._h, "tf_hold_study_chunks")
        del keep_f, keep_e
        return self.held

    def hold_mask_chunks(self, label, chunks):
        """hold_mask from the file's own chunks: the dataset record of a bool or uint8 [n,H,W,C] mask, C = 1 or 2."""
        self._held_or_raise()
        m, keep = self._chunked(chunks, "mask", 4, (np.bool_, np.uint8))
        self._hold_mask("tf_hold_mask_chunks", label, (m.shape[1], m.shape[2]), m.shape[3], tuple(m.shape), lambda slot: self._L.tf_hold_mask_chunks(self._h, slot, C.byref(m)))
        del keep

    # ---- deflate on the device (include/teeflow.h, tf_deflate): a dataset's chunks, each into the bytes of zlib.compress(chunk, 9) ----
    @staticmethod
    def deflate_bound(chunk_bytes):
        """zlib's compressBound: the most bytes the stream of a chunk of chunk_bytes takes"""
        b = int(chunk_bytes)
        return b + (b >> 12) + (b >> 14) + (b >> 25) + 13

    def _deflate_call(self, name, n, chunk_bytes, ndim, call):
        """the outputs of the three deflate calls: (blob uint8 [total], off uint64 [n], len uint32 [n], coord int64 [n,ndim] or None)"""
        blob = np.empty(max(n * self.deflate_bound(chunk_bytes), 1), np.uint8)
        off, ln, status = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.int32)
        coord = None if ndim is None else np.zeros((n, ndim), np.int64)
        _lib.check(call(n, blob, off, ln, coord, status), self._h, name)
        return blob[:int(ln.sum(dtype=np.uint64))].copy(), off, ln, coord

    def deflate(self, chunks):
        """Equal-sized chunks (a sequence of bytes-like objects of one length, or a C-contiguous uint8 [n,chunk_bytes] array) -> (blob,
        off, len): chunk i's zlib stream is blob[off[i]:off[i] + len[i]], the bytes of zlib.compress(chunk, 9)."""
        if isinstance(chunks, np.ndarray):
            if chunks.dtype != np.uint8 or chunks.ndim != 2 or not chunks.flags.c_contiguous:
                raise OpticalFlowCalculationError("chunks must be a C-contiguous uint8 [n,chunk_bytes] array or a sequence of bytes")
            packed = chunks
        else:
            chunks = [bytes(c) for c in chunks]
            if len({len(c) for c in chunks}) > 1:
                raise OpticalFlowCalculationError("deflate takes chunks of one size per call")
            packed = np.frombuffer(b"".join(chunks), np.uint8).reshape(len(chunks), len(chunks[0]) if chunks else 0)
        n, cb = packed.shape
        keep = packed if packed.size else np.zeros(1, np.uint8)
        blob, off, ln, _ = self._deflate_call("tf_deflate", n, cb, None, lambda n_, b, o, l, c, s: self._L.tf_deflate(
            self._h, keep.ctypes.data, n_, cb, b.ctypes.data, b.size, o.ctypes.data, l.ctypes.data, s.ctypes.data))
        return blob, off, ln

    @staticmethod
    def _chunk_grid(shape, chunks, what):
        shape, chunks = tuple(int(v) for v in shape), tuple(int(v) for v in chunks)
        if not 1 <= len(shape) <= 4 or len(chunks) != len(shape) or min(shape + chunks) < 1:
            raise OpticalFlowCalculationError(f"{what}: need 1 to 4 dimensions with no empty side and as many chunk extents, got {shape} in chunks of {chunks}")
        return shape, chunks, int(np.prod([-(-s // c) for s, c in zip(shape, chunks)], dtype=np.int64))

    @staticmethod
    def _deflated_record(shape, dtype, chunks, blob, off, ln, coord):
        """the outputs as a dataset record of analysis.chunks_record: what hold_study_chunks / hold_mask_chunks and the writer take"""
        return {"shape": shape, "dtype": str(np.dtype(dtype)), "chunks": chunks, "coord": coord, "filter_mask": np.zeros(len(ln), np.uint32),
                "off": off, "len": ln, "blob": blob}

    def deflate_array(self, arr, chunks):
        """An array of 1 to 4 dimensions with 1-, 2- or 4-byte elements, cut into chunks of `chunks` elements per dimension as HDF5
        stores them (whole chunks, zero beyond the edge, in h5py's order) -> its dataset record (analysis.chunks_record's layout),
        every chunk the bytes of zlib.compress(chunk, 9)."""
        arr = np.ascontiguousarray(arr)
        if arr.dtype.itemsize not in (1, 2, 4):
            raise OpticalFlowCalculationError(f"deflate_array takes 1-, 2- or 4-byte elements, got {arr.dtype}")
        shape, chunks, n = self._chunk_grid(arr.shape, chunks, "deflate_array")
        sh, ch = np.array(shape, np.int64), np.array(chunks, np.int64)
        cb = int(np.prod(chunks, dtype=np.int64)) * arr.dtype.itemsize
        out = self._deflate_call("tf_deflate_array", n, cb, len(shape), lambda n_, b, o, l, c, s: self._L.tf_deflate_array(
            self._h, arr.ctypes.data, len(shape), sh.ctypes.data, ch.ctypes.data, arr.dtype.itemsize, n_, b.ctypes.data, b.size, o.ctypes.data, l.ctypes.data,
            c.ctypes.data, s.ctypes.data))
        return self._deflated_record(shape, arr.dtype, chunks, *out)

    def held_deflate(self, what, chunks):
        """deflate_array of an array of the held study, read where it is: what = "flow" (float16 [N,H,W,2]), "echo" (float16 [n,H,W]) or
        the label of a held mask (bool [n,H,W,C]) -> its dataset record.  Nothing is uploaded."""
        held = self._held_or_raise()
        N, H, W, n_echo = (int(v) for v in held[:4])
        if what == "flow":
            kind, slot, shape, dt = _lib.HELD_FLOW, 0, (N, H, W, 2), np.float16
        elif what == "echo":
            if not n_echo:
                raise OpticalFlowCalculationError("the held study has no echo")
            kind, slot, shape, dt = _lib.HELD_ECHO, 0, (n_echo, H, W), np.float16
        else:
            slot = self._held_slot(what)
            kind, shape, dt = _lib.HELD_MASK, (int(held[5 + 2 * slot]), H, W, int(held[6 + 2 * slot])), np.bool_
        shape, chunks, n = self._chunk_grid(shape, chunks, "held_deflate")
        ch = np.array(chunks, np.int64)
        cb = int(np.prod(chunks, dtype=np.int64)) * np.dtype(dt).itemsize
        out = self._deflate_call("tf_held_deflate", n, cb, len(shape), lambda n_, b, o, l, c, s: self._L.tf_held_deflate(
            self._h, kind, slot, ch.ctypes.data, n_, b.ctypes.data, b.size, o.ctypes.data, l.ctypes.data, c.ctypes.data, s.ctypes.data))
        return self._deflated_record(shape, dt, chunks, *out)

    def hold_next(self, on=True):
        """Arm (or disarm) the next study call to leave its payload held: what hold=True does for the calc_study_*_payload calls.  The
        library spends the flag on the next study call, whatever becomes of it; armed, a submitted or a float32 study is refused."""
        _lib.check(self._L.tf_hold_next(self._h, 1 if on else 0), self._h, "tf_hold_next")

    def release_study(self):
        """Free the held study's device memory; held_* calls are refused until a study is held again."""
        _lib.check(self._L.tf_release_study(self._h), self._h, "tf_release_study")
        self._held_shape()

    def _held_slot(self, label):
        self._held_shape()
        return self._held_labels.slot_of(label)

    def held_av_centroids(self, label, n):
        """av_centroids of the first n frames of the held mask `label` -> (centroids float64 [n,2], areas int64 [n])."""
        slot, n = self._held_slot(label), int(n)
        return self._centroids("tf_held_av_centroids", (slot, n), n)

    def held_first_region_areas(self, label, n):
        """first_region_areas of the first n frames of the held mask `label` -> int64 [n]."""
        slot, n = self._held_slot(label), int(n)
        return self._region_areas("tf_held_first_region_areas", (slot, n), n)

    def _held_project_param(self, fn, label, param, spacing, grad_f64, n_used, centroids, return_arrays, polar=False):
        """the held form of a param projection (the polar one takes no centroids); an n_used the library will refuse sizes the outputs as
        one frame, n = 1, so that the library's message is the one raised"""
        slot, n_used = self._held_slot(label), int(n_used)
        s = self._held_shape()
        n = n_used if 1 <= n_used <= s[0] else 1
        cent = ()
        if centroids is not None:
            cent = (np.ascontiguousarray(centroids, dtype=np.float64).reshape(-1, 2),)
            if n == n_used and cent[0].shape[0] != n_used:
                raise OpticalFlowCalculationError(f"{cent[0].shape[0]} centroids for {n_used} frames")
        lead = (n_used, slot, int(param), float(spacing), 1 if grad_f64 else 0, *(c.ctypes.data for c in cent))
        return self._project(fn, lead, (n, int(s[1]), int(s[2])), return_arrays, polar)

    def held_radlong_project_param(self, label, param, spacing, grad_f64, n_used, centroids, return_arrays=False):
        """radlong_project_param of the held flow and the held mask `label`: -> (minmax, nonzero, rad, long) as there."""
        return self._held_project_param("tf_held_radlong_project_param", label, param, spacing, grad_f64, n_used, centroids, return_arrays)

    def held_polar_project_param(self, label, param, spacing, grad_f64, n_used, return_arrays=False):
        """polar_project_param of the held flow and the held mask `label`: -> (minmax, nonzero, ang_mode, mag, ang) as there."""
        return self._held_project_param("tf_held_polar_project_param", label, param, spacing, grad_f64, n_used, None, return_arrays, polar=True)

    def held_radlong_overlay(self, lut_rad, lut_long):
        """radlong_overlay with the held study's echo, of the planes the last (held_)radlong_project_param call left on the device:
        -> (out uint8 [n,H,2W,3], info float64 [3])."""
        return self._overlay("tf_held_radlong_overlay", lut_rad, lut_long)

    def held_magnitude_overlay(self, label, param, spacing, grad_f64, norm_f64, n_used, lut):
        """magnitude_overlay of the held flow and echo and the held mask `label` (which covers every held frame): -> (out, info,
        frame_info) as there.  An n_used the library will refuse sizes the outputs as one frame, so that the library's message is
        the one raised."""
        slot, n_used = self._held_slot(label), int(n_used)
        s = self._held_shape()
        n = n_used if 1 <= n_used <= s[0] else 1
        lead = (n_used, slot, int(param), float(spacing), 1 if grad_f64 else 0, 1 if norm_f64 else 0)
        return self._magnitude_overlay("tf_held_magnitude_overlay", lead, (n, int(s[1]), int(s[2])), lut)

    def wase_compensate(self, flows, bkgd_mask, scale=1.0):
        """Reference :647-652, 659 for every flow of a study at once, on the device: returns (flows - background[p]) * scale
        and the float32 backgrounds.  flows float32 [P,H,W,2]; bkgd_mask bool [N,H,W,2] (mask_dict['bkgd'])."""
        flows = np.array(flows, dtype=np.float32, order="C", copy=True)
        mask = np.ascontiguousarray(bkgd_mask)
        if flows.ndim != 4 or flows.shape[3] != 2:
            raise OpticalFlowCalculationError(f"flows must be [P,H,W,2], got {flows.shape}")
        if mask.dtype != np.bool_ or mask.ndim != 4 or mask.shape[1:] != flows.shape[1:]:
            raise OpticalFlowCalculationError(f"bkgd mask must be bool [N,{flows.shape[1]},{flows.shape[2]},2], got {mask.dtype} {mask.shape}")
        P, H, W, _ = flows.shape
        bg = np.empty(P, np.float32)
        _lib.check(self._L.tf_wase_compensate(self._h, flows.ctypes.data, P, mask.view(np.uint8).ctypes.data, mask.shape[0], H, W,
                                              float(scale), bg.ctypes.data), self._h, "tf_wase_compensate")
        return flows, bg

    # ---- a bkgd_comp="WASE" study in one call: the flows stay on the device between the solve and the compensation -------------
    def calc_study_wase(self, nparr, bkgd_mask, scale=1.0, pad_last=False, chain=False):
        """calc_study, then wase_compensate of its flows, in one device call: RGB study uint8 [N,H,W,3] and bkgd_mask bool [n,H,W,2]
        (mask_dict['bkgd']) -> ((flow - background[p]) * scale float32 [N-1,H,W,2], backgrounds float32 [N-1]), with the bits of
        wase_compensate(calc_study(nparr), bkgd_mask, scale).  `pad_last` as in calc_study."""
        return self._study(nparr, scale, pad_last, bkgd_mask=bkgd_mask, chain=chain)

    def calc_study_wase_payload(self, nparr, bkgd_mask, scale=1.0, pad_last=True, echo=True, hold=False, chain=False):
        """calc_study_wase with the flows rounded to float16 by the output kernel -> (flow16, echo16 | None, backgrounds): flow16 has
        the bits of calc_study_wase(...)[0].astype(np.float16), echo16 is echo_frames(nparr) from the same upload.  `hold` as in
        calc_study_payload."""
        return self._study(nparr, scale, pad_last, f16=True, echo=echo, bkgd_mask=bkgd_mask, hold=hold, chain=chain)

    def calc_study_saliency_wase(self, nparr, bkgd_mask, scale=1.0, pad_last=False, map_dtype="f32", chain=False):
        """calc_study_wase with the saliency maps as the solver's frames (calc_study_saliency) -> (flows float32, backgrounds)."""
        return self._study(nparr, scale, pad_last, saliency=True, map_dtype=map_dtype, bkgd_mask=bkgd_mask, chain=chain)

    def calc_study_saliency_wase_payload(self, nparr, bkgd_mask, scale=1.0, pad_last=True, echo=True, map_dtype="f32", hold=False, chain=False):
        """calc_study_saliency_wase with float16 flows and the `echo` of the RGB frames -> (flow16, echo16 | None, backgrounds).  `hold`
        as in calc_study_payload."""
        return self._study(nparr, scale, pad_last, saliency=True, map_dtype=map_dtype, f16=True, echo=echo, bkgd_mask=bkgd_mask, hold=hold, chain=chain)

    def calc_pairs(self, I0s, I1s, init=None):
        """B independent pairs: uint8 or float32 [B,H,W] x2 -> float32 [B,H,W,2] (float frames: DualTVL1 scales them by 255 like cv2, DeepFlow
        takes them as they are like cv2).  `init`: the pairs' initial flows [B,H,W,2], read under setUseInitialFlow(True) as calc reads
        `flow`."""
        I0s = _u8_image_stack(I0s, "I0s", 3, allow_f32=True)
        I1s = _u8_image_stack(I1s, "I1s", 3, allow_f32=True)
        if I0s.shape != I1s.shape or I0s.dtype != I1s.dtype:
            raise OpticalFlowCalculationError(f"I0s and I1s differ: {I0s.shape} {I0s.dtype} vs {I1s.shape} {I1s.dtype}")
        B, H, W = I0s.shape
        init = self._initial_flows(init, (B, H, W, 2), "init")
        out = self._out((B, H, W, 2))
        st = _lib.TfStats()
        if init is not None:
            _lib.check(self._L.tf_calc_pairs_init(self._h, I0s.ctypes.data, I1s.ctypes.data, int(I0s.dtype == np.float32), init.ctypes.data, B, H, W,
                                                  out.ctypes.data, C.byref(st)), self._h, "tf_calc_pairs_init")
        else:
            fn = self._L.tf_calc_pairs_f32 if I0s.dtype == np.float32 else self._L.tf_calc_pairs
            _lib.check(fn(self._h, I0s.ctypes.data, I1s.ctypes.data, B, H, W, out.ctypes.data, C.byref(st)), self._h, "tf_calc_pairs")
        self._finish(st)
        return out

    def calc_pairs_device(self, dI0s_ptr, dI1s_ptr, B, H, W, dflow_ptr, scale=1.0, dinit_ptr=None):
        """Device-resident form: raw device pointers (e.g. tensor.data_ptr()); result written to dflow_ptr.  `dinit_ptr`: the pairs'
        initial flows, device float32 [B,H,W,2] in pixels per frame (not times `scale`), read under setUseInitialFlow(True) -- the
        library refuses the call when the flag is set and there is none; it may be dflow_ptr itself."""
        st = _lib.TfStats()
        if dinit_ptr is None:
            _lib.check(self._L.tf_calc_pairs_device(self._h, C.c_void_p(dI0s_ptr), C.c_void_p(dI1s_ptr), int(B), int(H), int(W),
                                                    float(scale), C.c_void_p(dflow_ptr), C.byref(st)), self._h, "tf_calc_pairs_device")
        else:
            _lib.check(self._L.tf_calc_pairs_init_device(self._h, C.c_void_p(dI0s_ptr), C.c_void_p(dI1s_ptr), C.c_void_p(dinit_ptr), int(B), int(H),
                                                         int(W), float(scale), C.c_void_p(dflow_ptr), C.byref(st)), self._h, "tf_calc_pairs_init_device")
        self._finish(st)
        return self.last_stats

    # ---- jobs in flight: the same calls, queued on the engine's lanes inside the library and collected later ------------------
    def submit_pairs_device(self, dI0s_ptr, dI1s_ptr, B, H, W, dflow_ptr, scale=1.0):
        """tf_submit_pairs_device: queue the batch on the engine's lanes and return a ticket at once; `wait(ticket)` returns its
        statistics.  The device buffers must stay untouched until then.  Consecutive jobs overlap on the GPU (one batch's tail
        under the next one's full launches), which a stream of synchronous calls cannot do."""
        t = C.c_int(-1)
        _lib.check(self._L.tf_submit_pairs_device(self._h, C.c_void_p(dI0s_ptr), C.c_void_p(dI1s_ptr), int(B), int(H), int(W), float(scale),
                                                  C.c_void_p(dflow_ptr), C.byref(t)), self._h, "tf_submit_pairs_device")
        self._jobs[t.value] = None
        return t.value

    def submit_seq_device(self, dframes_ptr, N, H, W, dflow_ptr, scale=1.0, chain=False):
        """tf_submit_seq_device: calc_seq_device without waiting -- device frames uint8 [N,H,W], device float32 [N-1,H,W,2] * scale -> ticket;
        `wait(ticket)` returns its statistics.  The device buffers must stay untouched until then.  `chain` as in calc_batch."""
        t = C.c_int(-1)
        if chain:
            self.chain_next()
        _lib.check(self._L.tf_submit_seq_device(self._h, C.c_void_p(dframes_ptr), int(N), int(H), int(W), float(scale), C.c_void_p(dflow_ptr),
                                                C.byref(t)), self._h, "tf_submit_seq_device")
        self._jobs[t.value] = None
        return t.value

    def submit_batch(self, frames, scale=1.0, chain=False):
        """calc_batch without waiting: frames uint8 [N,H,W] -> ticket; `wait(ticket)` returns float32 [N-1,H,W,2].  A chained job is one
        unit of the lane queue: chains submitted together run side by side, one per lane."""
        frames = _u8_image_stack(frames, "frames", 3)
        N, H, W = frames.shape
        if N < 2:
            raise OpticalFlowCalculationError("need at least 2 frames")
        out = self._out((N - 1, H, W, 2))
        t = C.c_int(-1)
        if chain:
            self.chain_next()
        _lib.check(self._L.tf_submit_seq(self._h, frames.ctypes.data, N, H, W, float(scale), out.ctypes.data, C.byref(t)), self._h, "tf_submit_seq")
        self._jobs[t.value] = _Job(out, inputs=(frames,))               # the library reads `frames` and writes `out` until the wait
        return t.value

    def submit_study(self, nparr, scale=1.0, pad_last=False, chain=False):
        """calc_study without waiting: RGB study uint8 [N,H,W,3] -> ticket; `wait(ticket)` returns float32 [N-1,H,W,2] (or [N,H,W,2] with
        the last flow repeated, `pad_last`).  The frames are conditioned on the device before this returns (nparr may be reused at once)."""
        return self._study(nparr, scale, pad_last, submit=True, chain=chain)

    def submit_pairs(self, I0s, I1s):
        """calc_pairs without waiting: uint8 [B,H,W] x2 -> ticket; `wait(ticket)` returns float32 [B,H,W,2]."""
        I0s = _u8_image_stack(I0s, "I0s", 3)
        I1s = _u8_image_stack(I1s, "I1s", 3)
        if I0s.shape != I1s.shape:
            raise OpticalFlowCalculationError(f"I0s and I1s differ: {I0s.shape} vs {I1s.shape}")
        B, H, W = I0s.shape
        out = self._out((B, H, W, 2))
        t = C.c_int(-1)
        _lib.check(self._L.tf_submit_pairs(self._h, I0s.ctypes.data, I1s.ctypes.data, B, H, W, out.ctypes.data, C.byref(t)), self._h, "tf_submit_pairs")
        self._jobs[t.value] = _Job(out, inputs=(I0s, I1s))
        return t.value

    def wait(self, ticket):
        """Collect a submitted job: its flows (host forms) or its statistics (device form).  `last_stats` / `last_iters()` then
        describe that job.  A failed job raises here."""
        if ticket not in self._jobs:
            raise OpticalFlowCalculationError(f"unknown ticket {ticket!r} (already waited for?)")
        job = self._jobs.pop(ticket)
        st = _lib.TfStats()
        _lib.check(self._L.tf_wait(self._h, int(ticket), C.byref(st)), self._h, "tf_wait")
        self._finish(st)
        return self.last_stats if job is None else self._collect(job)      # (None: the device form, nothing of the host's to hand back)

    def calc_seq_device(self, dframes_ptr, N, H, W, dflow_ptr, scale=1.0, chain=False):
        """tf_calc_seq_device: device frames uint8 [N,H,W] -> device float32 [N-1,H,W,2] * scale.  `chain` as in calc_batch."""
        st = _lib.TfStats()
        if chain:
            self.chain_next()
        _lib.check(self._L.tf_calc_seq_device(self._h, C.c_void_p(dframes_ptr), int(N), int(H), int(W), float(scale),
                                              C.c_void_p(dflow_ptr), C.byref(st)), self._h, "tf_calc_seq_device")
        self._finish(st)
        return self.last_stats


    # ---- multi-GPU exchange: RCCL all-gather issued by the library itself ------------------
    @staticmethod
    def comm_unique_id():
        """128 opaque bytes from ncclGetUniqueId: rank 0 makes them, the launcher hands them to every rank."""
        L = _lib.load()
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES)()
        _lib.check(L.tf_comm_unique_id(buf), None, "tf_comm_unique_id")
        return bytes(buf)

    def comm_init_rank(self, nranks, rank, id_bytes):
        """Join an `nranks`-rank RCCL communicator as `rank` (one process per GPU)."""
        if len(id_bytes) != _lib.COMM_ID_BYTES:
            raise OpticalFlowCalculationError(f"communicator id must be {_lib.COMM_ID_BYTES} bytes")
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES).from_buffer_copy(id_bytes)
        _lib.check(self._L.tf_comm_init_rank(self._h, int(nranks), int(rank), buf), self._h, "tf_comm_init_rank")
        self.has_comm = True

    def allgather(self, d_send_ptr, count_floats, d_recv_ptr):
        """Enqueue this rank's part of the all-gather of the (u,v) fields (device pointers, `count_floats` per rank);
        returns a ticket for comm_wait.  Returns at once: the exchange runs beside whatever is solved next."""
        t = C.c_int(-1)
        _lib.check(self._L.tf_allgather_flows(self._h, C.c_void_p(d_send_ptr), C.c_size_t(int(count_floats)), C.c_void_p(d_recv_ptr),
                                              C.byref(t)), self._h, "tf_allgather_flows")
        return t.value

    def comm_wait(self, ticket=-1):
        """Block until the all-gather `ticket` (default: every one issued so far) has finished."""
        _lib.check(self._L.tf_comm_wait(self._h, int(ticket)), self._h, "tf_comm_wait")


def createOptFlow_DeepFlow(device_id=0, **kw):
    """Name-compatible factory for cv2.optflow.createOptFlow_DeepFlow() (reference :568)."""
    return DenseFlow(device_id=device_id, algo="deepflow", **kw)


def createOptFlow_DualTVL1(device_id=0, **kw):
    """Name-compatible factory for cv2.optflow.createOptFlow_DualTVL1() (reference :577)."""
    return DenseFlow(device_id=device_id, **kw)


def cuda_OpticalFlowDual_TVL1_create(device_id=0, **kw):
    """Counterpart of cv2.cuda.OpticalFlowDual_TVL1.create() (reference :575): the CUDA branch's semantics -- 300 iterations
    in one loop per warp, no median filtering, error looked at on odd iterations only, weight-normalised Catmull-Rom warp
    with clamp addressing (TF_VARIANT_CUDA).  As on the reference's CUDA branch, nothing is set on it."""
    return DenseFlow(device_id=device_id, variant="cuda", **kw)
