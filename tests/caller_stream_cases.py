"""Solves and tail calls on a caller's stream (include/teeflow.h, tf_set_stream; DenseFlow.set_stream): the inputs, what the CPU says
they must give, and each scenario as a function of (eng, torch, stream), so that the same code runs on a torch side stream and on the
legacy default stream.  A helper module of tests/test_gpu_caller_stream.py: nothing here is collected.

The parent process (pytest, the `oracle` fixture) calls build() and saves the result as an .npz; a child process that has imported torch
before the first engine (the two must share one HIP runtime) calls run_group() on it.  Everything a scenario compares with comes from
that file: the C oracles, the oracle's stages composed on the CPU (tests/tvl1_init_cases.composed, tests/tvl1_chain_cases) and the host
twins of the tail calls (frames, masks, analysis).  No scenario compares a handle on a caller's stream with a handle on its own.

`eng` is a Handles: eng(**kw) makes a DenseFlow on the caller's stream (own=True: on its own), eng.z is the .npz.  `stream` is a Caller.
A scenario that fails ends the child at once: nothing more is started on the GPU behind a failure."""
import ctypes as C
import os
import sys
import time
import traceback

import numpy as np

from tests import tvl1_chain_cases as CC

REFUSAL = "tf_submit_* needs the handle's own stream"
OVER = dict(warps=1)                              # tvl1_init_cases' "odd-37x53": one warp per level keeps the composed solves short
SCALE = 0.7                                       # of the study forms: a product that rounds, in float32 and again in float16
FRAME_RATE = 50.0
# the long producer of the stream-order scenario: PASSES in-place passes over GIB bytes.  Sized on an MI355X (the summary of the change
# that added this file has the figures): the producer must outlast a call on the handle's own stream, which the control asserts
GIB, PASSES = 1 << 30, 200


# ---- the parent's side: inputs and expected results ---------------------------------------------------------------------------------
def _study_masks(n, H, W):
    """{'rv': a drifting disc, 'av': two blobs of different size}, bool [n,H,W,2] (as tests/test_gpu_held_study.py makes them)"""
    yy, xx = np.mgrid[:H, :W]
    rv, av = np.zeros((n, H, W), bool), np.zeros((n, H, W), bool)
    for f in range(n):
        rv[f] = ((yy - H / 2 - f / 3) / (0.35 * H)) ** 2 + ((xx - W / 2 + f / 3) / (0.4 * W)) ** 2 < 1
        av[f] = ((yy - H / 3 - f / 2) ** 2 + (xx - W / 3) ** 2 < 30 + f) | ((yy - 3 * H / 4) ** 2 + (xx - 3 * W / 4) ** 2 < 9)
    return {k: np.ascontiguousarray(np.repeat(m[..., None], 2, axis=3)) for k, m in (("rv", rv), ("av", av))}


def _oracle_pairs(O, I0s, I1s, params=None):
    """(flows [B,H,W,2], iters [B,levels,warps,2]) of the C oracle, pair by pair"""
    flows, iters = [], []
    for a, b in zip(I0s, I1s):
        f, it, nl = O.tvl1_calc(a, b, params, return_iters=True)
        flows.append(f)
        iters.append(it[:nl])
    return np.stack(flows), np.stack(iters)


def build(O):
    """{name: array}: every input of the scenarios and what each call must return, computed on the CPU"""
    from tee_optical_flow_amd import analysis as A, frames as FR, masks
    from tee_optical_flow_amd.synth import speckle_pairs, speckle_sequence
    from tests import tvl1_chains_cases as LC
    from tests import tvl1_init_cases as IC
    from tests import tvl1_ref64_cases as K
    from tests.test_gpu_masks import _class_map
    from tests.test_masks_cpu import _Cfg
    z = {}
    # DualTVL1 pairs, 37x53: four levels, odd on every one.  Five pairs with an initial flow each (test_gpu_tvl1_init's batch)
    seeds = [3, 4, 5, 6, 7]
    I0s, I1s = (np.ascontiguousarray(a) for a in speckle_pairs(seeds, 37, 53))
    inits = np.stack([IC.initial_flow(s, 37, 53, 1.5) for s in seeds])
    z["sp_I0s"], z["sp_I1s"], z["sp_inits"] = I0s, I1s, inits
    z["sp_flow_dflt"], z["sp_iters_dflt"] = _oracle_pairs(O, I0s[:2], I1s[:2])                     # all defaults: five warps
    z["sp_flow_w1"], z["sp_iters_w1"] = _oracle_pairs(O, I0s, I1s, O.default_params(**OVER))
    comp = [IC.composed(O, I0s[b], I1s[b], K.params(**OVER), inits[b]) for b in range(len(seeds))]
    z["sp_seeded"], z["sp_seeded_iters"] = np.stack([c[0] for c in comp]), np.stack([c[1] for c in comp])
    z["sp_flow_cuda"], z["sp_iters_cuda"] = _oracle_pairs(O, I0s[:1], I1s[:1], O.default_params(variant=1))
    F0, F1 = IC.f32_frames(I0s[:2], I1s[:2], 11)
    z["f32_I0s"], z["f32_I1s"] = np.ascontiguousarray(F0), np.ascontiguousarray(F1)
    z["f32_flow"], z["f32_iters"] = _oracle_pairs(O, F0, F1)
    # a sequence of four 37x53 frames: three pairs, two sub-batches of a max_batch=2 handle
    seq = np.ascontiguousarray(speckle_sequence(5, 4, 37, 53))
    z["seq"] = seq
    z["seq_flow_dflt"], z["seq_iters_dflt"] = _oracle_pairs(O, seq[:-1], seq[1:])
    z["seq_flow_w1"], z["seq_iters_w1"] = _oracle_pairs(O, seq[:-1], seq[1:], O.default_params(**OVER))
    # DualTVL1 strips, 97x131: five pairs are three sub-batches of a max_batch=2 handle
    S0, S1 = (np.ascontiguousarray(a) for a in speckle_pairs(range(20, 25), 97, 131))
    z["st_I0s"], z["st_I1s"] = S0, S1
    z["st_flow"], z["st_iters"] = _oracle_pairs(O, S0, S1)
    # DeepFlow, 64x80: three pairs are two sub-batches of a max_batch=2 handle
    D0, D1 = (np.ascontiguousarray(a) for a in speckle_pairs(range(30, 33), 64, 80))
    z["df_I0s"], z["df_I1s"] = D0, D1
    z["df_flow"] = np.stack([O.deepflow_calc(a, b) for a, b in zip(D0, D1)])
    # chains: the existing cases `one` and `odd`, and the two lock-step chains derived from `odd`
    for cid in ("one", "odd"):
        fr = np.array(CC.frames(cid))
        z[f"ch_{cid}_frames"] = fr
        z[f"ch_{cid}_flow"], z[f"ch_{cid}_iters"], _ = CC.chain_case(O, cid)
    for name in ("tail", "fwd"):                             # test_gpu_tvl1_chains' case of max_batch = 3, S = 2: ragged, cut over time
        f = LC.derived(z["ch_odd_frames"])[name]
        z[f"lc_odd_{name}_flow"], z[f"lc_odd_{name}_iters"], _ = LC.expected(O, ("odd", name), f, CC.overrides("odd"))
    # an RGB study: five frames of 48x64 with three different channels, masks of the same size, a class map.  (Grey frames repeated as
    # RGB would not do: their luma is v / 255, so img2uint8's v * 255 / max meets exact rounding ties, which the last bit of the luma
    # decides -- and the host twin's luma goes through numpy's BLAS, which may fuse multiply and add, while the device evaluates the
    # plain order (tests/test_gpu_otsu.py).  The twin must not depend on that here: asserted.)
    N, H, W = 5, 48, 64
    rgb = np.ascontiguousarray(CC.rgb_of(speckle_sequence(31, N, H, W)))
    cond = FR.condition_frames(rgb)
    a = rgb.astype(np.float64) / 255.0
    plain = (a[..., 0] * 0.2125 + a[..., 1] * 0.7154) + a[..., 2] * 0.0721
    assert np.array_equal(cond, np.stack([FR.img2uint8(f) for f in plain])), "the host twin of condition_frames depends on the luma's last bit"
    F, Fit = _oracle_pairs(O, cond[:-1], cond[1:])
    padded = np.concatenate([F, F[-1:]])
    z["rgb"], z["rgb_cond"], z["rgb_flow"], z["rgb_iters"] = rgb, cond, F, Fit
    z["rgb_flow16"] = (padded * np.float32(SCALE)).astype(np.float16)
    z["rgb_echo16"] = FR.rgb2gray(rgb).astype(np.float16)
    maps = np.stack([O.saliency_fine_grained(f, np.uint8) for f in rgb])
    z["rgb_maps"] = maps
    z["rgb_sal_flow"], z["rgb_sal_iters"] = _oracle_pairs(O, maps[:-1], maps[1:])
    bkgd = np.random.default_rng(H).random((2, H, W, 2)) < 0.3
    bg = np.empty(N - 1, np.float32)
    wase = np.empty_like(F)
    for p in range(N - 1):                                    # pipeline.wase_background and the reference's order (:647-652, :659)
        m = F[p] * bkgd
        bg[p] = np.mean(m[m != 0])
        wase[p] = (F[p] - bg[p]) * np.float32(SCALE)
    assert np.isfinite(bg).all() and bg.dtype == np.float32
    z["rgb_bkgd"], z["rgb_wase_flow"], z["rgb_wase_bg"] = bkgd, wase, bg
    z["rgb_otsu"] = masks.predict_movie_thres(rgb, config=_Cfg(30))["otsu"]
    cmap = _class_map(N * 1000 + H, N, H, W, 2)
    host = masks.clean_mask(cmap, "RVIO_2class", config=_Cfg(30))
    z["cmap"], z["cmap_ids"] = cmap, np.array(list(masks._MODE_LABELS["RVIO_2class"].values()), np.uint8)
    z["cmap_planes"] = np.stack([host[k] for k in host])
    # the held tail of the study's float16 payload: frames [0, n) with n < N, so that the gradient reads frame n too
    m, n = _study_masks(N, H, W), N - 1
    found = [A._largest_component(m["av"][i, :, :, 0]) for i in range(n)]
    cent = np.array([f[0] for f in found], np.float64)
    z["held_rv"], z["held_av"], z["held_n"] = m["rv"], m["av"], np.int64(n)
    z["held_cent"], z["held_area"] = cent, np.array([f[1] for f in found], np.int64)
    z["held_grad_f64"] = np.bool_(A.gradient_is_f64(FRAME_RATE))
    z["held_rad"], z["held_long"] = A.calculate_comp_magnitude(A.param_field(z["rgb_flow16"], m["rv"], "acceleration", FRAME_RATE, n), cent)
    z["held_mag"], z["held_ang"] = A.polar_field(z["rgb_flow16"], m["rv"], "PWR", FRAME_RATE, n)
    return {k: np.asarray(v) for k, v in z.items()}


# ---- the child's side ----------------------------------------------------------------------------------------------------------------
class Caller:
    """The caller's stream: `kind` "side" is a torch.cuda.Stream() handed over as its cuda_stream, "default" is the legacy default
    stream, handed over as 0 (what torch.cuda.current_stream().cuda_stream reports for torch's default stream)."""

    def __init__(self, torch, kind):
        self.kind = kind
        self.torch_stream = torch.cuda.Stream(0) if kind == "side" else torch.cuda.default_stream(0)
        self.ptr = int(self.torch_stream.cuda_stream)
        assert (self.ptr != 0) == (kind == "side"), (kind, self.ptr)

    def attach(self, e):
        e.set_stream(self.ptr, external=True)

    def idle(self):
        """has everything enqueued on the stream completed?  (no synchronisation: hipStreamQuery)"""
        return self.torch_stream.query()


class Handles:
    """eng(**kw): a DenseFlow on the caller's stream; own=True leaves it on its own.  Every handle is closed when the scenario ends."""

    def __init__(self, z, stream, shared):
        self.z, self.stream, self.shared, self.open = z, stream, shared, []

    def __call__(self, own=False, **kw):
        import tee_optical_flow_amd as T
        e = T.DenseFlow(device_id=0, **kw)
        self.open.append(e)
        if not own:
            self.stream.attach(e)
        return e

    def close_all(self):
        for e in self.open:
            e.close()
        self.open = []


def same(got, want, what):
    """bit for bit, type and shape included; prints the count before it asserts"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = int(np.count_nonzero(got.view(u) != want.view(u)))
    print(f"  {what}: {bad} of {got.size} values differ", flush=True)
    assert bad == 0, f"{what}: {bad} of {got.size} values differ"


def drained(stream, what):
    """scenario 3: a call returns only after its work has drained -- the caller's stream is idle before any synchronisation"""
    assert stream.idle(), f"{what}: the call returned with work still on the caller's stream"


def refused(e, name, call):
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import _lib
    jobs = e.counter("queue_jobs")
    try:
        t = call()
    except T.OpticalFlowCalculationError as err:
        print(f"  {name}: code {err.code}: {err}", flush=True)
        assert err.code == _lib.TF_ERR_UNSUPPORTED and REFUSAL in str(err), (name, err)
    else:
        raise AssertionError(f"{name} on a caller's stream was not refused (ticket {t})")
    assert not e._jobs and e.counter("queue_jobs") == jobs and e.counter("queue_outstanding") == 0, f"{name}: a refused call left a ticket or a job"


# ---- 1 (and 3): solves on the caller's stream are the oracle's ---------------------------------------------------------------------------
def solves_are_the_oracles(eng, torch, stream):
    from tee_optical_flow_amd import _lib
    z = eng.z
    tv = eng(max_batch=2)
    jobs = tv.counter("queue_jobs")
    flow = tv.calc(z["sp_I0s"][0], z["sp_I1s"][0], None)
    drained(stream, "calc")
    same(flow, z["sp_flow_dflt"][0], "calc 37x53")
    same(tv.last_iters(), z["sp_iters_dflt"][:1], "calc 37x53 iteration counts")
    # the overlapped copy-out: a pinned result, three sub-batches, the third waits for the first's copy (kb >= 2)
    S0, S1 = z["st_I0s"], z["st_I1s"]
    flows = tv.calc_pairs(S0, S1)
    drained(stream, "calc_pairs, pinned")
    assert flows.base is not None, "the result is not in pinned memory: the overlapped path was not entered"
    same(flows, z["st_flow"], "calc_pairs 5 x 97x131, pinned result")
    same(tv.last_iters(), z["st_iters"], "its iteration counts")
    # the in-order copy-out: the same call into a pageable array
    out = np.full(z["st_flow"].shape, np.nan, np.float32)
    st = _lib.TfStats()
    _lib.check(tv._L.tf_calc_pairs(tv._h, S0.ctypes.data, S1.ctypes.data, len(S0), 97, 131, out.ctypes.data, C.byref(st)), tv._h, "tf_calc_pairs")
    drained(stream, "tf_calc_pairs, pageable")
    tv._finish(st)
    same(out, z["st_flow"], "tf_calc_pairs 5 x 97x131, pageable result")
    same(tv.last_iters(), z["st_iters"], "its iteration counts")
    seq = tv.calc_batch(z["seq"])
    drained(stream, "calc_batch")
    same(seq, z["seq_flow_dflt"], "calc_batch 4 x 37x53")
    same(tv.last_iters(), z["seq_iters_dflt"], "its iteration counts")
    f32 = tv.calc_pairs(z["f32_I0s"], z["f32_I1s"])
    drained(stream, "calc_pairs, float32 frames")
    same(f32, z["f32_flow"], "calc_pairs, float32 frames")
    same(tv.last_iters(), z["f32_iters"], "its iteration counts")
    assert tv.counter("queue_jobs") == jobs and tv.counter("queue_outstanding") == 0, "a call on a caller's stream went to the lanes"
    cu = eng(variant="cuda")
    flow = cu.calc(z["sp_I0s"][0], z["sp_I1s"][0], None)
    drained(stream, "calc, variant cuda")
    same(flow, z["sp_flow_cuda"][0], "calc 37x53, variant cuda")
    same(cu.last_iters(), z["sp_iters_cuda"], "its iteration counts")
    df = eng(algo="deepflow", max_batch=2)
    flows = df.calc_pairs(z["df_I0s"], z["df_I1s"])
    drained(stream, "DeepFlow calc_pairs")
    print(f"  DeepFlow: coop_launches {df.counter('coop_launches')}, coop_aborts {df.counter('coop_aborts')}", flush=True)
    same(flows, z["df_flow"], "DeepFlow calc_pairs 3 x 64x80")
    assert df.counter("coop_aborts") == 0 and df.counter("queue_jobs") == 0


# ---- 2 (and 3): stream order on the input side ---------------------------------------------------------------------------------------
def input_side_stream_order(eng, torch, stream):
    """The frames (and the seeds) are zeros until a long producer on the caller's stream, and the copies enqueued behind it, have run; the
    device-pointer calls are made at once, with no synchronisation.  On the caller's stream they must see the real frames.  The control
    makes the same calls with the handle on its own stream: they return while the caller's stream is still busy (asserted: without it the
    test would be blind) and give the all-zero flow of zero frames, which is how a call that is not ordered behind the producer fails."""
    z = eng.z
    dev = torch.device("cuda", 0)
    I0s, I1s, seq, inits = z["sp_I0s"], z["sp_I1s"], z["seq"], z["sp_inits"]
    (B, H, W), N = I0s.shape, len(seq)
    src = torch.from_numpy(np.concatenate([I0s, I1s, seq])).to(dev)
    src_init = torch.from_numpy(inits).to(dev)
    frames, dinit = torch.zeros_like(src), torch.zeros_like(src_init)
    p0 = frames.data_ptr()
    p1, ps = p0 + B * H * W, p0 + 2 * B * H * W
    if "big" not in eng.shared:
        eng.shared["big"] = torch.zeros(GIB // 4, dtype=torch.float32, device=dev)
    big = eng.shared["big"]
    outs = {"pairs": torch.empty((B, H, W, 2), dtype=torch.float32, device=dev), "seq": torch.empty((N - 1, H, W, 2), dtype=torch.float32, device=dev),
            "seeded": torch.empty((B, H, W, 2), dtype=torch.float32, device=dev)}
    # ("queue_lanes" 0: on its own stream, too, the handle solves every call alone, in the buffers the warm-up calls have made -- a lane
    # that allocates in the middle of the control could wait for the device and hide what the control is there to show)
    e = eng(own=True, max_batch=2, **OVER)
    e.set_tuning("queue_lanes", 0)

    def seeded():
        e.setUseInitialFlow(True)
        try:
            e.calc_pairs_device(p0, p1, B, H, W, outs["seeded"].data_ptr(), dinit_ptr=dinit.data_ptr())
        finally:
            e.setUseInitialFlow(False)

    calls = {"pairs": (lambda: e.calc_pairs_device(p0, p1, B, H, W, outs["pairs"].data_ptr()), z["sp_flow_w1"], z["sp_iters_w1"]),
             "seq": (lambda: e.calc_seq_device(ps, N, H, W, outs["seq"].data_ptr()), z["seq_flow_w1"], z["seq_iters_w1"]),
             "seeded": (seeded, z["sp_seeded"], z["sp_seeded_iters"])}

    def round_(name):
        """zero inputs, everything synchronised; then, on the caller's stream and with no synchronisation: the producer, the copies,
        the call, a torch op on its output -> (producer ms, the call's wall ms, was the stream idle at return, the op's result)"""
        frames.zero_()
        dinit.zero_()
        outs[name].fill_(7.0)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(PASSES):
            big.add_(1.0)
        b.record()
        frames.copy_(src, non_blocking=True)
        dinit.copy_(src_init, non_blocking=True)
        t0 = time.perf_counter()
        calls[name][0]()
        wall = (time.perf_counter() - t0) * 1e3
        idle = stream.idle()
        seen = outs[name].clone()
        it = e.last_iters()
        torch.cuda.synchronize()
        return a.elapsed_time(b), wall, idle, seen.cpu().numpy(), it

    torch.cuda.synchronize()
    for name in calls:                                       # warm-up: every buffer of the three shapes exists before a producer runs
        calls[name][0]()
    torch.cuda.synchronize()
    for name, (_, want, want_it) in calls.items():
        e.set_stream(0, external=False)
        prod, wall, idle, seen, _ = round_(name)
        print(f"  control {name} [{stream.kind}]: producer {prod:.1f} ms, the call on the handle's own stream returned after {wall:.1f} ms, "
              f"caller's stream idle at return: {idle}; non-zero flow values {int(np.count_nonzero(seen))}, values equal to the oracle's "
              f"{int(np.count_nonzero(seen == want))} of {seen.size}", flush=True)
        assert not idle, f"control {name}: the producer ({prod:.1f} ms) ended before the call returned ({wall:.1f} ms): the test is blind"
        assert not np.array_equal(seen, want), f"control {name}: a call that was not ordered behind the producer gave the oracle's flow"
        assert np.count_nonzero(seen) == 0, f"control {name}: zero frames gave a non-zero flow"
        stream.attach(e)
        prod, wall, idle, seen, it = round_(name)
        print(f"  {name} [{stream.kind}]: producer {prod:.1f} ms, the call on the caller's stream returned after {wall:.1f} ms", flush=True)
        assert idle, f"{name}: the call returned with work still on the caller's stream"
        same(seen, want, f"{name}_device behind the producer, read by a torch op enqueued right after the call")
        same(it, want_it, "its iteration counts")
        same(outs[name].cpu().numpy(), want, "the same output after synchronisation")
    same(dinit.cpu().numpy(), inits, "the seeds are not written")


# ---- 4: seeded and chained forms alone on the handle ------------------------------------------------------------------------------------
def seeded_and_chained_forms_alone(eng, torch, stream):
    z = eng.z
    e = eng(max_batch=2, **OVER)
    e.setUseInitialFlow(True)
    flows = e.calc_pairs(z["sp_I0s"], z["sp_I1s"], init=z["sp_inits"])
    drained(stream, "calc_pairs(init=)")
    same(flows, z["sp_seeded"], "calc_pairs(init=), three sub-batches")
    same(e.last_iters(), z["sp_seeded_iters"], "its iteration counts")
    assert e.counter("queue_jobs") == 0 and e.counter("queue_outstanding") == 0
    for cid, mb in (("odd", 3), ("one", 2)):                 # four and three pairs: two sub-batches each
        c = eng(max_batch=mb, **CC.overrides(cid))
        c.setUseInitialFlow(True)
        steps = c.counter("chain_steps")
        got = c.calc_batch(z[f"ch_{cid}_frames"], chain=True)
        drained(stream, "calc_batch(chain=True)")
        same(got, z[f"ch_{cid}_flow"], f"calc_batch(chain=True) of `{cid}`, max_batch {mb}")
        same(c.last_iters(), z[f"ch_{cid}_iters"].astype(np.int32), "its iteration counts")
        assert c.counter("chain_steps") - steps == len(got) and c.counter("queue_jobs") == 0
    for cid, mb, names in (("odd", 3, ("tail", "fwd")),):     # 6 frame slots, S = 2: one step per sub-batch, then S = 1
        fr = z[f"ch_{cid}_frames"]
        chains = {"tail": fr[1:], "fwd": fr}                 # tvl1_chains_cases.derived
        c = eng(max_batch=mb, **CC.overrides(cid))
        c.setUseInitialFlow(True)
        got = c.calc_chains([np.ascontiguousarray(chains[n]) for n in names])
        drained(stream, "calc_chains")
        iters = c.last_iters()
        for n, g, it in zip(names, got, iters):
            same(g, z[f"lc_{cid}_{n}_flow"], f"calc_chains of `{cid}`, max_batch {mb}: chain {n}")
            same(it, z[f"lc_{cid}_{n}_iters"].astype(np.int32), "its iteration counts")
        assert c.counter("queue_jobs") == 0 and c.counter("queue_outstanding") == 0, "a lock-step call on a caller's stream went to the lanes"


# ---- 5: study and tail calls --------------------------------------------------------------------------------------------------------------
def study_and_tail_calls(eng, torch, stream):
    """Every call against the host twin or oracle that the GPU test of that call uses (build() names them); none of them has only a
    fixture for a reference, so none is compared with the handle on its own stream."""
    z = eng.z
    rgb, F = z["rgb"], z["rgb_flow"]
    N, H, W = rgb.shape[:3]
    e = eng(max_batch=3)                                     # four pairs: two sub-batches
    same(e.condition_frames(rgb), z["rgb_cond"], "condition_frames")
    drained(stream, "condition_frames")
    same(e.calc_study(rgb), F, "calc_study")
    same(e.last_iters(), z["rgb_iters"], "its iteration counts")
    drained(stream, "calc_study")
    f16, e16 = e.calc_study_payload(rgb, scale=SCALE)
    drained(stream, "calc_study_payload")
    same(f16, z["rgb_flow16"], "calc_study_payload: float16 flow")
    same(e16, z["rgb_echo16"], "calc_study_payload: echo")
    same(e.calc_study_saliency(rgb, map_dtype="u8"), z["rgb_sal_flow"], "calc_study_saliency, u8 maps")
    same(e.last_iters(), z["rgb_sal_iters"], "its iteration counts")
    drained(stream, "calc_study_saliency")
    out, bg = e.calc_study_wase(rgb, z["rgb_bkgd"], scale=SCALE)
    drained(stream, "calc_study_wase")
    same(out, z["rgb_wase_flow"], "calc_study_wase: flows")
    same(bg, z["rgb_wase_bg"], "calc_study_wase: backgrounds")
    same(e.otsu_masks(rgb, 30), z["rgb_otsu"], "otsu_masks")
    drained(stream, "otsu_masks")
    same(e.clean_masks(z["cmap"], list(z["cmap_ids"]), 30), z["cmap_planes"], "clean_masks")
    drained(stream, "clean_masks")
    same(e.saliency_frames(rgb, dtype=np.uint8), z["rgb_maps"], "saliency_frames")
    drained(stream, "saliency_frames")
    # a study left held by the call that solves it, and the held tail
    e.hold_next()
    f16, e16 = e.calc_study_payload(rgb, scale=SCALE)
    drained(stream, "calc_study_payload, held")
    same(f16, z["rgb_flow16"], "calc_study_payload with hold_next: float16 flow")
    held = e.held
    assert held is not None and (held.N, held.H, held.W, held.n_echo) == (N, H, W, N), held
    e.hold_mask("rv", z["held_rv"])
    e.hold_mask("av", z["held_av"])
    n, g64 = int(z["held_n"]), bool(z["held_grad_f64"])
    cent, area = e.held_av_centroids("av", n)
    drained(stream, "held_av_centroids")
    same(cent, z["held_cent"], "held_av_centroids: centroids")
    same(area, z["held_area"], "held_av_centroids: areas")
    _, _, rad, lon = e.held_radlong_project_param("rv", 1, 1 / FRAME_RATE, g64, n, cent, return_arrays=True)
    drained(stream, "held_radlong_project_param")
    same(rad, z["held_rad"], "held_radlong_project_param(acceleration): rad")
    same(lon, z["held_long"], "held_radlong_project_param(acceleration): long")
    _, _, _, mag, ang = e.held_polar_project_param("rv", 2, 1 / FRAME_RATE, g64, n, return_arrays=True)
    drained(stream, "held_polar_project_param")
    same(mag, z["held_mag"], "held_polar_project_param(PWR): mag")
    same(ang, z["held_ang"], "held_polar_project_param(PWR): ang")
    assert e.counter("queue_jobs") == 0


# ---- 6: refusals and the way back -----------------------------------------------------------------------------------------------------------
def refusals_and_the_way_back(eng, torch, stream):
    import tee_optical_flow_amd as T
    z = eng.z
    dev = torch.device("cuda", 0)
    I0s, I1s, seq = z["sp_I0s"], z["sp_I1s"], z["seq"]
    (B, H, W), N = I0s.shape, len(seq)
    rgb = np.ascontiguousarray(np.repeat(seq[..., None], 3, axis=3))
    dfr = torch.from_numpy(np.concatenate([I0s, I1s, seq])).to(dev)
    p0 = dfr.data_ptr()
    p1, ps = p0 + B * H * W, p0 + 2 * B * H * W
    dpairs = torch.zeros((B, H, W, 2), dtype=torch.float32, device=dev)
    da, db = (torch.zeros((N - 1, H, W, 2), dtype=torch.float32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    e = eng(max_batch=2, **OVER)
    submits = {"submit_pairs": lambda: e.submit_pairs(I0s, I1s), "submit_batch": lambda: e.submit_batch(seq),
               "submit_study": lambda: e.submit_study(rgb), "submit_pairs_device": lambda: e.submit_pairs_device(p0, p1, B, H, W, dpairs.data_ptr()),
               "submit_seq_device": lambda: e.submit_seq_device(ps, N, H, W, da.data_ptr())}
    for name, call in submits.items():
        refused(e, name, call)
    # a chain flag armed before a refused call is spent: the next sequence call is a plain one -- which, with useInitialFlow set, is
    # refused for carrying no initial flow (include/teeflow.h)
    e.setUseInitialFlow(True)
    for name in ("submit_batch", "submit_study", "submit_seq_device"):
        e.chain_next()
        refused(e, name + " (armed)", submits[name])
        try:
            e.calc_batch(seq)
        except T.OpticalFlowCalculationError as err:
            assert "tf_calc_pairs_init" in str(err), err
        else:
            raise AssertionError(f"the chain flag armed before the refused {name} was still armed for the next call")
    e.setUseInitialFlow(False)
    same(e.calc_pairs(I0s, I1s), z["sp_flow_w1"], "the next synchronous call")
    same(e.last_iters(), z["sp_iters_w1"], "its iteration counts")
    drained(stream, "calc_pairs after the refusals")
    assert e.counter("queue_jobs") == 0
    # back on the handle's own stream: the lanes again
    e.set_stream(0, external=False)
    units = e.counter("queue_units_done")
    back = e.calc_pairs(I0s, I1s)
    d = (e.counter("queue_jobs"), e.counter("queue_units_done") - units)
    print(f"  back on the own stream: queue jobs {d[0]}, units done {d[1]}", flush=True)
    assert d == (1, 3), "a call of three sub-batches did not go through the lanes"
    same(back, z["sp_flow_w1"], "calc_pairs back on the own stream")
    e.calc_seq_device(ps, N, H, W, da.data_ptr())
    it = e.last_iters()
    st = e.wait(e.submit_seq_device(ps, N, H, W, db.data_ptr()))
    assert st["n_pairs"] == N - 1 and not e._jobs
    same(db.cpu().numpy(), da.cpu().numpy(), "submit_seq_device against calc_seq_device")
    same(e.last_iters(), it, "its iteration counts")
    same(db.cpu().numpy()[:1], z["seq_flow_w1"][:1], "submit_seq_device against the oracle, pair 0")
    # switching with a job in flight
    ticket = e.submit_pairs(I0s, I1s)
    stream.attach(e)
    mid = e.calc_pairs(I0s[::-1], I1s[::-1])
    drained(stream, "calc_pairs beside a job in flight")
    same(mid, z["sp_flow_w1"][::-1], "a call on the caller's stream with a job in flight on the lanes")
    same(e.wait(ticket), z["sp_flow_w1"], "the job submitted before the switch")
    same(e.last_iters(), z["sp_iters_w1"], "its iteration counts")
    assert e.counter("queue_outstanding") == 0 and not e._jobs


# ---- 7: sharing and closing -------------------------------------------------------------------------------------------------------------------
def two_handles_share_the_stream_and_close(eng, torch, stream):
    z = eng.z
    tv, df = eng(), eng(algo="deepflow")
    for k in (0, 1):
        same(tv.calc(z["sp_I0s"][k], z["sp_I1s"][k], None), z["sp_flow_dflt"][k], f"DualTVL1 pair {k}, beside DeepFlow")
        same(tv.last_iters(), z["sp_iters_dflt"][k:k + 1], "its iteration counts")
        same(df.calc(z["df_I0s"][k], z["df_I1s"][k], None), z["df_flow"][k], f"DeepFlow pair {k}, beside DualTVL1")
        drained(stream, "alternating calls")
    assert df.counter("coop_aborts") == 0
    tv.close()                                               # with the caller's stream still set
    df.close()
    x = torch.ones(1 << 16, device=torch.device("cuda", 0))
    x.add_(1.0)
    stream.torch_stream.synchronize()
    assert stream.idle() and float(x.sum().item()) == 2.0 * (1 << 16), "the caller's stream is not usable after close()"


# ---- 8: profiling changes nothing (run on a handle's own stream by the parent, on a caller's stream by a child) ---------------------------
def launch_profile(e):
    """tf_dbg_launch_profile's records of the last profiled solve: (level, warp, first iteration), in issue order (bench.py's layout)"""
    n = e._L.tf_dbg_launch_profile(e._h, None, None, None, None, 0)
    lv, wp, it = (np.zeros(max(n, 1), np.int32) for _ in range(3))
    ms = np.zeros(max(n, 1), np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert e._L.tf_dbg_launch_profile(e._h, ptr(lv), ptr(wp), ptr(it), ptr(ms), n) == n
    return lv[:n], wp[:n], it[:n], ms[:n]


def check_profile(e, I0s, I1s, want, want_it):
    """calc_pairs of one sub-batch, which the handle solves itself, with and without tf_set_profile(1): the same bits and iteration
    counts, and the oracle's; iter_ms > 0 only while profiling; and the launch list against the iteration counts.

    What the list can say about the counts.  A launch serves every pair of the batch and carries `step` iterations (two in the
    two-per-launch forms, which a default handle with an even innerIterations takes), from its first iteration `it` up to the stage's
    budget `total` = inner x outer.  The counts are per pair.  So per (level, warp) stage, with n the largest count of any pair:
      - the launches' first iterations are 0, step, 2 step, ... without a gap, and the stages come coarsest level first, warp after warp;
      - the iterations the list covers, sum of max(0, min(step, total - it)), are at least n: no executed iteration lacks a launch;
      - a stage that ran its whole budget (n == total) is covered exactly: the sum equals n;
      - a stage that stopped early has at most three launches beyond the ceil(n / step) that carry its iterations: one in which a
        pair of a two-per-launch form replays its last iteration, one that no pair enters and that reports so, and one the host has
        enqueued before it reads that report (DEFAULT_LAG = 1 in the engine);
      - the list is as long as tf_stats.iter_launches, which the engine counts separately.
    An equality for every stage is not a property the list has: the host learns of a stop from the launch after it."""
    e.set_profile(0)
    base = np.array(e.calc_pairs(I0s, I1s))
    base_it, off_ms = e.last_iters(), e.last_stats["iter_ms"]
    e.set_profile(1)
    try:
        got = np.array(e.calc_pairs(I0s, I1s))
        it, st = e.last_iters(), e.last_stats
        lv, wp, first, ms = launch_profile(e)
    finally:
        e.set_profile(0)
    after = np.array(e.calc_pairs(I0s, I1s))
    after_ms = e.last_stats["iter_ms"]
    print(f"  iter_ms: {off_ms} before, {st['iter_ms']:.3f} profiled, {after_ms} after; {len(lv)} launch records, iter_launches {st['iter_launches']}", flush=True)
    same(got, base, "profiled against unprofiled")
    same(it, base_it, "their iteration counts")
    same(got, want, "profiled against the oracle")
    same(it, want_it, "its iteration counts against the oracle's")
    same(after, want, "unprofiled again")
    assert off_ms == 0 and after_ms == 0 and st["iter_ms"] > 0
    assert len(lv) == st["iter_launches"] and len(lv) > 0 and (ms >= 0).all()
    levels, warps = it.shape[1], it.shape[2]
    total = e.getInnerIterations() * e.getOuterIterations()
    step = 2 if e.getInnerIterations() % 2 == 0 else 1
    stages = [(l, w) for l in range(levels - 1, -1, -1) for w in range(warps)]
    cut = np.flatnonzero((np.diff(lv) != 0) | (np.diff(wp) != 0)) + 1
    parts = np.split(np.arange(len(lv)), cut)
    assert [(int(lv[p[0]]), int(wp[p[0]])) for p in parts] == stages, "the list's stages are not the solve's, coarsest level first"
    for (l, w), p in zip(stages, parts):
        n = int(it[:, l, w, 0].max())
        covered = int(np.clip(total - first[p], 0, step).sum())
        extra = len(p) - (n + step - 1) // step
        print(f"  level {l} warp {w}: {len(p)} launches cover {covered} iterations; executed, per pair {it[:, l, w, 0].tolist()}", flush=True)
        assert np.array_equal(first[p], step * np.arange(len(p))), f"level {l} warp {w}: first iterations {first[p].tolist()}"
        assert covered >= n, f"level {l} warp {w}: {n} iterations executed, the launches cover {covered}"
        if n == total:
            assert covered == total, f"level {l} warp {w}: the whole budget of {total} ran, the launches cover {covered}"
        else:
            assert 0 <= extra <= 3, f"level {l} warp {w}: {len(p)} launches for {n} iterations"


def profiling_changes_nothing(eng, torch, stream):
    z = eng.z
    check_profile(eng(), z["st_I0s"][:3], z["st_I1s"][:3], z["st_flow"][:3], z["st_iters"][:3])
    drained(stream, "profiled calls")


GROUPS = {
    "solves": (solves_are_the_oracles, two_handles_share_the_stream_and_close, profiling_changes_nothing),
    "order": (input_side_stream_order,),
    "chains": (seeded_and_chained_forms_alone, refusals_and_the_way_back),
    "study": (study_and_tail_calls,),
}


def run_group(torch, group, npz):
    """the child's main: every scenario of `group` on a side stream, then on the default stream"""
    z = dict(np.load(npz))
    torch.zeros(1, device="cuda:0")                          # torch initialises HIP before the first engine does
    torch.cuda.synchronize()
    shared = {}
    for kind in ("side", "default"):
        stream = Caller(torch, kind)
        for fn in GROUPS[group]:
            eng = Handles(z, stream, shared)
            print(f"{fn.__name__} [{kind}]", flush=True)
            t0 = time.perf_counter()
            try:
                with torch.cuda.stream(stream.torch_stream):
                    fn(eng, torch, stream)
                eng.close_all()
                torch.cuda.synchronize()
            except BaseException:
                traceback.print_exc()
                sys.stdout.flush()
                sys.stderr.flush()
                os._exit(1)                                  # at once: no handle is closed and nothing else is started behind a failure
            print(f"ok {fn.__name__} [{kind}] {time.perf_counter() - t0:.2f} s", flush=True)
    print(f"group {group} ok", flush=True)
