"""WASE background without a GPU: the summation order that csrc/teeflow_wase.hip.h implements,
restated in pure Python float32, equals numpy's np.mean bit for bit -- this is what pins the device kernels' algorithm
to the numpy the reference runs on (checked here against the installed numpy; the fixture in tests/golden was produced
under numpy 1.26)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NP_BUFSIZE, PW_BLOCK = 8192, 128


def pairwise(a):
    n = len(a)
    if n < 8:
        r = f32(0.0)
        for x in a:
            r = f32(r + x)
        return r
    if n <= PW_BLOCK:
        r = [f32(a[j]) for j in range(8)]
        lim = n - n % 8
        for i in range(8, lim, 8):
            for j in range(8):
                r[j] = f32(r[j] + a[i + j])
        res = f32(f32(f32(r[0] + r[1]) + f32(r[2] + r[3])) + f32(f32(r[4] + r[5]) + f32(r[6] + r[7])))
        for i in range(lim, n):
            res = f32(res + a[i])
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return f32(pairwise(a[:n2]) + pairwise(a[n2:]))


def numpy_order_mean(a):
    total = f32(0.0)
    for i in range(0, len(a), NP_BUFSIZE):
        total = f32(total + pairwise(a[i:i + NP_BUFSIZE]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return f32(np.float64(total) / np.float64(len(a)))


def leaves(n):
    """Leaves of numpy's split tree over n <= 8192 elements."""
    if n <= PW_BLOCK:
        return 1
    n2 = n // 2 - n // 2 % 8
    return leaves(n2) + leaves(n - n2)


def piece_lengths():
    """The 386 lengths inside one piece at which the restatement below, and the device (tests/test_gpu_wase.py, one flow per length),
    are checked: 1 ... 299, 80 seeded draws from 300 ... 8191 of which 10 are forced among the lengths of 7689 ... 8190 whose tree has
    65 leaves (a second round of the kernel's 64 leaf groups), the ends of that range and of the 64-leaf range before it, 8191, 8192."""
    rng = np.random.default_rng(386)
    second_round = [n for n in range(7689, 8191) if leaves(n) == 65]
    ks = list(range(1, 300)) + rng.integers(300, 8192, 70).tolist() + rng.choice(second_round, 10, replace=False).tolist()
    ks += [7688, 7689, 8184, 8185, 8190, 8191, 8192]
    assert len(ks) == 386 and sum(leaves(k) == 65 for k in ks) >= 10 and max(map(leaves, ks)) == 65
    return ks


MULTI_PIECE_LENGTHS = [8192 * j + r for j in (1, 2, 3) for r in (0, 1, 7, 8, 9, 127, 128, 129)]   # j full pieces and a last one of r


def test_restated_summation_order_equals_numpy_mean():
    assert np.getbufsize() == NP_BUFSIZE
    rng = np.random.default_rng(5)
    lengths = list(range(1, 140)) + [255, 256, 257, 1000, 4097, 8191, 8192, 8193, 16384, 20000, 65537, 100003]
    # the very points at which the device is checked (tests/test_gpu_wase.py; the C++ tree walks, tests/csrc/verify_wase_tree.cpp, take
    # every length to 8192), and the values around two and three pieces
    lengths += piece_lengths() + MULTI_PIECE_LENGTHS + [8192 * j + d for j in (2, 3) for d in (-1, 0, 1)]
    for n in lengths:
        a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f32)
        assert numpy_order_mean(a).tobytes() == np.mean(a).tobytes(), n


def test_wase_background_is_that_mean_over_all_frames_masks():
    from tee_optical_flow_amd.pipeline import wase_background
    rng = np.random.default_rng(6)
    N, H, W = 5, 12, 17
    flow = rng.standard_normal((H, W, 2)).astype(f32)
    flow[2:4, 3:9] = 0.0
    mask = rng.random((N, H, W, 2)) < 0.4
    masked = flow * mask
    a = masked.reshape(-1)
    a = a[a != 0]
    assert wase_background(flow, mask).tobytes() == numpy_order_mean(a).tobytes()
    # count of terms: every frame's mask counts, exact zeros of the flow do not
    assert len(a) == int((mask & (flow != 0)[None]).sum())


def test_tree_walks_of_the_piece_sum_kernel_for_every_length(tmp_path):
    """csrc/wase_tree.h, the two stack walks thread 0 of k_wase_piece_sums runs, against the recursive pairwise sum for n = 1 .. 8192:
    leaves tile [0, n), at most WASE_MAX_LEAVES of them, both stacks inside their 16 slots, sums equal bit for bit."""
    exe = tmp_path / "vwt"
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "tee_optical_flow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "verify_wase_tree.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "OK leaves 65 depth 8"          # the maxima over all lengths; the arrays hold 128 and 16


@pytest.mark.parametrize("seed", [1, 2])
def test_fuzzer_draw_on_the_host(seed):
    """tools/fuzz_wase.py --host: the generator of tests/test_gpu_fuzz_wase.py with the seeds it uses, no GPU: at most one case in ten
    is of the non-finite family, every other has a finite numpy background, and np.mean equals the restated order on every selection."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_wase.py"), "12", str(seed), "--host"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "12/12 cases identical" in r.stdout and "'non_finite': 1}" in r.stdout, r.stdout[-500:]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import fuzz_wase as F
    finally:
        sys.path.pop(0)
    for cases in (9, 10, 150, 155):
        fams = [F.family_of(seed, c) for c in range(cases)]
        assert fams.count(F.NON_FINITE) * 10 <= cases and set(fams) <= set(F.FAMILIES + (F.NON_FINITE,))
    assert set(F.family_of(seed, c) for c in range(150)) == set(F.FAMILIES + (F.NON_FINITE,))
