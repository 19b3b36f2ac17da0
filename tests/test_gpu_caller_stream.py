"""The engine on a caller's stream (include/teeflow.h, tf_set_stream; DenseFlow.set_stream(ptr, external=True)): what a PyTorch user
gets who runs it in stream order with their own work.  Every scenario of tests/caller_stream_cases.py runs twice, on a torch side stream
handed over as its cuda_stream and on the legacy default stream handed over as 0, and compares with the CPU: the C oracles, the oracle's
stages composed (seeded and chained solves) and the host twins of the tail calls -- never with the same handle on its own stream.

torch and the engine must share one HIP runtime, and in the pytest process the session's engine has usually initialised HIP first, so each
group of scenarios runs in a fresh child process that imports torch before the package (as tests/test_gpu_comm.py and
tests/test_gpu_tvl1_init.py do); one child at a time, each with its own time limit.  The expected results are computed here, once per
session, and handed to the child as an .npz under tmp_path.  Each test prints the child's figures before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import caller_stream_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, ROOT)
from tests import caller_stream_cases as S
S.run_group(torch, GROUP, NPZ)
"""

_built = {}


@pytest.fixture
def cases(oracle, tmp_path):
    """the inputs and the CPU's results of every scenario (computed once, shared, never written) as an .npz for the child"""
    if not _built:
        _built.update(S.build(oracle))
        for a in _built.values():
            a.setflags(write=False)
    path = str(tmp_path / "caller_stream.npz")
    np.savez(path, **_built)
    return path


def run_group(group, npz):
    script = CHILD.replace("ROOT", repr(ROOT)).replace("GROUP", repr(group)).replace("NPZ", repr(npz))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    print(r.stdout[-12000:])
    assert r.returncode == 0 and f"group {group} ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    for fn in S.GROUPS[group]:
        for kind in ("side", "default"):
            assert f"ok {fn.__name__} [{kind}]" in r.stdout, f"{fn.__name__} did not run on the {kind} stream"


def test_solves_sharing_closing_and_profiling_on_a_callers_stream(cases):
    """Scenarios 1, 3, 7 and the caller's-stream half of 8.  calc, calc_pairs into a pinned result (the overlapped copy-out: three
    sub-batches, so the wait for a staging half's last copy is reached) and into a pageable one (in order), calc_batch, float32 frames,
    the CUDA-class variant and DeepFlow give the oracle's bits and iteration counts, and the caller's stream is idle when each returns;
    a DualTVL1 and a DeepFlow handle called alternately on one stream are each exact, close() with the stream still set leaves the
    stream usable; profiling changes no bit (check_profile's docstring says what the launch list must show)."""
    run_group("solves", cases)


def test_device_calls_are_ordered_behind_the_work_that_makes_their_inputs(cases):
    """Scenario 2 (and 3): calc_pairs_device, calc_seq_device and calc_pairs_device with dinit_ptr, made with no synchronisation behind
    a long producer and the copies that fill the frames and the seeds, give the oracle's flows of the real frames; the control, the
    same calls on the handle's own stream, returns while the caller's stream is busy (asserted) and gives the zero flow of zero frames."""
    run_group("order", cases)


def test_seeded_chained_forms_refusals_and_the_way_back(cases):
    """Scenarios 4 and 6: calc_pairs(init=), calc_batch(chain=True) over two sub-batches and calc_chains with ragged chains cut over
    time are the composed oracle chains, solved by the handle alone; every tf_submit_* form is refused with TF_ERR_UNSUPPORTED and
    leaves no ticket, an armed chain flag is spent by the refused call, the next call is exact; back on the handle's own stream the
    lanes take a call of three sub-batches, submit_seq_device equals calc_seq_device and the oracle; a switch to the caller's stream
    with a job in flight leaves both results exact."""
    run_group("chains", cases)


def test_study_and_tail_calls_on_a_callers_stream(cases):
    """Scenario 5: condition_frames, calc_study, calc_study_payload, calc_study_saliency (u8 maps), calc_study_wase, otsu_masks,
    clean_masks, saliency_frames, and a study held by hold_next with held_av_centroids, held_radlong_project_param and
    held_polar_project_param, each byte-equal to its host twin or oracle (caller_stream_cases.build names them).  None of these calls
    has only a fixture for a reference, so none is compared with the handle back on its own stream."""
    run_group("study", cases)


def test_profiling_changes_nothing(engine, oracle):
    """Scenario 8 on the handle's own stream: calc_pairs of three 97x131 pairs (one sub-batch, which the handle solves itself, so the
    launch records are its own) with tf_set_profile(1) gives the bits and iteration counts of tf_set_profile(0) and of the oracle;
    iter_ms is positive while profiling and 0 before and after; the launch list agrees with the iteration counts in the sense
    check_profile's docstring works out."""
    from tee_optical_flow_amd.synth import speckle_pairs
    I0s, I1s = (np.ascontiguousarray(a) for a in speckle_pairs(range(20, 23), 97, 131))
    if _built:
        want, want_it = _built["st_flow"][:3], _built["st_iters"][:3]
    else:
        want, want_it = S._oracle_pairs(oracle, I0s, I1s)
    S.check_profile(engine, I0s, I1s, want, want_it)
