"""DualTVL1's chained sequence (include/teeflow.h, tf_chain_next): the cases and the CPU chain the device is compared with.  A helper
module shared by tests/test_tvl1_chain_cpu.py and tests/test_gpu_tvl1_chain.py: nothing here is collected.

The expected chain is the video idiom over tests/tvl1_init_cases.composed, the oracle's solve restated over its exported stages:
pair 0 from zero (composed(init=None), the oracle's own solve bit for bit), pair k from pair k-1's float32 flow."""
import functools

import numpy as np

from tests import tvl1_init_cases as IC
from tests import tvl1_ref64_cases as K

SEED = 5
# id -> (the case of tvl1_init_cases.CASES whose parameter overrides it takes, (H, W), frames)
CASES = {
    "odd": ("odd-37x53", (37, 53), 5),            # five levels, odd sizes on every one
    "one": ("one", (72, 88), 4),                  # one level: the seed is what the first stage reads
    "short": ("short-3x2", (97, 131), 4),         # three levels, two warps
    "trunc": ("trunc-24x40", (24, 40), 4),        # 24 -> 19 -> 15: two levels of five
}
TILES_TOO = ("one", "odd")                        # run once more with iter_variant 0


def overrides(cid):
    return IC.CASES[CASES[cid][0]][0]


@functools.lru_cache(maxsize=None)
def frames(cid):
    """uint8 [N, H, W] of a case, read-only"""
    from tee_optical_flow_amd.synth import speckle_sequence
    _, (H, W), N = CASES[cid]
    fr = np.ascontiguousarray(speckle_sequence(SEED, N, H, W))
    fr.setflags(write=False)
    return fr


def rgb_of(gray):
    """gray uint8 [N, H, W] -> RGB frames [N, H, W, 3] with three different channels (so that conditioning is more than a copy)"""
    g = gray.astype(np.int16)
    return np.stack([gray, np.clip(g + 9, 0, 255).astype(np.uint8), np.clip(g - 7, 0, 255).astype(np.uint8)], -1)


def composed_chain(O, fr, P, chained=True):
    """-> (flows float32 [N-1, H, W, 2], iters int32 [N-1, levels, warps, 2], levels): the loop flow = calc(fr[k], fr[k+1], flow) over
    composed; `chained=False`: every pair from zero"""
    flows, iters, prev, levels = [], [], None, 0
    for k in range(len(fr) - 1):
        prev, it, levels = IC.composed(O, fr[k], fr[k + 1], P, prev if chained else None)
        flows.append(prev)
        iters.append(it)
    return np.stack(flows), np.stack(iters), levels


_chains = {}


def chain_case(O, cid, chained=True):
    """composed_chain of a case; computed once per process and shared, read-only"""
    if (cid, chained) not in _chains:
        out = composed_chain(O, frames(cid), K.params(**overrides(cid)), chained)
        out[0].setflags(write=False)
        out[1].setflags(write=False)
        _chains[cid, chained] = out
    return _chains[cid, chained]
