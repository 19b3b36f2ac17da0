"""The chained sequence without a GPU: the CPU chain of tests/tvl1_chain_cases has the two properties the device tests lean on, and
pipeline._study_solve(chain=True) picks the chained cell of the model, or refuses.  Each test prints its figures before it asserts."""
import numpy as np
import pytest

from tests import tvl1_chain_cases as CC


@pytest.mark.parametrize("cid", list(CC.CASES))
def test_composed_chain_starts_plain_and_then_reads_its_seed(oracle, cid):
    """pair 0 is the unseeded composition (and the oracle's solve); every value of every later pair differs from the unseeded one, so
    "the seed was read" is a condition the reference meets on these inputs"""
    fr = CC.frames(cid)
    chain, cit, levels = CC.chain_case(oracle, cid)
    plain, pit, plevels = CC.chain_case(oracle, cid, chained=False)
    assert chain.shape == (len(fr) - 1,) + fr.shape[1:] + (2,) and chain.dtype == np.float32 and levels == plevels
    for k in range(len(chain)):
        print(cid, k, "values equal to the unseeded solve:", int(np.sum(chain[k] == plain[k])), "of", chain[k].size,
              "inner iterations", int(cit[k, ..., 0].sum()), "against", int(pit[k, ..., 0].sum()))
    assert np.array_equal(chain[0], plain[0]) and np.array_equal(cit[0], pit[0])
    assert np.array_equal(chain[0], oracle.tvl1_calc(fr[0], fr[1], oracle.default_params(**CC.overrides(cid))))
    for k in range(1, len(chain)):
        assert (chain[k] != plain[k]).all(), f"pair {k}"
        assert np.isfinite(chain[k]).all()


class _Recorder:
    """a model with DenseFlow's study grid that records the one call made on it"""
    device_unit_scale = device_payload = device_wase = device_chain = True
    algo = "TVL1"

    def __init__(self, flag=False):
        self.calls, self.flag, self.flag_at_call = [], flag, None

    def getUseInitialFlow(self):
        return self.flag

    def setUseInitialFlow(self, v):
        self.flag = bool(v)

    def __getattr__(self, name):
        if not name.startswith(("calc_", "submit_")):
            raise AttributeError(name)

        def cell(*a, **kw):
            self.calls.append((name, kw))
            self.flag_at_call = self.flag
            n = a[0].shape[0]
            out = np.zeros((n,) + a[0].shape[1:3] + (2,), np.float32)
            if name.startswith("submit_"):
                return 7
            if "payload" in name:
                return (out, None, None) if "wase" in name else (out, None)
            return (out, None) if "wase" in name else out
        return cell

    def wait(self, ticket):
        return np.zeros((4, 8, 8, 2), np.float32)

    def study_chunks(self, rgb, scale, flow_chunks, echo_chunks=None, **kw):
        self.calls.append(("study_chunks", dict(kw, scale=scale, flow_chunks=flow_chunks, echo_chunks=echo_chunks)))
        self.flag_at_call = self.flag
        return {"flow": "flow record", "echo": "echo record"}


CELLS = [
    (dict(payload=True, chunks=True), "study_chunks"),
    (dict(), "calc_study"), (dict(payload=True), "calc_study_payload"), (dict(bkgd_comp="WASE"), "calc_study_wase"),
    (dict(bkgd_comp="WASE", payload=True), "calc_study_wase_payload"), (dict(saliency=True), "calc_study_saliency"),
    (dict(saliency=True, bkgd_comp="WASE", payload=True), "calc_study_saliency_wase_payload"), (dict(submit=True), "submit_study"),
    (dict(submit=True, payload=True), "submit_study_payload"),
]


@pytest.mark.parametrize("kw,cell", CELLS, ids=[c for _, c in CELLS])
@pytest.mark.parametrize("flag", [False, True])
def test_study_solve_picks_the_chained_cell(monkeypatch, kw, cell, flag):
    """(the chunks form: study_chunks in the chunks h5py gives the datasets -- asked of a stand-in, the default interpreter has no h5py --
    and collect() returns the records)"""
    from tee_optical_flow_amd import hdf5_out, pipeline
    monkeypatch.setattr(hdf5_out, "auto_chunks", lambda shape, dtype: ("chunks of", tuple(shape), np.dtype(dtype)))
    rgb = np.zeros((4, 8, 8, 3), np.uint8)
    masks = {"bkgd": np.ones((4, 8, 8, 2), bool)}
    kw = dict(kw)
    bkgd = kw.pop("bkgd_comp", "none")
    for chain in (True, False):
        m = _Recorder(flag)
        collect = pipeline._study_solve(m, rgb, lambda: rgb[..., 0], masks, bkgd, 2.0, chain=chain, **kw)
        assert m.flag is flag, "the model's flag was not put back when the call on the model had returned"
        result = collect()
        (name, got), = m.calls
        assert name == cell and got.get("chain", False) is chain, (name, got)
        assert got["scale"] == 2.0
        if cell == "study_chunks":
            assert got["flow_chunks"] == ("chunks of", (4, 8, 8, 2), np.float16) and got["echo_chunks"] == ("chunks of", (4, 8, 8), np.float16)
            assert result == {"flow": "flow record", "echo": "echo record"}
        else:
            assert got["pad_last"] is True
        assert m.flag is flag, "the model's flag was not put back"
        assert m.flag_at_call is (True if chain else flag)


def test_study_solve_chains_calc_batch_where_that_is_the_models_all():
    from tee_optical_flow_amd import pipeline

    class Batch:
        device_chain, algo, flag = True, "TVL1", True

        def getUseInitialFlow(self):
            return self.flag

        def calc_batch(self, frames, **kw):
            self.kw = kw
            return np.zeros((len(frames) - 1, 8, 8, 2), np.float32)

    m = Batch()
    out = pipeline.flow_for_study(np.zeros((4, 8, 8), np.uint8), m, chain=True)
    assert m.kw == {"chain": True} and out.shape == (4, 8, 8, 2)
    pipeline.flow_for_study(np.zeros((4, 8, 8), np.uint8), m)
    assert m.kw == {}


def test_chain_is_refused_for_deepflow_and_for_a_model_without_it(tmp_path):
    from tee_optical_flow_amd import pipeline
    from tee_optical_flow_amd.exceptions import ConfigurationError

    class Plain:                                  # a cv2-like model: calc / calc_batch only
        def calc_batch(self, frames):
            raise AssertionError("solved")

    class Deep(_Recorder):
        algo = "deepflow"

    rgb = np.zeros((4, 8, 8, 3), np.uint8)
    deep = Deep()
    for model in (Plain(), deep):
        with pytest.raises(ConfigurationError, match="chain=True"):
            pipeline._study_solve(model, rgb, lambda: rgb[..., 0], None, "none", 1.0, chain=True)
        with pytest.raises(ConfigurationError, match="chain=True"):
            pipeline.flow_for_study(rgb[..., 0], model, chain=True)
        with pytest.raises(ConfigurationError, match="chain=True"):
            pipeline.process_video(None, None, mode="otsu", nparr=rgb, flow_model=model, chain=True)
        with pytest.raises(ConfigurationError, match="chain=True"):
            pipeline.process_folder(str(tmp_path), str(tmp_path / "out"), flow_model=model, chain=True)
    assert not deep.calls and deep.flag is False
    with pytest.raises(ConfigurationError, match="TVL1"):
        pipeline.process_video(None, None, mode="otsu", nparr=rgb, OF_algo="deepflow", chain=True)
    with pytest.raises(ConfigurationError, match="TVL1"):
        pipeline.process_folder(str(tmp_path), str(tmp_path / "out"), OF_algo="deepflow", chain=True)
    assert not (tmp_path / "out").exists(), "refused before any work"
