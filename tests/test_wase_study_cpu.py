"""Routing of bkgd_comp="WASE" studies to the one-call device forms (DenseFlow.calc_study_wase & co.), with stand-in models: no GPU."""
import logging

import numpy as np
import pytest


def _study():
    from tee_optical_flow_amd.synth import speckle_sequence
    g = speckle_sequence(7, 5, 24, 32)
    nparr = np.repeat(g[..., None], 3, axis=3)
    bk = np.zeros((5, 24, 32, 2), bool)
    bk[1:, :6] = True
    return nparr, bk


MD = {"pixel_spacing": 0.04, "frame_rate": 50.0, "R_wave_data_present": False, "R_times": None}


class _Recorder:
    """A model with the float16 study calls and the device WASE forms; every other study call raises."""
    device_payload = True
    device_wase = True

    def __init__(self):
        self.calls = []

    def _flow16(self, nparr):
        N, H, W, _ = nparr.shape
        return (np.arange(N * H * W * 2, dtype=np.float32).reshape(N, H, W, 2) / 64).astype(np.float16)

    def calc_study_wase_payload(self, nparr, bkgd_mask, scale=1.0, pad_last=True, echo=True):
        self.calls.append(("rgb", nparr, bkgd_mask, scale, pad_last, echo))
        return self._flow16(nparr), None, np.zeros(nparr.shape[0] - 1, np.float32)

    def calc_study_saliency_wase_payload(self, nparr, bkgd_mask, scale=1.0, pad_last=True, echo=True, map_dtype="f32"):
        self.calls.append(("saliency", nparr, bkgd_mask, scale, pad_last, echo, map_dtype))
        return -self._flow16(nparr), None, np.zeros(nparr.shape[0] - 1, np.float32)

    def _no(self, *a, **k):
        raise RuntimeError("a study call without the compensation was used under bkgd_comp='WASE'")
    calc_study_payload = submit_study_payload = calc_study_saliency_payload = calc_study = calc_batch = wase_compensate = _no


@pytest.mark.parametrize("no_saliency", [True, False])
def test_device_payload_with_wase_calls_the_one_call_form_once(caplog, no_saliency):
    from tee_optical_flow_amd import pipeline
    nparr, bk = _study()
    model = _Recorder()
    pipeline._payload_fallbacks.clear()
    with caplog.at_level(logging.WARNING, logger=pipeline.logger.name):
        out = pipeline.process_video(None, None, None, verbose=False, mode="RVIO_2class", bkgd_comp="WASE", no_saliency=no_saliency, nparr=nparr,
                                     metadata=MD, mask_dict={"bkgd": bk}, flow_model=model, payload="device", saliency_map="u8")
    assert not [r for r in caplog.records if "payload='device' not used" in r.getMessage()] and not pipeline._payload_fallbacks
    assert len(model.calls) == 1
    kind, frames, mask, scale, pad_last, echo = model.calls[0][:6]
    assert kind == ("rgb" if no_saliency else "saliency")
    assert np.array_equal(frames, nparr) and mask is bk
    assert scale == 0.04 * 50.0 and pad_last is True and echo is False          # no save_path: no file, no echo
    if not no_saliency:
        assert model.calls[0][6] == "u8"
    want = model._flow16(nparr)
    assert out.dtype == np.float16 and np.array_equal(out, want if no_saliency else -want)


def test_flow_for_study_takes_the_float32_one_call_form_on_the_host_path():
    from tee_optical_flow_amd import pipeline
    nparr, bk = _study()
    calls = []

    class Model:
        def calc_study_wase(self, nparr, bkgd_mask, scale=1.0, pad_last=False):
            calls.append(("rgb", bkgd_mask, scale, pad_last))
            return np.full((nparr.shape[0], 24, 32, 2), 3.0, np.float32), np.zeros(nparr.shape[0] - 1, np.float32)

        def calc_study_saliency_wase(self, nparr, bkgd_mask, scale=1.0, pad_last=False, map_dtype="f32"):
            calls.append(("saliency", bkgd_mask, scale, pad_last, map_dtype))
            return np.full((nparr.shape[0], 24, 32, 2), 4.0, np.float32), np.zeros(nparr.shape[0] - 1, np.float32)

        def _no(self, *a, **k):
            raise RuntimeError("the study was solved without its compensation")
        calc_study = calc_study_saliency = calc_batch = wase_compensate = _no

    out = pipeline.flow_for_study(None, Model(), {"bkgd": bk}, "WASE", 2.0, nparr_rgb=nparr)
    assert calls == [("rgb", bk, 2.0, True)] and out.shape == (5, 24, 32, 2) and (out == 3.0).all()
    out = pipeline.flow_for_study(None, Model(), {"bkgd": bk}, "WASE", 2.0, nparr_rgb=nparr, saliency=True, saliency_map="u8")
    assert calls[1:] == [("saliency", bk, 2.0, True, "u8")] and (out == 4.0).all()
    # and through process_video(payload="host")
    del calls[:]
    out = pipeline.process_video(None, None, None, verbose=False, mode="RVIO_2class", bkgd_comp="WASE", no_saliency=True, nparr=nparr, metadata=MD,
                                 mask_dict={"bkgd": bk}, flow_model=Model(), payload="host")
    assert len(calls) == 1 and calls[0][0] == "rgb" and calls[0][1] is bk and calls[0][2:] == (0.04 * 50.0, True)
    assert out.dtype == np.float32 and (out == 3.0).all()


def test_refusal_message_names_wase_for_a_model_without_device_wase():
    from tee_optical_flow_amd import pipeline

    class Plain:
        device_payload = True

    kind, msg = pipeline._device_payload_refused(Plain(), "WASE")
    assert kind == "bkgd_comp" and "WASE" in msg
    assert pipeline._device_payload_refused(_Recorder(), "WASE") is None
    assert pipeline._device_payload_refused(_Recorder(), "none") is None and pipeline._device_payload_refused(Plain(), "none") is None
    assert pipeline._device_payload_refused(None, "WASE") is None                # the folder walk before it has made its own DenseFlow


def test_dense_flow_declares_the_device_wase_forms():
    from tee_optical_flow_amd import _lib
    from tee_optical_flow_amd.dense_flow import DenseFlow
    assert DenseFlow.device_wase is True
    for name in ("calc_study_wase", "calc_study_wase_payload", "calc_study_saliency_wase", "calc_study_saliency_wase_payload"):
        assert callable(getattr(DenseFlow, name))
    assert {"tf_calc_seq_rgb_wase", "tf_calc_seq_saliency_wase"} <= set(_lib.EXPORTED_SYMBOLS)
