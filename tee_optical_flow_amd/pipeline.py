"""Study-level driver around the flow engine: the part of the reference's process_video() / process_folder() that sits
directly on either side of the hot path.

Reference: /root/reference/optical_flow/calculate_optical_flow.py
  :564-578  model construction          -> make_flow_model
  :584-600  per-pair loop, pad, scale   -> flow_for_study   (ONE batched engine call instead of N-1 cv2 calls)
  :627-660  calculate_optical_flow()    -> calculate_optical_flow (same signature/behaviour, incl. WASE quirks)
  :478-625  process_video()             -> process_video (same signature; `nparr=`/`metadata=` inject frames where the
                                           DICOM blob / pydicom are absent)
  :243-290  process_folder()            -> process_folder (same signature and chunk / skip / per-file isolation rules;
                                           studies are dealt round-robin over ranks and the gzip-9 HDF5 write of study k
                                           runs beside the solve of study k+1)
"""
import logging
import os
import traceback
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from contextlib import contextmanager, suppress
from dataclasses import dataclass, field, replace
from functools import partial

import numpy as np

from . import hdf5_out
from .config import default_optical_flow_config
from .dense_flow import DenseFlow
from .exceptions import ConfigurationError, DICOMReadError, OpticalFlowCalculationError
from .frames import (JPEG_BASELINE_TRANSFER_SYNTAX, JPEG_LOSSLESS_TRANSFER_SYNTAXES, JPEG_STATUS_TEXT, PHOTOMETRIC_FORMS, RLE_STATUS_TEXT,
                     RLE_TRANSFER_SYNTAX, condition_frames, encapsulated_frames, jpeg_decode_frame, jpeg_record, jpegll_decode_frame, jpegll_record,
                     rle_decode_frame, rle_record, ybr_full_to_rgb, ycc_to_rgb_libjpeg)

logger = logging.getLogger(__name__)


def make_flow_model(OF_algo="TVL1", config=None, device_id=0, tvl1_variant="cpu"):
    """Reference :564-578.  tvl1_variant='cpu' (default, the parity target) is the reference's non-CUDA branch:
    createOptFlow_DualTVL1() + setLambda(config.lambda_value) (:577-578).  tvl1_variant='cuda' APPROXIMATES what the
    reference runs on a CUDA box (:572-575): cv2.cuda.OpticalFlowDual_TVL1.create() with NOTHING set on it -- lambda_value is
    silently ignored there, and so it is here.  Parity of that variant is unpinned: it restates
    the CUDA class's four known differences from memory, not cuda::resize's sampling or nvcc's FMA contraction."""
    if config is None:
        config = default_optical_flow_config()
    if OF_algo == "TVL1":
        if tvl1_variant == "cuda":
            return DenseFlow(device_id=device_id, variant="cuda")
        m = DenseFlow(device_id=device_id)
        m.setLambda(config.lambda_value)
        return m
    if OF_algo == "deepflow":
        return DenseFlow(device_id=device_id, algo="deepflow")      # reference :568, all-default DeepFlow
    raise OpticalFlowCalculationError("OF_algo only supports deepflow or TVL1")


def wase_background(flow, bkgd_mask):
    """Reference :647-652 verbatim semantics: ONE scalar = mean of the non-zero entries of flow[h,w,c]*mask[n,h,w,c]
    broadcast over ALL n frames, taken over both components together (Appendix C.3).  Closed form of the O(N) numpy
    expression: sum(flow*cnt) / sum(cnt*[flow != 0]) with cnt = sum_n mask -- evaluated exactly as numpy would."""
    masked = flow * bkgd_mask
    return np.mean(masked[masked != 0])


def calculate_optical_flow(saliency_1, saliency_2, mask_dict, OF_model, bkgd_comp="none", OF_algo="TVL1"):
    """Drop-in for the reference function of the same name (:627-660)."""
    if OF_algo in ("deepflow", "TVL1"):
        flow = OF_model.calc(saliency_1, saliency_2, None)
    else:
        raise OpticalFlowCalculationError("OF_algo only supports deepflow or TVL1")
    return _compensate(flow, mask_dict, bkgd_comp)


def _compensate(flow, mask_dict, bkgd_comp):
    if bkgd_comp == "WASE":
        background = wase_background(flow, mask_dict["bkgd"])
    elif bkgd_comp == "none":
        background = 0
    else:
        raise OpticalFlowCalculationError(f"bkgd_comp value must be [WASE, none], got {bkgd_comp}!")
    return flow - background


_saliency_warned = [False]


def _check_chain(chain, model=None, OF_algo=None):
    """chain=True needs DualTVL1 and a model that solves a chained sequence (DenseFlow.device_chain): refused before any work."""
    if not chain:
        return
    if OF_algo == "deepflow" or getattr(model, "algo", None) == "deepflow":
        raise ConfigurationError("chain=True needs OF_algo='TVL1': DeepFlow takes no initial flow")
    if model is not None and not getattr(model, "device_chain", False):
        raise ConfigurationError(f"chain=True: the flow model ({type(model).__name__}) does not solve chained sequences "
                                 "(DenseFlow with useInitialFlow does)")


def flow_for_study(frames_u8, OF_model, mask_dict=None, bkgd_comp="none", conversion_factor=1.0, nparr_rgb=None, saliency=False,
                   saliency_map="f32", chain=False):
    """Reference :584-600 for already-conditioned uint8 frames [N,H,W]: N-1 flows, last one duplicated, scaled.
    All N-1 pairs are solved by ONE batched call (tf_calc_seq); background compensation (per pair) and the unit
    scale are applied in the reference's order: (flow - background) * conversion_factor.
    `saliency=True` is the no_saliency=False branch (:559-560, :586): the frames' fine-grained saliency maps, computed on the
    device from `nparr_rgb`, are what the solver sees -- `saliency_map` "f32" (default): as CV_32F in [0,1], what computeSaliency()
    returns under the reference's opencv-contrib >= 4.5 (DualTVL1 then scales by 255 in float, DeepFlow takes [0,1] frames as they
    are); "u8": the 8-bit maps (opencv-contrib 3.x).  Parity of the whole branch is UNPINNED (oracle/saliency_oracle.c).
    `chain=True`: the video idiom instead of the reference's loop -- every pair starts from the flow of the pair before it (_study_solve)."""
    return _study_solve(OF_model, nparr_rgb, lambda: frames_u8, mask_dict, bkgd_comp, conversion_factor, saliency=saliency, saliency_map=saliency_map,
                        chain=chain)()


@contextmanager
def _chain_armed(model, chain):
    """A chained call on `model` is made with useInitialFlow set: set here where it is not, and put back when the call has returned."""
    arm = chain and not model.getUseInitialFlow()
    if arm:
        model.setUseInitialFlow(True)
    try:
        yield
    finally:
        if arm:
            model.setUseInitialFlow(False)


def _study_solve(model, rgb, gray_frames, mask_dict, bkgd_comp, factor, saliency=False, saliency_map="f32", payload=False, echo=False, submit=False,
                 chain=False, hold=False, chunks=False):
    """The one place that picks a study's call on the model: -> collect, a callable that returns the study's flow array [N,H,W,2], scaled
    by `factor` and the last flow repeated (`payload`: the pair (float16 flow array, float16 echo or None) of the study file).  rgb: the
    study's uint8 RGB frames, or None; gray_frames: () -> the conditioned frames, asked for only where calc_batch is the model's all.
    The model's study methods form a grid, calc_study[_saliency][_wase][_payload] (DenseFlow has every cell).  The cell asked for is
    used where the model has it: it compensates, scales and repeats the last flow itself -- `submit`: as submit_study[_payload], solved
    while the caller goes on, where the model offers that form.  Without it, and never under `payload`: the model's unscaled float32
    cell calc_study[_saliency], or calc_batch on the conditioned frames; then wase_compensate (or numpy's _compensate), the repeat and
    the scale on the host, in the reference's order (flow - background) * factor.
    `chain`: the same cell, chained (DenseFlow's chain=True: pair 0 from zero, pair k from pair k-1's flow; about N-1 single-pair solves
    per study).  The model is used with useInitialFlow set -- set for the call on the model where it is not, and put back (_chain_armed):
    a submitted job keeps the parameters it was queued with.  DeepFlow, or a model without `device_chain`, raises ConfigurationError.
    `hold` (with `payload`, never with `submit`): the payload also stays held on the model's device (hold=True of its payload cells).
    `chunks` (with `payload`, never with `submit` or `hold`; a plain RGB study): model.study_chunks in the chunks h5py gives the study's
    datasets; collect() returns the records {"flow": record, "echo": record} and no array."""
    _check_chain(chain, model)

    def call(name, *args, **kwargs):
        with _chain_armed(model, chain):
            return getattr(model, name)(*args, **kwargs)
    if bkgd_comp not in ("WASE", "none"):
        raise OpticalFlowCalculationError(f"bkgd_comp value must be [WASE, none], got {bkgd_comp}!")
    wase = bkgd_comp == "WASE"
    plain = "calc_study_saliency" if saliency else "calc_study"
    cell = plain + ("_wase" if wase else "") + ("_payload" if payload else "")
    kw = {"map_dtype": saliency_map} if saliency else {}
    ckw = {"chain": True} if chain else {}                       # (a model without the capability never sees the word)
    kw.update(ckw)
    if saliency and not payload:
        if rgb is None or not hasattr(model, plain):
            raise OpticalFlowCalculationError("no_saliency=False needs the device engine (DenseFlow.calc_study_saliency) and the "
                                              "study's frames; there is no CPU saliency path")
        if not _saliency_warned[0]:
            _saliency_warned[0] = True
            logger.warning("no_saliency=False: the saliency preprocessing (StaticSaliencyFineGrained, map handed over as %s) is a restatement of "
                           "opencv-contrib that no OpenCV output pins; files written on this branch are not verified against the reference's", saliency_map)
    if chunks:
        shape = rgb.shape[:3]
        records = call("study_chunks", rgb, factor, hdf5_out.auto_chunks(shape + (2,), np.float16), hdf5_out.auto_chunks(shape, np.float16), **ckw)
        return lambda: records
    # (device_unit_scale is asked of the plain gray cell alone: every later cell was born with `scale` and `pad_last`)
    if payload or (rgb is not None and hasattr(model, cell) and (cell != "calc_study" or getattr(model, "device_unit_scale", False))):
        if payload:
            kw["echo"] = echo
            if hold:
                kw["hold"] = True
        if submit and not hold and cell in ("calc_study", "calc_study_payload") and hasattr(model, cell.replace("calc", "submit")):
            # conditioning now, the solve queued on the engine's lanes: the next study's solve is on the GPU while this one finishes
            ticket = call(cell.replace("calc", "submit"), rgb, scale=factor, pad_last=True, **kw)
            return lambda: model.wait(ticket)
        got = call(cell, rgb, *((mask_dict["bkgd"],) if wase else ()), scale=factor, pad_last=True, **kw)
        if wase:                                                 # (the backgrounds are not kept)
            got = got[:2] if payload else got[0]
        return lambda: got
    if rgb is not None and hasattr(model, plain):
        flows = call(plain, rgb, **kw)                           # conditioning (:588) or saliency maps (:586) + all pairs on the device
    else:
        flows = call("calc_batch", gray_frames(), **ckw)         # float32 [N-1,H,W,2]
    compensates = wase and hasattr(model, "wase_compensate")
    if compensates:                                              # device: O(N^2 H W) products, numpy's summation order kept
        flows, _ = model.wase_compensate(flows, mask_dict["bkgd"], scale=factor)   # (flow - background) * factor
    elif wase:
        flows = np.stack([_compensate(flows[i], mask_dict, "WASE") for i in range(flows.shape[0])])
    flows = np.concatenate([flows, flows[-1:]], axis=0)          # copy last optical flow (:599)
    result = flows if compensates else flows * factor            # (:600)
    return lambda: result


_payload_fallbacks = set()          # kinds of reason already logged ("model", "bkgd_comp", "frames")


def _check_payload(payload):
    if payload not in ("host", "device"):
        raise ConfigurationError(f"payload must be 'host' or 'device', not {payload!r}")


def _is_rgb_u8(nparr):
    """uint8 RGB frames [N,H,W,3]: what the device's study calls take"""
    return nparr.ndim == 4 and nparr.shape[3] == 3 and nparr.dtype == np.uint8


def _device_payload_refused(model, bkgd_comp, nparr=None):
    """Why payload="device" cannot serve, as (kind, message) (None: it can): the model must offer the float16 study calls (DenseFlow.device_payload),
    a study with background compensation needs a model that compensates on the device too (DenseFlow.device_wase; without it WASE works on
    float32 flows on the host path), and its frames -- once read -- must be uint8 RGB."""
    if model is not None and not getattr(model, "device_payload", False):
        return "model", f"the flow model ({type(model).__name__}) does not offer the float16 study calls"
    # (no model yet: the walk makes a DenseFlow, which offers both)
    if bkgd_comp != "none" and not (bkgd_comp == "WASE" and (model is None or getattr(model, "device_wase", False))):
        return "bkgd_comp", f"bkgd_comp={bkgd_comp!r} works on float32 flows"
    if nparr is not None and not _is_rgb_u8(nparr):
        return "frames", f"the frames are not uint8 RGB [N,H,W,3] but {nparr.dtype} {nparr.shape}"
    return None


def _payload_served(payload, model, bkgd_comp, nparr=None):
    """Whether payload="device" is asked for and serves.  Where it is refused: one message per kind of reason, whatever the shapes or
    names in it (a folder of gray studies of many sizes says it once)."""
    refused = _device_payload_refused(model, bkgd_comp, nparr) if payload == "device" else None
    if refused is not None and refused[0] not in _payload_fallbacks:
        _payload_fallbacks.add(refused[0])
        logger.warning(f"payload='device' not used, the host casts flow and echo to float16 instead: {refused[1]}")
    return payload == "device" and refused is None


_deflate_fallbacks = set()          # reasons already logged


def _check_deflate(deflate, payload):
    if deflate not in ("host", "device"):
        raise ConfigurationError(f"deflate must be 'host' or 'device', not {deflate!r}")
    if deflate == "device" and payload != "device":
        raise ConfigurationError("deflate='device' compresses the payload the engine holds: it needs payload='device'")


def _deflate_fallback(reason):
    if reason is not None and reason not in _deflate_fallbacks:
        _deflate_fallbacks.add(reason)
        logger.warning(f"deflate='device' not used, the host compresses the file's chunks instead: {reason}")


def _held_records(model, flow_shape, echo_shape):
    """{"flow": record, "echo": record} of the study `model` holds (held_deflate: nothing is uploaded), in the chunks h5py gives the
    datasets; made now, while the study is held."""
    records = {"flow": model.held_deflate("flow", hdf5_out.auto_chunks(flow_shape, np.float16))}
    if echo_shape is not None:
        records["echo"] = model.held_deflate("echo", hdf5_out.auto_chunks(echo_shape, np.float16))
    return records


def _device_deflater(model, flow16, echo16):
    """create_gzip9's `deflater` for a study whose payload `model` holds: the records of `flow` and `echo` from the held arrays.  The
    masks stay with the host's thread pool, like the waveforms and whatever else the file gets: a mask is long runs, where zlib skips what
    the device's search walks position by position (profiles/r22_deflate.txt: the device is slower on masks than 16 host threads)."""
    records = _held_records(model, flow16.shape, None if echo16 is None else echo16.shape)

    def deflater(name, data, chunks):
        rec = records.get(name)
        return rec if rec is not None and tuple(rec["shape"]) == data.shape and tuple(rec["chunks"]) == tuple(chunks) and np.dtype(rec["dtype"]) == data.dtype else None
    return deflater


def _records_deflater(records):
    """create_gzip9's `deflater` over records made elsewhere (the walk's writer stage): a dataset's record as it is -- one that does not
    fit its dataset is create_gzip9's to refuse -- and None for every other dataset (masks, waveforms: the host's threads)."""
    return lambda name, data, chunks: records.get(name)


@dataclass
class _HandOver:
    """One study on its way to its file: all that save_optical_flow_to_hdf5 needs, from the solve to the writer (process_video writes it
    in line, process_folder's writer stage in a thread or a worker process).  `flow` and `echo` are arrays, hdf5_out.Described where
    `records` ({dataset name: record}, deflate="device" in the walk) are all there is of them, or shared-memory descriptors in transit;
    `echo` None: the writer makes it from `nparr`.  `deflater` (process_video(deflate="device")) writes in line and is never pickled."""
    save_path: str
    flow: object
    nparr: object
    mask_dict: dict
    metadata: dict
    waveforms: dict
    patient_id: object
    heart_rate: object
    config: object
    mode: str
    no_saliency: bool
    include_waveforms: bool
    save_mask_subset: object = None
    echo: object = None
    nframes: object = None
    records: dict = field(default_factory=dict)
    deflater: object = None

    def write(self):                              # (the writer is looked up now: tools replace it on its module)
        deflate = self.deflater or (_records_deflater(self.records) if self.records else None)
        hdf5_out.save_optical_flow_to_hdf5(self.save_path, self.flow, self.nparr, self.mask_dict, self.metadata, self.waveforms, self.patient_id,
                                           self.heart_rate, self.config, self.mode, self.no_saliency, self.include_waveforms,
                                           self.save_mask_subset, echo=self.echo, nframes=self.nframes, deflate=deflate)

    def over_arrays(self, fn):
        """A copy with fn(value, dtype) in every slot that can be a big array -- the one list of them: the walk packs them into shared
        memory by it, the worker maps them back.  dtype: what the file stores the slot as, None where that is the value's own."""
        return replace(self, flow=fn(self.flow, np.float16), echo=fn(self.echo, np.float16), nparr=fn(self.nparr, None),
                       mask_dict={k: fn(v, None) for k, v in self.mask_dict.items()},
                       records={k: dict(rec, blob=fn(rec["blob"], np.uint8)) for k, rec in self.records.items() if rec is not None})


def _study_route(model, nparr, from_device, deflate, plain, walk):
    """How a study's `flow` and `echo` get to its file, as (route, reason): "host" -- float32 flows, the host casts --, "device" -- the
    float16 payload calls (`from_device`: payload="device" serves), the host compresses --, and under `deflate` (deflate="device", a file
    is written) "hold" -- the payload call with hold=True, then held_deflate -- or, in the walk, "chunks" -- study_chunks, a `plain` RGB
    study on a model with `device_study_chunks`: no float16 array on the host.  reason: None, or why the host compresses after all, the
    first that holds in the caller's order (`walk`: process_folder's; else process_video's, which has the arrays anyway)."""
    name, holds = type(model).__name__, hasattr(model, "held_deflate")
    chunks = walk and plain and getattr(model, "device_study_chunks", False) and hasattr(model, "study_chunks")
    unserved = (not from_device, "payload='device' does not serve this study")
    if walk:
        reasons = [(not _is_rgb_u8(nparr), "the frames are not uint8 RGB [N,H,W,3]"),
                   (not (getattr(model, "device_payload", False) and (chunks or holds)), f"the flow model ({name}) has neither study_chunks nor held_deflate"),
                   unserved,                      # (next: `echo`, half of `flow`; the record route has no array for HDF5's filter)
                   (int(np.prod(nparr.shape[:3])) * 2 < hdf5_out.MIN_PARALLEL_BYTES,
                    "`flow` or `echo` is under create_gzip9's min_parallel_bytes and goes through HDF5's own filter")]
    else:
        reasons = [unserved, (not holds, f"the flow model ({name}) has no held_deflate")]
    why = next((text for met, text in reasons if met), None) if deflate else None
    return ("chunks" if chunks else "hold", None) if deflate and why is None else ("device" if from_device else "host", why)


def _prep_frames(nparr, flipLR):
    """Reference :533-548: greyscale stacks become RGB, optional left-right flip."""
    nparr = np.asarray(nparr)
    if nparr.ndim == 3 and nparr.shape[0] > 1:
        nparr = np.repeat(nparr[..., None], 3, axis=3)
    if flipLR:
        nparr = np.flip(nparr, axis=2)
    return nparr


_frames_fallbacks = set()           # reasons already logged


def _check_frames(frames):
    if frames not in ("host", "device"):
        raise ConfigurationError(f"frames must be 'host' or 'device', not {frames!r}")


def _frames_fallback(reason):
    if reason not in _frames_fallbacks:
        _frames_fallbacks.add(reason)
        logger.warning(f"frames='device' not used, the host prepares the frames instead: {reason}")


def _stored_form(arr, photometric):
    """The device form (frames.FRAME_FORMS) of pixel data `arr` as stored under `photometric` (None: by its shape), or None with the
    reason why the host has to prepare it."""
    arr = np.asarray(arr)
    if photometric is None:
        photometric = "MONOCHROME2" if arr.ndim == 3 else "RGB"
    form = PHOTOMETRIC_FORMS.get(str(photometric))
    if form is None:
        return None, f"PhotometricInterpretation {photometric!r} has no device form"
    if arr.dtype != np.uint8 or arr.ndim != (3 if form == "GRAY" else 4) or (form != "GRAY" and arr.shape[3] != 3) or min(arr.shape) < 1:
        return None, f"the pixel data is not uint8 {'[N,H,W]' if form == 'GRAY' else '[N,H,W,3]'}"
    if form == "GRAY" and arr.shape[0] < 2:
        return None, "a grey stack of one frame stays grey (reference :533-536)"
    return form, None


def _stored_to_rgb(arr, photometric, path=None):
    """What read_study gives for pixel data as stored: the twin's conversion for the YBR forms, the data itself for RGB and grey; any
    other interpretation is the study file's own converter's (read again through read_study)."""
    if photometric in ("YBR_FULL", "YBR_FULL_422"):
        return ybr_full_to_rgb(arr)
    if photometric in (None, "RGB", "MONOCHROME2") or path is None:
        return arr
    return read_study(path)[0]


@dataclass(frozen=True)
class RleFrames:
    """A study's pixel data as a DICOM RLE Lossless file stores it (transfer syntax 1.2.840.10008.1.2.5, 8-bit samples): frame i is the
    len[i] bytes at blob[off[i]:] (blob uint8, off uint64, len uint32: frames.rle_record's), `shape` = (N, H, W), `samples` 1 or 3 a
    pixel.  `photometric`: the dataset's PhotometricInterpretation where dicom_rle_frames read one.  What frames="device" hands to
    DenseFlow.hold_frames_rle in an array's place; decode() is the host's way to the array (frames.rle_decode_frame, the twin)."""
    blob: object
    off: object
    len: object
    shape: tuple
    samples: int
    photometric: object = None

    @property
    def record(self):
        return self.blob, self.off, self.len

    def decode(self):
        """-> uint8 [N,H,W] (samples == 1) or [N,H,W,samples], as pydicom's pixel_array gives them; DICOMReadError for a frame that does not decode"""
        N, H, W = self.shape
        blob = np.asarray(self.blob, np.uint8)
        out = np.empty((N, H, W) if self.samples == 1 else (N, H, W, self.samples), np.uint8)
        for i in range(N):
            a = int(self.off[i])
            out[i], status = rle_decode_frame(blob[a:a + int(self.len[i])].tobytes(), H, W, self.samples)
            if status:
                raise DICOMReadError(f"RLE Lossless frame {i} did not decode: status {status} ({RLE_STATUS_TEXT[status]})")
        return out


def _rle_refusal(ds):
    """Why a dataset in the RLE Lossless transfer syntax is not decoded from its stored bytes, or None"""
    bits, samples = int(getattr(ds, "BitsAllocated", 0) or 0), int(getattr(ds, "SamplesPerPixel", 0) or 0)
    if bits != 8:
        return f"RLE Lossless pixel data with BitsAllocated = {bits}: only 8-bit samples are decoded from the stored bytes"
    if samples not in (1, 3):
        return f"RLE Lossless pixel data with SamplesPerPixel = {samples}: only 1 or 3 samples are decoded from the stored bytes"
    return None


def _is_rle(ds):
    return str(getattr(getattr(ds, "file_meta", None), "TransferSyntaxUID", "")) == RLE_TRANSFER_SYNTAX


def dicom_rle_frames(ds):
    """The pixel data of an 8-bit RLE Lossless dataset as it is stored -> RleFrames; None for any other dataset (another transfer
    syntax, samples that are not 8-bit, a sample count other than 1 or 3), which is read through its pixel_array as ever.  A pure
    function of any dataset-like object: reads file_meta.TransferSyntaxUID, PixelData, Rows, Columns, SamplesPerPixel, NumberOfFrames
    (1 where absent), BitsAllocated and PhotometricInterpretation; frames.encapsulated_frames cuts PixelData into frames.  No pydicom."""
    if not _is_rle(ds) or _rle_refusal(ds) is not None:
        return None
    N, H, W = int(getattr(ds, "NumberOfFrames", 1) or 1), int(ds.Rows), int(ds.Columns)
    blob, off, ln = rle_record(encapsulated_frames(ds.PixelData, N))
    return RleFrames(blob, off, ln, (N, H, W), int(ds.SamplesPerPixel), str(getattr(ds, "PhotometricInterpretation", "")) or None)


def _rle_form(rle, photometric):
    """_stored_form for RLE frames: the device form of their planes under `photometric` (None: by the sample count), or None with the reason"""
    if photometric is None:
        photometric = "MONOCHROME2" if rle.samples == 1 else "RGB"
    form = PHOTOMETRIC_FORMS.get(str(photometric))
    if form is None:
        return None, f"PhotometricInterpretation {photometric!r} has no device form"
    if rle.samples != (1 if form == "GRAY" else 3):
        return None, f"PhotometricInterpretation {photometric!r} with {rle.samples} samples a pixel"
    if form == "GRAY" and rle.shape[0] < 2:
        return None, "a grey stack of one frame stays grey (reference :533-536)"
    return form, None


_rle_fallbacks = set()              # reasons already logged


def _rle_fallback(reason):
    if reason not in _rle_fallbacks:
        _rle_fallbacks.add(reason)
        logger.warning(f"RLE Lossless pixel data not decoded on the device, the host decodes it instead: {reason}")


# ---- JPEG Baseline pixel data as stored (transfer syntax 1.2.840.10008.1.2.4.50, 8-bit samples) ----------------------------------------
JPEG_COLOR_ROUTES = ("libjpeg", "dicom")


@dataclass(frozen=True)
class JpegFrames(RleFrames):
    """A study's pixel data as a DICOM JPEG Baseline file stores it: RleFrames' fields, each frame a full interchange stream
    (frames.jpeg_record's record).  `color`: how Y, Cb, Cr become RGB under PhotometricInterpretation YBR_FULL / YBR_FULL_422 --
    "libjpeg" (the default: libjpeg's fixed-point tables, what a Pillow-backed reader yields) or "dicom" (the float inverse of PS3.3
    C.7.6.3.1.2, frames.ybr_full_to_rgb).  Which of the two equals pydicom's ds.pixel_array depends on the handler pydicom picks:
    unpinned.  What frames="device" hands to DenseFlow.hold_frames_jpeg in an array's place; decode() is the host's way."""
    color: str = "libjpeg"

    def decode(self):
        """-> the streams' own components, upsampled, no colour transform: uint8 [N,H,W] (samples == 1) or [N,H,W,samples]; by PIL
        where it imports and takes the stream, otherwise by the twin frames.jpeg_decode_frame (slow); DICOMReadError for a frame that
        does not decode"""
        N, H, W = self.shape
        blob = np.asarray(self.blob, np.uint8)
        out = np.empty((N, H, W) if self.samples == 1 else (N, H, W, self.samples), np.uint8)
        for i in range(N):
            a = int(self.off[i])
            buf = blob[a:a + int(self.len[i])].tobytes()
            arr = _pil_components(buf, out.shape[1:])
            if arr is None:
                arr, status = jpeg_decode_frame(buf, H, W, self.samples)
                if status:
                    raise DICOMReadError(f"JPEG Baseline frame {i} did not decode: status {status} ({JPEG_STATUS_TEXT[status]})")
            out[i] = arr
        return out


def _pil_components(buf, shape):
    """One JPEG stream's own components by PIL on libjpeg-turbo (the decoder the device equals), or None where PIL does not import, is
    built on another libjpeg (libjpeg 9 upsamples the chroma differently: measured, up to 88 counts on a 4:2:0 stream), does not take
    the stream or gives another shape -- the twin decides then"""
    try:
        import io
        from PIL import Image, features
        if not features.check_feature("libjpeg_turbo"):
            return None
        im = Image.open(io.BytesIO(buf))
        if im.format != "JPEG" or im.mode not in ("L", "RGB", "YCbCr"):
            return None
        if im.mode != "L":
            im.draft("YCbCr", None)
            if im.mode != "YCbCr":
                return None
        arr = np.asarray(im)
    except Exception:                                                      # (whatever PIL makes of a malformed stream: the twin's status is the answer)
        return None
    return arr if arr.shape == tuple(shape) and arr.dtype == np.uint8 else None


def _jpeg_refusal(ds):
    """Why a dataset in the JPEG Baseline transfer syntax is not decoded from its stored bytes, or None"""
    bits, samples = int(getattr(ds, "BitsAllocated", 0) or 0), int(getattr(ds, "SamplesPerPixel", 0) or 0)
    if bits != 8:
        return f"JPEG Baseline pixel data with BitsAllocated = {bits}: only 8-bit samples are decoded from the stored bytes"
    if samples not in (1, 3):
        return f"JPEG Baseline pixel data with SamplesPerPixel = {samples}: only 1 or 3 samples are decoded from the stored bytes"
    return None


def _is_jpeg(ds):
    return str(getattr(getattr(ds, "file_meta", None), "TransferSyntaxUID", "")) == JPEG_BASELINE_TRANSFER_SYNTAX


def dicom_jpeg_frames(ds, jpeg_color="libjpeg"):
    """The pixel data of an 8-bit JPEG Baseline dataset as it is stored -> JpegFrames; None for any other dataset (another transfer
    syntax, samples that are not 8-bit, a sample count other than 1 or 3), which is read through its pixel_array as ever.  A pure
    function of any dataset-like object, as dicom_rle_frames: frames.encapsulated_frames cuts PixelData into frames.  No pydicom."""
    if jpeg_color not in JPEG_COLOR_ROUTES:
        raise ConfigurationError(f"jpeg_color must be one of {JPEG_COLOR_ROUTES}, not {jpeg_color!r}")
    if not _is_jpeg(ds) or _jpeg_refusal(ds) is not None:
        return None
    N, H, W = int(getattr(ds, "NumberOfFrames", 1) or 1), int(ds.Rows), int(ds.Columns)
    blob, off, ln = jpeg_record(encapsulated_frames(ds.PixelData, N))
    return JpegFrames(blob, off, ln, (N, H, W), int(ds.SamplesPerPixel), str(getattr(ds, "PhotometricInterpretation", "")) or None, jpeg_color)


def _jpeg_form(jf, photometric):
    """-> (device form, colour route of hold_frames_jpeg, None) for JPEG frames under `photometric` (None: the frames' own, else by the
    sample count), or (None, None, the reason).  MONOCHROME2 -> GRAY; RGB -> RGB, no transform; YBR_FULL / YBR_FULL_422 -> YBR_FULL,
    through libjpeg's tables (jf.color "libjpeg") or the DICOM float inverse ("dicom")."""
    photometric = photometric or jf.photometric or ("MONOCHROME2" if jf.samples == 1 else "RGB")
    form, why = _rle_form(jf, photometric)
    if why is not None:
        return None, None, why
    return form, ("libjpeg" if form == "YBR_FULL" and jf.color == "libjpeg" else "none"), None


def _jpeg_host(jf, photometric):
    """JPEG frames decoded on the host -> (array, the photometric it is now stored under): under the libjpeg route YBR data comes
    back as RGB (None), as a Pillow-backed reader returns it; otherwise the components under their interpretation"""
    photometric = photometric or jf.photometric
    arr = jf.decode()
    if jf.color == "libjpeg" and photometric in ("YBR_FULL", "YBR_FULL_422") and jf.samples == 3:
        return ycc_to_rgb_libjpeg(arr), None
    return arr, (photometric if photometric in PHOTOMETRIC_FORMS else None)


_jpeg_fallbacks = set()             # reasons already logged


def _jpeg_fallback(reason):
    if reason not in _jpeg_fallbacks:
        _jpeg_fallbacks.add(reason)
        logger.warning(f"JPEG Baseline pixel data not decoded on the device, the host decodes it instead: {reason}")


# ---- JPEG Lossless pixel data as stored (SOF3, predictor 1; transfer syntaxes 1.2.840.10008.1.2.4.70 and .57, 8-bit samples) ------------
@dataclass(frozen=True)
class JpegLosslessFrames(RleFrames):
    """A study's pixel data as a DICOM JPEG Lossless file stores it: RleFrames' fields, each frame a full interchange stream with an
    SOF3 frame header (frames.jpegll_record's record).  The codec applies no colour transform: the samples are what
    PhotometricInterpretation says, as RLE Lossless planes are.  What frames="device" hands to DenseFlow.hold_frames_jpeg_lossless in an
    array's place; decode() is the host's way."""

    def decode(self):
        """-> the encoded arrays: uint8 [N,H,W] (samples == 1) or [N,H,W,samples]; by PIL where it imports on libjpeg-turbo, takes the
        stream and gives the right shape and mode, otherwise by the twin frames.jpegll_decode_frame (slow); DICOMReadError for a frame
        that does not decode"""
        N, H, W = self.shape
        blob = np.asarray(self.blob, np.uint8)
        out = np.empty((N, H, W) if self.samples == 1 else (N, H, W, self.samples), np.uint8)
        for i in range(N):
            a = int(self.off[i])
            buf = blob[a:a + int(self.len[i])].tobytes()
            arr = _pil_lossless(buf, out.shape[1:])
            if arr is None:
                arr, status = jpegll_decode_frame(buf, H, W, self.samples)
                if status:
                    raise DICOMReadError(f"JPEG Lossless frame {i} did not decode: status {status} ({JPEG_STATUS_TEXT[status]})")
            out[i] = arr
        return out


def _pil_lossless(buf, shape):
    """One JPEG Lossless stream's samples by PIL on libjpeg-turbo (3.0 and later decode SOF3), or None where PIL does not import, is
    built on another libjpeg, does not take the stream, or gives another mode (L for one sample, RGB -- the samples as stored, no colour
    transform -- for three) or shape: the twin decides then.  On a valid stream the two agree, there being one decoding; what libjpeg makes
    of a malformed one (it masks a sample to 8 bits where the twin gives status 3) is not pinned."""
    try:
        import io
        from PIL import Image, features
        if not features.check_feature("libjpeg_turbo"):
            return None
        im = Image.open(io.BytesIO(buf))
        if im.format != "JPEG" or im.mode != ("L" if len(shape) == 2 else "RGB"):
            return None
        arr = np.asarray(im)
    except Exception:                                                      # (whatever PIL makes of a malformed stream: the twin's status is the answer)
        return None
    return arr if arr.shape == tuple(shape) and arr.dtype == np.uint8 else None


def _jpegll_refusal(ds):
    """Why a dataset in a JPEG Lossless transfer syntax is not decoded from its stored bytes, or None"""
    bits, samples = int(getattr(ds, "BitsAllocated", 0) or 0), int(getattr(ds, "SamplesPerPixel", 0) or 0)
    if bits != 8:
        return f"JPEG Lossless pixel data with BitsAllocated = {bits}: only 8-bit samples are decoded from the stored bytes"
    if samples not in (1, 3):
        return f"JPEG Lossless pixel data with SamplesPerPixel = {samples}: only 1 or 3 samples are decoded from the stored bytes"
    return None


def _is_jpegll(ds):
    return str(getattr(getattr(ds, "file_meta", None), "TransferSyntaxUID", "")) in JPEG_LOSSLESS_TRANSFER_SYNTAXES


def dicom_jpegll_frames(ds):
    """The pixel data of an 8-bit JPEG Lossless dataset (either transfer syntax of frames.JPEG_LOSSLESS_TRANSFER_SYNTAXES) as it is
    stored -> JpegLosslessFrames; None for any other dataset (another transfer syntax, samples that are not 8-bit, a sample count other
    than 1 or 3), which is read through its pixel_array as ever.  A pure function of any dataset-like object, as dicom_jpeg_frames:
    frames.encapsulated_frames cuts PixelData into frames.  No pydicom."""
    if not _is_jpegll(ds) or _jpegll_refusal(ds) is not None:
        return None
    N, H, W = int(getattr(ds, "NumberOfFrames", 1) or 1), int(ds.Rows), int(ds.Columns)
    blob, off, ln = jpegll_record(encapsulated_frames(ds.PixelData, N))
    return JpegLosslessFrames(blob, off, ln, (N, H, W), int(ds.SamplesPerPixel), str(getattr(ds, "PhotometricInterpretation", "")) or None)


_jpegll_fallbacks = set()           # reasons already logged


def _jpegll_fallback(reason):
    if reason not in _jpegll_fallbacks:
        _jpegll_fallbacks.add(reason)
        logger.warning(f"JPEG Lossless pixel data not decoded on the device, the host decodes it instead: {reason}")


class _DeviceFrames:
    """A study's frames held on the flow model's device (frames="device"): the token every device call takes, and the RGB for what
    still runs on the host, downloaded once.  `stored`: the pixel data as an array, or as RleFrames / JpegFrames / JpegLosslessFrames
    (the device decodes them)."""

    def __init__(self, model, stored, form, flip, color="none"):
        if isinstance(stored, JpegFrames):
            token = model.hold_frames_jpeg(stored.record, stored.shape[1], stored.shape[2], stored.samples, form, color=color, flip=flip)
        elif isinstance(stored, JpegLosslessFrames):
            token = model.hold_frames_jpeg_lossless(stored.record, stored.shape[1], stored.shape[2], stored.samples, form, flip=flip)
        elif isinstance(stored, RleFrames):
            token = model.hold_frames_rle(stored.record, stored.shape[1], stored.shape[2], stored.samples, form, flip=flip)
        else:
            token = model.hold_frames(stored, form, flip=flip)
        self.model, self.token, self._rgb = model, token, None

    def host(self):
        if self._rgb is None:
            self._rgb = self.model.download_frames()
        return self._rgb


def process_video(dcm_path, save_path, segmentor_model=None, verbose=True, mode="A4C", bkgd_comp="none", flipLR=False,
                  no_saliency=False, OF_algo="TVL1", save_mask_subset=None, include_waveforms=False, waveform_folder=None,
                  config=None, *, nparr=None, metadata=None, patient_id="", heart_rate=0, waveforms=None, flow_model=None,
                  mask_dict=None, _defer_save=None, saliency_map="f32", payload="host", chain=False, deflate="host", frames="host"):
    """Same positional signature as the reference (:478-483).  Keyword-only extras let a caller inject what the
    offline image cannot provide: `nparr` (frames instead of a DICOM), `metadata`, `mask_dict` (segmentation result),
    `flow_model`.  Returns the float32 flow array [N,H,W,2] that was written.  `payload="device"`: the engine hands over the file's
    float16 `flow` and `echo` (DenseFlow.calc_study_payload, or calc_study_wase_payload under bkgd_comp="WASE"; uint8 RGB frames, a model with
    `device_payload` and, for WASE, `device_wase` --
    otherwise the host path, with one logged reason) and the float16 array that was written is returned; the file is the same.
    `chain=True` (OF_algo="TVL1"): the study's pairs are solved as a chain, each from the flow before it (_study_solve); the file's layout
    and attributes are those of the plain solve.
    `deflate="device"` (needs payload="device"): the study is solved with hold=True and the file's gzip chunks are compressed on the
    device: `flow` and `echo`, from the held payload (DenseFlow.held_deflate); the masks and the waveforms stay with the host's
    threads (_device_deflater says why); the chunks are the bytes of zlib level 9 and a dataset under 1 MiB goes through HDF5's own filter
    either way (create_gzip9), so the file is the one deflate="host" writes.  Where payload="device" does not
    serve, or the model has no held_deflate, the host compresses, with one logged reason.
    `frames="device"`: the reference's frame preparation (:524-548: colour space, gray2rgb, flipLR) runs on the flow model's device.  The
    pixel data goes there once, as the file stores it (read_study_stored; DenseFlow.hold_frames), and the masks and the solve read it
    there: Otsu masks and the segmentor's glue where the model offers them, every study call.  What runs on the host -- a host
    segmentor, host Otsu, an `echo` the writer makes -- gets the RGB by one download.  YBR_FULL and YBR_FULL_422 convert as
    frames.ybr_full_to_rgb (parity with pydicom's converter is unpinned); any other interpretation, pixel data that is not uint8, or a
    model without hold_frames takes the host path with one logged reason per walk.  The file is the one frames="host" writes.
    8-bit RLE Lossless pixel data (read_study_stored gives it as RleFrames, taken before ds.pixel_array is touched; an .npz study may
    carry it in `nparr`'s place) is held from its compressed bytes (DenseFlow.hold_frames_rle: the device decodes it); a model without
    hold_frames_rle gets what frames.rle_decode_frame decodes, with one logged reason per walk, and frames="host" decodes it likewise.
    8-bit JPEG Baseline pixel data (JpegFrames: dicom_jpeg_frames, or an .npz with `jpeg_blob`, `jpeg_off`, `jpeg_len`, `rows`, `cols`,
    `samples`, `photometric`) is held likewise by DenseFlow.hold_frames_jpeg (_jpeg_form says in which form and by which colour
    route); a model without it, a refused dataset and a frame the device gives a status for take the host's decode (PIL where it
    imports, else frames.jpeg_decode_frame), with one logged reason per walk.  frames="host" and read_study read a DICOM file through
    ds.pixel_array as ever.
    8-bit JPEG Lossless pixel data (JpegLosslessFrames: dicom_jpegll_frames, or an .npz with `jpegll_blob`, `jpegll_off`, `jpegll_len`,
    `rows`, `cols`, `samples`, `photometric`) is held by DenseFlow.hold_frames_jpeg_lossless in the form _rle_form names, with the same
    three host fallbacks (PIL where it imports and takes the stream, else frames.jpegll_decode_frame), one logged reason per walk."""
    return _process_video_begin(dcm_path, save_path, segmentor_model, verbose, mode, bkgd_comp, flipLR, no_saliency, OF_algo, save_mask_subset,
                                include_waveforms, waveform_folder, config, nparr=nparr, metadata=metadata, patient_id=patient_id,
                                heart_rate=heart_rate, waveforms=waveforms, flow_model=flow_model, mask_dict=mask_dict, _defer_save=_defer_save,
                                saliency_map=saliency_map, payload=payload, chain=chain, deflate=deflate, frames=frames)()


def _process_video_begin(dcm_path, save_path, segmentor_model=None, verbose=True, mode="A4C", bkgd_comp="none", flipLR=False,
                         no_saliency=False, OF_algo="TVL1", save_mask_subset=None, include_waveforms=False, waveform_folder=None,
                         config=None, *, nparr=None, metadata=None, patient_id="", heart_rate=0, waveforms=None, flow_model=None,
                         mask_dict=None, _defer_save=None, saliency_map="f32", _submit=False, payload="host", chain=False, deflate="host",
                         frames="host", _photometric=None):
    """process_video in two halves: everything up to the flow solve, then a callable that collects the flows and does the rest (waveforms,
    hand-over to the HDF5 writer) and returns the flow array.  `_submit` (process_folder): where the engine offers it (gray-frame branch,
    no background compensation, a model the caller holds) the solve is only SUBMITTED here -- DenseFlow.submit_study, tf_submit_seq_rgb --
    so that the next study's solve is on the GPU while this one finishes."""
    _check_payload(payload)
    _check_deflate(deflate, payload)
    _check_chain(chain, flow_model, OF_algo)
    _check_frames(frames)
    if config is None:
        config = default_optical_flow_config()
    if mode == "otsu":
        if bkgd_comp != "none":
            raise ConfigurationError(f"bkgd_comp {bkgd_comp} is not supported in mode=otsu, can only support bkgd_comp=none")
        if save_mask_subset is not None:
            raise ConfigurationError("In mode=otsu, save_mask_subset must be None")
    if nparr is None:
        # the reference's own call shape, process_video(dcm_path, save_path, ...) (:519-531): read the study file.  `.dcm` needs
        # pydicom (DICOMReadError without it, like a failed _read_dicom_file); `.npy` / `.npz` are the offline injection formats.
        if frames == "device":                    # the pixel data as stored: converted, made RGB and flipped on the device below
            nparr, _photometric, md_file, pid_file, hr_file = read_study_stored(dcm_path)
        else:
            nparr, md_file, pid_file, hr_file = read_study(dcm_path)
        if metadata is None:
            metadata = md_file
        patient_id = patient_id or pid_file
        heart_rate = heart_rate or hr_file
    rle = nparr if isinstance(nparr, RleFrames) else None   # RLE Lossless or JPEG Baseline pixel data as stored: decoded on the device below, or here
    if rle is not None and frames == "host":
        if isinstance(rle, JpegFrames):
            nparr, still = _jpeg_host(rle, _photometric)
            nparr = ybr_full_to_rgb(nparr) if still in ("YBR_FULL", "YBR_FULL_422") else nparr
        else:
            nparr = rle.decode()
        rle = None
    if rle is None:
        nparr = np.asarray(nparr)
    if metadata is None:
        metadata = {"pixel_spacing": None, "frame_rate": None, "R_wave_data_present": False, "R_times": None}
    if frames == "host":
        nparr = _prep_frames(nparr, flipLR)
    ps, fr = metadata["pixel_spacing"], metadata["frame_rate"]
    conversion_factor = 1.0 if ps is None or fr is None else ps * fr
    if mask_dict is None and mode != "otsu":      # (otsu: made below, once the flow model exists -- on its device when it offers otsu_masks)
        if mode in ("A4C", "RVIO_2class"):
            if segmentor_model is None:
                raise ConfigurationError(f"mode={mode} needs segmentor_model (a module with image_encoder / prompt_encoder / "
                                         "mask_decoder, reference :47-88) or a precomputed mask_dict=")
        else:
            raise ConfigurationError(f"Input for mode must be [A4C, otsu, RVIO_2class], not {mode}.")
    own = flow_model is None
    model = make_flow_model(OF_algo, config) if own else flow_model
    walk = _defer_save is not None                # process_folder: the writer stage takes the study
    held = None                                   # frames="device": the study's frames on the model's device
    try:
        if isinstance(rle, JpegFrames):           # (frames="device")
            form, color, why = _jpeg_form(rle, _photometric)
            if why is None and not hasattr(model, "hold_frames_jpeg"):
                why = f"the flow model ({type(model).__name__}) has no hold_frames_jpeg"
            if why is None:
                try:
                    held = _DeviceFrames(model, rle, form, flipLR, color)
                    nparr = held.token
                except OpticalFlowCalculationError as e:                  # a frame whose status is not 0: the held frames are as they were
                    why = f"the device did not decode it ({e})"
            if why is not None:                   # the host decodes; what it gives goes the way of any stored array, below
                _jpeg_fallback(why)
                nparr, _photometric = _jpeg_host(rle, _photometric)
        elif isinstance(rle, JpegLosslessFrames):  # (frames="device")
            form, why = _rle_form(rle, _photometric)
            if why is None and not hasattr(model, "hold_frames_jpeg_lossless"):
                why = f"the flow model ({type(model).__name__}) has no hold_frames_jpeg_lossless"
            if why is None:
                try:
                    held = _DeviceFrames(model, rle, form, flipLR)
                    nparr = held.token
                except OpticalFlowCalculationError as e:                  # a frame whose status is not 0: the held frames are as they were
                    why = f"the device did not decode it ({e})"
            if why is not None:                   # the host decodes; what it gives goes the way of any stored array, below
                _jpegll_fallback(why)
                nparr = rle.decode()
        elif rle is not None:                     # (frames="device")
            form, why = _rle_form(rle, _photometric)
            if why is None and not hasattr(model, "hold_frames_rle"):
                why = f"the flow model ({type(model).__name__}) has no hold_frames_rle"
            if why is None:
                held = _DeviceFrames(model, rle, form, flipLR)
                nparr = held.token
            else:                                 # the twin decodes; what it gives goes the way of any stored array, below
                _rle_fallback(why)
                nparr = rle.decode()
        if frames == "device" and held is None:
            form, why = _stored_form(nparr, _photometric)
            if why is None and not hasattr(model, "hold_frames"):
                why = f"the flow model ({type(model).__name__}) has no hold_frames"
            if why is None:
                held = _DeviceFrames(model, nparr, form, flipLR)
                nparr = held.token                # (stands for the RGB frames in every device call: it has their shape and dtype)
            else:
                _frames_fallback(why)
                nparr = _prep_frames(np.asarray(_stored_to_rgb(nparr, _photometric, dcm_path)), flipLR)
        via_host = {"host_frames": held.host} if held is not None else {}     # (for what of the masks runs on the host: one download)
        if mask_dict is None and mode == "otsu":
            # reference :184-213, on the flow model's device when it offers it (DenseFlow.otsu_masks), else numpy / scipy on the host
            from .masks import predict_movie_thres
            mask_dict = predict_movie_thres(nparr, verbose=verbose, config=config, engine=model, **via_host)
        elif mask_dict is None:
            # reference :549-550; the masks are cleaned on the flow model's device when it offers it (DenseFlow.clean_masks)
            from .masks import predict_movie
            mask_dict = predict_movie(nparr, segmentor_model, mode=mode, verbose=verbose, config=config, engine=model, **via_host)
        rgb_u8 = _is_rgb_u8(nparr)
        from_device = _payload_served(payload, model, bkgd_comp, nparr)
        if not no_saliency and not rgb_u8:
            # the reference's default branch (:559-560, :586): cv2.saliency.StaticSaliencyFineGrained on every frame
            raise OpticalFlowCalculationError(f"no_saliency=False needs uint8 RGB frames [N,H,W,3], got {nparr.dtype} {nparr.shape}")
        route, why = _study_route(model, nparr, from_device, deflate == "device" and save_path is not None, no_saliency and bkgd_comp == "none", walk)
        _deflate_fallback(why)
        # the echo (from the upload the conditioning / saliency pass reads) only where a file is written; "hold" and "chunks": the study is
        # solved now, synchronously, and its chunks are made while it is held
        rgb = None if not rgb_u8 else nparr if held is not None else np.ascontiguousarray(nparr)
        solved = _study_solve(model, rgb, (lambda: condition_frames(held.host())) if held is not None else partial(condition_frames, nparr), mask_dict, bkgd_comp,
                              conversion_factor, saliency=not no_saliency, saliency_map=saliency_map, payload=route != "host",
                              echo=save_path is not None, submit=_submit and not own and route in ("host", "device"), chain=chain,
                              hold=route == "hold", chunks=route == "chunks")
        if route == "host":                       # collect(): the solve's result under the hand-over record's names
            collect = lambda: {"flow": solved()}
        elif route == "device":
            collect = lambda: dict(zip(("flow", "echo"), solved()))
        elif not walk:                            # "hold" in process_video, which returns the arrays: the deflater is made now, while the
            flow16, echo16 = solved()             # model holds the payload (and before a model of this call's own closes)
            held = {"flow": flow16, "echo": echo16, "deflater": _device_deflater(model, flow16, echo16)}
            collect = lambda: held
        else:                                     # the walk: the writer stage gets the records and what they describe, no array ("hold":
            shape = nparr.shape[:3]               # the arrays the call returned go here)
            made = {"flow": hdf5_out.Described(shape + (2,), np.float16), "echo": hdf5_out.Described(shape, np.float16),
                    "records": solved() if route == "chunks" else _held_records(model, shape + (2,), shape)}
            collect = lambda: made
        # (an `echo` the writer makes needs the RGB: fetched now, while these frames are the held ones)
        host_rgb = held.host() if held is not None and save_path is not None and route == "host" else None
    finally:
        if own:
            model.close()

    def finish():
        got = collect()
        # waveforms (reference :602-620): loaded and validated by the reference's rules unless the caller injected a result dict;
        # without a valid ECG and a valid arterial waveform the whole block is dropped (waveforms_present = False)
        waveform_results, with_waveforms = {}, include_waveforms
        if with_waveforms:
            from .waveforms import load_all_waveforms, waveforms_to_write
            waveform_results = waveforms if waveforms is not None else load_all_waveforms(dcm_path, waveform_folder, config, verbose)
            if not waveforms_to_write(waveform_results):
                with_waveforms = False
        if save_path is not None:
            frames_out, n_out = nparr, None
            if held is not None:                  # the writer needs the RGB only for an `echo` nobody has made
                n_out = nparr.shape[0]
                frames_out = None if got.get("echo") is not None else host_rgb
            out = _HandOver(save_path=save_path, nparr=frames_out, nframes=n_out, mask_dict=mask_dict, metadata=metadata, waveforms=waveform_results,
                            patient_id=patient_id, heart_rate=heart_rate, config=config, mode=mode, no_saliency=no_saliency,
                            include_waveforms=with_waveforms, save_mask_subset=save_mask_subset, **got)
            if _defer_save is not None:           # process_folder: the writer stage takes it while the next study is solved
                _defer_save(out)
            else:
                out.write()
        return got["flow"]
    return finish


def read_study(path):
    """Frames + metadata of one study file.  `.dcm` needs pydicom (absent in this image -> DICOMReadError, as the
    reference's _read_dicom_file failure, :520-522); `.npy` (uint8 [N,H,W] or [N,H,W,3]) and `.npz` (key `nparr`, optional
    `pixel_spacing`, `frame_rate`, `patient_id`, `heart_rate`, `photometric`) are the injection formats of the offline image.
    `photometric` (RGB, YBR_FULL, YBR_FULL_422, MONOCHROME2; without it the frames are RGB or grey, as ever) says how `nparr` is stored:
    YBR data is converted here as frames.ybr_full_to_rgb converts it, in pydicom's place.  In `nparr`'s place an .npz may carry RLE
    Lossless pixel data as stored -- `rle_blob`, `rle_off`, `rle_len`, `rows`, `cols`, `samples` (_npz_stored) -- which is decoded here
    by frames.rle_decode_frame, in pydicom's place likewise."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        return np.load(path, allow_pickle=False), None, "", 0
    if ext == ".npz":
        z = np.load(path, allow_pickle=False)
        arr, photometric = _npz_stored(z, path), _npz_photometric(z, path)
        if isinstance(arr, JpegFrames):                                   # (the offline stand-in for a Pillow-backed handler: PIL, or the twin)
            arr, photometric = _jpeg_host(arr, photometric)
        elif isinstance(arr, RleFrames):                                  # (the offline stand-in for pydicom's RLE handler: the twin)
            arr = arr.decode()
        if photometric in ("YBR_FULL", "YBR_FULL_422"):                   # (the offline stand-in for pydicom's converter: the twin)
            arr = ybr_full_to_rgb(arr)
        return (arr,) + _npz_study(z)
    ds, arr, pydicom = _read_dicom(path)
    return dicom_to_study(ds, arr, _pydicom_color_converter(pydicom))


def _npz_study(z):
    """(metadata, patient id, heart rate) of an .npz study"""
    md = {"pixel_spacing": float(z["pixel_spacing"]) if "pixel_spacing" in z else None,
          "frame_rate": float(z["frame_rate"]) if "frame_rate" in z else None, "R_wave_data_present": False, "R_times": None}
    return md, str(z["patient_id"]) if "patient_id" in z else "", int(z["heart_rate"]) if "heart_rate" in z else 0


def _npz_stored(z, path):
    """The pixel data of an .npz study as it is stored: `nparr`, or, in its place, RLE Lossless frames under `rle_blob`, `rle_off`,
    `rle_len` (frames.rle_record's) with `rows`, `cols` and `samples` -> RleFrames"""
    if "jpeg_blob" in z:
        return _npz_jpeg(z, path)
    if "jpegll_blob" in z:
        return _npz_jpegll(z, path)
    if "rle_blob" not in z:
        return z["nparr"]
    try:
        blob, off, ln = np.ascontiguousarray(z["rle_blob"], np.uint8), np.ascontiguousarray(z["rle_off"], np.uint64), np.ascontiguousarray(z["rle_len"], np.uint32)
        H, W, samples = int(z["rows"]), int(z["cols"]), int(z["samples"])
    except KeyError as e:
        raise DICOMReadError(f"Failed to read {path}: an RLE study needs rle_blob, rle_off, rle_len, rows, cols and samples ({e} is missing)") from e
    if (blob.ndim != 1 or off.ndim != 1 or off.shape != ln.shape or off.size < 1 or H < 1 or W < 1 or samples not in (1, 3)
            or int((off + ln.astype(np.uint64)).max()) > blob.size):
        raise DICOMReadError(f"Failed to read {path}: rle_off / rle_len do not describe frames of {H} x {W} x {samples} inside rle_blob's {blob.size} bytes")
    return RleFrames(blob, off, ln, (int(off.size), H, W), samples)


def _npz_jpeg(z, path):
    """JPEG Baseline frames of an .npz study under `jpeg_blob`, `jpeg_off`, `jpeg_len` (frames.jpeg_record's) with `rows`, `cols`,
    `samples` and, optionally, `photometric` and `jpeg_color` -> JpegFrames"""
    try:
        blob, off, ln = np.ascontiguousarray(z["jpeg_blob"], np.uint8), np.ascontiguousarray(z["jpeg_off"], np.uint64), np.ascontiguousarray(z["jpeg_len"], np.uint32)
        H, W, samples = int(z["rows"]), int(z["cols"]), int(z["samples"])
    except KeyError as e:
        raise DICOMReadError(f"Failed to read {path}: a JPEG study needs jpeg_blob, jpeg_off, jpeg_len, rows, cols and samples ({e} is missing)") from e
    color = str(z["jpeg_color"]) if "jpeg_color" in z else "libjpeg"
    if (blob.ndim != 1 or off.ndim != 1 or off.shape != ln.shape or off.size < 1 or H < 1 or W < 1 or samples not in (1, 3)
            or int((off + ln.astype(np.uint64)).max()) > blob.size or color not in JPEG_COLOR_ROUTES):
        raise DICOMReadError(f"Failed to read {path}: jpeg_off / jpeg_len / jpeg_color do not describe frames of {H} x {W} x {samples} inside jpeg_blob's {blob.size} bytes")
    return JpegFrames(blob, off, ln, (int(off.size), H, W), samples, _npz_photometric(z, path), color)


def _npz_jpegll(z, path):
    """JPEG Lossless frames of an .npz study under `jpegll_blob`, `jpegll_off`, `jpegll_len` (frames.jpegll_record's) with `rows`,
    `cols`, `samples` and, optionally, `photometric` -> JpegLosslessFrames"""
    try:
        blob, off, ln = (np.ascontiguousarray(z["jpegll_blob"], np.uint8), np.ascontiguousarray(z["jpegll_off"], np.uint64),
                         np.ascontiguousarray(z["jpegll_len"], np.uint32))
        H, W, samples = int(z["rows"]), int(z["cols"]), int(z["samples"])
    except KeyError as e:
        raise DICOMReadError(f"Failed to read {path}: a JPEG Lossless study needs jpegll_blob, jpegll_off, jpegll_len, rows, cols and samples ({e} is missing)") from e
    if (blob.ndim != 1 or off.ndim != 1 or off.shape != ln.shape or off.size < 1 or H < 1 or W < 1 or samples not in (1, 3)
            or int((off + ln.astype(np.uint64)).max()) > blob.size):
        raise DICOMReadError(f"Failed to read {path}: jpegll_off / jpegll_len do not describe frames of {H} x {W} x {samples} inside jpegll_blob's {blob.size} bytes")
    return JpegLosslessFrames(blob, off, ln, (int(off.size), H, W), samples, _npz_photometric(z, path))


def _npz_photometric(z, path):
    """The optional `photometric` key of an .npz study: how `nparr` is stored (None: as RGB or grey frames, as ever)."""
    if "photometric" not in z:
        return None
    photometric = str(z["photometric"])
    if photometric not in PHOTOMETRIC_FORMS:
        raise DICOMReadError(f"Failed to read {path}: photometric must be one of {sorted(PHOTOMETRIC_FORMS)}, got {photometric!r}")
    return photometric


def _stored_rle(ds, path):
    """An RLE Lossless dataset's pixel data as RleFrames, cut from PixelData before pixel_array is touched; None for any other dataset,
    and -- with one logged reason -- for RLE data the stored bytes are not decoded from (samples that are not 8-bit)"""
    if not _is_rle(ds):
        return None
    why = _rle_refusal(ds)
    if why is not None:
        _rle_fallback(why)
        return None
    try:
        return dicom_rle_frames(ds)
    except ValueError as e:
        raise DICOMReadError(f"Failed to read DICOM file: {path} ({e})") from e


def _stored_jpeg(ds, path):
    """_stored_rle for a JPEG Baseline dataset: JpegFrames, or None -- with one logged reason where the stored bytes are not decoded"""
    if not _is_jpeg(ds):
        return None
    why = _jpeg_refusal(ds)
    if why is not None:
        _jpeg_fallback(why)
        return None
    try:
        return dicom_jpeg_frames(ds)
    except ValueError as e:
        raise DICOMReadError(f"Failed to read DICOM file: {path} ({e})") from e


def _stored_jpegll(ds, path):
    """_stored_rle for a JPEG Lossless dataset: JpegLosslessFrames, or None -- with one logged reason where the stored bytes are not decoded"""
    if not _is_jpegll(ds):
        return None
    why = _jpegll_refusal(ds)
    if why is not None:
        _jpegll_fallback(why)
        return None
    try:
        return dicom_jpegll_frames(ds)
    except ValueError as e:
        raise DICOMReadError(f"Failed to read DICOM file: {path} ({e})") from e


def _read_dicom(path, stored=False):
    """`stored` (read_study_stored): the pixel data as the file stores it where that has a device form (_stored_rle, _stored_jpeg, _stored_jpegll, tried in that order)"""
    try:
        import pydicom
    except ImportError as e:
        raise DICOMReadError(f"Failed to read DICOM file: {path} (pydicom is not installed)") from e
    try:
        ds = pydicom.dcmread(path)
        arr = _stored_rle(ds, path) if stored else None
        if arr is None and stored:
            arr = _stored_jpeg(ds, path)
        if arr is None and stored:
            arr = _stored_jpegll(ds, path)
        if arr is None:
            arr = ds.pixel_array
    except (IOError, OSError, KeyError, AttributeError) as e:             # reference _read_dicom_file (:307-312) -> DICOMReadError (:521-522)
        raise DICOMReadError(f"Failed to read DICOM file: {path}") from e
    return ds, arr, pydicom


def read_study_stored(path):
    """read_study without the colour-space step: (pixel data as the file stores it, its PhotometricInterpretation or None, metadata,
    patient id, heart rate), for frames="device".  The interpretation is named only where the data is to be converted: pydicom's own
    should_change_PhotometricInterpretation_to_RGB(ds) decides that for a DICOM file, the `photometric` key for an .npz; None means RGB
    or grey frames by their shape.  8-bit RLE Lossless pixel data -- a DICOM file in that transfer syntax (dicom_rle_frames, taken
    before ds.pixel_array is touched), an .npz with `rle_blob` & co. -- comes as RleFrames, not decoded; JPEG Baseline and JPEG Lossless pixel data likewise as JpegFrames and
    JpegLosslessFrames."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        return np.load(path, allow_pickle=False), None, None, "", 0
    if ext == ".npz":
        z = np.load(path, allow_pickle=False)
        return (_npz_stored(z, path), _npz_photometric(z, path)) + _npz_study(z)
    ds, arr, pydicom = _read_dicom(path, stored=True)
    convert = pydicom.pixel_data_handlers.numpy_handler.should_change_PhotometricInterpretation_to_RGB(ds)
    _, md, pid, hr = dicom_to_study(ds, arr)
    return arr, str(ds.PhotometricInterpretation) if convert else None, md, pid, hr


def _pydicom_color_converter(pydicom):
    """The reference's colour-space step (calculate_optical_flow.py:524-526) as a callable (ds, arr) -> arr."""
    def convert(ds, arr):
        handlers = pydicom.pixel_data_handlers
        if handlers.numpy_handler.should_change_PhotometricInterpretation_to_RGB(ds):
            return handlers.convert_color_space(arr, ds.PhotometricInterpretation, "RGB")
        return arr
    return convert


def extract_dicom_metadata(ds):
    """The reference's _extract_dicom_metadata (calculate_optical_flow.py:315-365) on any dataset-like object, rule for rule:
    pixel spacing = PhysicalDeltaX of the first ultrasound region (tag 0018,6011), R-wave times when RWaveTimeVector is
    present and not a bare float, frame rate = CineRate as stored, else round(1000 / FrameTime), else
    round(1000 / FrameTimeVector[1]).  The rounding matters: conversion_factor = pixel_spacing * frame_rate scales every
    stored flow value (:538-541)."""
    md = {"pixel_spacing": None, "frame_rate": None, "R_times": None, "R_wave_data_present": False}
    try:
        md["pixel_spacing"] = ds[0x0018, 0x6011][0]["PhysicalDeltaX"].value
    except (KeyError, AttributeError, IndexError, TypeError):
        pass
    try:
        if type(ds.RWaveTimeVector) != float and ds.RWaveTimeVector is not None:      # noqa: E721  (the reference's own test)
            md["R_times"] = np.asarray(ds.RWaveTimeVector)
            md["R_wave_data_present"] = True
    except (AttributeError, KeyError, TypeError):
        pass
    try:
        md["frame_rate"] = ds.CineRate
    except (AttributeError, KeyError):
        try:
            md["frame_rate"] = np.round(1000 / float(ds.FrameTime))
        except (AttributeError, KeyError, ValueError, ZeroDivisionError):
            try:
                md["frame_rate"] = np.round(1000 / float(ds.FrameTimeVector[1]))
            except (AttributeError, KeyError, IndexError, ValueError, ZeroDivisionError):
                pass
    return md


def dicom_to_study(ds, arr, convert_color=None):
    """(frames, metadata, patient id, heart rate) of a read DICOM dataset, as process_video uses them (:524-531, :405-417):
    colour space converted to RGB when the dataset asks for it, metadata per extract_dicom_metadata."""
    if convert_color is not None:
        arr = convert_color(ds, arr)
    return arr, extract_dicom_metadata(ds), str(getattr(ds, "PatientID", "")), int(getattr(ds, "HeartRate", 0) or 0)


# ---- shared-memory transport between process_folder's stages -------------------------------------------------------------
# A 65-frame 512x512 study is ~50 MB of frames, ~35 MB of masks, 17 MB of `echo` and 68 MB of float16 flow.  Through the pools'
# pipes every one of those bytes is pickled, written, read and unpickled under the caller's interpreter lock (measured: 460 of a
# study's 700 ms in the caller's thread were spent receiving the reader stage's result).  Arrays above _SHM_MIN bytes therefore
# travel as POSIX shared-memory blocks: the producer fills a block and sends its name, the consumer maps it; the process_folder
# call that owns the study unlinks its blocks when the writer stage is done with them (or on any error).  If /dev/shm is too
# small for a study (containers often give it 64 MB; writing past the limit would be a SIGBUS), that study's arrays travel
# pickled, as before.
_SHM_MIN = int(os.environ.get("TEEFLOW_SHM_MIN_BYTES", 1 << 20))      # (the environment reaches spawned workers; tests lower it)
_SHM_MARGIN = 1 << 30
_shm_stats = {"mapped": 0, "created": 0}                             # blocks this process mapped / created (tests, tools)


def _shm_room(nbytes):
    try:
        st = os.statvfs("/dev/shm")
    except OSError:
        return False
    return st.f_bavail * st.f_frsize > 2 * nbytes + _SHM_MARGIN


def _shm_put(arr, dtype=None, keep=None):
    """ndarray -> ("shm", name, shape, dtype) with the data in a new shared-memory block, or the array itself when it is small / there
    is no room; as `dtype` where given, cast while copying (float32 flow -> the file's float16).  `keep`: the list that takes the block,
    still mapped, for its owner to release; without it this process's mapping is closed and the block stays."""
    arr = np.asarray(arr)
    view, blk, desc = _shm_new(arr.shape, dtype or arr.dtype)
    if blk is None:
        return np.ascontiguousarray(arr, dtype)
    try:
        view[...] = arr
    except BaseException:
        _shm_release([blk], unlink=True)
        raise
    del view
    if keep is None:
        blk.close()
    else:
        keep.append(blk)
    return desc


def _shm_new(shape, dtype):
    """An empty shared-memory array for the caller to fill: (view, block, descriptor), or (None, None, None) without room."""
    from multiprocessing import shared_memory
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    if nbytes < _SHM_MIN or not _shm_room(nbytes):
        return None, None, None
    blk = shared_memory.SharedMemory(create=True, size=nbytes)
    _shm_stats["created"] += 1
    return np.ndarray(shape, dtype, buffer=blk.buf), blk, ("shm", blk.name, tuple(shape), np.dtype(dtype).str)


def _is_shm(x):
    return isinstance(x, tuple) and len(x) == 4 and x[0] == "shm"


def _shm_get(x, blocks):
    """Descriptor -> ndarray view (its block is appended to `blocks`, which keeps the mapping alive); anything else passes through."""
    if not _is_shm(x):
        return x
    from multiprocessing import shared_memory
    blk = shared_memory.SharedMemory(name=x[1])
    blocks.append(blk)
    _shm_stats["mapped"] += 1
    return np.ndarray(x[2], np.dtype(x[3]), buffer=blk.buf)


def _shm_release(blocks, unlink):
    for blk in blocks:
        with suppress(OSError, BufferError):                 # a view is still alive somewhere: the mapping goes with it
            blk.close()
        if unlink:
            with suppress(OSError):
                blk.unlink()                                  # by name: works whatever is still mapped
    del blocks[:]


def _shm_unlink_names(descs):
    """Unlink blocks this process never mapped (a study that failed before its arrays were used)."""
    from multiprocessing import shared_memory
    for d in descs:
        if _is_shm(d):
            with suppress(OSError):
                _shm_release([shared_memory.SharedMemory(name=d[1])], unlink=True)


def _prepare_study_shm(reader, path, mode, flipLR, config, want_echo, otsu_ahead=True, frames="host"):
    """_prepare_study in a worker process, the big arrays returned as shared-memory descriptors."""
    nparr, md, pid, hr, masks_ahead, echo, photometric = _prepare_study(reader, path, mode, flipLR, config, want_echo, otsu_ahead,
                                                                                 *(("device",) if frames == "device" else ()))
    made = []
    try:
        if isinstance(nparr, RleFrames):                      # the blob travels as one uint8 array; the small tables go pickled
            nparr = replace(nparr, blob=_shm_put(nparr.blob)); made.append(nparr.blob)
        else:
            nparr = _shm_put(nparr); made.append(nparr)
        if masks_ahead is not None:
            packed = {}
            for k, v in masks_ahead.items():
                packed[k] = _shm_put(v); made.append(packed[k])
            masks_ahead = packed
        if echo is not None:
            echo = _shm_put(echo); made.append(echo)
    except BaseException:
        _shm_unlink_names(made)
        raise
    return nparr, md, pid, hr, masks_ahead, echo, photometric


def _save_study_shm(out):
    """Writer stage in a worker process: map what of the hand-over record arrived as descriptors, write the file, drop the mappings (the
    owner unlinks)."""
    blocks = []
    try:
        mapped = out.over_arrays(lambda x, dtype: _shm_get(x, blocks))
        mapped.write()
        del mapped
    finally:
        _shm_release(blocks, unlink=False)


def _default_stage_workers():
    """Worker processes per stage when the caller does not say: the deflate of a study is ~9 core-seconds and the mask stage ~0.6, the
    caller's thread needs a core of its own; 3 + 3 on the 16 cores of a one-GPU box (2 + 2 measured 747 ms per study, 3 + 3 616 ms,
    5 + 6 613 ms), never fewer than 2 nor more than 4 per stage."""
    try:
        cpus = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        cpus = os.cpu_count() or 4
    return max(2, min(4, cpus // 5))


class StudyWorkers:
    """Worker processes for process_folder's reader/mask and deflate/write stages, for callers that hold a flow model (or a segmentor on
    the GPU) across many calls: create this object BEFORE anything in the process touches the GPU -- starting a process from a
    GPU-initialised one is not safe on ROCm hosts -- and hand it to process_folder(workers=...).  process_folder(workers="process" /
    "auto") makes its own for one call, the same way: this class is the only place where worker processes are started."""

    def __init__(self, n_readers=None, n_writers=None):
        import multiprocessing as mp
        from concurrent.futures import ProcessPoolExecutor
        n_readers = _default_stage_workers() if n_readers is None else n_readers
        n_writers = _default_stage_workers() if n_writers is None else n_writers
        ctx = mp.get_context("spawn")
        self.n_readers, self.n_writers = max(1, n_readers), max(1, n_writers)
        self.readers = ProcessPoolExecutor(self.n_readers, mp_context=ctx)
        self.writers = ProcessPoolExecutor(self.n_writers, mp_context=ctx)
        try:                                              # make the pools start their processes now (an executor starts them lazily, on submit)
            for f in [self.readers.submit(os.getpid) for _ in range(self.n_readers)] + [self.writers.submit(os.getpid) for _ in range(self.n_writers)]:
                f.result()
        except BaseException:
            self.close()
            raise

    def close(self):
        self.readers.shutdown(wait=True)
        self.writers.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _StageThreads:
    """process_folder's stages in one thread each, in StudyWorkers' shape: reader 1 study ahead, n_writers + 1 = 2 waiting for the writer."""
    n_readers = n_writers = 1

    def __init__(self):
        self.readers, self.writers = ThreadPoolExecutor(1), ThreadPoolExecutor(1)

    close = StudyWorkers.close


def _prepare_study(reader, path, mode, flipLR, config, want_echo, otsu_ahead=True, frames="host"):
    """Reader stage of process_folder (module level: it also runs in worker processes).  Reads the study and -- for the Otsu mode,
    which is pure numpy/scipy -- computes its masks one study ahead of the GPU; with the solver at milliseconds per pair, this host
    work and the gzip-9 write are what a study costs.  `want_echo`: also the `echo` dataset (rgb2gray of the frames as float16,
    reference :400-402), so that the writer process does not need the RGB frames.
    frames="device" (the walk asks for it only with the default reader): the pixel data as stored and its PhotometricInterpretation
    (read_study_stored), nothing converted, flipped or made from it here -- the walk holds it on the device and makes masks and echo there
    or from one download."""
    if frames == "device":
        arr, photometric, md, pid, hr = read_study_stored(path)
        return arr, md, pid, hr, None, None, photometric
    nparr, md, pid, hr = reader(path)
    masks_ahead = None
    prepped = _prep_frames(nparr, flipLR)
    if mode == "otsu" and otsu_ahead:               # (process_folder(otsu_masks="device"): the walk makes them on the engine instead)
        from .masks import predict_movie_thres
        masks_ahead = predict_movie_thres(prepped, verbose=False, config=config)
    echo = None
    if want_echo:
        from .frames import rgb2gray
        echo = rgb2gray(prepped).astype(np.float16)
    return nparr, md, pid, hr, masks_ahead, echo, None


def _spawn_unsafe_reason(reader):
    """Why worker PROCESSES cannot serve this call, or None.  They are started with the spawn method (a process must never be forked
    from one that has initialised the GPU): the child re-imports the caller's `__main__` module from its file and unpickles `reader`.
    So (1) `reader` must pickle -- a lambda or a closure does not -- and (2) if `__main__` is a script, the call must come from under
    its `if __name__ == "__main__":` guard; otherwise the child would run the script's top level again and die in its bootstrap
    (every study would then come back as BrokenProcessPool).  Both are checked here, before a pool exists."""
    import pickle
    import sys
    try:
        pickle.dumps(reader)
    except Exception as e:
        return f"reader={reader!r} does not pickle ({type(e).__name__}: {e})"
    import __main__
    main_file = getattr(__main__, "__file__", None)
    if not main_file or not os.path.exists(main_file):
        return None                                           # python -c / interactive: spawn has no __main__ file to re-run
    fr = sys._getframe()
    while fr is not None and not (fr.f_code.co_name == "<module>" and fr.f_globals.get("__name__") == "__main__"):
        fr = fr.f_back
    if fr is None:
        return None                                           # not called from __main__'s module-level code (a thread, an importing tool)
    try:
        import ast
        with open(main_file) as fh:
            tree = ast.parse(fh.read())
    except (OSError, SyntaxError, ValueError):
        return f"cannot read {main_file} to see whether the call is under its __main__ guard"

    def is_guard(test):
        if not (isinstance(test, ast.Compare) and len(test.ops) == 1 and isinstance(test.ops[0], ast.Eq)):
            return False
        sides = [test.left, test.comparators[0]]
        return any(isinstance(x, ast.Name) and x.id == "__name__" for x in sides) and \
            any(isinstance(x, ast.Constant) and x.value == "__main__" for x in sides)
    for node in ast.walk(tree):
        if isinstance(node, ast.If) and is_guard(node.test) and node.body and node.body[0].lineno <= fr.f_lineno <= node.body[-1].end_lineno:
            return None
    return (f"the call comes from module-level code of the script {os.path.basename(main_file)} (line {fr.f_lineno}) outside an "
            "`if __name__ == '__main__':` block, which a spawned worker would run again")


def process_folder(dcm_folder, save_folder, segmentor_model=None, nchunks=10, chunk_index=0, mode="RVIO_2class", bkgd_comp="none",
                   flipLR=False, verbose=True, recalculate=False, no_saliency=True, OF_algo="TVL1", save_mask_subset=None,
                   include_waveforms=False, waveform_folder=None, pixel_spacing=None, frame_rate=None, process_subset=False,
                   file_subset_list=(), *, rank=0, world=1, extensions=("dcm",), reader=read_study, flow_model=None, config=None,
                   device_id=0, workers="auto", n_readers=None, n_writers=None, studies_in_flight=2, otsu_masks="host", payload="host",
                   chain=False, deflate="host", frames="host"):
    """Drop-in for the reference's process_folder (:243-290), same positional signature and the same rules:
      * the folder listing is cut into `nchunks` slices of len // nchunks files, this call takes slice `chunk_index`
        (the remainder files are dropped, as the reference does -- SURVEY.md Appendix C.8);
      * a study whose `<name>.hdf5` exists is skipped unless `recalculate`;
      * every study runs inside its own try/except: a failure is logged, recorded and the walk goes on (:276-284);
      * files with another extension are skipped with a warning (reference: 'dcm' only; `extensions` widens that to the
        .npy/.npz injection formats);
      * like the reference, `pixel_spacing` / `frame_rate` are accepted and ignored, and `config` is not forwarded unless given.
    Beyond the reference: the slice is dealt round-robin over `world` ranks (one process per GPU, rank r takes files
    r, r+world, ...: no exchange is needed, studies are independent), one flow model serves all studies of the call, and
    the walk is a three-stage pipeline: the reader stage loads study k+1 (and computes its Otsu masks and the `echo` dataset), the
    caller's thread solves study k on the GPU, the writer stage deflates/writes study k-1.  `workers`: "process" runs the reader and
    writer stages in `n_readers` + `n_writers` worker PROCESSES (spawned here, before this call's first GPU call; the mask stage and
    the deflate both hold the interpreter lock, which is why threads bought 3 %), "thread" in one thread each, "auto" takes
    processes when this call creates the flow model itself (no `flow_model`, no `segmentor_model`: nothing in the caller's hands has
    initialised the GPU yet as far as this function can tell) and more than one study is to do.  `studies_in_flight` (2): a study's flow solve is
    submitted to the engine's lanes (tf_submit_seq_rgb) and collected only when the NEXT study's has been submitted, so the GPU goes from one
    study's solve to the next without waiting for this thread (1 = solve and collect study by study, as rounds 2-4 did).
    `otsu_masks` (mode="otsu" only): "host" (default) has the reader stage compute the Otsu masks one study ahead with numpy / scipy;
    "device" has the reader stage skip them, and the walk makes them on the flow model (DenseFlow.otsu_masks, tf_otsu_masks; a model
    without that method computes them on the host, in the caller's thread).  The files are the same either way.
    `payload`: "host" (default) receives float32 flows and casts them to the file's float16 on the host (while copying them to the writer
    stage), and makes `echo` in the reader stage or the writer; "device" has the engine hand over both float16 arrays
    (DenseFlow.submit_study_payload / calc_study_payload / calc_study_saliency_payload: rounded by the output kernel, half the download;
    the echo from the frames the conditioning pass uploads anyway) -- the reader stage then makes no echo and the hand-over to the
    writer stage is a plain copy.  It needs a model with `device_payload`, uint8 RGB frames and, for bkgd_comp="WASE", a model with `device_wase` (such
    studies are solved and compensated by one synchronous call, DenseFlow.calc_study_wase_payload); otherwise the host
    path serves, and the reason is logged once.  The files are the same either way.
    `chain=True` (OF_algo="TVL1"): every study is solved as a chain (process_video); the walk submits chained studies like plain ones,
    each one unit of the engine's lanes.
    `deflate`: "host" (default) has the writer stage compress every chunk of the file with zlib level 9; "device" (needs payload="device",
    else ConfigurationError) has the engine compress `flow` and `echo`, byte for byte what zlib level 9 makes of them, so the files are
    the same.  A plain RGB study on a model with `device_study_chunks` is solved straight into its chunks (DenseFlow.study_chunks): no
    float16 array exists on the host.  A saliency or WASE study is solved by its payload call with hold=True and compressed from the held
    payload (held_deflate).  Either way the writer stage receives the two records and the arrays' shapes and dtypes (in worker processes
    the compressed bytes travel as shared-memory blocks of the study's), and the masks, the waveforms and RWaveTime stay with the
    host's threads.  Such a study is solved synchronously, here, before the walk goes on: `studies_in_flight` has no effect for it
    (logged once).  The host compresses instead, with one logged reason per walk, where the model has neither route, the frames are not
    uint8 RGB, payload="device" does not serve the study, or `flow` or `echo` is under create_gzip9's min_parallel_bytes and so goes
    through HDF5's own filter.
    `frames`: "host" (default) has the reader stage prepare the frames (colour space, gray2rgb, flipLR; the reference's :524-548);
    "device" has it hand the pixel data over as stored (read_study_stored: the default `reader` only), and the walk holds it on the flow
    model once per study (DenseFlow.hold_frames), where it is converted, made RGB and flipped and where masks and solve read it
    (process_video's doc).  The reader stage then makes neither Otsu masks nor `echo` ahead: masks come from the device where
    otsu_masks="device" or the segmentor sits on the GPU, else from one download of the RGB.  The files are the same either way."""
    if otsu_masks not in ("host", "device"):
        raise ConfigurationError(f"otsu_masks must be 'host' or 'device', not {otsu_masks!r}")
    _check_payload(payload)
    _check_deflate(deflate, payload)
    _check_chain(chain, flow_model, OF_algo)
    _check_frames(frames)
    _frames_fallbacks.clear()                                       # one logged reason per walk
    _rle_fallbacks.clear()
    _jpeg_fallbacks.clear()
    _jpegll_fallbacks.clear()
    if deflate == "device":
        _deflate_fallbacks.clear()                                  # one logged reason per walk
        if studies_in_flight > 1:
            logger.info("process_folder: deflate='device' solves a study synchronously and compresses it while it is held: "
                        "studies_in_flight=%d has no effect for such studies", studies_in_flight)
    os.makedirs(save_folder, exist_ok=True)
    file_list = sorted(os.listdir(dcm_folder))                      # os.listdir order is arbitrary; sorted = same slices on every rank
    if process_subset:
        if len(file_subset_list) == 0:
            logger.error("ERROR! File subset list is empty!")
            return []
        file_list = [f for f in file_list if f in file_subset_list]
    if include_waveforms and waveform_folder is None:
        logger.error("ERROR if include_waveform is selected, must define waveform_folder!")
        return []
    split, todo = len(file_list) // nchunks, []
    for filename in file_list[chunk_index * split:(chunk_index + 1) * split][rank::world]:
        stem, ext = os.path.splitext(filename)
        save_path = os.path.join(save_folder, stem + ".hdf5")
        if os.path.exists(save_path) and not recalculate:
            if verbose:
                logger.debug(f"File {save_path} exists! Skipping file {filename}")
            continue
        if ext.lower().lstrip(".") not in extensions:
            logger.warning(f"File extension must be one of {extensions}, found {ext}, skipping")
            continue
        todo.append((filename, save_path))
    use_proc = (workers == "process" or (workers == "auto" and flow_model is None and segmentor_model is None)) and len(todo) > 1
    walk = _FolderWalk(dcm_folder, todo, reader, workers, use_proc, n_readers, n_writers, flow_model, (OF_algo, config, device_id),
                       studies_in_flight, verbose, otsu_ahead=otsu_masks == "host", payload=payload,
                       prepare_args=(mode, flipLR, config if config is not None else default_optical_flow_config()),
                       video_args=dict(segmentor_model=segmentor_model, verbose=verbose, mode=mode, bkgd_comp=bkgd_comp, flipLR=flipLR,
                                       no_saliency=no_saliency, OF_algo=OF_algo, save_mask_subset=save_mask_subset,
                                       include_waveforms=include_waveforms, waveform_folder=waveform_folder, config=config, payload=payload,
                                       chain=chain, deflate=deflate), frames=frames)
    try:
        walk.run()
    finally:
        walk.close()
    return walk.errors


class _Study:
    """One study of a folder walk: the reader stage's result, what of it this process holds in shared memory, what goes on to the writer."""

    def __init__(self, filename, save_path):
        self.filename, self.save_path = filename, save_path
        self.descs, self.blocks = [], []                  # the reader stage's shared-memory descriptors; the mappings this process holds
        self.nparr = self.masks = self.echo = None        # frames, Otsu masks, `echo`: views into `blocks`, or plain arrays
        self.mask_descs = self.echo_desc = None           # what the writer stage gets in their place
        self.md = self.pid = self.hr = self.finish = None  # metadata, patient id, heart rate; _process_video_begin's second half
        self.photometric = None                           # frames="device": how `nparr` is stored (read_study_stored)

    def take(self, prepared, mapped):
        """Unpack what _prepare_study / _prepare_study_shm returned (nothing else knows its layout); `mapped`: and map its blocks."""
        nparr, self.md, self.pid, self.hr, masks, echo, self.photometric = tuple(prepared) + (None,) * (7 - len(prepared))
        rle = isinstance(nparr, RleFrames)                    # (its blob is the array that travels)
        self.descs = [d for d in [nparr.blob if rle else nparr, echo] + list((masks or {}).values()) if _is_shm(d)]
        if mapped:
            self.echo_desc, self.mask_descs = echo, masks if masks is not None and any(_is_shm(v) for v in masks.values()) else None
            nparr = replace(nparr, blob=_shm_get(nparr.blob, self.blocks)) if rle else _shm_get(nparr, self.blocks)
            if masks is not None:
                masks = {k: _shm_get(v, self.blocks) for k, v in masks.items()}
            echo = _shm_get(echo, self.blocks)
        self.nparr, self.masks, self.echo = nparr, masks, echo
        return self

    def release(self):
        """Give the study's shared memory up: close and unlink what this process mapped or created, unlink by name what it never mapped."""
        held = {blk.name for blk in self.blocks}
        self.nparr = self.masks = self.echo = self.finish = None
        _shm_release(self.blocks, unlink=True)
        _shm_unlink_names([d for d in self.descs if d[1] not in held])
        self.descs = []


class _FolderWalk:
    """process_folder's three-stage walk over `todo` = [(filename, save_path)]: the reader stage is `stages.n_readers` studies ahead, this
    thread begins (submits) a study's solve and finishes the oldest of `in_flight`, the writer stage takes what finish() defers.
    Worker processes (`use_proc`: asked for, and more than one study to do) are started here, before run() creates the flow model."""

    def __init__(self, dcm_folder, todo, reader, workers, use_proc, n_readers, n_writers, flow_model, model_args, in_flight, verbose,
                 otsu_ahead, payload, prepare_args, video_args, frames="host"):
        self.dcm_folder, self.todo, self.reader, self.in_flight, self.verbose = dcm_folder, todo, reader, in_flight, verbose
        self.otsu_ahead, self.prepare_args, self.video_args = otsu_ahead, prepare_args, video_args
        self.model, self.own_model, self.model_args = flow_model, flow_model is None, model_args
        self.errors = []            # (filename, error string), process_folder's result
        self.futs = {}              # index into todo -> reader stage future nobody has taken yet
        self.studies = {}           # save_path -> _Study, from its reader result until its release
        self.begun = deque()        # studies whose solve is submitted and not yet collected
        self.pending = []           # (study, writer stage future)
        # stages: StudyWorkers or _StageThreads; owned: the walk's to give up for threads and to close; fallback: why threads after all
        self.stages, self.owned, self.fallback = workers, not isinstance(workers, StudyWorkers), None
        if self.owned:
            self.stages = _StageThreads()
            if use_proc and (why := _spawn_unsafe_reason(reader)) is not None:
                logger.warning(f"process_folder: worker processes not used, threads instead: {why}")
                self.fallback = why
            elif use_proc:
                try:
                    self.stages = StudyWorkers(min(_default_stage_workers() if n_readers is None else n_readers, len(todo)), n_writers)
                except Exception as e:
                    self.pools_failed(e)
        self.proc = isinstance(self.stages, StudyWorkers)
        # payload="device": the engine makes the echo, so the reader stage is asked for none (a study whose frames turn out not to be
        # uint8 RGB still takes the host path: its frames then travel to the writer, which makes the echo)
        self.device_echo = _payload_served(payload, flow_model, video_args["bkgd_comp"])
        # frames="device": the reader stage hands the pixel data over as stored (read_study_stored).  Only the default reader can: a
        # reader of the caller's returns frames the host has prepared already
        self.frames = frames
        if frames == "device" and reader is not read_study:
            _frames_fallback(f"reader={getattr(reader, '__name__', reader)!r} returns prepared frames; only the default reader gives the pixel data as stored")
            self.frames = "host"

    def failed(self, name, e, trace=False):
        logger.error(f"Error processing {name}: {e}")
        if trace and self.verbose:
            traceback.print_exc()
        self.errors.append((name, f"{type(e).__name__}: {e}"))

    def pools_failed(self, e):
        """Called under `except`: raise on unless `e` condemns worker pools of the walk's own, not the study -- a worker died, an
        argument or a result would not pickle; then the stages go on in threads, as rounds 2-3 ran them."""
        import pickle
        from concurrent.futures.process import BrokenProcessPool
        if not (self.owned and (isinstance(e, (BrokenProcessPool, pickle.PicklingError))
                                or (isinstance(e, (AttributeError, TypeError)) and "pickle" in str(e).lower()))):
            raise
        self.fallback = f"{type(e).__name__}: {e}"
        logger.warning(f"process_folder: worker processes failed ({self.fallback}); the reader and writer stages continue in threads")

    def submit(self, k):
        if k < len(self.todo) and k not in self.futs:
            self.futs[k] = self.stages.readers.submit(_prepare_study_shm if self.proc else _prepare_study, self.reader,
                                                      os.path.join(self.dcm_folder, self.todo[k][0]), *self.prepare_args, self.proc and not self.device_echo,
                                                      self.otsu_ahead, *(("device",) if self.frames == "device" else ()))

    def read(self, k, study):
        try:
            return study.take(self.futs.pop(k).result(), self.proc)
        except Exception as e:
            if not self.proc:
                raise
            self.pools_failed(e)
        # studies already handed to the writer pool are reaped (and reported) as they are, what the reader pool has ready is freed
        self.reap(block=True)
        self.drop_read_ahead(wait=False)
        for pool in (self.stages.writers, self.stages.readers):
            pool.shutdown(wait=False, cancel_futures=True)
        self.stages, self.proc = _StageThreads(), False
        self.submit(k)
        return study.take(self.futs.pop(k).result(), False)

    def drop_read_ahead(self, wait):
        """Reader results nobody took: free their blocks (`wait`: for every one of them; else only those that are there already)."""
        for k, fut in list(self.futs.items()):
            del self.futs[k]
            with suppress(Exception):
                if wait or (not fut.cancel() and fut.done()):
                    _Study(*self.todo[k]).take(fut.result(), mapped=False).release()

    @staticmethod
    def to_block(study, x, dtype):
        """`x` for the writer process: an array as `dtype` in a new shared-memory block of the study's (its descriptor; a plain array
        without room).  dtype None (frames and masks get no new block) and what is no array (None, hdf5_out.Described) pass through."""
        return x if dtype is None or x is None or isinstance(x, hdf5_out.Described) else _shm_put(x, dtype, study.blocks)

    def defer(self, study, out):
        """The study's hand-over record goes to the writer stage.  A writer process needs neither the RGB frames (the reader stage or the
        engine made `echo` from them) nor float32 flow (the file holds float16); what is big travels as shared-memory names: the flow
        goes straight into a new block (cast on the way if the engine handed float32 over), so do the engine's echo and, under
        deflate="device", the records' blobs (flow and echo are then hdf5_out.Described); the masks and the reader stage's `echo` stay
        in its blocks."""
        if self.proc:
            packed = out.over_arrays(partial(self.to_block, study))
            packed.nframes = out.nframes if out.nframes is not None else int(np.asarray(out.nparr).shape[0])
            if packed.echo is None:
                packed.echo = study.echo_desc
            if packed.echo is not None:
                packed.nparr = None
            if study.mask_descs is not None and out.mask_dict is study.masks:
                packed.mask_dict = study.mask_descs
            fut = self.stages.writers.submit(_save_study_shm, packed)
        else:
            fut = self.stages.writers.submit(out.write)
        self.pending.append((study, fut))

    def drop(self, study):
        self.studies.pop(study.save_path, None)
        study.release()

    def reap(self, block):
        # at most a few studies wait for the writer: a faster solver must not pile finished studies up in host memory
        while self.pending and (block or len(self.pending) > self.stages.n_writers + 1 or self.pending[0][1].done()):
            study, fut = self.pending.pop(0)
            try:
                fut.result()
            except Exception as e:                                   # the writer's failure belongs to that study
                self.failed(os.path.basename(study.save_path), e)
            self.drop(study)

    def finish_oldest(self):
        study, deferred = self.begun.popleft(), len(self.pending)
        try:
            study.finish()
        except Exception as e:
            self.failed(study.filename, e, trace=True)
        if len(self.pending) == deferred:                             # nothing was handed to the writer stage: the study's blocks go now
            self.drop(study)
        self.reap(block=False)

    def run(self):
        for k in range(min(self.stages.n_readers, len(self.todo))):
            self.submit(k)
        for k, (filename, save_path) in enumerate(self.todo):
            if self.verbose:
                logger.info(f"Processing file: {filename}...")
            self.submit(k)                                            # (already there unless the pools have just been given up)
            self.submit(k + self.stages.n_readers)
            study = self.studies[save_path] = _Study(filename, save_path)
            try:
                self.read(k, study)
                if self.model is None:
                    self.model = make_flow_model(*self.model_args)
                study.finish = _process_video_begin(os.path.join(self.dcm_folder, filename), save_path, nparr=study.nparr, metadata=study.md,
                                                    patient_id=study.pid, heart_rate=study.hr, flow_model=self.model, mask_dict=study.masks,
                                                    _defer_save=partial(self.defer, study), _submit=self.in_flight > 1, frames=self.frames,
                                                    _photometric=study.photometric, **self.video_args)
                self.begun.append(study)
            except Exception as e:
                self.failed(filename, e, trace=True)
                self.drop(study)
            while len(self.begun) >= max(1, self.in_flight):
                self.finish_oldest()
        while self.begun:
            self.finish_oldest()
        self.reap(block=True)

    def close(self):
        """What is left when run() ended or raised, in this order."""
        while self.begun:                                             # submitted solves are collected before the model goes
            with suppress(Exception):
                self.begun.popleft().finish()
        for _study, fut in self.pending:                              # writers still at work keep their study's blocks until done
            with suppress(Exception):
                fut.result()
        self.drop_read_ahead(wait=True)
        for study in list(self.studies.values()):
            self.drop(study)
        if self.owned:
            self.stages.close()
        if self.own_model and self.model is not None:
            self.model.close()
