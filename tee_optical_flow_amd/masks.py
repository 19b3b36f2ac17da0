"""Mask glue of the reference, restated with numpy/scipy (+ torch/PIL for the segmentor call) so the study driver runs
where skimage / torchvision are absent.  Mirrors /root/reference/optical_flow/calculate_optical_flow.py:
  :47-88    evaluate_1_slice   (one frame through a SAM-style module: image_encoder / prompt_encoder / mask_decoder)
  :90-111   moving_avg_mask
  :113-182  clean_mask
  :184-213  predict_movie_thres (mode='otsu')
  :215-241  predict_movie      (modes 'A4C', 'RVIO_2class')
moving_avg_mask / predict_movie_thres are pinned by tests/golden/reference_host_side.npz, clean_mask by
tests/golden/reference_clean_mask.npz (host path here, device path DenseFlow.clean_masks), predict_movie_thres also by
tests/golden/reference_otsu.npz (host path here, device path DenseFlow.otsu_masks).  The segmentor itself stays stock
PyTorch(-ROCm), as north_star says; the frame glue around it (PIL's two resizes, the normalised tensor, the argmax) has a device path
(DenseFlow.segmentor_input / segmentor_classmap, predict_movie's `engine=`) whose CPU statement is pil_resize_bilinear,
pil_nearest_index and segmentor_lut below, pinned to PIL by tests/test_segmentor_glue_cpu.py and tests/golden/segmentor_glue.npz."""
import numpy as np

from .config import default_optical_flow_config
from .frames import rgb2gray


def threshold_otsu(image, nbins=256):
    """skimage.filters.threshold_otsu for a float image (histogram over [min, max], bin centres)."""
    image = np.asarray(image, dtype=np.float64)
    first = image.ravel()[0]
    if np.all(image == first):                          # skimage: a one-valued image has no histogram to split
        return first
    hist, edges = np.histogram(image.ravel(), bins=nbins, range=(image.min(), image.max()))
    centers = (edges[:-1] + edges[1:]) / 2.0
    hist = hist.astype(np.float64)
    w1 = np.cumsum(hist)
    w2 = np.cumsum(hist[::-1])[::-1]
    m1 = np.cumsum(hist * centers) / w1
    m2 = (np.cumsum((hist * centers)[::-1]) / w2[::-1])[::-1]
    var12 = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return centers[:-1][np.argmax(var12)]


def remove_small_objects(mask, min_size):
    """skimage.morphology.remove_small_objects on a bool image (1-connectivity)."""
    from scipy import ndimage
    lab, n = ndimage.label(mask)
    if n == 0:
        return mask.copy()
    sizes = np.bincount(lab.ravel())
    small = sizes < min_size
    small[0] = False
    out = mask.copy()
    out[small[lab]] = False
    return out


def moving_avg_mask(arr, n=4, threshold=0.49, config=None):
    if config is not None:
        n, threshold = config.moving_avg_window, config.moving_avg_threshold
    arr2 = np.vstack((arr[:1], arr, arr[-1:], arr[-1:]))
    s = np.cumsum(arr2.astype(float), axis=0)
    s[n:] = s[n:] - s[:-n]
    return s[n - 1:] / n > threshold


def _frames_arg(nparr, engine, host_frames):
    """(what a device call takes, () -> the frames on the host): an array is both; a HeldFrames token (DenseFlow.hold_frames) is read
    on the device where it is, and downloaded -- by `host_frames`, or engine.download_frames -- only where the host has to work."""
    from .dense_flow import HeldFrames
    if isinstance(nparr, HeldFrames):
        return nparr, host_frames or engine.download_frames
    return np.asarray(nparr), lambda: nparr


def predict_movie_thres(nparr, verbose=False, config=None, *, engine=None, host_frames=None):
    """{'otsu': bool [N,H,W,2]} -- NB the reference calls moving_avg_mask WITHOUT config (Appendix C.5).
    With an `engine` that has `otsu_masks` (DenseFlow) and uint8 [N,H,W,3] frames with N, H, W >= 2, the work runs on the device
    (tf_otsu_masks, exact); otherwise, and for the shapes where the reference's np.squeeze changes what it computes, on the host.
    `nparr` may be the token of frames the engine holds (`host_frames`: () -> their RGB, for the host path)."""
    from scipy.ndimage import binary_fill_holes
    if config is None:
        config = default_optical_flow_config()
    arr, on_host = _frames_arg(nparr, engine, host_frames)
    if (engine is not None and hasattr(engine, "otsu_masks") and arr.dtype == np.uint8 and arr.ndim == 4 and arr.shape[3] == 3
            and min(arr.shape[:3]) >= 2):
        return {"otsu": engine.otsu_masks(arr, config.min_mask_size)}
    nparr = on_host()
    masks = []
    for i in range(nparr.shape[0]):
        g = rgb2gray(np.squeeze(nparr[i]))
        m = g > threshold_otsu(g)
        masks.append(remove_small_objects(binary_fill_holes(m), config.min_mask_size))
    arr = moving_avg_mask(np.squeeze(np.stack(masks)))
    return {"otsu": np.repeat(arr[:, :, :, None], 2, axis=3)}


_MODE_LABELS = {
    "A4C": {"lv_inner": 1, "lv": 2, "la_inner": 3, "la": 4, "rv_inner": 5, "ra_inner": 6, "rv": 7, "ra": 8},
    "RVIO_2class": {"rv": 1, "av": 2},
    "MouseRV_A4C": {"rv": 1, "rv_inner": 2},
}


def clean_mask(arr, mode="A4C", verbose=False, config=None, *, engine=None):
    """Reference :113-182: class map [N,H,W] -> {label: bool [N,H,W,2]} + 'bkgd'; None for an unknown mode.
    With an `engine` that has `clean_masks` (DenseFlow) and a uint8 [N,H,W] map with N, H, W >= 2, the work runs on the device
    (tf_clean_masks, exact); otherwise, and for the shapes where the reference's np.squeeze changes what it computes, on the host."""
    from scipy.ndimage import binary_fill_holes
    if config is None:
        config = default_optical_flow_config()
    if mode not in _MODE_LABELS:
        return None
    arr = np.asarray(arr)
    if (engine is not None and hasattr(engine, "clean_masks") and arr.dtype == np.uint8 and arr.ndim == 3
            and min(arr.shape) >= 2):
        labels = _MODE_LABELS[mode]
        planes = engine.clean_masks(arr, list(labels.values()), config.min_mask_size)
        return dict(zip(list(labels) + ["bkgd"], planes))
    out = {}
    aggregate = np.zeros(arr.shape, dtype=bool)
    for k, cls in _MODE_LABELS[mode].items():
        m = moving_avg_mask(np.squeeze(arr == cls))                 # NB: called without config, as the reference does
        clean = np.stack([remove_small_objects(binary_fill_holes(m[i]), config.min_mask_size) for i in range(m.shape[0])])
        aggregate = np.logical_or(clean, aggregate)
        out[k] = np.repeat(clean[:, :, :, None], 2, axis=3)
    out["bkgd"] = np.repeat(np.logical_not(aggregate)[:, :, :, None], 2, axis=3)
    return out


def evaluate_1_slice(frame, model):
    """Reference :47-88 without torchvision: RGB frame uint8 [H,W,3] -> class map uint8 [H,W].  PIL bilinear resize to
    1024 x 1024 (what transforms.Resize does on a PIL image), ToTensor, ImageNet normalisation, the three SAM sub-modules,
    argmax over classes, NEAREST resize back.  The tensor goes to the model's own device (the reference hard-codes .cuda())."""
    import torch
    from PIL import Image
    img = Image.fromarray(np.asarray(frame)).convert("RGB")
    orig_size = img.size
    img = img.resize((1024, 1024), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    x = ((x - mean) / std).unsqueeze(0)
    try:
        dev = next(model.parameters()).device
    except (StopIteration, AttributeError):
        dev = torch.device("cpu")
    x = x.to(dev)
    with torch.no_grad():
        emb = model.image_encoder(x)
        sparse, dense = model.prompt_encoder(points=None, boxes=None, masks=None)
        pred, _ = model.mask_decoder(image_embeddings=emb, image_pe=model.prompt_encoder.get_dense_pe(),
                                     sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense, multimask_output=True)
        pred = pred.argmax(dim=1).cpu().float()
    pil_mask = Image.fromarray(pred[0].numpy().astype(np.uint8), "L").resize(orig_size, resample=Image.NEAREST)
    return np.asarray(pil_mask, dtype=np.uint8)


PIL_PRECISION_BITS = 22                 # Pillow's fixed point for 8-bit resampling: 32 - 8 - 2


def pil_bilinear_coeffs(n_in, n_out):
    """The tables of one pass of Image.resize(..., BILINEAR) along an axis of n_in samples resized to n_out:
    (ksize, bounds int32 [n_out,2] = (first source index, taps), coeff int32 [n_out,ksize]).  Python floats are C doubles and the
    operations come in Pillow's order, so the tables are Pillow's (csrc/pil_resample_tables.h is the same text in C++)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    coeff = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w, ww = [], 0.0
        for x in range(n):
            a = abs((x + xmin - center + 0.5) / fs)
            w.append(1.0 - a if a < 1.0 else 0.0)
            ww += w[-1]
        for x in range(n):
            coeff[xx, x] = int(0.5 + (w[x] / ww if ww != 0.0 else w[x]) * (1 << PIL_PRECISION_BITS))
        bounds[xx] = (xmin, n)
    return ksize, bounds, coeff


def _pil_bilinear_pass(img, n_out):
    """one pass along axis 1 of a uint8 array [A, n_in, ...] -> uint8 [A, n_out, ...]"""
    _, bounds, coeff = pil_bilinear_coeffs(img.shape[1], n_out)
    out = np.empty((img.shape[0], n_out) + img.shape[2:], np.uint8)
    for xx in range(n_out):
        x0, n = bounds[xx]
        acc = np.full((img.shape[0],) + img.shape[2:], 1 << (PIL_PRECISION_BITS - 1), np.int32)
        for t in range(n):
            acc += img[:, x0 + t].astype(np.int32) * coeff[xx, t]
        out[:, xx] = np.clip(acc >> PIL_PRECISION_BITS, 0, 255)
    return out


def pil_resize_bilinear(img, size):
    """np.asarray(Image.fromarray(img).resize((out_w, out_h), Image.BILINEAR)) for a uint8 image [H,W] or [H,W,C], bit for bit, with
    `size` = (out_h, out_w) in numpy's order: the horizontal pass, a uint8 image, the vertical pass; an axis that keeps its length is
    left alone, as Pillow does."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError(f"pil_resize_bilinear takes a uint8 image [H,W] or [H,W,C], got {img.dtype} {img.shape}")
    out_h, out_w = int(size[0]), int(size[1])
    if out_w != img.shape[1]:
        img = _pil_bilinear_pass(img, out_w)
    if out_h != img.shape[0]:
        img = _pil_bilinear_pass(img.swapaxes(0, 1), out_h).swapaxes(0, 1)
    return np.ascontiguousarray(img)


def pil_nearest_index(n_in, n_out):
    """Source index of every output index along one axis of Image.resize(..., NEAREST): int32 [n_out].  Pillow adds the step up as it
    goes (a running double sum, not a product); the clamp to n_in - 1 never acts on the sizes checked and keeps a gather in bounds."""
    a = n_in / n_out
    xo = a * 0.5
    idx = np.empty(n_out, np.int32)
    for x in range(n_out):
        idx[x] = min(int(xo), n_in - 1)
        xo += a
    return idx


_SEGMENTOR_LUT = None


def segmentor_lut():
    """float32 [3,256]: the value evaluate_1_slice's tensor holds in channel c for byte b -- ((b / 255) - mean[c]) / std[c] in float32,
    computed once with the very torch CPU expression evaluate_1_slice uses, so it is exact by construction."""
    global _SEGMENTOR_LUT
    if _SEGMENTOR_LUT is None:
        import torch
        x = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).repeat(3, 1, 1).float().div(255.0)
        mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
        _SEGMENTOR_LUT = np.ascontiguousarray(((x - mean) / std).view(3, 256).numpy())
    return _SEGMENTOR_LUT


def _model_device(model):
    try:
        return next(model.parameters()).device
    except (StopIteration, AttributeError):
        return None


def _predict_classmaps_device(nparr, model, engine, chunk):
    """The frames' class maps uint8 [N,H,W] with the glue on `engine`'s device: per chunk one segmentor_input into a reused tensor, the
    three sub-modules one frame at a time on views of it (exactly evaluate_1_slice's calls), one segmentor_classmap."""
    import torch
    N, H, W = nparr.shape[:3]
    chunk = max(1, min(int(chunk), N))
    x = None
    maps = []
    with torch.no_grad():
        for f0 in range(0, N, chunk):
            n = min(chunk, N - f0)
            x = engine.segmentor_input(nparr[f0:f0 + n], (1024, 1024), out=x)
            logits = []
            for i in range(n):
                emb = model.image_encoder(x[i:i + 1])
                sparse, dense = model.prompt_encoder(points=None, boxes=None, masks=None)
                pred, _ = model.mask_decoder(image_embeddings=emb, image_pe=model.prompt_encoder.get_dense_pe(),
                                             sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense, multimask_output=True)
                logits.append(pred)
            maps.append(engine.segmentor_classmap(torch.cat(logits, dim=0), (H, W)))
    return np.concatenate(maps)


def predict_movie(nparr, model, mode="A4C", verbose=False, config=None, *, engine=None, chunk=16, host_frames=None):
    """Reference :215-241: every frame through the segmentor, then clean_mask (on `engine`'s device when it has clean_masks).
    With an `engine` that has `segmentor_input` (DenseFlow), uint8 [N,H,W,3] frames and a model whose parameters sit on that engine's
    GPU, the glue around the model -- both resizes, the normalised tensor, the argmax -- runs on the device too, `chunk` frames per
    call (exact: tf_segmentor_input, tf_segmentor_classmap); in every other case evaluate_1_slice runs frame by frame on the host.
    `nparr` may be the token of frames the engine holds: the device glue reads them in chunks token[a:b]; `host_frames`: () -> their
    RGB, for the host path."""
    if config is None:
        config = default_optical_flow_config()
    arr, on_host = _frames_arg(nparr, engine, host_frames)
    dev = _model_device(model)
    if (engine is not None and hasattr(engine, "segmentor_input") and arr.dtype == np.uint8 and arr.ndim == 4 and arr.shape[3] == 3
            and min(arr.shape[:3]) >= 1 and dev is not None and dev.type == "cuda" and dev.index == engine.device_id):   # (a bare "cuda": host path)
        preds = _predict_classmaps_device(arr, model, engine, chunk)
    else:
        nparr = on_host()
        preds = np.stack([evaluate_1_slice(nparr[i], model) for i in range(nparr.shape[0])])
    return clean_mask(preds, mode, verbose, config=config, engine=engine)
