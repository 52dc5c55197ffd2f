"""Metrics of the reference's evaluation loops -- mirror of metrics.py:43-244.

Pixel metrics (metrics.py:172-244: compute_RMSE / compute_PSNR / compute_SSIM, same arguments, same (input, gt, pred) float
triples) on the HIP kernel `mtd_image_metrics`.

Perceptual metrics (metrics.py:43-168: compute_PL / compute_TML on the five VGG-19 feature maps relu1_1 ... relu5_1, same
arguments plus the keyword `vgg`): the feature stack is `VGG19Features`, built from a torchvision `vgg19` state dict that the
caller hands over (no pretrained weights ship with this package), its convolutions are `kernels.conv` launches, the pools
`mtd_maxpool2x2`, the L1 means `kernels.loss_terms` and the per-patch Gram-matrix distance `mtd_patch_gram_l1`.
Inference only: no gradient flows through them.

FID (metrics.py:17-41, module/piq/fid.py): the statistic -- float64 mean and covariance of a feature set, the Newton-Schulz
square root of the covariance product with its data-dependent stop, the distance and the reference's singular fallback -- runs
on the HIP kernels of csrc/fid.hip (fid_statistics / fid_distance64 / compute_FID).  The feature network (the
reference: piq's InceptionV3 on a downloaded checkpoint) is `InceptionV3Features(state_dict)` (inception.py): the
checkpoint is the caller's to hand over, the network runs on the HIP kernels.  compute_feat takes it -- or any other callable the
caller built -- as `extractor`.

Per-slice forms for a batch of B slices taken as B samples (engine.test_MTD_GAN_Ours under `model.test_per_slice`):
pixel_metrics_each / pixel_metrics_per_slice (`mtd_image_metrics_each`), patch_gram_l1_each (`mtd_patch_gram_l1_each`) and
perceptual_metrics_per_slice.  Their reductions have the bits of the one-slice calls above.

Further full-reference metrics the reference vendors in module/piq -- MS-SSIM (ssim.py: multi_scale_ssim), VIFp (vif.py: vif_p)
and GMSD (gmsd.py: gmsd) -- image by image on the HIP kernels of csrc/iqa.hip (`mtd_iqa_each`): iqa_metrics_each /
iqa_metrics_per_slice and compute_MS_SSIM / compute_VIF / compute_GMSD (engine.test_MTD_GAN_Ours under `model.test_iqa`).

KID (module/piq/kid.py, vendored by the reference beside fid.py) from the same (N, D) feature rows as FID, in float64 on the HIP
kernels of csrc/kid.hip (`mtd_kid`): kid_distance64 / compute_KID (engine.test_MTD_GAN_Ours under `model.test_kid`).

MSID (module/piq/msid.py) and the Inception Score (module/piq/isc.py) from the same feature rows, in float64 on the HIP kernels
of csrc/msid.hip (`mtd_msid_descriptor`, `mtd_msid_distance`, `mtd_inception_score`): msid_descriptor64 /
msid_distance64 / compute_MSID and inception_score64 / is_distance64 / compute_IS (engine.test_MTD_GAN_Ours under
`model.test_msid` and `model.test_is`).

HaarPSI (module/piq/haarpsi.py: haarpsi with scales=3), the Haar wavelet perceptual similarity index, image by image on the HIP
kernels of csrc/haarpsi.hip (`mtd_haarpsi_each`): haarpsi_each / haarpsi_per_slice and compute_HaarPSI
(engine.test_MTD_GAN_Ours under `model.test_haarpsi`).

FSIM (module/piq/fsim.py: fsim with chromatic=False), the feature similarity index from phase congruency and gradient magnitude,
image by image on the HIP kernels of csrc/fsim.hip (`mtd_fsim_each`): fsim_each / fsim_per_slice and compute_FSIM
(engine.test_MTD_GAN_Ours under `model.test_fsim`).  The log-Gabor filter table and its three noise constants are built on the
host once per (pooled size, options) and uploaded once per device (fsim_filter_table / fsim_constants).

VSI (module/piq/vsi.py: vsi) and MDSI (module/piq/mdsi.py: mdsi), the visual saliency-induced index and the mean deviation
similarity index, image by image on the HIP kernels of csrc/vsi.hip and csrc/mdsi.hip (`mtd_vsi_each`, `mtd_mdsi_each`; DESIGN
3.19): vsi_each / vsi_per_slice / compute_VSI and mdsi_each / mdsi_per_slice / compute_MDSI (engine.test_MTD_GAN_Ours under
`model.test_vsi` / `model.test_mdsi`).  SDSP's log-Gabor table is built on the host once per (omega_0, sigma_f) and uploaded once
per device (vsi_log_gabor_table).

BRISQUE (module/piq/brisque.py: brisque) and total variation (module/piq/tv.py: total_variation), the two no-reference metrics,
image by image and each image set on its own on the HIP kernels of csrc/brisque.hip (`mtd_brisque_each`, `mtd_tv_each`; DESIGN
3.21): brisque_each / brisque_per_slice / compute_BRISQUE and tv_each / tv_per_slice / compute_TV (engine.test_MTD_GAN_Ours under
`model.test_brisque` / `model.test_tv`).  BRISQUE's support vector regression is the caller's (brisque_weights); the Gaussian
filter and the shape look-up tables are built on the host with piq's roundings and uploaded once per device
(brisque_gaussian_table / brisque_ggd_tables).

LPIPS and DISTS (module/piq/perceptual.py: LPIPS and DISTS on torchvision's VGG-16 with ImageNet normalisation) image by image
(DESIGN 3.18): the feature stack is `VGG16Features`, built like `VGG19Features` from a state dict the caller hands over, with the
normalisation folded exactly into its first layer and max or L2 pooling (`mtd_l2pool3x3s2`); the reductions over the maps run on
the HIP kernels of csrc/lpips.hip (`mtd_lpips_level_each`, `mtd_channel_moments_each`, `mtd_dists_finish`): lpips_each /
lpips_per_slice / compute_LPIPS and dists_each / dists_per_slice / compute_DISTS (engine.test_MTD_GAN_Ours under
`model.perceptual_vgg16` with `model.test_lpips` / `model.test_dists`).  The learned weights are the caller's too (lpips_weights /
dists_weights)."""
import functools
import math

import numpy as np
import torch

from . import _lib
from . import kernels as K
from .inception import InceptionV3Features  # noqa: F401  -- the public name is metrics.InceptionV3Features


def _pair_sums(a, b, clip_a=False):
    """(sum of squared error, sum of the SSIM map, pixel count) of two (B,1,H,W) CUDA tensors; one device->host copy."""
    if a.dim() != 4 or b.dim() != 4 or a.shape != b.shape or a.shape[1] != 1:
        raise AssertionError("pixel metrics expect two (B,1,H,W) tensors of the same shape")
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError("pixel metrics: HIP path needs CUDA tensors (no CPU fallback)")
    a, b = a.contiguous().float(), b.contiguous().float()
    B, _, H, W = a.shape
    L = _lib.lib()
    out = torch.empty(2, dtype=torch.float64, device=a.device)
    ws = K.workspace(L.mtd_image_metrics_ws_bytes(B, H, W), a.device)
    _lib.check(L.mtd_image_metrics(a.data_ptr(), b.data_ptr(), B, H, W, 1 if clip_a else 0, out.data_ptr(), ws.data_ptr(), K.stream_ptr()),
               "mtd_image_metrics")
    sse, ssum = out.tolist()
    return sse, ssum, B * H * W


def _psnr(sse, n, data_range):
    mse = np.float32(np.float32(sse / n) + np.float32(1e-10))
    return float(np.float32(10.0) * np.log10(np.float32(data_range ** 2) / mse))


def compute_RMSE(input, target, pred):
    """metrics.py:174-181."""
    r = []
    for a in (input, target, pred):
        sse, _, n = _pair_sums(a, target)
        r.append(float(np.sqrt(np.float32(sse / n))))
    return tuple(r)


def compute_PSNR(input, target, pred, data_range=1.0):
    """metrics.py:184-197: MSE over the whole batch tensor, + 1e-10."""
    r = []
    for a in (input, target, pred):
        sse, _, n = _pair_sums(a, target)
        r.append(_psnr(sse, n, data_range))
    return tuple(r)


def compute_SSIM(input, target, pred, data_range=1.0):
    """metrics.py:200-244 (window 11, sigma 1.5, size_average)."""
    if data_range != 1.0:
        raise NotImplementedError("SSIM kernel is built for data_range 1.0 (C1 = 1e-4, C2 = 9e-4), as the reference calls it")
    r = []
    for a in (input, target, pred):
        _, ssum, n = _pair_sums(a, target)
        r.append(float(np.float32(ssum / n)))
    return tuple(r)


def pixel_metrics(input, target, pred):
    """All nine numbers of the test loop in three launches: dict of (input, gt, pred) triples."""
    out = {"rmse": [], "psnr": [], "ssim": []}
    for a in (input, target, pred):
        sse, ssum, n = _pair_sums(a, target)
        out["rmse"].append(float(np.sqrt(np.float32(sse / n))))
        out["psnr"].append(_psnr(sse, n, 1.0))
        out["ssim"].append(float(np.float32(ssum / n)))
    return {k: tuple(v) for k, v in out.items()}


# The shared pieces of the image-by-image metrics below (the *_each functions on (input, target, pred)).  Each function calls the
# checks where its own refusals stand, so which error a doubly wrong call meets first is the function's choice, not the helpers'.
def _image_shape(what, input, target, pred):
    """(B, H, W) of three (B,1,H,W) tensors of one shape; AssertionError otherwise (`what`: the message's subject and verb)."""
    for t in (input, target, pred):
        if t.dim() != 4 or t.shape != target.shape or t.shape[1] != 1:
            raise AssertionError(f"{what} (B,1,H,W) tensors of the same shape")
    return target.shape[0], target.shape[2], target.shape[3]


def _need_cuda(name, input, target, pred):
    for t in (input, target, pred):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: HIP path needs CUDA tensors (no CPU fallback)")


def _fp32_sources(input, target, pred):
    """The three as contiguous fp32 tensors; the same tensor twice stays the same pointer (a kernel that transforms its sources
    then transforms it once)."""
    kept = {}
    for t in (input, target, pred):
        if id(t) not in kept:
            kept[id(t)] = t.contiguous().float()
    return [kept[id(t)] for t in (input, target, pred)]


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def _who_triples(vals):
    """A (3, B) tensor as nested lists -> the list of B (input, gt, pred) triples."""
    return [tuple(vals[k][i] for k in range(3)) for i in range(len(vals[0]))]


def _batch_means(name, data_range, each, *args, **kw):
    """The body of the compute_* wrappers: the data_range guard, then the three means over the batch of each(*args, **kw) -- a
    (3, B) tensor, or IQA's (1, 3, B) -- as a (3,) device tensor."""
    if data_range != 1.0:
        raise NotImplementedError(f"{name}: the kernels are built for data_range 1.0, as the test loop calls the pixel metrics")
    return each(*args, **kw).reshape(3, -1).mean(dim=1)


def _device_cached(cache, key, device, build):
    """build()'s device tensors, kept per (key, device index) in `cache`: 16 entries, cleared when full."""
    key += (device.index if device.index is not None else torch.cuda.current_device(),)
    got = cache.get(key)
    if got is None:
        got = build()
        if len(cache) >= 16:
            cache.clear()
        cache[key] = got
    return got


def _parts(on, *shape, device, fill=torch.empty):
    """The float64 parts tensor of a *_each call, or None when the caller did not ask for parts."""
    return fill(shape, dtype=torch.float64, device=device) if on else None


def _each_call(each, ws_bytes, srcs, out_shape, ws_args, args, rows=None, target=True):
    """What every *_each function ends in: each(the three source pointers, 3, [the target's,] *args, the float64 result of
    `out_shape`, [`rows` or NULL -- rows=False: the entry has no parts argument --,] the workspace of ws_bytes(*ws_args), the
    stream), checked -> the result, or (result, rows) where rows is a tensor."""
    import ctypes
    dev = srcs[1].device
    out = torch.empty(out_shape, dtype=torch.float64, device=dev)
    ws = K.workspace(ws_bytes(*ws_args), dev)
    ptrs = (ctypes.c_void_p * 3)(*(t.data_ptr() for t in srcs))
    head = (ptrs, 3, srcs[1].data_ptr()) if target else (ptrs, 3)
    tail = () if rows is False else (None if rows is None else rows.data_ptr(),)
    _lib.check(each(*head, *args, out.data_ptr(), *tail, ws.data_ptr(), K.stream_ptr()), each.__name__)
    return (out, rows) if torch.is_tensor(rows) else out


def pixel_metrics_each(input, target, pred, clip_pred=False):
    """The sums of pixel_metrics image by image, without a host read: a (3, B, 2) float64 device tensor, [k][i] = (sum of squared
    error, sum of the SSIM map) of slice i of (input, target, pred)[k] against slice i of target -- the bits of a one-slice
    mtd_image_metrics call (mtd_image_metrics_each: two launches for the three pairs of the batch).  `clip_pred`: clip the
    prediction to [0, 1] on the way in."""
    B, H, W = _image_shape("pixel metrics expect", input, target, pred)
    _need_cuda("pixel metrics", input, target, pred)
    import ctypes
    clips = (ctypes.c_int * 3)(0, 0, 1 if clip_pred else 0)
    L = _lib.lib()
    return _each_call(L.mtd_image_metrics_each, L.mtd_image_metrics_each_ws_bytes, _fp32_sources(input, target, pred), (3, B, 2),
                      (3, B, H, W), (B, H, W, clips), rows=False)


def _slice_triples(sums, n):
    """sums: pixel_metrics_each's tensor as nested lists.  dict rmse / psnr / ssim -> list of B (input, gt, pred) triples, by the
    formulas of pixel_metrics with n = H * W."""
    B = len(sums[0])
    return {"rmse": [tuple(float(np.sqrt(np.float32(sums[k][i][0] / n))) for k in range(3)) for i in range(B)],
            "psnr": [tuple(_psnr(sums[k][i][0], n, 1.0) for k in range(3)) for i in range(B)],
            "ssim": [tuple(float(np.float32(sums[k][i][1] / n)) for k in range(3)) for i in range(B)]}


def pixel_metrics_per_slice(input, target, pred):
    """pixel_metrics of every slice of a batch: dict rmse / psnr / ssim -> list of B (input, gt, pred) triples, each equal to
    pixel_metrics(input[i:i+1], target[i:i+1], pred[i:i+1]).  Two launches and one device -> host copy for the batch."""
    sums = pixel_metrics_each(input, target, pred).tolist()
    return _slice_triples(sums, target.shape[2] * target.shape[3])


# ================================================================================================ MS-SSIM, VIFp, GMSD
IQA_METRICS = ("ms_ssim", "vif", "gmsd")                       # the order of the rows of iqa_metrics_each and of mtd_iqa_each's mask bits
IQA_MIN_SIDE = {"ms_ssim": 161, "vif": 41, "gmsd": 2}          # piq's own limits (ssim.py:424, vif.py:58; gmsd pools 2 x 2)
IQA_PARTS = 20


def _iqa_which(which):
    """The chosen metrics in the order of IQA_METRICS; ValueError for anything but a non-empty selection of those names."""
    names = (which,) if isinstance(which, str) else tuple(which) if isinstance(which, (tuple, list)) else None
    if not names or any(n not in IQA_METRICS for n in names) or len(set(names)) != len(names):
        raise ValueError(f"iqa metrics: a non-empty tuple of names from {IQA_METRICS} expected, got {which!r}")
    return tuple(n for n in IQA_METRICS if n in names)


def iqa_metrics_each(input, target, pred, which=IQA_METRICS, sigma_n_sq=2.0, parts=False):
    """MS-SSIM, VIFp and GMSD (piq's multi_scale_ssim, vif_p and gmsd with their defaults, data_range 1) of every slice of
    (input, target, pred) against the same slice of target, without a host read: a (len(which), 3, B) float64 device tensor, rows
    in the order ms_ssim, vif, gmsd whatever the order of `which`.  With parts=True also the (3, B, 20) float64 stage values:
    [0..9] MS-SSIM (cs mean, SSIM mean) of the five levels, [10..17] VIFp (num, den) of the four scales, [18..19] GMSD (mean,
    variance) of the GMS map; zero for metrics not in `which`.  A slice's values depend neither on the batch it is in nor on
    the other two image sets (mtd_iqa_each: fp32 filters, per-image sums in double in a fixed order).
    `sigma_n_sq` is VIFp's visual-noise variance on the [0, 1] scale: the vendored vif_p does NOT rescale the images to
    [0, 255], so its default 2.0 is taken as it stands; pass 2 / 255**2 for the convention of the original [0, 255] code.
    MS-SSIM needs sides of at least 161, VIFp of at least 41, GMSD of at least 2 (ValueError, as piq raises)."""
    which = _iqa_which(which)
    B, H, W = _image_shape("iqa metrics expect", input, target, pred)
    _need_cuda("iqa metrics", input, target, pred)
    for n in which:
        if H < IQA_MIN_SIDE[n] or W < IQA_MIN_SIDE[n]:
            raise ValueError(f"iqa metrics: {n} needs images of at least {IQA_MIN_SIDE[n]}x{IQA_MIN_SIDE[n]}, got {H}x{W}")
    if not sigma_n_sq > 0:
        raise ValueError(f"iqa metrics: sigma_n_sq must be positive, got {sigma_n_sq!r}")
    mask = sum(1 << IQA_METRICS.index(n) for n in which)
    L = _lib.lib()
    srcs = _fp32_sources(input, target, pred)
    return _each_call(L.mtd_iqa_each, L.mtd_iqa_ws_bytes, srcs, (len(which), 3, B), (mask, 3, B, H, W), (B, H, W, mask, float(sigma_n_sq)),
                      _parts(parts, 3, B, IQA_PARTS, device=srcs[1].device, fill=torch.zeros))


def _iqa_triples(which, vals):
    """vals: iqa_metrics_each's tensor as nested lists -> dict metric -> list of B (input, gt, pred) triples."""
    return {n: [tuple(vals[r][k][i] for k in range(3)) for i in range(len(vals[r][0]))] for r, n in enumerate(which)}


def iqa_metrics_per_slice(input, target, pred, which=IQA_METRICS, sigma_n_sq=2.0):
    """iqa_metrics_each as host numbers: dict metric -> list of B (input, gt, pred) triples (the kernels' float64
    scores).  One device -> host copy for the batch."""
    which = _iqa_which(which)
    return _iqa_triples(which, iqa_metrics_each(input, target, pred, which, sigma_n_sq).tolist())


def compute_MS_SSIM(input, target, pred, data_range=1.0):
    """piq's multi_scale_ssim(a, target) with its defaults for a = input, target, pred: (input, gt, pred) floats, each the mean
    over the batch of the per-image scores (reduction='mean').  Sides of at least 161."""
    return tuple(_batch_means("ms_ssim", data_range, iqa_metrics_each, input, target, pred, ("ms_ssim",)).tolist())


def compute_VIF(input, target, pred, data_range=1.0, sigma_n_sq=2.0):
    """piq's vif_p(a, target) likewise.  The vendored vif_p does not rescale to [0, 255]: sigma_n_sq = 2.0 applies to the [0, 1]
    images as they are (iqa_metrics_each).  Sides of at least 41."""
    return tuple(_batch_means("vif", data_range, iqa_metrics_each, input, target, pred, ("vif",), sigma_n_sq=sigma_n_sq).tolist())


def compute_GMSD(input, target, pred, data_range=1.0):
    """piq's gmsd(a, target) likewise.  Sides of at least 2."""
    return tuple(_batch_means("gmsd", data_range, iqa_metrics_each, input, target, pred, ("gmsd",)).tolist())


# ================================================================================================ HaarPSI
HAARPSI_MIN_SIDE = 16                                           # piq's own limit: 2 ** (scales + 1), checked before the subsampling
HAARPSI_OPTIONS = ("c", "alpha", "subsample")


def haarpsi_check_options(c=30.0, alpha=4.2, subsample=True):
    """ValueError unless c and alpha are positive finite numbers and subsample a bool."""
    if not all(_number(v) and v > 0 for v in (c, alpha)):
        raise ValueError(f"haarpsi: c and alpha must be positive, got {c!r}, {alpha!r}")
    if not isinstance(subsample, bool):
        raise ValueError(f"haarpsi: subsample must be a bool, got {subsample!r}")


def haarpsi_each(input, target, pred, c=30.0, alpha=4.2, subsample=True, parts=False):
    """HaarPSI (piq's haarpsi with scales=3, data_range 1) of every slice of (input, target, pred) against the same slice of
    target, without a host read: a (3, B) float64 device tensor.  With parts=True also the (3, B, 4) float64 sums: (num, den) of
    the orientation of the Haar filter as it is, then of its transpose (num = sum sigmoid(alpha sim) w, den = sum w).  A slice's
    values depend neither on the batch it is in nor on the other two image sets (mtd_haarpsi_each: fp32 filters; similarity,
    sigmoid and per-image sums in double in a fixed order; two launches for the three pairs of the batch).  Two all-zero images
    give +inf, as piq does.  Sides of at least 16, with subsample or without (ValueError, as piq raises)."""
    B, H, W = _image_shape("haarpsi expects", input, target, pred)
    _need_cuda("haarpsi", input, target, pred)
    if H < HAARPSI_MIN_SIDE or W < HAARPSI_MIN_SIDE:
        raise ValueError(f"haarpsi needs images of at least {HAARPSI_MIN_SIDE}x{HAARPSI_MIN_SIDE}, got {H}x{W}")
    haarpsi_check_options(c, alpha, subsample)
    sub = 1 if subsample else 0
    L = _lib.lib()
    srcs = _fp32_sources(input, target, pred)
    return _each_call(L.mtd_haarpsi_each, L.mtd_haarpsi_ws_bytes, srcs, (3, B), (3, B, H, W, sub), (B, H, W, sub, float(c), float(alpha)),
                      _parts(parts, 3, B, 4, device=srcs[1].device))


def haarpsi_per_slice(input, target, pred, c=30.0, alpha=4.2, subsample=True):
    """haarpsi_each as host numbers: a list of B (input, gt, pred) triples (the kernels' float64 scores).  One device -> host
    copy for the batch."""
    return _who_triples(haarpsi_each(input, target, pred, c, alpha, subsample).tolist())


def compute_HaarPSI(input, target, pred, data_range=1.0, **kw):
    """piq's haarpsi(a, target) with its defaults (or c, alpha, subsample) for a = input, target, pred: (input, gt, pred) floats,
    each the mean over the batch of the per-image scores (reduction='mean').  Sides of at least 16."""
    return tuple(_batch_means("haarpsi", data_range, haarpsi_each, input, target, pred, **kw).tolist())


# ================================================================================================ FSIM
FSIM_MIN_SIDE, FSIM_MAX_SIDE = 16, 512                          # of the pooled map; each side a power of two (the LDS transforms' lengths)
FSIM_SUMS = 4                                                   # num, den, sum pc, sum gm; the parts rows hold the T_o behind them
FSIM_OPTIONS = ("scales", "orientations", "min_length", "mult", "sigma_f", "delta_theta", "k")


def fsim_pooled_size(H, W):
    """-> (ks, h, w): piq's average-pool kernel max(1, round(min(H, W) / 256)) -- Python's round, to even: 384 -> 2, 640 -> 2 --
    and the sides of the pooled map (stride ks, floor)."""
    ks = max(1, round(min(H, W) / 256))
    return ks, H // ks, W // ks


def fsim_check_options(scales=4, orientations=4, min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2, k=2.0):
    """ValueError unless scales is an int in 1..4, orientations an int in 1..8, min_length, mult and delta_theta positive
    numbers, sigma_f a positive number other than 1 and k a finite number."""
    integer = lambda v, lo, hi: isinstance(v, int) and not isinstance(v, bool) and lo <= v <= hi          # noqa: E731
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)      # noqa: E731
    if not integer(scales, 1, 4) or not integer(orientations, 1, 8):
        raise ValueError(f"fsim: scales an int in 1..4 and orientations an int in 1..8, got {scales!r}, {orientations!r}")
    if not all(number(v) and v > 0 for v in (min_length, mult, sigma_f, delta_theta)) or sigma_f == 1 or not number(k):
        raise ValueError("fsim: min_length, mult, delta_theta positive numbers, sigma_f a positive number other than 1, k a number; got "
                         f"{min_length!r}, {mult!r}, {delta_theta!r}, {sigma_f!r}, {k!r}")


def _fsim_frequencies(n):
    """The n frequencies of a transform axis in storage order (0, 1/n, ..., then the negative ones), float32."""
    k = (torch.arange(n) + n // 2) % n - n // 2
    return k.float() / n


@functools.lru_cache(maxsize=16)
def fsim_filter_table(h, w, scales=4, orientations=4, min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2):
    """The (orientations * scales, h, w) float32 host table of piq's log-Gabor filters for even h, w, orientation-major, zero
    frequency at [0, 0]: a radial factor per scale (log-Gabor profile times a Butterworth low-pass of cutoff 0.45 and order 15,
    zero at the zero frequency) times an angular Gaussian per orientation, both built for all scales / orientations at once from
    broadcast frequency axes.  float32 throughout, as piq's grid is even in a float64 run, and each element through piq's
    sequence of roundings, so the bytes are those of piq's own table (tests/golden/fsim_piq.npz holds their CRC-32).  Cached; do
    not modify the result."""
    fy, fx = _fsim_frequencies(h)[:, None], _fsim_frequencies(w)[None, :]
    radius = torch.sqrt(fy * fy + fx * fx)                                          # (h, w)
    butterworth = 1.0 / (1.0 + (radius / 0.45) ** 30)
    direction = torch.atan2(-fx, fy).expand(h, w)
    radius[0, 0] = 1                                                                # log(0) stays out; the factor is zeroed below
    centres = torch.tensor([1.0 / (min_length * mult ** s) for s in range(scales)])[:, None, None]
    radial = torch.exp(-torch.log(radius / centres) ** 2 / (2 * math.log(sigma_f) ** 2)) * butterworth          # (S, h, w)
    radial[:, 0, 0] = 0
    angles = [o * math.pi / orientations for o in range(orientations)]
    ca, sa = (torch.tensor([f(a) for a in angles])[:, None, None] for f in (math.cos, math.sin))
    sd, cd = torch.sin(direction), torch.cos(direction)
    away = torch.atan2(sd * ca - cd * sa, cd * ca + sd * sa).abs()                  # (O, h, w): angle to the orientation, unwrapped
    width = math.pi / (orientations * delta_theta)
    angular = torch.exp(-away ** 2 / (2 * width ** 2))
    return (angular[:, None] * radial[None]).reshape(orientations * scales, h, w).contiguous()


def fsim_constants(table, scales, orientations):
    """The (3, orientations) float64 constants of the noise threshold from the float32 table: em_n[o] = sum filter[o, 0]^2, and
    from the Gram matrix over the scales of f = real(ifft2(filter)) sqrt(h w): sum_an2[o] its trace, sum_ai_aj[o] the sum of its
    upper triangle."""
    h, w = table.shape[-2:]
    t = table.double().view(orientations, scales, h, w)
    f = torch.fft.ifft2(t).real * math.sqrt(h * w)
    gram = torch.einsum("osyx,otyx->ost", f, f)
    trace = gram.diagonal(dim1=1, dim2=2).sum(dim=1)
    return torch.stack([(t[:, 0] ** 2).sum(dim=[1, 2]), trace, (gram.sum(dim=[1, 2]) - trace) / 2]).contiguous()


_fsim_device_tables = {}


def _fsim_tables(h, w, scales, orientations, min_length, mult, sigma_f, delta_theta, device):
    def build():
        table = fsim_filter_table(h, w, scales, orientations, min_length, mult, sigma_f, delta_theta)
        return table.to(device), fsim_constants(table, scales, orientations).to(device)
    return _device_cached(_fsim_device_tables, (h, w, scales, orientations, min_length, mult, sigma_f, delta_theta), device, build)


def fsim_each(input, target, pred, scales=4, orientations=4, min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2, k=2.0, parts=False):
    """FSIM (piq's fsim with chromatic=False, data_range 1) of every slice of (input, target, pred) against the same slice of
    target, without a host read: a (3, B) float64 device tensor.  With parts=True also the (3, B, 4 + orientations) float64 rows
    num = sum GM PC pc_max, den = sum pc_max, the sums of the source's phase-congruency and gradient maps, and its noise thresholds
    T_0 .. T_{O-1}.  A slice's values depend neither on the batch it is in nor on the other two image sets (mtd_fsim_each: fp32
    LDS transforms, everything after them in double in a fixed order); an image set passed twice (target as a source) is
    transformed once.  Two all-zero images give exactly 1, as piq does.  The pooled map (fsim_pooled_size) must have sides that
    are powers of two in 16..512: 64 x 64 patches, 256 x 256, 512 x 512 and 1024 x 1024 slices, 512 x 256 ...; anything else is a
    ValueError that names the pooled size."""
    B, H, W = _image_shape("fsim expects", input, target, pred)
    fsim_check_options(scales, orientations, min_length, mult, sigma_f, delta_theta, k)
    ks, h, w = fsim_pooled_size(H, W)
    if not all(FSIM_MIN_SIDE <= n <= FSIM_MAX_SIDE and n & (n - 1) == 0 for n in (h, w)):
        raise ValueError(f"fsim: {H}x{W} images pool (kernel {ks}) to {h}x{w}; the kernels take pooled sides that are powers of two in "
                         f"{FSIM_MIN_SIDE}..{FSIM_MAX_SIDE}")
    _need_cuda("fsim", input, target, pred)
    srcs = _fp32_sources(input, target, pred)                    # (the same tensor twice stays the same pointer: transformed once)
    table, consts = _fsim_tables(h, w, scales, orientations, min_length, mult, sigma_f, delta_theta, srcs[1].device)
    L = _lib.lib()
    return _each_call(L.mtd_fsim_each, L.mtd_fsim_ws_bytes, srcs, (3, B), (3, B, h, w, scales, orientations),
                      (B, H, W, ks, scales, orientations, float(k), table.data_ptr(), consts.data_ptr()),
                      _parts(parts, 3, B, FSIM_SUMS + orientations, device=srcs[1].device))


def fsim_per_slice(input, target, pred, **kw):
    """fsim_each as host numbers: a list of B (input, gt, pred) triples (the kernels' float64 scores).  One device -> host copy
    for the batch."""
    return _who_triples(fsim_each(input, target, pred, **kw).tolist())


def compute_FSIM(input, target, pred, data_range=1.0, **kw):
    """piq's fsim(a, target, chromatic=False) with its defaults (or the seven options) for a = input, target, pred: (input, gt,
    pred) floats, each the mean over the batch of the per-image scores (reduction='mean')."""
    return tuple(_batch_means("fsim", data_range, fsim_each, input, target, pred, **kw).tolist())


# ================================================================================================ VSI and MDSI
VSI_MIN_SIDE, VSI_MAX_SIDE = 16, 1024                           # of the image; any side in between (SDSP's transforms are always 256 x 256)
VSI_PARTS = 6                                                   # num, den, sum vs, sum gm, min vs_m, max vs_m
VSI_OPTIONS = ("c1", "c2", "c3", "alpha", "beta", "omega_0", "sigma_f", "sigma_d", "sigma_c")
MDSI_MIN_SIDE, MDSI_MAX_SIDE = 16, 1024
MDSI_PARTS = 3                                                  # mean re, mean im, sum of the deviations
MDSI_OPTIONS = ("c1", "c2", "c3", "combination", "alpha", "beta", "gamma", "rho", "q", "o")
MDSI_COMBINATIONS = ("sum", "mult")


def vsi_kernel_size(H, W):
    """piq's pooling kernel of vsi and mdsi: max(1, round(min(H, W) / 256)) -- Python's round, half to even: 384 -> 2, 640 -> 2,
    641 -> 3.  The pooled map has ceil(H / k) x ceil(W / k) pixels: both metrics pad k - 1 pixels per axis before the floor pooling
    (VSI [k // 2, (k - 1) // 2] in replicate mode, MDSI [(k - 1) // 2, k // 2] with zeros)."""
    return max(1, round(min(H, W) / 256))


def vsi_check_options(c1=1.27, c2=386., c3=130., alpha=0.4, beta=0.02, omega_0=0.021, sigma_f=1.34, sigma_d=145., sigma_c=0.001):
    """ValueError unless c1, c2, c3, omega_0, sigma_f, sigma_d, sigma_c are positive finite numbers and alpha, beta finite numbers."""
    if not all(_number(v) and v > 0 for v in (c1, c2, c3, omega_0, sigma_f, sigma_d, sigma_c)) or not (_number(alpha) and _number(beta)):
        raise ValueError("vsi: c1, c2, c3, omega_0, sigma_f, sigma_d, sigma_c positive numbers, alpha and beta numbers; got "
                         f"{c1!r}, {c2!r}, {c3!r}, {omega_0!r}, {sigma_f!r}, {sigma_d!r}, {sigma_c!r}, {alpha!r}, {beta!r}")


def mdsi_check_options(c1=140., c2=55., c3=550., combination="sum", alpha=0.6, beta=0.1, gamma=0.2, rho=1., q=0.25, o=0.25):
    """ValueError unless combination is 'sum' or 'mult', c1, c2, c3, rho are positive finite numbers and alpha, beta, gamma, q, o
    finite numbers."""
    if not (isinstance(combination, str) and combination in MDSI_COMBINATIONS):
        raise ValueError(f"mdsi: combination must be one of {MDSI_COMBINATIONS}, got {combination!r}")
    if not all(_number(v) and v > 0 for v in (c1, c2, c3, rho)) or not all(_number(v) for v in (alpha, beta, gamma, q, o)):
        raise ValueError("mdsi: c1, c2, c3, rho positive numbers, alpha, beta, gamma, q, o numbers; got "
                         f"{c1!r}, {c2!r}, {c3!r}, {rho!r}, {alpha!r}, {beta!r}, {gamma!r}, {q!r}, {o!r}")


@functools.lru_cache(maxsize=16)
def vsi_log_gabor_table(omega_0=0.021, sigma_f=1.34):
    """The (256, 256) float32 host table of SDSP's log-Gabor filter, zero frequency at [0, 0]: exp(-log(r / omega_0)^2 /
    (2 sigma_f^2)) on the radius r of the frequency (in cycles per pixel, -1/2 .. 1/2 - 1/256 per axis), zero beyond r = 1/2 and
    at the zero frequency.  float32 throughout and each element through piq's sequence of roundings, so the bytes are those of
    piq's own table (tests/golden/vsi_mdsi_piq.npz holds their CRC-32).  Cached; do not modify the result."""
    n = 256
    f = ((torch.arange(n) + n // 2) % n - n // 2).float() / n                       # storage order: 0, 1/n, ..., then the negative ones
    radius = torch.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
    radius = radius * (radius <= 0.5)                                               # (log(0) = -inf there: exp(-inf) = 0)
    radius[0, 0] = 1
    table = torch.exp(-torch.log(radius / omega_0) ** 2 / (2 * sigma_f ** 2))
    table[0, 0] = 0
    return table.contiguous()


_vsi_device_tables = {}


def _vsi_table(omega_0, sigma_f, device):
    return _device_cached(_vsi_device_tables, (omega_0, sigma_f), device, lambda: vsi_log_gabor_table(omega_0, sigma_f).to(device))


def _each_sources(name, input, target, pred, lo, hi):
    """The shared argument checks of vsi_each / mdsi_each / brisque_each / tv_each -> (contiguous fp32 sources, B, H, W)."""
    B, H, W = _image_shape(f"{name} expects", input, target, pred)
    if not (lo <= H <= hi and lo <= W <= hi):
        raise ValueError(f"{name}: the kernels take images with sides in {lo}..{hi}, got {H}x{W}")
    _need_cuda(name, input, target, pred)
    return _fp32_sources(input, target, pred), B, H, W


def vsi_each(input, target, pred, c1=1.27, c2=386., c3=130., alpha=0.4, beta=0.02, omega_0=0.021, sigma_f=1.34, sigma_d=145., sigma_c=0.001,
             parts=False):
    """VSI (piq's vsi, data_range 1, the grey channel three times) of every slice of (input, target, pred) against the same slice
    of target, without a host read: a (3, B) float64 device tensor.  With parts=True also the (3, B, 6) float64 rows num = sum s
    vs_max, den = sum vs_max, the sums of the source's pooled saliency and gradient maps, and the minimum and maximum of its
    saliency map before it is stretched to [0, 1].  A slice's values depend neither on the batch it is in nor on the other two
    image sets (mtd_vsi_each: fp32 LDS transforms at 256 x 256, everything else in double in a fixed order); an image set passed
    twice (target as a source) is transformed once, and an image against itself gives exactly 1.  Sides in 16..1024, not
    necessarily powers of two; anything else is a ValueError."""
    import ctypes
    vsi_check_options(c1, c2, c3, alpha, beta, omega_0, sigma_f, sigma_d, sigma_c)
    srcs, B, H, W = _each_sources("vsi", input, target, pred, VSI_MIN_SIDE, VSI_MAX_SIDE)
    k = vsi_kernel_size(H, W)
    table = _vsi_table(float(omega_0), float(sigma_f), srcs[1].device)
    opts = (ctypes.c_double * 7)(c1, c2, c3, alpha, beta, sigma_d, sigma_c)
    L = _lib.lib()
    return _each_call(L.mtd_vsi_each, L.mtd_vsi_ws_bytes, srcs, (3, B), (3, B, H, W, k), (B, H, W, k, table.data_ptr(), opts),
                      _parts(parts, 3, B, VSI_PARTS, device=srcs[1].device))


def mdsi_each(input, target, pred, c1=140., c2=55., c3=550., combination="sum", alpha=0.6, beta=0.1, gamma=0.2, rho=1., q=0.25, o=0.25,
              parts=False):
    """MDSI (piq's mdsi, data_range 1, the grey channel three times) of every slice of (input, target, pred) against the same
    slice of target, without a host read: a (3, B) float64 device tensor.  With parts=True also the (3, B, 3) float64 rows: the
    means of the real and imaginary part of gcs^q and the sum of |gcs^q - mean|^rho.  All double in a fixed order (mtd_mdsi_each): a
    slice's values depend neither on the batch it is in nor on the other two image sets, and an image against itself gives exactly
    0 (with combination 'mult', or the default alpha).  Sides in 16..1024; anything else is a ValueError."""
    import ctypes
    mdsi_check_options(c1, c2, c3, combination, alpha, beta, gamma, rho, q, o)
    srcs, B, H, W = _each_sources("mdsi", input, target, pred, MDSI_MIN_SIDE, MDSI_MAX_SIDE)
    k = vsi_kernel_size(H, W)
    opts = (ctypes.c_double * 9)(c1, c2, c3, alpha, beta, gamma, rho, q, o)
    L = _lib.lib()
    return _each_call(L.mtd_mdsi_each, L.mtd_mdsi_ws_bytes, srcs, (3, B), (3, B, H, W, k), (B, H, W, k, opts, MDSI_COMBINATIONS.index(combination)),
                      _parts(parts, 3, B, MDSI_PARTS, device=srcs[1].device))


def vsi_per_slice(input, target, pred, **kw):
    """vsi_each as host numbers: a list of B (input, gt, pred) triples (the kernels' float64 scores).  One device -> host copy
    for the batch."""
    return _who_triples(vsi_each(input, target, pred, **kw).tolist())


def mdsi_per_slice(input, target, pred, **kw):
    """mdsi_each as host numbers: a list of B (input, gt, pred) triples.  One device -> host copy for the batch."""
    return _who_triples(mdsi_each(input, target, pred, **kw).tolist())


def compute_VSI(input, target, pred, data_range=1.0, **kw):
    """piq's vsi(a, target) with its defaults (or the nine options) for a = input, target, pred: (input, gt, pred) floats, each the
    mean over the batch of the per-image scores (reduction='mean')."""
    return tuple(_batch_means("vsi", data_range, vsi_each, input, target, pred, **kw).tolist())


def compute_MDSI(input, target, pred, data_range=1.0, **kw):
    """piq's mdsi(a, target) with its defaults (or the ten options) for a = input, target, pred: (input, gt, pred) floats, each
    the mean over the batch of the per-image scores (reduction='mean')."""
    return tuple(_batch_means("mdsi", data_range, mdsi_each, input, target, pred, **kw).tolist())


# ================================================================================================ BRISQUE and total variation
BRISQUE_MIN_SIDE, BRISQUE_MAX_SIDE = 16, 1024
BRISQUE_PARTS = 37                                              # the 36 features before the range scaling, then the score
BRISQUE_OPTIONS = ("kernel_size", "kernel_sigma")
BRISQUE_MAX_KERNEL = 15
TV_MIN_SIDE, TV_MAX_SIDE = 16, 1024
TV_NORMS = ("l1", "l2", "l2_squared")                           # the order of MTD_TV_L1, MTD_TV_L2, MTD_TV_L2_SQUARED
TV_OPTIONS = ("norm_type",)


def brisque_check_options(kernel_size=7, kernel_sigma=7 / 6, interpolation="nearest"):
    """ValueError unless kernel_size is an odd int in 3..15, kernel_sigma a positive finite number and interpolation 'nearest'
    (the one resampling rule the kernels have)."""
    if interpolation != "nearest":
        raise ValueError(f"brisque: the kernels resample with interpolation 'nearest' only, got {interpolation!r}")
    if not (isinstance(kernel_size, int) and not isinstance(kernel_size, bool) and 3 <= kernel_size <= BRISQUE_MAX_KERNEL and kernel_size % 2 == 1):
        raise ValueError(f"brisque: kernel_size must be an odd int in 3..{BRISQUE_MAX_KERNEL}, got {kernel_size!r}")
    if not (_number(kernel_sigma) and kernel_sigma > 0):
        raise ValueError(f"brisque: kernel_sigma must be a positive number, got {kernel_sigma!r}")


def tv_check_options(norm_type="l2"):
    """ValueError unless norm_type is one of TV_NORMS."""
    if not (isinstance(norm_type, str) and norm_type in TV_NORMS):
        raise ValueError(f"tv: norm_type must be one of {TV_NORMS}, got {norm_type!r}")


@functools.lru_cache(maxsize=16)
def brisque_gaussian_table(kernel_size=7, kernel_sigma=7 / 6):
    """The (kernel_size, kernel_size) float32 host table of the MSCN map's Gaussian filter, normalised to sum 1 in two dimensions:
    float32 throughout and each element through piq's sequence of roundings (functional/filters.py: gaussian_filter), so the bytes
    are those of piq's own filter (tests/golden/brisque_tv_piq.npz holds their CRC-32).  Cached; do not modify the result."""
    brisque_check_options(kernel_size, kernel_sigma)
    c = torch.arange(kernel_size).to(dtype=torch.float32)
    c -= (kernel_size - 1) / 2.
    sq = c ** 2
    table = (-(sq.unsqueeze(0) + sq.unsqueeze(1)) / (2 * kernel_sigma ** 2)).exp()
    table /= table.sum()
    return table.contiguous()


@functools.lru_cache(maxsize=1)
def brisque_ggd_tables():
    """The (3, 9801) float64 host table of the shape look-ups: piq's grid gamma = arange(0.2, 10.001, 0.001) -- built in float32
    and widened, as piq's `.to(x)` widens it in a float64 run --, the generalised Gaussian's r(gamma) = G(1/g) G(3/g) / G(2/g)^2
    and the asymmetric one's G(2/g)^2 / (G(1/g) G(3/g)), both by piq's expressions on lgamma in float64.  Cached; do not modify."""
    gamma = torch.arange(0.2, 10.001, 0.001).double()
    one, two, three = torch.lgamma(1. / gamma), torch.lgamma(2. / gamma), torch.lgamma(3. / gamma)
    return torch.stack([gamma, (one + three - 2 * two).exp(), torch.exp(2 * two - one - three)]).contiguous()


def brisque_weights(obj):
    """The support vector regression of BRISQUE as one (n_sv, 37) float64 table, column 0 the coefficient and columns 1..36 the
    support vector: `obj` is piq's (sv_coef, sv) pair -- floating-point tensors of shapes (n_sv,) or (n_sv, 1), and (n_sv, 36) --,
    a path that torch.load reads to such a pair (the format of piq's brisque_svm_weights.pt), or a table this function returned.
    ValueError otherwise, for a non-finite entry and for n_sv == 0.  No weights ship with this package, and the published file
    was never seen here: the layout is the one module/piq/brisque.py reads."""
    obj = _load_weights_file(obj)
    checked = torch.is_tensor(obj) and obj.dtype == torch.float64 and obj.dim() == 2 and obj.shape[1] == 37
    if checked:
        table = obj.detach()
    else:
        if not isinstance(obj, (list, tuple)) or len(obj) != 2 or not all(torch.is_tensor(t) and t.is_floating_point() for t in obj):
            raise ValueError("brisque_weights: a pair (sv_coef, sv) of floating-point tensors expected, got "
                             f"{[tuple(t.shape) for t in obj] if isinstance(obj, (list, tuple)) and all(torch.is_tensor(t) for t in obj) else type(obj).__name__}")
        coef, sv = obj
        if sv.dim() != 2 or sv.shape[1] != 36 or tuple(coef.shape) not in ((sv.shape[0],), (sv.shape[0], 1)):
            raise ValueError(f"brisque_weights: sv_coef of shape (n_sv,) or (n_sv, 1) and sv of shape (n_sv, 36) expected, got "
                             f"{tuple(coef.shape)} and {tuple(sv.shape)}")
        table = torch.cat([coef.detach().double().reshape(-1, 1), sv.detach().double()], dim=1)
    if table.shape[0] == 0:
        raise ValueError("brisque_weights: no support vector (n_sv == 0)")
    if not (checked and table.is_cuda) and not bool(torch.isfinite(table).all()):       # (no host read for a table already on the device)
        raise ValueError("brisque_weights: a coefficient or support vector entry is not finite")
    return table.contiguous()


_brisque_device_tables = {}


def brisque_each(input, target, pred, *, weights, kernel_size=7, kernel_sigma=7 / 6, interpolation="nearest", parts=False):
    """BRISQUE (piq's brisque, data_range 1, two scales) of every slice of input, target and pred, each image set on its own (the
    metric has no reference image), without a host read: a (3, B) float64 device tensor.  `weights`: the support vector regression
    in a form brisque_weights takes (the caller's: none ships with this package).  With parts=True also the (3, B, 37) float64
    rows: the 36 features before the range scaling (per scale alpha, sigma^2, then for the shifts (0,1), (1,0), (1,1), (-1,1) alpha,
    eta, sigma_l^2, sigma_r^2), then the score.  All double in a fixed order (mtd_brisque_each): a slice's values depend neither on
    the batch it is in nor on the other two image sets; an image set passed twice is computed once.
    One deviation from piq: where piq asserts -- an MSCN map of zero variance (its first assert is `.all()` over the batch, which
    would make a slice depend on its batch), a product map without a negative or a positive value, a zero left or right sigma --
    the slice's score and parts are NaN and the other slices are untouched.  Sides in 16..1024, kernel_size odd in 3..15,
    interpolation 'nearest'; anything else is a ValueError."""
    brisque_check_options(kernel_size, kernel_sigma, interpolation)
    table = brisque_weights(weights)
    srcs, B, H, W = _each_sources("brisque", input, target, pred, BRISQUE_MIN_SIDE, BRISQUE_MAX_SIDE)
    dev = srcs[1].device
    table = table.to(dev)
    taps = _device_cached(_brisque_device_tables, ("taps", kernel_size, float(kernel_sigma)), dev,
                          lambda: brisque_gaussian_table(kernel_size, kernel_sigma).to(dev))
    ggd = _device_cached(_brisque_device_tables, ("ggd",), dev, lambda: brisque_ggd_tables().to(dev))
    L = _lib.lib()
    return _each_call(L.mtd_brisque_each, L.mtd_brisque_ws_bytes, srcs, (3, B), (3, B, H, W),
                      (B, H, W, kernel_size, taps.data_ptr(), ggd.data_ptr(), ggd.shape[1], table.data_ptr(), table.shape[0]),
                      _parts(parts, 3, B, BRISQUE_PARTS, device=dev), target=False)


def tv_each(input, target, pred, norm_type="l2"):
    """Total variation (piq's total_variation) of every slice of input, target and pred, each image set on its own, without a host
    read: a (3, B) float64 device tensor.  norm_type 'l1': the sum of |dy| and |dx| of neighbouring pixels; 'l2': the square root of
    the sum of their squares; 'l2_squared': that sum.  All double in a fixed order (mtd_tv_each): a slice's value depends neither
    on the batch it is in nor on the other two image sets; a constant slice gives exactly 0.  Sides in 16..1024 (ValueError)."""
    tv_check_options(norm_type)
    srcs, B, H, W = _each_sources("tv", input, target, pred, TV_MIN_SIDE, TV_MAX_SIDE)
    L = _lib.lib()
    return _each_call(L.mtd_tv_each, L.mtd_tv_ws_bytes, srcs, (3, B), (3, B, H, W), (B, H, W, TV_NORMS.index(norm_type)), rows=False, target=False)


def brisque_per_slice(input, target, pred, **kw):
    """brisque_each as host numbers: a list of B (input, gt, pred) triples.  One device -> host copy for the batch."""
    return _who_triples(brisque_each(input, target, pred, **kw).tolist())


def tv_per_slice(input, target, pred, **kw):
    """tv_each as host numbers: a list of B (input, gt, pred) triples.  One device -> host copy for the batch."""
    return _who_triples(tv_each(input, target, pred, **kw).tolist())


def compute_BRISQUE(input, target, pred, data_range=1.0, **kw):
    """piq's brisque(a) with its defaults (or kernel_size, kernel_sigma) on the caller's `weights` for a = input, target, pred:
    (input, gt, pred) floats, each the mean over the batch of the per-image scores (reduction='mean')."""
    return tuple(_batch_means("brisque", data_range, brisque_each, input, target, pred, **kw).tolist())


def compute_TV(input, target, pred, data_range=1.0, **kw):
    """piq's total_variation(a, norm_type=...) for a = input, target, pred: (input, gt, pred) floats, each the mean over the batch
    of the per-image values (reduction='mean')."""
    return tuple(_batch_means("tv", data_range, tv_each, input, target, pred, **kw).tolist())


# ================================================================================================ perceptual metrics
# torchvision vgg19().features: index of each conv -> (C_in, C_out); ReLU follows at index + 1
_VGG19_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (16, 256, 256),
                (19, 256, 512), (21, 512, 512), (23, 512, 512), (25, 512, 512), (28, 512, 512))
_VGG19_POOL_AFTER = (3, 8, 17, 26)          # nn.MaxPool2d(2, 2) at indices 4, 9, 18, 27
_VGG19_TAPS = (1, 6, 11, 20, 29)            # relu1_1, relu2_1, relu3_1, relu4_1, relu5_1 (metrics.py:53-62)
LEVEL_WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)      # metrics.py:82,118
TML_PATCH = 16                              # TextureMatchingLoss(patch_size=16, use_patch=True), the reference's default
_MAX_MAP_BYTES = (1 << 31) - 1              # the conv entry points address a map with 32-bit byte offsets: strictly below 2^31 bytes


def maxpool2x2(x):
    """nn.MaxPool2d(2, 2) of a contiguous NHWC fp32 map (mtd_maxpool2x2)."""
    B, H, W, Cc = x.shape
    out = torch.empty((B, H // 2, W // 2, Cc), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mtd_maxpool2x2(x.data_ptr(), out.data_ptr(), B, H, W, Cc, K.stream_ptr()), "mtd_maxpool2x2")
    return out


def patch_gram_l1(x, y, out=None):
    """Sum over the 16 x 16 patches and all C^2 entries of |G(x) - G(y)| of two contiguous NHWC fp32 maps: one device double
    (mtd_patch_gram_l1; written to the 1-element float64 tensor `out` when given)."""
    if x.shape != y.shape or x.dim() != 4 or not (x.is_cuda and y.is_cuda) or not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("patch_gram_l1: two contiguous CUDA NHWC maps of one shape expected")
    B, h, w, Cc = x.shape
    L = _lib.lib()
    need = L.mtd_patch_gram_l1_ws_bytes(B, h, w, Cc)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=x.device)
    ws = K.workspace(max(need, 8), x.device)
    _lib.check(L.mtd_patch_gram_l1(x.data_ptr(), y.data_ptr(), B, h, w, Cc, out.data_ptr(), ws.data_ptr(), K.stream_ptr()), "mtd_patch_gram_l1")
    return out


def patch_gram_l1_each(x, y, out=None, out_stride=1):
    """patch_gram_l1 image by image: B device doubles, [i] with the bits of patch_gram_l1(x[i:i+1], y[i:i+1])
    (mtd_patch_gram_l1_each).  With `out`, a float64 tensor (or view) of at least (B - 1) * out_stride + 1 elements, image i's sum
    goes to its element i * out_stride and nothing else is written."""
    if x.shape != y.shape or x.dim() != 4 or not (x.is_cuda and y.is_cuda) or not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("patch_gram_l1_each: two contiguous CUDA NHWC maps of one shape expected")
    B, h, w, Cc = x.shape
    if out_stride < 1:
        raise ValueError("patch_gram_l1_each: out_stride of at least 1 expected")
    if out is None:
        out = torch.empty((B - 1) * out_stride + 1, dtype=torch.float64, device=x.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() < (B - 1) * out_stride + 1:
        raise ValueError("patch_gram_l1_each: `out` must be a contiguous float64 tensor of at least (B - 1) * out_stride + 1 elements")
    L = _lib.lib()
    ws = K.workspace(max(L.mtd_patch_gram_l1_ws_bytes(B, h, w, Cc), 8), x.device)
    _lib.check(L.mtd_patch_gram_l1_each(x.data_ptr(), y.data_ptr(), B, h, w, Cc, out.data_ptr(), out_stride, ws.data_ptr(), K.stream_ptr()),
               "mtd_patch_gram_l1_each")
    return out


def l2pool3x3s2(x):
    """DISTS's L2Pool2d(3, stride 2, padding 1) of a contiguous NHWC fp32 map: sqrt(hann3x3 * x^2 + 1e-12), ceil(H / 2) x ceil(W / 2)
    outputs (mtd_l2pool3x3s2)."""
    B, H, W, Cc = x.shape
    out = torch.empty((B, (H + 1) // 2, (W + 1) // 2, Cc), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mtd_l2pool3x3s2(x.data_ptr(), out.data_ptr(), B, H, W, Cc, K.stream_ptr()), "mtd_l2pool3x3s2")
    return out


def _vgg_walk(layers, t, taps, pool_after, pool):
    """The conv / ReLU / pool / tap walk of a torchvision VGG `features` stack on an NHWC chunk t: `layers` are (features index,
    weight (N, C, 3, 3), bias) of the 3 x 3 convs in order, a ReLU follows each at index + 1; the map is tapped where that index
    is in `taps` and pooled by `pool` where it is in `pool_after`.  Returns the tapped maps."""
    maps = []
    for idx, w, b in layers:
        B, H, W, Cc = t.shape
        N = w.shape[0]
        out = torch.empty((B, H, W, N), dtype=torch.float32, device=t.device)
        K.conv(t, w, K.geom_fwd(B, H, W, 3, 1, 1), N, Cc, Cc * 9, 9, out, bias=b, act=_lib.ACT_RELU)
        t = out
        if idx + 1 in taps:
            maps.append(t)
        if idx + 1 in pool_after:
            t = pool(t)
    return maps


def _vgg_state(name, weights, convs):
    """The (weight, bias) pairs of `convs` from a torchvision-layout state dict or a path to one; ValueError for a missing key or
    a wrong shape."""
    if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
        weights = torch.load(weights, map_location="cpu", weights_only=True)
    pairs = []
    for idx, cin, cout in convs:
        got = []
        for leaf, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            key = f"features.{idx}.{leaf}"
            if key not in weights:
                raise ValueError(f"{name}: the state dict has no {key!r}")
            t = weights[key]
            if not torch.is_tensor(t) or tuple(t.shape) != shape:
                raise ValueError(f"{name}: {key!r} has shape {tuple(getattr(t, 'shape', ()))}, expected {shape}")
            got.append(t.detach())
        pairs.append((idx, got[0], got[1]))
    return pairs


class VGG19Features:
    """The feature part of torchvision's VGG-19 up to relu5_1 on the HIP conv kernels, for single-channel images.

    `weights`: a state dict in torchvision's `vgg19` key layout (features.{0,2,5,...,28}.{weight,bias}; other keys such as
    classifier.* are ignored) or a path to one (read with torch.load(..., weights_only=True)).  The reference feeds
    x.repeat(1, 3, 1, 1) without ImageNet normalisation (metrics.py:87,145), so the first layer is folded to 1 -> 64 channels:
    its three input-channel slices are summed once, here.  The weights go to the device of the first call's input, once."""

    def __init__(self, weights):
        self.layers = []                     # (features index, weight (N, C, 3, 3), bias (N,)) in fp32, first layer folded
        for idx, w, b in _vgg_state("VGG19Features", weights, _VGG19_CONVS):
            if idx == 0:
                w = w.double().sum(dim=1, keepdim=True)
            self.layers.append((idx, w.float().contiguous(), b.float().contiguous()))
        self._device = None

    def to(self, device):
        device = torch.device(device)
        if self._device != device:
            self.layers = [(i, w.to(device), b.to(device)) for i, w, b in self.layers]
            self._device = device
        return self

    def _chunk(self, x):
        """The five maps of one chunk of images, (B, H, W, 1) in NHWC."""
        return _vgg_walk(self.layers, x, _VGG19_TAPS, _VGG19_POOL_AFTER, maxpool2x2)

    @torch.no_grad()
    def __call__(self, x):
        """x: (B, 1, H, W) fp32 CUDA, H, W >= 16.  Returns the NHWC maps relu1_1 ... relu5_1:
        (B, H, W, 64), (B, H/2, W/2, 128), (B, H/4, W/4, 256), (B, H/8, W/8, 512), (B, H/16, W/16, 512) (floor at every pool)."""
        if x.dim() != 4 or x.shape[1] != 1:
            raise AssertionError("VGG19Features expects a (B,1,H,W) tensor")
        if not x.is_cuda:
            raise RuntimeError("VGG19Features: HIP path needs CUDA tensors (no CPU fallback)")
        B, _, H, W = x.shape
        if H < 16 or W < 16:
            raise ValueError(f"VGG19Features: images of at least 16 x 16 expected (four pools before relu5_1), got {H} x {W}")
        per_image = H * W * 64 * 4                   # relu1_1, the largest map
        if per_image > _MAX_MAP_BYTES:
            raise ValueError(f"VGG19Features: a {H} x {W} image gives a first feature map of 2^31 bytes or more")
        self.to(x.device)
        x = x.detach().contiguous().float().reshape(B, H, W, 1)       # one channel: NCHW and NHWC coincide
        step = max(1, _MAX_MAP_BYTES // per_image)
        if B <= step:
            return self._chunk(x)
        parts = [self._chunk(x[i:i + step]) for i in range(0, B, step)]
        return [torch.cat([p[lvl] for p in parts]) for lvl in range(5)]


def _perceptual_inputs(name, input, target, pred, vgg, min_side):
    if not isinstance(vgg, VGG19Features):
        raise TypeError(f"{name}: pass the feature network as vgg=VGG19Features(state_dict) (no pretrained weights ship with this package)")
    for t in (input, target, pred):
        if t.dim() != 4 or t.shape != target.shape or t.shape[1] != 1:
            raise AssertionError(f"{name} expects three (B,1,H,W) tensors of the same shape")
        if not t.is_cuda:
            raise RuntimeError(f"{name}: HIP path needs CUDA tensors (no CPU fallback)")
    H, W = target.shape[2:]
    if H < min_side or W < min_side:
        raise ValueError(f"{name}: images of at least {min_side} x {min_side} expected, got {H} x {W}"
                         + (" (relu5_1 must hold one 16 x 16 patch; the reference returns NaN here)" if min_side > 16 else ""))


def _stacked_features(vgg, target, others):
    """The network once on the stacked images: per level (target map, [map of each other])."""
    B = target.shape[0]
    maps = vgg(torch.cat([target] + list(others)))
    return [(m[:B], [m[(k + 1) * B:(k + 2) * B] for k in range(len(others))]) for m in maps]


def _pl_values(levels, who):
    """who: indices into (target, *others) with 0 = the target itself, whose distance to itself is the constant 0 (no launch).
    One float per entry of `who`."""
    terms = []
    for k in who:
        if k == 0:
            continue
        for wgt, (ft, fo) in zip(LEVEL_WEIGHTS, levels):
            terms.append(K.make_term(1, fo[k - 1], ft, scale=wgt / ft.numel()))
    dev = levels[0][0].device
    vals = K.loss_terms(terms, dev)
    others = [k for k in who if k != 0]
    sums = K.scalar_sums([(vals[5 * i:5 * i + 5], None) for i in range(len(others))], dev)
    if len(others) == len(who):
        return sums
    zero = torch.zeros(1, dtype=torch.float32, device=dev)
    return torch.cat([zero if k == 0 else sums[others.index(k):others.index(k) + 1] for k in who])      # (layout only)


def _tml_values(levels, who):
    """As _pl_values: the target's own entry costs no Gram launch, its five sums stay 0."""
    import ctypes
    dev = levels[0][0].device
    sums = torch.zeros(5 * len(who), dtype=torch.float64, device=dev)
    scales = (ctypes.c_double * 5)()
    for lvl, (wgt, (ft, fo)) in enumerate(zip(LEVEL_WEIGHTS, levels)):
        B, h, w, Cc = ft.shape
        scales[lvl] = wgt / (float(B * (h // TML_PATCH) * (w // TML_PATCH)) * Cc * Cc)
        for i, k in enumerate(who):
            if k != 0:
                patch_gram_l1(fo[k - 1], ft, out=sums[5 * i + lvl:5 * i + lvl + 1])
    out = torch.empty(len(who), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().mtd_scaled_sums_f64(sums.data_ptr(), len(who), 5, scales, out.data_ptr(), K.stream_ptr()), "mtd_scaled_sums_f64")
    return out


def _triple(vals, option):
    return (vals[0], vals[1], vals[2]) if option else vals[0]


@torch.no_grad()
def compute_PL(input, target, pred, option=True, device=None, *, vgg):
    """metrics.py:93-106: sum_i w_i * mean|f_i(a) - f_i(target)| over the five VGG-19 maps, w = [1/32, 1/16, 1/8, 1/4, 1], for
    a = input, target, pred (option=True: a triple of 0-dim device tensors, the middle one the constant 0) or pred alone.
    `device` is accepted for the reference's signature; the tensors' device is used.  H, W >= 16."""
    _perceptual_inputs("compute_PL", input, target, pred, vgg, 16)
    levels = _stacked_features(vgg, target, (input, pred) if option else (pred,))
    return _triple(_pl_values(levels, (1, 0, 2) if option else (1,)), option)


@torch.no_grad()
def compute_TML(input, target, pred, option=True, device=None, *, vgg):
    """metrics.py:156-168 with its defaults (patch 16, use_patch=True): sum_i w_i * mean over (B * patches, C, C) of
    |G(f_i(a)) - G(f_i(target))|, G the unnormalised Gram matrix of a 16 x 16 patch of the map.  H, W >= 256, so that relu5_1
    holds a patch (the reference's nn.Unfold yields no patch below that and its mean is NaN): ValueError otherwise."""
    _perceptual_inputs("compute_TML", input, target, pred, vgg, 16 * TML_PATCH)
    levels = _stacked_features(vgg, target, (input, pred) if option else (pred,))
    return _triple(_tml_values(levels, (1, 0, 2) if option else (1,)), option)


@torch.no_grad()
def perceptual_metrics(input, target, pred, vgg):
    """PL and TML of the test loop from ONE pass of the network: a device vector (input_pl, gt_pl, pred_pl, input_tml, gt_tml,
    pred_tml), the same values as compute_PL / compute_TML."""
    _perceptual_inputs("perceptual_metrics", input, target, pred, vgg, 16 * TML_PATCH)
    levels = _stacked_features(vgg, target, (input, pred))
    return torch.cat([_pl_values(levels, (1, 0, 2)), _tml_values(levels, (1, 0, 2))])


def _pl_each(levels):
    """PL of every image of the two others against the target: (2, B) floats, one loss_terms call of 2 * 5 * B terms (a term per
    image and level on the image's slice of the map, scale w_level / (h * w * C): the bits of the one-image term) and one
    launch for the sums over the levels."""
    B = levels[0][0].shape[0]
    terms = []
    for k in range(2):
        for i in range(B):
            for wgt, (ft, fo) in zip(LEVEL_WEIGHTS, levels):
                terms.append(K.make_term(1, fo[k][i], ft[i], scale=wgt / ft[i].numel()))
    dev = levels[0][0].device
    vals = K.loss_terms(terms, dev)
    return K.scalar_sums([(vals[5 * j:5 * j + 5], None) for j in range(2 * B)], dev).reshape(2, B)


def _tml_each(levels):
    """TML of every image: (3, B) floats, rows input, gt (the constant 0, no launch), pred.  Ten patch_gram_l1_each calls write
    a (who, image, level) table of doubles, one mtd_scaled_sums_f64 weighs the levels."""
    import ctypes
    B = levels[0][0].shape[0]
    dev = levels[0][0].device
    sums = torch.zeros(3 * B * 5, dtype=torch.float64, device=dev)
    scales = (ctypes.c_double * 5)()
    for lvl, (wgt, (ft, fo)) in enumerate(zip(LEVEL_WEIGHTS, levels)):
        _, h, w, Cc = ft.shape
        scales[lvl] = wgt / (float((h // TML_PATCH) * (w // TML_PATCH)) * Cc * Cc)
        for k, who in enumerate((0, 2)):
            patch_gram_l1_each(fo[k], ft, out=sums[who * B * 5 + lvl:], out_stride=5)
    out = torch.empty(3 * B, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().mtd_scaled_sums_f64(sums.data_ptr(), 3 * B, 5, scales, out.data_ptr(), K.stream_ptr()), "mtd_scaled_sums_f64")
    return out.reshape(3, B)


@torch.no_grad()
def perceptual_metrics_per_slice(input, target, pred, vgg):
    """perceptual_metrics of every slice of a batch from ONE pass of the network on the 3B stacked images: a (6, B) float32
    device tensor, rows input_pl, gt_pl, pred_pl, input_tml, gt_tml, pred_tml (the gt rows the constant 0).  The reductions of
    slice i are those of a one-slice call on slice i of the maps, bit for bit; the maps themselves come from convolutions on 3B
    images, which may take another plan than on 3."""
    _perceptual_inputs("perceptual_metrics_per_slice", input, target, pred, vgg, 16 * TML_PATCH)
    levels = _stacked_features(vgg, target, (input, pred))
    pl = _pl_each(levels)
    zero = torch.zeros((1, target.shape[0]), dtype=torch.float32, device=pl.device)
    return torch.cat([pl[0:1], zero, pl[1:2], _tml_each(levels)])


# ================================================================================================ LPIPS, DISTS
# torchvision vgg16().features: index of each conv -> (C_in, C_out); ReLU follows at index + 1
_VGG16_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
                (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
_VGG16_POOL_AFTER = (3, 8, 15, 22)          # the pools at indices 4, 9, 16, 23 (the one at 30 lies behind the last tap)
_VGG16_TAPS = (3, 8, 15, 22, 29)            # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (perceptual.py: lpips_layers, dists_layers)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
LPIPS_CHANNELS = (64, 128, 256, 512, 512)
DISTS_CHANNELS = (3, 64, 128, 256, 512, 512)
LPIPS_DISTANCES = ("mse", "mae")            # MTD_LPIPS_MSE / MTD_LPIPS_MAE


def vgg16_first_layer(weight, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The first conv of VGG-16 on a grey image x normalised per channel, (x - mean_c) / std_c, as a conv on the two channels
    (x, 1): (N, 3, 3, 3) -> (N, 2, 3, 3) float64 with [:, 0] = sum_c w_c / std_c and [:, 1] = -sum_c w_c mean_c / std_c.  Zero
    padding then pads both channels, which is what the reference's padding after the normalisation does: the constant part is
    NOT a bias, it is absent where a tap lies outside the image.  mean and std are rounded to float32 first: piq holds them as
    float32 tensors whatever the image's dtype."""
    w = weight.double()
    m = torch.tensor(mean, dtype=torch.float32).double().view(1, 3, 1, 1)
    sd = torch.tensor(std, dtype=torch.float32).double().view(1, 3, 1, 1)
    return torch.cat([(w / sd).sum(dim=1, keepdim=True), -(w * m / sd).sum(dim=1, keepdim=True)], dim=1)


class VGG16Features:
    """The feature part of torchvision's VGG-16 up to relu5_3 on the HIP conv kernels, for single-channel images, as piq's LPIPS
    and DISTS use it (module/piq/perceptual.py): the grey image is broadcast against the three ImageNet constants, (x - mean) /
    std, and tapped after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3.

    `weights`: a state dict in torchvision's `vgg16` key layout (features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias};
    other keys are ignored) or a path to one (read with torch.load(..., weights_only=True)); no pretrained weights ship with this
    package.  The normalisation is folded into the first layer exactly (vgg16_first_layer: two input channels, the image and
    ones, in float64 on the host).  The weights go to the device of the first call's input, once."""

    def __init__(self, weights, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        if len(mean) != 3 or len(std) != 3 or not all(float(v) > 0 for v in std):
            raise ValueError(f"VGG16Features: three means and three positive stds expected, got {mean!r}, {std!r}")
        self.layers = []                     # (features index, weight (N, C, 3, 3), bias (N,)) in fp32, first layer folded to (x, 1)
        for idx, w, b in _vgg_state("VGG16Features", weights, _VGG16_CONVS):
            if idx == 0:
                w = vgg16_first_layer(w, mean, std)
            self.layers.append((idx, w.float().contiguous(), b.float().contiguous()))
        self._device = None

    def to(self, device):
        device = torch.device(device)
        if self._device != device:
            self.layers = [(i, w.to(device), b.to(device)) for i, w, b in self.layers]
            self._device = device
        return self

    @torch.no_grad()
    def __call__(self, x, pool="max"):
        """x: (B, 1, H, W) fp32 CUDA, H, W >= 16.  Returns the NHWC maps relu1_2 ... relu5_3 with 64, 128, 256, 512, 512 channels.
        pool="max": nn.MaxPool2d(2, 2), sides H, H//2, H//4 ... (floor); pool="l2": DISTS's L2Pool2d(3, 2, 1), sides H,
        ceil(H/2), ... (ceil at every pool)."""
        if pool not in ("max", "l2"):
            raise ValueError(f"VGG16Features: pool must be 'max' or 'l2', got {pool!r}")
        if x.dim() != 4 or x.shape[1] != 1:
            raise AssertionError("VGG16Features expects a (B,1,H,W) tensor")
        if not x.is_cuda:
            raise RuntimeError("VGG16Features: HIP path needs CUDA tensors (no CPU fallback)")
        B, _, H, W = x.shape
        if H < 16 or W < 16:
            raise ValueError(f"VGG16Features: images of at least 16 x 16 expected (four pools before relu5_3), got {H} x {W}")
        per_image = H * W * 64 * 4                   # relu1_2, the largest map
        if per_image > _MAX_MAP_BYTES:
            raise ValueError(f"VGG16Features: a {H} x {W} image gives a first feature map of 2^31 bytes or more")
        self.to(x.device)
        x = x.detach().contiguous().float().reshape(B, H, W, 1)
        x = torch.cat([x, torch.ones_like(x)], dim=3)                  # the channels (x, 1) of the folded first layer
        pool_fn = maxpool2x2 if pool == "max" else l2pool3x3s2
        step = max(1, _MAX_MAP_BYTES // per_image)
        if B <= step:
            return _vgg_walk(self.layers, x, _VGG16_TAPS, _VGG16_POOL_AFTER, pool_fn)
        parts = [_vgg_walk(self.layers, x[i:i + step], _VGG16_TAPS, _VGG16_POOL_AFTER, pool_fn) for i in range(0, B, step)]
        return [torch.cat([p[lvl] for p in parts]) for lvl in range(5)]


def _load_weights_file(obj):
    if isinstance(obj, (str, bytes)) or hasattr(obj, "__fspath__"):
        return torch.load(obj, map_location="cpu", weights_only=True)
    return obj


def lpips_weights(obj):
    """LPIPS's linear-layer weights as one float64 table of 64 + 128 + 256 + 512 + 512 = 1472 entries (level after level, on the
    device the entries came from): `obj` is a list / tuple of five tensors with 64, 128, 256, 512, 512 elements of any shape (piq's
    lpips_weights.pt holds them as (1, C, 1, 1)), a path to such a file, or a table this function returned.  ValueError with the
    offending shape otherwise.  The published file was never seen here: the layout is the one module/piq/perceptual.py reads."""
    obj = _load_weights_file(obj)
    total = sum(LPIPS_CHANNELS)
    if torch.is_tensor(obj) and obj.dtype == torch.float64 and obj.dim() == 1 and obj.numel() == total:
        return obj.contiguous()
    if not isinstance(obj, (list, tuple)) or len(obj) != 5 or not all(torch.is_tensor(t) for t in obj):
        raise ValueError(f"lpips_weights: a list of five tensors with {LPIPS_CHANNELS} elements expected, got "
                         f"{[tuple(t.shape) for t in obj] if isinstance(obj, (list, tuple)) and all(torch.is_tensor(t) for t in obj) else type(obj).__name__}")
    for t, n in zip(obj, LPIPS_CHANNELS):
        if t.numel() != n or not (t.is_floating_point()):
            raise ValueError(f"lpips_weights: a floating-point tensor of {n} elements expected, got shape {tuple(t.shape)} {t.dtype}")
    return torch.cat([t.detach().double().flatten() for t in obj]).contiguous()


def dists_weights(obj):
    """DISTS's alpha and beta as one (2, 1475) float64 table (row 0 alpha, row 1 beta; 1475 = 3 + 64 + 128 + 256 + 512 + 512, the
    first three for the raw image): `obj` is a dict with `alpha` and `beta` of 1475 elements each in any shape (piq's
    dists_weights.pt holds them as (1, 1475, 1, 1)), a path to such a file, or a table this function returned.  ValueError with the
    offending shape otherwise.  The published file was never seen here: the layout is the one module/piq/perceptual.py reads."""
    obj = _load_weights_file(obj)
    total = sum(DISTS_CHANNELS)
    if torch.is_tensor(obj) and obj.dtype == torch.float64 and tuple(obj.shape) == (2, total):
        return obj.contiguous()
    if not isinstance(obj, dict) or "alpha" not in obj or "beta" not in obj:
        raise ValueError(f"dists_weights: a dict with 'alpha' and 'beta' of {total} elements each expected, got "
                         f"{sorted(obj) if isinstance(obj, dict) else type(obj).__name__}")
    rows = []
    for name in ("alpha", "beta"):
        t = obj[name]
        if not torch.is_tensor(t) or t.numel() != total or not t.is_floating_point():
            raise ValueError(f"dists_weights: {name!r} must be a floating-point tensor of {total} elements, got shape "
                             f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t).__name__)}")
        rows.append(t.detach().double().flatten())
    return torch.stack(rows).contiguous()


def lpips_level_each(t, a, b, weights, distance="mse", out=None, out_stride=1, other_stride=None):
    """Per image i and other map o = a (k = 0), b (k = 1; b may be None): sum over pixels and channels of
    w_c d(o_c / (|o| + 1e-10), t_c / (|t| + 1e-10)) of contiguous NHWC fp32 maps of one shape, C in {64, 128, 256, 512}, as device
    doubles at out[k * other_stride + i * out_stride] (mtd_lpips_level_each); nothing else of `out` is written.  weights: C
    float64 entries on the maps' device."""
    if distance not in LPIPS_DISTANCES:
        raise ValueError(f"lpips: distance must be one of {LPIPS_DISTANCES}, got {distance!r}")
    maps = [m for m in (t, a, b) if m is not None]
    if a is None or any(m.shape != t.shape or m.dim() != 4 or not m.is_cuda or not m.is_contiguous() or m.dtype != torch.float32 for m in maps):
        raise ValueError("lpips_level_each: contiguous CUDA NHWC fp32 maps of one shape expected")
    B, h, w, Cc = t.shape
    if weights.dtype != torch.float64 or weights.numel() != Cc or not weights.is_cuda or not weights.is_contiguous():
        raise ValueError(f"lpips_level_each: {Cc} contiguous float64 weights on the device expected")
    n = 2 if b is not None else 1
    if other_stride is None:
        other_stride = B * out_stride
    need = (n - 1) * other_stride + (B - 1) * out_stride + 1
    if out is None:
        out = torch.zeros(need, dtype=torch.float64, device=t.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() < need or out_stride < 1 or other_stride < 0:
        raise ValueError("lpips_level_each: `out` must be a contiguous float64 tensor that holds every addressed element")
    L = _lib.lib()
    nbytes = L.mtd_lpips_level_ws_bytes(B, h, w, Cc)
    if not nbytes:
        raise ValueError(f"lpips_level_each: maps of shape {tuple(t.shape)} are not taken (C in 64, 128, 256, 512)")
    ws = K.workspace(nbytes, t.device)
    _lib.check(L.mtd_lpips_level_each(t.data_ptr(), a.data_ptr(), b.data_ptr() if b is not None else None, B, h, w, Cc, weights.data_ptr(),
                                      LPIPS_DISTANCES.index(distance), out.data_ptr(), out_stride, other_stride, ws.data_ptr(), K.stream_ptr()),
               "mtd_lpips_level_each")
    return out


def channel_moments_each(t, a, b=None):
    """(B, C, 2 + 3 n) float64 table of per-image, per-channel sums over the pixels of contiguous NHWC fp32 maps of one shape
    (C = 1 or a multiple of 4 up to 1024): (sum t, sum t^2) and per other map o = a, b (b may be None) (sum o, sum o^2, sum o t)
    (mtd_channel_moments_each)."""
    maps = [m for m in (t, a, b) if m is not None]
    if a is None or any(m.shape != t.shape or m.dim() != 4 or not m.is_cuda or not m.is_contiguous() or m.dtype != torch.float32 for m in maps):
        raise ValueError("channel_moments_each: contiguous CUDA NHWC fp32 maps of one shape expected")
    B, h, w, Cc = t.shape
    n = 2 if b is not None else 1
    L = _lib.lib()
    nbytes = L.mtd_channel_moments_ws_bytes(B, h, w, Cc, n)
    if not nbytes:
        raise ValueError(f"channel_moments_each: maps of shape {tuple(t.shape)} are not taken (C = 1 or a multiple of 4 up to 1024)")
    out = torch.empty((B, Cc, 2 + 3 * n), dtype=torch.float64, device=t.device)
    ws = K.workspace(nbytes, t.device)
    _lib.check(L.mtd_channel_moments_each(t.data_ptr(), a.data_ptr(), b.data_ptr() if b is not None else None, B, h, w, Cc, out.data_ptr(),
                                          ws.data_ptr(), K.stream_ptr()), "mtd_channel_moments_each")
    return out


def dists_finish(tables, pixels, weights, self_row=-1, parts=False):
    """DISTS's closing formula on the six moment tables (channel_moments_each of the raw image and the five maps, one n and B):
    (rows, B) float64 scores 1 - sum(alpha S1 + beta S2), rows = the others in order, plus, with self_row >= 0, a row at that
    index for the target against itself (S1 = S2 = 1 exactly).  pixels: h * w per level; weights: dists_weights' table on the
    device.  With parts=True also the (rows, B, 6) level sums (mtd_dists_finish)."""
    import ctypes
    if len(tables) != 6 or len(pixels) != 6:
        raise ValueError("dists_finish: six tables and six pixel counts expected")
    B, _, Kk = tables[0].shape
    n = (Kk - 2) // 3
    for tb, c in zip(tables, (1,) + DISTS_CHANNELS[1:]):
        if tb.dtype != torch.float64 or tuple(tb.shape) != (B, c, Kk) or not tb.is_cuda or not tb.is_contiguous():
            raise ValueError(f"dists_finish: a contiguous CUDA float64 table of shape {(B, c, Kk)} expected, got {tuple(tb.shape)}")
    if weights.dtype != torch.float64 or tuple(weights.shape) != (2, sum(DISTS_CHANNELS)) or not weights.is_cuda or not weights.is_contiguous():
        raise ValueError("dists_finish: dists_weights' (2, 1475) float64 table on the device expected")
    rows = n + (1 if self_row >= 0 else 0)
    dev = tables[0].device
    out = torch.empty((rows, B), dtype=torch.float64, device=dev)
    lv = torch.empty((rows, B, 6), dtype=torch.float64, device=dev) if parts else None
    ptrs = (ctypes.c_void_p * 6)(*(tb.data_ptr() for tb in tables))
    px = (ctypes.c_longlong * 6)(*(int(p) for p in pixels))
    _lib.check(_lib.lib().mtd_dists_finish(ptrs, px, n, B, self_row, weights[0].data_ptr(), weights[1].data_ptr(), out.data_ptr(),
                                           lv.data_ptr() if parts else None, K.stream_ptr()), "mtd_dists_finish")
    return (out, lv) if parts else out


def _vgg16_inputs(name, input, target, pred, vgg):
    if not isinstance(vgg, VGG16Features):
        raise TypeError(f"{name}: pass the feature network as vgg=VGG16Features(state_dict) (no pretrained weights ship with this package)")
    _, H, W = _image_shape(f"{name} expects three", input, target, pred)
    _need_cuda(name, input, target, pred)
    if H < 16 or W < 16:
        raise ValueError(f"{name}: images of at least 16 x 16 expected, got {H} x {W}")


@torch.no_grad()
def lpips_each(input, target, pred, *, vgg, weights, distance="mse", parts=False):
    """LPIPS (piq's LPIPS: VGG-16, unit-normalised features, learned channel weights, data_range 1; replace_pooling=False) of
    every slice of (input, target, pred) against the same slice of target, without a host read: a (3, B) float64 device tensor,
    rows input, gt, pred; the gt row is the constant 0 (no reduction is launched for it).  One network pass on the 3B stacked
    images, one mtd_lpips_level_each per level (the target's map read once for both others), one launch weighs the levels by
    1 / (h w).  With parts=True also the (3, B, 5) per-level values.  vgg: VGG16Features; weights: lpips_weights' table or any
    form it takes; distance: "mse" (piq's default) or "mae".  H, W >= 16."""
    import ctypes
    _vgg16_inputs("lpips_each", input, target, pred, vgg)
    if distance not in LPIPS_DISTANCES:
        raise ValueError(f"lpips: distance must be one of {LPIPS_DISTANCES}, got {distance!r}")
    B = target.shape[0]
    dev = target.device
    table = lpips_weights(weights).to(dev)
    maps = vgg(torch.cat([target, input, pred]).float(), pool="max")
    sums = torch.zeros((3, B, 5), dtype=torch.float64, device=dev)
    scales = (ctypes.c_double * 5)()
    c0 = 0
    for lvl, m in enumerate(maps):
        _, h, w, Cc = m.shape
        scales[lvl] = 1.0 / float(h * w)
        lpips_level_each(m[:B], m[B:2 * B], m[2 * B:], table[c0:c0 + Cc], distance, out=sums.view(-1)[lvl:], out_stride=5, other_stride=2 * B * 5)
        c0 += Cc
    out = torch.empty((3, B), dtype=torch.float64, device=dev)
    lv = torch.empty((3, B, 5), dtype=torch.float64, device=dev) if parts else None
    _lib.check(_lib.lib().mtd_scaled_sums_f64_f64(sums.data_ptr(), 3 * B, 5, scales, out.data_ptr(), lv.data_ptr() if parts else None, K.stream_ptr()),
               "mtd_scaled_sums_f64_f64")
    return (out, lv) if parts else out


@torch.no_grad()
def dists_each(input, target, pred, *, vgg, weights, parts=False):
    """DISTS (piq's DISTS: VGG-16 with L2 pooling, the raw image as level 0, structure and texture similarity of the per-channel
    moments, data_range 1) of every slice of (input, target, pred) against the same slice of target, without a host read: a
    (3, B) float64 device tensor, rows input, gt, pred; the gt row is the constant 1 - sum(alpha + beta) of the finish arithmetic.
    One network pass (pool="l2") on the 3B stacked images, one mtd_channel_moments_each per level, one mtd_dists_finish.  With
    parts=True also the (3, B, 6) per-level sums of alpha S1 + beta S2.  vgg: VGG16Features; weights: dists_weights' table or any
    form it takes.  H, W >= 16."""
    _vgg16_inputs("dists_each", input, target, pred, vgg)
    B, _, H, W = target.shape
    dev = target.device
    table = dists_weights(weights).to(dev)
    stacked = torch.cat([target, input, pred]).float().contiguous()
    maps = [stacked.reshape(3 * B, H, W, 1)] + vgg(stacked, pool="l2")
    tables = [channel_moments_each(m[:B], m[B:2 * B], m[2 * B:]) for m in maps]
    return dists_finish(tables, [m.shape[1] * m.shape[2] for m in maps], table, self_row=1, parts=parts)


def lpips_per_slice(input, target, pred, **kw):
    """lpips_each as host numbers: a list of B (input, gt, pred) triples.  One device -> host copy for the batch."""
    return _who_triples(lpips_each(input, target, pred, **kw).tolist())


def dists_per_slice(input, target, pred, **kw):
    """dists_each as host numbers: a list of B (input, gt, pred) triples.  One device -> host copy for the batch."""
    return _who_triples(dists_each(input, target, pred, **kw).tolist())


def compute_LPIPS(input, target, pred, data_range=1.0, **kw):
    """piq's LPIPS(reduction='mean')(a, target) for a = input, target, pred: a triple of 0-dim float64 device tensors, each the mean
    over the batch of the per-image scores.  Keywords as lpips_each (vgg, weights, distance)."""
    return tuple(_batch_means("lpips", data_range, lpips_each, input, target, pred, **kw).unbind())


def compute_DISTS(input, target, pred, data_range=1.0, **kw):
    """piq's DISTS(reduction='mean')(a, target) likewise.  Keywords as dists_each (vgg, weights)."""
    return tuple(_batch_means("dists", data_range, dists_each, input, target, pred, **kw).unbind())


# ================================================================================================ FID
FID_MAX_ITERS = 100                        # _sqrtm_newton_schulz(num_iters=100), fid.py:24
FID_EPS = 1e-6                              # _compute_fid(eps=1e-6), fid.py:64


def _fid_feats(name, feats):
    if not torch.is_tensor(feats) or feats.dim() != 2:
        raise AssertionError(f"{name} expects (N, D) feature tensors")
    if feats.shape[0] < 2:
        raise ValueError(f"{name}: at least two feature rows expected, got {feats.shape[0]} (the covariance divides by N - 1; "
                         "the reference returns NaN here)")
    if feats.shape[1] < 1:
        raise ValueError(f"{name}: features of dimension 0")
    if not feats.is_cuda:
        raise RuntimeError(f"{name}: HIP path needs CUDA tensors (no CPU fallback)")
    if feats.dtype != torch.float32:
        raise TypeError(f"{name}: fp32 features expected, got {feats.dtype}")
    return feats.detach().contiguous()


@torch.no_grad()
def fid_statistics(feats):
    """fid.py:135-146 on the float64 copy the reference makes (fid.py:186-187): (mu (D,), sigma (D, D)) in float64 from (N, D) fp32
    CUDA features, mean first, then the product of the centred columns (mtd_fid_stats).  N < 2 raises ValueError."""
    x = _fid_feats("fid_statistics", feats)
    N, D = x.shape
    mu = torch.empty(D, dtype=torch.float64, device=x.device)
    sigma = torch.empty((D, D), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().mtd_fid_stats(x.data_ptr(), N, D, mu.data_ptr(), sigma.data_ptr(), None, K.stream_ptr()), "mtd_fid_stats")
    return mu, sigma


def _fid_solve(mu1, s1, mu2, s2, offset):
    """One solve: (out, iters) on the device -- out = [fid, tr sqrt(S1 S2), last err, finite flag] in float64."""
    D = mu1.numel()
    L = _lib.lib()
    out = torch.empty(4, dtype=torch.float64, device=mu1.device)
    iters = torch.empty(1, dtype=torch.int32, device=mu1.device)
    ws = K.workspace(L.mtd_fid_ws_bytes(D), mu1.device)
    _lib.check(L.mtd_fid_distance(mu1.data_ptr(), s1.data_ptr(), mu2.data_ptr(), s2.data_ptr(), D, offset, FID_MAX_ITERS, out.data_ptr(),
                                  iters.data_ptr(), ws.data_ptr(), K.stream_ptr()), "mtd_fid_distance")
    return out, iters


@torch.no_grad()
def fid_distance64(stats1, stats2):
    """fid.py:64-91 on two (mu, sigma) pairs of fid_statistics: a 0-dim float64 device tensor.  The iteration and its stop run
    on the device; the host reads the result once per solve, for the reference's fallback: if the square root is not finite,
    solve once more with 1e-6 on both diagonals (fid.py:84-88)."""
    (mu1, s1), (mu2, s2) = stats1, stats2
    D = mu1.numel()
    for mu, s in (stats1, stats2):
        if not (mu.is_cuda and s.is_cuda):
            raise RuntimeError("fid_distance64: HIP path needs CUDA tensors (no CPU fallback)")
        if mu.dtype != torch.float64 or s.dtype != torch.float64 or tuple(mu.shape) != (D,) or tuple(s.shape) != (D, D):
            raise AssertionError("fid_distance64 expects two (mu (D,), sigma (D, D)) float64 pairs of one D")
    mu1, s1, mu2, s2 = (t.contiguous() for t in (mu1, s1, mu2, s2))
    out, _ = _fid_solve(mu1, s1, mu2, s2, 0.0)
    if out.tolist()[3] == 0.0:
        print(f"FID calculation produces singular product; adding {FID_EPS} to diagonal of cov estimates")
        out, _ = _fid_solve(mu1, s1, mu2, s2, FID_EPS)
    return out[0]


@torch.no_grad()
def compute_FID(input_feats, target_feats, pred_feats):
    """metrics.py:33-41: (FID(input, target), FID(target, target), FID(pred, target)) as 0-dim float32 device tensors.  The
    target's statistics are computed once and serve all three."""
    st = fid_statistics(target_feats)
    return tuple(fid_distance64(st if f is target_feats else fid_statistics(f), st).float() for f in (input_feats, target_feats, pred_feats))


# ================================================================================================ KID
KID_MMD_ESTS = ("unbiased", "biased", "u-statistic")          # MTD_KID_UNBIASED / _BIASED / _USTAT
KID_PARTS = 21                                                # MTD_KID_PARTS; the names: include/mtdgan_hip.h
KID_MAX_SUBSETS = 65535 // 3                                  # grid z of the tile kernel is 3 * S


def _kid_feats(name, feats):
    if not torch.is_tensor(feats) or feats.dim() != 2:
        raise AssertionError(f"{name} expects (N, D) feature tensors")
    if feats.shape[1] < 1:
        raise ValueError(f"{name}: features of dimension 0")
    if feats.dtype != torch.float32:
        raise TypeError(f"{name}: fp32 features expected, got {feats.dtype}")
    return feats.detach().contiguous()


def kid_draw_subsets(n_pred, n_targ, m, n_subsets):
    """The subsets as kid.py:230-232 draws them, from torch's global CPU generator: per subset first
    torch.randperm(n_pred)[:m], then torch.randperm(n_targ)[:m] -- a caller's seeded generator stays in step with piq.  Two
    (n_subsets, m) int64 CPU tensors.  Where a subset is the whole set, its indices are taken in sorted order (the draw is still
    made): the result then does not depend on the seed, and differs from piq's, which sums the same terms in the drawn order,
    only in rounding."""
    pi, ti = [], []
    for _ in range(n_subsets):
        a = torch.randperm(n_pred)[:m]
        b = torch.randperm(n_targ)[:m]
        pi.append(torch.arange(n_pred) if m == n_pred else a)
        ti.append(torch.arange(n_targ) if m == n_targ else b)
    return torch.stack(pi), torch.stack(ti)


def _kid_plan(n_pred, n_targ, D, degree, gamma, coef0, var_at_m, average, n_subsets, subset_size, ret_var, mmd_est, subsets):
    """Every check of kid_distance64 that needs no device, and the draw: (pred_idx, trgt_idx) int32 CPU tables of shape (S, m) and
    the scalar arguments of mtd_kid.  ValueError before the library is touched."""
    import numbers
    if isinstance(degree, bool) or not isinstance(degree, numbers.Integral) or not 1 <= degree <= 8:
        raise ValueError(f"kid: degree must be an integer in 1..8, got {degree!r}")
    if mmd_est not in KID_MMD_ESTS:
        raise ValueError(f"kid: mmd_est must be one of {KID_MMD_ESTS}, got {mmd_est!r}")
    if subsets is not None:
        if not (isinstance(subsets, (tuple, list)) and len(subsets) == 2):
            raise ValueError("kid: subsets must be a (pred_idx, trgt_idx) pair of (S, m) integer tensors")
        pi, ti = (torch.as_tensor(t) for t in subsets)
        if pi.dim() != 2 or pi.shape != ti.shape or pi.is_floating_point() or ti.is_floating_point() or pi.dtype == torch.bool or ti.dtype == torch.bool:
            raise ValueError("kid: subsets must be a (pred_idx, trgt_idx) pair of (S, m) integer tensors of one shape")
        if pi.is_cuda or ti.is_cuda:
            raise ValueError("kid: subsets are checked on the host: pass CPU tensors (the call itself reads nothing back from the device)")
        S, m = pi.shape
    else:
        S, m = (n_subsets, subset_size) if average else (1, n_pred)
        if isinstance(S, bool) or isinstance(m, bool) or not isinstance(S, numbers.Integral) or not isinstance(m, numbers.Integral):
            raise ValueError(f"kid: n_subsets and subset_size must be integers, got {S!r} and {m!r}")
    if S < 1 or S > KID_MAX_SUBSETS:
        raise ValueError(f"kid: 1 to {KID_MAX_SUBSETS} subsets expected, got {S}")
    if m > n_pred or m > n_targ:
        raise ValueError(f"kid: a subset of {m} rows cannot be drawn from sets of {n_pred} and {n_targ} rows (piq fails an assertion here)")
    if m < 2:
        raise ValueError(f"kid: subsets of at least two rows expected, got {m} (the estimate divides by m - 1)")
    if ret_var and m < 3:
        raise ValueError(f"kid: the variance estimate needs subsets of at least three rows, got {m} (it divides by m - 2)")
    if var_at_m is None:
        var_at_m = min(n_pred, n_targ)
    if isinstance(var_at_m, bool) or not isinstance(var_at_m, numbers.Integral) or (ret_var and var_at_m < 2):
        raise ValueError(f"kid: var_at_m must be an integer of at least 2, got {var_at_m!r}")
    gamma = 1.0 / D if gamma is None else float(gamma)
    if subsets is None:
        pi, ti = kid_draw_subsets(n_pred, n_targ, m, S)
    elif bool((pi < 0).any() or (pi >= n_pred).any() or (ti < 0).any() or (ti >= n_targ).any()):
        raise ValueError("kid: a subset index lies outside its feature set")
    return pi.to(torch.int32).contiguous(), ti.to(torch.int32).contiguous(), dict(
        m=int(m), S=int(S), degree=int(degree), gamma=gamma, coef0=float(coef0), mmd_est=KID_MMD_ESTS.index(mmd_est),
        want_var=1 if ret_var else 0, var_at_m=int(var_at_m))


@torch.no_grad()
def kid_distance64(pred_feats, target_feats, *, degree=3, gamma=None, coef0=1, var_at_m=None, average=False, n_subsets=50, subset_size=1000,
                   ret_var=False, mmd_est="unbiased", subsets=None, parts=False):
    """piq's KID (module/piq/kid.py) of two (N, D) fp32 CUDA feature sets in float64 on the HIP kernels of csrc/kid.hip (mtd_kid;
    DESIGN 3.15): the MMD^2 estimate with the kernel (gamma <x, y> + coef0)^degree, gamma = 1 / D by default, averaged over the
    subsets -- a 0-dim float64 device tensor, with ret_var the pair (score, variance estimate); with parts=True the (S,
    KID_PARTS) float64 table of every named sum of each subset comes last.  No host read inside the call: the index tables go
    host -> device, nothing comes back.

    average=False: one subset of m = N_pred rows of each set; average=True: n_subsets subsets of subset_size rows.  The subsets
    are drawn as piq draws them (kid_draw_subsets), from torch's global CPU generator, so torch.manual_seed(s) before the call
    gives the subsets piq takes after the same seed; `subsets=(pred_idx, trgt_idx)`, two (S, m) integer CPU tensors, overrides
    the draw (and average / n_subsets / subset_size).  Where a subset is the whole set its rows are taken in sorted order, so
    the default call on equally long sets gives the same bits whatever the seed.  var_at_m defaults to min(N_pred, N_targ), as
    piq's class computes it.  mmd_est: piq's "unbiased" (its class's only choice), "biased" or "u-statistic".

    ValueError, before anything is launched: m > N_pred or m > N_targ (piq fails an assertion), m < 2, ret_var with m < 3 (piq
    divides by zero in both), a degree that is not an integer in 1..8, an unknown mmd_est, an index outside its set.
    KID(target, target) is not 0 under the unbiased estimator but a small negative number: piq's value, reproduced."""
    x, y = _kid_feats("kid_distance64", pred_feats), _kid_feats("kid_distance64", target_feats)
    if x.shape[1] != y.shape[1] or x.device != y.device:
        raise AssertionError("kid_distance64 expects two feature sets of one dimension on one device")
    pi, ti, a = _kid_plan(x.shape[0], y.shape[0], x.shape[1], degree, gamma, coef0, var_at_m, average, n_subsets, subset_size, ret_var, mmd_est, subsets)
    if not (x.is_cuda and y.is_cuda):                  # (after the argument checks: those need no device)
        raise RuntimeError("kid_distance64: HIP path needs CUDA tensors (no CPU fallback)")
    L = _lib.lib()
    dev = x.device
    xi, yi = pi.to(dev, non_blocking=True), ti.to(dev, non_blocking=True)
    out = torch.empty(2 + 2 * a["S"], dtype=torch.float64, device=dev)
    table = torch.empty((a["S"], KID_PARTS), dtype=torch.float64, device=dev) if parts else None
    ws = K.workspace(L.mtd_kid_ws_bytes(a["m"], a["S"]), dev)
    _lib.check(L.mtd_kid(x.data_ptr(), x.shape[0], y.data_ptr(), y.shape[0], x.shape[1], xi.data_ptr(), yi.data_ptr(), a["m"], a["S"], a["degree"],
                         a["gamma"], a["coef0"], a["mmd_est"], a["want_var"], a["var_at_m"], out.data_ptr(), table.data_ptr() if parts else None,
                         ws.data_ptr(), K.stream_ptr()), "mtd_kid")
    res = (out[0], out[1]) if ret_var else (out[0],)
    if parts:
        res = res + (table,)
    return res if len(res) > 1 else res[0]


@torch.no_grad()
def compute_KID(input_feats, target_feats, pred_feats, **kw):
    """(KID(input, target), KID(target, target), KID(pred, target)) as 0-dim float32 device tensors, the mirror of compute_FID;
    with ret_var=True three (score, variance) pairs.  **kw: the keyword arguments of kid_distance64 (not `parts`).  Each of the
    three is a call of its own and draws anew, in the order input, gt, pred -- what three piq calls after one seed give; the
    target's subset is NOT shared between them."""
    if kw.get("parts"):
        raise ValueError("compute_KID: `parts` belongs to kid_distance64")
    out = []
    for f in (input_feats, target_feats, pred_feats):
        r = kid_distance64(f, target_feats, **kw)
        out.append(tuple(v.float() for v in r) if isinstance(r, tuple) else r.float())
    return tuple(out)


# ================================================================================================ MSID, IS
MSID_NORMALIZATIONS = ("empty", "complete", "er", "none")
MSID_MODES = ("max", "l2")                                    # MTD_MSID_MAX / MTD_MSID_L2
MSID_MAX_N = 32768                                            # MTD_MSID_MAX_N
MSID_EPSILON, MSID_NORMALIZATION = 1e-6, 1e6                  # msid.py:13-14


def msid_tables(ts, n, k, normalize):
    """What MSID needs from (ts, n, k) alone, by msid.py's own numpy expressions IN THE DTYPE `ts` ARRIVES IN (piq's default ts is
    float32, and the rounding of exp(ts) and sub in that dtype is about 0.1 absolute in the descriptor), widened to float64
    afterwards: (tables (3, len(ts)) = exp(ts) (msid.py:218), sub (:219), the divisor of _normalize_msid (:242-256); c (:389))."""
    import numpy as np
    expts = np.exp(ts)
    sub = -ts * n / np.exp(ts)
    if normalize == "empty":
        div = np.full(ts.shape, n, dtype=np.float64)
    elif normalize == "complete":
        div = 1 + (n - 1) * np.exp(-(1 + 1 / (n - 1)) * ts)
    elif normalize == "er":
        xs = np.linspace(0, 1, n)
        er_spectrum = 4 / np.sqrt(k) * xs + 1 - 2 / np.sqrt(k)
        div = np.exp(-np.outer(ts, er_spectrum)).sum(-1) + MSID_EPSILON
    else:
        div = np.ones(ts.shape, dtype=np.float64)
    c = np.exp(-2 * (ts + 1 / ts))
    return np.stack([np.asarray(v, dtype=np.float64) for v in (expts, sub, div)]), np.asarray(c, dtype=np.float64)


def _msid_ts(ts):
    import numpy as np
    if ts is None:
        return torch.logspace(-1, 1, 256).numpy()                # msid.py:313,338
    ts = ts.detach().cpu().numpy() if torch.is_tensor(ts) else np.asarray(ts)
    if ts.ndim != 1 or ts.size < 1 or ts.size > 65536 or ts.dtype not in (np.float32, np.float64):
        raise ValueError("msid: ts must be a one-dimensional float32 or float64 array of 1..65536 temperatures")
    return ts


def _msid_plan(n, ts, k, m, niters, rademacher, normalized_laplacian, normalize, starting_vectors):
    """Every check of msid_descriptor64 that needs no device, and the draw: (ts as numpy, float64 (n, niters) starting vectors as a
    CPU tensor).  ValueError before the library is touched."""
    import numbers
    import numpy as np
    for name, v, lo, hi in (("k", k, 1, 63), ("m", m, 2, 32), ("niters", niters, 1, 4096)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
            raise ValueError(f"msid: {name} must be an integer in {lo}..{hi}, got {v!r}")
    if normalize is None:
        normalize = "none"
    if normalize not in MSID_NORMALIZATIONS:
        raise ValueError(f"msid: normalize must be one of {MSID_NORMALIZATIONS}, got {normalize!r}")
    if not k + 2 <= n <= MSID_MAX_N:
        raise ValueError(f"msid: a set of {n} rows with k = {k}: k + 2 <= N <= {MSID_MAX_N} expected (piq partitions each row's distances at k + 1)")
    if normalize == "complete" and n < 2:
        raise ValueError("msid: the 'complete' normalisation divides by n - 1")
    ts = _msid_ts(ts)
    if starting_vectors is None:
        sv = np.random.randn(n, int(niters))                     # msid.py:69-73, numpy's global generator
        if rademacher:
            sv = np.sign(sv)
        sv = torch.from_numpy(sv)
    else:
        sv = starting_vectors if torch.is_tensor(starting_vectors) else torch.from_numpy(np.asarray(starting_vectors))
        if sv.dim() != 2 or tuple(sv.shape) != (n, niters) or sv.dtype != torch.float64:
            raise ValueError(f"msid: starting_vectors must be a float64 ({n}, {niters}) array or tensor")
    return ts, normalize, sv


@torch.no_grad()
def msid_descriptor64(feats, *, ts=None, k=5, m=10, niters=100, rademacher=False, normalized_laplacian=True, normalize="empty",
                      starting_vectors=None, parts=False):
    """piq's `_msid_descriptor` (module/piq/msid.py) of one (N, D) fp32 CUDA feature set in float64 on the HIP kernels of
    csrc/msid.hip (mtd_msid_descriptor): the k-nearest-neighbour graph, its Laplacian, m Lanczos steps on niters
    starting vectors at once with piq's reorthogonalisation and breaks, the quadrature, the variance reduction, the
    normalisation, x 1e6 -- a (len(ts),) float64 device tensor.  The feature rows never leave the device and nothing is read
    back inside the call; the starting vectors and the temperature tables go host -> device.

    ts=None: piq's float32 logspace(-1, 1, 256); a float32 or float64 array is used in the dtype it arrives in, as piq does
    (msid_tables).  When `starting_vectors` is omitted they are drawn on the host as np.random.randn(n, niters) (np.sign of it
    under `rademacher`) from numpy's global generator, so np.random.seed(s) before the call gives what piq computes after the
    same seed; a float64 (n, niters) array or tensor overrides the draw.  parts=True: a dict(nbr (N, k + 1) int32: each row's
    k + 1 nearest in rising order, itself included where it is among them; rowptr (N + 1), col (2 N (k + 1), the first rowptr[N]
    valid): the graph's CSR; T (niters, m, m); traces (2, len(ts))) comes second.

    ValueError, before anything is launched: k outside 1..63, m outside 2..32, niters outside 1..4096, N outside k + 2..32768, an
    unknown normalize, a ts or starting_vectors of the wrong shape or dtype."""
    x = _kid_feats("msid_descriptor64", feats)
    ts, normalize, sv = _msid_plan(x.shape[0], ts, k, m, niters, rademacher, normalized_laplacian, normalize, starting_vectors)
    if not x.is_cuda:                                  # (after the argument checks: those need no device)
        raise RuntimeError("msid_descriptor64: HIP path needs CUDA tensors (no CPU fallback)")
    L = _lib.lib()
    dev, (N, D), nts = x.device, x.shape, int(ts.shape[0])
    tables, _ = msid_tables(ts, N, k, normalize)
    import numpy as np
    host = torch.from_numpy(np.concatenate([ts.astype(np.float64), tables.reshape(-1)]))
    tab = host.to(dev, non_blocking=True)
    start = sv.to(dev, non_blocking=True).contiguous()
    nbr = torch.empty((N, k + 1), dtype=torch.int32, device=dev)
    rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
    col = torch.empty(2 * N * (k + 1), dtype=torch.int32, device=dev)
    T = torch.empty((niters, m, m), dtype=torch.float64, device=dev)
    traces = torch.empty((2, nts), dtype=torch.float64, device=dev)
    desc = torch.empty(nts, dtype=torch.float64, device=dev)
    ws = K.workspace(L.mtd_msid_ws_bytes(N, D, k, m, niters, nts), dev)
    _lib.check(L.mtd_msid_descriptor(x.data_ptr(), N, D, k, m, niters, 1 if normalized_laplacian else 0, start.data_ptr(), tab.data_ptr(),
                                     tab[nts:].data_ptr(), nts, nbr.data_ptr(), rowptr.data_ptr(), col.data_ptr(), T.data_ptr(), traces.data_ptr(),
                                     desc.data_ptr(), ws.data_ptr(), K.stream_ptr()), "mtd_msid_descriptor")
    return (desc, dict(nbr=nbr, rowptr=rowptr, col=col, T=T, traces=traces)) if parts else desc


@torch.no_grad()
def msid_distance64(pred_feats, target_feats, *, msid_mode="max", ts=None, k=5, m=10, niters=100, rademacher=False, normalized_laplacian=True,
                    normalize="empty", starting_vectors=None):
    """piq's MSID (module/piq/msid.py) of two (N, D) fp32 CUDA feature sets -- they may differ in N and in D -- as a 0-dim float64
    device tensor: max_t c(t) |d_pred - d_targ| with c = exp(-2 (t + 1 / t)) in 'max' mode, the l2 norm of the difference in 'l2'
    mode, of the two msid_descriptor64.  The starting vectors are drawn for the predicted set first and then for the target, as
    piq does; `starting_vectors=(for_pred, for_targ)` overrides both draws.  Every argument of both sets is checked before
    anything is drawn or launched."""
    if msid_mode not in MSID_MODES:
        raise ValueError(f"msid: msid_mode must be one of {MSID_MODES}, got {msid_mode!r}")
    if starting_vectors is not None and not (isinstance(starting_vectors, (tuple, list)) and len(starting_vectors) == 2):
        raise ValueError("msid: starting_vectors must be a (for_pred, for_targ) pair")
    x, y = _kid_feats("msid_distance64", pred_feats), _kid_feats("msid_distance64", target_feats)
    if x.device != y.device:
        raise AssertionError("msid_distance64 expects two feature sets on one device")
    kw = dict(ts=ts, k=k, m=m, niters=niters, rademacher=rademacher, normalized_laplacian=normalized_laplacian, normalize=normalize)
    svs = []
    for f, sv in zip((x, y), starting_vectors or (None, None)):      # every check, and both draws in piq's order, before the first launch
        ts_np, _, sv = _msid_plan(f.shape[0], ts, k, m, niters, rademacher, normalized_laplacian, normalize, sv)
        svs.append(sv)
    if not (x.is_cuda and y.is_cuda):
        raise RuntimeError("msid_distance64: HIP path needs CUDA tensors (no CPU fallback)")
    dp, dt = (msid_descriptor64(f, starting_vectors=sv, **kw) for f, sv in zip((x, y), svs))
    _, c = msid_tables(ts_np, x.shape[0], k, "none")
    cd = torch.from_numpy(c).to(x.device, non_blocking=True)
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().mtd_msid_distance(dp.data_ptr(), dt.data_ptr(), cd.data_ptr(), dp.shape[0], MSID_MODES.index(msid_mode), out.data_ptr(),
                                            K.stream_ptr()), "mtd_msid_distance")
    return out[0]


@torch.no_grad()
def compute_MSID(input_feats, target_feats, pred_feats, **kw):
    """(MSID(input, target), MSID(target, target), MSID(pred, target)) as 0-dim float32 device tensors, the mirror of compute_KID.
    **kw: the keyword arguments of msid_distance64.  Each of the three is a call of its own and draws anew, in the order input,
    gt, pred -- what three piq calls after one seed give; the target's descriptor is NOT shared between them (piq recomputes it
    with fresh vectors, so MSID(target, target) is not 0)."""
    if "parts" in kw:
        raise ValueError("compute_MSID: `parts` belongs to msid_descriptor64")
    return tuple(msid_distance64(f, target_feats, **kw).float() for f in (input_feats, target_feats, pred_feats))


def _is_plan(n, num_splits):
    import numbers
    if isinstance(num_splits, bool) or not isinstance(num_splits, numbers.Integral) or not 1 <= num_splits <= 65535:
        raise ValueError(f"inception score: num_splits must be an integer in 1..65535, got {num_splits!r}")
    if n // num_splits < 1:
        raise ValueError(f"inception score: {n} rows cannot be cut into {num_splits} splits (piq returns nan from empty slices)")


@torch.no_grad()
def inception_score64(feats, num_splits=10):
    """piq's `inception_score` (module/piq/isc.py) of (N, D) fp32 CUDA rows in float64 on the HIP kernel of csrc/msid.hip
    (mtd_inception_score): the rows' softmax, per split of N // num_splits consecutive rows (the remainder is dropped)
    exp(mean KL(p(y|x) || p(y))); (mean, unbiased standard deviation) of the split scores as 0-dim float64 device tensors.  With one
    split the standard deviation is nan, as piq's.  ValueError, before anything is launched: num_splits < 1 or N // num_splits < 1."""
    x = _kid_feats("inception_score64", feats)
    _is_plan(x.shape[0], num_splits)
    if not x.is_cuda:
        raise RuntimeError("inception_score64: HIP path needs CUDA tensors (no CPU fallback)")
    L = _lib.lib()
    out = torch.empty(2 + num_splits, dtype=torch.float64, device=x.device)
    ws = K.workspace(L.mtd_is_ws_bytes(x.shape[0], x.shape[1], num_splits), x.device)
    _lib.check(L.mtd_inception_score(x.data_ptr(), x.shape[0], x.shape[1], num_splits, out.data_ptr(), ws.data_ptr(), K.stream_ptr()), "mtd_inception_score")
    return out[0], out[1]


@torch.no_grad()
def is_distance64(pred_feats, target_feats, num_splits=10, distance="l1"):
    """piq's IS (isc.py:58-104): the l1 or l2 distance between the two sets' Inception Scores (of two scalars: |a - b| either
    way), a 0-dim float64 device tensor."""
    if distance not in ("l1", "l2"):
        raise ValueError("Distance should be one of {`l1`, `l2`}")
    x, y = _kid_feats("is_distance64", pred_feats), _kid_feats("is_distance64", target_feats)
    _is_plan(x.shape[0], num_splits)
    _is_plan(y.shape[0], num_splits)
    if not (x.is_cuda and y.is_cuda):
        raise RuntimeError("is_distance64: HIP path needs CUDA tensors (no CPU fallback)")
    return (inception_score64(x, num_splits)[0] - inception_score64(y, num_splits)[0]).abs()


@torch.no_grad()
def compute_IS(input_feats, target_feats, pred_feats, **kw):
    """(IS(input, target), IS(target, target), IS(pred, target)) as 0-dim float32 device tensors; **kw: num_splits, distance.
    piq's inception_score expects raw InceptionV3 logits, whose softmax is p(y|x); what the rows are is the extractor's business:
    InceptionV3Features here stops at pool3, so with it the score is that of the softmax over the 2048 pooled features."""
    return tuple(is_distance64(f, target_feats, **kw).float() for f in (input_feats, target_feats, pred_feats))


@torch.no_grad()
def compute_feat(input, target, pred, device=None, *, extractor):
    """metrics.py:17-31 with the feature network handed over: `extractor` is InceptionV3Features(state_dict) (the reference: piq's
    InceptionV3; the checkpoint is the caller's) or any callable on a (B, 3, H, W) batch, which runs in whatever the caller built
    it from.  It is applied to x.repeat(1, 3, 1, 1) of each image set -- to x itself where the extractor says
    `takes_single_channel = True`, as InceptionV3Features does (its first layer is folded to one input channel) -- and returns a
    tensor, or a list / tuple of exactly one; the result is flattened to (B, D).  `device` is accepted for the reference's
    signature; the tensors' device is used."""
    if not callable(extractor):
        raise TypeError("compute_feat: pass the feature network as extractor=<callable> (no feature network ships with this package)")
    if not (input.shape == target.shape and target.shape == pred.shape):
        raise AssertionError("compute_feat expects three tensors of the same shape")
    single = getattr(extractor, "takes_single_channel", False) is True
    feats = []
    for x in (input, target, pred):
        f = extractor(x if single else x.repeat(1, 3, 1, 1))
        if isinstance(f, (list, tuple)):
            if len(f) != 1:
                raise AssertionError(f"feature_encoder must return list with features from one layer. Got {len(f)}")
            f = f[0]
        feats.append(f.flatten(1))
    return tuple(feats)
