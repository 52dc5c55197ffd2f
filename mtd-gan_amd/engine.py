"""Mirror of the reference's step engine for MTD-GAN: engine.train_MTD_GAN_Ours (engine.py:26-76).

Same 9 positional arguments and the same returned dict {meter name: round(global average, 7)}.  The body
of one iteration is `train_iteration` (D step with PCGrad, then G step); the reference performs ~25 host
synchronisations per iteration (16 `.item()` in MetricLogger.update plus 9 `if dot < 0` in PCGrad), this
one gathers the 17 logged scalars into one device vector and copies it to the host once per iteration."""
from . import _options
import collections
import functools
import os

import torch


def train_iteration(model, x, y, optimizer_G, optimizer_D, method_D, dp=None):
    """engine.py:38-55.  Returns (names, device tensor of the logged values)."""
    D, G = model.Discriminator, model.Generator
    # ---- Discriminator
    optimizer_D.zero_grad()
    D.zero_grad()
    d_losses, d_details = model.d_loss(x, y)
    if method_D is not None:
        method_D.backward(losses=d_losses, shared_parameters=list(D.shared_parameters()),
                          task_specific_parameters=list(D.task_specific_parameters()),
                          last_shared_parameters=list(D.last_shared_parameters()))
    else:
        d_losses.backward()                 # engine.py:56-63: the ablation wrappers return one scalar
        if dp is not None:
            dp.all_reduce_avg_list([p.grad for p in D.parameters() if p.grad is not None])
    if d_losses.is_cuda:
        from .train_step import d_optimizer_step
        d_optimizer_step(D, optimizer_D, dp)         # FusedAdamW on one GPU: the update's launch writes the 3x3 weights' views too
    else:
        optimizer_D.step()
    # ---- Generator
    optimizer_G.zero_grad()
    G.zero_grad()
    g_loss, g_details = model.g_loss(x, y)
    g_loss.backward()
    if dp is not None:
        _all_reduce_generator_grads(model, G, dp)
    optimizer_G.step()
    if d_losses.is_cuda:
        from . import discriminator_path
        discriminator_path.settle_tail(d_losses.device)      # (joined by the G step's discriminator pass already, unless that pass never ran)
    names = ["d_loss"] + list(d_details.keys()) + ["g_loss"] + list(g_details.keys())
    if d_losses.is_cuda:
        from . import kernels as K
        one = lambda t: (t.detach().reshape(-1).float().contiguous(), None)
        vals = K.scalar_sums([one(d_losses)] + [one(v) for v in d_details.values()] + [one(g_loss)] + [one(v) for v in g_details.values()],
                             d_losses.device)     # the 17 logged values in one launch (d_loss = the sum of the stacked task losses)
    else:       # (host tensors: the loop's own CPU tests drive it with stand-in models; the networks themselves refuse CPU tensors)
        vals = torch.stack([d_losses.detach().sum()] + [v.detach().reshape(()) for v in d_details.values()] + [g_loss.detach().reshape(())]
                           + [v.detach().reshape(()) for v in g_details.values()])
    return names, vals


def _all_reduce_generator_grads(model, G, dp):
    """The generator's gradients across ranks: one in-place collective on the flat buffer they are views of
    (train_step._GStepFn.backward), on the RCCL side stream; the generic bucket-and-scatter route for anything else."""
    flat = getattr(model, "_ggrad_flat", None)
    grads = [p.grad for p in G.parameters()]
    if flat is not None and all(g is not None and g.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() for g in grads):
        if hasattr(dp, "all_reduce_avg_inline"):
            dp.all_reduce_avg_inline(flat)          # on the current stream: the optimizer launch that follows needs it at once
        else:
            dp.all_reduce_avg(flat)
            dp.wait()
    else:
        dp.all_reduce_avg_list(grads)


class _Meter:
    def __init__(self):
        self.total, self.count = 0.0, 0

    def update(self, value, n):
        self.total += value * n
        self.count += n

    @property
    def global_avg(self):
        return self.total / self.count


_gc_frozen = [False]


def freeze_long_lived_objects(force=False):
    """Collect, then move everything alive (modules, parameter tables, cached descriptors, the interpreter's own ~1e6 objects)
    to the garbage collector's permanent generation.  A full collection otherwise walks all of them every ~160 eager
    iterations -- 90-120 ms on the host (tools/hiccup_probe.py), three iterations' worth of GPU work.  Nothing is leaked that
    would have been freed: reference counting still frees frozen objects; only cycles among them are never looked for again.
    This changes PROCESS-WIDE interpreter state, so a library entry point does it only when asked: `MTD_GC_FREEZE=1` in the
    environment (train_MTD_GAN_Ours then calls it before its first iteration) or an explicit call with force=True (bench.py's
    workloads do, and say so in their line).  Once per process."""
    if _gc_frozen[0] or not (force or _options.product("MTD_GC_FREEZE", "0") == "1"):
        return
    import gc
    gc.collect()
    gc.freeze()
    _gc_frozen[0] = True


class LoggedScalars:
    """The iteration's ONE device -> host copy, taken off the host's critical path: the 17 logged values go to a pinned
    buffer with an asynchronous copy and are read one iteration later (or at once when a line is due to be printed), so the
    host keeps enqueuing the next iteration instead of waiting for this one to finish on the GPU.  The reference's
    MetricLogger.update calls `.item()` 16 times per iteration (utils.py:60-65)."""

    def __init__(self, meters, batch_size):
        self.meters, self.batch_size, self.pending = meters, batch_size, None
        self._ring, self._turn = [None, None], 0       # two pinned buffers, used in turn (one is pending while the other fills)

    def push(self, names, vals, lr):
        if vals.is_cuda:
            self._turn ^= 1
            host = self._ring[self._turn]
            if host is None or host.shape != vals.shape or host.dtype != vals.dtype:
                host = self._ring[self._turn] = torch.empty(vals.shape, dtype=vals.dtype, pin_memory=True)
            host.copy_(vals, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        else:
            host, ev = vals, None
        self.drain()
        self.pending = (names, host, ev, lr)

    def drain(self):
        if self.pending is None:
            return
        names, host, ev, lr = self.pending
        self.pending = None
        if ev is not None:
            ev.synchronize()
        for k, v in zip(names, host.tolist()):
            self.meters.setdefault(k, _Meter()).update(v, self.batch_size)
        self.meters.setdefault("lr", _Meter()).update(lr, self.batch_size)


def train_MTD_GAN_Ours(model, data_loader, optimizer_G, optimizer_D, device, epoch, print_freq, batch_size, method_D, dp=None):
    """`dp`: optional data-parallel hook (parallel.DataParallelSync).  With PCGrad it defaults to the hook attached to the
    weight method (method_D.method.dp); the ablation wrappers' path (method_D=None) has no weight method to carry it, so a
    multi-process run passes it here -- and a process group of more than one rank without a hook is refused rather than
    left to train unsynchronised replicas."""
    model.Generator.train(True)
    model.Discriminator.train(True)
    if method_D is None and type(model).__name__ == "MTD_GAN_Method":
        raise NotImplementedError("the reference's method_D=None branch calls .backward() on MTD_GAN_Method's 3-vector and raises; "
                                  "use WeightMethods('pcgrad') (method_D=None is the ablation wrappers' path)")
    meters = {}
    if dp is None:
        dp = getattr(getattr(method_D, "method", None), "dp", None)
    if dp is None and torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise RuntimeError("train_MTD_GAN_Ours: torch.distributed is initialised with more than one rank but no data-parallel hook was "
                           "given (pass dp=parallel.DataParallelSync(device), or attach it to the weight method): the ranks would "
                           "train unsynchronised replicas")
    n_it = len(data_loader)
    freeze_long_lived_objects()
    logged = LoggedScalars(meters, batch_size)
    from .train_step import recorded_iteration
    for it, batch_data in enumerate(data_loader):
        x = batch_data["n_20"].to(device).float()
        y = batch_data["n_100"].to(device).float()
        # (a recorded launch list replays the iteration from its third occurrence on where that applies -- train_step.
        # RecordedTrainStep: same launches, none of the Python around them; MTD_LIST=0 keeps every iteration eager)
        names, vals = recorded_iteration(model, x, y, optimizer_G, optimizer_D, method_D, dp)
        logged.push(names, vals, optimizer_G.param_groups[0]["lr"])
        if print_freq and (it % print_freq == 0 or it == n_it - 1):
            logged.drain()                            # a printed line shows this iteration, as the reference's does
            print(f"Train: [epoch:{epoch}] [{it}/{n_it}] " + "  ".join(f"{k}: {m.global_avg:.4f}" for k, m in meters.items()), flush=True)
    logged.drain()
    order = ["lr"] + [k for k in meters if k != "lr"]
    return {k: round(meters[k].global_avg, 7) for k in order}


# ================================================================================================ evaluation loops
def _l1(loss, pred, target):
    """The reference passes nn.L1Loss; its mean runs as one loss-term launch.  Any other callable is applied as given."""
    from . import kernels as K
    if isinstance(loss, torch.nn.L1Loss) and loss.reduction == "mean":
        p, t = pred.contiguous(), target.contiguous()
        return K.loss_terms([K.make_term(1, p, t, scale=1.0 / p.numel())], p.device)[0]
    return loss(pred, target)


def _save_png(path, img):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:                      # PNG dumps are cosmetic; the metrics do not depend on them
        return
    plt.imsave(path, img.squeeze().cpu().numpy(), cmap="gray")


@torch.no_grad()
def valid_MTD_GAN_Ours(model, loss, data_loader, device, epoch, save_dir, print_freq):
    """Mirror of engine.py:78-106: whole-slice generator inference + L1 loss; returns {'L1_loss': global average}.
    Slices may be 64, 128, 256 or 512 pixels square (the reference validates on 512 x 512); with
    `model.Generator.allow_any_size = True`, any H x W with 16 <= H, W <= 512 (cropped slices, other matrix sizes).
    `model.Generator.activation_dtype = torch.float16` runs the 128 / 256 / 512 squares with binary16 activation storage
    (fp32 arithmetic, input and output; PSNR within 1e-4 dB of the fp32 pass); nothing here changes for it.
    `model.Generator.sliding_window = dict(roi_size=(64, 64), sw_batch_size=..., overlap=..., mode=...)` evaluates each slice
    window by window instead (the reference's sliding_window_inference calls, engine.py:345): the generator then
    runs on the 64 x 64 maps it was trained on, and REDCNN_Generator-based models can be evaluated on slices at all."""
    model.Generator.eval()
    model.Discriminator.eval()
    m = _Meter()
    n_it = len(data_loader)
    last = None
    for it, batch_data in enumerate(data_loader):
        x = batch_data["n_20"].to(device).float()
        y = batch_data["n_100"].to(device).float()
        pred = model.Generator(x)
        m.update(float(_l1(loss, pred, y)), 1)
        last = (x, y, pred)
        if print_freq and (it % print_freq == 0 or it == n_it - 1):
            print(f"Valid: [epoch:{epoch}] [{it}/{n_it}] L1_loss: {m.global_avg:.6f}", flush=True)
    if save_dir and last is not None:
        import os
        os.makedirs(save_dir, exist_ok=True)
        for tag, t in zip(("input_n_20", "gt_n_100", "pred_n_100"), last):
            _save_png(os.path.join(save_dir, f"epoch_{epoch}_{tag}.png"), t[0])
    return {"L1_loss": round(m.global_avg, 7)}


def _l1_each(loss, pred, target):
    """_l1 of every slice: B device values.  nn.L1Loss's mean is one loss-term launch of B terms, each the one-slice term."""
    from . import kernels as K
    B = pred.shape[0]
    if isinstance(loss, torch.nn.L1Loss) and loss.reduction == "mean":
        p, t = pred.contiguous(), target.contiguous()
        return K.loss_terms([K.make_term(1, p[i], t[i], scale=1.0 / p[i].numel()) for i in range(B)], p.device)
    return torch.stack([torch.as_tensor(loss(pred[i:i + 1], target[i:i + 1]), device=pred.device).reshape(()) for i in range(B)])


def _update_triple(meters, name, triple):
    """One sample's (input, gt, pred) values into the meters {input,gt,pred}_<name>, made in that order where they are new."""
    for who, v in zip(("input", "gt", "pred"), triple):
        meters.setdefault(f"{who}_{name}", _Meter()).update(v, 1)


def _feature_metric_option(model, attr, what, call):
    """An opt-in metric of the FID feature rows: absent or falsy -> None; True -> {} (the defaults of metrics.<call>); a dict -> its
    keyword arguments (not `parts`).  It needs `model.fid_features`, whose feature rows it is computed from.  Anything else:
    ValueError, before anything runs on the device."""
    cfg = getattr(model, attr, None)
    if not cfg:
        return None
    if cfg is not True and not (isinstance(cfg, dict) and all(isinstance(k, str) for k in cfg) and "parts" not in cfg):
        raise ValueError(f"model.{attr}: True or a dict of metrics.{call}'s keyword arguments (without `parts`); got {cfg!r}")
    if getattr(model, "fid_features", None) is None:
        raise ValueError(f"model.{attr} needs model.fid_features: {what} is computed from the feature rows of that extractor")
    return {} if cfg is True else dict(cfg)


def _kid_option(model):
    """`model.test_kid` of test_MTD_GAN_Ours (metrics.kid_distance64's keyword arguments): _feature_metric_option."""
    return _feature_metric_option(model, "test_kid", "KID", "kid_distance64")


def _msid_option(model):
    """`model.test_msid` of test_MTD_GAN_Ours (metrics.msid_distance64's keyword arguments): _feature_metric_option."""
    return _feature_metric_option(model, "test_msid", "MSID", "msid_distance64")


def _is_option(model):
    """`model.test_is` of test_MTD_GAN_Ours (metrics.is_distance64's num_splits, distance): _feature_metric_option."""
    return _feature_metric_option(model, "test_is", "the Inception Score", "is_distance64")


# ---------------------------------------------------------------------- the opt-in per-slice metrics of test_MTD_GAN_Ours
# One entry of _PER_SLICE per metric; the table's order is the order of the meter keys, the CSV columns and the blocks of the
# per-slice host read.
#   attr     the `model.test_*` attribute that switches the metric on
#   parse    parse(model, entry) -> the keyword arguments of `each`, or None where the attribute is absent or off; ValueError for
#            any other value, before anything runs on the device
#   each     the name of metrics.<each>(input, target, pred, **keywords) -> a (3, B) float64 device tensor, rows input, gt, pred
#            (looked up when used: metrics is imported lazily) -- or (names, 3, B) with several result names, of which the
#            keyword `which` holds those chosen
#   columns  result name -> CSV column label; the meters are {input,gt,pred}_<name>
#   text     the entry's part of parse's error message
# Two keyword names are the loop's own, so no `each` may use them for anything else: `which` (a tuple of result names: the names
# chosen of an entry with several, _names) and `weights` (a tensor the loop moves to the device once, _test_loop).
_PerSlice = collections.namedtuple("_PerSlice", "attr parse each columns text")


def _iqa_parse(model, e):
    """absent or falsy -> None; True -> all of metrics.IQA_METRICS; a tuple of names from it -> those, in the order of
    metrics.IQA_METRICS whatever the tuple's."""
    from . import metrics as M
    cfg = getattr(model, e.attr, None)
    if not cfg:
        return None
    try:
        if cfg is not True and not isinstance(cfg, (tuple, list)):
            raise ValueError("not a tuple")
        return dict(which=M.IQA_METRICS if cfg is True else M._iqa_which(cfg))
    except ValueError:
        raise ValueError(f"model.{e.attr}: {e.text} {M.IQA_METRICS}; got {cfg!r}") from None


def _checked_parse(model, e):
    """absent or falsy -> None; True -> {} (the defaults of metrics.X_each); a dict with keys from metrics.X_OPTIONS that
    metrics.X_check_options accepts -> those keyword arguments (X: `each` without its `_each`)."""
    from . import metrics as M
    cfg = getattr(model, e.attr, None)
    if not cfg:
        return None
    if cfg is True:
        return {}
    stem = e.each[:-len("_each")]
    try:
        if not isinstance(cfg, dict) or set(cfg) - set(getattr(M, f"{stem.upper()}_OPTIONS")):
            raise ValueError("not a dict of the options")
        getattr(M, f"{stem}_check_options")(**cfg)
    except ValueError as err:
        raise ValueError(f"model.{e.attr}: True or a dict with the keys {e.text}; got {cfg!r} ({err})") from None
    return dict(cfg)


def _vgg16_parse(model, e, form=lambda e, cfg: (cfg, {})):
    """A metric on `model.perceptual_vgg16` with weights of the caller's: absent, None, False or empty -> None; the weights in a
    form metrics.X_weights takes -> the keyword arguments vgg and weights (the float64 table).  form(entry, value) -> (weights,
    further keyword arguments) opens a wrapped value."""
    from . import metrics as M
    cfg = getattr(model, e.attr, None)
    if cfg is None or cfg is False or (isinstance(cfg, (dict, list, tuple, str)) and not cfg):
        return None
    cfg, more = form(e, cfg)
    if cfg is True:
        raise ValueError(f"model.{e.attr}: no weights ship with this package; pass {e.text}")
    try:
        table = getattr(M, e.each[:-len("_each")] + "_weights")(cfg)
    except (ValueError, OSError) as err:
        raise ValueError(f"model.{e.attr}: {err}") from None
    vgg = getattr(model, "perceptual_vgg16", None)
    if not isinstance(vgg, M.VGG16Features):
        label, = e.columns.values()
        raise ValueError(f"model.{e.attr} needs model.perceptual_vgg16 = metrics.VGG16Features(state_dict): {label} is computed on its maps")
    return dict(vgg=vgg, weights=table, **more)


def _lpips_form(e, cfg):
    """`model.test_lpips`: the weights, or `dict(weights=..., distance="mse" | "mae")` -> (weights, dict(distance=...))."""
    from . import metrics as M
    distance = "mse"
    if isinstance(cfg, dict):
        if set(cfg) - {"weights", "distance"} or "weights" not in cfg:
            raise ValueError(f"model.{e.attr}: the weights, or a dict with the keys weights and distance; got the keys {sorted(cfg)}")
        cfg, distance = cfg["weights"], cfg.get("distance", "mse")
    if distance not in M.LPIPS_DISTANCES:
        raise ValueError(f"model.{e.attr}: distance must be one of {M.LPIPS_DISTANCES}, got {distance!r}")
    return cfg, dict(distance=distance)


def _brisque_parse(model, e):
    """`model.test_brisque`: absent, None, False or empty -> None; the support vector regression in a form metrics.brisque_weights
    takes, or `dict(weights=..., kernel_size=..., kernel_sigma=...)` -> the keyword arguments of metrics.brisque_each, the float64
    table under `weights`.  True: ValueError, no weights ship with this package."""
    from . import metrics as M
    cfg = getattr(model, e.attr, None)
    if cfg is None or cfg is False or (isinstance(cfg, (dict, list, tuple, str)) and not cfg):
        return None
    more = {}
    if isinstance(cfg, dict):
        if set(cfg) - {"weights", *M.BRISQUE_OPTIONS} or "weights" not in cfg:
            raise ValueError(f"model.{e.attr}: the weights, or a dict with the keys weights, {', '.join(M.BRISQUE_OPTIONS)}; got the keys {sorted(cfg)}")
        more = {k: v for k, v in cfg.items() if k != "weights"}
        cfg = cfg["weights"]
    if cfg is True:
        raise ValueError(f"model.{e.attr}: no weights ship with this package; pass {e.text}")
    try:
        M.brisque_check_options(**more)
        table = M.brisque_weights(cfg)
    except (ValueError, OSError) as err:
        raise ValueError(f"model.{e.attr}: {err}") from None
    return dict(weights=table, **more)


_PER_SLICE = (
    _PerSlice("test_iqa", _iqa_parse, "iqa_metrics_each", {"ms_ssim": "MS_SSIM", "vif": "VIF", "gmsd": "GMSD"}, "True or a tuple of names from"),
    _PerSlice("test_haarpsi", _checked_parse, "haarpsi_each", {"haarpsi": "HaarPSI"}, "c, alpha (positive numbers), subsample (a bool)"),
    _PerSlice("test_fsim", _checked_parse, "fsim_each", {"fsim": "FSIM"},
              "scales (1..4), orientations (1..8), min_length, mult, sigma_f, delta_theta (positive numbers, sigma_f not 1), k (a number)"),
    _PerSlice("test_lpips", functools.partial(_vgg16_parse, form=_lpips_form), "lpips_each", {"lpips": "LPIPS"}, "LPIPS's five linear-layer weight tensors or a path to them"),
    _PerSlice("test_dists", _vgg16_parse, "dists_each", {"dists": "DISTS"}, "DISTS's dict of alpha and beta or a path to it"),
    _PerSlice("test_vsi", _checked_parse, "vsi_each", {"vsi": "VSI"},
              "c1, c2, c3, omega_0, sigma_f, sigma_d, sigma_c (positive numbers), alpha, beta (numbers)"),
    _PerSlice("test_mdsi", _checked_parse, "mdsi_each", {"mdsi": "MDSI"},
              "c1, c2, c3, rho (positive numbers), combination ('sum' or 'mult'), alpha, beta, gamma, q, o (numbers)"),
    _PerSlice("test_brisque", _brisque_parse, "brisque_each", {"brisque": "BRISQUE"}, "BRISQUE's (sv_coef, sv) pair or a path to it"),
    _PerSlice("test_tv", _checked_parse, "tv_each", {"tv": "TV"}, "norm_type ('l1', 'l2' or 'l2_squared')"),
)


def _per_slice_options(model):
    """The (entry, keyword arguments) pairs of the entries of _PER_SLICE that the model switches on, in the table's order."""
    return [(e, kw) for e in _PER_SLICE for kw in (e.parse(model, e),) if kw is not None]


def _names(e, kw):
    """The result names of an active entry: those chosen by `which`, or the entry's one."""
    return kw.get("which", tuple(e.columns))


def _table_option(attr, model):
    """One attribute's parse alone: `model.<attr>` -> the keyword arguments or None."""
    e, = (e for e in _PER_SLICE if e.attr == attr)
    return e.parse(model, e)


_haarpsi_option, _fsim_option, _lpips_option, _dists_option, _vsi_option, _mdsi_option = (
    functools.partial(_table_option, attr) for attr in ("test_haarpsi", "test_fsim", "test_lpips", "test_dists", "test_vsi", "test_mdsi"))


def _iqa_option(model):
    """`model.test_iqa` as the tuple of chosen names, or None."""
    kw = _table_option("test_iqa", model)
    return kw and kw["which"]


def _test_batch_per_slice(loss, batch_data, x, y, pred, vgg, fid_features, feats, meters, rows, active=()):
    """One loader batch of test_MTD_GAN_Ours under `model.test_per_slice`: B meter updates and B rows from one host read.
    active: _per_slice_options' pairs."""
    from . import kernels as K, metrics as M
    B, _, H, W = x.shape
    clipped = K.clip01(pred.contiguous())
    parts = [_l1_each(loss, pred, y).double().flatten(), M.pixel_metrics_each(x, y, clipped).flatten()]
    if vgg is not None:
        parts.append(M.perceptual_metrics_per_slice(x, y, clipped, vgg).double().flatten())
    if fid_features is not None:
        for rows_, f in zip(feats, M.compute_feat(x, y, clipped, extractor=fid_features)):
            rows_.append(f.float())
    for e, kw in active:                              # (name, who, slice) float64 each, behind the others in the table's order
        parts.append(getattr(M, e.each)(x, y, clipped, **kw).flatten())
    vals = torch.cat(parts).tolist()                  # every per-slice value of the batch in one device -> host copy
    l1 = vals[:B]
    sums = [[vals[B + (k * B + i) * 2:B + (k * B + i) * 2 + 2] for i in range(B)] for k in range(3)]
    six = [vals[7 * B + r * B:7 * B + (r + 1) * B] for r in range(6)] if vgg is not None else None
    pm = M._slice_triples(sums, H * W)
    paths = batch_data.get("path_n_20") if isinstance(batch_data, dict) else None
    for i in range(B):
        meters.setdefault("L1_loss", _Meter()).update(l1[i], 1)
        perceptual = ()
        if six is not None:
            for j, name in enumerate(("pl", "tml")):
                _update_triple(meters, name, [six[3 * j + k][i] for k in range(3)])
            perceptual = (six[2][i], six[5][i])
        for name in ("rmse", "psnr", "ssim"):
            _update_triple(meters, name, pm[name][i])
        more = ()
        q = (13 if vgg is not None else 7) * B        # where the table's blocks start: each name's is 3 B values, who-major
        for e, kw in active:
            for name in _names(e, kw):
                triple = vals[q + i:q + 3 * B:B]
                _update_triple(meters, name, triple)
                more += (triple[2],)
                q += 3 * B
        path = paths[i] if paths is not None else f"slice_{len(rows)}"
        rows.append((path,) + perceptual + (pm["rmse"][i][2], pm["psnr"][i][2], pm["ssim"][i][2]) + more)


class _PngSink:
    """`model.test_save_png` of test_MTD_GAN_Ours: per loader batch one scanline launch on the 3B stacked images (x, y and the RAW
    prediction, as engine.py:157-159 saves them), one asynchronous copy of the bytes into pinned host memory, and -- once the
    batch's metrics have been read, which the loop waits for anyway -- three writer submits per slice."""

    def __init__(self, save_dir, depth, level, threads):
        from . import image_io
        os.makedirs(save_dir, exist_ok=True)
        self.save_dir, self.depth = save_dir, depth
        self.writer = image_io.PngWriter(threads, level)

    @classmethod
    def from_model(cls, model, save_dir):
        """Absent or falsy -> None; True -> depth 8, zlib level 6, image_io.default_threads(); or a dict of those three."""
        cfg = getattr(model, "test_save_png", None)
        if not cfg:
            return None
        cfg = {} if cfg is True else cfg
        if not isinstance(cfg, dict) or set(cfg) - {"depth", "level", "threads"}:
            raise ValueError(f"model.test_save_png: True or a dict with the keys depth, level, threads; got {cfg!r}")
        depth = cfg.get("depth", 8)
        if depth not in (8, 16):
            raise ValueError(f"model.test_save_png: depth must be 8 or 16, got {depth!r}")
        if not save_dir:
            raise ValueError("model.test_save_png is set but test_MTD_GAN_Ours was given no save_dir to write the images to")
        return cls(save_dir, depth, cfg.get("level", 6), cfg.get("threads"))

    def begin(self, x, y, pred):
        from . import image_io
        B, C, H, W = x.shape
        if C != 1 or y.shape != x.shape or pred.shape != x.shape:
            raise ValueError(f"test_save_png: expected single-channel x, y and prediction of one shape, got {tuple(x.shape)}, "
                             f"{tuple(y.shape)}, {tuple(pred.shape)}")
        rows = image_io.gray_png_rows(torch.cat([x, y, pred]).reshape(3 * B, H, W), self.depth)
        host = torch.empty(rows.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(rows, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return host, ev, (B, H, W)

    def submit(self, images, batch_data, k0):
        """k0: slices before this batch (the `slice_{k}` names of batches without paths, counted as the CSV counts)."""
        from . import image_io
        host, ev, (B, H, W) = images
        ev.synchronize()
        p20 = batch_data.get("path_n_20") if isinstance(batch_data, dict) else None
        p100 = batch_data.get("path_n_100") if isinstance(batch_data, dict) else None
        planes = host.numpy()          # (views of the pinned buffer: they keep it alive until the workers are done with it)
        for i in range(B):
            names = image_io.png_names(p20[i] if p20 is not None else None, p100[i] if p100 is not None else None, k0 + i)
            for which, name in enumerate(names):
                self.writer.submit(os.path.join(self.save_dir, name), planes[which * B + i], H, W, self.depth)


class _StoredInput:
    """`model.test_from_stored` of test_MTD_GAN_Ours: the loader's batches hold the stored pixel values of the DICOM files and one
    (slope, intercept) pair per slice, and one fused launch per dose level windows them (dicom_io.stored_to_window)."""

    def __init__(self, a_min, a_max):
        self.a_min, self.a_max = a_min, a_max

    @classmethod
    def from_model(cls, model):
        """Absent or falsy -> None; True -> the training window [-160, 240]; or a dict with a_min and / or a_max."""
        from . import dicom_io
        cfg = getattr(model, "test_from_stored", None)
        if not cfg:
            return None
        cfg = {} if cfg is True else cfg
        if not isinstance(cfg, dict) or set(cfg) - {"a_min", "a_max"}:
            raise ValueError(f"model.test_from_stored: True or a dict with the keys a_min, a_max; got {cfg!r}")
        a_min, a_max = float(cfg.get("a_min", dicom_io.A_MIN)), float(cfg.get("a_max", dicom_io.A_MAX))
        if not a_max > a_min:
            raise ValueError(f"model.test_from_stored: a_max must exceed a_min, got {a_min!r}, {a_max!r}")
        return cls(a_min, a_max)

    def window(self, batch_data, key, device):
        """-> (windowed float32 (B, 1, H, W), the stored words on the device, their (B, 2) rescale table on the device)"""
        from . import dicom_io
        name = "rescale_" + key
        if not isinstance(batch_data, dict) or name not in batch_data:
            raise ValueError(f"model.test_from_stored: the batch carries no '{name}', the (B, 2) (slope, intercept) pairs of '{key}'")
        words = batch_data[key]
        if not isinstance(words, torch.Tensor) or words.dtype not in (torch.int16, torch.uint16) or words.dim() != 4 or words.shape[1] != 1:
            raise ValueError(f"model.test_from_stored: batch['{key}'] must be an int16 or uint16 tensor (B, 1, H, W) of stored pixel "
                             f"values, got {getattr(words, 'dtype', type(words))} {tuple(getattr(words, 'shape', ()))}")
        words = words.to(device).contiguous()
        table = dicom_io.rescale_table(batch_data[name], words.shape[0], words.device)
        return dicom_io.stored_to_window(words, table, self.a_min, self.a_max), words, table


class _DcmSink:
    """`model.test_save_dcm` of test_MTD_GAN_Ours: per loader batch one launch takes the RAW prediction back to stored pixel
    values (dicom_io.window_to_stored: clipped, the reference's truncation, the input's own word where the input lies outside
    the window), one asynchronous copy brings the int16 slices to pinned host memory, and -- once the batch's metrics have been
    read -- the callable gets one call per slice."""

    def __init__(self, write, stored):
        self.write, self.stored = write, stored

    @classmethod
    def from_model(cls, model, stored):
        """Absent or falsy -> None; else a callable(path_n_20, stored_int16_2d_numpy, k).  stored: the _StoredInput, or None."""
        cfg = getattr(model, "test_save_dcm", None)
        if not cfg:
            return None
        if not callable(cfg):
            raise ValueError(f"model.test_save_dcm: a callable(path_n_20, stored_int16_2d, k), e.g. dicom_io.pydicom_writer(dcm_dir); got {cfg!r}")
        if stored is None:
            raise ValueError("model.test_save_dcm needs model.test_from_stored: the way back to stored pixel values takes the "
                             "(slope, intercept) pairs and the stored input of every slice")
        return cls(cfg, stored)

    def begin(self, pred, words, table):
        from . import dicom_io
        out = dicom_io.window_to_stored(pred.float(), table, self.stored.a_min, self.stored.a_max, clip=True, rounding="trunc",
                                        outside="input", reference=words)
        host = torch.empty(out.shape, dtype=torch.int16, pin_memory=True)
        host.copy_(out, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return host, ev

    def submit(self, slices, batch_data, k0):
        host, ev = slices
        ev.synchronize()
        paths = batch_data.get("path_n_20") if isinstance(batch_data, dict) else None
        planes = host.numpy()
        for i in range(planes.shape[0]):
            self.write(paths[i] if paths is not None else None, planes[i, 0], k0 + i)


@torch.no_grad()
def test_MTD_GAN_Ours(model, loss, data_loader, device, save_dir):
    """Mirror of engine.py:108-183: whole-slice inference, L1, RMSE / PSNR / SSIM of (input, gt, clipped prediction) per slice,
    pred_results.csv.  The perceptual metrics PL and TML (engine.py:139-140, VGG-19 features) are computed when the model carries
    the feature network: `model.perceptual_vgg = metrics.VGG19Features(state_dict)` -- the torchvision `vgg19` checkpoint is the
    caller's to hand over, none ships with this package.  The result then gains input_pl / gt_pl / pred_pl / input_tml / gt_tml /
    pred_tml and the CSV the reference's PL and TML columns (slices of at least 256 x 256: metrics.compute_TML); without the
    attribute (or with None) the keys and the CSV are those of the pixel metrics alone.  FID (engine.py:145-146,179-181) is
    computed when the model carries a feature extractor: `model.fid_features = metrics.InceptionV3Features(state_dict)` (the
    reference's network on the HIP kernels; the checkpoint is the caller's to hand over, none ships with this package)
    or any callable on a (B, 3, H, W) batch (metrics.compute_feat).  The three feature
    rows of every slice stay on the device and the result gains input_fid / gt_fid / pred_fid after the loop
    (metrics.compute_FID: float64 statistics and matrix square root on the HIP kernels; at least two slices);
    without the attribute (or with None) nothing changes.  Slice sizes as in valid_MTD_GAN_Ours (any 16..512 per side with `model.Generator.allow_any_size = True`; the 128 / 256 / 512 squares with
    binary16 activation storage under `model.Generator.activation_dtype = torch.float16`: predictions and metrics stay fp32;
    window by window under `model.Generator.sliding_window = dict(...)`).
    A loader batch is ONE sample, as in the reference: the metrics reduce over the whole batch tensor and the CSV gets one row
    per batch, so the reference's per-slice rows need batches of one slice.  `model.test_per_slice = True` takes a batch of B
    slices as B samples instead: one generator call, one VGG pass on the 3B images and one feature pass per image
    set, then per-slice L1, pixel and perceptual values -- the reductions of the batch-of-one loop, bit for bit, on the batch's
    maps -- in ONE device -> host copy per batch, B meter updates and B CSV rows (`path_n_20[i]`; `slice_{k}` counts slices).
    Keys, key order, CSV columns and the FID block are unchanged; it composes with the three generator settings above, which end
    at `Generator(x)`.  Without the attribute (or with a falsy value) nothing changes.
    `model.test_save_png = True` (or `dict(depth=8 | 16, level=..., threads=...)`) writes the reference's three PNGs per slice into
    save_dir (engine.py:157-159): input, target and the raw prediction are quantised to PNG scanlines on the device in
    one launch per loader batch, the bytes are copied to the host once, and image_io.PngWriter compresses them on worker threads
    that are joined before this function returns (a worker's error is raised then).  Greyscale files under the reference's names
    (image_io.png_names); depth 8 holds imsave's grey levels, depth 16 round(clip(., 0, 1) * 65535) without a stretch.  On the
    default path a batch of more than one slice is refused (ValueError): the reference's `.squeeze()` has no image for it; use
    `test_per_slice`, where B slices give 3B files.  Without the attribute (or with a falsy value) nothing changes.
    `model.test_from_stored = True` (or `dict(a_min=..., a_max=...)`) reads the loader's batches as the DICOM files'
    stored pixel values: `n_20` / `n_100` are int16 or uint16 (B, 1, H, W), `rescale_n_20` / `rescale_n_100` their (B, 2)
    (RescaleSlope, RescaleIntercept) pairs, and one fused launch per dose level (dicom_io.stored_to_window: the reference's
    get_pixels_hu and the window [-160, 240], or the dict's) replaces `.float()`; everything after it sees the floats that
    window_slices gives on get_pixels_hu's HU.  `model.test_save_dcm = callable(path_n_20, stored_int16_2d_numpy, k)` (for
    instance dicom_io.pydicom_writer(dcm_dir), which fills the reference's /dcm/ folder) is called once per slice with the
    prediction back in stored pixel values (dicom_io.window_to_stored of the raw prediction: clipped, the reference's truncation,
    the input's own word where the input's HU lies outside the window): one launch and one device -> host copy per loader batch,
    read after the batch's metrics.  It needs `test_from_stored`, and like the PNGs `test_per_slice` for batches of more than one
    slice (ValueError otherwise).  Without the attributes (or with falsy values) nothing changes.
    `model.test_iqa = True` (or a tuple of names from ("ms_ssim", "vif", "gmsd")) adds the reference's vendored piq
    metrics MS-SSIM, VIFp and GMSD of (input, gt, clipped prediction) against gt on the HIP kernels of csrc/iqa.hip
    (metrics.iqa_metrics_each): the result gains {input,gt,pred}_{ms_ssim,vif,gmsd} after the other per-sample keys and the CSV the
    columns MS_SSIM, VIF, GMSD (of those chosen, in that order) after SSIM, holding the prediction's values.  On the default path a
    batch gives one value per metric and image set (the mean over its slices, piq's reduction='mean'); under `test_per_slice` the
    B values per slice travel in the batch's one device -> host copy.  Slices of at least 161 x 161 for MS-SSIM, 41 x 41 for
    VIFp (ValueError otherwise).  Any other value of the attribute is refused (ValueError) before anything runs; without it (or
    with a falsy value) nothing changes.
    `model.test_haarpsi = True` (or `dict(c=..., alpha=..., subsample=...)`) adds the reference's vendored piq metric
    HaarPSI (haarpsi with scales=3) of (input, gt, clipped prediction) against gt on the HIP kernels of csrc/haarpsi.hip
    (metrics.haarpsi_each): the result gains input_haarpsi / gt_haarpsi / pred_haarpsi after the `test_iqa` keys (before the FID /
    KID keys) and the CSV the column HaarPSI after the IQA columns, holding the prediction's value.  On the default path a batch
    gives one value per image set (the mean over its slices, piq's reduction='mean', one more host read); under `test_per_slice`
    the 3 B values travel in the batch's one device -> host copy, behind the IQA block.  Slices of at least 16 x 16 (ValueError
    otherwise).  Any other value of the attribute -- a dict with other keys, a non-positive c or alpha, a subsample that is not a
    bool -- is refused (ValueError) before anything runs; without it (or with a falsy value) nothing changes.
    `model.test_fsim = True` (or a dict of scales, orientations, min_length, mult, sigma_f, delta_theta, k) adds the
    reference's vendored piq metric FSIM (fsim with chromatic=False) of (input, gt, clipped prediction) against gt on the HIP
    kernels of csrc/fsim.hip (metrics.fsim_each): the result gains input_fsim / gt_fsim / pred_fsim after the HaarPSI keys (before
    the FID / KID keys) and the CSV the column FSIM after HaarPSI, holding the prediction's value.  On the default path a batch
    gives one value per image set (the mean over its slices, one more host read); under `test_per_slice` the 3 B values travel
    in the batch's one device -> host copy, behind the HaarPSI block.  The slices must pool (metrics.fsim_pooled_size) to sides
    that are powers of two in 16..512 (ValueError otherwise).  Any other value of the attribute is refused (ValueError) before
    anything runs; without it (or with a falsy value) nothing changes.
    `model.test_lpips = <weights>` (LPIPS's five linear-layer weight tensors or a path to them, or `dict(weights=...,
    distance="mse" | "mae")`) and `model.test_dists = <weights>` (DISTS's dict of alpha and beta, or a path) add the
    reference's vendored piq metrics LPIPS and DISTS of (input, gt, clipped prediction) against gt on the feature network
    `model.perceptual_vgg16 = metrics.VGG16Features(state_dict)` (the torchvision `vgg16` checkpoint and both weight files are the
    caller's to hand over, none ships with this package) and the HIP kernels of csrc/lpips.hip (metrics.lpips_each /
    dists_each): the result gains {input,gt,pred}_lpips and {input,gt,pred}_dists after the FSIM keys (before the FID / KID keys)
    and the CSV the columns LPIPS and DISTS after FSIM, holding the prediction's values.  On the default path a batch gives one
    value per image set (the mean over its slices, one more host read each); under `test_per_slice` the 3 B values of each travel
    in the batch's one device -> host copy, behind the FSIM block.  Slices of at least 16 x 16.  Weights in another form, another
    distance, or either option without `perceptual_vgg16` are refused (ValueError) before anything runs; without the attributes
    (or with None / False) nothing changes.
    `model.test_vsi = True` (or a dict of c1, c2, c3, alpha, beta, omega_0, sigma_f, sigma_d, sigma_c) and `model.test_mdsi = True`
    (or a dict of c1, c2, c3, combination, alpha, beta, gamma, rho, q, o) add the reference's vendored piq metrics VSI
    and MDSI of (input, gt, clipped prediction) against gt on the HIP kernels of csrc/vsi.hip and csrc/mdsi.hip (metrics.vsi_each /
    mdsi_each): the result gains {input,gt,pred}_vsi and {input,gt,pred}_mdsi after the DISTS keys (before the FID / KID keys) and
    the CSV the columns VSI and MDSI after DISTS, holding the prediction's values.  On the default path a batch gives one value
    per image set (the mean over its slices, one more host read each); under `test_per_slice` the 3 B values of each travel in
    the batch's one device -> host copy, behind the DISTS block.  Slices with sides in 16..1024 (ValueError otherwise).  Any other
    value of either attribute is refused (ValueError) before anything runs; without them (or with falsy values) nothing changes.
    `model.test_brisque = <weights>` (piq's (sv_coef, sv) pair of the support vector regression or a path to it, or
    `dict(weights=..., kernel_size=..., kernel_sigma=...)`; none ships with this package) and `model.test_tv = True` (or
    `dict(norm_type="l1" | "l2" | "l2_squared")`) add the reference's vendored piq no-reference metrics BRISQUE and
    total variation of input, gt and the clipped prediction, each on its own, on the HIP kernels of csrc/brisque.hip
    (metrics.brisque_each / tv_each): the result gains {input,gt,pred}_brisque and {input,gt,pred}_tv after the MDSI keys (before
    the FID / KID keys) and the CSV the columns BRISQUE and TV after MDSI, holding the prediction's values.  A slice on which piq
    would assert (a constant one) has the BRISQUE value NaN.  Batches as for VSI and MDSI; sides in 16..1024.  Any other value
    of either attribute is refused (ValueError) before anything runs; without them (or with None / False) nothing changes.
    `model.test_kid = True` (or a dict of metrics.kid_distance64's keyword arguments) adds piq's Kernel Inception
    Distance after the loop, from the same feature rows as FID and therefore only with `model.fid_features` (ValueError
    otherwise, before anything runs): the result gains input_kid / gt_kid / pred_kid behind the FID keys (metrics.compute_KID:
    float64 on the HIP kernels of csrc/kid.hip, returned as float32) and, with ret_var, input_kid_var / gt_kid_var / pred_kid_var;
    the three or six values cross in one device -> host copy.  The subsets are drawn from torch's global CPU generator as piq
    draws them, three calls' worth in the order input, gt, pred.  The CSV does not change.  Without the attribute (or with a
    falsy value) nothing changes.
    `model.test_msid = True` / `model.test_is = True` (or dicts of metrics.msid_distance64's / metrics.is_distance64's keyword
    arguments) add piq's Multi-Scale Intrinsic Distance and the distance of Inception Scores in the same way, from the
    same feature rows (ValueError without `model.fid_features`, before anything runs): input_msid / gt_msid / pred_msid, then
    input_is / gt_is / pred_is, behind the KID keys (metrics.compute_MSID / compute_IS: float64 on the HIP kernels of
    csrc/msid.hip, returned as float32; three values per metric in one device -> host copy).  MSID's starting vectors are drawn
    from numpy's global generator as piq draws them, three calls' worth in the order input, gt, pred; gt_msid is therefore not
    0.  The CSV does not change; without the attributes nothing changes."""
    active = _per_slice_options(model)                   # (a bad value is refused before anything else is set up)
    after = (_kid_option(model), _msid_option(model), _is_option(model))
    stored = _StoredInput.from_model(model)
    dcm = _DcmSink.from_model(model, stored)
    png = _PngSink.from_model(model, save_dir)
    if png is None:
        return _test_loop(model, loss, data_loader, device, save_dir, None, stored, dcm, active, after)
    try:
        return _test_loop(model, loss, data_loader, device, save_dir, png, stored, dcm, active, after)
    finally:
        png.writer.close()


def _test_loop(model, loss, data_loader, device, save_dir, png, stored, dcm, active, after):
    """The body of test_MTD_GAN_Ours; png: the _PngSink of `model.test_save_png`, stored: the _StoredInput of
    `model.test_from_stored`, dcm: the _DcmSink of `model.test_save_dcm`, or None each; active: _per_slice_options' pairs;
    after: the parsed options of the metrics of the feature rows (kid, msid, is), None where off."""
    from . import metrics as M
    model.Generator.eval()
    vgg = getattr(model, "perceptual_vgg", None)
    fid_features = getattr(model, "fid_features", None)
    per_slice = bool(getattr(model, "test_per_slice", False))
    for _, kw in active:                                 # the small weight tables go to the device once, not once per batch
        if "weights" in kw:
            kw["weights"] = kw["weights"].to(device)
    kid, msid, isc = after
    feats = ([], [], [])
    meters = {}
    rows = []
    for batch_data in data_loader:
        if dcm is not None and not per_slice and len(batch_data["n_20"]) != 1:         # (before anything is launched)
            raise ValueError(f"test_save_dcm: a loader batch of {len(batch_data['n_20'])} slices on the default path, where a batch is "
                             "one sample; set model.test_per_slice = True for batches of slices")
        if stored is not None:
            x, words, table = stored.window(batch_data, "n_20", device)
            y = stored.window(batch_data, "n_100", device)[0]
        else:
            x = batch_data["n_20"].to(device).float()
            y = batch_data["n_100"].to(device).float()
        if png is not None and not per_slice and x.shape[0] != 1:
            raise ValueError(f"test_save_png: a loader batch of {x.shape[0]} slices on the default path, where a batch is one sample "
                             "and the reference saves its one image; set model.test_per_slice = True for batches of slices")
        pred = model.Generator(x)
        k0 = len(rows)
        if png is not None:
            images = png.begin(x, y, pred)                     # one launch and the copy of the bytes, behind the generator
        if dcm is not None:
            slices = dcm.begin(pred, words, table)             # likewise
        if per_slice:
            _test_batch_per_slice(loss, batch_data, x, y, pred, vgg, fid_features, feats, meters, rows, active)
            if png is not None:
                png.submit(images, batch_data, k0)
            if dcm is not None:
                dcm.submit(slices, batch_data, k0)
            continue
        meters.setdefault("L1_loss", _Meter()).update(float(_l1(loss, pred, y)), 1)
        from . import kernels as K
        clipped = K.clip01(pred.contiguous())
        perceptual = ()
        if vgg is not None:
            six = M.perceptual_metrics(x, y, clipped, vgg).tolist()        # the slice's six values in one device -> host copy
            for j, name in enumerate(("pl", "tml")):
                _update_triple(meters, name, six[3 * j:3 * j + 3])
            perceptual = (six[2], six[5])
        if fid_features is not None:
            for rows_, f in zip(feats, M.compute_feat(x, y, clipped, extractor=fid_features)):
                rows_.append(f.float())
        pm = M.pixel_metrics(x, y, clipped)
        for name, triple in pm.items():
            _update_triple(meters, name, triple)
        more = ()
        for e, kw in active:         # the batch is one sample: the mean over its slices, piq's reduction='mean' (one more host read each)
            means = getattr(M, e.each)(x, y, clipped, **kw).mean(dim=-1).reshape(-1, 3).tolist()
            for name, triple in zip(_names(e, kw), means):
                _update_triple(meters, name, triple)
                more += (triple[2],)
        path = batch_data.get("path_n_20", [f"slice_{len(rows)}"])[0] if isinstance(batch_data, dict) else f"slice_{len(rows)}"
        rows.append((path,) + perceptual + (pm["rmse"][2], pm["psnr"][2], pm["ssim"][2]) + more)
        if png is not None:
            png.submit(images, batch_data, k0)
        if dcm is not None:
            dcm.submit(slices, batch_data, k0)
    if save_dir:
        import os
        os.makedirs(save_dir, exist_ok=True)
        with open(os.path.join(save_dir, "pred_results.csv"), "w") as f:
            f.write((",PATH,PL,TML,RMSE,PSNR,SSIM" if vgg is not None else ",PATH,RMSE,PSNR,SSIM")
                    + "".join("," + e.columns[name] for e, kw in active for name in _names(e, kw)) + "\n")
            for i, r in enumerate(rows):
                f.write(f"{i}," + ",".join(str(v) for v in r) + "\n")
    if fid_features is not None:
        sets = [torch.cat(f, dim=0) for f in feats]
        _update_triple(meters, "fid", torch.stack(M.compute_FID(*sets)).tolist())       # the three values in one device -> host copy
        if kid is not None:
            triple = M.compute_KID(*sets, **kid)
            with_var = bool(kid.get("ret_var"))
            vals = torch.stack([t[j] for j in range(2) for t in triple] if with_var else list(triple)).tolist()       # three or six values, one copy
            for j, name in enumerate(("kid", "kid_var") if with_var else ("kid",)):
                _update_triple(meters, name, vals[3 * j:3 * j + 3])
        for name, opt, compute in (("msid", msid, M.compute_MSID), ("is", isc, M.compute_IS)):
            if opt is not None:
                _update_triple(meters, name, torch.stack(compute(*sets, **opt)).tolist())       # three values, one copy
    return {k: round(mm.global_avg, 7) for k, mm in meters.items()}
