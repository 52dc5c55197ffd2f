"""The reference's module/sliding_window.py on the device: its five multi-output variants of monai's sliding-window inference,
which run Multi_Task_Discriminator_Skip (or one of the ablation discriminators) over a whole slice, window by window.  Same
names, same leading arguments, same return values; each is inferers.sliding_window_inference_multi with
drop_empty_chunks=True (the reference's `if window_data.sum(): cls_list.append(cls_prob)`; the one difference, any nonzero
element instead of a nonzero sum, is stated there).  The discriminators in eval() under torch.no_grad() are predictors as they
stand.  Semantics restate the reference's loop (monai is not a dependency); what the kernels do not take is
refused by name."""
from ..inferers import sliding_window_inference_multi


def _run(who, outputs, inputs, roi_size, sw_batch_size, predictor, overlap, mode, sigma_scale, padding_mode, cval, sw_device, device,
         progress, args, kwargs):
    mode, padding_mode = getattr(mode, "value", mode), getattr(padding_mode, "value", padding_mode)
    for name, value, default in (("padding_mode", padding_mode, "constant"), ("cval", cval, 0.0), ("sw_device", sw_device, None),
                                 ("device", device, None), ("progress", progress, False)):
        if value != default:
            raise NotImplementedError(f"{who}: {name} is accepted at its default {default!r} only (inputs smaller than the roi are not "
                                      f"padded, windows and results stay on the inputs' device, no progress bar), got {value!r}")
    fn = (lambda w: predictor(w, *args, **kwargs)) if args or kwargs else predictor
    out = sliding_window_inference_multi(inputs, roi_size, sw_batch_size, fn, overlap, mode, sigma_scale, outputs=outputs,
                                         drop_empty_chunks=True)
    return tuple(out[n] for n in outputs) if len(outputs) > 1 else out[outputs[0]]


def sliding_window_inference_three_output(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, mode="constant", sigma_scale=0.125,
                                          padding_mode="constant", cval=0.0, sw_device=None, device=None, progress=False, *args,
                                          **kwargs):
    """predictor -> (cls, seg, rec).  Returns (cls (kept, 1), seg (B, 1, H, W), rec (B, 1, H, W)); module/sliding_window.py:126."""
    return _run("sliding_window_inference_three_output", ("cls", "seg", "rec"), inputs, roi_size, sw_batch_size, predictor, overlap, mode,
                sigma_scale, padding_mode, cval, sw_device, device, progress, args, kwargs)


def sliding_window_inference_two_output_seg_rec(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, mode="constant",
                                                sigma_scale=0.125, padding_mode="constant", cval=0.0, sw_device=None, device=None,
                                                progress=False, *args, **kwargs):
    """predictor -> (seg, rec).  Returns (seg, rec); module/sliding_window.py:227."""
    return _run("sliding_window_inference_two_output_seg_rec", ("seg", "rec"), inputs, roi_size, sw_batch_size, predictor, overlap, mode,
                sigma_scale, padding_mode, cval, sw_device, device, progress, args, kwargs)


def sliding_window_inference_two_output_cls_rec(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, mode="constant",
                                                sigma_scale=0.125, padding_mode="constant", cval=0.0, sw_device=None, device=None,
                                                progress=False, *args, **kwargs):
    """predictor -> (cls, rec).  Returns (cls (kept, 1), rec); module/sliding_window.py:321."""
    return _run("sliding_window_inference_two_output_cls_rec", ("cls", "rec"), inputs, roi_size, sw_batch_size, predictor, overlap, mode,
                sigma_scale, padding_mode, cval, sw_device, device, progress, args, kwargs)


def sliding_window_inference_two_output_cls_seg(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, mode="constant",
                                                sigma_scale=0.125, padding_mode="constant", cval=0.0, sw_device=None, device=None,
                                                progress=False, *args, **kwargs):
    """predictor -> (cls, seg).  Returns (cls (kept, 1), seg); module/sliding_window.py:415."""
    return _run("sliding_window_inference_two_output_cls_seg", ("cls", "seg"), inputs, roi_size, sw_batch_size, predictor, overlap, mode,
                sigma_scale, padding_mode, cval, sw_device, device, progress, args, kwargs)


def sliding_window_inference_cls_output(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, mode="constant", sigma_scale=0.125,
                                        padding_mode="constant", cval=0.0, sw_device=None, device=None, progress=False, *args, **kwargs):
    """predictor -> cls.  Returns cls (kept, 1): scores only, nothing is blended; module/sliding_window.py:765."""
    return _run("sliding_window_inference_cls_output", ("cls",), inputs, roi_size, sw_batch_size, predictor, overlap, mode, sigma_scale,
                padding_mode, cval, sw_device, device, progress, args, kwargs)
