"""Host side of multi-output sliding-window inference (inferers.sliding_window_inference_multi, module/sliding_window.py):
the float64 restatement of tests/_sw_multi_ref.py against the reference's own functions and against the committed fixture,
every refusal before a device is touched, and the new C entry points' declarations and argument checks."""
import ctypes
import enum
import importlib.util
import math
import os
import re
import sys
import types

import pytest
import torch

import _sw_multi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mtd_sw_blend_multi", "mtd_sw_finish_multi", "mtd_sw_gather_flags")
EINVAL = -1


# ---------------------------------------------------------------------------------- the reference's own functions
def _monai_stubs():
    """The four monai helpers module/sliding_window.py uses, written from their documented behaviour, and the names it imports
    beside them."""
    class BlendMode(enum.Enum):
        CONSTANT = "constant"
        GAUSSIAN = "gaussian"

    class PytorchPadMode(enum.Enum):
        CONSTANT = "constant"
        REFLECT = "reflect"
        REPLICATE = "replicate"
        CIRCULAR = "circular"

    def look_up_option(opt, supported):
        return opt if isinstance(opt, supported) else supported(opt)

    def fall_back_tuple(user, default):
        """user broadcast to the default's length; entries that are None or not positive fall back to the default's."""
        user = (user,) * len(default) if not isinstance(user, (tuple, list)) else tuple(user)
        return tuple(u if u is not None and u > 0 else d for u, d in zip(user, default))

    def get_valid_patch_size(image_size, patch_size):
        """the patch size, no larger than the image along any axis."""
        return tuple(min(i, p) for i, p in zip(image_size, fall_back_tuple(patch_size, image_size)))

    def dense_patch_slices(image_size, patch_size, scan_interval):
        """every patch of a dense scan as a tuple of slices, first axis outermost: along an axis the starts are d * interval
        up to the first patch that reaches the border, which is pulled back to end at it."""
        axes = []
        for size, p, iv in zip(image_size, patch_size, scan_interval):
            n = 1 if iv == 0 else next((d for d in range(math.ceil(size / iv)) if d * iv + p >= size), 0) + 1
            axes.append([min(d * iv, size - p) for d in range(n)])
        out = [()]
        for ax, p in zip(axes, patch_size):
            out = [o + (slice(s, s + p),) for o in out for s in ax]
        return out

    def compute_importance_map(patch_size, mode=BlendMode.CONSTANT, sigma_scale=0.125, device="cpu"):
        """constant: ones.  gaussian: the outer product of exp(-t^2 / (2 sigma^2)) per axis, sigma = n * sigma_scale and
        t = -(n-1)/2 .. (n-1)/2, clamped from below at max(its smallest entry, 1e-3); fp32."""
        mode = look_up_option(mode, BlendMode)
        if mode == BlendMode.CONSTANT:
            return torch.ones(tuple(patch_size), dtype=torch.float32, device=device)
        m = None
        for n in patch_size:
            t = torch.arange(n, dtype=torch.float64) - (n - 1) / 2.0
            a = torch.exp(t * t / (-2.0 * (n * sigma_scale) ** 2))
            m = a if m is None else m.unsqueeze(-1) * a
        m = m.float()
        return m.clamp_(min=max(m.min().item(), 1e-3)).to(device)

    mods = {n: types.ModuleType(n) for n in ("monai", "monai.data", "monai.data.utils", "monai.utils")}
    mods["monai.data.utils"].__dict__.update(compute_importance_map=compute_importance_map, dense_patch_slices=dense_patch_slices,
                                             get_valid_patch_size=get_valid_patch_size)
    mods["monai.utils"].__dict__.update(BlendMode=BlendMode, PytorchPadMode=PytorchPadMode, fall_back_tuple=fall_back_tuple,
                                        look_up_option=look_up_option, optional_import=lambda *a, **k: (None, False))
    return mods


@pytest.fixture(scope="module")
def reference():
    """module/sliding_window.py of the reference tree, imported under the monai stubs (skip where the tree is absent)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    try:
        import _refboot
    finally:
        sys.path.pop(0)
    path = os.path.join(_refboot.REF, "module", "sliding_window.py")
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    stubs = _monai_stubs()
    saved = {n: sys.modules.get(n) for n in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("_reference_sliding_window", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in saved.items():
            if m is None:
                del sys.modules[n]
            else:
                sys.modules[n] = m
    return mod


def reference_cases(ref):
    """What the fixture holds, computed by the reference's three_output: name -> fp32 tensor."""
    out = {}
    for name, (shape, roi, overlap, sb, modes, kind) in R.FIXTURE_CASES.items():
        x = R.case_input(shape, kind, seed=sum(shape))
        out[f"{name}/x"] = x
        if kind == "empty":
            for chunk in (3, 4):
                out[f"{name}/c{chunk}/cls"] = ref.sliding_window_inference_three_output(x, roi, chunk, R.toy_predictor, overlap, modes[0])[0]
            continue
        for mode in modes:
            cls, seg, rec = ref.sliding_window_inference_three_output(x, roi, sb, R.toy_predictor, overlap, mode)
            out.update({f"{name}/{mode}/cls": cls, f"{name}/{mode}/seg": seg, f"{name}/{mode}/rec": rec})
    return out


def test_restatement_matches_the_reference(reference):
    got = reference_cases(reference)
    for name, (shape, roi, overlap, sb, modes, kind) in R.FIXTURE_CASES.items():
        x = got[f"{name}/x"]
        if kind == "empty":
            for chunk, kept in ((3, list(range(6))), (4, list(range(4)))):
                r = R.restate(x, roi, chunk, overlap, modes[0])
                assert r["kept"] == kept and torch.equal(r["cls"], got[f"{name}/c{chunk}/cls"]), chunk
                assert torch.equal(r["cls"], r["scores"][kept].reshape(-1, 1))
            continue
        for mode in modes:
            r = R.restate(x, roi, sb, overlap, mode)
            assert torch.equal(r["cls"], got[f"{name}/{mode}/cls"]) and tuple(r["cls"].shape) == (r["counts"][0] * r["counts"][1], 1)
            for n in ("seg", "rec"):
                err = (got[f"{name}/{mode}/{n}"].double() - r[n]).abs().max().item()
                print(f"{name} {mode} {n}: k {r['k']}, max err {err:.3e}, bound {R.bound(r['k'], r['maxabs'][n]):.3e}")
                assert err <= R.bound(r["k"], r["maxabs"][n])


def test_restatement_matches_the_reference_siblings(reference):
    """The two-output and the cls-only functions are the same loop with fewer outputs."""
    shape, roi, overlap, sb, _modes, kind = R.FIXTURE_CASES["odd_roi"]
    x = R.case_input(shape, kind, seed=sum(shape))
    r = R.restate(x, roi, sb, overlap, "gaussian")
    pick = lambda *idx: (lambda w: tuple(R.toy_predictor(w)[i] for i in idx) if len(idx) > 1 else R.toy_predictor(w)[idx[0]])
    b = lambda n: R.bound(r["k"], r["maxabs"][n])
    seg, rec = reference.sliding_window_inference_two_output_seg_rec(x, roi, sb, pick(1, 2), overlap, "gaussian")
    assert (seg.double() - r["seg"]).abs().max().item() <= b("seg") and (rec.double() - r["rec"]).abs().max().item() <= b("rec")
    cls, rec = reference.sliding_window_inference_two_output_cls_rec(x, roi, sb, pick(0, 2), overlap, "gaussian")
    assert torch.equal(cls, r["cls"]) and (rec.double() - r["rec"]).abs().max().item() <= b("rec")
    cls, seg = reference.sliding_window_inference_two_output_cls_seg(x, roi, sb, pick(0, 1), overlap, "gaussian")
    assert torch.equal(cls, r["cls"]) and (seg.double() - r["seg"]).abs().max().item() <= b("seg")
    assert torch.equal(reference.sliding_window_inference_cls_output(x, roi, sb, pick(0), overlap, "gaussian"), r["cls"])


def test_reference_reproduces_the_fixture(reference):
    got, fix = reference_cases(reference), R.load_fixture()
    assert sorted(got) == sorted(fix)
    for k, v in got.items():
        assert v.dtype == torch.float32 and fix[k].dtype == torch.float32 and v.shape == fix[k].shape, k
        if "/gaussian/" in k and not k.endswith("cls"):
            # the map's exp is evaluated by this machine's libm: one rounding of the map apart at the most
            assert (v - fix[k]).abs().max().item() <= 4 * R.U * max(1.0, fix[k].abs().max().item()), k
        else:
            assert torch.equal(v, fix[k]), k


def test_fixture_is_small_data():
    assert os.path.getsize(R.FIXTURE) < 200 * 1024
    fix = R.load_fixture()
    for name, (shape, _roi, _ov, _sb, _modes, kind) in R.FIXTURE_CASES.items():
        assert torch.equal(fix[f"{name}/x"], R.case_input(shape, kind, seed=sum(shape))), name       # the inputs are the seeded ones


def test_restatement_matches_the_fixture():
    """Runs without the reference tree: the fixture's reference values against the float64 restatement."""
    fix = R.load_fixture()
    for name, (shape, roi, overlap, sb, modes, kind) in R.FIXTURE_CASES.items():
        x = fix[f"{name}/x"]
        if kind == "empty":
            for chunk in (3, 4):
                assert torch.equal(R.restate(x, roi, chunk, overlap, modes[0])["cls"], fix[f"{name}/c{chunk}/cls"])
            continue
        for mode in modes:
            r = R.restate(x, roi, sb, overlap, mode)
            assert torch.equal(r["cls"], fix[f"{name}/{mode}/cls"])
            for n in ("seg", "rec"):
                assert (fix[f"{name}/{mode}/{n}"].double() - r[n]).abs().max().item() <= R.bound(r["k"], r["maxabs"][n]), (name, mode, n)


# ------------------------------------------------------------------------------------------------------- refusals
def _x(*shape):
    return torch.zeros(*shape)


def test_multi_refusals_name_what_is_accepted():
    from mtd_gan_amd.inferers import sliding_window_inference_multi as f
    with pytest.raises(NotImplementedError, match="CUDA"):                               # a CPU tensor, otherwise fine
        f(_x(1, 1, 96, 96), (64, 64), 4, R.toy_predictor, overlap=0.5)
    with pytest.raises(NotImplementedError, match="single-channel"):
        f(_x(1, 3, 96, 96), (64, 64), 4, R.toy_predictor)
    with pytest.raises(ValueError, match="roi"):
        f(_x(1, 1, 48, 96), (64, 64), 4, R.toy_predictor)
    for overlap in (-0.1, 1.0, (0.3, 0.3)):
        with pytest.raises(ValueError, match="overlap"):
            f(_x(1, 1, 96, 96), (64, 64), 4, R.toy_predictor, overlap=overlap)
    with pytest.raises(ValueError, match="mode"):
        f(_x(1, 1, 96, 96), (64, 64), 4, R.toy_predictor, mode="linear")
    with pytest.raises(ValueError, match="sw_batch_size"):
        f(_x(1, 1, 96, 96), (64, 64), 0, R.toy_predictor)
    with pytest.raises(ValueError, match="inputs"):
        f(_x(1, 96, 96), (64, 64), 4, R.toy_predictor)
    with pytest.raises(NotImplementedError, match="float32"):
        f(_x(1, 1, 96, 96).double(), (64, 64), 4, R.toy_predictor)
    # the keyword arguments of this call, refused before the tensor is looked at
    for outputs in ((), ("seg", "seg"), ("cls", "cls_map"), (1, "seg")):
        with pytest.raises(ValueError, match="outputs"):
            f(_x(1, 1, 96, 96), (64, 64), 4, R.toy_predictor, outputs=outputs)
    with pytest.raises(ValueError, match="score_map"):
        f(_x(1, 1, 96, 96), (64, 64), 4, R.toy_predictor, outputs=("seg", "rec"), score_map=True)
    with pytest.raises(ValueError, match="clip"):
        f(_x(1, 1, 96, 96), (64, 64), 4, R.toy_predictor, clip=("cls",))
    with pytest.raises(ValueError, match="clip"):
        f(_x(1, 1, 96, 96), (64, 64), 4, R.toy_predictor, clip=("cls_map",))           # no score map asked for
    with pytest.raises(NotImplementedError, match="at most 4"):
        f(_x(1, 1, 96, 96), (64, 64), 4, R.toy_predictor, outputs=("a", "b", "c", "d", "e"))
    with pytest.raises(NotImplementedError, match="at most 4"):
        f(_x(1, 1, 96, 96), (64, 64), 4, R.toy_predictor, outputs=("cls", "a", "b", "c", "d"), score_map=True)


def test_predictor_outputs_are_checked():
    from mtd_gan_amd.inferers import _check_predictions
    w = _x(3, 1, 64, 64)
    names = ("cls", "seg", "rec")
    assert len(_check_predictions((_x(3, 1), w + 1, w), w, names)) == 3
    assert len(_check_predictions([_x(3), w, w], w, names)) == 3
    assert len(_check_predictions(_x(3, 1), w, ("cls",))) == 1                         # a bare tensor for one name
    assert len(_check_predictions(w, w, ("seg",))) == 1
    for bad in ((_x(3, 1), w), w, None, (_x(3, 1), w, w, w)):
        with pytest.raises(ValueError, match="one tensor per output name"):
            _check_predictions(bad, w, names)
    for bad, name in (((_x(3, 2), w, w), "cls"), ((_x(2, 1), w, w), "cls"), ((_x(3, 1).double(), w, w), "cls"),
                      ((_x(3, 1), _x(3, 1, 64, 63), w), "seg"), ((_x(3, 1), w, _x(3, 64, 64)), "rec"), ((_x(3, 1), w, w.half()), "rec"),
                      ((_x(3, 1), None, w), "seg"), ((w, w, w), "cls")):
        with pytest.raises(ValueError, match=f"predictor output '{name}'"):
            _check_predictions(bad, w, names)


def test_kept_windows_is_the_chunk_rule():
    from mtd_gan_amd.inferers import kept_windows
    flags = [1, 1, 1, 1, 0, 0, 0, 0]
    assert kept_windows(flags, 3) == [0, 1, 2, 3, 4, 5] and kept_windows(flags, 4) == [0, 1, 2, 3]
    assert kept_windows(flags, 1) == [0, 1, 2, 3] and kept_windows(flags, 100) == list(range(8))
    assert kept_windows([0, 0, 0], 2) == [] and kept_windows([0, 0, 1], 2) == [2]


@pytest.mark.parametrize("fn,outputs", [("sliding_window_inference_three_output", 3), ("sliding_window_inference_two_output_seg_rec", 2),
                                        ("sliding_window_inference_two_output_cls_rec", 2),
                                        ("sliding_window_inference_two_output_cls_seg", 2), ("sliding_window_inference_cls_output", 1)])
def test_reference_names_refuse_before_a_device_is_touched(fn, outputs):
    from mtd_gan_amd.module import sliding_window as M
    f = getattr(M, fn)
    x, p = _x(1, 1, 96, 96), R.toy_predictor
    for kw, name in ((dict(padding_mode="reflect"), "padding_mode"), (dict(cval=1.0), "cval"), (dict(sw_device="cpu"), "sw_device"),
                     (dict(device="cpu"), "device"), (dict(progress=True), "progress")):
        with pytest.raises(NotImplementedError, match=f"{fn}: {name} "):
            f(x, (64, 64), 4, p, 0.5, "constant", 0.125, **kw)
    with pytest.raises(NotImplementedError, match="CUDA"):                               # the defaults pass, spelled out or not
        f(x, (64, 64), 4, p, 0.5, "gaussian", 0.125, "constant", 0.0, None, None, False)
    with pytest.raises(ValueError, match="roi"):
        f(_x(1, 1, 48, 96), (64, 64), 4, p)
    with pytest.raises(ValueError, match="mode"):
        f(x, (64, 64), 4, p, 0.5, "linear")


# ------------------------------------------------------------------------------------------------ the C entry points
@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    return ctypes.CDLL(_lib.LIB_PATH)


def test_new_entry_points_are_declared_and_bound(built_lib):
    from mtd_gan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\bint (mtd_sw_[a-z_]+)\s*\(([^;]*)\);", hdr)}
    L = _lib.lib()
    for n in ENTRIES:
        assert n in _lib.EXPORTS and n in declared, n
        f = getattr(L, n)
        assert f.restype is ctypes.c_int and len(f.argtypes) == declared[n].count(",") + 1, n        # one ctypes type per parameter
        for ctype, param in zip(f.argtypes, declared[n].split(",")):
            want = ctypes.c_void_p if "*" in param else ctypes.c_longlong if "long long" in param else ctypes.c_int
            assert ctype is want, (n, param.strip())


def _bind(lib):
    ci, ll, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    lib.mtd_sw_blend_multi.restype, lib.mtd_sw_blend_multi.argtypes = ci, [ci, vp, vp, vp, vp] + [ci] * 7 + [ll, ci, vp]
    lib.mtd_sw_finish_multi.restype, lib.mtd_sw_finish_multi.argtypes = ci, [ci, vp, vp, vp, vp] + [ci] * 7 + [vp]
    lib.mtd_sw_gather_flags.restype, lib.mtd_sw_gather_flags.argtypes = ci, [vp] + [ci] * 7 + [ll, ci, vp, vp, vp]
    return lib


def test_entry_points_refuse_bad_arguments_without_gpu(built_lib):
    """Host pointers that are never dereferenced as device memory: plane counts, null planes and geometry are refused before
    anything is launched."""
    L = _bind(built_lib)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    geom = (1, 80, 99, 64, 64, 44, 44)
    ptrs = lambda *v: (ctypes.c_void_p * 5)(*v)
    ints = (ctypes.c_int * 5)(0, 1, 0, 0, 0)
    full = ptrs(p, p, p, p, p)
    for nplanes in (0, 5, -1):
        assert L.mtd_sw_blend_multi(nplanes, full, ints, full, p, *geom, 0, 1, None) == EINVAL, nplanes
        assert L.mtd_sw_finish_multi(nplanes, full, ints, full, p, *geom, None) == EINVAL, nplanes
    for n in (1, 2, 3, 4):                                           # a null plane pointer, in either list, at every position
        for hole in range(n):
            holed = ptrs(*[None if i == hole else p for i in range(5)])
            assert L.mtd_sw_blend_multi(n, holed, ints, full, p, *geom, 0, 1, None) == EINVAL, (n, hole)
            assert L.mtd_sw_blend_multi(n, full, ints, holed, p, *geom, 0, 1, None) == EINVAL, (n, hole)
            assert L.mtd_sw_finish_multi(n, holed, ints, full, p, *geom, None) == EINVAL, (n, hole)
            assert L.mtd_sw_finish_multi(n, full, ints, holed, p, *geom, None) == EINVAL, (n, hole)
    assert L.mtd_sw_blend_multi(2, None, ints, full, p, *geom, 0, 1, None) == EINVAL          # null arrays, null map
    assert L.mtd_sw_blend_multi(2, full, None, full, p, *geom, 0, 1, None) == EINVAL
    assert L.mtd_sw_blend_multi(2, full, ints, full, None, *geom, 0, 1, None) == EINVAL
    assert L.mtd_sw_finish_multi(2, full, ints, None, p, *geom, None) == EINVAL
    assert L.mtd_sw_gather_flags(None, *geom, 0, 1, p, p, None) == EINVAL
    assert L.mtd_sw_gather_flags(p, *geom, 0, 1, None, p, None) == EINVAL
    assert L.mtd_sw_gather_flags(p, *geom, 0, 1, p, None, None) == EINVAL
    for bad, w0, n in (((1, 60, 99, 64, 64, 44, 44), 0, 1),           # H < rh
                       ((1, 80, 99, 64, 64, 0, 44), 0, 1),            # interval 0
                       ((1, 80, 99, 64, 64, 65, 44), 0, 1),           # interval > roi
                       ((1, 80, 99, 64, 64, 44, 44), 3, 2),           # 4 windows: [3, 5) runs past the list
                       ((1, 80, 99, 64, 64, 44, 44), 0, 0),
                       ((0, 80, 99, 64, 64, 44, 44), 0, 1)):
        assert L.mtd_sw_blend_multi(2, full, ints, full, p, *bad, w0, n, None) == EINVAL, (bad, w0, n)
        assert L.mtd_sw_gather_flags(p, *bad, w0, n, p, p, None) == EINVAL, (bad, w0, n)
    for bad in ((1, 60, 99, 64, 64, 44, 44), (1, 80, 99, 64, 64, 0, 44), (0, 80, 99, 64, 64, 44, 44)):
        assert L.mtd_sw_finish_multi(2, full, ints, full, p, *bad, None) == EINVAL, bad


def test_wrappers_refuse_plane_lists_before_the_library():
    from mtd_gan_amd import kernels as K
    t = _x(1, 1, 8, 8)
    with pytest.raises(ValueError, match="1 to 4 planes"):
        K.sw_blend_multi([t] * 5, [False] * 5, t, [t] * 5, (8, 8), (8, 8), 0, 1)
    with pytest.raises(ValueError, match="1 to 4 planes"):
        K.sw_blend_multi([], [], t, [], (8, 8), (8, 8), 0, 1)
    with pytest.raises(ValueError, match="1 to 4 planes"):
        K.sw_blend_multi([t, t], [False], t, [t, t], (8, 8), (8, 8), 0, 1)
    with pytest.raises(ValueError, match="1 to 4 planes"):
        K.sw_finish_multi([t, t], t, (8, 8), (8, 8), [False, False], outs=[t])
