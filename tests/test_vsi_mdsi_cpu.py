"""VSI and MDSI without a GPU: the float64 restatements of tests/_vsi_ref.py and tests/_mdsi_ref.py against what
the reference's own module/piq/vsi.py and mdsi.py computed (tests/golden/vsi_mdsi_piq.npz, written by tools/pin_vsi_mdsi.py), the
conditions the fixture's inputs were chosen to meet, the pooling-kernel rule, the host log-Gabor table, the test loop's option
checks, and the argument refusals of the entry points that need no device (through the built library's ABI, with addresses of
host memory)."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import _mdsi_ref as MR
import _vsi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREADS = ("vsi_score", "vsi_sums", "vsi_limits", "mdsi_score", "mdsi_means", "mdsi_dev")


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    return _lib.lib()


def _rel(got, want):
    """The largest relative distance; where the wanted value is exactly zero the value must be exactly zero too."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    zero = want == 0
    assert (got[zero] == 0).all(), (got, want)
    return float(np.max(np.abs(got - want)[~zero] / np.abs(want[~zero]))) if (~zero).any() else 0.0


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_float64_restatements_agree_with_the_reference(golden, index):
    """The same operations in float64; the order of the sums and of a few products differs: 1e-11 relative on every score and
    part (the bound tests/test_fsim_cpu.py holds its restatement to)."""
    B, H, W, kind, vopts, mopts = R.CASES[index]
    x, y, pred = R.case_inputs(index)
    assert tuple(x.shape) == (B, 1, H, W) and x.dtype == torch.float32
    assert R.crc(x, y, pred) == int(golden[f"crc_{index}"]), "the seeded inputs are not the ones the fixture was written from"
    for k, src in enumerate((x, y, pred)):
        score, parts = R.vsi(src.double(), y.double(), **vopts)
        assert tuple(parts.shape) == (B, len(R.PART_NAMES))
        e = _rel(score.numpy(), golden[f"vsi_score64_{index}"][k])
        assert e <= 1e-11, ("vsi score", k, e)
        for j, name in enumerate(R.PART_NAMES):
            e = _rel(parts[:, j].numpy(), golden[f"vsi_parts64_{index}"][k][:, j])
            assert e <= 1e-11, (name, k, e)
        score, parts = MR.mdsi(src.double(), y.double(), **mopts)
        assert tuple(parts.shape) == (B, len(MR.PART_NAMES))
        e = _rel(score.numpy(), golden[f"mdsi_score64_{index}"][k])
        assert e <= 1e-11, ("mdsi score", k, e)
        for j, name in enumerate(MR.PART_NAMES):
            e = _rel(parts[:, j].numpy(), golden[f"mdsi_parts64_{index}"][k][:, j])
            assert e <= 1e-11, (name, k, e)


def test_fixture_conditions(golden):
    """Conditions on the chosen inputs, not tolerances: the target against itself exactly 1.0 (VSI) and 0.0 (MDSI) in both
    precisions of the reference; den > 1 on every VSI row but the constant pair's, which scores exactly 1.0 through the eps
    terms; the faint input has pixels with negative gs_total and so a mean with an imaginary part; the cases of _vsi_ref; the
    recorded float32 -> float64 distances those of the stored values."""
    meta = json.loads(str(golden["meta"]))
    assert [tuple(c) for c in meta["cases"]] == [tuple(c) for c in R.CASES]
    spread = dict.fromkeys(SPREADS, 0.0)
    for index, (B, H, W, kind, vopts, mopts) in enumerate(R.CASES):
        for tag, dt in (("32", np.float32), ("64", np.float64)):
            for name, shape in (("vsi_score", (3, B)), ("vsi_parts", (3, B, 6)), ("mdsi_score", (3, B)), ("mdsi_parts", (3, B, 3))):
                assert golden[f"{name}{tag}_{index}"].shape == shape and golden[f"{name}{tag}_{index}"].dtype == dt, (name, tag, index)
            assert (golden[f"vsi_score{tag}_{index}"][1] == 1.0).all() and (golden[f"mdsi_score{tag}_{index}"][1] == 0.0).all(), index
            if kind == "constant":
                assert (golden[f"vsi_score{tag}_{index}"] == 1.0).all() and (golden[f"vsi_parts{tag}_{index}"][..., :3] == 0).all()
            else:
                assert (golden[f"vsi_parts{tag}_{index}"][..., 1] > 1).all(), index
        v32, v64, m32, m64 = (golden[f"{n}_{index}"] for n in ("vsi_parts32", "vsi_parts64", "mdsi_parts32", "mdsi_parts64"))
        for name, a, b in (("vsi_score", golden[f"vsi_score32_{index}"], golden[f"vsi_score64_{index}"]), ("vsi_sums", v32[..., :4], v64[..., :4]),
                           ("vsi_limits", v32[..., 4:], v64[..., 4:]), ("mdsi_score", golden[f"mdsi_score32_{index}"], golden[f"mdsi_score64_{index}"]),
                           ("mdsi_means", m32[..., :2], m64[..., :2]), ("mdsi_dev", m32[..., 2], m64[..., 2])):
            spread[name] = max(spread[name], _rel(a, b))
    assert spread == meta["spread"]
    x, y, pred = R.case_inputs(R.FAINT)
    gs = MR.gs_total(x.double(), y.double())
    assert float(gs.min()) < -0.5 and float((gs < 0).double().mean()) > 0.5
    assert abs(float(golden[f"mdsi_parts64_{R.FAINT}"][0, 0, 1])) > 0.01         # the mean's imaginary part
    assert (golden[f"mdsi_parts64_{R.FAINT - 1}"][..., 1] == 0).all()            # ... which is exactly zero without negative values
    assert os.path.getsize(R.GOLDEN) < 64 * 1024


KERNELS = [((16, 16), 1), ((256, 256), 1), ((383, 400), 1), ((384, 384), 2), ((384, 512), 2), ((385, 400), 2), ((512, 512), 2), ((640, 640), 2),
           ((641, 648), 3), ((700, 641), 3), ((1024, 1024), 4), ((1024, 16), 1)]


@pytest.mark.parametrize("size, want", KERNELS)
def test_kernel_size_rule(size, want):
    """Python's round, half to even: 384 / 256 = 1.5 -> 2, 640 / 256 = 2.5 -> 2, 641 -> 3 -- and both pad rules leave
    ceil(side / k) pooled pixels."""
    from mtd_gan_amd import metrics as M
    assert M.vsi_kernel_size(*size) == want == R.kernel_size(*size)
    if size[0] * size[1] <= 1 << 19:
        z = torch.zeros(1, 1, *size)
        for before, after, mode in ((want // 2, (want - 1) // 2, "replicate"), ((want - 1) // 2, want // 2, "constant")):
            assert tuple(R.pool(z, want, before, after, mode).shape[2:]) == tuple(-(-s // want) for s in size)


@pytest.mark.parametrize("index", [0, 8])
def test_host_log_gabor_table_has_the_bytes_of_the_references(golden, index):
    """metrics.vsi_log_gabor_table (frequencies in storage order) and the restatement's table (centred grid, rolled) are written
    independently; both must give the bytes of the table the reference's own _log_gabor built when the fixture was written."""
    from mtd_gan_amd import metrics as M
    vopts = R.CASES[index][4]
    table = M.vsi_log_gabor_table(vopts["omega_0"], vopts["sigma_f"])
    assert table.dtype == torch.float32 and tuple(table.shape) == (256, 256) and table.is_contiguous()
    assert R.crc(table) == int(golden[f"log_gabor_crc_{index}"]), "the host table is not the reference's"
    assert R.crc(R.log_gabor_table(vopts["omega_0"], vopts["sigma_f"])) == int(golden[f"log_gabor_crc_{index}"])
    assert float(table[0, 0]) == 0 and float(table[128, 128]) == 0 and float(table.max()) <= 1.0 and float(table.min()) >= 0.0
    assert int(golden["log_gabor_crc_0"]) != int(golden["log_gabor_crc_8"])
    assert all(int(golden[f"log_gabor_crc_{i}"]) == int(golden["log_gabor_crc_0"]) for i in range(len(R.CASES)) if i != 8)


class _NoLoader:
    def __iter__(self):
        raise AssertionError("the loader must not be read before the option is checked")


BAD_VSI = ["yes", 3, ("c1", 1.27), dict(scales=4), dict(c1=1.27, reduction="mean"), dict(c1=0), dict(c2=-1.0), dict(c3="130"), dict(alpha=None),
           dict(beta=float("nan")), dict(omega_0=0.0), dict(sigma_f=-1.34), dict(sigma_d=0), dict(sigma_c=float("inf")), dict(c1=True),
           dict(combination="sum"), dict(data_range=1.0)]
BAD_MDSI = ["yes", 3, ("c1", 140.), dict(scales=4), dict(c1=140., reduction="mean"), dict(c1=0), dict(c2=-55.), dict(c3="550"), dict(alpha=None),
            dict(beta=float("nan")), dict(gamma="0.2"), dict(rho=0), dict(rho=-1.0), dict(q=float("inf")), dict(o=None), dict(combination="prod"),
            dict(combination=1), dict(omega_0=0.021), dict(data_range=1.0)]


@pytest.mark.parametrize("bad", BAD_VSI)
def test_engine_refuses_a_bad_test_vsi_before_anything_runs(bad):
    from mtd_gan_amd import engine
    model = types.SimpleNamespace(test_vsi=bad)       # no Generator: anything past the option check would fail otherwise
    with pytest.raises(ValueError, match="test_vsi.*c1.*sigma_c"):
        engine.test_MTD_GAN_Ours(model, None, _NoLoader(), torch.device("cpu"), None)


@pytest.mark.parametrize("bad", BAD_MDSI)
def test_engine_refuses_a_bad_test_mdsi_before_anything_runs(bad):
    from mtd_gan_amd import engine
    model = types.SimpleNamespace(test_mdsi=bad)
    with pytest.raises(ValueError, match="test_mdsi.*c1.*combination"):
        engine.test_MTD_GAN_Ours(model, None, _NoLoader(), torch.device("cpu"), None)


def test_engine_option_values():
    from mtd_gan_amd import engine
    vsi = lambda **kw: engine._vsi_option(types.SimpleNamespace(**kw))            # noqa: E731
    mdsi = lambda **kw: engine._mdsi_option(types.SimpleNamespace(**kw))          # noqa: E731
    for opt, name in ((vsi, "test_vsi"), (mdsi, "test_mdsi")):
        assert opt() is None and opt(**{name: None}) is None and opt(**{name: False}) is None
        assert opt(**{name: True}) == {}
    assert vsi(test_vsi=dict(c1=2, beta=-0.5)) == dict(c1=2, beta=-0.5)
    assert vsi(test_vsi=dict(R.OTHER)) == R.OTHER and vsi(test_vsi=dict(R.DEFAULTS)) == R.DEFAULTS
    assert mdsi(test_mdsi=dict(combination="mult", q=-1)) == dict(combination="mult", q=-1)
    assert mdsi(test_mdsi=dict(R.MDSI_OTHER)) == R.MDSI_OTHER and mdsi(test_mdsi=dict(R.MDSI_DEFAULTS)) == R.MDSI_DEFAULTS
    for bad in BAD_VSI:
        with pytest.raises(ValueError):
            vsi(test_vsi=bad)
    for bad in BAD_MDSI:
        with pytest.raises(ValueError):
            mdsi(test_mdsi=bad)
    assert vsi(test_mdsi=True, test_fsim=True) is None and mdsi(test_vsi=True) is None          # the options do not see each other
    assert engine._fsim_option(types.SimpleNamespace(test_vsi=True, test_mdsi=True)) is None


def test_header_declares_and_lib_binds_the_entry_points(built_lib):
    from mtd_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    for n, arity in (("mtd_vsi_ws_bytes", 5), ("mtd_vsi_each", 13), ("mtd_mdsi_ws_bytes", 5), ("mtd_mdsi_each", 13)):
        assert re.search(r"^(size_t|int) %s\(" % n, header, re.M), n
        assert n in _lib.EXPORTS and len(getattr(built_lib, n).argtypes) == arity, n
    for name, value in (("MTD_VSI_PARTS", 6), ("MTD_VSI_OPTIONS", 7), ("MTD_VSI_MIN_SIDE", 16), ("MTD_VSI_MAX_SIDE", 1024), ("MTD_MDSI_PARTS", 3),
                        ("MTD_MDSI_OPTIONS", 9), ("MTD_MDSI_MIN_SIDE", 16), ("MTD_MDSI_MAX_SIDE", 1024)):
        assert re.search(r"^#define %s %d$" % (name, value), header, re.M), name


def _vsi_ws_model(na, B, H, W, k):
    """The chunk rule of DESIGN 3.19 restated: (images per chunk, bytes)."""
    hp, wp = -(-H // k), -(-W // k)
    tiles, blocks = -(-hp // 16) * -(-wp // 16), -(-H * W // 4096)
    per_slot = 48 * 65536 + 64 * 48 + blocks * 16 + 16
    per_image = (na + 1) * per_slot + na * tiles * 32
    Bc = max(1, min(B, (64 << 20) // per_image, 8192))
    return Bc, Bc * per_image


def _mdsi_ws_model(na, B, H, W, k):
    hp, wp = -(-H // k), -(-W // k)
    per_image = na * (-(-hp // 16) * -(-wp // 16) * 16 + 16)
    Bc = max(1, min(B, (16 << 20) // per_image, 8192))
    return Bc, Bc * per_image


def test_workspaces_follow_the_chunk_rule_and_stay_bounded(built_lib):
    for args in ((3, 1, 512, 512, 2), (3, 8, 512, 512, 2), (3, 1000, 512, 512, 2), (1, 64, 256, 256, 1), (3, 2, 16, 16, 1), (3, 64, 64, 64, 1),
                 (2, 5, 385, 400, 2), (3, 1, 1024, 1024, 4), (3, 100000, 16, 16, 1), (3, 1, 641, 648, 3), (3, 7, 300, 500, 1)):
        assert built_lib.mtd_vsi_ws_bytes(*args) == _vsi_ws_model(*args)[1], args
        assert built_lib.mtd_mdsi_ws_bytes(*args) == _mdsi_ws_model(*args)[1], args
    for B in (1, 8, 64, 1 << 20):
        for na in (1, 2, 3):
            for H, W, k in ((16, 16, 1), (512, 512, 2), (1024, 1024, 4), (1024, 1024, 1)):
                assert 0 < built_lib.mtd_vsi_ws_bytes(na, B, H, W, k) <= 64 << 20, (na, B, H, W, k)
                assert 0 < built_lib.mtd_mdsi_ws_bytes(na, B, H, W, k) <= 16 << 20, (na, B, H, W, k)
    assert _vsi_ws_model(3, 8, 512, 512, 2)[0] == 5                # 512 x 512 slices: five images of every set per chunk
    assert _mdsi_ws_model(3, 8192, 512, 512, 2)[0] == 1360


def test_refusals_return_before_any_launch(built_lib):
    """The refused calls touch neither their pointers nor the device."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    vopts = (ctypes.c_double * 7)(1.27, 386., 130., 0.4, 0.02, 145., 0.001)
    mopts = (ctypes.c_double * 9)(140., 55., 550., 0.6, 0.1, 0.2, 1., 0.25, 0.25)

    def vsi(srcs=ptrs, na=3, target=p, B=1, H=64, W=64, k=1, table=p, opts=vopts, out=p, parts=p, ws=p):
        return built_lib.mtd_vsi_each(srcs, na, target, B, H, W, k, table, opts, out, parts, ws, None)

    def mdsi(srcs=ptrs, na=3, target=p, B=1, H=64, W=64, k=1, opts=mopts, mult=0, out=p, parts=p, ws=p):
        return built_lib.mtd_mdsi_each(srcs, na, target, B, H, W, k, opts, mult, out, parts, ws, None)
    # na outside 1..3, B < 1, a side outside 16..1024, k outside 1..8
    for na, B, H, W, k in ((0, 1, 64, 64, 1), (4, 1, 64, 64, 1), (3, 0, 64, 64, 1), (3, -1, 64, 64, 1), (3, 1, 15, 64, 1), (3, 1, 64, 15, 1),
                           (3, 1, 1025, 64, 1), (3, 1, 64, 1025, 1), (3, 1, 64, 64, 0), (3, 1, 64, 64, -1), (3, 1, 64, 64, 9), (3, 1, 65536, 65536, 8)):
        assert built_lib.mtd_vsi_ws_bytes(na, B, H, W, k) == 0 and built_lib.mtd_mdsi_ws_bytes(na, B, H, W, k) == 0, (na, B, H, W, k)
        assert vsi(na=na, B=B, H=H, W=W, k=k) == -1 and mdsi(na=na, B=B, H=H, W=W, k=k) == -1, (na, B, H, W, k)
    for null in ("srcs", "target", "table", "opts", "out", "ws"):
        assert vsi(**{null: None}) == -1, null
    for null in ("srcs", "target", "opts", "out", "ws"):
        assert mdsi(**{null: None}) == -1, null
    for f in (vsi, mdsi):
        assert f(srcs=(ctypes.c_void_p * 3)(p, None, p)) == -1
        assert f(srcs=(ctypes.c_void_p * 3)(p, p, None), parts=None) == -1
    for j, bad in ((0, 0.0), (1, -1.0), (2, float("nan")), (3, float("inf")), (4, float("nan")), (5, 0.0), (6, 0.0), (6, float("inf"))):
        o = (ctypes.c_double * 7)(*vopts)
        o[j] = bad
        assert vsi(opts=o) == -1, (j, bad)
    for j, bad in ((0, 0.0), (1, -1.0), (2, float("nan")), (3, float("inf")), (4, float("nan")), (5, float("-inf")), (6, 0.0), (6, -1.0),
                   (7, float("nan")), (8, float("inf"))):
        o = (ctypes.c_double * 9)(*mopts)
        o[j] = bad
        assert mdsi(opts=o) == -1, (j, bad)
    assert mdsi(mult=2) == -1 and mdsi(mult=-1) == -1


def test_python_surface_refusals_without_a_device():
    from mtd_gan_amd import metrics as M
    x = torch.zeros(2, 1, 64, 64)
    for fn, name in ((M.vsi_each, "vsi"), (M.vsi_per_slice, "vsi"), (M.compute_VSI, "vsi"), (M.mdsi_each, "mdsi"), (M.mdsi_per_slice, "mdsi"),
                     (M.compute_MDSI, "mdsi")):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(x, x, x)
        with pytest.raises(AssertionError):
            fn(x[:1], x, x)
        with pytest.raises(AssertionError):
            fn(x[:, :, :32], x, x)
        with pytest.raises(AssertionError):
            fn(x[0], x[0], x[0])
        with pytest.raises(ValueError, match="64x15"):
            fn(x[:, :, :, :15], x[:, :, :, :15], x[:, :, :, :15])
        big = torch.zeros(1, 1, 1025, 16)
        with pytest.raises(ValueError, match="1025x16"):
            fn(big, big, big)
        for kw in (dict(c1=0), dict(c2=None), dict(alpha=float("nan"))):
            with pytest.raises(ValueError, match=name):
                fn(x, x, x, **kw)
    with pytest.raises(ValueError, match="vsi"):
        M.vsi_each(x, x, x, sigma_c=0)
    with pytest.raises(ValueError, match="mdsi.*combination"):
        M.mdsi_each(x, x, x, combination="both")
    for fn in (M.compute_VSI, M.compute_MDSI):
        with pytest.raises(NotImplementedError):
            fn(x, x, x, data_range=255.0)
    assert (M.VSI_MIN_SIDE, M.VSI_MAX_SIDE) == (M.MDSI_MIN_SIDE, M.MDSI_MAX_SIDE) == (R.MIN_SIDE, R.MAX_SIDE) == (16, 1024)
    assert M.VSI_OPTIONS == tuple(R.DEFAULTS) and M.MDSI_OPTIONS == tuple(R.MDSI_DEFAULTS)
    assert (M.VSI_PARTS, M.MDSI_PARTS) == (len(R.PART_NAMES), len(MR.PART_NAMES))
