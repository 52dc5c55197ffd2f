"""CPU side of tests/test_direct_conv_gpu.py: its case tables reach every kernel and every launch-shape edge of csrc/conv_direct.hip
that they claim, proved from the planners restated in tests/_direct_plan.py; the restated weight-gradient plan gives the slab count
of the library itself (mtd_conv_wgrad_ws_bytes needs no device); and mtd_conv_direct / mtd_conv_wgrad_ws_bytes refuse what they
have to before anything is launched.

REDCNN's 5 x 5 layers: none of these kernels, and no other.  mtd_conv_direct's fast paths and mtd_conv_wgrad take at most 16 taps
(T <= 16; check_wargs refuses more), and only direct_fwd_kernel would loop over 25.  Nothing sends it such a launch:
REDCNN_Generator.forward raises NotImplementedError unless the module was built as (1, 32, 10, 3, 1) -- the ablation wrappers'
3 x 3, 32-channel, padding-1 configuration, whose 1 -> 32 / 32 -> 1 ends run on fwd_c1_tile / fwd_n1_planes / wgrad_wide and whose
32 -> 32 layers are the generator's MFMA kernels.  The class's own defaults (96 channels, kernel 5, padding 0) have no HIP path."""
import ctypes

import pytest

import _direct_plan as plan
import test_direct_conv_gpu as gpu

CONV_LABELS = ["c1_tile_plain_lrelu", "c1_tile_plain_relu", "c1_tile_plain_none", "c1_tile_general", "c1", "n1_planes_1", "n1_planes_2",
               "n1_planes_4", "n1", "generic"]
WGRAD_LABELS = ["wide_tile_fast", "wide_tile_general", "wide_gather", "dwgrad_1", "dwgrad_2", "dwgrad_8"]


def _conv_plans():
    """[(case, plan)] over every launch of every conv case."""
    return [(c, p) for c in gpu.CONV_CASES for p in gpu.conv_plans(c)]


def _of(label, plans=None):
    return [(c, p) for c, p in (plans or _conv_plans()) if p["label"] == label]


def _wgrad_plans():
    return [(c, gpu.wgrad_case_plan(c)) for c in gpu.WGRAD_CASES]


# ------------------------------------------------------------------------------------------------------- the case tables
def test_case_ids_are_unique():
    for table in (gpu.CONV_CASES, gpu.WGRAD_CASES):
        ids = [c["id"] for c in table]
        assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("case", gpu.CONV_CASES, ids=[c["id"] for c in gpu.CONV_CASES])
def test_conv_case_lands_on_its_label(case):
    plans = gpu.conv_plans(case)
    assert len(plans) == (4 if case["kind"][0] == "dgrad_s2" else 1)
    for p in plans:
        assert p["refusal"] is None and p["label"] == case["label"], p
    # each slice is wider than its channels, and a multiple of 4 unless the case is about scalar stores
    in_ld, in_off, out_ld, out_off = gpu.conv_lds(case)
    assert in_ld % 4 == 0 and in_ld > case["C"] and in_off + case["C"] <= in_ld
    assert out_ld > case["N"] and out_off > 0 and out_off + case["N"] < out_ld          # guard channels on both sides
    assert out_ld % 4 == 0 or case["id"] in ("c1t_scalar", "c1_full")


@pytest.mark.parametrize("case", gpu.WGRAD_CASES, ids=[c["id"] for c in gpu.WGRAD_CASES])
def test_wgrad_case_lands_on_its_label(case):
    p = gpu.wgrad_case_plan(case)
    assert p["refusal"] is None and p["label"] == case["label"], p
    p_ld, p_off, q_ld, q_off = gpu.wgrad_lds(case)
    assert p_ld % 4 == 0 and p_ld > case["N"] and p_off + case["N"] <= p_ld
    assert q_ld % 4 == 0 and q_ld > case["C"] and q_off + case["C"] <= q_ld


def test_every_kernel_is_reached():
    conv = {p["label"] for _, p in _conv_plans()}
    assert conv == set(CONV_LABELS)
    wgrad = {p["label"] for _, p in _wgrad_plans()}
    assert wgrad == set(WGRAD_LABELS)
    # the data-gradient geometries (reversed taps; placement into a larger map) reach each family that can take them
    kinds = {(p["label"], c["kind"][0]) for c, p in _conv_plans()}
    assert {("c1_tile_plain_none", "dgrad_s1"), ("n1_planes_2", "dgrad_s1"), ("c1", "dgrad_s2"), ("n1", "dgrad_s2"),
            ("generic", "dgrad_s2")} <= kinds
    assert all(not p["identity"] for c, p in _conv_plans() if c["kind"][0] == "dgrad_s2")


def test_tile_kernel_edges():
    tiles = [(c, p) for c, p in _conv_plans() if p["label"].startswith("c1_tile")]
    by_id = {c["id"]: p for c, p in tiles}
    assert {p["R"] for _, p in tiles} >= {1, 2}
    assert (by_id["c1t_r2"]["R_first"], by_id["c1t_r2"]["R"]) == (2, 2)
    assert (by_id["c1t_r3to2"]["R_first"], by_id["c1t_r3to2"]["R"]) == (3, 2)            # one step of the search
    assert (by_id["c1t_r3to1"]["R_first"], by_id["c1t_r3to1"]["R"]) == (3, 1)            # the search falls through to 1
    assert {p["G"] for _, p in tiles} >= {1, 8, 32, 256} and {p["PL"] for _, p in tiles} >= {256, 32, 8, 1}
    assert all(p["nblk"] > 1 for _, p in tiles)
    assert by_id["c1t_r2"]["nblk"] == 16 * 32                                             # tiles of several images in one grid
    # the general epilogue with 16-byte stores and with scalar ones
    general = _of("c1_tile_general", tiles)
    assert {p["vec_store"] for _, p in general} == {True, False}
    assert any(c["add1"] and c["add2"] and c["mask"] for c, _ in general)
    # the pair switch on an image boundary stays on the tile kernel, inside an image it does not
    assert by_id["c1t_pair"]["label"] == "c1_tile_plain_lrelu"
    pair = {c["id"]: c for c in gpu.CONV_CASES}
    assert pair["c1t_pair"]["split"] % (32 * 32) == 0 and 0 < pair["c1t_pair"]["split"] < by_id["c1t_pair"]["M"]
    assert any(p["T"] == 1 for _, p in tiles)


def test_c1_kernel_edges():
    c1 = _of("c1")
    by_id = {c["id"]: (c, p) for c, p in c1}
    assert any(c["W"] % p["PL"] for c, p in c1 if c["kind"] == gpu.FWD3)                   # width no multiple of PL
    assert any(p["T"] == 16 for _, p in c1)
    c, p = by_id["c1_pair_mid"]
    assert c["split"] % (32 * 32) != 0 and 32 * 32 < c["split"] < p["M"]
    c, p = by_id["c1_big"]
    assert p["M"] > 2048 * p["PL"] and p["ppb"] > p["PL"] and p["M"] % p["ppb"] != 0 and p["nblk"] % 8 != 0
    assert sum(1 for c, _ in c1 if c["id"] == "c1_dgrad_s2") == 4
    assert any(not p["vec_store"] and c["add1"] and c["add2"] and c["mask"] for c, p in c1)


def test_n1_kernel_edges():
    n1 = _of("n1")
    by_id = {c["id"]: (c, p) for c, p in n1}
    assert {p["G"] for _, p in n1} >= {1, 2, 8, 64}
    for ident in ("n1_g1", "n1_g2", "n1_g8"):
        c, p = by_id[ident]
        assert p["M"] % p["PPW"] != 0, ident                                             # ragged live lanes
    assert {p["nblk"] % 8 for _, p in n1} >= {1, 7}
    assert by_id["n1_nblk9"][1]["nblk"] == 9 and by_id["n1_nblk23"][1]["nblk"] == 23     # (q, r) = (1, 1) and (2, 7)
    assert any(p["nblk"] < 8 for _, p in n1)                                             # q = 0
    assert any(p["T"] == 16 for _, p in n1)
    c, p = by_id["n1_full"]
    assert c["add1"] and c["add2"] and c["mask"] and c["act"] != "none" and 63 < c["split"] < p["M"] and c["split"] % 63
    c, p = by_id["n1_h12"]
    assert c["C"] == 32 and c["W"] == 64 and c["H"] % 8 != 0


def test_planes_kernel_edges():
    for inst in (1, 2, 4):
        items = _of(f"n1_planes_{inst}")
        assert {p["nblk"] for _, p in items} >= {1, 6}, inst                             # one workgroup; 3 images of 2 tiles
        assert all(p["in_bytes"] < 2 ** 31 and c["C"] == 32 * inst for c, p in items)
    planes = [(c, p) for c, p in _conv_plans() if p["label"].startswith("n1_planes")]
    assert any(p["T"] == 1 for _, p in planes) and any(c["kind"][0] == "dgrad_s1" for c, _ in planes)
    assert any(c["add1"] and c["add2"] and c["mask"] and c["split"] and c["split"] % (16 * 64) == 0 for c, _ in planes)


def test_generic_kernel_edges():
    generic = _of("generic")
    assert any(p["total"] > plan.GENERIC_MAX_BLOCKS * 256 and p["passes"] == 2 for _, p in generic)
    assert {(c["C"], c["N"]) for c, _ in generic} >= {(1, 1), (3, 1), (1, 3), (96, 1), (1, 96), (512, 1)}
    assert {p["vec_loads"] for _, p in generic} == {True, False}
    assert any(c["add1"] and c["add2"] and c["mask"] and c["split"] for c, _ in generic)
    assert any(c["B"] == 5 and (c["H"], c["W"]) == (1, 1) and c["C"] == 512 for c, _ in generic)


def test_wide_kernel_edges():
    plans = _wgrad_plans()
    wide = [(c, p) for c, p in plans if p["label"].startswith("wide")]
    for side in (True, False):
        assert {p["V"] for _, p in wide if p["n_is_one"] == side or p["V"] == 1} >= {1, 4, 32, 128, 256}, side
    assert {p["VEC"] for _, p in wide} == {1, 4}
    fast = [(c, p) for c, p in plans if p["label"] == "wide_tile_fast"]
    assert all(p["T"] == 9 and p["GW"] >= p["step"] and p["ragged"] == 0 for _, p in fast)
    assert any((p["ppb"] // p["step"]) % 4 != 0 for _, p in fast)                        # the four-deep loop ends mid-group
    assert any((p["ppb"] // p["step"]) % 4 == 0 for _, p in fast)
    assert any(p["GW"] == p["step"] for _, p in fast) and any(c["kind"] == gpu.TCONV3 for c, _ in fast)
    general = [(c, p) for c, p in plans if p["label"] == "wide_tile_general"]
    assert any(p["T"] == 1 for _, p in general) and any(p["T"] == 9 and p["GW"] < p["step"] for _, p in general)
    gather = [(c, p) for c, p in plans if p["label"] == "wide_gather"]
    assert any(p["T"] == 16 and not p["n_is_one"] for _, p in gather)
    assert any(p["ragged"] != 0 and (c["H"], c["W"]) == (20, 28) for c, p in gather)
    assert any(not c["db"] for c, _ in gather)
    assert {p["n_is_one"] for _, p in gather} == {True, False}


def test_direct_wgrad_kernel_edges():
    dw = [(c, p) for c, p in _wgrad_plans() if p["label"].startswith("dwgrad")]
    by_id = {c["id"]: (c, p) for c, p in dw}
    assert {p["V"] for _, p in dw} >= {96, 6, 512, 2048}
    assert {(p["label"], p["n_is_one"]) for _, p in dw} >= {("dwgrad_1", True), ("dwgrad_1", False), ("dwgrad_2", True),
                                                            ("dwgrad_8", True), ("dwgrad_8", False)}
    assert by_id["dw_linear"][1]["CH"] == 2 and by_id["dw_2048_n1"][1]["CH"] == 8
    assert any(p["V"] % 4 for _, p in dw) and any(p["V"] < p["VL"] for _, p in dw)       # channel lanes without a channel
    assert any(p["nblk"] > 1 and p["ragged"] for _, p in dw)
    assert {c["db"] for c, _ in dw} == {True, False}
    c, p = by_id["dw_misaligned"]
    assert c["wide_off"] % 4 == 1 and gpu.wgrad_case_plan(dict(c, wide_off=4))["label"] == "wide_tile_fast"
    c, p = by_id["dw_n1_s2"]
    assert c["N"] == 1 and c["kind"] == gpu.FWD4S2
    c, p = by_id["dw_256_k4"]
    assert (p["T"] * p["V"] + p["V"]) * 16 > 48 * 1024


# ------------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.mtd_conv_direct.restype, L.mtd_conv_direct.argtypes = ctypes.c_int, [ctypes.POINTER(_lib.ConvArgs), ctypes.c_void_p]
    L.mtd_conv_wgrad_ws_bytes.restype, L.mtd_conv_wgrad_ws_bytes.argtypes = ctypes.c_size_t, [ctypes.POINTER(_lib.WgradArgs)]
    return L


FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced


def _wgrad_args(case):
    from mtd_gan_amd import _lib
    g, w_sn, w_sc, _, _ = gpu.wgrad_launch(case)
    p_ld, p_off, q_ld, q_off = gpu.wgrad_lds(case)
    a = _lib.WgradArgs()
    a.g = g
    a.p, a.p_ld, a.N = FAKE + 4 * p_off, p_ld, case["N"]
    a.q, a.q_ld, a.C = FAKE + 4 * q_off, q_ld, case["C"]
    a.dw, a.w_sn, a.w_sc = FAKE, w_sn, w_sc
    a.db = FAKE if case["db"] else None
    return a


@pytest.mark.parametrize("case", gpu.WGRAD_CASES, ids=[c["id"] for c in gpu.WGRAD_CASES])
def test_restated_slab_count_is_the_librarys(built_lib, case):
    """mtd_conv_wgrad_ws_bytes = 4 wgrad_ws_floats(mtd_direct_wgrad_nslab): the restated plan has the library's workgroup count, so
    its choice between the wide and the direct kernel, Mw, CL and ppb are the library's for every case."""
    a = _wgrad_args(case)
    assert built_lib.mtd_conv_wgrad_ws_bytes(ctypes.byref(a)) == 4 * plan.wgrad_ws_floats(gpu.wgrad_case_plan(case))


def _conv_args(**change):
    """A valid 32 -> 1 launch (3 x 3, 8 x 8 map) on placeholder pointers, with fields changed."""
    from mtd_gan_amd import _lib, kernels as K
    a = _lib.ConvArgs()
    a.g = K.geom_fwd(1, 8, 8, 3, 1, 1)
    a.inp, a.in_ld, a.C = FAKE, 32, 32
    a.w, a.w_sn, a.w_sc, a.w_st, a.N = FAKE, 288, 9, 1, 1
    a.out, a.out_ld = FAKE, 1
    for name, value in change.items():
        if name.startswith("g_"):
            setattr(a.g, name[2:], value)
        else:
            setattr(a, name, value)
    return a


def test_conv_direct_refuses_before_any_launch(built_lib):
    f = built_lib.mtd_conv_direct
    refusals = [(dict(out2=FAKE, out2_ld=1), plan.EINVAL),
                (dict(act=plan.ACT_RELU_ADD), plan.EINVAL),
                (dict(in_ld=31), plan.EINVAL),
                (dict(in_ld=34), plan.EALIGN),                         # C % 4 == 0: 16-byte loads need in_ld % 4 == 0 ...
                (dict(in_ld=30, C=28), plan.EALIGN),
                (dict(inp=FAKE + 4), plan.EALIGN),                     # ... and an aligned base
                (dict(g_out_oy=1), plan.EINVAL),                       # the last row lands on row 8 of an 8-row map
                (dict(g_OWF=7), plan.EINVAL),
                (dict(g_out_sx=2), plan.EINVAL),
                (dict(out_ld=0), plan.EINVAL),
                (dict(N=0), plan.EINVAL),
                (dict(g_TH=0), plan.EINVAL),
                (dict(w=None), plan.EINVAL)]
    for change, code in refusals:
        a = _conv_args(**change)
        assert f(ctypes.byref(a), None) == code, change
        if "w" in change:
            continue
        # the restatement refuses the same arguments with the same code
        got = plan.conv_plan(a.g, a.N, a.C, a.in_ld, a.out_ld, in_aligned=a.inp % 16 == 0, out_aligned=a.out % 16 == 0, act=a.act,
                             out2=bool(a.out2))
        assert got["refusal"] == code, change
    assert f(None, None) == plan.EINVAL
    ok = _conv_args()
    assert plan.conv_plan(ok.g, 1, 32, 32, 1)["label"] == "n1"         # (the unchanged arguments are a launch: not made here)


def test_wgrad_ws_bytes_refuses_more_than_16_taps(built_lib):
    from mtd_gan_amd import kernels as K
    case = dict(gpu.WGRAD_CASES[0], kind=("fwd", 5, 1, 2))
    a = _wgrad_args(case)
    assert a.g.TH * a.g.TW == 25
    assert built_lib.mtd_conv_wgrad_ws_bytes(ctypes.byref(a)) == 0
    assert plan.wgrad_plan(a.g, a.N, a.C, a.p_ld, a.q_ld)["refusal"] == plan.EINVAL
    for th, tw in ((4, 4), (2, 8), (1, 16)):                             # 16 taps are taken, 17 are not
        a.g = K.geom_fwd(1, 32, 32, 3, 1, 1)
        a.g.TH, a.g.TW = th, tw
        assert built_lib.mtd_conv_wgrad_ws_bytes(ctypes.byref(a)) > 0
    a.g.TH, a.g.TW = 1, 17
    assert built_lib.mtd_conv_wgrad_ws_bytes(ctypes.byref(a)) == 0
    assert built_lib.mtd_conv_wgrad_ws_bytes(None) == 0
