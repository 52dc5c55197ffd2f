"""The planners of the forward and data-gradient convs (mtd-gan_amd/csrc/conv_plan.h) pinned on the CPU: tests/conv_plan_dump.cpp,
compiled with g++ under the address and undefined-behaviour sanitizers, prints for every layer shape of a fixed grid what the
three planners answer -- the implicit-GEMM route, tile and split of K of a single launch and of the multi form, the derived
launch flags; the Winograd form, workgroup shape, split and group answers; the stride-2 Winograd form -- under the default rule
and under every override.  tests/golden/conv_plans_{igemm,wino,s2}.csv are that output from the planners as they were before
they moved into the header; a change of plan shows up as changed rows (the header of the dump program says how to regenerate a
table when that is the purpose).  The built library's query entry points, which need no device, must give the same answers, and
kernels.IGEMM_CONFIGS the header's names."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TABLES = ("igemm", "wino", "s2")
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced
K1, K3, K3T, K4S2, KDG = range(5)
V_OUT4, V_WS4, V_BIAS4, V_MASK, V_MASK4, V_ADD1, V_OUT2, V_RELU_ADD, V_CTR, V_LD2 = (1 << i for i in range(10))
EINVAL = -1


def _golden(name):
    return os.path.join(HERE, "golden", f"conv_plans_{name}.csv")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """Runs the dump program in every mode, the default rows and the lab rows in processes of their own; the environment is
    emptied so that no MTD_* variable of the caller reaches it."""
    exe = tmp_path_factory.mktemp("conv_plan") / "conv_plan_dump"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DMTD_LAB", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "conv_plan_dump.cpp"), "-o", str(exe)], check=True)

    def run(*mode):
        r = subprocess.run([str(exe), *mode], env={}, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr          # a sanitizer report is a non-zero exit and text on stderr
        return r.stdout.splitlines()
    return {"igemm": run("igemm") + run("igemm", "lab"), "wino": run("wino"), "s2": run("s2"), "names": run("names")}


@pytest.fixture(scope="module")
def tables():
    out = {}
    for name in TABLES:
        with open(_golden(name)) as f:
            lines = f.read().splitlines()
        cols = lines[0].split(",")
        assert all(len(ln.split(",")) == len(cols) for ln in lines)
        out[name] = [dict(zip(cols, [ln.split(",")[0]] + [int(v) for v in ln.split(",")[1:]])) for ln in lines[1:]]
    return out


@pytest.mark.parametrize("name", TABLES)
def test_plans_are_the_golden_table(dump, name):
    with open(_golden(name)) as f:
        golden = f.read().splitlines()
    assert len(dump[name]) == len(golden)
    for got, want in zip(dump[name], golden):
        assert got == want
    assert os.path.getsize(_golden(name)) <= 64 * 1024


def test_grid_reaches_every_rule(tables):
    ig = tables["igemm"]
    default = [r for r in ig if r["mode"] == "D" and (r["fcfg"], r["fsplit"], r["var"]) == (-1, -1, 0)]
    M = lambda r: r["B"] * r["H"] * r["W"]                                                                       # noqa: E731
    # the tile rules of a single launch; down1 (16 taps, 64 -> 64) at 65536 and 32768 pixels; the four-class data gradients
    assert {r["cfg"] for r in default if r["kind"] != K4S2} >= {0, 1, 3, 6}
    down1 = {M(r): (r["cfg"], r["splitk"]) for r in default if r["kind"] == K4S2 and r["N"] == r["C"] == 64}
    assert down1[65536] == (2, 1) and down1[32768] == (3, 1)
    assert {r["mcfg"] for r in default if r["kind"] == KDG and r["sets"] == 4 and r["msplitk"] == 1 and r["mroute"] >= 16} >= {0, 1, 2}
    # the routes: halo tiles, the persistent kernel, a tile kernel, the refusals (a second output, RELU_ADD off the persistent
    # kernel), single launches and the multi form
    assert {r["route"] for r in default} >= {0, 1, 2, 3, 6, 9, 10}
    assert {r["mroute"] for r in default if r["sets"] > 1} >= {1, 6, 9, 10, 16, 17, 18, 19}
    refused = {r["var"] for r in ig if r["route"] == EINVAL}
    assert V_RELU_ADD in refused and V_OUT2 in refused and (V_RELU_ADD | V_MASK) in refused
    assert any(r["route"] == 9 and r["var"] == V_RELU_ADD for r in ig) and any(r["route"] == 10 and r["var"] == V_OUT2 | V_MASK for r in ig)
    assert {(r["relu"], r["tail"]) for r in ig} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # every override with every slice count; cfgs 4, 5, 7, 8 occur by override only
    assert {(r["fcfg"], r["fsplit"]) for r in ig} >= {(c, s) for c in range(-1, 11) for s in (-1, 1, 3, 1000)}
    assert {r["cfg"] for r in ig if r["fcfg"] >= 0} >= {4, 5, 7, 8} and not {r["cfg"] for r in default} & {4, 5, 7, 8}
    # pixel counts on both sides of every threshold, every channel count, maps that are not square or no multiple of 4 wide
    assert {M(r) for r in default} >= {2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144}
    assert {r["N"] for r in default} == {r["C"] for r in default} == {32, 64, 128, 256, 512} and {r["sets"] for r in default} == {1, 2, 3, 4}
    assert {r["kind"] for r in default} == {K1, K3, K3T, K4S2, KDG} and any(r["H"] != r["W"] for r in default) and any(r["W"] % 4 for r in default)
    # the derived flags: both bits of `wide`, the in-kernel finish in both forms, splits up to the cap's neighbourhood
    assert {r["wide"] for r in ig} == {0, 1, 2, 3} and {r["fin"] for r in ig} == {0, 1, 2} and {r["splitk"] for r in ig} >= {1, 2, 3, 4, 8, 16}
    # the lab rows: round 2's tiles and the unsplit grids of exactly 256 workgroups
    lab = {(r["N"], r["C"], r["B"]): (r["cfg"], r["splitk"]) for r in ig if r["mode"] == "L" and r["sets"] == 1}
    assert lab[(256, 64, 4)] == (2, 1) and lab[(128, 128, 4)] == (7, 1) and lab[(256, 128, 1)] == (6, 1) and lab[(256, 512, 1)] == (6, 2)

    w = [r for r in tables["wino"] if r["ok"]]
    assert {r["nb"] for r in w} == {1, 2, 4} and {r["lean"] for r in w} == {0, 1} and {r["px"] for r in w} == {4, 6, 20, 22}
    assert max(r["splitk"] for r in w) > 1 and {r["xcd"] for r in w} == {1, 2} and {(r["g2"], r["g3"]) for r in w} == {(0, 0), (1, 1)}
    assert {r["var"] for r in w if r["c32"]} >= {0, V_ADD1, V_MASK, V_MASK | V_ADD1, V_MASK | V_OUT2}      # the persistent 32 -> 32 kernel
    assert any(r["N"] == 32 and not r["c32"] and r["nb"] == 1 for r in w)                                   # ... and a layer it refuses
    assert any(not r["ok"] for r in tables["wino"]) and {r["f4"] for r in w} == {0, 8} and {r["wsplit"] for r in w} == {0, 1}

    s = [r for r in tables["s2"] if r["elig"]]
    assert {r["groups"] for r in s} == {1, 4} and {r["nb"] for r in s} == {2, 4} and {r["lean"] for r in s} == {0, 1}
    assert {(r["groups"], r["pays"]) for r in s} == {(1, 0), (1, 1), (4, 0), (4, 1)} and {r["sets"] for r in s} == {1, 2, 3, 4}
    assert any(not r["elig"] for r in tables["s2"]) and max(r["splitk"] for r in s) > 1


# ------------------------------------------------------------------------------------------------------- the library
def _geom(r, cls=0):
    from mtd_gan_amd import kernels as K
    B, H, W = r["B"], r["H"], r["W"]
    g = {K1: lambda: K.geom_fwd(B, H, W, 1, 1, 0), K3: lambda: K.geom_fwd(B, H, W, 3, 1, 1), K3T: lambda: K.geom_dgrad_s1(B, H, W, 3, 1),
         K4S2: lambda: K.geom_fwd(B, 2 * H, 2 * W, 4, 2, 1), KDG: lambda: K.geom_dgrad_s2(B, 2 * H, 2 * W, cls >> 1, cls & 1)}[r["kind"]]()
    assert (g.OH, g.OW) == (H, W)
    return g


def _fill(a, r, cls=0):
    """The arguments of a row, as args_of() of the dump program builds them."""
    N, Cc, var = r["N"], r["C"], r["var"]
    a.g = _geom(r, cls)
    a.inp, a.in_ld, a.C = FAKE, Cc, Cc
    a.w, a.w_sn, a.w_sc, a.w_st, a.N = FAKE, Cc, 1, N * Cc, N
    a.out, a.out_ld = FAKE + (4 if var & V_OUT4 else 0), N + (2 if var & V_LD2 else 0)
    a.ws, a.ws_bytes = FAKE + (4 if var & V_WS4 else 0), 1 << 40
    if var & V_BIAS4:
        a.bias = FAKE + 4
    if var & V_MASK:
        a.mask, a.mask_ld = FAKE + (4 if var & V_MASK4 else 0), N
    if var & V_ADD1:
        a.add1, a.add1_ld = FAKE, N
    if var & V_OUT2:
        a.out2, a.out2_ld = FAKE, N
    if var & V_RELU_ADD:
        a.act = 3
    if var & V_CTR:
        a.tile_ctr, a.tile_ctr_len = FAKE, 1 << 20


def _sets(r, n, same=True, w_st=None):
    from mtd_gan_amd import _lib
    arr = (_lib.ConvArgs * n)()
    for i in range(n):
        _fill(arr[i], r, 0 if same else i)
        if w_st is not None:
            arr[i].w_st = w_st
    return arr


def check_library(L, tables):
    """The device-free exports of library L against the tables' default rows, under every override; the overrides are reset."""
    A, ci, cz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    for name, res, args in (("mtd_conv_igemm_ws_bytes", cz, [A]), ("mtd_conv_igemm_multi_ws_bytes", cz, [A, ci]), ("mtd_conv_relu_add_ok", ci, [A]),
                            ("mtd_resfft_block_tail_ok", ci, [A]), ("mtd_conv_winograd_ok", ci, [A]), ("mtd_conv_winograd_patch_w", ci, [A]),
                            ("mtd_conv_winograd_ws_bytes", cz, [A]), ("mtd_conv_winograd_group_ok", ci, [A, ci]), ("mtd_conv_winograd_s2_ok", ci, [A, ci]),
                            ("mtd_conv_winograd_s2_ws_bytes", cz, [A, ci]), ("mtd_conv_igemm_override", ci, [ci, ci]),
                            ("mtd_conv_winograd_f4_min_w", ci, [ci]), ("mtd_set_option", ci, [ctypes.c_char_p, ci]),
                            ("mtd_get_option", ci, [ctypes.c_char_p, ctypes.POINTER(ci)])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    assert L.mtd_lab_build() == 0
    old_min_w, old_split = L.mtd_conv_winograd_f4_min_w(-1), ci(-1)
    assert old_min_w == 8 and L.mtd_get_option(b"wino_split", ctypes.byref(old_split)) == 0
    try:
        for r in tables["igemm"]:
            if r["mode"] != "D":              # (the lab rows need a -DMTD_LAB library)
                continue
            L.mtd_conv_igemm_override(r["fcfg"], r["fsplit"])
            a = _sets(r, r["sets"])
            assert L.mtd_conv_igemm_ws_bytes(a) == r["ws"], r
            assert L.mtd_conv_igemm_multi_ws_bytes(a, r["sets"]) == r["mws"], r
            assert L.mtd_conv_relu_add_ok(a) == r["relu"], r
            assert L.mtd_resfft_block_tail_ok(a) == r["tail"], r
        L.mtd_conv_igemm_override(-1, -1)
        for r in tables["wino"]:
            assert L.mtd_conv_winograd_f4_min_w(r["f4"]) >= 0 and L.mtd_set_option(b"wino_split", r["wsplit"]) == 0
            a = _sets(r, 3)
            assert L.mtd_conv_winograd_ok(a) == r["ok"], r
            assert L.mtd_conv_winograd_patch_w(a) == r["px"], r
            a = _sets(r, 3, w_st=r["px"])        # the launch: the form the weights were built for travels in w_st
            assert L.mtd_conv_winograd_ws_bytes(a) == r["ws"], r
            assert L.mtd_conv_winograd_group_ok(a, 2) == r["g2"] and L.mtd_conv_winograd_group_ok(a, 3) == r["g3"], r
        for r in tables["s2"]:
            a = _sets(r, 4, same=False)
            assert L.mtd_conv_winograd_s2_ok(a, r["sets"]) == (1 + r["pays"] if r["elig"] else 0), r
            assert L.mtd_conv_winograd_s2_ws_bytes(a, r["sets"]) == r["ws"], r
    finally:
        L.mtd_conv_igemm_override(-1, -1)
        L.mtd_conv_winograd_f4_min_w(old_min_w)
        L.mtd_set_option(b"wino_split", old_split.value)


def test_library_queries_agree_with_the_tables(tables):
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    check_library(ctypes.CDLL(_lib.LIB_PATH), tables)


def test_python_kernel_names_are_the_table_of_the_header(dump, tables):
    from mtd_gan_amd import kernels as K
    names = [ln.split(",", 1) for ln in dump["names"]]
    assert [int(i) for i, _ in names] == list(range(len(names))) and len(names) == 40
    assert [n for _, n in names] == K.IGEMM_CONFIGS
    assert K.IGEMM_CONFIGS[K.IGEMM_CFG_C32P] == "igemm_c32p_kernel" and K.IGEMM_CONFIGS[K.IGEMM_CFG_C32T] == "igemm_c32t_kernel"
    assert K.IGEMM_CONFIGS[K.IGEMM_CFG_128x32] == "igemm_kernel<1, 1, 4, 1>" and K.IGEMM_CONFIGS[K.IGEMM_CFG_32x128] == "igemm_kernel<1, 1, 1, 4>"
    assert [K.IGEMM_CONFIGS[c] for c in (K.IGEMM_CFG_TB_128x32, K.IGEMM_CFG_TB_256x32)] == ["igemm_tb_kernel<1>", "igemm_tb_kernel<2>"]
    # the tile shapes: the rows of the igemm table that an override put on tile kernel 0 .. 8
    forced = {r["cfg"]: (r["BM"], r["BN"]) for r in tables["igemm"] if r["fcfg"] == r["cfg"]}
    assert [forced[c] for c in range(K.IGEMM_CFG_TILES)] == list(zip(K.IGEMM_TILE_BM, K.IGEMM_TILE_BN))
