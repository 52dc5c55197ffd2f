"""The weight-gradient planner (mtd-gan_amd/csrc/conv_wgrad_plan.h) pinned on the CPU: tests/wgrad_plan_dump.cpp, compiled with g++
under the address and undefined-behaviour sanitizers, prints the plan of every layer shape of a fixed grid -- kernel, tile shape,
pixel split, waves, for one launch and for one half of a pair launch, the pair plan under the three pair modes, the half_scale
answer and the workspace -- under the default rule and under every override.  tests/golden/wgrad_plans.csv is that output from
the planner as it was before it moved into the header; a change of plan shows up as changed rows (the header of the dump
program says how to regenerate the table when that is the purpose).  The built library's query entry points, which need no
device, must give the same answers, and kernels.WGRAD_CFG_* / WGRAD_CONFIGS the same numbers and names."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "wgrad_plans.csv")
FAKE = 4096          # a non-null, 16-byte aligned address that is never dereferenced
K1, K3, K3T, K4S2 = range(4)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """Runs the dump program in its three modes; the environment is emptied so that no MTD_* variable of the caller reaches it."""
    exe = tmp_path_factory.mktemp("wgrad_plan") / "wgrad_plan_dump"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DMTD_LAB", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "wgrad_plan_dump.cpp"), "-o", str(exe)], check=True)

    def run(*mode):
        r = subprocess.run([str(exe), *mode], env={}, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr          # a sanitizer report is a non-zero exit and text on stderr
        return r.stdout.splitlines()
    return {"rows": run() + run("lab"), "names": run("names")}


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        lines = f.read().splitlines()
    cols = lines[0].split(",")
    rows = [dict(zip(cols, [ln.split(",")[0]] + [int(v) for v in ln.split(",")[1:]])) for ln in lines[1:]]
    assert all(len(ln.split(",")) == len(cols) for ln in lines)
    return rows


def test_plans_are_the_golden_table(dump):
    with open(GOLDEN) as f:
        golden = f.read().splitlines()
    assert len(dump["rows"]) == len(golden)
    for got, want in zip(dump["rows"], golden):
        assert got == want
    assert os.path.getsize(GOLDEN) <= 64 * 1024


def test_grid_reaches_every_plan(table):
    default = [r for r in table if r["mode"] == "D" and (r["fcfg"], r["fsplit"]) == (-1, -1)]
    assert {r["cfg"] for r in default} == {0, 1, 2, 4, 5, 7, 8, 9, 10, 11, 12, 13, 15, 16, 18, 19}
    assert {r["cfg"] for r in table} >= {3, 6}                                           # by override only
    assert {r["kind"] for r in default} == {K1, K3, K3T, K4S2}
    assert {r["H"] for r in default} >= {1, 2, 4, 6, 8, 12, 16, 32, 64} and any(r["H"] != r["W"] for r in default)
    assert {r["N"] for r in default} == {r["C"] for r in default} == {32, 64, 96, 128, 192, 256, 512, 1024}
    assert any(r["N"] != r["C"] for r in default) and {r["B"] for r in default} == {1, 2, 4, 16, 32, 64}
    # every override the planner reacts to, one it ignores, and forced slice counts
    assert {r["fcfg"] for r in table} == {-2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 13, 15, 16, 18, 19} and {r["fsplit"] for r in table} == {-1, 1, 3, 1000}
    # one half of a pair launch is planned differently, and every kind of pair plan occurs
    assert any((r["ppw"], r["nsplit"]) != (r["ppw2"], r["nsplit2"]) for r in default)
    assert {r["p1cfg"] for r in default if r["p1ok"]} == {15, 16, 18} and {r["p2cfg"] for r in default if r["p2ok"]} == {16, 18}
    assert {r["p3cfg"] for r in default if r["p3ok"]} >= {1, 2, 4, 5, 10, 11, 12, 13, 15, 16, 18}
    assert {r["half"] for r in default} == {0, 1}
    # a Winograd-eligible layer with fewer than two slices falls through to the kernels below (reachable only with the lab
    # switches that lower the minimum map side: the rows of mode L)
    lab = {(r["kind"], r["B"], r["H"]): r["cfg"] for r in table if r["mode"] == "L"}
    assert lab[(K3, 1, 2)] == 12 and lab[(K3, 1, 4)] == 11 and lab[(K3, 1, 6)] == 16
    assert lab[(K4S2, 1, 2)] == 13 and lab[(K4S2, 2, 6)] == 13


# ------------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    A = ctypes.POINTER(_lib.WgradArgs)
    for name, res, args in (("mtd_conv_wgrad_plan_cfg", ctypes.c_int, [A]), ("mtd_conv_wgrad_ws_bytes", ctypes.c_size_t, [A]),
                            ("mtd_conv_wgrad_half_scale_ok", ctypes.c_int, [A]), ("mtd_conv_wgrad_pair_ok", ctypes.c_int, [A, ctypes.c_int]),
                            ("mtd_conv_wgrad_pair_ws_bytes", ctypes.c_size_t, [A, ctypes.c_int]),
                            ("mtd_conv_wgrad_override", ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
                            ("mtd_conv_wgrad_pair_mode", ctypes.c_int, [ctypes.c_int])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    yield L
    L.mtd_conv_wgrad_override(-1, -1)
    L.mtd_conv_wgrad_pair_mode(-1)


def _args(r):
    from mtd_gan_amd import _lib, kernels as K
    B, H, W = r["B"], r["H"], r["W"]
    a = _lib.WgradArgs()
    a.g = {K1: lambda: K.geom_fwd(B, H, W, 1, 1, 0), K3: lambda: K.geom_fwd(B, H, W, 3, 1, 1), K3T: lambda: K.geom_dgrad_s1(B, H, W, 3, 1),
           K4S2: lambda: K.geom_fwd(B, 2 * H, 2 * W, 4, 2, 1)}[r["kind"]]()
    assert (a.g.OH, a.g.OW) == (H, W)
    T = a.g.TH * a.g.TW
    a.p, a.p_ld, a.N = FAKE, r["N"], r["N"]
    a.q, a.q_ld, a.C = FAKE, r["C"], r["C"]
    a.dw, a.w_sn, a.w_sc = FAKE, r["C"] * T, T
    return a


def test_library_queries_agree_with_the_table(built_lib, table):
    L = built_lib
    assert L.mtd_lab_build() == 0
    for r in table:
        if r["mode"] != "D":              # (the lab rows need a -DMTD_LAB library)
            continue
        a = _args(r)
        L.mtd_conv_wgrad_override(r["fcfg"], r["fsplit"])
        assert L.mtd_conv_wgrad_plan_cfg(ctypes.byref(a)) == r["cfg"], r
        assert L.mtd_conv_wgrad_ws_bytes(ctypes.byref(a)) == 4 * r["ws"], r
        for mode in (1, 2, 3):
            L.mtd_conv_wgrad_pair_mode(mode)
            assert L.mtd_conv_wgrad_pair_ok(ctypes.byref(a), r["B"] // 2) == r[f"p{mode}ok"], (mode, r)
            assert L.mtd_conv_wgrad_pair_ws_bytes(ctypes.byref(a), r["B"] // 2) == 4 * r[f"p{mode}ws"], (mode, r)
        a.half_scale = a.half_scale2 = FAKE
        a.m_first = 32
        assert L.mtd_conv_wgrad_half_scale_ok(ctypes.byref(a)) == r["half"], r
    L.mtd_conv_wgrad_override(-1, -1)
    L.mtd_conv_wgrad_pair_mode(-1)


def test_python_plan_numbers_are_the_table_of_the_header(dump):
    from mtd_gan_amd import kernels as K
    names = [ln.split(",", 1) for ln in dump["names"]]
    assert [int(i) for i, _ in names] == list(range(len(names)))
    assert [n for _, n in names] == K.WGRAD_CONFIGS
    assert K.WGRAD_CONFIGS[K.WGRAD_CFG_WINO] == "wgrad_wino_kernel" and K.WGRAD_CONFIGS[K.WGRAD_CFG_WINO_S2] == "wgrad_wino_s2_kernel"
    assert K.WGRAD_CONFIGS[K.WGRAD_CFG_WINO32] == "wgrad_wino32_kernel"
