"""Host side of FID's InceptionV3 feature network (metrics.InceptionV3Features, inception.py) without a GPU: the state-dict
contract, the BatchNorm fold, the layer table against the restatement the GPU tests compare with (tests/_inception_ref.py), the
refusals of the new entry points and compute_feat's single-channel route."""
import os
import re

import pytest
import torch

import _inception_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mtd_resize_bilinear", "mtd_pool3x3", "mtd_global_avgpool")
EINVAL = -1


@pytest.fixture(scope="module")
def state():
    return R.seeded_state_dict(0)


@pytest.fixture(scope="module")
def net(state):
    from mtd_gan_amd.metrics import InceptionV3Features
    return InceptionV3Features(state)


@pytest.fixture(scope="module")
def cpu_lib():
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    return _lib.lib()


def test_state_dict_validation_names_the_key(state, net):
    from mtd_gan_amd.metrics import InceptionV3Features
    assert any(k.startswith("fc.") for k in state) and any(k.startswith("AuxLogits.") for k in state)       # accepted above, ignored
    key = "Mixed_6c.branch7x7dbl_3.bn.running_var"
    with pytest.raises(ValueError, match=re.escape(key)):
        InceptionV3Features({k: v for k, v in state.items() if k != key})
    wrong = dict(state)
    wrong["Mixed_7a.branch7x7x3_2.conv.weight"] = torch.zeros(192, 192, 7, 1)
    with pytest.raises(ValueError, match=r"Mixed_7a\.branch7x7x3_2\.conv\.weight"):
        InceptionV3Features(wrong)
    wrong = dict(state)
    wrong["Conv2d_3b_1x1.bn.bias"] = torch.zeros(96)
    with pytest.raises(ValueError, match=r"Conv2d_3b_1x1\.bn\.bias"):
        InceptionV3Features(wrong)


def test_state_dict_from_a_file(tmp_path, state, net):
    from mtd_gan_amd.metrics import InceptionV3Features
    path = tmp_path / "pt_inception.pth"
    torch.save(state, path)
    again = InceptionV3Features(str(path), resize_input=False)
    assert all(torch.equal(again.layers[n].weight, net.layers[n].weight) and torch.equal(again.layers[n].bias, net.layers[n].bias) for n in net.layers)
    assert again.takes_single_channel is True and not again.resize_input and again.normalize_input


def test_batchnorm_fold_is_the_float64_formula(state, net):
    from mtd_gan_amd import inception as I
    for name, (cin, cout, _k, _s, _p) in R.all_layers().items():
        w, g, b, m, v = (state[f"{name}.{leaf}"].double() for leaf in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"))
        root = (v + 1e-3).sqrt()
        wf = (w * g[:, None, None, None] / root[:, None, None, None]).float()
        bf = (b - m * g / root).float()
        L = net.layers[name]
        assert L.weight.dtype == torch.float32 and L.bias.dtype == torch.float32
        assert torch.equal(L.weight[:cout, :cin], wf), name
        assert torch.equal(L.bias[:cout], bf), name
    # ... and folded is the same function as conv -> BatchNorm, in float64
    name, spec = "Mixed_6b.branch7x7_2", R.all_layers()["Mixed_6b.branch7x7_2"]
    x = torch.randn(1, 128, 9, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    wf, bf = I.fold_batchnorm(*(state[f"{name}.{leaf}"] for leaf in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")))
    folded = torch.relu(torch.nn.functional.conv2d(x, wf, bf, padding=spec[4]))
    assert (folded - R.layer(state, name, spec, x)).abs().max().item() < 1e-12


def test_first_layer_is_folded_to_one_channel(net):
    L = net.layers["Conv2d_1a_3x3"]
    assert tuple(L.weight.shape) == (32, 3, 3, 3) and len(L.single) == 1
    w1 = L.single[0][0]
    assert tuple(w1.shape) == (32, 1, 3, 3) and w1.dtype == torch.float32
    assert (w1.double() - L.weight.double().sum(dim=1, keepdim=True)).abs().max().item() < 1e-6
    assert all(net.layers[n].single is None for n in net.layers if n != "Conv2d_1a_3x3")


def test_table_matches_the_restatement():
    from mtd_gan_amd import inception as I
    two = lambda v: v if isinstance(v, tuple) else (v, v)
    ref = {n: (ci, co, two(k), two(s), two(p)) for n, (ci, co, k, s, p) in R.all_layers().items()}
    assert len(I.CONVS) == 94 and list(I.CONVS) == list(ref)
    assert I.CONVS == ref
    assert [I.block_width(n) for n in I.BLOCKS] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    assert {n: I.block_width(n) for n in I.BLOCKS} == R.WIDTHS
    # the blocks' pools: the average without the padding everywhere but in Mixed_7c
    pools = {n: [op for chain, ends in br for op in chain + ends if not isinstance(op, str)] for n, (_c, br) in I.BLOCKS.items()}
    assert pools["Mixed_7b"] == [I.POOL_AVG_S1P1] and pools["Mixed_7c"] == [I.POOL_MAX_S1P1]
    assert pools["Mixed_6a"] == [I.POOL_MAX_S2] and pools["Mixed_7a"] == [I.POOL_MAX_S2]
    assert all(pools[n] == [I.POOL_AVG_S1P1] for n in pools if n[:7] in ("Mixed_5", "Mixed_6") and n != "Mixed_6a")
    assert [s for s in I.NET if s[0] == "pool"] == [("pool", I.POOL_MAX_S2)] * 2
    assert I.InceptionV3Features._largest_map_bytes((299, 299)) == 147 * 147 * 64 * 4
    assert I.InceptionV3Features._largest_map_bytes((74, 299)) == 0 and I.InceptionV3Features._largest_map_bytes((75, 75)) > 0


def test_padded_lanes_are_exact_zeros(net):
    from mtd_gan_amd import inception as I
    assert (I.padded(48), I.padded(80), I.padded(3), I.padded(1), I.padded(288)) == (64, 96, 3, 1, 288)
    seen = 0
    for name, (cin, cout, k, _s, _p) in I.CONVS.items():
        L = net.layers[name]
        assert tuple(L.weight.shape) == (I.padded(cout), I.padded(cin)) + k and tuple(L.bias.shape) == (I.padded(cout),)
        if cout in (48, 80):        # producer side: zero rows and zero bias, so relu(...) leaves exact zeros in the lanes
            assert (L.weight[cout:] == 0).all() and (L.bias[cout:] == 0).all() and L.weight[:cout].abs().sum() > 0
            seen += 1
        if cin in (48, 80):         # consumer side: zero input-channel weights
            assert (L.weight[:, cin:] == 0).all() and L.weight[:, :cin].abs().sum() > 0
            seen += 1
        assert sum(r1 - r0 for _w, (r0, r1) in L.parts) == k[0] and all(w.shape[2] * w.shape[3] <= I.MAX_TAPS for w, _r in L.parts)
        assert torch.equal(torch.cat([w for w, _r in L.parts], dim=2), L.weight)
    assert seen == 8                # branch5x5_1 / _2 of three A blocks, Conv2d_3b_1x1 / Conv2d_4a_3x3
    assert [r for _w, r in net.layers["Mixed_5b.branch5x5_2"].parts] == [(0, 3), (3, 5)]


def test_rect_geometry():
    from mtd_gan_amd import kernels as K
    g = K.geom_fwd_rect(2, 17, 19, (1, 7), (1, 1), (0, 3))
    assert (g.B, g.IH, g.IW, g.OH, g.OW, g.TH, g.TW, g.KW, g.off_y, g.off_x, g.in_sy, g.in_sx) == (2, 17, 19, 17, 19, 1, 7, 7, 0, -3, 1, 1)
    g = K.geom_fwd_rect(1, 9, 8, (3, 3), (2, 2))
    assert (g.OH, g.OW, g.OHF, g.OWF, g.in_sy, g.in_sx, g.off_y, g.off_x) == (4, 3, 4, 3, 2, 2, 0, 0)
    g = K.geom_fwd_rect(1, 9, 9, (5, 5), (1, 1), (2, 2), rows=(3, 5))
    assert (g.OH, g.OW, g.TH, g.TW, g.KW, g.off_y, g.off_x, g.ky0) == (9, 9, 2, 5, 5, 1, -2, 0)
    sq = K.geom_fwd(3, 12, 10, 3, 1, 1)
    assert bytes(K.geom_fwd_rect(3, 12, 10, (3, 3), (1, 1), (1, 1))) == bytes(sq)


def test_new_entry_points_are_declared_and_bound():
    from mtd_gan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    declared = set(re.findall(r"\b(mtd_[a-z0-9_]+)\s*\(", hdr))
    for n in ENTRIES:
        assert n in _lib.EXPORTS and n in declared, n
    assert "fid_inception.py" in hdr


def test_entry_points_refuse_bad_arguments_without_a_device(cpu_lib):
    """Null pointers, B <= 0, a leading dimension smaller than the channel count and a bad mode are answered before anything
    touches the device (the pointers below are never dereferenced)."""
    L, p, q = cpu_lib, 4096, 8192
    pool = [p, 32, q, 32, 2, 8, 8, 32, 0, None]                  # in, in_ld, out, out_ld, B, H, W, C, mode, stream
    for i, v in ((0, None), (2, None), (4, 0), (4, -1), (1, 31), (3, 31), (8, 3), (8, -1), (5, 0), (7, 0)):
        bad = list(pool)
        bad[i] = v
        assert L.mtd_pool3x3(*bad) == EINVAL, (i, v)
    assert L.mtd_pool3x3(p, 32, q, 32, 2, 2, 8, 32, 0, None) == EINVAL      # stride-2 pool of a map below 3 rows
    gap = [p, 32, q, 32, 2, 8, 8, 32, None]                      # in, in_ld, out, out_ld, B, H, W, C, stream
    for i, v in ((0, None), (2, None), (4, 0), (1, 31), (3, 31), (5, 0), (7, -4)):
        bad = list(gap)
        bad[i] = v
        assert L.mtd_global_avgpool(*bad) == EINVAL, (i, v)
    rs = [p, 3 * 64, 64, 1, q, 3, 2, 3, 8, 8, 299, 299, 1, None]  # in, in_sb, in_sc, in_sp, out, out_ld, B, C, H, W, OH, OW, normalize, stream
    for i, v in ((0, None), (4, None), (6, 0), (6, -2), (5, 2), (7, 0), (7, 5), (8, 0), (11, 0), (3, 0)):
        bad = list(rs)
        bad[i] = v
        assert L.mtd_resize_bilinear(*bad) == EINVAL, (i, v)


def test_cpu_tensors_are_refused(net):
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 1, 64, 64))
    with pytest.raises(RuntimeError):
        net(torch.zeros(2, 3, 64, 64))
    with pytest.raises(AssertionError):
        net(torch.zeros(1, 2, 64, 64))
    with pytest.raises(AssertionError):
        net(torch.zeros(3, 64, 64))
    # ... and by the pieces a caller can run alone: nothing on the host ever reaches a kernel as a pointer
    from mtd_gan_amd import inception as I
    with pytest.raises(RuntimeError):
        net.run_block("Mixed_5b", torch.zeros(1, 5, 5, 192))
    with pytest.raises(RuntimeError):
        net.conv_layer("Conv2d_2a_3x3", torch.zeros(1, 9, 9, 32))
    L = net.layers["Conv2d_2a_3x3"]
    with pytest.raises(RuntimeError):
        I.conv_relu(torch.zeros(1, 9, 9, 32), L.parts, L.bias, L.k, L.s, L.p)
    for fn in (lambda: I.pool3x3(torch.zeros(1, 8, 8, 32), I.POOL_MAX_S2), lambda: I.global_avgpool(torch.zeros(1, 8, 8, 32)),
               lambda: I.resize_bilinear(torch.zeros(1, 1, 8, 8), (299, 299))):
        with pytest.raises(RuntimeError):
            fn()


def test_compute_feat_routes_by_takes_single_channel():
    from mtd_gan_amd import metrics as M
    g = torch.Generator().manual_seed(5)
    x, y, p = (torch.rand(2, 1, 6, 4, generator=g) for _ in range(3))

    class Recorder:
        def __init__(self):
            self.seen = []

        def __call__(self, t):
            self.seen.append(t)
            return t.mean(dim=(2, 3))

    plain = Recorder()                                           # a plain callable: x.repeat(1, 3, 1, 1), as ever
    out = M.compute_feat(x, y, p, extractor=plain)
    assert [tuple(t.shape) for t in plain.seen] == [(2, 3, 6, 4)] * 3
    assert all(torch.equal(t, s.repeat(1, 3, 1, 1)) for t, s in zip(plain.seen, (x, y, p)))
    assert [tuple(f.shape) for f in out] == [(2, 3)] * 3
    for flag in (False, 1, "yes"):                               # only the literal True opts in
        other = Recorder()
        other.takes_single_channel = flag
        M.compute_feat(x, y, p, extractor=other)
        assert [tuple(t.shape) for t in other.seen] == [(2, 3, 6, 4)] * 3
    single = Recorder()
    single.takes_single_channel = True
    out = M.compute_feat(x, y, p, extractor=single)
    assert all(t is s for t, s in zip(single.seen, (x, y, p)))
    assert [tuple(f.shape) for f in out] == [(2, 1)] * 3
    assert M.InceptionV3Features.takes_single_channel is True
