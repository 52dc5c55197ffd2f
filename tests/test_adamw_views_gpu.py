"""mtd_adamw_views -- the AdamW launch that also writes the derived views of the 3x3 weights it updates -- against the three
launches it stands for: mtd_adamw_multi_pre / _dyn, then mtd_winograd_weights and mtd_pack_weights on the updated weights.
Every output buffer bit for bit (torch.equal): parameters, both moments, every Winograd view (F(2x2) and F(2x4), forward and
data-gradient form) and every [tap][n][c] view (both forms)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, C, kh, kw) / (n,): three viewed 3x3 weights between tensors of the plain path -- a bias, a 4x4 stride-2 weight and a tensor
# whose last block is partly empty (2 * 2048 + 77 elements), so that the viewed tensors' blocks start behind a block that ends mid-way
SHAPES = [(64, 64, 3, 3), (64,), (128, 64, 3, 3), (64, 64, 4, 4), (2 * 2048 + 77,), (64, 128, 3, 3)]
GUARD = 64          # floats behind every view buffer that no launch may touch
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def _scalars(step=3, lr=1e-4, wd=5e-4):
    from mtd_gan_amd.optimizers import FusedAdamW
    return FusedAdamW._scalars(dict(betas=(BETA1, BETA2), lr=lr, weight_decay=wd), step)


def _state(dev):
    g = torch.Generator().manual_seed(11)
    out = []
    for s in SHAPES:
        p = torch.randn(s, generator=g)
        grad = torch.randn(s, generator=g) * 0.3
        m = torch.randn(s, generator=g) * 0.1
        v = torch.rand(s, generator=g) * 0.01
        out.append(tuple(t.to(dev) for t in (p, grad, m, v)))
    return out


def _tables(state, dev):
    """(AdamwTensor list, span list, wino descs, pack descs, the view buffers in table order) for one copy of the state"""
    from mtd_gan_amd import _lib as L, kernels as K
    kfwd = K._wino_kmap(K.geom_fwd(1, 8, 8, 3, 1, 1))
    kbwd = K._wino_kmap(K.geom_dgrad_s1(1, 8, 8, 3, 1))
    assert len(kfwd) == 9 and len(kbwd) == 9 and kfwd != kbwd
    tensors, spans, wino, pack, bufs = [], [], [], [], []
    for (p, g, m, v) in state:
        t = L.AdamwTensor()
        t.p, t.g, t.m, t.v, t.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
        tensors.append(t)
        s = L.AdamwViewsSpan()
        if p.dim() == 4 and p.shape[2] == 3:
            n, c = p.shape[0], p.shape[1]
            s.N, s.C, s.wino_first, s.wino_count, s.pack_first, s.pack_count = n, c, len(wino), 4, len(pack), 2
            forms = ((n, c, 9 * c, 9, kfwd), (c, n, 9, 9 * c, kbwd))          # forward view, data-gradient view
            for px in (4, 6):
                for (vn, vc, sn, sc, kmap) in forms:
                    dst = torch.full((4 * px * vn * vc + GUARD,), 7.0, device=dev)
                    d = L.WinoWeightDesc()
                    d.src, d.dst, d.sn, d.sc, d.st, d.N, d.C, d.px = p.data_ptr(), dst.data_ptr(), sn, sc, 1, vn, vc, px
                    for i, k in enumerate(kmap):
                        d.kmap[i] = k
                    wino.append(d)
                    bufs.append(dst)
            for (vn, vc, sn, sc, _k) in forms:
                dst = torch.full((9 * vn * vc + GUARD,), 7.0, device=dev)
                d = L.PackDesc()
                d.src, d.dst, d.N, d.C, d.T, d.sn, d.sc = p.data_ptr(), dst.data_ptr(), vn, vc, 9, sn, sc
                pack.append(d)
                bufs.append(dst)
        spans.append(s)
    return tensors, spans, wino, pack, bufs


@pytest.mark.parametrize("form", ["pre", "dyn"])
def test_fused_launch_equals_the_three_launches_bit_for_bit(hip_lib, form):
    from mtd_gan_amd import _lib as L, kernels as K
    dev = torch.device("cuda")
    lib = L.lib()
    sc = _scalars()
    dyn = torch.tensor(sc, dtype=torch.float32, device=dev)
    ref, fused = _state(dev), _state(dev)
    vp = lambda host: C.cast(host, C.c_void_p)
    # ---- the three launches
    tensors, _spans, wino, pack, bufs_ref = _tables(ref, dev)
    tab, host = K.device_table(tensors, dev)
    if form == "pre":
        K.check(lib.mtd_adamw_multi_pre(tab.data_ptr(), vp(host), len(tensors), BETA1, BETA2, EPS, sc[0], sc[1], sc[2], K.stream_ptr()), "pre")
    else:
        K.check(lib.mtd_adamw_multi_dyn(tab.data_ptr(), vp(host), len(tensors), BETA1, BETA2, EPS, C.c_void_p(dyn.data_ptr()), K.stream_ptr()), "dyn")
    wtab, whost = K.device_table(wino, dev)
    K.check(lib.mtd_winograd_weights(wtab.data_ptr(), vp(whost), len(wino), K.stream_ptr()), "wino")
    ptab, phost = K.device_table(pack, dev)
    K.check(lib.mtd_pack_weights(ptab.data_ptr(), vp(phost), len(pack), K.stream_ptr()), "pack")
    # ---- the one launch
    tensors, spans, wino, pack, bufs = _tables(fused, dev)
    assert len(wino) == 12 and len(pack) == 6
    tab, host = K.device_table(tensors, dev)
    stab, shost = K.device_table(spans, dev)
    wtab, whost = K.device_table(wino, dev)
    ptab, phost = K.device_table(pack, dev)
    K.check(lib.mtd_adamw_views(tab.data_ptr(), vp(host), len(tensors), stab.data_ptr(), vp(shost), wtab.data_ptr(), vp(whost), len(wino),
                                ptab.data_ptr(), vp(phost), len(pack), BETA1, BETA2, EPS,
                                *((sc[0], sc[1], sc[2], None) if form == "pre" else (0.0, 0.0, 0.0, C.c_void_p(dyn.data_ptr()))),
                                K.stream_ptr()), "views")
    torch.cuda.synchronize()
    start = _state(dev)
    differ = lambda a, b: (int((a != b).sum()), float((a - b).abs().max()))
    for i, ((p, g, m, v), (pr, _gr, mr, vr)) in enumerate(zip(fused, ref)):
        print(f"tensor {i} {tuple(p.shape)}: (elements that differ, max |diff|) p {differ(p, pr)} m {differ(m, mr)} v {differ(v, vr)}")
    for i, (a, b) in enumerate(zip(bufs, bufs_ref)):
        print(f"view buffer {i} ({a.numel() - GUARD} floats): {differ(a, b)}")
    for i, ((p, g, m, v), (pr, gr, mr, vr), (p0, _g0, m0, v0)) in enumerate(zip(fused, ref, start)):
        assert not torch.equal(pr, p0) and not torch.equal(mr, m0) and not torch.equal(vr, v0), i      # the reference did update
        assert torch.equal(p, pr) and torch.equal(m, mr) and torch.equal(v, vr) and torch.equal(g, gr), i
    for i, (a, b) in enumerate(zip(bufs, bufs_ref)):
        assert bool((b[:-GUARD] != 7.0).any()) and bool((b[-GUARD:] == 7.0).all()), i
        assert torch.equal(a, b), i


def test_entry_point_refuses_views_that_do_not_fit_their_tensor(hip_lib):
    """The kernel writes views without bounds checks: the entry point must refuse a view of another shape or source, the split
    form, a tile-unaligned tensor and a span that reaches past the view tables -- before anything is launched."""
    from mtd_gan_amd import _lib as L, kernels as K
    dev = torch.device("cuda")
    lib = L.lib()
    vp = lambda host: C.cast(host, C.c_void_p)

    def call(mutate):
        state = _state(dev)
        tensors, spans, wino, pack, bufs = _tables(state, dev)
        mutate(tensors, spans, wino, pack)
        before = [t.clone() for s in state for t in s]
        rc = lib.mtd_adamw_views(K.device_table(tensors, dev)[0].data_ptr(), vp((L.AdamwTensor * len(tensors))(*tensors)), len(tensors),
                                 K.device_table(spans, dev)[0].data_ptr(), vp((L.AdamwViewsSpan * len(spans))(*spans)),
                                 K.device_table(wino, dev)[0].data_ptr(), vp((L.WinoWeightDesc * len(wino))(*wino)), len(wino),
                                 K.device_table(pack, dev)[0].data_ptr(), vp((L.PackDesc * len(pack))(*pack)), len(pack),
                                 BETA1, BETA2, EPS, 1.0, 1e-4, 1.0, None, K.stream_ptr())
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, [t for s in state for t in s]))        # nothing ran
        return rc

    def bad_shape(t, s, w, p): w[0].N = 128
    def bad_src(t, s, w, p): w[1].src = t[2].p
    def split_form(t, s, w, p): w[2].px = 22
    def bad_tap(t, s, w, p): w[3].kmap[4] = 9
    def bad_pack_taps(t, s, w, p): p[0].T = 16
    def past_table(t, s, w, p): s[5].wino_first = 10
    def views_on_plain(t, s, w, p): s[1].wino_count = 1
    def unaligned(t, s, w, p): s[0].N, s[0].C = 32, 128 + 8
    for mutate in (bad_shape, bad_src, split_form, bad_tap, bad_pack_taps, past_table, views_on_plain, unaligned):
        assert call(mutate) != 0, mutate.__name__


def test_optimizer_step_with_views_leaves_current_views_in_the_cache(hip_lib):
    """FusedAdamW.step(views=...) against step() followed by prepack_winograd / prepack: same parameters, same view contents, and
    the fused step leaves nothing for the two prepack calls to do (they launch nothing: the cache holds the views as current)."""
    from mtd_gan_amd import kernels as K
    from mtd_gan_amd.optimizers import FusedAdamW
    dev = torch.device("cuda")

    def run(fused, graph_mode):
        g = torch.Generator().manual_seed(5)
        ws = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in ((64, 64, 3, 3), (64,), (128, 64, 3, 3), (64, 64, 4, 4))]
        opt = FusedAdamW(ws, lr=1e-3, weight_decay=5e-4)
        opt.graph_mode = graph_mode
        wino, pack = [], []
        for w in (ws[0], ws[2]):
            n, c = w.shape[0], w.shape[1]
            for r in (64, 2):             # a map that takes F(2x4) and one that takes F(2x2)
                wino.append((w, n, c, 9 * c, 9, K.geom_fwd(1, r, r, 3, 1, 1)))
                wino.append((w, c, n, 9, 9 * c, K.geom_dgrad_s1(1, r, r, 3, 1)))
            pack += [(w, n, c, 9 * c, 9), (w, c, n, 9, 9 * c)]
        pack.append((ws[3], 64, 64, 64 * 16, 16))              # a 4x4 view: never the fused launch's
        out = None
        for _step in range(2):
            for w in ws:
                w.grad = torch.randn(w.shape, generator=g).to(dev)
            opt.step(views=(wino, pack)) if fused else opt.step()
            misses = K.STATS["table_miss"]
            cached = len(K._pack_cache)
            K.prepack_winograd(wino)
            K.prepack(pack)
            if fused and _step == 1:       # (step 0 uploaded the 4x4 view's table; from then on that one is a hit)
                assert K.STATS["table_miss"] == misses
            if fused:
                assert len(K._pack_cache) == cached + 1          # only the 4x4 view was missing
            out = [w.detach().clone() for w in ws]
            out += [K.winograd_weight_view(*v)[0].clone() for v in wino] + [K.packed_weight_view(*v)[0].clone() for v in pack]
        assert {K.winograd_weight_view(*v)[1] for v in wino} == {4, 6}
        torch.cuda.synchronize()
        K.release_views(ws)
        return out

    for graph_mode in (False, True):
        a, b = run(True, graph_mode), run(False, graph_mode)
        assert len(a) == len(b) == 4 + 8 + 5
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (graph_mode, i)
