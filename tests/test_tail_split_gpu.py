"""The D-to-G hand-over in two ranges (train_step.TAIL_SPLIT: the deep layers' optimizer launch, derived views and power iteration
on the side stream under the G step's level 1-3 convs, joined at conv41) against the one-stream hand-over: the same iterations
bit for bit, eager and as a recorded launch list."""
import random

import pytest
import torch

import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu
B = 2


def _build(dev):
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    from mtd_gan_amd.module.weight_methods import WeightMethods
    from mtd_gan_amd.optimizers import FusedAdamW
    torch.manual_seed(5)
    m = MTD_GAN_Method().cuda().train()
    wm = WeightMethods("pcgrad", n_tasks=3, device=dev)
    oD = FusedAdamW(m.Discriminator.parameters(), lr=1e-4, weight_decay=5e-4)
    oG = FusedAdamW(m.Generator.parameters(), lr=1e-4, weight_decay=5e-4)
    random.seed(123)                # the PCGrad projection orders
    torch.manual_seed(99)           # the dropout draws
    return m, wm, oD, oG


def _snapshot(m, oD, oG):
    st = {k: v.clone() for k, v in m.state_dict().items()}          # generator and discriminator, u / v of the spectral norm included
    for tag, o in (("D", oD), ("G", oG)):
        for i, p in enumerate(o.param_groups[0]["params"]):
            if p in o.state:
                st[f"{tag}.m{i}"], st[f"{tag}.v{i}"] = o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone()
    return st


def _run(dev, batches, split, fused, recorded):
    from mtd_gan_amd import engine, train_step as TS
    old = TS.TAIL_SPLIT, TS.TAIL_FUSED
    TS.TAIL_SPLIT, TS.TAIL_FUSED = split, fused
    try:
        m, wm, oD, oG = _build(dev)
        logged = []
        for x, y in batches:
            step = TS.recorded_iteration if recorded else engine.train_iteration
            _names, vals = step(m, x, y, oG, oD, wm, None)
            logged.append(vals.clone())
        torch.cuda.synchronize()
        return _snapshot(m, oD, oG), logged, m
    finally:
        TS.TAIL_SPLIT, TS.TAIL_FUSED = old


@pytest.fixture(scope="module")
def one_stream(hip_lib):
    """The reference of every test here, computed once: four eager iterations with neither the split nor the fused views."""
    dev = torch.device("cuda")
    batches = [tuple(t.cuda() for t in orc.synthetic_ldct(B, seed=40 + i)) for i in range(4)]
    sd, logged, _m = _run(dev, batches, 0, False, False)
    return dev, batches, sd, logged


def _same(sd, logged, ref_sd, ref_logged, n):
    assert len(logged) == n
    for i in range(n):
        assert torch.equal(logged[i], ref_logged[i]), (i, logged[i], ref_logged[i])
    assert sd.keys() == ref_sd.keys() and any(k.startswith("D.m") for k in sd) and any(k.startswith("G.v") for k in sd)
    for k in sd:
        assert torch.equal(sd[k], ref_sd[k]), k


def test_two_iterations_split_on_equal_split_off(one_stream):
    from mtd_gan_amd import kernels as K
    dev, batches, _sd4, ref_logged = one_stream
    assert K.side_stream(dev).enabled
    off = _run(dev, batches[:2], 0, True, False)
    on = _run(dev, batches[:2], 2, True, False)
    plain = _run(dev, batches[:2], 2, False, False)            # the split without the fused views
    _same(on[0], on[1], off[0], off[1], 2)
    _same(plain[0], plain[1], off[0], off[1], 2)
    for i in range(2):                                         # ... and both are the one-stream, three-launch hand-over
        assert torch.equal(on[1][i], ref_logged[i]), i


def test_recorded_list_with_the_split_equals_eager(one_stream):
    """Two eager iterations, the third recorded with the split, the fourth replayed: the four one-stream eager iterations, bit for
    bit; and the list holds the split -- the D step's two update launches on two streams."""
    from mtd_gan_amd import train_step as TS
    dev, batches, ref_sd, ref_logged = one_stream
    sd, logged, m = _run(dev, batches, 1, True, True)
    st = m._mtd_recorded
    assert isinstance(st, TS.RecordedTrainStep) and st.iterations == 2      # recorded at the third iteration, one replay
    launches = [(getattr(op[0], "__name__", ""), op[1]) for op in st.list.ops]
    streams = [args[-1].value for name, args in launches if name == "mtd_adamw_views"]
    assert len(streams) == 2 and streams[0] != streams[1], streams
    _same(sd, logged, ref_sd, ref_logged, 4)
