"""The CPU model of binary16 activation storage (tests/_half_model.py) held to the oracle: it is the yardstick of
tests/test_half_storage_gpu.py, so it must BE the oracle's generator when nothing is rounded, and the storage contract must keep
the project's PSNR bar on its own."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mtdgan_oracle as orc  # noqa: E402
import _half_model as hm  # noqa: E402
from _metrics import rel  # noqa: E402


def _case(S, B=1):
    g = orc.seeded_fill(orc.g_param_shapes(), seed=7)
    x, y = orc.synthetic_ldct(B, seed=5, size=S)
    return g, x, y


def test_model_without_rounding_is_the_oracle():
    g, x, _ = _case(128)
    ref = orc.generator_forward(g, x)
    got = hm.generator_forward(g, x, hm.identity)
    e = rel(got, ref)
    print(f"model(identity) vs oracle, S = 128: rel = {e:.3e}")
    assert e < 1e-5          # (the separable transform is not bit-identical to rfft2 / irfft2)


def test_block_model_without_rounding_is_the_oracle_block():
    g, _, _ = _case(128)
    x = torch.randn(1, 32, 128, 128, generator=torch.Generator().manual_seed(3)).relu()
    p = "enforce.4."
    w = (g[p + "img_conv.weight"], g[p + "img_conv.bias"], g[p + "fft_conv.weight"], g[p + "fft_conv.bias"])
    e = rel(hm.block(x, *w, hm.identity), orc.resfft_block(x, *w))
    print(f"block model(identity) vs oracle block: rel = {e:.3e}")
    assert e < 1e-5


def test_half_round_is_one_binary16_rounding():
    t = torch.tensor([0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 70000.0, -1e9, 65504.0])
    want = torch.tensor([0.0, 1.0, 1.0, 1.0 + 2.0 ** -9, 0.0, 2.0 ** -23, 65504.0, -65504.0, 65504.0])      # ties to even; saturation, no infinities
    assert torch.equal(hm.half_round(t), want)


def test_binary16_storage_keeps_the_psnr_bar_at_128():
    g, x, y = _case(128)
    ref = orc.generator_forward(g, x)
    got = hm.generator_forward(g, x, hm.half_round)
    assert torch.isfinite(got).all()
    e = rel(got, ref)
    d_psnr = abs(orc.psnr(got.clip(0, 1), y).item() - orc.psnr(ref.clip(0, 1), y).item())
    print(f"model(binary16) vs oracle, S = 128: rel = {e:.3e}, PSNR change = {d_psnr:.2e} dB")
    assert d_psnr < 0.01
    assert 0.0 < e < 1e-2    # rounded at all, and nowhere near the bf16 figures (4e-3 .. 1.4e-2 came from 8 mantissa bits; binary16: 3.5e-4)
