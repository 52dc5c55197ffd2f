"""The task weightings next to PCGrad on the GPU (module/weight_methods.py, csrc/weighting.hip, train_step.DStepTape.run_weighted /
run_cagrad) against the reference's own results recorded by tools/pin_weight_methods.py in tests/golden/weight_methods_b2.npz and
tests/golden/cagrad_gram_cases.npz."""
import json
import os
import random

import numpy as np
import pytest
import torch

import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3                      # the parity bound of tests/test_step_gpu.py
FAMILY_A = ["ls", "scaleinvls", "stl", "uw", "rlw", "dwa"]
# fp32 kernels against the reference's fp32 CPU arithmetic: a chain of at most ~10 operations of 6e-8 each, expf / logf of the
# device library within 2 ulp of the host's
F32 = dict(rtol=1e-5, atol=1e-7)


def _fixture():
    z = np.load(os.path.join(GOLD, "weight_methods_b2.npz"))
    return z, json.loads(str(z["meta"]))


def _model(batch):
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    z = json.load(open(os.path.join(GOLD, "step_seeded.json")))
    full = {"Generator." + k: v for k, v in orc.seeded_fill(orc.g_param_shapes(), seed=z["gfill"]).items()}
    full.update({"Discriminator." + k: v for k, v in orc.seeded_fill(orc.d_state_shapes(), seed=z["dfill"]).items()})
    m = MTD_GAN_Method()
    m.load_state_dict(full)
    m.cuda().train()
    g = torch.Generator().manual_seed(z["mask_seed"])
    masks = [(torch.rand(batch, 512, generator=g) >= 0.3).float() / 0.7 for _ in range(5)]
    return m, masks


def _method(name, meta):
    from mtd_gan_amd.module.weight_methods import WeightMethods
    wm = WeightMethods(name, n_tasks=3, device=torch.device("cuda"), **meta["method_kw"][name])
    if name == "uw":
        with torch.no_grad():
            wm.method.logsigma.copy_(torch.tensor(meta["uw_logsigma"]))
    return wm


def _d_step(name, meta, batch=2):
    m, masks = _model(batch)
    m.Discriminator._inject_masks = [k.clone() for k in masks[:4]]
    x, y = orc.synthetic_ldct(batch, seed=1234)
    wm = _method(name, meta)
    random.seed(77)
    if name == "rlw":
        torch.manual_seed(meta["rlw_seed"])
    losses, _ = m.d_loss(x.cuda(), y.cuda())
    D = m.Discriminator
    out = wm.backward(losses=losses, shared_parameters=list(D.shared_parameters()), task_specific_parameters=list(D.task_specific_parameters()),
                      last_shared_parameters=list(D.last_shared_parameters()))
    torch.cuda.synchronize()
    return m, wm, losses, out


def test_cagrad_coeff_kernel_on_every_gram_case(hip_lib):
    """mtd_cagrad_coeff against scipy SLSQP at ftol 1e-14 (recorded): phi at the kernel's minimiser is not above the tight value by
    more than 2 x the 99th percentile of (phi_default - phi_tight) / |phi_tight| that the reference's own default-tolerance solve
    shows on these cases, on EVERY case; the merged gradient (through the Gram matrix: |sum_k d_k g_k| / |sum_k c_k g_k|) is within
    2 x the 99th percentile of the default-vs-tight difference on all but at most 1 % of the cases; no NaN anywhere."""
    from mtd_gan_amd import kernels as K
    z = np.load(os.path.join(GOLD, "cagrad_gram_cases.npz"))
    band = json.loads(str(z["band"]))
    N = len(z["T"])
    outs = []
    for i in range(N):
        T = int(z["T"][i])
        gram = torch.tensor(z["gram"][i, :T, :T].reshape(-1), dtype=torch.float64, device="cuda")
        outs.append(K.cagrad_coeff(gram, T, float(z["c"][i])))
    res = torch.stack(outs).double().cpu().numpy()
    over, worst, worst_phi = 0, 0.0, -1.0
    for i in range(N):
        T, c = int(z["T"][i]), float(z["c"][i])
        A = z["gram"][i, :T, :T]
        coeff, ww = res[i, :T], res[i, 5:5 + T]
        assert np.all(np.isfinite(res[i, :T])) and np.all(np.isfinite(ww)) and np.isfinite(res[i, 4]), (i, str(z["kind"][i]))
        assert abs(ww.sum() - 1.0) < 1e-5 and ww.min() >= 0.0
        c0 = c * np.sqrt(A.mean() + 1e-8) + 1e-8
        phi = float(ww @ A @ np.ones(T) / T + c0 * np.sqrt(max(ww @ A @ ww, 0.0) + 1e-8))
        pt = float(z["phi_tight"][i])
        worst_phi = max(worst_phi, (phi - pt) / abs(pt))
        assert phi <= pt + band["phi_rel_slack"] * abs(pt), (i, str(z["kind"][i]), phi, pt)
        ct = z["coeff_tight"][i, :T]
        d = coeff - ct
        e = np.sqrt(max(d @ A @ d, 0.0)) / (np.sqrt(max(ct @ A @ ct, 0.0)) + 1e-30)
        worst = max(worst, e)
        over += e > band["merged_bound"]
    print(f"{N} Gram cases: phi - phi_tight (relative) worst {worst_phi:.2e} (slack {band['phi_rel_slack']:.2e}); merged difference worst "
          f"{worst:.2e} (bound {band['merged_bound']:.2e}), {over} over")
    assert over <= band["max_excluded"] * N


def test_task_weights_kernel_vs_reference(hip_lib):
    """mtd_task_weights per loss weighting on recorded task losses (a loss of 1e-6 among them): loss, weights, d loss / d L_k and
    d loss / d logsigma against the reference's get_weighted_loss + autograd; the dwa sequence over window + 3 calls."""
    z, meta = _fixture()
    for name in ("ls", "scaleinvls", "stl", "uw", "rlw"):
        for j, ls in enumerate(z["kernel.losses"]):
            wm = _method(name, meta).method
            torch.manual_seed(meta["rlw_seed"] + j)
            loss, weights = wm._launch(torch.tensor(ls, dtype=torch.float32, device="cuda"))
            want = z["kernel." + name][j]
            np.testing.assert_allclose(float(loss), want[0], err_msg=f"{name} loss {j}", **F32)
            np.testing.assert_allclose(weights.cpu().numpy(), want[1:4], err_msg=f"{name} weights {j}", **F32)
            np.testing.assert_allclose(wm._c[:3].cpu().numpy(), want[4:7], err_msg=f"{name} c {j}", **F32)
            if name == "uw":
                np.testing.assert_allclose(wm._aux[5:8].cpu().numpy(), want[7:10], err_msg=f"uw dlogsigma {j}", **F32)
    wm = _method("dwa", meta).method
    for j, ls in enumerate(z["dwa.seq_losses"]):
        loss, weights = wm._launch(torch.tensor(ls, dtype=torch.float32, device="cuda"))
        np.testing.assert_allclose(weights.cpu().numpy(), z["dwa.seq_weights"][j], err_msg=f"dwa weights after call {j}", **F32)
        np.testing.assert_allclose(float(loss), z["dwa.seq_loss"][j], err_msg=f"dwa loss {j}", **F32)
        np.testing.assert_allclose(wm._c[:3].cpu().numpy(), z["dwa.seq_weights"][j] / 3.0, err_msg=f"dwa c {j}", **F32)
    assert wm.running_iterations == len(z["dwa.seq_losses"])
    assert not np.allclose(z["dwa.seq_weights"][-1], 1.0)            # (the fixture reaches the branch of :709-715)


@pytest.mark.parametrize("name", FAMILY_A + ["cagrad"])
def test_d_step_per_method_vs_reference(hip_lib, name):
    """One D step at B = 2 through WeightMethods(name).backward(losses=model.d_loss(x, y)[0], ...) against the reference's:
    every sampled gradient element at the float64 value within max(1e-3, 2 x the reference's own fp32-vs-float64 error on that
    tensor) of the tensor's max-abs, the tensor's max-abs and norm within 5e-3 (the bounds of
    test_step_gpu.py::test_d_step_task_gradients_b32_vs_reference_samples), the returned loss and weights within 1e-3, and the
    SET of parameters that received a .grad."""
    z, meta = _fixture()
    m, wm, losses, (loss, extra) = _d_step(name, meta)
    D = m.Discriminator
    names = [n for n, _ in D.named_parameters()]
    assert names == meta["names"]
    got_set = [n for n, p in D.named_parameters() if p.grad is not None]
    assert got_set == meta["reached"][name]
    lf = torch.tensor(meta["losses_f64"])
    assert ((losses.double().cpu() - lf).abs() / lf.abs()).max().item() < TOL
    if name == "cagrad":
        assert loss is None and extra == {}
        tape = losses._mtd_tape
        cw = torch.tensor(z["cagrad.coeff_f64"])
        assert ((tape.coeff[:3].double().cpu() - cw).abs().max() / cw.abs().max()).item() < TOL
    else:
        assert abs(float(loss) - float(z[name + ".loss"])) <= TOL * abs(float(z[name + ".loss"]))
        w = torch.tensor(z[name + ".weights"])
        assert ((extra["weights"].double().cpu() - w).abs().max() / w.abs().max()).item() < TOL
    if name == "uw":
        gl = torch.tensor(z["uw.logsigma_grad_f64"])
        assert ((wm.method.logsigma.grad.double().cpu() - gl).abs().max() / gl.abs().max()).item() < TOL
        assert wm.parameters()[0] is wm.method.logsigma and wm.method.logsigma.is_cuda and wm.method.logsigma.requires_grad
    bad, worst, checked = [], 0.0, 0
    for j, (n, p) in enumerate(D.named_parameters()):
        if p.grad is None:
            continue
        flat = p.grad.reshape(-1)
        f64, maxabs, err32, norm = z[name + ".f64"][j], float(z[name + ".maxabs"][j]), float(z[name + ".err32"][j]), float(z[name + ".norm_f64"][j])
        idx = [(i * 2654435761 + 12345) % flat.numel() for i in range(len(f64))]
        got = flat[torch.tensor(idx, device=flat.device)].double().cpu().tolist()
        bound = max(TOL, 2 * err32) * maxabs
        for i, (a, b) in enumerate(zip(got, f64)):
            worst = max(worst, abs(a - b) / (maxabs + 1e-30))
            checked += 1
            if abs(a - b) > bound + 1e-30:
                bad.append((n, i, a, b, bound))
        mx, nr = flat.abs().max().item(), flat.double().norm().item()
        if abs(mx - maxabs) > 5e-3 * maxabs + 1e-30:
            bad.append((n, "maxabs", mx, maxabs))
        if abs(nr - norm) > 5e-3 * norm + 1e-30:
            bad.append((n, "norm", nr, norm))
    print(f"{name}: {checked} gradient elements, worst error relative to the tensor's max-abs {worst:.2e}; {len(bad)} over the bound")
    assert not bad, bad[:12]


def test_generic_route_on_a_small_graph(hip_lib):
    """Losses without a recorded tape: a 3-task graph over one shared and one task-specific tensor, against plain torch."""
    from mtd_gan_amd.module.weight_methods import WeightMethods, cagrad_host_model
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(11)
    s0, t0 = torch.randn(1003, generator=g), torch.randn(17, generator=g)
    a = torch.randn(3, 1003, generator=g).to(dev)

    def graph():
        s, t = s0.clone().to(dev).requires_grad_(True), t0.clone().to(dev).requires_grad_(True)
        losses = torch.stack([((s * a[0]).sum() + t.sum()) ** 2 * 1e-3 + 1.0, (s - a[1]).pow(2).mean() + t.pow(2).sum(), (s * a[2]).tanh().pow(2).sum() + 0.5])
        return s, t, losses
    s, t, losses = graph()
    per_task = [torch.autograd.grad(losses[i], [s, t], retain_graph=True, allow_unused=True) for i in range(3)]
    w = [0.7, 1.3, 0.4]
    s, t, losses = graph()
    loss, extra = WeightMethods("ls", n_tasks=3, device=dev, task_weights=w).backward(losses=losses, shared_parameters=[s], task_specific_parameters=[t])
    want_s = sum(wk * pt[0] for wk, pt in zip(w, per_task))
    want_t = sum(wk * (pt[1] if pt[1] is not None else 0) for wk, pt in zip(w, per_task))
    assert torch.allclose(s.grad, want_s, rtol=1e-5, atol=1e-6 * want_s.abs().max().item())
    assert torch.allclose(t.grad, want_t, rtol=1e-5, atol=1e-6 * want_t.abs().max().item())
    assert abs(float(loss) - float((losses.detach().cpu() * torch.tensor(w)).sum())) < 1e-5 * abs(float(loss))
    assert torch.allclose(extra["weights"].cpu(), torch.tensor(w))
    s, t, losses = graph()
    wm = WeightMethods("cagrad", n_tasks=3, device=dev)
    assert wm.backward(losses=losses, shared_parameters=[s], task_specific_parameters=[t]) == (None, {})
    G = torch.stack([pt[0] for pt in per_task]).double().cpu()
    coeff, _phi, _ww = cagrad_host_model((G @ G.t()).numpy(), 0.4)
    want_s = (torch.tensor(coeff)[:, None] * G).sum(0)
    assert ((s.grad.double().cpu() - want_s).abs().max() / want_s.abs().max()).item() < 1e-4
    want_t = sum(pt[1] for pt in per_task if pt[1] is not None)
    assert torch.allclose(t.grad, want_t, rtol=1e-5, atol=1e-6 * want_t.abs().max().item())


@pytest.mark.parametrize("name", ["ls", "cagrad"])
def test_recorded_list_equals_eager(hip_lib, name):
    """Two eager iterations, one recorded, three replayed against six eager ones: every discriminator (and generator) tensor equal
    bit for bit.  rlw and uw are kept eager, with the reason reported."""
    from mtd_gan_amd import engine, train_step as TS
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    from mtd_gan_amd.module.weight_methods import WeightMethods
    from mtd_gan_amd.optimizers import FusedAdamW
    dev = torch.device("cuda")
    batches = [tuple(t.cuda() for t in orc.synthetic_ldct(4, seed=70 + i)) for i in range(6)]
    kw = dict(task_weights=[0.7, 1.3, 0.4]) if name == "ls" else {}
    ends = {}
    for mode in ("eager", "list"):
        torch.manual_seed(5)
        m = MTD_GAN_Method().cuda().train()
        wm = WeightMethods(name, n_tasks=3, device=dev, **kw)
        oD = FusedAdamW(m.Discriminator.parameters(), lr=1e-4, weight_decay=5e-4)
        oG = FusedAdamW(m.Generator.parameters(), lr=1e-4, weight_decay=5e-4)
        torch.manual_seed(99)
        for i, (x, y) in enumerate(batches):
            if mode == "eager":
                engine.train_iteration(m, x, y, oG, oD, wm, None)
            else:
                TS.recorded_iteration(m, x, y, oG, oD, wm, None)
                if i >= 2:
                    assert isinstance(m._mtd_recorded, TS.RecordedTrainStep), getattr(m, "_mtd_list_error", None)
        torch.cuda.synchronize()
        ends[mode] = {k: v.clone() for k, v in m.state_dict().items()}
        if mode == "list":
            assert m._mtd_recorded.iterations == 4
    for k in ends["eager"]:
        assert torch.equal(ends["list"][k], ends["eager"][k]), k
    for refused in ("rlw", "uw"):
        wm = WeightMethods(refused, n_tasks=3, device=dev)
        assert not TS.RecordedTrainStep.usable(m, oG, oD, wm, *batches[0])
        assert TS.RecordedTrainStep.method_refusal(wm)


def test_data_parallel_hook_is_refused(hip_lib):
    from mtd_gan_amd.module.weight_methods import WeightMethods

    class TwoRanks:
        world = 2

        def all_reduce_avg(self, flat, after=()):
            raise AssertionError("no collective may be issued")
    for name, kw in (("ls", {}), ("cagrad", {}), ("dwa", {})):
        wm = WeightMethods(name, n_tasks=3, device=torch.device("cuda"), **kw)
        wm.method.dp = TwoRanks()
        with pytest.raises(NotImplementedError):
            wm.backward(losses=torch.ones(3, device="cuda"), shared_parameters=[], task_specific_parameters=[])


def test_unit_weights_leave_the_task_vectors_bit_identical(hip_lib):
    """ls with w = (1, 1, 1) against the PCGrad route on the same inputs: the three task vectors and the listed task-specific
    gradients are the same bits -- the weight pointer multiplies the cotangent's coefficient by exactly 1.0f and nothing else moved."""
    _z, meta = _fixture()
    meta = dict(meta, method_kw=dict(meta["method_kw"], ls=dict(task_weights=[1.0, 1.0, 1.0]), pcgrad={}))
    m0, _wm0, l0, _ = _d_step("pcgrad", meta)
    m1, _wm1, l1, _ = _d_step("ls", meta)
    assert torch.equal(l0, l1)
    S0, S1 = l0._mtd_tape.task_vectors, l1._mtd_tape.task_vectors
    for i in range(3):
        assert torch.equal(S0[i], S1[i]), i
    for p, q in zip(m0.Discriminator.task_specific_parameters(), m1.Discriminator.task_specific_parameters()):
        assert torch.equal(p.grad, q.grad)
    assert m0.Discriminator.c_fc.weight_orig.grad is None and m1.Discriminator.c_fc.weight_orig.grad is not None
