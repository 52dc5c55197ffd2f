"""Mirror of the reference's `module/weight_methods.py` (:727-761 WeightMethods facade / METHODS table) for eight of its
eleven task weightings of the discriminator step:

  pcgrad                              :409-468   gradient surgery (what train.py uses by default)
  cagrad                              :471-588   conflict-averse gradient
  ls, scaleinvls, stl, uw, rlw, dwa   :275-316, 375-406, 591-602, 678-724   weightings of the losses

backward(losses=..., shared_parameters=..., task_specific_parameters=..., last_shared_parameters=...) writes `.grad` and returns
what the reference returns: (None, {}) for pcgrad / cagrad, (loss, dict(weights=...)) for the loss weightings.
  * losses produced by MTD_GAN_Method.d_loss carry the recorded discriminator passes: the fused per-task backward runs
    (train_step.DStepTape.run_pcgrad / run_cagrad / run_weighted);
  * any other autograd graph takes the generic route: torch.autograd on the graph, the same HIP kernels for the Gram matrix, the
    coefficients and the combination (pcgrad, cagrad) or for the weights (the loss weightings).
Nothing reads a loss or a gradient back to the host: the reference's `.cpu()` / `.item()` per step (and CAGrad's scipy solve)
are the kernels mtd_task_weights and mtd_cagrad_coeff.  The loss weightings therefore return device tensors that are views of a
buffer the next call overwrites -- clone what has to outlive the step.

PCGrad's shuffle order is drawn from Python's `random` exactly as the reference does (one in-place shuffle of a 3-element list
per task), RLW's weights from `torch.randn(n_tasks)` on the CPU generator: seeding reproduces the reference's draws.

Which parameters get a gradient follows the reference: pcgrad sets the two lists' only (`c_fc` is in neither and stays frozen);
the loss weightings call loss.backward() and cagrad calls losses[i].backward(), which reach every parameter in the graph -- on
the tape that adds `c_fc` (STL too: the main loss is an element of the stacked losses, so autograd hands zeros to the rest).

NOT here: `mgda`, `imtl`, `nashmtl`.  They derive task weights from the shared gradients and then apply them to the task-specific
parameters too, which the D step's single task-specific bucket (one sum over the tasks, written while the passes run) cannot
give: it needs one bucket per task or a second trip through the decoders, i.e. another cut of the discriminator backward.
`nashmtl` also needs cvxpy.  Those names fail the METHODS assertion as before.

Data parallelism: only pcgrad takes a `dp` hook of more than one rank; the others raise NotImplementedError (the RLW draw, the
DWA state and the UW gradients would each need a collective decision).
"""
from typing import List, Union

import torch

from .. import kernels as K
from .. import train_step as TS


class WeightMethod:
    def __init__(self, n_tasks: int, device: torch.device):
        self.n_tasks = n_tasks
        self.device = device

    def parameters(self) -> List[torch.Tensor]:
        return []


class PCGrad(WeightMethod):
    def __init__(self, n_tasks: int, device: torch.device, reduction="sum"):
        super().__init__(n_tasks, device=device)
        assert reduction in ["mean", "sum"]
        self.reduction = reduction
        self.dp = None                 # optional data-parallel hook (parallel.DataParallelSync)

    def get_weighted_loss(self, losses, **kwargs):
        raise NotImplementedError

    def _set_pc_grads(self, losses, shared_parameters, task_specific_parameters=None):
        if isinstance(shared_parameters, torch.Tensor):
            shared_parameters = [shared_parameters]
        if isinstance(task_specific_parameters, torch.Tensor):
            task_specific_parameters = [task_specific_parameters]
        shared_parameters = list(shared_parameters)
        tape = getattr(losses, "_mtd_tape", None)
        if tape is not None and not tape.consumed:
            tape.run_pcgrad(shared_parameters, list(task_specific_parameters) if task_specific_parameters is not None else None,
                            self.reduction, self.dp)
            return
        # ---- generic autograd graph
        T = len(losses)
        if T > 4:
            raise NotImplementedError("HIP PCGrad kernels handle up to 4 tasks")
        sizes = [p.numel() for p in shared_parameters]
        flat = []
        for i in range(T):
            gs = torch.autograd.grad(losses[i], shared_parameters, retain_graph=True)
            flat.append(torch.cat([g.reshape(-1) for g in gs]).contiguous())
        orders = TS.shuffle_orders(T)
        orders_dev = torch.tensor([j for o in orders for j in o], dtype=torch.int32).to(flat[0].device, non_blocking=True)
        gram = K.pcgrad_gram(flat)
        merged = torch.empty_like(flat[0])
        K.pcgrad_combine(flat, gram, orders_dev, merged)
        if self.reduction == "mean":
            merged = merged / self.n_tasks
        ofs = 0
        for p, sz in zip(shared_parameters, sizes):
            p.grad = merged[ofs:ofs + sz].view_as(p)
            ofs += sz
        if task_specific_parameters is not None:
            task_specific_parameters = list(task_specific_parameters)
            ts = torch.autograd.grad(losses.sum(), task_specific_parameters)
            for p, g in zip(task_specific_parameters, ts):
                p.grad = g

    def backward(self, losses, parameters=None, shared_parameters=None, task_specific_parameters=None, **kwargs):
        self._set_pc_grads(losses, shared_parameters, task_specific_parameters)
        return None, {}          # NOTE: aligned with the reference (weight_methods.py:466-468)

    def __call__(self, losses, **kwargs):
        return self.backward(losses, **kwargs)


def _as_list(params):
    if params is None:
        return None
    return [params] if isinstance(params, torch.Tensor) else list(params)


def _single_rank(self):
    dp = getattr(self, "dp", None)
    if dp is not None and int(getattr(dp, "world", getattr(dp, "world_size", 1))) > 1:
        raise NotImplementedError(f"{type(self).__name__}: data parallelism over more than one rank is implemented for pcgrad only")


def _outside_lists(D, shared, tspec):
    """Parameters of the discriminator that are in neither list (c_fc), in module order."""
    listed = {id(p) for p in shared} | {id(p) for p in (tspec or [])}
    return [p for p in D.parameters() if id(p) not in listed and p.requires_grad]


class _LossWeighting(WeightMethod):
    """Common part of the loss weightings: c_k = d loss / d L_k from one mtd_task_weights launch, then the gradient of
    sum_k c_k L_k.  self._c: the c_k; self._aux: [loss, weights[4], d loss / d logsigma[4]] (device, rewritten per call)."""
    method_id = None
    window, temp = 0, 1.0

    def __init__(self, n_tasks, device):
        super().__init__(n_tasks, device=device)
        if n_tasks > 4:
            raise NotImplementedError("the HIP task-weight kernel handles up to 4 tasks")
        self.dp = None
        dev = torch.device(device)
        self._c = torch.zeros(4, dtype=torch.float32, device=dev) if dev.type == "cuda" else None
        self._aux = torch.zeros(9, dtype=torch.float32, device=dev) if dev.type == "cuda" else None

    def _state(self):
        return None

    def _params(self):
        return None

    def _launch(self, losses):
        if not losses.is_cuda:
            raise RuntimeError(f"{type(self).__name__}: the HIP path needs CUDA losses")
        if self._c is None or self._c.device != losses.device:
            raise RuntimeError(f"{type(self).__name__} was built for device {self.device}, the losses live on {losses.device}")
        assert len(losses) == self.n_tasks
        lv = losses.detach()
        if lv.dtype != torch.float32 or not lv.is_contiguous():
            lv = lv.float().contiguous()
        K.task_weights(self.method_id, lv, self._state(), self._params(), self._c, self._aux, self.window, self.temp)
        self._after_launch()
        return self._aux[0], self._aux[1:1 + self.n_tasks]

    def _after_launch(self):
        pass

    def get_weighted_loss(self, losses, **kwargs):
        """(loss, dict(weights=...)) as the reference; `loss` is differentiable through the task losses with d loss / d L_k = c_k
        (on a graph that autograd knows; for the losses of d_loss use backward())."""
        loss, weights = self._launch(losses)
        if losses.requires_grad:
            c = self._c[:self.n_tasks]
            loss = loss.detach() + (torch.sum(losses * c) - torch.sum(losses.detach() * c))
        return loss, dict(weights=weights)

    def backward(self, losses, shared_parameters=None, task_specific_parameters=None, last_shared_parameters=None, representation=None, **kwargs):
        _single_rank(self)
        tape = getattr(losses, "_mtd_tape", None)
        if tape is not None and not tape.consumed:
            if self.n_tasks != 3:
                raise ValueError("the recorded discriminator step has 3 tasks")
            loss, weights = self._launch(losses)
            shared, tspec = _as_list(shared_parameters), _as_list(task_specific_parameters)
            D = tape.method.Discriminator
            tape.run_weighted(shared, tspec, self._c, _outside_lists(D, shared, tspec))
            self._set_own_grads()
            return loss, dict(weights=weights)
        # ---- generic autograd graph: loss.backward() of the reference, the weights from the same kernel
        loss, weights = self._launch(losses)
        torch.autograd.backward(torch.sum(losses * self._c[:self.n_tasks]))
        self._set_own_grads()
        return loss, dict(weights=weights)

    def _set_own_grads(self):
        pass

    def __call__(self, losses, **kwargs):
        return self.backward(losses, **kwargs)


def _task_weight_tensor(task_weights, n_tasks, device):
    if task_weights is None:
        task_weights = torch.ones((n_tasks,))
    if not isinstance(task_weights, torch.Tensor):
        task_weights = torch.tensor(task_weights)
    assert len(task_weights) == n_tasks
    return task_weights.to(device)


class LinearScalarization(_LossWeighting):
    """L = sum_k w_k L_k (reference :275-294)."""
    method_id = K.TW_LS

    def __init__(self, n_tasks: int, device: torch.device, task_weights: Union[List[float], torch.Tensor] = None):
        super().__init__(n_tasks, device=device)
        self.task_weights = _task_weight_tensor(task_weights, n_tasks, device)
        self._w = self.task_weights.detach().float().contiguous()        # uploaded once

    def _params(self):
        return self._w


class ScaleInvariantLinearScalarization(LinearScalarization):
    """L = sum_k w_k log L_k (reference :297-316): c_k = w_k / L_k."""
    method_id = K.TW_SCALEINV


class STL(_LossWeighting):
    """Single task learning (reference :375-388): L = L_main."""
    method_id = K.TW_STL

    def __init__(self, n_tasks, device: torch.device, main_task):
        super().__init__(n_tasks, device=device)
        self.main_task = main_task
        self.weights = torch.zeros(n_tasks, device=device)
        self.weights[main_task] = 1.0

    def _params(self):
        return self.weights

class Uncertainty(_LossWeighting):
    """Uncertainty weighting (reference :391-406): L = sum_k 0.5 (exp(-s_k) L_k + s_k), s = logsigma (learnable)."""
    method_id = K.TW_UW

    def __init__(self, n_tasks, device: torch.device):
        super().__init__(n_tasks, device=device)
        self.logsigma = torch.tensor([0.0] * n_tasks, device=device, requires_grad=True)

    def _state(self):
        return self.logsigma.detach()

    def _set_own_grads(self):
        self.logsigma.grad = self._aux[5:5 + self.n_tasks]

    def get_weighted_loss(self, losses, **kwargs):
        loss, extra = super().get_weighted_loss(losses, **kwargs)
        if self.logsigma.requires_grad:      # d loss / d logsigma through autograd as well
            g = self._aux[5:5 + self.n_tasks]
            loss = loss + (torch.sum(self.logsigma * g) - torch.sum(self.logsigma.detach() * g))
        return loss, extra

    def parameters(self) -> List[torch.Tensor]:
        return [self.logsigma]


class RLW(_LossWeighting):
    """Random loss weighting (reference :591-602): softmax of a fresh torch.randn(n_tasks) drawn on the HOST generator, as the
    reference draws it; the three floats reach the kernel through a pinned slot (no copy in the stream)."""
    method_id = K.TW_RLW

    def __init__(self, n_tasks, device: torch.device):
        super().__init__(n_tasks, device=device)
        self._slot = None
        self.last_draw = None

    def _params(self):
        if self._slot is None:
            self._slot = K.HostScalars(self._c.device, 4, torch.float32)
        self.last_draw = torch.randn(self.n_tasks)
        self._slot.set(self.last_draw.tolist())
        return self._slot.device_ptr()

    def _after_launch(self):
        self._slot.consumed()


class DynamicWeightAverage(_LossWeighting):
    """Dynamic weight average (reference :678-724).  The ring of the last 2 * iteration_window task losses, the weights and the
    iteration counter live on the device (the reference reads the losses back per step)."""
    method_id = K.TW_DWA

    def __init__(self, n_tasks, device: torch.device, iteration_window: int = 25, temp=2.0):
        super().__init__(n_tasks, device=device)
        self.iteration_window = self.window = int(iteration_window)
        self.temp = temp
        dev = torch.device(device)
        self._dwa = None
        if dev.type == "cuda":
            self._dwa = torch.ones(1 + 4 + 2 * self.window * n_tasks, dtype=torch.float32, device=dev)
            self._dwa[:1].view(torch.int32).zero_()

    def _state(self):
        return self._dwa

    @property
    def running_iterations(self):
        """Calls so far (reads the device: a synchronisation -- for inspection, not for the step)."""
        return int(self._dwa[:1].view(torch.int32).item())

    @property
    def weights(self):
        return self._dwa[1:1 + self.n_tasks]


class CAGrad(WeightMethod):
    """Conflict-averse gradient (reference :471-588): shared parameters get n_tasks (mean_k g_k + lambda sum_k ww_k g_k) / (1 + c^2),
    everything else the graphs reach the gradient of the plain sum.  ww, lambda: mtd_cagrad_coeff on the Gram matrix."""

    def __init__(self, n_tasks, device: torch.device, c=0.4):
        super().__init__(n_tasks, device=device)
        self.c = c
        self.dp = None

    def get_weighted_loss(self, losses, shared_parameters, **kwargs):
        """As the reference: sets .grad (accumulating into what is there for everything but the shared parameters) and returns None."""
        _single_rank(self)
        shared = _as_list(shared_parameters)
        tape = getattr(losses, "_mtd_tape", None)
        if tape is not None and not tape.consumed:
            D = tape.method.Discriminator
            tspec = list(D.task_specific_parameters())
            tape.run_cagrad(shared, tspec, self.c, _outside_lists(D, shared, tspec))
            return None
        T = len(losses)
        if T > 4:
            raise NotImplementedError("the HIP CAGrad kernels handle up to 4 tasks")
        flat = []
        for i in range(T):
            # losses[i].backward(retain_graph=True) of the reference: every leaf accumulates, the shared ones are collected and cleared
            losses[i].backward(retain_graph=True)
            flat.append(torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in shared]).float().contiguous())
            for p in shared:
                p.grad = None
        gram = K.pcgrad_gram(flat)
        coeff = K.cagrad_coeff(gram, T, self.c)
        n = flat[0].numel()
        pad = torch.empty((n + 3) // 4 * 4, dtype=torch.float32, device=flat[0].device)
        merged = K.pcgrad_axpy(flat, coeff, 1.0, pad[:n])
        ofs = 0
        for p in shared:
            p.grad = merged[ofs:ofs + p.numel()].view_as(p).clone()
            ofs += p.numel()
        self.gram, self.coeff = gram, coeff
        return None

    def backward(self, losses, parameters=None, shared_parameters=None, task_specific_parameters=None, **kwargs):
        self.get_weighted_loss(losses, shared_parameters)
        return None, {}          # NOTE: aligned with the reference (weight_methods.py:587-588)

    def __call__(self, losses, **kwargs):
        return self.backward(losses, **kwargs)


def cagrad_host_model(gram, c):
    """numpy float64 model of mtd_cagrad_coeff, the same enumeration the kernel runs (csrc/weighting.hip): per face of the simplex
    the stationary point of phi in closed form, the feasible candidate with the smallest phi wins.  gram: (T, T), T <= 4.
    Returns (coefficients[T], phi, ww[T]).  For tests and for tools/pin_weight_methods.py; the step never calls it."""
    import numpy as np
    A = np.asarray(gram, dtype=np.float64)
    T = A.shape[0]
    scale = float(np.abs(A).max())
    c0 = float(c) * np.sqrt(max(A.mean(), 0.0) + 1e-8) + 1e-8
    Ab = A.sum(1) / T

    def phi(x):
        return float(x @ Ab + c0 * np.sqrt(max(x @ A @ x, 0.0) + 1e-8))
    best = (np.inf, None)
    for mask in range(1, 1 << T):
        idx = [i for i in range(T) if mask >> i & 1]
        m = len(idx)
        cands = []
        if m == 1:
            cands.append(np.ones(1))
        elif scale > 0.0:
            M = np.zeros((m + 1, m + 1))
            M[:m, :m] = A[np.ix_(idx, idx)]
            M[:m, m] = M[m, :m] = scale
            rhs = np.zeros((m + 1, 2))
            rhs[m, 0] = scale
            rhs[:m, 1] = -Ab[idx]
            try:
                if np.linalg.cond(M) > 1e13:
                    raise np.linalg.LinAlgError
                sol = np.linalg.solve(M, rhs)
            except np.linalg.LinAlgError:
                continue
            x0, x1 = sol[:m, 0], sol[:m, 1]
            As = A[np.ix_(idx, idx)]
            q00, q01, q11 = x0 @ As @ x0, x0 @ As @ x1, x1 @ As @ x1
            qa, qb, qc = q11 - c0 * c0, 2.0 * q01, max(q00, 0.0) + 1e-8
            roots = []
            if abs(qa) <= 1e-300:
                if qb != 0.0:
                    roots.append(-qc / qb)
            else:
                disc = qb * qb - 4.0 * qa * qc
                if disc >= 0.0:
                    t = -0.5 * (qb + (np.sqrt(disc) if qb >= 0.0 else -np.sqrt(disc)))
                    roots.append(t / qa)
                    if t != 0.0:
                        roots.append(qc / t)
            cands += [x0 + u * x1 for u in roots if 0.0 < u < 1e300]
        for xs in cands:
            if not (np.all(xs >= -1e-9) and np.all(xs <= 1.0 + 1e-9)):
                continue
            x = np.zeros(T)
            x[idx] = np.maximum(xs, 0.0)
            if not x.sum() > 0.0:
                continue
            x /= x.sum()
            p = phi(x)
            if p < best[0]:
                best = (p, x)
    p, ww = best
    w32 = ww.astype(np.float32).astype(np.float64)
    lam = c0 / (np.sqrt(max(w32 @ A @ w32, 0.0)) + 1e-8)
    coeff = T / (1.0 + float(c) ** 2) * (1.0 / T + lam * w32)
    return coeff, p, ww


class WeightMethods:
    def __init__(self, method: str, n_tasks: int, device: torch.device, **kwargs):
        assert method in METHODS, f"unknown method {method}."
        self.method = METHODS[method](n_tasks=n_tasks, device=device, **kwargs)

    def get_weighted_loss(self, losses, **kwargs):
        return self.method.get_weighted_loss(losses, **kwargs)

    def backward(self, losses, **kwargs):
        return self.method.backward(losses, **kwargs)

    def __ceil__(self, losses, **kwargs):
        return self.backward(losses, **kwargs)

    def parameters(self):
        return self.method.parameters()


# the reference's table (:749-761) without mgda / imtl / nashmtl (see the module docstring)
METHODS = dict(stl=STL, ls=LinearScalarization, uw=Uncertainty, pcgrad=PCGrad, cagrad=CAGrad,
               scaleinvls=ScaleInvariantLinearScalarization, rlw=RLW, dwa=DynamicWeightAverage)
