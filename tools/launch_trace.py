"""The launches of a scenario as text, one line per entry of a recorded kernels.LaunchList, for comparing two trees: a refactor of
the host-side schedules must leave `diff` of the two outputs empty.

A line holds the entry point's name and its arguments in the C signature's order (the argtypes of _lib.py say which argument is a
pointer): scalars as they are; argument structs and descriptor tables (recognised by the host array a recording keeps) field by
field, Geom included; every pointer -- arguments, struct fields, the stream -- as the index of its first appearance in the list (0
for null).  Under a recording no address is reused, so two lists with the same lines read and write the same buffers in the same
order whatever order the buffers were allocated in.  Event records / waits and recorded torch operations appear with their streams.

    python tools/launch_trace.py step   --out FILE [--batch 2] [--pair-decoders 1] [--lockstep 1] [--root TREE]
    python tools/launch_trace.py module --out FILE [--batch 2] [--root TREE]

step:   the third, recorded iteration of train_step.recorded_iteration on bench.py's seeded full-step workload (MTD_FORCE_DP=1 in
        the environment: through the one-rank data-parallel path).
module: forward + backward through the module surface of Multi_Task_Discriminator_Skip (train / eval, need_rec True / False) and
        of the five partial discriminators, one recording each.
--root: the tree to trace (default: this one) -- an export of another commit that holds a built library.
"""
import argparse
import ctypes as C
import os
import sys


class Namer:
    """Addresses, events and streams -> the index of their first appearance."""

    def __init__(self):
        self.ids = {"p": {}, "e": {}}

    def __call__(self, kind, key):
        if not key:
            return "0"
        ids = self.ids[kind]
        return kind + str(ids.setdefault(key, len(ids) + 1))


def struct_text(s, ptr):
    out = []
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is C.c_void_p:
            out.append(f"{name}={ptr('p', v)}")
        elif isinstance(v, C.Structure):
            out.append(f"{name}=({struct_text(v, ptr)})")
        elif isinstance(v, C.Array):
            out.append(f"{name}={list(v)}")
        else:
            out.append(f"{name}={v!r}")
    return " ".join(out)


def value_text(a, typ, ptr, tables):
    """One argument of a recorded C call."""
    if hasattr(a, "_obj"):                                    # byref(struct or array of structs)
        a = a._obj
    if isinstance(a, C.Array):
        return "[" + " | ".join(struct_text(e, ptr) if isinstance(e, C.Structure) else repr(e) for e in a) + "]"
    if isinstance(a, C.Structure):
        return "(" + struct_text(a, ptr) + ")"
    if isinstance(a, C._Pointer):
        return "(" + struct_text(a.contents, ptr) + ")" if a else "0"
    if isinstance(a, C.c_void_p):
        a = a.value
    if typ is C.c_void_p:
        tab = tables.get(a)
        if tab is not None:                                   # a host descriptor table: its contents, not its address
            return "table[" + " | ".join(struct_text(e, ptr) for e in tab) + "]"
        return ptr("p", a)
    return repr(a.value if hasattr(a, "value") else a)


def torch_arg_text(a, ptr):
    import torch
    if torch.is_tensor(a):
        return f"tensor({ptr('p', a.data_ptr())} {tuple(a.shape)} {tuple(a.stride())} {a.dtype})"
    if isinstance(a, torch.cuda.Stream):
        return ptr("p", a.cuda_stream)
    if isinstance(a, torch.cuda.Event):
        return ptr("e", id(a))
    if isinstance(a, (int, float, bool, str, type(None))):
        return repr(a)
    return type(a).__name__


def trace(lst):
    """The lines of a kernels.LaunchList."""
    ptr = Namer()
    tables = {}
    for k in lst.keep:                                        # (device table, host ctypes array, pinned staging): kernels.device_table
        if isinstance(k, tuple) and len(k) == 3 and isinstance(k[1], C.Array):
            tables[C.addressof(k[1])] = k[1]
    lines = []
    for f, args in lst.ops:
        stream = ""
        if type(f).__name__ == "_OnStream":                   # a torch operation re-issued under a side stream
            stream, f = " on " + ptr("p", f.stream.cuda_stream), f.fn
        types = getattr(f, "argtypes", None)
        if types is not None:
            name = f.__name__
            text = [value_text(a, t, ptr, tables) for a, t in zip(args, types)]
        else:
            owner = getattr(f, "__self__", None)
            name = getattr(f, "__name__", type(f).__name__)
            if getattr(f, "mtd_collective", False):
                name = "collective"
            text = [torch_arg_text(a, ptr) for a in args]
            if owner is not None:
                text.insert(0, torch_arg_text(owner, ptr))
        lines.append(name + stream + ": " + ", ".join(text))
    return lines


def record_step(a, torch, dev):
    from mtd_gan_amd import _options, discriminator_path as DP, train_step as TS
    DP.PAIR_DECODERS = bool(a.pair_decoders)
    DP.LOCKSTEP = a.lockstep
    if _options.product("MTD_FORCE_DP", "0") == "1":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    w = TS.FullStepWorkload(dev, 0, 1, a.batch)
    for _ in range(3):
        w.step_list()
    torch.cuda.synchronize()
    if not isinstance(w.recorded, TS.RecordedTrainStep):
        raise RuntimeError(f"the third iteration was not recorded: {getattr(w.model, '_mtd_list_error', None)}")
    return [(f"step B={a.batch} PAIR_DECODERS={DP.PAIR_DECODERS} LOCKSTEP={DP.LOCKSTEP} dp={w.dp is not None}", trace(w.recorded.list))]


def record_modules(a, torch, dev):
    from mtd_gan_amd import kernels as K
    from mtd_gan_amd.arch.Ours import networks as NW
    out = []
    x = torch.rand(a.batch, 1, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev)

    def run(tag, D, call):
        def fwd_bwd():
            xin = x.clone().requires_grad_(True)
            outs = call(D, xin)
            outs = [o for o in (outs if isinstance(outs, tuple) else (outs,)) if o is not None]
            torch.autograd.backward([o.sum() for o in outs])
            K.side_stream(dev).join()
        fwd_bwd()                                             # (workspaces and derived views exist)
        torch.manual_seed(9)                                  # the dropout draw
        lst = K.LaunchList()
        lst.record(fwd_bwd, dev)
        out.append((tag, trace(lst)))

    torch.manual_seed(3)
    D = NW.Multi_Task_Discriminator_Skip(1, 64).to(dev)
    for train in (True, False):
        D.train(train)
        for need_rec in (True, False):
            run(f"Multi_Task_Discriminator_Skip train={train} need_rec={need_rec}", D, lambda D, xin, n=need_rec: D(xin, need_rec=n))
    for cls in ("CLS_Discriminator", "SEG_Discriminator", "CLS_SEG_Discriminator", "CLS_REC_Discriminator", "SEG_REC_Discriminator"):
        Dp = getattr(NW, cls)(1, 64).to(dev).train()
        run(cls, Dp, lambda D, xin: D(xin))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenario", choices=("step", "module"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--pair-decoders", type=int, default=1)
    ap.add_argument("--lockstep", type=int, default=1)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import mtd_gan_amd
    print("tracing", os.path.dirname(mtd_gan_amd.__file__))
    assert torch.cuda.is_available(), "launch_trace records on the GPU"
    dev = torch.device("cuda", 0)
    sections = (record_step if a.scenario == "step" else record_modules)(a, torch, dev)
    with open(a.out, "w") as fh:
        for tag, lines in sections:
            fh.write(f"# {tag}: {len(lines)} entries\n")
            fh.write("\n".join(lines) + "\n")
            print(f"{tag}: {len(lines)} entries")


if __name__ == "__main__":
    main()
