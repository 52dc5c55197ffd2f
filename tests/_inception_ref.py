"""FID's InceptionV3 (piq's fid_inception with output block 3) restated in plain torch for the parity tests: table-driven, NCHW, in
whatever dtype the input has (float64 for the reference, float32 for the error of an ordinary fp32 evaluation).  Written from the
layer table of the network and the block forwards of the reference; parity of the HIP network is pinned to THIS file (torchvision
is not available where the tests run, so piq's own class cannot be instantiated: parity with piq itself is unpinned).

Every layer is conv (no bias) -> BatchNorm(eps 1e-3, running statistics) -> ReLU, evaluated as such -- unfolded."""
import torch
import torch.nn.functional as F

EPS = 1e-3
ROW7, COL7 = ((1, 7), 1, (0, 3)), ((7, 1), 1, (3, 0))
ROW3, COL3 = ((1, 3), 1, (0, 1)), ((3, 1), 1, (1, 0))

# layer -> (C_in, C_out, kernel, stride, padding)
STEM = [("Conv2d_1a_3x3", 3, 32, 3, 2, 0), ("Conv2d_2a_3x3", 32, 32, 3, 1, 0), ("Conv2d_2b_3x3", 32, 64, 3, 1, 1), "maxpool",
        ("Conv2d_3b_1x1", 64, 80, 1, 1, 0), ("Conv2d_4a_3x3", 80, 192, 3, 1, 0), "maxpool"]
# block -> (kind, C_in, parameter): A: pool features, C: channels_7x7, E: the pool in front of branch_pool
BLOCK_LIST = [("Mixed_5b", "A", 192, 32), ("Mixed_5c", "A", 256, 64), ("Mixed_5d", "A", 288, 64), ("Mixed_6a", "B", 288, None),
              ("Mixed_6b", "C", 768, 128), ("Mixed_6c", "C", 768, 160), ("Mixed_6d", "C", 768, 160), ("Mixed_6e", "C", 768, 192),
              ("Mixed_7a", "D", 768, None), ("Mixed_7b", "E", 1280, "avg"), ("Mixed_7c", "E", 2048, "max")]
WIDTHS = {"Mixed_5b": 256, "Mixed_5c": 288, "Mixed_5d": 288, "Mixed_6a": 768, "Mixed_6b": 768, "Mixed_6c": 768, "Mixed_6d": 768,
          "Mixed_6e": 768, "Mixed_7a": 1280, "Mixed_7b": 2048, "Mixed_7c": 2048}


def block_layers(kind, cin, par):
    """branch layer -> (C_in, C_out, kernel, stride, padding) of one block kind."""
    if kind == "A":
        return {"branch1x1": (cin, 64, 1, 1, 0), "branch5x5_1": (cin, 48, 1, 1, 0), "branch5x5_2": (48, 64, 5, 1, 2),
                "branch3x3dbl_1": (cin, 64, 1, 1, 0), "branch3x3dbl_2": (64, 96, 3, 1, 1), "branch3x3dbl_3": (96, 96, 3, 1, 1),
                "branch_pool": (cin, par, 1, 1, 0)}
    if kind == "B":
        return {"branch3x3": (cin, 384, 3, 2, 0), "branch3x3dbl_1": (cin, 64, 1, 1, 0), "branch3x3dbl_2": (64, 96, 3, 1, 1),
                "branch3x3dbl_3": (96, 96, 3, 2, 0)}
    if kind == "C":
        c7 = par
        return {"branch1x1": (cin, 192, 1, 1, 0), "branch7x7_1": (cin, c7, 1, 1, 0), "branch7x7_2": (c7, c7) + ROW7, "branch7x7_3": (c7, 192) + COL7,
                "branch7x7dbl_1": (cin, c7, 1, 1, 0), "branch7x7dbl_2": (c7, c7) + COL7, "branch7x7dbl_3": (c7, c7) + ROW7,
                "branch7x7dbl_4": (c7, c7) + COL7, "branch7x7dbl_5": (c7, 192) + ROW7, "branch_pool": (cin, 192, 1, 1, 0)}
    if kind == "D":
        return {"branch3x3_1": (cin, 192, 1, 1, 0), "branch3x3_2": (192, 320, 3, 2, 0), "branch7x7x3_1": (cin, 192, 1, 1, 0),
                "branch7x7x3_2": (192, 192) + ROW7, "branch7x7x3_3": (192, 192) + COL7, "branch7x7x3_4": (192, 192, 3, 2, 0)}
    if kind == "E":
        return {"branch1x1": (cin, 320, 1, 1, 0), "branch3x3_1": (cin, 384, 1, 1, 0), "branch3x3_2a": (384, 384) + ROW3, "branch3x3_2b": (384, 384) + COL3,
                "branch3x3dbl_1": (cin, 448, 1, 1, 0), "branch3x3dbl_2": (448, 384, 3, 1, 1), "branch3x3dbl_3a": (384, 384) + ROW3,
                "branch3x3dbl_3b": (384, 384) + COL3, "branch_pool": (cin, 192, 1, 1, 0)}
    raise KeyError(kind)


def all_layers():
    """Every conv of the network: full layer name -> (C_in, C_out, kernel, stride, padding), in forward order."""
    out = {s[0]: s[1:] for s in STEM if not isinstance(s, str)}
    for name, kind, cin, par in BLOCK_LIST:
        for leaf, spec in block_layers(kind, cin, par).items():
            out[f"{name}.{leaf}"] = spec
    return out


def _two(v):
    return v if isinstance(v, tuple) else (v, v)


def seeded_state_dict(seed, only=None):
    """A torchvision-layout Inception3 state dict with seeded values that keep activations O(1) through all 94 layers: He-scaled
    conv weights, gamma ~ 1, small beta and running mean, running variance in [0.5, 1.5]; plus the fc / AuxLogits /
    num_batches_tracked entries a real checkpoint carries.  only: a block name -- just that block's layers (block tests)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (cin, cout, k, _s, _p) in all_layers().items():
        if only is not None and not name.startswith(only + "."):
            continue
        kh, kw = _two(k)
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
        sd[f"{name}.bn.weight"] = 1.0 + 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_var"] = 0.5 + torch.rand(cout, generator=g)
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(1000)
    if only is None:
        sd["fc.weight"], sd["fc.bias"] = torch.zeros(1008, 2048), torch.zeros(1008)
        sd["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    return sd


def layer(sd, name, spec, x):
    """BasicConv2d: relu(batch_norm(conv2d(x))) with the running statistics, in x's dtype."""
    _cin, _cout, k, s, p = spec
    t = lambda leaf: sd[f"{name}.{leaf}"].to(x.dtype)
    y = F.conv2d(x, t("conv.weight"), None, stride=_two(s), padding=_two(p))
    y = F.batch_norm(y, t("bn.running_mean"), t("bn.running_var"), t("bn.weight"), t("bn.bias"), training=False, eps=EPS)
    return F.relu(y)


def avgpool(x):
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


def block(sd, name, x):
    """One Mixed_* block on an NCHW map."""
    kind, cin, par = next(b[1:] for b in BLOCK_LIST if b[0] == name)
    spec = block_layers(kind, cin, par)
    run = lambda leaf, t: layer(sd, f"{name}.{leaf}", spec[leaf], t)
    chain = lambda t, *leaves: t if not leaves else chain(run(leaves[0], t), *leaves[1:])
    if kind == "A":
        outs = [run("branch1x1", x), chain(x, "branch5x5_1", "branch5x5_2"), chain(x, "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"),
                run("branch_pool", avgpool(x))]
    elif kind == "B":
        outs = [run("branch3x3", x), chain(x, "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), F.max_pool2d(x, 3, stride=2)]
    elif kind == "C":
        outs = [run("branch1x1", x), chain(x, "branch7x7_1", "branch7x7_2", "branch7x7_3"),
                chain(x, "branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"), run("branch_pool", avgpool(x))]
    elif kind == "D":
        outs = [chain(x, "branch3x3_1", "branch3x3_2"), chain(x, "branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"),
                F.max_pool2d(x, 3, stride=2)]
    else:
        a = run("branch3x3_1", x)
        b = chain(x, "branch3x3dbl_1", "branch3x3dbl_2")
        pooled = avgpool(x) if par == "avg" else F.max_pool2d(x, 3, stride=1, padding=1)
        outs = [run("branch1x1", x), run("branch3x3_2a", a), run("branch3x3_2b", a), run("branch3x3dbl_3a", b), run("branch3x3dbl_3b", b),
                run("branch_pool", pooled)]
    return torch.cat(outs, 1)


def features(sd, x, resize_input=True, normalize_input=True):
    """(B, 3, H, W) in [0, 1] -> (B, 2048), in x's dtype."""
    if resize_input:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    if normalize_input:
        x = 2 * x - 1
    for s in STEM:
        x = F.max_pool2d(x, 3, stride=2) if isinstance(s, str) else layer(sd, s[0], s[1:], x)
    for name, _kind, _cin, _par in BLOCK_LIST:
        x = block(sd, name, x)
    return x.mean(dim=(2, 3))
