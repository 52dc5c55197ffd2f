"""FID's InceptionV3 feature network on the HIP kernels -- mirror of module/piq/feature_extractors/fid_inception.py:27-316 with
output_blocks=[3], as metrics.py:17-31 (compute_feat) builds it.  DESIGN 3.9.

The caller hands over the checkpoint (a state dict in torchvision's `Inception3` key layout; the reference downloads pt_inception-
2015-12-05); no weights ship with this package.  Every layer is conv (no bias) -> BatchNorm(eps 1e-3, eval) -> ReLU: the
BatchNorm is folded into the conv on the host in float64, once, and the 94 convolutions are `kernels.conv` launches with bias and
ReLU in their epilogue.  The ends of a block's branches write straight into their channel slice of the block's output, the three
3x3 pools, the input resize and the final mean are the kernels of csrc/inception.hip.  Inference only."""
import torch

from . import _lib
from . import kernels as K

POOL_MAX_S2, POOL_MAX_S1P1, POOL_AVG_S1P1 = 0, 1, 2      # MTD_POOL_*
BN_EPS = 1e-3                        # torchvision BasicConv2d: nn.BatchNorm2d(eps=0.001)
INPUT_SIDE = 299                     # fid_inception.py:151-154
MAX_TAPS = 16                        # the tap tables of the conv kernels (conv_plan.h check_args, mtd_pack_weights)
_MAX_MAP_BYTES = (1 << 31) - 1       # the conv entry points address a map with 32-bit byte offsets: strictly below 2^31 bytes
FIRST = "Conv2d_1a_3x3"


def _pair(v):
    return v if isinstance(v, tuple) else (v, v)


def _build_tables():
    """(convs, blocks, net).  convs: layer name -> (C_in, C_out, (kh, kw), (sh, sw), (ph, pw)) in forward order; blocks: block name
    -> (C_in, branches), a branch = (chain, ends): the ops of `chain` run one after the other from the block's input, every op of
    `ends` reads the chain's result and writes the next channel slice of the block's output; an op is a layer name or a pool mode.
    net: the ops of the whole network, ("conv", name) | ("pool", mode) | ("block", name)."""
    convs, blocks, net = {}, {}, []

    def conv(name, cin, cout, k=1, s=1, p=0):
        convs[name] = (cin, cout, _pair(k), _pair(s), _pair(p))
        return name

    def stem(name, *a, **kw):
        net.append(("conv", conv(name, *a, **kw)))

    def block(name, cin, branches):
        blocks[name] = (cin, branches)
        net.append(("block", name))

    stem(FIRST, 3, 32, k=3, s=2)
    stem("Conv2d_2a_3x3", 32, 32, k=3)
    stem("Conv2d_2b_3x3", 32, 64, k=3, p=1)
    net.append(("pool", POOL_MAX_S2))
    stem("Conv2d_3b_1x1", 64, 80)
    stem("Conv2d_4a_3x3", 80, 192, k=3)
    net.append(("pool", POOL_MAX_S2))
    for m, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):          # FIDInceptionA
        block(m, cin, [
            ([], [conv(f"{m}.branch1x1", cin, 64)]),
            ([conv(f"{m}.branch5x5_1", cin, 48)], [conv(f"{m}.branch5x5_2", 48, 64, k=5, p=2)]),
            ([conv(f"{m}.branch3x3dbl_1", cin, 64), conv(f"{m}.branch3x3dbl_2", 64, 96, k=3, p=1)], [conv(f"{m}.branch3x3dbl_3", 96, 96, k=3, p=1)]),
            ([POOL_AVG_S1P1], [conv(f"{m}.branch_pool", cin, pf)])])
    m = "Mixed_6a"                                                                                       # InceptionB
    block(m, 288, [
        ([], [conv(f"{m}.branch3x3", 288, 384, k=3, s=2)]),
        ([conv(f"{m}.branch3x3dbl_1", 288, 64), conv(f"{m}.branch3x3dbl_2", 64, 96, k=3, p=1)], [conv(f"{m}.branch3x3dbl_3", 96, 96, k=3, s=2)]),
        ([], [POOL_MAX_S2])])
    for m, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):          # FIDInceptionC
        row, col = dict(k=(1, 7), p=(0, 3)), dict(k=(7, 1), p=(3, 0))
        block(m, 768, [
            ([], [conv(f"{m}.branch1x1", 768, 192)]),
            ([conv(f"{m}.branch7x7_1", 768, c7), conv(f"{m}.branch7x7_2", c7, c7, **row)], [conv(f"{m}.branch7x7_3", c7, 192, **col)]),
            ([conv(f"{m}.branch7x7dbl_1", 768, c7), conv(f"{m}.branch7x7dbl_2", c7, c7, **col), conv(f"{m}.branch7x7dbl_3", c7, c7, **row),
              conv(f"{m}.branch7x7dbl_4", c7, c7, **col)], [conv(f"{m}.branch7x7dbl_5", c7, 192, **row)]),
            ([POOL_AVG_S1P1], [conv(f"{m}.branch_pool", 768, 192)])])
    m = "Mixed_7a"                                                                                       # InceptionD
    block(m, 768, [
        ([conv(f"{m}.branch3x3_1", 768, 192)], [conv(f"{m}.branch3x3_2", 192, 320, k=3, s=2)]),
        ([conv(f"{m}.branch7x7x3_1", 768, 192), conv(f"{m}.branch7x7x3_2", 192, 192, k=(1, 7), p=(0, 3)),
          conv(f"{m}.branch7x7x3_3", 192, 192, k=(7, 1), p=(3, 0))], [conv(f"{m}.branch7x7x3_4", 192, 192, k=3, s=2)]),
        ([], [POOL_MAX_S2])])
    for m, cin, pool in (("Mixed_7b", 1280, POOL_AVG_S1P1), ("Mixed_7c", 2048, POOL_MAX_S1P1)):          # FIDInceptionE1 / E2
        row, col = dict(k=(1, 3), p=(0, 1)), dict(k=(3, 1), p=(1, 0))
        block(m, cin, [
            ([], [conv(f"{m}.branch1x1", cin, 320)]),
            ([conv(f"{m}.branch3x3_1", cin, 384)], [conv(f"{m}.branch3x3_2a", 384, 384, **row), conv(f"{m}.branch3x3_2b", 384, 384, **col)]),
            ([conv(f"{m}.branch3x3dbl_1", cin, 448), conv(f"{m}.branch3x3dbl_2", 448, 384, k=3, p=1)],
             [conv(f"{m}.branch3x3dbl_3a", 384, 384, **row), conv(f"{m}.branch3x3dbl_3b", 384, 384, **col)]),
            ([pool], [conv(f"{m}.branch_pool", cin, 192)])])
    return convs, blocks, net


CONVS, BLOCKS, NET = _build_tables()


def block_width(name):
    """Channels of a block's output: the sum over its branch ends (a pool end passes the block's input channels on)."""
    cin, branches = BLOCKS[name]
    return sum(CONVS[op][1] if isinstance(op, str) else cin for _chain, ends in branches for op in ends)


def padded(c):
    """The channel count a map of c channels is stored with: the implicit GEMM takes multiples of 32 (48 -> 64, 80 -> 96, zero
    lanes); the image itself (1 or 3 channels) goes through the direct kernels as it is."""
    return c if c <= 3 else (c + 31) // 32 * 32


def out_side(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def fold_batchnorm(w, gamma, beta, mean, var, eps=BN_EPS):
    """Eval-mode BatchNorm folded into the bias-free conv in front of it, in float64:
    w' = w gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps).  Returns float64 (w', b')."""
    w, gamma, beta, mean, var = (t.detach().double() for t in (w, gamma, beta, mean, var))
    root = torch.sqrt(var + eps)
    return w * gamma.view(-1, 1, 1, 1) / root.view(-1, 1, 1, 1), beta - mean * gamma / root


def split_taps(w):
    """A (N, C, kh, kw) weight as the tensors of the launches that carry it: whole kernel rows, at most MAX_TAPS taps each --
    [(rows r0 .. r1 - 1 as a contiguous tensor, (r0, r1))]; one entry unless kh kw > MAX_TAPS (the 5x5 layers: rows 0-2 and 3-4)."""
    kh, kw = w.shape[2:]
    if kh * kw <= MAX_TAPS:
        return [(w.contiguous(), (0, kh))]
    per = MAX_TAPS // kw
    if per < 1:
        raise ValueError(f"a kernel row of {kw} taps does not fit one launch ({MAX_TAPS} taps)")
    return [(w[:, :, r:r + per].contiguous(), (r, min(r + per, kh))) for r in range(0, kh, per)]


# ------------------------------------------------------------------------------------------------ the kernels of csrc/inception.hip
def _on_device(name, x, out=None):
    if not x.is_cuda or x.dtype != torch.float32 or (out is not None and (out.device != x.device or out.dtype != torch.float32)):
        raise RuntimeError(f"{name}: HIP path needs fp32 CUDA tensors on one device (no CPU fallback)")


def resize_bilinear(x, size, normalize=False):
    """F.interpolate(x, size, mode="bilinear", align_corners=False) of a contiguous (B, C, H, W) fp32 CUDA batch, C <= 4, then
    2 x - 1 if `normalize`: an NHWC (B, OH, OW, C) map (mtd_resize_bilinear).  size == (H, W) only changes the layout."""
    _on_device("resize_bilinear", x)
    B, Cc, H, W = x.shape
    out = torch.empty((B, size[0], size[1], Cc), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mtd_resize_bilinear(x.data_ptr(), Cc * H * W, H * W, 1, out.data_ptr(), Cc, B, Cc, H, W, size[0], size[1],
                                              1 if normalize else 0, K.stream_ptr()), "mtd_resize_bilinear")
    return out


def pool_out_side(n, mode):
    return (n - 3) // 2 + 1 if mode == POOL_MAX_S2 else n


def pool3x3(x, mode, out=None):
    """One of the network's three 3x3 pools of an NHWC fp32 map (a channel slice of a wider map will do), into `out` -- as a rule a
    channel slice of a block's output -- or a new map (mtd_pool3x3)."""
    _on_device("pool3x3", x, out)
    B, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((B, pool_out_side(H, mode), pool_out_side(W, mode), Cc), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (B, pool_out_side(H, mode), pool_out_side(W, mode), Cc):
        raise ValueError(f"pool3x3: mode {mode} of a {tuple(x.shape)} map into {tuple(out.shape)}: shapes do not fit")
    _lib.check(_lib.lib().mtd_pool3x3(x.data_ptr(), K.ld_of(x), out.data_ptr(), K.ld_of(out), B, H, W, Cc, mode, K.stream_ptr()), "mtd_pool3x3")
    return out


def global_avgpool(x):
    """(B, H, W, C) NHWC fp32 -> (B, C): the mean over the map (mtd_global_avgpool)."""
    _on_device("global_avgpool", x)
    B, H, W, Cc = x.shape
    out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mtd_global_avgpool(x.data_ptr(), K.ld_of(x), out.data_ptr(), Cc, B, H, W, Cc, K.stream_ptr()), "mtd_global_avgpool")
    return out


def conv_relu(x, parts, bias, k, s, p, out=None):
    """relu(conv2d(x, W, stride s, padding p) + bias) of an NHWC map on kernels.conv, W given as split_taps(W).  `out`: an NHWC map
    or channel slice of N channels (default: a new map).  More than one part: the leading ones leave their partial sums in a
    scratch map, the last adds them up (add1) under the bias and the ReLU."""
    B, H, W, Cc = x.shape
    if not x.is_cuda or any(t.device != x.device for t in [bias] + [w for w, _rows in parts]):
        raise RuntimeError("conv_relu: the map, the weights and the bias must be on one CUDA device (no CPU fallback)")
    N = parts[0][0].shape[0]
    kh = parts[-1][1][1]
    kw = parts[0][0].shape[3]
    OH, OW = out_side(H, kh, s[0], p[0]), out_side(W, kw, s[1], p[1])
    if out is None:
        out = torch.empty((B, OH, OW, N), dtype=torch.float32, device=x.device)
    if any(w.shape[1] != Cc or w.shape[0] != N for w, _rows in parts) or bias.numel() != N or tuple(out.shape) != (B, OH, OW, N) or out.device != x.device:
        raise ValueError(f"conv_relu: a {tuple(parts[0][0].shape)} layer on a {tuple(x.shape)} map into {tuple(out.shape)}: shapes do not fit")
    acc = None
    for i, (w, rows) in enumerate(parts):
        taps = (rows[1] - rows[0]) * kw
        geom = K.geom_fwd_rect(B, H, W, (kh, kw), s, p, rows if len(parts) > 1 else None)
        if i + 1 < len(parts):
            nxt = torch.empty((B, OH, OW, N), dtype=torch.float32, device=x.device)
            K.conv(x, w, geom, N, Cc, Cc * taps, taps, nxt, add1=acc)
            acc = nxt
        else:
            K.conv(x, w, geom, N, Cc, Cc * taps, taps, out, add1=acc, bias=bias, act=_lib.ACT_RELU)
    return out


class _Layer:
    """One folded conv: weight (N', C', kh, kw) and bias (N') in fp32 with the zero lanes of the padded channel counts, `parts` =
    split_taps(weight), and for the first layer `single`, the parts of its 1 -> 32 form."""
    __slots__ = ("k", "s", "p", "weight", "bias", "parts", "single")


class InceptionV3Features:
    """piq's FID InceptionV3 up to the final average pool (output block 3) on the HIP kernels: (B, 3, H, W) or (B, 1, H, W) fp32 CUDA
    images -> (B, 2048) fp32 features.

    `weights`: a state dict in torchvision's `Inception3` key layout -- <layer>.conv.weight and <layer>.bn.{weight, bias,
    running_mean, running_var} for the 94 layers of CONVS; fc.*, AuxLogits.* and num_batches_tracked are ignored -- or a path to one
    (read with torch.load(..., weights_only=True)).  A missing key or a wrong shape raises ValueError naming the key.  The
    BatchNorms are folded in float64 here, once; the weights go to the device of the first call's input, once.

    A single-channel batch stands for x.repeat(1, 3, 1, 1) (metrics.py:23-25): the first layer's three input slices are summed once,
    here, and `takes_single_channel` tells compute_feat to hand the images over as they are.

    resize_input: bilinear resize to 299 x 299 (F.interpolate, align_corners=False, no antialiasing); normalize_input: 2 x - 1
    (inputs in [0, 1]).  The reference's assertion that the input lies in that range (fid_inception.py:146-148) is NOT reproduced:
    it is a device -> host read per call, and the test loop feeds windowed inputs and a clipped prediction."""

    takes_single_channel = True

    def __init__(self, weights, resize_input=True, normalize_input=True):
        if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            weights = torch.load(weights, map_location="cpu", weights_only=True)
        self.resize_input, self.normalize_input = bool(resize_input), bool(normalize_input)
        self.layers = {}
        for name, (cin, cout, k, s, p) in CONVS.items():
            got = []
            for leaf, shape in (("conv.weight", (cout, cin) + k), ("bn.weight", (cout,)), ("bn.bias", (cout,)),
                                ("bn.running_mean", (cout,)), ("bn.running_var", (cout,))):
                key = f"{name}.{leaf}"
                if key not in weights:
                    raise ValueError(f"InceptionV3Features: the state dict has no {key!r}")
                t = weights[key]
                if not torch.is_tensor(t) or tuple(t.shape) != shape:
                    raise ValueError(f"InceptionV3Features: {key!r} has shape {tuple(getattr(t, 'shape', ()))}, expected {shape}")
                got.append(t)
            wf, bf = fold_batchnorm(*got)
            L = _Layer()
            L.k, L.s, L.p, L.single = k, s, p, None
            w = torch.zeros((padded(cout), padded(cin)) + k, dtype=torch.float64)
            w[:cout, :cin] = wf
            b = torch.zeros(padded(cout), dtype=torch.float64)
            b[:cout] = bf
            L.weight, L.bias = w.float().contiguous(), b.float().contiguous()
            L.parts = split_taps(L.weight)
            if name == FIRST:
                L.single = split_taps(wf.sum(dim=1, keepdim=True).float())
            self.layers[name] = L
        self._device = None

    def to(self, device):
        device = torch.device(device)
        if self._device != device:
            for L in self.layers.values():
                L.weight, L.bias = L.weight.to(device), L.bias.to(device)
                L.parts = split_taps(L.weight)
                if L.single is not None:
                    L.single = [(w.to(device), rows) for w, rows in L.single]
            self._device = device
        return self

    # -------------------------------------------------------------------------------------------- schedule
    def conv_layer(self, name, x, out=None):
        """Layer `name` (conv + folded BatchNorm + ReLU) of an NHWC map with the layer's padded input channel count (the image
        itself: 3 channels, or 1 for the first layer's folded form)."""
        if not x.is_cuda:
            raise RuntimeError("InceptionV3Features: HIP path needs CUDA tensors (no CPU fallback)")
        self.to(x.device)
        L = self.layers[name]
        parts = L.single if (L.single is not None and x.shape[3] == 1) else L.parts
        if x.shape[3] != parts[0][0].shape[1]:
            raise ValueError(f"InceptionV3Features: {name} takes {parts[0][0].shape[1]} channels, got {x.shape[3]}")
        return conv_relu(x, parts, L.bias, L.k, L.s, L.p, out)

    def _op(self, op, x, out=None):
        return self.conv_layer(op, x, out) if isinstance(op, str) else pool3x3(x, op, out)

    def run_block(self, name, x):
        """One Mixed_* block of an NHWC (B, H, W, C_in) map: the NHWC block output, every branch end in its channel slice."""
        cin, branches = BLOCKS[name]
        B, H, W, Cc = x.shape
        if Cc != cin:
            raise ValueError(f"InceptionV3Features: {name} takes {cin} channels, got {Cc}")
        out, off = None, 0
        for chain, ends in branches:
            t = x
            for op in chain:
                t = self._op(op, t)
            for op in ends:
                if isinstance(op, str):
                    _ci, width, k, s, p = CONVS[op]
                    oh, ow = out_side(t.shape[1], k[0], s[0], p[0]), out_side(t.shape[2], k[1], s[1], p[1])
                else:
                    width, oh, ow = cin, pool_out_side(t.shape[1], op), pool_out_side(t.shape[2], op)
                if out is None:
                    out = torch.empty((B, oh, ow, block_width(name)), dtype=torch.float32, device=x.device)
                self._op(op, t, out[:, :, :, off:off + width])
                off += width
        return out

    def _chunk(self, x, side):
        t = resize_bilinear(x, side, self.normalize_input)
        for step in NET:
            if step[0] == "conv":
                t = self.conv_layer(step[1], t)
            elif step[0] == "pool":
                t = pool3x3(t, step[1])
            else:
                t = self.run_block(step[1], t)
        return global_avgpool(t)

    @staticmethod
    def _largest_map_bytes(side):
        """Bytes per image of the largest map (Conv2d_2b_3x3's: 64 channels at 147 x 147 for the 299 x 299 input), or 0 where the
        image is too small to reach the last block."""
        h, w = side
        largest = h * w * 3
        for step in NET:
            if step[0] == "conv":
                _ci, cout, k, s, p = CONVS[step[1]]
                h, w, c = out_side(h, k[0], s[0], p[0]), out_side(w, k[1], s[1], p[1]), padded(cout)
            elif step[0] == "pool":
                h, w = pool_out_side(h, step[1]), pool_out_side(w, step[1])
            else:
                cin, branches = BLOCKS[step[1]]
                if any(not isinstance(op, str) and op == POOL_MAX_S2 for _chain, ends in branches for op in ends):
                    h, w = pool_out_side(h, POOL_MAX_S2), pool_out_side(w, POOL_MAX_S2)
                c = max(block_width(step[1]), cin)
            if h < 1 or w < 1:
                return 0
            largest = max(largest, h * w * c)
        return largest * 4

    @torch.no_grad()
    def __call__(self, x):
        """x: (B, 3, H, W) or (B, 1, H, W) fp32 CUDA (without resize_input: H, W >= 75).  Returns (B, 2048) fp32."""
        if x.dim() != 4 or x.shape[1] not in (1, 3):
            raise AssertionError("InceptionV3Features expects a (B,3,H,W) or (B,1,H,W) tensor")
        if not x.is_cuda:
            raise RuntimeError("InceptionV3Features: HIP path needs CUDA tensors (no CPU fallback)")
        B, _, H, W = x.shape
        if B < 1 or H < 1 or W < 1:
            raise ValueError(f"InceptionV3Features: empty batch {tuple(x.shape)}")
        side = (INPUT_SIDE, INPUT_SIDE) if self.resize_input else (H, W)
        per_image = self._largest_map_bytes(side)
        if per_image == 0:
            raise ValueError(f"InceptionV3Features: a {H} x {W} image does not reach the last block (at least 75 x 75 without resize_input)")
        if per_image > _MAX_MAP_BYTES:
            raise ValueError(f"InceptionV3Features: a {H} x {W} image gives a map of 2^31 bytes or more")
        self.to(x.device)
        x = x.detach().contiguous().float()
        step = max(1, _MAX_MAP_BYTES // per_image)
        if B <= step:
            return self._chunk(x, side)
        return torch.cat([self._chunk(x[i:i + step], side) for i in range(0, B, step)])
