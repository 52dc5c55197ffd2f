/*
 * libmtdgan_hip.so -- C ABI of the MI355X (gfx950) kernels behind the MTD-GAN training hot path.
 *
 * The reference (babbu3682/MTD-GAN) is pure Python: it has no FFI of its own, every op below is an
 * ATen call made from the reference file:line cited at the entry point that replaces it.  This header
 * is therefore the boundary a maintainer binds with ctypes/cffi; the host-side
 * mirror of the reference's module surface lives in mtd-gan_amd/ (arch/Ours/networks.py etc.).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated; activations are NHWC with an explicit
 *     leading dimension `ld` (floats between consecutive pixels, >= channels) so channel slices of a
 *     wider tensor can be read/written in place; weights keep PyTorch's OIHW (Conv2d) / IOHW
 *     (ConvTranspose2d) layout and are addressed through (w_sn, w_sc) element strides;
 *   - the library never allocates, frees or synchronises; work is enqueued on `stream`
 *     (a hipStream_t passed as void*); workspaces are sized by the *_ws_bytes helpers;
 *   - every entry point returns 0 on success, a negative MTD_E* code for argument errors, or a
 *     positive hipError_t from the launch.
 */
#ifndef MTDGAN_HIP_H
#define MTDGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTD_OK 0
#define MTD_EINVAL (-1)   /* bad shape / null pointer / unsupported combination */
#define MTD_EALIGN (-2)   /* pointer or leading dimension not 16-byte aligned where required */
#define MTD_EWS (-3)      /* workspace too small */

#define MTD_ACT_NONE 0
#define MTD_ACT_RELU 1
#define MTD_ACT_LRELU 2   /* LeakyReLU(0.2) -- arch/Ours/networks.py:182 etc. */
/* Round 4: relu(acc * scale + bias) + add1 + add2 -- the residual operands added AFTER the activation: x + relu(conv3x3(x) + b)
 * of FFT_ConvBlock.forward (networks.py:31-35) in one launch for whole-slice inference, where the block's third term then
 * needs one operand less.  Only where mtd_conv_relu_add_ok() says so (mtd_conv_igemm on the generator-shaped 32-channel 3x3
 * layers whose plan is the persistent kernel; no mask, no out2); every other entry point answers MTD_EINVAL to it. */
#define MTD_ACT_RELU_ADD 3

/* Gather geometry shared by conv forward, data-gradient and weight-gradient kernels.
 * For launch-grid pixel (b, oy, ox), tap (ty, tx):
 *     iy = oy*in_sy + off_y + ty*tap_dy        ix = ox*in_sx + off_x + tx*tap_dx
 *     kidx = (ky0 + ty*ky_step)*KW + (kx0 + tx*kx_step)          (index into the kh*kw plane)
 * and the result pixel is written at (oy*out_sy + out_oy, ox*out_sx + out_ox) of an OHF x OWF image.
 *   conv fwd  (k,s,p): in_s=s, off=-p, tap_d=+1, TH=TW=k, ky0=0, ky_step=1, out_s=1, out_o=0
 *   dgrad s=1 (k,p)  : in_s=1, off=+p, tap_d=-1, TH=TW=k               (also ConvTranspose2d fwd)
 *   dgrad s=2 k=4 p=1: one launch per output parity (py,px): TH=TW=2, ky0=(py+1)&1, ky_step=2,
 *                      off=(py+1-ky0)/2, tap_d=-1, out_s=2, out_o=py */
typedef struct {
    int B, IH, IW;          /* gathered tensor: batch, height, width                      */
    int OH, OW;             /* launch grid (pixels enumerated per image)                  */
    int in_sy, in_sx, off_y, off_x, tap_dy, tap_dx;
    int TH, TW, KW;
    int ky0, kx0, ky_step, kx_step;
    int OHF, OWF, out_sy, out_sx, out_oy, out_ox;
} mtd_geom;

/* Implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 *   out[pix, n] = mask'( act( scale * sum_{tap,c} in[gather(pix,tap), c] * W(n,c,tap) + bias[n]
 *                              + add1[pix,n] + add2[pix,n] ) )
 * Replaces F.conv2d / F.conv_transpose2d / F.linear call sites: arch/Ours/networks.py:18-19,32
 * (block convs), :97-162 (generator encoder/decoder), :385-472 (discriminator), and their autograd
 * data-gradients.  Requires C % 32 == 0, N % 32 == 0 (other shapes: mtd_conv_direct) and a weight view that
 * is contiguous along c (w_sc == 1, 16-byte aligned rows): 1x1 convs / Linear are that natively, other views
 * are re-laid out once per optimizer step by mtd_pack_weights into [tap][n][c]. */
typedef struct {
    mtd_geom g;
    const float* in;  int in_ld;  int C;
    const float* w;   long long w_sn, w_sc, w_st; /* W(n,c,kidx) = w[n*w_sn + c*w_sc + kidx*w_st] */
    int N;
    float* out;       int out_ld;
    const float* scale;                          /* device scalar (1/sigma) or NULL        */
    const float* bias;                           /* [N] or NULL                            */
    const float* add1; int add1_ld;
    const float* add2; int add2_ld;
    int act;
    const float* mask; int mask_ld; float mask_slope;  /* v *= (mask>0 ? 1 : mask_slope)  */
    float* ws; size_t ws_bytes;                  /* split-K slabs (see mtd_conv_igemm_ws_bytes) */
    const float* scale2; int scale_split;        /* optional second scale: launch-grid pixels >= scale_split use *scale2.  Two
                                                    discriminator passes with their own spectral-norm sigma share one launch
                                                    (batch halves); 0 / NULL = one scale for all pixels */
    float* out2; int out2_ld;                    /* optional second output: the value BEFORE the mask factor (out gets it after).
                                                    A data-gradient launch then also hands the next layer's activation-masked
                                                    cotangent over.  Halo-tile kernel only (C == 32, 3x3, 64-pixel rows,
                                                    >= 32768 pixels); MTD_EINVAL on every other path */
    unsigned* tile_ctr; int tile_ctr_len;        /* LAB BUILDS ONLY since round 5 (ignored by the shipped library: the variant lost twice).
                                                    Optional arrival counters of split-K launches: tile_ctr_len zero-initialised
                                                    words that only these launches touch (they leave them zero).  With one word
                                                    per output tile the last slice to arrive at a tile sums the slabs, in slice
                                                    order, and runs the epilogue in the same kernel; NULL / too few = a second
                                                    launch (splitk_epilogue_kernel) does.  Same bits either way.  Launches that
                                                    may run concurrently (different streams) need different counters */
} mtd_conv_args;

size_t mtd_conv_igemm_ws_bytes(const mtd_conv_args* a);
int mtd_conv_igemm(const mtd_conv_args* a, void* stream);
/* ---- Winograd F(2x2, 3x3) form of the same contract (csrc/conv_winograd.hip) for the 3x3 stride-1 "same" layers
 * (arch/Ours/networks.py:181-221 conv{l}1/2, :230-301 *_dconv{l}1/2 and their data gradients): 16 instead of 36
 * multiplications per 2x2 output tile, fp32 MFMA, same epilogue, same split-K workspace contract.
 *   mtd_winograd_weights   transforms `count` weight views (once per optimizer step) into [xi 0..15][C/8][N][8] floats;
 *                          kmap[a*3+b] = index in the kh x kw plane of the filter entry that multiplies input offset
 *                          (-1+a, -1+b) (mtd_winograd_kmap derives it from a geometry: a forward conv and the data
 *                          gradient of the same layer use different maps); table in device memory + the same on the host.
 *   mtd_conv_winograd      a->w = the transformed weights (w_sn / w_sc ignored; w_st = 6 says they are the F(2x4, 3x3) form).  Requires 3x3, stride 1, OH x OW ==
 *                          IH x IW both even, C % 16 == 0, N % 64 == 0 (or C = N = 32 in the F(2x4, 3x3) form), no out2:
 *                          mtd_conv_winograd_ok().  The generator's 32 -> 32 channel layers (arch/Ours/networks.py:95-164) with one
 *                          residual operand at most, no scales and no mask run on a persistent kernel of their own
 *                          (csrc/conv_wino_c32.h; what whole-slice inference spends its conv time in), which also implements
 *                          MTD_ACT_RELU_ADD; with N % 64 == 0 that activation is refused as before. */
/* px: patch width of the transform along x -- 6: F(2x4, 3x3) (round 4: F(2,3) down the rows, F(4,3) along them, 24 positions,
 * 3 multiplications per output pixel; dst holds 24 N C floats), 0 or 4: F(2x2, 3x3) (16 N C floats).  A conv launch says which
 * weights it was given through a->w_st (6 or not); mtd_conv_winograd_patch_w tells the caller which form the library's plan
 * wants for a layer (0: not in the Winograd domain at all).
 * Round 5: px + 16 (20, 22) = the SPLIT-BF16 form of the same transform -- every transformed weight as three bf16 pieces whose sum
 * is the fp32 value exactly, dst = [xi][C/16][plane 0..2][N][16 c] bf16 (4 px N C x 6 bytes; C % 16 == 0): the operand of
 * csrc/conv_winograd_split.h, which forms each fp32 product from six bf16 MFMA products at fp32 accuracy.  The plan asks for it
 * on every layer with N % 64 == 0 after mtd_set_option("wino_split", 1) (off by default: see the option). */
typedef struct { const float* src; float* dst; long long sn, sc, st; int N, C; int kmap[9]; int px; } mtd_wino_weight_desc;
size_t mtd_winograd_weight_floats(int N, int C);      /* 36 N C: enough for every form */
int mtd_conv_winograd_patch_w(const mtd_conv_args* a);
int mtd_conv_winograd_f4_min_w(int min_w);      /* tuning / test hook: narrowest map width that takes F(2x4, 3x3); 0 = never, < 0 = query; returns the previous value */
int mtd_winograd_kmap(const mtd_geom* g, int* kmap9);
int mtd_winograd_weights(const mtd_wino_weight_desc* table_dev, const mtd_wino_weight_desc* table_host, int count, void* stream);
int mtd_conv_winograd_ok(const mtd_conv_args* a);
size_t mtd_conv_winograd_ws_bytes(const mtd_conv_args* a);
int mtd_conv_winograd(const mtd_conv_args* a, void* stream);
/* Two or three convs of ONE shape in one launch (round 6): the mirror layers of the discriminator's pixel-level and restoration
 * decoders (networks.py:420-467: s_dconv{l}k / r_dconv{l}k) and the data gradients of one layer in backward passes that are advanced
 * together.  a[0 .. count) as for mtd_conv_winograd, each with its own operands and workspace (mtd_conv_winograd_ws_bytes of any).
 * The split of K is planned for the group's whole grid (1 / count of the slices per problem): the results equal single calls of
 * mtd_conv_winograd up to the grouping of the K sum (a few 1e-6), bit for bit where neither splits K. */
int mtd_conv_winograd_group_ok(const mtd_conv_args* a, int count);
int mtd_conv_winograd_group(const mtd_conv_args* a, int count, void* stream);

/* ---- Binary16 activation storage for whole-slice inference (engine.py:89,129: the generator on whole 512 x 512 slices).
 * Arithmetic, weights and biases stay fp32; only the maps that one launch stores for a later one are IEEE binary16, rounded to
 * nearest-even from the fp32 value and saturated at +-65504.  mtd_conv_st_args = mtd_conv_args plus the storage type of a.in, a.add1
 * and a.out: a pointer of a binary16 operand travels behind its float type, its stride counts ELEMENTS as before.
 *   mtd_conv_winograd_st   the generator's 32 -> 32 channel layers (networks.py:99-160 encoder / decoder, :18,32 the block's conv) on
 *                          the persistent F(2x4, 3x3) kernel, in / add1 / out all MTD_ST_F16 (all MTD_ST_F32: mtd_conv_winograd
 *                          itself).  a.w = the fp32 transformed weights of mtd_winograd_weights; one residual operand at most,
 *                          MTD_ACT_RELU_ADD included, no scale / mask / out2 / add2.  Anything else: MTD_EINVAL, nothing is launched.
 *   mtd_conv_direct_st     the first layer (networks.py:97 encoder.0, 1 -> N: in MTD_ST_F32, out MTD_ST_F16, no add / mask operands,
 *                          3x3 "same" geometry) and the last (networks.py:162 decoder.0, C -> 1: in MTD_ST_F16, add1 and out
 *                          MTD_ST_F32).  Anything else: MTD_EINVAL. */
enum { MTD_ST_F32 = 0, MTD_ST_F16 = 1 };
typedef struct { mtd_conv_args a; int in_type, add1_type, out_type; } mtd_conv_st_args;
int mtd_conv_winograd_st(const mtd_conv_st_args* a, void* stream);
int mtd_conv_direct_st(const mtd_conv_st_args* a, void* stream);

/* ---- Winograd F(3x3, 2x2) for the 4x4 / stride-2 / padding-1 layers (csrc/conv_wino_s2.h; arch/Ours/networks.py:185-215 down1..3:
 * Conv2d(k4, s2, p1) forward and its four-parity data gradient): the forward conv is a 2x2 stride-1 conv over the 4 C channels of
 * the space-to-depth image of the padded input (never formed: each phase is read at pixel stride 2), each parity class of the
 * data gradient a 2x2 stride-1 conv over the cotangent; 16 multiplications per 3x3 output tile instead of 36.
 *   mtd_winograd_s2_kmap     for a forward geometry (TH = TW = 4, in_s = 2, tap_d = 1): groups = 4 and, per phase (py, px) = group
 *                            2 py + px, the filter entries at correlation positions (jy, jx): kmap16[4 group + 2 jy + jx];
 *                            for a class geometry (TH = TW = 2, in_s = 1, tap_d = +-1): groups = 1, kmap16[0..3].
 *   mtd_winograd_s2_weights  dst = [xi 0..15][groups C / 8][N][8] floats (16 groups N C), once per optimizer step.
 *   mtd_conv_winograd_s2     a[0 .. count) as for mtd_conv_igemm_multi (count = 1: a plain launch), a[i].w = set i's transformed
 *                            weights.  Requires C % 16 == 0, N % 64 == 0, no out2, not MTD_ACT_RELU_ADD; the sets share every operand
 *                            but w, ws and the geometry's offsets: mtd_conv_winograd_s2_ok() (0: no; 1: in the domain; 2: and the
 *                            plan expects it to beat mtd_conv_igemm / _multi on this shape).  Same epilogue, and with split-K the
 *                            same workspace contract: mtd_conv_winograd_s2_ws_bytes() bytes for EACH set. */
typedef struct { const float* src; float* dst; long long sn, sc, st; int N, C, groups; int kmap[16]; } mtd_wino_s2_weight_desc;
int mtd_winograd_s2_kmap(const mtd_geom* g, int* groups, int* kmap16);
int mtd_winograd_s2_weights(const mtd_wino_s2_weight_desc* table_dev, const mtd_wino_s2_weight_desc* table_host, int count, void* stream);
int mtd_conv_winograd_s2_ok(const mtd_conv_args* a, int count);
size_t mtd_conv_winograd_s2_ws_bytes(const mtd_conv_args* a, int count);
int mtd_conv_winograd_s2(const mtd_conv_args* a, int count, void* stream);

/* Up to four launches of ONE shape (same pixels, N, C, taps) as one grid -- the four input-parity classes of a stride-2
 * data gradient (arch/Ours/networks.py down{l}: Conv2d(k4, s2, p1) backward w.r.t. its input), each a 2x2-tap stride-1
 * gather that writes every other pixel of the same output.  a[0..count) are complete argument sets; with split-K each
 * needs its own workspace of mtd_conv_igemm_multi_ws_bytes(a, count) bytes.  No out2. */
size_t mtd_conv_igemm_multi_ws_bytes(const mtd_conv_args* a, int count);
int mtd_conv_igemm_multi(const mtd_conv_args* a, int count, void* stream);

/* dst[(t*N + n)*C + c] = src[n*sn + c*sc + t]  for `count` weight tensors in one launch (table in device
 * memory + the same table on the host for sizing).  N and C multiples of 32, T <= 16. */
typedef struct { const float* src; float* dst; int N, C, T; long long sn, sc; } mtd_pack_desc;
int mtd_pack_weights(const mtd_pack_desc* table_dev, const mtd_pack_desc* table_host, int count, void* stream);

/* Same contract on the vector ALU for degenerate channel counts (C==1, N==1, N or C not a multiple
 * of 32): generator encoder.0 / decoder.0 (networks.py:97,162), discriminator conv11, *_dconv61/62,
 * enc_out/dec_out/rec_out (networks.py:385,441-442,466-472). */
int mtd_conv_direct(const mtd_conv_args* a, void* stream);
int mtd_conv_relu_add_ok(const mtd_conv_args* a);      /* nonzero: mtd_conv_igemm takes these arguments with act = MTD_ACT_RELU_ADD */

/* Weight gradient:  dW(n,c,kidx) (+)= sum_pix p[pix,n] * q[gather(pix,tap),c]
 * (autograd of the conv call sites above).  dw is addressed like W.
 * db (optional, [N]) (+)= sum_pix p[pix,n].  accumulate: bit 0 adds into dw, bit 1 adds into db. */
typedef struct {
    mtd_geom g;
    const float* p; int p_ld; int N;
    const float* q; int q_ld; int C;
    float* dw; long long w_sn, w_sc;
    float* db;
    int accumulate;
    float* ws; size_t ws_bytes;
    /* optional (round 6): the two halves of a paired discriminator pass in ONE launch of the small-map kernels.  half_scale != NULL:
     * the cotangent is multiplied, as it is used, by *half_scale for pixels [0, m_first) and by *half_scale2 for the rest -- dw then
     * holds G_1 / sigma_1 + G_2 / sigma_2 (each half's raw gradient scaled by its own 1 / sigma: what the spectral-norm correction
     * adds up anyway, mtd_sn_grad_layer.prescaled).  db stays the unscaled sum.  m_first must be a multiple of 32 (a chunk of the K
     * loop never straddles the halves); only the register-operand kernels take it (mtd_conv_wgrad_half_scale_ok). */
    const float* half_scale; const float* half_scale2; int m_first;
} mtd_wgrad_args;

size_t mtd_conv_wgrad_ws_bytes(const mtd_wgrad_args* a);
int mtd_conv_wgrad(const mtd_wgrad_args* a, void* stream);
int mtd_conv_wgrad_half_scale_ok(const mtd_wgrad_args* a);      /* nonzero: mtd_conv_wgrad takes these arguments with half_scale set */
/* The kernel the plan picks for these arguments: index into the weight-gradient name table of the launch profiler
 * (16 = wgrad_wino_kernel, Winograd F(2x2,3x3): 4/9 of the layer's multiplications), -1 = the vector-ALU kernels of
 * mtd_conv_direct's domain, MTD_EINVAL = invalid arguments.  Nothing is launched.  (Host-side flop accounting of bench.py.) */
int mtd_conv_wgrad_plan_cfg(const mtd_wgrad_args* a);

/* The two image ranges [0, b_first), [b_first, B) of one batch, a weight gradient each (a->dw and dw2; both bias
 * gradients into a->db, the second accumulated) from ONE launch of the slab-producing kernel: the paired discriminator
 * passes of the D step (D(y) | D(fake) as one batch of 2B, networks.py:1959-1970) need the halves' gradients apart,
 * because each half has its own spectral-norm sigma, u, v.  Same arithmetic per range as mtd_conv_wgrad on that range
 * up to the order of the slab sums.  _ok: nonzero if the layer qualifies (B == 2 b_first, N and C multiples of 32, and a plan
 * whose kernel has the pair form: all but the row-window kernels of the 16-pixel-aligned 3x3 / 1x1 stride-1 layers below
 * 64 channels), else the caller runs mtd_conv_wgrad twice.  _ws_bytes: 0 if it does not qualify. */
int mtd_conv_wgrad_pair_ok(const mtd_wgrad_args* a, int b_first);
/* which plans pair: 0 none, 1 the default rule (Winograd and stride-2 halo-window kernels: the ones a pair launch is
 * faster for), 2 Winograd only, 3 every kernel that has the pair form (tests), -1 the MTD_WGRAD_PAIR environment
 * variable's choice (default 1).  Returns the previous mode. */
int mtd_conv_wgrad_pair_mode(int mode);
size_t mtd_conv_wgrad_pair_ws_bytes(const mtd_wgrad_args* a, int b_first);
int mtd_conv_wgrad_pair(const mtd_wgrad_args* a, float* dw2, int b_first, void* stream);
/* The same with the gradients taken from a->p + p_add, added as the operands are loaded (the decoders' weight gradients of
 * the D step are sums over two task passes' cotangents -- discriminator_path.cot -- and a weight gradient is linear in its
 * cotangent: no pass of its own for the sum).  p_add: shape, pixel stride and alignment of a->p.  Only where
 * mtd_conv_wgrad_pair_ok returns 2 (1: pair form without the second cotangent, 0: no pair form). */
int mtd_conv_wgrad_pair_sum(const mtd_wgrad_args* a, const float* p_add, float* dw2, int b_first, void* stream);

/* Deferred form for a backward pass with many small layers (the generator: 41 conv layers of 32 channels, each with
 * 256 partial-sum slabs).  mtd_conv_wgrad_slabs runs only the slab-producing kernel into a->ws, which must stay
 * untouched until the reduce; *nslab == 0 means the kernel wrote dw / db itself and nothing is left to do.
 * mtd_conv_wgrad_reduce_multi then sums the slabs of `count` layers and scatters into their dw / db in ONE launch
 * (same fixed two-level order as mtd_conv_wgrad's own reduce).  N and C must be multiples of 32. */
typedef struct {
    mtd_wgrad_args a;          /* as passed to mtd_conv_wgrad_slabs (a.ws = the slabs) */
    int T;                     /* taps */
    int nslab;
    long long slab_stride;     /* floats */
    int first_block;           /* filled by the caller: prefix sum of blocks (mtd_conv_wgrad_reduce_blocks) */
    int pad_;
} mtd_wgrad_reduce_desc;
int mtd_conv_wgrad_slabs(const mtd_wgrad_args* a, int* nslab, long long* slab_stride, void* stream);
/* mtd_conv_wgrad_slabs plus mtd_rfft_rows(x, x_ld, R, B, col_weight) -- in one launch when the layer runs on the row-window
 * kernel (3x3, stride 1, one 32 x 32 tile: the generator's blocks, whose weight gradient and spectral backward chain start from
 * the same cotangent), otherwise as two launches. */
int mtd_conv_wgrad_slabs_rfft(const mtd_wgrad_args* a, int* nslab, long long* slab_stride, const float* x, int x_ld, float* R,
                              int B, int col_weight, void* stream);
int mtd_conv_wgrad_reduce_blocks(const mtd_wgrad_reduce_desc* d);
int mtd_conv_wgrad_reduce_multi(const mtd_wgrad_reduce_desc* table_dev, const mtd_wgrad_reduce_desc* table_host, int count, void* stream);

/* ---- Res-FFT-Conv block spectral path (arch/Ours/networks.py:21-30), H = W = 64, C = 32 ------
 * Spectra are stored as [B][kw 0..32][h or kh 0..63][2 (re,im)][32 channels].                  */

/* rows: real FFT along W of x (NHWC, ld), ortho scale 1/8.  col_weight: 0 = none (rfft2 forward),
 * 1 = w(kw) in {1,2,...,2,1} (irfft2 backward). */
int mtd_rfft_rows(const float* x, int x_ld, float* R, int B, int col_weight, void* stream);

/* Tail of a Res-FFT-Conv block in ONE launch (arch/Ours/networks.py:32-36: `x + relu(img_conv(x)) + irfft2(...)`):
 *     out2 = act(conv3x3(in) + bias)        the spatial branch (kept: the backward pass uses it as its ReLU mask; may be NULL)
 *     out  = in + out2 + irfft_rows(T)      T = output of mtd_spec_mix_fwd / _fwd4
 * i.e. mtd_conv_igemm(out = out2) + mtd_irfft_rows(T, out, add1 = in, add2 = out2) without the second launch and its
 * re-reads: the halo-tile conv kernel's tiles are complete image rows, so the inverse row transform runs between its MFMA
 * loop and its epilogue and `in` is taken from the halo tile.  C = N = 32, 3x3 stride 1 "same", 64 x 64 maps, >= 32768
 * pixels, no add / mask / scale2 operands: mtd_resfft_block_tail_ok() says whether a->... qualifies (else MTD_EINVAL). */
int mtd_resfft_block_tail_ok(const mtd_conv_args* a);
int mtd_resfft_block_tail(const mtd_conv_args* a, const float* T, void* stream);

/* columns + channel mix + columns back, one kernel:
 *   S = FFT_H(R)/8 ; Z = W2 . [Re S; Im S] + b2 ; T = IFFT_H(relu(Z))/8
 * w2t is W2 transposed ([k][o], 64x64).  S_save / Z_save ([B][33][64][64]) may be NULL (inference). */
int mtd_spec_mix_fwd(const float* R, const float* w2t, const float* b2, float* T,
                     float* S_save, float* Z_save, int B, void* stream);

/* backward of the above given gR = weighted row-FFT of the upstream gradient:
 *   gZ = FFT_H(gR)/8 * (Z>0) ; gS = W2^T gZ ; gT = IFFT_H(gS)/8 (columns 1..31 halved: rfft2 backward)
 *   dW2 partials (slab per workgroup) and db2 partials go to ws; mtd_spec_mix_wgrad_reduce sums them. */
size_t mtd_spec_mix_bwd_ws_bytes(int B);
int mtd_spec_mix_bwd(const float* gR, const float* w2, const float* S_save, const float* Z_save,
                     float* gT, float* ws, int B, void* stream);
/* Four-wave forms of the two calls above (csrc/resfft4.hip): same mathematics, layouts and slab format; the saved
 * pre-activation is a SIGN MASK of mtd_spec_mix_zmask_bytes(B) bytes (128 64-bit words per patch and kw pair) instead of
 * a float tensor.  S_save and zmask may be NULL in the forward call (no tape). */
size_t mtd_spec_mix_zmask_bytes(int B);
int mtd_spec_mix_fwd4(const float* R, const float* w2t, const float* b2, float* T, float* S_save, void* zmask, int B, void* stream);
int mtd_spec_mix_bwd4(const float* gR, const float* w2, const float* S_save, const void* zmask, float* gT, float* ws, int B,
                      void* stream);
int mtd_spec_mix_wgrad_reduce(const float* ws, int B, float* dw2, float* db2, int accumulate, void* stream);
/* the same reduce for `count` blocks' slab sets in one launch (dw2 and ws 16-byte aligned) */
typedef struct { const float* ws; float* dw2; float* db2; int nslab; int accumulate; } mtd_mix_reduce_desc;
int mtd_spec_mix_wgrad_reduce_multi(const mtd_mix_reduce_desc* table_dev, const mtd_mix_reduce_desc* table_host, int count, void* stream);

/* rows back: c2r along W (uses only Re of columns 0 and 32), ortho 1/8, fused epilogue
 *   out = (y + add1 + add2) * (mask > 0 ? 1 : 0)     (add1/add2/mask optional, NHWC with own ld) */
int mtd_irfft_rows(const float* T, float* out, int out_ld, const float* add1, int add1_ld,
                   const float* add2, int add2_ld, const float* mask, int mask_ld, int B, void* stream);

/* The same three steps for square maps of side S = 128, 256 or 512 (whole-slice inference, reference engine.py:89,129:
 * the generator runs on 512 x 512 images and rfft2 becomes a 512-point transform); these fp32 entry points take S = 64 too (an
 * instantiation of the same kernels, tested like the other sides; the generator sends 64 x 64 maps to the training kernels above).
 * Any other S is MTD_EINVAL.  Pixel strides are at least 32 floats (MTD_EINVAL) and multiples of 4, all bases 16-byte aligned
 * (MTD_EALIGN); add1 / add2 may be NULL.  Forward only; spectra are
 * [B][kw 0..S/2][h 0..S-1][Re 32 | Im 32], ortho scaling 1/sqrt(S) per dimension.  mtd_rfft_rows_any and mtd_spec_mix_any write
 * exact zeros into the imaginary halves of columns 0 and S/2 of R and T; mtd_spec_mix_any and mtd_irfft_rows_any do not read them
 * (torch's c2r ignores them too), and the two columns' real parts go through one packed transform each way. */
int mtd_rfft_rows_any(const float* x, int x_ld, float* R, int B, int S, void* stream);
int mtd_spec_mix_any(const float* R, const float* w2t, const float* b2, float* T, int B, int S, void* stream);
int mtd_irfft_rows_any(const float* T, float* out, int out_ld, const float* add1, int add1_ld, const float* add2,
                       int add2_ld, int B, int S, void* stream);
/* The same three launches with binary16 storage (networks.py:21-36 on whole slices, S = 128 / 256 / 512): x, R, T, add1, add2 and out
 * are binary16 maps with the layouts above (strides in elements and multiples of 4, 16-byte aligned bases); w2t and b2 stay
 * fp32, and so does every value inside a launch (the LDS lines, the transforms, the MFMA channel mix). */
int mtd_rfft_rows_any_h(const void* x, int x_ld, void* R, int B, int S, void* stream);
int mtd_spec_mix_any_h(const void* R, const float* w2t, const float* b2, void* T, int B, int S, void* stream);
int mtd_irfft_rows_any_h(const void* T, void* out, int out_ld, const void* add1, int add1_ld, const void* add2,
                         int add2_ld, int B, int S, void* stream);

/* The same three steps for maps of any size 16 <= H, W <= 512, chosen independently (odd, non-square and prime sides included;
 * the shapes the entry points above refuse).  Spectra as above, [B][kw 0..W/2][h 0..H-1][Re 32 | Im 32] with W/2 + 1 columns
 * (odd W: the last column is an ordinary one, weight 2 on the way back), ortho 1/sqrt(H W) overall.  Transforms: mixed radix
 * 2/3/4/5/7 for 7-smooth lengths, Bluestein (power-of-two convolution of length M >= 2N - 1) otherwise.  ws: a device buffer of
 * at least mtd_spectral_gen_ws_bytes(B, H, W) bytes (the Bluestein filter spectra; 0 = arguments out of range), used in
 * stream order.  mtd_spec_mix_gen zeroes the imaginary halves of column 0 and (even W) column W/2 of T.  R and T: 4-byte
 * aligned; no other alignment needed.  Arguments out of range or null pointers: MTD_EINVAL, nothing launched.
 * mtd_spectral_gen_plan(n, out) reports the plan of a length: returns the number of passes, out[0] = Bluestein length M
 * (0: mixed radix), out[1..] = the radices in decimation-in-frequency order (out: 16 ints). */
size_t mtd_spectral_gen_ws_bytes(int B, int H, int W);
int mtd_spectral_gen_plan(int n, int* out);
int mtd_rfft_rows_gen(const float* x, int x_ld, float* R, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);
int mtd_spec_mix_gen(const float* R, const float* w2t, const float* b2, float* T, int B, int H, int W, void* ws, size_t ws_bytes,
                     void* stream);
int mtd_irfft_rows_gen(const float* T, float* out, int out_ld, const float* add1, int add1_ld, const float* add2, int add2_ld,
                       int B, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* 64x64 transpose of the 1x1 spectral conv weight (W2[o][k] -> W2T[k][o]). */
int mtd_transpose64(const float* src, float* dst, void* stream);
/* n transposes in one launch; ptrs_dev (device): [src_0, dst_0, src_1, dst_1, ...] (the 21 blocks' mix weights, once per step) */
int mtd_transpose64_multi(const float* const* ptrs_dev, int n, void* stream);

/* ---- element-wise helpers -------------------------------------------------------------------- */
/* out[p,c] = g[p,c] * (y[p,c] > 0 ? 1 : slope)  over npix x C, each tensor with its own ld. */
int mtd_act_grad(const float* g, int g_ld, const float* y, int y_ld, float* out, int out_ld,
                 long long npix, int C, float slope, void* stream);
/* out[i] = a[i] * b[i]  (Dropout mask at networks.py:417 and its gradient), n contiguous floats */
int mtd_mul(const float* a, const float* b, float* out, long long n, void* stream);
int mtd_add(const float* a, const float* b, float* out, long long n, void* stream);      /* out = a + b (sum of two tasks' cotangents before a shared weight gradient) */
/* Round 4: the iteration's remaining bookkeeping as library launches, so that the whole step is a list of C-ABI calls
 * (kernels.LaunchList records and replays it).  They replace torch ops of the host mirror, not reference call sites of their
 * own: nn.Dropout's multiplier (networks.py:313 c_drop; the uniform draws stay torch's generator), the upstream scalar of
 * g_loss.backward() (engine.py:52), the sums behind d_loss's stack (networks.py:1992) and the 17 logged values (engine.py:64-73),
 * and the zero fill of the gradient buffers' non-overwritten entries. */
int mtd_dropout_mask(const float* r, float p, float keep_scale, float* out, long long n, void* stream);   /* out = r >= p ? keep_scale : 0 */
int mtd_scale_by(const float* a, const float* s, float* out, long long n, void* stream);                  /* out = a * s[0], s in device memory */
typedef struct { const float* a; const float* b; int na, nb; } mtd_sum_desc;                              /* sum(a[0..na)) + sum(b[0..nb)) */
int mtd_scalar_sums(const mtd_sum_desc* table_dev, int count, float* out, void* stream);
typedef struct { float* p; long long n; } mtd_zero_desc;
int mtd_zero_multi(const mtd_zero_desc* table_dev, const mtd_zero_desc* table_host, int count, void* stream);
/* sums[t] = sum of the 32-bit patterns of tensor t modulo 2^64 (an order-independent integer checksum).  Data-parallel
 * replicas must hold bit-identical parameters after every update (train.py:93-98 relies on nn.DataParallel for that; here the
 * ranks compare these sums after the first replayed iterations: parallel.DataParallelSync.replicas_agree). */
int mtd_checksum_multi(const mtd_zero_desc* table_dev, const mtd_zero_desc* table_host, int count, unsigned long long* sums, void* stream);
/* dst[0..bytes) = src_pinned[0..bytes): src is page-locked host memory mapped into the device address space
 * (hipHostMalloc / torch pin_memory), read by a kernel on `stream`; bytes % 16 == 0, both 16-byte aligned.
 * Used for the descriptor tables (mtd_*_layer / mtd_loss_term / mtd_adamw_tensor arrays). */
int mtd_upload(const void* src_pinned, void* dst, size_t bytes, void* stream);
/* out[p, 0..C) = a[p, 0..C)  (strided copy: concat / slice), optional accumulate */
int mtd_copy_channels(const float* a, int a_ld, float* out, int out_ld, long long npix, int C,
                      int accumulate, void* stream);
/* bilinear x2, align_corners=False (nn.Upsample at networks.py:230-260) and its adjoint */
int mtd_upsample2x_fwd(const float* in, int in_ld, float* out, int out_ld, int B, int H, int W, int C, void* stream);
int mtd_upsample2x_bwd(const float* gout, int gout_ld, float* gin, int gin_ld, int B, int H, int W, int C, void* stream);
/* same with four channels per thread and the LeakyReLU-gradient mask of the consumer fused in: gin = U^T(gout) * (y > 0 ? 1 : slope)
 * (y == NULL: no mask).  Needs C and the strides to be multiples of 4 and 16-byte aligned bases (MTD_EALIGN otherwise). */
int mtd_upsample2x_bwd_masked(const float* gout, int gout_ld, float* gin, int gin_ld, const float* y, int y_ld, float slope,
                              int B, int H, int W, int C, void* stream);
/* PixelShuffle(2) (networks.py:166-175): in [B,H,W,4C] -> out [B,2H,2W,C] and adjoint */
int mtd_pixel_shuffle2_fwd(const float* in, int in_ld, float* out, int out_ld, int B, int H, int W, int C, void* stream);
int mtd_pixel_shuffle2_bwd(const float* gout, int gout_ld, float* gin, int gin_ld, int B, int H, int W, int C, void* stream);

/* ---- spectral norm (torch.nn.utils.spectral_norm at networks.py:181-300), batched over layers -- */
typedef struct {
    const float* w;     /* weight_orig viewed as [rows][cols]                                   */
    float* u;           /* [rows]  updated in place when train                                   */
    float* v;           /* [cols]  updated in place when train                                   */
    float* sigma;       /* out: sigma, inv_sigma = sigma[1]                                      */
    float* u_save;      /* out (optional): copies of the u, v used by this forward (for backward) */
    float* v_save;
    int rows, cols;
} mtd_sn_layer;
size_t mtd_sn_ws_bytes(const mtd_sn_layer* layers_host, int n_layers);
int mtd_sn_power_iter(const mtd_sn_layer* layers_dev, const mtd_sn_layer* layers_host, int n_layers,
                      int train, float* ws, void* stream);
/* nit train-mode power iterations on the same weights back to back (the discriminator step's four passes, networks.py:1957-1992 calls
 * D four times before any weight changes): the tables hold nit * n_layers entries, iteration-major; entry [i * n_layers + l] says where
 * iteration i leaves layer l's sigma / u_save / v_save (w, u, v, rows, cols as in entry l).  nit + 1 passes over the weights instead
 * of 2 nit: W v of one iteration and W^T (W v) of the next share a pass.  Same workspace as mtd_sn_power_iter; results differ from nit
 * calls of it by rounding (~1e-7). */
int mtd_sn_power_iter_multi(const mtd_sn_layer* layers_dev, const mtd_sn_layer* layers_host, int n_layers, int nit,
                            float* ws, void* stream);
/* g_orig (+)= G/sigma - <G,W>/sigma^2 * u v^T       */
typedef struct {
    const float* G; const float* w; const float* u; const float* v; const float* sigma;
    float* g_out; int rows, cols; int accumulate;
    /* optional second pass over the same weight (a batch-paired discriminator pass has one sigma, u, v per half):
     * g_out (+)= corr(G, u, v, sigma) and then += corr(G2, u2, v2, sigma2), in that order; G2 == NULL: single pass */
    const float* G2; const float* u2; const float* v2; const float* sigma2;
    /* prescaled != 0 (round 6): G already holds G_1 / sigma_1 + G_2 / sigma_2 (mtd_wgrad_args.half_scale) and G2 is NULL:
     * g_out (+)= G - <G_1,W>/sigma_1^2 u v^T - <G_2,W>/sigma_2^2 u2 v2^T; the two dot products must come from the activation-side
     * form below (the raw gradients no longer exist apart); u2 / v2 / sigma2 non-NULL says that there are two passes. */
    int prescaled;
    /* optional (round 6): <G, W> WITHOUT reading G or W.  With y = conv(x, W)/sigma + b and gy the cotangent of y,
     *   <G, W> = sum_pix gy . (W * x) = sigma * sum_{pix,n} gy[pix,n] (y[pix,n] - b[n]),
     * and y comes back from the saved activation a = LeakyReLU(y): y = a > 0 ? a : a * act_inv_slope.  act_gy != NULL selects this
     * form for the layer: a reduction over two [M][N] activation-sized tensors -- on the 4x4 ... 1x1 maps a few hundred KB where the
     * weight-side dot reads G, G2 and W (3 x 9.4 MB for a 512 -> 512 3x3 layer).  The caller picks it where M < cols.
     * act_gy2: a second cotangent added on load (NULL: none).  Pixels [0, act_M_first) belong to the first pass (sigma), the rest to
     * the second (sigma2); act_M_first == act_M for a single pass.  Needs rows % 4 == 0, 16-byte aligned bases and strides. */
    const float* act_gy; const float* act_gy2; const float* act_a; const float* act_bias;
    int act_gy_ld, act_gy2_ld, act_a_ld, act_M, act_M_first; float act_inv_slope;
} mtd_sn_grad_layer;
size_t mtd_sn_grad_ws_bytes(const mtd_sn_grad_layer* layers_host, int n_layers);
int mtd_sn_grad(const mtd_sn_grad_layer* layers_dev, const mtd_sn_grad_layer* layers_host, int n_layers,
                float* ws, void* stream);

/* ---- PCGrad (module/weight_methods.py:449-464) ---------------------------------------------- */
/* gram[a*T+b] = <g_a, g_b> over n elements, T <= 4 task vectors g0..g3 (flat, contiguous; unused = NULL) */
size_t mtd_pcgrad_ws_bytes(long long n, int T);
int mtd_pcgrad_gram(const float* g0, const float* g1, const float* g2, const float* g3, int T, long long n,
                    double* gram, void* ws, void* stream);
/* coefficients from the Gram matrix on the device (orders: T*T ints, shuffle order per i), then
 * merged = sum_k w_k g_k.  No host synchronisation.  coeff_out: T floats (device). */
int mtd_pcgrad_combine(const float* g0, const float* g1, const float* g2, const float* g3, int T, long long n,
                       const double* gram, const int* orders, float* merged, float* coeff_out, void* stream);

/* The two halves of mtd_pcgrad_combine on their own, for module/pcgrad.py::PCGrad (the optimizer wrapper,
 * pcgrad.py:50-69): the projections run on the flat gradient of ALL optimizer parameters, then parameters every
 * objective reaches get the mean of the projected gradients and the others their sum -- one coefficient replay, one
 * axpy (merged = scale * sum_k coeff[k] g_k over n elements) per run of parameters with the same reduction. */
int mtd_pcgrad_coeff(const double* gram, const int* orders, int T, float* coeff_out, void* stream);
int mtd_pcgrad_axpy(const float* g0, const float* g1, const float* g2, const float* g3, int T, long long n,
                    const float* coeff, float scale, float* merged, void* stream);

/* ---- the other task weightings of the D step (module/weight_methods.py:275-316, 375-406, 471-588, 591-602, 678-724) ----
 * mtd_task_weights: one single-wavefront launch turns the T <= 4 device-resident task losses into
 *   c_out[k]      = d loss / d L_k, the factor the loss cotangents of task k are scaled by (mtd_loss_term.wptr),
 *   aux_out[0]    = the weighted loss the method returns, aux_out[1 .. 1+T) = the weight vector it reports,
 *   aux_out[5 .. 5+T) = d loss / d logsigma_k (MTD_TW_UW only).              aux_out: 9 floats.
 * params: T floats the device can read -- the task weights (LS, SCALEINV), the one-hot vector (STL), the host's normal draw
 * (RLW: a pinned slot, so that a recorded launch does not bake one draw in); unused by UW / DWA.
 * state: UW: the T log sigmas (read only).  DWA: mtd_task_weights_state_floats() floats that the kernel owns between calls --
 * [0] the iteration counter (int bits, starts at 0), [1 .. 5) the weights (start at 1), then the ring of 2 * window rows of T
 * costs (start at 1); window / temp: DWA's iteration_window and temperature. */
enum { MTD_TW_LS = 0, MTD_TW_SCALEINV = 1, MTD_TW_STL = 2, MTD_TW_UW = 3, MTD_TW_RLW = 4, MTD_TW_DWA = 5 };
size_t mtd_task_weights_state_floats(int method, int T, int window);
int mtd_task_weights(int method, const float* losses, int T, float* state, const float* params, int window, float temp,
                     float* c_out, float* aux_out, void* stream);
/* CAGrad (:510-543, :563): from the T x T Gram matrix (T <= 4) of the task gradients the T coefficients of
 * n_tasks * (mean_k g_k + lambda sum_k ww_k g_k) / (1 + c^2), ww = argmin over the simplex of x^T A b + c0 sqrt(x^T A x + 1e-8),
 * b = 1/T, c0 = c sqrt(mean(A) + 1e-8) + 1e-8, lambda = c0 / (|sum_k ww_k g_k| + 1e-8).  Exact (stationary point per face of the
 * simplex, in fp64), fixed work, no host read.  coeff_out: 9 floats -- [0 .. T) the coefficients, [4] phi at ww, [5 .. 5+T) ww. */
int mtd_cagrad_coeff(const double* gram, int T, float c, float* coeff_out, void* stream);

/* ---- fused multi-tensor AdamW (train.py:122-126; torch.optim.AdamW semantics) ---------------- */
typedef struct { float* p; const float* g; float* m; float* v; long long n; } mtd_adamw_tensor;
int mtd_adamw_multi(const mtd_adamw_tensor* tensors_dev, const mtd_adamw_tensor* tensors_host, int count,
                    float lr, float beta1, float beta2, float eps, float wd, int step, void* stream);
/* same, with (1 - lr*wd, lr/bias_correction1, 1/sqrt(bias_correction2)) read from dyn[0..2] (device memory):
 * lets a captured hipGraph be replayed with a new step count */
int mtd_adamw_multi_pre(const mtd_adamw_tensor* tensors_dev, const mtd_adamw_tensor* tensors_host, int count, float beta1,
                        float beta2, float eps, float decay, float step_size, float inv_sqrt_bc2, void* stream);
int mtd_adamw_multi_dyn(const mtd_adamw_tensor* tensors_dev, const mtd_adamw_tensor* tensors_host, int count,
                        float beta1, float beta2, float eps, const float* dyn, void* stream);
/* The same update, and in the same launch the derived views of the 3x3 weights it has just written: what mtd_winograd_weights
 * (wino[], px 4 / 6, not the split form) and mtd_pack_weights (pack[], T = 9) would write after it, bit for bit, without reading
 * the weights back from memory.  spans[i] belongs to tensors[i]: N = 0 -- no views, the plain update; otherwise tensors[i] is a
 * contiguous [N][C][9] weight with N % 16 == 0 and C % 16 == 0 and wino[wino_first .. wino_first + wino_count) /
 * pack[pack_first .. pack_first + pack_count) are views of it -- src = p, st = 1 and (sn, sc) = (9 C, 9), view shape (N, C): the
 * forward view, or (9, 9 C), view shape (C, N): the data-gradient view.  dyn != NULL: (decay, step_size, inv_sqrt_bc2) are
 * read from dyn[0..2] as in mtd_adamw_multi_dyn; NULL: the three arguments as in mtd_adamw_multi_pre. */
typedef struct { int N, C, wino_first, wino_count, pack_first, pack_count; } mtd_adamw_views_span;
int mtd_adamw_views(const mtd_adamw_tensor* tensors_dev, const mtd_adamw_tensor* tensors_host, int count,
                    const mtd_adamw_views_span* spans_dev, const mtd_adamw_views_span* spans_host,
                    const mtd_wino_weight_desc* wino_dev, const mtd_wino_weight_desc* wino_host, int n_wino,
                    const mtd_pack_desc* pack_dev, const mtd_pack_desc* pack_host, int n_pack,
                    float beta1, float beta2, float eps, float decay, float step_size, float inv_sqrt_bc2,
                    const float* dyn, void* stream);

/* ---- loss terms (losses.py:10-15,99-138; networks.py:1962-1977,1998-2002), batched by descriptor table --
 * kind 0: m*(a-t)^2 with t = b[i] or tconst, m = (mx[i]-my[i] != 0) or 1   (ls_gan / NDS_Loss / F.mse_loss)
 * kind 1: |a-b| (F.l1_loss)      kind 2: sqrt((a-b)^2 + eps^2) (CharbonnierLoss)
 * value[k] = scale * sum_i term;   grads: grad_out[i] (+)= coef * d term_i / d a_i                        */
typedef struct {
    int kind;
    const float* a; const float* b; float tconst;
    const float* mx; const float* my;
    long long n; float scale; float eps;
    float* grad_out; float coef; int accumulate;
    const float* wptr;      /* optional device-resident factor: the written cotangent is (coef * *wptr) * d term (NULL: coef * d term) */
} mtd_loss_term;
size_t mtd_loss_terms_ws_bytes(int nterms);
int mtd_loss_terms(const void* terms_dev, int nterms, float* out, void* ws, void* stream);
int mtd_loss_term_grads(const void* terms_dev, int nterms, void* stream);
/* x.clip(0,1) (networks.py:1969-1970) and its gradient mask (inclusive bounds, as torch.clamp) */
int mtd_clip01(const float* x, float* out, long long n, void* stream);
int mtd_clip01_bwd(const float* g, const float* x, float* out, long long n, void* stream);
/* EdgeLoss (losses.py:113-138) on B images of 64x64: out[0] = scale * sum sqrt(lap(a-b)^2 + eps^2);
 * grad_out (optional) (+)= coef * d(sum)/da */
size_t mtd_edge_loss_ws_bytes(int B);
int mtd_edge_loss(const float* a, const float* b, int B, float scale, float eps, float* out, float* grad_out,
                  float coef, int accumulate, void* ws, void* stream);

/* ---- pixel metrics of the evaluation loops (metrics.py:172-244; engine.py:78-183) -------------------------------
 * For a batch of B single-channel H x W images a, b (contiguous): out2[0] = sum (a' - b)^2, out2[1] = sum of the SSIM map
 * of (a', b) (11x11 Gaussian window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2), a' = clip(a, 0, 1) if clip_a.
 * RMSE = sqrt(out2[0] / n), PSNR = 10 log10(1 / (out2[0] / n + 1e-10)), SSIM = out2[1] / n with n = B*H*W. */
size_t mtd_image_metrics_ws_bytes(int B, int H, int W);
int mtd_image_metrics(const float* a, const float* b, int B, int H, int W, int clip_a, double* out2, void* ws, void* stream);
/* The same sums image by image, for na in 1..3 sources a[k] (B, H, W) against one b: out (na, B, 2) doubles, out[k][i] = the two
 * sums of image i of (a[k]', b), a[k]' = clip(a[k], 0, 1) if clip_a[k].  One tile launch over na * B images and one finishing launch
 * (a workgroup per source and image, which sums that image's tile partials).  mtd_image_metrics runs the same two kernels with
 * one source and the batch as one group of the finish, so out[k][i] has the bits of
 * mtd_image_metrics(a[k] + i*H*W, b + i*H*W, 1, H, W, clip_a[k], ...).  a and clip_a are read on the host during the call
 * (their first na entries).  na * B > 65535, null pointers, non-positive sizes: MTD_EINVAL (the _ws_bytes query then returns 0
 * for na or a size out of range). */
size_t mtd_image_metrics_each_ws_bytes(int na, int B, int H, int W);
int mtd_image_metrics_each(const float* const a[3], int na, const float* b, int B, int H, int W, const int clip_a[3], double* out,
                           void* ws, void* stream);

/* ---- further full-reference metrics of the test loop (module/piq: ssim.py multi_scale_ssim, vif.py vif_p, gmsd.py gmsd) --
 * DESIGN 3.14.  Single-channel fp32 images (B, H, W) in [0, 1] (data_range 1), na in 1..3 sources a[k] against one target b, image
 * by image.  which_mask: MTD_IQA_MS_SSIM | MTD_IQA_VIF | MTD_IQA_GMSD.
 *   MS-SSIM  11 x 11 Gaussian (sigma 1.5) on valid windows, five levels weighted (0.0448, 0.2856, 0.3001, 0.2363, 0.1333),
 *            C1 = 0.01^2, C2 = 0.03^2; between levels replicate-pad left and top by max(h % 2, w % 2), then a 2 x 2 average
 *            pool; score = prod relu(v_l)^w_l, v_l the mean of the cs map (last level: of the SSIM map).  H, W >= 161.
 *   VIFp     scales 1..4 with Gaussians of 17, 9, 5, 3 taps (sigma = taps / 5) on valid windows, each scale after the first
 *            filtered with its own window and subsampled by two; score = (sum num + 1e-8) / (sum den + 1e-8) with
 *            num = sum log10(1 + g^2 s_t / (s_v + sigma_n_sq)), den = sum log10(1 + s_t / sigma_n_sq).  sigma_n_sq > 0 is
 *            taken on the [0, 1] scale as given (the vendored vif_p does not rescale to [0, 255]).  H, W >= 41.
 *   GMSD     zero-pad bottom and right by max(H % 2, W % 2), 2 x 2 average pool, Prewitt / 3 with zero padding, GMS with
 *            t = 170 / 255^2; score = population standard deviation of the GMS map.  H, W >= 2.
 * out: (n selected metrics in the order above, na, B) doubles, the finished scores.  parts (optional, may be null):
 * (na, B, MTD_IQA_PARTS) doubles, [0..9] MS-SSIM (cs mean, SSIM mean) of levels 0..4, [10..17] VIFp (num, den) of scales 1..4,
 * [18..19] GMSD (mean, variance) of the GMS map; only the selected metrics' entries are written.  fp32 filter arithmetic, per-image
 * sums in double in a fixed order: an image's numbers depend neither on the batch nor on its source slot.  a is read on the
 * host during the call (its first na entries).  Null pointers, which_mask outside 1..7, na outside 1..3, a side below a
 * selected metric's minimum, (na + 1) * B > 65535, H * W > 2^30, sigma_n_sq <= 0: MTD_EINVAL before any launch (the _ws_bytes
 * query then returns 0). */
#define MTD_IQA_MS_SSIM 1
#define MTD_IQA_VIF 2
#define MTD_IQA_GMSD 4
#define MTD_IQA_PARTS 20
size_t mtd_iqa_ws_bytes(int which_mask, int na, int B, int H, int W);
int mtd_iqa_each(const float* const a[3], int na, const float* b, int B, int H, int W, int which_mask, float sigma_n_sq, double* out,
                 double* parts, void* ws, void* stream);

/* ---- Haar wavelet perceptual similarity index of the test loop (module/piq: haarpsi.py haarpsi, scales = 3) -- DESIGN 3.16.
 * Single-channel fp32 images (B, H, W) in [0, 1] (data_range 1), na in 1..3 sources a[k] against one target b, image by image.
 *   rescale by 255; with subsample != 0 zero-pad bottom and right by max(H % 2, W % 2) (the same pad in both dimensions) and
 *   take a 2 x 2 average pool with stride 2 (floor); for k = 2, 4, 8 zero-pad k/2 - 1 on top and left and k/2 on bottom and right
 *   and cross-correlate with the k x k Haar filter (top k/2 rows +1/k, bottom k/2 rows -1/k) and with its transpose; per
 *   orientation w = max(|cx|, |cy|) at k = 8 and sim = the mean over k = 2, 4 of (2 |cx| |cy| + c) / (cx^2 + cy^2 + c);
 *   num = sum sigmoid(alpha sim) w and den = sum w over both orientations and all pixels; s = (num + eps) / (den + eps) with
 *   float32's eps; score = (log(s / (1 - s)) / alpha)^2 (two all-zero images: +inf, as piq gives).
 * out: (na, B) doubles, the finished scores.  parts (optional, may be null): (na, B, MTD_HAARPSI_PARTS) doubles, (num, den) of
 * the filter as it is and then of its transpose.  fp32 filter arithmetic; similarity, sigmoid and per-image sums in double in a
 * fixed order: an image's numbers depend neither on the batch nor on its source slot.  c and alpha arrive as floats (piq's
 * float32 call rounds them likewise).  a is read on the host during the call (its first na entries).  ws: mtd_haarpsi_ws_bytes.
 * Null pointers, na outside 1..3, B < 1, na * B > 65535, a side below MTD_HAARPSI_MIN_SIDE (piq's 2^(scales + 1), with subsample
 * or without), H * W > 2^30, more than 65535 tile rows, c <= 0, alpha <= 0: MTD_EINVAL before any launch (the _ws_bytes query
 * then returns 0). */
#define MTD_HAARPSI_PARTS 4
#define MTD_HAARPSI_MIN_SIDE 16
size_t mtd_haarpsi_ws_bytes(int na, int B, int H, int W, int subsample);
int mtd_haarpsi_each(const float* const a[3], int na, const float* b, int B, int H, int W, int subsample, float c, float alpha,
                     double* out, double* parts, void* ws, void* stream);

/* ---- feature similarity index of the test loop (module/piq: fsim.py fsim, chromatic = False) -- DESIGN 3.17.
 * Single-channel fp32 images (B, H, W) in [0, 1] (data_range 1), na in 1..3 sources srcs[k] against one target, image by image.
 *   rescale by 255 and average-pool ks x ks (stride ks, floor) to the h x w = H / ks x W / ks map; the phase-congruency map from
 *   the scales * orientations log-Gabor filters of `filters` (device, (orientations * scales, h, w) fp32, orientation-major, zero
 *   frequency at [0, 0]) applied in the frequency domain: even / odd = real / imaginary part of ifft2(fft2(image) * filter), per
 *   orientation the energy sum_s (even mean_e + odd mean_o - |even mean_o - odd mean_e|) less the noise threshold T_o, which
 *   comes from the median (the element of rank (h w - 1) / 2) of the scale-0 squared amplitude and `consts` (device, 3 *
 *   orientations doubles: em_n[o], sum_an2[o], sum_ai_aj[o]) and k; pc = (sum_o max(energy_o - T_o, 0) + eps) / (sum an + eps);
 *   the Scharr gradient magnitude of the pooled map (zero padding 1); score = sum GM PC max(pc_a, pc_b) / sum max(pc_a, pc_b)
 *   with the similarity constants 0.85 and 160.  eps is float32's; two all-zero images score exactly 1.
 * out: (na, B) doubles.  parts (optional, may be null): (na, B, MTD_FSIM_SUMS + orientations) doubles: num, den, the sums of the
 * source's phase-congruency and gradient maps, then the source's T_0 .. T_{O-1}.  fp32 transforms (radix-2 passes in LDS);
 * everything from the filter responses on and every per-image sum in double in a fixed order: an image's numbers depend neither on
 * the batch nor on its source slot.  A source whose pointer equals the target's shares the target's maps.  srcs is read on the
 * host during the call (its first na entries).  ws: mtd_fsim_ws_bytes (of the POOLED sides); the batch is walked in chunks sized so
 * that the workspace stays within 64 MiB, and the orientations in groups where one image of every set would not fit otherwise:
 * at 256 x 256 pooled maps it is within 64 MiB for every allowed option and batch (DESIGN 3.17 has the rule).
 * Null pointers, na outside 1..3, B < 1, ks < 1, a pooled side that is not a power of two in MTD_FSIM_MIN_SIDE .. MTD_FSIM_MAX_SIDE,
 * scales outside 1..4, orientations outside 1..8, H * W > 2^30, a NaN k: MTD_EINVAL before any launch (the _ws_bytes query then
 * returns 0).
 * mtd_fsim_median: out[c] = the element of rank (n - 1) / 2 (torch.median's) of the n non-negative floats at values + c * n, by
 * the radix select mtd_fsim_each's thresholds use. */
#define MTD_FSIM_SUMS 4
#define MTD_FSIM_MIN_SIDE 16
#define MTD_FSIM_MAX_SIDE 512
size_t mtd_fsim_ws_bytes(int na, int B, int h, int w, int scales, int orientations);
int mtd_fsim_each(const void* const* srcs, int na, const void* target, int B, int H, int W, int ks, int scales, int orientations, float k,
                  const float* filters, const double* consts, double* out, double* parts, void* ws, void* stream);
int mtd_fsim_median(const float* values, int n, int count, float* out, void* stream);

/* ---- visual saliency-induced index and mean deviation similarity index of the test loop (module/piq: vsi.py vsi, mdsi.py mdsi)
 * -- DESIGN 3.19.  Single-channel fp32 images (B, H, W) in [0, 1] (data_range 1; piq copies the grey channel three times), na in
 * 1..3 sources srcs[k] against one target, image by image.  k is piq's pooling kernel max(1, round(min(H, W) / 256)) with
 * Python's round (half to even), computed by the caller; the pooled map has (H + k - 1) / k x (W + k - 1) / k pixels (VSI pads
 * [k / 2, (k - 1) / 2] in replicate mode, MDSI [(k - 1) / 2, k / 2] with zeros).  `options` is read on the host during the call,
 * as srcs is (its first na entries).  A source whose pointer equals the target's shares the target's maps (VSI).  Everything
 * but the 256 x 256 transforms of VSI's saliency map (fp32, radix-2 passes in LDS) is double, every per-image sum in a fixed
 * order: an image's numbers depend neither on the batch nor on its source slot.  The batch is walked in chunks sized so that
 * the workspace (the _ws_bytes query) stays within 64 MiB (VSI) / 16 MiB (MDSI).
 * mtd_vsi_each: log_gabor: device, (256, 256) fp32, zero frequency at [0, 0] (piq's _log_gabor); options: c1, c2, c3, alpha, beta,
 *   sigma_d, sigma_c.  out: (na, B) doubles.  parts (optional, may be null): (na, B, MTD_VSI_PARTS) doubles: num, den, the sums of
 *   the source's pooled saliency and gradient maps, the minimum and maximum of its saliency map before it is stretched to [0, 1].
 * mtd_mdsi_each: options: c1, c2, c3, alpha, beta, gamma, rho, q, o; mult: 0 combination 'sum', 1 'mult'.  out: (na, B) doubles.
 *   parts (optional): (na, B, MTD_MDSI_PARTS) doubles: the means of the real and imaginary part of gcs^q and the sum of
 *   |gcs^q - mean|^rho.
 * Null pointers, na outside 1..3, B < 1, k outside 1..8, a side outside MTD_*_MIN_SIDE .. MTD_*_MAX_SIDE, an option that is not
 * finite, a c1, c2, c3 (or MDSI's rho) that is not positive, a zero sigma, another mult: MTD_EINVAL before any launch (the
 * _ws_bytes query then returns 0). */
#define MTD_VSI_MIN_SIDE 16
#define MTD_VSI_MAX_SIDE 1024
#define MTD_VSI_PARTS 6
#define MTD_VSI_OPTIONS 7
#define MTD_MDSI_MIN_SIDE 16
#define MTD_MDSI_MAX_SIDE 1024
#define MTD_MDSI_PARTS 3
#define MTD_MDSI_OPTIONS 9
size_t mtd_vsi_ws_bytes(int na, int B, int H, int W, int k);
int mtd_vsi_each(const void* const* srcs, int na, const void* target, int B, int H, int W, int k, const float* log_gabor,
                 const double* options, double* out, double* parts, void* ws, void* stream);
size_t mtd_mdsi_ws_bytes(int na, int B, int H, int W, int k);
int mtd_mdsi_each(const void* const* srcs, int na, const void* target, int B, int H, int W, int k, const double* options, int mult,
                  double* out, double* parts, void* ws, void* stream);

/* ---- the no-reference statistics of the test loop (module/piq: brisque.py brisque, tv.py total_variation) -- DESIGN 3.21.
 * Single-channel fp32 images (B, H, W) in [0, 1] (data_range 1), na in 1..3 sources srcs[k], each on its own (there is no target),
 * image by image.  srcs is read on the host during the call (its first na entries); a pointer that occurs twice is computed once
 * and written to both slots.  Everything is double, every per-image sum in a fixed order: an image's numbers depend neither on the
 * batch nor on its source slot.
 * mtd_brisque_each: ks: the odd side 3..MTD_BRISQUE_MAX_KERNEL of the Gaussian filter, taps: device, its ks * ks fp32 taps (piq's
 *   gaussian_filter, normalised); tables: device, 3 * nt doubles: piq's gamma grid, the GGD r_table, the AGGD r_table; weights:
 *   device, (n_sv, 37) doubles: the SVR coefficient, then the support vector.  Two scales: 255 * image, and its `nearest` resample
 *   to (H / 2, W / 2) (source index min(floor(dst * scale), size - 1), scale = size / (size / 2) in fp32).  out: (na, B) doubles.
 *   parts (optional, may be null): (na, B, MTD_BRISQUE_PARTS) doubles: the 36 features before the range scaling (per scale alpha,
 *   sigma^2, then per shift alpha, eta, sigma_l^2, sigma_r^2), then the score.  Where piq asserts (an MSCN map whose sigma is within
 *   1e-8 of zero, a product map without a negative or without a positive value, a zero left or right sigma) the image's score
 *   and parts are NaN; the other images are untouched.  The batch is walked in chunks sized so that the workspace (the _ws_bytes
 *   query) stays within 64 MiB.
 * mtd_tv_each: norm: MTD_TV_L1 (sum |dy| + sum |dx|), MTD_TV_L2 (the square root of sum dy^2 + sum dx^2), MTD_TV_L2_SQUARED, of
 *   the differences of neighbouring pixels of the image itself (not scaled).  out: (na, B) doubles.
 * Null pointers, na outside 1..3, B < 1, a side outside MTD_*_MIN_SIDE .. MTD_*_MAX_SIDE, an even ks or one outside its range,
 * nt < 1, n_sv < 1, another norm: MTD_EINVAL before any launch (the _ws_bytes query then returns 0). */
#define MTD_BRISQUE_MIN_SIDE 16
#define MTD_BRISQUE_MAX_SIDE 1024
#define MTD_BRISQUE_MAX_KERNEL 15
#define MTD_BRISQUE_PARTS 37
#define MTD_TV_MIN_SIDE 16
#define MTD_TV_MAX_SIDE 1024
#define MTD_TV_L1 0
#define MTD_TV_L2 1
#define MTD_TV_L2_SQUARED 2
size_t mtd_brisque_ws_bytes(int na, int B, int H, int W);
int mtd_brisque_each(const void* const* srcs, int na, int B, int H, int W, int ks, const float* taps, const double* tables, int nt,
                     const double* weights, int n_sv, double* out, double* parts, void* ws, void* stream);
size_t mtd_tv_ws_bytes(int na, int B, int H, int W);
int mtd_tv_each(const void* const* srcs, int na, int B, int H, int W, int norm, double* out, void* ws, void* stream);

/* ---- perceptual metrics of the test loop (metrics.py:43-168: PL and TML on VGG-19 features; engine.py:139-140) ------
 * The convolutions of the feature stack are mtd_conv_* launches; these are the other pieces.  Maps are contiguous NHWC fp32,
 * 16-byte aligned (MTD_EALIGN).
 *   mtd_maxpool2x2        nn.MaxPool2d(2, 2): out (B, H/2, W/2, C) from in (B, H, W, C), floor semantics (an odd last row or
 *                         column is dropped), NaN propagates as in torch.  Any B >= 1, H, W >= 2, C a multiple of 4 (else
 *                         MTD_EINVAL).  One float4 of channels per thread and round; at most MTD_MAXPOOL_MAX_BLOCKS workgroups
 *                         of 256 threads, so maps of more than 256 * MTD_MAXPOOL_MAX_BLOCKS output float4 take further rounds.
 *   mtd_patch_gram_l1     X, Y (B, h, w, C), C in {64, 128, 256, 512}.  Over the non-overlapping 16 x 16 patches ((h/16) * (w/16) per
 *                         image; remainder rows / columns are never read) with G(F) = sum over the patch's 256 pixels of f f^T
 *                         (C x C, not normalised): out[0] = sum over patches and all C^2 entries of |G(X) - G(Y)|, in double.
 *                         The mean of nn.L1Loss is out[0] / (B * patches * C^2).  fp32 MFMA products; the reduction has a fixed
 *                         order (per-workgroup partials in ws, mtd_patch_gram_l1_ws_bytes(B, h, w, C) bytes, then one finishing
 *                         pass), and X, Y run through the same instructions: X == Y gives exactly 0.  No patch (h or w < 16), any
 *                         other C, null pointers: MTD_EINVAL (the _ws_bytes query then returns 0).
 *   mtd_patch_gram_l1_each  the same sum image by image: out[i * out_stride] = the sum over the patches of image i, i < B
 *                         (out_stride >= 1 doubles, so that a level writes straight into a (who, image, level) table).  The same
 *                         kernel and workspace (mtd_patch_gram_l1_ws_bytes); the finishing pass runs a workgroup per image, which
 *                         walks that image's partials in the order of a one-image call: out[i * out_stride] has the bits of
 *                         mtd_patch_gram_l1 on image i alone, and X == Y gives exactly 0 for every image.  Shape rules and errors
 *                         as mtd_patch_gram_l1; out_stride < 1: MTD_EINVAL.
 *   mtd_scaled_sums_f64   out[g] = (float) sum_{i < per} scales_host[i] * in[g * per + i] for g < groups: the weighted sum over
 *                         the five feature levels of several loss values at once.  per <= MTD_SCALED_SUMS_MAX; scales_host is
 *                         read on the host during the call. */
#define MTD_MAXPOOL_MAX_BLOCKS 2048
#define MTD_SCALED_SUMS_MAX 8
int mtd_maxpool2x2(const float* in, float* out, int B, int H, int W, int C, void* stream);
size_t mtd_patch_gram_l1_ws_bytes(int B, int h, int w, int C);
int mtd_patch_gram_l1(const float* X, const float* Y, int B, int h, int w, int C, double* out, void* ws, void* stream);
int mtd_patch_gram_l1_each(const float* X, const float* Y, int B, int h, int w, int C, double* out, long long out_stride, void* ws,
                           void* stream);
int mtd_scaled_sums_f64(const double* in, int groups, int per, const double* scales_host, float* out, void* stream);

/* ---- LPIPS and DISTS of the test loop (module/piq/perceptual.py: LPIPS, DISTS on VGG-16 features) -- DESIGN 3.18 ----------
 * The convolutions of the feature stack are mtd_conv_* launches and its max-pools mtd_maxpool2x2; these are the other pieces.
 * Maps are contiguous NHWC fp32, 16-byte aligned where C is a multiple of 4 (MTD_EALIGN).  No atomics; every per-image number is
 * a double formed in a fixed order in two stages (workgroup partials in ws, then a finish), and image i of a batch has the bits
 * of the one-image call on image i.  Null pointers and shapes outside the rules: MTD_EINVAL before any launch (a _ws_bytes
 * query then returns 0).
 *   mtd_l2pool3x3s2       DISTS's L2Pool2d(3, stride 2, padding 1): out (B, ceil(H/2), ceil(W/2), C) from in (B, H, W, C),
 *                         out = sqrt(sum over the 3 x 3 window of k x^2 + 1e-12), k = [[1,2,1],[2,4,2],[1,2,1]] / 16, zeros outside
 *                         the map; the taps are added row-major in fp32 (fmaf(k, x * x, acc)).  Any B, H, W >= 1, C a multiple
 *                         of 4.  One float4 of channels per thread and round; at most MTD_L2POOL_MAX_BLOCKS workgroups of 256
 *                         threads, so maps of more than 256 * MTD_L2POOL_MAX_BLOCKS output float4 take further rounds.
 *   mtd_lpips_level_each  t, a and b (b may be null) of shape (B, h, w, C), C in {64, 128, 256, 512}, h * w < 2^30, B <= 65535;
 *                         weights: C device doubles.  For o = a (k = 0) and o = b (k = 1, when given):
 *                           out[k * other_stride + i * out_stride] = sum over the pixels of image i and c of w_c d(o_c / (|o| + 1e-10), t_c / (|t| + 1e-10)),
 *                         |.| the 2-norm over a pixel's channels, d(x, y) = (x - y)^2 (MTD_LPIPS_MSE) or |x - y| (MTD_LPIPS_MAE);
 *                         the spatial mean is this over h * w.  Floats are converted on load and everything is double: a pixel's
 *                         norms are sums over its C channels (a lane's 4 or 8 in sequence, then a butterfly over the
 *                         LP = min(C / 4, 64) lanes of the pixel), 1 / (|.| + 1e-10) is one division per pixel and map.  o == t
 *                         (the same values) gives exactly 0; an all-zero pixel contributes 0.  Launch arithmetic: a workgroup
 *                         of 256 threads takes P = 4 * 64 / LP pixels per round, an image gets
 *                         nblk = min(ceil(h w / P), MTD_LPIPS_MAX_BLOCKS) workgroups and so R = ceil(h w / (P nblk)) rounds.  A
 *                         lane adds its C / LP terms of R pixels in sequence, then 6 butterfly steps, the 4 waves in 2 steps,
 *                         the finish ceil(nblk / 256) partials per thread and an 8-step tree: no number passes through more than
 *                         (C / LP) R + 6 + 2 + ceil(nblk / 256) + 8 additions (the summation depth).  ws:
 *                         mtd_lpips_level_ws_bytes(B, h, w, C).  out_stride < 1 or another distance flag: MTD_EINVAL.
 *   mtd_scaled_sums_f64_f64  mtd_scaled_sums_f64 with a double result: out[g] = sum_i scales_host[i] * in[g * per + i], added in
 *                         the order of i; parts (optional, may be null) gets the groups * per scaled terms.
 *   mtd_channel_moments_each  t, a and b (b may be null) of shape (B, h, w, C), C = 1 or a multiple of 4 up to 1024,
 *                         h * w < 2^30, B <= 65535.  out: (B, C, K) doubles, K = 2 + 3 n_others, per image and channel
 *                         (sum t, sum t^2) and then per other map (sum o, sum o^2, sum o t) over the pixels.  A product of two
 *                         floats is exact in double, so only the additions round.  Launch arithmetic: a thread owns a float4 of
 *                         channels (the one channel when C = 1), PL = 256 / (C / 4) (256 when C = 1) threads share a channel group
 *                         and walk a pixel range with stride PL; an image is cut into
 *                         ranges = min(ceil(h w / (PL * MTD_MOMENTS_WALK)), MTD_MOMENTS_MAX_RANGES) ranges of
 *                         ceil(h w / ranges) pixels.  A thread adds ceil(range / PL) terms in sequence, the PL threads meet in
 *                         a halving tree (ceil(log2 PL) steps) and the finish adds the ranges in index order: the summation
 *                         depth is ceil(range / PL) + ceil(log2 PL) + ranges.  ws: mtd_channel_moments_ws_bytes.
 *   mtd_dists_finish      tables[l], l < MTD_DISTS_LEVELS = 6: the moment tables of the raw image (C = 1) and the five VGG-16
 *                         maps (C = 64, 128, 256, 512, 512), all of one n_others and B; pixels[l]: h * w of level l; alpha, beta:
 *                         1475 = 3 + 64 + 128 + 256 + 512 + 512 device doubles each, whose first three all weigh the grey channel.
 *                         With mu = sum / n, var = sum of squares / n - mu^2, cov = sum o t / n - mu_o mu_t:
 *                           S1 = (2 mu_o mu_t + 1e-6) / (mu_o^2 + mu_t^2 + 1e-6), S2 = (2 cov + 1e-6) / (var_o + var_t + 1e-6),
 *                           out[r * B + i] = 1 - sum over levels (sum over channels of alpha S1 + beta S2),
 *                         a level's channels by a 256-thread fixed-order sum, the levels in order.  Rows r: the others in
 *                         order; with self_row in 0 .. n_others one more row is inserted at that index for the target against
 *                         itself, whose S1 and S2 are exactly 1 in this arithmetic (no table is read for it): n_others +
 *                         (self_row >= 0) rows.  parts (optional, may be null): (rows, B, 6) doubles, the level sums.  tables
 *                         and pixels are read on the host during the call. */
#define MTD_L2POOL_MAX_BLOCKS 2048
#define MTD_LPIPS_MAX_BLOCKS 1024
#define MTD_LPIPS_MSE 0
#define MTD_LPIPS_MAE 1
#define MTD_MOMENTS_MAX_RANGES 256
#define MTD_MOMENTS_WALK 32
#define MTD_DISTS_LEVELS 6
#define MTD_DISTS_WEIGHTS 1475
int mtd_l2pool3x3s2(const float* in, float* out, int B, int H, int W, int C, void* stream);
size_t mtd_lpips_level_ws_bytes(int B, int h, int w, int C);
int mtd_lpips_level_each(const float* t, const float* a, const float* b, int B, int h, int w, int C, const double* weights, int distance,
                         double* out, long long out_stride, long long other_stride, void* ws, void* stream);
int mtd_scaled_sums_f64_f64(const double* in, int groups, int per, const double* scales_host, double* out, double* parts, void* stream);
size_t mtd_channel_moments_ws_bytes(int B, int h, int w, int C, int n_others);
int mtd_channel_moments_each(const float* t, const float* a, const float* b, int B, int h, int w, int C, double* out, void* ws, void* stream);
int mtd_dists_finish(const double* const tables[MTD_DISTS_LEVELS], const long long pixels[MTD_DISTS_LEVELS], int n_others, int B, int self_row,
                     const double* alpha, const double* beta, double* out, double* parts, void* stream);

/* ---- Frechet distance of the test loop (module/piq/fid.py; metrics.py:33-41, engine.py:179-181) -- DESIGN 3.8 -----------
 * The statistic only: the feature network stays the caller's.  float64 throughout, products on v_mfma_f64_16x16x4_f64.  All
 * matrices are contiguous row-major, D x D doubles, 1 <= D <= 16384, 8-byte aligned; no size is special (edge tiles and the
 * tail of the sum are index-checked in the kernel) and NO buffer is padded: neither the caller's matrices nor the workspace,
 * which holds D x D matrices exactly.  No floating-point atomics: every sum has a fixed order, two calls on the same inputs
 * give the same bits.  Null pointers and sizes out of range: MTD_EINVAL, nothing launched.  The library allocates nothing.
 *   mtd_fid_ws_bytes   bytes of `ws` for mtd_fid_distance / mtd_fid_residual at this D (six D x D matrices, the per-workgroup
 *                      partials, the state); 0 = D out of range.  Used in stream order.
 *   mtd_fid_stats      X (N, D) fp32 contiguous -> mu (D) = column means, sigma (D, D) = (X - mu)^T (X - mu) / (N - 1): two
 *                      passes as fid.py:124-132,144-145, the centring in float64 on the way into the product.  N < 2: MTD_EINVAL
 *                      (the reference divides by zero there).  ws is not used (may be NULL).
 *   mtd_fid_gemm       C = alpha * A . B + beta_eye * I.  C must not overlap A or B.
 *   mtd_fid_residual   out[0] = |A - scale * (Y . Y)|_F^2; the difference is not stored.
 *   mtd_fid_distance   out[0] = |mu1 - mu2|^2 + tr s1 + tr s2 - 2 tr sqrt((s1 + offset I)(s2 + offset I)), out[1] = that trace
 *                      of the square root, out[2] = the last err, out[3] = 1.0 if every element of the square root is finite,
 *                      else 0.0 (fid.py:85); iters[0] = the round the iteration ended at.  Newton-Schulz as fid.py:42-61:
 *                      Y0 = M / |M|_F, Z0 = I; per round T = 0.5 (3 I - Z Y), Y <- Y T, Z <- T Z, err = |M - S S|_F / |M|_F with
 *                      S = sqrt(|M|_F) Y; ends at err <= 1e-5 or after max_iters rounds (the reference: 100).  The stop is taken
 *                      ON THE DEVICE: max_iters rounds are enqueued, each launch reads a state word first and returns at once
 *                      when it is set; the host reads nothing back during the call.  offset: 0, or the reference's 1e-6 of its
 *                      second solve (fid.py:87-88; the traces of s1 and s2 stay those of the matrices as given).
 *                      max_iters <= 0: MTD_EINVAL. */
size_t mtd_fid_ws_bytes(int D);
int mtd_fid_stats(const float* X, int N, int D, double* mu, double* sigma, void* ws, void* stream);
int mtd_fid_gemm(const double* A, const double* B, double* C, int D, double alpha, double beta_eye, void* stream);
int mtd_fid_residual(const double* A, const double* Y, double scale, int D, double* out, void* ws, void* stream);
int mtd_fid_distance(const double* mu1, const double* s1, const double* mu2, const double* s2, int D, double offset,
                     int max_iters, double* out, int* iters, void* ws, void* stream);

/* ---- Kernel Inception Distance (module/piq/kid.py) from the same (N, D) fp32 feature rows -- DESIGN 3.15 ------------------
 * For every subset s of S: the m rows X[xi[s][i]] and Y[yi[s][i]] (xi, yi: (S, m) int tables on the device), the polynomial
 * kernel K(A, B) = (gamma A B^T + coef0)^degree (integer degree 1..8, by repeated multiplication) in float64 on
 * v_mfma_f64_16x16x4_f64, and kid.py's _mmd2_and_variance on K_XX, K_XY, K_YY.  The m x m matrices are never stored: each
 * 64 x 64 tile is reduced to its row sums, column sums, sum of squares and diagonal sums where it is computed.  No size is
 * special, no buffer is padded, no floating-point atomics: two calls give the same bits, and a subset's values depend neither
 * on its place among the S subsets nor on S.  The values of the index tables are the caller's to check (an index outside its
 * matrix reads as a row of zeros).  Nothing is allocated or synchronised; all work is enqueued on `stream`.
 *   mtd_kid_ws_bytes   bytes of `ws` (exactly S * 3 * ceil(m / 64)^2 tile records of MTD_KID_TILE_REC doubles); 0 = m or S out
 *                      of range.
 *   mtd_kid            out[0], out[1] = the means over the subsets, in subset order, of out[2 + 2 s] = mmd2 and out[3 + 2 s] =
 *                      var_est of subset s (0.0 when want_var == 0); out holds 2 + 2 S doubles.  mmd_est: MTD_KID_UNBIASED
 *                      (kid.py's default), MTD_KID_BIASED, MTD_KID_USTAT.  var_at_m: the m of kid.py:137 (the caller passes
 *                      min(Nx, Ny) for kid.py's behaviour).  parts: NULL, or (S, MTD_KID_PARTS) doubles per subset:
 *                        [0] Kt_XX_sum  [1] Kt_YY_sum  [2] K_XY_sum  [3] sum_diag_X  [4] sum_diag_Y  [5] trace(K_XY)
 *                        [6] sum_diag2_X  [7] sum_diag2_Y  [8] Kt_XX_2_sum  [9] Kt_YY_2_sum  [10] K_XY_2_sum
 *                        [11] |Kt_XX_sums|^2  [12] |Kt_YY_sums|^2  [13] |K_XY_sums_1|^2  [14] |K_XY_sums_0|^2
 *                        [15] dot_XX_XY  [16] dot_YY_YX  [17] zeta1_est  [18] zeta2_est  [19] mmd2  [20] var_est
 *                      ([17], [18], [20] are 0.0 when want_var == 0).
 *                      MTD_EINVAL, nothing launched: a null X, Y, xi, yi, out or ws; m < 2; want_var with m < 3 or
 *                      var_at_m < 2; D < 1; degree outside 1..8; S < 1; 3 S > 65535; m > Nx or m > Ny; m > 2^20; an unknown
 *                      mmd_est. */
#define MTD_KID_PARTS 21
#define MTD_KID_TILE_REC 132
enum { MTD_KID_UNBIASED = 0, MTD_KID_BIASED = 1, MTD_KID_USTAT = 2 };
size_t mtd_kid_ws_bytes(int m, int S);
int mtd_kid(const float* X, int Nx, const float* Y, int Ny, int D, const int* xi, const int* yi, int m, int S, int degree,
            double gamma, double coef0, int mmd_est, int want_var, int var_at_m, double* out, double* parts, void* ws,
            void* stream);

/* ---- Multi-Scale Intrinsic Distance (module/piq/msid.py) and Inception Score (module/piq/isc.py) from the same (N, D) fp32
 * feature rows -- DESIGN 3.20 -------------------------------------------------------------------------------------------------
 * float64 arithmetic throughout; the starting vectors, temperatures and temperature tables are float64 on the device and the
 * caller's.  k + 2 <= N <= MTD_MSID_MAX_N (msid.py:33 partitions at k + 1), 1 <= k <= 63, 2 <= m <= 32, 1 <= nv <= 4096, 1 <= nts <= 65536, D >= 1.  No
 * floating-point atomics: two calls give the same bits.  Nothing is allocated or synchronised and nothing is read back: the two
 * global stop conditions of the Lanczos iteration are words on the device that later launches read at entry, so the number of
 * launches depends on (N, m) alone.  Null pointers and sizes out of range: MTD_EINVAL, nothing launched.  Every stage takes the
 * one workspace of mtd_msid_ws_bytes and uses it from its start; nothing in it lives from one stage to the next.
 *   mtd_msid_ws_bytes     bytes of `ws` for every call below at these sizes (the largest of: |X_j|^2 and one panel of
 *                         mtd_msid_panel_rows(N) x N distances; the N x ceil(N / 32) bit mask and the degrees; the Lanczos
 *                         state with V (m, N, nv); the (2, nts, nv) quadrature table); 0 = a size out of range.
 *   mtd_msid_distances    dist (rows, N) = dd[j] - 2 X_i . X_j for row0 <= i < row0 + rows, dd[j] = |X_j|^2 (msid.py:29-32), the
 *                         products on v_mfma_f64_16x16x4_f64.  The panel that mtd_msid_neighbours selects from.
 *   mtd_msid_neighbours   nbr (N, k + 1) ints: per row the indices of its k + 1 smallest distances in rising (distance, index)
 *                         order -- the row itself among them wherever it is that near (msid.py:33; the graph drops it).  The
 *                         N x N distances are never held whole: panels of mtd_msid_panel_rows(N) rows, each selected from at
 *                         once.  A NaN distance is never selected; -1 fills a row with fewer than k + 1 candidates.
 *   mtd_msid_graph        the union of nbr's edges with their transposes, self dropped, all values 1 (msid.py:34-37,235-237) as
 *                         CSR: rowptr (N + 1) ints, col (2 N (k + 1)) ints of which the first rowptr[N] are written, each row's
 *                         columns rising.  Entries of nbr outside 0..N-1 are ignored.  A row's degree is rowptr[i + 1] - rowptr[i].
 *   mtd_msid_lanczos      msid.py:49-135 on the Laplacian of that graph (normalized != 0: I - D^-1/2 A D^-1/2, else D - A) and
 *                         the nv columns of start (N, nv): T (nv, m, m), and V (m, N, nv) where V is not NULL.  col_len: the
 *                         length of col (offsets of rowptr are clamped to it, columns outside 0..N-1 are skipped).  Full
 *                         reorthogonalisation, up to 100 further passes while any signed innerprod exceeds 1e-5, the break
 *                         when every |beta| <= 1e-6 or the passes did not converge; rows of T and V after a break stay zero.
 *                         (m - 2) * 306 + 8 launches and three memsets (m >= 3), of which (m - 2) * 299 return at entry when
 *                         no extra pass is needed.
 *   mtd_msid_quadrature   traces (2, nts): n * mean over the vectors of sum_j f(-t lambda_j) v_0j^2 (msid.py:193-199), f = exp
 *                         then f = identity, by implicit QL per vector; zero rows of T give eigenvalue 0 with first component 0.
 *   mtd_msid_combine      desc[t] = ((traces[0][t] - traces[1][t] / tables[0][t]) + tables[1][t]) / tables[2][t] * 1e6 with tables
 *                         (3, nts) = exp(ts), sub, the normalisation's divisor (msid.py:218-220,242-256,289).
 *   mtd_msid_distance     out[0] = max_t c[t] |dp[t] - dt[t]| (MTD_MSID_MAX; a NaN is handed on) or |dp - dt|_2 (MTD_MSID_L2; c
 *                         is not read).
 *   mtd_msid_descriptor   the stages chained: neighbours, graph, lanczos (V in the workspace), quadrature, combine.
 *   mtd_is_ws_bytes       bytes of `ws` of mtd_inception_score; 0 = N, D or S < 1, S > 65535 or N / S < 1.
 *   mtd_inception_score   isc.py:20-55 on logits X (N, D): out[0] = the mean, out[1] = the unbiased standard deviation (S == 1:
 *                         nan) of out[2 + s] = exp(mean KL(p(y|x) || p(y))) over the rows of split s, s < S; a split is N / S
 *                         consecutive rows, the remainder is dropped.  One workgroup per split. */
#define MTD_MSID_MAX_N 32768
enum { MTD_MSID_MAX = 0, MTD_MSID_L2 = 1 };
size_t mtd_msid_ws_bytes(int N, int D, int k, int m, int nv, int nts);
int mtd_msid_panel_rows(int N);
int mtd_msid_distances(const float* X, int N, int D, int row0, int rows, double* dist, void* ws, void* stream);
int mtd_msid_neighbours(const float* X, int N, int D, int k, int* nbr, void* ws, void* stream);
int mtd_msid_graph(const int* nbr, int N, int k, int* rowptr, int* col, void* ws, void* stream);
int mtd_msid_lanczos(const int* rowptr, const int* col, int col_len, int N, const double* start, int nv, int m, int normalized,
                     double* T, double* V, void* ws, void* stream);
int mtd_msid_quadrature(const double* T, int nv, int m, int N, const double* ts, int nts, double* traces, void* ws, void* stream);
int mtd_msid_combine(const double* traces, const double* tables, int nts, double* desc, void* stream);
int mtd_msid_distance(const double* dp, const double* dt, const double* c, int nts, int mode, double* out, void* stream);
int mtd_msid_descriptor(const float* X, int N, int D, int k, int m, int nv, int normalized, const double* start, const double* ts,
                        const double* tables, int nts, int* nbr, int* rowptr, int* col, double* T, double* traces, double* desc,
                        void* ws, void* stream);
size_t mtd_is_ws_bytes(int N, int D, int S);
int mtd_inception_score(const float* X, int N, int D, int S, double* out, void* ws, void* stream);

/* ---- FID's InceptionV3 feature network (module/piq/feature_extractors/fid_inception.py:134-168 and the block forwards
 * :198-316, built by metrics.py:17-31 compute_feat) -- DESIGN 3.9 --------------------------------------------------------
 * The 94 convolutions are mtd_conv_* launches; these are the other pieces.  Maps are NHWC fp32 on the caller's stream; source and
 * destination each have their own pixel stride (in_ld, out_ld >= C), so a pool reads a block's input and writes into a channel
 * slice of the block's output.  16-byte accesses along channels where C, both strides and both bases allow, value by value
 * otherwise: no alignment is required.  Null pointers, B <= 0, a stride smaller than the channel count, an unknown mode:
 * MTD_EINVAL, nothing launched.
 *   mtd_resize_bilinear  fid_inception.py:150-158: F.interpolate(size = (OH, OW), mode = "bilinear", align_corners = False), no
 *                        antialiasing, then 2 x - 1 when normalize != 0.  The source value of (b, c, y, x) is
 *                        in[b in_sb + c in_sc + (y W + x) in_sp] (an NCHW batch: in_sc = H W, in_sp = 1), 1 <= C <=
 *                        MTD_RESIZE_MAX_C, any H, W >= 1; out is (B, OH, OW, C) with pixel stride out_ld.  Source coordinates in
 *                        double; OH == H and OW == W copies bit for bit (before the 2 x - 1).
 *   mtd_pool3x3          :103 and torchvision's InceptionB / InceptionD: MTD_POOL_MAX_S2 = max_pool2d(3, stride 2), floor, H, W >= 3;
 *                        :311 MTD_POOL_MAX_S1P1 = max_pool2d(3, stride 1, padding 1), the padding never wins;
 *                        :215,243,276 MTD_POOL_AVG_S1P1 = avg_pool2d(3, stride 1, padding 1, count_include_pad = False): the sum of
 *                        the taps inside the image divided by their number (4 / 6 / 9).  NaN propagates as in torch.
 *   mtd_global_avgpool   :127 AdaptiveAvgPool2d((1, 1)): out[b out_ld + c] = mean over the H W pixels, summed in pixel order in
 *                        double by one thread per (b, c): the same bits on every grid, no atomics. */
#define MTD_RESIZE_MAX_C 4
enum { MTD_POOL_MAX_S2 = 0, MTD_POOL_MAX_S1P1 = 1, MTD_POOL_AVG_S1P1 = 2 };
int mtd_resize_bilinear(const float* in, long long in_sb, long long in_sc, long long in_sp, float* out, int out_ld, int B, int C,
                        int H, int W, int OH, int OW, int normalize, void* stream);
int mtd_pool3x3(const float* in, int in_ld, float* out, int out_ld, int B, int H, int W, int C, int mode, void* stream);
int mtd_global_avgpool(const float* in, int in_ld, float* out, int out_ld, int B, int H, int W, int C, void* stream);

/* ---- training-patch front end (create_datasets/Mayo.py:117-136, the "window_patch" pipeline, on the device) ----------
 * Input: the two dose levels of one or more CT slices in Hounsfield units as the reference's get_pixels_hu produces them
 * (int16, Mayo.py:19-43), resident in HBM.  mtd_foreground_bbox = CropForegroundd(source_key = full dose, select x > 0
 * after windowing, i.e. HU > a_min): per slice [y0, y1, x0, x1), the whole slice when nothing is foreground.
 * mtd_window_patches = ScaleIntensityRanged(a_min, a_max -> 0..1, clip) + crop to the box + SpatialPadd(roi) (symmetric,
 * zeros) + one roi x roi sample per descriptor (RandSpatialCropSamplesd: origin = floor(u * (size - roi + 1))) followed by
 * RandRotate90d (rot_k quarter turns, np.rot90 on axes (H, W)), RandFlipd over both axes (flip != 0) and RandRotated
 * (angle radians about the patch centre, bilinear, border padding, align_corners = False; 0 = not applied), as ONE gather
 * per output pixel.  The random draws are the caller's (the reference's come from monai's RandomState): uy, ux in [0, 1).
 * Outputs: (n, 1, roi, roi) float32 for each dose level. */
typedef struct { int slice; float uy, ux; int rot_k; int flip; float angle; } mtd_patch_desc;
int mtd_foreground_bbox(const short* hu_full, int n_slices, int H, int W, float a_min, int* bbox, void* stream);
int mtd_window_patches(const short* hu_low, const short* hu_full, int n_slices, int H, int W, const int* bbox,
                       const mtd_patch_desc* descs, int n, float a_min, float a_max, int roi, float* out_low, float* out_full,
                       void* stream);
/* whole slices (valid / test pipelines, Mayo.py:150-157): out[i] = clip((hu[i] - a_min) / (a_max - a_min), 0, 1) */
int mtd_hu_window(const short* hu, long long n, float a_min, float a_max, float* out, void* stream);

/* ---- greyscale PNG scanlines of the test loop's slices (csrc/png_gray.hip; image_io.py; reference engine.py:157-159) ----
 * x: n single-channel float32 images (n, H, W), contiguous.  out: (n, H, 1 + W * depth / 8) bytes, every row the PNG filter
 * byte 0 followed by its W samples -- what zlib takes as it is.  Any H, W >= 1 and any alignment of `out`; every byte of out
 * is written once and no other byte is touched.  One call covers all n images (three launches at depth 8, one at depth 16; grids capped and strided).
 *   depth 8  "stretch": what matplotlib's imsave(cmap="gray") gives a float32 image.  vmin / vmax = smallest / largest FINITE
 *            pixel of the image (two-stage reduction through ws, no atomics); r = float32(double(x) - double(vmin));
 *            r = float32(double(r) / (double(vmax) - double(vmin))) (the divisor is NOT rounded to float32); t = r * 256 in
 *            float32, t == 256 -> 255; level = lut[trunc(t)], below 0 -> lut[0], at or above 256 -> lut[255].  vmin == vmax:
 *            lut[0] everywhere.  A non-finite pixel: 0.  lut: 256 bytes on the device, the caller's (image_io.GRAY_LUT).
 *   depth 16 "fixed":   v = round-half-even(clamp(x, 0, 1) * 65535) in float32, most significant byte first; a non-finite
 *            pixel: 0.  lut and ws are not read (may be NULL).
 * ws: mtd_gray_png_rows_ws_bytes(n, H, W, depth) bytes, 8-byte aligned (0 for depth 16 and for refused shapes).
 * MTD_EINVAL: null pointers, n, H or W < 1, another depth, n * H * (1 + W * depth / 8) >= 2^31; MTD_EALIGN: x not 4-byte or ws
 * not 8-byte aligned.  Nothing is launched then.  The library allocates nothing. */
size_t mtd_gray_png_rows_ws_bytes(int n, int H, int W, int depth);
int mtd_gray_png_rows(const float* x, int n, int H, int W, int depth, const unsigned char* lut, unsigned char* out, void* ws,
                      void* stream);

/* ---- stored DICOM pixel values <-> Hounsfield units <-> window (csrc/dicom_domain.hip; dicom_io.py) ----------
 * The reference's get_pixels_hu (create_datasets/Mayo.py:19-43) and dicom_denormalize + save_dicom (utils.py:167-194), per pixel,
 * in their own operations.  The arrays are (S, H, W), contiguous, and taken as one run of S H W elements, S H W < 2^31; the
 * pointers need only their element's alignment (16-byte accesses where the phase allows, scalar head and tail).  rescale:
 * S pairs of doubles (slope, intercept) on the device, slice s at rescale[2 s].  One launch each; every output element is
 * written once and nothing else is touched.  No workspace, no allocation, no synchronisation.
 *   mtd_stored_to_hu      p = the word as int16 (a uint16 array is reinterpreted, 63536 = -2000); p == -2000 -> 0;
 *                         if slope != 1: p = (int16) trunc(slope * (double) p); hu = p + (int16) trunc(intercept), 16-bit wrap-around.
 *   mtd_stored_to_window  the same HU, then out = clip(((float) hu - a_min) / (a_max - a_min), 0, 1): bit for bit what mtd_hu_window
 *                         gives on mtd_stored_to_hu's output.  hu_out (may be NULL): the int16 HU as well.
 *   mtd_window_to_stored  v is clipped to [0, 1] if clip; hu = (a_max - a_min) * v, then + a_min (fp32, two roundings);
 *                         t = hu - (float) intercept; s = (int16) trunc(t); if slope != 1: s = (int16) trunc((float) s / (float) slope).
 *                         rounding 0: both casts truncate toward zero (the reference); 1: both round to nearest, ties to even.
 *                         outside 0: nothing more (the reference); 1: where the HU of ref_stored's word (mtd_stored_to_hu's
 *                         arithmetic, same rescale) lies outside [a_min, a_max], that word is written instead.  ref_stored is
 *                         read only then (may be NULL otherwise) and must not overlap out.
 * Every cast to int16 SATURATES (below -32768 -> -32768, above 32767 -> 32767, NaN -> 0): the reference's numpy casts are defined
 * only for values inside the range, where both agree.
 * MTD_EINVAL: null pointers, S, H or W < 1, S H W >= 2^31, a_max <= a_min, rounding or outside not 0 / 1, outside 1 without
 * ref_stored; MTD_EALIGN: a pointer short of its element's alignment (2 / 4 / 8 bytes).  Nothing is launched then. */
int mtd_stored_to_hu(const short* stored, int S, int H, int W, const double* rescale, short* hu_out, void* stream);
int mtd_stored_to_window(const short* stored, int S, int H, int W, const double* rescale, float a_min, float a_max, float* out,
                         short* hu_out, void* stream);
int mtd_window_to_stored(const float* v, int S, int H, int W, const double* rescale, float a_min, float a_max, int clip, int rounding,
                         int outside, const short* ref_stored, short* out, void* stream);

/* ---- sliding-window inference around a patch predictor (csrc/sliding_window.hip; inferers.py) ---------------------------
 * The reference evaluates its patch-trained models with monai's sliding_window_inference (engine.py:345,378,835).  Windows
 * of rh x rw are laid over (B, H, W) single-channel slices: per axis of length `size`, interval iv (1 <= iv <= roi),
 *     n = ceil((size - roi) / iv) + 1 windows (1 when size == roi),   start(d) = min(d * iv, size - roi);
 * the global window list runs over images outermost, then window rows, then window columns.  Nothing of it is stored.
 *   mtd_sw_gather  copies windows [w0, w0 + n) into the contiguous (n, rh, rw) buffer `out` (16-byte vectors where the
 *                  alignment of a window allows, scalar loads otherwise).
 *   mtd_sw_blend   acc(B, H, W) += sum over the windows [w0, w0 + n) of map(rh, rw) * pred(n, rh, rw): every covered pixel
 *                  adds its terms in increasing window index to the value acc holds (fused multiply-add, no atomics), so acc
 *                  must start as zeros and the chunks must come in order; the bits do not depend on how the list was cut.
 *                  Only the rows / columns / images that bound the chunk are launched; pixels outside it move no data.
 *   mtd_sw_finish  out = acc / wsum, wsum = map summed over the windows that cover the pixel (recomputed from the geometry,
 *                  same order), then clip to [0, 1] if clip01.  out may be acc.
 * A pixel covered by exactly one window carries that window's prediction through blend and finish unchanged (bit for bit).
 * MTD_EINVAL: null pointers, size < roi, iv outside 1..roi, a window range outside the list, B * H * W or n * rh * rw >= 2^31,
 * H or B > 65535. */
int mtd_sw_gather(const float* in, int B, int H, int W, int rh, int rw, int ivy, int ivx, long long w0, int n, float* out,
                  void* stream);
int mtd_sw_blend(const float* pred, const float* map, int B, int H, int W, int rh, int rw, int ivy, int ivx, long long w0, int n,
                 float* acc, void* stream);
int mtd_sw_finish(const float* acc, const float* map, int B, int H, int W, int rh, int rw, int ivy, int ivx, int clip01, float* out,
                  void* stream);
/* Several outputs of one predictor pass (inferers.sliding_window_inference_multi; the reference's module/sliding_window.py runs
 * its multi-task discriminators this way): 1 <= nplanes <= 4 planes share the geometry, the map and one launch.  preds, scalar,
 * accs, clip01 and outs are HOST arrays of nplanes entries, read before the launch (the descriptors travel in the kernel
 * arguments).
 *   mtd_sw_blend_multi   plane k: accs[k](B, H, W) += map * preds[k] over the windows [w0, w0 + n), as mtd_sw_blend.  scalar[k] == 0:
 *                        preds[k] is a map (n, rh, rw); scalar[k] != 0: preds[k] is (n) and every pixel of window w contributes
 *                        preds[k][w].  A pixel's covering windows are found once and walked once for all planes; per plane the
 *                        operations are mtd_sw_blend's, so accs[k] holds the bits one mtd_sw_blend on that plane (a scalar plane
 *                        expanded to (n, rh, rw)) would give.
 *   mtd_sw_finish_multi  plane k: outs[k] = accs[k] / wsum, clipped to [0, 1] if clip01[k]; wsum is computed once per pixel.
 *                        outs[k] may be accs[k].  The bits of mtd_sw_finish per plane.
 *   mtd_sw_gather_flags  mtd_sw_gather, and flags[i] = 1 if window w0 + i holds an element != 0.0f (-0.0f is zero, a NaN is
 *                        not), else 0, for i in [0, n): the call zeroes flags[0, n) on the stream, then every wave that saw a
 *                        nonzero element stores the constant 1 (plain byte stores, no atomics).
 * MTD_EINVAL as above, and for nplanes outside 1..4, a null array or a null plane pointer. */
int mtd_sw_blend_multi(int nplanes, const float* const* preds, const int* scalar, float* const* accs, const float* map, int B, int H,
                       int W, int rh, int rw, int ivy, int ivx, long long w0, int n, void* stream);
int mtd_sw_finish_multi(int nplanes, const float* const* accs, const int* clip01, float* const* outs, const float* map, int B, int H,
                        int W, int rh, int rw, int ivy, int ivx, void* stream);
int mtd_sw_gather_flags(const float* in, int B, int H, int W, int rh, int rw, int ivy, int ivx, long long w0, int n, float* out,
                        unsigned char* flags, void* stream);

/* ---- backward of one 32 -> 32 channel 3x3 generator layer in ONE launch (csrc/conv_c32_bwd.hip) ----------------------
 * d: the data gradient exactly as mtd_conv_igemm would take it (it must be a launch of the halo-tile kernel: C == N == 32,
 * 3x3, stride 1, 64-pixel rows, whole four-row tiles); w: the weight + bias gradient of the same layer exactly as
 * mtd_conv_wgrad_slabs would take it (reference: the backward of arch/Ours/networks.py:21-36 img_conv and :95-164
 * encoder / decoder layers, which autograd runs as two ATen kernels).  Slabs go to w->ws (mtd_conv_c32_bwd_ws_bytes),
 * to be summed by mtd_conv_wgrad_reduce_multi.  mtd_conv_c32_bwd_ok: 1 if the pair is eligible. */
int mtd_conv_c32_bwd_ok(const mtd_conv_args* d, const mtd_wgrad_args* w);
size_t mtd_conv_c32_bwd_ws_bytes(const mtd_conv_args* d, const mtd_wgrad_args* w);
int mtd_conv_c32_bwd(const mtd_conv_args* d, const mtd_wgrad_args* w, int* nslab, long long* slab_stride, void* stream);
/* The same launch closing the backward pass of a Res-FFT-Conv block (autograd of arch/Ours/networks.py:21-36):
 *     d->out = mask'( dgrad + add1 + add2 + irfft_rows(gT) ),   gT = output of mtd_spec_mix_bwd / _bwd4,
 * i.e. mtd_conv_c32_bwd followed by mtd_irfft_rows(gT, out, add1 = that result, mask) without the second launch: the
 * rfft2-backward row transform is 33 more MFMAs per 32-pixel block against an inverse-DFT matrix in LDS.  64 x 64 maps. */
int mtd_conv_c32_bwd_irfft(const mtd_conv_args* d, const mtd_wgrad_args* w, const float* gT, int* nslab, long long* slab_stride,
                           void* stream);
int mtd_conv_c32_bwd_stamps(unsigned long long* host256);   /* lab (MTD_C32F_STAMPS=1): clock stamps of the last launch's first 16 workgroups */

/* ---- launch profiler (bench.py's roofline leg) ---------------------------------------------------------------
 * When enabled, mtd_conv_igemm / mtd_conv_wgrad time their MAIN kernel (not the split-K / slab reductions that
 * follow it) with a pair of HIP events on the stream they were given (see mtd_prof_mode).  mtd_prof_collect synchronises those events
 * and returns one record per launch.  kernel: 0 = igemm_kernel, 1 = wgrad_kernel, 2 = the HBM-bound spectral kernels of the
 * whole-slice inference path (cfg 0 rfft_rows_any, 1 spec_mix_any, 2 irfft_rows_any: flops 0, bytes set); cfg = tile configuration index
 * (the template instantiation); flops = 2*M*N*C*taps (dense algorithmic count).
 * Not for use while a hipGraph is being captured. */
/* Tuning hook (tools/tune_igemm.py): force the tile configuration (0..8, -1 = automatic) and the split-K factor of
 * every following mtd_conv_igemm call in this process.  9 / 10 leave the plan automatic and pick the persistent / the
 * halo-tile kernel for the generator-shaped layers (C == 32, 3x3, M >= 32768). */
int mtd_conv_igemm_override(int cfg, int splitk);
int mtd_conv_wgrad_override(int cfg, int nsplit);      /* same for mtd_conv_wgrad: tile/tap-group config 0..6, pixel splits */

typedef struct mtd_prof_record {
    int kernel, cfg, splitk, N, C, taps;
    long long M;
    double flops;
    float ms;
    int _pad;
    double bytes;     /* algorithmic HBM bytes of the launch: every distinct operand element read once, every result written once */
} mtd_prof_record;
int mtd_prof_enable(int capacity);                       /* capacity <= 0 switches profiling off and frees events */
int mtd_prof_collect(mtd_prof_record* out, int max_records);   /* returns the number of completed records */
/* Timing mode of the profiler: 1 (default) = the events ride on the kernel's dispatch packet (duration = the dispatch's
 * own begin / end timestamps, what a kernel trace reports); 0 = hipEventRecord before / after the launch.  attach < 0
 * only queries.  Returns the mode in effect, MTD_EINVAL while records are pending. */
int mtd_prof_mode(int attach);

const char* mtd_version(void);

/* ---- run-time options.  The shipped library reads NO environment variable (round 5): the kernel-selection and tuning
 * switches of earlier rounds exist only in a build with -DMTD_LAB (mtd_lab_build() == 1; tools/ probes).  What may be changed
 * at run time goes through these two calls, by name; unknown names return MTD_EINVAL.
 *   "c32f_safe_wait"  0 (default) | 1: the fused 32-channel backward launch waits for ALL outstanding vector-memory operations
 *                     before it hands a halo buffer to the next DMA, instead of the counted wait (a checking mode:
 *                     tests/test_kernels_gpu.py::test_fused_c32_backward_counted_waits_same_bits).
 *   "wino_split"      0 (default) | 1: the 3x3 stride-1 layers with N % 64 == 0 run their Winograd products on the fp32 MFMA
 *                     (wino_conv_kernel) | on the bf16 matrix pipe from exact three-way bf16 splits of both operands (six
 *                     products per fp32 product, fp32 accumulation: fp32 accuracy at 2.7x the fp32 MFMA rate;
 *                     csrc/conv_winograd_split.h).  Measured (profiles/r5_wino3_parts.txt): the launches are bound by the
 *                     vector-memory path, not the matrix pipe -- 5-20 % per launch on hot inputs, nothing in the step -- so
 *                     the fp32 kernel stays the default.  Callers that cache mtd_conv_winograd_patch_w's answers drop them
 *                     after a change (tests/test_kernels_gpu.py::test_winograd_conv_vs_torch runs both).
 * Plan-level tuning hooks with their own entry points: mtd_conv_winograd_f4_min_w, mtd_conv_wgrad_plan_cfg, mtd_prof_mode. */
int mtd_set_option(const char* name, int value);
int mtd_get_option(const char* name, int* value);
int mtd_lab_build(void);

#ifdef __cplusplus
}
#endif
#endif
