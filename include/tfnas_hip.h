/*
 * tfnas_hip.h -- C ABI of the MI355X (gfx950) hot path of the TF-NAS supernet search step.
 *
 * The reference has NO native/FFI boundary for this path: its boundary is the Python
 * nn.Module API of models/model_search.py.  This header is therefore the boundary *we* define below that
 * API: the Python modules in tf-nas_amd/tfnas_amd/model_search.py (same class names, constructor and
 * forward(x, sampling, mode) signatures as the reference) call these entry points through ctypes with raw
 * device pointers.  Each entry point cites the reference code whose arithmetic it replaces.
 *
 * Conventions
 *  - all tensors are fp32, activations are NHWC
 *    ("channels_last"): x[n][h][w][c], c fastest;
 *  - the caller (PyTorch) owns and allocates every buffer, including saved-for-backward tensors and
 *    scratch; sizes come from tfnas_cell_ws();
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises;
 *  - return value: 0 ok, <0 invalid argument (TFNAS_E*), >0 a hipError_t;
 *  - re-entrant per stream; every mode and every kernel-variant choice of a launch is given in its descriptor (gemm_mode, flags,
 *    route, sync_fn); the library reads no environment variable.  The only
 *    process-global state is the DEFAULTS of three modes (tfnas_set_gemm_mode / _lazy_join / _stats_sync), a registry of library-owned side streams (one per
 *    caller stream and device, created on first use by tfnas_mixedop_bwd with need_wgrad; released by
 *    tfnas_shutdown()) and the opt-in tfnas_prof_* timers; results never depend on either.
 *
 * A "cell" is one MixedOP (18 per network); its G "groups" are the MBConv candidates evaluated in this
 * call: G = 8 in the soft (alpha-step) mode, G = 1 in the sampled (w-step) mode.  All groups' expanded
 * channels live side by side in one [pixels][M] tensor (M = sum of padded mid widths) so that the 1x1
 * expand of all candidates is ONE GEMM and every per-channel pass (BN statistics, depthwise, SE) runs
 * once over the concatenation.
 */
#ifndef TFNAS_HIP_H
#define TFNAS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4, additive: TFNAS_PATH_EXTENDED (TfnasPathDesc.path_flags, the word that had to be 0) -- tfnas_path_plan takes every cell
 * tfnas_cell_plan takes in cell mode (the three kinds, TFNAS_CELL_KINDS with or without TFNAS_CELL_SKIP groups, packed groups) and
 * the pass-through cell of a sampled skip; without the bit it refuses them as before.  No struct, no entry point changed.
 * 4, additive: TFNAS_CELL_MIXK -- a packed TfnasGroup.k: MixConv candidates, one depthwise whose channel segments are 3 x 3 | 5 x 5 | 7 x 7.
 * 4, additive: TFNAS_CELL_DILATION -- TfnasGroup.dil: depthwise candidates with taps two pixels apart (3 x 3 and 5 x 5).
 * 4, additive: TFNAS_CELL_SKIP -- TFNAS_GROUP_SKIP: the identity candidate in a residual TFNAS_CELL_KINDS cell.
 * 4, additive: TFNAS_CELL_SE_STYLE -- TfnasCellDesc.se_style: the squeeze-excite hidden activation and gate function of a cell.
 * 4, additive: TFNAS_CELL_KINDS -- a per-group kind (TfnasGroup.kind): plain, expand-free and Fused-MBConv candidates in ONE cell.
 * 4, additive: TFNAS_CELL_FUSED -- a Fused-MBConv block (dense 3 x 3 convolution, no depthwise) through tfnas_mixedop_* / tfnas_mbconv_*.
 * 4, additive: TFNAS_CELL_NOEXPAND -- a block without expand convolution (mid <= in channels) through tfnas_mixedop_* / tfnas_mbconv_*.
 * 4, additive: TFNAS_ACT_RELU6 / TFNAS_ACT_HSWISH in a descriptor whose flags carry TFNAS_CELL_ACTS (cells, affine blocks, head;
 * materialised route and LDS tile depthwise kernels only).
 * 4, additive: tfnas_cls_wgrad_ex (tfnas_cls_wgrad + the search epoch's running loss / top-1 / top-5 / invalid-target meter).
 * 4, additive: tfnas_cls_ce_ex / tfnas_cls_reduce (the derived network's retrain tail: label smoothing, rank, forward-only form,
 * device-side upstream gradient, running meter).
 * 4, additive: TFNAS_CELL_ACCUM_WGRAD (weight gradients added to their destinations, per launch) and tfnas_path_set_wgrad_accum.
 * 4 (round 6): every route switch of a launch lives in its descriptor (TfnasCellDesc.route: TFNAS_ROUTE_*); the library reads no
 * environment variable at launch time (the TFNAS_* variables only seed the Python-side defaults, functions.route_from_env).
 * tfnas_cell_route() + TfnasCellDesc.fwd_route: a backward refuses a descriptor whose route differs from the forward's.
 * TfnasCellDesc.wgrad_stream[3]: caller-owned streams for the three weight-gradient forks of ONE launch (the stem cell's backward
 * runs alone on the chip: its four weight-gradient kernels spread over the queues the two finished paths left idle).
 * tfnas_cls_ce / tfnas_cls_wgrad: classifier + cross-entropy of the weight step in two launches.
 * 3 (round 5): tfnas_fx_supported (fused per-image route of the late cells); per-launch modes in TfnasCellDesc (gemm_mode, flags,
 * sync_fn / sync_user / sync_world: the process-wide setters only provide defaults).
 * 2 (round 4): arithmetic modes of the GEMMs (tfnas_set_gemm_mode); the per-group input / output mode of TfnasCellDesc (xg /
 * og), TfnasPathDesc.dual, tfnas_path_set_side_stream2 and tfnas_path_defer_join / tfnas_path_join were measured and removed */
#define TFNAS_ABI_VERSION 4
#define TFNAS_MAX_GROUPS 8
#define TFNAS_MAX_SINK 4
#define TFNAS_MAX_CELLS 32

/* TfnasCellDesc.mode */
#define TFNAS_MODE_CELL 0   /* a MixedOP cell: 1x1 expand from an NHWC input (default)                          */
#define TFNAS_MODE_STEM 1   /* first_stem + second_stem (model_search.py:219-220) as ONE cell whose "expand" is the
                               3x3 stride-2 pad-1 convolution of the 3-channel NCHW image (x = image, ic = 27 =
                               im2col depth, w_expand = first_stem.conv.weight [32][3*3*3]); G = 1, no dx           */
#define TFNAS_MODE_HEAD 2   /* feature_mix_layer + global average pool (model_search.py:299-300): E = x W^T,
                               pooled = mean_hw act(BN(E)); only tfnas_head_fwd/bwd accept it.  g[0].mc must be a
                               multiple of 4 (else TFNAS_EINVAL from tfnas_cell_plan and every head entry point): the
                               [N][mc] rows of pooled / dpooled move in quads                                       */

#define TFNAS_ACT_RELU 0
#define TFNAS_ACT_SWISH 1
/* The reference's other two (models/layers.py:38-47), accepted only from a descriptor whose flags carry TFNAS_CELL_ACTS, in
 * TFNAS_MODE_CELL (tfnas_mixedop_*, tfnas_mbconv_*, the path level) and TFNAS_MODE_HEAD; TFNAS_MODE_STEM refuses them.
 * With z the BatchNorm output, at all three sites (after BN1, after BN2, the SE hidden layer; the SE gate stays a sigmoid):
 *   RELU6   min(max(z, 0), 6);           derivative 1 where 0 < z < 6 (strict), else 0
 *   HSWISH  z * min(max(z + 3, 0), 6) / 6; derivative (2 z + 3) / 6 where -3 < z < 3 (strict), 1 where z >= 3, 0 where z <= -3
 * A cell with one of them always materialises E (tfnas_efree_supported and tfnas_fx_supported return 0) and runs its depthwise
 * passes on the LDS tile kernels whatever TfnasCellDesc.route asks, the depthwise weight gradient in its own launch: the ring,
 * register-window, E-free and fused per-image kernels exist for ReLU and Swish only. */
#define TFNAS_ACT_RELU6 2
#define TFNAS_ACT_HSWISH 3

#define TFNAS_EINVAL (-1)   /* bad geometry / alignment (ic, oc must be multiples of 4) */
#define TFNAS_ENULL (-2)    /* required pointer is NULL */
#define TFNAS_ERANGE (-3)   /* count out of range */

/* One MBConv candidate (reference: MBInvertedResBlock, models/layers.py:431-561).  Weight pointers are
 * the reference's OIHW nn.Parameter storages used as-is:
 *   w_expand [mc][ic]      inverted_bottleneck.conv.weight  [mc,ic,1,1]
 *   w_dw     [mc][k*k]     depth_conv.conv.weight           [mc,1,k,k]
 *   w_proj   [oc][mc]      point_linear.conv.weight         [oc,mc,1,1]
 *   w_se_r   [se][mc], b_se_r [se]   squeeze_excite.conv_reduce.{weight,bias}
 *   w_se_e   [mc][se], b_se_e [mc]   squeeze_excite.conv_expand.{weight,bias}
 * g_* are the matching gradient outputs (same shapes), only read/written when need_wgrad != 0.
 * k: 3, 5 or -- in a descriptor whose flags carry TFNAS_CELL_K7 -- 7 (pad k / 2); any other value, and 7 without the bit, is
 * TFNAS_EINVAL.  A cell with a 7 x 7 group runs its depthwise passes on the LDS tile
 * kernels whatever TFNAS_ROUTE_DW_* asks (the register-window and ring kernels are built for 3 and 5), keeps the depthwise weight
 * gradient in its own launch, and always materialises E: tfnas_efree_supported and tfnas_fx_supported return 0 for it.  The groups'
 * depthwise weight gradients share one row of partial sums: sum of mc * k * k above 4 Mi - 1024 floats is TFNAS_ERANGE
 * (tfnas_cell_plan, tfnas_cell_ws); eight 7 x 7 groups of 1536 channels fit. */
typedef struct TfnasGroup {
    int32_t mc;       /* mid channels (any integer > 0, e.g. 53)            [in]  */
    int32_t k;        /* depthwise kernel size: 3 or 5; 7 with TFNAS_CELL_K7; with TFNAS_CELL_MIXK also a packed word
                         (0x53, 0x73, 0x75, 0x753: one nibble per channel segment)  [in]  */
    int32_t se;       /* squeeze-excite width (a multiple of 4), 0 = no SE   [in]  */
    int32_t mcp;      /* mc rounded up to a multiple of 4                   [plan] */
    int32_t off;      /* first column of this group in the [.][M] tensors (multiple of 32) [plan] */
    int32_t se_off;   /* first column in the [N][SE] hidden tensors         [plan] */
    int32_t kind;     /* TFNAS_GROUP_*: read only from a descriptor whose flags carry TFNAS_CELL_KINDS [in]  */
    int32_t dil;      /* depthwise dilation: 0 or 1 = none, 2 = taps two pixels apart (pad 2 * (k / 2), k 3 or 5); read only
                         from a descriptor whose flags carry TFNAS_CELL_DILATION (this word was padding, pad1, before) [in]  */
    const float *w_expand, *w_dw, *w_proj, *w_se_r, *b_se_r, *w_se_e, *b_se_e;
    float *g_expand, *g_dw, *g_proj, *g_se_r, *gb_se_r, *g_se_e, *gb_se_e;
} TfnasGroup;

typedef struct TfnasCellDesc {
    int32_t N, H, W;          /* input batch / height / width                       [in] */
    int32_t ic, oc;           /* cell in/out channels (multiples of 4)              [in] */
    int32_t stride;           /* 1 or 2 (depthwise stride; pad = k/2)               [in] */
    int32_t act;              /* TFNAS_ACT_*                                        [in] */
    int32_t has_res;          /* 1 when ic==oc && stride==1 (layers.py:537)         [in] */
    int32_t G;                /* number of groups, 1..8                             [in] */
    int32_t need_wgrad;       /* backward also produces weight gradients            [in] */
    int32_t Ho, Wo;           /* output height / width                              [plan] */
    int32_t M;                /* row length of the [.][M] tensors: groups padded to 32-float (128 B) boundaries [plan] */
    int32_t SE;               /* sum of se over groups                              [plan] */
    float eps;                /* BatchNorm eps (1e-5)                               [in] */
    int32_t mode;             /* TFNAS_MODE_CELL / _STEM / _HEAD                    [in] */
    int32_t Hi, Wi;           /* stem mode: height / width of the NCHW input image  [in] */
    int32_t stor;             /* must be 0 (fp32 storage of the [pixels][M] stream tensors E, D, dZ, dEh).  Rounds 1-3 had a
                                 second build that kept these four tensors in bf16 (stor = 1); it measured 0.99-1.04x of the
                                 fp32 iteration pair (the step is not bound by HBM bytes) and was removed.          [in] */
    int32_t gemm_mode;        /* 0: the process default (tfnas_set_gemm_mode); TFNAS_GEMM_EXPLICIT | TFNAS_GEMM_*: the arithmetic
                                 of THIS launch's 1x1 GEMMs, whatever the default is (two models in one process in different
                                 modes: an fp32-exact search net beside a bf16-GEMM derived net)                      [in] */
    int32_t flags;            /* TFNAS_CELL_LAZY_JOIN: tfnas_mbconv_bwd returns without joining its weight-gradient side
                                 stream (see tfnas_set_lazy_join, which sets the default for descriptors without the bit);
                                 TFNAS_CELL_ACCUM_WGRAD: the backward adds its weight gradients to their destinations;
                                 TFNAS_CELL_K7: groups may have depthwise kernel size 7;
                                 TFNAS_CELL_ACTS: act may be TFNAS_ACT_RELU6 / TFNAS_ACT_HSWISH;
                                 TFNAS_CELL_NOEXPAND: the one group has no expand convolution;
                                 TFNAS_CELL_FUSED: the one group is a Fused-MBConv block (dense 3 x 3 convolution);
                                 TFNAS_CELL_KINDS: every group has a kind of its own (TfnasGroup.kind);
                                 TFNAS_CELL_SE_STYLE: se_style may be non-zero;
                                 TFNAS_CELL_SKIP: groups may be TFNAS_GROUP_SKIP, the identity candidate;
                                 TFNAS_CELL_DILATION: groups may have depthwise dilation 2 (TfnasGroup.dil);
                                 TFNAS_CELL_MIXK: TfnasGroup.k may be a packed word of two or three kernel sizes          [in]
                                 (bit 4 was TFNAS_CELL_FXP, the fused per-image project dgrad of round 5: measured equal to the
                                 default kernels over two rounds and deleted in round 6) */
    TfnasGroup g[TFNAS_MAX_GROUPS];
    /* per-launch cross-rank statistics hook (see tfnas_set_stats_sync: that one is the default for descriptors with
       sync_fn == NULL); sync_world >= 1 */
    int (*sync_fn)(void *user, double *table, uint64_t ndoubles, void *stream);
    void *sync_user;
    int32_t sync_world;
    int32_t route;            /* TFNAS_ROUTE_* bits: deviations of THIS launch from the library's measured per-launch policy
                                 (0 = the policy).  The library reads no environment variable at launch time: every kernel
                                 variant is selected here, per launch, so variants can be compared in one process           [in] */
    int32_t fwd_route;        /* backward only: the value tfnas_cell_route() returned for the descriptor the FORWARD of these
                                 buffers ran with (0 = not given: the backward trusts its own decision).  A backward whose own
                                 route differs in a way that changes what the saved buffers mean (the fused per-image route
                                 leaves ehat = BN1(E), not E, in the E buffer) returns TFNAS_EINVAL instead of silently
                                 normalising twice                                                                          [in] */
    int32_t se_style;         /* TFNAS_SE_*: hidden activation and gate function of the cell's squeeze-excite branches; non-zero
                                 only in a descriptor whose flags carry TFNAS_CELL_SE_STYLE (0 = the cell's act, logistic gate).
                                 This word was padding (pad_route) before: no struct changed size.  It is not part of the route:
                                 tfnas_cell_route() ignores it, forward and backward each read it from their descriptor      [in] */
    void *wgrad_stream[3];    /* optional caller-owned streams for the weight-gradient kernels of this launch: fork 0 = project,
                                 1 = squeeze-excite + depthwise, 2 = expand weight gradient.  NULL entries: the library-owned
                                 side stream of the caller's stream.  Every stream used is joined before tfnas_mixedop_bwd
                                 returns.  tfnas_mixedop_bwd only; with any entry set its `part` buffer must hold FOUR pieces
                                 of tfnas_sizeof(7) floats (chain | fork 0 | fork 1 | fork 2: concurrent forks do not share
                                 split-K scratch) instead of two                                                            [in] */
} TfnasCellDesc;
#define TFNAS_GEMM_EXPLICIT 0x1000
#define TFNAS_CELL_LAZY_JOIN 1
/* TfnasCellDesc.flags: every weight-gradient output of the launch is ADDED to what its destination already holds, g <- g + v,
 * where v is bit for bit what the same launch stores without the bit (BLAS beta = 1; one more read of each gradient, no extra
 * launch, no scratch).  Destinations: the g_* pointers of every group and, in the affine entry points, TfnasBnAffine.g_weight /
 * g_bias.  Statistics outputs are never accumulated.  Honoured by tfnas_mixedop_bwd (cell, stem and head modes),
 * tfnas_mbconv_bwd, tfnas_head_bwd, tfnas_head_wgrad, tfnas_head_affine_bwd and, through the planned cells,
 * tfnas_paths_bwd (tfnas_path_set_wgrad_accum).  This is how gradients are summed over micro-batches and over several backward
 * passes through the same weights (autograd's .grad semantics).
 * Ordering is the caller's: a launch with the bit set must not read a gradient range that another stream may still be writing --
 * the side stream that tfnas_mbconv_bwd leaves unjoined with TFNAS_CELL_LAZY_JOIN (tfnas_side_join first, or keep every launch
 * that touches the range on the same caller stream, whose side stream is then the same), the caller-owned wgrad_stream[] forks
 * of an earlier launch, and the other bi-sampling path of tfnas_paths_bwd (two paths never share a gradient range).
 * (0x2, 0x4, 0x8 are undefined; 0x10 was TFNAS_CELL_FXP, retired: all are refused.) */
#define TFNAS_CELL_ACCUM_WGRAD 0x20
/* TfnasCellDesc.flags: the caller knows depthwise kernel size 7 (TfnasGroup.k).  Additive like TFNAS_CELL_ACCUM_WGRAD: without the
 * bit every descriptor is accepted or refused exactly as before it existed (k = 7 is TFNAS_EINVAL: callers that probe
 * tfnas_cell_plan for what the library can run, and fall back otherwise, keep seeing that); with it, groups may have k = 7 and
 * nothing else changes -- a descriptor of 3 x 3 / 5 x 5 groups plans, routes and launches the same with or without the bit.  Checked
 * by tfnas_cell_plan and again by every entry point (the descriptor's modes may change between the two).  The Python mirror sets it
 * for every descriptor that holds a 7 x 7 group (functions.HipModes.apply). */
#define TFNAS_CELL_K7 0x80
/* TfnasCellDesc.flags: the caller knows the activations TFNAS_ACT_RELU6 and TFNAS_ACT_HSWISH.  Additive in the same way: without
 * the bit act = 2, 3 stay TFNAS_EINVAL; with it a ReLU / Swish descriptor plans, routes and launches the same, and act may also be
 * 2 or 3 (any other value is TFNAS_EINVAL either way).  Checked by tfnas_cell_plan and again by every entry point.  The Python
 * mirror sets it for every descriptor with one of the two (functions.HipModes.apply). */
#define TFNAS_CELL_ACTS 0x100
/* TfnasCellDesc.flags: the caller knows cells WITHOUT an expand convolution -- the reference's MBInvertedResBlock with
 * mid_channels <= in_channels (models/layers.py:463-482: no inverted_bottleneck), the "expand ratio 1" block of the MobileNet family
 * and the reference's own second_stem:  out = BN3(project(SE(act(BN2(dw(x)))))) [+ x].  Additive like TFNAS_CELL_K7: without the
 * bit every descriptor is accepted, refused, planned, routed and launched exactly as before it existed.  With it the descriptor
 * describes ONE such block:
 *   geometry   mode == TFNAS_MODE_CELL, G == 1, g[0].mc == ic, g[0].w_expand == NULL and g[0].g_expand == NULL; anything else --
 *              G > 1, mc != ic, an expand pointer, stem or head mode -- is TFNAS_EINVAL, and so is tfnas_path_plan on a cell that
 *              carries the bit (unless the path says TFNAS_PATH_EXTENDED).  A mixed cell in which only SOME candidates lack the expand convolution is deliberately out of scope.
 *              k in {3, 5, 7 (TFNAS_CELL_K7)}, all four activations (two with TFNAS_CELL_ACTS), stride 1 | 2, se 0 or a multiple of
 *              4, ic any multiple of 4 >= 4, has_res as for any cell.
 *   arithmetic D = dw(x) on the raw cell input: no BatchNorm and no activation before the depthwise convolution; `act` applies after
 *              BN2 and in the SE hidden layer only.  Everything after D is the ordinary cell.
 *   workspace  tfnas_cell_ws reports E = 0 and dxp = 4 (the minimum).  The entry points accept E == NULL (dxp too) and never touch
 *              E, stats1, red1 or cb1 (their slots in stats / red / bsmall keep their offsets).  dEh STAYS [N*H*W][M]: it is never a
 *              gradient tensor here, but still the scratch of the project dgrad's BN2-backward records and of the SE backward's
 *              K-split partials.  The backward writes dx [N*H*W][ic] straight from the depthwise backward-data pass, the residual
 *              gradient added in the same store (in the affine form with drop-connect: the unscaled dout).
 *   routes     tfnas_efree_supported and tfnas_fx_supported return 0, tfnas_cell_route returns TFNAS_ROUTE_TAKEN_VALID.  The cell
 *              runs its depthwise passes on the LDS tile kernels (their raw-input form) whatever TFNAS_ROUTE_DW_* asks, the depthwise
 *              weight gradient in its own launch (the 7 x 7 rule).  TFNAS_ROUTE_XG_* and TFNAS_ROUTE_GRAM2 mean nothing to it and are
 *              ignored; the SE and TFNAS_ROUTE_WGRAD_INLINE bits are honoured; weight-gradient fork 2 (wgrad_stream[2]) is never used.
 *   modes      tfnas_mixedop_fwd/bwd (sampled form, wmix == NULL) and tfnas_mbconv_fwd/bwd; TFNAS_CELL_ACCUM_WGRAD,
 *              TFNAS_CELL_LAZY_JOIN, wgrad_stream[], the GEMM modes (the project GEMMs) and the sync-stats hook (two forward tables,
 *              two backward tables) as for any cell.
 *   affine     BatchNorm site 0 does not exist: every site-0 pointer of TfnasBnAffine must be NULL (else TFNAS_EINVAL).
 * Checked by tfnas_cell_plan and again by every entry point.  The Python mirror sets it for a block whose inverted_bottleneck is
 * None (functions.HipModes.apply). */
#define TFNAS_CELL_NOEXPAND 0x200
/* TfnasCellDesc.flags: the caller knows Fused-MBConv blocks (EfficientNetV2, MobileNet-EdgeTPU, MnasNet-fused): ONE dense 3 x 3
 * convolution in place of the 1 x 1 expand plus the depthwise convolution,
 *   out = BN_b(project(SE(act(BN_a(conv3x3(x, W_f[mc][ic][3][3], stride, padding 1)))))) [+ x].
 * Additive like TFNAS_CELL_NOEXPAND: without the bit every descriptor is accepted, refused, planned, routed and launched exactly
 * as before it existed.  With it the descriptor describes ONE such block:
 *   geometry   mode == TFNAS_MODE_CELL, G == 1, g[0].k == 3, stride 1 | 2, ic a multiple of 4, any g[0].mc >= 1 (ragged widths
 *              included), se 0 or a multiple of 4, all four activations (two with TFNAS_CELL_ACTS), has_res as for any cell.
 *              g[0].w_expand / g_expand hold the dense weight / its gradient in torch's OIHW order [mc][ic][3][3]; g[0].w_dw and
 *              g[0].g_dw are NULL.  Two groups, k != 3, a depthwise pointer, the bit together with TFNAS_CELL_NOEXPAND, stem or
 *              head mode are TFNAS_EINVAL, and so is tfnas_path_plan on a cell that carries the bit (unless the path says
 *              TFNAS_PATH_EXTENDED).  A width whose
 *              weight-gradient partial row (9 ic mc floats) does not fit the partial-row scratch, or whose repacked weight
 *              (9 ic mcp floats) does not fit it next to 128 statistics rows of 2 M floats, is TFNAS_ERANGE at plan time (the
 *              widest block of the supernet, 192 -> 1536, fits); the depthwise-only limits do not apply.
 *              No bias, no 5 x 5 / 7 x 7, always a project convolution.
 *   arithmetic D = conv3x3(x) on the raw cell input in the launch's GEMM mode (gemm_mode: split-bf16 by default, fp32 or bf16 on
 *              request, fp32 accumulation; the weight gradient always in fp32 MFMA like every weight gradient of the library).
 *              Everything after D is the ordinary cell: BN_a / BN_b are BatchNorm sites 1 and 2.
 *   workspace  tfnas_cell_ws reports E = 0 and dxp = 4.  The entry points accept E == NULL (dxp too) and never touch E, stats1,
 *              red1 or cb1.  The convolution writes D at Ho x Wo.  dEh keeps its size [N*H*W][M]: after the SE backward has used
 *              it as scratch it holds dd, the gradient w.r.t. D [N*Ho*Wo][M], which the weight-gradient and the data-gradient
 *              GEMM both read.  The backward writes dx [N*H*W][ic] from the data-gradient GEMM, the residual gradient added in
 *              the same store (in the affine form with drop-connect: the unscaled dout); dx == NULL skips that launch.
 *   routes     tfnas_efree_supported and tfnas_fx_supported return 0, tfnas_cell_route returns TFNAS_ROUTE_TAKEN_VALID.
 *              TFNAS_ROUTE_DW_*, TFNAS_ROUTE_XG_* and TFNAS_ROUTE_GRAM2 mean nothing to it and are ignored; the SE, FOLD and
 *              TFNAS_ROUTE_WGRAD_INLINE bits are honoured; weight-gradient fork 2 (wgrad_stream[2]) is never used: the SE and
 *              the convolution weight gradients share fork 1.
 *   modes      tfnas_mixedop_fwd/bwd (sampled form, wmix == NULL) and tfnas_mbconv_fwd/bwd; TFNAS_CELL_ACCUM_WGRAD,
 *              TFNAS_CELL_LAZY_JOIN, wgrad_stream[], the GEMM modes, the sync-stats hook (two forward tables, two backward
 *              tables), need_wgrad = 0 and dx == NULL as for any cell.
 *   affine     BatchNorm site 0 does not exist: every site-0 pointer of TfnasBnAffine must be NULL (else TFNAS_EINVAL).
 * Checked by tfnas_cell_plan and again by every entry point.  The Python mirror sets it for a one-block plan whose block is a
 * layers.FusedMBConvBlock (functions.HipModes.apply). */
#define TFNAS_CELL_FUSED 0x400
/* TfnasCellDesc.flags: the caller knows cells whose candidates differ in kind.  Additive like the two bits above: without the bit
 * TfnasGroup.kind is not read and every descriptor means what it meant before (TFNAS_CELL_NOEXPAND / TFNAS_CELL_FUSED with G > 1
 * stay TFNAS_EINVAL).  With it every group g says what it is in g.kind:
 *   TFNAS_GROUP_MBCONV    expand 1 x 1 + BN + act + depthwise k x k (the ordinary candidate)
 *   TFNAS_GROUP_NOEXPAND  depthwise k x k of the raw cell input: mc == ic, w_expand == NULL and g_expand == NULL
 *   TFNAS_GROUP_FUSED     dense 3 x 3 convolution of the raw cell input: k == 3, the OIHW weight [mc][ic][3][3] in w_expand /
 *                         g_expand, w_dw == NULL and g_dw == NULL
 * and the cell computes  out = sum_g wmix[g] BN3_g(project_g(SE_g(act(BN2_g(front_g(x)))))) [+ x]  in the caller's group order
 * (dwmix[g] belongs to group g).  Rules, checked by tfnas_cell_plan and again by every entry point:
 *   - mode == TFNAS_MODE_CELL only; TFNAS_CELL_NOEXPAND and TFNAS_CELL_FUSED must both be clear; a kind outside 0..2, a NOEXPAND
 *     group with mc != ic or an expand pointer, a FUSED group with k != 3 or a depthwise pointer are TFNAS_EINVAL;
 *   - TFNAS_CELL_K7 / TFNAS_CELL_ACTS apply as before; the size limits of the one-block kinds hold per group (the dense weight's
 *     partial row and repacked copy of every FUSED group; the depthwise weight-gradient row of the MBCONV groups and of the
 *     NOEXPAND groups): TFNAS_ERANGE;
 *   - tfnas_mbconv_fwd/bwd and tfnas_path_plan (without TFNAS_PATH_EXTENDED) refuse the bit (TFNAS_EINVAL); tfnas_efree_supported and tfnas_fx_supported return
 *     0 when any group is not plain: the plain groups of such a cell always materialise E (E == NULL is TFNAS_ENULL);
 *   - tfnas_cell_ws reports E = 0 when no group is plain (E, stats1, red1, cb1 are then never touched);
 *   - a descriptor whose groups are ALL TFNAS_GROUP_MBCONV, and a ONE-group descriptor of any kind, plan, size, route and run
 *     exactly like the same descriptor without the bit (the one group under its own TFNAS_CELL_NOEXPAND / _FUSED bit).
 * Launch sequence of a cell with groups of more than one kind: the fronts run per kind on their own groups' columns
 * of the [pixels][M] tensors -- the MBCONV groups' expand + depthwise, the NOEXPAND groups' raw-input depthwise, one dense
 * convolution per FUSED group -- then everything from the SE squeeze to the mix runs once over all groups.  The backward runs
 * the shared prefix once, then the MBCONV groups' tail, the NOEXPAND groups', the FUSED groups'.  dx is written by the first
 * branch in that order (with the residual gradient, once) and read-added-stored by every later one on the caller's stream: a
 * fixed summation order, no atomics, bit-reproducible.  Weight gradients go to the forks as for the one-block kinds (fork 1
 * carries the SE, depthwise and dense-convolution weight gradients in stream order).  TFNAS_CELL_ACCUM_WGRAD, dx == NULL,
 * need_wgrad == 0, the dwmix-only early return, wgrad_stream[] and the sync-stats hook keep their meaning. */
#define TFNAS_CELL_KINDS 0x800
/* TfnasCellDesc.flags: the caller knows squeeze-excite styles (TfnasCellDesc.se_style).  Every SE branch of the library computes
 *   gate = G(W_e . A(W_r . pool(D) + b_r) + b_e)
 * and without the bit A is the cell's `act` and G the logistic function, as in the reference (models/layers.py:510-523, :550).
 * MobileNetV3's SE has a ReLU hidden layer and a hard-sigmoid gate whatever the block's activation is.  Additive like TFNAS_CELL_K7:
 * without the bit se_style must be 0 (anything else is TFNAS_EINVAL) and every descriptor plans, routes and launches as before.
 * With it:
 *   bits 0-3   hidden activation A: 0 = the cell's act | 1 + TFNAS_ACT_* = that activation (TFNAS_SE_HIDDEN(act)); ReLU6 and
 *              hard-swish need TFNAS_CELL_ACTS as they do in `act`
 *   bits 4-7   gate G: 0 logistic | 1 hard-sigmoid min(max(v + 3, 0), 6) / 6 (TFNAS_SE_GATE_HSIGMOID); its derivative is 1/6 where
 *              0 < gate < 1 and 0 elsewhere, taken from the saved gate itself: no workspace grows
 *   any undefined value of either nibble and any higher bit is TFNAS_EINVAL.
 * One style per cell, as `act` is one per cell: it applies to every SE group of the cell whatever its kind (plain, expand-free,
 * Fused-MBConv, the groups of a TFNAS_CELL_KINDS cell).  A styled cell without SE groups is legal and runs like the unstyled
 * one.  A descriptor that spells the defaults (TFNAS_SE_HIDDEN(act) with the logistic gate) launches the kernels the unstyled one
 * launches.  TFNAS_MODE_CELL only (tfnas_mixedop_*, tfnas_mbconv_*, the path level): TFNAS_MODE_STEM and TFNAS_MODE_HEAD refuse a
 * non-zero style -- the stem keeps the reference's SE.  tfnas_cell_ws, tfnas_cell_route, tfnas_efree_supported and
 * tfnas_fx_supported do not depend on it.  Checked by tfnas_cell_plan and again by every entry point. */
#define TFNAS_CELL_SE_STYLE 0x1000
#define TFNAS_SE_HIDDEN(act) (1 + (act))
#define TFNAS_SE_HIDDEN_MASK 0xf
#define TFNAS_SE_GATE_SHIFT 4
#define TFNAS_SE_GATE_MASK 0xf0
#define TFNAS_SE_GATE_LOGISTIC 0
#define TFNAS_SE_GATE_HSIGMOID (1 << TFNAS_SE_GATE_SHIFT)
#define TFNAS_GROUP_MBCONV 0
#define TFNAS_GROUP_NOEXPAND 1
#define TFNAS_GROUP_FUSED 2
/* TfnasCellDesc.flags: the caller knows the skip (identity) candidate of the MobileNet-family search spaces -- the reference's
 * commented-out 'skip' primitive (models/model_search.py:16,28; models/layers.py:274-319).  Additive like the bits above: without
 * the bit every descriptor is accepted, refused, planned, sized, routed and launched exactly as before (TfnasGroup.kind = 3 stays
 * TFNAS_EINVAL).  With it a group may say TFNAS_GROUP_SKIP in g.kind: the candidate that returns the cell's input.  The cell computes
 *   out = sum_{g computing} wmix[g] BN3_g(project_g(...)) + (sum_{ALL g} wmix[g]) x
 * which is the reference's sum_g w_g op_g(x): every MBConv candidate of a residual cell adds x itself, the identity candidate is x.
 * Backward: dwmix[g] of a computing group as before; dwmix[g] of a skip group = <dout, x> (the per-channel sums the BN3 backward
 * pass forms anyway, added in double in a fixed order); dx gains (sum of ALL wmix[g]) dout, once.  A skip group is not a kind: it
 * has no weights, no BatchNorm site, no columns of the [pixels][M] tensors and no Pr slot.  Rules, checked by tfnas_cell_plan and
 * again by every entry point before any pointer is looked at (TFNAS_EINVAL unless stated):
 *   - TFNAS_CELL_KINDS must be set too; mode == TFNAS_MODE_CELL; has_res == 1 (hence ic == oc, stride == 1);
 *   - a SKIP group has mc == 0, k == 0, se == 0 and every weight and gradient pointer NULL; the plan gives it mcp = 0 and no
 *     columns (M and SE are those of the other groups);
 *   - SKIP groups come after every other group, so wmix[g] / dwmix[g] of the G' = G - nskip computing groups keep their indices;
 *     at least one group computes (G' >= 1: a caller that samples the skip alone launches nothing);
 *   - such a cell is always a mixed cell: it is never folded into the unflagged or one-block form, even when its computing groups
 *     are all plain or there is one.  tfnas_efree_supported and tfnas_fx_supported return 0, tfnas_cell_route returns
 *     TFNAS_ROUTE_TAKEN_VALID, and a plain group needs its E buffer (E == NULL is TFNAS_ENULL): the residual gradient is added
 *     once at the end over all mix weights, which the one-kind routes -- adding it inside their own dgrad kernels -- cannot do;
 *   - a descriptor that carries the bit but has no SKIP group plans, sizes, routes and runs bit for bit like the same descriptor
 *     without the bit;
 *   - tfnas_cell_ws reports, field for field, what the descriptor without its SKIP groups (flags & ~TFNAS_CELL_SKIP, G = G')
 *     reports: Pr, stats3, red3 and the partial rows are sized by G'; wmix and dwmix are the caller's [G];
 *   - tfnas_mbconv_fwd/bwd, tfnas_path_plan, TFNAS_MODE_STEM and TFNAS_MODE_HEAD refuse the bit as they refuse TFNAS_CELL_KINDS.  A
 *     path that says TFNAS_PATH_EXTENDED takes it, and takes a ONE-group descriptor whose group is TFNAS_GROUP_SKIP as the
 *     pass-through cell of a sampled path (below: the path level) -- the per-cell entry points keep refusing that descriptor (a skip
 *     needs a computing group before it).
 * Launch sequence: everything runs on the first G' groups as for any TFNAS_CELL_KINDS cell; four kernels see G -- the forward mix
 * and the residual-gradient pass (the sum of the mix weights), the BN3-backward sums (the <dout, x> accumulator of a residual cell)
 * and the dwmix kernel (one wave per entry).  TFNAS_CELL_ACCUM_WGRAD, dx == NULL, need_wgrad == 0, the dwmix-only early return,
 * wgrad_stream[], the sync-stats hook (table lengths follow G'), se_style, TFNAS_CELL_K7 and TFNAS_CELL_ACTS keep their meaning. */
#define TFNAS_CELL_SKIP 0x2000
#define TFNAS_GROUP_SKIP 3
/* TfnasCellDesc.flags: the caller knows dilated depthwise convolutions (TfnasGroup.dil) -- the dil_conv_3x3 / dil_conv_5x5 candidates
 * of the DARTS-family spaces and the dilated late stages of MobileNet-family backbones: a 3 x 3 with its taps two pixels apart
 * covers 5 x 5 with 9 taps, a 5 x 5 covers 9 x 9 with 25.  Additive like TFNAS_CELL_K7: without the bit TfnasGroup.dil is not read
 * and every descriptor is accepted, refused, planned, sized, routed and launched exactly as before (0x4000 stays undefined and
 * refused).  With the bit a descriptor whose groups all have dil 0 or 1 plans, sizes, routes and launches identically, and a group
 * may have dil == 2 with k 3 or 5: padding 2 * (k / 2), so the output size stays (H - 1) / stride + 1 as for every k.  Rules,
 * checked by tfnas_cell_plan and again by every entry point (TFNAS_EINVAL):
 *   - dil outside {0, 1, 2}; k == 7 with dil == 2; a dilated TFNAS_GROUP_FUSED or TFNAS_GROUP_SKIP group; a dilated TFNAS_CELL_FUSED
 *     cell; a dilated group in TFNAS_MODE_STEM or TFNAS_MODE_HEAD;
 *   - allowed: plain MBConv groups and expand-free groups (TFNAS_CELL_NOEXPAND, or TFNAS_GROUP_NOEXPAND of a TFNAS_CELL_KINDS cell), in
 *     sampled and soft launches of tfnas_mixedop_fwd/bwd, in tfnas_mbconv_fwd/bwd, in tfnas_path_plan and the path level; all four
 *     activations, both strides, SE or none, every se_style.
 * A cell with a dilated group follows the 7 x 7 rule: it always materialises E (tfnas_efree_supported and tfnas_fx_supported return
 * 0, tfnas_cell_route returns TFNAS_ROUTE_TAKEN_VALID), runs every depthwise pass on the LDS tile kernels whatever TFNAS_ROUTE_DW_*
 * asks, and keeps the depthwise weight gradient in a launch of its own.  Dilation changes neither the workspace (tfnas_cell_ws)
 * nor the weight-gradient partial row (sum of mc * k * k) nor any planned word (M, SE, off, mcp, se_off): the weight stays
 * [mc][k * k].  At stride 2 every tap of a dilated group lands on an even input row and column: the odd pixels of its data
 * gradient (dEh; dx of an expand-free group) are exactly zero and are stored as such.  TFNAS_CELL_ACCUM_WGRAD,
 * TFNAS_CELL_LAZY_JOIN, wgrad_stream[], the sync-stats hook and the GEMM modes keep their meaning.  The Python mirror sets the bit
 * for every descriptor that holds a dilated group, and only those (functions.HipModes.apply). */
#define TFNAS_CELL_DILATION 0x8000
/* TfnasCellDesc.flags: the caller knows MixConv groups (Tan & Le, "MixConv: Mixed Depthwise Convolutional Kernels", the MixNet
 * family): ONE depthwise convolution whose channels are split into two or three contiguous segments, segment 0 3 x 3 (or 5 x 5),
 * the next 5 x 5 (or 7 x 7), an optional third 7 x 7; everything else of the block is the ordinary MBConv.  Additive like
 * TFNAS_CELL_K7: without the bit (0x10000; 0x4000 stays undefined and refused, as the dilation bit left it) every descriptor is
 * accepted, refused, planned, sized, routed and launched exactly as before.  With the bit TfnasGroup.k may be a PACKED word: nibble s (bits 4s .. 4s+3) is the
 * kernel size of channel segment s -- two or three non-zero nibbles, strictly ascending, each 3, 5 or 7, everything above zero:
 * 0x53, 0x73, 0x75, 0x753.  A plain k (3, 5, 7) under the bit means what it means without it, and a descriptor that carries the
 * bit but has no packed group plans, sizes, routes and runs bit for bit like the same descriptor without the bit.
 * Segments: q = mcp / 4 channel quads, n segments; segment s gets q / n quads, segment 0 the q % n remaining ones as well;
 * segment s covers channels [4 Q_s, min(4 Q_s+1, mc)).  Where mc is a multiple of 4 n this is MixNet's own _split_channels
 * (equal parts, remainder to the first); for ragged widths the split points stay 16-byte aligned (the kernels' float4 accesses).
 * Weights: w_dw / g_dw point to ONE packed buffer, segment s [mc_s][k_s * k_s] at float offset sum_{t<s} mc_t k_t^2, in all
 * sum_s mc_s k_s^2 floats; the weight-gradient partial row (TFNAS_ERANGE when it does not fit) has exactly this layout.
 * Rules, checked by tfnas_cell_plan and again by every entry point (TFNAS_EINVAL):
 *   - any other packed word; a word with a 7 without TFNAS_CELL_K7; q < n (a segment without a quad); a packed k in a group with
 *     dil == 2, in a TFNAS_GROUP_FUSED or TFNAS_GROUP_SKIP group, in a TFNAS_CELL_FUSED cell, in TFNAS_MODE_STEM or
 *     TFNAS_MODE_HEAD; tfnas_path_plan on a cell with a packed group (unless the path says TFNAS_PATH_EXTENDED);
 *   - allowed: plain MBConv groups and expand-free groups (TFNAS_CELL_NOEXPAND, or TFNAS_GROUP_NOEXPAND of a TFNAS_CELL_KINDS cell), in
 *     sampled and soft launches of tfnas_mixedop_fwd/bwd and in tfnas_mbconv_fwd/bwd; all four activations, both strides, SE or
 *     none, every se_style; a soft cell may hold packed groups beside plain 3 / 5 / 7, dilated, FUSED and SKIP groups.
 * A cell with a packed group follows the 7 x 7 rule: it always materialises E (tfnas_efree_supported and tfnas_fx_supported return
 * 0, tfnas_cell_route returns TFNAS_ROUTE_TAKEN_VALID), runs every depthwise pass on the LDS tile kernels whatever TFNAS_ROUTE_DW_*
 * asks -- each segment in the launch of its own kernel size -- and keeps the depthwise weight gradient in a launch of its own.
 * tfnas_cell_ws and every planned word (M, SE, off, mcp, se_off) are what they are for the same group with a plain k.
 * TFNAS_CELL_ACCUM_WGRAD, TFNAS_CELL_LAZY_JOIN, wgrad_stream[], the sync-stats hook, the GEMM modes, need_wgrad == 0 and
 * dx == NULL keep their meaning.  The Python mirror sets the bit for every descriptor that holds a packed group, and only those
 * (functions.HipModes.apply). */
#define TFNAS_CELL_MIXK 0x10000
/* TfnasCellDesc.route (ABI 4; rounds 2-5 read these from TFNAS_* environment variables latched once per process) */
#define TFNAS_ROUTE_FX_OFF 0x1        /* frozen-weight launches of the 14 x 14 / 7 x 7 cells through the materialised route instead
                                         of the fused per-image kernels (csrc/fx_kernels.hip)                                   */
#define TFNAS_ROUTE_FOLD_OFF 0x2      /* per-image BN2-backward tables in their own pass over (dZ, D) (k_bn2_pool) instead of the
                                         epilogue of k_project_dgrad + k_bn2_gather                                             */
#define TFNAS_ROUTE_DWWG_OFF 0x4      /* 3x3 depthwise weight gradient of the stride-1 ring cells from its own kernel instead of
                                         the backward-data pass                                                                 */
#define TFNAS_ROUTE_DWWG2_OFF 0x8     /* the same for the register-window pass of the stride-2 cells                           */
#define TFNAS_ROUTE_XG_OFF 0x10       /* expand weight gradient never in Gram form                                              */
#define TFNAS_ROUTE_XG_ALL 0x20       /* ... in Gram form wherever the shape allows (default: where E >= 100 MB)                */
#define TFNAS_ROUTE_DW_SHIFT 6        /* 2 bits: 0 per-launch policy, 1 register-window kernels wherever the geometry allows,   */
#define TFNAS_ROUTE_DW_MASK 0xc0      /*         2 LDS ring / tile kernels only, 3 tile kernels only (7 x 7 cells,
                                         TFNAS_ACT_RELU6 / _HSWISH cells, TFNAS_CELL_NOEXPAND cells and cells with a
                                         dilated or a packed group, TFNAS_CELL_DILATION / _MIXK: always 3)                                        */
#define TFNAS_ROUTE_SE_SHIFT 8        /* 2 bits: 0 wave-level MFMA kernels for the excite FCs, 1 one fused per-image kernel,    */
#define TFNAS_ROUTE_SE_MASK 0x300     /*         2 LDS-tiled GEMMs                                                              */
#define TFNAS_ROUTE_WGRAD_INLINE 0x400 /* weight-gradient kernels on the caller's stream (no side stream)                       */
#define TFNAS_ROUTE_GRAM2 0x800       /* BN1-backward correction operator through the round-2 split-K GEMM + reduction instead
                                         of the one-launch k_gram1 (csrc/gemm_kernels.hip)                                      */
#define TFNAS_ROUTE_ALL 0xfff
/* tfnas_cell_route(): TFNAS_ROUTE_TAKEN_VALID | the routes a forward of the (planned) descriptor takes */
#define TFNAS_ROUTE_TAKEN_VALID 0x1
#define TFNAS_ROUTE_TAKEN_FX 0x2      /* fused per-image route: the E buffer holds ehat = BN1(x W1^T) after the forward         */

/* Element counts / offsets of every caller-allocated buffer of one cell. */
typedef struct TfnasCellWs {
    /* forward (saved for backward) */
    uint64_t E;        /* floats  [N*H*W][M]      raw 1x1-expand output (pre-BN)            */
    uint64_t D;        /* floats  [N*Ho*Wo][M]    raw depthwise output (pre-BN)             */
    uint64_t Pr;       /* floats  [G][N*Ho*Wo][oc] raw 1x1-project outputs (pre-BN)         */
    uint64_t fsmall;   /* floats  pooled[N][M] | gate[N][M] | hpre[N][SE]                   */
    uint64_t off_pooled, off_gate, off_hpre;
    uint64_t stats;    /* doubles stats1[M][2] | stats2[M][2] | stats3[G*oc][2]  (sum,sumsq) */
    uint64_t off_stats1, off_stats2, off_stats3;
    uint64_t out;      /* floats  [N*Ho*Wo][oc]                                             */
    /* backward scratch */
    uint64_t dZ;       /* floats  [N*Ho*Wo][M]                                              */
    uint64_t dEh;      /* floats  [N*H*W][M]                                                */
    uint64_t bsmall;   /* floats  dgate[N][M] | dpooled[N][M] | dgl[N][M] | dhpre[N][SE] | cb1[M][4] */
    uint64_t off_dgate, off_dpooled, off_dgl, off_dhpre, off_cb1;
    uint64_t red;      /* doubles red3[G*oc][2] | resdot[oc] | red2[M][2] | red1[M][2]      */
    uint64_t off_red3, off_red2, off_red1, off_resdot;   /* resdot = per-channel <dout, x> of residual cells */
    uint64_t part;     /* floats  scratch for per-workgroup partial sums (fwd and bwd), summed in a fixed order by a second
                          tiny kernel -- no floating-point atomics, deterministic results.  A multiple of tfnas_sizeof(7)
                          floats; the last tfnas_sizeof(8) 4-byte words of every tfnas_sizeof(7)-float piece are reserved.
                          Doubled when d.need_wgrad is set: tfnas_mixedop_bwd runs the weight-gradient kernels on
                          a library-owned side stream (forked from / joined to `stream` inside the call) and gives
                          them the second half.                                                              */
    uint64_t dx;       /* floats  [N*H*W][ic]                                               */
    uint64_t dxp;      /* floats  split-K partial tiles of the expand dgrad (may be tiny); pass NULL to disable */
} TfnasCellWs;

int tfnas_abi_version(void);

/* ---- cross-rank BatchNorm statistics ("sync-stats") -------------------------------------------------------------------------
 * Data-parallel runs normalise with PER-RANK batch statistics by default (what un-synced DDP / nn.DataParallel do; the
 * reference's search is effectively single-GPU).  With a hook installed every BatchNorm site uses the
 * statistics of the GLOBAL batch -- the analogue of apex's convert_syncbn_model in the reference's retrain script
 * (train_eval_amp.py:155-157) -- forward (sum, sum of squares per channel) and backward (the two BatchNorm-backward sums).
 * fn(user, table, ndoubles, stream) is called by every launch sequence right after a table of per-channel sums has been
 * reduced on `stream` and before any consumer of it is enqueued.  It must enqueue, ordered on `stream`, an all-reduce(SUM) of
 * table[0 .. ndoubles) over the ranks followed by a multiplication by 1 / world: the kernels keep dividing by the LOCAL element
 * count, so the scaled sums give exactly the global mean / variance / gradient means.  Returns 0 or an error code (propagated).
 * world: number of ranks (unbiased running-variance correction of the affine path).  fn = NULL: off (the default).
 * Process-global; E-free mode (statistics from the Gram matrix of x) is refused while a hook is installed. */
typedef int (*tfnas_stats_sync_fn)(void *user, double *table, uint64_t ndoubles, void *stream);
int tfnas_set_stats_sync(tfnas_stats_sync_fn fn, void *user, int world);

/* Destroys the library-owned side streams / events (after synchronising them).  Optional; safe to call more than once. */
int tfnas_shutdown(void);

/* sizeof() of the ABI structs, for binding self-checks: which = 0 TfnasGroup, 1 TfnasCellDesc, 2 TfnasCellWs,
 * 3 TfnasStage, 4 TfnasPathDesc, 5 TfnasPathWs, 6 TfnasBnAffine, 9 TfnasOptGroups;  7 = floats of one `part` scratch piece,
 * 8 = reserved words at the end of each piece (TfnasCellWs.part). */
uint64_t tfnas_sizeof(int which);

/* Fill the [plan] fields of a descriptor from its [in] fields.  Returns TFNAS_E* on bad geometry. */
int tfnas_cell_plan(TfnasCellDesc *d);

/* Buffer sizes for a planned descriptor. */
int tfnas_cell_ws(const TfnasCellDesc *d, TfnasCellWs *ws);

/* 1 when the cell can run without the expanded tensor E ("E-free" mode: pass E = NULL to tfnas_mixedop_fwd AND to the
 * matching tfnas_mixedop_bwd; the depthwise kernels then recompute act(BN1(x W_expand^T)) from the narrow cell input,
 * and BN1's batch statistics come from the ic x ic Gram matrix of x).  Currently: TFNAS_MODE_CELL, need_wgrad = 0
 * (the alpha-step: frozen weights), ic in {16, 24, 40}, kernel sizes 3 / 5 without dilation, ReLU / Swish.  Same arithmetic contract as the E path (fp32, <= 1e-3). */
int tfnas_efree_supported(const TfnasCellDesc *d);
/* What a forward of the (planned) descriptor does with the saved buffers -- a pure function of the descriptor (geometry,
 * need_wgrad, route, sync hook): TFNAS_ROUTE_TAKEN_VALID | TFNAS_ROUTE_TAKEN_*.  Callers that plan the backward with a descriptor
 * of their own (other need_wgrad, another sync hook) store it in that descriptor's fwd_route; the backward then refuses
 * (TFNAS_EINVAL) instead of misreading the E buffer.  The Python mirror does this for every launch (functions._cell_forward). */
int tfnas_cell_route(const TfnasCellDesc *d);
/* 1 when an E-free launch of the (planned) cell takes the FUSED PER-IMAGE route (csrc/fx_kernels.hip): stride 1, images of at
 * most 14 x 14 pixels, 64 <= ic <= 192 (a multiple of 16), frozen weights -- the supernet's cells at 14 x 14 and 7 x 7.  One kernel
 * per direction runs expand 1x1 + BN1 + activation + depthwise k x k (models/layers.py:542-552) for a group of whole images x a
 * slice of mid channels; neither E nor its gradient is ever written (the dEh buffer of tfnas_mixedop_bwd is used as scratch for
 * partial sums of dx).  Implies tfnas_efree_supported (so: 0 for a cell with a 7 x 7 group, a dilated group or
 * TFNAS_ACT_RELU6 / _HSWISH). */
int tfnas_fx_supported(const TfnasCellDesc *d);

/* MixedOP forward.
 *   soft mode  (G=8, wmix = device float[8] = gumbel-softmax weights):
 *       out = sum_g wmix[g] * (BN3(project_g(SE_g(act(BN2(dw_g(act(BN1(expand_g(x))))))))) [+ x])
 *       replaces MixedOP.forward soft branch, models/model_search.py:86-91 (line 89)
 *   sampled mode (G=1, wmix = NULL meaning weight 1):
 *       out = m_ops[idx](x);  replaces models/model_search.py:84-85 -> MBInvertedResBlock.forward layers.py:539-561
 * BN everywhere = batch statistics, biased variance, no affine (layers.py:469,498,533). */
int tfnas_mixedop_fwd(const TfnasCellDesc *d, const float *x, const float *wmix,
                      float *E, float *D, float *Pr, float *fsmall, double *stats, float *part,
                      float *out, void *stream);

/* MixedOP backward (what autograd does for the graph above).  Produces dx [N*H*W][ic], dwmix[G]
 * (d loss / d wmix[g]; may be NULL in sampled mode) and, when d->need_wgrad, the g_* weight gradients
 * (overwritten; added to the destinations with TFNAS_CELL_ACCUM_WGRAD).  dZ/dEh/bsmall/red/part are scratch.  dx may be NULL when the input needs
 * no gradient: with need_wgrad == 0 only dwmix is produced (everything else is skipped). */
int tfnas_mixedop_bwd(const TfnasCellDesc *d, const float *x, const float *wmix,
                      const float *E, const float *D, const float *Pr, const float *fsmall,
                      const double *stats, const float *dout,
                      float *dZ, float *dEh, float *bsmall, double *red, float *part, /* then: dx, dxp, dwmix */
                      float *dx, float *dxp, float *dwmix, void *stream);

/* ---- derived-network ("retrain") path: one MBConv block with AFFINE BatchNorm + running statistics + drop-connect ------------
 * Reference: models/model_eval.py:31-244 (Network / NetworkCfg: a chain of MBInvertedResBlock(affine=True), layers.py:431-561),
 * tools/utils.py:77-86 (drop_connect), trained by train_eval.py.  Same kernels as the search cells (G must be 1); the affine
 * transform is folded into the per-channel statistics tables (csrc/bn_affine.hip).
 * BatchNorm site i: 0 = after the 1x1 expand (stem mode: after the 3x3 image conv; head: after the 1x1 feature-mix conv),
 * 1 = after the depthwise conv, 2 = after the 1x1 project.  Channels: mc, mc, oc.
 * gamma == 0 cannot be represented by the fold (|gamma| is clamped to 1e-12, csrc/bn_affine.hip), and the fold is CONDITIONED by
 * |beta / gamma|: consumers subtract m_eff = mu - beta / r_eff in fp32, and the backward forms gamma * sum(d * xhat) as
 * S2y - beta * S1, so results lose about log2 |beta / gamma| bits of fp32 precision by construction.  The tests hold the path to
 * 2e-5 + 1e-4 * max|ref| against float64 for |beta / gamma| <= 10 (tests/test_gpu_affine_f64.py); beyond that the error grows
 * in proportion. */
typedef struct TfnasBnAffine {
    const float *weight[3], *bias[3];          /* gamma / beta (device); NULL = that site has no affine part          */
    float *g_weight[3], *g_bias[3];            /* their gradients, written by the backward when non-NULL               */
    float *running_mean[3], *running_var[3];   /* training: updated with `momentum` (unbiased variance, torch semantics);
                                                  eval: read instead of the batch statistics; NULL: mean 0 / var 1 / no update */
    float momentum;                            /* torch default 0.1                                                    */
    int32_t eval;                              /* 1: normalise with the running statistics (model.eval())              */
} TfnasBnAffine;

/* out = [drop_scale[n] *] BN3(project(SE(act(BN2(dw(act(BN1(expand(x)))))))) [+ x]   with affine BatchNorms.
 * drop_scale: device float[N] = floor(keep + U[0,1)) / keep per image (residual blocks in training) or NULL.
 * Buffers as tfnas_mixedop_fwd (sizes from tfnas_cell_ws); d->G must be 1, wmix is not used. */
int tfnas_mbconv_fwd(const TfnasCellDesc *d, const TfnasBnAffine *bn, const float *drop_scale, const float *x,
                     float *E, float *D, float *Pr, float *fsmall, double *stats, float *part, float *out, void *stream);

/* Backward of tfnas_mbconv_fwd: dx, the block's weight gradients (d->need_wgrad, g_* of the group) and the BatchNorm
 * parameter gradients (bn->g_weight / g_bias).  dout_s: scratch [N*Ho*Wo][oc] floats, only needed with drop_scale.
 * In eval mode (bn->eval) the backward treats the statistics as constants (no batch-statistics terms). */
int tfnas_mbconv_bwd(const TfnasCellDesc *d, const TfnasBnAffine *bn, const float *drop_scale, const float *x,
                     const float *E, const float *D, const float *Pr, const float *fsmall, const double *stats,
                     const float *dout, float *dout_s, float *dZ, float *dEh, float *bsmall, double *red, float *part,
                     float *dx, float *dxp, void *stream);

/* Head with affine BatchNorm (feature_mix_layer of model_eval.py:98 + global pool): site 0 of `bn`. */
int tfnas_head_affine_fwd(const TfnasCellDesc *d, const TfnasBnAffine *bn, const float *x, float *E, double *stats,
                          float *part, float *pooled, void *stream);
int tfnas_head_affine_bwd(const TfnasCellDesc *d, const TfnasBnAffine *bn, const float *x, const float *E,
                          const double *stats, const float *dpooled, float *dEh, float *cb1, double *red, float *part,
                          float *dx, float *dxp, void *stream);

/* Network head (mode TFNAS_MODE_HEAD): pooled[N][mc] = mean over pixels of act(BN(x W_expand^T)).
 * Replaces feature_mix_layer (ConvLayer 1x1 + BN + swish) + AdaptiveAvgPool2d(1), models/model_search.py:299-300.
 * Buffers: E [N*H*W][M], stats doubles [M][2], part = scratch (ws.part floats).
 * g[0].mc must be a multiple of 4 (TFNAS_EINVAL otherwise, here and in every other head entry point): the kernels load and store
 * the [N][mc] rows of pooled / dpooled 16 bytes at a time, and tfnas_cls_ce asks the same of its C. */
int tfnas_head_fwd(const TfnasCellDesc *d, const float *x, float *E, double *stats, float *part, float *pooled,
                   void *stream);
/* Backward of tfnas_head_fwd: dx [N*H*W][ic] and (need_wgrad) g_expand.  dEh [N*H*W][M], cb1 [M][4] floats and
 * red doubles [M][2] are scratch. */
int tfnas_head_bwd(const TfnasCellDesc *d, const float *x, const float *E, const double *stats, const float *dpooled,
                   float *dEh, float *cb1, double *red, float *part, float *dx, float *dxp, void *stream);

/* The head's weight gradient alone (what tfnas_head_bwd does last when need_wgrad is set): g_expand of the group from dEh / E / cb1
 * as tfnas_head_bwd left them.  A leaf of the backward: the weight step calls tfnas_head_bwd with need_wgrad = 0 on a path's stream
 * and this on that path's weight-gradient stream, so that the cells' backward does not queue up behind it.  part: scratch of its
 * own (tfnas_cell_ws().part floats).  The two forms are bit-identical: dx of tfnas_head_bwd does not depend on need_wgrad, and
 * g_expand of this call is what the one-call form stores. */
int tfnas_head_wgrad(const TfnasCellDesc *d, const float *x, const float *E, const float *dEh, const float *cb1, float *part,
                     void *stream);

/* ---- classifier + cross-entropy tail (models/model_search.py:301-303 `self.classifier(x)`; train_search.py:107 nn.CrossEntropyLoss
 * as called at :333, :376-379, :410, and their autograd; train_eval.py:228-293 with CrossEntropyLabelSmooth, :72-85,126) -------------
 * Every route makes TWO launches: one for everything that depends on ONE image, one for everything that sums over images.  Each has
 * a plain form (the weight step's critical chain carries nothing optional) and a form with the optional parts.  pooled [N][C], W
 * [K][C], bias [K] or NULL, target int64 [N]; fixed summation orders, no atomics.
 *
 * The per-image launch.  tfnas_cls_ce:
 *   logits[n][k] = bias[k] + sum_c pooled[n][c] W[k][c];  loss_n[n] = logsumexp_k logits[n] - logits[n][target[n]]
 *   dlogits[n][k] = scale * (softmax(logits[n])[k] - [k == target[n]])   (scale = 1 / N: the mean reduction of CrossEntropyLoss)
 *   dpooled[n][c] = sum_k dlogits[n][k] W[k][c]
 * and a target outside [0, K) contributes nothing (loss_n = 0, zero gradient rows).
 * tfnas_cls_ce_ex = tfnas_cls_ce with a label-smoothing factor eps in [0, 1) (num_classes == K) and the target's rank:
 *   loss_n[n]     = lse - (1 - eps) logits[n][t] - (eps / K) sum_k logits[n][k]            (t = target[n], lse = logsumexp_k logits[n])
 *   dlogits[n][k] = scale * (softmax(logits[n])[k] - (1 - eps) [k == t] - eps / K);   dpooled[n][c] = sum_k dlogits[n][k] W[k][c]
 *   rank[n]       = #{k: logits[n][k] > logits[n][t]} + #{k < t: logits[n][k] == logits[n][t]}
 * so top-1 is rank < 1 and top-5 is rank < 5 without a topk.  TIE RULE: among equal logits the lower class index ranks first (exactly
 * one class has rank 0); torch.topk promises no order among ties, so the two can differ on a row whose target logit is tied.
 * eps == 0 gives logits, loss_n, dlogits and dpooled bit-identical to tfnas_cls_ce.  A target outside [0, K) (compared on all 64
 * bits) is FLAGGED, not skipped: loss_n[n] = NaN, rank[n] = -1, that image's dlogits and dpooled rows are zero, and no load or store
 * is indexed by it.  dlogits == NULL && dpooled == NULL is the forward-only form (validation): the gradient phase and its LDS are
 * skipped; exactly one of them NULL is TFNAS_EINVAL, as is eps outside [0, 1).
 * Limits of both: C % 4 == 0 (else TFNAS_EINVAL), 4 <= C <= 4096, K <= 4096, LDS (C + K + KG * C floats, KG = min(8, K,
 * 1024 / (C / 4)), 0 when forward-only) <= 64 KiB else TFNAS_ERANGE.
 *
 * The summation launch: one workgroup per 4-class x 256-feature tile of dW, and one that sums db, the loss and the counts.
 * tfnas_cls_wgrad, over the npath <= 2 bi-sampling paths of a weight step (npath device pointers each):
 *   dW[k][c] = sum_p sum_n dlogits_p[n][k] pooled_p[n][c];  db[k] = sum_p sum_n dlogits_p[n][k];  loss = loss_scale * sum_p sum_n loss_n_p[n]
 * (overwritten, not accumulated; loss may be NULL: sum further micro-batches with tfnas_add_into).
 * tfnas_cls_wgrad_ex = tfnas_cls_wgrad + the running meter of a search epoch (train_search.py:387-391: objs_w.update(loss_w, n),
 * top1 / top5 of the GUMBEL path's logits), folded into the same launch: same grid, tiles and summation orders, so dW, db and loss
 * are bit-identical to tfnas_cls_wgrad on the same inputs, with or without a meter.
 *   rank0  int32 [N]: rank[] of path 0 as tfnas_cls_ce_ex wrote it for the launch that produced dlogits[0] / loss_n[0].  Read only
 *     when meter is given; meter == NULL makes the call equal tfnas_cls_wgrad.
 *   meter[0] += sum_p sum_n loss_n_p[n]   (ALL npath paths: N * (loss_g + loss_r) of the mean-reduced losses); the counts are path 0's.
 * TFNAS_ENULL: meter without rank0, or a missing array, path pointer, dW or db; TFNAS_ERANGE: npath outside 1..2, N, C or K < 1.
 * tfnas_cls_reduce, over the N images of ONE path, for a backward pass under any upstream gradient:
 *   dW[k][c] (=|+=) g * sum_n dlogits[n][k] pooled[n][c];   db[k] (=|+=) g * sum_n dlogits[n][k]
 *   g = *gscale, a DEVICE scalar -- the upstream d loss of a backward pass, no host read -- or 1 when gscale is NULL;
 *   accumulate = 1 adds to what dW / db hold, 0 overwrites.  dW == NULL && db == NULL: metrics only (pooled / dlogits unused, one
 *   workgroup).  With gscale == NULL and accumulate == 0 dW and db are bit-identical to tfnas_cls_wgrad_ex(npath = 1).
 *   out[4]   = {mean loss_n, #(rank < 1), #(rank < 5), #(rank < 0: invalid targets)} as floats (NULL: not wanted)
 * TFNAS_ENULL: loss_n / rank missing, only some of (dW, db, pooled, dlogits) given, or no destination at all; C, K <= 4096.
 *
 * The meter of both _ex summation forms, 5 doubles on the device (NULL: none):
 *   meter[5] += {sum loss_n, #(0 <= rank < 1), #(0 <= rank < 5), N, #(rank < 0)}, i.e. meter[0] .. meter[4], in double,
 * added by one thread in that order with ordinary loads and stores, no atomics: launches that share a meter must be
 * ordered by their stream; the host zeroes it and reads it, e.g. once per epoch.  An invalid target carries over from the per-image
 * launch: tfnas_cls_ce_ex gives loss_n = NaN for it, so meter[0] (and loss / out[0]) become NaN while meter[4] counts it;
 * tfnas_cls_ce gives 0, so a path computed by it contributes nothing. */
int tfnas_cls_ce(int N, int C, int K, const float *pooled, const float *W, const float *bias, const int64_t *target, float scale,
                 float *logits, float *loss_n, float *dlogits, float *dpooled, void *stream);
int tfnas_cls_ce_ex(int N, int C, int K, const float *pooled, const float *W, const float *bias, const int64_t *target, float scale,
                    float eps, float *logits, float *loss_n, int32_t *rank, float *dlogits, float *dpooled, void *stream);
int tfnas_cls_wgrad(int npath, int N, int C, int K, const float *const *pooled, const float *const *dlogits,
                    const float *const *loss_n, float loss_scale, float *dW, float *db, float *loss, void *stream);
int tfnas_cls_wgrad_ex(int npath, int N, int C, int K, const float *const *pooled, const float *const *dlogits,
                       const float *const *loss_n, const int32_t *rank0, float loss_scale, float *dW, float *db, float *loss,
                       double *meter, void *stream);
int tfnas_cls_reduce(int N, int C, int K, const float *pooled, const float *dlogits, const float *loss_n, const int32_t *rank,
                     const float *gscale, int accumulate, float *dW, float *db, float *out, double *meter, void *stream);
/* dst[i] += src[i], count floats (a multiple of 4): the second path's share of a shared parameter's gradient. */
int tfnas_add_into(float *dst, const float *src, uint64_t count, void *stream);

/* Gumbel-softmax over the candidates of `ncell` cells in one launch + expected cell latency.
 *   w[c][i] = softmax_i((log_alpha[c][i] - log(e[c][i])) / T)      (F.gumbel_softmax, model_search.py:87)
 *   cell_lat[c] = sum_i w[c][i] * lat[c][i]                          (model_search.py:90)
 * log_alpha: `ncell` device pointers (each float[8]) -- the reference keeps one nn.Parameter per cell.
 * e: Exp(1) draws, lat: looked-up latencies (model_search.py:93-111), both device float[ncell][8]. */
int tfnas_arch_fwd(int ncell, const float *const *log_alpha, const float *e, const float *lat, float T,
                   float *w, float *cell_lat, void *stream);

/* Backward of tfnas_arch_fwd: dla[c][j] = (1/T) w_j (gt_j - sum_i gt_i w_i), gt_i = dw[c][i] + dlat[c]*lat[c][i].
 * dlog_alpha: `ncell` device pointers receiving float[8] each. */
int tfnas_arch_bwd(int ncell, const float *w, const float *lat, const float *dw, const float *dcell_lat,
                   float T, float *const *dlog_alpha, void *stream);

/* Sampled-mode index selection for `ncell` cells (model_search.py:59-81):
 *   mode 0 'gumbel'/'gumbel_2': pos = argmax gumbel_softmax(log_softmax(log_alpha[mask]), T)
 *   mode 1 'min_alphas', mode 2 'max_alphas': argmin / argmax of log_alpha[mask]
 * mask: device uint8[ncell][8] (the `switches`); pos_out: device int32[ncell] = position among the
 * switched-on candidates (the caller maps it like fink_ori_idx, model_search.py:49-56). */
int tfnas_arch_sample(int ncell, const float *const *log_alpha, const uint8_t *mask, const float *e, float T,
                      int mode, int32_t *pos_out, void *stream);

/* Projection of the architecture parameters after the Adam step (train_search.py:421-422):
 *   p <- log_softmax(p) in place, for n 1-D fp32 device tensors of len[i] <= 8 elements each (log_alphas and betas),
 * one launch for all of them.  p: n device pointers (host array), len: host int32[n]. */
int tfnas_arch_project(int n, float *const *p, const int32_t *len, void *stream);

/* Sink-connecting stage output (MixedStage.forward tail, models/model_search.py:202-204):
 *   bw = softmax(betas[K]);  out = sum_k bw[k]*res[k];  out_lat = sum_k bw[k]*(cell_lat[0]+..+cell_lat[k])
 * res: K device pointers to [count] floats each; cell_lat: device float[K] or NULL (sampled mode: lat 0).
 * bw_out: device float[K] (saved for backward). */
int tfnas_sink_fwd(int K, const float *betas, const float *const *res, const float *cell_lat,
                   uint64_t count, float *out, float *out_lat, float *bw_out, void *stream);

/* Backward of tfnas_sink_fwd: dres[k] = bw[k]*dout; dbetas via the softmax Jacobian of
 * (<dout,res[k]> + dlat*cum_k); dcell_lat[j] = dlat * sum_{k>=j} bw[k].  dot_scratch: device double[K]. */
int tfnas_sink_bwd(int K, const float *bw, const float *const *res, const float *cell_lat, const float *dout,
                   const float *dlat, uint64_t count, float *const *dres, float *dbetas, float *dcell_lat,
                   double *dot_scratch, void *stream);

/* ================================================================================================================
 * Path level: a whole chain of MixedOP cells + the sink-connecting stage mixes of a Network in ONE call per direction.
 *
 * Replaces the body of Network.forward between the stems and the head (models/model_search.py:285-297: six
 * MixedStage.forward calls, :157-206) and its autograd backward, for one "path":
 *   sampled mode  (every cell G = 1)  -- one of the two bi-sampling paths of train_w_arch's weight step
 *                                        (train_search.py:375-379) or train_wo_arch's / validate's single path;
 *   soft mode     (every cell G = 8)  -- the architecture step (train_search.py:409-413).
 * The per-cell entry points above stay (they are what MixedOP.forward calls when a user drives the modules one by one);
 * the path entry points exist because the per-cell route costs one Python/autograd round trip, ~10 tensor allocations
 * and ~25 launches *per cell*, and the weight step then spends a third of its wall time waiting for the host.
 * Differences to 18 x tfnas_mixedop_fwd/bwd + 6 x tfnas_sink_fwd/bwd (same kernels otherwise, bit-identical results):
 *   - all buffers come from ONE caller-allocated arena (sizes from tfnas_path_plan);
 *   - the sink gradient bw[k]*dsink is added in the dx epilogue of the following cell instead of K scaled copies per
 *     stage and one elementwise add per block;
 *   - weight-gradient kernels run on a side stream and may lag ONE cell behind the data-gradient chain (the per-cell
 *     entry joins at the end of every cell);
 *   - several paths (the two bi-sampling paths) are enqueued interleaved, cell by cell, on their own streams.
 * ================================================================================================================ */
#define TFNAS_MAX_STAGES 8
/* TfnasPathDesc.path_flags: the caller knows the cells beside the plain ones -- the other kinds, cells of several kinds, skip and
 * packed groups, the pass-through cell (tfnas_path_plan).  Without the bit such a path is TFNAS_EINVAL, as it always was. */
#define TFNAS_PATH_EXTENDED 0x1

typedef struct TfnasStage {
    int32_t ncell;          /* MixedOP blocks of this stage (model_search.py:126-155: 2,3,4,4,4,1)            [in] */
    int32_t start_res;      /* 0: the stage input is itself a depth choice (ic==oc && stride==1), else 1      [in] */
    int32_t first_cell;     /* index of the stage's first cell in TfnasPathDesc.cell                          [plan] */
    int32_t nres;           /* ncell + 1 - start_res = len(betas)                                            [plan] */
    const float *betas;     /* device float[nres]                                                            [in] */
    float *dbetas;          /* device float[nres] or NULL (architecture parameters frozen: weight step)       [in] */
} TfnasStage;

typedef struct TfnasPathDesc {
    int32_t ncell, nstage;
    int32_t soft;           /* 1: cells carry G = 8 groups, wmix/cell_lat are consumed and d wmix / d cell_lat produced */
    int32_t need_dx0;       /* backward produces the gradient of the path input                               */
    int32_t efree_mask_lo;  /* bit c set: cell c runs E-free (E never materialised; needs tfnas_efree_supported) */
    int32_t path_flags;     /* 0 or TFNAS_PATH_EXTENDED; any other bit: TFNAS_EINVAL (ABI 1: dual; then a word that had to be 0) */
    TfnasStage stage[TFNAS_MAX_STAGES];
    TfnasCellDesc cell[TFNAS_MAX_CELLS];   /* [in] fields + weight / gradient pointers bound; N, H, W chained by plan */
} TfnasPathDesc;

/* Arena requirement of a planned path, in floats (the arena must be 256-byte aligned). */
typedef struct TfnasPathWs {
    uint64_t saved;         /* forward results kept for backward (E, D, Pr, small tensors, statistics, cell / stage outputs) */
    uint64_t scratch;       /* forward + backward scratch (partials, dZ, dEh, gradient ring)                  */
    uint64_t total;         /* saved + scratch                                                                */
    uint64_t out_count;     /* elements of the path output [N][Ho][Wo][oc] of the last stage */
    int32_t out_h, out_w, out_c, pad;
} TfnasPathWs;

/* Opaque path context: the planned descriptor, arena offsets, one library-owned side stream and the events that order
 * it against the caller's stream.  One context per concurrently running path. */
int tfnas_path_create(void **ctx);
int tfnas_path_destroy(void *ctx);
/* Use `stream` (owned by the caller, must outlive the context) for the weight-gradient kernels instead of a stream the library
 * creates.  HIP maps streams onto a few hardware queues in creation order; a caller that has measured which of its streams
 * really run concurrently (tfnas_amd/streams.py) hands the good ones in here. */
int tfnas_path_set_side_stream(void *ctx, void *stream);
/* Validate + plan every cell (tfnas_cell_plan), chain the geometry (cell i+1's input extent = cell i's output), lay out
 * the arena.  May be called again on the same context with different candidates / widths (every weight step does).
 * Cells: plain TFNAS_MODE_CELL descriptors (dilated groups included); anything below is TFNAS_EINVAL in a path without
 * TFNAS_PATH_EXTENDED, as it always was.  With the bit: TFNAS_MODE_CELL descriptors of every kind -- plain, TFNAS_CELL_NOEXPAND, TFNAS_CELL_FUSED, TFNAS_CELL_KINDS with or without
 * TFNAS_CELL_SKIP groups, packed (TFNAS_CELL_MIXK) and dilated groups: the rules of tfnas_cell_plan are the rules.  A sampled path
 * (soft == 0) keeps G == 1 in every cell.  The E slot of the arena is laid out for the cells that have an E; an efree_mask_lo bit
 * is legal only where tfnas_efree_supported says so (plain cells), TFNAS_EINVAL elsewhere.  The sink-connecting gradient
 * dx += bw[k] * dsink of a cell whose input is a depth choice is the LAST term of dx on every tail: in the epilogue of the expand
 * dgrad (plain cells), in one pass over dx behind the depthwise backward-data pass / the dense dgrad / the residual pass (the
 * other kinds, cells of several kinds), each product rounded on its own.
 * The pass-through cell -- a sampled skip: flags = TFNAS_CELL_KINDS | TFNAS_CELL_SKIP (| TFNAS_CELL_ACCUM_WGRAD, ignored), G == 1,
 * g[0].kind == TFNAS_GROUP_SKIP and nothing else in the group, ic == oc, stride 1, in a sampled path only (anything else:
 * TFNAS_EINVAL).  It is planned here, never by tfnas_cell_plan; it owns no workspace; its output IS its input (the stage's sink
 * and the next cell read the tensor it was handed); forward: no launch; backward: one launch for a whole run of such cells,
 * dx = dout + (bw[a] dsink + bw[a+1] dsink + ...) over the sink slots the tensor fills, the shares summed in slot order; no
 * weight-gradient fork, no event. */
int tfnas_path_plan(void *ctx, const TfnasPathDesc *pd, TfnasPathWs *ws);
/* Set (bit c of cell_mask = 1) or clear TFNAS_CELL_ACCUM_WGRAD on planned cell c of the context, without re-planning: the arena
 * and every offset stay where they are, so a caller may decide between a forward and its backward whether that backward
 * overwrites or accumulates the cells' weight gradients.  TFNAS_EINVAL before the first tfnas_path_plan; TFNAS_ERANGE when
 * a bit at or above ncell is set.  The next tfnas_path_plan takes the flags from its descriptor again. */
int tfnas_path_set_wgrad_accum(void *ctx, uint32_t cell_mask);

/* Forward of `npath` planned paths, enqueued interleaved cell by cell: path p runs on streams[p] with arena[p].
 *   x0[p]     device [N][H][W][ic0] input of the first cell (second_stem output)
 *   wmix[p]   soft mode: device float[ncell][8] gumbel-softmax weights (tfnas_arch_fwd); NULL in sampled mode
 *   cell_lat[p] soft mode: device float[ncell] expected cell latencies; NULL otherwise
 *   out[p]    device [out_count] = last stage's sink output;  out_lat[p]: device float[nstage] per-stage expected latency
 *             (soft mode; NULL otherwise). */
int tfnas_paths_fwd(int npath, void *const *ctx, const float *const *x0, const float *const *wmix,
                    const float *const *cell_lat, float *const *arena, float *const *out, float *const *out_lat,
                    void *const *streams);

/* Backward of the same.  dout[p]: gradient of out[p];  dout_lat[p]: device float[nstage] or NULL;
 * produces dx0[p] (if need_dx0), dwmix[p] float[ncell][8] and dcell_lat[p] float[ncell] (soft mode), stage dbetas, and the
 * cells' weight gradients at the g_* pointers of the planned descriptors (need_wgrad cells).
 * On return every path's side stream has been joined to its stream, also on an error return.
 * The context remembers the route word (tfnas_cell_route) of every cell's last tfnas_paths_fwd; a cell whose backward would take
 * another route (the process-default GEMM mode or the statistics hook changed in between) returns TFNAS_EINVAL before it launches.
 * stage_begin / stage_end: walk only the stages [stage_begin, stage_end) (in reverse order; stage_end = -1: to the last one).
 * A backward may be issued as consecutive segments, last stages first -- (k, -1) then (0, k) -- so that the caller can start
 * reducing the late stages' weight gradients (89 % of the parameters) across ranks while the early stages are still running. */
int tfnas_paths_bwd(int npath, void *const *ctx, const float *const *x0, const float *const *wmix,
                    const float *const *cell_lat, float *const *arena, const float *const *dout,
                    const float *const *dout_lat, float *const *dx0, float *const *dwmix, float *const *dcell_lat,
                    void *const *streams, int stage_begin, int stage_end);

/* ---- fused optimizer steps ------------------------------------------------------------------
 * Weight step tail, train_search.py:381-385: clip_grad_norm_(weight_parameters, max_norm) then SGD(momentum, weight decay,
 * dampening 0) on the parameters that received a gradient.  w / g / m: flat fp32 arenas with identical layout (weights,
 * gradients, momentum); (off[i], len[i]) i < nranges <= 64: the float ranges to update (multiples of 4; typically one per
 * sampled candidate).  total = ||g over all ranges|| * grad_scale (grad_scale = 1 / world_size after a SUM all-reduce);
 * g <- g * grad_scale * min(1, max_norm / (total + 1e-6));  m <- momentum*m + (g + wd*w);  w <- w - lr*m.
 * max_norm <= 0 disables clipping.  scratch: device doubles, >= sum ceil(len/8192).  norm_out: device float or NULL.
 * goff: NULL (gradients at the same offsets as the weights) or the offsets of the ranges inside `g` when `g` is the packed
 * all-reduce message built by tfnas_pack_ranges.  Two launches, no atomics, deterministic.
 * The ranges must be disjoint -- (off[i], len[i]) among themselves and, with goff, (goff[i], len[i]) among themselves:
 * overlapping ranges return TFNAS_EINVAL before anything is launched. */
int tfnas_sgd_clip_step(float *w, float *g, float *m, int nranges, const uint64_t *off, const uint64_t *goff, const uint64_t *len,
                        float max_norm, float lr, float momentum, float wd, float grad_scale, double *scratch,
                        uint64_t scratch_doubles, float *norm_out, void *stream);

/* The same step with an exponential moving average of the weights kept in the pass that stores them (the retrain path: the
 * MobileNetV3 / MixNet / EfficientNet / FBNet recipes report the EMA's accuracy).  ema: a fourth arena with the layout of w;
 * ema_alpha = 1 - decay, the step weight itself (so that 1 - 0.9999 is never formed in fp32).  Launches, norm, clip and SGD update
 * are those of tfnas_sgd_clip_step, bit for bit; where w' is stored, ema <- fma(ema_alpha, w' - ema, ema) is stored too.  Two
 * launches, no atomics, deterministic.  Refused before anything is launched: ema NULL (TFNAS_ENULL); ema_alpha outside [0, 1] or
 * not finite (TFNAS_EINVAL); ema == w, g or m (TFNAS_EINVAL); and everything tfnas_sgd_clip_step refuses. */
int tfnas_sgd_clip_ema_step(float *w, float *g, float *m, int nranges, const uint64_t *off, const uint64_t *goff,
                            const uint64_t *len, float max_norm, float lr, float momentum, float wd, float grad_scale, float *ema,
                            float ema_alpha, double *scratch, uint64_t scratch_doubles, float *norm_out, void *stream);

/* ema[off[i] .. +len[i]) <- fma(ema_alpha, src[same] - ema[same], ema[same]) for nranges <= 64 disjoint ranges (multiples of 4) of
 * two buffers with one layout, in one launch: the EMA formula above on its own -- for the BatchNorm running statistics, which no
 * optimizer pass touches, and for the weights after a step that torch's optimizer made.  src is only read.  Refused before the
 * launch: a NULL pointer (TFNAS_ENULL); ema_alpha outside [0, 1] or not finite, ema == src, overlapping or misaligned ranges
 * (TFNAS_EINVAL); nranges outside [1, 64] (TFNAS_ERANGE). */
int tfnas_ema_lerp(float *ema, const float *src, int nranges, const uint64_t *off, const uint64_t *len, float ema_alpha,
                   void *stream);

/* ---- retrain step tail for parameter groups, Nesterov SGD and RMSprop ---------------------------------------------------
 * What the published MobileNetV3 / MixNet / EfficientNet / FBNet recipes train with: no weight decay on BatchNorm gamma / beta
 * and on biases (two parameter groups), and Nesterov SGD or RMSprop, torch's form or TensorFlow's.  w / g / m / v / ema: flat fp32
 * arenas of `total` floats with one layout (weights, gradients, momentum, squared-gradient average, weight EMA); total is a
 * multiple of 64 because every arena slot is padded to 64 floats.  A group's parameters are not contiguous in the arena, so the
 * groups are not ranges: gmap holds ONE byte per 64-float block of the arena (total / 64 bytes of device memory, built once per
 * arena by the caller), the group id of that block.  Block b is updated with lr[gmap[b]] and wd[gmap[b]]; momentum, alpha, eps
 * and the flags are one value per call.  A map byte >= ngroups means "leave this block alone": nothing of w, m, v or ema in it
 * is stored (its gradient is still scaled, and still counts in the norm).
 *
 *   total_norm = ||g[0, total)|| * grad_scale;  coef = min(1, max_norm / (total_norm + 1e-6))  (max_norm <= 0: coef = 1)
 *   g' = g * grad_scale * coef   (stored back, as after clip_grad_norm_);   d = g' + wd_k * w
 *   TFNAS_OPT_SGD         m' = momentum * m + d;   w' = w - lr_k * m'                 (torch.optim.SGD, dampening 0)
 *     | TFNAS_OPT_NESTEROV                         w' = w - lr_k * (d + momentum * m')
 *   TFNAS_OPT_RMSPROP     v' = alpha * v + (1 - alpha) * d^2;   u = d / (sqrt(v') + eps)   (torch.optim.RMSprop, not centered)
 *                         momentum > 0:  m' = momentum * m + u;  w' = w - lr_k * m'
 *                         momentum == 0: w' = w - lr_k * u       (m is neither read nor written)
 *   TFNAS_OPT_RMSPROP_TF  v' = v + (1 - alpha) * (d^2 - v);   m' = momentum * m + lr_k * d / sqrt(v' + eps);   w' = w - m'
 *                         (TensorFlow's form: eps inside the root, the rate inside the momentum)
 *   ema != NULL:          ema' = fma(ema_alpha, w' - ema, ema), stored where w' is stored (ema_alpha = 1 - decay, the step weight)
 *
 * The square root and the division are the correctly rounded fp32 ones.  The gaps between the slots (zero in every arena) stay
 * zero under every kind -- which is why eps <= 0 is refused for RMSprop: 0 / (sqrt(0) + 0) would put a NaN there.  Two launches
 * (the squared-norm pass of tfnas_sgd_clip_step over [0, total), then the update), no atomics, deterministic.  scratch: device
 * doubles, >= ceil(total / 8192).  norm_out: device float or NULL.
 * Refused before anything is launched: d, w, g, m, gmap or scratch NULL, v NULL for an RMSprop kind (TFNAS_ENULL); total 0 or
 * not a multiple of 64; an unknown kind or flag bit (TFNAS_OPT_NESTEROV with a kind other than TFNAS_OPT_SGD included); a
 * non-finite lr[k] / wd[k] (k < ngroups), momentum, alpha, eps, max_norm or grad_scale; alpha outside [0, 1] or eps <= 0 for an
 * RMSprop kind; momentum < 0, or <= 0 with Nesterov; with ema: ema_alpha outside [0, 1] or not finite, ema == w, g, m or v
 * (TFNAS_EINVAL); ngroups outside [1, 8]; scratch_doubles too small (TFNAS_ERANGE). */
#define TFNAS_OPT_MAX_GROUPS 8
#define TFNAS_OPT_SGD 0
#define TFNAS_OPT_RMSPROP 1
#define TFNAS_OPT_RMSPROP_TF 2
#define TFNAS_OPT_NESTEROV 1    /* TfnasOptGroups.flags */

typedef struct TfnasOptGroups {
    int32_t kind;       /* TFNAS_OPT_SGD / _RMSPROP / _RMSPROP_TF */
    int32_t flags;      /* 0 or TFNAS_OPT_NESTEROV */
    int32_t ngroups;    /* 1 .. TFNAS_OPT_MAX_GROUPS */
    float lr[TFNAS_OPT_MAX_GROUPS];
    float wd[TFNAS_OPT_MAX_GROUPS];
    float momentum;
    float alpha;        /* RMSprop: decay of the squared-gradient average (not read by TFNAS_OPT_SGD) */
    float eps;          /* RMSprop (not read by TFNAS_OPT_SGD) */
    float max_norm;
    float grad_scale;
    float ema_alpha;    /* read only with ema != NULL */
} TfnasOptGroups;       /* tfnas_sizeof(9) */

int tfnas_opt_groups_step(const TfnasOptGroups *d, float *w, float *g, float *m, float *v, float *ema, const uint8_t *gmap,
                          uint64_t total, double *scratch, uint64_t scratch_doubles, float *norm_out, void *stream);

/* dst[doff[i] .. +len[i]) = src[off[i] .. +len[i]) for nranges <= 64 ranges (one launch): gathers the sampled candidates'
 * gradient ranges into ONE contiguous buffer = one RCCL all-reduce message (no torch.cat, no copy back: the SGD step reads
 * the reduced message through `goff`).  The ranges must be disjoint, in src and in dst: overlapping (off[i], len[i]) or
 * (doff[i], len[i]) return TFNAS_EINVAL before anything is launched. */
int tfnas_pack_ranges(const float *src, float *dst, int nranges, const uint64_t *off, const uint64_t *doff,
                      const uint64_t *len, void *stream);

/* Architecture step tail, train_search.py:414-422: clip_grad_norm_(arch_parameters, max_norm), Adam (torch semantics:
 * weight decay added to the gradient, bias correction with `step` >= 1, eps outside the square root) and the projection
 * p <- log_softmax(p), for n <= 32 parameters of len[i] <= 8 floats, in ONE launch.  p / g: host arrays of n device pointers;
 * m / v: device float[n][8] Adam moments (row i, first len[i] entries). */
int tfnas_arch_adam_project(int n, float *const *p, const float *const *g, const int32_t *len, float *m, float *v,
                            float max_norm, float lr, float beta1, float beta2, float eps, float wd, int step,
                            float grad_scale, float *norm_out, void *stream);

/* ---- lazy join of the weight-gradient side stream (derived-network training step) ------------------------------------------
 * tfnas_mixedop_bwd / tfnas_mbconv_bwd run their weight-gradient kernels on a library-owned side stream per caller stream and
 * join it before they return.  With tfnas_set_lazy_join(1), tfnas_mbconv_bwd returns WITHOUT joining: the weight gradients of a
 * block then overlap with the data-gradient chain of the blocks below it.  The caller must (1) keep every buffer passed to the
 * call alive until the side stream is done with it (PyTorch: tensor.record_stream on tfnas_side_stream(stream)), and
 * (2) call tfnas_side_join(stream) before anything on `stream` reads the weight gradients (the optimizer step).
 * (train_eval.py:228-252 has no such notion: one stream; this is scheduling only, the results are bit-identical.) */
int tfnas_set_lazy_join(int on);
int tfnas_side_stream(void *stream, void **side);   /* *side = the library-owned side stream paired with `stream` (created on first use) */
int tfnas_side_join(void *stream);

/* ---- arithmetic of the 1x1-convolution GEMMs --------------------------------------------------------------------------------
 * The reference runs its pointwise convolutions in fp32 (models/layers.py:463-478, 528-534; the search is never AMP).  gfx950
 * executes fp32 MFMA at 1/16 of its bf16 MFMA rate, so the row-tiled GEMMs (expand / project forward and data gradients) split
 * every fp32 operand EXACTLY into three bf16 planes and accumulate the six products that matter in fp32 (csrc/gemm_x3.h):
 *   TFNAS_GEMM_X3   (6, default)  six bf16 MFMAs per element pair, error <= 2^-23 |a||b| per product: fp32-level accuracy
 *   TFNAS_GEMM_F32  (0)           v_mfma_f32_16x16x4_f32, bit-identical to an fmaf chain
 *   TFNAS_GEMM_X2   (3)           three products (error ~2^-16)
 *   TFNAS_GEMM_BF16 (1)           plain bf16 operands, fp32 accumulation (the reduced-precision mode of the derived network's
 *                                 training step; train_eval_amp.py:176-180 in the reference)
 * Process-wide default (TFNAS_GEMM_X3 until set; the library reads no environment variable -- the Python mirror passes TFNAS_GEMM =
 * x3 | f32 | x2 | bf16 on to this call when it loads the library); a descriptor's own gemm_mode wins.  Returns TFNAS_EINVAL for
 * any other mode.  tfnas_gemm_mode() returns the current one. */
#define TFNAS_GEMM_F32 0
#define TFNAS_GEMM_BF16 1
#define TFNAS_GEMM_X2 3
#define TFNAS_GEMM_X3 6
/* OR-ed into the mode: every row-tiled GEMM launch uses it.  Without the flag the library keeps the fp32 loop where the split
 * loop measured slower (the data-gradient GEMMs of one-candidate launches and of the large images). */
#define TFNAS_GEMM_EVERYWHERE 0x100
int tfnas_set_gemm_mode(int mode);
int tfnas_gemm_mode(void);

/* ---- optional diagnostics (used by bench.py for the `roofline` object) --------------------------------------
 * Per-kernel-family timing with HIP events recorded on the launch stream.  tfnas_prof_enable(mask) turns the
 * families whose bit is set on (0 = off, the default); tfnas_prof_collect() waits for the recorded events of
 * one family, returns their count and summed duration in ms, and clears them.  Not re-entrant. */
int tfnas_prof_enable(unsigned mask);
int tfnas_prof_count(void);
const char *tfnas_prof_name(int id);
int tfnas_prof_collect(int id, uint64_t *launches, double *total_ms);
/* of the launches the LAST tfnas_prof_collect(id) returned: those that covered all candidates of a cell (alpha-step launches of
 * the depthwise families), count and summed ms -- the same kernels run at two very different sizes in the two step kinds */
int tfnas_prof_last_split(int id, uint64_t *soft_launches, double *soft_ms);

#ifdef __cplusplus
}
#endif
#endif /* TFNAS_HIP_H */
