// Internal launcher prototypes (one per kernel family); the extern "C" surface is in capi.hip.
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include "tfnas_hip.h"

// cross-rank BatchNorm statistics hook (tfnas_set_stats_sync, capi.hip)
struct StatsSync {
    tfnas_stats_sync_fn fn;
    void* user;
    int world;
};
extern StatsSync g_stats_sync;              // the process default (tfnas_set_stats_sync); a descriptor's own hook wins
static inline StatsSync sync_of(const TfnasCellDesc& d) {
    if (d.sync_fn) return StatsSync{d.sync_fn, d.sync_user, d.sync_world > 0 ? d.sync_world : 1};
    return g_stats_sync;
}
static inline bool stats_sync_on(const TfnasCellDesc& d) { return sync_of(d).fn != nullptr; }
static inline int stats_sync(const TfnasCellDesc& d, double* table, size_t ndoubles, hipStream_t s) {
    const StatsSync y = sync_of(d);
    return y.fn ? y.fn(y.user, table, (uint64_t)ndoubles, (void*)s) : 0;
}
static inline uint64_t stats_world(const TfnasCellDesc& d) {
    const StatsSync y = sync_of(d);
    return (y.fn && y.world > 1) ? (uint64_t)y.world : 1;
}

// route switches of a launch (TfnasCellDesc.route, tfnas_hip.h: TFNAS_ROUTE_*); 0 = the library's measured per-launch policy
static inline int route_dw(const TfnasCellDesc& d) { return (d.route & TFNAS_ROUTE_DW_MASK) >> TFNAS_ROUTE_DW_SHIFT; }   // 0 auto, 1 direct, 2 lds, 3 tiled
static inline int route_se(const TfnasCellDesc& d) { return (d.route & TFNAS_ROUTE_SE_MASK) >> TFNAS_ROUTE_SE_SHIFT; }   // 0 wave, 1 fused, 2 gemm
static inline bool route_side(const TfnasCellDesc& d) { return !(d.route & TFNAS_ROUTE_WGRAD_INLINE); }
// TFNAS_CELL_ACCUM_WGRAD: every weight-gradient store of the launch adds to its destination (g <- g + v)
static inline int wgrad_accum(const TfnasCellDesc& d) { return (d.flags & TFNAS_CELL_ACCUM_WGRAD) ? 1 : 0; }
// TFNAS_ACT_RELU6 / TFNAS_ACT_HSWISH: the kernel families built for ReLU and Swish only (ring, register-window, E-free, fused
// per-image, the FOLD epilogue of the project dgrad) are never planned for such a cell and refuse it if asked
static constexpr bool act_tile_only(int act) { return act == TFNAS_ACT_RELU6 || act == TFNAS_ACT_HSWISH; }
// TFNAS_CELL_NOEXPAND: a block without expand convolution (G = 1, mc == ic).  D = dw(x) on the raw cell input: no E, no BatchNorm
// site 0, the depthwise passes on the raw-input form of the LDS tile kernels, dx from the depthwise backward-data pass itself
static inline bool cell_noexpand(const TfnasCellDesc& d) { return (d.flags & TFNAS_CELL_NOEXPAND) != 0; }
// TFNAS_CELL_FUSED: a Fused-MBConv block (G = 1, k = 3): D = conv3x3(x) with the dense OIHW weight in w_expand, no depthwise
// weight, no E, no BatchNorm site 0; the three implicit GEMMs of conv_kernels.hip stand where the depthwise passes stand
static inline bool cell_fused(const TfnasCellDesc& d) { return (d.flags & TFNAS_CELL_FUSED) != 0; }
// The kind of a cell, decided once per function that forks on it (the table's Python twin: tfnas_amd/_lib.py, BlockKind).  A
// descriptor with both bits is refused by every entry point (capi.hip: check_kind) before anything asks.
enum CellKind { TFNAS_KIND_MBCONV, TFNAS_KIND_NOEXPAND, TFNAS_KIND_FUSED };
static inline CellKind cell_kind(const TfnasCellDesc& d) {
    return cell_fused(d) ? TFNAS_KIND_FUSED : cell_noexpand(d) ? TFNAS_KIND_NOEXPAND : TFNAS_KIND_MBCONV;
}
// the two facts of a kind the host code asks for repeatedly: an E buffer, a BatchNorm site 0 (today: the plain MBConv cell has both)
static inline bool cell_has_E(const TfnasCellDesc& d) { return cell_kind(d) == TFNAS_KIND_MBCONV; }
static inline bool cell_has_bn0(const TfnasCellDesc& d) { return cell_kind(d) == TFNAS_KIND_MBCONV; }
// TFNAS_CELL_KINDS: a cell whose groups each have a kind of their own (TfnasGroup.kind).  "Mixed" is not a fourth kind: the entry
// points canonicalise the descriptor first (capi.hip: kinds_canon -- all groups plain: the bit is dropped; one group: its one-block
// bit instead), so past them the bit means a cell with several groups of which at least one is not plain.  Its launch sequences
// run every kind's front / tail on a SUB-descriptor: the groups of that kind only (same M, same off / se_off: the same columns
// of the [pixels][M] tensors), the kind's one-block bit set next to TFNAS_CELL_KINDS -- cell_kind() of a sub-descriptor is its
// groups' kind.  A launcher handed one must leave the other groups' columns of every shared table alone (reduce_pair_rows).
// (Shared: stats2 -- every kind's front writes its own columns.  stats1, red1 and cb1 belong to the plain groups alone: their other
// columns are never read, and whole-row reductions into them may leave anything there.)
static inline bool cell_mixed(const TfnasCellDesc& d) { return (d.flags & TFNAS_CELL_KINDS) != 0; }
static inline CellKind group_kind(const TfnasCellDesc& d, int g) {
    return cell_mixed(d) && !cell_fused(d) && !cell_noexpand(d) ? (CellKind)d.g[g].kind : cell_kind(d);
}
// TFNAS_CELL_SKIP: groups of a mixed residual cell may be TFNAS_GROUP_SKIP, the identity candidate.  It is not a kind either: a
// skip group binds no field, has no BatchNorm site and no columns anywhere; it adds its mix weight to the residual term, one entry
// to dwmix (<dout, x>) and nothing else.  Skip groups stand last (capi.hip: check_kind), so the launch sequences run on the
// descriptor of the first G' = G - skip_groups(d) groups (capi.hip: skip_strip) and only the four kernels that sum or emit mix
// weights are told the caller's G (launch_mix_fwd, launch_mix_dw, launch_dx_add_res: `nw`).
static inline bool cell_skip(const TfnasCellDesc& d) { return (d.flags & TFNAS_CELL_SKIP) != 0; }
static inline int skip_groups(const TfnasCellDesc& d) {
    int n = 0;
    if (cell_skip(d) && cell_mixed(d))
        for (int g = d.G < TFNAS_MAX_GROUPS ? d.G : TFNAS_MAX_GROUPS; g > 0 && d.g[g - 1].kind == TFNAS_GROUP_SKIP; --g) ++n;
    return n;
}
// TFNAS_CELL_DILATION: the depthwise dilation of group g (TfnasGroup.dil) -- 1, or 2 = taps two pixels apart.  Without the bit the
// word is not read (it was padding): every group is undilated.  The entry points refuse any other value (capi.hip: check_dilation).
__host__ __device__ static inline int group_dil(const TfnasCellDesc& d, int g) {
    return ((d.flags & TFNAS_CELL_DILATION) && d.g[g].dil == 2) ? 2 : 1;
}
// a cell with a dilated group follows the 7 x 7 rule: E materialised, LDS tile kernels in every depthwise pass, the depthwise weight
// gradient in a launch of its own (dwconv_kernels.hip: dw_tile_only; efree_supported, fx_plan)
static inline bool cell_dilated(const TfnasCellDesc& d) {
    for (int g = 0; g < d.G && g < TFNAS_MAX_GROUPS; ++g)
        if (group_dil(d, g) != 1) return true;
    return false;
}
// TFNAS_CELL_MIXK: TfnasGroup.k of group g may be a PACKED word -- a MixConv group, one depthwise convolution whose channels are
// split into two or three contiguous segments of ascending kernel size, nibble s = the kernel size of segment s (0x53, 0x73,
// 0x75, 0x753: capi.hip, check_mixk).  Without the bit no word is packed (a value above 7 is refused as it always was).  Every
// reader of TfnasGroup.k past the entry points asks these, never the raw word.
__host__ __device__ static inline bool group_packed(const TfnasCellDesc& d, int g) {
    return (d.flags & TFNAS_CELL_MIXK) && d.g[g].k > 0xf;
}
__host__ __device__ static inline int group_nseg(const TfnasCellDesc& d, int g) {
    return group_packed(d, g) ? ((d.g[g].k >> 8) ? 3 : 2) : 1;
}
__host__ __device__ static inline int seg_k(const TfnasCellDesc& d, int g, int s) {
    return group_packed(d, g) ? ((d.g[g].k >> (4 * s)) & 0xf) : d.g[g].k;
}
// first channel QUAD of segment s of an n-segment group of q = mcp / 4 quads (s = n: q itself): q / n quads each, the q % n
// remaining ones to segment 0 -- where mc is a multiple of 4 n MixNet's own _split_channels; every split point a multiple of 4
// channels (16 bytes: the kernels' float4 accesses).  Segment s covers channels [4 Q_s, min(4 Q_s+1, mc)).
__host__ __device__ static inline int seg_quad0(int q, int n, int s) {
    const int base = n == 1 ? q : n == 2 ? (q >> 1) : q / 3;       // (q / n with constant divisors: no division sequence in the kernels)
    return s == 0 ? 0 : s * base + (q - n * base);
}
// floats of group g's depthwise weight (and of its block of the weight-gradient partial row): mc * k * k, a packed group the sum
// over its segments [mc_s][k_s * k_s], in segment order
__host__ __device__ static inline size_t group_dw_floats(const TfnasCellDesc& d, int g) {
    const int n = group_nseg(d, g), q = d.g[g].mcp >> 2, mc = d.g[g].mc;
    if (n == 1) return (size_t)mc * d.g[g].k * d.g[g].k;       // (a plain group: what it always was, planned or not)
    size_t f = 0;
    for (int s = 0; s < n; ++s) {
        const int lo = 4 * seg_quad0(q, n, s), hi4 = 4 * seg_quad0(q, n, s + 1), hi = hi4 < mc ? hi4 : mc, ks = seg_k(d, g, s);
        f += (size_t)(hi - lo) * ks * ks;
    }
    return f;
}
// a cell with a packed group follows the 7 x 7 rule like a dilated one: only the tile kernels take their chunk from a segment
static inline bool cell_packed(const TfnasCellDesc& d) {
    for (int g = 0; g < d.G && g < TFNAS_MAX_GROUPS; ++g)
        if (group_packed(d, g)) return true;
    return false;
}
// group-aware forms of the two facts: some group has an E buffer / a BatchNorm site 0
static inline bool any_group_has_E(const TfnasCellDesc& d) {
    for (int g = 0; g < d.G; ++g)
        if (group_kind(d, g) == TFNAS_KIND_MBCONV) return true;
    return false;
}
// TFNAS_CELL_SE_STYLE (TfnasCellDesc.se_style, checked by the entry points): the hidden activation of the cell's squeeze-excite
// branches resolved to a TFNAS_ACT_* (0 in the low nibble: the cell's own), and their gate function (SE_GATE_*)
enum SeGate { SE_GATE_LOGISTIC = 0, SE_GATE_HSIGMOID = 1 };
static inline int se_hidden_act(const TfnasCellDesc& d) {
    const int h = d.se_style & TFNAS_SE_HIDDEN_MASK;
    return h ? h - 1 : d.act;
}
static inline int se_gate(const TfnasCellDesc& d) { return (d.se_style & TFNAS_SE_GATE_MASK) >> TFNAS_SE_GATE_SHIFT; }
// the activation fork of a launcher (inside a function returning int): the statements run with ACT = the launch's activation as a
// compile-time constant; any other value is TFNAS_EINVAL
#define ACT_DISPATCH(act, ...)                                                                        \
    if ((act) == TFNAS_ACT_RELU) { constexpr int ACT = TFNAS_ACT_RELU; __VA_ARGS__; }                 \
    else if ((act) == TFNAS_ACT_SWISH) { constexpr int ACT = TFNAS_ACT_SWISH; __VA_ARGS__; }          \
    else if ((act) == TFNAS_ACT_RELU6) { constexpr int ACT = TFNAS_ACT_RELU6; __VA_ARGS__; }          \
    else if ((act) == TFNAS_ACT_HSWISH) { constexpr int ACT = TFNAS_ACT_HSWISH; __VA_ARGS__; }        \
    else return TFNAS_EINVAL;
// the same for the gate function of the squeeze-excite kernels: GATE = SE_GATE_* as a compile-time constant
#define SE_GATE_DISPATCH(gate, ...)                                                                   \
    if ((gate) == SE_GATE_LOGISTIC) { constexpr int GATE = SE_GATE_LOGISTIC; __VA_ARGS__; }           \
    else if ((gate) == SE_GATE_HSIGMOID) { constexpr int GATE = SE_GATE_HSIGMOID; __VA_ARGS__; }      \
    else return TFNAS_EINVAL;

// gemm_kernels.hip
int gemm_mode();            // arithmetic of the row-tiled GEMMs (tfnas_hip.h: TFNAS_GEMM_*): the process default ...
int set_gemm_mode(int m);
int gemm_mode_of(const TfnasCellDesc& d);   // ... and the descriptor's own (TFNAS_GEMM_EXPLICIT), else that default
// What one 1x1-convolution GEMM family launches, chosen once by the family's planner (gemm_plan_*: a pure function of the
// descriptor and the few facts the launcher gets from its arguments); the launcher carries it out: one dispatch, then the reductions.
enum GemmVariant { GEMM_PLAIN, GEMM_STEM, GEMM_XG, GEMM_FOLD, GEMM_GRAM1 };
struct GemmPlan {
    GemmVariant var;        // stem im2col operand / Gram-form expand wgrad / FOLD epilogue / one-launch Gram operator
    int mm;                 // arithmetic of this launch (TFNAS_GEMM_*; the families with the fp32 loop only: 0)
    int nt, tiles;          // column-tile width in 16-column MFMA tiles, column tiles of the N extent
    int splits;             // K-splits of the GEMM launch (1: none)
    int rps;                // K extent of a split: rows (weight gradients), 16-channel chunks (expand_gram); project_fwd: rows per
                            // k_pr_reduce workgroup
    int parts;              // partial tiles the family's own reduction kernel sums (k_pr_reduce, k_dx_reduce); 0: not launched
    dim3 grid, grid2;       // of the GEMM, of that reduction kernel
    size_t shm;             // dynamic LDS bytes of the GEMM
    size_t out, out_main;   // weight gradients: floats of one split's partial output; of which the groups' own gradients (the
                            // rest: the extension rows of GEMM_XG)
};
GemmPlan gemm_plan_expand_fwd(const TfnasCellDesc& d);
GemmPlan gemm_plan_project_fwd(const TfnasCellDesc& d);
GemmPlan gemm_plan_project_dgrad(const TfnasCellDesc& d, bool fold);       // fold: rec is given
GemmPlan gemm_plan_project_wgrad(const TfnasCellDesc& d);
GemmPlan gemm_plan_expand_gram(const TfnasCellDesc& d, size_t scratch_floats);
// split: dxp is given (room for the K-split partials; tfnas_cell_ws sizes it from this plan's `splits`).  nsl >= 0: the fused
// per-image route -- dxp[0 .. nsl) already hold partial sums, the GEMM adds one more partial tile and is never split
GemmPlan gemm_plan_expand_dgrad(const TfnasCellDesc& d, bool split, int nsl = -1);
GemmPlan gemm_plan_expand_wgrad(const TfnasCellDesc& d);
int launch_expand_fwd(const TfnasCellDesc& d, const float* x, float* E, double* stats1, float* part,
                      hipStream_t s);
int launch_project_fwd(const TfnasCellDesc& d, const float* D, const float* gate, const double* stats2,
                       float* Pr, double* stats3, float* part, hipStream_t s);
// D / stats2 / rec non-NULL: FOLD variant -- the per-image BN2-backward tables are accumulated in the epilogue into `rec`
// (project_fold_ok(d, floats of rec) must hold); launch_bn2_gather then replaces launch_bn2_pool
int launch_project_dgrad(const TfnasCellDesc& d, const float* dout, const float* Pr, const double* stats3,
                         const double* red3, const float* wmix, float* dZ, hipStream_t s, const float* D = nullptr,
                         const double* stats2 = nullptr, float* rec = nullptr);
constexpr int FOLD_SLOTS = 4, FOLD_Q = 5;       // records of the FOLD epilogue: rec[((row_tile * 4 + slot) * 5 + q) * M + channel]
static inline bool project_fold_ok(const TfnasCellDesc& d, size_t scratch_floats) {
    const int HW = d.Ho * d.Wo;
    const size_t nrt = ((size_t)d.N * HW + 127) / 128;
    if (act_tile_only(d.act)) return false;          // (the epilogue forks ReLU / Swish; such a cell runs k_bn2_pool)
    return HW >= 43 && nrt * FOLD_SLOTS * FOLD_Q * (size_t)d.M <= scratch_floats;
}
int launch_project_wgrad(const TfnasCellDesc& d, const float* dout, const float* Pr, const float* D,
                         const float* gate, const double* stats2, const double* stats3, const double* red3,
                         const float* wmix, float* part, hipStream_t s);
size_t expand_gram_floats(const TfnasCellDesc& d);
int launch_expand_gram(const TfnasCellDesc& d, const float* cb1, float* scratch, size_t scratch_floats, float* gram,
                       hipStream_t s);
// (nsl >= 0: the fused route's form -- dEh unused, dxp[0 .. nsl) hold launch_fx_bwd's partial sums)
int launch_expand_dgrad(const TfnasCellDesc& d, const float* dEh, const float* x, const float* cb1, const float* gram,
                        const float* dout, const float* wmix, float* dx, float* dxp, hipStream_t s,
                        const float* add_src = nullptr, const float* add_scale = nullptr, int nsl = -1);
int launch_expand_wgrad(const TfnasCellDesc& d, const float* dEh, const float* E, const float* cb1,
                        const float* x, float* part, hipStream_t s);
// dx += (sum of the nw mix weights) * dout: the residual gradient of a mixed residual cell, after its last branch
// (nw: entries of wmix -- d.G, plus the skip groups of the caller's descriptor)
int launch_dx_add_res(const TfnasCellDesc& d, int nw, const float* dout, const float* wmix, float* dx, hipStream_t s);

// dwconv_kernels.hip: the depthwise k x k convolution in three kernel families, each with the geometry struct its kernels take by
// value: k = 3 | 5 in all of them, k = 7 and dilation 2 (k = 3 | 5) in the LDS tile kernels only (a cell with such a group is
// planned onto those in every pass); ReLU | Swish in all of them, ReLU6 | hard-swish in the tile kernels only (act_tile_only: the same rule).
// Register-window kernels (dw_direct.inc):
struct DwDirect {
    int chunks;      // 32-channel chunks of the groups with this kernel size
    int ncg;         // column groups per image: ceil(Wo / (4 * JW))
    int nseg;        // waves per (chunk, column group), a multiple of 4
    int per;         // macro-steps per wave
    int steps;       // N * (Ho + A)
    int nwg;         // chunks * ncg * nseg / 4
};
// LDS ring kernels of the stride-1 cells (dw_stream.inc):
struct DwSlide {
    int TH, TW;            // rows per block, columns of the band (multiple of 4)
    int CC, CCP, cq_shift; // channels per workgroup, pixel stride in LDS (floats)
    int RB, L1;            // ring rows, ring columns (pixels) = TW + K - 1
    int chunks, gx;        // channel chunks of this launch, image lanes (= partial rows)
};
// LDS tile kernels (dwconv_kernels.hip):
struct DwGeom {
    int T0, T1;        // tile height / width (in outputs for fwd & wgrad, in inputs for bwd-data)
    int CC;            // channels per workgroup (16/32/64)
    int cq_shift;      // log2(CC/4)
    int tilesH, tilesW, ntiles;   // ntiles = N * tilesH * tilesW
    int L0, L1;        // LDS tile extent (rows, cols)
};
// What one depthwise pass launches, chosen once by the pass's planner from the descriptor (route bits included), whether E is
// present and whether x is given; the launcher carries it out: the k = 3 launch, the k = 5 launch, the k = 7 launch, the dilated
// k = 3 and k = 5 launches (the last three: DW_TILE only), then the reductions of the `rows` partial rows.
enum DwFamily { DW_DIRECT, DW_RING, DW_TILE };
constexpr int DW_NK = 5;  // launch slots of a pass, one per (kernel size, dilation): (3, 1) (5, 1) (7, 1) (3, 2) (5, 2)
struct DwPlan {
    DwFamily fam;
    int rows;             // partial rows of the pass
    int chunks[DW_NK];    // channel chunks of each slot's launch (0: not launched)
    DwDirect direct[2];   // geometry of the k = 3 / k = 5 launch: the planned family's member
    DwSlide ring[2];
    DwGeom tile[DW_NK];
    int jw;               // DW_DIRECT: output columns per lane (JW)
    bool pipe;            // DW_RING: the register-prefetch variant (PIPE)
    int kq;               // E-free: ic / 4 of the expand recomputed from x (KQ); 0: E is read
    bool fuse_wgrad;      // backward-data: the pass also writes every group's g_dw, so launch_dw_wgrad is not called
};
// E == nullptr: E-free mode (efree.h) -- the expanded activation is recomputed from x inside the depthwise kernels
int launch_dw_fwd(const TfnasCellDesc& d, const float* E, const float* x, const double* stats1, float* D,
                  double* stats2, float* part, hipStream_t s);
bool efree_supported(const TfnasCellDesc& d);
static inline bool efree_ic_ok(int ic) { return ic == 16 || ic == 24 || ic == 40; }   // (efree.h: the tile / ring E-free kernels)
int launch_expand_stats_gram(const TfnasCellDesc& d, const float* x, double* stats1, float* part, hipStream_t s);
int launch_x_colsum(const float* x, int P, int ic, int rps, int nb, float* part, hipStream_t s);
// fx_kernels.hip: fused per-image route of the late cells (fx.h) -- E-free cells with 64 <= ic <= 192 and images <= 14 x 14
bool fx_supported(const TfnasCellDesc& d);
int launch_fx_stats(const TfnasCellDesc& d, const float* x, double* stats1, float* part, hipStream_t s);
// E != nullptr ("stored-ehat mode"): the forward also leaves ehat = BN1(x W1^T) in E and the backward reads it back instead of
// recomputing it; E == nullptr: nothing is stored, the backward rebuilds ehat from x
int launch_fx_fwd(const TfnasCellDesc& d, const float* x, const double* stats1, float* E, float* D, double* stats2,
                  float* part, hipStream_t s);
// backward: the partial sums of dE (rstd . W1) into scratch[0 .. nsl * P * ic) (nsl returned), the BN1-backward sums into
// red1 and the cb1 table; the caller finishes with launch_expand_gram + launch_expand_dgrad(dxp = scratch, nsl)
int launch_fx_bwd(const TfnasCellDesc& d, const float* x, const float* Eh, const double* stats1, const double* stats2,
                  const double* red2, const float* dZ, const float* D, const float* gate, const float* dpooled, float* scratch,
                  size_t scratch_floats, double* red1, float* cb1, float* part, int* nsl, hipStream_t s);
bool dw_wgrad_row_fits(const TfnasCellDesc& d);     // the depthwise weight-gradient partial row fits the partials region
DwPlan dw_plan_bwd_data(const TfnasCellDesc& d, bool efree, bool has_x);
// p = dw_plan_bwd_data(d, E == nullptr, x != nullptr); cb1: also fill the BN1 table
int launch_dw_bwd_data(const DwPlan& p, const TfnasCellDesc& d, const float* dZ, const float* gate, const float* dpooled,
                       const float* D, const double* stats2, const double* red2, const float* E, const float* x,
                       const double* stats1, float* dEh, double* red1, float* part, hipStream_t s, float* cb1 = nullptr);
// cell_noexpand(d): dx [N*H*W][ic] = dw^T(dd) (+ dres [N*H*W][ic], the residual gradient, or NULL) in one tile-kernel pass
// accum: dx += instead (a later branch of a mixed cell; ONE group per launch then: every NOEXPAND group owns all of dx)
int launch_dw_bwd_dx(const TfnasCellDesc& d, const float* dZ, const float* gate, const float* dpooled, const float* D,
                     const double* stats2, const double* red2, const float* dres, float* dx, hipStream_t s, bool accum = false);
int launch_reduce_bn1(const TfnasCellDesc& d, const float* part, int nb, const double* stats1, double* red1, float* cb1,
                      hipStream_t s);
int launch_dw_wgrad(const TfnasCellDesc& d, const float* dZ, const float* gate, const float* dpooled, const float* D,
                    const double* stats2,
                    const double* red2, const float* E, const double* stats1, float* part, hipStream_t s);

// conv_kernels.hip: the dense 3x3 convolution of a cell_fused(d) block, x [N*H*W][ic] NHWC, weight OIHW in g[0].w_expand
// forward: D [N*Ho*Wo][M] and the BatchNorm statistics of D (partial rows in `part`, reduced into stats2; the repacked weight at
// the top of `part`)
int launch_conv_fwd(const TfnasCellDesc& d, const float* x, float* D, double* stats2, float* part, hipStream_t s);
// dd [N*Ho*Wo][M] = the gradient w.r.t. D (BatchNorm + activation + SE gate backward of dZ), pad columns zero
int launch_conv_dd(const TfnasCellDesc& d, const float* dZ, const float* D, const float* gate, const float* dpooled,
                   const double* stats2, const double* red2, float* dd, hipStream_t s);
// g[0].g_expand (OIHW) = or += the weight gradient, K-split over pixels through `part`
int launch_conv_wgrad(const TfnasCellDesc& d, const float* dd, const float* x, float* part, hipStream_t s);
bool conv_wgrad_row_fits(const TfnasCellDesc& d);     // the partial weight gradient of one split (9 ic mc floats) fits the partials
                                                       // region, the repacked weight next to 128 statistics rows (tfnas_cell_plan: else TFNAS_ERANGE)
// dx [N*H*W][ic] = conv^T(dd) (+ dres [N*H*W][ic], the residual gradient, or NULL); `part`: scratch of the repacked weight
// accum: dx += instead (a later branch of a mixed cell)
int launch_conv_dgrad(const TfnasCellDesc& d, const float* dd, const float* dres, float* dx, float* part, hipStream_t s,
                      bool accum = false);

// pointwise_kernels.hip (SE squeeze, BN2 backward statistics, mixing epilogue, BN constant tables)
// se_kernels.hip (SE excite FCs as small GEMMs: launch_se_fc_fwd / launch_se_fc_bwd / launch_se_wgrad)
int launch_se_pool(const TfnasCellDesc& d, const float* D, const double* stats2, float* pooled, hipStream_t s);
int launch_se_fc_fwd(const TfnasCellDesc& d, const float* pooled, float* hpre, float* gate, float* scratch,
                     size_t scratch_floats, hipStream_t s);
// nw: entries of wmix (and of dwmix) -- d.G, plus the skip groups of the caller's descriptor (cell_skip), which stand after the
// d.G computing groups: they add to the residual weight / get <dout, x> alone
int launch_mix_fwd(const TfnasCellDesc& d, int nw, const float* Pr, const double* stats3, const float* wmix,
                   const float* x, float* out, hipStream_t s);
int launch_mix_bwd_stats(const TfnasCellDesc& d, const float* dout, const float* Pr, const double* stats3,
                         const float* x, double* red3, float* part, hipStream_t s);
int launch_mix_dw(const TfnasCellDesc& d, int nw, const double* red3, const double* resdot, float* dwmix, hipStream_t s);
int launch_se_bwd_reduce(const TfnasCellDesc& d, const float* dZ, const float* D, const double* stats2,
                         float* dgate, hipStream_t s);
int launch_se_fc_bwd(const TfnasCellDesc& d, const float* dgate, const float* gate, const float* hpre, float* dhpre,
                     float* dpooled, float* scratch, size_t scratch_floats, hipStream_t s);
int launch_se_wgrad(const TfnasCellDesc& d, const float* dgate, const float* gate, const float* dhpre,
                    const float* hpre, const float* pooled, hipStream_t s);
bool bn2_fused_fits(const TfnasCellDesc& d);
int launch_bn2_pool(const TfnasCellDesc& d, const float* dZ, const float* D, const double* stats2, float* dgate,
                    float* pp, hipStream_t s);
int launch_bn2_gather(const TfnasCellDesc& d, const float* rec, float* dgate, float* pp, hipStream_t s);
int launch_bn2_finish(const TfnasCellDesc& d, const float* pp, const float* gate, const float* dpooled, double* red2,
                      hipStream_t s);
int launch_bn2_bwd(const TfnasCellDesc& d, const float* dZ, const float* D, const double* stats2, const float* gate,
                   const float* dpooled, double* red2, float* part, hipStream_t s);
int launch_head_pool(const TfnasCellDesc& d, const float* E, const double* stats1, float* pooled, hipStream_t s);
int launch_head_bwd(const TfnasCellDesc& d, const float* E, const double* stats1, const float* dpooled, float* dEh,
                    double* red1, float* part, hipStream_t s);
// out[c] = sum_{b<nb} part[b*stride + c]  (double and/or float output); the deterministic replacement of atomics
// accum != 0: the float output is added to what out_f already holds (out_f[c] += (float)sum: the
// weight-gradient outputs of a TFNAS_CELL_ACCUM_WGRAD launch; the double output is always overwritten)
int launch_reduce_rows(const float* part, int nb, int ncols, size_t stride, double* out_d, float* out_f,
                       hipStream_t s, int accum = 0);
// `rows` partial rows of 2 * M (sum, sumsq) pairs -> a [M][2] table of doubles.  One launch over the whole row; for a
// sub-descriptor of a mixed cell one launch per group over its own columns: the table is shared with the other kinds' groups,
// whose columns of these partial rows were never written.
static inline int reduce_pair_rows(const TfnasCellDesc& d, const float* part, int rows, double* table, hipStream_t s) {
    if (!cell_mixed(d)) return launch_reduce_rows(part, rows, 2 * d.M, 2 * (size_t)d.M, table, nullptr, s);
    for (int g = 0; g < d.G; ++g) {
        const size_t o = 2 * (size_t)d.g[g].off;
        const int rc = launch_reduce_rows(part + o, rows, 2 * d.g[g].mcp, 2 * (size_t)d.M, table + o, nullptr, s);
        if (rc) return rc;
    }
    return 0;
}
/* One `part` scratch region = TFNAS_PART_ALLOC floats (16 MiB): TFNAS_PART_FLOATS for per-workgroup partial rows / split-K
   tiles; the last TFNAS_TAIL_SLOTS words are reserved (they held the ticket counters of the removed "last workgroup reduces"
   epilogues; the size of the region is part of the workspace ABI and stays). */
#define TFNAS_PART_ALLOC ((size_t)4 << 20)
#define TFNAS_TAIL_SLOTS ((size_t)1024)
#define TFNAS_PART_FLOATS (TFNAS_PART_ALLOC - TFNAS_TAIL_SLOTS)
int launch_bn1_consts(const TfnasCellDesc& d, const double* stats1, const double* red1, float* cb1,
                      hipStream_t s);

// arch_kernels.hip
int launch_arch_fwd(int ncell, const float* const* la, const float* e, const float* lat, float T, float* w,
                    float* cell_lat, hipStream_t s);
int launch_arch_bwd(int ncell, const float* w, const float* lat, const float* dw, const float* dcl, float T,
                    float* const* dla, hipStream_t s);
int launch_arch_project(int n, float* const* p, const int32_t* len, hipStream_t s);
int launch_arch_sample(int ncell, const float* const* la, const uint8_t* mask, const float* e, float T, int mode,
                       int32_t* pos, hipStream_t s);
int launch_sink_fwd(int K, const float* betas, const float* const* res, const float* cell_lat, uint64_t count,
                    float* out, float* out_lat, float* bw, hipStream_t s);
int launch_scale_copy(float* dst, const float* src, const float* scale, uint64_t count, hipStream_t s);
// dx = src + ((w[0][0] g + w[1][0] g) + ...), K <= TFNAS_MAX_SINK terms, `count` floats (a multiple of 4); src may be dx
int launch_dx_add_sink(float* dx, const float* src, const float* g, int K, const float* const* w, uint64_t count, hipStream_t s);
// dres[k] may be NULL (that depth output's share is added elsewhere: path level)
int launch_sink_bwd(int K, const float* bw, const float* const* res, const float* cell_lat, const float* dout,
                    const float* dlat, uint64_t count, float* const* dres, float* dbetas, float* dcell_lat,
                    double* dots, hipStream_t s);

// opt_kernels.hip
int launch_pack_ranges(const float* src, float* dst, int nranges, const uint64_t* off, const uint64_t* doff,
                       const uint64_t* len, hipStream_t s);
int launch_sgd_clip_step(float* w, float* g, float* m, int nranges, const uint64_t* off, const uint64_t* goff,
                         const uint64_t* len, float max_norm,
                         float lr, float momentum, float wd, float grad_scale, double* scratch, uint64_t scratch_doubles,
                         float* norm_out, hipStream_t s);
int launch_sgd_clip_ema_step(float* w, float* g, float* m, int nranges, const uint64_t* off, const uint64_t* goff,
                             const uint64_t* len, float max_norm, float lr, float momentum, float wd, float grad_scale,
                             float* ema, float ema_alpha, double* scratch, uint64_t scratch_doubles, float* norm_out,
                             hipStream_t s);
int launch_ema_lerp(float* ema, const float* src, int nranges, const uint64_t* off, const uint64_t* len, float ema_alpha,
                    hipStream_t s);
int launch_opt_groups_step(const TfnasOptGroups* d, float* w, float* g, float* m, float* v, float* ema, const uint8_t* gmap,
                           uint64_t total, double* scratch, uint64_t scratch_doubles, float* norm_out, hipStream_t s);
int launch_arch_adam_project(int n, float* const* p, const float* const* g, const int32_t* len, float* m, float* v,
                             float max_norm, float lr, float b1, float b2, float eps, float wd, int step, float grad_scale,
                             float* norm_out, hipStream_t s);

// bn_affine.hip (derived-network path: affine BatchNorm folded into the statistics tables, drop-connect)
int launch_bn_fwd_fix(double* stats, int nch, uint64_t cnt, float eps, const float* gamma, const float* beta, float* rmean,
                      float* rvar, float momentum, int eval, hipStream_t s, uint64_t world = 1);
int launch_bn_bwd_fix(double* red, int nch, uint64_t cnt, const float* gamma, const float* beta, float* dgamma, float* dbeta,
                      hipStream_t s, int accum = 0);
int launch_rowscale(float* out, const float* y, const float* res, const float* scale, int N, uint64_t per_image,
                    hipStream_t s);
