// Dense 3x3 convolution of the Fused-MBConv block (TFNAS_CELL_FUSED) as three implicit GEMMs on the row-tiled core of
// gemm_core.h / gemm_x3.h: forward, weight gradient, data gradient.  x is the NHWC cell input [N*H*W][ic], the weight is torch's
// OIHW [mc][ic][3][3] (TfnasGroup.w_expand), D / dd are [N*Ho*Wo][M] like every mid-channel stream of a cell.  pad 1, stride 1 | 2,
// no padded copy of x: a tap outside the image is a masked (zero) operand element.
//
// Reference arithmetic: ConvLayer (models/layers.py: Conv2d(k = 3, padding 1, bias = False) -> BatchNorm2d -> act) followed by the
// SE / project / BatchNorm chain of MBInvertedResBlock.forward, and the autograd backward of that convolution.
//
// The K index of the forward is (tap, channel): ic % 4 == 0, so every float4 of the im2col operand lies inside one tap.  The B
// operand's K index has stride 9 in OIHW: forward and data gradient repack the weight once per launch (k_conv_repack).
#include <stdlib.h>
#include "gemm_core.h"
#include "gemm_x3.h"
#include "kernels.h"
#include "prof.h"

// resident workgroups per CU (tiles of at most 64 columns): as the narrow 1x1 GEMMs (gemm_kernels.hip)
constexpr int conv_lb(int mm) { return mm == 0 ? 4 : 3; }
constexpr int conv_wgrad_lb(int nt) { return nt >= 3 ? 3 : 4; }

// ============================================================================ forward
// D[p][m] = sum_{tap, c} x[n][S ho + ky - 1][S wo + kx - 1][c] * w[m][c][tap],   p = (n, ho, wo), tap = 3 ky + kx
// rows: output pixels; K = 9 ic ordered (tap, c); columns: mid channels.
// epilogue: D, and this workgroup's (sum, sumsq) partial row of D per channel -> part (reduced into stats2 = BN_a statistics),
// the format of the depthwise forward (dw_flush_stats) and of k_expand_fwd.
template <int NT, int MM>
__global__ __launch_bounds__(256, conv_lb(MM)) void k_conv_fwd(TfnasCellDesc d, const float* __restrict__ x,
                                                               float* __restrict__ D, float* __restrict__ part,
                                                               const float* __restrict__ wf) {
    using T = GT<NT>;
    static_assert(T::B_ITERS == 1, "one B item per thread: its K position is the same in every chunk");
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    const int BX = blockIdx.x, n0 = blockIdx.y * T::BN;
    const int mc = d.g[0].mc, mcp = d.g[0].mcp, off = d.g[0].off, M = d.M;
    const int H = d.H, W = d.W, Wo = d.Wo, HWo = d.Ho * d.Wo, S = d.stride, ic = d.ic;
    const int Po = d.N * HWo, K = 9 * ic;
    const int nrt = (Po + 127) >> 7, nchunks = (K + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4, wrow = (tid >> 6) * 32;

    float cs[NT], cq[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) cs[j] = cq[j] = 0.f;

    for (int rt = BX; rt < nrt; rt += gridDim.x) {
        f32x4 acc[2][NT];
        acc_zero<NT>(acc);
        // the lane's two output pixels stay the same for the whole K loop
        int hi0[2], wi0[2];
        bool rok[2];
        const float* img[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = rt * 128 + wrow + 16 * i + lr, pc = min(p, Po - 1);
            const int n = pc / HWo, r = pc - n * HWo, ho = r / Wo, wo = r - ho * Wo;
            rok[i] = p < Po;
            hi0[i] = ho * S - 1;
            wi0[i] = wo * S - 1;
            img[i] = x + (size_t)n * H * W * ic;
        }
        // chunk bookkeeping (pre): the (tap, channel) of the lane's A quad
        int a_ky = 0, a_kx = 0, a_ch = 0;
        bool a_ok = false;
        auto pre = [&](int c) {
            const int ka = c * 16 + 4 * lk;
            a_ok = ka < K;
            const int ta = a_ok ? ka / ic : 0;
            a_ch = a_ok ? ka - ta * ic : 0;
            a_ky = ta / 3;
            a_kx = ta - 3 * a_ky;
        };
        auto tap_ok = [&](int i) -> bool {
            const int hi = hi0[i] + a_ky, wi = wi0[i] + a_kx;
            return a_ok && (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W;
        };
        auto la = [&](int c, int i, int kl) -> f32x4 {
            const int hi = hi0[i] + a_ky, wi = wi0[i] + a_kx;
            const size_t a = tap_ok(i) ? ((size_t)hi * W + wi) * ic + a_ch : 0;      // (clamped: masked in xa)
            return ld4(img[i] + a);
        };
        auto xa = [&](f32x4 r, int c, int i, int kl) -> f32x4 { return (rok[i] && tap_ok(i)) ? r : zero4(); };
        auto lb = [&](int c, int n, int kl) -> f32x4 {
            return ld4(wf + (size_t)min(n0 + n, mc - 1) * K + min(c * 16 + kl, K - 4));
        };
        auto xb = [&](f32x4 r, int c, int n, int kl) -> f32x4 { return (c * 16 + kl < K && n0 + n < mc) ? r : zero4(); };
        gemm_adirect<NT, true, MM>(pre, la, xa, lb, xb, nchunks, acc, lds);
        emit_tile_rows<NT>(acc, lds, [&](int lrow, int lc, f32x4 v) {
            const int p = rt * 128 + lrow;
            if (p < Po && n0 + lc < mcp) st4_nt(D + ((size_t)p * M + off + n0 + lc), v);
        });
        acc_colstats<NT>(acc, cs, cq);
    }
    flush_colstats<NT>(cs, cq, lds, part + (size_t)BX * 2 * M + 2 * (size_t)off, n0, mcp);
}

// ============================================================================ BN_a-backward operand
// dd[p][m] = the gradient w.r.t. the raw convolution output D (bn2_dd, tfnas_dev.h), written once as a [N*Ho*Wo][M] stream (pad
// columns mc .. mcp: zeros) that the weight-gradient and the data-gradient GEMM both read with plain loads.  (Forming it inside
// the two GEMMs' loaders reads dZ and D twice each -- four stream passes against these five -- and costs an activation fork and a
// per-image gate load in both K loops.)
template <int ACT>
__global__ __launch_bounds__(256) void k_conv_dd(TfnasCellDesc d, const float* __restrict__ dZ, const float* __restrict__ D,
                                                 const float* __restrict__ gate, const float* __restrict__ dpooled,
                                                 const double* __restrict__ stats2, const double* __restrict__ red2,
                                                 float* __restrict__ dd) {
    __shared__ f32x4 cst2[64];
    const int mc = d.g[0].mc, mcp = d.g[0].mcp, off = d.g[0].off, M = d.M;
    const int HWo = d.Ho * d.Wo, Po = d.N * HWo, c0 = blockIdx.y * 64;
    const int tid = threadIdx.x, q = tid & 15, ch = c0 + 4 * q;
    fill_cst2(cst2, d, 64, c0, mc, off, stats2, red2);
    __syncthreads();
    if (ch >= mcp) return;
    const bool has_se = d.g[0].se > 0;
    const float inv_hw = 1.f / (float)HWo;
    for (int p = blockIdx.x * 16 + (tid >> 4); p < Po; p += gridDim.x * 16) {
        const size_t a = (size_t)p * M + off + ch;
        const f32x4 dz = ld4_nt(dZ + a), dv = ld4_nt(D + a);
        f32x4 g4 = zero4(), dp4 = zero4();
        if (has_se) {
            const size_t t = (size_t)(p / HWo) * M + off + ch;
            g4 = ld4(gate + t);
            dp4 = ld4(dpooled + t) * splat4(inv_hw);
        }
        f32x4 r = bn2_dd<ACT>(cst2, 4 * q, dz, dv, has_se, g4, dp4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ch + j >= mc) r[j] = 0.f;
        st4(dd + a, r);
    }
}

// ============================================================================ weight gradient (TN, split-K over pixels)
// part[split][(m ic + c) 9 + tap] = sum_{p in split} dd[p][m] * x[n][S ho + ky - 1][S wo + kx - 1][c]     (OIHW, like the weight)
// rows: mid channels (128 per tile); columns: (tap, c), 9 ic of them; K: output pixels.  k_reduce_rows sums the splits.
struct RawTap { f32x4 v; bool ok; };
template <int NT>
__global__ __launch_bounds__(256, conv_wgrad_lb(NT)) void k_conv_wgrad(TfnasCellDesc d, const float* __restrict__ dd,
                                                                       const float* __restrict__ x, int rows_per_split,
                                                                       float* __restrict__ part, size_t out_size) {
    using T = GT<NT>;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    const int ic = d.ic, mc = d.g[0].mc, mcp = d.g[0].mcp, off = d.g[0].off, M = d.M;
    const int H = d.H, W = d.W, Wo = d.Wo, HWo = d.Ho * d.Wo, S = d.stride, Po = d.N * HWo, NC = 9 * ic;
    float* __restrict__ gw = part + (size_t)blockIdx.x * out_size;
    const int m0 = blockIdx.y * 128, n0 = blockIdx.z * T::BN;
    const int r0 = blockIdx.x * rows_per_split, r1 = min(Po, r0 + rows_per_split);
    const int nchunks = (r1 - r0 + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4, wrow = (tid >> 6) * 32;

    // per-thread constants of the K loop: its quad of mid channels (A), the (tap, channel quad) of its B items
    const int mch = m0 + (tid & 31) * 4;
    const bool chok = mch < mcp;
    const size_t acol = (size_t)off + min(mch, mcp - 4);
    constexpr int BQ = T::BN / 4;
    int bky[T::B_ITERS], bkx[T::B_ITERS], bch[T::B_ITERS];
    bool bok[T::B_ITERS];
#pragma unroll
    for (int i = 0; i < T::B_ITERS; ++i) {
        const int idx = tid + 256 * i, cc = n0 + (idx % BQ) * 4;
        bok[i] = idx < T::B_ITEMS && cc < NC;
        const int tap = bok[i] ? cc / ic : 0;
        bch[i] = bok[i] ? cc - tap * ic : 0;
        bky[i] = tap / 3;
        bkx[i] = tap - 3 * bky[i];
    }

    f32x4 acc[2][NT];
    acc_zero<NT>(acc);
    auto la = [&](int c, int i, int kl, int m) -> f32x4 {
        const int p = min(r0 + c * 16 + kl, r1 - 1);
        return ld4(dd + (size_t)p * M + acol);
    };
    auto xa = [&](f32x4 r, int c, int i, int kl, int m) -> f32x4 { return (chok && r0 + c * 16 + kl < r1) ? r : zero4(); };
    auto lb = [&](int c, int i, int kl, int n) -> RawTap {
        const int p = min(r0 + c * 16 + kl, r1 - 1);         // (item slots past the tile: kl >= 16, clamped like any row)
        const int im = p / HWo, r = p - im * HWo, ho = r / Wo, wo = r - ho * Wo;
        const int hi = ho * S - 1 + bky[i], wi = wo * S - 1 + bkx[i];
        RawTap t;
        t.ok = bok[i] && (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W;
        const size_t a = t.ok ? ((size_t)hi * W + wi) * ic + bch[i] : 0;
        t.v = ld4(x + (size_t)im * H * W * ic + a);
        return t;
    };
    auto xb = [&](RawTap t, int c, int i, int kl, int n) -> f32x4 { return (t.ok && r0 + c * 16 + kl < r1) ? t.v : zero4(); };
    gemm_mainloop2<NT, false, false, false>(la, xa, lb, xb, nchunks, acc, lds);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int cc = n0 + 16 * j + lr;
        if (cc >= NC) continue;
        const int tap = cc / ic, c = cc - tap * ic;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = m0 + wrow + 16 * i + 4 * lq + r;
                if (ch < mc) gw[((size_t)ch * ic + c) * 9 + tap] = acc[i][j][r];
            }
    }
}

// ============================================================================ data gradient
// dx[q][c] = sum_{tap, m} dd[n][(hi + 1 - ky) / S][(wi + 1 - kx) / S][m] * w[m][c][tap]  (+ dres[q][c]),   q = (n, hi, wi)
// rows: input pixels; K = 9 mcp ordered (tap, m) (dd's pad columns are zeros); columns: input channels.  At stride 2 a tap
// contributes only where both divisions are exact (row / column parity); every other element is a masked zero.
// dres: the residual-branch gradient [N*H*W][ic] of a residual block (NULL otherwise), added in the same store.
// accum: dx already holds the data gradient of the cell's earlier branches (a mixed cell, kernels.h: cell_mixed): the same
// store adds it, each element read and written by the one thread that owns it -- no atomics, a fixed order on the stream.
template <int NT, int MM>
__global__ __launch_bounds__(256, conv_lb(MM)) void k_conv_dgrad(TfnasCellDesc d, const float* __restrict__ dd,
                                                                 const float* __restrict__ dres, float* __restrict__ dx,
                                                                 const float* __restrict__ wd, int accum) {
    using T = GT<NT>;
    static_assert(T::B_ITERS == 1, "one B item per thread: its K position is the same in every chunk");
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    const int n0 = blockIdx.y * T::BN;
    const int mcp = d.g[0].mcp, off = d.g[0].off, M = d.M;
    const int W = d.W, HW = d.H * d.W, Ho = d.Ho, Wo = d.Wo, S = d.stride, ic = d.ic;
    const int P = d.N * HW, K = 9 * mcp;
    const int nrt = (P + 127) >> 7, nchunks = (K + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4, wrow = (tid >> 6) * 32;
    constexpr int BQ = T::BN / 4;
    const int bkl = tid / BQ, bcol = n0 + (tid % BQ) * 4;       // the thread's B item: K row of the chunk, column quad
    const bool bcok = tid < T::B_ITEMS && bcol < ic;
    const int bcc = min(bcol, ic - 4);

    for (int rt = blockIdx.x; rt < nrt; rt += gridDim.x) {
        f32x4 acc[2][NT];
        acc_zero<NT>(acc);
        int hi1[2], wi1[2];
        bool rok[2];
        const float* img[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = rt * 128 + wrow + 16 * i + lr, qc = min(q, P - 1);
            const int n = qc / HW, r = qc - n * HW, hi = r / W, wi = r - hi * W;
            rok[i] = q < P;
            hi1[i] = hi + 1;
            wi1[i] = wi + 1;
            img[i] = dd + (size_t)n * Ho * Wo * M + off;
        }
        int a_ky = 0, a_kx = 0, a_m = 0;
        bool a_ok = false;
        auto pre = [&](int c) {
            const int ka = c * 16 + 4 * lk;
            a_ok = ka < K;
            const int ta = a_ok ? ka / mcp : 0;
            a_m = a_ok ? ka - ta * mcp : 0;
            a_ky = ta / 3;
            a_kx = ta - 3 * a_ky;
        };
        // the output pixel a tap of input pixel i reads, and whether it exists
        auto src = [&](int i, int& ho, int& wo) -> bool {
            const int th = hi1[i] - a_ky, tw = wi1[i] - a_kx;
            ho = S == 2 ? th >> 1 : th;
            wo = S == 2 ? tw >> 1 : tw;
            const bool par = S == 1 || !((th | tw) & 1);
            return a_ok && par && th >= 0 && tw >= 0 && ho < Ho && wo < Wo;
        };
        auto la = [&](int c, int i, int kl) -> f32x4 {
            int ho, wo;
            const size_t a = src(i, ho, wo) ? ((size_t)ho * Wo + wo) * M + a_m : 0;      // (clamped: masked in xa)
            return ld4(img[i] + a);
        };
        auto xa = [&](f32x4 r, int c, int i, int kl) -> f32x4 {
            int ho, wo;
            return (rok[i] && src(i, ho, wo)) ? r : zero4();
        };
        auto lb = [&](int c, int kl, int n) -> f32x4 { return ld4(wd + (size_t)min(c * 16 + bkl, K - 1) * ic + bcc); };
        auto xb = [&](f32x4 r, int c, int kl, int n) -> f32x4 { return (c * 16 + bkl < K && bcok) ? r : zero4(); };
        gemm_adirect<NT, false, MM>(pre, la, xa, lb, xb, nchunks, acc, lds);
        emit_tile_rows<NT>(acc, lds, [&](int lrow, int lc, f32x4 v) {
            const int q = rt * 128 + lrow;
            if (q < P && n0 + lc < ic) {
                const size_t a = (size_t)q * ic + n0 + lc;
                if (dres) v += ld4_nt(dres + a);
                if (accum) v += ld4_nt(dx + a);
                st4_nt(dx + a, v);
            }
        });
    }
}

// ============================================================================ weight repack
// The B operand's K index has stride 9 in OIHW.  Once per launch the weight is repacked into the top of the launch's `part`
// scratch -- forward: wf[m][tap * ic + c] (K-contiguous rows of 9 ic);  data gradient: wd[tap * mcp + m][c] (rows of ic, the pad
// rows m >= mc zero) -- so that the GEMMs' B loaders are one 16-byte load per quad.  Measured against gathering the four scalars of
// a quad straight from the L2-resident weight: the repack wins 13-17 % of the forward and 7-10 % of the data
// gradient, its own launch included.
__global__ __launch_bounds__(256) void k_conv_repack(TfnasCellDesc d, float* __restrict__ wf, float* __restrict__ wd) {
    const int ic = d.ic, mc = d.g[0].mc, mcp = d.g[0].mcp;
    const float* __restrict__ w = d.g[0].w_expand;
    const int total = (wf ? mc : mcp) * 9 * ic;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        if (wf) {
            const int m = idx / (9 * ic), k = idx - m * 9 * ic, tap = k / ic, c = k - tap * ic;
            wf[idx] = w[((size_t)m * ic + c) * 9 + tap];
        } else {
            const int kk = idx / ic, c = idx - kk * ic, tap = kk / mcp, m = kk - tap * mcp;
            wd[idx] = m < mc ? w[((size_t)m * ic + c) * 9 + tap] : 0.f;
        }
    }
}
static size_t conv_repack_floats(const TfnasCellDesc& d) { return ((size_t)9 * d.ic * d.g[0].mcp + 63) & ~(size_t)63; }

// ============================================================================ host: plans and launchers
#define CONV_MM(mode, ...)                                     \
    switch (mode) {                                            \
        case 0: { constexpr int MM = 0; __VA_ARGS__; } break;  \
        case 1: { constexpr int MM = 1; __VA_ARGS__; } break;  \
        case 3: { constexpr int MM = 3; __VA_ARGS__; } break;  \
        default: { constexpr int MM = 6; __VA_ARGS__; } break; \
    }

// persistent row blocks of a row-tiled launch (the rule of the 1x1 GEMMs, gemm_kernels.hip: row_blocks): the gx that minimises
// rounds x tiles per workgroup, the larger on ties, at most `cap`
static int conv_row_blocks(int rows, int col_tiles, size_t cap, int slots) {
    const int nrt = cdiv(rows, 128);
    int lim = nrt;
    if ((size_t)lim > cap) lim = (int)cap;
    if (lim > 1024) lim = 1024;
    if (lim < 1) lim = 1;
    long best_cost = -1;
    int best = 1;
    for (int gx = 1; gx <= lim; ++gx) {
        const long cost = (long)cdiv(gx * col_tiles, slots) * cdiv(nrt, gx);
        if (best_cost < 0 || cost <= best_cost) {
            best_cost = cost;
            best = gx;
        }
    }
    return best;
}

// one split's partial weight gradient (9 ic mc floats) fits the partials region, and so does the repacked weight next to
// CONV_MIN_STAT_ROWS of the forward's statistics partial rows (2 M floats each)
constexpr size_t CONV_MIN_STAT_ROWS = 128;
bool conv_wgrad_row_fits(const TfnasCellDesc& d) {
    return 9 * (size_t)d.ic * d.g[0].mc <= TFNAS_PART_FLOATS &&
           conv_repack_floats(d) + CONV_MIN_STAT_ROWS * 2 * (size_t)d.M <= TFNAS_PART_FLOATS;
}

int launch_conv_fwd(const TfnasCellDesc& d, const float* x, float* D, double* stats2, float* part, hipStream_t s) {
    if (!cell_fused(d) || !x || !d.g[0].w_expand) return TFNAS_EINVAL;
    ProfScope _prof(TK_CONV_FWD, s);
    const int mm = gemm_mode_of(d), wide = d.g[0].mcp > 32;
    const int tiles = cdiv(d.g[0].mcp, wide ? 64 : 32);
    const size_t rpf = conv_repack_floats(d);
    if (!conv_wgrad_row_fits(d)) return TFNAS_ERANGE;      // (tfnas_cell_plan refused it: the repacked weight has its room)
    float* wrp = part + (TFNAS_PART_FLOATS - rpf);
    hipLaunchKernelGGL(k_conv_repack, dim3(cdiv((int)rpf, 1024)), dim3(256), 0, s, d, wrp, nullptr);
    size_t cap = (TFNAS_PART_FLOATS - rpf) / (2 * (size_t)d.M);  // the partial rows must fit, at most 1024 (k_reduce_rows)
    if (cap > 1024) cap = 1024;
    const dim3 grid(conv_row_blocks(d.N * d.Ho * d.Wo, tiles, cap, 256 * conv_lb(mm)), tiles);
    CONV_MM(mm, {
        if (wide) hipLaunchKernelGGL((k_conv_fwd<4, MM>), grid, dim3(256), 0, s, d, x, D, part, wrp);
        else hipLaunchKernelGGL((k_conv_fwd<2, MM>), grid, dim3(256), 0, s, d, x, D, part, wrp);
    })
    _prof.stop();
    return reduce_pair_rows(d, part, grid.x, stats2, s);       // (a FUSED group of a mixed cell: its own columns of stats2 only)
}

int launch_conv_dd(const TfnasCellDesc& d, const float* dZ, const float* D, const float* gate, const float* dpooled,
                   const double* stats2, const double* red2, float* dd, hipStream_t s) {
    if (!cell_fused(d)) return TFNAS_EINVAL;
    ProfScope _prof(TK_CONV_DD, s);
    const int Po = d.N * d.Ho * d.Wo, cy = cdiv(d.g[0].mcp, 64);
    int gx = cdiv(Po, 16);
    if (gx > 2048 / cy) gx = 2048 / cy > 0 ? 2048 / cy : 1;
    ACT_DISPATCH(d.act, {
        hipLaunchKernelGGL((k_conv_dd<ACT>), dim3(gx, cy), dim3(256), 0, s, d, dZ, D, gate, dpooled, stats2, red2, dd);
    })
    return (int)hipGetLastError();
}

int launch_conv_wgrad(const TfnasCellDesc& d, const float* dd, const float* x, float* part, hipStream_t s) {
    if (!cell_fused(d) || !d.g[0].g_expand) return TFNAS_EINVAL;
    if (!conv_wgrad_row_fits(d)) return TFNAS_ERANGE;
    ProfScope _prof(TK_CONV_WGRAD, s);
    static const int cands[] = {2, 3, 4};
    const int nc = 9 * d.ic, nt = pick_nt(nc, cands, 3), rows = d.N * d.Ho * d.Wo;
    const int mtiles = cdiv(d.g[0].mcp, 128), ztiles = cdiv(nc, 16 * nt);
    const size_t out = (size_t)nc * d.g[0].mc;
    // ONE resident round of workgroups, at least 128 pixels per split, the partial rows must fit (plan_row_splits' rule)
    int splits = 256 * conv_wgrad_lb(nt) / (mtiles * ztiles);
    if ((size_t)splits > TFNAS_PART_FLOATS / out) splits = (int)(TFNAS_PART_FLOATS / out);
    if (splits < 1) splits = 1;
    int rps = cdiv(rows, splits);
    if (rps < 128) rps = 128;
    rps = (rps + 15) / 16 * 16;
    splits = cdiv(rows, rps);
    const dim3 grid(splits, mtiles, ztiles);
    switch (nt) {
        case 2: hipLaunchKernelGGL((k_conv_wgrad<2>), grid, dim3(256), 0, s, d, dd, x, rps, part, out); break;
        case 3: hipLaunchKernelGGL((k_conv_wgrad<3>), grid, dim3(256), 0, s, d, dd, x, rps, part, out); break;
        default: hipLaunchKernelGGL((k_conv_wgrad<4>), grid, dim3(256), 0, s, d, dd, x, rps, part, out); break;
    }
    _prof.stop();
    return launch_reduce_rows(part, splits, (int)out, out, nullptr, d.g[0].g_expand, s, wgrad_accum(d));
}

int launch_conv_dgrad(const TfnasCellDesc& d, const float* dd, const float* dres, float* dx, float* part, hipStream_t s,
                      bool accum) {
    if (!cell_fused(d) || !dx || !d.g[0].w_expand) return TFNAS_EINVAL;
    ProfScope _prof(TK_CONV_DGRAD, s);
    const size_t rpf = conv_repack_floats(d);
    if (!conv_wgrad_row_fits(d)) return TFNAS_ERANGE;      // (tfnas_cell_plan refused it: the repacked weight has its room)
    float* wrp = part + (TFNAS_PART_FLOATS - rpf);
    hipLaunchKernelGGL(k_conv_repack, dim3(cdiv((int)rpf, 1024)), dim3(256), 0, s, d, nullptr, wrp);
    const int mm = gemm_mode_of(d), wide = d.ic > 32;
    const int tiles = cdiv(d.ic, wide ? 64 : 32);
    const dim3 grid(conv_row_blocks(d.N * d.H * d.W, tiles, 1024, 256 * conv_lb(mm)), tiles);
    CONV_MM(mm, {
        if (wide) hipLaunchKernelGGL((k_conv_dgrad<4, MM>), grid, dim3(256), 0, s, d, dd, dres, dx, wrp, (int)accum);
        else hipLaunchKernelGGL((k_conv_dgrad<2, MM>), grid, dim3(256), 0, s, d, dd, dres, dx, wrp, (int)accum);
    })
    return (int)hipGetLastError();
}
