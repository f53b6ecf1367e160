// Depthwise k x k convolution kernels (NHWC fp32) of the MBConv candidates, LDS-tiled.
//
// Reference arithmetic: depth_conv of MBInvertedResBlock (models/layers.py:484-507, forward :547):
//   Conv2d(mc, mc, k, stride, pad=k//2, groups=mc, bias=False) -> BN -> act
// The BN1+act that PRECEDES the depthwise conv is fused into the tile load (applied once per element,
// zero padding applied after it, exactly like conv padding of the activated tensor); the BN2 batch
// statistics of the conv output are accumulated in the epilogue.
//
// Work decomposition: a workgroup owns one chunk of CC channels of one group and walks over spatial tiles
// (persistent, grid-stride): the depthwise weights and BN constants of the chunk are staged in LDS once, the
// per-channel statistics are accumulated in registers across tiles and flushed with ONE set of double atomics
// per workgroup.  Threads are (channel-quad, strip) pairs; a strip is 4 consecutive pixels along W, so every
// LDS access is one ds_read_b128 of 4 channels and the k-wide sliding window lives in registers.  Tile loads
// are issued 4 at a time per thread before any of them is consumed (memory-level parallelism).
#include <cstring>
#include <type_traits>
#include "tfnas_dev.h"
#include "kernels.h"
#include "prof.h"
#include "efree.h"

__device__ __forceinline__ int floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// XCD-aware tile order.  Workgroup b is observed to run on XCD b % 8 and every XCD has a private L2; spatially
// adjacent tiles share halo pixels, so they should be in flight on the SAME XCD.  With gridDim.x a multiple of 8 the
// workgroups of XCD x take the contiguous tile range [x*gx/8, (x+1)*gx/8) of every grid-stride round (pure speed
// heuristic: any placement gives the same results).
__device__ __forceinline__ int xcd_first_tile() {
    const int gx = gridDim.x, bx = blockIdx.x;
    return (gx & 7) ? bx : (bx & 7) * (gx >> 3) + (bx >> 3);
}

// locate (group, first channel) of channel-chunk `cy` among the groups whose kernel size is K.  DIL = 0 (the register-window and
// ring kernels: never planned for a cell with a dilated group, dw_tile_only): the dilation is not looked at; DIL = 1 | 2 (the tile
// kernels): the groups of that kernel size AND that dilation (kernels.h: group_dil) -- one launch per (K, DIL) pair
template <int K, int DIL = 0>
__device__ __forceinline__ bool dw_locate(const TfnasCellDesc& d, int cy, int CC, int& g, int& c0) {
    for (g = 0; g < d.G; ++g) {
        if (d.g[g].k != K) continue;
        if (DIL != 0 && group_dil(d, g) != DIL) continue;
        const int t = (d.g[g].mcp + CC - 1) / CC;
        if (cy < t) {
            c0 = cy * CC;
            return true;
        }
        cy -= t;
    }
    return false;
}

// The channel chunk of a TILE kernel: a chunk of one SEGMENT (TFNAS_CELL_MIXK; a plain group is one segment: the group).  c0: its
// first channel in the group; mc / mcp: the segment's own end, min(4 Q_s+1, mc) and 4 Q_s+1 (kernels.h: seg_quad0) -- everything
// a tile kernel bounds by the group's width it bounds by these, because the overhanging lanes of a segment's last chunk are the
// NEXT segment's columns, written by another workgroup of another launch; cs: the segment's first channel and woff: the float
// offset of the segment's [mc_s][K * K] block in the group's packed depthwise weight (and in its block of the partial row).
struct DwSeg {
    int g, c0, mc, mcp, cs, woff;
};
// locate chunk `cy` among the segments whose kernel size is K, in group order then segment order (the host's twin: dw_chunks); a
// chunk never straddles a segment.  DIL = 1 | 2: the groups of that dilation (a packed group is never dilated).  All of it is
// wave-uniform (kernel arguments and blockIdx.y): scalar code.
template <int K, int DIL>
__device__ __forceinline__ bool dw_locate_seg(const TfnasCellDesc& d, int cy, int CC, DwSeg& sg) {
    for (int g = 0; g < d.G; ++g) {
        if (group_dil(d, g) != DIL) continue;
        const int n = group_nseg(d, g), q = d.g[g].mcp >> 2, mc = d.g[g].mc;
        int woff = 0;
        for (int s = 0; s < n; ++s) {
            const int ks = seg_k(d, g, s), lo = 4 * seg_quad0(q, n, s), hi = 4 * seg_quad0(q, n, s + 1);
            const int top = hi < mc ? hi : mc;
            if (ks == K) {
                const int t = (hi - lo + CC - 1) / CC;
                if (cy < t) {
                    sg = DwSeg{g, lo + cy * CC, top, hi, lo, woff};
                    return true;
                }
                cy -= t;
            }
            woff += (top - lo) * ks * ks;
        }
    }
    return false;
}

// sum the per-thread float4 partials of all threads that share a channel quad (tid % CQ) and store the CC
// per-channel totals as this workgroup's partial pair: acc[2*c + which] (acc = row blockIdx.x of the partials
// matrix, already offset to the group's first channel); k_reduce_rows sums the rows afterwards
__device__ __forceinline__ void dw_flush_pair(f32x4 a, f32x4 b, float* red, int CC, int c0, int mcp, float* acc,
                                              bool = false) {
    const int tid = threadIdx.x, CQ = CC >> 2;
    __syncthreads();
    st4(red + tid * 8, a);
    st4(red + tid * 8 + 4, b);
    __syncthreads();
    if (tid < CC && c0 + tid < mcp) {
        const int cq = tid >> 2, comp = tid & 3;
        float s = 0.f, q = 0.f;
        for (int t = cq; t < 256; t += CQ) {
            s += red[t * 8 + comp];
            q += red[t * 8 + 4 + comp];
        }
        acc[2 * (size_t)(c0 + tid) + 0] = s;
        acc[2 * (size_t)(c0 + tid) + 1] = q;
    }
}

// Statistics epilogue of the depthwise kernels: this workgroup's partial pair row (row `lane`); a k_reduce_rows / k_reduce_bn1
// launch sums the rows in double.  (Rounds 2-3 also had the producer's last workgroup sum them -- ticket counters + coherent
// read-back; measured no faster in two rounds and removed)
__device__ __forceinline__ void dw_flush_stats(f32x4 a, f32x4 b, float* lds, int CC, int c0, int mcp, int off, int M, float* part,
                                               int lane) {
    dw_flush_pair(a, b, lds, CC, c0, mcp, part + (size_t)lane * 2 * M + 2 * (size_t)off);
}

// (w: row 0 = channel `cs`, the first of the chunk's segment -- DwSeg; mc: the segment's end)
__device__ __forceinline__ void stage_weights(float* wts, const float* __restrict__ w, int KK, int CC, int c0, int mc, int cs = 0) {
    for (int idx = threadIdx.x; idx < KK * CC; idx += 256) {
        const int cl = idx % CC, t = idx / CC;
        wts[t * CC + cl] = (c0 + cl < mc) ? w[(size_t)(c0 + cl - cs) * KK + t] : 0.f;
    }
}

// Cooperative load of an [L0 x L1] pixel tile x CC channels into LDS (layout [pix][CC]).
// fetch(pix_row, pix_col, cq, ok) -> f32x4 is called only to build the value AFTER the raw loads were issued:
//   addr(r, c, cq, valid&) returns the element offset; xf(v, cq) transforms the loaded vector.
// two-source variant: both sources share the addressing; xf(v0, v1, cq) combines them (8 loads in flight)
template <class FAddr, class FXf>
__device__ __forceinline__ void load_tile2(float* tile, int L0, int L1, int CC, int cq_shift,
                                           const float* __restrict__ src0, const float* __restrict__ src1, FAddr addr,
                                           FXf xf) {
    const int CQ = CC >> 2, total = L0 * L1 * CQ;
    const float inv_l1 = 1.f / (float)L1;
    for (int base = 0; base < total; base += 1024) {
        f32x4 v0[4], v1[4];
        int pix[4], cqv[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = base + u * 256 + threadIdx.x;
            pix[u] = idx >> cq_shift;
            cqv[u] = idx & (CQ - 1);
            const int r = (int)(((float)pix[u] + 0.5f) * inv_l1);
            const int c = pix[u] - r * L1;
            size_t a = 0;
            ok[u] = idx < total && addr(r, c, cqv[u], a);
            v0[u] = ok[u] ? ld4_nt(src0 + a) : zero4();
            v1[u] = ok[u] ? ld4_nt(src1 + a) : zero4();
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = base + u * 256 + threadIdx.x;
            if (idx < total) st4(tile + pix[u] * CC + 4 * cqv[u], ok[u] ? xf(v0[u], v1[u], cqv[u]) : zero4());
        }
    }
}

template <class FAddr, class FXf>
__device__ __forceinline__ void load_tile(float* tile, int L0, int L1, int CC, int cq_shift, const float* __restrict__ src,
                                          FAddr addr, FXf xf) {
    const int CQ = CC >> 2, total = L0 * L1 * CQ;
    const float inv_l1 = 1.f / (float)L1;
    for (int base = 0; base < total; base += 1024) {
        f32x4 v[4];
        int pix[4], cqv[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = base + u * 256 + threadIdx.x;
            pix[u] = idx >> cq_shift;
            cqv[u] = idx & (CQ - 1);
            const int r = (int)(((float)pix[u] + 0.5f) * inv_l1);
            const int c = pix[u] - r * L1;
            size_t a = 0;
            ok[u] = idx < total && addr(r, c, cqv[u], a);
            v[u] = ok[u] ? ld4_nt(src + a) : zero4();
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = base + u * 256 + threadIdx.x;
            if (idx < total) st4(tile + pix[u] * CC + 4 * cqv[u], ok[u] ? xf(v[u], cqv[u]) : zero4());
        }
    }
}

// ============================================================================ forward
// KQ = 0: the tile is loaded from E.  KQ = ic/4 > 0 (E-free, efree.h): the tile is recomputed from the cell input x.
// RAW (TFNAS_CELL_NOEXPAND: a block without expand convolution, mc == ic): the tile is the cell input x itself, rows of ic floats,
// neither normalised nor activated -- no BN1 table is built or read (stats1 and E are not touched), ACT is unused (instantiated 0).
// DIL (TFNAS_CELL_DILATION): taps DIL pixels apart, padding DIL * (K / 2) -- the window covers KE = DIL * (K - 1) + 1 pixels each
// way, the tile origin moves out to ho0 * S - DIL * (K / 2), tap row ky is tile row oh * S + ky * DIL and tap kx of output j reads
// win[j * S + kx * DIL] of a 3 * S + KE wide register window (window entries no tap reads are never loaded: all indices are
// compile-time).  DIL = 2: K 3 | 5, KQ = 0 only.
template <int K, int S, int ACT, int KQ, bool RAW = false, int DIL = 1>
__global__ __launch_bounds__(256, 4) void k_dw_fwd(TfnasCellDesc d, const float* __restrict__ E,
                                                   const float* __restrict__ x,
                                                   const double* __restrict__ stats1, float* __restrict__ D,
                                                   float* __restrict__ part, DwGeom gm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int g, c0, lane = blockIdx.x, cy = blockIdx.y;
    static_assert(DIL == 1 || (DIL == 2 && KQ == 0 && (K == 3 || K == 5)), "dilation 2: 3 x 3 / 5 x 5 from E or raw x");
    if (KQ > 0) efree_lane_chunk(lane, cy);
    DwSeg sg;
    if constexpr (KQ > 0) {      // (E-free: never a packed group -- efree_supported)
        if (!dw_locate<K, DIL>(d, cy, gm.CC, g, c0)) return;
        sg = DwSeg{g, c0, d.g[g].mc, d.g[g].mcp, 0, 0};
    } else {
        if (!dw_locate_seg<K, DIL>(d, cy, gm.CC, sg)) return;
        g = sg.g, c0 = sg.c0;
    }
    const int mc = sg.mc, mcp = sg.mcp, off = d.g[g].off;      // (the SEGMENT's end: DwSeg)
    const int CC = gm.CC, CQ = CC >> 2, TH = gm.T0, TW = gm.T1;
    const int H = d.H, W = d.W, Ho = d.Ho, Wo = d.Wo, M = d.M;
    const int tid = threadIdx.x;
    const int IH = gm.L0, IW = gm.L1;

    const int tile_floats = max(IH * IW * CC, 2048);
    float* in_tile = lds;
    float* wts = lds + tile_floats;
    float2* cst = reinterpret_cast<float2*>(wts + K * K * CC);

    if constexpr (!RAW) {
    if (tid < CC)
        cst[tid] = (c0 + tid < mc) ? bn_consts(stats1 + 2 * (size_t)(off + c0 + tid), 1.0 / ((double)d.N * H * W), d.eps)
                                   : make_float2(0.f, 0.f);
    }
    stage_weights(wts, d.g[g].w_dw + sg.woff, K * K, CC, c0, mc, sg.cs);
    ExpandB<(KQ > 0 ? KQ : 2)> xb;
    if (KQ > 0) {
        __syncthreads();
        expand_b_load(xb, d.g[g].w_expand, d.ic, c0, mc, cst);
    }

    constexpr int KE = DIL * (K - 1) + 1, WIN = 3 * S + KE;
    const int nsw = TW >> 2, nstrips = TH * nsw;
    f32x4 ssum = zero4(), ssq = zero4();
    for (int t = KQ > 0 ? lane : xcd_first_tile(); t < gm.ntiles; t += gridDim.x) {
        const int tw = t % gm.tilesW, th = (t / gm.tilesW) % gm.tilesH, n = t / (gm.tilesW * gm.tilesH);
        const int ho0 = th * TH, wo0 = tw * TW;
        const int hi0 = ho0 * S - DIL * (K / 2), wi0 = wo0 * S - DIL * (K / 2);
        __syncthreads();     // previous tile fully consumed (and cst/wts visible on the first pass)
        if (KQ > 0) {
            const float inv_iw = 1.f / (float)IW;
            expand_tile<(KQ > 0 ? KQ : 2), ACT>(in_tile, IH * IW, CC, x, xb, [&](int p, size_t& a) {
                const int r = (int)(((float)p + 0.5f) * inv_iw), c = p - r * IW;
                const int hi = hi0 + r, wi = wi0 + c;
                a = ((size_t)(n * H + hi) * W + wi) * d.ic;
                return hi >= 0 && hi < H && wi >= 0 && wi < W;
            });
        } else if constexpr (RAW) {
            load_tile(in_tile, IH, IW, CC, gm.cq_shift, x,
                      [&](int r, int c, int cq, size_t& a) {
                          const int hi = hi0 + r, wi = wi0 + c;
                          a = ((size_t)(n * H + hi) * W + wi) * d.ic + c0 + 4 * cq;
                          return hi >= 0 && hi < H && wi >= 0 && wi < W && c0 + 4 * cq < mcp;
                      },
                      [&](f32x4 v, int) { return v; });
        } else
        load_tile(in_tile, IH, IW, CC, gm.cq_shift, E,
                  [&](int r, int c, int cq, size_t& a) {
                      const int hi = hi0 + r, wi = wi0 + c;
                      a = ((size_t)(n * H + hi) * W + wi) * M + off + c0 + 4 * cq;
                      return hi >= 0 && hi < H && wi >= 0 && wi < W && c0 + 4 * cq < mcp;
                  },
                  [&](f32x4 v, int cq) {
#pragma unroll
                      for (int j = 0; j < 4; ++j) {
                          const float2 c = cst[4 * cq + j];
                          v[j] = act_f<ACT>((v[j] - c.x) * c.y);
                      }
                      return v;
                  });
        __syncthreads();
        for (int item = tid; item < nstrips * CQ; item += 256) {
            const int cq = item & (CQ - 1), st = item >> gm.cq_shift;
            const int oh = st / nsw, ow0 = (st - oh * nsw) * 4;
            f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
#pragma unroll 1
            for (int ky = 0; ky < K; ++ky) {
                const float* rowp = in_tile + ((oh * S + ky * DIL) * IW + ow0 * S) * CC + 4 * cq;
                const float* wp = wts + ky * K * CC + 4 * cq;
                f32x4 win[WIN];
#pragma unroll
                for (int u = 0; u < WIN; ++u) win[u] = ld4(rowp + u * CC);
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const f32x4 wv = ld4(wp + kx * CC);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] += win[j * S + kx * DIL] * wv;
                }
            }
            const int ho = ho0 + oh;
            if (ho < Ho && c0 + 4 * cq < mcp) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int wo = wo0 + ow0 + j;
                    if (wo < Wo) {
                        st4_nt(D + (((size_t)(n * Ho + ho) * Wo + wo) * M + off + c0 + 4 * cq), acc[j]);
                        ssum += acc[j];
                        ssq += acc[j] * acc[j];
                    }
                }
            }
        }
    }
    dw_flush_stats(ssum, ssq, in_tile, CC, c0, mcp, off, M, part, lane);
}

// (the BN2-backward operand dd of a depthwise output element -- bn2_dd, fill_cst2 -- is in tfnas_dev.h: the dense
//  convolution of conv_kernels.hip forms it the same way)

// ============================================================================ backward w.r.t. input
// dA1[n][hi][wi][c] = sum_{ky,kx} dd[n][(hi+p-ky)/S][(wi+p-kx)/S][c] * w[c][ky][kx]   (only exact divisions)
// epilogue: deh = dA1 * act'(ehat) -> dEh, and the BN1-backward sums (T1 = sum deh, T2 = sum deh*ehat)
// KQ > 0 (E-free, efree.h): ehat of the tile's input pixels is recomputed from x into a second LDS tile instead of
// being read from E.
// RAW (TFNAS_CELL_NOEXPAND, mc == ic): the depthwise input is the cell input, so dA1 IS the branch's dx.  The epilogue stores it to
// `dEh` = dx [N*H*W][ic] (row stride ic), plus `x` = the residual gradient dout [N*H*W][ic] when non-NULL (has_res: oc == ic,
// stride 1), in the same store.  No BN1-backward sums: E, stats1 and `part` are not touched.  dx_accum: dx already holds the data
// gradient of the cell's earlier branches (a mixed cell) and the same store adds it -- read and written by the one thread that
// owns the element, its load issued with the residual's before the tap loop.
// DIL: PAD = DIL * (K / 2) and tap (ky, kx) of input (hi, wi) reads output ((hi + PAD - ky * DIL) / S, (wi + PAD - kx * DIL) / S).
// Stride 2 with DIL = 2: PAD and every tap offset are even, so only even input rows and columns receive anything -- the odd
// pixels pass the parity tests of no tap, keep acc = 0 and are STORED as zero like every other element of the tile (dEh, and the dx
// of the RAW form, are written everywhere the pass owns).
template <int K, int S, int ACT, int KQ, bool RAW = false, int DIL = 1>
__global__ __launch_bounds__(256, 4) void k_dw_bwd_data(TfnasCellDesc d, const float* __restrict__ dZ,
                                                        const float* __restrict__ gate, const float* __restrict__ dpooled,
                                                        const float* __restrict__ D, const double* __restrict__ stats2,
                                                        const double* __restrict__ red2, const float* __restrict__ E,
                                                        const float* __restrict__ x,
                                                        const double* __restrict__ stats1, float* __restrict__ dEh,
                                                        float* __restrict__ part, DwGeom gm, int dx_accum) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int g, c0, lane = blockIdx.x, cy = blockIdx.y;
    static_assert(DIL == 1 || (DIL == 2 && KQ == 0 && (K == 3 || K == 5)), "dilation 2: 3 x 3 / 5 x 5 from E or raw x");
    if (KQ > 0) efree_lane_chunk(lane, cy);
    DwSeg sg;
    if constexpr (KQ > 0) {      // (E-free: never a packed group -- efree_supported)
        if (!dw_locate<K, DIL>(d, cy, gm.CC, g, c0)) return;
        sg = DwSeg{g, c0, d.g[g].mc, d.g[g].mcp, 0, 0};
    } else {
        if (!dw_locate_seg<K, DIL>(d, cy, gm.CC, sg)) return;
        g = sg.g, c0 = sg.c0;
    }
    const int mc = sg.mc, mcp = sg.mcp, off = d.g[g].off;      // (the SEGMENT's end: DwSeg)
    const int CC = gm.CC, CQ = CC >> 2, TIH = gm.T0, TIW = gm.T1;
    const int H = d.H, W = d.W, Ho = d.Ho, Wo = d.Wo, M = d.M;
    constexpr int PAD = DIL * (K / 2), KE = DIL * (K - 1) + 1;
    const int tid = threadIdx.x;
    const int OH = gm.L0, OW = gm.L1;      // LDS tile extent (host: worst case over tile origins)

    const int tile_floats = max(OH * OW * CC, 2048);
    float* dd_tile = lds;
    float* wts = lds + tile_floats;
    f32x4* cst2 = reinterpret_cast<f32x4*>(wts + K * K * CC);
    float2* cst1 = reinterpret_cast<float2*>(cst2 + CC);

    fill_cst2(cst2, d, CC, c0, mc, off, stats2, red2);
    if constexpr (!RAW) {
    if (tid < CC)
        cst1[tid] = (c0 + tid < mc) ? bn_consts(stats1 + 2 * (size_t)(off + c0 + tid), 1.0 / ((double)d.N * H * W), d.eps)
                                    : make_float2(0.f, 0.f);
    }
    stage_weights(wts, d.g[g].w_dw + sg.woff, K * K, CC, c0, mc, sg.cs);
    float* eh_tile = reinterpret_cast<float*>(cst1 + CC);     // [TIH*TIW][CC] (E-free only)
    ExpandB<(KQ > 0 ? KQ : 2)> xb;
    if (KQ > 0) {
        __syncthreads();
        expand_b_load(xb, d.g[g].w_expand, d.ic, c0, mc, cst1);
    }

    const int nsw = TIW >> 2, nstrips = TIH * nsw;
    const bool has_se = d.g[g].se > 0;
    const float inv_hw = 1.f / (float)(Ho * Wo);
    f32x4 t1 = zero4(), t2 = zero4();
    for (int t = KQ > 0 ? lane : xcd_first_tile(); t < gm.ntiles; t += gridDim.x) {
        const int tw = t % gm.tilesW, th = (t / gm.tilesW) % gm.tilesH, n = t / (gm.tilesW * gm.tilesH);
        const int hi0 = th * TIH, wi0 = tw * TIW;
        const int oh0 = floordiv(hi0 + PAD - (KE - 1), S), ow0 = floordiv(wi0 + PAD - (KE - 1), S);
        __syncthreads();
        // this thread always stages the same channel quad (256 % CQ == 0): its SE gate / pool-path terms of image n
        const int mycq = tid & (CQ - 1);
        f32x4 g4 = zero4(), dp4 = zero4();
        if (has_se && c0 + 4 * mycq < mcp) {
            g4 = ld4(gate + (size_t)n * M + off + c0 + 4 * mycq);
            dp4 = ld4(dpooled + (size_t)n * M + off + c0 + 4 * mycq) * splat4(inv_hw);
        }
        load_tile2(dd_tile, OH, OW, CC, gm.cq_shift, dZ, D,
                   [&](int r, int c, int cq, size_t& a) {
                       const int ho = oh0 + r, wo = ow0 + c;
                       a = ((size_t)(n * Ho + ho) * Wo + wo) * M + off + c0 + 4 * cq;
                       return ho >= 0 && ho < Ho && wo >= 0 && wo < Wo && c0 + 4 * cq < mcp;
                   },
                   [&](f32x4 v, f32x4 dv, int cq) { return bn2_dd<ACT>(cst2, 4 * cq, v, dv, has_se, g4, dp4); });
        if (KQ > 0) {
            const float inv_iw = 1.f / (float)TIW;
            expand_tile<(KQ > 0 ? KQ : 2), 2>(eh_tile, TIH * TIW, CC, x, xb, [&](int p, size_t& a) {
                const int r = (int)(((float)p + 0.5f) * inv_iw), c = p - r * TIW;
                const int hi = hi0 + r, wi = wi0 + c;
                a = ((size_t)(n * H + hi) * W + wi) * d.ic;
                return hi < H && wi < W;
            });
        }
        __syncthreads();

        for (int item = tid; item < nstrips * CQ; item += 256) {
            const int cq = item & (CQ - 1), st = item >> gm.cq_shift;
            // stride 2: which taps reach an input row depends on the row's parity, and a wave holds the strips of 2-4
            // consecutive rows -- in natural order half of its lanes sat out every ky iteration of the tap loop.  Rows are
            // therefore dealt even-first (0, 2, 4, .., 1, 3, ..): the rows of a wave share their parity.
            const int ihp = st / nsw, iw0 = (st - ihp * nsw) * 4;
            const int half = (TIH + 1) >> 1;
            const int ih = (S == 2) ? (ihp < half ? 2 * ihp : 2 * (ihp - half) + 1) : ihp;
            const int hi = hi0 + ih;
            f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
            // issue the epilogue's E loads now so that their latency hides under the tap loop
            f32x4 ev[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int wi = wi0 + iw0 + j;
                const bool okj = hi < H && wi < W && c0 + 4 * cq < mcp;
                if constexpr (RAW) {      // the residual gradient of the same dx element (x: dout of a residual block, else NULL)
                    const size_t a = ((size_t)(n * H + hi) * W + wi) * d.ic + c0 + 4 * cq;
                    ev[j] = (okj && x) ? ld4_nt(x + a) : zero4();
                    if (okj && dx_accum) ev[j] += ld4_nt(dEh + a);
                }
                else if (KQ > 0) ev[j] = ld4(eh_tile + (ih * TIW + iw0 + j) * CC + 4 * cq);
                else ev[j] = okj ? ld4_nt(E + (((size_t)(n * H + hi) * W + wi) * M + off + c0 + 4 * cq)) : zero4();
            }
            if (S == 1) {
                // column of output (wi + PAD - kx * DIL) relative to ow0 = wi0 + PAD - (KE-1):  iw0 + j - kx * DIL + KE - 1
#pragma unroll 1
                for (int ky = 0; ky < K; ++ky) {
                    const int r = hi + PAD - ky * DIL - oh0;
                    const float* rowp = dd_tile + (r * OW + iw0) * CC + 4 * cq;
                    const float* wp = wts + ky * K * CC + 4 * cq;
                    f32x4 win[KE + 3];
#pragma unroll
                    for (int u = 0; u < KE + 3; ++u) win[u] = ld4(rowp + u * CC);
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        const f32x4 wv = ld4(wp + kx * CC);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j] += win[j - kx * DIL + KE - 1] * wv;
                    }
                }
            } else {
                const int base = wi0 + iw0;   // multiple of 4 -> even
#pragma unroll 1
                for (int ky = 0; ky < K; ++ky) {
                    const int tt = hi + PAD - ky * DIL;
                    if (tt & 1) continue;
                    const int r = tt / 2 - oh0;   // tt even: exact also for negatives
                    const float* wp = wts + ky * K * CC + 4 * cq;
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        const f32x4 wv = ld4(wp + kx * CC);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if ((j + PAD - kx * DIL) & 1) continue;   // compile-time after unrolling
                            const int c = base / 2 + (j + PAD - kx * DIL) / 2 - ow0;
                            acc[j] += ld4(dd_tile + (r * OW + c) * CC + 4 * cq) * wv;
                        }
                    }
                }
            }
            if (hi < H && c0 + 4 * cq < mcp) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int wi = wi0 + iw0 + j;
                    if (wi < W) {
                        if constexpr (RAW) {
                            st4_nt(dEh + (((size_t)(n * H + hi) * W + wi) * d.ic + c0 + 4 * cq), acc[j] + ev[j]);
                        } else {
                        const size_t a = ((size_t)(n * H + hi) * W + wi) * M + off + c0 + 4 * cq;
                        const f32x4 e = ev[j];
                        f32x4 deh;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float2 c = cst1[4 * cq + q];
                            const float eh = KQ > 0 ? e[q] : (e[q] - c.x) * c.y;
                            deh[q] = acc[j][q] * act_d<ACT>(eh);
                            t1[q] += deh[q];
                            t2[q] += deh[q] * eh;
                        }
                        st4_nt(dEh + a, deh);
                        }
                    }
                }
            }
        }
    }
    if constexpr (!RAW) dw_flush_stats(t1, t2, dd_tile, CC, c0, mcp, off, M, part, lane);
}

// ============================================================================ weight gradient
// part[bx][poff_g + c*K*K + ky*K + kx] = sum over this workgroup's tiles of dd[n][ho][wo][c] * a1[n][ho*S+ky-p][wo*S+kx-p][c]
// (a1 = act(BN1(E))); k_reduce_rows sums the workgroups into g_dw
// KR: tap rows of one workgroup.  KR = K (3 x 3, 5 x 5): all of them.  7 x 7: 49 float4 accumulators are 196 registers before the
// 13-wide window and the operands, past the 256 that two workgroups per CU leave a thread, so the rows are split over blockIdx.z
// (KR = 4: rows 0-3 and 4-6, 28 and 21 accumulators); each part stages the tile itself and writes its own K * KR-float slice of
// every channel's K * K block of the partial row.
// (KY0, KR as template arguments: tap rows [KY0, KY0 + KR) with every accumulator index a compile-time constant)
// RAW (TFNAS_CELL_NOEXPAND): a1 is the cell input itself -- `E` = x [N*H*W][ic], row stride ic; stats1 is not touched.
// DIL: as in k_dw_fwd (a1 at [ho*S + ky*DIL - DIL*p][wo*S + kx*DIL - DIL*p]); the partial row keeps its mc * K * K layout.
template <int K, int S, int ACT, int KY0, int KR, bool RAW, int DIL>
__device__ __forceinline__ void dw_wgrad_rows(const TfnasCellDesc& d, const float* __restrict__ dZ,
                                              const float* __restrict__ gate, const float* __restrict__ dpooled,
                                              const float* __restrict__ D, const double* __restrict__ stats2,
                                              const double* __restrict__ red2, const float* __restrict__ E,
                                              const double* __restrict__ stats1, float* __restrict__ part,
                                              size_t out_size, const DwGeom& gm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    DwSeg sg;
    if (!dw_locate_seg<K, DIL>(d, blockIdx.y, gm.CC, sg)) return;
    const int g = sg.g, c0 = sg.c0;
    const int mc = sg.mc, mcp = sg.mcp, off = d.g[g].off;      // (the SEGMENT's end: DwSeg)
    size_t poff = sg.woff;                                     // (the segment's block inside the group's block of the row)
    for (int gg = 0; gg < g; ++gg) poff += group_dw_floats(d, gg);
    float* __restrict__ gw = part + (size_t)blockIdx.x * out_size + poff;
    const int CC = gm.CC, CQ = CC >> 2, TH = gm.T0, TW = gm.T1;
    const int H = d.H, W = d.W, Ho = d.Ho, Wo = d.Wo, M = d.M;
    const int tid = threadIdx.x;
    const int IH = gm.L0, IW = gm.L1;

    const int tile_floats = max(IH * IW * CC, 4 * KR * K * CC);
    float* in_tile = lds;
    f32x4* cst2 = reinterpret_cast<f32x4*>(lds + tile_floats);
    float2* cst1 = reinterpret_cast<float2*>(cst2 + CC);

    fill_cst2(cst2, d, CC, c0, mc, off, stats2, red2);
    if constexpr (!RAW) {
    if (tid < CC)
        cst1[tid] = (c0 + tid < mc) ? bn_consts(stats1 + 2 * (size_t)(off + c0 + tid), 1.0 / ((double)d.N * H * W), d.eps)
                                    : make_float2(0.f, 0.f);
    }

    constexpr int KE = DIL * (K - 1) + 1, WIN = 3 * S + KE;
    const int nsw = TW >> 2, nstrips = TH * nsw;
    const bool has_se = d.g[g].se > 0;
    const float inv_hw = 1.f / (float)(Ho * Wo);
    f32x4 wacc[KR * K];
#pragma unroll
    for (int u = 0; u < KR * K; ++u) wacc[u] = zero4();
    for (int t = xcd_first_tile(); t < gm.ntiles; t += gridDim.x) {
        const int tw = t % gm.tilesW, th = (t / gm.tilesW) % gm.tilesH, n = t / (gm.tilesW * gm.tilesH);
        const int ho0 = th * TH, wo0 = tw * TW;
        const int hi0 = ho0 * S - DIL * (K / 2), wi0 = wo0 * S - DIL * (K / 2);
        const int mycq = tid & (CQ - 1);
        f32x4 g4 = zero4(), dp4 = zero4();
        if (has_se && c0 + 4 * mycq < mcp) {
            g4 = ld4(gate + (size_t)n * M + off + c0 + 4 * mycq);
            dp4 = ld4(dpooled + (size_t)n * M + off + c0 + 4 * mycq) * splat4(inv_hw);
        }
        // The (dZ, D) operands of this thread's FIRST item of the tile are requested before the E tile is staged: both are
        // plain global loads with ~2 us of latency at 2 waves per SIMD, and a tile has one item per thread (T0*T1/4 strips x CQ
        // = 256), so without this the two latencies were paid one after the other for every tile.
        const int nitems = nstrips * CQ;
        auto item_ops = [&](int item, f32x4 (&dd)[4], f32x4 (&dv)[4], bool (&ok)[4]) {
            const int cq = item & (CQ - 1), st = item >> gm.cq_shift;
            const int oh = st / nsw, ow0 = (st - oh * nsw) * 4;
            const int ho = ho0 + oh;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int wo = wo0 + ow0 + j;
                ok[j] = ho < Ho && wo < Wo && c0 + 4 * cq < mcp;
                const size_t a = ((size_t)(n * Ho + ho) * Wo + wo) * M + off + c0 + 4 * cq;
                dd[j] = ok[j] ? ld4_nt(dZ + a) : zero4();
                dv[j] = ok[j] ? ld4_nt(D + a) : zero4();
            }
        };
        // (KR < K: the accumulators leave no registers to hold them across the staging)
        constexpr bool PF = KR == K;       // (one part)
        f32x4 pdd[PF ? 4 : 1], pdv[PF ? 4 : 1];
        bool pok[4] = {false, false, false, false};
        if constexpr (PF) {
            if (tid < nitems) item_ops(tid, pdd, pdv, pok);
        }
        __syncthreads();
        if constexpr (RAW) {
            load_tile(in_tile, IH, IW, CC, gm.cq_shift, E,
                      [&](int r, int c, int cq, size_t& a) {
                          const int hi = hi0 + r, wi = wi0 + c;
                          a = ((size_t)(n * H + hi) * W + wi) * d.ic + c0 + 4 * cq;
                          return hi >= 0 && hi < H && wi >= 0 && wi < W && c0 + 4 * cq < mcp;
                      },
                      [&](f32x4 v, int) { return v; });
        } else
        load_tile(in_tile, IH, IW, CC, gm.cq_shift, E,
                  [&](int r, int c, int cq, size_t& a) {
                      const int hi = hi0 + r, wi = wi0 + c;
                      a = ((size_t)(n * H + hi) * W + wi) * M + off + c0 + 4 * cq;
                      return hi >= 0 && hi < H && wi >= 0 && wi < W && c0 + 4 * cq < mcp;
                  },
                  [&](f32x4 v, int cq) {
#pragma unroll
                      for (int j = 0; j < 4; ++j) {
                          const float2 c = cst1[4 * cq + j];
                          v[j] = act_f<ACT>((v[j] - c.x) * c.y);
                      }
                      return v;
                  });
        __syncthreads();
        for (int item = tid; item < nitems; item += 256) {
            const int cq = item & (CQ - 1), st = item >> gm.cq_shift;
            const int oh = st / nsw, ow0 = (st - oh * nsw) * 4;
            f32x4 dd[4], dv[4];
            bool ok[4];
            if constexpr (PF) {
                if (item == tid) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        dd[j] = pdd[j];
                        dv[j] = pdv[j];
                        ok[j] = pok[j];
                    }
                } else {
                    item_ops(item, dd, dv, ok);
                }
            } else {
                item_ops(item, dd, dv, ok);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) dd[j] = ok[j] ? bn2_dd<ACT>(cst2, 4 * cq, dd[j], dv[j], has_se, g4, dp4) : zero4();
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const float* rowp = in_tile + ((oh * S + (KY0 + r) * DIL) * IW + ow0 * S) * CC + 4 * cq;
                f32x4 win[WIN];
#pragma unroll
                for (int u = 0; u < WIN; ++u) win[u] = ld4(rowp + u * CC);
#pragma unroll
                for (int kx = 0; kx < K; ++kx)
#pragma unroll
                    for (int j = 0; j < 4; ++j) wacc[r * K + kx] += dd[j] * win[j * S + kx * DIL];
            }
        }
    }
    // reduce over the threads sharing a channel quad: first inside the wave, then across the 4 waves
    for (int o = CQ; o < 64; o <<= 1) {
#pragma unroll
        for (int u = 0; u < KR * K; ++u) {
#pragma unroll
            for (int q = 0; q < 4; ++q) wacc[u][q] += __shfl_xor(wacc[u][q], o, 64);
        }
    }
    __syncthreads();
    float* wred = in_tile;   // [4 waves][KR*K][CC]
    const int lane = tid & 63, wv = tid >> 6;
    if (lane < CQ) {
#pragma unroll
        for (int u = 0; u < KR * K; ++u) st4(wred + (wv * KR * K + u) * CC + 4 * lane, wacc[u]);
    }
    __syncthreads();
    for (int idx = tid; idx < KR * K * CC; idx += 256) {
        const int cl = idx % CC, u = idx / CC;
        if (c0 + cl < mc) {
            float s = 0.f;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) s += wred[(ww * KR * K + u) * CC + cl];
            gw[(size_t)(c0 + cl - sg.cs) * (K * K) + KY0 * K + u] = s;
        }
    }
}
template <int K, int S, int ACT, int KR = K, bool RAW = false, int DIL = 1>
__global__ __launch_bounds__(256, 2) void k_dw_wgrad(TfnasCellDesc d, const float* __restrict__ dZ,
                                                     const float* __restrict__ gate, const float* __restrict__ dpooled,
                                                     const float* __restrict__ D, const double* __restrict__ stats2,
                                                     const double* __restrict__ red2, const float* __restrict__ E,
                                                     const double* __restrict__ stats1, float* __restrict__ part,
                                                     size_t out_size, DwGeom gm) {
    static_assert(KR == K || (KR < K && 2 * KR >= K), "one part, or two over blockIdx.z");
    static_assert(DIL == 1 || (DIL == 2 && (K == 3 || K == 5)), "dilation 2: 3 x 3 / 5 x 5");
    if constexpr (KR == K) {
        dw_wgrad_rows<K, S, ACT, 0, K, RAW, DIL>(d, dZ, gate, dpooled, D, stats2, red2, E, stats1, part, out_size, gm);
    } else if (blockIdx.z == 0) {
        dw_wgrad_rows<K, S, ACT, 0, KR, RAW, DIL>(d, dZ, gate, dpooled, D, stats2, red2, E, stats1, part, out_size, gm);
    } else {
        dw_wgrad_rows<K, S, ACT, KR, K - KR, RAW, DIL>(d, dZ, gate, dpooled, D, stats2, red2, E, stats1, part, out_size, gm);
    }
}

#include "dw_stream.inc"
#include "dw_direct.inc"

// ============================================================================ host side
// One planner per pass (dw_plan_fwd, dw_plan_bwd_data, dw_plan_wgrad) picks the kernel family and computes its geometry; the
// launchers below only carry the plan out.  Families in order of preference, each one falling through to the next:
//   1. register-window kernels (dw_direct.inc) where the measured policy dwd_*_use picks them and dwd_plan finds a grid;
//   2. LDS ring kernels (dw_stream.inc) unless the route asks for tiles, where the ring fits (stride 1); E-free only for
//      ic 24 / 40 (dws_efree_ic);
//   3. LDS tile kernels (above).
// TfnasCellDesc.route, TFNAS_ROUTE_DW_*: 0 per launch, whichever kernel measured faster | 1 register-window kernels wherever the
// geometry allows | 2 ring / tile kernels only | 3 tile kernels only: every choice is compared with the oracle
// (tests/test_gpu_cell.py::test_variant_against_oracle)

// channel chunks of the groups with kernel size K and dilation dil (the kernels' twin: dw_locate)
// -- in segments (TFNAS_CELL_MIXK, dw_locate_seg): a plain group is one segment of mcp channels, a packed group hands each of its
// segments to the slot of that segment's kernel size
static int dw_chunks(const TfnasCellDesc& d, int K, int CC, int dil = 1) {
    int t = 0;
    for (int g = 0; g < d.G; ++g) {
        if (group_dil(d, g) != dil) continue;
        const int n = group_nseg(d, g), q = d.g[g].mcp >> 2;
        for (int s = 0; s < n; ++s)
            if (seg_k(d, g, s) == K) t += cdiv(4 * (seg_quad0(q, n, s + 1) - seg_quad0(q, n, s)), CC);
    }
    return t;
}
// the (kernel size, dilation) pair of launch slot i of a pass (kernels.h: DW_NK): 3, 5, 7 undilated, then 3 and 5 with dilation 2
static int dw_slot_k(int i) { return i < 3 ? 3 + 2 * i : 3 + 2 * (i - 3); }
static int dw_slot_dil(int i) { return i < 3 ? 1 : 2; }

// floats of one weight-gradient partial row: the groups' mc x K x K blocks in group order
static size_t dw_wout_size(const TfnasCellDesc& d) {
    size_t n = 0;
    for (int g = 0; g < d.G; ++g) n += group_dw_floats(d, g);       // (a packed group: the sum over its segments)
    return n;
}

// a group with a kernel size other than 3 / 5 (that is 7: tfnas_cell_plan).  The register-window and the ring kernels hold K x K
// taps or accumulators in registers and are built for 3 and 5 only: such a cell takes the tile kernels in every pass, whatever
// TFNAS_ROUTE_DW_* asks, never fuses the weight gradient into the backward-data pass, and always has E (efree_supported).
// The same holds for a cell with TFNAS_ACT_RELU6 / TFNAS_ACT_HSWISH: only the tile kernels are instantiated for them, and for a
// cell without expand convolution (TFNAS_CELL_NOEXPAND): only the tile kernels have the raw-input form; and for a cell with a
// dilated group (TFNAS_CELL_DILATION): only the tile kernels have the tap spacing as a template argument.
static bool dw_tile_only(const TfnasCellDesc& d) {
    if (act_tile_only(d.act) || cell_noexpand(d) || cell_dilated(d) || cell_packed(d)) return true;     // (packed: segments)
    for (int g = 0; g < d.G; ++g)
        if (d.g[g].k != 3 && d.g[g].k != 5) return true;
    return false;
}
// the weight-gradient partial row (with 7 x 7 groups up to mc x 49 floats each) must fit the partials region at least once:
// otherwise the descriptor is refused (tfnas_cell_plan, tfnas_cell_ws, launch_dw_wgrad).  Eight groups of 1536 channels at
// 7 x 7 -- the elasticity bound -- are 602 112 floats: 6 rows.
bool dw_wgrad_row_fits(const TfnasCellDesc& d) { return dw_wout_size(d) <= TFNAS_PART_FLOATS; }

// every group has kernel size 3 (or 5 where k5 is set)
static bool dw_groups_k(const TfnasCellDesc& d, bool k5) {
    if (cell_packed(d)) return false;     // (a packed word is not a kernel size: never a fused weight gradient)
    for (int g = 0; g < d.G; ++g)
        if (d.g[g].k != 3 && !(k5 && d.g[g].k == 5)) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------- tile kernels
// force32: the E-free producer (efree.h) works on 32-channel chunks
// K: the EFFECTIVE extent of the taps, dil * (k - 1) + 1 -- all the tile geometry knows of a kernel size is the halo.  The two
// dilated extents, 5 and 9: 5 has the geometry of a 5 x 5; 9 lands in the 16-channel regime of the 7 x 7 at stride 2 forward
// (15 x 39 pixels x 32 channels = 73 KB) and stays at 32 channels at stride 1 backward (17 x 25 pixels x 32 channels = 53.1 KB,
// under the 56 KB switch; 57.0 KB with the taps and the constant tables) -- every launcher checks its total against 64 KB.
static void pick_tile(int N, int Th, int Tw, int K, int S, bool fwd_like, DwGeom& gm, bool force32) {
    // T1 (width) multiple of 4 (strips), up to 16; T0 so that a tile has ~128 (64 for stride 2) pixels
    gm.T1 = Tw >= 16 ? 16 : ((Tw + 3) / 4) * 4;
    const int target = (S == 2 && fwd_like) ? 64 : 128;
    gm.T0 = target / gm.T1;
    if (gm.T0 > Th) gm.T0 = Th;
    if (gm.T0 < 1) gm.T0 = 1;
    gm.tilesH = cdiv(Th, gm.T0);
    gm.tilesW = cdiv(Tw, gm.T1);
    gm.ntiles = N * gm.tilesH * gm.tilesW;
    if (fwd_like) {
        gm.L0 = (gm.T0 - 1) * S + K;
        gm.L1 = (gm.T1 - 1) * S + K;
    } else {
        gm.L0 = (gm.T0 + K - 2) / S + 2;      // worst case over tile origins of floor((a+T+K-2)/S)-floor(a/S)+1
        gm.L1 = (gm.T1 + K - 2) / S + 2;
    }
    const int px = gm.L0 * gm.L1;
    const int items32 = gm.T0 * (gm.T1 / 4) * 8;
    gm.CC = 32;
    if (px * 32 * 4 > 56 * 1024) gm.CC = 16;
    else if (items32 < 192 && px * 64 * 4 <= 40 * 1024) gm.CC = 64;
    if (force32) gm.CC = 32;
    gm.cq_shift = gm.CC == 16 ? 2 : gm.CC == 32 ? 3 : 4;
}

static int dw_grid_x(const DwGeom& gm, int chunks, int target_blocks) {
    int gx = cdiv(target_blocks, chunks);
    if (gx > gm.ntiles) gx = gm.ntiles;
    return gx < 1 ? 1 : gx;
}

// Tiles of Th x Tw (outputs for fwd_like, inputs otherwise).  The launches of one pass (3, 5, 7, dilated 3, dilated 5) share grid.x
// so that they fill the same rows of the partials matrix.
static void dw_tile_plan(const TfnasCellDesc& d, int Th, int Tw, bool fwd_like, int target_blocks, size_t row_floats,
                         bool force32, DwPlan& p) {
    int gx = 1 << 30;
    for (int i = 0; i < DW_NK; ++i) {
        const int kk = dw_slot_k(i), dil = dw_slot_dil(i);
        pick_tile(d.N, Th, Tw, dil * (kk - 1) + 1, d.stride, fwd_like, p.tile[i], force32);
        p.chunks[i] = dw_chunks(d, kk, p.tile[i].CC, dil);
        if (!p.chunks[i]) continue;
        const int g1 = dw_grid_x(p.tile[i], p.chunks[i], target_blocks);
        if (g1 < gx) gx = g1;
    }
    const size_t cap = TFNAS_PART_FLOATS / (row_floats ? row_floats : 1);
    if ((size_t)gx > cap) gx = (int)cap;
    if (gx > 1024) gx = 1024;                      // partial rows to reduce afterwards
    if (gx >= 8) gx &= ~7;                         // multiple of 8 for the XCD-aware tile order
    p.fam = DW_TILE;
    p.rows = gx < 1 ? 1 : gx;
}

// ---------------------------------------------------------------------------------------------------- ring kernels
// geometry of the ring kernels for d.H x d.W images (stride 1): false if unsupported
static bool pick_slide(const TfnasCellDesc& d, int K, DwSlide& gm) {
    if (K != 3 && K != 5) return false;   // (dw_tile_only)
    if (act_tile_only(d.act)) return false;
    const int ws_min = 14;                // (7-wide images: only the weight gradient gained, and the register-window kernel has it)
    if (d.stride != 1 || d.W > 56 || d.W < ws_min) return false;
    if ((size_t)d.N * d.H * d.W * d.M >= ((size_t)1 << 30)) return false;     // 32-bit element offsets
    gm.TW = (d.W + 3) & ~3;
    gm.L1 = gm.TW + K - 1;
    gm.CC = 32;
    gm.CCP = gm.CC;                       // (pixel stride of the LDS ring; the kernels have CC = CCP = 32 compiled in; bank conflicts: ring_swz)
    gm.cq_shift = 3;
    const int per_row = (gm.TW >> 2) * (gm.CC >> 2);
    gm.TH = 256 / per_row;
    if (gm.TH > 7) gm.TH = 7;
    while (gm.TH > 1 && (gm.TH * gm.L1 * (gm.CC >> 2) > 1024 ||
                         (size_t)(gm.TH - 1 + K) * gm.L1 * gm.CCP * sizeof(float) > 46 * 1024))
        --gm.TH;
    gm.RB = gm.TH - 1 + K;
    if (gm.TH < 1 || gm.TH > d.H || gm.TH * gm.L1 * (gm.CC >> 2) > 1024 ||
        (size_t)gm.RB * gm.L1 * gm.CCP * sizeof(float) > 48 * 1024 || gm.RB * gm.L1 * gm.CCP < 2048)
        return false;
    gm.chunks = dw_chunks(d, K, gm.CC);
    return true;
}

// the ring kernels for both kernel sizes, one image lane (= partial row) count: false if the route or a geometry rules them out
static bool dws_plan(const TfnasCellDesc& d, size_t row_floats, DwPlan& p) {
    if (route_dw(d) == 3 || dw_tile_only(d)) return false;
    int gx = d.N;
    for (int i = 0; i < 2; ++i) {
        if (!pick_slide(d, 3 + 2 * i, p.ring[i])) return false;
        p.chunks[i] = p.ring[i].chunks;
        if (!p.chunks[i]) continue;
        int g1 = cdiv(4096, p.chunks[i]);
        if (g1 < 8) g1 = 8;
        if (g1 < gx) gx = g1;
    }
    const size_t cap = TFNAS_PART_FLOATS / (row_floats ? row_floats : 1);
    if ((size_t)gx > cap) gx = (int)cap;
    if (gx > d.N) gx = d.N;
    if (gx >= 8) gx &= ~7;
    p.fam = DW_RING;
    p.rows = gx < 1 ? 1 : gx;
    p.ring[0].gx = p.ring[1].gx = p.rows;
    return true;
}

// The E-free ring kernels (rows recomputed from x, KQ = ic / 4) are compiled for these ic only.
static bool dws_efree_ic(int ic) { return ic == 24 || ic == 40; }

// Register-prefetch (PIPE) variants where measured faster: 56-wide images (LDS-limited to 3 workgroups per CU whatever the
// register count) and the wide soft-mode launches at 28x28; the 4+-wave variants elsewhere (sampled launches, 14x14).
static bool dws_pipe(const TfnasCellDesc& d) {
    return d.W > 40 || (d.W > 20 && d.M >= 512);
}

// ---------------------------------------------------------------------------------------------------- register-window kernels
// weight gradient, measured: 1.5x on the stride-2 cells, 1.1-2.8x at 14 x 14 / 7 x 7, 0.8-1.1x against the ring kernel at
// 56 x 56 / 28 x 28 stride 1
static bool dwd_wgrad_use(const TfnasCellDesc& d) {
    const int r = route_dw(d);
    return r == 1 || (r == 0 && (d.stride == 2 || d.W <= 14 || d.W > 56));
}
// forward, measured (sampled launches at B = 128): against the LDS-tiled kernel of the stride-2 cells 1.4-1.7x at 112 x 112 /
// 56 x 56 (k5; k3 equal), equal at 28 x 28, slower below (a wave's prologue -- K*K taps and the constants of its two channels --
// is paid for a dozen rows); against the ring kernels of the stride-1 cells 0.8-1.0x
static bool dwd_fwd_use(const TfnasCellDesc& d) {
    const int r = route_dw(d);
    return r == 1 || (r == 0 && ((d.stride == 2 && d.H >= 56) || d.W > 56));   // (W > 56: no ring kernel either -- the stems)
}
// backward w.r.t. the input, measured: 1.2-1.7x against the LDS-tiled kernel on every stride-2 cell (112 x 112 ... 14 x 14),
// 0.7-1.1x against the ring kernels of the stride-1 cells
static bool dwd_bwd_use(const TfnasCellDesc& d) {
    const int r = route_dw(d);
    return r == 1 || (r == 0 && (d.stride == 2 || d.W > 56));
}
static int dwd_jw(const TfnasCellDesc& d) {
    return (d.Wo <= 8 || d.Wo == 56) ? 2 : 4;
}

// kind 0: weight gradient (macro-steps per image Ho + A, row_floats = the weight-gradient row), kind 1: forward (H + P or
// Ho + 1 macro-steps, rows of 2 * M statistics partials), kind 2: backward w.r.t. the input (Ho + P or Ho + 1 dd-row events).
// False: unsupported geometry (p is then planned again by the next family).
static bool dwd_plan(const TfnasCellDesc& d, size_t row_floats, int jw, int kind, DwPlan& p) {
    constexpr int lpp = 16;                                  // lanes per pixel of the k_dwd_* kernels (2 channels each)
    if (d.stride != 1 && d.stride != 2) return false;
    if (dw_tile_only(d)) return false;
    if ((size_t)d.N * d.H * d.W * d.M >= ((size_t)1 << 30)) return false;                 // 32-bit element offsets
    for (int g = 0; g < d.G; ++g)
        if (d.g[g].mc & 1) return false;
    // one resident round: 256 CUs x 4 SIMDs x the waves per SIMD the kernel's registers allow (launch bounds); a wave walks at
    // least `minper` macro-steps (its prologue -- constants from the double statistics -- and the R-1 warm-up steps are paid once)
    const int wscale = 100, minper_w = 8, minper_f = 8;      // (% of a round; minper_f 16: +10..15 % on the 28 x 28 / 14 x 14 stride-2 cells)
    const int minper = kind == 0 ? minper_w : (kind == 1 ? minper_f : (d.stride == 1 ? minper_f : minper_f / 2));
    const int ncg = cdiv(d.Wo, (64 / lpp) * jw);
    DwDirect* gms = p.direct;
    int nseg = 1 << 30;
    int steps_k[2] = {0, 0};
    for (int i = 0; i < 2; ++i) {
        const int kk = 3 + 2 * i;
        gms[i].chunks = dw_chunks(d, kk, 2 * lpp);
        if (!gms[i].chunks) continue;
        int per_img;
        if (kind == 0) per_img = d.Ho + (d.stride == 1 ? kk / 2 : 1);
        else if (kind == 1) per_img = d.stride == 1 ? d.H + kk / 2 : d.Ho + 1;
        else per_img = d.Ho + (d.stride == 1 ? kk / 2 : 1);
        const int steps = d.N * per_img;
        steps_k[i] = steps;
        int occ;
        if (kind == 0) occ = kk == 3 ? 4 : (jw == 2 ? 3 : 2);
        else if (kind == 1) occ = kk == 3 ? 4 : (jw == 2 ? 4 : 3);
        else occ = dwd_bwd_occ(kk, d.stride, jw);
        const int want = 1024 * occ * wscale / 100;
        int ns = want / (gms[i].chunks * ncg);
        if (ns > steps / minper) ns = steps / minper;
        ns &= ~3;
        if (ns < 4) ns = 4;
        if (ns < nseg) nseg = ns;
    }
    size_t cap = TFNAS_PART_FLOATS / (row_floats ? row_floats : 1);
    if (cap > 1024) cap = 1024;
    while (nseg > 4 && (size_t)ncg * (nseg >> 2) > cap) nseg -= 4;
    if ((size_t)ncg * (nseg >> 2) > cap) return false;
    for (int i = 0; i < 2; ++i) {
        gms[i].ncg = ncg;
        gms[i].nseg = nseg;
        gms[i].steps = steps_k[i];
        gms[i].per = cdiv(steps_k[i], nseg);
        gms[i].nwg = gms[i].chunks * ncg * (nseg >> 2);
        p.chunks[i] = gms[i].chunks;
    }
    p.fam = DW_DIRECT;
    p.rows = ncg * (nseg >> 2);
    p.jw = jw;
    return true;
}

// ---------------------------------------------------------------------------------------------------- planners
static DwPlan dw_plan_fwd(const TfnasCellDesc& d, bool efree, bool has_x) {
    DwPlan p = {};
    const size_t row = 2 * (size_t)d.M;
    if (!efree && dwd_fwd_use(d) && dwd_plan(d, row, dwd_jw(d), 1, p)) return p;
    p.kq = efree ? d.ic / 4 : 0;
    if ((!efree || (dws_efree_ic(d.ic) && has_x)) && dws_plan(d, row, p)) {
        p.pipe = !efree && dws_pipe(d);
        return p;
    }
    dw_tile_plan(d, d.Ho, d.Wo, true, 4096, row, efree, p);
    return p;
}

DwPlan dw_plan_bwd_data(const TfnasCellDesc& d, bool efree, bool has_x) {
    DwPlan p = {};
    const size_t row = 2 * (size_t)d.M, wout = dw_wout_size(d);
    const bool direct = !efree && dwd_bwd_use(d);
    if (direct) {
        const int jw = d.stride == 2 ? 2 : dwd_jw(d);          // (stride 2: a lane owns 2 * JW input columns)
        // the weight gradient of the stride-2 cells from this pass (k_dwd_bwd<.., WG>; its partial rows go behind the statistics
        // partials) unless TFNAS_ROUTE_DWWG2_OFF asks for its own kernel
        p.fuse_wgrad = d.need_wgrad && !(d.route & TFNAS_ROUTE_DWWG2_OFF) && d.stride == 2 && dw_groups_k(d, true) &&
                       dwd_plan(d, row + wout + 64, jw, 2, p);
        if (p.fuse_wgrad || dwd_plan(d, row, jw, 2, p)) return p;
        // (a geometry the register-window pass refuses takes the ring / tile kernels without fusing the weight gradient)
    }
    p.kq = efree ? d.ic / 4 : 0;
    if ((!efree || (dws_efree_ic(d.ic) && has_x)) && dws_plan(d, row, p)) {
        // The 3 x 3 weight gradient of the stride-1 ring cells from this pass (WGR variant of k_dws_bwd) unless
        // TFNAS_ROUTE_DWWG_OFF asks for its own kernel.  3 x 3 taps only: 9 more float4 accumulators fit the register budget of
        // two waves per SIMD; 5 x 5 needs 25 (100 registers on top of 130-170: 900-1100 bytes of scratch per thread at 256
        // registers -- measured in the ISA, not launched).  Images >= 28 wide: measured alone at B = 128 (DESIGN.md section 4c,
        // one 3 x 3 candidate, whole cell): 56 x 56 1.17 -> 0.94 ms, 28 x 28 0.57 -> 0.51 ms, 14 x 14 equal (there the separate
        // register-window weight gradient is already cheap and the fused pass runs at two waves per SIMD instead of four); in
        // the pair the change is inside the noise (69.3-69.7 vs 69.4-69.9 ms)
        p.fuse_wgrad = !direct && !efree && d.need_wgrad && !(d.route & TFNAS_ROUTE_DWWG_OFF) && dw_groups_k(d, false) &&
                       d.W >= 28 && (size_t)p.rows * (row + 64 + wout) <= TFNAS_PART_FLOATS;
        p.pipe = !efree && !p.fuse_wgrad && dws_pipe(d);
        return p;
    }
    dw_tile_plan(d, d.H, d.W, false, 4096, row, efree, p);
    return p;
}

static DwPlan dw_plan_wgrad(const TfnasCellDesc& d) {
    DwPlan p = {};
    const size_t wout = dw_wout_size(d);
    if (dwd_wgrad_use(d) && dwd_plan(d, wout, dwd_jw(d), 0, p)) return p;
    if (dws_plan(d, wout, p)) {
        p.pipe = dws_pipe(d);
        return p;
    }
    dw_tile_plan(d, d.Ho, d.Wo, true, 2048, wout, false, p);
    return p;
}

// ---------------------------------------------------------------------------------------------------- launchers
// (A tile launch also has a dilation, 1 | 2: dw_tile_dispatch_d below.)
// Template arguments of a launch from its runtime kernel size (3 | 5, and 7 where TILE), stride (1 | 2), activation (ReLU | Swish,
// and ReLU6 | hard-swish where TILE) and variant (one of Vs): calls f(K, S, ACT, V) with std::integral_constant arguments.  False
// if the kernel size, the activation or the variant is not among them -- the launchers return TFNAS_EINVAL.  (Every combination
// is instantiated: a kernel without a stride or variant parameter ignores that argument.)  dw_dispatch: the register-window and
// ring launches (3 | 5, two activations); dw_tile_dispatch: the tile launches (3 | 5 | 7, four activations).
template <bool TILE, int... Vs, class F>
static bool dw_dispatch_k(int k, int stride, int act, int v, F&& f) {
    bool hit = false;
    auto with_v = [&](auto K, auto S, auto A) {
        ((v == Vs ? (f(K, S, A, std::integral_constant<int, Vs>{}), hit = true) : false) || ...);
    };
    auto with_a = [&](auto K, auto S) {
        if (act == TFNAS_ACT_RELU) with_v(K, S, std::integral_constant<int, TFNAS_ACT_RELU>{});
        else if (act == TFNAS_ACT_SWISH) with_v(K, S, std::integral_constant<int, TFNAS_ACT_SWISH>{});
        else if constexpr (TILE) {
            if (act == TFNAS_ACT_RELU6) with_v(K, S, std::integral_constant<int, TFNAS_ACT_RELU6>{});
            else if (act == TFNAS_ACT_HSWISH) with_v(K, S, std::integral_constant<int, TFNAS_ACT_HSWISH>{});
        }
    };
    auto with_s = [&](auto K) {
        if (stride == 1) with_a(K, std::integral_constant<int, 1>{});
        else with_a(K, std::integral_constant<int, 2>{});
    };
    if (k == 3) with_s(std::integral_constant<int, 3>{});
    else if (k == 5) with_s(std::integral_constant<int, 5>{});
    else if constexpr (TILE) {
        if (k == 7) with_s(std::integral_constant<int, 7>{});
    }
    return hit;
}
template <int... Vs, class F>
static bool dw_dispatch(int k, int stride, int act, int v, F&& f) {
    return dw_dispatch_k<false, Vs...>(k, stride, act, v, f);
}
template <int... Vs, class F>
static bool dw_tile_dispatch(int k, int stride, int act, int v, F&& f) {
    return dw_dispatch_k<true, Vs...>(k, stride, act, v, f);
}
// the tile launch of slot (k, dil): f(K, S, ACT, V, DIL).  Dilation 2: kernel sizes 3 | 5 and the variant 0 (KQ = 0: E or the raw
// input is read) only -- anything else is not instantiated and returns false
template <int... Vs, class F>
static bool dw_tile_dispatch_d(int k, int dil, int stride, int act, int v, F&& f) {
    if (dil == 1)
        return dw_tile_dispatch<Vs...>(k, stride, act, v, [&](auto K, auto S, auto A, auto V) {
            f(K, S, A, V, std::integral_constant<int, 1>{});
        });
    if (dil != 2 || (k != 3 && k != 5) || v != 0) return false;
    return dw_tile_dispatch<0>(k, stride, act, 0, [&](auto K, auto S, auto A, auto V) {
        if constexpr (K != 7) f(K, S, A, V, std::integral_constant<int, 2>{});
    });
}
// variant of the launches with the weight gradient fused into the backward-data pass (k_dwd_bwd<.., WG>, k_dws_bwd<.., WGR>)
constexpr int DW_WG = -1;
// variant of a ring launch: 0 plain, 1 register prefetch (PIPE), KQ (6 | 10: E-free), DW_WG
static int dws_variant(const DwPlan& p) { return p.fuse_wgrad ? DW_WG : p.kq ? p.kq : (int)p.pipe; }

// sum the weight-gradient partial rows into each group's g_dw
static int dw_reduce_wgrad(const TfnasCellDesc& d, const float* wpart, int rows, size_t wout, hipStream_t s) {
    size_t poff = 0;
    for (int g = 0; g < d.G; ++g) {
        const int n = (int)group_dw_floats(d, g);      // (a packed group: its segments' blocks are contiguous, one reduction)
        const int rc = launch_reduce_rows(wpart + poff, rows, n, wout, nullptr, d.g[g].g_dw, s, wgrad_accum(d));
        if (rc) return rc;
        poff += n;
    }
    return 0;
}

int launch_dw_fwd(const TfnasCellDesc& d, const float* E, const float* x, const double* stats1, float* D,
                  double* stats2, float* part, hipStream_t s) {
    const bool raw = cell_noexpand(d);           // D = dw(x): the tile kernels' raw-input form (E and stats1 are not touched)
    if (raw ? !x : (!E && (!efree_ic_ok(d.ic) || dw_tile_only(d)))) return TFNAS_EINVAL;
    const DwPlan p = dw_plan_fwd(d, !raw && E == nullptr, x != nullptr);
    for (int i = 0; i < DW_NK; ++i) {
        if (!p.chunks[i]) continue;
        const int kk = dw_slot_k(i), dil = dw_slot_dil(i);
        ProfScope _prof(TK_DW_FWD, s, d.G > 2);
        bool ok = false;
        if (p.fam != DW_TILE && i >= 2) return TFNAS_EINVAL;     // (never planned: dw_tile_only)
        if (p.fam == DW_DIRECT) {
            const DwDirect gm = p.direct[i];
            ok = dw_dispatch<2, 4>(kk, d.stride, d.act, p.jw, [&](auto K, auto S, auto A, auto JW) {
                hipLaunchKernelGGL((k_dwd_fwd<K, S, A, JW>), dim3(gm.nwg), dim3(256), 0, s, d, E, stats1, D, part, gm);
            });
        } else if (p.fam == DW_RING) {
            const DwSlide gm = p.ring[i];
            const size_t shm = (size_t)(gm.RB * gm.L1 * gm.CCP + kk * kk * gm.CC + 2 * gm.CC) * sizeof(float);
            ok = dw_dispatch<0, 1, 6, 10>(kk, d.stride, d.act, dws_variant(p), [&](auto K, auto, auto A, auto V) {
                hipLaunchKernelGGL((k_dws_fwd<K, A, V == 1, V == 1 ? 0 : V>), dim3(p.rows * gm.chunks), dim3(256), shm, s, d, E,
                                   stats1, D, part, gm, V > 1 ? x : nullptr);
            });
        } else {
            const DwGeom gm = p.tile[i];
            const int tile = gm.L0 * gm.L1 * gm.CC > 2048 ? gm.L0 * gm.L1 * gm.CC : 2048;
            const size_t shm = (size_t)(tile + kk * kk * gm.CC + 2 * gm.CC) * sizeof(float);
            if (shm > 64 * 1024) return TFNAS_ERANGE;
            if (raw)        // (no activation before the depthwise: one instantiation per K, S)
                ok = dw_tile_dispatch_d<0>(kk, dil, d.stride, TFNAS_ACT_RELU, 0, [&](auto K, auto S, auto, auto, auto DIL) {
                    hipLaunchKernelGGL((k_dw_fwd<K, S, TFNAS_ACT_RELU, 0, true, DIL>), dim3(p.rows, p.chunks[i]), dim3(256), shm, s,
                                       d, nullptr, x, nullptr, D, part, gm);
                });
            else
            ok = dw_tile_dispatch_d<0, 4, 6, 10>(kk, dil, d.stride, d.act, p.kq, [&](auto K, auto S, auto A, auto KQ, auto DIL) {
                if constexpr ((K != 7 && !act_tile_only(A)) || KQ == 0)     // (no E-free 7 x 7 / ReLU6 / hard-swish kernels: refused above)
                    hipLaunchKernelGGL((k_dw_fwd<K, S, A, KQ, false, DIL>), dim3(p.rows, p.chunks[i]), dim3(256), shm, s, d, E, x,
                                       stats1, D, part, gm);
            });
        }
        if (!ok) return TFNAS_EINVAL;
    }
    return reduce_pair_rows(d, part, p.rows, stats2, s);       // (some groups of a mixed cell: their own columns of stats2 only)
}

int launch_dw_bwd_data(const DwPlan& p, const TfnasCellDesc& d, const float* dZ, const float* gate, const float* dpooled,
                       const float* D, const double* stats2, const double* red2, const float* E, const float* x,
                       const double* stats1, float* dEh, double* red1, float* part, hipStream_t s, float* cb1) {
    if (cell_noexpand(d)) return TFNAS_EINVAL;       // (launch_dw_bwd_dx)
    if (!E && (!efree_ic_ok(d.ic) || dw_tile_only(d))) return TFNAS_EINVAL;
    const size_t wout = dw_wout_size(d);
    float* wpart = part + (((size_t)p.rows * 2 * d.M + 63) & ~(size_t)63);    // (fuse_wgrad: behind the statistics partials)
    for (int i = 0; i < DW_NK; ++i) {
        if (!p.chunks[i]) continue;
        const int kk = dw_slot_k(i), dil = dw_slot_dil(i);
        ProfScope _prof(TK_DW_BWD_DATA, s, d.G > 2);
        bool ok = false;
        if (p.fam != DW_TILE && i >= 2) return TFNAS_EINVAL;     // (never planned: dw_tile_only)
        if (p.fam == DW_DIRECT) {
            const DwDirect gm = p.direct[i];
            ok = dw_dispatch<2, 4, DW_WG>(kk, d.stride, d.act, p.fuse_wgrad ? DW_WG : p.jw, [&](auto K, auto S, auto A, auto V) {
                if constexpr (V == DW_WG)           // (stride 2, JW = 2 only)
                    hipLaunchKernelGGL((k_dwd_bwd<K, 2, A, 2, true>), dim3(gm.nwg), dim3(256), 0, s, d, dZ, gate, dpooled, D,
                                       stats2, red2, E, stats1, dEh, part, gm, wpart, wout);
                else
                    hipLaunchKernelGGL((k_dwd_bwd<K, S, A, V>), dim3(gm.nwg), dim3(256), 0, s, d, dZ, gate, dpooled, D, stats2,
                                       red2, E, stats1, dEh, part, gm);
            });
        } else if (p.fam == DW_RING) {
            const DwSlide gm = p.ring[i];
            size_t shm = (size_t)(gm.RB * gm.L1 * gm.CCP + kk * kk * gm.CC + 4 * gm.CC + 2 * gm.CC +
                                  (p.kq ? gm.TH * gm.TW * gm.CCP : 0)) * sizeof(float);
            if (p.fuse_wgrad && shm < (size_t)4 * kk * kk * gm.CC * sizeof(float)) shm = (size_t)4 * kk * kk * gm.CC * sizeof(float);
            ok = dw_dispatch<0, 1, 6, 10, DW_WG>(kk, d.stride, d.act, dws_variant(p), [&](auto K, auto, auto A, auto V) {
                if constexpr (V == DW_WG) {
                    // (3 x 3 only: dw_plan_bwd_data; the non-prefetching variant: with the 9 accumulators the prefetching one spills)
                    if constexpr (K == 3)
                        hipLaunchKernelGGL((k_dws_bwd<K, A, false, 0, true>), dim3(p.rows * gm.chunks), dim3(256), shm, s, d, dZ,
                                           gate, dpooled, D, stats2, red2, E, stats1, dEh, part, gm, nullptr, wpart, wout);
                } else {
                    hipLaunchKernelGGL((k_dws_bwd<K, A, V == 1, V == 1 ? 0 : V>), dim3(p.rows * gm.chunks), dim3(256), shm, s, d,
                                       dZ, gate, dpooled, D, stats2, red2, E, stats1, dEh, part, gm, V > 1 ? x : nullptr);
                }
            });
        } else {
            const DwGeom gm = p.tile[i];
            const int tile = gm.L0 * gm.L1 * gm.CC > 2048 ? gm.L0 * gm.L1 * gm.CC : 2048;
            const size_t shm = (size_t)(tile + kk * kk * gm.CC + 4 * gm.CC + 2 * gm.CC + (p.kq ? gm.T0 * gm.T1 * gm.CC : 0)) *
                               sizeof(float);
            if (shm > 64 * 1024) return TFNAS_ERANGE;
            ok = dw_tile_dispatch_d<0, 4, 6, 10>(kk, dil, d.stride, d.act, p.kq, [&](auto K, auto S, auto A, auto KQ, auto DIL) {
                if constexpr ((K != 7 && !act_tile_only(A)) || KQ == 0)
                    hipLaunchKernelGGL((k_dw_bwd_data<K, S, A, KQ, false, DIL>), dim3(p.rows, p.chunks[i]), dim3(256), shm, s, d, dZ,
                                       gate, dpooled, D, stats2, red2, E, x, stats1, dEh, part, gm, 0);
            });
        }
        if (!ok) return TFNAS_EINVAL;
    }
    if (p.fuse_wgrad) {
        ProfScope _prof(TK_DW_WGRAD, s);
        const int rc = dw_reduce_wgrad(d, wpart, p.rows, wout, s);
        if (rc) return rc;
    }
    if (cb1) return launch_reduce_bn1(d, part, p.rows, stats1, red1, cb1, s);
    return launch_reduce_rows(part, p.rows, 2 * d.M, 2 * (size_t)d.M, red1, nullptr, s);
}

// A cell without expand convolution (TFNAS_CELL_NOEXPAND): the depthwise backward-data pass writes the cell's dx [N*H*W][ic] itself,
// dx = dw^T(dd) (+ dres: the residual gradient dout of a residual block, NULL otherwise).  Tile kernels only, no BN1-backward sums,
// no partial rows, no reduction.
int launch_dw_bwd_dx(const TfnasCellDesc& d, const float* dZ, const float* gate, const float* dpooled, const float* D,
                     const double* stats2, const double* red2, const float* dres, float* dx, hipStream_t s, bool accum) {
    if (!cell_noexpand(d) || !dx) return TFNAS_EINVAL;
    if (accum && d.G != 1) return TFNAS_EINVAL;      // (two groups' workgroups would read-add-store the same dx elements)
    const DwPlan p = dw_plan_bwd_data(d, false, false);
    if (p.fam != DW_TILE) return TFNAS_EINVAL;       // (never planned: dw_tile_only)
    for (int i = 0; i < DW_NK; ++i) {
        if (!p.chunks[i]) continue;
        const int kk = dw_slot_k(i), dil = dw_slot_dil(i);
        ProfScope _prof(TK_DW_BWD_DATA, s, false);
        const DwGeom gm = p.tile[i];
        const int tile = gm.L0 * gm.L1 * gm.CC > 2048 ? gm.L0 * gm.L1 * gm.CC : 2048;
        const size_t shm = (size_t)(tile + kk * kk * gm.CC + 4 * gm.CC + 2 * gm.CC) * sizeof(float);
        if (shm > 64 * 1024) return TFNAS_ERANGE;
        const bool ok = dw_tile_dispatch_d<0>(kk, dil, d.stride, d.act, 0, [&](auto K, auto S, auto A, auto, auto DIL) {
            hipLaunchKernelGGL((k_dw_bwd_data<K, S, A, 0, true, DIL>), dim3(p.rows, p.chunks[i]), dim3(256), shm, s, d, dZ, gate,
                               dpooled, D, stats2, red2, nullptr, dres, nullptr, dx, nullptr, gm, (int)accum);
        });
        if (!ok) return TFNAS_EINVAL;
    }
    return (int)hipGetLastError();
}

// tap rows of one k_dw_wgrad workgroup (KR).  All K of them, except: 7 x 7 -- 4 (rows 0-3 | 4-6); the dilated 5 x 5 at stride 1
// -- 3 (rows 0-2 | 3-4): its 25 accumulators beside the 12-wide register window (stride + 9 taps' extent) spill 36-48 bytes of
// scratch at 256 registers, 15 do not.  (At stride 2 the window holds only the 8 even entries and all 25 fit: 249-251 registers.)
static constexpr int dw_wgrad_kr(int k, int stride, int dil) { return k == 7 ? 4 : (k == 5 && dil == 2 && stride == 1) ? 3 : k; }

int launch_dw_wgrad(const TfnasCellDesc& d, const float* dZ, const float* gate, const float* dpooled, const float* D,
                    const double* stats2, const double* red2, const float* E, const double* stats1, float* part,
                    hipStream_t s) {
    if (!dw_wgrad_row_fits(d)) return TFNAS_ERANGE;
    const DwPlan p = dw_plan_wgrad(d);
    const size_t wout = dw_wout_size(d);
    for (int i = 0; i < DW_NK; ++i) {
        if (!p.chunks[i]) continue;
        const int kk = dw_slot_k(i), dil = dw_slot_dil(i);
        ProfScope _prof(TK_DW_WGRAD, s);
        if (p.fam != DW_TILE && i >= 2) return TFNAS_EINVAL;     // (never planned: dw_tile_only)
        if (p.fam == DW_DIRECT) {
            const DwDirect gm = p.direct[i];
            dw_dispatch<2, 4>(kk, d.stride, d.act, p.jw, [&](auto K, auto S, auto A, auto JW) {
                hipLaunchKernelGGL((k_dwd_wgrad<K, S, A, JW>), dim3(gm.nwg), dim3(256), 0, s, d, dZ, gate, dpooled, D, stats2,
                                   red2, E, stats1, part, wout, gm);
            });
        } else if (p.fam == DW_RING) {
            const DwSlide gm = p.ring[i];
            int ring = gm.RB * gm.L1 * gm.CCP;
            if (ring < 4 * kk * kk * gm.CC) ring = 4 * kk * kk * gm.CC;     // cross-wave reduction reuses the ring
            const size_t shm = (size_t)(ring + 4 * gm.CC + 2 * gm.CC) * sizeof(float);
            dw_dispatch<0, 1>(kk, d.stride, d.act, p.pipe, [&](auto K, auto, auto A, auto PIPE) {
                hipLaunchKernelGGL((k_dws_wgrad<K, A, PIPE == 1>), dim3(p.rows * gm.chunks), dim3(256), shm, s, d, dZ, gate,
                                   dpooled, D, stats2, red2, E, stats1, part, wout, gm);
            });
        } else {
            const DwGeom gm = p.tile[i];
            const int kr = dw_wgrad_kr(kk, d.stride, dil);     // tap rows per workgroup (k_dw_wgrad: KR), parts over blockIdx.z
            int tile = gm.L0 * gm.L1 * gm.CC;
            if (tile < 4 * kr * kk * gm.CC) tile = 4 * kr * kk * gm.CC;
            const size_t shm = (size_t)(tile + 4 * gm.CC + 2 * gm.CC) * sizeof(float);
            if (shm > 64 * 1024) return TFNAS_ERANGE;
            if (cell_noexpand(d))        // (E = the cell input x, raw)
                dw_tile_dispatch_d<0>(kk, dil, d.stride, d.act, 0, [&](auto K, auto S, auto A, auto, auto DIL) {
                    constexpr int KR = dw_wgrad_kr(K, S, DIL);
                    hipLaunchKernelGGL((k_dw_wgrad<K, S, A, KR, true, DIL>), dim3(p.rows, p.chunks[i], (K + KR - 1) / KR), dim3(256),
                                       shm, s, d, dZ, gate, dpooled, D, stats2, red2, E, nullptr, part, wout, gm);
                });
            else
            dw_tile_dispatch_d<0>(kk, dil, d.stride, d.act, 0, [&](auto K, auto S, auto A, auto, auto DIL) {
                constexpr int KR = dw_wgrad_kr(K, S, DIL);
                hipLaunchKernelGGL((k_dw_wgrad<K, S, A, KR, false, DIL>), dim3(p.rows, p.chunks[i], (K + KR - 1) / KR), dim3(256), shm,
                                   s, d, dZ, gate, dpooled, D, stats2, red2, E, stats1, part, wout, gm);
            });
        }
    }
    const int rc = dw_reduce_wgrad(d, part, p.rows, wout, s);
    return rc ? rc : (int)hipGetLastError();
}
