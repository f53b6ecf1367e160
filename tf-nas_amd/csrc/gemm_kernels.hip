// 1x1-convolution (pointwise) kernels of the MBConv candidates as fp32 MFMA GEMMs with fused
// BatchNorm / activation / SE prologues and BatchNorm-statistics epilogues.
//
// Reference arithmetic: MBInvertedResBlock.forward, models/layers.py:539-561
//   expand  = inverted_bottleneck.conv (layers.py:463-478)   project = point_linear.conv (layers.py:528-534)
// and the autograd backward of those convolutions + BatchNorm2d(affine=False, batch stats).
#include <stdlib.h>
#include <string.h>
#include "gemm_core.h"
#include "gemm_x3.h"
#include "kernels.h"
#include "prof.h"

// ---------------------------------------------------------------------------- stem im2col operand
// TFNAS_MODE_STEM: the "expand" is first_stem's 3x3 stride-2 pad-1 convolution of the 3-channel NCHW image
// (models/model_search.py:219).  It runs through the same GEMM kernels with a gathering operand loader:
// A(p, t) = img[n][t/9][2*ho + (t%9)/3 - 1][2*wo + t%3 - 1]  (t < 27 = im2col depth, OIHW weight order).
__device__ __forceinline__ f32x4 stem_patch4(const float* __restrict__ img, const TfnasCellDesc& d, int p, int t0) {
    const int HW = d.H * d.W, n = p / HW, r = p - n * HW, ho = r / d.W, wo = r - ho * d.W;
    f32x4 v = zero4();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = t0 + j;
        if (t < 27) {
            const int ci = t / 9, rem = t - 9 * ci, ky = rem / 3, kx = rem - 3 * ky;
            const int hi = 2 * ho + ky - 1, wi = 2 * wo + kx - 1;
            if (hi >= 0 && hi < d.Hi && wi >= 0 && wi < d.Wi) v[j] = img[((size_t)(n * 3 + ci) * d.Hi + hi) * d.Wi + wi];
        }
    }
    return v;
}

// resident workgroups per CU the row-tiled GEMM kernels are compiled for (register cap 512 / n per lane): 5-/7-tile and
// narrower variants
constexpr int kLbBig = 3, kLbSmall = 4;
// the split-bf16 loop (MM != 0) keeps two chunks of raw operands and three A planes in registers: one resident workgroup less
constexpr int kLbX3Big = 2, kLbX3Small = 3;
constexpr int gemm_lb(int nt, int mm) { return mm == 0 ? (nt >= 5 ? kLbBig : kLbSmall) : (nt >= 5 ? kLbX3Big : kLbX3Small); }

// raw registers of the two-phase loaders (gemm_core.h): what the load phase leaves for the transform phase
struct Raw2 { f32x4 a, b; };             // two stream pieces (D | gate,  dOut | Pr,  dEh | E)
struct RawWS { f32x4 w; float s; };      // a weight quad and its row scale

// ============================================================================ expand forward
// E[p][off_g + m] = sum_c x[p][c] * w_expand_g[m][c]      for all groups in one launch
// epilogue: per-workgroup partial (sum, sumsq) of E per channel -> part (reduced into stats1 = BN1 statistics)
template <int NT, bool STEM, int MM>
__global__ __launch_bounds__(256, gemm_lb(NT, MM)) void k_expand_fwd(TfnasCellDesc d, const float* __restrict__ x,
                                                    float* __restrict__ E, float* __restrict__ part) {
    using T = GT<NT>;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    // all-candidate launches: consecutive workgroups (dispatch order) take consecutive COLUMN tiles of one row block -- the 256-byte
    // row pieces they store are then neighbours in memory instead of 4 * M bytes apart (measured alone, B = 128: cell 10 220 -> 190 us,
    // cell 3 186 -> 167 us, cell 1 443 -> 424 us; one-candidate launches 3-10 % slower that way and keep the row-block-fastest order)
    const int L_ = blockIdx.x + gridDim.x * blockIdx.y;
    const bool ctf_ = d.G > 1;
    const int BX = ctf_ ? L_ / (int)gridDim.y : (int)blockIdx.x;
    int ty = ctf_ ? L_ % (int)gridDim.y : (int)blockIdx.y, g = 0;
    for (; g < d.G - 1; ++g) {
        const int t = (d.g[g].mcp + T::BN - 1) / T::BN;
        if (ty < t) break;
        ty -= t;
    }
    const int mc = d.g[g].mc, mcp = d.g[g].mcp, off = d.g[g].off;
    const float* __restrict__ w = d.g[g].w_expand;
    const int n0 = ty * T::BN;
    const int P = d.N * d.H * d.W, ic = d.ic, M = d.M;
    const int nrt = (P + 127) >> 7, nchunks = (ic + 15) >> 4;
    const int tid = threadIdx.x;

    float cs[NT], cq[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) cs[j] = cq[j] = 0.f;

    for (int rt = BX; rt < nrt; rt += gridDim.x) {
        f32x4 acc[2][NT];
        acc_zero<NT>(acc);
        // the lane's two A rows stay the same for the whole K loop: row pointers and validity live in registers.  Stem: derived per
        // tile from a fresh copy of the thread index, as the staging indices below -- the gathering loader has no register to spare
        // and <4, true, 0> spilled 19 of them.  The plain variants keep the hoisted indices: with the copies they need 12-38
        // registers less, fit one more workgroup per CU and ran SLOWER (B = 128, alpha-step: <5, false, 6> 342 -> 437 us,
        // <4, false, 6> 144 -> 150 us)
        int tr = tid;
        if (STEM) asm volatile("" : "+v"(tr));
        const int lr = tr & 15, wrow = (tr >> 6) * 32;
        int prow[2];
        const float* arow[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            prow[i] = rt * 128 + wrow + 16 * i + lr;
            arow[i] = x + (size_t)min(prow[i], P - 1) * ic;
        }
        auto la = [&](int c, int i, int kl) -> f32x4 {
            const int k = c * 16 + kl;
            if (STEM) return (prow[i] < P && k < ic) ? stem_patch4(x, d, prow[i], k) : zero4();
            return ld4(arow[i] + min(k, ic - 4));
        };
        auto xa = [&](f32x4 r, int c, int i, int kl) -> f32x4 {
            if (STEM) return r;
            return (prow[i] < P && c * 16 + kl < ic) ? r : zero4();
        };
        auto lb = [&](int c, int n, int kl) -> f32x4 {
            const int col = n0 + n, k = c * 16 + kl;
            if (STEM) return (col < mc) ? ld4_guard(w + (size_t)col * ic, k, ic, false) : zero4();
            return ld4(w + (size_t)min(col, mc - 1) * ic + min(k, ic - 4));        // ic % 4 == 0: k < ic <=> k + 3 < ic
        };
        auto xb = [&](f32x4 r, int c, int n, int kl) -> f32x4 {
            if (STEM) return r;
            return (n0 + n < mc && c * 16 + kl < ic) ? r : zero4();
        };
        PreNone pre;
        gemm_adirect<NT, true, MM>(pre, la, xa, lb, xb, nchunks, acc, lds);
        int te = tid;
        if (STEM) asm volatile("" : "+v"(te));
        emit_tile_rows<NT, false>(acc, lds, [&](int lrow, int lc, f32x4 v) {
            const int p = rt * 128 + lrow;
            if (p < P && n0 + lc < mcp) st4_nt(E + ((size_t)p * M + off + n0 + lc), v);
        }, SlabNone(), te);
        acc_colstats<NT>(acc, cs, cq);
    }
    flush_colstats<NT>(cs, cq, lds, part + (size_t)BX * 2 * M + 2 * (size_t)off, n0, mcp);
}

// ============================================================================ project forward
// Pr[g][p][o] = sum_c z_g[p][c] * w_proj_g[o][c],   z = act(BN2(D)) * gate   (fused into the A load)
// epilogue: stats3[g][o] (BN3 batch statistics)
// (launch bounds: the 7-tile variant otherwise takes 149 VGPRs + 56 AGPRs = 2 waves/SIMD, measured 1.5 resident; capping
//  it at 168 registers buys the third wave: -17 % on the 112-channel cells)
template <int NT, int ACT, int MM>
__global__ __launch_bounds__(256, gemm_lb(NT, MM)) void k_project_fwd(TfnasCellDesc d, const float* __restrict__ D,
                                                     const float* __restrict__ gate,
                                                     const double* __restrict__ stats2, float* __restrict__ Pr,
                                                     float* __restrict__ part, int nsplit, float* __restrict__ prp) {
    using T = GT<NT>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // nsplit > 1 (under-filled launches: few row tiles, long K): K-split ks of group g adds chunks [cb, ce); split 0
    // writes Pr, split z > 0 its partial tile to prp[z-1]; k_pr_reduce sums them and takes the BN3 statistics
    // blockIdx.z -> group in order of DEcreasing K (= mid width): a workgroup's run time is proportional to its group's K
    // and the launch is 1-2 rounds of resident workgroups, so the long ones must not be the last to start (with the
    // natural order the 7x7 cells dispatched the widest group last: 1.5 instead of 1.0 long-workgroup times)
    const int zr = blockIdx.z / nsplit, ks = blockIdx.z - zr * nsplit;
    int g = 0;
    for (int c = 0; c < d.G; ++c) {
        int rank = 0;
        for (int o = 0; o < d.G; ++o) rank += (d.g[o].mcp > d.g[c].mcp) || (d.g[o].mcp == d.g[c].mcp && o < c);
        if (rank == zr) g = c;
    }
    const int mc = d.g[g].mc, mcp = d.g[g].mcp, off = d.g[g].off;
    const bool has_se = d.g[g].se > 0, w_al = (mc & 3) == 0;
    const float* gbase = has_se ? gate : D;        // the gate load is unconditional (see gemm_core.h: no branches
    const size_t se01 = has_se ? 1 : 0;            // around the loads of the prefetch phase)
    const float* __restrict__ w = d.g[g].w_proj;
    const int n0 = blockIdx.y * T::BN;
    const int HW = d.Ho * d.Wo, Po = d.N * HW, oc = d.oc, M = d.M;
    const int nrt = (Po + 127) >> 7, nchunks_all = (mcp + 15) >> 4;
    const int per = (nchunks_all + nsplit - 1) / nsplit, cb = ks * per;
    const int nchunks = max(0, min(nchunks_all, cb + per) - cb);
    float* __restrict__ dst = ks == 0 ? Pr : prp + (size_t)(ks - 1) * d.G * Po * oc;
    const int tid = threadIdx.x, lr = tid & 15, wrow = (tid >> 6) * 32;

    float2* cst = reinterpret_cast<float2*>(lds + T::LDS_FLOATS);
    for (int c = tid; c < ((mcp + 15) & ~15); c += 256)
        cst[c] = (c < mc) ? bn_consts(stats2 + 2 * (size_t)(off + c), 1.0 / (double)Po, d.eps) : make_float2(0.f, 0.f);
    __syncthreads();

    float cs[NT], cq[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) cs[j] = cq[j] = 0.f;

    for (int rt = blockIdx.x; rt < nrt; rt += gridDim.x) {
        f32x4 acc[2][NT];
        acc_zero<NT>(acc);
        // the lane's two A rows stay the same for the whole K loop: element offsets of the rows in D and in the gate table
        // (one division per row tile instead of one per chunk) and validity live in registers
        size_t arow[2], grow[2];
        bool rok[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = rt * 128 + wrow + 16 * i + lr, pc = min(p, Po - 1);
            rok[i] = p < Po;
            arow[i] = (size_t)pc * M + off;
            grow[i] = ((size_t)(pc / HW) * M + off) * se01;
        }
        auto la = [&](int c, int i, int kl) -> Raw2 {
            const int k = min((cb + c) * 16 + kl, mcp - 4);
            Raw2 r;
            r.a = ld4(D + (arow[i] + k));
            r.b = ld4(gbase + grow[i] + k * se01);                // no SE: one fixed (ignored) quad
            return r;
        };
        auto xa = [&](Raw2 r, int c, int i, int kl) -> f32x4 {
            const int k = (cb + c) * 16 + kl;
            f32x4 v = r.a;
            const int kc = min(k, mcp - 4);
            const float2 c0 = cst[kc], c1 = cst[kc + 1], c2 = cst[kc + 2], c3 = cst[kc + 3];
            v.x = act_f<ACT>((v.x - c0.x) * c0.y);
            v.y = act_f<ACT>((v.y - c1.x) * c1.y);
            v.z = act_f<ACT>((v.z - c2.x) * c2.y);
            v.w = act_f<ACT>((v.w - c3.x) * c3.y);
            if (has_se) v *= r.b;
            return (rok[i] && k < mcp) ? v : zero4();
        };
        auto lb = [&](int c, int n, int kl) -> f32x4 {
            const int o = n0 + n, k = (cb + c) * 16 + kl;
            if (MM == 0 && !w_al) return (o < oc) ? ld4_guard(w + (size_t)o * mc, k, mc, false) : zero4();
            return ld4(w + (size_t)min(o, oc - 1) * mc + min(k, mc - 4));          // mc % 4 == 0: k < mc <=> k + 3 < mc
        };
        auto xb = [&](f32x4 r, int c, int n, int kl) -> f32x4 {
            if (MM == 0 && !w_al) return r;
            return (n0 + n < oc && (cb + c) * 16 + kl < mc) ? r : zero4();
        };
        PreNone pre;
        gemm_adirect<NT, true, MM>(pre, la, xa, lb, xb, nchunks, acc, lds);
        // (the staging indices derive from a copy of the thread index taken afresh per tile: see k_project_dgrad)
        int te = tid;
        asm volatile("" : "+v"(te));
        emit_tile_rows<NT, false>(acc, lds, [&](int lrow, int lc, f32x4 v) {
            const int p = rt * 128 + lrow;
            if (p < Po && n0 + lc < oc) st4(dst + ((size_t)g * Po + p) * oc + n0 + lc, v);
        }, SlabNone(), te);
        acc_colstats<NT>(acc, cs, cq);
    }
    if (nsplit == 1)
        flush_colstats<NT>(cs, cq, lds, part + (size_t)blockIdx.x * 2 * d.G * oc + 2 * (size_t)g * oc, n0, oc);
}

// Pr[g][p][:] += sum_z prp[z][g][p][:] and the per-workgroup partial (sum, sumsq) of the finished Pr per (g, column):
// part[bx][2*(g*oc + o) + {0,1}] (the layout of k_project_fwd's own statistics epilogue).  Flat float4 stream; a
// thread's elements are `stride` float4 apart with stride a multiple of oc/4, so its column quad never changes.
__global__ __launch_bounds__(256) void k_pr_reduce(float* __restrict__ Pr, const float* __restrict__ prp, int nz, int G,
                                                   int Po, int oc, int rps, float* __restrict__ part) {
    __shared__ f32x4 rs[256], rq[256];
    const int tid = threadIdx.x, ocq = oc >> 2, stride = (256 / ocq) * ocq;
    const int g = blockIdx.y;
    const int r0 = blockIdx.x * rps, r1 = min(Po, r0 + rps);
    const size_t base = ((size_t)g * Po + r0) * ocq, zs = (size_t)G * Po * ocq;
    f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(Pr) + base;
    const f32x4* __restrict__ z4 = reinterpret_cast<const f32x4*>(prp) + base;
    const int n4 = (r1 - r0) * ocq;
    f32x4 s = zero4(), q = zero4();
    if (tid < stride) {
        for (int i = tid; i < n4; i += stride) {
            f32x4 v = p4[i];
            for (int z = 0; z < nz; ++z) v += z4[(size_t)z * zs + i];
            p4[i] = v;
            s += v;
            q += v * v;
        }
    }
    rs[tid] = s;
    rq[tid] = q;
    __syncthreads();
    for (int c = tid; c < oc; c += 256) {
        const int cq = c >> 2, comp = c & 3;
        float ts = 0.f, tq = 0.f;
        for (int k = cq; k < stride; k += ocq) {
            ts += rs[k][comp];
            tq += rq[k][comp];
        }
        float* row = part + (size_t)blockIdx.x * 2 * G * oc + 2 * ((size_t)g * oc + c);
        row[0] = ts;
        row[1] = tq;
    }
}

// ---------------------------------------------------------------------------- BN3-backward operand
// dP_g[p][o] = A3[o] * (dOut[p][o] - B3[o] - phat[p][o]*C3[o]),  phat = (Pr - mean3)*rstd3,
// A3 = wmix_g * rstd3, B3 = S1/Po, C3 = S2/Po  (S1,S2 = red3 sums of dOut and dOut*phat)
struct Bn3Tab {  // 5 floats per output channel, in LDS
    float *mean, *rstd, *a3, *b3, *c3;
};
__device__ __forceinline__ Bn3Tab bn3_tab_fill(float* base, int ocp, const TfnasCellDesc& d, int g,
                                               const double* stats3, const double* red3, const float* wmix) {
    Bn3Tab t{base, base + ocp, base + 2 * ocp, base + 3 * ocp, base + 4 * ocp};
    const int Po = d.N * d.Ho * d.Wo;
    const double inv = 1.0 / (double)Po;
    const float wg = wmix ? wmix[g] : 1.f;
    for (int o = threadIdx.x; o < ocp; o += blockDim.x) {
        if (o < d.oc) {
            const float2 c = bn_consts(stats3 + 2 * ((size_t)g * d.oc + o), inv, d.eps);
            t.mean[o] = c.x;
            t.rstd[o] = c.y;
            t.a3[o] = wg * c.y;
            t.b3[o] = (float)(red3[2 * ((size_t)g * d.oc + o) + 0] * inv);
            t.c3[o] = (float)(red3[2 * ((size_t)g * d.oc + o) + 1] * inv);
        } else {
            t.mean[o] = t.rstd[o] = t.a3[o] = t.b3[o] = t.c3[o] = 0.f;
        }
    }
    return t;
}
__device__ __forceinline__ f32x4 bn3_dp(const Bn3Tab& t, int o, f32x4 dout, f32x4 pr) {
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float ph = (pr[j] - t.mean[o + j]) * t.rstd[o + j];
        r[j] = t.a3[o + j] * (dout[j] - t.b3[o + j] - ph * t.c3[o + j]);
    }
    return r;
}

// Folded form for k_project_dgrad: one float4 (mean, a3, a3 b3, rstd c3 a3) per output channel,
//   dP = a3 dOut - a3 b3 - (Pr - mean) (rstd c3 a3)      (the form k_project_wgrad keeps in registers)
// -- one ds_read_b128 and three VALU operations per element instead of five table reads and six operations.
__device__ __forceinline__ void bn3_fold_fill(f32x4* tab, int ocp, const TfnasCellDesc& d, int g, const double* stats3,
                                              const double* red3, const float* wmix) {
    const int Po = d.N * d.Ho * d.Wo;
    const double inv = 1.0 / (double)Po;
    const float wg = wmix ? wmix[g] : 1.f;
    for (int o = threadIdx.x; o < ocp; o += blockDim.x) {
        f32x4 t = zero4();
        if (o < d.oc) {
            const float2 c = bn_consts(stats3 + 2 * ((size_t)g * d.oc + o), inv, d.eps);
            const float a3 = wg * c.y;
            const float b3 = (float)(red3[2 * ((size_t)g * d.oc + o) + 0] * inv);
            const float c3 = (float)(red3[2 * ((size_t)g * d.oc + o) + 1] * inv);
            t = f32x4{c.x, a3, a3 * b3, c.y * c3 * a3};
        }
        tab[o] = t;
    }
}
__device__ __forceinline__ f32x4 bn3_fold_dp(const f32x4* tab, int o, f32x4 dout, f32x4 pr) {
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 t = tab[o + j];
        r[j] = (t.y * dout[j] - t.z) - (pr[j] - t.x) * t.w;
    }
    return r;
}

// ---------------------------------------------------------------------------- BN2-backward sums in the dgrad epilogue
// FOLD variant of k_project_dgrad (round 4): the per-image tables that k_bn2_pool computed in its own pass
// over (dZ, D) -- A1 = sum dZ act'(dhat), B1 = sum dZ act'(dhat) dhat, dgate = sum dZ act(dhat), A2 = sum act'(dhat),
// B2 = sum act'(dhat) dhat over the pixels of one image (pointwise_kernels.hip) -- are accumulated while the dZ tile is still in
// LDS: dZ is then written once and never read back for them (the D read stays).  A lane owns one or two COLUMNS of the tile and
// walks the 16 rows of its wave's slab: column-contiguous dword loads of D (256 B per row and wave), no cross-lane reduction.
// A wave's 32 rows touch at most two images (HW >= 43), a 128-row tile at most four: one record per (row tile, image slot)
//   rec[((rt * 4 + slot) * 5 + q) * M + channel],  slot = image - image_of(rt * 128),  q = A1 | B1 | dgate | A2 | B2
// each written by exactly one workgroup (no atomics, fixed summation order); k_bn2_gather sums an image's records.
//
// Everything about the rows is wave-uniform and kept in scalar registers: a wave's 32 rows are numbered R = 0..31, rows [0, S) belong
// to its first image, rows [S, E) to its second, rows from E on lie past the end of the tensor (S = 32: no boundary, E = 32: all
// valid).  Rows ascend, so every addend of the first image comes before every addend of the second: ONE running set of sums per
// lane is enough -- at row S it is parked in `done` and restarts from zero (fold_split).  The rows are evaluated four at a time in
// straight-line code (the exp/rcp latency of one row overlaps the arithmetic of its neighbours); a group of four rows that holds
// neither row S nor the end E -- all but at most two of a wave's eight -- is added without any per-row test.
//
// The sums are summed in exactly this order and from exactly these roundings (the records feed BatchNorm backward of the whole
// chain: a last-bit change here is visible after 25 training pairs): every addend is a ROUNDED product -- fold_rn keeps the
// compiler, which contracts a * b + c wherever it sees one, from fusing it into the accumulation.
__device__ __forceinline__ float fold_rn(float v) {
    asm("" : "+v"(v));
    return v;
}
constexpr int fold_nc(int nt) { return (16 * nt + 63) / 64; }          // columns of the tile per lane
template <int NC>
__device__ __forceinline__ void fold_split(float (&cur)[FOLD_Q][NC], float (&done)[FOLD_Q][NC], int c) {
#pragma unroll
    for (int q = 0; q < FOLD_Q; ++q) {
        done[q][c] = cur[q][c];
        cur[q][c] = 0.f;
    }
}
// slab of 16 rows x BN at `st` (leading dimension LDC) = wave rows [R0, R0 + 16), tensor rows from p0 (all wave-uniform)
template <int NT, int ACT, bool SE>
__device__ __forceinline__ void fold_slab(const float* st, int LDC, const float* __restrict__ Dcol, int M, int lane, int p0, int Po,
                                          int R0, int S, int E, const float2 (&c2)[fold_nc(NT)], const bool (&cok)[fold_nc(NT)],
                                          float (&cur)[FOLD_Q][fold_nc(NT)], float (&done)[FOLD_Q][fold_nc(NT)]) {
    constexpr int NC = fold_nc(NT);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (!cok[c]) continue;
        const int col = lane + 64 * c;
        float dv[16], zv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) dv[r] = __builtin_nontemporal_load(Dcol + (size_t)min(p0 + r, Po - 1) * M + col);
#pragma unroll
        for (int r = 0; r < 16; ++r) zv[r] = st[r * LDC + col];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float a[4][FOLD_Q];                                     // the addends of rows 4k .. 4k+3 (rows from E on: never added)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float z = zv[4 * k + j];
                const float dh = (dv[4 * k + j] - c2[c].x) * c2[c].y;
                const float ad = fold_rn(act_d<ACT>(dh)), zd = fold_rn(z * ad);
                a[j][0] = zd;
                a[j][1] = fold_rn(zd * dh);
                if (SE) {
                    a[j][2] = fold_rn(z * act_f<ACT>(dh));
                    a[j][3] = ad;
                    a[j][4] = fold_rn(ad * dh);
                }
            }
            auto add = [&](int j) {
#pragma unroll
                for (int q = 0; q < (SE ? FOLD_Q : 2); ++q) cur[q][c] += a[j][q];
            };
            const int lo = R0 + 4 * k;
            if (__builtin_expect((S >= lo && S < lo + 4) || E < lo + 4, 0)) {      // the image boundary or the tensor's end is here
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (lo + j == S) fold_split<NC>(cur, done, c);
                    if (lo + j < E) add(j);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) add(j);
            }
        }
    }
}

// ============================================================================ project dgrad
// dZ[p][off_g + c] = sum_o dP_g[p][o] * w_proj_g[o][c]
template <int NT, int MM, bool FOLD = false>
__global__ __launch_bounds__(256, gemm_lb(NT, MM)) void k_project_dgrad(TfnasCellDesc d, const float* __restrict__ dout,
                                                       const float* __restrict__ Pr,
                                                       const double* __restrict__ stats3,
                                                       const double* __restrict__ red3,
                                                       const float* __restrict__ wmix, float* __restrict__ dZ,
                                                       const float* __restrict__ D = nullptr,
                                                       const double* __restrict__ stats2 = nullptr,
                                                       float* __restrict__ rec = nullptr) {
    using T = GT<NT>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // (all-candidate launches: column tiles fastest, as in k_expand_fwd -- cell 10 414 -> 376 us, cell 15 232 -> 213 us)
    const int L_ = blockIdx.x + gridDim.x * blockIdx.y;
    const bool ctf_ = d.G > 1;
    const int BX = ctf_ ? L_ / (int)gridDim.y : (int)blockIdx.x;
    int ty = ctf_ ? L_ % (int)gridDim.y : (int)blockIdx.y, g = 0;
    for (; g < d.G - 1; ++g) {
        const int t = (d.g[g].mcp + T::BN - 1) / T::BN;
        if (ty < t) break;
        ty -= t;
    }
    const int mc = d.g[g].mc, mcp = d.g[g].mcp, off = d.g[g].off;
    const bool w_al = (mc & 3) == 0;
    const float* __restrict__ w = d.g[g].w_proj;
    const int n0 = ty * T::BN;
    const int Po = d.N * d.Ho * d.Wo, oc = d.oc, M = d.M;
    const int ocp = (oc + 15) & ~15;
    const int nrt = (Po + 127) >> 7, nchunks = ocp >> 4;
    const int tid = threadIdx.x, lr = tid & 15, wrow = (tid >> 6) * 32;

    f32x4* tab = reinterpret_cast<f32x4*>(lds + T::LDS_FLOATS);
    bn3_fold_fill(tab, ocp, d, g, stats3, red3, wmix);
    // FOLD: BN2 constants of this lane's one or two columns of the (fixed) column tile
    constexpr int NC = (T::BN + 63) / 64;
    float2 c2f[NC];
    bool cokf[NC];
    const int HW = d.Ho * d.Wo;
    const bool has_se = d.g[g].se > 0;
    if (FOLD) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int col = (tid & 63) + 64 * c;
            cokf[c] = col < T::BN && n0 + col < mcp;
            c2f[c] = (cokf[c] && n0 + col < mc) ? bn_consts(stats2 + 2 * (size_t)(off + n0 + col), 1.0 / (double)Po, d.eps)
                                               : make_float2(0.f, 0.f);
        }
    }
    __syncthreads();

    for (int rt = BX; rt < nrt; rt += gridDim.x) {
        f32x4 acc[2][NT];
        acc_zero<NT>(acc);
        const float* drow[2];
        const float* qrow[2];
        bool rok[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = rt * 128 + wrow + 16 * i + lr, pc = min(p, Po - 1);
            rok[i] = p < Po;
            drow[i] = dout + (size_t)pc * oc;
            qrow[i] = Pr + ((size_t)g * Po + pc) * oc;
        }
        auto la = [&](int c, int i, int kl) -> Raw2 {
            const int o = min(c * 16 + kl, oc - 4);
            Raw2 r;
            r.a = ld4(drow[i] + o);
            r.b = ld4(qrow[i] + o);
            return r;
        };
        auto xa = [&](Raw2 r, int c, int i, int kl) -> f32x4 {
            const int o = c * 16 + kl;
            const f32x4 v = bn3_fold_dp(tab, min(o, oc - 4), r.a, r.b);
            return (rok[i] && o < oc) ? v : zero4();
        };
        auto lb = [&](int c, int kl, int n) -> f32x4 {
            const int o = c * 16 + kl;
            if (MM == 0 && !w_al) return (o < oc) ? ld4_guard(w + (size_t)o * mc, n0 + n, mc, false) : zero4();
            return ld4(w + (size_t)min(o, oc - 1) * mc + min(n0 + n, mc - 4));
        };
        auto xb = [&](f32x4 r, int c, int kl, int n) -> f32x4 {
            if (MM == 0 && !w_al) return r;
            return (c * 16 + kl < oc && n0 + n < mc) ? r : zero4();
        };
        PreNone pre;
        gemm_adirect<NT, false, MM>(pre, la, xa, lb, xb, nchunks, acc, lds);
        // The thread index is taken afresh for the epilogue of every tile: what is derived from it would otherwise be hoisted out of
        // the row-tile loop and stay live across the K loop, which has no register to spare
        int te = tid;
        asm volatile("" : "+v"(te));
        if (!FOLD) {
            emit_tile_rows<NT>(acc, lds, [&](int lrow, int lc, f32x4 v) {
                const int p = rt * 128 + lrow;
                if (p < Po && n0 + lc < mcp) st4_nt(dZ + ((size_t)p * M + off + n0 + lc), v);
            }, SlabNone(), te);
        } else {
            constexpr int LDC = T::BN + 4;
            // the wave's rows, image boundary and valid end as scalars (see fold_slab)
            const int w = __builtin_amdgcn_readfirstlane(te >> 6), lane = te & 63;
            const int pw0 = rt * 128 + w * 32;
            const int imgA = min(pw0, Po - 1) / HW;
            const int S = min(max((imgA + 1) * HW - pw0, 0), 32), E = min(max(Po - pw0, 0), 32);
            float cur[FOLD_Q][NC], done[FOLD_Q][NC];
#pragma unroll
            for (int q = 0; q < FOLD_Q; ++q)
#pragma unroll
                for (int c = 0; c < NC; ++c) cur[q][c] = done[q][c] = 0.f;
            const float* Dcol = D + off + n0;
            // activation (Swish or ReLU: launch_project_dgrad refuses every other one for this variant) and SE form: one scalar
            // choice per slab
            const int form = (d.act == TFNAS_ACT_RELU ? 2 : 0) + (has_se ? 1 : 0);
            emit_tile_rows<NT>(acc, lds,
                               [&](int lrow, int lc, f32x4 v) {
                                   const int p = rt * 128 + lrow;
                                   if (p < Po && n0 + lc < mcp) st4_nt(dZ + ((size_t)p * M + off + n0 + lc), v);
                               },
                               [&](int i, const float* st) {        // the wave's slab i (16 rows x BN) is still in LDS
                                   const int p0 = pw0 + 16 * i;
                                   if (form == 0) fold_slab<NT, TFNAS_ACT_SWISH, false>(st, LDC, Dcol, M, lane, p0, Po, 16 * i, S, E, c2f, cokf, cur, done);
                                   else if (form == 1) fold_slab<NT, TFNAS_ACT_SWISH, true>(st, LDC, Dcol, M, lane, p0, Po, 16 * i, S, E, c2f, cokf, cur, done);
                                   else if (form == 2) fold_slab<NT, TFNAS_ACT_RELU, false>(st, LDC, Dcol, M, lane, p0, Po, 16 * i, S, E, c2f, cokf, cur, done);
                                   else fold_slab<NT, TFNAS_ACT_RELU, true>(st, LDC, Dcol, M, lane, p0, Po, 16 * i, S, E, c2f, cokf, cur, done);
                               }, te);
            // waves -> image slots of the tile, in wave order (emit_tile_rows ended with a barrier: the GEMM LDS is free)
            static_assert(4 * 2 * FOLD_Q * T::BN + 4 <= T::LDS_FLOATS, "fold staging does not fit the GEMM LDS buffer");
            float* comb = lds;                                      // [4 waves][2 segments][5][BN]
            int* meta = reinterpret_cast<int*>(lds + 4 * 2 * FOLD_Q * T::BN);
            const bool split = S < 32;                              // the running sums are the second image's: the first's are parked
#pragma unroll
            for (int q = 0; q < FOLD_Q; ++q)
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (lane + 64 * c < T::BN) {
                        comb[((w * 2 + 0) * FOLD_Q + q) * T::BN + lane + 64 * c] = split ? done[q][c] : cur[q][c];
                        comb[((w * 2 + 1) * FOLD_Q + q) * T::BN + lane + 64 * c] = split ? cur[q][c] : 0.f;
                    }
            if (lane == 0) meta[w] = imgA;
            __syncthreads();
            // one thread per (q, column): it walks the eight (wave, segment) entries once, in the order wave 0..3, segment 0, 1, and
            // adds each to the slot of its image (a scalar per entry) -- the records' summation order
            const int img0 = min(rt * 128, Po - 1) / HW, imgL = min(rt * 128 + 127, Po - 1) / HW;
            int slot[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) slot[e] = __builtin_amdgcn_readfirstlane(meta[e >> 1]) + (e & 1) - img0;
            const int nq = has_se ? FOLD_Q : 2;
            for (int o = te; o < nq * T::BN; o += 256) {
                const int q = o / T::BN, col = o - q * T::BN;
                if (n0 + col >= mcp) continue;
                float t[FOLD_SLOTS];
#pragma unroll
                for (int sl = 0; sl < FOLD_SLOTS; ++sl) t[sl] = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = comb[(e * FOLD_Q + q) * T::BN + col];
#pragma unroll
                    for (int sl = 0; sl < FOLD_SLOTS; ++sl)
                        if (slot[e] == sl) t[sl] += v;
                }
#pragma unroll
                for (int sl = 0; sl < FOLD_SLOTS; ++sl)
                    if (img0 + sl <= imgL) rec[(((size_t)rt * FOLD_SLOTS + sl) * FOLD_Q + q) * M + off + n0 + col] = t[sl];
            }
            __syncthreads();
        }
    }
}

// Weight-gradient GEMMs: workgroups per CU the register budget must allow (per-workgroup timelines, round 4: the 7-tile variants
// took 260 / 248 registers -> ONE workgroup per CU, a 330-workgroup launch ran as two rounds of 65 us with every SIMD waiting on
// one wave's loads).  The split count below is sized to exactly these resident slots.
constexpr int wgrad_lb(int nt) { return nt >= 5 ? 2 : (nt >= 3 ? 3 : 4); }

// ============================================================================ project wgrad (TN, split-K)
// part[split][poff_g + o*mc + c] = sum_{p in split} dP_g[p][o] * z_g[p][c]   (k_reduce_rows sums the splits)
// tile: M side = mid channels c (128), N side = output channels o (16*NT)
template <int NT, int ACT>
__global__ __launch_bounds__(256, wgrad_lb(NT)) void k_project_wgrad(TfnasCellDesc d, const float* __restrict__ dout,
                                                       const float* __restrict__ Pr, const float* __restrict__ D,
                                                       const float* __restrict__ gate,
                                                       const double* __restrict__ stats2,
                                                       const double* __restrict__ stats3,
                                                       const double* __restrict__ red3,
                                                       const float* __restrict__ wmix, int rows_per_split,
                                                       int ntiles_o, float* __restrict__ part, size_t out_size) {
    using T = GT<NT>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int g = blockIdx.z / ntiles_o, n0 = (blockIdx.z % ntiles_o) * T::BN;
    const int mc = d.g[g].mc, mcp = d.g[g].mcp, off = d.g[g].off;
    const bool has_se = d.g[g].se > 0;
    const float* gbase = has_se ? gate : D;
    const size_t se01 = has_se ? 1 : 0;
    size_t poff = 0;
    for (int gg = 0; gg < g; ++gg) poff += (size_t)d.g[gg].mc * d.oc;
    float* __restrict__ gw = part + (size_t)blockIdx.x * out_size + poff;
    const int m0 = blockIdx.y * 128;
    if (m0 >= mcp) return;
    const int HW = d.Ho * d.Wo, Po = d.N * HW, oc = d.oc, M = d.M;
    const int ocp = (oc + 15) & ~15;
    const int r0 = blockIdx.x * rows_per_split, r1 = min(Po, r0 + rows_per_split);
    const int nchunks = (r1 - r0 + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4, wrow = (tid >> 6) * 32;

    const Bn3Tab tab = bn3_tab_fill(lds + T::LDS_FLOATS, ocp, d, g, stats3, red3, wmix);
    // A thread stages the same 4 mid channels (A) and the same 4 output channels per B item in every K-chunk; only the
    // pixel advances (by 16 per chunk).  Everything that depends on the channel alone lives in registers: the loaders of
    // this kernel are VALU-issue bound (200 VALU instructions per 16 MFMAs before this), not bandwidth bound.
    const int mch = m0 + (tid & 31) * 4;
    const bool chok = mch < mcp;
    const size_t acol = (size_t)off + min(mch, mcp - 4);
    float2 c2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        c2[j] = (mch + j < mc) ? bn_consts(stats2 + 2 * (size_t)(off + mch + j), 1.0 / (double)Po, d.eps)
                               : make_float2(0.f, 0.f);
    __syncthreads();
    // BN3 backward with folded per-column constants:  dP = a3 (dOut - b3) - (Pr - mean) (rstd c3 a3)
    constexpr int BQ = T::BN / 4;
    int bcol[T::B_ITERS];
    bool bok[T::B_ITERS];
    f32x4 k_mean[T::B_ITERS], k_a3[T::B_ITERS], k_ab[T::B_ITERS], k_s[T::B_ITERS];
#pragma unroll
    for (int i = 0; i < T::B_ITERS; ++i) {
        const int idx = tid + 256 * i, o = n0 + (idx % BQ) * 4;
        bok[i] = idx < T::B_ITEMS && o < oc;
        bcol[i] = min(o, oc - 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int oo = bcol[i] + j;
            k_mean[i][j] = tab.mean[oo];
            k_a3[i][j] = tab.a3[oo];
            k_ab[i][j] = tab.a3[oo] * tab.b3[oo];
            k_s[i][j] = tab.rstd[oo] * tab.c3[oo] * tab.a3[oo];
        }
    }
    const float inv_hw = 1.f / (float)HW;
    const bool small_p = Po < (1 << 24);
    auto image_of = [&](int p) -> int {       // p / HW without the 22-instruction integer division (exact for p < 2^24)
        if (!small_p) return p / HW;
        int q = (int)((float)p * inv_hw);
        const int r = p - q * HW;
        q += (r >= HW) ? 1 : 0;
        q -= (r < 0) ? 1 : 0;
        return q;
    };

    f32x4 acc[2][NT];
    acc_zero<NT>(acc);
    auto la = [&](int c, int i, int kl, int m) -> Raw2 {
        const int p = min(r0 + c * 16 + kl, r1 - 1);
        Raw2 r;
        r.a = ld4(D + ((size_t)p * M + acol));
        r.b = ld4(gbase + ((size_t)image_of(p) * M + acol) * se01);        // no SE: one fixed (ignored) quad
        return r;
    };
    auto xa = [&](Raw2 r, int c, int i, int kl, int m) -> f32x4 {
        f32x4 v = r.a;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = act_f<ACT>((v[j] - c2[j].x) * c2[j].y);
        if (has_se) v *= r.b;
        return (chok && r0 + c * 16 + kl < r1) ? v : zero4();
    };
    auto lb = [&](int c, int i, int kl, int n) -> Raw2 {
        const int p = min(r0 + c * 16 + kl, r1 - 1);
        Raw2 r;
        r.a = ld4(dout + (size_t)p * oc + bcol[i]);
        r.b = ld4(Pr + ((size_t)g * Po + p) * oc + bcol[i]);
        return r;
    };
    auto xb = [&](Raw2 r, int c, int i, int kl, int n) -> f32x4 {
        const f32x4 v = (k_a3[i] * r.a - k_ab[i]) - (r.b - k_mean[i]) * k_s[i];
        return (bok[i] && r0 + c * 16 + kl < r1) ? v : zero4();
    };
    gemm_mainloop2<NT, false, false, false>(la, xa, lb, xb, nchunks, acc, lds);
    // The gradient is [oc][mc] (mid channel fastest) and a lane's accumulator quad is 4 consecutive mid channels of one
    // output channel: one 16-byte store per quad (the four lane groups of an output channel then cover 64 contiguous
    // bytes) instead of four 4-byte stores that each scatter a wave over 64 different cache lines.
    const bool vec = (mc & 3) == 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ch0 = m0 + wrow + 16 * i + 4 * lq;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int o = n0 + 16 * j + lr;
            if (o >= oc) continue;
            float* dst = gw + (size_t)o * mc + ch0;
            if (vec && ch0 + 3 < mc) {
                st4(dst, acc[i][j]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ch0 + r < mc) dst[r] = acc[i][j][r];
            }
        }
    }
}

// ---------------------------------------------------------------------------- BN1-backward operand
// de[p][c] = rstd1 * (deh - T1/P - ehat*T2/P), ehat = (E-mean1)*rstd1, deh = dA1*act'(ehat) (stored by the
// depthwise-backward kernel);  cb1[c] = (mean1, rstd1, T1/P, T2/P)
__device__ __forceinline__ f32x4 bn1_de(const f32x4* cb, f32x4 deh, f32x4 e) {
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 t = cb[j];
        const float eh = (e[j] - t.x) * t.y;
        r[j] = t.y * (deh[j] - t.z - eh * t.w);
    }
    return r;
}

// (sink_add, the separately rounded dx + w*g of the sink-connecting gradient: tfnas_dev.h)

// ============================================================================ expand dgrad, without reading E
// dx[p][c] = sum_m de[p][m] * W[m][c]  (+ sumw * dout[p][c] for residual cells),  m over all mid channels of all groups,
//   de = rstd * (deh - t1 - ehat*t2),  ehat = (E - mu) * rstd,  (mu, rstd, t1, t2) = cb1[m]   (BN1 backward).
// E is itself linear in x (E[p][m] = sum_c' x[p][c'] W[m][c']), so the ehat term collapses to an ic x ic operator:
//   dx = deh (rstd.W)  -  x G  +  b,      G[c'][c] = sum_m W[m][c'] s_m W[m][c],   s_m = rstd_m^2 t2_m,
//                                          b[c]    = sum_m (s_m mu_m - rstd_m t1_m) W[m][c].
// The kernel therefore streams ONE [P][M] tensor (deh) with plain loads instead of two with a BN transform per element,
// scales the (small) weight operand by rstd, and appends ceil(ic/16) K-chunks whose A operand is x and whose B operand
// is -G; b is added in the epilogue.  G | b come from k_expand_gram ([ic+4][ic] floats, row ic = b).
// K (up to 6912) is split over blockIdx.z when the output grid alone cannot fill the chip (7x7 / 14x14 cells: 49..196 row
// tiles): split z writes its partial tile to dxp[z] and k_dx_reduce adds them (and b, and the residual term).
template <int NT, int MM>
__global__ __launch_bounds__(256, gemm_lb(NT, MM)) void k_expand_dgrad(TfnasCellDesc d, const float* __restrict__ dEh,
                                                      const float* __restrict__ x, const float* __restrict__ cb1,
                                                      const float* __restrict__ gram, const float* __restrict__ dout,
                                                      const float* __restrict__ wmix, float* __restrict__ dx,
                                                      float* __restrict__ dxp, int nsplit,
                                                      const float* __restrict__ add_src,
                                                      const float* __restrict__ add_scale, int xonly_slot = -1) {
    using T = GT<NT>;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    const int n0 = blockIdx.y * T::BN;
    const int P = d.N * d.H * d.W, ic = d.ic, M = d.M;
    const int nrt = (P + 127) >> 7;
    const int tid = threadIdx.x, lr = tid & 15, wrow = (tid >> 6) * 32;
    const int zs = (int)blockIdx.z;
    int mchunks = 0;
    for (int g = 0; g < d.G; ++g) mchunks += (d.g[g].mcp + 15) >> 4;
    const int nchunks_all = mchunks + ((ic + 15) >> 4);      // mid-channel chunks, then the x / -G chunks
    // xonly_slot >= 0 (fused per-image route, fx_kernels.hip: the dE (rstd . W) term already sits in dxp[0 .. xonly_slot) as
    // partial sums): only the trailing x / -G chunks, written as one more partial tile dxp[xonly_slot]; k_dx_reduce adds them up
    const bool xonly = xonly_slot >= 0;
    const int per = xonly ? nchunks_all - mchunks : (nchunks_all + nsplit - 1) / nsplit;
    const int cbeg = xonly ? mchunks : zs * per;
    const int nchunks = max(0, min(nchunks_all, cbeg + per) - cbeg);
    float* __restrict__ dst = xonly ? dxp + (size_t)xonly_slot * P * ic : (nsplit > 1 ? dxp + (size_t)blockIdx.z * P * ic : dx);
    const bool plain = nsplit == 1 && !xonly;
    const bool add_res = d.has_res && plain;
    const bool add_sink = add_src != nullptr && plain;
    const float sink_w = add_src ? add_scale[0] : 0.f;
    float sumw = 1.f;
    if (wmix) {
        sumw = 0.f;
        for (int g = 0; g < d.G; ++g) sumw += wmix[g];
    }

    for (int rt = blockIdx.x; rt < nrt; rt += gridDim.x) {
        f32x4 acc[2][NT];
        acc_zero<NT>(acc);
        // chunk -> operand sources, worked out once per chunk (pre) for the four loader pieces: mid-channel chunks of
        // group g read dEh / rstd-scaled W_g, the trailing chunks read x / -G
        bool is_x;                       // chunk of the x / -G part
        int k0, klim_a, klim_b, ld_a;    // first k of the chunk; valid k of A (mcp | ic) and of B (mc | ic); A row stride
        size_t aoff;                     // element offset of the group's columns in a dEh row
        const float* bsrc;               // W_g or G
        const float* ssrc;               // rstd of the group's channels (cb1[...].y), stride 4
        auto pre = [&](int c) {
            c += cbeg;
            if (c >= mchunks) {
                is_x = true;
                k0 = (c - mchunks) * 16;
                klim_a = klim_b = ld_a = ic;
                aoff = 0;
                bsrc = gram;
                ssrc = cb1 + 1;
                return;
            }
            int g = 0;
            for (; g < d.G - 1; ++g) {
                const int t = (d.g[g].mcp + 15) >> 4;
                if (c < t) break;
                c -= t;
            }
            is_x = false;
            k0 = c * 16;
            klim_a = d.g[g].mcp;
            klim_b = d.g[g].mc;
            ld_a = M;
            aoff = d.g[g].off;
            bsrc = d.g[g].w_expand;
            ssrc = cb1 + 4 * (size_t)d.g[g].off + 1;
        };
        int prow[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) prow[i] = rt * 128 + wrow + 16 * i + lr;
        auto la = [&](int c, int i, int kl) -> f32x4 {
            const int pc = min(prow[i], P - 1), k = min(k0 + kl, klim_a - 4);
            return ld4((is_x ? x : dEh) + (size_t)pc * ld_a + aoff + k);       // wave-uniform select, one unconditional load
        };
        auto xa = [&](f32x4 r, int c, int i, int kl) -> f32x4 {
            return (prow[i] < P && k0 + kl < klim_a) ? r : zero4();
        };
        auto lb = [&](int c, int kl, int n) -> RawWS {
            const int kc = min(k0 + kl, klim_b - 1), col = min(n0 + n, ic - 4);
            RawWS r;
            r.w = ld4(bsrc + (size_t)kc * ic + col);
            r.s = ssrc[is_x ? 0 : 4 * (size_t)kc];      // rstd only: a dword load (a quad whose other lanes die lets their
                                                        // registers be reused before the MFMAs -> a wait); ignored for -G
            return r;
        };
        auto xb = [&](RawWS r, int c, int kl, int n) -> f32x4 {
            const f32x4 v = is_x ? -r.w : splat4(r.s) * r.w;
            return (n0 + n < ic && k0 + kl < klim_b) ? v : zero4();
        };
        gemm_adirect<NT, false, MM>(pre, la, xa, lb, xb, nchunks, acc, lds);
        // (the staging indices derive from a copy of the thread index taken afresh per tile: see k_project_dgrad)
        int te = tid;
        asm volatile("" : "+v"(te));
        emit_tile_rows<NT>(acc, lds, [&](int lrow, int lc, f32x4 v) {
            const int p = rt * 128 + lrow, c = n0 + lc;
            if (p < P && c < ic) {
                if (plain) v += ld4(gram + (size_t)ic * ic + c);
                if (add_res) v += splat4(sumw) * ld4(dout + (size_t)p * d.oc + c);
                if (add_sink) v = sink_add(v, sink_w, ld4(add_src + (size_t)p * ic + c));
                st4(dst + (size_t)p * ic + c, v);
            }
        }, SlabNone(), te);
    }
}

// dx = sum_z dxp[z] + b (+ sumw * dout for residual cells) (+ add_scale * add_src: sink-connecting gradient)
__global__ __launch_bounds__(256) void k_dx_reduce(TfnasCellDesc d, const float* __restrict__ dxp, int nsplit,
                                                   const float* __restrict__ gram, const float* __restrict__ dout,
                                                   const float* __restrict__ wmix, float* __restrict__ dx,
                                                   const float* __restrict__ add_src,
                                                   const float* __restrict__ add_scale) {
    const float sink_w = add_src ? add_scale[0] : 0.f;
    const size_t n4 = (size_t)d.N * d.H * d.W * d.ic / 4;
    const int iq = d.ic / 4;
    const float* __restrict__ bias = gram + (size_t)d.ic * d.ic;
    float sumw = 1.f;
    if (wmix) {
        sumw = 0.f;
        for (int g = 0; g < d.G; ++g) sumw += wmix[g];
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 v = ld4(bias + 4 * (int)(i % iq));
        if (d.has_res) v += splat4(sumw) * ld4(dout + 4 * i);
        for (int z = 0; z < nsplit; ++z) v += ld4(dxp + (size_t)z * n4 * 4 + 4 * i);
        if (add_src) v = sink_add(v, sink_w, ld4(add_src + 4 * i));
        st4(dx + 4 * i, v);
    }
}

// dx += (sum_g wmix[g]) * dout: the residual gradient of a cell whose groups differ in kind (kernels.h: cell_mixed), added ONCE
// after the last branch's data gradient (every branch runs with has_res = 0: the branches see sub-descriptors, whose group
// indices do not index wmix).  One more pass over dx [N*H*W][ic], the narrowest tensor of the backward; each element read and
// written by one thread.  wmix == NULL: weight 1.  G: the entries of wmix, skip groups included (launch_dx_add_res: nw).
__global__ __launch_bounds__(256) void k_dx_add_res(const float* __restrict__ dout, const float* __restrict__ wmix, int G,
                                                    float* __restrict__ dx, size_t n4) {
    float sumw = 1.f;
    if (wmix) {
        sumw = 0.f;
        for (int g = 0; g < G; ++g) sumw += wmix[g];
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256)
        st4(dx + 4 * i, ld4(dx + 4 * i) + splat4(sumw) * ld4(dout + 4 * i));
}
int launch_dx_add_res(const TfnasCellDesc& d, int nw, const float* dout, const float* wmix, float* dx, hipStream_t s) {
    if (!d.has_res || !dout || !dx) return TFNAS_EINVAL;
    const size_t n4 = (size_t)d.N * d.H * d.W * d.ic / 4;
    size_t gx = (n4 + 255) / 256;
    if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(k_dx_add_res, dim3((unsigned)gx), dim3(256), 0, s, dout, wmix, nw, dx, n4);
    return (int)hipGetLastError();
}

// ============================================================================ BN1-backward correction operator
// part[split][(ic+4)*ic]:  rows c' < ic: G[c'][c] = sum_m W[m][c'] s_m W[m][c];  row ic: b[c] = sum_m coef_m W[m][c];
// s_m = rstd_m^2 t2_m, coef_m = s_m mu_m - rstd_m t1_m   (see k_expand_dgrad).  GEMM rows = input channels (+ the b row),
// columns = input channels, K = all mid channels of all groups, split over blockIdx.x (k_reduce_rows sums the splits).
template <int NT>
__global__ __launch_bounds__(256) void k_expand_gram(TfnasCellDesc d, const float* __restrict__ cb1, int chunks_per_split,
                                                     int nsplit, float* __restrict__ part) {
    using T = GT<NT>;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    const int ic = d.ic;
    const int m0 = blockIdx.y * 128, n0 = blockIdx.z * T::BN;
    const int xs = (int)blockIdx.x;             // K-split: partial tile at part[blockIdx.x]
    int mchunks = 0;
    for (int g = 0; g < d.G; ++g) mchunks += (d.g[g].mcp + 15) >> 4;
    const int cbeg = xs * chunks_per_split;
    const int nchunks = max(0, min(mchunks, cbeg + chunks_per_split) - cbeg);
    const f32x4* cb = reinterpret_cast<const f32x4*>(cb1);
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4, wrow = (tid >> 6) * 32;
    float* __restrict__ out = part + (size_t)blockIdx.x * (size_t)(ic + 4) * ic;

    f32x4 acc[2][NT];
    acc_zero<NT>(acc);
    auto locate = [&](int c, int& g, int& k0) {
        c += cbeg;
        g = 0;
        for (; g < d.G - 1; ++g) {
            const int t = (d.g[g].mcp + 15) >> 4;
            if (c < t) break;
            c -= t;
        }
        k0 = c * 16;
    };
    auto fa = [&](int c, int kl, int m) -> f32x4 {       // A(m..m+3, k) = s_k W[k][m..m+3]; row ic = coef_k
        int g, k0;
        locate(c, g, k0);
        const int k = k0 + kl, r = m0 + m;
        if (k >= d.g[g].mc || r > ic) return zero4();
        const f32x4 t = cb[d.g[g].off + k];
        const float sk = t.y * t.y * t.w;
        if (r == ic) {
            f32x4 v = zero4();
            v.x = sk * t.x - t.y * t.z;
            return v;
        }
        return splat4(sk) * ld4(d.g[g].w_expand + (size_t)k * ic + r);
    };
    auto fb = [&](int c, int kl, int n) -> f32x4 {
        int g, k0;
        locate(c, g, k0);
        const int k = k0 + kl;
        return (k < d.g[g].mc && n0 + n < ic) ? ld4(d.g[g].w_expand + (size_t)k * ic + n0 + n) : zero4();
    };
    gemm_mainloop<NT, false, false>(fa, fb, nchunks, acc, lds);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + wrow + 16 * i + 4 * lq + r;
            if (row <= ic) {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int cc = n0 + 16 * j + lr;
                    if (cc < ic) out[(size_t)row * ic + cc] = acc[i][j][r];
                }
            }
        }
}

// One-launch form of the same operator (round 6; the default -- TFNAS_ROUTE_GRAM2 selects the split-K GEMM + reduction above).
// G | b is tiny (ic <= 320, K = all mid channels: 6..130 MFLOP) and sits on the data-gradient chain of EVERY cell between the
// BN1-backward reduction and k_expand_dgrad; as a 128-row LDS-tiled GEMM split over K plus a k_reduce_rows launch it cost 13..28 us
// + 5 us per cell (w-step trace, round 6: 40 + 40 launches, 0.9 ms of chain time per w-step).  Here a workgroup owns a 16 x 32 tile
// of the output; its waves take batches of 32 mid channels round-robin, a lane loads its own MFMA operands straight from W
// (A[i][k] = s_k W[k][r0 + i], B[k][j] = W[k][c0 + j]: 64-byte row pieces, W stays in L2), a batch of GB steps' loads is in flight
// before their v_mfma_f32_16x16x4_f32; the waves' partial tiles are summed in double through LDS in wave order
// (deterministic).  The kernel is bound by its dependent load rounds (~1.5 us each).
#ifndef GRAM1_MAX_K
#define GRAM1_MAX_K 1536
#endif
constexpr int GRAM1_GB = 8;
// GRAM1_NW waves per workgroup: 4 inside the cells' backward (four queues keep every CU busy there: a 1 024-thread workgroup waits
// for a whole CU to drain -- in situ 44 us on average, 400 us worst case, against 17 us for the 256-thread form, rocprofv3 statistics
// of round 6), 16 for the head (K = 1 280, in the quiet stretch between the paths' forward and backward: 25-70 -> 10 us)
template <int GRAM1_NW>
__global__ __launch_bounds__(64 * GRAM1_NW) void k_gram1(TfnasCellDesc d, const float* __restrict__ cb1, float* __restrict__ gram) {
    __shared__ float part[GRAM1_NW][2][16][17];
    const int ic = d.ic;
    const int r0 = blockIdx.y * 16, c0 = blockIdx.x * 32;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, kq = lane >> 4;
    const f32x4* cb = reinterpret_cast<const f32x4*>(cb1);
    const int r = r0 + li, ca = c0 + li, cb_ = c0 + 16 + li;
    const bool row_w = r < ic, row_b = r == ic, oka = ca < ic, okb = cb_ < ic;
    const int ra = row_w ? r : 0, caa = oka ? ca : 0, cbb = okb ? cb_ : 0;      // clamped addresses, values masked below
    f32x4 acc0 = zero4(), acc1 = zero4();
    // the waves take batches of GB steps (4 mid channels each) round-robin over the concatenation of all groups' steps
    int base = 0;                                   // batches before this group
    for (int g = 0; g < d.G; ++g) {
        const float* __restrict__ W = d.g[g].w_expand;
        const int mc = d.g[g].mc, off = d.g[g].off;
        const int nstep = (mc + 3) >> 2, nbatch = (nstep + GRAM1_GB - 1) / GRAM1_GB;
        // first batch of this group that belongs to this wave: (base + b) % NW == wave
        int b = (wave - base % GRAM1_NW + GRAM1_NW) % GRAM1_NW;
        for (; b < nbatch; b += GRAM1_NW) {
            const int s0 = b * GRAM1_GB;
            float a[GRAM1_GB], b0[GRAM1_GB], b1[GRAM1_GB];
            f32x4 t[GRAM1_GB];
#pragma unroll
            for (int u = 0; u < GRAM1_GB; ++u) {
                const int m = 4 * (s0 + u) + kq;
                const int mm = m < mc ? m : mc - 1;
                const float* wr = W + (size_t)mm * ic;
                t[u] = cb[off + mm];
                a[u] = wr[ra];
                b0[u] = wr[caa];
                b1[u] = wr[cbb];
            }
#pragma unroll
            for (int u = 0; u < GRAM1_GB; ++u) {
                const int m = 4 * (s0 + u) + kq;
                const bool okm = m < mc;
                const float sk = t[u].y * t[u].y * t[u].w;
                float av = row_w ? sk * a[u] : (row_b ? sk * t[u].x - t[u].y * t[u].z : 0.f);
                av = okm ? av : 0.f;
                const float bv0 = (okm && oka) ? b0[u] : 0.f, bv1 = (okm && okb) ? b1[u] : 0.f;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv1, acc1, 0, 0, 0);
            }
        }
        base += nbatch;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        part[wave][0][4 * kq + q][li] = acc0[q];
        part[wave][1][4 * kq + q][li] = acc1[q];
    }
    __syncthreads();
    for (int e = tid; e < 512; e += 64 * GRAM1_NW) {
        const int h = e >> 8, row = (e >> 4) & 15, col = e & 15;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < GRAM1_NW; ++w) v += (double)part[w][h][row][col];          // (wave order: deterministic)
        const int rr = r0 + row, cc = c0 + 16 * h + col;
        if (rr <= ic && cc < ic) gram[(size_t)rr * ic + cc] = (float)v;
    }
}

// ============================================================================ expand wgrad (TN, split-K)
// XG = false (stem; TFNAS_XG=0):  part[split][poff_g + m*ic + c] = sum_{p in split} de[p][off_g+m] * x[p][c]  with the
//   BN1-backward operand de = rstd (deh - t1 - ehat t2) formed per element from dEh AND E (k_reduce_rows sums the splits).
// XG = true (default): E is not read.  E is linear in x (E[p][m] = sum_c' W[m][c'] x[p][c']), so
//   sum_p de[p][m] x[p][c] = r_m ( R[m][c] - t1_m sx[c] - t2_m r_m ( (W Gx)[m][c] - mu_m sx[c] ) ),
//   R = sum_p deh x^T,  Gx = sum_p x x^T (ic x ic),  sx = sum_p x,  (mu, r, t1, t2) = cb1[m]
// and the kernel streams ONE [P][M] tensor with plain loads: the rows of R, and -- as ic + 1 more "mid channels" behind the
// last group's rows (operand = x itself / the constant 1) -- the rows of Gx | sx.  k_reduce_rows sums the splits in double,
// k_expand_wgrad_fix applies the formula in double (autograd of inverted_bottleneck.conv + BatchNorm2d, layers.py:463-482).
template <int NT, bool STEM, bool XG>
__global__ __launch_bounds__(256, wgrad_lb(NT)) void k_expand_wgrad(TfnasCellDesc d, const float* __restrict__ dEh,
                                                      const float* __restrict__ E, const float* __restrict__ cb1,
                                                      const float* __restrict__ x, int rows_per_split,
                                                      float* __restrict__ part, size_t out_size, size_t out_main) {
    using T = GT<NT>;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    const int ic = d.ic;
    int ty = blockIdx.y, g = 0;
    for (; g < d.G - 1; ++g) {
        const int t = (d.g[g].mcp + 127) >> 7;
        if (ty < t) break;
        ty -= t;
    }
    const int mc = d.g[g].mc, mcp = d.g[g].mcp, off = d.g[g].off;
    const bool last = XG && g == d.G - 1;           // the group whose row space carries the ic + 1 extension rows
    size_t poff = 0;
    for (int gg = 0; gg < g; ++gg) poff += (size_t)d.g[gg].mc * ic;
    float* __restrict__ gw = part + (size_t)blockIdx.x * out_size + poff;
    float* __restrict__ gx = part + (size_t)blockIdx.x * out_size + out_main;
    const int m0 = ty * 128, n0 = blockIdx.z * T::BN;
    const int P = d.N * d.H * d.W, M = d.M;
    const int r0 = blockIdx.x * rows_per_split, r1 = min(P, r0 + rows_per_split);
    const int nchunks = (r1 - r0 + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4, wrow = (tid >> 6) * 32;

    // per-thread constants of the K loop (see k_project_wgrad): the thread's 4 mid channels and its BN1-backward constants,
    // folded:  de = rstd (deh - t1 - (E - mu) rstd t2)  =  rstd deh - rstd t1 - (E - mu) (rstd^2 t2)
    const int mch = m0 + (tid & 31) * 4;
    const bool chok = mch < mcp;
    const size_t acol = (size_t)off + min(mch, mcp - 4);
    f32x4 k_mu = zero4(), k_r = zero4(), k_rt1 = zero4(), k_s = zero4();
    if (!XG) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 t = (mch + j < mcp) ? reinterpret_cast<const f32x4*>(cb1)[off + mch + j] : zero4();
            k_mu[j] = t.x;
            k_r[j] = t.y;
            k_rt1[j] = t.y * t.z;
            k_s[j] = t.y * t.y * t.w;
        }
    }
    // XG: one base pointer and row pitch per thread -- its quad of dEh columns, or (extension rows) its quad of x columns
    const int ext = mch - mcp;                       // >= 0: extension row (x channel `ext`; ext == ic: the constant 1)
    const bool ax = last && ext >= 0 && ext < ic, aone = last && ext == ic;
    const float* __restrict__ abase = ax ? x + ext : dEh + acol;
    const size_t apitch = ax ? (size_t)ic : (size_t)M;
    const bool aok = chok || ax;
    constexpr int BQ = T::BN / 4;
    int bcol[T::B_ITERS];
    bool bok[T::B_ITERS];
#pragma unroll
    for (int i = 0; i < T::B_ITERS; ++i) {
        const int idx = tid + 256 * i, cc = n0 + (idx % BQ) * 4;
        bok[i] = idx < T::B_ITEMS && cc < ic;
        bcol[i] = STEM ? cc : min(cc, ic - 4);
    }

    f32x4 acc[2][NT];
    acc_zero<NT>(acc);
    auto la = [&](int c, int i, int kl, int m) -> Raw2 {
        const int p = min(r0 + c * 16 + kl, r1 - 1);
        Raw2 r;
        if (XG) {
            r.a = ld4(abase + (size_t)p * apitch);
            r.b = r.a;
        } else {
            const size_t at = (size_t)p * M + acol;
            r.a = ld4(dEh + at);
            r.b = ld4(E + at);
        }
        return r;
    };
    auto xa = [&](Raw2 r, int c, int i, int kl, int m) -> f32x4 {
        if (XG) {
            f32x4 v = aok ? r.a : zero4();
            if (aone) v.x = 1.f;
            return (r0 + c * 16 + kl < r1) ? v : zero4();
        }
        const f32x4 v = (k_r * r.a - k_rt1) - (r.b - k_mu) * k_s;
        return (chok && r0 + c * 16 + kl < r1) ? v : zero4();
    };
    auto lb = [&](int c, int i, int kl, int n) -> f32x4 {
        if (STEM) {
            const int p = r0 + c * 16 + kl;
            return (p < r1 && bok[i]) ? stem_patch4(x, d, p, bcol[i]) : zero4();
        }
        const int p = min(r0 + c * 16 + kl, r1 - 1);
        return ld4(x + (size_t)p * ic + bcol[i]);
    };
    auto xb = [&](f32x4 r, int c, int i, int kl, int n) -> f32x4 {
        if (STEM) return r;
        return (bok[i] && r0 + c * 16 + kl < r1) ? r : zero4();
    };
    gemm_mainloop2<NT, false, false, false>(la, xa, lb, xb, nchunks, acc, lds);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ch = m0 + wrow + 16 * i + 4 * lq + r;
            float* __restrict__ row = nullptr;
            if (ch < mc) row = gw + (size_t)ch * ic;
            else if (last && ch >= mcp && ch - mcp <= ic) row = gx + (size_t)(ch - mcp) * ic;
            if (row) {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int cc = n0 + 16 * j + lr;
                    if (cc < ic) row[cc] = acc[i][j][r];
                }
            }
        }
}

// red: the split sums of k_expand_wgrad<XG> in double -- R of every group | Gx [ic][ic] | sx [ic]
//   g_expand_g[m][c] = r ( R - t1 sx[c] - t2 r ( sum_c' W[m][c'] Gx[c'][c] - mu sx[c] ) ),   (mu, r, t1, t2) = cb1[off_g + m]
// A workgroup owns 64 consecutive outputs; the four waves take interleaved quarters of the c' sum (combined through LDS in
// wave order: bit-reproducible).
__global__ __launch_bounds__(256) void k_expand_wgrad_fix(TfnasCellDesc d, const float* __restrict__ cb1,
                                                          const double* __restrict__ red, size_t out_main) {
    __shared__ double ps[4][64];
    const int ic = d.ic, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t e = (size_t)blockIdx.x * 64 + lane;
    const bool ok = e < out_main;
    int g = 0;
    size_t poff = 0;
    for (; g < d.G - 1; ++g) {
        const size_t n = (size_t)d.g[g].mc * ic;
        if (e < poff + n) break;
        poff += n;
    }
    const int m = ok ? (int)((e - poff) / ic) : 0, c = ok ? (int)(e - poff - (size_t)m * ic) : 0;
    const double* __restrict__ Gx = red + out_main;
    const float* __restrict__ w = d.g[g].w_expand + (size_t)m * ic;
    double wg0 = 0.0, wg1 = 0.0;
    for (int k = 4 * wv; k < ic; k += 16) {            // ic % 4 == 0 (cells; the stem keeps the per-element form)
        const f32x4 wq = ld4(w + k);
        wg0 += (double)wq.x * Gx[(size_t)k * ic + c] + (double)wq.z * Gx[(size_t)(k + 2) * ic + c];
        wg1 += (double)wq.y * Gx[(size_t)(k + 1) * ic + c] + (double)wq.w * Gx[(size_t)(k + 3) * ic + c];
    }
    ps[wv][lane] = wg0 + wg1;
    __syncthreads();
    if (wv == 0 && ok) {
        const double wg = (ps[0][lane] + ps[1][lane]) + (ps[2][lane] + ps[3][lane]);
        const f32x4 t = reinterpret_cast<const f32x4*>(cb1)[d.g[g].off + m];
        const double sx = Gx[(size_t)ic * ic + c], mu = t.x, r = t.y, t1 = t.z, t2 = t.w;
        const float v = (float)(r * (red[e] - t1 * sx - t2 * r * (wg - mu * sx)));
        float* __restrict__ o = d.g[g].g_expand + (e - poff);
        *o = (d.flags & TFNAS_CELL_ACCUM_WGRAD) ? *o + v : v;
    }
}

// ============================================================================ host: launch plans and launchers
// (gemm_plan_* fill a GemmPlan, kernels.h; the family's launcher carries it out: one dispatch, then the reductions)
static const int kNtSmall[] = {1, 2, 3, 4, 5, 7};   // N extents that are channel counts (ic / oc)
static constexpr int kGtLdsFloats[8] = {0, GT<1>::LDS_FLOATS, GT<2>::LDS_FLOATS, GT<3>::LDS_FLOATS, GT<4>::LDS_FLOATS,
                                        GT<5>::LDS_FLOATS, 0, GT<7>::LDS_FLOATS};

#define NT_CASE(n, ...) case n: { constexpr int NT = n; __VA_ARGS__; } break;
// the group-tiled families (column tiles cannot straddle groups): pick_nt_groups only returns 4, 5 or 7
#define DISPATCH_NT_GROUPS(nt, ...)   \
    switch (nt) {                     \
        NT_CASE(4, __VA_ARGS__)       \
        NT_CASE(5, __VA_ARGS__)       \
        NT_CASE(7, __VA_ARGS__)       \
        default: return TFNAS_EINVAL; \
    }
#define DISPATCH_NT(nt, ...)                         \
    switch (nt) {                                    \
        NT_CASE(1, __VA_ARGS__)                      \
        NT_CASE(2, __VA_ARGS__)                      \
        NT_CASE(3, __VA_ARGS__)                      \
        default: DISPATCH_NT_GROUPS(nt, __VA_ARGS__) \
    }
#define DISPATCH_MM(mode, ...)                                 \
    switch (mode) {                                            \
        case 0: { constexpr int MM = 0; __VA_ARGS__; } break;  \
        case 1: { constexpr int MM = 1; __VA_ARGS__; } break;  \
        case 3: { constexpr int MM = 3; __VA_ARGS__; } break;  \
        default: { constexpr int MM = 6; __VA_ARGS__; } break; \
    }
#define DISPATCH_ACT(act, ...) ACT_DISPATCH(act, __VA_ARGS__)       // (kernels.h: four-way, any other value TFNAS_EINVAL)

// Arithmetic of the row-tiled 1x1-convolution GEMMs (gemm_x3.h): 6 = split-bf16 with six products per element pair (fp32-level
// accuracy on the bf16 matrix pipe; the default), 0 = v_mfma_f32_16x16x4_f32, 3 = split-bf16 keeping the 2^-16 terms,
// 1 = plain bf16.  tfnas_set_gemm_mode sets the process default (6 until then; the Python mirror seeds it from TFNAS_GEMM),
// with TFNAS_GEMM_EVERYWHERE: no per-launch shape policy (tests compare every mode with the oracle).
static int g_gemm_mode = 6;
int gemm_mode() { return g_gemm_mode & 7; }
int set_gemm_mode(int m) {
    const int base = m & ~TFNAS_GEMM_EVERYWHERE;
    if (base != 0 && base != 1 && base != 3 && base != 6) return TFNAS_EINVAL;
    g_gemm_mode = m;
    return 0;
}
// the launch's mode word: the descriptor's own (TFNAS_GEMM_EXPLICIT) or the process default
static inline int gemm_word(const TfnasCellDesc& d) { return (d.gemm_mode & TFNAS_GEMM_EXPLICIT) ? d.gemm_mode : g_gemm_mode; }
int gemm_mode_of(const TfnasCellDesc& d) { return gemm_word(d) & 7; }
// Which arithmetic this descriptor's launch of a pass runs.
// Ragged mid widths (mc % 4 != 0 after the elasticity re-masking): the split-bf16 instantiations only have the aligned weight
// loaders (the guarded ones cost ~50 registers, i.e. a resident workgroup), such launches keep the fp32 loop.
// The data-gradient GEMMs gain little from the bf16 pipe (their K loops are bound by the BN3-backward transform / the chunk ->
// group bookkeeping and, with one candidate or large images, by bytes): measured per cell at B = 128, split-bf16
// vs fp32 MFMA: all-candidate launches of the 14x14 / 7x7 cells 0.94-0.98x, 28x28 up to 1.19x, one-candidate launches 0.9-1.8x.
// They keep the fp32 loop except where they won.
static int gemm_arith(const TfnasCellDesc& d, bool dgrad) {
    for (int g = 0; g < d.G; ++g)
        if (d.g[g].mc & 3) return 0;
    const int m = gemm_mode_of(d);
    if (!dgrad || m == 0 || (gemm_word(d) & TFNAS_GEMM_EVERYWHERE)) return m;
    if (m == 1) return m;                                  // plain bf16 is a reduced-precision MODE, not a policy: everywhere
    return (d.G > 1 && d.Ho * d.Wo <= 196) ? m : 0;
}
static inline int gemm_slots(int nt, int mm) { return 256 * gemm_lb(nt, mm); }

// kernels with a statistics epilogue: at most 1024 partial rows (k_reduce_rows folds 512 per round trip) and they must fit
static size_t stats_row_cap(size_t row_floats) {
    const size_t fit = TFNAS_PART_FLOATS / (row_floats ? row_floats : 1);
    return fit < 1024 ? fit : 1024;
}

// Number of persistent row blocks (grid.x) of a row-tiled GEMM launch.  The launch runs gx * other workgroups on
// `slots` resident workgroup slots (256 CUs x 3 or 4 per CU, set by the kernel's launch bounds) and each workgroup walks
// ceil(nrt / gx) row tiles, so the launch takes about ceil(gx*other / slots) * ceil(nrt / gx) tile times.  The old rule
// (~4096 workgroups in total) left the 14x14 / 7x7 cells with a nearly empty last round (e.g. 2.04 rounds -> 3: 68 %
// efficient); this picks the gx that minimises the product, the larger gx on ties (finer dynamic balancing), subject to
// `cap` (partial rows of the statistics epilogues must fit the scratch buffer and stay <= 1024).
static int row_blocks(int rows, int other_blocks, size_t cap, int slots, int max_gx = 1024) {
    const int nrt = cdiv(rows, 128);
    const int other = other_blocks > 0 ? other_blocks : 1;
    int lim = nrt;
    if ((size_t)lim > cap) lim = (int)cap;
    if (lim > max_gx) lim = max_gx;                    // (bounds the host-side search; measured per kernel family)
    if (lim < 1) lim = 1;
    long best_cost = -1;
    int best = 1;
    for (int gx = 1; gx <= lim; ++gx) {
        const long cost = (long)cdiv(gx * other, slots) * cdiv(nrt, gx);
        if (best_cost < 0 || cost <= best_cost) {
            best_cost = cost;
            best = gx;
        }
    }
    return best;
}

// Column-tile width of the GEMMs whose N extent is the mid channels of EVERY group (tiles cannot straddle groups): the
// candidate that pads the group widths least (72 | 144 -> 5 x 16: 960 columns for 864, where 4 x 16 needs 1280 and
// 20 tiles instead of 12; 336 | 672 -> 7 x 16 exactly), the wider one on ties.
static int pick_nt_groups(const TfnasCellDesc& d) {
    // only for cells with narrow groups (the HBM-bound 56x56 / 28x28 cells): on the matrix-bound later cells the 64-wide
    // tile at 4 waves/SIMD beats the 80- / 112-wide ones at 3 even when those fit exactly (measured)
    int min_mcp = 1 << 30;
    for (int g = 0; g < d.G; ++g) min_mcp = d.g[g].mcp < min_mcp ? d.g[g].mcp : min_mcp;
    if (min_mcp >= 200) return 4;
    static const int cands[] = {4, 5, 7};
    int best = 4;
    long best_pad = -1;
    for (int i = 0; i < 3; ++i) {
        long pad = 0;
        for (int g = 0; g < d.G; ++g) pad += (long)cdiv(d.g[g].mcp, 16 * cands[i]) * 16 * cands[i];
        if (best_pad < 0 || pad < best_pad || (pad == best_pad && cands[i] > best)) {
            best_pad = pad;
            best = cands[i];
        }
    }
    return best;
}
// sums over the groups: tiles of `width` mid channels, widest group, floats of a [mc][n] weight per group
static int group_tiles(const TfnasCellDesc& d, int width, int last_extra = 0) {
    int t = 0;
    for (int g = 0; g < d.G; ++g) t += cdiv(d.g[g].mcp + (g == d.G - 1 ? last_extra : 0), width);
    return t;
}
static int max_mcp(const TfnasCellDesc& d) {
    int m = 0;
    for (int g = 0; g < d.G; ++g) m = d.g[g].mcp > m ? d.g[g].mcp : m;
    return m;
}
static size_t mid_floats(const TfnasCellDesc& d, int n) {
    size_t f = 0;
    for (int g = 0; g < d.G; ++g) f += (size_t)d.g[g].mc * n;
    return f;
}
// a plan whose N extent is a channel count (ic / oc): the width that pads it least
static GemmPlan plan_cols(int n) {
    GemmPlan p{};
    p.nt = pick_nt(n, kNtSmall, 6);
    p.tiles = cdiv(n, 16 * p.nt);
    return p;
}

GemmPlan gemm_plan_expand_fwd(const TfnasCellDesc& d) {
    GemmPlan p{};
    p.var = d.mode == TFNAS_MODE_STEM ? GEMM_STEM : GEMM_PLAIN;
    // stem: 32 output channels -> 32-wide tiles (a 64-wide tile would be half empty)
    p.nt = p.var == GEMM_STEM ? (d.g[0].mcp <= 32 ? 2 : 4) : pick_nt_groups(d);
    p.mm = gemm_arith(d, false);
    p.tiles = group_tiles(d, 16 * p.nt);
    p.grid = dim3(row_blocks(d.N * d.H * d.W, p.tiles, stats_row_cap(2 * (size_t)d.M), gemm_slots(p.nt, p.mm)), p.tiles);
    return p;
}

int launch_expand_fwd(const TfnasCellDesc& d, const float* x, float* E, double* stats1, float* part,
                      hipStream_t s) {
    ProfScope _prof(TK_EXPAND_FWD, s);
    const GemmPlan p = gemm_plan_expand_fwd(d);
    DISPATCH_MM(p.mm, {
        if (p.var == GEMM_STEM)
            hipLaunchKernelGGL((p.nt == 2 ? k_expand_fwd<2, true, MM> : k_expand_fwd<4, true, MM>), p.grid, dim3(256), 0, s, d, x, E, part);
        else
            DISPATCH_NT_GROUPS(p.nt, { hipLaunchKernelGGL((k_expand_fwd<NT, false, MM>), p.grid, dim3(256), 0, s, d, x, E, part); })
    })
    _prof.stop();
    return reduce_pair_rows(d, part, p.grid.x, stats1, s);
}

// caps of the K-splits of the w-step's one-candidate launches (see gemm_plan_expand_dgrad); build flags, tools/README.md
#ifndef TFNAS_WSPLIT_DGRAD
#define TFNAS_WSPLIT_DGRAD 2
#endif
#ifndef TFNAS_WSPLIT_PFWD
#define TFNAS_WSPLIT_PFWD 2
#endif
GemmPlan gemm_plan_project_fwd(const TfnasCellDesc& d) {
    GemmPlan p = plan_cols(d.oc);
    p.mm = gemm_arith(d, false);
    const int mcp_max = max_mcp(d), ncols2 = 2 * d.G * d.oc;
    const int Po = d.N * d.Ho * d.Wo, nrt = cdiv(Po, 128);
    p.shm = (kGtLdsFloats[p.nt] + 2 * ((mcp_max + 15) & ~15)) * sizeof(float);
    // K-split for under-filled launches (sampled mode on the 14x14 / 7x7 cells: 150-400 workgroups walking 30-72
    // K-chunks back to back at ~2 us per chunk -- one workgroup per CU cannot hide the load latency)
    int nsplit = 1;
    const int wgs = nrt * p.tiles * d.G, kch = cdiv(mcp_max, 16);
    if (wgs < 512 && kch >= 16 && (d.oc & 3) == 0 && d.oc <= 1024) {
        nsplit = cdiv(1024, wgs);
        if (nsplit > 4) nsplit = 4;
        if (nsplit > kch / 8) nsplit = kch / 8;
        if (d.need_wgrad && d.G == 1 && nsplit > TFNAS_WSPLIT_PFWD) nsplit = TFNAS_WSPLIT_PFWD;      // (see gemm_plan_expand_dgrad)
        const size_t per = (size_t)d.G * Po * d.oc, rows2 = 256 * (size_t)ncols2;
        while (nsplit > 1 && (nsplit - 1) * per + rows2 > TFNAS_PART_FLOATS) --nsplit;
    }
    p.splits = nsplit;
    p.parts = nsplit - 1;
    // split: every split takes all row tiles; k_pr_reduce adds the partial products and writes the statistics rows
    if (p.parts) p.grid = dim3(nrt, p.tiles, d.G * nsplit);
    else p.grid = dim3(row_blocks(Po, p.tiles * d.G, stats_row_cap((size_t)ncols2), gemm_slots(p.nt, p.mm)), p.tiles, d.G);
    int gx2 = cdiv(Po, 64);
    if (gx2 > 256) gx2 = 256;
    p.rps = cdiv(Po, gx2);
    p.grid2 = dim3(cdiv(Po, p.rps), d.G);
    return p;
}

int launch_project_fwd(const TfnasCellDesc& d, const float* D, const float* gate, const double* stats2,
                       float* Pr, double* stats3, float* part, hipStream_t s) {
    ProfScope _prof(TK_PROJECT_FWD, s);
    const GemmPlan p = gemm_plan_project_fwd(d);
    const int ncols2 = 2 * d.G * d.oc, Po = d.N * d.Ho * d.Wo;
    // split: the partial products of splits 1.. go to prp = `part`, the statistics rows of k_pr_reduce behind them
    float* prp = p.parts ? part : nullptr;
    float* rows = part + (size_t)p.parts * d.G * Po * d.oc;
    DISPATCH_MM(p.mm, DISPATCH_NT(p.nt, DISPATCH_ACT(d.act, {
        hipLaunchKernelGGL((k_project_fwd<NT, ACT, MM>), p.grid, dim3(256), p.shm, s, d, D, gate, stats2, Pr, part, p.splits, prp);
    })))
    if (p.parts) hipLaunchKernelGGL(k_pr_reduce, p.grid2, dim3(256), 0, s, Pr, prp, p.parts, d.G, Po, d.oc, p.rps, rows);
    _prof.stop();
    return launch_reduce_rows(rows, p.parts ? p.grid2.x : p.grid.x, ncols2, (size_t)ncols2, stats3, nullptr, s);
}

GemmPlan gemm_plan_project_dgrad(const TfnasCellDesc& d, bool fold) {
    GemmPlan p{};
    p.var = fold ? GEMM_FOLD : GEMM_PLAIN;
    p.nt = pick_nt_groups(d);
    p.mm = gemm_arith(d, true);
    p.tiles = group_tiles(d, 16 * p.nt);
    p.grid = dim3(row_blocks(d.N * d.Ho * d.Wo, p.tiles, 1u << 30, gemm_slots(p.nt, p.mm)), p.tiles);
    p.shm = (kGtLdsFloats[p.nt] + 4 * ((d.oc + 15) & ~15)) * sizeof(float);
    return p;
}

int launch_project_dgrad(const TfnasCellDesc& d, const float* dout, const float* Pr, const double* stats3,
                         const double* red3, const float* wmix, float* dZ, hipStream_t s, const float* D,
                         const double* stats2, float* rec) {
    ProfScope _prof(TK_PROJECT_DGRAD, s);
    if (rec && (!D || !stats2)) return TFNAS_ENULL;
    if (rec && d.act != TFNAS_ACT_RELU && d.act != TFNAS_ACT_SWISH) return TFNAS_EINVAL;     // (FOLD epilogue: project_fold_ok)
    const GemmPlan p = gemm_plan_project_dgrad(d, rec != nullptr);
    DISPATCH_MM(p.mm, DISPATCH_NT_GROUPS(p.nt, {
        if (p.var == GEMM_FOLD)
            hipLaunchKernelGGL((k_project_dgrad<NT, MM, true>), p.grid, dim3(256), p.shm, s, d, dout, Pr, stats3, red3, wmix, dZ,
                               D, stats2, rec);
        else
            hipLaunchKernelGGL((k_project_dgrad<NT, MM>), p.grid, dim3(256), p.shm, s, d, dout, Pr, stats3, red3, wmix, dZ);
    }))
    return (int)hipGetLastError();
}

// K-splits of a weight-gradient plan (nt, tiles, out set): grid = (splits, mtiles, ztiles), `scratch` floats for the partial tiles
static void plan_row_splits(GemmPlan& p, int rows, int mtiles, int ztiles, size_t scratch) {
    // ONE resident round: as many workgroups as the chip holds of this variant (256 CUs x wgrad_lb), never a second, mostly
    // empty round (cell 10: 55 splits x 6 tiles = 330 workgroups on 256 slots ran 2 x 65 us); at least 128 rows (8 K-chunks)
    // per split; partial tiles must fit the scratch
    const int target = 256 * wgrad_lb(p.nt), min_rows = 128, out_tiles = mtiles * ztiles;
    int splits = target / (out_tiles > 0 ? out_tiles : 1);
    const size_t cap = scratch / (p.out > 0 ? p.out : 1);
    if ((size_t)splits > cap) splits = (int)cap;
    if (splits < 1) splits = 1;
    int rps = cdiv(rows, splits);
    if (rps < min_rows) rps = min_rows;
    p.rps = ((rps + 15) / 16) * 16;
    p.splits = cdiv(rows, p.rps);
    p.grid = dim3(p.splits, mtiles, ztiles);
}
// the splits' partial weight gradients of every group -> its `dst` ([mc][n] floats per group, rows of p.out floats)
static int reduce_group_wgrads(const TfnasCellDesc& d, const GemmPlan& p, const float* part, int n, float* TfnasGroup::*dst,
                               hipStream_t s) {
    size_t poff = 0;
    for (int g = 0; g < d.G; ++g) {
        const int cols = d.g[g].mc * n;
        int rc = launch_reduce_rows(part + poff, p.splits, cols, p.out, nullptr, d.g[g].*dst, s, wgrad_accum(d));
        if (rc) return rc;
        poff += cols;
    }
    return (int)hipGetLastError();
}

GemmPlan gemm_plan_project_wgrad(const TfnasCellDesc& d) {
    GemmPlan p = plan_cols(d.oc);
    p.out = mid_floats(d, d.oc);
    plan_row_splits(p, d.N * d.Ho * d.Wo, cdiv(max_mcp(d), 128), p.tiles * d.G, TFNAS_PART_FLOATS);
    p.shm = (kGtLdsFloats[p.nt] + 5 * ((d.oc + 15) & ~15)) * sizeof(float);
    return p;
}

int launch_project_wgrad(const TfnasCellDesc& d, const float* dout, const float* Pr, const float* D,
                         const float* gate, const double* stats2, const double* stats3, const double* red3,
                         const float* wmix, float* part, hipStream_t s) {
    ProfScope _prof(TK_PROJECT_WGRAD, s);
    const GemmPlan p = gemm_plan_project_wgrad(d);
    DISPATCH_NT(p.nt, DISPATCH_ACT(d.act, {
        hipLaunchKernelGGL((k_project_wgrad<NT, ACT>), p.grid, dim3(256), p.shm, s, d, dout, Pr, D, gate, stats2,
                           stats3, red3, wmix, p.rps, p.tiles, part, p.out);
    }))
    _prof.stop();
    return reduce_group_wgrads(d, p, part, d.oc, &TfnasGroup::g_proj, s);
}

// floats of the correction operator G | b
size_t expand_gram_floats(const TfnasCellDesc& d) { return (size_t)(d.ic + 4) * d.ic; }
static int mid_chunks(const TfnasCellDesc& d) { return group_tiles(d, 16); }      // K-chunks over all mid channels of all groups

GemmPlan gemm_plan_expand_gram(const TfnasCellDesc& d, size_t scratch_floats) {
    GemmPlan p{};
    // policy (measured, B = 128, alternating bench runs): with the K of ONE candidate (the sampled launches of the w-step, the head)
    // the single launch wins; with all eight candidates' K (4 000 mid channels: 8 dependent load rounds per wave) it is at best equal
    // to the split-K GEMM + reduction (a 4-wave version: alpha-step +0.3 ms), which stays for those launches
    if (!(d.route & TFNAS_ROUTE_GRAM2) && mid_floats(d, 1) <= GRAM1_MAX_K) {
        // one launch, no K-split partials, no reduction (k_gram1); the scratch is not used
        p.var = GEMM_GRAM1;
        p.grid = dim3(cdiv(d.ic, 32), cdiv(d.ic + 1, 16));
        return p;
    }
    p = plan_cols(d.ic);
    const size_t gsz = expand_gram_floats(d);
    const int mchunks = mid_chunks(d), mtiles = cdiv(d.ic + 1, 128);
    int splits = cdiv(512, mtiles * p.tiles);
    if (splits > mchunks / 4) splits = mchunks / 4;               // at least 4 K-chunks per split
    if ((size_t)splits > scratch_floats / gsz) splits = (int)(scratch_floats / gsz);
    if (splits < 1) splits = 1;
    p.rps = cdiv(mchunks, splits);
    p.splits = cdiv(mchunks, p.rps);
    p.grid = dim3(p.splits, mtiles, p.tiles);
    return p;
}

// G | b -> gram ([ic+4][ic] floats); `scratch` holds the K-split partials (scratch_floats available)
int launch_expand_gram(const TfnasCellDesc& d, const float* cb1, float* scratch, size_t scratch_floats, float* gram,
                       hipStream_t s) {
    ProfScope _prof(TK_SMALL, s);
    const GemmPlan p = gemm_plan_expand_gram(d, scratch_floats);
    if (p.var == GEMM_GRAM1) {
        for (int g = 0; g < d.G; ++g)
            if (d.g[g].mc < 1) return TFNAS_EINVAL;
        if (d.mode == TFNAS_MODE_HEAD) hipLaunchKernelGGL(k_gram1<16>, p.grid, dim3(1024), 0, s, d, cb1, gram);
        else hipLaunchKernelGGL(k_gram1<4>, p.grid, dim3(256), 0, s, d, cb1, gram);
        return (int)hipGetLastError();
    }
    const size_t gsz = expand_gram_floats(d);
    if (scratch_floats < gsz) return TFNAS_ERANGE;
    DISPATCH_NT(p.nt, { hipLaunchKernelGGL(k_expand_gram<NT>, p.grid, dim3(256), 0, s, d, cb1, p.rps, p.splits, scratch); })
    _prof.stop();
    return launch_reduce_rows(scratch, p.splits, (int)gsz, gsz, nullptr, gram, s);
}

GemmPlan gemm_plan_expand_dgrad(const TfnasCellDesc& d, bool split, int nsl) {
    GemmPlan p = plan_cols(d.ic);
    p.mm = gemm_arith(d, true);
    const int P = d.N * d.H * d.W, out_tiles = cdiv(P, 128) * p.tiles;
    // K-splits: only when the (row tile x column tile) grid cannot fill the chip
    p.splits = 1;
    if (split && nsl < 0 && out_tiles < 512) {
        const int mchunks = mid_chunks(d);
        int ns = cdiv(1024, out_tiles);
        if (ns > 16) ns = 16;
        if (ns > mchunks / 4) ns = mchunks / 4;      // at least 4 K-chunks per split
        // one-candidate launches of the weight step run beside three other queues: the chip is full anyway, and every extra split is
        // one more [P][ic] partial written, read back and summed (k_dx_reduce).  Capped at 2 (round 6, four alternating bench pairs on
        // one box: w-step 16.55 -> 16.37 ms; a cap of 1 loses: the 196-tile launches of the 14 x 14 cells then walk 40+ K-chunks each)
        // (cells only: the head's weight gradient is a leaf that may run in a call of its own -- tfnas_head_wgrad after
        //  tfnas_head_bwd with need_wgrad = 0, as the weight step does -- and dx must not depend on which form the caller chose)
        if (d.need_wgrad && d.G == 1 && d.mode != TFNAS_MODE_HEAD && ns > TFNAS_WSPLIT_DGRAD) ns = TFNAS_WSPLIT_DGRAD;
        p.splits = ns < 1 ? 1 : ns;
    }
    p.grid = dim3(row_blocks(P, p.tiles * p.splits, 1u << 30, gemm_slots(p.nt, p.mm), 4096), p.tiles, p.splits);
    p.parts = nsl >= 0 ? nsl + 1 : (p.splits > 1 ? p.splits : 0);
    size_t blocks = cdiv64((size_t)P * d.ic / 4, 256 * 2);
    p.grid2 = dim3((unsigned)(blocks > 2048 ? 2048 : blocks));
    return p;
}

// nsl >= 0, the fused per-image route (fx_kernels.hip): dxp[0 .. nsl) hold the partial sums of dE (rstd . W1); this adds the
// BN1-backward correction -x G (one more partial tile, MFMA) and sums everything (+ b, + residual, + sink gradient) into dx
int launch_expand_dgrad(const TfnasCellDesc& d, const float* dEh, const float* x, const float* cb1, const float* gram,
                        const float* dout, const float* wmix, float* dx, float* dxp, hipStream_t s,
                        const float* add_src, const float* add_scale, int nsl) {
    const GemmPlan p = gemm_plan_expand_dgrad(d, dxp != nullptr, nsl);
    {
        ProfScope _prof(TK_EXPAND_DGRAD, s);
        DISPATCH_MM(p.mm, DISPATCH_NT(p.nt, {
            hipLaunchKernelGGL((k_expand_dgrad<NT, MM>), p.grid, dim3(256), 0, s, d, dEh, x, cb1, gram, dout, wmix, dx, dxp, p.splits,
                               add_src, add_scale, nsl);
        }))
    }
    if (p.parts) {
        ProfScope _p2(TK_SMALL, s);
        hipLaunchKernelGGL(k_dx_reduce, p.grid2, dim3(256), 0, s, d, dxp, p.parts, gram, dout, wmix, dx, add_src, add_scale);
    }
    return (int)hipGetLastError();
}

// XG: the double sums of the splits live in the top of `part` (2 floats per element, 16-byte aligned)
static size_t xg_red_floats(const GemmPlan& p) { return p.var == GEMM_XG ? 2 * p.out + 4 : 0; }

GemmPlan gemm_plan_expand_wgrad(const TfnasCellDesc& d) {
    GemmPlan p = plan_cols(d.ic);
    // Expand weight gradient without reading E (Gram form, k_expand_wgrad<XG>) where E is at least 100 MB (measured alone at
    // B = 128, DESIGN.md section 4d: cell 0 0.33 -> 0.24 ms, cells 1 / 2 equal; from 28 x 28 on E comes from the last-level cache and the
    // extension rows + the fix-up launch cost more than the second stream: cell 10 0.08 -> 0.11 ms); TFNAS_ROUTE_XG_OFF: never,
    // TFNAS_ROUTE_XG_ALL: wherever the shape allows (tests); every choice is compared with the oracle (tests/test_gpu_cell.py)
    const int P = d.N * d.H * d.W;
    if (d.mode == TFNAS_MODE_STEM) p.var = GEMM_STEM;
    else if (!(d.route & TFNAS_ROUTE_XG_OFF) && (d.ic & 3) == 0 &&
             ((d.route & TFNAS_ROUTE_XG_ALL) || (size_t)P * d.M * sizeof(float) >= ((size_t)100 << 20)))
        p.var = GEMM_XG;
    const int next = p.var == GEMM_XG ? d.ic + 1 : 0;               // extension rows behind the last group's
    p.out_main = mid_floats(d, d.ic);
    p.out = p.out_main + (size_t)next * d.ic;
    plan_row_splits(p, P, group_tiles(d, 128, next), p.tiles, TFNAS_PART_FLOATS - xg_red_floats(p));
    return p;
}

int launch_expand_wgrad(const TfnasCellDesc& d, const float* dEh, const float* E, const float* cb1,
                        const float* x, float* part, hipStream_t s) {
    ProfScope _prof(TK_EXPAND_WGRAD, s);
    const GemmPlan p = gemm_plan_expand_wgrad(d);
    const size_t red_floats = xg_red_floats(p);
    if (p.var != GEMM_XG && !E) return TFNAS_ENULL;
    if (red_floats + p.out > TFNAS_PART_FLOATS) return TFNAS_ERANGE;
    if (p.var == GEMM_STEM && p.nt != 2) return TFNAS_EINVAL;      // ic = 27 (tfnas_cell_plan): plan_cols gives the stem 2
    DISPATCH_NT(p.nt, {
        auto k = p.var == GEMM_XG ? k_expand_wgrad<NT, false, true> : k_expand_wgrad<NT, false, false>;
        if (p.var == GEMM_STEM) k = k_expand_wgrad<2, true, false>;
        hipLaunchKernelGGL(k, p.grid, dim3(256), 0, s, d, dEh, E, cb1, x, p.rps, part, p.out, p.out_main);
    })
    _prof.stop();
    if (p.var != GEMM_XG) return reduce_group_wgrads(d, p, part, d.ic, &TfnasGroup::g_expand, s);
    double* red = reinterpret_cast<double*>((uintptr_t)(part + TFNAS_PART_FLOATS - red_floats + 3) & ~(uintptr_t)15);
    int rc = launch_reduce_rows(part, p.splits, (int)p.out, p.out, red, nullptr, s);
    if (rc) return rc;
    ProfScope _p2(TK_EXPAND_WGRAD, s);
    hipLaunchKernelGGL(k_expand_wgrad_fix, dim3((unsigned)cdiv64(p.out_main, 64)), dim3(256), 0, s, d, cb1, red, p.out_main);
    return (int)hipGetLastError();
}
