// Depthwise weight gradient, register-window form (no LDS staging, no barriers in the main loop).  Included by
// dwconv_kernels.hip after dw_stream.inc.
//
//   g_dw[c][ky][kx] = sum_{n,ho,wo} dd[n][ho][wo][c] * a1[n][ho*S+ky-p][wo*S+kx-p][c]
//   (a1 = act(BN1(E)), dd = BN2-backward of dZ: bn2_dd; reference arithmetic: autograd of depth_conv, models/layers.py:484-507)
//
// Why: the LDS-tiled / ring kernels read K x (3S + K) operands from LDS per four output pixels and K x K x 4 FMAs -- they
// are bound by LDS bandwidth and by the barriers between their load and compute phases (k_dw_wgrad at 112 x 112: 0.5-0.6 ms
// for 0.46-0.92 GB, five times its HBM time).  Here a WAVE owns (32 channels, 4 column blocks of JW output columns) and walks
// down the input rows of its images; a lane holds two channels of one column block:
//   * the input row of the step lives in registers (WIN = (JW-1)*S + K pixels, loaded once from global memory -- the halo
//     overlap of neighbouring lanes is served by the vector L1 / L2) and is used for EVERY ky it contributes to;
//   * the dd rows those ky need are a rolling register window of R rows (R = K for stride 1, (K+1)/2 for stride 2): one new
//     row per macro-step (= S input rows);
//   * the loads of step e+1 are in flight while the FMAs of step e run; waves are independent (no __syncthreads).
// Images are stacked: the walk is over N * (Ho + A) macro-steps (A warm-up steps per image that only load dd rows; the
// zero rows loaded past the end of an image are exactly the zero rows the next image needs above its first row), split
// evenly over `nseg` waves, each of which starts R-1 macro-steps early with the FMAs disabled.
// Partial sums: one row of part[] per workgroup (its 4 waves are 4 consecutive segments), summed by k_reduce_rows.

// Geometry: DwDirect (kernels.h).

// the input rows are re-read by the neighbouring column blocks (halo) and by the K x K kernel of the next column group:
// ordinary (cached) loads for E, non-temporal ones for the once-through dZ / D rows
#ifndef DWD_E_AUX
#define DWD_E_AUX 0
#endif
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 zero2() { f32x2 z = {0.f, 0.f}; return z; }

// two consecutive channels at ELEMENT offset `off`
template <int AUX>
__device__ __forceinline__ f32x2 dwd_ld2(const BufView& b, unsigned off) {
    const u32x2 u = __builtin_amdgcn_raw_buffer_load_b64(b.r, (int)(off * 4u), 0, AUX);
    f32x2 r = {__uint_as_float(u.x), __uint_as_float(u.y)};
    return r;
}

template <int K, int S, int ACT, int JW>
__global__ __launch_bounds__(256, (K == 3 ? 4 : (JW == 2 ? 3 : 2))) void k_dwd_wgrad(
    TfnasCellDesc d, const float* __restrict__ dZ, const float* __restrict__ gate, const float* __restrict__ dpooled,
    const float* __restrict__ D, const double* __restrict__ stats2, const double* __restrict__ red2,
    const float* __restrict__ E, const double* __restrict__ stats1, float* __restrict__ part, size_t out_size, DwDirect gm) {
    constexpr int P = K / 2, A = (S == 1) ? P : 1, R = (S == 1) ? K : (K + 1) / 2, WIN = (JW - 1) * S + K;
    // 16 lanes x 2 channels = one 128-byte line per pixel, 4 column blocks per wave (32 lanes per pixel -- 64-channel chunks --
    // measured the same or slower)
    constexpr int LPP = 16, CC = 2 * LPP, NB = 64 / LPP;
    __shared__ float wred[4 * K * K * CC];

    // XCD-aware order: the workgroups of one XCD (blockIdx % 8) take a contiguous range of units (neighbouring segments and
    // column groups share halo pixels in the same L2)
    int b = blockIdx.x;
    if ((gm.nwg & 7) == 0) b = (b & 7) * (gm.nwg >> 3) + (b >> 3);
    const int segq = gm.nseg >> 2;
    // chunk index fastest: the 128-byte slices the chunks of one pixel read share cache lines whenever M * 4 is not a multiple
    // of 128 (M = 48, 72, 120, 144 ...) -- they must meet in the same L2, close in time
    const int cy = b % gm.chunks, pos = b / gm.chunks;
    const int sq = pos % segq, cg = pos / segq;
    int g, c0;
    if (!dw_locate<K>(d, cy, CC, g, c0)) return;
    const int mc = d.g[g].mc, off = d.g[g].off;
    size_t poff = 0;
    for (int gg = 0; gg < g; ++gg) poff += (size_t)d.g[gg].mc * d.g[gg].k * d.g[gg].k;

    const int tid = threadIdx.x, l = tid & 63, l16 = l & (LPP - 1), cb = l / LPP;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: the walk's control flow stays scalar
    const int H = d.H, W = d.W, Ho = d.Ho, Wo = d.Wo, M = d.M, N = d.N;
    const int ch = c0 + 2 * l16;                       // first of this lane's two channels (inside the group)
    const bool ch_ok = ch < mc;                        // (mc is even: widths are multiples of 4 or 8)

    // per-channel constants: BN1 (mean, rstd), BN2 (mean, rstd, R1/Po, R2/Po)
    f32x2 m1 = zero2(), r1 = zero2(), m2 = zero2(), r2 = zero2(), q1 = zero2(), q2 = zero2();
    if (ch_ok) {
        const double inv1 = 1.0 / ((double)N * H * W), inv2 = 1.0 / ((double)N * Ho * Wo);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const size_t c = (size_t)(off + ch + j);
            const float2 a = bn_consts(stats1 + 2 * c, inv1, d.eps);
            const float2 bq = bn_consts(stats2 + 2 * c, inv2, d.eps);
            m1[j] = a.x; r1[j] = a.y; m2[j] = bq.x; r2[j] = bq.y;
            q1[j] = (float)(red2[2 * c] * inv2);
            q2[j] = (float)(red2[2 * c + 1] * inv2);
        }
    }
    const bool has_se = d.g[g].se > 0;
    const float inv_hw = 1.f / (float)(Ho * Wo);

    // column geometry of this lane
    const int wo0 = (cg * NB + cb) * JW, wi0 = wo0 * S - P;
    unsigned emask = 0, dmask = 0;                     // valid input columns (bit u) / output columns (bit j)
#pragma unroll
    for (int u = 0; u < WIN; ++u) emask |= (ch_ok && wi0 + u >= 0 && wi0 + u < W) ? (1u << u) : 0u;
#pragma unroll
    for (int j = 0; j < JW; ++j) dmask |= (ch_ok && wo0 + j < Wo) ? (1u << j) : 0u;
    const int e_lane = wi0 * M + off + ch, d_lane = wo0 * M + off + ch;      // (e_lane may be negative: masked columns)
    const unsigned se_lane = (unsigned)(off + ch);

    const size_t numel_e = (size_t)N * H * W * M, numel_d = (size_t)N * Ho * Wo * M;
    BufView bZ, bD, bE;
    bZ.bind(dZ, numel_d);
    bD.bind(D, numel_d);
    bE.bind(E, numel_e);

    // this wave's range of macro-steps
    const int seg = sq * 4 + wv;
    const int s0 = seg * gm.per, s1 = min(gm.steps, s0 + gm.per);
    const int sw = max(0, s0 - (R - 1));
    const int HA = Ho + A;
    int n = sw / HA, t = sw - n * HA - A;              // position of the NEXT event to issue (image, macro-step), sub-row 0
    int sidx = sw;                                     // its macro-step index
    const int nev = s1 > s0 ? (s1 - sw) * S : 0;

    f32x2 wacc[K * K];
#pragma unroll
    for (int u = 0; u < K * K; ++u) wacc[u] = zero2();
    f32x2 win[R][JW];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < JW; ++j) win[i][j] = zero2();
    f32x2 cur[WIN], nx[WIN], ndz[JW], ndv[JW], ng = zero2(), ndp = zero2();
    bool p_row = false, p_dd = false, p_fma = false;   // flags of the pending (issued) event

    // issue the loads of the event at (n, t, sub-row r)
    auto issue = [&](int r) {
        const int hi = t * S + r;
        p_row = t >= 0 && hi < H && n < N;
        p_fma = p_row && sidx >= s0;
        const unsigned ebase = (unsigned)((n * H + hi) * W) * (unsigned)M;
#pragma unroll
        for (int u = 0; u < WIN; ++u) {
            const bool ok = p_fma && ((emask >> u) & 1u);
            nx[u] = dwd_ld2<DWD_E_AUX>(bE, ok ? ebase + (unsigned)(e_lane + u * M) : BUF_OOB);
        }
        if (r == 0) {
            const int ho = t + A;
            p_dd = ho < Ho && n < N;
            const unsigned dbase = (unsigned)((n * Ho + ho) * Wo) * (unsigned)M;
#pragma unroll
            for (int j = 0; j < JW; ++j) {
                const bool ok = p_dd && ((dmask >> j) & 1u);
                const unsigned o = ok ? dbase + (unsigned)(d_lane + j * M) : BUF_OOB;
                ndz[j] = dwd_ld2<TFNAS_LD_AUX>(bZ, o);
                ndv[j] = dwd_ld2<TFNAS_LD_AUX>(bD, o);
            }
            if (has_se && p_dd && ch_ok) {
                const size_t a = (size_t)n * M + se_lane;
                ng = *reinterpret_cast<const f32x2*>(gate + a);
                ndp = *reinterpret_cast<const f32x2*>(dpooled + a) * inv_hw;
            }
        }
    };
    // move to the event after (n, t, r)
    auto advance = [&](int r) {
        if (r == S - 1) {
            ++sidx;
            if (++t == Ho) {
                t = -A;
                ++n;
            }
        }
    };

    if (nev > 0) issue(0);
    for (int ev = 0; ev < nev;) {
#pragma unroll
        for (int ph = 0; ph < R; ++ph) {
#pragma unroll
            for (int r = 0; r < S; ++r) {
                if (ev < nev) {
                    // ---- the pending loads become the current operands
                    if (r == 0) {
#pragma unroll
                        for (int j = 0; j < JW; ++j) {
                            f32x2 dz = ndz[j];
                            if (has_se) dz = dz * ng + ndp;
                            f32x2 v;
#pragma unroll
                            for (int q = 0; q < 2; ++q) {
                                const float dh = (ndv[j][q] - m2[q]) * r2[q];
                                const float ddh = dz[q] * act_d<ACT>(dh);
                                v[q] = r2[q] * (ddh - q1[q] - dh * q2[q]);
                            }
                            win[ph][j] = (p_dd && ((dmask >> j) & 1u)) ? v : zero2();
                        }
                    }
                    const bool fma = p_fma;
                    if (fma) {
#pragma unroll
                        for (int u = 0; u < WIN; ++u) {
                            f32x2 v;
#pragma unroll
                            for (int q = 0; q < 2; ++q) v[q] = act_f<ACT>((nx[u][q] - m1[q]) * r1[q]);
                            cur[u] = ((emask >> u) & 1u) ? v : zero2();
                        }
                    }
                    // ---- next event's loads
                    advance(r);
                    ++ev;
                    if (ev < nev) issue(r == S - 1 ? 0 : r + 1);
                    // ---- FMAs of the current event: every ky this input row contributes to
                    if (fma) {
#pragma unroll
                        for (int ky = 0; ky < K; ++ky) {
                            if ((r + P + ky) % S != 0) continue;
                            const int i = (S == 1) ? ky : (2 - r - P + ky) / 2;      // rows behind the newest dd row
                            const int slot = (ph - i + 2 * R) % R;
#pragma unroll
                            for (int kx = 0; kx < K; ++kx)
#pragma unroll
                                for (int j = 0; j < JW; ++j) wacc[ky * K + kx] += win[slot][j] * cur[j * S + kx];
                        }
                    }
                }
            }
        }
    }

    // sum the column blocks of the wave, then the 4 waves of the workgroup
#pragma unroll
    for (int u = 0; u < K * K; ++u) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float v = wacc[u][q];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            wacc[u][q] = v;
        }
    }
    if (cb == 0) {
#pragma unroll
        for (int u = 0; u < K * K; ++u) {
            wred[(wv * K * K + u) * CC + 2 * l16] = wacc[u][0];
            wred[(wv * K * K + u) * CC + 2 * l16 + 1] = wacc[u][1];
        }
    }
    __syncthreads();
    float* __restrict__ gw = part + (size_t)(cg * segq + sq) * out_size + poff;
    for (int idx = tid; idx < K * K * CC; idx += 256) {
        const int cl = idx % CC, u = idx / CC;
        if (c0 + cl < mc) {
            float s = 0.f;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) s += wred[(ww * K * K + u) * CC + cl];
            gw[(size_t)(c0 + cl) * (K * K) + u] = s;
        }
    }
}


// two consecutive channels to ELEMENT offset `off`
__device__ __forceinline__ void dwd_st2(const BufView& b, unsigned off, f32x2 v) {
    u32x2 u = {__float_as_uint(v.x), __float_as_uint(v.y)};
    __builtin_amdgcn_raw_buffer_store_b64(u, b.r, (int)(off * 4u), 0, TFNAS_ST_AUX);
}

// ---------------------------------------------------------------------------------------------------- forward
// D[n][ho][wo][c] = sum_{ky,kx} w[c][ky][kx] * a1[n][ho*S+ky-p][wo*S+kx-p][c]   (+ the (sum, sumsq) rows of BN2)
// Same walk as the weight gradient: the input row of the event is in registers and is accumulated into EVERY output row it
// contributes to -- a rolling window of R output-row accumulators (JW columns each); a row is stored (and added to the
// statistics) after its last input row.  A wave owns the output rows that COMPLETE in its range of macro-steps and starts
// R-1 macro-steps early (inside the same image) with stores disabled.
template <int K, int S, int ACT, int JW>
__global__ __launch_bounds__(256, (K == 3 ? 4 : (JW == 2 ? 4 : 3))) void k_dwd_fwd(
    TfnasCellDesc d, const float* __restrict__ E, const double* __restrict__ stats1, float* __restrict__ D,
    float* __restrict__ part, DwDirect gm) {
    constexpr int P = K / 2, R = (S == 1) ? K : (K + 1) / 2, WIN = (JW - 1) * S + K;
    constexpr int XT = (S == 1) ? P : 1;      // flush macro-steps per image: the rows still open complete, and the window slots the
                                              // next image's first rows take over are zero again
    constexpr int RC = (S == 1) ? 0 : (K == 3 ? 1 : 0);      // sub-row after which the oldest row of the window completes
    constexpr int LPP = 16, NB = 4, CC = 32;
    __shared__ float sred[4 * 2 * CC];

    int b = blockIdx.x;
    if ((gm.nwg & 7) == 0) b = (b & 7) * (gm.nwg >> 3) + (b >> 3);
    const int segq = gm.nseg >> 2;
    const int cy = b % gm.chunks, pos = b / gm.chunks;
    const int sq = pos % segq, cg = pos / segq;
    int g, c0;
    if (!dw_locate<K>(d, cy, CC, g, c0)) return;
    const int mc = d.g[g].mc, mcp = d.g[g].mcp, off = d.g[g].off;

    const int tid = threadIdx.x, l = tid & 63, l16 = l & (LPP - 1), cb = l / LPP;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = d.H, W = d.W, Ho = d.Ho, Wo = d.Wo, M = d.M, N = d.N;
    const int ch = c0 + 2 * l16;
    const bool ch_ok = ch < mcp;                       // pad channels (mc <= c < mcp) are written as zeros

    f32x2 m1 = zero2(), r1 = zero2();
    f32x2 wk[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) wk[t] = zero2();
    {
        const double inv1 = 1.0 / ((double)N * H * W);
        const float* __restrict__ wdw = d.g[g].w_dw;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (ch + j < mc) {
                const float2 a = bn_consts(stats1 + 2 * (size_t)(off + ch + j), inv1, d.eps);
                m1[j] = a.x;
                r1[j] = a.y;
#pragma unroll
                for (int t = 0; t < K * K; ++t) wk[t][j] = wdw[(size_t)(ch + j) * (K * K) + t];
            }
        }
    }

    const int wo0 = (cg * NB + cb) * JW, wi0 = wo0 * S - P;
    unsigned emask = 0, omask = 0;
#pragma unroll
    for (int u = 0; u < WIN; ++u) emask |= (ch_ok && wi0 + u >= 0 && wi0 + u < W) ? (1u << u) : 0u;
#pragma unroll
    for (int j = 0; j < JW; ++j) omask |= (ch_ok && wo0 + j < Wo) ? (1u << j) : 0u;
    const int e_lane = wi0 * M + off + ch, d_lane = wo0 * M + off + ch;

    BufView bE, bD;
    bE.bind(E, (size_t)N * H * W * M);
    bD.bind(D, (size_t)N * Ho * Wo * M);

    const int HA = (S == 1 ? H : Ho) + XT;             // macro-steps per image
    const int seg = sq * 4 + wv;
    const int s0 = seg * gm.per, s1 = min(gm.steps, s0 + gm.per);
    const int sw = max(max(0, s0 - (R - 1)), (s0 / HA) * HA);
    int n = sw / HA, t = sw - n * HA;                  // position of the NEXT event to issue
    int sidx = sw;
    const int nev = s1 > s0 ? (s1 - sw) * S : 0;

    f32x2 acc[R][JW];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < JW; ++j) acc[i][j] = zero2();
    f32x2 cur[WIN], nx[WIN], ssum = zero2(), ssq = zero2();
    bool p_row = false;
    // position of the CURRENT event (the one whose loads are pending)
    int c_n = 0, c_t = 0, c_s = 0;

    auto issue = [&](int r) {
        const int hi = t * S + r;
        p_row = hi < H && n < N;
        c_n = n; c_t = t; c_s = sidx;
        const unsigned ebase = (unsigned)((n * H + hi) * W) * (unsigned)M;
#pragma unroll
        for (int u = 0; u < WIN; ++u) {
            const bool ok = p_row && ((emask >> u) & 1u);
            nx[u] = dwd_ld2<DWD_E_AUX>(bE, ok ? ebase + (unsigned)(e_lane + u * M) : BUF_OOB);
        }
    };
    auto advance = [&](int r) {
        if (r == S - 1) {
            ++sidx;
            if (++t == HA) {
                t = 0;
                ++n;
            }
        }
    };

    if (nev > 0) issue(0);
    for (int ev = 0; ev < nev;) {
#pragma unroll
        for (int ph = 0; ph < R; ++ph) {
#pragma unroll
            for (int r = 0; r < S; ++r) {
                if (ev < nev) {
                    const bool row = p_row;
                    const int e_n = c_n, e_t = c_t, e_s = c_s;
                    if (r == 0) {                                  // the slot of the row that becomes the newest
#pragma unroll
                        for (int j = 0; j < JW; ++j) acc[ph][j] = zero2();
                    }
                    if (row) {
#pragma unroll
                        for (int u = 0; u < WIN; ++u) {
                            f32x2 v;
#pragma unroll
                            for (int q = 0; q < 2; ++q) v[q] = act_f<ACT>((nx[u][q] - m1[q]) * r1[q]);
                            cur[u] = ((emask >> u) & 1u) ? v : zero2();
                        }
                    }
                    advance(r);
                    ++ev;
                    if (ev < nev) issue(r == S - 1 ? 0 : r + 1);
                    if (row) {
#pragma unroll
                        for (int ky = 0; ky < K; ++ky) {
                            if ((r + P + ky) % S != 0) continue;
                            const int i = (S == 1) ? ky : (2 - r - P + ky) / 2;      // rows behind the newest output row
                            const int slot = (ph - i + 2 * R) % R;
#pragma unroll
                            for (int kx = 0; kx < K; ++kx)
#pragma unroll
                                for (int j = 0; j < JW; ++j) acc[slot][j] += wk[ky * K + kx] * cur[j * S + kx];
                        }
                    }
                    if (r == RC) {                                 // the oldest row of the window is complete
                        const int hoc = (S == 1 ? e_t + P : e_t + 1) - (R - 1);
                        if (e_s >= s0 && hoc >= 0 && hoc < Ho) {
                            const int slot = (ph + 1) % R;
                            const unsigned dbase = (unsigned)((e_n * Ho + hoc) * Wo) * (unsigned)M;
#pragma unroll
                            for (int j = 0; j < JW; ++j) {
                                const bool ok = (omask >> j) & 1u;
                                const f32x2 v = acc[slot][j];
                                dwd_st2(bD, ok ? dbase + (unsigned)(d_lane + j * M) : BUF_OOB, v);
                                if (ok) {
                                    ssum += v;
                                    ssq += v * v;
                                }
                            }
                        }
                    }
                }
            }
        }
    }

    // (sum, sumsq) of this workgroup's outputs: column blocks of the wave, then the 4 waves
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        float a = ssum[q], c = ssq[q];
        a += __shfl_xor(a, 16, 64);
        a += __shfl_xor(a, 32, 64);
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        ssum[q] = a;
        ssq[q] = c;
    }
    if (cb == 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            sred[(wv * 2 + 0) * CC + 2 * l16 + q] = ssum[q];
            sred[(wv * 2 + 1) * CC + 2 * l16 + q] = ssq[q];
        }
    }
    __syncthreads();
    if (tid < 2 * CC) {
        const int cl = tid >> 1, which = tid & 1;
        if (c0 + cl < mcp) {
            float a = 0.f;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) a += sred[(ww * 2 + which) * CC + cl];
            part[(size_t)(cg * segq + sq) * 2 * M + 2 * (size_t)(off + c0 + cl) + which] = a;
        }
    }
}


// ---------------------------------------------------------------------------------------------------- backward w.r.t. input
// dA1[n][hi][wi][c] = sum_{ky,kx} dd[n][(hi+p-ky)/S][(wi+p-kx)/S][c] * w[c][ky][kx]   (exact divisions only)
// dEh = dA1 * act'(ehat), partial rows of T1 = sum dEh, T2 = sum dEh * ehat (BN1 backward).
// An event is one dd row (formed once from dZ / D, with its column halo): it is accumulated into the K input rows it
// reaches -- a rolling window of K accumulator rows of JW*S input columns; after the event the S oldest rows are complete:
// their E rows (requested together with the dd row) give ehat, the row is scaled by act'(ehat), stored and added to the sums.
// waves per SIMD the backward kernel's registers allow (accumulator window K x JW*S, K*K taps, dd row + its raw loads)
__host__ __device__ constexpr int dwd_bwd_occ(int K, int S, int JW) {
    return K == 3 ? (S == 1 ? (JW == 2 ? 4 : 3) : (JW == 2 ? 3 : 2)) : (S == 1 ? (JW == 2 ? 3 : 2) : 2);
}
// WG (the w-step of the stride-2 cells): the depthwise weight gradient from the same pass.  When an input row completes, its
// a1 = act(ehat) meets the dd rows that reach it -- the current event's and the RW - 1 before it, kept in registers -- in exactly
// the (dd column, tap) pairs of the data-gradient FMAs:  g_dw[ky][kx] += dd[t'][wo] * a1[hi][wi],  ky = hi + P - t' S.
// Partial rows wpart[(cg * segq + sq)][poff_g + c * K * K + tap], summed by k_reduce_rows; the separate k_dwd_wgrad launch and its
// second read of E, dZ and D disappear (cell 0 at B = 128: 0.9 GB per sampled candidate).
template <int K, int S, int ACT, int JW, bool WG = false>
__global__ __launch_bounds__(256, dwd_bwd_occ(K, S, JW)) void k_dwd_bwd(
    TfnasCellDesc d, const float* __restrict__ dZ, const float* __restrict__ gate, const float* __restrict__ dpooled,
    const float* __restrict__ D, const double* __restrict__ stats2, const double* __restrict__ red2,
    const float* __restrict__ E, const double* __restrict__ stats1, float* __restrict__ dEh, float* __restrict__ part,
    DwDirect gm, float* __restrict__ wpart = nullptr, size_t wout_size = 0) {
    constexpr int P = K / 2, JI = JW * S, RW = (S == 1) ? K : (K + 1) / 2;      // RW: events a row collects from
    constexpr int WD = (S == 1) ? JW + K - 1 : JW + (K == 3 ? 1 : 2);          // dd columns of an event (with halo)
    constexpr int WD0 = (S == 1) ? -P : (K == 3 ? 0 : -1);                      // first dd column relative to wo0
    constexpr int XT = (S == 1) ? P : 1;
    constexpr int LPP = 16, NB = 4, CC = 32;
    __shared__ float sred[4 * 2 * CC];
    __shared__ float wredw[WG ? 4 * K * K * CC : 1];

    int b = blockIdx.x;
    if ((gm.nwg & 7) == 0) b = (b & 7) * (gm.nwg >> 3) + (b >> 3);
    const int segq = gm.nseg >> 2;
    const int cy = b % gm.chunks, pos = b / gm.chunks;
    const int sq = pos % segq, cg = pos / segq;
    int g, c0;
    if (!dw_locate<K>(d, cy, CC, g, c0)) return;
    const int mc = d.g[g].mc, mcp = d.g[g].mcp, off = d.g[g].off;

    const int tid = threadIdx.x, l = tid & 63, l16 = l & (LPP - 1), cb = l / LPP;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = d.H, W = d.W, Ho = d.Ho, Wo = d.Wo, M = d.M, N = d.N;
    const int ch = c0 + 2 * l16;
    const bool ch_ok = ch < mcp;

    f32x2 m1 = zero2(), r1 = zero2(), m2 = zero2(), r2 = zero2(), q1 = zero2(), q2 = zero2();
    f32x2 wacc[WG ? K * K : 1], ddp[WG ? RW : 1][WD];       // tap sums; dd rows by age (0 = the current event's)
#pragma unroll
    for (int t = 0; t < (WG ? K * K : 1); ++t) wacc[t] = zero2();
#pragma unroll
    for (int a = 0; a < (WG ? RW : 1); ++a)
#pragma unroll
        for (int u = 0; u < WD; ++u) ddp[a][u] = zero2();
    f32x2 wk[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) wk[t] = zero2();
    {
        const double inv1 = 1.0 / ((double)N * H * W), inv2 = 1.0 / ((double)N * Ho * Wo);
        const float* __restrict__ wdw = d.g[g].w_dw;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (ch + j < mc) {
                const size_t c = (size_t)(off + ch + j);
                const float2 a = bn_consts(stats1 + 2 * c, inv1, d.eps);
                const float2 bq = bn_consts(stats2 + 2 * c, inv2, d.eps);
                m1[j] = a.x; r1[j] = a.y; m2[j] = bq.x; r2[j] = bq.y;
                q1[j] = (float)(red2[2 * c] * inv2);
                q2[j] = (float)(red2[2 * c + 1] * inv2);
#pragma unroll
                for (int t = 0; t < K * K; ++t) wk[t][j] = wdw[(size_t)(ch + j) * (K * K) + t];
            }
        }
    }
    const bool has_se = d.g[g].se > 0;
    const float inv_hw = 1.f / (float)(Ho * Wo);

    const int wo0 = (cg * NB + cb) * JW, wi0 = wo0 * S, wd0 = wo0 + WD0;
    unsigned dmask = 0, imask = 0;                      // valid dd columns (bit u) / input columns (bit c)
#pragma unroll
    for (int u = 0; u < WD; ++u) dmask |= (ch < mc && wd0 + u >= 0 && wd0 + u < Wo) ? (1u << u) : 0u;
#pragma unroll
    for (int c = 0; c < JI; ++c) imask |= (ch_ok && wi0 + c < W) ? (1u << c) : 0u;
    const int d_lane = wd0 * M + off + ch, e_lane = wi0 * M + off + ch;
    const unsigned se_lane = (unsigned)(off + ch);

    const size_t numel_e = (size_t)N * H * W * M, numel_d = (size_t)N * Ho * Wo * M;
    BufView bZ, bD, bE, bO;
    bZ.bind(dZ, numel_d);
    bD.bind(D, numel_d);
    bE.bind(E, numel_e);
    bO.bind(dEh, numel_e);

    const int HA = Ho + XT;                            // events per image: its dd rows + XT zero rows
    const int seg = sq * 4 + wv;
    const int s0 = seg * gm.per, s1 = min(gm.steps, s0 + gm.per);
    const int sw = max(max(0, s0 - (RW - 1)), (s0 / HA) * HA);
    int n = sw / HA, t = sw - n * HA;                  // position of the NEXT event to issue (image, dd row)
    int sidx = sw;
    const int nev = s1 > s0 ? s1 - sw : 0;

    f32x2 acc[K][JI];
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int c = 0; c < JI; ++c) acc[i][c] = zero2();
    f32x2 ndz[WD], ndv[WD], ne[S][JI], ng = zero2(), ndp = zero2(), ddr[WD];
    f32x2 t1 = zero2(), t2 = zero2();
    bool p_dd = false, p_own = false;
    int c_n = 0, c_t = 0;

    auto issue = [&]() {
        p_dd = t < Ho && n < N;
        p_own = sidx >= s0;
        c_n = n; c_t = t;
        const unsigned dbase = (unsigned)((n * Ho + t) * Wo) * (unsigned)M;
#pragma unroll
        for (int u = 0; u < WD; ++u) {
            const bool ok = p_dd && ((dmask >> u) & 1u);
            const unsigned o = ok ? dbase + (unsigned)(d_lane + u * M) : BUF_OOB;
            ndz[u] = dwd_ld2<TFNAS_LD_AUX>(bZ, o);
            ndv[u] = dwd_ld2<TFNAS_LD_AUX>(bD, o);
        }
        if (has_se && p_dd && ch < mc) {
            const size_t a = (size_t)n * M + se_lane;
            ng = *reinterpret_cast<const f32x2*>(gate + a);
            ndp = *reinterpret_cast<const f32x2*>(dpooled + a) * inv_hw;
        }
        // the E rows of the input rows that complete after this event
#pragma unroll
        for (int r = 0; r < S; ++r) {
            const int hi = t * S - P + r;
            const bool rok = p_own && hi >= 0 && hi < H && n < N;
            const unsigned ebase = (unsigned)((n * H + hi) * W) * (unsigned)M;
#pragma unroll
            for (int c = 0; c < JI; ++c) {
                const bool ok = rok && ((imask >> c) & 1u);
                ne[r][c] = dwd_ld2<TFNAS_LD_AUX>(bE, ok ? ebase + (unsigned)(e_lane + c * M) : BUF_OOB);
            }
        }
    };
    auto advance = [&]() {
        ++sidx;
        if (++t == HA) {
            t = 0;
            ++n;
        }
    };

    if (nev > 0) issue();
    for (int ev = 0; ev < nev;) {
#pragma unroll
        for (int ph = 0; ph < K; ++ph) {
            if (ev < nev) {
                const bool ddok = p_dd, own = p_own;
                const int e_n = c_n, e_t = c_t;
                // rows that enter the window with this event
#pragma unroll
                for (int ky = K - S; ky < K; ++ky)
#pragma unroll
                    for (int c = 0; c < JI; ++c) acc[(S * ph + ky) % K][c] = zero2();
                if (ddok) {
#pragma unroll
                    for (int u = 0; u < WD; ++u) {
                        f32x2 dz = ndz[u];
                        if (has_se) dz = dz * ng + ndp;
                        f32x2 v;
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const float dh = (ndv[u][q] - m2[q]) * r2[q];
                            const float ddh = dz[q] * act_d<ACT>(dh);
                            v[q] = r2[q] * (ddh - q1[q] - dh * q2[q]);
                        }
                        ddr[u] = ((dmask >> u) & 1u) ? v : zero2();
                    }
                }
                if (WG) {
#pragma unroll
                    for (int a = RW - 1; a > 0; --a)
#pragma unroll
                        for (int u = 0; u < WD; ++u) ddp[a][u] = ddp[a - 1][u];
#pragma unroll
                    for (int u = 0; u < WD; ++u) ddp[0][u] = ddok ? ddr[u] : zero2();      // (zero rows between the images)
                }
                // E rows of the completing input rows -> ehat (kept in place)
                f32x2 eh[S][JI];
#pragma unroll
                for (int r = 0; r < S; ++r)
#pragma unroll
                    for (int c = 0; c < JI; ++c) eh[r][c] = (ne[r][c] - m1) * r1;
                advance();
                ++ev;
                if (ev < nev) issue();
                if (ddok) {
#pragma unroll
                    for (int ky = 0; ky < K; ++ky) {
                        const int slot = (S * ph + ky) % K;
#pragma unroll
                        for (int c = 0; c < JI; ++c) {
#pragma unroll
                            for (int kx = 0; kx < K; ++kx) {
                                if ((c + P - kx + 2 * S) % S != 0) continue;
                                const int u = (c + P - kx + 2 * S) / S - 2 - WD0;        // dd column inside the event's row
                                if (u < 0 || u >= WD) continue;
                                acc[slot][c] += ddr[u] * wk[ky * K + kx];
                            }
                        }
                    }
                }
                // the S oldest rows of the window are complete
                if (own) {
#pragma unroll
                    for (int r = 0; r < S; ++r) {
                        const int hi = e_t * S - P + r;
                        if (hi >= 0 && hi < H) {
                            const int slot = (S * ph + r) % K;
                            const unsigned obase = (unsigned)((e_n * H + hi) * W) * (unsigned)M;
#pragma unroll
                            for (int c = 0; c < JI; ++c) {
                                const bool ok = (imask >> c) & 1u;
                                f32x2 v;
#pragma unroll
                                for (int q = 0; q < 2; ++q) v[q] = acc[slot][c][q] * act_d<ACT>(eh[r][c][q]);
                                dwd_st2(bO, ok ? obase + (unsigned)(e_lane + c * M) : BUF_OOB, v);
                                if (ok) {
                                    t1 += v;
                                    t2 += v * eh[r][c];
                                }
                                if (WG) {
                                    f32x2 a1;
#pragma unroll
                                    for (int q = 0; q < 2; ++q) a1[q] = ok ? act_f<ACT>(eh[r][c][q]) : 0.f;
#pragma unroll
                                    for (int a = 0; a < RW; ++a) {
                                        const int ky = r + a * S;               // the tap row through which dd row e_t - a reaches row hi
                                        if (ky >= K) continue;
#pragma unroll
                                        for (int kx = 0; kx < K; ++kx) {
                                            if ((c + P - kx + 2 * S) % S != 0) continue;
                                            const int u = (c + P - kx + 2 * S) / S - 2 - WD0;
                                            if (u < 0 || u >= WD) continue;
                                            wacc[ky * K + kx] += ddp[a][u] * a1;
                                        }
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }

#pragma unroll
    for (int q = 0; q < 2; ++q) {
        float a = t1[q], c = t2[q];
        a += __shfl_xor(a, 16, 64);
        a += __shfl_xor(a, 32, 64);
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        t1[q] = a;
        t2[q] = c;
    }
    if (cb == 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            sred[(wv * 2 + 0) * CC + 2 * l16 + q] = t1[q];
            sred[(wv * 2 + 1) * CC + 2 * l16 + q] = t2[q];
        }
    }
    __syncthreads();
    if (tid < 2 * CC) {
        const int cl = tid >> 1, which = tid & 1;
        if (c0 + cl < mcp) {
            float a = 0.f;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) a += sred[(ww * 2 + which) * CC + cl];
            part[(size_t)(cg * segq + sq) * 2 * M + 2 * (size_t)(off + c0 + cl) + which] = a;
        }
    }
    if (WG) {
        // tap sums: over the 4 column blocks of the wave (lanes 16 apart), then over the 4 waves through LDS in wave order
#pragma unroll
        for (int t = 0; t < K * K; ++t)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float a = wacc[t][q];
                a += __shfl_xor(a, 16, 64);
                a += __shfl_xor(a, 32, 64);
                wacc[t][q] = a;
            }
        if (cb == 0) {
#pragma unroll
            for (int t = 0; t < K * K; ++t)
#pragma unroll
                for (int q = 0; q < 2; ++q) wredw[(wv * K * K + t) * CC + 2 * l16 + q] = wacc[t][q];
        }
        __syncthreads();
        size_t poff = 0;
        for (int gg = 0; gg < g; ++gg) poff += (size_t)d.g[gg].mc * d.g[gg].k * d.g[gg].k;
        float* __restrict__ gw = wpart + (size_t)(cg * segq + sq) * wout_size + poff;
        for (int idx = tid; idx < K * K * CC; idx += 256) {
            const int cl = idx % CC, t = idx / CC;
            if (c0 + cl < mc) {
                float a = 0.f;
#pragma unroll
                for (int ww = 0; ww < 4; ++ww) a += wredw[(ww * K * K + t) * CC + cl];
                gw[(size_t)(c0 + cl) * (K * K) + t] = a;
            }
        }
    }
}
