// Classifier + cross-entropy tail of a search step (reference: `x = self.classifier(x)` models/model_search.py:301-303, a
// LinearLayer(1280, num_classes) with bias, and `criterion = nn.CrossEntropyLoss()` train_search.py:107 as called at :333,376-379,410
// and differentiated by loss.backward()).
//
// Rounds 1-5 left this to stock torch ops: per sampled path a GEMM, log-softmax, nll, their three backward kernels, two more GEMMs and
// a bias reduction -- ten launches of 3-9 us on the w-step's critical chain, twice (bi-sampling), between the end of the cells' forward
// and the start of their backward, when nothing else is on the chip.  Here: ONE launch per path for everything that depends on one
// image (logits, loss, d logits, d pooled) and ONE launch for what sums over images and paths (dW, db, the loss scalar).
// Deterministic: fixed summation orders, no atomics.
//
// Both launches have their optional parts compiled out of the weight step's kernels (k_cls_ce, k_cls_wgrad) and in their other
// forms: k_cls_ce_ex -- label smoothing, the target's rank (top-1 / top-5 without a topk), NaN / rank -1 on an out-of-range label, a
// forward-only form (the retrain path, reference: train_eval.py:228-293 with CrossEntropyLabelSmooth, :72-85,126; the metered search
// steps); k_cls_wgrad_ex -- an epoch's running sums on the device; k_cls_reduce -- those, one path, a device-resident upstream
// gradient and accumulation.  What the forms share is written once: cls_ce_body, cls_dw_tile, cls_db_row, cls_sum_row.
#include "tfnas_dev.h"
#include "kernels.h"
#include "prof.h"

// One workgroup of 16 waves per image (the launch sits on the step's critical chain with nothing beside it: latency rounds, not
// occupancy, are what counts -- a first 4-wave version took 45 us, five dependent load rounds per class batch).  pooled[n] is staged
// in LDS; wave w takes classes w, w + 16, ... in batches of CB with every W load of a batch in flight before the first FMA, lanes
// stride the C features in float4 pieces; softmax / loss in one wave; then d pooled = d logits . W with the K classes split over
// KG thread groups (a thread owns four feature columns x one class range, partial sums combined through LDS in group order).
//
// EX (the retrain tail): smoothing factor eps, loss_n = lse - (1 - eps) l_t - (eps / K) sum_k l_k and d logits = scale (softmax -
// (1 - eps) [k == t] - eps / K), both written as the hard-target value plus an eps term that is skipped when eps == 0 (bit-identical
// to the plain form then); rank[n] = #{k: l_k > l_t} + #{k < t: l_k == l_t} (ties go to the lower class index, so exactly one class
// has rank 0) from the same single-wave pass as the sum of exp, sum_k l_k from the pass that takes the max; a target outside [0, K)
// gives loss_n = NaN, rank = -1 and zero gradient rows, and nothing is ever indexed by it; d pooled == NULL (then d logits is too):
// forward only, the kernel ends after the softmax wave and the launch asks for no [KG][C] LDS.
constexpr int CLS_CB = 4, CLS_T = 1024;
template <bool EX>
__device__ __forceinline__ void cls_ce_body(float* sm, int C, int K, int KG, const float* __restrict__ pooled,
                                            const float* __restrict__ W, const float* __restrict__ bias,
                                            const int64_t* __restrict__ target, float scale, float eps, float* __restrict__ logits,
                                            float* __restrict__ loss_n, int32_t* __restrict__ rank, float* __restrict__ dlogits,
                                            float* __restrict__ dpooled) {
    float* xs = sm;                          // [C]
    float* lg = sm + C;                      // [K rounded up to 4] logits, then d logits
    float* pp = lg + ((K + 3) & ~3);         // [KG][C] partial d pooled
    const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    constexpr int NW = CLS_T / 64;
    const float* xp = pooled + (size_t)n * C;
    for (int c = 4 * tid; c < C; c += 4 * CLS_T) st4(xs + c, ld4(xp + c));
    __syncthreads();
    for (int k0 = wave; k0 < K; k0 += NW * CLS_CB) {
        float acc[CLS_CB];
#pragma unroll
        for (int u = 0; u < CLS_CB; ++u) acc[u] = 0.f;
        for (int c0 = 0; c0 < C; c0 += 1024) {
            // four float4 pieces per lane and class (1024 features per round: C = 1280 is two rounds, the second mostly masked)
            f32x4 wv[CLS_CB][4];
#pragma unroll
            for (int u = 0; u < CLS_CB; ++u) {
                const float* wr = W + (size_t)min(k0 + NW * u, K - 1) * C;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = c0 + 256 * q + 4 * lane;
                    wv[u][q] = ld4(wr + (c < C ? c : 0));
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + 256 * q + 4 * lane;
                const f32x4 xv = c < C ? ld4(xs + c) : zero4();
#pragma unroll
                for (int u = 0; u < CLS_CB; ++u)
                    acc[u] = fmaf(xv.x, wv[u][q].x, fmaf(xv.y, wv[u][q].y, fmaf(xv.z, wv[u][q].z, fmaf(xv.w, wv[u][q].w, acc[u]))));
            }
        }
#pragma unroll
        for (int u = 0; u < CLS_CB; ++u) {
            const float v = wave_sum(acc[u]);
            const int k = k0 + NW * u;
            if (lane == 0 && k < K) lg[k] = v + (bias ? bias[k] : 0.f);
        }
    }
    __syncthreads();
    if (wave == 0) {
        // log-softmax over K classes in one wave: max, sum of exp, in a fixed (lane-strided, then butterfly) order
        float m = -INFINITY, sl = 0.f;
        for (int k = lane; k < K; k += 64) {
            m = fmaxf(m, lg[k]);
            if constexpr (EX) sl += lg[k];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        const int64_t tl = target[n];
        int t = (int)tl;
        bool tok = t >= 0 && t < K;                          // (ignore_index-style targets contribute nothing; the reference has none)
        float lt = 0.f;
        int rk = 0;
        if constexpr (EX) {
            sl = wave_sum(sl);
            tok = tl >= 0 && tl < (int64_t)K;                // (on all 64 bits: 2^32 + 3 is not class 3)
            t = tok ? (int)tl : -1;
            if (tok) lt = lg[t];
        }
        float s = 0.f;
        for (int k = lane; k < K; k += 64) {
            s += expf(lg[k] - m);
            if constexpr (EX) rk += (lg[k] > lt || (lg[k] == lt && k < t)) ? 1 : 0;
        }
        s = wave_sum(s);
        const float lse = m + logf(s);
        if constexpr (EX) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) rk += __shfl_xor(rk, o, 64);
            if (lane == 0) {
                float v = lse - lt;
                if (eps != 0.f) v += eps * (lt - sl * (1.f / (float)K));
                loss_n[n] = tok ? v : NAN;
                rank[n] = tok ? rk : -1;
            }
        } else {
            if (lane == 0) loss_n[n] = tok ? lse - lg[t] : 0.f;
        }
        const float inv = 1.f / s;
        const bool bwd = !EX || dpooled != nullptr;
        const float epsk = eps / (float)K;
        for (int k = lane; k < K; k += 64) {
            const float l = lg[k];
            logits[(size_t)n * K + k] = l;
            if (bwd) {
                float d = expf(l - m) * inv - (k == t ? 1.f : 0.f);
                if constexpr (EX) {
                    if (eps != 0.f) d += (k == t ? eps : 0.f) - epsk;
                }
                const float g = tok ? scale * d : 0.f;
                dlogits[(size_t)n * K + k] = g;
                lg[k] = g;
            }
        }
    }
    if constexpr (EX) {
        if (!dpooled) return;                                // (a kernel argument: the whole workgroup leaves together)
    }
    __syncthreads();
    const int nq = C >> 2, kper = (K + KG - 1) / KG;
    for (int it = tid; it < nq * KG; it += CLS_T) {
        const int cq = it % nq, kg = it / nq;
        const int kb = kg * kper, ke = min(K, kb + kper);
        f32x4 a = zero4();
        int k = kb;
        for (; k + 8 <= ke; k += 8) {
            f32x4 wv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) wv[u] = ld4(W + (size_t)(k + u) * C + 4 * cq);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float g = lg[k + u];
                a.x = fmaf(g, wv[u].x, a.x); a.y = fmaf(g, wv[u].y, a.y); a.z = fmaf(g, wv[u].z, a.z); a.w = fmaf(g, wv[u].w, a.w);
            }
        }
        for (; k < ke; ++k) {
            const f32x4 wv = ld4(W + (size_t)k * C + 4 * cq);
            const float g = lg[k];
            a.x = fmaf(g, wv.x, a.x); a.y = fmaf(g, wv.y, a.y); a.z = fmaf(g, wv.z, a.z); a.w = fmaf(g, wv.w, a.w);
        }
        st4(pp + (size_t)kg * C + 4 * cq, a);
    }
    __syncthreads();
    for (int cq = tid; cq < nq; cq += CLS_T) {
        f32x4 a = ld4(pp + 4 * cq);
        for (int kg = 1; kg < KG; ++kg) {
            const f32x4 b = ld4(pp + (size_t)kg * C + 4 * cq);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        st4(dpooled + (size_t)n * C + 4 * cq, a);
    }
}

__global__ __launch_bounds__(CLS_T) void k_cls_ce(int C, int K, int KG, const float* __restrict__ pooled, const float* __restrict__ W,
                                                  const float* __restrict__ bias, const int64_t* __restrict__ target, float scale,
                                                  float* __restrict__ logits, float* __restrict__ loss_n,
                                                  float* __restrict__ dlogits, float* __restrict__ dpooled) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    cls_ce_body<false>(sm, C, K, KG, pooled, W, bias, target, scale, 0.f, logits, loss_n, nullptr, dlogits, dpooled);
}

__global__ __launch_bounds__(CLS_T) void k_cls_ce_ex(int C, int K, int KG, const float* __restrict__ pooled,
                                                     const float* __restrict__ W, const float* __restrict__ bias,
                                                     const int64_t* __restrict__ target, float scale, float eps,
                                                     float* __restrict__ logits, float* __restrict__ loss_n, int32_t* __restrict__ rank,
                                                     float* __restrict__ dlogits, float* __restrict__ dpooled) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    cls_ce_body<true>(sm, C, K, KG, pooled, W, bias, target, scale, eps, logits, loss_n, rank, dlogits, dpooled);
}

struct ClsPaths {
    const float* pooled[2];
    const float* dlogits[2];
    const float* loss_n[2];
};

// dW[k][c] = sum over paths and images of d logits[n][k] * pooled[n][c]  (blockIdx.y < ceil(K / 4): four classes x 256 features per
// workgroup, image loop unrolled by 8);  the last blockIdx.y row: db[k] = sum d logits[.][k] and loss = scale * sum loss_n.
// EX (k_cls_reduce): every sum is multiplied by gs (the upstream d loss, read from the device) and stored or, with acc, added to
// what the destination holds.
template <bool EX>
__device__ __forceinline__ void cls_put(float* dst, float v, float gs, int acc) {
    if constexpr (EX) {
        v *= gs;
        if (acc) v += *dst;
    }
    *dst = v;
}

// db[k] = sum over paths and images of d logits[n][k], one thread per class, images in order, in double
template <bool EX>
__device__ __forceinline__ void cls_db_row(int npath, int N, int K, const ClsPaths& P, float gs, int acc, float* __restrict__ db) {
    for (int k = threadIdx.x; k < K; k += 256) {
        double s = 0.0;
        for (int p = 0; p < npath; ++p)
            for (int n = 0; n < N; ++n) s += (double)P.dlogits[p][(size_t)n * K + k];
        cls_put<EX>(db + k, (float)s, gs, acc);
    }
}

// the four-class x 256-feature tile of dW of workgroup (blockIdx.x, blockIdx.y)
template <bool EX>
__device__ __forceinline__ void cls_dw_tile(float (*dl)[4], int npath, int N, int C, int K, const ClsPaths& P, float gs, int acc,
                                            float* __restrict__ dW) {
    const int tid = threadIdx.x;
    const int k0 = blockIdx.y * 4, c = blockIdx.x * 256 + tid;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int p = 0; p < npath; ++p) {
        const float* __restrict__ xp = P.pooled[p];
        const float* __restrict__ gp = P.dlogits[p];
        for (int nb = 0; nb < N; nb += 256) {
            __syncthreads();
            {
                const int n = nb + tid;
#pragma unroll
                for (int q = 0; q < 4; ++q) dl[tid][q] = (n < N && k0 + q < K) ? gp[(size_t)n * K + k0 + q] : 0.f;
            }
            __syncthreads();
            const int cnt = min(256, N - nb);
            if (c < C) {
                int i = 0;
                for (; i + 8 <= cnt; i += 8) {
                    float xv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) xv[u] = xp[(size_t)(nb + i + u) * C + c];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        a0 = fmaf(dl[i + u][0], xv[u], a0);
                        a1 = fmaf(dl[i + u][1], xv[u], a1);
                        a2 = fmaf(dl[i + u][2], xv[u], a2);
                        a3 = fmaf(dl[i + u][3], xv[u], a3);
                    }
                }
                for (; i < cnt; ++i) {
                    const float xv = xp[(size_t)(nb + i) * C + c];
                    a0 = fmaf(dl[i][0], xv, a0);
                    a1 = fmaf(dl[i][1], xv, a1);
                    a2 = fmaf(dl[i][2], xv, a2);
                    a3 = fmaf(dl[i][3], xv, a3);
                }
            }
        }
    }
    if (c < C) {
        if (k0 + 0 < K) cls_put<EX>(dW + (size_t)(k0 + 0) * C + c, a0, gs, acc);
        if (k0 + 1 < K) cls_put<EX>(dW + (size_t)(k0 + 1) * C + c, a1, gs, acc);
        if (k0 + 2 < K) cls_put<EX>(dW + (size_t)(k0 + 2) * C + c, a2, gs, acc);
        if (k0 + 3 < K) cls_put<EX>(dW + (size_t)(k0 + 3) * C + c, a3, gs, acc);
    }
}

// The first wave of the last blockIdx.y row, for all three summation kernels: sum of loss_n over npath paths in double (paths outer,
// images lane-strided, then the xor butterfly: a fixed order) and, with RANKS and a rank array, the counts rank < 1, rank < 5 and
// rank < 0 of those images.  Every lane returns the totals; without RANKS the counts are compiled out (k_cls_wgrad).
struct ClsRowSum {
    double s;
    int c1, c5, bad;
};
template <bool RANKS>
__device__ __forceinline__ ClsRowSum cls_sum_row(int npath, int N, const ClsPaths& P, const int32_t* __restrict__ rank) {
    const int lane = threadIdx.x;
    ClsRowSum r = {0.0, 0, 0, 0};
    for (int p = 0; p < npath; ++p)
        for (int n = lane; n < N; n += 64) r.s += (double)P.loss_n[p][n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r.s += __shfl_xor(r.s, o, 64);
    if constexpr (RANKS) {
        if (!rank) return r;                                 // (a kernel argument: the whole wave takes the same side)
        for (int n = lane; n < N; n += 64) {
            const int k = rank[n];
            r.bad += k < 0 ? 1 : 0;
            r.c1 += (k >= 0 && k < 1) ? 1 : 0;
            r.c5 += (k >= 0 && k < 5) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            r.c1 += __shfl_xor(r.c1, o, 64);
            r.c5 += __shfl_xor(r.c5, o, 64);
            r.bad += __shfl_xor(r.bad, o, 64);
        }
    }
    return r;
}

// meter += {sum loss_n, top-1, top-5, N, invalid}: one thread, ordinary loads and stores -- launches that share a meter are ordered
// by their stream
__device__ __forceinline__ void cls_meter_add(double* __restrict__ meter, const ClsRowSum& r, int N) {
    meter[0] += r.s;
    meter[1] += (double)r.c1;
    meter[2] += (double)r.c5;
    meter[3] += (double)N;
    meter[4] += (double)r.bad;
}

// The three summation kernels share one shape: blockIdx.y < ceil(K / 4) is a dW tile; workgroup (0, last row) does db, then its first
// wave calls cls_sum_row and thread 0 stores what that kernel owes.  k_cls_wgrad: loss[0] alone, no rank or meter code.
__global__ __launch_bounds__(256) void k_cls_wgrad(int npath, int N, int C, int K, ClsPaths P, float loss_scale,
                                                   float* __restrict__ dW, float* __restrict__ db, float* __restrict__ loss) {
    __shared__ float dl[256][4];
    const int tid = threadIdx.x;
    if ((int)blockIdx.y == (K + 3) >> 2) {
        if (blockIdx.x != 0) return;
        cls_db_row<false>(npath, N, K, P, 1.f, 0, db);
        if (tid >= 64) return;
        const ClsRowSum r = cls_sum_row<false>(npath, N, P, nullptr);
        if (tid == 0 && loss) loss[0] = (float)(r.s * (double)loss_scale);
        return;
    }
    cls_dw_tile<false>(dl, npath, N, C, K, P, 1.f, 0, dW);
}

// k_cls_wgrad + the search epoch's running meter (the w block of tail.SearchMeter): the loss sum of ALL paths, the counts of path
// 0's rank0 (the host passes NULL without a meter).
__global__ __launch_bounds__(256) void k_cls_wgrad_ex(int npath, int N, int C, int K, ClsPaths P, const int32_t* __restrict__ rank0,
                                                      float loss_scale, float* __restrict__ dW, float* __restrict__ db,
                                                      float* __restrict__ loss, double* __restrict__ meter) {
    __shared__ float dl[256][4];
    const int tid = threadIdx.x;
    if ((int)blockIdx.y == (K + 3) >> 2) {
        if (blockIdx.x != 0) return;
        cls_db_row<false>(npath, N, K, P, 1.f, 0, db);
        if (tid >= 64) return;
        const ClsRowSum r = cls_sum_row<true>(npath, N, P, rank0);
        if (tid == 0 && loss) loss[0] = (float)(r.s * (double)loss_scale);
        if (tid == 0 && meter) cls_meter_add(meter, r, N);
        return;
    }
    cls_dw_tile<false>(dl, npath, N, C, K, P, 1.f, 0, dW);
}

// The retrain tail's reduction over the images of ONE path: every dW / db sum is multiplied by gs (the upstream d loss, read from the
// device) and stored or, with acc, added.  Without dW / db (metrics only) the grid is the row's one workgroup.  Thread 0 writes
// out[4] = {mean loss, top-1 count, top-5 count, invalid count} and adds to the meter.
__global__ __launch_bounds__(256) void k_cls_reduce(int N, int C, int K, ClsPaths P, const int32_t* __restrict__ rank,
                                                    const float* __restrict__ gscale, int acc, float* __restrict__ dW,
                                                    float* __restrict__ db, float* __restrict__ out, double* __restrict__ meter) {
    __shared__ float dl[256][4];
    const int tid = threadIdx.x;
    const float gs = gscale ? gscale[0] : 1.f;
    if ((int)blockIdx.y == (dW ? (K + 3) >> 2 : 0)) {
        if (blockIdx.x != 0) return;
        if (db) cls_db_row<true>(1, N, K, P, gs, acc, db);
        if (tid >= 64 || !(out || meter)) return;
        const ClsRowSum r = cls_sum_row<true>(1, N, P, rank);
        if (tid == 0 && out) {
            out[0] = (float)(r.s / (double)N);
            out[1] = (float)r.c1;
            out[2] = (float)r.c5;
            out[3] = (float)r.bad;
        }
        if (tid == 0 && meter) cls_meter_add(meter, r, N);
        return;
    }
    cls_dw_tile<true>(dl, 1, N, C, K, P, gs, acc, dW);
}

// dst += src (n floats, a multiple of 4): the second bi-sampling path's share of a shared parameter's gradient
__global__ __launch_bounds__(256) void k_add_into(float* __restrict__ dst, const float* __restrict__ src, size_t n4) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 a = ld4(dst + 4 * i);
        const f32x4 b = ld4(src + 4 * i);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        st4(dst + 4 * i, a);
    }
}

// The per-image launch of both forms.  KG, the class groups of the d pooled phase: as many as fill the 1024 threads with (four
// feature columns x class range) items; none, and no [KG][C] LDS, in the forward-only form.
static int cls_ce_launch(bool ex, int N, int C, int K, const float* pooled, const float* W, const float* bias, const int64_t* target,
                         float scale, float eps, float* logits, float* loss_n, int32_t* rank, float* dlogits, float* dpooled,
                         void* stream) {
    int KG = 0;
    if (dpooled) {
        KG = CLS_T / (C >> 2);
        if (KG < 1) KG = 1;
        if (KG > 8) KG = 8;
        if (KG > K) KG = K;
    }
    const size_t shm = ((size_t)C + ((K + 3) & ~3) + (size_t)KG * C) * sizeof(float);
    if (shm > 64 * 1024) return TFNAS_ERANGE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope _prof(TK_SMALL, s);
    if (ex)
        hipLaunchKernelGGL(k_cls_ce_ex, dim3(N), dim3(CLS_T), shm, s, C, K, KG, pooled, W, bias, target, scale, eps, logits, loss_n,
                           rank, dlogits, dpooled);
    else
        hipLaunchKernelGGL(k_cls_ce, dim3(N), dim3(CLS_T), shm, s, C, K, KG, pooled, W, bias, target, scale, logits, loss_n, dlogits,
                           dpooled);
    return (int)hipGetLastError();
}

extern "C" int tfnas_cls_ce(int N, int C, int K, const float* pooled, const float* W, const float* bias, const int64_t* target,
                            float scale, float* logits, float* loss_n, float* dlogits, float* dpooled, void* stream) {
    if (!pooled || !W || !target || !logits || !loss_n || !dlogits || !dpooled) return TFNAS_ENULL;
    if (N < 1 || K < 1 || K > 4096 || C < 4 || C > 4096) return TFNAS_ERANGE;
    if (C & 3) return TFNAS_EINVAL;
    return cls_ce_launch(false, N, C, K, pooled, W, bias, target, scale, 0.f, logits, loss_n, nullptr, dlogits, dpooled, stream);
}

extern "C" int tfnas_cls_ce_ex(int N, int C, int K, const float* pooled, const float* W, const float* bias, const int64_t* target,
                               float scale, float eps, float* logits, float* loss_n, int32_t* rank, float* dlogits, float* dpooled,
                               void* stream) {
    if (!pooled || !W || !target || !logits || !loss_n || !rank) return TFNAS_ENULL;
    if (N < 1 || K < 1 || K > 4096 || C < 4 || C > 4096) return TFNAS_ERANGE;
    if (C & 3) return TFNAS_EINVAL;
    if ((dlogits == nullptr) != (dpooled == nullptr)) return TFNAS_EINVAL;       // both (training) or neither (forward only)
    if (!(eps >= 0.f && eps < 1.f)) return TFNAS_EINVAL;
    return cls_ce_launch(true, N, C, K, pooled, W, bias, target, scale, eps, logits, loss_n, rank, dlogits, dpooled, stream);
}

// The summation launch of all three forms: packs the npath paths' pointers, one workgroup per dW tile plus the last row -- that row
// alone without dW (tfnas_cls_reduce, metrics only).  `dst` is loss (the wgrad forms) or out[4] (REDUCE).
enum ClsSum { CLS_WGRAD, CLS_WGRAD_EX, CLS_REDUCE };
static int cls_sum_launch(ClsSum form, int npath, int N, int C, int K, const float* const* pooled, const float* const* dlogits,
                          const float* const* loss_n, const int32_t* rank, float loss_scale, const float* gscale, int acc, float* dW,
                          float* db, float* dst, double* meter, void* stream) {
    ClsPaths P = {};
    for (int p = 0; p < npath; ++p) {
        P.pooled[p] = pooled[p];
        P.dlogits[p] = dlogits[p];
        P.loss_n[p] = loss_n[p];
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope _prof(TK_SMALL, s);
    const dim3 grid = dW ? dim3(cdiv(C, 256), cdiv(K, 4) + 1) : dim3(1, 1);
    if (form == CLS_WGRAD)
        hipLaunchKernelGGL(k_cls_wgrad, grid, dim3(256), 0, s, npath, N, C, K, P, loss_scale, dW, db, dst);
    else if (form == CLS_WGRAD_EX)
        hipLaunchKernelGGL(k_cls_wgrad_ex, grid, dim3(256), 0, s, npath, N, C, K, P, rank, loss_scale, dW, db, dst, meter);
    else
        hipLaunchKernelGGL(k_cls_reduce, grid, dim3(256), 0, s, N, C, K, P, rank, gscale, acc, dW, db, dst, meter);
    return (int)hipGetLastError();
}

extern "C" int tfnas_cls_reduce(int N, int C, int K, const float* pooled, const float* dlogits, const float* loss_n,
                                const int32_t* rank, const float* gscale, int accumulate, float* dW, float* db, float* out,
                                double* meter, void* stream) {
    const bool grads = dW || db;
    if (!loss_n || !rank) return TFNAS_ENULL;
    if (grads && (!dW || !db || !pooled || !dlogits)) return TFNAS_ENULL;
    if (!grads && !out && !meter) return TFNAS_ENULL;        // nothing to write
    if (N < 1 || K < 1 || K > 4096 || C < 1 || C > 4096) return TFNAS_ERANGE;
    if (accumulate != 0 && accumulate != 1) return TFNAS_EINVAL;
    return cls_sum_launch(CLS_REDUCE, 1, N, C, K, &pooled, &dlogits, &loss_n, rank, 1.f, gscale, accumulate, dW, db, out, meter,
                          stream);
}

// the checks of tfnas_cls_wgrad and tfnas_cls_wgrad_ex, then the launch
static int cls_wgrad(ClsSum form, int npath, int N, int C, int K, const float* const* pooled, const float* const* dlogits,
                     const float* const* loss_n, const int32_t* rank0, float loss_scale, float* dW, float* db, float* loss,
                     double* meter, void* stream) {
    if (!pooled || !dlogits || !loss_n || !dW || !db) return TFNAS_ENULL;
    if (meter && !rank0) return TFNAS_ENULL;
    if (npath < 1 || npath > 2 || N < 1 || K < 1 || C < 1) return TFNAS_ERANGE;
    for (int p = 0; p < npath; ++p)
        if (!pooled[p] || !dlogits[p] || !loss_n[p]) return TFNAS_ENULL;
    return cls_sum_launch(form, npath, N, C, K, pooled, dlogits, loss_n, meter ? rank0 : nullptr, loss_scale, nullptr, 0, dW, db, loss,
                          meter, stream);
}

extern "C" int tfnas_cls_wgrad(int npath, int N, int C, int K, const float* const* pooled, const float* const* dlogits,
                               const float* const* loss_n, float loss_scale, float* dW, float* db, float* loss, void* stream) {
    return cls_wgrad(CLS_WGRAD, npath, N, C, K, pooled, dlogits, loss_n, nullptr, loss_scale, dW, db, loss, nullptr, stream);
}

extern "C" int tfnas_cls_wgrad_ex(int npath, int N, int C, int K, const float* const* pooled, const float* const* dlogits,
                                  const float* const* loss_n, const int32_t* rank0, float loss_scale, float* dW, float* db,
                                  float* loss, double* meter, void* stream) {
    return cls_wgrad(CLS_WGRAD_EX, npath, N, C, K, pooled, dlogits, loss_n, rank0, loss_scale, dW, db, loss, meter, stream);
}

extern "C" int tfnas_add_into(float* dst, const float* src, uint64_t count, void* stream) {
    if (!dst || !src) return TFNAS_ENULL;
    if (count & 3) return TFNAS_EINVAL;
    if (!count) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope _prof(TK_SMALL, s);
    size_t blocks = cdiv64(count / 4, 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_add_into, dim3((unsigned)blocks), dim3(256), 0, s, dst, src, (size_t)(count / 4));
    return (int)hipGetLastError();
}
