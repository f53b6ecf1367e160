// Fused optimizer steps of the search loop: gradient-norm clipping + the parameter update in two
// launches for the weights (multi-range SGD) and ONE launch for the architecture parameters (Adam + log-softmax projection).
//
// Reference: train_search.py:381-385 (clip_grad_norm_(weight_parameters, 5) + SGD(momentum 0.9, wd 1e-5).step()) and
// :414-422 (clip_grad_norm_(arch_parameters, 5) + Adam(lr 0.01, betas (0.5, 0.999), wd 5e-4).step() + the per-parameter
// log_softmax projection).  torch.optim only touches parameters whose .grad is not None; with bi-sampling that is the two
// sampled candidates of every cell plus stems / head -- here: a list of ranges of the flat weight / gradient / momentum
// arenas (tfnas_amd/path.py: WeightArena), one range per sampled candidate.
#include "tfnas_dev.h"
#include "kernels.h"
#include "prof.h"

#define OPT_MAX_RANGES 64
#define OPT_CHUNK 8192                     // floats per workgroup: 256 threads x 8 float4

struct OptRanges {
    int n;
    int nblocks;
    uint64_t off[OPT_MAX_RANGES];          // float offsets into the arenas (multiples of 4)
    uint64_t goff[OPT_MAX_RANGES];         // float offsets of the same ranges in the gradient buffer (== off, or packed)
    uint64_t len[OPT_MAX_RANGES];          // floats (multiples of 4: arena slots are padded to 64)
    int first_block[OPT_MAX_RANGES + 1];   // prefix sum of ceil(len / OPT_CHUNK)
};

// workgroup b -> [beg, end) in the arenas and gbeg = start of the same chunk in the gradient buffer
__device__ __forceinline__ bool opt_locate(const OptRanges& R, int b, uint64_t& beg, uint64_t& end, uint64_t& gbeg) {
    int r = 0;
    while (r + 1 < R.n && b >= R.first_block[r + 1]) ++r;
    const uint64_t lo = (uint64_t)(b - R.first_block[r]) * OPT_CHUNK;
    if (lo >= R.len[r]) return false;
    beg = R.off[r] + lo;
    gbeg = R.goff[r] + lo;
    const uint64_t hi = lo + OPT_CHUNK < R.len[r] ? lo + OPT_CHUNK : R.len[r];
    end = R.off[r] + hi;
    return true;
}

__device__ __forceinline__ double block_sum_d(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// partial[b] = sum of g^2 over workgroup b's chunk (double; fixed order -> deterministic)
__global__ __launch_bounds__(256) void k_opt_sqnorm(const float* __restrict__ g, OptRanges R, double* __restrict__ partial) {
    __shared__ double sh[4];
    uint64_t beg, end, gbeg;
    double acc = 0.0;
    if (opt_locate(R, blockIdx.x, beg, end, gbeg)) {
        for (uint64_t i = 4 * (uint64_t)threadIdx.x; i < end - beg; i += 1024) {
            const f32x4 v = ld4(g + gbeg + i);
            acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
    }
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// total = sqrt(sum partial) * grad_scale;  coef = min(1, max_norm / (total + 1e-6))   (torch.nn.utils.clip_grad_norm_)
// g' = g * grad_scale * coef;  d = g' + wd * w;  m = momentum * m + d;  w -= lr * m    (torch.optim.SGD, dampening 0)
__global__ __launch_bounds__(256) void k_opt_sgd(float* __restrict__ w, float* __restrict__ g, float* __restrict__ m,
                                                 OptRanges R, const double* __restrict__ partial, float max_norm, float lr,
                                                 float momentum, float wd, float grad_scale, float* __restrict__ norm_out) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < R.nblocks; i += 256) acc += partial[i];
    acc = block_sum_d(acc, sh);
    const float total = (float)sqrt(acc) * grad_scale;
    float coef = max_norm > 0.f ? max_norm / (total + 1e-6f) : 1.f;
    coef = coef > 1.f ? 1.f : coef;
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = total;
    const float gs = grad_scale * coef;
    uint64_t beg, end, gbeg;
    if (!opt_locate(R, blockIdx.x, beg, end, gbeg)) return;
    for (uint64_t k = 4 * (uint64_t)threadIdx.x; k < end - beg; k += 1024) {
        const uint64_t i = beg + k;
        f32x4 gv = ld4(g + gbeg + k), wv = ld4(w + i), mv = ld4(m + i);
        gv = gv * splat4(gs);
        st4(g + gbeg + k, gv);                           // (the clipped gradient stays readable, as after clip_grad_norm_)
        const f32x4 d = gv + splat4(wd) * wv;
        mv = splat4(momentum) * mv + d;
        wv = wv - splat4(lr) * mv;
        st4(m + i, mv);
        st4(w + i, wv);
    }
}

__device__ __forceinline__ f32x4 ema_lerp4(f32x4 e, f32x4 v, float alpha) {
    f32x4 r;
    r.x = __builtin_fmaf(alpha, v.x - e.x, e.x);
    r.y = __builtin_fmaf(alpha, v.y - e.y, e.y);
    r.z = __builtin_fmaf(alpha, v.z - e.z, e.z);
    r.w = __builtin_fmaf(alpha, v.w - e.w, e.w);
    return r;
}

// k_opt_sgd with an exponential moving average of the weights (tfnas_sgd_clip_ema_step): where w' is stored -- it sits in a
// register there -- e' = fma(alpha, w' - e, e) is stored too: one more read and one more write of an arena-sized buffer, no
// launch.  A sibling and not a template parameter of k_opt_sgd: as the <false> instantiation of a shared body that kernel came
// out with its address set-up scheduled differently, and its device code is to stay what it was.  The test that
// holds w' / g' / m' / norm of the two kernels to the same bits (tests/test_gpu_ema_kernels.py) keeps the copies together.
__global__ __launch_bounds__(256) void k_opt_sgd_ema(float* __restrict__ w, float* __restrict__ g, float* __restrict__ m,
                                                     OptRanges R, const double* __restrict__ partial, float max_norm, float lr,
                                                     float momentum, float wd, float grad_scale, float* __restrict__ norm_out,
                                                     float* __restrict__ ema, float ema_alpha) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < R.nblocks; i += 256) acc += partial[i];
    acc = block_sum_d(acc, sh);
    const float total = (float)sqrt(acc) * grad_scale;
    float coef = max_norm > 0.f ? max_norm / (total + 1e-6f) : 1.f;
    coef = coef > 1.f ? 1.f : coef;
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = total;
    const float gs = grad_scale * coef;
    uint64_t beg, end, gbeg;
    if (!opt_locate(R, blockIdx.x, beg, end, gbeg)) return;
    for (uint64_t k = 4 * (uint64_t)threadIdx.x; k < end - beg; k += 1024) {
        const uint64_t i = beg + k;
        f32x4 gv = ld4(g + gbeg + k), wv = ld4(w + i), mv = ld4(m + i);
        gv = gv * splat4(gs);
        st4(g + gbeg + k, gv);
        const f32x4 d = gv + splat4(wd) * wv;
        mv = splat4(momentum) * mv + d;
        wv = wv - splat4(lr) * mv;
        st4(m + i, mv);
        st4(w + i, wv);
        st4(ema + i, ema_lerp4(ld4(ema + i), wv, ema_alpha));
    }
}

// ema[ranges] = fma(alpha, src - ema, ema): the same formula on its own (BatchNorm running statistics, which no optimizer pass
// touches; the parameters of a step that torch's optimizer made)
__global__ __launch_bounds__(256) void k_ema_lerp(float* __restrict__ ema, const float* __restrict__ src, OptRanges R, float alpha) {
    uint64_t beg, end, gbeg;
    if (!opt_locate(R, blockIdx.x, beg, end, gbeg)) return;
    for (uint64_t k = 4 * (uint64_t)threadIdx.x; k < end - beg; k += 1024)
        st4(ema + beg + k, ema_lerp4(ld4(ema + beg + k), ld4(src + beg + k), alpha));
}

// dst[packed] = src[ranges]: the sampled candidates' gradient ranges as ONE contiguous message for the all-reduce
__global__ __launch_bounds__(256) void k_opt_pack(const float* __restrict__ src, float* __restrict__ dst, OptRanges R) {
    uint64_t beg, end, gbeg;
    if (!opt_locate(R, blockIdx.x, beg, end, gbeg)) return;
    for (uint64_t k = 4 * (uint64_t)threadIdx.x; k < end - beg; k += 1024) st4(dst + gbeg + k, ld4(src + beg + k));
}

static int fill_ranges(OptRanges& R, int nranges, const uint64_t* off, const uint64_t* goff, const uint64_t* len) {
    if (nranges < 1 || nranges > OPT_MAX_RANGES) return TFNAS_ERANGE;
    R.n = nranges;
    int nb = 0;
    for (int i = 0; i < nranges; ++i) {
        if ((off[i] & 3) || (len[i] & 3) || len[i] == 0 || (goff && (goff[i] & 3))) return TFNAS_EINVAL;
        R.off[i] = off[i];
        R.goff[i] = goff ? goff[i] : off[i];
        R.len[i] = len[i];
        R.first_block[i] = nb;
        nb += (int)((len[i] + OPT_CHUNK - 1) / OPT_CHUNK);
    }
    R.first_block[nranges] = nb;
    R.nblocks = nb;
    // ranges must be disjoint, in the arenas and in the gradient buffer: two workgroups would otherwise update the same floats
    // (and the norm would count them twice).  <= 64 ranges: a plain O(n^2) loop
    for (int i = 0; i < nranges; ++i)
        for (int j = i + 1; j < nranges; ++j) {
            if (R.off[i] < R.off[j] + R.len[j] && R.off[j] < R.off[i] + R.len[i]) return TFNAS_EINVAL;
            if (goff && R.goff[i] < R.goff[j] + R.len[j] && R.goff[j] < R.goff[i] + R.len[i]) return TFNAS_EINVAL;
        }
    return 0;
}

int launch_pack_ranges(const float* src, float* dst, int nranges, const uint64_t* off, const uint64_t* doff,
                       const uint64_t* len, hipStream_t s) {
    OptRanges R;
    int rc = fill_ranges(R, nranges, off, doff, len);
    if (rc) return rc;
    ProfScope _prof(TK_SMALL, s);
    hipLaunchKernelGGL(k_opt_pack, dim3(R.nblocks), dim3(256), 0, s, src, dst, R);
    return (int)hipGetLastError();
}

int launch_sgd_clip_step(float* w, float* g, float* m, int nranges, const uint64_t* off, const uint64_t* goff,
                         const uint64_t* len, float max_norm,
                         float lr, float momentum, float wd, float grad_scale, double* scratch, uint64_t scratch_doubles,
                         float* norm_out, hipStream_t s) {
    OptRanges R;
    int rc = fill_ranges(R, nranges, off, goff, len);
    if (rc) return rc;
    const int nb = R.nblocks;
    if ((uint64_t)nb > scratch_doubles) return TFNAS_ERANGE;
    ProfScope _prof(TK_SMALL, s);
    hipLaunchKernelGGL(k_opt_sqnorm, dim3(nb), dim3(256), 0, s, g, R, scratch);
    hipLaunchKernelGGL(k_opt_sgd, dim3(nb), dim3(256), 0, s, w, g, m, R, scratch, max_norm, lr, momentum, wd, grad_scale,
                       norm_out);
    return (int)hipGetLastError();
}

// the step weight of an EMA: 1 - decay as the caller formed it, in [0, 1] (a NaN fails both comparisons)
static bool ema_alpha_ok(float a) { return a >= 0.f && a <= 1.f; }

int launch_sgd_clip_ema_step(float* w, float* g, float* m, int nranges, const uint64_t* off, const uint64_t* goff,
                             const uint64_t* len, float max_norm, float lr, float momentum, float wd, float grad_scale,
                             float* ema, float ema_alpha, double* scratch, uint64_t scratch_doubles, float* norm_out,
                             hipStream_t s) {
    if (!ema_alpha_ok(ema_alpha)) return TFNAS_EINVAL;
    if (ema == w || ema == g || ema == m) return TFNAS_EINVAL;
    OptRanges R;
    int rc = fill_ranges(R, nranges, off, goff, len);
    if (rc) return rc;
    const int nb = R.nblocks;
    if ((uint64_t)nb > scratch_doubles) return TFNAS_ERANGE;
    ProfScope _prof(TK_SMALL, s);
    hipLaunchKernelGGL(k_opt_sqnorm, dim3(nb), dim3(256), 0, s, g, R, scratch);
    hipLaunchKernelGGL(k_opt_sgd_ema, dim3(nb), dim3(256), 0, s, w, g, m, R, scratch, max_norm, lr, momentum, wd, grad_scale,
                       norm_out, ema, ema_alpha);
    return (int)hipGetLastError();
}

int launch_ema_lerp(float* ema, const float* src, int nranges, const uint64_t* off, const uint64_t* len, float ema_alpha,
                    hipStream_t s) {
    if (!ema_alpha_ok(ema_alpha)) return TFNAS_EINVAL;
    if (ema == src) return TFNAS_EINVAL;
    OptRanges R;
    int rc = fill_ranges(R, nranges, off, nullptr, len);
    if (rc) return rc;
    ProfScope _prof(TK_SMALL, s);
    hipLaunchKernelGGL(k_ema_lerp, dim3(R.nblocks), dim3(256), 0, s, ema, src, R, ema_alpha);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Retrain tail for parameter groups (tfnas_opt_groups_step): the whole arena [0, total) with a per-64-float-block group id
// (gmap) that selects lr / wd from a table of <= 8 groups; SGD (plain / Nesterov), RMSprop (torch's form, with and without
// momentum) and RMSprop in TensorFlow's form, each with and without the weight EMA.  Grid, chunking and prologue of k_opt_sgd.
enum { OG_SGD = 0, OG_NESTEROV = 1, OG_RMS = 2, OG_RMS_NOMOM = 3, OG_RMS_TF = 4 };

struct OptGroupsK {
    int ngroups, nblocks;
    float lr[TFNAS_OPT_MAX_GROUPS], wd[TFNAS_OPT_MAX_GROUPS];
    float momentum, alpha, one_minus_alpha, eps, max_norm, grad_scale, ema_alpha;
};

// one element of the update; v / m are in-out where the mode keeps them
template <int MODE>
__device__ __forceinline__ float og_update(float w, float gc, float& m, float& v, float lr, float wd, const OptGroupsK& A) {
    const float d = gc + wd * w;
    if (MODE == OG_SGD || MODE == OG_NESTEROV) {
        m = A.momentum * m + d;
        return MODE == OG_SGD ? w - lr * m : w - lr * (d + A.momentum * m);
    } else if (MODE == OG_RMS || MODE == OG_RMS_NOMOM) {
        v = A.alpha * v + A.one_minus_alpha * (d * d);
        const float u = d / (__builtin_sqrtf(v) + A.eps);
        if (MODE == OG_RMS_NOMOM) return w - lr * u;
        m = A.momentum * m + u;
        return w - lr * m;
    } else {
        v = v + A.one_minus_alpha * (d * d - v);
        m = A.momentum * m + (lr * d) / __builtin_sqrtf(v + A.eps);
        return w - m;
    }
}

template <int MODE, bool EMA>
__global__ __launch_bounds__(256) void k_opt_groups(float* __restrict__ w, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, float* __restrict__ ema,
                                                    const uint8_t* __restrict__ gmap, uint64_t total_floats, OptGroupsK A,
                                                    const double* __restrict__ partial, float* __restrict__ norm_out) {
    constexpr bool HAS_M = MODE != OG_RMS_NOMOM, HAS_V = MODE >= OG_RMS;
    __shared__ double sh[4];
    __shared__ float s_lr[TFNAS_OPT_MAX_GROUPS], s_wd[TFNAS_OPT_MAX_GROUPS];
    if (threadIdx.x < TFNAS_OPT_MAX_GROUPS) {             // (visible after the barriers of block_sum_d)
        s_lr[threadIdx.x] = A.lr[threadIdx.x];
        s_wd[threadIdx.x] = A.wd[threadIdx.x];
    }
    double acc = 0.0;
    for (int i = threadIdx.x; i < A.nblocks; i += 256) acc += partial[i];
    acc = block_sum_d(acc, sh);
    const float total = (float)sqrt(acc) * A.grad_scale;
    float coef = A.max_norm > 0.f ? A.max_norm / (total + 1e-6f) : 1.f;
    coef = coef > 1.f ? 1.f : coef;
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = total;
    const float gs = A.grad_scale * coef;
    const uint64_t beg = (uint64_t)blockIdx.x * OPT_CHUNK;
    const uint64_t end = beg + OPT_CHUNK < total_floats ? beg + OPT_CHUNK : total_floats;
    for (uint64_t i = beg + 4 * (uint64_t)threadIdx.x; i < end; i += 1024) {
        f32x4 gv = ld4(g + i);
        gv = gv * splat4(gs);
        st4(g + i, gv);
        const unsigned id = gmap[i >> 6];                 // the group of this float4's 64-float block: the same for 16 lanes
        if (id >= (unsigned)A.ngroups) continue;          // not in the table: the block's w / m / v / ema stay as they are
        const float lr = s_lr[id], wd = s_wd[id];
        f32x4 wv = ld4(w + i), mv = splat4(0.f), vv = splat4(0.f);
        if (HAS_M) mv = ld4(m + i);
        if (HAS_V) vv = ld4(v + i);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float mc = mv[c], vc = vv[c];
            wv[c] = og_update<MODE>(wv[c], gv[c], mc, vc, lr, wd, A);
            mv[c] = mc;
            vv[c] = vc;
        }
        if (HAS_V) st4(v + i, vv);
        if (HAS_M) st4(m + i, mv);
        st4(w + i, wv);
        if (EMA) st4(ema + i, ema_lerp4(ld4(ema + i), wv, A.ema_alpha));
    }
}

template <int MODE>
static void og_launch(bool with_ema, int nb, hipStream_t s, float* w, float* g, float* m, float* v, float* ema,
                      const uint8_t* gmap, uint64_t total, const OptGroupsK& A, const double* partial, float* norm_out) {
    if (with_ema)
        hipLaunchKernelGGL((k_opt_groups<MODE, true>), dim3(nb), dim3(256), 0, s, w, g, m, v, ema, gmap, total, A, partial, norm_out);
    else
        hipLaunchKernelGGL((k_opt_groups<MODE, false>), dim3(nb), dim3(256), 0, s, w, g, m, v, ema, gmap, total, A, partial, norm_out);
}

int launch_opt_groups_step(const TfnasOptGroups* d, float* w, float* g, float* m, float* v, float* ema, const uint8_t* gmap,
                           uint64_t total, double* scratch, uint64_t scratch_doubles, float* norm_out, hipStream_t s) {
    if (!d || !w || !g || !m || !gmap || !scratch) return TFNAS_ENULL;
    const bool rms = d->kind == TFNAS_OPT_RMSPROP || d->kind == TFNAS_OPT_RMSPROP_TF;
    if (d->kind != TFNAS_OPT_SGD && !rms) return TFNAS_EINVAL;
    if (rms && !v) return TFNAS_ENULL;
    if (total == 0 || (total & 63)) return TFNAS_EINVAL;
    if (d->ngroups < 1 || d->ngroups > TFNAS_OPT_MAX_GROUPS) return TFNAS_ERANGE;
    if (d->flags & ~TFNAS_OPT_NESTEROV) return TFNAS_EINVAL;
    const bool nesterov = (d->flags & TFNAS_OPT_NESTEROV) != 0;
    if (nesterov && d->kind != TFNAS_OPT_SGD) return TFNAS_EINVAL;
    for (int k = 0; k < d->ngroups; ++k)
        if (!std::isfinite(d->lr[k]) || !std::isfinite(d->wd[k])) return TFNAS_EINVAL;
    if (!std::isfinite(d->momentum) || !std::isfinite(d->max_norm) || !std::isfinite(d->grad_scale)) return TFNAS_EINVAL;
    if (!std::isfinite(d->alpha) || !std::isfinite(d->eps)) return TFNAS_EINVAL;
    if (rms && (!(d->alpha >= 0.f && d->alpha <= 1.f) || !(d->eps > 0.f))) return TFNAS_EINVAL;
    if (d->momentum < 0.f || (nesterov && !(d->momentum > 0.f))) return TFNAS_EINVAL;
    if (ema) {
        if (!ema_alpha_ok(d->ema_alpha)) return TFNAS_EINVAL;
        if (ema == w || ema == g || ema == m || ema == v) return TFNAS_EINVAL;
    }
    const uint64_t nb64 = (total + OPT_CHUNK - 1) / OPT_CHUNK;
    if (nb64 > scratch_doubles) return TFNAS_ERANGE;
    if (nb64 > 0x7fffffffull) return TFNAS_ERANGE;
    const int nb = (int)nb64;
    OptRanges R;
    const uint64_t zero = 0;
    int rc = fill_ranges(R, 1, &zero, nullptr, &total);
    if (rc) return rc;
    OptGroupsK A;
    A.ngroups = d->ngroups;
    A.nblocks = nb;
    for (int k = 0; k < TFNAS_OPT_MAX_GROUPS; ++k) {
        A.lr[k] = k < d->ngroups ? d->lr[k] : 0.f;
        A.wd[k] = k < d->ngroups ? d->wd[k] : 0.f;
    }
    A.momentum = d->momentum;
    A.alpha = d->alpha;
    A.one_minus_alpha = (float)(1.0 - (double)d->alpha);
    A.eps = d->eps;
    A.max_norm = d->max_norm;
    A.grad_scale = d->grad_scale;
    A.ema_alpha = ema ? d->ema_alpha : 0.f;
    {   // (a scope per kernel: tfnas_prof_collect counts this step's two launches as two)
        ProfScope _prof(TK_SMALL, s);
        hipLaunchKernelGGL(k_opt_sqnorm, dim3(nb), dim3(256), 0, s, g, R, scratch);
    }
    ProfScope _prof(TK_SMALL, s);
    const bool e = ema != nullptr;
    if (d->kind == TFNAS_OPT_SGD) {
        if (nesterov) og_launch<OG_NESTEROV>(e, nb, s, w, g, m, v, ema, gmap, total, A, scratch, norm_out);
        else og_launch<OG_SGD>(e, nb, s, w, g, m, v, ema, gmap, total, A, scratch, norm_out);
    } else if (d->kind == TFNAS_OPT_RMSPROP) {
        if (d->momentum > 0.f) og_launch<OG_RMS>(e, nb, s, w, g, m, v, ema, gmap, total, A, scratch, norm_out);
        else og_launch<OG_RMS_NOMOM>(e, nb, s, w, g, m, v, ema, gmap, total, A, scratch, norm_out);
    } else {
        og_launch<OG_RMS_TF>(e, nb, s, w, g, m, v, ema, gmap, total, A, scratch, norm_out);
    }
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Architecture parameters: <= 32 tensors of <= 8 floats.  One workgroup: clip over all of them, Adam, projection.
struct ArchOpt {
    int n;
    int len[TFNAS_MAX_CELLS];
    float* p[TFNAS_MAX_CELLS];
    const float* g[TFNAS_MAX_CELLS];
};

__global__ __launch_bounds__(256) void k_arch_adam_project(ArchOpt A, float* __restrict__ m, float* __restrict__ v,
                                                           float max_norm, float lr, float b1, float b2, float eps, float wd,
                                                           float bias1, float bias2_sqrt, float grad_scale,
                                                           float* __restrict__ norm_out) {
    __shared__ float sq[256];
    __shared__ float newp[256];
    const int t = threadIdx.x >> 3, j = threadIdx.x & 7;       // tensor, element (256 threads = 32 tensors x 8)
    const bool live = t < A.n && j < A.len[t];
    float gv = live ? A.g[t][j] * grad_scale : 0.f;
    sq[threadIdx.x] = gv * gv;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sq[threadIdx.x] += sq[threadIdx.x + o];
        __syncthreads();
    }
    const float total = sqrtf(sq[0]);
    float coef = max_norm > 0.f ? max_norm / (total + 1e-6f) : 1.f;
    coef = coef > 1.f ? 1.f : coef;
    if (threadIdx.x == 0 && norm_out) *norm_out = total;
    float pv = 0.f;
    if (live) {
        pv = A.p[t][j];
        gv = gv * coef + wd * pv;                               // torch Adam: weight decay is added to the gradient
        const int k = t * 8 + j;
        const float mk = b1 * m[k] + (1.f - b1) * gv;
        const float vk = b2 * v[k] + (1.f - b2) * gv * gv;
        m[k] = mk;
        v[k] = vk;
        const float denom = sqrtf(vk) / bias2_sqrt + eps;
        pv = pv - (lr / bias1) * (mk / denom);
    }
    newp[threadIdx.x] = live ? pv : -INFINITY;
    __syncthreads();
    if (live) {                                                 // p <- log_softmax(p) over the tensor (train_search.py:421-422)
        float mx = -INFINITY;
        for (int i = 0; i < A.len[t]; ++i) mx = fmaxf(mx, newp[t * 8 + i]);
        float se = 0.f;
        for (int i = 0; i < A.len[t]; ++i) se += expf(newp[t * 8 + i] - mx);
        A.p[t][j] = (pv - mx) - logf(se);
    }
}

int launch_arch_adam_project(int n, float* const* p, const float* const* g, const int32_t* len, float* m, float* v,
                             float max_norm, float lr, float b1, float b2, float eps, float wd, int step, float grad_scale,
                             float* norm_out, hipStream_t s) {
    if (n < 1 || n > TFNAS_MAX_CELLS) return TFNAS_ERANGE;
    ArchOpt A;
    A.n = n;
    for (int i = 0; i < n; ++i) {
        if (!p[i] || !g[i]) return TFNAS_ENULL;
        if (len[i] < 1 || len[i] > 8) return TFNAS_ERANGE;
        A.len[i] = len[i];
        A.p[i] = p[i];
        A.g[i] = g[i];
    }
    const double bias1 = 1.0 - pow((double)b1, (double)step), bias2 = 1.0 - pow((double)b2, (double)step);
    ProfScope _prof(TK_SMALL, s);
    hipLaunchKernelGGL(k_arch_adam_project, dim3(1), dim3(256), 0, s, A, m, v, max_norm, lr, b1, b2, eps, wd, (float)bias1,
                       (float)sqrt(bias2), grad_scale, norm_out);
    return (int)hipGetLastError();
}
