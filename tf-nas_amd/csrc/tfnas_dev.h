// Device-side helpers shared by all gfx950 kernels of the TF-NAS hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tfnas_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define TFNAS_THREADS 256

#define HIP_TRY(expr)                         \
    do {                                      \
        hipError_t _e = (expr);               \
        if (_e != hipSuccess) return (int)_e; \
    } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline uint64_t cdiv64(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// ----------------------------------------------------------------------------- activations
// reference: Swish = x * sigmoid(x) (models/layers.py:26-35), ReLU (layers.py:470-471), ReLU6 / HardSwish (layers.py:38-47)
// 1/(1+e^-x) through v_exp_f32 + v_rcp_f32 (1 ulp each).  An IEEE `/` costs ~10 more VALU instructions per element
// (v_div_scale x2, fma chain, v_div_fmas, v_div_fixup), and the operand loaders that apply the activation are VALU-issue
// bound: 682 VALU instructions per 32 MFMAs in k_project_fwd<4, swish> before this.
__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
// ReLU6 = min(max(x, 0), 6), hard-swish = x * min(max(x + 3, 0), 6) / 6 (layers.py:38-47): no transcendental.  The derivatives
// are torch's: hardtanh backward is 1 strictly inside (0, 6); hardswish backward is (2x + 3) / 6 strictly inside (-3, 3), 1 from 3
// up, 0 from -3 down.  ReLU6's lower kink decides exactly as ReLU's does (x > 0).
// Every fork is exhaustive: a value the kernels were not written for does not compile.
template <int ACT>
__device__ __forceinline__ float act_f(float x) {
    static_assert(ACT == TFNAS_ACT_RELU || ACT == TFNAS_ACT_SWISH || ACT == TFNAS_ACT_RELU6 || ACT == TFNAS_ACT_HSWISH,
                  "unknown activation");
    if constexpr (ACT == TFNAS_ACT_RELU) return fmaxf(x, 0.f);
    else if constexpr (ACT == TFNAS_ACT_SWISH) return x * sigmoid_f(x);
    else if constexpr (ACT == TFNAS_ACT_RELU6) return fminf(fmaxf(x, 0.f), 6.f);
    else return x * fminf(fmaxf(x + 3.f, 0.f), 6.f) * (1.f / 6.f);
}
// derivative w.r.t. the pre-activation x
template <int ACT>
__device__ __forceinline__ float act_d(float x) {
    static_assert(ACT == TFNAS_ACT_RELU || ACT == TFNAS_ACT_SWISH || ACT == TFNAS_ACT_RELU6 || ACT == TFNAS_ACT_HSWISH,
                  "unknown activation");
    if constexpr (ACT == TFNAS_ACT_RELU) return x > 0.f ? 1.f : 0.f;
    else if constexpr (ACT == TFNAS_ACT_SWISH) {
        const float s = sigmoid_f(x);
        return s * (1.f + x * (1.f - s));
    } else if constexpr (ACT == TFNAS_ACT_RELU6) return (x > 0.f && x < 6.f) ? 1.f : 0.f;
    else return x >= 3.f ? 1.f : (x > -3.f ? (2.f * x + 3.f) * (1.f / 6.f) : 0.f);
}
template <int ACT>
__device__ __forceinline__ f32x4 act_f4(f32x4 v) {
    f32x4 r;
    r.x = act_f<ACT>(v.x); r.y = act_f<ACT>(v.y); r.z = act_f<ACT>(v.z); r.w = act_f<ACT>(v.w);
    return r;
}
template <int ACT>
__device__ __forceinline__ f32x4 act_d4(f32x4 v) {
    f32x4 r;
    r.x = act_d<ACT>(v.x); r.y = act_d<ACT>(v.y); r.z = act_d<ACT>(v.z); r.w = act_d<ACT>(v.w);
    return r;
}
// The gate function of the squeeze-excite branch (TfnasCellDesc.se_style, GATE = SE_GATE_* of kernels.h): 0 the logistic function,
// 1 torch's hardsigmoid min(max(v + 3, 0), 6) / 6.  The backward keeps only the gate itself, so the derivative is written in
// it: dgl = dgate * gate * (1 - gate), or dgate / 6 strictly inside 0 < gate < 1 (v strictly inside (-3, 3): hardsigmoid's
// backward), 0 where the gate saturated.
template <int GATE>
__device__ __forceinline__ float se_gate_f(float v) {
    static_assert(GATE == 0 || GATE == 1, "unknown gate");
    if constexpr (GATE == 0) return sigmoid_f(v);
    else return fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f);
}
template <int GATE>
__device__ __forceinline__ float se_gate_bwd(float dgate, float gate) {
    static_assert(GATE == 0 || GATE == 1, "unknown gate");
    if constexpr (GATE == 0) return dgate * gate * (1.f - gate);
    else return (gate > 0.f && gate < 1.f) ? dgate * (1.f / 6.f) : 0.f;
}
template <int GATE>
__device__ __forceinline__ f32x4 se_gate_bwd4(f32x4 dgate, f32x4 gate) {
    if constexpr (GATE == 0) {
        const f32x4 one4 = {1.f, 1.f, 1.f, 1.f};
        return dgate * gate * (one4 - gate);
    } else {
        f32x4 r;
        r.x = se_gate_bwd<GATE>(dgate.x, gate.x); r.y = se_gate_bwd<GATE>(dgate.y, gate.y);
        r.z = se_gate_bwd<GATE>(dgate.z, gate.z); r.w = se_gate_bwd<GATE>(dgate.w, gate.w);
        return r;
    }
}

// ----------------------------------------------------------------------------- batch-norm constants
// stats layout: [channel][2] doubles = (sum, sum of squares) over `cnt` elements.
// BN of the search net: (x-mean)/sqrt(var_biased+eps), no affine (layers.py:469,498,533).
// eps < 0: the table already holds the EFFECTIVE (mean, rstd) of an affine / eval-mode BatchNorm, written by k_bn_fwd_fix
// (bn_affine.hip): gamma*(x-mu)*rho + beta == (x - mean_eff) * rstd_eff with rstd_eff = gamma*rho, mean_eff = mu - beta/rstd_eff.
__device__ __forceinline__ float2 bn_consts(const double* st, double inv_cnt, float eps) {
    if (eps < 0.f) return make_float2((float)st[0], (float)st[1]);
    double m = st[0] * inv_cnt;
    double v = st[1] * inv_cnt - m * m;
    if (v < 0.0) v = 0.0;
    return make_float2((float)m, (float)(1.0 / sqrt(v + (double)eps)));
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
// non-temporal variants for the once-through [pixels][M] streams E, D, dZ, dEh (fp32; see dw_stream.inc)
#ifdef TFNAS_NO_NT
__device__ __forceinline__ f32x4 ld4_nt(const float* p) { return ld4(p); }
__device__ __forceinline__ void st4_nt(float* p, f32x4 v) { st4(p, v); }
#else
__device__ __forceinline__ f32x4 ld4_nt(const float* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
}
__device__ __forceinline__ void st4_nt(float* p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); }
#endif

__device__ __forceinline__ f32x4 zero4() { f32x4 z = {0.f, 0.f, 0.f, 0.f}; return z; }
__device__ __forceinline__ f32x4 splat4(float a) { f32x4 z = {a, a, a, a}; return z; }

// dx + w*g with the product rounded separately (what the sink's scaled copy followed by autograd's add computed before the
// two were folded into this epilogue): keeps the path level bit-identical to the per-cell route
__device__ __forceinline__ f32x4 sink_add(f32x4 v, float w, f32x4 g) {
    // the product must be rounded on its own: -ffp-contract=fast would fuse it into the add (HIP's __fmul_rn / __fadd_rn
    // are plain * and +, and `#pragma clang fp contract(off)` did not survive inlining here) -- the empty asm makes each
    // product opaque to the contraction pass
    float px = w * g.x, py = w * g.y, pz = w * g.z, pw = w * g.w;
    asm volatile("" : "+v"(px), "+v"(py), "+v"(pz), "+v"(pw));
    f32x4 r;
    r.x = v.x + px; r.y = v.y + py; r.z = v.z + pz; r.w = v.w + pw;
    return r;
}

// load 4 consecutive floats that may be unaligned / partially out of range [0, lim)
__device__ __forceinline__ f32x4 ld4_guard(const float* base, int idx, int lim, bool aligned) {
    f32x4 r = zero4();
    if (aligned && idx + 3 < lim) return ld4(base + idx);
    if (idx < lim) r.x = base[idx];
    if (idx + 1 < lim) r.y = base[idx + 1];
    if (idx + 2 < lim) r.z = base[idx + 2];
    if (idx + 3 < lim) r.w = base[idx + 3];
    return r;
}

// ---------------------------------------------------------------------------- BN2-backward operand
// From dZ (gradient w.r.t. the gated activation that feeds the project conv) to dd (gradient w.r.t. the raw depthwise
// output D), i.e. the backward of  D -> BN2 -> act -> (* gate, SE pool path):
//   dhat = (D - mean2) * rstd2 ; da = dZ*gate + dpooled/HW  (SE groups; else dZ) ; ddh = da * act'(dhat)
//   dd   = rstd2 * (ddh - R1/Po - dhat * R2/Po)            R1 = sum ddh, R2 = sum ddh*dhat  (k_bn2_bwd)
// cst2[c] = (mean2, rstd2, R1/Po, R2/Po).  ddh is recomputed here instead of being written back by k_bn2_bwd
// (saves one write + nothing extra to read: dZ replaces ddh).
template <int ACT>
__device__ __forceinline__ f32x4 bn2_dd(const f32x4* cst2, int cl, f32x4 dz, f32x4 dv, bool has_se, f32x4 gate4,
                                        f32x4 dpool4) {
    f32x4 r;
    if (has_se) dz = dz * gate4 + dpool4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 t = cst2[cl + j];
        const float dh = (dv[j] - t.x) * t.y;
        const float ddh = dz[j] * act_d<ACT>(dh);
        r[j] = t.y * (ddh - t.z - dh * t.w);
    }
    return r;
}
__device__ __forceinline__ void fill_cst2(f32x4* cst2, const TfnasCellDesc& d, int CC, int c0, int mc, int off,
                                          const double* stats2, const double* red2) {
    const int tid = threadIdx.x;
    if (tid < CC) {
        f32x4 t = zero4();
        if (c0 + tid < mc) {
            const double inv = 1.0 / ((double)d.N * d.Ho * d.Wo);
            const float2 c = bn_consts(stats2 + 2 * (size_t)(off + c0 + tid), inv, d.eps);
            t.x = c.x;
            t.y = c.y;
            t.z = (float)(red2[2 * (size_t)(off + c0 + tid) + 0] * inv);
            t.w = (float)(red2[2 * (size_t)(off + c0 + tid) + 1] * inv);
        }
        cst2[tid] = t;
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// atomic accumulate into double / float device memory (ordinary coarse-grained allocations)
__device__ __forceinline__ void atomic_add_f64(double* p, double v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void atomic_add_f32(float* p, float v) { unsafeAtomicAdd(p, v); }
