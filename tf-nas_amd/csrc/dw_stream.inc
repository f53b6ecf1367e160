// ====================================================================================================================
// Row-streaming variants (stride 1).  A workgroup owns (channel chunk, image lane).  The images of a lane are stacked into
// ONE tall virtual image, separated by PAD rows of zeros (the bottom padding of one image doubles as the top padding of
// the next):   virtual row v = i * (H + PAD) + PAD + h   <->   row h of the lane's i-th image.
// The workgroup walks down that stream in blocks of TH rows through an LDS ring of RB = TH - 1 + K rows (slot = v mod RB):
//     issue the global loads of block s+1 (registers)  ->  compute the TH output rows of step s
//     ->  barrier  ->  transform + store block s+1 over the TH oldest rows  ->  barrier
// so every source row is fetched from HBM exactly once (the tile kernels above re-read the (K-1)-wide halo of every tile:
// 1.4x (k3) / 1.9x (k5) fetch inflation on 8x16 tiles; a band spans the whole image width, so there is no horizontal
// halo either) and the loads of the next block are in flight during the whole compute phase.  After block s the ring
// holds rows ((s+1)*TH - RB, (s+1)*TH - 1], i.e. exactly the windows of the output rows [s*TH - PAD, (s+1)*TH - PAD).
// Output rows that fall on separator rows are skipped.
//
// These kernels are instruction-issue bound before they are bandwidth bound (one step is only TH*W*CC outputs), so the
// per-step code is kept lean: every thread stages the same (row-in-block, column, channel quad) elements in every block
// and computes the same (row-in-step, strip, channel quad) item in every step; the position of the block / step in the
// stream is wave-uniform (scalar registers) and a thread only adds its constant row offset; global addresses are 32-bit
// element offsets from a uniform base (tensors here are < 2^30 elements; checked on the host); accesses are buffer
// instructions whose hardware range check replaces the branches around out-of-image loads.
// Geometry: DwSlide (kernels.h).

// LDS ring, pixel swizzle.  A pixel is CC = 32 floats = HALF of the 64-bank row, and the strips of the 16 lanes that one
// ds_read_b128 lane group serves are 4 pixels apart: with pixels in natural order all four strips of a group start on the same
// bank half and every window read is a 2-way conflict (SQ_LDS_BANK_CONFLICT 31-41 % of the LDS cycles in rounds 1-3; padding the
// pixel stride cures it but costs a ring row of the 56-wide images).  Ring column c is stored at c ^ ((c >> 2) & 1): odd strips
// keep their pixel pairs swapped, so neighbouring strips sit on opposite bank halves and the four (strip, channel-half)
// quarters of a lane group cover all 64 banks.  A reader of strip s = ow0 / 4 finds window element u at u ^ ((s + (u >> 2)) & 1).
__device__ __forceinline__ int ring_swz(int c) { return c ^ ((c >> 2) & 1); }
// per-lane base pointers of the window reads: element u of the window is at base[(u >> 2) & 1][u & 1] + u * CCP
struct WinBase {
    const float* b[2][2];
    __device__ __forceinline__ void set(const float* rowp, int d0, int d1) {
        b[0][0] = rowp + d0; b[0][1] = rowp - d0; b[1][0] = rowp + d1; b[1][1] = rowp - d1;
    }
    __device__ __forceinline__ const float* at(int u) const { return b[(u >> 2) & 1][u & 1]; }
};

// 1-D grid -> (chunk, lane).  Workgroup L runs on XCD L % 8; consecutive slots of one XCD take consecutive channel
// chunks of the SAME lane (= same images), so neighbouring chunks of a pixel go through one L2.
__device__ __forceinline__ void dws_decode(const DwSlide& gm, int& cy, int& lane) {
    const int L = blockIdx.x;
    if (gm.gx & 7) {
        cy = L % gm.chunks;
        lane = L / gm.chunks;
    } else {
        const int x = L & 7, q = L >> 3;
        cy = q % gm.chunks;
        lane = (q / gm.chunks) * 8 + x;
    }
}

// Buffer-addressed view of an fp32 tensor (< 4 GiB): uniform resource descriptor + one 32-bit element offset per lane;
// offsets at or beyond `numel` read zeros / drop the store (hardware range check), so no branch guards the access.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// aux = 2: the `nt` (non-temporal) bit of the gfx940+ buffer instructions.  The [pixels][M] tensors are 0.2-3.7 GB streams
// that are read / written exactly once per kernel: keeping them out of the L2 replacement order is worth -10..-20 % on the
// 56x56 / 28x28 launches (and a few % on the smaller ones).
#ifndef TFNAS_LD_AUX
#define TFNAS_LD_AUX 2
#endif
#ifndef TFNAS_ST_AUX
#define TFNAS_ST_AUX 2
#endif
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
struct BufView {
    __amdgpu_buffer_rsrc_t r;
    __device__ __forceinline__ void bind(const float* p, size_t numel) {
        r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)(unsigned)(numel * 4), 0x00020000);
    }
    __device__ __forceinline__ f32x4 ld4(unsigned off) const {
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(off * 4u), 0, TFNAS_LD_AUX));
    }
    __device__ __forceinline__ void st4(unsigned off, f32x4 v) const {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)(off * 4u), 0, TFNAS_ST_AUX);
    }
};
constexpr unsigned BUF_OOB = 0x3fffffffu;      // element offset that is out of range for every tensor (numel < 2^30)

// Wave-uniform position in the stream: image i, row h in [-PAD, H) (h < 0 = separator row), ring slot.
struct StreamPos {
    int i, h, slot;
    __device__ __forceinline__ void advance(int TH, int H, int PAD, int RB) {
        h += TH;
        if (h >= H) {
            h -= H + PAD;
            ++i;
        }
        slot += TH;
        if (slot >= RB) slot -= RB;
    }
};

// geometry shared by the loaders / items of one workgroup (all uniform)
struct StreamGeo {
    int H, PAD, RB, TH, nimg;
    unsigned WM;           // elements per image row
    unsigned img_stride;   // elements between consecutive images of the lane: gx * H * W * M
    unsigned lane_base;    // element offset of (image `lane`, row 0, col 0, first channel of the chunk)
    int row_floats;        // LDS floats per ring row
    // row offset `r` (0 <= r < TH <= H + PAD) below `p`: image / row / validity of that row
    __device__ __forceinline__ void locate(const StreamPos& p, int r, int& ii, int& hh) const {
        const int h = p.h + r;
        const bool wrap = h >= H;
        hh = wrap ? h - (H + PAD) : h;
        ii = wrap ? p.i + 1 : p.i;
    }
    __device__ __forceinline__ unsigned row_off(int ii, int hh) const {
        return lane_base + (unsigned)ii * img_stride + (unsigned)hh * WM;
    }
    __device__ __forceinline__ int slot_of(const StreamPos& p, int r) const {
        const int s = p.slot + r;
        return s >= RB ? s - RB : s;
    }
};

// One block (TH virtual rows x L1 columns x CC channels) of the stream, staged through registers (<= 4 float4 per thread
// and source).  Element u of a thread = float4 number u*256 + tid of the block in (row, column, channel quad) order.
template <bool TWO>
struct RingBlock {
    f32x4 v0[4], v1[TWO ? 4 : 1];
    int rr[4];               // row within the block
    unsigned goff[4];        // col * M + 4*cq
    int loff[4];             // (col + PAD) * CCP + 4*cq, or -1: no element
    unsigned okmask;         // bit u: element u of the block in flight is inside an image
    unsigned colmask;        // bit u: column / channel of element u exist
    int img[4];              // image index of the element in flight (for per-image operands of the transform)

    __device__ __forceinline__ void init(const DwSlide& gm, int Ws, int M, int nch, int PAD) {
        const int CQ = gm.CC >> 2, L1 = gm.L1, total = gm.TH * L1 * CQ;
        colmask = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = u * 256 + threadIdx.x;
            const int pix = idx >> gm.cq_shift, cq = idx & (CQ - 1);
            const int r = pix / L1, c = pix - r * L1, col = c - PAD;
            rr[u] = r;
            if (idx < total && col >= 0 && col < Ws && 4 * cq < nch) colmask |= 1u << u;
            goff[u] = (unsigned)(col * M + 4 * cq);
            loff[u] = idx < total ? ring_swz(c) * gm.CCP + 4 * cq : -1;
        }
    }
    // issue the loads of the block at `p`
    __device__ __forceinline__ void issue(const StreamGeo& ge, const StreamPos& p, const BufView& src0,
                                          const BufView& src1) {
        okmask = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int ii, hh;
            ge.locate(p, rr[u], ii, hh);
            const bool k = ((colmask >> u) & 1u) && hh >= 0 && ii < ge.nimg;
            if (k) okmask |= 1u << u;
            img[u] = ii;
            const unsigned a = k ? ge.row_off(ii, hh) + goff[u] : BUF_OOB;
            v0[u] = src0.ld4(a);
            if (TWO) v1[u] = src1.ld4(a);
        }
    }
    // transform and store the block at `p` into the ring; xf(v0, v1, image index) for in-image elements, zeros otherwise
    template <class FXf>
    __device__ __forceinline__ void commit(float* ring, const StreamGeo& ge, const StreamPos& p, FXf xf) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (loff[u] >= 0) {
                f32x4 t = zero4();
                if ((okmask >> u) & 1u) t = xf(v0[u], v1[TWO ? u : 0], img[u]);   // (xf may load per-image operands)
                st4(ring + ge.slot_of(p, rr[u]) * ge.row_floats + loff[u], t);
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------- forward (S = 1)
// KQ > 0 (E-free, efree.h): the block of a1 rows is recomputed from x into the ring (MFMA, the expand GEMM's contraction in
// the order of expand_tile) instead of being loaded from E -- E is neither written nor read for this cell.
template <int K, int ACT, bool PIPE, int KQ = 0>
__global__ __launch_bounds__(256, PIPE ? 3 : 4) void k_dws_fwd(TfnasCellDesc d, const float* __restrict__ E,
                                                    const double* __restrict__ stats1, float* __restrict__ D,
                                                    float* __restrict__ part, DwSlide gm,
                                                    const float* __restrict__ x = nullptr) {
    static_assert(!(PIPE && KQ > 0), "the E-free loader has no register-prefetch form");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int cy, lane, g, c0;
    dws_decode(gm, cy, lane);
    if (!dw_locate<K>(d, cy, gm.CC, g, c0)) return;
    const int mc = d.g[g].mc, mcp = d.g[g].mcp, off = d.g[g].off;
    constexpr int CC = 32, CCP = 32, CQ = CC >> 2;                // (= gm.CC, gm.CCP: pick_slide; compile-time -> immediate LDS offsets)
    const int TH = gm.TH, L1 = gm.L1, RB = gm.RB;
    const int H = d.H, W = d.W, M = d.M;
    constexpr int PAD = K / 2;
    const int tid = threadIdx.x;

    float* ring = lds;
    float* wts = lds + RB * L1 * CCP;
    float2* cst = reinterpret_cast<float2*>(wts + K * K * CC);
    if (tid < CC)
        cst[tid] = (c0 + tid < mc) ? bn_consts(stats1 + 2 * (size_t)(off + c0 + tid), 1.0 / ((double)d.N * H * W), d.eps)
                                   : make_float2(0.f, 0.f);
    stage_weights(wts, d.g[g].w_dw, K * K, CC, c0, mc);
    __syncthreads();
    ExpandB<(KQ > 0 ? KQ : 2)> xb;
    if (KQ > 0) expand_b_load(xb, d.g[g].w_expand, d.ic, c0, mc, cst);

    StreamGeo ge;
    ge.H = H; ge.PAD = PAD; ge.RB = RB; ge.TH = TH;
    ge.nimg = (d.N - lane + gm.gx - 1) / gm.gx;                   // images of this lane: lane, lane + gx, ...
    ge.WM = (unsigned)W * M;
    ge.img_stride = (unsigned)gm.gx * H * ge.WM;
    ge.lane_base = (unsigned)lane * H * ge.WM + off + c0;
    ge.row_floats = L1 * CCP;
    const int nsteps = (ge.nimg * (H + PAD) + PAD + TH - 1) / TH; // outputs up to virtual row nimg*(H+PAD) - 1

    // this thread's channel quad (the same for its loads and its item: 256 % CQ == 0): BN constants in registers
    const int cq = tid & (CQ - 1);
    float2 bc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bc[j] = cst[4 * cq + j];
    auto xf = [&](f32x4 v, f32x4, int) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = act_f<ACT>((v[j] - bc[j].x) * bc[j].y);
        return v;
    };
    RingBlock<false> rb;
    rb.init(gm, W, M, mcp - c0, PAD);
    StreamPos bpos = {0, -PAD, 0};                                // block 0 starts at virtual row 0
    BufView bE, bD;
    bE.bind(E, (size_t)d.N * H * W * M);
    bD.bind(D, (size_t)d.N * H * W * M);
    if (PIPE) {
        rb.issue(ge, bpos, bE, bE);
        rb.commit(ring, ge, bpos, xf);
        bpos.advance(TH, H, PAD, RB);
        __syncthreads();
    }

    // this thread's item of every step: output row (s*TH - PAD + oh), strip ow0..ow0+3, channel quad cq
    const int nsw = gm.TW >> 2, st = tid >> gm.cq_shift;
    const int oh = st / nsw, ow0 = (st - oh * nsw) * 4;
    const bool item_ok = oh < TH && c0 + 4 * cq < mcp;
    const int npx = W - ow0 < 4 ? W - ow0 : 4;                    // valid pixels of the strip
    const float* ring_item = ring + ow0 * CCP + 4 * cq;
    const int swz0 = ((ow0 >> 2) & 1) * CCP, swz1 = CCP - swz0;   // (ring_swz: this strip's pixel-pair swaps, window pixels 0-3 / 4-7)
    const float* wts_item = wts + 4 * cq;
    const unsigned ooff = (unsigned)(ow0 * M + 4 * cq);
    constexpr bool REGW = (K == 3) && PIPE;                      // 3x3 taps in registers only where 160 VGPRs are allowed
    f32x4 wreg[REGW ? 9 : 1];
    if (REGW) {
#pragma unroll
        for (int t = 0; t < 9; ++t) wreg[t] = ld4(wts_item + t * CC);
    }
    // step 0 produces the virtual rows [-PAD, TH - PAD): one image period before image 0's row (H - PAD)
    StreamPos spos = {-1, H - PAD, RB - 2 * PAD};                 // slot of the first window row: (vo - PAD) mod RB

    f32x4 ssum = zero4(), ssq = zero4();
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (PIPE) {
            if (more) rb.issue(ge, bpos, bE, bE);
        } else if (KQ > 0) {
            const float inv_l1 = 1.f / (float)L1;
            expand_tile_to<(KQ > 0 ? KQ : 2), ACT>(
                TH * L1, x, xb,
                [&](int p, size_t& a) {
                    const int r = (int)(((float)p + 0.5f) * inv_l1), col = p - r * L1 - PAD;
                    int bi, bh;
                    ge.locate(bpos, r, bi, bh);
                    a = (((size_t)(lane + bi * gm.gx) * H + bh) * W + col) * d.ic;
                    return col >= 0 && col < W && bh >= 0 && bi < ge.nimg;
                },
                [&](int p) {
                    const int r = (int)(((float)p + 0.5f) * inv_l1), c = p - r * L1;
                    return ring + ge.slot_of(bpos, r) * ge.row_floats + ring_swz(c) * CCP;
                });
            bpos.advance(TH, H, PAD, RB);
            __syncthreads();
        } else {
            rb.issue(ge, bpos, bE, bE);                           // block s
            rb.commit(ring, ge, bpos, xf);
            bpos.advance(TH, H, PAD, RB);
            __syncthreads();
        }
        int ii, hh;
        ge.locate(spos, oh, ii, hh);
        if (item_ok && hh >= 0 && ii >= 0 && ii < ge.nimg) {
            int slot = ge.slot_of(spos, oh);
            f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
            if (REGW) {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const float* rowp = ring_item + slot * ge.row_floats;
                    WinBase wb;
                    wb.set(rowp, swz0, swz1);
                    f32x4 win[6];
#pragma unroll
                    for (int u = 0; u < 6; ++u) win[u] = ld4(wb.at(u) + u * CCP);
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j] += win[j + kx] * wreg[ky * 3 + kx];
                    slot = (slot + 1 == RB) ? 0 : slot + 1;
                }
            } else {
#pragma unroll 1
                for (int ky = 0; ky < K; ++ky) {
                    const float* rowp = ring_item + slot * ge.row_floats;
                    WinBase wb;
                    wb.set(rowp, swz0, swz1);
                    const float* wp = wts_item + ky * K * CC;
                    f32x4 win[K + 3];
#pragma unroll
                    for (int u = 0; u < K + 3; ++u) win[u] = ld4(wb.at(u) + u * CCP);
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        const f32x4 wv = ld4(wp + kx * CC);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j] += win[j + kx] * wv;
                    }
                    slot = (slot + 1 == RB) ? 0 : slot + 1;
                }
            }
            const unsigned o = ge.row_off(ii, hh) + ooff;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < npx) {
                    bD.st4(o + (unsigned)(j * M), acc[j]);
                    ssum += acc[j];
                    ssq += acc[j] * acc[j];
                }
            }
        }
        spos.advance(TH, H, PAD, RB);
        __syncthreads();                                          // the TH oldest rows are no longer read
        if (PIPE) {
            if (more) {
                rb.commit(ring, ge, bpos, xf);
                bpos.advance(TH, H, PAD, RB);
            }
            __syncthreads();
        }
    }
    dw_flush_stats(ssum, ssq, ring, CC, c0, mcp, off, M, part, lane);
}

// ---------------------------------------------------------------------------------------------------- backward data (S = 1)
// dA1[hi][wi] = sum_{ky,kx} dd[hi+p-ky][wi+p-kx] w[ky][kx]: for stride 1 this is the forward stencil on the dd stream with
// the taps flipped in both directions, so the weights are staged flipped and the tap loop is the forward one.  dd (the
// BN2-backward of dZ, see bn2_dd) is formed when a block of (dZ, D) rows is committed to the ring; the epilogue multiplies
// by act'(ehat) (E centre element, loaded at the start of the step), stores dEh and accumulates the BN1-backward sums.
// PIPE = true: the (dZ, D) loads of block s+1 stay in registers across the compute phase of step s (3 waves/SIMD: the
// choice for 56-wide images, whose 46 KB ring allows three workgroups per CU anyway).  PIPE = false: block s is loaded
// and committed at the start of step s; without the prefetch registers the kernel fits 128 VGPRs, and the fourth wave
// per SIMD hides the load latency better than the prefetch did on the narrower images (-7..-15 % at 28x28 / 14x14).
// KQ > 0 (E-free): ehat of the step's output rows is recomputed from x into a second LDS tile (expand_tile_to, OUT = 2) instead
// of being loaded from E.
// WGR (round 4): the depthwise WEIGHT gradient from the same pass.  The ring holds dd with its halo and the item has a1 = act(ehat)
// of its own pixels, so  g_dw[K-1-r][K-1-c] += a1[hi][wi] * dd[hi-p+r][wi-p+c]  uses exactly the window values of the data
// gradient (weights are staged flipped, so window slot (r, c) belongs to tap (K-1-r, K-1-c)): K*K more float4 accumulators per
// thread, no extra memory traffic -- the separate weight-gradient kernel re-read E, dZ and D (3 of the 18 tensor passes of a
// sampled stride-1 cell; the w-step is bandwidth-bound in aggregate, DESIGN.md section 4c).  Partial rows wpart[lane][wout_size]
// like k_dws_wgrad's.
template <int K, int ACT, bool PIPE, int KQ = 0, bool WGR = false>
__global__ __launch_bounds__(256, WGR ? 2 : ((PIPE || KQ > 0) ? 3 : 4)) void k_dws_bwd(TfnasCellDesc d, const float* __restrict__ dZ,
                                                    const float* __restrict__ gate, const float* __restrict__ dpooled,
                                                    const float* __restrict__ D, const double* __restrict__ stats2,
                                                    const double* __restrict__ red2, const float* __restrict__ E,
                                                    const double* __restrict__ stats1, float* __restrict__ dEh,
                                                    float* __restrict__ part, DwSlide gm,
                                                    const float* __restrict__ x = nullptr,
                                                    float* __restrict__ wpart = nullptr, size_t wout_size = 0) {
    static_assert(!(PIPE && KQ > 0), "the E-free variant has no register-prefetch form");
    static_assert(!(WGR && KQ > 0), "the fused weight gradient needs a materialised E");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int cy, lane, g, c0;
    dws_decode(gm, cy, lane);
    if (!dw_locate<K>(d, cy, gm.CC, g, c0)) return;
    const int mc = d.g[g].mc, mcp = d.g[g].mcp, off = d.g[g].off;
    constexpr int CC = 32, CCP = 32, CQ = CC >> 2;                // (= gm.CC, gm.CCP: pick_slide; compile-time -> immediate LDS offsets)
    const int TH = gm.TH, L1 = gm.L1, RB = gm.RB;
    const int H = d.H, W = d.W, M = d.M;          // stride 1: dd and E / dEh have the same extent
    constexpr int PAD = K / 2;
    const int tid = threadIdx.x;

    float* ring = lds;
    float* wts = lds + RB * L1 * CCP;
    f32x4* cst2 = reinterpret_cast<f32x4*>(wts + K * K * CC);
    float2* cst1 = reinterpret_cast<float2*>(cst2 + CC);
    float* eht = reinterpret_cast<float*>(cst1 + CC);             // KQ > 0: [TH][TW][CCP] normalised E of the step's output rows
    fill_cst2(cst2, d, CC, c0, mc, off, stats2, red2);
    if (tid < CC)
        cst1[tid] = (c0 + tid < mc) ? bn_consts(stats1 + 2 * (size_t)(off + c0 + tid), 1.0 / ((double)d.N * H * W), d.eps)
                                    : make_float2(0.f, 0.f);
    for (int idx = tid; idx < K * K * CC; idx += 256) {           // flipped taps: wts[t][c] = w[c][K*K-1-t]
        const int cl = idx % CC, t = idx / CC;
        wts[t * CC + cl] = (c0 + cl < mc) ? d.g[g].w_dw[(size_t)(c0 + cl) * (K * K) + (K * K - 1 - t)] : 0.f;
    }
    __syncthreads();
    ExpandB<(KQ > 0 ? KQ : 2)> xb;
    if (KQ > 0) expand_b_load(xb, d.g[g].w_expand, d.ic, c0, mc, cst1);

    StreamGeo ge;
    ge.H = H; ge.PAD = PAD; ge.RB = RB; ge.TH = TH;
    ge.nimg = (d.N - lane + gm.gx - 1) / gm.gx;
    ge.WM = (unsigned)W * M;
    ge.img_stride = (unsigned)gm.gx * H * ge.WM;
    ge.lane_base = (unsigned)lane * H * ge.WM + off + c0;
    ge.row_floats = L1 * CCP;
    const int nsteps = (ge.nimg * (H + PAD) + PAD + TH - 1) / TH;

    const int cq = tid & (CQ - 1);
    const bool has_se = d.g[g].se > 0;
    const float inv_hw = 1.f / (float)(H * W);
    f32x4 c2r[4];
    float2 c1r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c2r[j] = cst2[4 * cq + j];
        c1r[j] = cst1[4 * cq + j];
    }
    const float* gate_c = gate + off + c0 + 4 * cq;               // + image * M
    const float* dpool_c = dpooled + off + c0 + 4 * cq;
    auto xf = [&](f32x4 dz, f32x4 dv, int i) {
        f32x4 g4 = zero4(), dp4 = zero4();
        if (has_se) {
            const size_t n = (size_t)(lane + i * gm.gx) * M;
            g4 = ld4(gate_c + n);
            dp4 = ld4(dpool_c + n) * splat4(inv_hw);
        }
        return bn2_dd<ACT>(c2r, 0, dz, dv, has_se, g4, dp4);
    };
    const size_t numel = (size_t)d.N * H * W * M;
    BufView bZ, bDd, bE, bO;
    bZ.bind(dZ, numel);
    bDd.bind(D, numel);
    bE.bind(E, numel);
    bO.bind(dEh, numel);
    RingBlock<true> rb;
    rb.init(gm, W, M, mcp - c0, PAD);
    StreamPos bpos = {0, -PAD, 0};
    if (PIPE) {
        rb.issue(ge, bpos, bZ, bDd);
        rb.commit(ring, ge, bpos, xf);
        bpos.advance(TH, H, PAD, RB);
        __syncthreads();
    }

    const int nsw = gm.TW >> 2, st = tid >> gm.cq_shift;
    const int oh = st / nsw, ow0 = (st - oh * nsw) * 4;
    const bool item_ok = oh < TH && c0 + 4 * cq < mcp;
    const int npx = W - ow0 < 4 ? W - ow0 : 4;
    const float* ring_item = ring + ow0 * CCP + 4 * cq;
    const int swz0 = ((ow0 >> 2) & 1) * CCP, swz1 = CCP - swz0;   // (ring_swz: this strip's pixel-pair swaps, window pixels 0-3 / 4-7)
    const float* wts_item = wts + 4 * cq;
    const unsigned ooff = (unsigned)(ow0 * M + 4 * cq);
    StreamPos spos = {-1, H - PAD, RB - 2 * PAD};

    f32x4 t1 = zero4(), t2 = zero4();
    f32x4 wacc[WGR ? K * K : 1];
#pragma unroll
    for (int u = 0; u < (WGR ? K * K : 1); ++u) wacc[u] = zero4();
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (PIPE) {
            if (more) rb.issue(ge, bpos, bZ, bDd);
        } else {
            rb.issue(ge, bpos, bZ, bDd);               // block s
            if (KQ > 0) {                              // (x comes from L2: the MFMAs run while the dZ / D block is in flight)
                const int TW = gm.TW;
                const float inv_tw = 1.f / (float)TW;
                expand_tile_to<(KQ > 0 ? KQ : 2), 2>(
                    TH * TW, x, xb,
                    [&](int p, size_t& a) {
                        const int r = (int)(((float)p + 0.5f) * inv_tw), col = p - r * TW;
                        int bi, bh;
                        ge.locate(spos, r, bi, bh);
                        a = (((size_t)(lane + bi * gm.gx) * H + bh) * W + col) * d.ic;
                        return col < W && bh >= 0 && bi >= 0 && bi < ge.nimg;
                    },
                    [&](int p) { return eht + p * CCP; });
            }
            rb.commit(ring, ge, bpos, xf);
            bpos.advance(TH, H, PAD, RB);
            __syncthreads();
        }
        int ii, hh;
        ge.locate(spos, oh, ii, hh);
        if (item_ok && hh >= 0 && ii >= 0 && ii < ge.nimg) {
            const unsigned o = ge.row_off(ii, hh) + ooff;
            f32x4 ev[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (KQ > 0) ev[j] = ld4(eht + (oh * gm.TW + ow0 + j) * CCP + 4 * cq);      // already (E - mean) * rstd
                else ev[j] = bE.ld4(j < npx ? o + (unsigned)(j * M) : BUF_OOB);
            }
            int slot = ge.slot_of(spos, oh);
            f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
            if (!WGR) {
#pragma unroll 1
                for (int ky = 0; ky < K; ++ky) {
                    const float* rowp = ring_item + slot * ge.row_floats;
                    WinBase wb;
                    wb.set(rowp, swz0, swz1);
                    const float* wp = wts_item + ky * K * CC;
                    f32x4 win[K + 3];
#pragma unroll
                    for (int u = 0; u < K + 3; ++u) win[u] = ld4(wb.at(u) + u * CCP);
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        const f32x4 wv = ld4(wp + kx * CC);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j] += win[j + kx] * wv;
                    }
                    slot = (slot + 1 == RB) ? 0 : slot + 1;
                }
            } else {
                f32x4 a1v[4];                                     // act(ehat) of the item's pixels (0 outside the image)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        a1v[j][q] = j < npx ? act_f<ACT>((ev[j][q] - c1r[q].x) * c1r[q].y) : 0.f;
#pragma unroll
                for (int ky = 0; ky < K; ++ky) {                  // (unrolled: the accumulator index must be static)
                    const float* rowp = ring_item + slot * ge.row_floats;
                    WinBase wb;
                    wb.set(rowp, swz0, swz1);
                    const float* wp = wts_item + ky * K * CC;
                    f32x4 win[K + 3];
#pragma unroll
                    for (int u = 0; u < K + 3; ++u) win[u] = ld4(wb.at(u) + u * CCP);
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        const f32x4 wv = ld4(wp + kx * CC);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            acc[j] += win[j + kx] * wv;
                            wacc[(K - 1 - ky) * K + (K - 1 - kx)] += a1v[j] * win[j + kx];
                        }
                    }
                    slot = (slot + 1 == RB) ? 0 : slot + 1;
                    __builtin_amdgcn_sched_barrier(0);            // (one tap row at a time: without it the three rows' windows
                }                                                 //  are all loaded up front -- 250 registers + scratch)
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < npx) {
                    f32x4 deh;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float eh = KQ > 0 ? ev[j][q] : (ev[j][q] - c1r[q].x) * c1r[q].y;
                        deh[q] = acc[j][q] * act_d<ACT>(eh);
                        t1[q] += deh[q];
                        t2[q] += deh[q] * eh;
                    }
                    bO.st4(o + (unsigned)(j * M), deh);
                }
            }
        }
        spos.advance(TH, H, PAD, RB);
        __syncthreads();
        if (PIPE) {
            if (more) {
                rb.commit(ring, ge, bpos, xf);
                bpos.advance(TH, H, PAD, RB);
            }
            __syncthreads();
        }
    }
    dw_flush_stats(t1, t2, ring, CC, c0, mcp, off, M, part, lane);
    if (WGR) {
        // (as k_dws_wgrad) reduce over the threads sharing a channel quad: inside the wave, then across the 4 waves through the ring
        for (int o = CQ; o < 64; o <<= 1) {
#pragma unroll
            for (int u = 0; u < K * K; ++u) {
#pragma unroll
                for (int q = 0; q < 4; ++q) wacc[u][q] += __shfl_xor(wacc[u][q], o, 64);
            }
        }
        __syncthreads();
        float* wred = ring;   // [4 waves][K*K][CC]  (the host sizes the ring for it)
        const int wl = tid & 63, wv = tid >> 6;
        if (wl < CQ) {
#pragma unroll
            for (int u = 0; u < K * K; ++u) st4(wred + (wv * K * K + u) * CC + 4 * wl, wacc[u]);
        }
        __syncthreads();
        size_t poff = 0;
        for (int gg = 0; gg < g; ++gg) poff += (size_t)d.g[gg].mc * d.g[gg].k * d.g[gg].k;
        float* __restrict__ gw = wpart + (size_t)lane * wout_size + poff;
        for (int idx = tid; idx < K * K * CC; idx += 256) {
            const int cl = idx % CC, u = idx / CC;
            if (c0 + cl < mc) {
                float sum = 0.f;
#pragma unroll
                for (int ww = 0; ww < 4; ++ww) sum += wred[(ww * K * K + u) * CC + cl];
                gw[(size_t)(c0 + cl) * (K * K) + u] = sum;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- weight gradient (S = 1)
// g_dw[c][ky][kx] = sum_{n,h,w} dd[n][h][w][c] * a1[n][h+ky-p][w+kx-p][c],  a1 = act(BN1(E)) streamed through the ring (with
// its halo, read once), dd formed per item from the (dZ, D) centre elements.  Every thread keeps the K*K accumulators of
// its channel quad in registers over the whole stream; partial rows part[lane][out_size] are summed by k_reduce_rows.
template <int K, int ACT, bool PIPE>
__global__ __launch_bounds__(256, (!PIPE && K == 3) ? 4 : 2) void k_dws_wgrad(TfnasCellDesc d, const float* __restrict__ dZ,
                                                      const float* __restrict__ gate, const float* __restrict__ dpooled,
                                                      const float* __restrict__ D, const double* __restrict__ stats2,
                                                      const double* __restrict__ red2, const float* __restrict__ E,
                                                      const double* __restrict__ stats1, float* __restrict__ part,
                                                      size_t out_size, DwSlide gm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int cy, lane, g, c0;
    dws_decode(gm, cy, lane);
    if (!dw_locate<K>(d, cy, gm.CC, g, c0)) return;
    const int mc = d.g[g].mc, mcp = d.g[g].mcp, off = d.g[g].off;
    constexpr int CC = 32, CCP = 32, CQ = CC >> 2;                // (= gm.CC, gm.CCP: pick_slide; compile-time -> immediate LDS offsets)
    const int TH = gm.TH, L1 = gm.L1, RB = gm.RB;
    const int H = d.H, W = d.W, M = d.M;
    constexpr int PAD = K / 2;
    const int tid = threadIdx.x;

    float* ring = lds;
    f32x4* cst2 = reinterpret_cast<f32x4*>(lds + RB * L1 * CCP);
    float2* cst1 = reinterpret_cast<float2*>(cst2 + CC);
    fill_cst2(cst2, d, CC, c0, mc, off, stats2, red2);
    if (tid < CC)
        cst1[tid] = (c0 + tid < mc) ? bn_consts(stats1 + 2 * (size_t)(off + c0 + tid), 1.0 / ((double)d.N * H * W), d.eps)
                                    : make_float2(0.f, 0.f);
    __syncthreads();

    StreamGeo ge;
    ge.H = H; ge.PAD = PAD; ge.RB = RB; ge.TH = TH;
    ge.nimg = (d.N - lane + gm.gx - 1) / gm.gx;
    ge.WM = (unsigned)W * M;
    ge.img_stride = (unsigned)gm.gx * H * ge.WM;
    ge.lane_base = (unsigned)lane * H * ge.WM + off + c0;
    ge.row_floats = L1 * CCP;
    const int nsteps = (ge.nimg * (H + PAD) + PAD + TH - 1) / TH;

    const int cq = tid & (CQ - 1);
    const bool has_se = d.g[g].se > 0;
    const float inv_hw = 1.f / (float)(H * W);
    f32x4 c2r[4];
    float2 c1r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c2r[j] = cst2[4 * cq + j];
        c1r[j] = cst1[4 * cq + j];
    }
    auto xf = [&](f32x4 v, f32x4, int) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = act_f<ACT>((v[j] - c1r[j].x) * c1r[j].y);
        return v;
    };
    const size_t numel = (size_t)d.N * H * W * M;
    BufView bZ, bDd, bE;
    bZ.bind(dZ, numel);
    bDd.bind(D, numel);
    bE.bind(E, numel);
    RingBlock<false> rb;
    rb.init(gm, W, M, mcp - c0, PAD);
    StreamPos bpos = {0, -PAD, 0};
    if (PIPE) {
        rb.issue(ge, bpos, bE, bE);
        rb.commit(ring, ge, bpos, xf);
        bpos.advance(TH, H, PAD, RB);
        __syncthreads();
    }

    const int nsw = gm.TW >> 2, st = tid >> gm.cq_shift;
    const int oh = st / nsw, ow0 = (st - oh * nsw) * 4;
    const bool item_ok = oh < TH && c0 + 4 * cq < mcp;
    const int npx = W - ow0 < 4 ? W - ow0 : 4;
    const float* ring_item = ring + ow0 * CCP + 4 * cq;
    const int swz0 = ((ow0 >> 2) & 1) * CCP, swz1 = CCP - swz0;   // (ring_swz: this strip's pixel-pair swaps, window pixels 0-3 / 4-7)
    const unsigned ooff = (unsigned)(ow0 * M + 4 * cq);
    const float* gate_c = gate + off + c0 + 4 * cq;
    const float* dpool_c = dpooled + off + c0 + 4 * cq;
    StreamPos spos = {-1, H - PAD, RB - 2 * PAD};

    f32x4 wacc[K * K];
#pragma unroll
    for (int u = 0; u < K * K; ++u) wacc[u] = zero4();
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (PIPE) {
            if (more) rb.issue(ge, bpos, bE, bE);
        } else {
            rb.issue(ge, bpos, bE, bE);                           // block s
            rb.commit(ring, ge, bpos, xf);
            bpos.advance(TH, H, PAD, RB);
            __syncthreads();
        }
        int ii, hh;
        ge.locate(spos, oh, ii, hh);
        if (item_ok && hh >= 0 && ii >= 0 && ii < ge.nimg) {
            const unsigned o = ge.row_off(ii, hh) + ooff;
            f32x4 dd[4], dv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned a = j < npx ? o + (unsigned)(j * M) : BUF_OOB;
                dd[j] = bZ.ld4(a);
                dv[j] = bDd.ld4(a);
            }
            f32x4 g4 = zero4(), dp4 = zero4();
            if (has_se) {
                const size_t n = (size_t)(lane + ii * gm.gx) * M;
                g4 = ld4(gate_c + n);
                dp4 = ld4(dpool_c + n) * splat4(inv_hw);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) dd[j] = j < npx ? bn2_dd<ACT>(c2r, 0, dd[j], dv[j], has_se, g4, dp4) : zero4();
            int slot = ge.slot_of(spos, oh);
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const float* rowp = ring_item + slot * ge.row_floats;
                WinBase wb;
                wb.set(rowp, swz0, swz1);
                f32x4 win[K + 3];
#pragma unroll
                for (int u = 0; u < K + 3; ++u) win[u] = ld4(wb.at(u) + u * CCP);
#pragma unroll
                for (int kx = 0; kx < K; ++kx)
#pragma unroll
                    for (int j = 0; j < 4; ++j) wacc[ky * K + kx] += dd[j] * win[j + kx];
                slot = (slot + 1 == RB) ? 0 : slot + 1;
            }
        }
        spos.advance(TH, H, PAD, RB);
        __syncthreads();
        if (PIPE) {
            if (more) {
                rb.commit(ring, ge, bpos, xf);
                bpos.advance(TH, H, PAD, RB);
            }
            __syncthreads();
        }
    }
    // reduce over the threads sharing a channel quad: first inside the wave, then across the 4 waves
    for (int o = CQ; o < 64; o <<= 1) {
#pragma unroll
        for (int u = 0; u < K * K; ++u) {
#pragma unroll
            for (int q = 0; q < 4; ++q) wacc[u][q] += __shfl_xor(wacc[u][q], o, 64);
        }
    }
    __syncthreads();
    float* wred = ring;   // [4 waves][K*K][CC]
    const int wl = tid & 63, wv = tid >> 6;
    if (wl < CQ) {
#pragma unroll
        for (int u = 0; u < K * K; ++u) st4(wred + (wv * K * K + u) * CC + 4 * wl, wacc[u]);
    }
    __syncthreads();
    size_t poff = 0;
    for (int gg = 0; gg < g; ++gg) poff += (size_t)d.g[gg].mc * d.g[gg].k * d.g[gg].k;
    float* __restrict__ gw = part + (size_t)lane * out_size + poff;
    for (int idx = tid; idx < K * K * CC; idx += 256) {
        const int cl = idx % CC, u = idx / CC;
        if (c0 + cl < mc) {
            float sum = 0.f;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) sum += wred[(ww * K * K + u) * CC + cl];
            gw[(size_t)(c0 + cl) * (K * K) + u] = sum;
        }
    }
}
