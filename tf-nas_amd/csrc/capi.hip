// extern "C" surface of libtfnas_hip.so (declared in include/tfnas_hip.h): descriptor planning, workspace
// sizing and the per-cell forward / backward launch sequences.
#include <string.h>
#include "tfnas_dev.h"
#include "kernels.h"
#include "cell_impl.h"

#include <stdlib.h>
#include <mutex>
#include <vector>

// ---------------------------------------------------------------------------------------------------------------
// Weight-gradient side stream.  The weight-gradient kernels of a cell are leaves of the backward dependency chain
// (nothing downstream in the same call consumes them), and like most kernels of the sampled w-step they are
// latency- rather than throughput-bound, so they are enqueued on a second HIP stream owned by the library
// (one per caller stream and device) and overlap with the data-gradient chain of the same cell: fork events
// after the producers of their operands, one join before tfnas_mixedop_bwd returns control to the caller's stream
// (so from the caller's point of view everything is still ordered on `stream`).  They use the second half of `part`.
// TFNAS_ROUTE_WGRAD_INLINE in the descriptor disables the side stream (everything on the caller's stream, identical results).
// TfnasCellDesc.wgrad_stream[k] != NULL: fork k goes to that caller-owned stream instead.
struct SideCtx {
    int device;
    hipStream_t main, side;
    hipEvent_t fork[4], join;
};
static std::mutex g_side_mu;
static std::vector<SideCtx*> g_side;

static SideCtx* side_for(hipStream_t s) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_side_mu);
    for (SideCtx* c : g_side)
        if (c->main == s && c->device == dev) return c;
    SideCtx* c = new SideCtx();
    c->device = dev;
    c->main = s;
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess) { delete c; return nullptr; }
    bool ok = hipEventCreateWithFlags(&c->join, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 4; ++i) ok = ok && hipEventCreateWithFlags(&c->fork[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) { delete c; return nullptr; }
    g_side.push_back(c);
    return c;
}
static int side_join(SideCtx* c, hipStream_t main) {
    if (!c) return 0;
    hipError_t e = hipEventRecord(c->join, c->side);
    if (e == hipSuccess) e = hipStreamWaitEvent(main, c->join, 0);
    return (int)e;
}

// Joins the side stream on every exit path of a cell backward (cell_bwd_entry): an early error return must not leave weight-gradient
// kernels running on buffers the caller is about to free.
struct SideJoinGuard {
    SideCtx* c = nullptr;
    hipStream_t main = nullptr;
    hipStream_t extra[3] = {nullptr, nullptr, nullptr};     // caller-owned weight-gradient streams of this launch (wgrad_stream[])
    bool joined = false;
    int join_extra() {
        int rc = 0;
        if (!c) return 0;
        for (int k = 0; k < 3; ++k) {
            hipStream_t x = extra[k];
            if (!x || x == main) continue;
            bool dup = false;
            for (int q = 0; q < k; ++q) dup = dup || extra[q] == x;
            if (dup) continue;
            // (the context's fork events are free again here: every fork's wait was enqueued long ago)
            hipError_t e = hipEventRecord(c->fork[3], x);
            if (e == hipSuccess) e = hipStreamWaitEvent(main, c->fork[3], 0);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(x);
                if (!rc) rc = (int)e;
            }
        }
        return rc;
    }
    int join() {
        joined = true;
        const int r0 = side_join(c, main), r1 = join_extra();
        return r0 ? r0 : r1;
    }
    ~SideJoinGuard() {
        if (!joined && c) {
            if (side_join(c, main) != 0) (void)hipStreamSynchronize(c->side);
            (void)join_extra();
        }
    }
};

// Lazy join (derived-network training step): tfnas_mbconv_bwd leaves its weight-gradient kernels running on the side stream
// when this is on; the caller keeps every buffer they read alive (torch: record_stream on the side stream's handle) and joins
// once before it consumes the gradients (tfnas_side_join).
static int g_lazy_join = 0;
extern "C" int tfnas_set_lazy_join(int on) {
    g_lazy_join = on ? 1 : 0;
    return 0;
}
extern "C" int tfnas_side_stream(void* stream, void** side) {
    if (!side) return TFNAS_ENULL;
    *side = nullptr;
    SideCtx* c = side_for(S(stream));
    if (c) *side = (void*)c->side;
    return 0;
}
extern "C" int tfnas_side_join(void* stream) {
    return side_join(side_for(S(stream)), S(stream));
}

extern "C" int tfnas_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_side_mu);
    for (SideCtx* c : g_side) {
        (void)hipStreamSynchronize(c->side);
        for (int i = 0; i < 4; ++i) (void)hipEventDestroy(c->fork[i]);
        (void)hipEventDestroy(c->join);
        (void)hipStreamDestroy(c->side);
        delete c;
    }
    g_side.clear();
    return 0;
}

StatsSync g_stats_sync = {nullptr, nullptr, 1};

extern "C" int tfnas_set_stats_sync(tfnas_stats_sync_fn fn, void* user, int world) {
    if (fn && world < 1) return TFNAS_ERANGE;
    g_stats_sync.fn = fn;
    g_stats_sync.user = user;
    g_stats_sync.world = fn ? world : 1;
    return 0;
}

extern "C" int tfnas_abi_version(void) { return TFNAS_ABI_VERSION; }
extern "C" int tfnas_set_gemm_mode(int mode) { return set_gemm_mode(mode); }
extern "C" int tfnas_gemm_mode(void) { return gemm_mode(); }

extern "C" uint64_t tfnas_sizeof(int which) {
    switch (which) {
        case 0: return sizeof(TfnasGroup);
        case 1: return sizeof(TfnasCellDesc);
        case 2: return sizeof(TfnasCellWs);
        case 3: return sizeof(TfnasStage);
        case 4: return sizeof(TfnasPathDesc);
        case 5: return sizeof(TfnasPathWs);
        case 6: return sizeof(TfnasBnAffine);
        case 7: return TFNAS_PART_ALLOC;      // floats of one `part` scratch region ...
        case 8: return TFNAS_TAIL_SLOTS;      // ... whose last this-many 4-byte words are reserved
        case 9: return sizeof(TfnasOptGroups);
        default: return 0;
    }
}

// the activation of a descriptor: ReLU / Swish; ReLU6 / hard-swish from a caller that set TFNAS_CELL_ACTS, never in a stem
static int check_act(const TfnasCellDesc* d) {
    if (d->act == TFNAS_ACT_RELU || d->act == TFNAS_ACT_SWISH) return 0;
    if (d->act != TFNAS_ACT_RELU6 && d->act != TFNAS_ACT_HSWISH) return TFNAS_EINVAL;
    if (!(d->flags & TFNAS_CELL_ACTS) || d->mode == TFNAS_MODE_STEM) return TFNAS_EINVAL;
    return 0;
}

// the squeeze-excite style of a descriptor (tfnas_hip.h: TFNAS_CELL_SE_STYLE): 0, or -- from a caller that set the bit, in cell mode
// -- a defined hidden activation (ReLU6 / hard-swish with TFNAS_CELL_ACTS, as in `act`) and a defined gate, nothing above bit 7
static int check_se_style(const TfnasCellDesc* d) {
    const int st = d->se_style;
    if (st == 0) return 0;
    if (!(d->flags & TFNAS_CELL_SE_STYLE) || d->mode != TFNAS_MODE_CELL) return TFNAS_EINVAL;
    if (st & ~(TFNAS_SE_HIDDEN_MASK | TFNAS_SE_GATE_MASK)) return TFNAS_EINVAL;
    const int hid = st & TFNAS_SE_HIDDEN_MASK, gate = st & TFNAS_SE_GATE_MASK;
    if (hid > TFNAS_SE_HIDDEN(TFNAS_ACT_HSWISH)) return TFNAS_EINVAL;
    if (gate != TFNAS_SE_GATE_LOGISTIC && gate != TFNAS_SE_GATE_HSIGMOID) return TFNAS_EINVAL;
    if ((hid == TFNAS_SE_HIDDEN(TFNAS_ACT_RELU6) || hid == TFNAS_SE_HIDDEN(TFNAS_ACT_HSWISH)) && !(d->flags & TFNAS_CELL_ACTS))
        return TFNAS_EINVAL;
    return 0;
}

// the kind bits of a descriptor.  Both newer kinds are ONE block in cell mode; TFNAS_CELL_NOEXPAND: mc == ic channels, no expand
// weight or gradient pointer; TFNAS_CELL_FUSED: a dense 3 x 3 weight (w_expand), no depthwise pointer; never both bits
// TFNAS_CELL_KINDS: the same rules per group (TfnasGroup.kind), any G; the two one-block bits must then be clear
// TFNAS_CELL_SKIP (with TFNAS_CELL_KINDS only): groups may be TFNAS_GROUP_SKIP, the identity candidate -- a residual cell, the skip
// groups last and empty (no width, no kernel size, no SE, no pointer), at least one computing group before them
static int check_kind(const TfnasCellDesc* d) {
    if (cell_skip(*d) && !cell_mixed(*d)) return TFNAS_EINVAL;
    if (cell_mixed(*d)) {
        if (d->mode != TFNAS_MODE_CELL || cell_noexpand(*d) || cell_fused(*d)) return TFNAS_EINVAL;
        if (cell_skip(*d) && (d->has_res != 1 || d->ic != d->oc || d->stride != 1)) return TFNAS_EINVAL;
        bool skips = false;
        for (int g = 0; g < d->G && g < TFNAS_MAX_GROUPS; ++g) {
            const TfnasGroup& gr = d->g[g];
            if (cell_skip(*d) && gr.kind == TFNAS_GROUP_SKIP) {
                if (g == 0 || gr.mc != 0 || gr.k != 0 || gr.se != 0) return TFNAS_EINVAL;
                if (gr.w_expand || gr.w_dw || gr.w_proj || gr.w_se_r || gr.b_se_r || gr.w_se_e || gr.b_se_e || gr.g_expand ||
                    gr.g_dw || gr.g_proj || gr.g_se_r || gr.gb_se_r || gr.g_se_e || gr.gb_se_e)
                    return TFNAS_EINVAL;
                skips = true;
                continue;
            }
            if (skips) return TFNAS_EINVAL;           // (a computing group after a skip: wmix / dwmix indices would move)
            if (gr.kind < TFNAS_GROUP_MBCONV || gr.kind > TFNAS_GROUP_FUSED) return TFNAS_EINVAL;
            if (gr.kind == TFNAS_GROUP_NOEXPAND && (gr.mc != d->ic || gr.w_expand || gr.g_expand)) return TFNAS_EINVAL;
            if (gr.kind == TFNAS_GROUP_FUSED && (gr.k != 3 || gr.w_dw || gr.g_dw)) return TFNAS_EINVAL;
        }
        return 0;
    }
    const CellKind kind = cell_kind(*d);
    if (kind == TFNAS_KIND_MBCONV) return 0;
    if (cell_noexpand(*d) && cell_fused(*d)) return TFNAS_EINVAL;
    if (d->mode != TFNAS_MODE_CELL || d->G != 1) return TFNAS_EINVAL;
    const TfnasGroup& g = d->g[0];
    if (kind == TFNAS_KIND_NOEXPAND && (g.mc != d->ic || g.w_expand || g.g_expand)) return TFNAS_EINVAL;
    if (kind == TFNAS_KIND_FUSED && (g.k != 3 || g.w_dw || g.g_dw)) return TFNAS_EINVAL;
    return 0;
}

// the depthwise dilations of a descriptor (tfnas_hip.h: TFNAS_CELL_DILATION; after check_kind: TfnasGroup.kind is read).  Without
// the bit TfnasGroup.dil is not read.  With it: 0 | 1 | 2 per group, and a dilated group has k 3 or 5, is a plain or an expand-free
// one (never Fused-MBConv, never a skip) and stands in a cell-mode descriptor
static int check_dilation(const TfnasCellDesc* d) {
    if (!(d->flags & TFNAS_CELL_DILATION)) return 0;
    for (int g = 0; g < d->G && g < TFNAS_MAX_GROUPS; ++g) {
        const TfnasGroup& gr = d->g[g];
        if (gr.dil < 0 || gr.dil > 2) return TFNAS_EINVAL;
        if (gr.dil != 2) continue;
        if (gr.k != 3 && gr.k != 5) return TFNAS_EINVAL;
        if (d->mode != TFNAS_MODE_CELL || cell_fused(*d)) return TFNAS_EINVAL;
        if (cell_mixed(*d) && (gr.kind == TFNAS_GROUP_FUSED || gr.kind == TFNAS_GROUP_SKIP)) return TFNAS_EINVAL;
    }
    return 0;
}

// the packed kernel-size words of a descriptor (tfnas_hip.h: TFNAS_CELL_MIXK; after check_kind and check_dilation).  Without the bit
// no word is packed: a k above 7 is refused by tfnas_cell_plan as it always was.  With it a plain k means what it means without,
// and a packed word is one of 0x53, 0x73, 0x75, 0x753 (two or three nibbles, strictly ascending, each 3 | 5 | 7, nothing above), in
// a plain or an expand-free group (never Fused-MBConv, never a skip, never dilated) of a cell-mode descriptor wide enough to give
// every segment a channel quad; a 7 needs TFNAS_CELL_K7 like a plain one
static int check_mixk(const TfnasCellDesc* d) {
    if (!(d->flags & TFNAS_CELL_MIXK)) return 0;
    for (int g = 0; g < d->G && g < TFNAS_MAX_GROUPS; ++g) {
        const TfnasGroup& gr = d->g[g];
        if (gr.k >= 0 && gr.k <= 0xf) continue;           // (a plain word: tfnas_cell_plan's own rules)
        if (gr.k != 0x53 && gr.k != 0x73 && gr.k != 0x75 && gr.k != 0x753) return TFNAS_EINVAL;
        if (gr.k != 0x53 && !(d->flags & TFNAS_CELL_K7)) return TFNAS_EINVAL;
        if (d->mode != TFNAS_MODE_CELL || cell_fused(*d)) return TFNAS_EINVAL;
        if (cell_mixed(*d) && (gr.kind == TFNAS_GROUP_FUSED || gr.kind == TFNAS_GROUP_SKIP)) return TFNAS_EINVAL;
        if (group_dil(*d, g) != 1) return TFNAS_EINVAL;
        if (gr.mc < 1 || (gr.mc + 3) / 4 < (gr.k > 0xff ? 3 : 2)) return TFNAS_EINVAL;      // (q < n: a segment without a quad)
    }
    return 0;
}

// the per-launch modes of a descriptor (callers may change them between tfnas_cell_plan and a launch: every entry point re-checks)
static int check_modes(const TfnasCellDesc* d) {
    TRY(check_act(d));
    if (d->gemm_mode != 0) {
        const int gm = d->gemm_mode & ~(TFNAS_GEMM_EXPLICIT | TFNAS_GEMM_EVERYWHERE);
        if (!(d->gemm_mode & TFNAS_GEMM_EXPLICIT) || (gm != 0 && gm != 1 && gm != 3 && gm != 6)) return TFNAS_EINVAL;
    }
    if (d->flags & ~(TFNAS_CELL_LAZY_JOIN | TFNAS_CELL_ACCUM_WGRAD | TFNAS_CELL_K7 | TFNAS_CELL_ACTS | TFNAS_CELL_NOEXPAND |
                     TFNAS_CELL_FUSED | TFNAS_CELL_KINDS | TFNAS_CELL_SE_STYLE | TFNAS_CELL_SKIP | TFNAS_CELL_DILATION |
                     TFNAS_CELL_MIXK))
        return TFNAS_EINVAL;
    TRY(check_kind(d));
    TRY(check_se_style(d));
    TRY(check_dilation(d));
    TRY(check_mixk(d));
    if (!(d->flags & TFNAS_CELL_K7)) {            // kernel size 7 is opt-in: without the bit it is refused as it always was
        for (int g = 0; g < d->G && g < TFNAS_MAX_GROUPS; ++g)
            if (d->g[g].k == 7) return TFNAS_EINVAL;          // (a packed word with a 7: check_mixk)
    }
    if (d->route & ~TFNAS_ROUTE_ALL) return TFNAS_EINVAL;
    if ((d->route & TFNAS_ROUTE_XG_OFF) && (d->route & TFNAS_ROUTE_XG_ALL)) return TFNAS_EINVAL;
    if ((d->route & TFNAS_ROUTE_SE_MASK) == TFNAS_ROUTE_SE_MASK) return TFNAS_EINVAL;     // (3 is not an excite-FC variant)
    if (d->fwd_route & ~(TFNAS_ROUTE_TAKEN_VALID | TFNAS_ROUTE_TAKEN_FX)) return TFNAS_EINVAL;
    if (d->sync_fn && d->sync_world < 1) return TFNAS_ERANGE;
    return 0;
}

// The canonical form of a (checked) descriptor, which everything past the checks works on: without TFNAS_CELL_KINDS the
// descriptor itself.  With it: all groups plain -- the bit dropped; one group -- its one-block bit instead (both then plan,
// size, route and run exactly like the descriptor a caller without the bit would have written); anything else keeps the bit: a
// mixed cell (kernels.h: cell_mixed).  TFNAS_CELL_SKIP: without a skip group the bit is dropped first (the descriptor is the one
// without the bit); with one the cell is mixed whatever its computing groups are -- never folded.
static TfnasCellDesc kinds_canon(const TfnasCellDesc& d) {
    TfnasCellDesc c = d;
    if (!cell_mixed(d)) return c;
    if (skip_groups(d) > 0) return c;
    c.flags &= ~TFNAS_CELL_SKIP;
    bool plain = true;
    for (int g = 0; g < d.G && g < TFNAS_MAX_GROUPS; ++g) plain = plain && d.g[g].kind == TFNAS_GROUP_MBCONV;
    if (plain || d.G == 1) {
        c.flags &= ~TFNAS_CELL_KINDS;
        if (!plain) c.flags |= d.g[0].kind == TFNAS_GROUP_FUSED ? TFNAS_CELL_FUSED : TFNAS_CELL_NOEXPAND;
    }
    return c;
}
TfnasCellDesc cell_canon(const TfnasCellDesc& d) { return kinds_canon(d); }     // (cell_impl.h: the path level's plan)
// the groups of one kind of a mixed cell as a sub-descriptor (kernels.h: cell_mixed): same geometry, M and offsets, the kind's
// one-block bit; returns how many there are.  group_alone: group g of a (sub-)descriptor as a one-group descriptor.
static int kind_subset(const TfnasCellDesc& d, CellKind kind, TfnasCellDesc& sub) {
    sub = d;
    int n = 0;
    for (int g = 0; g < d.G; ++g)
        if ((CellKind)d.g[g].kind == kind) sub.g[n++] = d.g[g];
    sub.G = n;
    sub.flags |= kind == TFNAS_KIND_FUSED ? TFNAS_CELL_FUSED : kind == TFNAS_KIND_NOEXPAND ? TFNAS_CELL_NOEXPAND : 0;
    return n;
}
// the computing groups of a (canonical) cell as a descriptor of their own: the first G' = G - skip_groups(d) groups, still a mixed
// cell (TFNAS_CELL_KINDS stays: its launch sequences add the residual once, over all mix weights)
static TfnasCellDesc skip_strip(const TfnasCellDesc& d) {
    TfnasCellDesc c = d;
    c.G -= skip_groups(d);
    c.flags &= ~TFNAS_CELL_SKIP;
    return c;
}
static TfnasCellDesc group_alone(const TfnasCellDesc& sub, int g) {
    TfnasCellDesc one = sub;
    one.g[0] = sub.g[g];
    one.G = 1;
    return one;
}

// (a canonical descriptor; a mixed cell: the limits of the one-block kinds hold per kind / per FUSED group)
static bool wgrad_row_fits(const TfnasCellDesc& d0) {
    const TfnasCellDesc d = skip_strip(d0);
    if (!cell_mixed(d)) return cell_fused(d) ? conv_wgrad_row_fits(d) : dw_wgrad_row_fits(d);
    TfnasCellDesc sub;
    if (kind_subset(d, TFNAS_KIND_MBCONV, sub) && !dw_wgrad_row_fits(sub)) return false;
    if (kind_subset(d, TFNAS_KIND_NOEXPAND, sub) && !dw_wgrad_row_fits(sub)) return false;
    const int nf = kind_subset(d, TFNAS_KIND_FUSED, sub);
    for (int g = 0; g < nf; ++g)
        if (!conv_wgrad_row_fits(group_alone(sub, g))) return false;
    return true;
}

extern "C" int tfnas_cell_plan(TfnasCellDesc* d) {
    if (!d) return TFNAS_ENULL;
    if (d->G < 1 || d->G > TFNAS_MAX_GROUPS) return TFNAS_ERANGE;
    if (d->mode < TFNAS_MODE_CELL || d->mode > TFNAS_MODE_HEAD) return TFNAS_EINVAL;
    if (d->mode == TFNAS_MODE_STEM) {
        /* x is the NCHW image; the 3x3 stride-2 pad-1 stem conv defines the cell's input extent */
        if (d->ic != 27 || d->G != 1 || d->Hi < 1 || d->Wi < 1 || d->has_res) return TFNAS_EINVAL;
        d->H = (d->Hi - 1) / 2 + 1;
        d->W = (d->Wi - 1) / 2 + 1;
    } else if (d->ic < 4 || (d->ic & 3)) {
        return TFNAS_EINVAL;
    }
    if (d->mode == TFNAS_MODE_HEAD && d->G != 1) return TFNAS_EINVAL;
    // the head's pooled / dpooled rows are [N][mc], moved in quads (k_head_pool, k_head_bwd): a ragged width would store over the
    // next image's row and past the buffer; every consumer of pooled needs a multiple of 4 anyway (tfnas_cls_ce)
    if (d->mode == TFNAS_MODE_HEAD && (d->g[0].mc & 3)) return TFNAS_EINVAL;
    if (d->stor != 0) return TFNAS_EINVAL;     // fp32 storage only (the bf16-storage build of rounds 1-3 was removed: tfnas_hip.h)
    if (d->N < 1 || d->H < 1 || d->W < 1 || d->oc < 4 || (d->oc & 3)) return TFNAS_EINVAL;
    if (d->oc > 1024) return TFNAS_EINVAL;
    if (d->stride != 1 && d->stride != 2) return TFNAS_EINVAL;
    TRY(check_act(d));                          // (ReLU6 / hard-swish: with TFNAS_CELL_ACTS only)
    if (d->has_res && (d->ic != d->oc || d->stride != 1)) return TFNAS_EINVAL;
    TRY(check_modes(d));
    // conv output size with pad = k/2 (same for k = 3, 5 and 7)
    d->Ho = (d->H - 1) / d->stride + 1;
    d->Wo = (d->W - 1) / d->stride + 1;
    int off = 0, se_off = 0;
    for (int g = 0; g < d->G; ++g) {
        TfnasGroup& gr = d->g[g];
        if (cell_skip(*d) && gr.kind == TFNAS_GROUP_SKIP) {      // (checked empty and last by check_kind: no columns of anything)
            gr.mcp = 0;
            gr.off = (off + 31) & ~31;
            gr.se_off = se_off;
            continue;
        }
        if (gr.mc < 1 || (gr.k != 3 && gr.k != 5 && gr.k != 7 &&      // (7: with TFNAS_CELL_K7 only, check_modes)
                          !group_packed(*d, g)) ||                     // (a packed word, TFNAS_CELL_MIXK: legal by check_mixk)
            gr.se < 0) return TFNAS_EINVAL;
        if (gr.se & 3) return TFNAS_EINVAL;       // SE widths are in_channels x {1, 2} in the search space; the excite
                                                  // GEMMs move hidden units in quads
        gr.mcp = (gr.mc + 3) & ~3;
        // every group starts on a 128-byte line of the [pixels][M] rows (and M is a multiple of 32 floats, so every row
        // does too): the 32-channel segments the depthwise kernels move and the 64-column GEMM tiles are then whole
        // lines.  Packed groups (72 / 144 / 120 / 336 floats wide) left most of them 32..96 bytes off, i.e. partial-line
        // writes and two lines fetched per segment.  The pad columns are never read or written.
        off = (off + 31) & ~31;
        gr.off = off;
        gr.se_off = se_off;
        off += gr.mcp;
        se_off += gr.se;
    }
    off = (off + 31) & ~31;
    if ((off & 511) == 0) off += 32;                  // no power-of-two-ish row stride (HBM channel aliasing)
    d->M = off;
    d->SE = se_off;
    if ((double)d->N * d->H * d->W >= 2147483647.0) return TFNAS_ERANGE;   // row indices are int, offsets size_t
    // one row of weight-gradient partials: depthwise (sum of mc * k * k); Fused-MBConv: the dense weight instead (9 ic mc)
    if (!wgrad_row_fits(kinds_canon(*d))) return TFNAS_ERANGE;
    return 0;
}

static int cell_ws_canon(const TfnasCellDesc* d, TfnasCellWs* ws);
extern "C" int tfnas_cell_ws(const TfnasCellDesc* d, TfnasCellWs* ws) {
    if (!d || !ws) return TFNAS_ENULL;
    memset(ws, 0, sizeof(*ws));
    if (cell_mixed(*d) && check_kind(d) != 0) return TFNAS_EINVAL;      // (TfnasGroup.kind is about to be read)
    // (skip groups own nothing of the workspace: what the descriptor without them reports, dwmix is the caller's [G])
    const TfnasCellDesc c = kinds_canon(skip_strip(kinds_canon(*d)));
    return cell_ws_canon(&c, ws);
}
static int cell_ws_canon(const TfnasCellDesc* d, TfnasCellWs* ws) {
    if (!wgrad_row_fits(*d)) return TFNAS_ERANGE;
    const uint64_t P = (uint64_t)d->N * d->H * d->W, Po = (uint64_t)d->N * d->Ho * d->Wo;
    const uint64_t M = d->M, N = d->N, SE = d->SE, G = d->G, oc = d->oc;
    // the four stream tensors: P*M / Po*M fp32 elements
    ws->E = any_group_has_E(*d) ? P * M : 0;             // (no expand convolution: D = dw(x) / D = conv3x3(x), nothing to save;
                                                         //  a mixed cell: the whole [pixels][M] tensor if any group is plain)
    ws->D = Po * M;
    ws->Pr = G * Po * oc;
    ws->off_pooled = 0;
    ws->off_gate = N * M;
    ws->off_hpre = 2 * N * M;
    ws->fsmall = 2 * N * M + N * SE + 4;
    ws->off_stats1 = 0;
    ws->off_stats2 = 2 * M;
    ws->off_stats3 = 4 * M;
    ws->stats = 4 * M + 2 * G * oc;
    ws->out = Po * oc;
    ws->dZ = Po * M;
    ws->dEh = P * M;                             // (an expand-free cell keeps it: scratch of the project dgrad's epilogue records and
                                                 //  of the SE backward's K-split partials, never a gradient tensor; a Fused-MBConv
                                                 //  cell then keeps dd [N*Ho*Wo][M] there)
    ws->off_dgate = 0;
    ws->off_dpooled = N * M;
    ws->off_dgl = 2 * N * M;
    ws->off_dhpre = 3 * N * M;
    ws->off_cb1 = 3 * N * M + ((N * SE + 3) & ~(uint64_t)3);
    ws->bsmall = ws->off_cb1 + 4 * M;
    ws->off_red3 = 0;
    ws->off_resdot = 2 * G * oc;                 /* [oc] per-channel <dout,x>, contiguous with red3 */
    ws->off_red2 = 2 * G * oc + oc;
    ws->off_red1 = ws->off_red2 + 2 * M;
    ws->red = ws->off_red1 + 2 * M;
    ws->part = (d->need_wgrad ? 2 : 1) * (uint64_t)TFNAS_PART_ALLOC;   // second half: weight-gradient side stream
    ws->dx = P * d->ic;
    {
        // (a mixed cell: the expand dgrad runs over its plain groups, kind_subset)
        TfnasCellDesc sub = *d;
        const bool has_E = cell_mixed(*d) ? kind_subset(*d, TFNAS_KIND_MBCONV, sub) > 0 : cell_has_E(*d);
        const int ns = (d->mode == TFNAS_MODE_STEM || !has_E) ? 1 : gemm_plan_expand_dgrad(sub, true).splits;
        ws->dxp = ns > 1 ? (uint64_t)ns * P * d->ic : 4;   /* split-K partials of the expand dgrad */
    }
    return 0;
}

// (the three queries below: of the canonical descriptor, so an all-plain TFNAS_CELL_KINDS cell answers like the unflagged one)
extern "C" int tfnas_efree_supported(const TfnasCellDesc* dp) { return (dp && efree_supported(kinds_canon(*dp))) ? 1 : 0; }
// (fx_plan refuses every mode but TFNAS_MODE_CELL, need_wgrad and ic < 64 -- the E-free widths 16 / 24 / 40 -- by itself)
extern "C" int tfnas_fx_supported(const TfnasCellDesc* dp) { return (dp && fx_supported(kinds_canon(*dp))) ? 1 : 0; }
// what a forward of this descriptor leaves in the saved buffers (tfnas_hip.h): the one decision of cell_fwd_impl that changes
// their MEANING is the fused per-image route (ehat instead of E); affine / eval BatchNorm launches (tfnas_mbconv_*) never take it
static int route_taken(const TfnasCellDesc& d, bool affine) {
    return TFNAS_ROUTE_TAKEN_VALID | ((!affine && fx_supported(d)) ? TFNAS_ROUTE_TAKEN_FX : 0);
}
extern "C" int tfnas_cell_route(const TfnasCellDesc* dp) { return dp ? route_taken(kinds_canon(*dp), false) : 0; }

// ---------------------------------------------------------------------------------------------------------------
// One cell, forward / backward: the launch sequences shared by the per-cell entry points below and by the path level
// (path.hip).
// BatchNorm channel counts / element counts of the three sites of a G = 1 block
static void bn_site(const TfnasCellDesc& d, int site, int& nch, uint64_t& cnt) {
    const uint64_t P = (uint64_t)d.N * d.H * d.W, Po = (uint64_t)d.N * d.Ho * d.Wo;
    nch = site == 2 ? d.oc : d.g[0].mc;
    cnt = site == 0 ? P : Po;
}
// an expand-free block and a Fused-MBConv block have no BatchNorm site 0: every site-0 pointer of their TfnasBnAffine must be NULL
static int check_bn_sites(const TfnasCellDesc& d, const TfnasBnAffine* bn) {
    if (cell_has_bn0(d)) return 0;
    if (bn->weight[0] || bn->bias[0] || bn->g_weight[0] || bn->g_bias[0] || bn->running_mean[0] || bn->running_var[0])
        return TFNAS_EINVAL;
    return 0;
}
static int bn_fwd_fix(const TfnasCellDesc& d, const TfnasBnAffine* bn, int site, double* stats, hipStream_t s) {
    int nch;
    uint64_t cnt;
    bn_site(d, site, nch, cnt);
    return launch_bn_fwd_fix(stats, nch, cnt, d.eps, bn->weight[site], bn->bias[site], bn->running_mean[site],
                             bn->running_var[site], bn->momentum, bn->eval, s, stats_world(d));   // (sync-stats: global batch)
}

// the front of a plain MBConv cell's forward: expand + BN1 + act + depthwise, by one of three routes; writes D and stats2
// (d: the launch's descriptor, eps = -1 with affine BatchNorm; d0: the caller's)
static int fwd_front_mbconv(const TfnasCellDesc& d, const TfnasCellDesc& d0, const CellFwdBufs& b, bool fx, bool sync,
                            double* stats1, double* stats2, hipStream_t s) {
    const TfnasBnAffine* bn = b.bn;
    if (fx) TRY(launch_fx_stats(d, b.x, stats1, b.part, s));                  // BN1 statistics from the Gram matrix of x
    else if (b.E) TRY(launch_expand_fwd(d, b.x, b.E, stats1, b.part, s));     // 1x1 expand (all groups) + BN1 statistics
    else TRY(launch_expand_stats_gram(d, b.x, stats1, b.part, s));            // E-free: BN1 statistics from the Gram matrix of x
    if (sync) TRY(stats_sync(d, stats1, 2 * (size_t)d.M, s));                    // sync-stats: global-batch sums (no-op without a hook)
    if (bn) TRY(bn_fwd_fix(d0, bn, 0, stats1, s));
    if (fx) TRY(launch_fx_fwd(d, b.x, stats1, b.E, b.D, stats2, b.part, s));  // expand + BN1 + act + depthwise in one kernel
    else TRY(launch_dw_fwd(d, b.E, b.x, stats1, b.D, stats2, b.part, s));     // BN1+act fused load, depthwise, BN2 statistics
    return 0;
}

// the fronts of a mixed cell, kind by kind on that kind's groups (sub-descriptors: kind_subset): the plain groups' materialised
// route, the expand-free groups' raw-input depthwise in one launch, one dense convolution per Fused-MBConv group.  Each writes
// its groups' columns of D and of stats2 and nothing else of either (reduce_pair_rows).
static int fwd_front_mixed(const TfnasCellDesc& d, const CellFwdBufs& b, bool sync, double* stats1, double* stats2, hipStream_t s) {
    TfnasCellDesc sub;
    if (kind_subset(d, TFNAS_KIND_MBCONV, sub)) {
        if (!b.E) return TFNAS_ENULL;
        TRY(fwd_front_mbconv(sub, sub, b, false, sync, stats1, stats2, s));
    }
    if (kind_subset(d, TFNAS_KIND_NOEXPAND, sub)) TRY(launch_dw_fwd(sub, nullptr, b.x, nullptr, b.D, stats2, b.part, s));
    const int nf = kind_subset(d, TFNAS_KIND_FUSED, sub);
    for (int g = 0; g < nf; ++g) TRY(launch_conv_fwd(group_alone(sub, g), b.x, b.D, stats2, b.part, s));
    return 0;
}

int cell_fwd_impl(const TfnasCellDesc& d0, const TfnasCellWs& ws, const CellFwdBufs& b, hipStream_t s, int* route) {
    double* stats1 = b.stats + ws.off_stats1;
    double* stats2 = b.stats + ws.off_stats2;
    double* stats3 = b.stats + ws.off_stats3;
    float* pooled = b.fsmall + ws.off_pooled;
    float* gate = b.fsmall + ws.off_gate;
    float* hpre = b.fsmall + ws.off_hpre;
    // affine / eval BatchNorm: the producers run as usual; their statistics tables are rewritten as effective (mean, rstd)
    // before the consumers -- which then run with eps = -1 (tfnas_dev.h: bn_consts) -- read them
    const TfnasBnAffine* bn = b.bn;
    // skip groups (kernels.h: cell_skip) take part in the mix alone: everything else runs on the computing groups' descriptor
    const int nw = d0.G;
    TfnasCellDesc dc = skip_strip(d0);
    if (bn) dc.eps = -1.f;
    const TfnasCellDesc& d = dc;
    // E-free late cells (14 x 14 / 7 x 7 images, 64..192 input channels): the fused per-image route (fx_kernels.hip)
    // (frozen weights only: fx_supported refuses need_wgrad; with E the forward leaves ehat there for the backward)
    // The launch's ONE route decision; the path level keeps the word for its backward (`route`).
    const int taken = route_taken(d0, bn != nullptr);
    if (route) *route = taken;
    const bool fx = (taken & TFNAS_ROUTE_TAKEN_FX) != 0;
    const bool sync = !(bn && bn->eval);          // (eval mode normalises with the running statistics: nothing to reduce)
    if (cell_mixed(d)) {                          // (no affine form: tfnas_mbconv_* refuse the bit)
        if (bn) return TFNAS_EINVAL;
        TRY(fwd_front_mixed(d, b, sync, stats1, stats2, s));
    } else
    switch (cell_kind(d)) {                       // ... D and stats2 are written:
    case TFNAS_KIND_FUSED:
        // Fused-MBConv: one dense 3 x 3 convolution of the raw cell input writes D and the BN_a statistics (no E, no stats1)
        TRY(launch_conv_fwd(d, b.x, b.D, stats2, b.part, s));
        break;
    case TFNAS_KIND_NOEXPAND:
        // no expand convolution, no BatchNorm site 0: the depthwise reads the raw cell input (E and stats1 are not touched)
        TRY(launch_dw_fwd(d, nullptr, b.x, nullptr, b.D, stats2, b.part, s));
        break;
    case TFNAS_KIND_MBCONV:
        TRY(fwd_front_mbconv(d, d0, b, fx, sync, stats1, stats2, s));
        break;
    }
    if (sync) TRY(stats_sync(d, stats2, 2 * (size_t)d.M, s));
    if (bn) TRY(bn_fwd_fix(d0, bn, 1, stats2, s));
    TRY(launch_se_pool(d, b.D, stats2, pooled, s));                           // SE squeeze (SE groups only)
    TRY(launch_se_fc_fwd(d, pooled, hpre, gate, b.part, TFNAS_PART_FLOATS, s));    // SE excite (K-split partials in `part`)
    TRY(launch_project_fwd(d, b.D, gate, stats2, b.Pr, stats3, b.part, s));   // BN2+act+gate fused load, 1x1 project, BN3 stats
    if (sync) TRY(stats_sync(d, stats3, 2 * (size_t)d.G * d.oc, s));
    if (bn) TRY(bn_fwd_fix(d0, bn, 2, stats3, s));
    if (b.drop_scale && d.has_res) {
        // drop-connect (tools/utils.py:77-86): out = scale[n] * BN3(.) + x -- the mix kernel without its residual, then one pass
        TfnasCellDesc dn = dc;
        dn.has_res = 0;
        TRY(launch_mix_fwd(dn, nw, b.Pr, stats3, b.wmix, b.x, b.out, s));
        return launch_rowscale(b.out, b.out, b.x, b.drop_scale, d.N, (uint64_t)d.Ho * d.Wo * d.oc, s);
    }
    TRY(launch_mix_fwd(d, nw, b.Pr, stats3, b.wmix, b.x, b.out, s));          // sum_g w_g BN3(.) + residual (all nw weights)
    return 0;
}

// make `side` wait for everything enqueued on `main` so far; returns the stream to launch on
static hipStream_t fork_to(const CellSide* so, int k, hipStream_t main) {
    if (!so || !so->side[k] || so->side[k] == main) return main;
    if (hipEventRecord(so->fork[k], main) != hipSuccess || hipStreamWaitEvent(so->side[k], so->fork[k], 0) != hipSuccess)
        return main;
    return so->side[k];
}

static int bn_bwd_fix(const TfnasCellDesc& d, const TfnasBnAffine* bn, int site, double* red, hipStream_t s) {
    int nch;
    uint64_t cnt;
    bn_site(d, site, nch, cnt);
    TRY(launch_bn_bwd_fix(red, nch, cnt, bn->weight[site], bn->bias[site], bn->g_weight[site], bn->g_bias[site], s,
                          wgrad_accum(d)));
    // eval mode: the statistics are constants, dx = r_eff * d -- the generic form r*(d - t1 - y*t2) with t1 = t2 = 0
    if (bn->eval) return (int)hipMemsetAsync(red, 0, sizeof(double) * 2 * (size_t)nch, s);
    return 0;
}

// dx = de W_expand (+ residual, + sink gradient) without reading E: the BN1-backward correction operator G | b goes to the top
// of `part`, then the expand dgrad (nsl >= 0: the fused route's form, launch_expand_dgrad)
static int expand_dx(const TfnasCellDesc& d, const float* dEh, const float* x, const float* cb1, float* part, const float* dout,
                     const float* wmix, float* dx, float* dxp, hipStream_t s, const float* add_src = nullptr,
                     const float* add_scale = nullptr, int nsl = -1) {
    const size_t room = TFNAS_PART_FLOATS - expand_gram_floats(d);
    float* gram = part + room;
    TRY(launch_expand_gram(d, cb1, part, room, gram, s));
    return launch_expand_dgrad(d, dEh, x, cb1, gram, dout, wmix, dx, dxp, s, add_src, add_scale, nsl);
}

// TFNAS_ROUTE_FOLD_OFF: BN2-backward tables in their own pass (k_bn2_pool) instead of the epilogue of k_project_dgrad; both
// are compared with the oracle (tests/test_gpu_cell.py::test_variant_against_oracle)

// One cell backward in flight: the launch's descriptor and buffers and the views into them.  The common prefix and the three
// kind-specific tails are member functions, so every launch line reads as it would inside one function.
namespace {
struct CellBwd {
    const TfnasCellDesc& d0;         // the caller's descriptor
    TfnasCellDesc d;                 // the launch's: eps = -1 with affine BatchNorm; without the caller's skip groups (skip_strip)
    int nw;                          // entries of wmix / dwmix: the caller's G
    const TfnasCellWs& ws;
    CellBwdBufs b;
    hipStream_t s;
    const CellSide* so;
    const TfnasBnAffine* bn;
    int taken;                       // the launch's ONE route decision (route_taken)
    const float* dout_res;           // the residual branch sees the unscaled gradient
    const double *stats1, *stats2, *stats3;
    const float *pooled, *gate, *hpre;
    float *dgate, *dpooled, *dhpre, *cb1;
    double *red3, *red2, *red1;
    float *part, *part_w, *part_w1, *part_w2;

    int run();
    int chain_mbconv(const TfnasCellDesc& d, bool whole);
    int add_sink();
    int tail_mixed();
    int tail_fused();
    int tail_noexpand();
    int tail_mbconv();
};

// everything up to and including the BN2 backward sums, then the tail of the cell's kind
int CellBwd::run() {
    if (d.need_wgrad) {
        for (int g = 0; g < d.G; ++g) {
            const TfnasGroup& gr = d.g[g];
            const CellKind kind = group_kind(d, g);
            if ((!gr.g_expand && kind != TFNAS_KIND_NOEXPAND) || (!gr.g_dw && kind != TFNAS_KIND_FUSED) || !gr.g_proj) return TFNAS_ENULL;
            if (gr.se > 0 && (!gr.g_se_r || !gr.gb_se_r || !gr.g_se_e || !gr.gb_se_e)) return TFNAS_ENULL;
        }
    }
    TRY(launch_mix_bwd_stats(d, b.dout, b.Pr, stats3, b.x, red3, part, s));           // BN3 backward sums (+ d wmix)
    TRY(stats_sync(d, red3, 2 * (size_t)d.G * d.oc, s));
    if (b.dwmix) TRY(launch_mix_dw(d, nw, red3, b.red + ws.off_resdot, b.dwmix, s));    // (skip entries: <dout, x> alone)
    if (bn) TRY(bn_bwd_fix(d0, bn, 2, red3, s));
    // Nothing upstream wants a gradient (first cell of the alpha-step: frozen weights, input = stem output):
    // d wmix is the only product, like autograd pruning the same sub-graph in the reference.
    if (!b.dx && !d.need_wgrad) return 0;
    // weight gradients: on the side stream, scratch = part_w
    if (d.need_wgrad)
        TRY(launch_project_wgrad(d, b.dout, b.Pr, b.D, gate, stats2, stats3, red3, b.wmix, part_w, fork_to(so, 0, s)));
    const bool fused2 = bn2_fused_fits(d);
    // dZ = dP W_proj; where the geometry allows, the per-image BN2-backward tables are accumulated in its epilogue (records in
    // dEh, which nothing reads or writes before the SE backward below) and gathered -- no second pass over dZ
    // (policy, measured per cell at B = 128: the epilogue's column-wise D loads cost more than k_bn2_pool's streaming pass on the
    //  write-bound all-candidate launches of the 112 x 112 / 56 x 56 cells -- cell 1: 0.99 -> 1.04 ms -- and less everywhere else:
    //  cell 10 sampled 0.126 -> 0.103 ms, cell 15 all candidates 0.286 -> 0.252 ms)
    const bool fold = fused2 && !(d.route & TFNAS_ROUTE_FOLD_OFF) && project_fold_ok(d, (size_t)ws.dEh) && (d.G == 1 || d.Ho * d.Wo <= 784);
    if (fold) {
        TRY(launch_project_dgrad(d, b.dout, b.Pr, stats3, red3, b.wmix, b.dZ, s, b.D, stats2, b.dEh));
        TRY(launch_bn2_gather(d, b.dEh, dgate, part, s));
    } else {
        TRY(launch_project_dgrad(d, b.dout, b.Pr, stats3, red3, b.wmix, b.dZ, s));
        if (fused2) TRY(launch_bn2_pool(d, b.dZ, b.D, stats2, dgate, part, s));   // d gate + per-image BN2-backward tables
        else TRY(launch_se_bwd_reduce(d, b.dZ, b.D, stats2, dgate, s));         // SE groups: d gate
    }
    // (K-split partials of the SE backward go through dEh, which is only written by the depthwise dgrad further down)
    TRY(launch_se_fc_bwd(d, dgate, gate, hpre, dhpre, dpooled, b.dEh, (size_t)ws.dEh, s));
    if (fused2) TRY(launch_bn2_finish(d, part, gate, dpooled, red2, s));      // BN2 backward sums
    else TRY(launch_bn2_bwd(d, b.dZ, b.D, stats2, gate, dpooled, red2, part, s));
    TRY(stats_sync(d, red2, 2 * (size_t)d.M, s));
    if (bn) TRY(bn_bwd_fix(d0, bn, 1, red2, s));
    if (cell_mixed(d)) return tail_mixed();
    switch (cell_kind(d)) {
    case TFNAS_KIND_FUSED: return tail_fused();
    case TFNAS_KIND_NOEXPAND: return tail_noexpand();
    case TFNAS_KIND_MBCONV: break;
    }
    return tail_mbconv();
}

// dx += add_scale[0] * add_src, the sink-connecting gradient (path level: the cell's input is a depth choice of its stage), for the
// tails whose last store of dx has no epilogue for it -- the depthwise backward-data pass, the dense dgrad, the residual pass of a
// mixed cell: one more pass over dx [N*H*W][ic], the narrowest tensor of the backward, with k_dx_reduce's rounding (sink_add) and
// as the LAST term, after the branch sum and after the residual term.  The plain tail keeps its epilogue (expand_dx).
int CellBwd::add_sink() {
    if (!b.add_src || !b.dx) return 0;
    if (!b.add_scale) return TFNAS_ENULL;
    return launch_dx_add_sink(b.dx, b.dx, b.add_src, 1, &b.add_scale, (uint64_t)d.N * d.H * d.W * d.ic, s);
}

int CellBwd::tail_fused() {
    // Fused-MBConv: dd, the gradient w.r.t. D, goes to dEh once (free since the SE backward above); the convolution's weight
    // gradient and its data gradient (which writes dx, + the unscaled residual gradient) both read it
    TRY(launch_conv_dd(d, b.dZ, b.D, gate, dpooled, stats2, red2, b.dEh, s));
    if (d.need_wgrad) {
        hipStream_t sw = fork_to(so, 1, s);
        if (d.SE > 0) TRY(launch_se_wgrad(d, dgate, gate, dhpre, hpre, pooled, sw));
        TRY(launch_conv_wgrad(d, b.dEh, b.x, part_w1, sw));
    }
    if (b.dx) TRY(launch_conv_dgrad(d, b.dEh, d.has_res ? dout_res : nullptr, b.dx, part, s));
    return add_sink();
}

int CellBwd::tail_noexpand() {
    // no expand convolution: the depthwise weight gradient reads the raw cell input, and the depthwise backward-data pass
    // writes dx itself (+ the unscaled residual gradient); no BN1 backward, no Gram operator, no expand dgrad / wgrad
    if (d.need_wgrad) {
        hipStream_t sw = fork_to(so, 1, s);
        if (d.SE > 0) TRY(launch_se_wgrad(d, dgate, gate, dhpre, hpre, pooled, sw));
        TRY(launch_dw_wgrad(d, b.dZ, gate, dpooled, b.D, stats2, red2, b.x, nullptr, part_w1, sw));
    }
    if (b.dx)
        TRY(launch_dw_bwd_dx(d, b.dZ, gate, dpooled, b.D, stats2, red2, d.has_res ? dout_res : nullptr, b.dx, s));
    return add_sink();
}

int CellBwd::tail_mbconv() {
    if (taken & TFNAS_ROUTE_TAKEN_FX) {
        // fused per-image route: depthwise dgrad + act' + the dE (rstd . W1) term of the expand dgrad in one kernel (dE never
        // materialised; partial sums per channel slice in the dEh buffer), then the BN1-backward correction -x G + b
        int nsl = 0;
        TRY(launch_fx_bwd(d, b.x, b.E, stats1, stats2, red2, b.dZ, b.D, gate, dpooled, b.dEh, (size_t)ws.dEh, red1, cb1, part, &nsl, s));
        if (b.dx) TRY(expand_dx(d, nullptr, b.x, cb1, part, dout_res, b.wmix, b.dx, b.dEh, s, b.add_src, b.add_scale, nsl));
        return 0;
    }
    return chain_mbconv(d, true);
}

// the materialised route of plain groups from the depthwise backward on: the cell's own descriptor (`whole`), or the plain groups of
// a mixed cell (tail_mixed launched the SE weight gradients of ALL groups itself, and adds the sink gradient after its last branch)
int CellBwd::chain_mbconv(const TfnasCellDesc& d, bool whole) {
    const bool se = whole && d.SE > 0;
    // the depthwise backward-data pass below, planned once; on the stride-1 ring cells and the stride-2 register-window cells
    // it also produces the depthwise weight gradient (same dd window, same E elements: no second read of E, dZ and D)
    const DwPlan dw_bwd = dw_plan_bwd_data(d, b.E == nullptr, b.x != nullptr);
    const bool dw_fused = dw_bwd.fuse_wgrad;
    if (d.need_wgrad) {
        // ONE fork for the SE and the depthwise weight gradients (every fork is an event record + a stream wait on the
        // host-bound w-step; cells without SE launch nothing for it)
        if (se || !dw_fused) {
            hipStream_t sw = fork_to(so, 1, s);
            if (se) TRY(launch_se_wgrad(d, dgate, gate, dhpre, hpre, pooled, sw));
            if (!dw_fused) TRY(launch_dw_wgrad(d, b.dZ, gate, dpooled, b.D, stats2, red2, b.E, stats1, part_w1, sw));
        }
    }
    // depthwise dgrad + BN1-backward sums; the reduction of its partial rows also fills the cb1 table
    if (bn || stats_sync_on(d)) {
        // (unfused: the reduction that also builds cb1 would use the sums before the affine fix / the cross-rank reduction)
        TRY(launch_dw_bwd_data(dw_bwd, d, b.dZ, gate, dpooled, b.D, stats2, red2, b.E, b.x, stats1, b.dEh, red1, part, s));
        TRY(stats_sync(d, red1, 2 * (size_t)d.M, s));
        if (bn) TRY(bn_bwd_fix(d0, bn, 0, red1, s));
        TRY(launch_bn1_consts(d, stats1, red1, cb1, s));
    } else {
        TRY(launch_dw_bwd_data(dw_bwd, d, b.dZ, gate, dpooled, b.D, stats2, red2, b.E, b.x, stats1, b.dEh, red1, part, s, cb1));
    }
    if (d.need_wgrad) TRY(launch_expand_wgrad(d, b.dEh, b.E, cb1, b.x, part_w2, fork_to(so, 2, s)));
    if (b.dx && d.mode != TFNAS_MODE_STEM)
        TRY(expand_dx(d, b.dEh, b.x, cb1, part, dout_res, b.wmix, b.dx, b.dxp, s, whole ? b.add_src : nullptr,
                      whole ? b.add_scale : nullptr));
    return 0;
}

// A cell whose groups differ in kind, after the shared prefix: the tail of each kind on that kind's groups (sub-descriptors,
// kind_subset), always in the order plain -> expand-free -> Fused-MBConv, groups in the caller's order inside a kind.
// dx: the FIRST branch that runs stores it, every later one read-adds-stores it, all on the chain stream `s` -- one fixed
// summation order, no atomics.  The branches run with has_res = 0 (their group indices do not index wmix); the residual gradient
// (sum of ALL mix weights) x dout is added once at the end.  dEh: the plain groups' dE and every Fused-MBConv group's dd live in
// their own groups' columns of the same rows, so the kinds never overwrite each other and the weight-gradient forks may lag.
// Fork 1 carries, in stream order, the SE weight gradients of all groups, then each kind's depthwise / dense weight gradients
// (they share that fork's scratch); fork 2 the plain groups' expand weight gradient.
int CellBwd::tail_mixed() {
    if (bn) return TFNAS_EINVAL;                      // (no affine form)
    TfnasCellDesc full = d, sub;
    full.has_res = 0;
    bool stored = false;                              // dx holds the sum of the branches so far
    if (d.need_wgrad && d.SE > 0) TRY(launch_se_wgrad(d, dgate, gate, dhpre, hpre, pooled, fork_to(so, 1, s)));
    if (kind_subset(full, TFNAS_KIND_MBCONV, sub)) {
        TRY(chain_mbconv(sub, false));
        stored = b.dx != nullptr;
    }
    if (kind_subset(full, TFNAS_KIND_NOEXPAND, sub)) {
        if (d.need_wgrad)
            TRY(launch_dw_wgrad(sub, b.dZ, gate, dpooled, b.D, stats2, red2, b.x, nullptr, part_w1, fork_to(so, 1, s)));
        for (int g = 0; b.dx && g < sub.G; ++g) {     // (one launch per group: each owns every element of dx)
            TRY(launch_dw_bwd_dx(group_alone(sub, g), b.dZ, gate, dpooled, b.D, stats2, red2, nullptr, b.dx, s, stored));
            stored = true;
        }
    }
    const int nf = kind_subset(full, TFNAS_KIND_FUSED, sub);
    for (int g = 0; g < nf; ++g) {
        const TfnasCellDesc one = group_alone(sub, g);
        TRY(launch_conv_dd(one, b.dZ, b.D, gate, dpooled, stats2, red2, b.dEh, s));
        if (d.need_wgrad) TRY(launch_conv_wgrad(one, b.dEh, b.x, part_w1, fork_to(so, 1, s)));
        if (b.dx) {
            TRY(launch_conv_dgrad(one, b.dEh, nullptr, b.dx, part, s, stored));
            stored = true;
        }
    }
    if (b.dx && d.has_res) TRY(launch_dx_add_res(d, nw, dout_res, b.wmix, b.dx, s));
    return add_sink();                                // (the path level's sink gradient: last, behind the residual term)
}
}  // namespace

int cell_bwd_impl(const TfnasCellDesc& d0, const TfnasCellWs& ws, const CellBwdBufs& b0, hipStream_t s, const CellSide* so,
                  int fwd_route) {
    const TfnasBnAffine* bn = b0.bn;
    // The launch's ONE route decision, against the forward's when the caller recorded it (per cell: tfnas_cell_route ->
    // TfnasCellDesc.fwd_route; path level: PathCtx): a backward that would read the E buffer differently from how the forward
    // wrote it (need_wgrad, the sync hook or the process-default GEMM mode changed in between) refuses before it launches anything
    const int taken = route_taken(d0, bn != nullptr);
    if ((fwd_route & TFNAS_ROUTE_TAKEN_VALID) && taken != fwd_route) return TFNAS_EINVAL;
    const CellBwdBufs& b = b0;
    CellBwd c = {d0, skip_strip(d0), d0.G, ws, b0, s, so, bn, taken, b0.dout,
                 b.stats + ws.off_stats1, b.stats + ws.off_stats2, b.stats + ws.off_stats3,
                 b.fsmall + ws.off_pooled, b.fsmall + ws.off_gate, b.fsmall + ws.off_hpre,
                 b.bsmall + ws.off_dgate, b.bsmall + ws.off_dpooled, b.bsmall + ws.off_dhpre, b.bsmall + ws.off_cb1,
                 b.red + ws.off_red3, b.red + ws.off_red2, b.red + ws.off_red1,
                 b.part, b.part_w,
                 b.part_w1 ? b.part_w1 : b.part_w,       // (forks on streams of their own must not share split-K scratch)
                 b.part_w2 ? b.part_w2 : b.part_w};
    if (bn) c.d.eps = -1.f;
    if (b0.drop_scale && d0.has_res) {
        if (!b0.dout_s) return TFNAS_ENULL;
        TRY(launch_rowscale(b0.dout_s, b0.dout, nullptr, b0.drop_scale, d0.N, (uint64_t)d0.Ho * d0.Wo * d0.oc, s));
        c.b.dout = b0.dout_s;
    }
    return c.run();
}

// E may be omitted only by a kind that has no E buffer (it is never touched) and -- where the entry point offers it -- in E-free
// mode (tfnas_efree_supported)
static int check_E(const TfnasCellDesc& d, const float* E, bool efree_counts) {
    if (E || !any_group_has_E(d) || (efree_counts && efree_supported(d))) return 0;
    return TFNAS_ENULL;
}

extern "C" int tfnas_mixedop_fwd(const TfnasCellDesc* dp, const float* x, const float* wmix, float* E, float* D,
                                 float* Pr, float* fsmall, double* stats, float* part, float* out, void* stream) {
    if (!dp || !x || !D || !Pr || !fsmall || !stats || !part || !out) return TFNAS_ENULL;
    if (dp->mode == TFNAS_MODE_HEAD) return TFNAS_EINVAL;
    TRY(check_modes(dp));
    const TfnasCellDesc d = kinds_canon(*dp);      // (TFNAS_CELL_KINDS: all groups plain / one group -> the unflagged descriptor)
    TRY(check_E(d, E, true));
    TfnasCellWs ws;
    TRY(tfnas_cell_ws(&d, &ws));
    CellFwdBufs b = {x, wmix, E, D, Pr, fsmall, stats, part, out};
    return cell_fwd_impl(d, ws, b, S(stream));
}

// What the two cell-backward entry points share: the library's side stream for the weight-gradient kernels (see SideCtx;
// scratch = the second piece of `part`), its join on every exit path, the launch sequence.  wgrad_stream: the caller-owned
// streams of the forks (tfnas_mixedop_bwd; NULL: none); lazy: leave the library's side stream unjoined (tfnas_mbconv_bwd)
static int cell_bwd_entry(const TfnasCellDesc& d, CellBwdBufs b, hipStream_t s, void* const* wgrad_stream, bool lazy) {
    TfnasCellWs ws;
    TRY(tfnas_cell_ws(&d, &ws));
    SideCtx* sc = (d.need_wgrad && route_side(d)) ? side_for(s) : nullptr;
    SideJoinGuard guard;
    guard.c = sc;
    guard.main = s;
    CellSide so = {};
    if (sc) {
        for (int i = 0; i < 3; ++i) {
            hipStream_t own = (wgrad_stream && wgrad_stream[i]) ? S(wgrad_stream[i]) : nullptr;
            so.side[i] = own ? own : sc->side;
            guard.extra[i] = own;
            so.fork[i] = sc->fork[i];
            if (own) {
                // forks on different streams run concurrently: one scratch piece each (tfnas_hip.h: `part` then holds FOUR pieces)
                b.part_w1 = b.part + 2 * TFNAS_PART_ALLOC;
                b.part_w2 = b.part + 3 * TFNAS_PART_ALLOC;
            }
        }
    }
    TRY(cell_bwd_impl(d, ws, b, s, sc ? &so : nullptr, d.fwd_route));
    if (lazy) {                                  // the caller joins later (tfnas_side_join)
        guard.joined = true;
        return guard.join_extra();               // (caller-owned streams of THIS launch are always joined here)
    }
    return guard.join();
}

extern "C" int tfnas_mixedop_bwd(const TfnasCellDesc* dp, const float* x, const float* wmix, const float* E,
                                 const float* D, const float* Pr, const float* fsmall, const double* stats,
                                 const float* dout, float* dZ, float* dEh, float* bsmall, double* red, float* part,
                                 float* dx, float* dxp, float* dwmix, void* stream) {
    if (!dp || !x || !D || !Pr || !fsmall || !stats || !dout || !dZ || !dEh || !bsmall || !red || !part)
        return TFNAS_ENULL;
    if (dp->mode == TFNAS_MODE_HEAD) return TFNAS_EINVAL;
    TRY(check_modes(dp));
    const TfnasCellDesc d = kinds_canon(*dp);
    TRY(check_E(d, E, true));
    CellBwdBufs b = {x, wmix, E, D, Pr, fsmall, stats, dout, dZ, dEh, bsmall, red, part, part + TFNAS_PART_ALLOC,
                     dx, dxp, dwmix, nullptr, nullptr};
    return cell_bwd_entry(d, b, S(stream), d.wgrad_stream, false);
}

extern "C" int tfnas_mbconv_fwd(const TfnasCellDesc* dp, const TfnasBnAffine* bn, const float* drop_scale, const float* x,
                                float* E, float* D, float* Pr, float* fsmall, double* stats, float* part, float* out,
                                void* stream) {
    if (!dp || !bn || !x || !D || !Pr || !fsmall || !stats || !part || !out) return TFNAS_ENULL;
    const TfnasCellDesc& d = *dp;
    if (d.mode == TFNAS_MODE_HEAD || d.G != 1) return TFNAS_EINVAL;
    if (cell_mixed(d)) return TFNAS_EINVAL;        // (derived blocks are one-block cells: their kind is a one-block bit)
    TRY(check_modes(dp));
    TRY(check_E(d, E, false));
    TRY(check_bn_sites(d, bn));
    TfnasCellWs ws;
    TRY(tfnas_cell_ws(dp, &ws));
    CellFwdBufs b = {x, nullptr, E, D, Pr, fsmall, stats, part, out};
    b.bn = bn;
    b.drop_scale = drop_scale;
    return cell_fwd_impl(d, ws, b, S(stream));
}

extern "C" int tfnas_mbconv_bwd(const TfnasCellDesc* dp, const TfnasBnAffine* bn, const float* drop_scale, const float* x,
                                const float* E, const float* D, const float* Pr, const float* fsmall, const double* stats,
                                const float* dout, float* dout_s, float* dZ, float* dEh, float* bsmall, double* red,
                                float* part, float* dx, float* dxp, void* stream) {
    if (!dp || !bn || !x || !D || !Pr || !fsmall || !stats || !dout || !dZ || !dEh || !bsmall || !red || !part)
        return TFNAS_ENULL;
    const TfnasCellDesc& d = *dp;
    if (d.mode == TFNAS_MODE_HEAD || d.G != 1) return TFNAS_EINVAL;
    if (d.wgrad_stream[0] || d.wgrad_stream[1] || d.wgrad_stream[2]) return TFNAS_EINVAL;     // (tfnas_mixedop_bwd only)
    if (cell_mixed(d)) return TFNAS_EINVAL;
    TRY(check_modes(dp));
    TRY(check_E(d, E, false));
    TRY(check_bn_sites(d, bn));
    CellBwdBufs b = {x, nullptr, E, D, Pr, fsmall, stats, dout, dZ, dEh, bsmall, red, part, part + TFNAS_PART_ALLOC,
                     dx, dxp, nullptr, nullptr, nullptr};
    b.bn = bn;
    b.drop_scale = drop_scale;
    b.dout_s = dout_s;
    return cell_bwd_entry(d, b, S(stream), nullptr, g_lazy_join || (d.flags & TFNAS_CELL_LAZY_JOIN));
}

// The head (1x1 conv 320->1280 + BN + swish + global average pool), forward / backward; bn != NULL: affine / eval BatchNorm,
// handled like site 0 of a cell (cell_fwd_impl)
static int head_fwd_impl(const TfnasCellDesc& d0, const TfnasBnAffine* bn, const float* x, float* E, double* stats, float* part,
                         float* pooled, hipStream_t s) {
    TfnasCellDesc dc = d0;
    if (bn) dc.eps = -1.f;
    const TfnasCellDesc& d = dc;
    TRY(launch_expand_fwd(d, x, E, stats, part, s));          // 1x1 conv 320->1280 + BN statistics
    TRY(stats_sync(d, stats, 2 * (size_t)d.M, s));
    if (bn) TRY(bn_fwd_fix(d0, bn, 0, stats, s));
    return launch_head_pool(d, E, stats, pooled, s);           // BN + swish + global average pool
}

static int head_bwd_impl(const TfnasCellDesc& d0, const TfnasBnAffine* bn, const float* x, const float* E, const double* stats,
                         const float* dpooled, float* dEh, float* cb1, double* red, float* part, float* dx, float* dxp,
                         hipStream_t s) {
    TfnasCellDesc dc = d0;
    if (bn) dc.eps = -1.f;
    const TfnasCellDesc& d = dc;
    TRY(launch_head_bwd(d, E, stats, dpooled, dEh, red, part, s));       // pool + swish backward, BN-backward sums
    TRY(stats_sync(d, red, 2 * (size_t)d.M, s));
    if (bn) TRY(bn_bwd_fix(d0, bn, 0, red, s));
    TRY(launch_bn1_consts(d, stats, red, cb1, s));
    TRY(expand_dx(d, dEh, x, cb1, part, nullptr, nullptr, dx, dxp, s));
    if (d.need_wgrad) TRY(launch_expand_wgrad(d, dEh, E, cb1, x, part, s));
    return 0;
}

// what every head entry point asks of its descriptor
static int check_head(const TfnasCellDesc* dp) {
    if (dp->mode != TFNAS_MODE_HEAD) return TFNAS_EINVAL;
    if (dp->g[0].mc & 3) return TFNAS_EINVAL;      // (pooled / dpooled rows move in quads: tfnas_cell_plan refuses it too)
    TRY(check_act(dp));
    TRY(check_se_style(dp));                       // (the head has no squeeze-excite: a non-zero style is refused)
    return check_kind(dp);
}

extern "C" int tfnas_head_affine_fwd(const TfnasCellDesc* dp, const TfnasBnAffine* bn, const float* x, float* E, double* stats,
                                     float* part, float* pooled, void* stream) {
    if (!dp || !bn || !x || !E || !stats || !part || !pooled) return TFNAS_ENULL;
    TRY(check_head(dp));
    return head_fwd_impl(*dp, bn, x, E, stats, part, pooled, S(stream));
}

extern "C" int tfnas_head_affine_bwd(const TfnasCellDesc* dp, const TfnasBnAffine* bn, const float* x, const float* E,
                                     const double* stats, const float* dpooled, float* dEh, float* cb1, double* red,
                                     float* part, float* dx, float* dxp, void* stream) {
    if (!dp || !bn || !x || !E || !stats || !dpooled || !dEh || !cb1 || !red || !part || !dx) return TFNAS_ENULL;
    TRY(check_head(dp));
    if (dp->need_wgrad && !dp->g[0].g_expand) return TFNAS_ENULL;
    return head_bwd_impl(*dp, bn, x, E, stats, dpooled, dEh, cb1, red, part, dx, dxp, S(stream));
}

extern "C" int tfnas_head_fwd(const TfnasCellDesc* dp, const float* x, float* E, double* stats, float* part,
                              float* pooled, void* stream) {
    if (!dp || !x || !E || !stats || !part || !pooled) return TFNAS_ENULL;
    TRY(check_head(dp));
    return head_fwd_impl(*dp, nullptr, x, E, stats, part, pooled, S(stream));
}

extern "C" int tfnas_head_bwd(const TfnasCellDesc* dp, const float* x, const float* E, const double* stats,
                              const float* dpooled, float* dEh, float* cb1, double* red, float* part, float* dx,
                              float* dxp, void* stream) {
    if (!dp || !x || !E || !stats || !dpooled || !dEh || !cb1 || !red || !part || !dx) return TFNAS_ENULL;
    TRY(check_head(dp));
    if (dp->need_wgrad && !dp->g[0].g_expand) return TFNAS_ENULL;
    return head_bwd_impl(*dp, nullptr, x, E, stats, dpooled, dEh, cb1, red, part, dx, dxp, S(stream));
}

extern "C" int tfnas_head_wgrad(const TfnasCellDesc* dp, const float* x, const float* E, const float* dEh, const float* cb1,
                                float* part, void* stream) {
    if (!dp || !x || !E || !dEh || !cb1 || !part) return TFNAS_ENULL;
    TRY(check_head(dp));
    const TfnasCellDesc& d = *dp;
    if (!d.g[0].g_expand) return TFNAS_ENULL;
    return launch_expand_wgrad(d, dEh, E, cb1, x, part, S(stream));
}

extern "C" int tfnas_arch_fwd(int ncell, const float* const* log_alpha, const float* e, const float* lat, float T,
                              float* w, float* cell_lat, void* stream) {
    if (ncell < 1 || ncell > TFNAS_MAX_CELLS) return TFNAS_ERANGE;
    if (!log_alpha || !e || !w) return TFNAS_ENULL;
    return launch_arch_fwd(ncell, log_alpha, e, lat, T, w, cell_lat, S(stream));
}

extern "C" int tfnas_arch_bwd(int ncell, const float* w, const float* lat, const float* dw, const float* dcell_lat,
                              float T, float* const* dlog_alpha, void* stream) {
    if (ncell < 1 || ncell > TFNAS_MAX_CELLS) return TFNAS_ERANGE;
    if (!w || !dlog_alpha) return TFNAS_ENULL;
    return launch_arch_bwd(ncell, w, lat, dw, dcell_lat, T, dlog_alpha, S(stream));
}

extern "C" int tfnas_arch_project(int n, float* const* p, const int32_t* len, void* stream) {
    if (n < 1 || n > TFNAS_MAX_CELLS) return TFNAS_ERANGE;
    if (!p || !len) return TFNAS_ENULL;
    for (int i = 0; i < n; ++i) {
        if (!p[i]) return TFNAS_ENULL;
        if (len[i] < 1 || len[i] > 8) return TFNAS_ERANGE;
    }
    return launch_arch_project(n, p, len, S(stream));
}

extern "C" int tfnas_arch_sample(int ncell, const float* const* log_alpha, const uint8_t* mask, const float* e,
                                 float T, int mode, int32_t* pos_out, void* stream) {
    if (ncell < 1 || ncell > TFNAS_MAX_CELLS) return TFNAS_ERANGE;
    if (!log_alpha || !mask || !pos_out || (mode == 0 && !e)) return TFNAS_ENULL;
    if (mode < 0 || mode > 2) return TFNAS_EINVAL;
    return launch_arch_sample(ncell, log_alpha, mask, e, T, mode, pos_out, S(stream));
}

extern "C" int tfnas_sink_fwd(int K, const float* betas, const float* const* res, const float* cell_lat,
                              uint64_t count, float* out, float* out_lat, float* bw_out, void* stream) {
    if (K < 1 || K > TFNAS_MAX_SINK) return TFNAS_ERANGE;
    if (!betas || !res || !out || !bw_out) return TFNAS_ENULL;
    if (count & 3) return TFNAS_EINVAL;
    return launch_sink_fwd(K, betas, res, cell_lat, count, out, out_lat, bw_out, S(stream));
}

extern "C" int tfnas_sink_bwd(int K, const float* bw, const float* const* res, const float* cell_lat,
                              const float* dout, const float* dlat, uint64_t count, float* const* dres,
                              float* dbetas, float* dcell_lat, double* dot_scratch, void* stream) {
    if (K < 1 || K > TFNAS_MAX_SINK) return TFNAS_ERANGE;
    if (!bw || !res || !dout || !dres || !dot_scratch) return TFNAS_ENULL;
    if (count & 3) return TFNAS_EINVAL;
    return launch_sink_bwd(K, bw, res, cell_lat, dout, dlat, count, dres, dbetas, dcell_lat, dot_scratch, S(stream));
}

extern "C" int tfnas_pack_ranges(const float* src, float* dst, int nranges, const uint64_t* off, const uint64_t* doff,
                                 const uint64_t* len, void* stream) {
    if (!src || !dst || !off || !doff || !len) return TFNAS_ENULL;
    return launch_pack_ranges(src, dst, nranges, off, doff, len, S(stream));
}

extern "C" int tfnas_sgd_clip_step(float* w, float* g, float* m, int nranges, const uint64_t* off, const uint64_t* goff,
                                   const uint64_t* len, float max_norm, float lr, float momentum, float wd, float grad_scale, double* scratch,
                                   uint64_t scratch_doubles, float* norm_out, void* stream) {
    if (!w || !g || !m || !off || !len || !scratch) return TFNAS_ENULL;
    return launch_sgd_clip_step(w, g, m, nranges, off, goff, len, max_norm, lr, momentum, wd, grad_scale, scratch, scratch_doubles,
                                norm_out, S(stream));
}

extern "C" int tfnas_sgd_clip_ema_step(float* w, float* g, float* m, int nranges, const uint64_t* off, const uint64_t* goff,
                                       const uint64_t* len, float max_norm, float lr, float momentum, float wd, float grad_scale,
                                       float* ema, float ema_alpha, double* scratch, uint64_t scratch_doubles, float* norm_out,
                                       void* stream) {
    if (!w || !g || !m || !off || !len || !scratch || !ema) return TFNAS_ENULL;
    return launch_sgd_clip_ema_step(w, g, m, nranges, off, goff, len, max_norm, lr, momentum, wd, grad_scale, ema, ema_alpha,
                                    scratch, scratch_doubles, norm_out, S(stream));
}

extern "C" int tfnas_ema_lerp(float* ema, const float* src, int nranges, const uint64_t* off, const uint64_t* len,
                              float ema_alpha, void* stream) {
    if (!ema || !src || !off || !len) return TFNAS_ENULL;
    return launch_ema_lerp(ema, src, nranges, off, len, ema_alpha, S(stream));
}

extern "C" int tfnas_opt_groups_step(const TfnasOptGroups* d, float* w, float* g, float* m, float* v, float* ema,
                                     const uint8_t* gmap, uint64_t total, double* scratch, uint64_t scratch_doubles,
                                     float* norm_out, void* stream) {
    return launch_opt_groups_step(d, w, g, m, v, ema, gmap, total, scratch, scratch_doubles, norm_out, S(stream));
}

extern "C" int tfnas_arch_adam_project(int n, float* const* p, const float* const* g, const int32_t* len, float* m, float* v,
                                       float max_norm, float lr, float beta1, float beta2, float eps, float wd, int step,
                                       float grad_scale, float* norm_out, void* stream) {
    if (!p || !g || !len || !m || !v) return TFNAS_ENULL;
    if (step < 1) return TFNAS_EINVAL;
    return launch_arch_adam_project(n, p, g, len, m, v, max_norm, lr, beta1, beta2, eps, wd, step, grad_scale, norm_out,
                                    S(stream));
}
