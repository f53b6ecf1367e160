// Host-side check of the library's block-kind handling, made to run under a sanitizer on a machine WITHOUT a GPU: it plans and
// sizes a descriptor of each kind (plain MBConv, TFNAS_CELL_NOEXPAND, TFNAS_CELL_FUSED) and a cell whose groups differ in kind
// (TFNAS_CELL_KINDS), and walks the refusal paths of the four cell entry points and the five head entry points -- NULL arguments and descriptors changed after their plan -- every one of
// which returns before anything is launched.  The buffers handed in are never touched (a few host floats stand for them).
//
// Build the library's objects with the sanitizer on the host side, this file with it, and link them into one program, e.g.
//   make -C tf-nas_amd/csrc BUILD=/tmp/san EXTRA='-Xarch_host -fsanitize=address,undefined' /tmp/san/capi.o ... (every object)
//   clang++ -std=c++17 -fsanitize=address,undefined -Iinclude -c tools/kind_refusals.cpp -o /tmp/san/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/san/*.o -o /tmp/san/kind_refusals && /tmp/san/kind_refusals
// It prints "kind_refusals: N checks ok" and exits 0, or names the first check that did not return what it should.
#include <stdio.h>
#include <string.h>

#include "tfnas_hip.h"

static int g_checks = 0, g_bad = 0;
#define EXPECT(call, want)                                                                   \
    do {                                                                                     \
        const int got_ = (call);                                                             \
        ++g_checks;                                                                          \
        if (got_ != (want)) {                                                                \
            ++g_bad;                                                                         \
            fprintf(stderr, "line %d: %s = %d, expected %d\n", __LINE__, #call, got_, want); \
        }                                                                                    \
    } while (0)

static float fbuf[8];
static double dbuf[8];
static float* const F = fbuf;      // stands for any float buffer: a refused call never reads or writes it
static double* const D = dbuf;

static TfnasCellDesc cell(int flags, int mc, int k = 3, int se = 8) {
    TfnasCellDesc d;
    memset(&d, 0, sizeof(d));
    d.N = 2, d.H = 9, d.W = 13, d.ic = 16, d.oc = 16, d.stride = 1, d.act = TFNAS_ACT_RELU, d.has_res = 1, d.G = 1;
    d.eps = 1e-5f, d.mode = TFNAS_MODE_CELL, d.flags = flags;
    d.route = TFNAS_ROUTE_WGRAD_INLINE;         // (no side stream: the backward's pointer checks come before any HIP call)
    d.g[0].mc = mc, d.g[0].k = k, d.g[0].se = se;
    return d;
}

static int fwd(const TfnasCellDesc* d, float* E) { return tfnas_mixedop_fwd(d, F, nullptr, E, F, F, F, D, F, F, nullptr); }
static int bwd(const TfnasCellDesc* d, const float* E) {
    return tfnas_mixedop_bwd(d, F, nullptr, E, F, F, F, D, F, F, F, F, D, F, F, F, nullptr, nullptr);
}
static int afwd(const TfnasCellDesc* d, const TfnasBnAffine* bn, float* E) {
    return tfnas_mbconv_fwd(d, bn, nullptr, F, E, F, F, F, D, F, F, nullptr);
}
static int abwd(const TfnasCellDesc* d, const TfnasBnAffine* bn, const float* E) {
    return tfnas_mbconv_bwd(d, bn, nullptr, F, E, F, F, F, D, F, nullptr, F, F, F, D, F, F, F, nullptr);
}

static void cells() {
    TfnasBnAffine bn;
    memset(&bn, 0, sizeof(bn));
    const int flags[3] = {0, TFNAS_CELL_NOEXPAND, TFNAS_CELL_FUSED};
    for (int kind = 0; kind < 3; ++kind) {
        TfnasCellDesc d = cell(flags[kind], kind == 1 ? 16 : 40);
        TfnasCellWs ws;
        EXPECT(tfnas_cell_plan(&d), 0);
        EXPECT(tfnas_cell_ws(&d, &ws), 0);
        EXPECT((int)(ws.E != 0), kind == 0);
        EXPECT(tfnas_cell_ws(&d, nullptr), TFNAS_ENULL);
        // NULL descriptor / NULL operand
        EXPECT(fwd(nullptr, F), TFNAS_ENULL);
        EXPECT(bwd(nullptr, F), TFNAS_ENULL);
        EXPECT(afwd(nullptr, &bn, F), TFNAS_ENULL);
        EXPECT(abwd(&d, nullptr, F), TFNAS_ENULL);
        // E may be NULL only where the kind has no E buffer (or in E-free mode, which wants frozen weights); the affine entry points of
        // such a kind then go on to the BatchNorm sites: site 0 must be empty
        if (kind == 0) {
            d.need_wgrad = 1;                    // (with frozen weights this geometry is an E-free one: E may then be NULL)
            EXPECT(fwd(&d, nullptr), TFNAS_ENULL);
            EXPECT(bwd(&d, nullptr), TFNAS_ENULL);
            d.need_wgrad = 0;
            EXPECT(afwd(&d, &bn, nullptr), TFNAS_ENULL);
            EXPECT(abwd(&d, &bn, nullptr), TFNAS_ENULL);
        } else {
            bn.weight[0] = F;
            EXPECT(afwd(&d, &bn, nullptr), TFNAS_EINVAL);
            EXPECT(abwd(&d, &bn, nullptr), TFNAS_EINVAL);
            bn.weight[0] = nullptr;
            bn.running_var[0] = F;
            EXPECT(afwd(&d, &bn, nullptr), TFNAS_EINVAL);
            bn.running_var[0] = nullptr;
        }
        // weight gradients wanted, no gradient pointer bound: refused after the plan is sized, before the first launch
        d.need_wgrad = 1;
        EXPECT(bwd(&d, F), TFNAS_ENULL);
        EXPECT(abwd(&d, &bn, F), TFNAS_ENULL);
        d.need_wgrad = 0;
        // a descriptor changed after its plan
        TfnasCellDesc c = d;
        c.flags = TFNAS_CELL_NOEXPAND | TFNAS_CELL_FUSED;
        EXPECT(tfnas_cell_plan(&c), TFNAS_EINVAL);
        EXPECT(fwd(&c, F), TFNAS_EINVAL);
        EXPECT(abwd(&c, &bn, F), TFNAS_EINVAL);
        c = d;
        c.flags |= 0x4000;                       // an unknown bit
        EXPECT(bwd(&c, F), TFNAS_EINVAL);
        if (kind != 0) {
            c = d;
            c.G = 2;
            EXPECT(fwd(&c, F), TFNAS_EINVAL);
            c = d;
            c.mode = TFNAS_MODE_STEM;
            EXPECT(afwd(&c, &bn, F), TFNAS_EINVAL);
            c = d;
            if (kind == 1) c.g[0].w_expand = F; else c.g[0].w_dw = F;
            EXPECT(fwd(&c, F), TFNAS_EINVAL);
            EXPECT(bwd(&c, F), TFNAS_EINVAL);
            c = d;
            if (kind == 1) c.g[0].g_expand = F; else c.g[0].g_dw = F;
            EXPECT(abwd(&c, &bn, F), TFNAS_EINVAL);
            c = d;
            if (kind == 1) c.g[0].mc = 24; else c.g[0].k = 5;
            EXPECT(tfnas_cell_plan(&c), TFNAS_EINVAL);
            EXPECT(afwd(&c, &bn, F), TFNAS_EINVAL);
        }
    }
}

static void heads() {
    TfnasBnAffine bn;
    memset(&bn, 0, sizeof(bn));
    TfnasCellDesc h = cell(0, 1280, 3, 0);
    h.H = h.W = 7, h.ic = 320, h.oc = 4, h.has_res = 0, h.act = TFNAS_ACT_SWISH, h.mode = TFNAS_MODE_HEAD;
    EXPECT(tfnas_cell_plan(&h), 0);
    for (int variant = 0; variant < 5; ++variant) {
        TfnasCellDesc c = h;
        int want = TFNAS_EINVAL;
        switch (variant) {
        case 0: c.mode = TFNAS_MODE_CELL; break;                              // not a head
        case 1: c.flags = TFNAS_CELL_NOEXPAND; break;                         // a kind bit on a head
        case 2: c.flags = TFNAS_CELL_FUSED; break;
        case 3: c.act = TFNAS_ACT_HSWISH; break;                              // hard-swish without TFNAS_CELL_ACTS
        case 4: c.need_wgrad = 1, want = TFNAS_ENULL; break;                  // weight gradient wanted, no pointer
        }
        if (variant != 4) {                                                    // (the forwards do not look at need_wgrad)
            EXPECT(tfnas_head_fwd(&c, F, F, D, F, F, nullptr), want);
            EXPECT(tfnas_head_affine_fwd(&c, &bn, F, F, D, F, F, nullptr), want);
        }
        EXPECT(tfnas_head_bwd(&c, F, F, D, F, F, F, D, F, F, F, nullptr), want);
        EXPECT(tfnas_head_affine_bwd(&c, &bn, F, F, D, F, F, F, D, F, F, F, nullptr), want);
        EXPECT(tfnas_head_wgrad(&c, F, F, F, F, F, nullptr), want);
    }
    EXPECT(tfnas_head_fwd(nullptr, F, F, D, F, F, nullptr), TFNAS_ENULL);
    EXPECT(tfnas_head_affine_fwd(&h, nullptr, F, F, D, F, F, nullptr), TFNAS_ENULL);
    EXPECT(tfnas_head_bwd(&h, F, nullptr, D, F, F, F, D, F, F, F, nullptr), TFNAS_ENULL);
    EXPECT(tfnas_head_affine_bwd(&h, &bn, F, F, D, nullptr, F, F, D, F, F, F, nullptr), TFNAS_ENULL);
    EXPECT(tfnas_head_wgrad(&h, F, F, nullptr, F, F, nullptr), TFNAS_ENULL);
}

// TFNAS_CELL_KINDS: a kind per group.  A three-group cell (plain 40, expand-free, Fused-MBConv 22) plans and sizes; every rule of
// the bit is refused by the plan and again by the entry points, before anything is launched.
static void mixed() {
    TfnasBnAffine bn;
    memset(&bn, 0, sizeof(bn));
    TfnasCellDesc d = cell(TFNAS_CELL_KINDS, 40);
    d.G = 3;
    d.g[1].mc = 16, d.g[1].k = 5, d.g[1].se = 0, d.g[1].kind = TFNAS_GROUP_NOEXPAND;
    d.g[2].mc = 22, d.g[2].k = 3, d.g[2].se = 8, d.g[2].kind = TFNAS_GROUP_FUSED;
    TfnasCellWs ws, ws0;
    EXPECT(tfnas_cell_plan(&d), 0);
    EXPECT(tfnas_cell_ws(&d, &ws), 0);
    EXPECT((int)(ws.E == (uint64_t)2 * 9 * 13 * d.M), 1);
    EXPECT(tfnas_efree_supported(&d), 0);
    EXPECT(tfnas_fx_supported(&d), 0);
    EXPECT(tfnas_cell_route(&d), TFNAS_ROUTE_TAKEN_VALID);
    // a plain group needs E; weight gradients wanted, no gradient pointer bound
    EXPECT(fwd(&d, nullptr), TFNAS_ENULL);
    EXPECT(bwd(&d, nullptr), TFNAS_ENULL);
    d.need_wgrad = 1;
    EXPECT(bwd(&d, F), TFNAS_ENULL);
    d.need_wgrad = 0;
    // the affine entry points refuse the bit (and more than one group)
    EXPECT(afwd(&d, &bn, F), TFNAS_EINVAL);
    EXPECT(abwd(&d, &bn, F), TFNAS_EINVAL);
    TfnasCellDesc c = cell(TFNAS_CELL_KINDS, 40);       // (one plain group: plans like the unflagged cell, still not for them)
    EXPECT(tfnas_cell_plan(&c), 0);
    EXPECT(afwd(&c, &bn, F), TFNAS_EINVAL);
    EXPECT(abwd(&c, &bn, F), TFNAS_EINVAL);
    // no plain group: no E buffer, E may be NULL (the call is then refused for its next fault: a missing gradient pointer)
    c = d;
    c.g[0].mc = 16, c.g[0].kind = TFNAS_GROUP_NOEXPAND;
    EXPECT(tfnas_cell_plan(&c), 0);
    EXPECT(tfnas_cell_ws(&c, &ws0), 0);
    EXPECT((int)(ws0.E == 0 && ws0.dxp == 4), 1);
    c.need_wgrad = 1;
    EXPECT(bwd(&c, nullptr), TFNAS_ENULL);
    // the rules, at the plan and at the entry points
    for (int variant = 0; variant < 9; ++variant) {
        c = d;
        switch (variant) {
        case 0: c.flags |= TFNAS_CELL_NOEXPAND; break;                        // a one-block bit beside it
        case 1: c.flags |= TFNAS_CELL_FUSED; break;
        case 2: c.g[1].kind = 3; break;                                       // a kind outside 0..2
        case 3: c.g[2].kind = -1; break;
        case 4: c.g[1].mc = 24; break;                                        // NOEXPAND: mc != ic
        case 5: c.g[1].w_expand = F; break;                                   // ... an expand pointer
        case 6: c.g[2].k = 5; break;                                          // FUSED: k != 3
        case 7: c.g[2].g_dw = F; break;                                       // ... a depthwise pointer
        case 8: c.g[0].k = 7; break;                                          // 7 x 7 without TFNAS_CELL_K7, as ever
        }
        EXPECT(tfnas_cell_plan(&c), TFNAS_EINVAL);
        EXPECT(fwd(&c, F), TFNAS_EINVAL);
        EXPECT(bwd(&c, F), TFNAS_EINVAL);
    }
    c = d;
    c.mode = TFNAS_MODE_STEM;
    EXPECT(fwd(&c, F), TFNAS_EINVAL);
    // without the bit the kind word is not read: the same words plan as three plain groups, and the one-block bits stay refused
    c = d;
    c.flags = 0;
    EXPECT(tfnas_cell_plan(&c), 0);
    c.flags = TFNAS_CELL_FUSED;
    EXPECT(tfnas_cell_plan(&c), TFNAS_EINVAL);
    c.flags = TFNAS_CELL_NOEXPAND;
    EXPECT(fwd(&c, F), TFNAS_EINVAL);
    // a head never carries the bit
    TfnasCellDesc h = cell(TFNAS_CELL_KINDS, 1280, 3, 0);
    h.H = h.W = 7, h.ic = 320, h.oc = 4, h.has_res = 0, h.act = TFNAS_ACT_SWISH, h.mode = TFNAS_MODE_HEAD;
    EXPECT(tfnas_cell_plan(&h), TFNAS_EINVAL);
    EXPECT(tfnas_head_fwd(&h, F, F, D, F, F, nullptr), TFNAS_EINVAL);
}

int main() {
    cells();
    heads();
    mixed();
    if (g_bad) {
        fprintf(stderr, "kind_refusals: %d of %d checks FAILED\n", g_bad, g_checks);
        return 1;
    }
    printf("kind_refusals: %d checks ok\n", g_checks);
    return 0;
}
