// Network graph, workspace planner, forward and backward schedules of the segmentation engine (engine_internal.h has the overview).
#include "engine_internal.h"

namespace {

// kernel size, stride, padding and tap count of a conv kind.  ConvTranspose and the 2^d stride-2 conv: k = 2, pad = 0, stride 2 on the fine side.
struct ConvGeom { int k, stride, pad, ntaps; };
ConvGeom conv_geom(int ck, int ndim) {
    ConvGeom g;
    g.k = (ck == CK_K3 || ck == CK_STEM3) ? 3 : (ck == CK_K2S2 || ck == CK_KT) ? 2 : 1;
    g.stride = g.k == 2 ? 2 : 1;
    g.pad = g.k == 3 ? 1 : 0;
    g.ntaps = ndim == 3 ? g.k * g.k * g.k : g.k * g.k;
    return g;
}

// ------------------------------------------------------------------------------------------------
// graph construction
// ------------------------------------------------------------------------------------------------
struct Builder {
    seg_engine& e;
    int nd;
    explicit Builder(seg_engine& e_) : e(e_), nd(e_.ndim) {}

    int param(const std::string& name, std::vector<int> shape) {
        Param p; p.name = name; p.shape = shape; p.off = e.nparam; p.numel = 1;
        for (int s : shape) p.numel *= s;
        // keep every tensor 64-float aligned inside the flat buffer (vector loads, 256-B alignment)
        e.nparam += (p.numel + 63) / 64 * 64;
        e.params.push_back(p);
        return (int)e.params.size() - 1;
    }
    std::vector<int> kshape(int a, int b, int k) {
        std::vector<int> s{a, b};
        for (int i = 0; i < nd; ++i) s.push_back(k);
        return s;
    }
    int tensor(int C, int lvl, bool image = false) {
        Ten t; t.C = C; t.lvl = lvl; t.image = image;
        e.tens.push_back(t);
        return (int)e.tens.size() - 1;
    }
    int cin(int in0, int in1) const { return e.tens[in0].C + (in1 >= 0 ? e.tens[in1].C : 0); }
    // input channels of the weight PARAMETER: an image conv on the zero-padded image tensor keeps the reference's shape [Cout][image channels][k^d]
    int cin_par(int in0, int in1) const { return e.tens[in0].image && e.pad_img ? e.in_ch : cin(in0, in1); }
    int conv_weight(const std::string& cname, int ck, int in0, int in1, int Cout) {
        const int k = conv_geom(ck, nd).k, cpar = cin_par(in0, in1);
        return param(cname + ".weight", ck == CK_KT ? kshape(cpar, Cout, k) : kshape(Cout, cpar, k));
    }
    // appends the UNIT step of a conv whose parameters exist: w, b (-1: no bias), GroupNorm gw / gb (-1: none); drop: channel dropout behind the GroupNorm
    int add_unit(int ck, int w, int b, int in0, int in1, int Cout, int lvl, int gw, int gb, bool drop = true) {
        Step s; s.type = ST_UNIT; s.ck = ck; s.in0 = in0; s.in1 = in1;
        s.Cin = cin(in0, in1);
        s.Cout = Cout; s.w = w; s.b = b;
        if (e.tens[in0].image && e.pad_img) s.cin_par = e.in_ch;
        if (gw >= 0) {
            s.gn_w = gw; s.gn_b = gb;
            if (drop) {
                s.mask_slot = (int)e.drop_ch.size();
                e.drop_ch.push_back(Cout);
            }
        }
        s.raw = tensor(Cout, lvl);
        e.steps.push_back(s);
        return (int)e.steps.size() - 1;
    }
    // conv (+ GroupNorm "<gname>.weight/.bias"; empty gname: none): creates the parameters in the reference's order, then the step
    int unit(int ck, const std::string& cname, bool bias, int in0, int in1, int Cout, int lvl_out, const std::string& gname, bool drop = true) {
        const int w = conv_weight(cname, ck, in0, in1, Cout);
        const int b = bias ? param(cname + ".bias", {Cout}) : -1;
        int gw = -1, gb = -1;
        if (!gname.empty()) { gw = param(gname + ".weight", {Cout}); gb = param(gname + ".bias", {Cout}); }
        return add_unit(ck, w, b, in0, in1, Cout, lvl_out, gw, gb, drop);
    }
    int act(int ua, int ub, int res) {
        Step s; s.type = ST_ACT; s.ua = ua; s.ub = ub; s.res = res;
        const Ten& r = e.tens[e.steps[ua].raw];
        s.out = tensor(r.C, r.lvl);
        e.steps.push_back(s);
        return s.out;
    }
    int pool(int in) {
        Step s; s.type = ST_POOL; s.in = in;
        s.out = tensor(e.tens[in].C, e.tens[in].lvl + 1);
        e.steps.push_back(s);
        return s.out;
    }
    void head(int in, const std::string& cname) {
        Step s; s.type = ST_HEAD; s.in = in; s.Cin = e.tens[in].C; s.Cout = e.ncls;
        s.w = param(cname + ".weight", kshape(e.ncls, s.Cin, 1));
        s.b = param(cname + ".bias", {e.ncls});
        e.steps.push_back(s);
    }

    // classification head on the activation `in`: fc_layers.0 (Linear(C, 128)), ReLU, fc_layers.2 (Linear(128, classes))
    void cls_head(int in, const std::string& name) {
        Step s; s.type = ST_CLS; s.in = in; s.Cin = e.tens[in].C; s.Cout = e.ncls;
        s.w = param(name + ".0.weight", {CLS_H, s.Cin});
        s.b = param(name + ".0.bias", {CLS_H});
        s.w2 = param(name + ".2.weight", {e.ncls, CLS_H});
        s.b2 = param(name + ".2.bias", {e.ncls});
        e.steps.push_back(s);
    }

    // InputTransition + four DownTransitions, shared by the VNet (VNet3d.py:25-59) and the ResNet classifiers (ResNet3d.py:24-58).  Returns the level-4
    // tensor; `skips` receives the outputs of levels 0 .. 4.  all_drop: channel dropout behind every GroupNorm (VNet); otherwise only behind down_conv
    // (ResNet: do1 is in place, so the residual `down` is the dropped tensor - drop(relu(.)) == relu(drop(.)) for multipliers >= 0, the VNet unit).
    int encoder(std::vector<int>& skips, bool all_drop) {
        const int F = e.feat;
        const int x = tensor(e.pad_img ? 16 : e.in_ch, 0, true);
        e.image_ten = x;
        // InputTransition (VNet3d.py:25-43): parameter order conv1, conv2, bn1; ONE GroupNorm for both branches
        const int ck3 = e.pad_img ? CK_K3 : CK_STEM3, ck1 = e.pad_img ? CK_K1 : CK_STEM1;
        const int w3 = conv_weight("in_tr.conv1", ck3, x, -1, F), b3 = param("in_tr.conv1.bias", {F});
        const int w1 = conv_weight("in_tr.conv2", ck1, x, -1, F), b1 = param("in_tr.conv2.bias", {F});
        const int gw = param("in_tr.bn1.weight", {F}), gb = param("in_tr.bn1.bias", {F});
        const int ua = add_unit(ck3, w3, b3, x, -1, F, 0, gw, gb, all_drop);
        const int ub = add_unit(ck1, w1, b1, x, -1, F, 0, gw, gb, all_drop);
        int prev = act(ua, ub, -1);
        skips.assign(1, prev);
        e.taps.push_back({"in_tr", prev});
        const int nconv_down[4] = {2, 3, 3, 3};
        for (int l = 1; l <= 4; ++l) {   // DownTransition (VNet3d.py:46-59)
            const int C = F << l;
            const std::string pre = "down_tr" + std::to_string(32 << (l - 1));
            const int ud = unit(CK_K2S2, pre + ".down_conv", true, prev, -1, C, l, pre + ".bn1");
            const int down = act(ud, -1, -1);
            int t = down;
            for (int i = 0; i < nconv_down[l - 1]; ++i) {
                const std::string op = pre + ".ops." + std::to_string(i);
                const int u = unit(CK_K3, op + ".conv1", true, t, -1, C, l, op + ".bn1", all_drop);
                t = act(u, -1, i == nconv_down[l - 1] - 1 ? down : -1);
            }
            prev = t;
            skips.push_back(prev);
            e.taps.push_back({pre, prev});
        }
        return prev;
    }

    void build_resnet() {   // networks/ResNet3d.py:72-118
        std::vector<int> skips;
        cls_head(encoder(skips, false), "fc_layers");
    }

    void build_vnet() {   // networks/VNet3d.py:102-158
        const int F = e.feat;
        std::vector<int> skips;
        int prev = encoder(skips, true);
        skips.pop_back();
        const int nconv_up[4] = {3, 3, 2, 1};
        for (int k = 0; k < 4; ++k) {    // UpTransition (VNet3d.py:62-80): parameter order up_conv, bn, ops, conv
            const int l = 3 - k, C = F << l;
            const std::string pre = "up_tr" + std::to_string(256 >> k);
            const int skip = skips.back(); skips.pop_back();
            const int uu = unit(CK_KT, pre + ".up_conv", true, prev, -1, C, l, pre + ".bn");
            const int gwu = e.steps[uu].gn_w, gbu = e.steps[uu].gn_b;
            const int up = act(uu, -1, -1);
            // the LUConv parameters are registered BEFORE `conv` in the reference module; keep state_dict order
            // by creating the ops' parameters first and the 1^d conv's afterwards.
            std::vector<int> opw, opb, opgw, opgb;
            for (int i = 0; i < nconv_up[k]; ++i) {
                const std::string op = pre + ".ops." + std::to_string(i);
                opw.push_back(param(op + ".conv1.weight", kshape(C, C, 3)));
                opb.push_back(param(op + ".conv1.bias", {C}));
                opgw.push_back(param(op + ".bn1.weight", {C}));
                opgb.push_back(param(op + ".bn1.bias", {C}));
            }
            const int cw = param(pre + ".conv.weight", kshape(C, 2 * C, 1));
            const int cb = param(pre + ".conv.bias", {C});
            const int uc = add_unit(CK_K1, cw, cb, up, skip, C, l, gwu, gbu);
            const int xcat = act(uc, -1, -1);
            int t = xcat;
            for (int i = 0; i < nconv_up[k]; ++i) {
                const int u = add_unit(CK_K3, opw[i], opb[i], t, -1, C, l, opgw[i], opgb[i]);
                t = act(u, -1, i == nconv_up[k] - 1 ? xcat : -1);
            }
            prev = t;
        }
        e.taps.push_back({"up_tr32", prev});      // the head's input (activation only: its gradient is virtual under a one-class head)
        head(prev, "out_tr.conv");
    }

    int unet_block(const std::string& mod, const std::string& name, int in0, int in1, int C, int lvl, bool first) {
        // Unet3d.py:64-86: conv3(no bias) GN drop relu, twice
        const int u1 = unit((first && !e.pad_img) ? CK_STEM3 : CK_K3, mod + "." + name + "conv1", false, in0, in1, C, lvl, mod + "." + name + "norm1");
        const int a1 = act(u1, -1, -1);
        const int u2 = unit(CK_K3, mod + "." + name + "conv2", false, a1, -1, C, lvl, mod + "." + name + "norm2");
        return act(u2, -1, -1);
    }
    void build_unet() {   // networks/Unet3d.py:6-62
        const int F = e.feat;
        const int x = tensor(e.pad_img ? 16 : e.in_ch, 0, true);
        e.image_ten = x;
        int t = x;
        std::vector<int> enc;
        for (int l = 0; l < 4; ++l) {
            const std::string nm = "enc" + std::to_string(l + 1);
            const int en = unet_block("encoder" + std::to_string(l + 1), nm, t, -1, F << l, l, l == 0);
            enc.push_back(en);
            t = pool(en);
        }
        t = unet_block("bottleneck", "bottleneck", t, -1, F << 4, 4, false);
        for (int l = 3; l >= 0; --l) {
            const std::string up = "upconv" + std::to_string(l + 1);
            const int uu = unit(CK_KT, up, true, t, -1, F << l, l, "");
            // plain ConvTranspose: its raw output IS the activation fed to the concat
            t = unet_block("decoder" + std::to_string(l + 1), "dec" + std::to_string(l + 1), e.steps[uu].raw, enc[l], F << l, l, false);
        }
        head(t, "conv");
    }
};

// ------------------------------------------------------------------------------------------------
// launch-argument builders (shared by planning, which asks for extents only, and the forward / backward launches)
// ------------------------------------------------------------------------------------------------
Taps make_taps(int ndim, int k, int pad) {
    Taps t; t.n = 0;
    const int kd = ndim == 3 ? k : 1;
    for (int a = 0; a < kd; ++a)
        for (int b = 0; b < k; ++b)
            for (int c = 0; c < k; ++c) {
                t.d[t.n] = (int8_t)(ndim == 3 ? a - pad : 0);
                t.h[t.n] = (int8_t)(b - pad);
                t.w[t.n] = (int8_t)(c - pad);
                ++t.n;
            }
    return t;
}

// Builders that take a workspace base `ws` return extents only for ws == nullptr (planning asks the kernels' support predicates before a workspace exists):
// every workspace pointer is then null, except the optional ones whose PRESENCE selects a kernel variant - those hold this marker.
void* const EXTENTS_ONLY_MARK = (void*)(uintptr_t)16;

// weight-gradient launch arguments of a UNIT; draw: tensor id of d(raw) or -1
WgradArgs make_wgrad_args(const seg_engine& E, const Step& s, int draw, char* ws) {
    const Ten& i0 = E.tens[s.in0];
    const Ten& ro = E.tens[s.raw];
    const int li = i0.lvl, lo = ro.lvl;
    const ConvGeom g = conv_geom(s.ck, E.ndim);
    auto P = [&](size_t off) -> const void* { return ws ? ws + off : nullptr; };
    WgradArgs w{};
    w.dw = E.g ? E.g + E.params[s.w].off : nullptr; w.N = E.N; w.sT = 1; w.sQ = g.ntaps;
    w.sd = E.ndim == 3 ? g.stride : 1; w.sh = g.stride; w.sw = g.stride;
    w.taps = make_taps(E.ndim, g.k, g.pad);
    if (s.ck == CK_KT) {
        // dW[ci][co][a] = sum_coarse X[m][ci] * dY[2m+a][co]
        w.dr = P(i0.off); w.P = s.Cin;
        w.x0 = draw >= 0 ? P(E.tens[draw].off) : nullptr; w.C0 = s.Cout; w.x1 = nullptr; w.C1 = 0; w.Q = s.Cout;
        w.ID = E.dim_d(lo); w.IH = E.dim_h(lo); w.IW = E.dim_w(lo);
        w.OD = E.dim_d(li); w.OH = E.dim_h(li); w.OW = E.dim_w(li);
        w.sP = (long long)s.Cout * g.ntaps;
    } else {
        w.dr = draw >= 0 ? P(E.tens[draw].off) : nullptr; w.P = s.Cout;
        w.x0 = P(i0.off); w.C0 = i0.C;
        w.x1 = s.in1 >= 0 ? P(E.tens[s.in1].off) : nullptr;
        w.C1 = s.in1 >= 0 ? E.tens[s.in1].C : 0;
        w.Q = s.Cin;
        w.ID = E.dim_d(li); w.IH = E.dim_h(li); w.IW = E.dim_w(li);
        w.OD = E.dim_d(lo); w.OH = E.dim_h(lo); w.OW = E.dim_w(lo);
        w.sP = (long long)(s.cin_par ? s.cin_par : s.Cin) * g.ntaps;
        if (s.ck == CK_STEM3 || s.ck == CK_STEM1) { w.stem = 1; w.Q = g.ntaps * s.Cin; }
        if (s.vact_unit >= 0) {          // x0 = the producer's raw output, activated on load
            const Step& pu = E.steps[s.vact_unit];
            w.x0 = P(E.tens[pu.raw].off);
            w.act_scale = (const float*)P(pu.scale); w.act_shift = (const float*)P(pu.shift);
            if (!ws) w.act_scale = w.act_shift = (const float*)EXTENTS_ONLY_MARK;
        }
    }
    return w;
}

// geometry of an implicit-GEMM conv launch whose GEMM rows are the voxels of level `lrow`.  Gather (lfine < 0): reads level `lsrc` at `stride` through
// k^d taps, K = taps x Kin.  Scatter: every row writes its 2^d block of level `lfine`, K = Kin.
void conv_geometry(const seg_engine& E, ConvArgs& a, int lsrc, int lrow, int lfine, int k, int stride, int Kin) {
    a.ID = E.dim_d(lsrc); a.IH = E.dim_h(lsrc); a.IW = E.dim_w(lsrc);
    a.OD = E.dim_d(lrow); a.OH = E.dim_h(lrow); a.OW = E.dim_w(lrow);
    a.scatter = lfine >= 0;
    if (a.scatter) { a.FD = E.dim_d(lfine); a.FH = E.dim_h(lfine); a.FW = E.dim_w(lfine); }
    a.sd = E.ndim == 3 ? stride : 1; a.sh = stride; a.sw = stride;
    a.taps = make_taps(E.ndim, k, k == 3 ? 1 : 0);
    a.K = a.scatter ? Kin : a.taps.n * Kin;
    a.Kpad = (a.K + 31) / 32 * 32;
}

// arguments of the forward launch of a generic (non-halo) conv UNIT: 2^d stride-2, 1^d on a (virtual) concat, ConvTranspose
ConvArgs make_fwd_conv_args(const seg_engine& E, const Step& s, char* ws) {
    const Ten& i0 = E.tens[s.in0];
    const Ten& ro = E.tens[s.raw];
    const ConvGeom g = conv_geom(s.ck, E.ndim);
    auto P = [&](size_t off) -> char* { return ws ? ws + off : nullptr; };
    ConvArgs a{};
    a.in0 = P(i0.off); a.C0 = i0.C;
    a.in1 = s.in1 >= 0 ? P(E.tens[s.in1].off) : nullptr;
    a.C1 = s.in1 >= 0 ? E.tens[s.in1].C : 0;
    a.w = P(s.wp_fwd); a.bias = (s.b >= 0 && E.p) ? E.p + E.params[s.b].off : nullptr; a.out = P(ro.off);
    a.stats = s.gn_w >= 0 ? (double*)P(s.stats) : nullptr;
    a.N = E.N; a.Cout = s.Cout;
    if (s.ck == CK_KT) {                 // scatter GEMM over the coarse rows
        conv_geometry(E, a, i0.lvl, i0.lvl, ro.lvl, g.k, g.stride, s.Cin);
        a.Ngemm = a.taps.n * s.Cout;
    } else {
        conv_geometry(E, a, i0.lvl, ro.lvl, -1, g.k, g.stride, s.Cin);
        a.Ngemm = s.Cout;
    }
    if (s.vact_unit >= 0) {              // in0 = the producer's raw output, activated on load
        const Step& pu = E.steps[s.vact_unit];
        a.in0 = P(E.tens[pu.raw].off);
        a.act_scale = (const float*)P(pu.scale); a.act_shift = (const float*)P(pu.shift);
        if (!ws) a.act_scale = a.act_shift = (const float*)EXTENTS_ONLY_MARK;
    }
    return a;
}

// data-gradient launch of a generic conv UNIT given d(raw) (tensor `draw`) into gradient tensor `g` of concat source `which`:
// 2^d stride 2 - scatter GEMM over the coarse rows; ConvTranspose - gather, stride 2 over the fine gradient; 3^d / 1^d - gather conv with flipped taps
ConvArgs make_dgrad_args(const seg_engine& E, const Step& s, int draw, int g, int which) {
    const int li = E.tens[s.in0].lvl, lo = E.tens[s.raw].lvl;
    const ConvGeom cg = conv_geom(s.ck, E.ndim);
    ConvArgs a{};
    a.in0 = E.ws + E.tens[draw].off; a.C0 = s.Cout; a.N = E.N;
    a.w = E.ws + (which ? s.wp_dg1 : s.wp_dg0); a.out = E.ws + E.tens[g].off;
    if (s.ck == CK_K2S2) {
        // d_in[2o+a][ci] = sum_co draw[o][co] W[co][ci][a]
        conv_geometry(E, a, lo, lo, li, cg.k, cg.stride, s.Cout);
        a.Cout = s.Cin; a.Ngemm = a.taps.n * s.Cin;
    } else if (s.ck == CK_KT) {
        // d_X[i][ci] = sum_{a,co} dY[2i+a][co] Wt[ci][co][a]
        conv_geometry(E, a, lo, li, -1, cg.k, cg.stride, s.Cout);
        a.Cout = a.Ngemm = s.Cin;
    } else {
        conv_geometry(E, a, lo, lo, -1, cg.k, 1, s.Cout);
        a.Cout = a.Ngemm = E.tens[which ? s.in1 : s.in0].C;
    }
    return a;
}

// both data-gradients of a 1^d conv on a (virtual) concat as ONE streaming launch over d(raw) (their packed weights lie back to back: one [C0 + C1][Kpad]
// matrix); `draw`, g0, g1: tensor ids or -1 (extents only).  Returns false where the launch does not apply.
bool make_dual_dgrad_args(const seg_engine& E, const Step& s, int draw, int g0, int g1, ConvArgs& b, char* ws) {
    if (s.ck != CK_K1 || s.in1 < 0 || E.tens[s.in0].image) return false;
    const int lo = E.tens[s.raw].lvl, C0 = E.tens[s.in0].C, C1 = E.tens[s.in1].C;
    auto P = [&](size_t off) -> char* { return ws ? ws + off : nullptr; };
    b = ConvArgs{};
    b.in0 = draw >= 0 ? P(E.tens[draw].off) : nullptr; b.C0 = s.Cout; b.N = E.N;
    conv_geometry(E, b, lo, lo, -1, 1, 1, s.Cout);
    b.w = P(s.wp_dg0); b.out = g0 >= 0 ? P(E.tens[g0].off) : nullptr; b.out1 = g1 >= 0 ? P(E.tens[g1].off) : EXTENTS_ONLY_MARK;
    b.Cout0 = C0; b.Cout = b.Ngemm = C0 + C1;
    return s.wp_dg1 == s.wp_dg0 + (size_t)C0 * b.Kpad * E.esz() && conv_uses_stream_kernel(b);
}

// halo conv at level l: the conv3x tiling `x` where the planner picked one, conv3_kernel (row-major weights) otherwise
void launch_halo_conv(const seg_engine& E, int x, int l, const void* in0, const void* in1, int C0, size_t wp, const float* bias, void* out, double* stats,
                      int Cin, int Cout, hipStream_t st, int stat_rep = STAT_REP) {
    if (x >= 0)
        launch_conv3x(x, in0, in1, C0, E.ws + wp, bias, out, stats, E.N, E.dim_d(l), E.dim_h(l), E.dim_w(l), Cin, Cout, E.ndim, E.dtype, st, stat_rep);
    else
        launch_conv3(in0, E.ws + wp, bias, out, stats, E.N, E.dim_d(l), E.dim_h(l), E.dim_w(l), Cin, Cout, E.ndim, E.dtype, st, in1, C0);
}

// statistics finalize of GroupNorm UNIT u (rep: the default, all STAT_REP replicas)
GnFinArgs gn_fin_args(const seg_engine& E, const Step& u) {
    GnFinArgs f{};
    f.stats = (double*)(E.ws + u.stats); f.gamma = E.p + E.params[u.gn_w].off; f.beta = E.p + E.params[u.gn_b].off;
    f.mask = E.mask_base(u.mask_slot);
    f.mask_ld = E.ld_mask();
    f.scale = (float*)(E.ws + u.scale); f.shift = (float*)(E.ws + u.shift);
    f.mean = (float*)(E.ws + u.mean); f.rstd = (float*)(E.ws + u.rstd);
    f.N = E.N; f.C = u.Cout; f.V = E.vol(E.tens[u.raw].lvl); f.eps = 1e-5f;
    return f;
}

// backward finalize of GroupNorm UNIT u (rep_q / rep_s: the default, all STAT_REP replicas)
GnBwdFinArgs gn_bwd_fin_args(const seg_engine& E, const Step& u) {
    GnBwdFinArgs f{};
    f.Q = (double*)(E.ws + u.Q); f.stats = (double*)(E.ws + u.stats);
    f.gamma = E.p + E.params[u.gn_w].off;
    f.mask = E.mask_base(u.mask_slot);
    f.mask_ld = E.ld_mask();
    f.mean = (float*)(E.ws + u.mean); f.rstd = (float*)(E.ws + u.rstd);
    f.dgamma = E.g + E.params[u.gn_w].off; f.dbeta = E.g + E.params[u.gn_b].off;
    f.dbias = u.b >= 0 ? E.g + E.params[u.b].off : nullptr;
    f.coef = (float*)(E.ws + u.coef);
    f.N = E.N; f.C = u.Cout; f.V = E.vol(E.tens[u.raw].lvl);
    return f;
}

// GroupNorm backward of UNIT ui given the gradient sources gl of its activation (shared by the single- and the dual-branch op)
void gn_bwd_args(const seg_engine& E, int ui, const std::vector<int>& gl, GnBwdArgs& a, GnBwdFinArgs& f) {
    const Step& u = E.steps[ui];
    const Ten& r = E.tens[u.raw];
    a = GnBwdArgs{};
    a.ndy = 0;
    for (int gi : gl) {
        if (E.tens[gi].virt && !E.head_din_needed) {
            const Step& hs = E.steps[E.head_step];
            a.vdl = E.cur_dlogits; a.vw = E.p + E.params[hs.w].off; a.vK = hs.Cout;
        } else a.dy[a.ndy++] = E.ws + E.tens[gi].off;
    }
    a.r = E.ws + r.off;
    a.scale = (float*)(E.ws + u.scale); a.shift = (float*)(E.ws + u.shift);
    a.Q = (double*)(E.ws + u.Q); a.coef = (float*)(E.ws + u.coef);
    a.dr = E.ws + E.tens[u.draw].off;
    a.N = E.N; a.C = r.C; a.V = E.vol(r.lvl);
    f = gn_bwd_fin_args(E, u);
    a.rep_q = f.rep_q = E.use_fold ? stat_rep_for(a.V) : 0;
    f.rep_s = u.stat_rep;
}

// max-pool over the fine tensor s.in (the caller sets out, or dout / din)
PoolArgs pool_args(const seg_engine& E, const Step& s) {
    const Ten& ti = E.tens[s.in];
    PoolArgs a{};
    a.in = E.ws + ti.off;
    a.N = E.N; a.D = E.dim_d(ti.lvl); a.H = E.dim_h(ti.lvl); a.W = E.dim_w(ti.lvl); a.C = ti.C;
    a.pd = E.ndim == 3 ? 2 : 1; a.ph = 2; a.pw = 2;
    return a;
}

// arguments of the fused input block behind ACT step `s` (pointers valid once the engine is bound)
seg_stemx_args stemx_args(const seg_engine& E, const Step& s) {
    const Step& ua = E.steps[s.ua];
    seg_stemx_args x{};
    x.img = E.ws + E.tens[ua.in0].off;
    x.w3 = E.ws + ua.wp_fwd; x.bias3 = ua.b >= 0 ? E.p + E.params[ua.b].off : nullptr;
    x.stats3 = (double*)(E.ws + ua.stats); x.scale3 = (float*)(E.ws + ua.scale); x.shift3 = (float*)(E.ws + ua.shift);
    x.Q3 = (double*)(E.ws + ua.Q); x.coef3 = (float*)(E.ws + ua.coef);
    if (s.ub >= 0) {
        const Step& ub = E.steps[s.ub];
        x.w1 = E.ws + ub.wp_fwd; x.bias1 = ub.b >= 0 ? E.p + E.params[ub.b].off : nullptr;
        x.stats1 = (double*)(E.ws + ub.stats); x.scale1 = (float*)(E.ws + ub.scale); x.shift1 = (float*)(E.ws + ub.shift);
        x.Q1 = (double*)(E.ws + ub.Q); x.coef1 = (float*)(E.ws + ub.coef);
    }
    x.out = E.ws + E.tens[s.out].off;
    x.partial = (float*)(E.ws + E.off_partial_stemx);
    x.N = E.N; x.D = E.dim_d(0); x.H = E.dim_h(0); x.W = E.dim_w(0); x.Cimg = E.tens[ua.in0].C;
    return x;
}

// ------------------------------------------------------------------------------------------------
// forward launches: one function per step type, called by the step's closure for every forward pass
// ------------------------------------------------------------------------------------------------
void fwd_ingest(seg_engine& E, hipStream_t st) {
    // the backward sums (Q) sit right behind the forward statistics: ONE fill clears both (a fill is a ~6 us launch on the main
    // stream); a backward pass that does not follow a forward pass directly clears Q itself
    const Ten& x = E.tens[E.image_ten];
    const size_t fill = E.stats_bytes + (E.off_Q == E.off_stats + E.stats_bytes ? E.Q_bytes : 0);
    const int pi = E.prof_begin(st, SEG_K_MISC, (double)fill + (double)E.N * E.vol(0) * (4.0 * E.in_ch + (double)x.C * E.esz()), 0.0);
    (void)hipMemsetAsync(E.ws + E.off_stats, 0, fill, st);
    E.q_clean = E.off_Q == E.off_stats + E.stats_bytes;
    launch_ingest(E.cur_x, E.ws + x.off, E.N, x.C, E.vol(0), E.dtype, st, E.in_ch, E.ride_on ? E.ride_ingest : StepRider{});
    E.prof_end(st, pi);
}

void fwd_unit(seg_engine& E, int si, hipStream_t st) {
    Step& s = E.steps[si];
    if (s.fused_stem) return;              // evaluated by the fused input block of its ACT step
    const Ten& i0 = E.tens[s.in0];
    const Ten& ro = E.tens[s.raw];
    const int ntaps = conv_geom(s.ck, E.ndim).ntaps;
    double* stats = s.gn_w >= 0 ? (double*)(E.ws + s.stats) : nullptr;
    const float* bias = s.b >= 0 ? E.p + E.params[s.b].off : nullptr;
    if (s.ck == CK_STEM3 || s.ck == CK_STEM1) {
        const int pi = E.prof_begin(st, SEG_K_STEM, E.tbytes(s.in0) + E.tbytes(s.raw), 2.0 * E.N * E.vol(0) * ntaps * i0.C * s.Cout);
        launch_stem_fwd(E.ws + i0.off, E.ws + s.wp_fwd, bias, E.ws + ro.off, stats, E.N, E.dim_d(0), E.dim_h(0), E.dim_w(0),
                        i0.C, s.Cout, s.ck == CK_STEM1, E.ndim, E.dtype, st);
        E.prof_end(st, pi);
    } else if (s.ck == CK_K3) {
        const int l = ro.lvl;
        const int pi = E.prof_begin(st, conv3_class(E.dim_w(l), s.Cin), E.tbytes(s.in0) + E.tbytes(s.raw), 2.0 * E.N * E.vol(l) * ntaps * s.Cin * s.Cout);
        // replicas this producer spreads the statistics over (read back by the folded finalize of the consumers)
        s.stat_rep = (s.x_fwd >= 0 && E.use_fold) ? stat_rep_for(E.vol(l)) : STAT_REP;
        launch_halo_conv(E, s.x_fwd, l, E.ws + i0.off, s.in1 >= 0 ? E.ws + E.tens[s.in1].off : nullptr, i0.C, s.wp_fwd, bias, E.ws + ro.off, stats,
                         s.Cin, s.Cout, st, s.stat_rep);
        E.prof_end(st, pi);
    } else {
        const ConvArgs a = make_fwd_conv_args(E, s, E.ws);
        const int li = i0.lvl, lo = ro.lvl;
        const int pi = E.prof_begin(st, SEG_K_CONV_GENERIC, E.tbytes(s.in0) + (s.in1 >= 0 ? E.tbytes(s.in1) : 0.0) + E.tbytes(s.raw),
                                    2.0 * E.N * E.vol(s.ck == CK_KT ? li : lo) * (double)a.K * a.Ngemm);
        s.stat_rep = (E.use_fold && !conv_uses_stream_kernel(a)) ? stat_rep_for(E.vol(lo)) : STAT_REP;
        launch_conv_igemm(a, E.dtype, st, s.stat_rep);
        E.prof_end(st, pi);
    }
    if (s.gn_w >= 0 && !s.fold_fin && !gn_bwd_group_eligible(s.Cout, E.vol(ro.lvl), (int)E.esz())) launch_gn_finalize(gn_fin_args(E, s), st);
}

// fused input block: statistics of both branches from the image, finalize, then recompute + normalise + add
void fwd_act_stem(seg_engine& E, const Step& s, hipStream_t st) {
    seg_stemx_args x = stemx_args(E, s);
    const int pi = E.prof_begin(st, SEG_K_STEM, E.tbytes(E.steps[s.ua].in0) * 2 + E.tbytes(s.out), 0.0);
    launch_stemx(x, 0, E.ndim, E.dtype, nullptr, nullptr, st);
    const GnFinArgs fa = gn_fin_args(E, E.steps[s.ua]);
    if (s.ub >= 0) {
        const GnFinArgs fb = gn_fin_args(E, E.steps[s.ub]);
        launch_gn_finalize(fa, st, &fb);      // both branches: one launch
    } else launch_gn_finalize(fa, st);
    launch_stemx(x, 1, E.ndim, E.dtype, nullptr, nullptr, st);
    E.prof_end(st, pi);
}

void fwd_act(seg_engine& E, int si, hipStream_t st) {
    const Step& s = E.steps[si];
    const Step& ua = E.steps[s.ua];
    if (s.vact) return;                    // applied by the reader of the tensor on load (its unit's op launched the statistics finalize)
    if (ua.fused_stem) { fwd_act_stem(E, s, st); return; }
    const Ten& ro = E.tens[ua.raw];
    if (s.ub < 0 && gn_bwd_group_eligible(ua.Cout, E.vol(ro.lvl), (int)E.esz())) {
        // small L2-resident tensor: statistics finalize + activation in one launch
        GnFinArgs f = gn_fin_args(E, ua);
        f.rep = ua.stat_rep;
        const int pi = E.prof_begin(st, SEG_K_GN_GROUP, E.tbytes(s.out) * (2 + (s.res >= 0)), 0.0);
        launch_gn_fwd_group(f, E.ws + ro.off, s.res >= 0 ? E.ws + E.tens[s.res].off : nullptr, E.ws + E.tens[s.out].off, E.dtype, st);
        E.prof_end(st, pi);
        return;
    }
    ActArgs a{};
    a.r1 = E.ws + ro.off; a.scale1 = (float*)(E.ws + ua.scale); a.shift1 = (float*)(E.ws + ua.shift);
    if (s.ub >= 0) {
        const Step& ub = E.steps[s.ub];
        a.r2 = E.ws + E.tens[ub.raw].off; a.scale2 = (float*)(E.ws + ub.scale); a.shift2 = (float*)(E.ws + ub.shift);
    }
    a.res = s.res >= 0 ? E.ws + E.tens[s.res].off : nullptr;
    a.out = E.ws + E.tens[s.out].off;
    a.N = E.N; a.C = E.tens[s.out].C; a.V = E.vol(E.tens[s.out].lvl);
    if (ua.fold_fin) {
        a.fold = 1;
        a.fin1 = gn_fin_args(E, ua); a.fin1.rep = ua.stat_rep;
        if (s.ub >= 0) { const Step& ub = E.steps[s.ub]; a.fin2 = gn_fin_args(E, ub); a.fin2.rep = ub.stat_rep; }
    }
    if (s.head_fused) {
        const Step& hs = E.steps[E.head_step];
        a.head_w = E.p + E.params[hs.w].off; a.head_b = E.p + E.params[hs.b].off;
        a.logits = E.cur_logits; a.probs = E.cur_probs; a.head_C = hs.Cout;
        if (E.ride_on && E.ride_zero) { a.zero_ptr = E.ride_zero; a.zero_n = E.ride_zero_n; E.head_zeroed = true; }
    }
    const int pi = E.prof_begin(st, SEG_K_GN_ACT, E.tbytes(s.out) * (2 + (s.ub >= 0) + (s.res >= 0)), 0.0);
    // train step whose head gradient comes from the reduce passes: the head inside this pass was the tensor's last reader
    const bool no_store = s.head_fused && E.head_no_store && si == E.head_w_act;
    launch_gn_act(a, E.dtype, st, no_store);
    E.prof_end(st, pi);
}

void fwd_pool(seg_engine& E, int si, hipStream_t st) {
    const Step& s = E.steps[si];
    PoolArgs a = pool_args(E, s);
    a.out = E.ws + E.tens[s.out].off;
    launch_maxpool_fwd(a, E.dtype, st);
}

void fwd_head(seg_engine& E, int si, hipStream_t st) {
    const Step& s = E.steps[si];
    if (s.head_fused) return;              // evaluated by the activation pass that wrote its input
    HeadArgs a;
    a.in = E.ws + E.tens[s.in].off; a.w = E.p + E.params[s.w].off; a.bias = E.p + E.params[s.b].off;
    a.logits = E.cur_logits; a.probs = E.cur_probs;
    a.N = E.N; a.V = (int)E.vol(0); a.Cin = s.Cin; a.C = s.Cout;
    if (E.ride_on && E.ride_zero) { a.zero_ptr = E.ride_zero; a.zero_n = E.ride_zero_n; E.head_zeroed = true; }
    const int pi = E.prof_begin(st, SEG_K_HEAD, E.tbytes(s.in) + 2.0 * 4.0 * E.N * E.vol(0) * s.Cout, 0.0);
    launch_head_fwd(a, E.dtype, st);
    E.prof_end(st, pi);
}

// classification head: both directions share one argument block (the backward launch reads what the forward launch left in the step's workspace)
ClsHeadArgs cls_head_args(const seg_engine& E, const Step& s) {
    ClsHeadArgs a{};
    a.act = E.ws + E.tens[s.in].off;
    a.w1 = E.p + E.params[s.w].off; a.b1 = E.p + E.params[s.b].off; a.w2 = E.p + E.params[s.w2].off; a.b2 = E.p + E.params[s.b2].off;
    a.logits = E.cur_logits; a.probs = E.cur_probs; a.dlogits = E.cur_dlogits;
    if (E.g) { a.dw1 = E.g + E.params[s.w].off; a.db1 = E.g + E.params[s.b].off; a.dw2 = E.g + E.params[s.w2].off; a.db2 = E.g + E.params[s.b2].off; }
    a.accumulate = 1;                      // the flat gradient buffer was cleared by the pass (zero_grads) or holds what the caller accumulates onto
    a.ws = E.ws + s.cls_ws;
    a.N = E.N; a.C = s.Cout; a.V = E.vol(E.tens[s.in].lvl);
    return a;
}
double cls_head_flops(const ClsHeadArgs& a) { return 2.0 * a.N * ((double)CLS_K * CLS_H + (double)CLS_H * a.C); }

void fwd_cls(seg_engine& E, int si, hipStream_t st) {
    const Step& s = E.steps[si];
    const ClsHeadArgs a = cls_head_args(E, s);
    const int pi = E.prof_begin(st, SEG_K_CLS_HEAD, E.tbytes(s.in) + 4.0 * (CLS_K * CLS_H + CLS_H * a.C), cls_head_flops(a));
    launch_cls_head_fwd(a, E.dtype, st);
    E.prof_end(st, pi);
}

// ------------------------------------------------------------------------------------------------
// backward launches (gin / gout / gl / draw / g0 / g1: gradient tensor ids fixed by the planner)
// ------------------------------------------------------------------------------------------------
void bwd_head(seg_engine& E, int si, int gin, hipStream_t st) {
    const Step& s = E.steps[si];
    HeadBwdArgs a;
    a.in = E.ws + E.tens[s.in].off; a.w = E.p + E.params[s.w].off; a.dlogits = E.cur_dlogits;
    // rank-K gradient: its readers (GroupNorm-backward passes) rebuild it from dlogits unless one of them cannot
    a.din = E.head_din_needed ? E.ws + E.tens[gin].off : nullptr;
    a.dw = E.g + E.params[s.w].off; a.db = E.g + E.params[s.b].off;
    a.N = E.N; a.V = (int)E.vol(0); a.Cin = s.Cin; a.C = s.Cout;
    const int pi = E.prof_begin(st, SEG_K_HEAD, E.tbytes(s.in) * (a.din ? 2.0 : 1.0) + 4.0 * E.N * E.vol(0) * s.Cout, 0.0);
    launch_head_bwd(a, E.dtype, st);
    E.prof_end(st, pi);
}

void bwd_cls(seg_engine& E, int si, int gin, hipStream_t st) {
    const Step& s = E.steps[si];
    ClsHeadArgs a = cls_head_args(E, s);
    a.dact = E.ws + E.tens[gin].off;
    const int pi = E.prof_begin(st, SEG_K_CLS_HEAD, E.tbytes(s.in) + 12.0 * (CLS_K * CLS_H + CLS_H * a.C), 3.0 * cls_head_flops(a));
    launch_cls_head_bwd(a, E.dtype, st);
    E.prof_end(st, pi);
}

void bwd_pool(seg_engine& E, int si, int gin, int gout, hipStream_t st) {
    PoolArgs a = pool_args(E, E.steps[si]);
    a.dout = E.ws + E.tens[gout].off; a.din = E.ws + E.tens[gin].off;
    launch_maxpool_bwd(a, E.dtype, st);
}

// fused input block: reduce (recomputing r), finalize per branch, then d(raw) in registers -> stem weight gradients; planned as one pass
// (Planner::mark_fused_stem): the reduce pass also collects the moments of the weight gradients, and a combine launch applies the coefficients
void bwd_act_stem(seg_engine& E, int si, const std::vector<int>& gl, hipStream_t st) {
    const Step& s = E.steps[si];
    seg_stemx_args x = stemx_args(E, s);
    x.ndy = (int)gl.size();
    for (int i = 0; i < x.ndy; ++i) x.dy[i] = E.ws + E.tens[gl[i]].off;
    E.flush_side(st);
    const double tb = E.tbytes(s.out);
    float* const dw3 = E.g + E.params[E.steps[s.ua].w].off;
    float* const dw1 = s.ub >= 0 ? E.g + E.params[E.steps[s.ub].w].off : nullptr;
    int pi = E.prof_begin(st, SEG_K_STEM, tb * x.ndy, 0.0);
    launch_stemx(x, E.stem_onepass ? 4 : 2, E.ndim, E.dtype, nullptr, nullptr, st);
    if (!E.stem_onepass) E.prof_end(st, pi);
    const GnBwdFinArgs fa = gn_bwd_fin_args(E, E.steps[s.ua]);
    if (s.ub >= 0) {
        const GnBwdFinArgs fb = gn_bwd_fin_args(E, E.steps[s.ub]);
        launch_gn_bwd_finalize(fa, st, &fb);  // both branches: one launch
    } else launch_gn_bwd_finalize(fa, st);
    if (E.stem_onepass) {
        launch_stemx(x, 5, E.ndim, E.dtype, dw3, dw1, st);
        E.prof_end(st, pi);
        return;
    }
    pi = E.prof_begin(st, SEG_K_STEM, tb * x.ndy, 0.0);
    launch_stemx(x, 3, E.ndim, E.dtype, dw3, dw1, st);
    E.prof_end(st, pi);
}

// both branches of the VNet input block (one GroupNorm module applied twice, networks/VNet3d.py:36-41) receive
// the SAME gradient sources: one reduce and one apply pass read them once for both (14 -> 10 tensor passes)
void bwd_act_dual(seg_engine& E, int uia, int uib, const std::vector<int>& gl, hipStream_t st) {
    GnBwdArgs a, b;
    GnBwdFinArgs fa{}, fb{};
    gn_bwd_args(E, uia, gl, a, fa);
    gn_bwd_args(E, uib, gl, b, fb);
    a.r2 = b.r; a.scale2 = b.scale; a.shift2 = b.shift; a.Q2 = b.Q; a.coef2 = b.coef; a.dr2 = b.dr;
    const double tb = E.tbytes(E.steps[uia].raw);
    int pi = E.prof_begin(st, SEG_K_GN_BWD_REDUCE, tb * (a.ndy + 2), 0.0);
    launch_gn_bwd_reduce(a, E.dtype, st);
    E.prof_end(st, pi);
    const bool fold = E.use_fold && a.C <= 256;
    if (!fold) { launch_gn_bwd_finalize(fa, st); launch_gn_bwd_finalize(fb, st); }
    pi = E.prof_begin(st, SEG_K_GN_BWD_APPLY, tb * (a.ndy + 4), 0.0);
    launch_gn_bwd_apply(a, E.dtype, st, fold ? &fa : nullptr, fold ? &fb : nullptr);
    E.prof_end(st, pi);
}

// GroupNorm backward of branch ui of ACT step asi
void bwd_act(seg_engine& E, int asi, int ui, const std::vector<int>& gl, hipStream_t st) {
    const Step& u = E.steps[ui];
    const Ten& r = E.tens[u.raw];
    GnBwdArgs a;
    GnBwdFinArgs f{};
    gn_bwd_args(E, ui, gl, a, f);
    if (E.use_coop && gn_bwd_coop_eligible(a, (int)E.esz())) {
        // 24^3 ... 6^3 levels: reduce + finalize + apply in one launch on ~one workgroup per CU (each tensor read once)
        const int pg = E.prof_begin(st, SEG_K_GN_GROUP, E.tbytes(u.raw) * (a.ndy + 2), 0.0);
        launch_gn_bwd_coop(a, f, E.dtype, st);
        E.prof_end(st, pg);
        return;
    }
    if (gn_bwd_group_eligible(r.C, a.V, (int)E.esz())) {
        const int pg = E.prof_begin(st, SEG_K_GN_GROUP, E.tbytes(u.raw) * (2 * a.ndy + 3), 0.0);
        launch_gn_bwd_group(a, f, E.dtype, st);
        E.prof_end(st, pg);
        return;
    }
    // the head's weight / bias gradient collected by this pair (Planner::mark_head_wfuse)
    GnHeadW hw{};
    if (u.head_w) {
        const Step& hs = E.steps[E.head_step];
        hw.sums = (double*)(E.ws + u.head_q); hw.dw = E.g + E.params[hs.w].off; hw.db = E.g + E.params[hs.b].off;
    }
    const GnHeadW* hwp = u.head_w ? &hw : nullptr;
    if (E.steps[asi].rq_fused) a.rep_q = f.rep_q = 0;      // the sums came with the data-gradient launch that wrote dy[0], spread over all STAT_REP replicas
    else {
        const int pi = E.prof_begin(st, SEG_K_GN_BWD_REDUCE, E.tbytes(u.raw) * (a.ndy + 1), 0.0);
        launch_gn_bwd_reduce(a, E.dtype, st, hwp);
        E.prof_end(st, pi);
    }
    const bool fold = E.use_fold && a.C <= 256;
    if (!fold) launch_gn_bwd_finalize(f, st);
    const int pi = E.prof_begin(st, SEG_K_GN_BWD_APPLY, E.tbytes(u.raw) * (a.ndy + 2), 0.0);
    launch_gn_bwd_apply(a, E.dtype, st, fold ? &f : nullptr, nullptr, hwp);
    E.prof_end(st, pi);
}

// halo conv UNIT: weight gradient (deterministic two-stage reduction) + data gradient(s)
void bwd_unit_halo(seg_engine& E, int si, int draw, int g0, int g1, hipStream_t st) {
    const Step& s = E.steps[si];
    const int lo = E.tens[s.raw].lvl;
    const double fl = 2.0 * E.N * E.vol(lo) * conv_geom(s.ck, E.ndim).ntaps * s.Cin * s.Cout;
    E.defer_wgrad(st, [this_ = &E, si, draw, fl, lo](hipStream_t ws_) {
        seg_engine& E = *this_;
        const Step& s = E.steps[si];
        const Ten& i0 = E.tens[s.in0];
        const int pi = E.prof_begin(ws_, SEG_K_WGRAD3, E.tbytes(draw) + E.tbytes(s.in0) + (s.in1 >= 0 ? E.tbytes(s.in1) : 0.0), fl);
        Wgrad3Reduce rd;
        float* slot = E.w3_slot(lo, ws_);
        launch_wgrad3(E.ws + E.tens[draw].off, E.ws + i0.off, slot, E.g + E.params[s.w].off,
                      E.N, E.dim_d(lo), E.dim_h(lo), E.dim_w(lo), s.Cout, s.Cin, E.ndim, E.dtype, ws_,
                      s.in1 >= 0 ? E.ws + E.tens[s.in1].off : nullptr, i0.C, s.cin_par, &rd);
        E.w3_pending.push_back(rd);
        if (E.w3_mode == 0 || !E.use_side) E.flush_w3();
        E.prof_end(ws_, pi);
    }, E.tbytes(draw), lo);
    const int gs[2] = {g0, g1}, xs[2] = {s.x_dg0, s.x_dg1}, ins[2] = {s.in0, s.in1};
    const size_t wps[2] = {s.wp_dg0, s.wp_dg1};
    for (int j = 0; j < 2; ++j) {
        if (gs[j] < 0) continue;
        const int C = E.tens[ins[j]].C;
        const int pi = E.prof_begin(st, conv3_class(E.dim_w(lo), s.Cout), E.tbytes(draw) + E.tbytes(gs[j]), fl * C / s.Cin);
        launch_halo_conv(E, xs[j], lo, E.ws + E.tens[draw].off, nullptr, 0, wps[j], nullptr, E.ws + E.tens[gs[j]].off, nullptr, s.Cout, C, st);
        E.prof_end(st, pi);
    }
}

// UNIT: weight gradient + data gradient(s) given d(raw)
void bwd_unit(seg_engine& E, int si, int draw, int g0, int g1, hipStream_t st) {
    const Step& s = E.steps[si];
    const Ten& i0 = E.tens[s.in0];
    const int li = i0.lvl, lo = E.tens[s.raw].lvl;
    // ---- bias gradient of convs without GroupNorm (the UNet up-convs): a column sum of d(raw).  On the main queue: the second queue carries the
    // critical tail of the UNet steps (moved there in round 5: UNet3d 2 x 128^3 4.46-4.49 vs 4.38-4.44 ms, profiles/r05_colsum_ab.log)
    if (s.gn_w < 0 && s.b >= 0) launch_colsum(E.ws + E.tens[draw].off, E.g + E.params[s.b].off, (long long)E.N * E.vol(lo), s.Cout, E.dtype, st);
    if (s.ck == CK_K3) { bwd_unit_halo(E, si, draw, g0, g1, st); return; }
    if (s.ck == CK_STEM3 || s.ck == CK_STEM1) {
        // The image stems close the backward pass: nothing is left on the main stream to overlap with, so both run on the main stream (in order
        // there) with their own scratch; the shared partial buffer belongs to whatever the weight-gradient stream is still reducing.  Step-24 trace:
        // with the 3^d stem on the side stream the main stream idled 256 us at the end of every step behind wgrad3(16ch@96^3) + the 1^d concat
        // wgrad + this kernel.
        E.flush_side(st);
        const int pi = E.prof_begin(st, SEG_K_STEM, E.tbytes(draw) + E.tbytes(s.in0), 0.0);
        launch_stem_wgrad(E.ws + E.tens[draw].off, E.ws + i0.off, (float*)(E.ws + E.off_partial_stem1), E.g + E.params[s.w].off,
                          E.N, E.dim_d(0), E.dim_h(0), E.dim_w(0), i0.C, s.Cout, s.ck == CK_STEM1, E.ndim, E.dtype, st);
        E.prof_end(st, pi);
        return;
    }
    // ---- weight gradient
    E.defer_wgrad(st, [this_ = &E, si, draw](hipStream_t ws_) {
        seg_engine& E = *this_;
        const Step& s = E.steps[si];
        WgradArgs w = make_wgrad_args(E, s, draw, E.ws);
        const int pi = E.prof_begin(ws_, SEG_K_WGRAD_GENERIC, E.tbytes(draw) + E.tbytes(s.in0) + (s.in1 >= 0 ? E.tbytes(s.in1) : 0.0), 0.0);
        launch_wgrad(w, (float*)(E.ws + E.cur_partial), E.dtype, ws_, s.cin_par);
        E.prof_end(ws_, pi);
    }, E.tbytes(draw), lo < li ? lo : li);
    // ---- data gradient(s)
    if (g0 >= 0 && g1 >= 0 && s.dual_dg) {
        // 1^d conv on a concat: both data-gradients from ONE pass over d(raw) (113 MB at the 96^3 level)
        ConvArgs b;
        if (make_dual_dgrad_args(E, s, draw, g0, g1, b, E.ws)) {
            if (s.rq_dg) {   // ... and the GroupNorm-backward sums of the up-conv unit whose (virtual) activation is the first source
                const Step& pu = E.steps[s.vact_unit];
                b.rq_r = E.ws + E.tens[pu.raw].off; b.rq_scale = (const float*)(E.ws + pu.scale); b.rq_shift = (const float*)(E.ws + pu.shift);
                b.rq_Q = (double*)(E.ws + pu.Q);
            }
            launch_conv_igemm(b, E.dtype, st, STAT_REP);
            return;
        }
    }
    if (g0 >= 0) launch_conv_igemm(make_dgrad_args(E, s, draw, g0, 0), E.dtype, st, STAT_REP);
    if (g1 >= 0) launch_conv_igemm(make_dgrad_args(E, s, draw, g1, 1), E.dtype, st, STAT_REP);
}

// ------------------------------------------------------------------------------------------------
// planning: workspace layout + forward / backward schedules
// ------------------------------------------------------------------------------------------------
struct Planner {
    seg_engine& E;
    size_t cur = 0;
    explicit Planner(seg_engine& e_) : E(e_) {}
    size_t alloc(size_t bytes) { size_t o = cur; cur = align_up(cur + bytes); return o; }
    size_t ten_bytes(const Ten& t) const { return (size_t)E.N * E.vol(t.lvl) * t.C * E.esz(); }
    int new_grad(int like) {
        Ten t; t.C = E.tens[like].C; t.lvl = E.tens[like].lvl;
        t.off = alloc(ten_bytes(t));
        E.tens.push_back(t);
        return (int)E.tens.size() - 1;
    }
    bool small_group(const Step& u) const { return gn_bwd_group_eligible(u.Cout, E.vol(E.tens[u.raw].lvl), (int)E.esz()); }   // one-launch small-tensor passes

    // `bwd`: the descriptor feeds the backward pass only (data-gradient layouts)
    void add_pack(bool bwd, size_t dst, long long src_off, int R1, int R2, int T, int Cc, long long s1, long long s2, long long sT, long long sC, int flip,
                  int frag = 0, int csrc = 0) {
        PackDesc d;
        d.frag = frag;
        d.csrc = csrc;
        d.src = (const float*)(uintptr_t)src_off;   // offsets; resolved in seg_bind
        d.dst = (void*)(uintptr_t)dst;
        d.R1 = R1; d.R2 = R2; d.T = T; d.Cc = Cc;
        d.Kpad = frag == 3 ? 480 : (T * Cc + 31) / 32 * 32;      // frag 3: 15 steps of two 16-channel taps (conv3x16r_kernel)
        d.s1 = s1; d.s2 = s2; d.sT = sT; d.sC = sC; d.flipT = flip;
        E.packdescs.push_back(d);
        E.pack_is_bwd.push_back(bwd ? 1 : 0);
        const long long tot = (long long)R1 * R2 * d.Kpad;
        if (tot > E.pack_max) E.pack_max = tot;
    }
    size_t alloc_pack(int rows, int K, int frag = 0) { return alloc((size_t)rows * (frag == 3 ? 480 : (K + 31) / 32 * 32) * E.esz()); }

    void plan() {
        reset();
        mark_fused_stem();
        mark_vact();
        mark_head_fuse();
        mark_head_wfuse();
        mark_fold();
        layout_workspace();
        layout_packed_weights();
        mark_dual_dgrad();
        alloc_partials();
        schedule_forward();
        if (!schedule_backward()) return;
        E.ws_bytes = align_up(cur, 4096);
        E.planned = true;
    }

    void reset() {
        E.fwd_ops.clear(); E.bwd_ops.clear(); E.bwd_writes.clear(); E.packdescs.clear(); E.pack_is_bwd.clear(); E.pack_max = 0;
        // drop gradient tensors of a previous plan
        size_t nfw = 0;
        for (auto& s : E.steps) {
            nfw = std::max<size_t>(nfw, std::max(s.raw, s.out) + 1);
            s.draw = -1;
        }
        E.tens.resize(std::max<size_t>(nfw, (size_t)E.image_ten + 1));
        for (auto& t : E.tens) t.grads.clear();
    }

    // ---- fused input block: an ACT whose unit(s) are image stems (3^d [+ 1^d]) without a residual
    void mark_fused_stem() {
        for (auto& s : E.steps) s.fused_stem = false;
        E.stem_onepass = false;
        if (!(E.use_stemx && E.feat == 16 && (long long)E.vol(0) * 16 * 4 < (1ll << 31))) return;
        for (auto& A : E.steps)
            if (A.type == ST_ACT && A.res < 0 && E.steps[A.ua].ck == CK_STEM3 && E.steps[A.ua].gn_w >= 0 &&
                (A.ub < 0 || (E.steps[A.ub].ck == CK_STEM1 && E.steps[A.ub].gn_w >= 0))) {
                E.steps[A.ua].fused_stem = true;
                if (A.ub >= 0) E.steps[A.ub].fused_stem = true;
                // the backward pass reads the gradient sources (tensors of A.out's size) once - like mark_vact where they cost bandwidth, SEG_STEMX_ONEPASS=2 anywhere
                if (E.use_stemx_onepass && (E.use_stemx_onepass >= 2 || (double)ten_bytes(E.tens[A.out]) >= 16e6)) E.stem_onepass = true;
            }
    }

    // ---- activations that are never written: the output of a single-branch ACT step without residual whose ONLY reader is the first source of a 1^d conv on a
    // (virtual) concat - the VNet up-conv -> concat -> conv chain, networks/VNet3d.py:72-77 - on tensors large enough for the two passes over it to cost
    // bandwidth (>= 16 MB: the 96^3 and 48^3 decoder levels of the benchmark; below, the launches are latency and the generic conv kernel applies).  The
    // reader's forward launch (streaming conv kernel) and its weight gradient (direct kernel) take the producer's raw output and apply scale / shift / ReLU on
    // load; the unit's gradient flow is unchanged.  16-bit run dtypes.
    void mark_vact() {
        for (auto& s : E.steps) { s.vact = false; s.vact_unit = -1; }
        if (!E.use_vact || E.dtype == DT_F32) return;
        for (auto& A : E.steps) {
            if (A.type != ST_ACT || A.ub >= 0 || A.res >= 0 || E.steps[A.ua].fused_stem || E.steps[A.ua].gn_w < 0) continue;
            if (E.use_vact < 2 && (double)ten_bytes(E.tens[A.out]) < 16e6) continue;
            int readers = 0, ci = -1;
            for (size_t k = 0; k < E.steps.size(); ++k) {
                const Step& c = E.steps[k];
                if (c.type == ST_UNIT) { if (c.in0 == A.out) { ++readers; ci = (int)k; } if (c.in1 == A.out) readers += 2; }
                else if (c.type == ST_ACT) { if (c.res == A.out) readers += 2; }
                else if (c.in == A.out) readers += 2;
            }
            if (readers != 1) continue;
            Step& c = E.steps[ci];
            if (c.ck != CK_K1 || E.tens[c.in0].image) continue;
            c.vact_unit = A.ua;
            if (conv_uses_stream_kernel(make_fwd_conv_args(E, c, nullptr)) && wgrad_act_supported(make_wgrad_args(E, c, -1, nullptr))) A.vact = true;
            else c.vact_unit = -1;
        }
    }

    // ---- the 1^d head evaluated by the activation pass that writes its input (16 channels, <= 4 classes)
    void mark_head_fuse() {
        for (auto& s : E.steps) s.head_fused = false;
        if (!E.use_head_fuse) return;
        for (auto& hs : E.steps) {
            if (hs.type != ST_HEAD) continue;
            for (auto& A : E.steps) {
                if (A.type != ST_ACT || A.out != hs.in || A.vact || A.ub >= 0 || E.steps[A.ua].fused_stem || E.steps[A.ua].gn_w < 0) continue;
                if (small_group(E.steps[A.ua])) continue;
                if (!gn_act_head_supported(E.tens[A.out].C, hs.Cout, false) || E.tens[A.out].lvl != 0) continue;
                A.head_fused = true; hs.head_fused = true;
            }
        }
    }

    // the GroupNorm backward of ACT step A is a gn_bwd_reduce_kernel + gn_bwd_apply_kernel pair that takes the virtual head source: one branch, a written
    // tensor, not the fused input block, not the one-launch small-tensor form (the co-operative form never takes a virtual source, the sums on a data-gradient
    // launch belong to never-written activations)
    bool reduce_pass_under_head(const Step& A) const {
        if (A.type != ST_ACT || A.ub >= 0 || A.vact) return false;
        const Step& u = E.steps[A.ua];
        return !u.fused_stem && u.gn_w >= 0 && !small_group(u);
    }
    int readers_of(int ten) const {
        int n = 0;
        for (auto& c : E.steps) {
            if (c.type == ST_UNIT) n += (c.in0 == ten) + (c.in1 == ten);
            else if (c.type == ST_ACT) n += c.res == ten;
            else n += c.in == ten;
        }
        return n;
    }

    // ---- weight / bias gradient of a one-class head from the GroupNorm-backward reduce passes of the units its input is made of (GnHeadW): the head's input
    // A.out = relu(GN(L)) [+ B.out], B.out = relu(GN(C)), is then read by nobody but the head's forward, and head_bwd_kernel (one launch, one pass over the
    // tensor) goes.  Like mark_vact only where the tensor costs bandwidth, SEG_HEAD_WFUSE=2 anywhere.
    void mark_head_wfuse() {
        for (auto& s : E.steps) { s.head_w = 0; s.head_q = 0; }
        E.head_w_act = -1;
        if (!E.use_head_wfuse || !E.use_vhead) return;
        for (auto& hs : E.steps) {
            if (hs.type != ST_HEAD || hs.Cout != 1) continue;
            for (size_t ai = 0; ai < E.steps.size(); ++ai) {
                Step& A = E.steps[ai];
                if (A.type != ST_ACT || A.out != hs.in || !reduce_pass_under_head(A)) continue;
                const int C = E.tens[A.out].C;
                if (C > 128 || readers_of(A.out) != 1) continue;
                if (E.use_head_wfuse < 2 && (double)ten_bytes(E.tens[A.out]) < 16e6) continue;
                Step* B = nullptr;
                if (A.res >= 0) {
                    for (auto& b : E.steps)
                        if (b.type == ST_ACT && b.out == A.res) B = &b;
                    // (two readers: A's residual and one conv - the virtual source plus ONE stored gradient)
                    if (!B || B->res >= 0 || !reduce_pass_under_head(*B) || E.tens[B->out].C != C || readers_of(B->out) != 2) continue;
                }
                E.steps[A.ua].head_w = 1;
                if (B) E.steps[B->ua].head_w = 2;
                E.head_w_act = (int)ai;
            }
        }
    }

    // ---- statistics finalize folded into the elementwise consumer (not for the fused input block / one-launch small tensors)
    void mark_fold() {
        for (auto& s : E.steps) s.fold_fin = false;
        if (!E.use_fold) return;
        for (auto& A : E.steps) {
            if (A.type != ST_ACT || A.vact || E.steps[A.ua].fused_stem || E.steps[A.ua].gn_w < 0) continue;
            const Step& ua = E.steps[A.ua];
            if (A.ub < 0 && small_group(ua)) continue;
            if (ua.Cout > 256) continue;
            E.steps[A.ua].fold_fin = true;
            if (A.ub >= 0) E.steps[A.ub].fold_fin = true;
        }
    }

    // ---- small persistent regions, forward tensors, GroupNorm buffers.  The order of the alloc calls IS the layout.
    void layout_workspace() {
        const int N = E.N;
        E.off_step = alloc(256);
        E.off_masks = alloc((size_t)E.drop_ch.size() * N * E.ld_mask() * 4);
        for (auto& t : E.tens) t.off = alloc(ten_bytes(t));
        // statistics (fp64) contiguous so one memset clears them; same for Q, right behind (the forward fill clears both when off_Q == off_stats + stats_bytes)
        const size_t s0 = cur;
        for (auto& s : E.steps)
            if (s.type == ST_UNIT && s.gn_w >= 0) s.stats = alloc((size_t)STAT_REP * N * s.Cout * 2 * 8);
        E.off_stats = s0; E.stats_bytes = cur - s0;
        const size_t q0 = cur;
        for (auto& s : E.steps)
            if (s.type == ST_UNIT && s.gn_w >= 0) s.Q = alloc((size_t)STAT_REP * N * s.Cout * 2 * 8);
        for (auto& s : E.steps)          // head weight-gradient sums: part of the Q region, so whatever clears Q clears them (only where the path is planned)
            if (s.type == ST_UNIT && s.head_w) s.head_q = alloc((size_t)STAT_REP * N * s.Cout * 2 * 8);
        E.off_Q = q0; E.Q_bytes = cur - q0;
        for (auto& s : E.steps)
            if (s.type == ST_UNIT && s.gn_w >= 0) {
                s.scale = alloc((size_t)N * s.Cout * 4);
                s.shift = alloc((size_t)N * s.Cout * 4);
                s.mean = alloc((size_t)N * GN_GROUPS * 4);
                s.rstd = alloc((size_t)N * GN_GROUPS * 4);
                s.coef = alloc((size_t)N * s.Cout * 3 * 4);
            }
        for (auto& s : E.steps)
            if (s.type == ST_CLS) s.cls_ws = alloc(cls_head_ws_bytes(N, E.vol(E.tens[s.in].lvl)));
    }

    // packed layouts of one UNIT's weights (forward, data-gradients) and, for halo convs, the conv3x tilings they are packed for
    void pack_unit(Step& s) {
        const int T = conv_geom(s.ck, E.ndim).ntaps, Ci = s.Cin, Co = s.Cout, N = E.N, dt = E.dtype;
        const long long woff = E.params[s.w].off;
        const int C0 = E.tens[s.in0].C, C1 = s.in1 >= 0 ? E.tens[s.in1].C : 0;
        switch (s.ck) {
            case CK_K3: case CK_K1: case CK_K2S2:
                s.x_fwd = s.x_dg0 = s.x_dg1 = -1;
                if (s.ck == CK_K3 && E.use_conv3x) {
                    // register-blocked halo kernel (conv3x.hip) wherever the shape allows: fragment-major weights
                    const int l = E.tens[s.raw].lvl, d_ = E.dim_d(l), h_ = E.dim_h(l), w_ = E.dim_w(l);
                    if (conv3x_supported(dt, E.ndim, N, d_, h_, w_, Ci, Co, C0, C1 > 0)) s.x_fwd = conv3x_pick(E.ndim, N, d_, h_, w_, Ci, Co, C1 > 0);
                    if (!E.tens[s.in0].image && conv3x_supported(dt, E.ndim, N, d_, h_, w_, Co, C0, 0, false))
                        s.x_dg0 = conv3x_pick(E.ndim, N, d_, h_, w_, Co, C0);
                    if (C1 && conv3x_supported(dt, E.ndim, N, d_, h_, w_, Co, C1, 0, false)) s.x_dg1 = conv3x_pick(E.ndim, N, d_, h_, w_, Co, C1);
                }
                s.wp_fwd = alloc_pack(Co, T * Ci, conv3x_cfg_frag(s.x_fwd));
                add_pack(false, s.wp_fwd, woff, Co, 1, T, Ci, (long long)(s.cin_par ? s.cin_par : Ci) * T, 0, 1, T, 0, s.x_fwd >= 0 ? conv3x_cfg_frag(s.x_fwd) : 0,
                         s.cin_par);                         // image convs on a zero-padded image tensor: the parameter has cin_par channels
                if (s.ck == CK_K2S2) {       // data-gradient = scatter GEMM, rows (a, ci), K = Cout
                    s.wp_dg0 = alloc_pack(T * Ci, Co);
                    add_pack(true, s.wp_dg0, woff, T, Ci, 1, Co, 1, T, 0, (long long)Ci * T, 0);
                } else {                     // data-gradient = gather conv with flipped taps, rows ci, k = (tap, co)
                    if (!E.tens[s.in0].image) {
                        s.wp_dg0 = alloc_pack(C0, T * Co, conv3x_cfg_frag(s.x_dg0));
                        add_pack(true, s.wp_dg0, woff, C0, 1, T, Co, T, 0, 1, (long long)Ci * T, 1, s.x_dg0 >= 0 ? conv3x_cfg_frag(s.x_dg0) : 0);
                    }
                    if (C1) {
                        s.wp_dg1 = alloc_pack(C1, T * Co, conv3x_cfg_frag(s.x_dg1));
                        add_pack(true, s.wp_dg1, woff + (long long)C0 * T, C1, 1, T, Co, T, 0, 1, (long long)Ci * T, 1, s.x_dg1 >= 0 ? conv3x_cfg_frag(s.x_dg1) : 0);
                    }
                }
                break;
            case CK_KT:                      // forward = scatter GEMM rows (a, co), K = Cin
                s.wp_fwd = alloc_pack(T * Co, Ci);
                add_pack(false, s.wp_fwd, woff, T, Co, 1, Ci, 1, T, 0, (long long)Co * T, 0);
                s.wp_dg0 = alloc_pack(Ci, T * Co);   // data-gradient = gather stride 2, rows ci, k = (a, co)
                add_pack(true, s.wp_dg0, woff, Ci, 1, T, Co, (long long)Co * T, 0, 1, T, 0);
                break;
            default:                         // image stems: [Cout][32] with k = tap*Cimg + ci (1^d stem: k = ci)
                s.wp_fwd = alloc_pack(Co, T * Ci);
                add_pack(false, s.wp_fwd, woff, Co, 1, T, Ci, (long long)Ci * T, 0, 1, T, 0);
                break;
        }
    }

    // ---- packed weights
    void layout_packed_weights() {
        for (auto& s : E.steps)
            if (s.type == ST_UNIT) pack_unit(s);
        // forward layouts first, backward-only layouts behind them: the second range is packed on the weight-gradient stream
        std::vector<PackDesc> fw, bw;
        for (size_t i = 0; i < E.packdescs.size(); ++i) (E.pack_is_bwd[i] ? bw : fw).push_back(E.packdescs[i]);
        E.npack_fwd = (int)fw.size();
        E.packdescs = fw;
        E.packdescs.insert(E.packdescs.end(), bw.begin(), bw.end());
        E.pack_is_bwd.assign(E.packdescs.size(), 0);
        for (size_t i = fw.size(); i < E.packdescs.size(); ++i) E.pack_is_bwd[i] = 1;
        E.off_packdesc = alloc(E.packdescs.size() * sizeof(PackDesc));
    }

    // ---- 1^d convs on a concat: one data-gradient launch for both sources; where the first source is a never-written activation (vact) of equal width, that
    // launch also carries the GroupNorm-backward sums of the activation's unit
    void mark_dual_dgrad() {
        for (auto& s : E.steps) { s.dual_dg = false; s.rq_dg = false; s.rq_fused = false; }
        for (auto& c : E.steps) {
            if (c.type != ST_UNIT) continue;
            ConvArgs b;
            c.dual_dg = make_dual_dgrad_args(E, c, -1, -1, -1, b, nullptr);
            if (!c.dual_dg || c.vact_unit < 0 || !E.use_rq_fuse || E.tens[c.in0].C != E.tens[c.in1].C) continue;
            for (auto& A : E.steps)
                if (A.type == ST_ACT && A.vact && A.ua == c.vact_unit) {
                    const Step& pu = E.steps[A.ua];
                    GnBwdArgs probe{}; probe.ndy = 1; probe.C = pu.Cout; probe.V = E.vol(E.tens[pu.raw].lvl); probe.N = E.N;
                    if (E.use_coop && gn_bwd_coop_eligible(probe, (int)E.esz())) continue;
                    if (small_group(pu)) continue;
                    A.rq_fused = c.rq_dg = true;
                }
        }
    }

    size_t wgrad3_partial(const Step& s) const {
        const int l = E.tens[s.raw].lvl;
        return wgrad3_partial_bytes(E.ndim, E.N, E.dim_d(l), E.dim_h(l), E.dim_w(l), s.Cout, s.Cin);
    }
    // ---- partial-tile buffers of the weight-gradient kernels
    void alloc_partials() {
        const int N = E.N, d0 = E.dim_d(0), h0 = E.dim_h(0), w0 = E.dim_w(0);
        size_t pmax = 0, p3 = 0;
        for (auto& s : E.steps) {
            if (s.type != ST_UNIT) continue;
            if (s.ck == CK_K3) { p3 = std::max(p3, wgrad3_partial(s)); pmax = std::max(pmax, p3); }
            else if (s.ck == CK_STEM3 || s.ck == CK_STEM1) pmax = std::max(pmax, stem_wgrad_partial_bytes(E.ndim, N, d0, h0, w0, s.Cout));
            else pmax = std::max(pmax, wgrad_partial_bytes(make_wgrad_args(E, s, -1, nullptr)));
        }
        E.off_partial = alloc(pmax);
        // halo weight gradients keep one partial-tile slot per layer until the reduce of their level visit (seg_engine::w3_slot)
        E.partial3_stride = align_up(p3);
        E.off_partial3 = alloc(E.partial3_stride * W3_BATCH);
        E.off_partial_stemx = alloc(E.stem_onepass ? stemx_moment_bytes(E.ndim, N, d0, h0, w0, E.in_ch) : stemx_partial_bytes(E.ndim, N, d0, h0, w0, E.in_ch));
        E.off_partial_stem1 = alloc(stem_wgrad_partial_bytes(E.ndim, N, d0, h0, w0, 16 * ((E.feat + 15) / 16)));
    }

    void schedule_forward() {
        seg_engine* e = &E;
        E.fwd_ops.push_back([e](hipStream_t st) { fwd_ingest(*e, st); });
        for (int si = 0; si < (int)E.steps.size(); ++si)
            switch (E.steps[si].type) {
                case ST_UNIT: E.fwd_ops.push_back([e, si](hipStream_t st) { fwd_unit(*e, si, st); }); break;
                case ST_ACT:  E.fwd_ops.push_back([e, si](hipStream_t st) { fwd_act(*e, si, st); }); break;
                case ST_POOL: E.fwd_ops.push_back([e, si](hipStream_t st) { fwd_pool(*e, si, st); }); break;
                case ST_CLS:  E.fwd_ops.push_back([e, si](hipStream_t st) { fwd_cls(*e, si, st); }); break;
                default:      E.fwd_ops.push_back([e, si](hipStream_t st) { fwd_head(*e, si, st); }); break;
            }
    }

    // one backward op: the parameters whose gradients it finishes + its launch
    void push_bwd(std::vector<int> writes, std::function<void(hipStream_t)> op) {
        E.bwd_writes.push_back(std::move(writes));
        E.bwd_ops.push_back(std::move(op));
    }
    // The steps in reverse.  new_grad calls fix the order (and offsets) of the gradient tensors; head_din_needed is settled here and read at launch time.
    bool schedule_backward() {
        seg_engine* e = &E;
        push_bwd({}, [e](hipStream_t st) {
            if (!e->q_clean) (void)hipMemsetAsync(e->ws + e->off_Q, 0, e->Q_bytes, st);
            e->q_clean = false;
        });
        for (int si = (int)E.steps.size() - 1; si >= 0; --si) {
            bool ok = true;
            switch (E.steps[si].type) {
                case ST_HEAD: plan_bwd_head(si); break;
                case ST_CLS:  plan_bwd_cls(si); break;
                case ST_POOL: ok = plan_bwd_pool(si); break;
                case ST_ACT:  ok = plan_bwd_act(si); break;
                default:      ok = plan_bwd_unit(si); break;
            }
            if (!ok) return false;
        }
        if (E.head_w_act >= 0 && E.head_din_needed) { g_err = "internal: the head's weight gradient rides on passes that do not take the virtual head source"; return false; }
        return true;
    }
    void plan_bwd_head(int si) {
        seg_engine* e = &E;
        const Step& s = E.steps[si];
        const int gin = new_grad(s.in);
        E.tens[gin].virt = E.use_vhead;
        E.head_din_needed = !E.use_vhead;
        E.head_step = si;
        E.tens[s.in].grads.push_back(gin);
        // head_w_act: the op stays (the op numbering of a plan does not depend on the switch) but launches nothing - w / b finish with the last reduce + apply
        // pair that collects them (plan_bwd_act)
        if (E.head_w_act >= 0) push_bwd({}, [](hipStream_t) {});
        else push_bwd({s.w, s.b}, [e, si, gin](hipStream_t st) { bwd_head(*e, si, gin, st); });
    }
    // the classification head opens the backward pass: its four parameters are registered last, so the finished gradients form a suffix from here on
    void plan_bwd_cls(int si) {
        seg_engine* e = &E;
        const Step& s = E.steps[si];
        const int gin = new_grad(s.in);
        E.tens[s.in].grads.push_back(gin);
        push_bwd({s.w, s.b, s.w2, s.b2}, [e, si, gin](hipStream_t st) { bwd_cls(*e, si, gin, st); });
    }
    bool plan_bwd_pool(int si) {
        seg_engine* e = &E;
        const Step& s = E.steps[si];
        const std::vector<int> gl = E.tens[s.out].grads;
        if (gl.size() != 1) { g_err = "internal: pool output needs exactly one gradient"; return false; }
        const int gout = gl[0];
        if (E.tens[gout].virt) E.head_din_needed = true;
        const int gin = new_grad(s.in);
        E.tens[s.in].grads.push_back(gin);
        push_bwd({}, [e, si, gin, gout](hipStream_t st) { bwd_pool(*e, si, gin, gout, st); });
        return true;
    }
    bool plan_bwd_act(int si) {
        seg_engine* e = &E;
        const Step& s = E.steps[si];
        const std::vector<int> gl = E.tens[s.out].grads;
        if (gl.empty() || gl.size() > 3) { g_err = "internal: unsupported gradient fan-in"; return false; }
        if (s.res >= 0) for (int gi : gl) E.tens[s.res].grads.push_back(gi);
        const Step& ua = E.steps[s.ua];
        // the fused input block, the dual-branch and the one-launch small-tensor passes read real tensors only
        const bool generic = !ua.fused_stem && s.ub < 0 && !small_group(ua);
        for (int gi : gl) if (E.tens[gi].virt && !generic) E.head_din_needed = true;
        if (ua.fused_stem) {
            std::vector<int> wr;
            for (int ui : {s.ua, s.ub})
                if (ui >= 0) { const Step& u = E.steps[ui]; wr.push_back(u.gn_w); wr.push_back(u.gn_b); wr.push_back(u.b); wr.push_back(u.w); }
            push_bwd(wr, [e, si, gl](hipStream_t st) { bwd_act_stem(*e, si, gl, st); });
            return true;
        }
        if (s.ub >= 0 && E.dual_gn_bwd && !small_group(ua)) {
            const int uia = s.ua, uib = s.ub;
            Step& a = E.steps[uia];
            Step& b = E.steps[uib];
            a.draw = new_grad(a.raw);
            b.draw = new_grad(b.raw);
            push_bwd({a.gn_w, a.gn_b, a.b, b.gn_w, b.gn_b, b.b}, [e, uia, uib, gl](hipStream_t st) { bwd_act_dual(*e, uia, uib, gl, st); });
            return true;
        }
        for (int ui : {s.ua, s.ub}) {
            if (ui < 0) continue;
            Step& u = E.steps[ui];
            u.draw = new_grad(u.raw);
            std::vector<int> wr{u.gn_w, u.gn_b, u.b};          // gamma/beta and (analytically) the conv bias
            if (u.head_w) {
                // the head's w / b are complete behind the LATER of the passes that collect them (backward order: unit 1, then unit 2 where there is one)
                bool later = false;
                for (auto& o : E.steps) later |= o.type == ST_UNIT && o.head_w > u.head_w;
                if (!later) { wr.push_back(E.steps[E.head_step].w); wr.push_back(E.steps[E.head_step].b); }
            }
            push_bwd(wr, [e, si, ui, gl](hipStream_t st) { bwd_act(*e, si, ui, gl, st); });
        }
        return true;
    }
    bool plan_bwd_unit(int si) {
        seg_engine* e = &E;
        const Step& s = E.steps[si];
        if (s.fused_stem) return true;      // weight gradients come out of the fused input block (its ACT op)
        int draw = s.draw;
        if (s.gn_w < 0) {
            // plain ConvTranspose (UNet up-conv): d(raw) is the (single) gradient of its output tensor
            const std::vector<int>& gl = E.tens[s.raw].grads;
            if (gl.size() != 1) { g_err = "internal: plain conv output needs exactly one gradient"; return false; }
            draw = gl[0];
            if (E.tens[draw].virt) E.head_din_needed = true;
        }
        if (draw < 0) { g_err = "internal: unit without output gradient"; return false; }
        int g0 = -1, g1 = -1;
        if (!E.tens[s.in0].image) { g0 = new_grad(s.in0); E.tens[s.in0].grads.push_back(g0); }
        if (s.in1 >= 0) { g1 = new_grad(s.in1); E.tens[s.in1].grads.push_back(g1); }
        push_bwd({s.w, s.gn_w < 0 ? s.b : -1}, [e, si, draw, g0, g1](hipStream_t st) { bwd_unit(*e, si, draw, g0, g1, st); });
        return true;
    }
};

}  // namespace

namespace segi {
void build_network(seg_engine& e, int net_kind) {
    Builder b(e);
    if (net_kind == SEG_NET_VNET) b.build_vnet();
    else if (net_kind == SEG_NET_UNET) b.build_unet();
    else b.build_resnet();
}
void plan_engine(seg_engine& e) {
    Planner pl(e);
    pl.plan();
}
}  // namespace segi
